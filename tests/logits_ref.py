"""Reference for the logits-processor tests: the contract of mmgl_logits_process (include/mmgl_hip.h) restated in
plain torch on the CPU, and transformers' own chain for the rows it is defined on.  Nothing here calls the code under test.

Per row, with h = the history without its masked columns and x = the row's logits:
  1. repetition_penalty p   for every distinct t of h in [0, V): x[t] = x[t] * p if x[t] < 0 else x[t] / p  (fp32, rounded once)
  2. no_repeat_ngram_size n for every i in [0, L-n] with h[i .. i+n-1) == h[L-n+1 .. L): x[h[i+n-1]] = -inf
  3. bans                   x[t] = -inf
A history token outside [0, V) is never an address and equals nothing (an n-gram that contains one neither matches nor bans).
"""
import torch


def compact(history_row, valid_row=None):
    """The history of one row as a Python list: the columns whose valid entry is 0 removed (valid covers the leading columns)."""
    h = [int(t) for t in history_row]
    if valid_row is None:
        return h
    v = [bool(b) for b in valid_row]
    return [t for c, t in enumerate(h) if c >= len(v) or v[c]]


def process_row(x, h, penalty=1.0, ngram=0, ban=()):
    """x: fp32 [V] (a copy is returned); h: list of ints."""
    x = x.clone()
    V = x.shape[0]
    assert x.dtype == torch.float32
    if penalty != 1.0:
        p = torch.tensor(float(penalty), dtype=torch.float32)
        seen = torch.tensor(sorted({t for t in h if 0 <= t < V}), dtype=torch.int64)       # distinct: each is penalised once
        x[seen] = torch.where(x[seen] < 0, x[seen] * p, x[seen] / p)
    L = len(h)
    if ngram > 0 and L >= ngram:
        pre = h[L - ngram + 1:]
        if all(0 <= t < V for t in pre):
            for i in range(L - ngram + 1):
                t = h[i + ngram - 1]
                if h[i:i + ngram - 1] == pre and 0 <= t < V:
                    x[t] = float("-inf")
    for t in ban:
        if 0 <= int(t) < V:
            x[int(t)] = float("-inf")
    return x


def process(logits, history=None, valid=None, penalty=1.0, ngram=0, ban=()):
    """logits [rows, V] bf16 / fp32 (any device): the restatement in fp32 on the upcast logits, rounded once to their dtype.
    history [rows, L] or None, valid [rows, n_masked] or None.  Returns a new CPU tensor."""
    x = logits.detach().cpu()
    out = torch.empty_like(x)
    for r in range(x.shape[0]):
        h = [] if history is None else compact(history[r].cpu().tolist(), None if valid is None else valid[r].cpu().tolist())
        out[r] = process_row(x[r].float(), h, penalty, ngram, ban).to(x.dtype)
    return out


def hf_chain(logits, h, penalty=1.0, ngram=0, suppress=(), eos=None, min_new=0, n_generated=0):
    """transformers' RepetitionPenalty -> NoRepeatNGram -> MinNewTokensLength -> SuppressTokens on one fp32 row x [V] with the
    (compacted) history h, all of whose tokens lie in [0, V).  n_generated: the new tokens so far (the EOS ban holds below min_new)."""
    from transformers import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                              SuppressTokensLogitsProcessor)
    ids = torch.tensor([h], dtype=torch.int64)
    scores = logits.detach().cpu().float().clone()[None]
    if penalty != 1.0:
        scores = RepetitionPenaltyLogitsProcessor(float(penalty))(ids, scores)
    if ngram > 0:
        scores = NoRepeatNGramLogitsProcessor(int(ngram))(ids, scores)
    if min_new > 0:
        prompt_len = len(h) - n_generated
        scores = MinNewTokensLengthLogitsProcessor(prompt_len, int(min_new), eos, device="cpu")(ids, scores)
    if len(suppress):
        scores = SuppressTokensLogitsProcessor(list(suppress), device="cpu")(ids, scores)
    return scores[0]
