"""The loops of generate(), once, for the three language models (MPTForCausalLM under CrossAttentionModel and SelfAttentionModel,
LlamaNeighborLM): the prompt check, the two selection tails and the loop "logits -> (processors) -> (keep the step's logits) ->
select -> write the ids column -> one cached decode step".  A model's generate() validates its keywords (sampling.py), checks the
prompt (check_prompt), picks a tail, runs its prefill and hands decode_loop three things: its _last_logits, a callable for one cached
decode step (tokens [rows, 1] -> hidden [rows, d]) and the prefill's last hidden row.  Beam search (beam_loop, below), prompt-lookup
decoding (lookup_loop, below) and contrastive search (contrastive_loop, below) have loops of another shape; they share check_prompt,
and contrastive search the processors' binding.

Semantics, the same for every model:
  * Prompts are right-padded to the common width T; every new token is appended at the same column for all rows, and all
    max_new_tokens steps run (nothing synchronises with the host to stop early).  The result is [rows, T + max_new_tokens] in the
    prompt's dtype; an embeddings prompt has no ids to repeat, so only the new tokens [rows, max_new_tokens] (int64) come back.
  * eos_token_id: a row that has emitted it gets pad_token_id (default config.pad_token_id) from then on, as in transformers' loops;
    None: no end-of-sequence handling.
  * Greedy (GreedyTail): argmax of the step's logits.  Sampled (SampledTail): transformers' temperature -> top_k -> top_p pipeline
    and the draw in one ops.sample_tokens launch that writes the ids column and the finished flags in place, from
    uniform numbers [max_new_tokens, rows] drawn once before the loop (sampling.sampling_u).
  * R = num_return_sequences > 1: the model prefills B rows and gives its cache a BeamState of R rows per prompt whose parent table
    stays the identity -- R independent rows that share the prompt's keys.  Step 0 draws R tokens from each of the B logits rows,
    every later step has B*R rows.  Rows b*R .. b*R + R - 1 of the result belong to prompt b.
  * proc (sampling.LogitsProcessors, None: off -- then nothing is added): one ops.process_logits call per step rewrites the logits
    in front of the selection, with the returned row so far -- the prompt without its masked columns, then the new
    tokens -- as history; on step 0 of R > 1 the R draws of a prompt share its logits row and the prompt as history.  An embeddings
    prompt may name the ids it stands for (history_ids / history_mask [B, Th]); without them its history is the new tokens.
  * guidance (guidance_scale = g, sampling.check_guidance; None: off): every prompt has a row with neighbors and a row without, in
    lockstep on the same tokens.  Each step's [2B, V] logits become B rows of lu + g (lc - lu) on log-probabilities
    in one ops.guidance_logits call; then, in transformers' order, the processors, return_step_logits and the selection run on
    those B rows, and the chosen token is fed to both rows of its pair.  The result has B rows.
  * return_step_logits: also the [rows, max_new_tokens, V] logits the tokens were picked from (the processed ones with proc, the
    guided scores with guidance)."""
import torch

from .. import ops
from .sampling import sampling_u


def check_prompt(input_ids, inputs_embeds, attention_mask, max_new_tokens, eos_token_id, pad_token_id, config, max_positions):
    """The prompt arguments of every generate(): either input_ids [B, T] or inputs_embeds [B, T, d_embed], on the GPU, with
    T + max_new_tokens - 1 positions inside the model's table.  Returns (B, T, n_new, pad_token_id, attention_mask) with the defaults
    filled in: pad_token_id from `config` when there is an EOS, a mask of ones."""
    if (input_ids is None) == (inputs_embeds is None):
        raise ValueError("generate() takes exactly one of input_ids and inputs_embeds")
    prompt = input_ids if input_ids is not None else inputs_embeds
    n_new = int(max_new_tokens)
    if n_new < 1:
        raise ValueError(f"max_new_tokens must be positive, got {max_new_tokens}")
    if not prompt.is_cuda:
        raise RuntimeError(f"generate() runs on the GPU only (the prompt is on {prompt.device}); there is no CPU path")
    if prompt.dim() != (2 if input_ids is not None else 3):
        raise ValueError(f"generate(): input_ids [B, T] or inputs_embeds [B, T, d_embed], got {tuple(prompt.shape)}")
    B, T = prompt.shape[:2]
    if T + n_new - 1 > max_positions:
        raise ValueError(f"generate(): {T} prompt columns + {n_new} new tokens exceed max_position_embeddings {max_positions}")
    if eos_token_id is not None and pad_token_id is None:
        pad_token_id = config.pad_token_id
        if pad_token_id is None:
            raise ValueError("generate(): eos_token_id needs a pad_token_id")
    if attention_mask is None:
        attention_mask = torch.ones(B, T, dtype=torch.int64, device=prompt.device)
    return B, T, n_new, pad_token_id, attention_mask


class GreedyTail:
    """select(logits, ids, c, s): argmax, the EOS bookkeeping, then the write of column c.  Returns the tokens [rows]."""
    ids_dtype = None                                           # the column write casts: ids are allocated in the prompt's dtype

    def __init__(self, rows, device, eos_token_id=None, pad_token_id=None):
        self.eos, self.pad = eos_token_id, pad_token_id
        self.finished = torch.zeros(rows, dtype=torch.bool, device=device)

    def __call__(self, logits, ids, c, s):
        tok = torch.argmax(logits, dim=-1)
        if self.eos is not None:
            tok = torch.where(self.finished, torch.full_like(tok, self.pad), tok)
            self.finished = self.finished | (tok == self.eos)
        ids[:, c] = tok
        return tok


class SampledTail:
    """select(logits, ids, c, s): one ops.sample_tokens launch on u[s] (u fp32 [n_new, rows], sampling.sampling_u) that writes
    column c and the finished flags in place.  Returns the column."""
    ids_dtype = torch.int64                                    # the kernel writes the int64 column itself

    def __init__(self, u, temperature, top_k, top_p, eos_token_id=None, pad_token_id=None):
        self.u, self.knobs, self.eos, self.pad = u, (temperature, top_k, top_p), eos_token_id, pad_token_id
        self.finished = torch.zeros(u.shape[1], dtype=torch.uint8, device=u.device) if eos_token_id is not None else None

    def __call__(self, logits, ids, c, s):
        col = ids[:, c]
        ops.sample_tokens(logits, self.u[s].view(logits.shape[0], -1), *self.knobs, self.finished, self.eos, self.pad, out=col)
        return col


def make_select(who, do_sample, n_new, B, R, device, seed, sample_u, temperature, top_k, top_p, eos_token_id, pad_token_id):
    """The selection tail of a decode_loop over B prompts with R rows each: a SampledTail on the uniform numbers [n_new, B*R] of
    sampling.sampling_u (`who` names the caller in its errors), or a GreedyTail."""
    if do_sample:
        return SampledTail(sampling_u(who, n_new, B * R, device, seed, sample_u), temperature, top_k, top_p, eos_token_id, pad_token_id)
    return GreedyTail(B, device, eos_token_id, pad_token_id)


def _bind_processors(proc, ids, prompt_mask, history_ids, history_mask, repeat=1):
    """Per-generation setup of the logits processors (sampling.LogitsProcessors) for a result buffer ids [rows, T + n_new].  Returns
    (hist, ids): hist is the buffer whose leading columns are each step's history -- ids itself, or, for an embeddings prompt with
    history_ids [B, Th], a new [B, Th + n_new] buffer that starts with them and whose last n_new columns become `ids`."""
    if history_ids is None:
        if history_mask is not None:
            raise ValueError("generate(): history_mask without history_ids")
        proc.bind(ids.device, prompt_mask, repeat)
        return ids, ids
    B, n_new = ids.shape
    if (not torch.is_tensor(history_ids) or history_ids.dtype != torch.int64 or history_ids.dim() != 2 or history_ids.shape[0] != B
            or history_ids.device != ids.device):
        raise ValueError(f"generate(): history_ids must be an int64 [{B}, Th] tensor on {ids.device}")
    Th = history_ids.shape[1]
    if history_mask is not None and (tuple(history_mask.shape) != (B, Th) or history_mask.device != ids.device):
        raise ValueError(f"generate(): history_mask must be a [{B}, {Th}] tensor on {ids.device}")
    hist = torch.empty(B, Th + n_new, dtype=torch.int64, device=ids.device)
    hist[:, :Th] = history_ids
    proc.bind(ids.device, history_mask, repeat)
    return hist, hist[:, Th:]


def decode_loop(last_logits, step, hidden, select, n_new, input_ids=None, prompt_mask=None, R=1, proc=None, history_ids=None,
                history_mask=None, return_step_logits=False, guidance=None):
    """The n_new steps behind a prefill whose last row is `hidden` [B, ...]: see the module docstring.  last_logits(hidden) ->
    [rows, V]; step(tokens [rows, 1]) -> the next hidden, called n_new - 1 times; select: a GreedyTail or a SampledTail over B*R
    rows; input_ids [B, T]: the prompt to return in front of the new tokens (None: an embeddings prompt); prompt_mask [B, T]: its
    valid columns, read by proc only.  guidance (a float g, None: off -- then nothing is added): `hidden` and every step have 2B rows,
    the B rows with neighbors and then the B rows without; R is 1.  Returns ids, or (ids, step logits)."""
    rows = hidden.shape[0] * R if guidance is None else hidden.shape[0] // 2
    T = 0 if input_ids is None else input_ids.shape[1]       # columns of the result in front of the new tokens
    ids = torch.empty(rows, T + n_new, dtype=select.ids_dtype or (torch.int64 if input_ids is None else input_ids.dtype),
                      device=hidden.device)
    if input_ids is not None:
        ids[:, :T] = input_ids if R == 1 else input_ids.repeat_interleave(R, dim=0)
    if proc is not None:
        hist, ids = _bind_processors(proc, ids, prompt_mask if input_ids is not None else None, history_ids, history_mask, R)
        Th = hist.shape[1] - n_new                             # step s chooses column Th + s of hist
    steps = []
    for s in range(n_new):
        logits = last_logits(hidden)
        if guidance is not None:
            logits = ops.guidance_logits(logits, rows, guidance)        # [2B, V] -> the B guided rows, in place
        shared = rows // logits.shape[0]                       # R on step 0 of R > 1 (the prefill's B rows, R draws each), else 1
        if proc is not None:
            proc(logits, hist[::shared, :Th + s], s, shared)
        if return_step_logits:
            steps.append(logits if shared == 1 else logits.repeat_interleave(shared, dim=0))
        tok = select(logits, ids, T + s, s)
        if s + 1 < n_new:
            hidden = step(tok[:, None] if guidance is None else tok.repeat(2)[:, None])
    if input_ids is not None:
        ids = ids.to(input_ids.dtype)
    elif not ids.is_contiguous():
        ids = ids.contiguous()                                 # the new-token columns of the history buffer (history_ids)
    return (ids, torch.stack(steps, dim=1)) if return_step_logits else ids


def lookup_loop(last_logits, verify, hidden, lookup, input_ids, prompt_mask, n_new, eos_token_id, pad_token_id, pos_offset, pos_max,
                return_stats=False):
    """Greedy generation by prompt-lookup decoding behind a prefill whose last row is `hidden` [B, ...]: the result
    of decode_loop with a GreedyTail -- [B, T + n_new] in the prompt's dtype, EOS followed by pad_token_id -- in fewer steps.
    lookup: the cache's LookupState; verify() -> hidden [B*(K+1), d]: one verify step on lookup.block; last_logits as in decode_loop.
    Call 0 of ops.lookup_accept takes the prefill's row (m_in = 1) and drafts the first block; every verify step is followed by one
    call (m_in = K + 1) that keeps the longest prefix of the block greedy decoding would have produced, appends it to ids and drafts
    the next block.  Rows advance at their own pace, so the number of steps depends on the data: before every verify step the host
    reads ONE int32 from the device -- the smallest token count over the rows -- and stops when it has reached n_new.  This is the
    one loop of generate() that reads from the device while it runs (decode_loop and beam search run a fixed number of steps and
    never do); a finished row waits for the others with its state frozen.  Every verify step gives every unfinished row at least one
    token and call 0 gave one, so at most n_new - 1 verify steps run.
    return_stats: also dict(steps = verify steps run, emitted = int32 [steps + 1, B], the tokens each call appended per row)."""
    B, T = input_ids.shape
    ids = torch.empty(B, T + n_new, dtype=torch.int64, device=input_ids.device)
    ids[:, :T] = input_ids
    mask = (prompt_mask != 0).to(torch.uint8)

    def accept(hid, m_in, call):
        ops.lookup_accept(last_logits(hid), m_in, lookup.block, lookup.n_draft, lookup.positions, ids, mask, lookup.gen, lookup.len,
                          lookup.finished, lookup.emitted[call], n_new, lookup.N, eos_token_id, pad_token_id, pos_offset, pos_max)

    accept(hidden, 1, 0)
    steps = 0
    while n_new > 1 and int(lookup.gen.min()) < n_new:          # the one 4-byte device read of a step
        assert steps < n_new - 1, f"prompt-lookup decoding: more than {n_new - 1} verify steps"
        accept(verify(), lookup.W, steps + 1)
        steps += 1
    ids = ids.to(input_ids.dtype)
    return (ids, dict(steps=steps, emitted=lookup.emitted[:steps + 1].clone())) if return_stats else ids


def beam_loop(last_logits, step, hidden, book, input_ids, n_new, W, vocab_size, eos_token_id, pad_token_id, length_penalty, early_stopping,
              return_scores=False, return_trace=False):
    """Beam search behind a prefill of B rows whose last row is `hidden` [B, ...], W hypotheses per sample on the
    beam-shared cache whose BeamState owns `book` (ops.BeamBook).  The prefill's logits seed the W beams (rows_in = 1 of ops.beam_topk,
    in place of HF's -1e9 start scores); step(tokens [B*W, 1]) -> hidden [B*W, d] is one decode step of the B*W rows, last_logits as
    in decode_loop.  Per step ops.beam_topk (two launches) picks each sample's 2W best continuations and ops.beam_advance (one
    launch) turns them into the next tokens, parents, running scores, table and pool of finished hypotheses; nothing synchronises
    with the host.
    Semantics of transformers' beam search: the first W non-EOS candidates run on; an EOS candidate among the first W (every one
    of them at the last step) enters the pool with score = log-prob sum / generated_length ** length_penalty; a sample is frozen
    once its pool is full under early_stopping=True or the early-stop heuristic is met.  All n_new steps run.
    Returns ids [B, T + n_new] -- the best pooled hypothesis, pad_token_id behind its last token -- then, as asked,
    sequences_scores fp32 [B] and the trace: per step a dict of the running beams' parents / tokens / scores [B, W] and the 2W
    candidates cand_index / cand_score [B, 2W]."""
    B, dev = input_ids.shape[0], input_ids.device
    start = torch.zeros(B, dtype=torch.float32, device=dev)
    history = torch.empty(n_new, B, W, dtype=torch.int64, device=dev)       # history[s, b, w]: the token slot w took at step s
    trace = []
    for s in range(n_new):
        logits = last_logits(hidden)
        cs, ci = ops.beam_topk(logits, start if s == 0 else book.beam_score, W, rows_in=1 if s == 0 else W)
        ops.beam_advance(cs, ci, book, s, vocab_size, eos_token_id, s == n_new - 1, early_stopping, float(s + 1) ** length_penalty)
        history[s] = book.tokens.view(B, W)
        if return_trace:
            trace.append(dict(parents=book.parents.view(B, W).clone(), tokens=book.tokens.view(B, W).clone(),
                              scores=book.beam_score.view(B, W).clone(), cand_index=ci, cand_score=cs))
        if s + 1 < n_new:
            hidden = step(history[s].reshape(B * W, 1))
    # the best pooled hypothesis of each sample: tokens 0 .. len-2 through its ancestry row, its own last token, then padding
    score, length, anc, last = (t.view(B, W, *t.shape[1:])[:, 0] for t in book.pool)
    cols = torch.arange(n_new, device=dev)[None, :]
    slot = torch.zeros(B, n_new, dtype=torch.int64, device=dev)
    slot[:, :n_new - 1] = anc[:, :n_new - 1]
    new = history.permute(1, 0, 2).gather(2, slot[:, :, None])[:, :, 0]                       # [B, n_new]
    length = length.long()[:, None]
    new = torch.where(cols < length - 1, new, torch.where(cols == length - 1, last[:, None], torch.full_like(new, pad_token_id)))
    ids = torch.cat([input_ids, new.to(input_ids.dtype)], dim=1)
    res = (ids,)
    if return_scores:
        res += (score.clone(),)
    if return_trace:
        res += (trace,)
    return res[0] if len(res) == 1 else res


def contrastive_loop(last_logits, step, prompt_hidden, src, input_ids, prompt_mask, n_new, k, penalty_alpha, vocab_size, eos_token_id=None,
                     pad_token_id=None, proc=None, return_step_logits=False, return_trace=False):
    """Contrastive search (Su et al. 2022) behind a prefill whose last_hidden_state is prompt_hidden [B, T, d]: every
    step ranks the k most likely next tokens by  (1 - alpha) p(token) - alpha max_j cos(h_token, h_j)  over the hidden rows h_j of the
    row so far, and takes the best.  Deterministic; [B, T + n_new] in the prompt's dtype, EOS followed by pad_token_id as GreedyTail.
    step(tokens [B*k, 1]) -> hidden [B*k, d]: one decode step of the k candidates of every sample on the beam-shared cache, whose
    parent table is `src` (BeamBook.src, the identity at first); last_logits as in decode_loop.
    The context buffer [B, T + n_new, d] starts as the prompt's hidden rows, its mask as the prompt's: a masked prompt column is no
    context (transformers ranks against it too; here it is the processors' rule, the row without its pad columns).  Step s:
    last_logits of the last chosen token's hidden row (the prefill's last row at s = 0) -> the processors -> ops.beam_topk (the k
    candidates and their log-probabilities) -> `step` on the B*k candidate tokens -> ops.contrastive_select, which picks, writes the
    ids column, the EOS flags, column s of `src` (tail column s of every row of the sample now names the chosen key), context row
    T + s and the dense [B, d] input of the next last_logits.  All n_new candidate steps run -- the last token's candidates must be
    forwarded to be ranked -- so T + n_new positions are needed; nothing synchronises with the host.
    Returns ids, then as asked the step logits [B, n_new, V] and the trace: per step a dict of candidates int32 [B, k], p / penalty /
    score fp32 [B, k] and selected int32 [B]."""
    B, T = input_ids.shape
    dev, d = input_ids.device, prompt_hidden.shape[-1]
    ids = torch.empty(B, T + n_new, dtype=torch.int64, device=dev)
    ids[:, :T] = input_ids
    ctx = torch.empty(B, T + n_new, d, dtype=prompt_hidden.dtype, device=dev)
    ctx[:, :T] = prompt_hidden
    valid = torch.zeros(B, T + n_new, dtype=torch.uint8, device=dev)
    valid[:, :T] = prompt_mask != 0
    finished = torch.zeros(B, dtype=torch.uint8, device=dev) if eos_token_id is not None else None
    start = torch.zeros(B, dtype=torch.float32, device=dev)
    if proc is not None:
        _bind_processors(proc, ids, prompt_mask, None, None)
    hidden = prompt_hidden[:, -1]
    steps, trace = [], []
    for s in range(n_new):
        logits = last_logits(hidden)
        if proc is not None:
            proc(logits, ids[:, :T + s], s)
        if return_step_logits:
            steps.append(logits)
        cs, ci = ops.beam_topk(logits, start, k, rows_in=1)
        cand = ci[:, :k].reshape(B * k, 1)
        res = ops.contrastive_select(step(cand), ctx, valid, cs, ci, penalty_alpha, T + s, s, src, ids[:, T + s], vocab_size, finished,
                                     eos_token_id, pad_token_id, trace=return_trace)
        hidden = res[0]
        if return_trace:
            trace.append(dict(candidates=cand.view(B, k), p=res[2][0], penalty=res[2][1], score=res[2][2], selected=res[1]))
    out = (ids.to(input_ids.dtype),)
    if return_step_logits:
        out += (torch.stack(steps, dim=1),)
    if return_trace:
        out += (trace,)
    return out[0] if len(out) == 1 else out
