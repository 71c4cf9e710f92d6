"""References for the beam-search tests: an fp64 restatement of mmgl_attn_decode_beam_fwd and mmgl_beam_topk (device-agnostic torch),
and the beam bookkeeping of generate(num_beams=W) in plain Python (integers and numpy float32 scalars: every value is a copy, an
integer, or one IEEE float32 division), which tests/test_beam_cpu.py holds against transformers' own beam search."""
import numpy as np
import torch


# ------------------------------------------------------------------------------------------ attention
def attn_beam_ref(q, k_pre, v_pre, valid, num_heads, W, k_tail=None, v_tail=None, src=None):
    """fp64: row (b, w) attends over  pre[b] ++ [tail[b*W + src[b*W + w, j], j] for j < n_tail].  Masked prefix keys weigh nothing; a
    sample whose prefix has no valid key is uniform over all its S_pre + n_tail keys (include/mmgl_hip.h).  Returns [B*W, d]."""
    R, d = q.shape
    B, S = k_pre.shape[:2]
    D = d // num_heads
    n_tail = 0 if k_tail is None else k_tail.shape[1]
    k = k_pre.double().repeat_interleave(W, 0)                                    # the EXPANDED cache: [B*W, S, d]
    v = v_pre.double().repeat_interleave(W, 0)
    ok = valid.bool().repeat_interleave(W, 0)
    if n_tail:
        rows = (torch.arange(R, device=q.device) // W * W)[:, None] + src[:, :n_tail].long()           # [R, n_tail] tail row per key
        cols = torch.arange(n_tail, device=q.device)[None, :].expand(R, -1)
        k = torch.cat([k, k_tail.double()[rows, cols]], 1)
        v = torch.cat([v, v_tail.double()[rows, cols]], 1)
        ok = torch.cat([ok, torch.ones(R, n_tail, dtype=torch.bool, device=q.device)], 1)
    dead = ~valid.bool().any(1).repeat_interleave(W, 0)                           # no valid PREFIX key
    sc = torch.einsum("rhd,rshd->rhs", q.double().reshape(R, num_heads, D), k.reshape(R, S + n_tail, num_heads, D))
    sc = sc.masked_fill(~ok[:, None, :], float("-inf"))
    sc[dead] = 0.0
    return torch.einsum("rhs,rshd->rhd", torch.softmax(sc, -1), v.reshape(R, S + n_tail, num_heads, D)).reshape(R, d)


# ------------------------------------------------------------------------------------------ candidate selection
def topk_ref(logits, beam_score, W, rows_in):
    """fp64 scores [B, rows_in * V] = beam_score + log_softmax(logits) of the storage-rounded logits, flat index r*V + v."""
    rows, V = logits.shape
    sc = beam_score.double()[:, None] + torch.log_softmax(logits.double(), -1)
    return sc.reshape(rows // rows_in, rows_in * V)


# ------------------------------------------------------------------------------------------ bookkeeping
class BookRef:
    """Plain-Python state of a beam search over B samples x W beams (what ops.BeamBook holds on the device)."""

    def __init__(self, B, W, n_cap):
        self.B, self.W, self.n_cap = B, W, max(n_cap, 1)
        self.tokens = [[0] * W for _ in range(B)]
        self.parents = [[0] * W for _ in range(B)]
        self.scores = [[np.float32(0.0)] * W for _ in range(B)]
        self.src = [[[w] * self.n_cap for w in range(W)] for _ in range(B)]
        self.pool = [[] for _ in range(B)]             # per sample at most W dicts(score, len, anc, tok), best first
        self.done = [False] * B


def advance_ref(book, cand_score, cand_index, n_cols, V, eos=None, last=False, early_stopping=False, divisor=1.0):
    """One step: cand_score / cand_index [B][2W] (sorted descending) -> the next running beams, parent table and pool.
      running   the first W candidates whose token is not EOS (score copied)
      src       new[w][:n_cols-1] = old[parent][:n_cols-1], new[w][n_cols-1] = parent; later columns untouched
      pool      a candidate among the first W that is EOS (any of them at the last step) enters with score / divisor, length n_cols + 1,
                ancestry old[parent][:n_cols-1] + [parent] and its token -- unless the sample is frozen (done, or early_stopping with
                a pool that was already full); the W best are kept, ties: older entry first, then candidate order (a stable sort)
      done      set once the pool is full and not  best running score / divisor > worst pooled score"""
    W, div = book.W, np.float32(divisor)
    for b in range(book.B):
        cand = [(np.float32(cand_score[b][r]), int(cand_index[b][r]) // V, int(cand_index[b][r]) % V) for r in range(2 * W)]
        old_src = [row[:] for row in book.src[b]]
        run = [c for c in cand if c[2] != eos][:W]
        assert len(run) == W
        for w, (s, p, t) in enumerate(run):
            book.tokens[b][w], book.parents[b][w], book.scores[b][w] = t, p, s
            if n_cols:
                book.src[b][w][:n_cols] = old_src[p][:n_cols - 1] + [p]
        frozen = book.done[b] or (early_stopping and len(book.pool[b]) == W)
        merged = list(book.pool[b])
        if not frozen:
            for s, p, t in cand[:W]:
                if t == eos or last:
                    anc = old_src[p][:n_cols - 1] + [p] if n_cols else []
                    merged.append(dict(score=np.float32(s / div), len=n_cols + 1, anc=anc, tok=t))
        book.pool[b] = sorted(merged, key=lambda e: -e["score"])[:W]             # stable
        if len(book.pool[b]) == W and not (np.float32(run[0][0] / div) > book.pool[b][-1]["score"]):
            book.done[b] = True
    return book


def finalize_ref(book, history, pad, n_new):
    """The best pooled hypothesis per sample: (new tokens [B][n_new] padded with `pad`, score [B]).  history[s][b][w]: the token
    slot w took at step s."""
    ids, scores = [], []
    for b in range(book.B):
        e = book.pool[b][0]
        toks = [int(history[t][b][e["anc"][t]]) for t in range(e["len"] - 1)] + [e["tok"]]
        ids.append(toks + [pad] * (n_new - len(toks)))
        scores.append(e["score"])
    return ids, scores


def beam_search_ref(step_logits, B, W, V, n_new, eos=None, pad=0, length_penalty=1.0, early_stopping=False, observe=None):
    """The whole search on a callable `step_logits(hypotheses) -> float32 log-prob rows`: hypotheses is a list over the live rows
    (B rows at step 0, then B*W) of token lists generated so far; returns [rows, V] log_softmax values (numpy float32).  Scores are
    accumulated in float32 as transformers does.  observe(s, total): called with every step's [B, rows_in * V] accumulated scores.
    Returns (new tokens [B][n_new], scores [B], book)."""
    book = BookRef(B, W, n_new - 1)
    history, hyps = [], [[] for _ in range(B)]
    for s in range(n_new):
        rows_in = 1 if s == 0 else W
        lp = np.asarray(step_logits(hyps), dtype=np.float32).reshape(B, rows_in, V)
        prev = np.zeros((B, 1), np.float32) if s == 0 else np.asarray(book.scores, np.float32)
        total = (lp + prev[:, :, None]).reshape(B, rows_in * V)
        if observe is not None:
            observe(s, total)
        order = np.argsort(-total, axis=1, kind="stable")[:, :2 * W]
        cs = np.take_along_axis(total, order, 1)
        advance_ref(book, cs, order, s, V, eos, s == n_new - 1, early_stopping, float(s + 1) ** length_penalty)
        history.append([row[:] for row in book.tokens])
        hyps = [[int(history[t][b][book.src[b][w][t]]) for t in range(s)] + [book.tokens[b][w]] for b in range(B) for w in range(W)]
    ids, scores = finalize_ref(book, history, pad, n_new)
    return ids, scores, book
