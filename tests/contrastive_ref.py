"""Contrastive search (Su et al. 2022, "A Contrastive Framework for Neural Text Generation"), restated from the published algorithm in
fp64 for the tests of ops.contrastive_select and generate(penalty_alpha, top_k):

    score(c) = (1 - alpha) p(c) - alpha max_j cos(h_c, h_j),   j over the context's hidden rows,

the lowest c among the maxima wins, a NaN score never does.  The cosine is 0 when either vector has norm 0 and the penalty is 0 for an
empty context.  Masked prompt columns are no context.  Two layers: the ranking alone (rank_ref, on given hidden rows)
and a model-level step that runs the model UNCACHED over prompt + chosen tokens + one candidate (step_ref / search_ref)."""
import torch


def penalty_ref(cand, ctx, valid):
    """cand [k, d], ctx [n, d], valid [n] (bool) -> max_j cos(cand_c, ctx_j) over the valid rows, fp64 [k]; 0 without a valid row."""
    cand, ctx = cand.double(), ctx.double()[valid.bool()]
    if ctx.shape[0] == 0:
        return torch.zeros(cand.shape[0], dtype=torch.float64)
    nc, nx = cand.norm(dim=1), ctx.norm(dim=1)
    den = nc[:, None] * nx[None, :]
    cos = torch.where(den > 0, (cand @ ctx.t()) / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
    cos = torch.where(torch.isnan(cos), torch.full_like(cos, float("-inf")), cos)
    pen = cos.amax(dim=1)
    return torch.where(torch.isinf(pen), torch.zeros_like(pen), pen)


def select_ref(score):
    """Lowest index among the maxima of score [k]; NaN never wins (all NaN: 0)."""
    best, sel = None, 0
    for c, s in enumerate(score.tolist()):
        if s == s and (best is None or s > best):
            best, sel = s, c
    return sel


def rank_ref(logp, cand, ctx, valid, alpha):
    """One sample: logp [k] candidate log-probabilities, cand [k, d], ctx [n, d], valid [n].  Returns dict(p, penalty, score fp64 [k],
    selected int, margin = best score - second best)."""
    p = torch.exp(logp.double())
    pen = penalty_ref(cand, ctx, valid)
    score = (1.0 - alpha) * p - alpha * pen
    top = torch.sort(score[~torch.isnan(score)], descending=True).values
    margin = float(top[0] - top[1]) if top.numel() > 1 else float("inf")
    return dict(p=p, penalty=pen, score=score, selected=select_ref(score), margin=margin)


def step_ref(hidden_fn, head_fn, ids, am, chosen, cands, alpha):
    """One step of the model-level restatement.  hidden_fn(ids [B, L], mask [B, L]) -> last_hidden_state [B, L, d] (uncached);
    head_fn(h [B, d]) -> logits [B, V]; ids / am [B, T]: the prompt; chosen [B, s]: the tokens chosen so far; cands [B, k]: the
    candidate tokens to rank (the product's own, by the comparison rule of DESIGN.md 4.8).
    Returns dict(logits [B, V], p, penalty, score fp64 [B, k], selected [B], margin [B])."""
    B, T = ids.shape
    s, k = chosen.shape[1], cands.shape[1]
    seq = torch.cat([ids, chosen], 1)
    mask = torch.cat([am, torch.ones(B, s, dtype=am.dtype)], 1)
    logits = head_fn(hidden_fn(seq, mask)[:, -1]).double()
    logp = torch.log_softmax(logits, -1).gather(1, cands.long())
    one = torch.ones(B, 1, dtype=am.dtype)
    # one uncached run per candidate slot: rows [0, T + s) are the context (causal: the same for every candidate), the last row is h_c
    runs = [hidden_fn(torch.cat([seq, cands[:, c:c + 1].long()], 1), torch.cat([mask, one], 1)).double() for c in range(k)]
    out = dict(logits=logits, p=[], penalty=[], score=[], selected=[], margin=[])
    for b in range(B):
        r = rank_ref(logp[b], torch.stack([runs[c][b, -1] for c in range(k)]), runs[0][b, :T + s], mask[b] != 0, alpha)
        for key in ("p", "penalty", "score", "selected", "margin"):
            out[key].append(r[key])
    for key in ("p", "penalty", "score"):
        out[key] = torch.stack(out[key])
    out["selected"], out["margin"] = torch.tensor(out["selected"]), torch.tensor(out["margin"], dtype=torch.float64)
    return out


def search_ref(hidden_fn, head_fn, ids, am, n_new, k, alpha):
    """The whole search on the reference's own tokens.  Returns (new tokens [B, n_new], the list of step_ref dicts)."""
    B = ids.shape[0]
    chosen, steps = torch.zeros(B, 0, dtype=torch.int64), []
    for _ in range(n_new):
        seq = torch.cat([ids, chosen], 1)
        mask = torch.cat([am, torch.ones(B, chosen.shape[1], dtype=am.dtype)], 1)
        logits = head_fn(hidden_fn(seq, mask)[:, -1]).double()
        cands = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :k]
        st = step_ref(hidden_fn, head_fn, ids, am, chosen, cands, alpha)
        st["candidates"] = cands
        steps.append(st)
        chosen = torch.cat([chosen, cands.gather(1, st["selected"][:, None])], 1)
    return chosen, steps
