"""References for the sampling tests: the contract of mmgl_sample_tokens (include/mmgl_hip.h) restated in fp64 numpy,
and the bounds the GPU tests hold the kernel to.  Nothing here calls the code under test.

x = logit / temperature is computed in fp32 (one IEEE division, as the kernel does) and everything after it in fp64:
  top-k   v survives iff fewer than k tokens have x > x_v                (ties with the k-th are kept)
  top-p   a survivor v is kept iff above(v) < top_p, above(v) = the softmax mass, over the survivors, of those with x > x_v
  draw    the smallest kept v, in vocabulary index order, with C_v > u Z_K, C the running sum of exp(x - max) over the kept set
"""
import math

import numpy as np
import torch


def scaled(logits, temperature):
    """logits: a torch tensor [..., V] (bf16 / fp32).  x = fp32(logit) / fp32(temperature) + 0, as fp64 numpy; NaN -> -inf."""
    x = (logits.detach().float().cpu() / torch.tensor(float(temperature), dtype=torch.float32) + 0.0).numpy().astype(np.float64)
    return np.where(np.isnan(x), -np.inf, x)


def warp_row(x, top_k, top_p):
    """x: fp64 [V].  Returns (survivors of top-k [V] bool, above [V] fp64 (1.0 outside the survivors), kept [V] bool)."""
    V = x.shape[0]
    surv = np.ones(V, dtype=bool)
    if 0 < top_k < V:
        kth = np.sort(x)[V - top_k]
        surv = x >= kth
    mx = x.max()
    p = np.where(surv, np.exp(x - mx), 0.0) if np.isfinite(mx) else surv.astype(np.float64)
    order = np.argsort(-x, kind="stable")
    xs, ps = x[order], p[order]
    excl = np.concatenate([[0.0], np.cumsum(ps)[:-1]])
    first = np.searchsorted(-xs, -x, side="left")              # the first sorted position holding x_v: everything before it is larger
    above = np.where(surv, excl[first] / ps.sum(), 1.0)
    kept = surv & ((above < top_p) | (x == mx))
    return surv, above, kept


def eps_p(V):
    """Bound on |kernel mass ratio - exact mass ratio|.  A mass is the integer trunc(2^40 expf(fl(x - max))) and
    integer sums are exact, so a term's relative error is |x - max| 2^-24 (the subtraction's rounding, carried through exp) plus
    2^-22 (expf within 2 ulp; the library documents 1) and its absolute error 2^-40 (the truncation).  Weighted by the softmax,
    sum p |x - max| / Z = H - ln Z <= ln V, so a sum of masses over Z is off by at most d = 2^-24 ln V + 2^-22 + V 2^-40, and a
    ratio of two such sums by 2 d (to first order; d < 2e-6)."""
    d = 2.0 ** -24 * math.log(max(V, 2)) + 2.0 ** -22 + V * 2.0 ** -40
    return 2.0 * d


def eps_u(V):
    """Bound for the draw: eps_p plus the 2^-32 the kernel's floor(u 2^32) may drop and one unit of 2^-40 in the target."""
    return eps_p(V) + 2.0 ** -30


def kept_bounds(surv, above, top_p, eps):
    """(lo, hi) for the kernel's kept count: #{above < top_p - eps} and #{above < top_p + eps} over the survivors (at least 1)."""
    lo = int((surv & (above < top_p - eps)).sum())
    hi = int((surv & (above < top_p + eps)).sum())
    return max(lo, 1), max(hi, 1)


def top_set(x, n):
    """The n largest of x as a bool mask, and whether n is a whole number of tie groups (the n-th and (n+1)-th differ)."""
    order = np.argsort(-x, kind="stable")
    mask = np.zeros(x.shape[0], dtype=bool)
    mask[order[:n]] = True
    whole = n == x.shape[0] or x[order[n - 1]] != x[order[n]]
    return mask, bool(whole)


def cdf(x, kept):
    """Index-order running sum C [V] of exp(x - max) over the kept set, normalised to C[-1] = 1."""
    mx = x[kept].max()
    p = np.where(kept, np.exp(x - mx), 0.0) if np.isfinite(mx) else kept.astype(np.float64)
    c = np.cumsum(p)
    return c / c[-1]


def draw_ok(c, kept, u, tok, eps):
    """The kernel criterion: tok is kept and C_{tok-1} - eps <= u < C_tok + eps."""
    if not (0 <= tok < c.shape[0]) or not kept[tok]:
        return False
    below = c[tok - 1] if tok > 0 else 0.0
    return below - eps <= u < c[tok] + eps


def eos_ref(tokens, finished, eos, pad):
    """The greedy loops' bookkeeping in plain Python: a finished draw gets pad; a draw that returns eos becomes finished."""
    out, fin = [], list(finished)
    for i, t in enumerate(tokens):
        if fin[i]:
            out.append(pad)
        else:
            out.append(t)
            if eos is not None and t == eos:
                fin[i] = 1
    return out, fin
