"""References for the neighbor-guidance tests: the contract of mmgl_guidance_logits (include/mmgl_hip.h) restated in
fp64, the per-element bound the GPU test holds the kernel to, and the deliberately wrong variants the CPU test shows that bound to
catch.  Nothing here calls the code under test.

logits [2B, V] in their storage type, read exactly into fp64 (NaN -> -inf).  Rows b and B + b are a pair:
  lc = log_softmax(row b),  lu = log_softmax(row B + b),  score = lu + g (lc - lu)
  a conditional -inf gives -inf; an unconditional -inf under a finite conditional gives lc.

The bound (bound()).  u = 2^-24 is fp32's unit roundoff, eps32 = 2u.  The kernel evaluates in fp32:
  d = x - max                 one rounding, |d| u, which expf turns into a relative error |d| u of that term
  e = expf(d)                 <= 2 ulp = 4u relative
  S = sum e                   n_add = ceil(V / 1024) + 6 + 16 - 1 additions of positive terms: <= n_add u relative on any term
  lse = max + logf(S)         logf <= 1 ulp = 2u |log S|, the addition u |lse|
  The |d| u terms weigh in with the softmax p: sum_v p_v |d_v| = H(p) - log S <= ln V, and log S <= ln V.  So
      |err lse| <= u (L(V) + |lse|),   L(V) = 3 ln V + ceil(V / 1024) + 25        (1 + 2 from the two ln V, 4 + 21 constants)
  lc = xc - lse_c             u |lc| + err lse_c;  lu likewise
  t = lc - lu                 u |t|;  g t: u g |t|;  s = lu + g t: u |s|          with |t| <= |lc| + |lu|, |s| <= |lu| + g (|lc| + |lu|)
  Summed:  |err s| <= u (2 |lu| + 4 g (|lc| + |lu|)) + u ((1 + g)(L + |lse_u|) + g (L + |lse_c|))
                   <= 2 eps32 (g (|lc| + |lu|) + |lu|) + (eps32 / 2) ((1 + g)(L + |lse_u|) + g (L + |lse_c|))
  (a fused multiply-add in s only drops a rounding).  Where the result is lc alone: 2 eps32 |lc| + (eps32 / 2)(L + |lse_c|).
  The store rounds once: half an ulp of the storage type at |reference| + that evaluation term."""
import math

import torch

EPS32 = 2.0 ** -23
VARIANTS = ("pair-adjacent", "swapped", "raw-logits", "g-on-lu")


def read64(logits):
    x = logits.detach().cpu().to(torch.float64)
    return torch.where(torch.isnan(x), torch.full_like(x, -math.inf), x)


def log_softmax64(x):
    """x fp64 [..., V] with at least one finite entry per row -> (x - lse, lse [..., 1])."""
    m = x.max(dim=-1, keepdim=True).values
    lse = m + torch.log(torch.exp(x - m).sum(dim=-1, keepdim=True))
    return x - lse, lse


def reference(logits, B, g, variant=None):
    """dict(score, lc, lu [B, V], lse_c, lse_u [B, 1]) in fp64.  variant: None, or one of VARIANTS -- a wrong implementation:
      pair-adjacent   row b is paired with row b + 1 instead of row B + b
      swapped         lc and lu change places
      raw-logits      the logits themselves in place of the log-probabilities
      g-on-lu         g scales lu: g lu + (lc - lu)"""
    assert variant is None or variant in VARIANTS, variant
    x = read64(logits)
    assert x.shape[0] == 2 * B
    xc = x[:B]
    xu = x[1:B + 1] if variant == "pair-adjacent" else x[B:]
    if variant == "swapped":
        xc, xu = xu, xc
    lc, lse_c = log_softmax64(xc)
    lu, lse_u = log_softmax64(xu)
    a, b = (xc, xu) if variant == "raw-logits" else (lc, lu)
    ninf = torch.full_like(a, -math.inf)
    t = torch.where(torch.isinf(a) | torch.isinf(b), torch.zeros_like(a), a - b)          # no inf - inf
    score = g * b + t if variant == "g-on-lu" else b + g * t
    score = torch.where(torch.isinf(xu), a, score)
    score = torch.where(torch.isinf(xc), ninf, score)
    return dict(score=score, lc=lc, lu=lu, lse_c=lse_c, lse_u=lse_u)


def guided_row_python(xc, xu, g):
    """The same formula on two Python lists of finite floats, with math.fsum: what reference() is checked against."""
    def logp(x):
        m = max(x)
        lse = m + math.log(math.fsum(math.exp(v - m) for v in x))
        return [v - lse for v in x]
    lc, lu = logp(xc), logp(xu)
    return [b + g * (a - b) for a, b in zip(lc, lu)]


def half_ulp(mag, dtype):
    """Half the spacing of `dtype` (bf16 / fp32) at the magnitudes mag (fp64, finite)."""
    bits = {torch.bfloat16: 7, torch.float32: 23}[dtype]
    _, e = torch.frexp(mag.clamp_min(2.0 ** -126))                   # mag = m 2^e, m in [0.5, 1): floor(log2 mag) = e - 1
    return torch.ldexp(torch.ones_like(mag), e - 1 - bits - 1)


def bound(ref, g, V, dtype):
    """Per-element bound [B, V] on |kernel - ref['score']| (module docstring); 0 where the reference is -inf (it must be met exactly)."""
    L = 3.0 * math.log(V) + math.ceil(V / 1024) + 25.0
    lc, lu = ref["lc"].abs(), ref["lu"].abs()
    lse_c, lse_u = ref["lse_c"].abs(), ref["lse_u"].abs()
    both = 2 * EPS32 * (g * (lc + lu) + lu) + EPS32 / 2 * ((1 + g) * (L + lse_u) + g * (L + lse_c))
    only_c = 2 * EPS32 * lc + EPS32 / 2 * (L + lse_c)
    ev = torch.where(torch.isinf(lu), only_c, both)
    dead = torch.isinf(ref["score"])
    ev = torch.where(dead, torch.zeros_like(ev), ev)
    mag = torch.where(dead, torch.zeros_like(ev), ref["score"].abs()) + ev
    return torch.where(dead, torch.zeros_like(ev), half_ulp(mag, dtype) + ev)


def kernel_inputs(B, V, dtype, seed, scale=3.0):
    """[2B, V] logits in `dtype` on the CPU: independent rows, so the two distributions of a pair differ by O(scale) per element."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(2 * B, V, generator=g) * scale).to(dtype)
