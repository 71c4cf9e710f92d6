"""fp64 references of the attention kernels: causal self-attention, masked cross-attention, general attention, packed encoder attention."""
import numpy as np
import torch

from bounds import U, _keep_scale, check_bound, check_bounds, first_indices, hash_keep, outside, row_head, sample_head_row
from row_ref import NormRef


# ------------------------------------------------------------------------------------------ causal self-attention (csrc/selfattn*.hip)
class SelfAttnRef:
    """fp64 reference of causal self-attention, forward and backward, on the device the (storage-rounded) operands live on, with the
    arguments of the kernels: q [B,T,H*D] already scaled, k, v [B,P+T,Hkv*D], key_valid [B,P+T], dout [B,T,H*D].  Key s is allowed
    for query t iff s <= t + P and key_valid[b,s] (key 0 is always valid: include/mmgl_hip.h); query head h reads kv head h // G.
    One (sample, head) at a time: T = 4097 needs one set of T x T fp64 matrices at once.

    With p = softmax over the allowed keys, dp = dO V^T, delta = sum_d dO O, Delta_i = sum_d |dO_id| |O_id| and
    S_i = max_j sum_d |q_id| |k_jd| over the allowed keys, `want` and `mag` of out, lse, dq, dk, dv are
        out = p V                       mag_out_i = sum_j p_ij |v_j|
        dv  = p^T dO                    mag_dv_j  = sum_i p_ij |dO_i|
        dq  = (p (dp - delta)) K        mag_dq_i  = sum_j p_ij (|dp_ij| + Delta_i) |k_j|
        dk  = (p (dp - delta))^T Q      mag_dk_j  = sum_i p_ij (|dp_ij| + Delta_i) |q_i|      (GQA: summed over the group's query heads)

    Per-element bound (every element is checked), a function of the reference alone, never of the kernel's output:
        |got - want| <= u |want| + (c + n 2^-24 S_i) mag            u = 2^-8 (bf16), 2^-23 (fp32)
        |lse_got - lse_want| <= n 2^-24 S_i + 2^-20                 (lse is fp32 for both dtypes)
    For dk, dv S_i is the largest S of the rows that reach key j (with GQA taken per query head, so the term is the group's sum of
    S mag), and GQA dk, dv also get u sum_g |per-head want|: each query head's gradient is stored once in the operand dtype before
    gqa_fold_kernel sums the group.  The count behind the constants:
      * u |want| is the half ulp of the one round-to-nearest store of the fp32 result.
      * c counts the roundings of the matrix operands.  bf16, c = 2^-7: P (forward, dV) and dS (dQ, dK) enter the second MFMA rounded
        to bf16, 2^-8 each, and delta is formed from the bf16-stored `out`, 2^-8 on Delta (hence Delta in mag_dq, mag_dk): 2^-8, counted
        with a factor 2 of room.  fp32, c = 2^-16: 256 fp32 roundings of 2^-24 on the magnitude sum, SkinnyRef's rationale.
      * n 2^-24 S_i mag is the fp32 error of a score, which reaches p through the exponent: n roundings of 2^-24 relative to
        sum_d |q||k| <= S_i.  n = 8 + D / kb: 8 for the LOG2E scale, the subtraction of the scaled maximum (itself a rounded
        product), exp2 (1 ulp), the sum and the logarithm of l, lse's own store and its LOG2E scale in the backward; D / kb for the
        fp32 accumulator, rounded once per MFMA k-block of kb products -- kb = 4 for mfma_f32_16x16x4f32 (fp32 operands: 32 chained
        accumulations at D = 128), kb = 16 for the bf16 MFMAs (32x32x16; a 16x16x32 counts as two).  (The first statement of this
        bound had n = 8 for every kernel; the fp32 kernels at D >= 32 reached 1.3-1.7 times that in lse on an MI355X, which is the
        accumulation chain it left out.)
    The constants are derived, not fitted to a GPU run; c may grow to 2^-6 (bf16) for a rounding that is found and counted, no
    further.  `allowed` [B,T,P+T] (bool) and `kv_head` (h -> kv head) replace the mask and the head mapping: the deliberately wrong
    references of tests/test_selfattn_ref_cpu.py."""
    NAMES = ("out", "lse", "dq", "dk", "dv")
    RAMP = 0.5                                        # slope of the recency ramp (inputs)
    C = {torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -16}

    @staticmethod
    def inputs(dtype, B, T, H, D, Hkv=None, P=0, seed=0, ramp=True, device="cpu"):
        """q, k, v, dout in `dtype`: randn, q scaled by 2 D^-0.5.  ramp: q[..., 0] = 1 in every head and k[..., 0] = 0.5 s for key
        position s (prefix included): the newest allowed key carries about 40 % of every row's weight at any T, so a key that leaks
        in or drops out at an edge moves the row far outside the bound (plain randn: weight 1 / t), and the running maximum of the
        online softmax lies in the last tile."""
        Hkv = Hkv or H
        g = torch.Generator().manual_seed(seed)
        q = torch.randn(B, T, H, D, generator=g) * (2 * D ** -0.5)
        k, v = torch.randn(B, P + T, Hkv, D, generator=g), torch.randn(B, P + T, Hkv, D, generator=g)
        dout = torch.randn(B, T, H, D, generator=g)
        if ramp:
            q[..., 0] = 1.0
            k[..., 0] = SelfAttnRef.RAMP * torch.arange(P + T, dtype=torch.float32)[None, :, None]
        return tuple(t.reshape(B, t.shape[1], -1).to(dtype).to(device) for t in (q, k, v, dout))

    @staticmethod
    def mask(B, T, layout="M0", L=None, P=0):
        """key_valid [B,P+T] uint8 (host), the P prefix keys and key 0 always valid.  M0: all valid.  M1: the last sample right-padded
        to valid length L.  M2: the WikiWeb2M layout prompt | pad | summary | pad in sample 0, hole edges at 70 and T - T // 5."""
        am = torch.ones(B, P + T, dtype=torch.uint8)
        if layout == "M1":
            assert 1 <= L < T
            am[B - 1, P + L:] = 0
        elif layout == "M2":
            assert 70 < T - T // 5 < T - T // 10
            am[0, P + 70:P + T - T // 5] = 0
            am[0, P + T - T // 10:] = 0
            if B > 1:
                am[1, P + T // 3:] = 0
        else:
            assert layout == "M0"
        return am

    @staticmethod
    def allowed(key_valid, T, P=0):
        """[B,T,P+T] bool: key s is allowed for query t iff s <= t + P and key_valid[b,s]."""
        s = torch.arange(P + T, device=key_valid.device)[None, :]
        t = torch.arange(T, device=key_valid.device)[:, None]
        return (s <= t + P)[None] & key_valid.bool()[:, None, :]

    def __init__(self, q, k, v, key_valid, dout, num_heads, num_kv_heads=None, prefix_len=0, allowed=None, kv_head=None):
        B, T, d = q.shape
        H, Hkv, P = num_heads, num_kv_heads or num_heads, prefix_len
        D, G, Tk = d // H, H // Hkv, k.shape[1]
        assert Tk == P + T and k.shape[2] == Hkv * D
        kv_head = kv_head or (lambda h: h // G)
        ok = (SelfAttnRef.allowed(key_valid, T, P) if allowed is None else allowed).to(q.device)
        q4, k4, v4, g4 = q.reshape(B, T, H, D), k.reshape(B, Tk, Hkv, D), v.reshape(B, Tk, Hkv, D), dout.reshape(B, T, H, D)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=q.device)
        self.B, self.T, self.Tk, self.H, self.Hkv, self.D, self.P = B, T, Tk, H, Hkv, D, P
        self.S = z(B, H, T)
        self.want = dict(out=z(B, T, H, D), lse=z(B, H, T), dq=z(B, T, H, D), dk=z(B, Tk, Hkv, D), dv=z(B, Tk, Hkv, D))
        self.mag = {n: torch.zeros_like(self.want[n]) for n in ("out", "dq", "dk", "dv")}
        self.smag = {n: torch.zeros_like(self.want[n]) for n in ("out", "dq", "dk", "dv")}       # sum of S mag
        self.habs = {n: torch.zeros_like(self.want[n]) for n in ("dk", "dv")}                    # sum_g |per-head want|
        for b in range(B):
            A = ok[b]
            for h in range(H):
                hk = kv_head(h)
                Q, K, V, dO = q4[b, :, h].double(), k4[b, :, hk].double(), v4[b, :, hk].double(), g4[b, :, h].double()
                S = (Q.abs() @ K.abs().t()).masked_fill_(~A, 0.0).amax(1)
                p = (Q @ K.t()).masked_fill_(~A, float("-inf"))
                lse = torch.logsumexp(p, 1)
                p = p.sub_(lse[:, None]).exp_()
                O = p @ V
                dp = dO @ V.t()
                delta, Delta = (dO * O).sum(1), (dO.abs() * O.abs()).sum(1)
                w = p * dp.abs().add_(Delta[:, None])
                ds = dp.sub_(delta[:, None]).mul_(p)
                Sk = torch.where(A, S[:, None], S.new_zeros(())).amax(0)[:, None]
                self.S[b, h], self.want["lse"][b, h] = S, lse
                for n, x, m in (("out", O, p @ V.abs()), ("dq", ds @ K, w @ K.abs())):
                    self.want[n][b, :, h], self.mag[n][b, :, h], self.smag[n][b, :, h] = x, m, S[:, None] * m
                for n, x, m in (("dk", ds.t() @ Q, w.t() @ Q.abs()), ("dv", p.t() @ dO, p.t() @ dO.abs())):
                    self.want[n][b, :, hk] += x
                    self.mag[n][b, :, hk] += m
                    self.smag[n][b, :, hk] += Sk * m
                    self.habs[n][b, :, hk] += x.abs()
                del p, dp, w, ds

    def bound(self, name, dtype):
        """The bound of tensor `name`, shaped like want[name] ([B,rows,heads,D]; lse [B,H,T])."""
        n = (8 + self.D // (16 if dtype == torch.bfloat16 else 4)) * 2.0 ** -24
        if name == "lse":
            return n * self.S + 2.0 ** -20
        b = U[dtype] * self.want[name].abs() + SelfAttnRef.C[dtype] * self.mag[name] + n * self.smag[name]
        if name in self.habs and self.Hkv < self.H:
            b = b + U[dtype] * self.habs[name]
        return b

    def outside(self, other, name, dtype):
        """From two references alone: the elements (bool, shaped like want[name]) at which `other` -- a deliberately wrong reference
        of the same call -- leaves this one's bound."""
        return outside(self.want[name], other.want[name], self.bound(name, dtype))

    def check(self, got, what, group="", dtype=None):
        """Asserts the bound on every element of got = (out, lse, dq, dk, dv) (any may be None: skipped); prints the largest
        err / bound of each and returns them by name."""
        dtype = dtype or got[0].dtype
        return check_bounds(((name, x, self.want[name], self.bound(name, dtype), sample_head_row, None)
                             for name, x in zip(SelfAttnRef.NAMES, got) if x is not None), what, group)


# ------------------------------------------------------------------------------------------ masked cross-attention (csrc/xattn.hip)
class XAttnRef(SelfAttnRef):
    """fp64 reference of mmgl_xattn_fwd / mmgl_xattn_bwd on the device the (storage-rounded) operands live on, with the arguments of
    the ABI: q [B,T,H*D] already scaled, k, v [B,S,H*D], key_valid [B,S], dout [B,T,H*D].  One (sample, head) at a time.

    Semantics (oracle.lm_ref.expand_mask + attention_core):
      * a sample with a valid key: p = softmax over its valid keys; a masked key gets exactly zero dk and dv.
      * a sample with no valid key: p = 1 / S on all S keys (every score clamps to finfo.min), and dS is multiplied by 0.5 -- autograd's
        split at the torch.maximum tie -- so dq and dk are halved, dv is not.  lse is the kernel's m + log l with m = 0: log S
        (include/mmgl_hip.h; the oracle's finfo.min + log S is another convention for the same row).

    With dp = dO V^T, delta = sum_j p dp, Delta_i = sum_j p_ij |dp_ij| and S_i = max_j sum_d |q_id| |k_jd| over the valid keys (0 for a
    sample with none: no score is formed), `want` and `mag` of out, lse, dq, dk, dv are those of SelfAttnRef with the weight
    w = tie p (|dp| + Delta):
        out = p V                 mag_out = p |V|              dq = (tie p (dp - delta)) K        mag_dq = w |K|
        dv  = p^T dO              mag_dv  = p^T |dO|           dk = (tie p (dp - delta))^T Q      mag_dk = w^T |Q|
    (Delta is sum p |dp| here, not sum |dO| |O|: these kernels form delta from p and dP in fp32 and never read `out` back.)

    Per-element bound (every element is checked), a function of the reference alone, never of the kernel's output:
        |got - want| <= u |want| + (c + n 2^-24 (S_i + ln S)) mag
        |lse_got - lse_want| <= n 2^-24 (S_i + ln S) + 2^-20
    u, c and n = 8 + D / kb are SelfAttnRef's, for its reasons: P and dS enter the second MFMA rounded to bf16, the score's fp32 error
    reaches p through the exponent, the accumulator rounds once per MFMA k-block.  The ln S term is this file's: the backward forms
    p = exp2(s LOG2E - lse LOG2E), two rounded products whose error is relative to |lse| <= S_i + ln S, not to the score alone.
    For dk / dv, S_i is the largest of the rows that reach the key: every row of the (sample, head).

    The keyword arguments build the deliberately wrong references of tests/test_xattn_ref_cpu.py: `allowed` [B,S] replaces the mask;
    `exists` [B,S] the keys a sample without a valid key spreads over; `uniform_n` (sample -> int) the count it divides by; `tie` the
    factor on dS there; `kv_head` (h -> head whose keys and values head h reads); `rows_kv` [T] the query rows that reach dk / dv."""
    EDGES = (0, 15, 16, 31, 32, 63, 64, 127, 128)
    BOOST, FACTOR = 4.0, 16.0        # k[edge key, 0] and the factor on dout's edge rows

    @staticmethod
    def edges(n):
        """The edge indices of a dimension of n: EDGES, n - 2, n - 1 and the first index of the last group of 32 (192 at n = 200: no
        member of EDGES, and the first key of the last dK / dV wave or key block), where they exist."""
        return sorted({e for e in XAttnRef.EDGES + (n - 2, n - 1, 32 * ((n - 1) // 32)) if 0 <= e < n})

    @staticmethod
    def inputs(dtype, B, T, S, H, D, seed=0, edge=True, device="cpu"):
        """q, k, v, dout in `dtype`: randn, q scaled by 2 D^-0.5.  edge: q[..., 0] = 1 in every head, k[s, 0] = BOOST on the edge keys
        and 0 elsewhere -- at most 12 keys share e^4 : 1 against the others, so an edge key carries several percent of every row at any
        S (plain randn at S = 256: 0.4 %) -- and dout times FACTOR on the edge rows, so a query row lost from dk / dv shows."""
        g = torch.Generator().manual_seed(seed)
        q = torch.randn(B, T, H, D, generator=g) * (2 * D ** -0.5)
        k, v = torch.randn(B, S, H, D, generator=g), torch.randn(B, S, H, D, generator=g)
        dout = torch.randn(B, T, H, D, generator=g)
        if edge:
            q[..., 0] = 1.0
            k[..., 0] = 0.0
            k[:, XAttnRef.edges(S), :, 0] = XAttnRef.BOOST
            dout[:, XAttnRef.edges(T)] *= XAttnRef.FACTOR
        return tuple(t.reshape(B, t.shape[1], -1).to(dtype).to(device) for t in (q, k, v, dout))

    @staticmethod
    def mask(B, S, first=0):
        """key_valid [B,S] uint8 (host).  Sample b has layout (first + b) % 3:  0 all valid;  1 holed: key S - 1, the edge keys 15, 32,
        64 and 128 and every key s % 5 == 3 masked (key 0 stays, and S = 1 keeps its one key);  2 no valid key."""
        am = torch.ones(B, S, dtype=torch.uint8)
        s = torch.arange(S)
        for b in range(B):
            lay = (first + b) % 3
            if lay == 1 and S > 1:
                am[b, (s % 5 == 3) | (s == S - 1) | (s == 15) | (s == 32) | (s == 64) | (s == 128)] = 0
                am[b, 0] = 1
            elif lay == 2:
                am[b] = 0
        return am

    def __init__(self, q, k, v, key_valid, dout, num_heads, allowed=None, exists=None, uniform_n=None, tie=0.5, kv_head=None, rows_kv=None):
        B, T, d = q.shape
        H, S = num_heads, k.shape[1]
        D = d // H
        assert k.shape == v.shape == (B, S, d) and dout.shape == q.shape and key_valid.shape == (B, S)
        dev = q.device
        ok = (key_valid if allowed is None else allowed).to(dev).bool()
        ex = torch.ones(B, S, dtype=torch.bool, device=dev) if exists is None else exists.to(dev).bool()
        uniform_n = uniform_n or (lambda b: S)
        kv_head = kv_head or (lambda h: h)
        rk = torch.ones(T, dtype=torch.float64, device=dev) if rows_kv is None else rows_kv.to(dev).double()
        q4, k4, v4, g4 = q.reshape(B, T, H, D), k.reshape(B, S, H, D), v.reshape(B, S, H, D), dout.reshape(B, T, H, D)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
        self.B, self.T, self.Tk, self.H, self.Hkv, self.D, self.P = B, T, S, H, H, D, 0
        self.S = z(B, H, T)                               # S_i + ln S: what a score rounding is relative to
        self.want = dict(out=z(B, T, H, D), lse=z(B, H, T), dq=z(B, T, H, D), dk=z(B, S, H, D), dv=z(B, S, H, D))
        self.mag = {n: torch.zeros_like(self.want[n]) for n in ("out", "dq", "dk", "dv")}
        self.smag = {n: torch.zeros_like(self.want[n]) for n in ("out", "dq", "dk", "dv")}
        self.habs = {}
        lnS = float(np.log(S))
        for b in range(B):
            A = ok[b]
            live = bool(A.any())
            for h in range(H):
                hk = kv_head(h)
                Q, K, V, dO = q4[b, :, h].double(), k4[b, :, hk].double(), v4[b, :, hk].double(), g4[b, :, h].double()
                if live:
                    Si = (Q.abs() @ K.abs().t())[:, A].amax(1) + lnS
                    sc = (Q @ K.t()).masked_fill_(~A[None, :], float("-inf"))
                    lse = torch.logsumexp(sc, 1)
                    p, f = sc.sub_(lse[:, None]).exp_(), 1.0
                else:
                    n = uniform_n(b)
                    Si = z(T) + lnS
                    lse = z(T) + float(np.log(n))
                    p, f = (ex[b].double() / n)[None, :].expand(T, S).contiguous(), tie
                O = p @ V
                dp = dO @ V.t()
                delta, Delta = (p * dp).sum(1), (p * dp.abs()).sum(1)
                w = p * dp.abs().add(Delta[:, None]) * f
                ds = dp.sub(delta[:, None]).mul_(p).mul_(f)
                Sk = Si.max()
                self.S[b, h], self.want["lse"][b, h] = Si, lse
                for n, x, m in (("out", O, p @ V.abs()), ("dq", ds @ K, w @ K.abs())):
                    self.want[n][b, :, h], self.mag[n][b, :, h], self.smag[n][b, :, h] = x, m, Si[:, None] * m
                pk, dsk, wk = p * rk[:, None], ds * rk[:, None], w * rk[:, None]
                for n, x, m in (("dk", dsk.t() @ Q, wk.t() @ Q.abs()), ("dv", pk.t() @ dO, pk.t() @ dO.abs())):
                    self.want[n][b, :, hk] += x
                    self.mag[n][b, :, hk] += m
                    self.smag[n][b, :, hk] += Sk * m

    def bound(self, name, dtype):
        """The bound of tensor `name`, shaped like want[name] ([B,rows,H,D]; lse [B,H,T])."""
        n = (8 + self.D // (16 if dtype == torch.bfloat16 else 4)) * 2.0 ** -24
        if name == "lse":
            return n * self.S + 2.0 ** -20
        return U[dtype] * self.want[name].abs() + SelfAttnRef.C[dtype] * self.mag[name] + n * self.smag[name]


# ------------------------------------------------------------------------------------------ general attention (csrc/attn_general.hip)
class GeneralAttnRef(XAttnRef):
    """fp64 reference of mmgl_attn_general_fwd / _bwd on the device the (storage-rounded) operands live on, with the arguments of the
    ABI: q [B,T,H*D] already scaled, k, v [B,S,H*D], key_valid [B,S], dout [B,T,H*D], head_mask [H] or None, causal, p_drop, seed.
    One (sample, head) at a time.

    Semantics (the header of csrc/attn_general.hip; oracle.lm_ref.attention_core with expand_mask / decoder_self_mask):
      * key s is allowed for row t iff key_valid[b,s] (and s <= t when causal).  A ROW without an allowed key has p = 1 / S on all S keys,
        future and padded ones included, and lse = +inf (the marker the backward keys off); every other row is a softmax over its
        allowed keys and lse = log sum exp.
      * W = head_mask[h] p (the `probs` output), Wd = W keep fp32(1 / (1 - p_drop)) with keep = hash_keep(seed, ...) at element index
        ((b H + h) T + t) S + s -- never the library's own mask --, out = Wd V.
      * dWd = dO V^T, delta = sum_s dWd Wd, dS = f p (hm keep / (1 - p) dWd - delta), f = 1 except on a row without an allowed key:
        0.5 there (autograd's split at the torch.maximum tie) and 0 on its keys that are both future and padded (finfo.min +
        finfo.min = -inf: the clamp constant wins outright).  dq = dS K, dk = dS^T Q, dv = Wd^T dO.

    want / mag are XAttnRef's with the head mask and the keep scale carried: with ks = keep / (1 - p), Delta = sum_s |dWd| |Wd| and
    w = f p (|hm| ks |dWd| + Delta),
        out = Wd V          mag = |Wd| |V|            dq = dS K          mag = w |K|
        dv  = Wd^T dO       mag = |Wd|^T |dO|         dk = dS^T Q        mag = w^T |Q|
    S_i = max over the allowed keys of sum_d |q_id| |k_jd|, + ln S (0 + ln S on a row without an allowed key: no score is formed); for
    dk / dv the largest S_i of the (sample, head).

    Per-element bound (every element is checked), a function of the reference alone:
        |got - want| <= u |want| + (c(len) + n 2^-24 (S_i + ln S)) mag          c(len) = max(2^-16, 2 len 2^-24)   (NormRef.c)
        |lse - want| <= n 2^-24 (S_i + ln S) + 2^-20                            (rows with an allowed key; the others: exactly +inf)
        |probs - want| <= u |want| + n 2^-24 (S_i + ln S) |want| + 2^-126 |hm|  (rows without an allowed key: exactly dtype(fp32(1 / S) hm))
    The count, from csrc/attn_general.hip -- all arithmetic is fp32 on the VALU for both dtypes, bf16 appears only in the one store of
    out, probs, dq, dk, dv, so c is the same for both:
      * u = 2^-8 (bf16) / 2^-23 (fp32): the half ulp of that one store (fp32: its last operation, counted at one ulp).
      * n = D + 8.  ag_dot is a chain of D fmaf, one rounding each relative to sum_d |q||k| <= S_i; 8 for the subtraction of the
        running maximum or of lse, __expf's LOG2E product and its exp2 (1 ulp = 2), the wave and chunk sums of l (positive terms: a
        relative error), __logf's log2 and LN2 product, and lse's own fp32 store, which the backward and pass 2 read back: these are
        relative to |lse| <= S_i + ln S.  (Not 8 + D / kb: no MFMA accumulates k-blocks here.)
      * c(len) counts the fp32 accumulation chains, 2 roundings of 2^-24 per link (the fmaf and its operand's own product), floor 2^-16
        (SkinnyRef's 256 roundings).  out: the S fmaf of acc over all key chunks, + 4 (hm p, the keep scale).  dv: the T fmaf over the
        row chunks of 32, + 4.  dq: S, + D for dWd's own ag_dot (relative to sum |dO||V|, which |dWd| stands for), + 6 + ceil(S / 64)
        for delta (wave_sum's 6 steps per chunk, the chunk adds), + 8.  dk: T + D + 6 + ceil(S / 64) + 8.
      * 2^-126 |hm| in probs, on the elements whose reference is not zero: __expf is v_exp_f32 of the LOG2E product, which flushes a
        result below the smallest normal fp32 to zero, so a probability under 2^-126 (key 0 seen from row 170 of the ramp: e^-85) is
        stored as 0.  The first statement of the bound had no such term and was relative only; an MI355X run left it on 851 of 360000
        probabilities at T = 200, all of them below 2^-126.  out, dq, dk, dv carry c mag, which dwarfs it.
    The constants are derived, not fitted; only a rounding found in the code and named may be added.

    Keyword arguments build the deliberately wrong references of tests/test_attn_general_ref_cpu.py: `keep` [B,H,T,S] (bool) replaces the
    hash mask (GeneralAttnRef.keep builds the shifted / transposed ones); `keep_scale` the factor 1 / (1 - p); `hm_of` (h -> index into
    head_mask); `hm_in_delta` False leaves the head mask out of delta; `uniform_keys` [B,S] the keys a row without an allowed key
    spreads over (it divides by their count); `tie`, `tie_double` the factors f; `allowed` [B,T,S] replaces the mask of the rows that
    have an allowed key (which rows have none is still decided by the true mask); `rows_kv` [T] the rows that reach dk / dv."""
    NAMES = ("out", "lse", "dq", "dk", "dv")
    EDGES = (0, 31, 32, 33, 63, 64, 65, 127, 128, 129)

    @staticmethod
    def edges(n):
        """The seams of AG_RB = 32, AG_ROWS = AG_KC = 64 on either side, n - 1 and the first index of the last group of 32."""
        return sorted({e for e in GeneralAttnRef.EDGES + (n - 1, 32 * ((n - 1) // 32)) if 0 <= e < n})

    @staticmethod
    def inputs(dtype, B, T, S, H, D, causal=False, seed=0, device="cpu"):
        """q, k, v, dout in `dtype`: randn, q scaled by 2 D^-0.5, q[..., 0] = 1; dout times FACTOR on the edge rows.  Cross: k[s, 0] =
        BOOST on the edge keys and 0 elsewhere (XAttnRef.inputs' recipe at this kernel's seams).  Causal: SelfAttnRef's recency ramp
        k[s, 0] = RAMP s, so the newest allowed key carries about 40 % of every row."""
        g = torch.Generator().manual_seed(seed)
        q = torch.randn(B, T, H, D, generator=g) * (2 * D ** -0.5)
        k, v = torch.randn(B, S, H, D, generator=g), torch.randn(B, S, H, D, generator=g)
        dout = torch.randn(B, T, H, D, generator=g)
        q[..., 0] = 1.0
        if causal:
            k[..., 0] = SelfAttnRef.RAMP * torch.arange(S, dtype=torch.float32)[None, :, None]
        else:
            k[..., 0] = 0.0
            k[:, GeneralAttnRef.edges(S), :, 0] = XAttnRef.BOOST
        dout[:, GeneralAttnRef.edges(T)] *= XAttnRef.FACTOR
        return tuple(t.reshape(B, t.shape[1], -1).to(dtype).to(device) for t in (q, k, v, dout))

    @staticmethod
    def causal_mask(B, T, left=0, holes=True):
        """key_valid [B,T] uint8 (host) for the causal cases.  Sample 0: the first `left` keys padded (rows 0 .. left - 1 have no allowed
        key) and, with `holes`, every key s > left with s % 7 == 5 and key T - 1 padded too: in the future of those rows, so doubly
        masked for them, ordinary holes for the rows below.  Sample 1: right-padded from T - T // 5 on.  Sample 2: all valid."""
        am = torch.ones(B, T, dtype=torch.uint8)
        s = torch.arange(T)
        am[0, :left] = 0
        if holes and T > left + 1:
            am[0, (s > left) & ((s % 7 == 5) | (s == T - 1))] = 0
        if B > 1 and T >= 5:
            am[1, T - T // 5:] = 0
        return am

    @staticmethod
    def keep(seed, B, H, T, S, p, device="cpu", dkey=0, drow=0, swap=False):
        """[B,H,T,S] bool from hash_keep at element index ((b H + h) T + t) S + s (+ dkey + drow S); swap: the index of a [B,H,S,T]
        layout, ((b H + h) S + s) T + t."""
        n = B * H * T * S
        kp = hash_keep(seed, n, p, start=dkey + drow * S)
        kp = torch.from_numpy(kp)
        kp = kp.view(B, H, S, T).transpose(2, 3) if swap else kp.view(B, H, T, S)
        return kp.contiguous().to(device)

    def __init__(self, q, k, v, key_valid, dout, num_heads, causal=False, head_mask=None, p_drop=0.0, seed=0, keep=None, keep_scale=None,
                 hm_of=None, hm_in_delta=True, uniform_keys=None, tie=0.5, tie_double=0.0, allowed=None, rows_kv=None):
        B, T, d = q.shape
        H, S = num_heads, k.shape[1]
        D = d // H
        assert k.shape == v.shape == (B, S, d) and dout.shape == q.shape and key_valid.shape == (B, S) and (not causal or S == T)
        dev = q.device
        valid = key_valid.to(dev).bool()
        ti, si = torch.arange(T, device=dev)[:, None], torch.arange(S, device=dev)[None, :]
        past = (si <= ti) if causal else torch.ones(T, S, dtype=torch.bool, device=dev)
        true_ok = valid[:, None, :] & past[None]                                  # [B,T,S]
        ok = true_ok if allowed is None else allowed.to(dev).bool()
        uni_rows = ~true_ok.any(2)                                                # [B,T]
        double = ~valid[:, None, :] & ~past[None]                                 # future and padded
        uk = torch.ones(B, S, dtype=torch.bool, device=dev) if uniform_keys is None else uniform_keys.to(dev).bool()
        hm = torch.ones(H, dtype=torch.float64, device=dev) if head_mask is None else head_mask.to(dev).float().double()
        hm_of = hm_of or (lambda h: h)
        if p_drop > 0:
            kp = (GeneralAttnRef.keep(seed, B, H, T, S, p_drop, dev) if keep is None else keep.to(dev)).double()
            kp = kp * (_keep_scale(p_drop) if keep_scale is None else keep_scale)
        else:
            kp = torch.ones(B, H, T, S, dtype=torch.float64, device=dev)
        rk = torch.ones(T, dtype=torch.float64, device=dev) if rows_kv is None else rows_kv.to(dev).double()
        q4, k4, v4, g4 = q.reshape(B, T, H, D), k.reshape(B, S, H, D), v.reshape(B, S, H, D), dout.reshape(B, T, H, D)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
        self.B, self.T, self.Tk, self.H, self.Hkv, self.D, self.P = B, T, S, H, H, D, 0
        self.dtype, self.uni_rows, self.valid, self.double, self.true_ok = q.dtype, uni_rows, valid, double, true_ok
        self.S = z(B, H, T)
        self.want = dict(out=z(B, T, H, D), lse=z(B, H, T), dq=z(B, T, H, D), dk=z(B, S, H, D), dv=z(B, S, H, D), probs=z(B, H, T, S))
        self.mag = {n: torch.zeros_like(self.want[n]) for n in ("out", "dq", "dk", "dv")}
        self.smag = {n: torch.zeros_like(self.want[n]) for n in ("out", "dq", "dk", "dv")}
        self.habs = {}
        self.hm = hm
        lnS = float(np.log(S))
        for b in range(B):
            A, U = ok[b], uni_rows[b]
            pu = (uk[b].double() / max(int(uk[b].sum()), 1))[None, :]
            f = torch.ones(T, S, dtype=torch.float64, device=dev)
            f[U] = tie
            f[U[:, None] & double[b]] = tie_double
            for h in range(H):
                Q, K, V, dO = q4[b, :, h].double(), k4[b, :, h].double(), v4[b, :, h].double(), g4[b, :, h].double()
                Si = (Q.abs() @ K.abs().t()).masked_fill_(~A, 0.0).amax(1).masked_fill_(U, 0.0) + lnS
                sc = (Q @ K.t()).masked_fill_(~A, float("-inf"))
                sc[U] = 0.0
                lse = torch.logsumexp(sc, 1)
                p = torch.where(U[:, None], pu.expand(T, S), sc.sub_(lse[:, None]).exp_())
                lse = lse.masked_fill(U, float("inf"))
                hmh, ks = hm[hm_of(h)], kp[b, h]
                W = hmh * p
                Wd = W * ks
                O = Wd @ V
                dWd = dO @ V.t()
                delta = (dWd * (Wd if hm_in_delta else p * ks)).sum(1)
                Delta = (dWd.abs() * Wd.abs()).sum(1)
                ds = f * p * (hmh * ks * dWd - delta[:, None])
                w = f * p * (hmh.abs() * ks * dWd.abs() + Delta[:, None])
                Sk = Si.max()
                self.S[b, h], self.want["lse"][b, h], self.want["probs"][b, h] = Si, lse, W
                for n, x, m in (("out", O, Wd.abs() @ V.abs()), ("dq", ds @ K, w @ K.abs())):
                    self.want[n][b, :, h], self.mag[n][b, :, h], self.smag[n][b, :, h] = x, m, Si[:, None] * m
                Wk, dsk, wk = Wd * rk[:, None], ds * rk[:, None], w * rk[:, None]
                for n, x, m in (("dk", dsk.t() @ Q, wk.t() @ Q.abs()), ("dv", Wk.t() @ dO, Wk.abs().t() @ dO.abs())):
                    self.want[n][b, :, h], self.mag[n][b, :, h], self.smag[n][b, :, h] = x, m, Sk * m

    def chain(self, name):
        """len of c(len): the links of the fp32 accumulation chain behind tensor `name` (class docstring)."""
        T, S, D = self.T, self.Tk, self.D
        return {"out": S + 4, "dv": T + 4, "dq": S + D + 6 + -(-S // 64) + 8, "dk": T + D + 6 + -(-S // 64) + 8}[name]

    def bound(self, name, dtype=None):
        """The bound of tensor `name`, shaped like want[name].  lse: +inf rows carry bound 0 (they are compared exactly)."""
        dtype = dtype or self.dtype
        n, u = (self.D + 8) * 2.0 ** -24, U[dtype]
        if name == "lse":
            return (n * self.S + 2.0 ** -20).masked_fill(self.uni_rows[:, None, :].expand_as(self.S), 0.0)
        if name == "probs":
            w = self.want["probs"].abs()
            b = (u + n * self.S[..., None]) * w + (w > 0) * self.hm.abs()[None, :, None, None] * 2.0 ** -126
            return b.masked_fill(self.uni_rows[:, None, :, None].expand_as(b), 0.0)
        return u * self.want[name].abs() + NormRef.c(self.chain(name)) * self.mag[name] + n * self.smag[name]

    def exact_probs(self, dtype=None):
        """What `probs` must hold bit for bit on the rows without an allowed key: dtype(fp32(fp32(1 / S)) hm) on all S keys."""
        uni = (torch.ones((), dtype=torch.float32) / torch.tensor(float(self.Tk), dtype=torch.float32)).to(self.hm.device)
        return (self.hm.float() * uni).to(dtype or self.dtype)                   # [H]

    def diff(self, other, name):
        """|other.want - self.want| with lse's +inf rows (equal on both sides) as 0."""
        a, b = other.want[name], self.want[name]
        return torch.where(torch.isinf(a) & torch.isinf(b), torch.zeros_like(a), (a - b).abs())

    def outside(self, other, name, dtype=None):
        return self.diff(other, name) > self.bound(name, dtype or self.dtype)

    def check(self, got, what, group="", dtype=None, rows=None, keys=None):
        """Asserts the bound on every element of got = dict(name -> tensor) (absent or None: skipped); prints the largest err / bound of
        each and returns them by name.  lse must be exactly +inf on the rows without an allowed key and probs exactly exact_probs()
        there.  `rows` [B,T] / `keys` [B,S] (bool) restrict the comparison of the row tensors / dk, dv to a subset, reported on its own."""
        dtype = dtype or self.dtype
        return check_bounds(self._items(got, what, dtype, rows, keys), what, group)

    def _items(self, got, what, dtype, rows, keys):
        """check()'s tensors, one by one, for bounds.check_bounds: the exactness assertions, then the elements the bound is for."""
        # how a [B,T] row selection (uni, rows) or a [B,S] key selection spreads over each tensor
        over = dict(out=lambda m: m[:, :, None, None], dq=lambda m: m[:, :, None, None], lse=lambda m: m[:, None, :],
                    probs=lambda m: m[:, None, :, None], dk=lambda m: m[:, :, None, None], dv=lambda m: m[:, :, None, None])
        uni = self.uni_rows
        for name in GeneralAttnRef.NAMES + ("probs",):
            x, part = got.get(name), keys if name in ("dk", "dv") else rows
            if x is None:
                continue
            want = self.want[name]
            x = x.detach().reshape(want.shape)
            sel = None if part is None else over[name](part).expand_as(want)
            empty = sel is not None and not bool(sel.any())
            if name in ("lse", "probs"):                 # the rows without an allowed key are compared exactly, the others against the bound
                at = over[name](uni).expand_as(want)
                if name == "lse":
                    assert bool((x[at] == float("inf")).all()), f"{what} lse: a row without an allowed key is not +inf"
                elif bool(uni.any()):
                    ex = self.exact_probs(dtype)[None, :, None, None].expand_as(x)
                    assert torch.equal(x[at], ex[at]), f"{what} probs: a row without an allowed key is not exactly fp32(1/S) hm"
                sel = ~at if sel is None else sel & ~at
            assert torch.isfinite(x[~at] if name == "lse" else x.float()).all(), f"{what} {name}: non-finite result"      # outside the selection too
            if empty or (part is None and (rows is not None or keys is not None)):
                continue
            yield name, x, want, self.bound(name, dtype), first_indices, sel


# ------------------------------------------------------------------------------------------ packed encoder attention (mmgl_encattn_fwd)
class EncAttnRef(XAttnRef):
    """fp64 reference of mmgl_encattn_fwd on the device the (storage-rounded) operands live on: q, k, v [ntok, H*D] (q already
    scaled), cu_seqlens [nseq + 1].  Per sequence an all-valid, non-causal attention with T = S = len; only `out` exists.  One
    (sequence, head) at a time: a sequence of 4097 tokens needs one 4097 x 4097 fp64 matrix (and its |.| twin) at once.

    The bound is XAttnRef's, with its u, its n = 8 + D / kb and c = 2^-7 (bf16) / 2^-16 (fp32) -- both routes (encattn_fwd_kernel of
    csrc/selfattn.hip, sa32_enc_fwd of csrc/selfattn32.hip) are the MFMA kernels those counts describe:
        |got - want| <= u |want| + (c + n 2^-24 (S_i + ln len)) mag,        mag_i = sum_j p_ij |v_j|.
    Keyword arguments build the deliberately wrong references of tests/test_attn_general_ref_cpu.py: `next_key` (the first key of the
    next sequence is visible too), `drop_last` (the last key of every sequence is not), `kv_head` (h -> head whose k, v head h reads)."""
    BOOST = 4.0

    @staticmethod
    def cu(lens, device="cpu"):
        return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=device)

    @staticmethod
    def inputs(dtype, lens, H, D, seed=0, device="cpu"):
        """q, k, v [ntok, H*D] in `dtype`: randn, q scaled by 2 D^-0.5, q[..., 0] = 1, k[s, 0] = BOOST on the first and the last key of
        every sequence and 0 elsewhere: a key leaking in from a neighbouring sequence, or the last key dropped, moves every row."""
        g = torch.Generator().manual_seed(seed)
        n = int(sum(lens))
        q = torch.randn(n, H, D, generator=g) * (2 * D ** -0.5)
        k, v = torch.randn(n, H, D, generator=g), torch.randn(n, H, D, generator=g)
        q[..., 0] = 1.0
        k[..., 0] = 0.0
        cu = np.concatenate([[0], np.cumsum(lens)])
        ends = sorted({int(x) for x in cu[:-1]} | {int(x) - 1 for x in cu[1:]})
        k[[e for e in ends if 0 <= e < n], :, 0] = EncAttnRef.BOOST
        return tuple(t.reshape(n, H * D).to(dtype).to(device) for t in (q, k, v))

    def __init__(self, q, k, v, cu_seqlens, num_heads, next_key=False, drop_last=False, kv_head=None):
        ntok, d = q.shape
        H = num_heads
        D = d // H
        dev = q.device
        cu = [int(x) for x in cu_seqlens.tolist()]
        assert cu[0] == 0 and cu[-1] <= ntok
        kv_head = kv_head or (lambda h: h)
        q3, k3, v3 = q.reshape(ntok, H, D), k.reshape(ntok, H, D), v.reshape(ntok, H, D)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
        self.H, self.D, self.cu_list, self.dtype = H, D, cu, q.dtype
        self.want, self.mag, self.smag, self.habs = dict(out=z(ntok, H, D)), dict(out=z(ntok, H, D)), dict(out=z(ntok, H, D)), {}
        for i in range(len(cu) - 1):
            a, e = cu[i], cu[i + 1]
            if e == a:
                continue
            ke = e - 1 if (drop_last and e - a > 1) else e
            ke = ke + 1 if (next_key and e < cu[-1]) else ke
            for h in range(H):
                hk = kv_head(h)
                Q, K, V = q3[a:e, h].double(), k3[a:ke, hk].double(), v3[a:ke, hk].double()
                Si = (Q.abs() @ K.abs().t()).amax(1) + float(np.log(e - a))
                p = torch.softmax(Q @ K.t(), 1)
                m = p @ V.abs()
                self.want["out"][a:e, h], self.mag["out"][a:e, h], self.smag["out"][a:e, h] = p @ V, m, Si[:, None] * m
                del p

    def rows(self, q_rows=None):
        """[ntok] bool: the rows mmgl_encattn_fwd writes with `q_rows` (the first q_rows of every sequence)."""
        cu = self.cu_list
        r = torch.zeros(self.want["out"].shape[0], dtype=torch.bool, device=self.want["out"].device)
        for i in range(len(cu) - 1):
            r[cu[i]:(cu[i + 1] if q_rows is None else min(cu[i + 1], cu[i] + q_rows))] = True
        return r

    def check(self, got, what, group="", q_rows=None):
        """Asserts the bound on every element of the rows that `q_rows` has written; prints and returns the largest err / bound."""
        return check_bound(got, self.want["out"], self.bound("out", self.dtype), f"{what} out", group, row_head, self.rows(q_rows)[:, None, None])
