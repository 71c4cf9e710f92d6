"""fp64 reference of T5's relative-position-bias attention (csrc/relbias.hip) with the kernels' arguments, and its per-element bounds."""
import numpy as np
import torch

from attn_ref import SelfAttnRef
from bounds import U, _keep_scale, check_bounds, first_indices, hash_keep, outside


class RelBiasRef:
    """q [B,T,H*D] (unscaled: T5 has no D^-0.5), k, v [B,S,H*D], key_valid [B,S] or None, dout [B,T,H*D], table [NB,H] or None,
    bucket_of int [T+S-1] (entry s - t + T - 1), causal (s <= t, T == S), dropout (p_drop, seed) on the probabilities with the
    kernels' counter hash of ((b H + h) T + t) S + s.  One (sample, head) at a time, on the (storage-rounded) operands.

        score = q . k + table[bucket_of[s - t + T - 1], h]        p = softmax over the allowed keys        pd = p keep / (1 - p_drop)
        out = pd V          dv = pd^T dO          dp = keep / (1 - p_drop) (dO V^T)          delta = sum_d dO O
        ds = p (dp - delta)          dq = ds K          dk = ds^T Q          dtable[n, h] = sum of ds over the allowed pairs of bucket n
    A row without an allowed key has p = 0 everywhere, lse = 0 and reaches no gradient (the kernels' documented deviation).

    Bounds, in SelfAttnRef's form and with its constants (attn_ref.py), every element checked:
        |got - want| <= u |want| + (c + n 2^-24 S_i) mag           |lse_got - lse_want| <= n 2^-24 S_i + 2^-20
    S_i = max over the allowed keys of sum_d |q||k| + |bias|; n = 9 + D / kb, one more than SelfAttnRef's for the bias add (the bias
    is the C-input of the first MFMA of the score: one more fp32 rounding in its accumulation chain); mag as there, with
    mag_dtable = sum of p (|dp| + Delta) over the bucket's pairs.  dtable is fp32 for both dtypes (u = 2^-23) and gets a further
    L 2^-24 mag for its chain of fp32 additions: L = 32 + 2 B ceil(T / 64) + (T + S - 1), counted from relbias.hip -- at most 16
    accumulator elements of a wave meet in one diagonal of its LDS row, 16 rows (4 lane groups x 4 waves) are folded per tile,
    rb_diag_kernel adds at most 2 tile rows per (sample, query block), rb_bucket_kernel at most T + S - 1 diagonals.
    `bias` [H,T,S] (fp64) and `allowed` [B,T,S] replace the table lookup and the mask: the deliberately wrong references."""
    NAMES = ("out", "lse", "dq", "dk", "dv", "dtable")

    @staticmethod
    def inputs(dtype, B, T, S, H, D, seed=0, device="cpu"):
        """q, k, v, dout in `dtype`: randn, q scaled by D^-0.5 so that q . k is O(1) next to an O(1) bias."""
        g = torch.Generator().manual_seed(seed)
        q = torch.randn(B, T, H * D, generator=g) * D ** -0.5
        k, v = torch.randn(B, S, H * D, generator=g), torch.randn(B, S, H * D, generator=g)
        dout = torch.randn(B, T, H * D, generator=g)
        return tuple(t.to(dtype).to(device) for t in (q, k, v, dout))

    @staticmethod
    def mask(B, S, layout):
        """key_valid [B,S] uint8.  M0: all valid.  M1: the last sample right-padded to about two thirds.  M2: a hole in the middle of
        sample 0.  Key 0 stays valid (a causal row 0 keeps a key)."""
        am = torch.ones(B, S, dtype=torch.uint8)
        if layout == "M1" and S > 1:
            am[B - 1, max(1, (2 * S) // 3):] = 0
        elif layout == "M2" and S > 2:
            am[0, max(1, S // 3):max(2, (2 * S) // 3)] = 0
        return am

    def __init__(self, q, k, v, key_valid, dout, num_heads, table=None, bucket_of=None, causal=False, p_drop=0.0, seed=0, bias=None,
                 allowed=None):
        B, T, d = q.shape
        S, H = k.shape[1], num_heads
        D = d // H
        dev = q.device
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
        self.B, self.T, self.Skeys, self.H, self.D = B, T, S, H, D
        if allowed is None:
            kv = torch.ones(B, S, dtype=torch.bool, device=dev) if key_valid is None else key_valid.bool().to(dev)
            allowed = kv[:, None, :].expand(B, T, S)
            if causal:
                assert T == S
                allowed = allowed & (torch.arange(S, device=dev)[None, :] <= torch.arange(T, device=dev)[:, None])[None]
        if bias is None and table is not None:
            idx = (torch.arange(S, device=dev)[None, :] - torch.arange(T, device=dev)[:, None] + T - 1)
            bias = table.double().to(dev)[bucket_of.long().to(dev)[idx]].permute(2, 0, 1)            # [H,T,S]
        self.bucket = None
        if table is not None:
            idx = (torch.arange(S, device=dev)[None, :] - torch.arange(T, device=dev)[:, None] + T - 1)
            self.bucket = bucket_of.long().to(dev)[idx]                                               # [T,S]
            NB = table.shape[0]
        q4, k4, v4, g4 = (t.reshape(B, t.shape[1], H, D) for t in (q, k, v, dout))
        self.S = z(B, H, T)
        self.want = dict(out=z(B, T, H, D), lse=z(B, H, T), dq=z(B, T, H, D), dk=z(B, S, H, D), dv=z(B, S, H, D))
        self.mag = {n: torch.zeros_like(self.want[n]) for n in ("out", "dq", "dk", "dv")}
        self.smag = {n: torch.zeros_like(self.want[n]) for n in ("out", "dq", "dk", "dv")}
        if table is not None:
            for d_ in (self.want, self.mag, self.smag):
                d_["dtable"] = z(NB, H)
        scale = _keep_scale(p_drop)
        for b in range(B):
            A = allowed[b]
            for h in range(H):
                Q, K, V, dO = q4[b, :, h].double(), k4[b, :, h].double(), v4[b, :, h].double(), g4[b, :, h].double()
                bh = bias[h] if bias is not None else z(T, S)
                Sx = (Q.abs() @ K.abs().t() + bh.abs()).masked_fill(~A, 0.0).amax(1)
                sc = (Q @ K.t() + bh).masked_fill(~A, float("-inf"))
                empty = ~A.any(1)
                lse = torch.logsumexp(sc.masked_fill(empty[:, None], 0.0), 1)
                p = (sc - lse[:, None]).exp().masked_fill(empty[:, None], 0.0)
                lse = lse.masked_fill(empty, 0.0)
                ks = torch.ones(T, S, dtype=torch.float64, device=dev)
                if p_drop > 0:
                    keep = hash_keep(seed, T * S, p_drop, start=(b * H + h) * T * S).reshape(T, S)
                    ks = torch.from_numpy(keep.astype(np.float64)).to(dev) * scale
                pd = p * ks
                O = pd @ V
                dp = (dO @ V.t()) * ks
                delta, Delta = (dO * O).sum(1), (dO.abs() * O.abs()).sum(1)
                w = p * (dp.abs() + Delta[:, None])
                ds = p * (dp - delta[:, None])
                Sk = torch.where(A, Sx[:, None], Sx.new_zeros(())).amax(0)[:, None]
                self.S[b, h], self.want["lse"][b, h] = Sx, lse
                for n, x, m in (("out", O, pd @ V.abs()), ("dq", ds @ K, w @ K.abs())):
                    self.want[n][b, :, h], self.mag[n][b, :, h], self.smag[n][b, :, h] = x, m, Sx[:, None] * m
                for n, x, m in (("dk", ds.t() @ Q, w.t() @ Q.abs()), ("dv", pd.t() @ dO, pd.t() @ dO.abs())):
                    self.want[n][b, :, h], self.mag[n][b, :, h], self.smag[n][b, :, h] = x, m, Sk * m
                if table is not None:
                    flat = self.bucket.reshape(-1)
                    self.want["dtable"][:, h].index_add_(0, flat, ds.reshape(-1))
                    self.mag["dtable"][:, h].index_add_(0, flat, w.reshape(-1))
                    self.smag["dtable"][:, h].index_add_(0, flat, (Sx[:, None] * w).reshape(-1))

    def chain(self):
        """L: the longest chain of fp32 additions behind a dtable element (class docstring)."""
        return 32 + 2 * self.B * ((self.T + 63) // 64) + (self.T + self.Skeys - 1)

    def bound(self, name, dtype):
        n = (9 + self.D // (16 if dtype == torch.bfloat16 else 4)) * 2.0 ** -24
        if name == "lse":
            return n * self.S + 2.0 ** -20
        if name == "dtable":
            return (2.0 ** -23 * self.want[name].abs() + (SelfAttnRef.C[dtype] + self.chain() * 2.0 ** -24) * self.mag[name]
                    + n * self.smag[name])
        return U[dtype] * self.want[name].abs() + SelfAttnRef.C[dtype] * self.mag[name] + n * self.smag[name]

    def outside(self, other, name, dtype):
        """The elements at which `other`, a deliberately wrong reference of the same call, leaves this one's bound."""
        return outside(self.want[name], other.want[name], self.bound(name, dtype))

    def check(self, got, what, dtype):
        """Asserts the bound on every element of got = dict(name -> tensor); prints the largest err / bound of each, returns them."""
        return check_bounds(((name, x.cpu(), self.want[name].cpu(), self.bound(name, dtype).cpu(), first_indices, None) for name, x in got.items()),
                            what, "relbias")
