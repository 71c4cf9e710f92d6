"""Fixture loading + comparison helpers shared by the test modules."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_FIXTURE_BYTES = 1 << 20    # every committed file stays below 1 MiB: a larger fixture is <stem>.npz + <stem>.part1.npz + ...


def load_golden(name):
    """The arrays of the fixture tests/golden/<name> (<stem>.npz) and of its continuation files <stem>.part1.npz, .part2.npz, ..."""
    out, k, path = {}, 0, os.path.join(GOLDEN, name)
    while os.path.exists(path):
        with np.load(path, allow_pickle=False) as z:
            out.update((n, z[n]) for n in z.files)
        k += 1
        path = os.path.join(GOLDEN, f"{name[:-4]}.part{k}.npz")
    if not out:
        raise FileNotFoundError(os.path.join(GOLDEN, name))
    return out


def save_golden(path, flat):
    """np.savez_compressed of `flat` as <stem>.npz plus as many continuation files as keep every file below MAX_FIXTURE_BYTES
    (consecutive runs of keys, in order); returns the paths written"""
    import glob
    stem = path[:-4]
    for n in range(1, len(flat) + 1):
        for old in glob.glob(stem + ".part*.npz"):
            os.remove(old)
        keys = list(flat)
        chunks = [keys[i * len(keys) // n:(i + 1) * len(keys) // n] for i in range(n)]
        paths = [path] + [f"{stem}.part{k}.npz" for k in range(1, n)]
        for p, ks in zip(paths, chunks):
            np.savez_compressed(p, **{key: flat[key] for key in ks})
        if all(os.path.getsize(p) < MAX_FIXTURE_BYTES for p in paths):
            return paths
    raise ValueError(f"{path}: a single array is larger than {MAX_FIXTURE_BYTES} bytes compressed")


class Fixture:
    def __init__(self, name):
        z = load_golden(name)
        self.meta = json.loads(str(z["meta"]))
        self.groups = {}
        for k in z:
            if k == "meta":
                continue
            g, n = k.split("/", 1)
            self.groups.setdefault(g, {})[n] = torch.from_numpy(np.array(z[k]))

    def __getattr__(self, g):
        try:
            return self.__dict__["groups"][g]
        except KeyError:
            raise AttributeError(g)

    @property
    def inp(self):
        return self.groups["in"]


def rel_err(a: torch.Tensor, b: torch.Tensor, floor: float = 1e-6) -> float:
    """max|a-b| / max(max|b|, floor) -- the 'relative fp32' measure BASELINE.json's 1e-3 tolerance is stated in.
    The floor keeps analytically-zero tensors (e.g. d k_proj.bias: softmax is invariant to a per-row score shift)
    from turning 1e-10 round-off into a relative error."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), floor)


def elementwise_err(a: torch.Tensor, b: torch.Tensor, floor_frac: float = 1e-3, abs_floor: float = 1e-6) -> float:
    """max over elements of |a - b| / (|b| + floor_frac * max|b|): an element-wise relative error (rel_err above is a max-norm measure:
    a small element of a tensor with a large maximum can be wrong by many times its own size and pass).  The floor -- a fraction of the
    tensor's largest magnitude -- keeps elements that are analytically ~0 from dividing round-off by nothing."""
    a = a.detach().double()
    b = b.detach().double().to(a.device)      # on the device `a` lives on: a [40960, 8192] gradient is checked where it was computed
    floor = max(floor_frac * b.abs().max().item(), abs_floor)      # abs_floor: analytically-zero tensors (d k_proj.bias) are round-off on both sides
    return ((a - b).abs() / (b.abs() + floor)).max().item()


def slice_err(a: torch.Tensor, b: torch.Tensor, keep, floor_frac: float = 1e-3) -> torch.Tensor:
    """Per-slice max-norm relative error: for every index along the dims in `keep` (e.g. (0, 2) of a [B, T, H, D] tensor: one
    (sample, head) slice), max|a - b| / max|b| over the slice's other elements.  Returns the errors indexed by the `keep` dims.
    A whole-tensor maximum hides a defect confined to one chunk, trip, head or split; this measure does not.  The floor -- a fraction
    of the WHOLE tensor's largest magnitude -- keeps an analytically-zero slice (dQ of a sample with one valid key) from dividing
    round-off by nothing."""
    a = a.detach().double()
    b = b.detach().double().to(a.device)
    red = [i for i in range(b.dim()) if i not in keep]
    d = (a - b).abs().amax(dim=red)
    m = b.abs().amax(dim=red)
    return (d / m.clamp_min(max(floor_frac * float(m.max()), 1e-30))).cpu()


def tile_err(a: torch.Tensor, b: torch.Tensor, tile: int = 256, floor_frac: float = 1e-3) -> float:
    """Largest slice_err over the tile x tile blocks of a 2-D tensor (ragged edge blocks included): a weight gradient whose one
    output tile or one K split is off shows here even when the tensor's maximum lies in another tile."""
    R, C = b.shape
    pr, pc = (-R) % tile, (-C) % tile
    pad = lambda t: torch.nn.functional.pad(t.detach().double(), (0, pc, 0, pr))
    a, b = pad(a), pad(b.to(a.device))
    return float(slice_err(a.view(-1, tile, a.shape[1] // tile, tile), b.view(-1, tile, b.shape[1] // tile, tile), (0, 2), floor_frac).max())


def assert_close(a, b, tol, what="", floor=1e-6):
    e = rel_err(a, b, floor)
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"
    return e


# ------------------------------------------------------------------------------------------ decode kernels (csrc/decode.hip)
class SkinnyRef:
    """fp64 reference of mmgl_gemm_skinny / mmgl_gemm_skinny_lora on the device the (storage-rounded) operands live on:
        want = act((x W^T + bias + s (x A^T) B^T) * scale) + residual
        mag  = (|x| |W|^T + |bias| + |s| (|x| |A|^T) |B|^T) * |scale| + |residual|
    and two deliberately wrong references of the same call, for the assertion that a comparison can fail: `drop_k` (the last 64 K
    columns of x left out of both products) and, with an adapter, `no_lora` (the rank-r term left out).

    Per-element bound (every element is checked):  |got - want| <= u |want| + 2^-16 mag,  u = 2^-8 (bf16) or 2^-23 (fp32).
      * u |want| is the half ulp of the one round-to-nearest store of the fp32 result; rounding alone reaches it, so it has no margin.
      * 2^-16 mag is 256 fp32 roundings of 2^-24 on the magnitude sum: the longest summation chain of either kernel at K = 8192 is
        below 100 on the MFMA kernel (64 MFMA steps, the in-MFMA tree, the 8-slot fold) and 128 + 6 on the plain one; it also covers
        a rounding decision, or a ReLU whose pre-activation lies within 2^-16 mag of zero, that the summation order flips.
    The bound is a function of the reference alone, never of the kernel's output."""

    def __init__(self, x, w, bias=None, relu=False, scale=1.0, residual=None, A=None, B=None, s=1.0):
        d = lambda t: t.detach().double()
        X, W = d(x), d(w)
        K = X.shape[1]
        tail = slice(max(K - 64, 0), K)
        pre = X @ W.t()
        mag = X.abs() @ W.abs().t()
        gone = X[:, tail] @ W[:, tail].t()
        lora = None
        if A is not None:
            Ad, Bd = d(A), d(B)
            lora = s * ((X @ Ad.t()) @ Bd.t())
            pre = pre + lora
            mag = mag + abs(s) * ((X.abs() @ Ad.abs().t()) @ Bd.abs().t())
            gone = gone + s * ((X[:, tail] @ Ad[:, tail].t()) @ Bd.t())
        if bias is not None:
            mag = mag + d(bias).abs()
        mag = mag * abs(scale)
        if residual is not None:
            mag = mag + d(residual).abs()

        def epilogue(y):
            if bias is not None:
                y = y + d(bias)
            y = y * scale
            if relu:
                y = torch.relu(y)
            return y if residual is None else y + d(residual)

        self.want, self.mag = epilogue(pre), mag
        self.drop_k = epilogue(pre - gone)
        self.no_lora = None if lora is None else epilogue(pre - lora)

    def bound(self, dtype):
        return 2.0 ** (-8 if dtype == torch.bfloat16 else -23) * self.want.abs() + 2.0 ** -16 * self.mag

    @staticmethod
    def assert_can_fail(refs, dtype, what):
        """From the references alone: a kernel that drops one 64-wide K unit (or the rank-r term) leaves the bound on >= 25 % of the
        elements (of the pooled `refs`: the calls of one test, where a single call has too few elements to count on)."""
        for name, pick in (("the last 64 K columns", lambda r: r.drop_k), ("the rank-r term", lambda r: r.no_lora)):
            if pick(refs[0]) is not None:
                out = sum(((pick(r) - r.want).abs() > r.bound(dtype)).sum().item() for r in refs)
                frac = out / sum(r.want.numel() for r in refs)
                assert frac >= 0.25, f"{what}: dropping {name} moves only {frac:.0%} of the elements out of the bound"

    def check(self, got, what, group="", can_fail=True):
        """Asserts the bound on every element of `got` (first, unless can_fail is off, that the comparison can fail); prints and
        returns the largest err / bound."""
        if can_fail:
            SkinnyRef.assert_can_fail([self], got.dtype, what)
        assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
        err, bound = (got.detach().double() - self.want).abs(), self.bound(got.dtype)
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        print(f"[bound {group}] {what}: max err/bound {ratio:.3f}")
        bad = (err > bound).nonzero()
        assert bad.numel() == 0, (f"{what}: {bad.shape[0]} of {err.numel()} elements outside the bound (max err/bound {ratio:.2f}); "
                                  f"rows {bad[:, 0].unique().tolist()[:16]}, columns {bad[:, 1].unique().tolist()[:16]}")
        return ratio


def attn_decode_ref(q, k, v, valid, num_heads):
    """fp64 reference of mmgl_attn_decode_fwd from the storage-rounded operands: q [B, d] (already scaled), k, v [B, S, d],
    valid [B, S]; softmax over the valid keys of each (sample, head), uniform over all S keys where none is valid.  Returns [B, d]."""
    B, S, d = k.shape
    D = d // num_heads
    sc = torch.einsum("bhd,bshd->bhs", q.double().reshape(B, num_heads, D), k.double().reshape(B, S, num_heads, D))
    ok = valid.bool()
    sc = sc.masked_fill(~ok[:, None, :], float("-inf"))
    sc[~ok.any(1)] = 0.0
    return torch.einsum("bhs,bshd->bhd", torch.softmax(sc, -1), v.double().reshape(B, S, num_heads, D)).reshape(B, d)


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
    U = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -23}
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
        b = SelfAttnRef.U[dtype] * self.want[name].abs() + SelfAttnRef.C[dtype] * self.mag[name] + n * self.smag[name]
        if name in self.habs and self.Hkv < self.H:
            b = b + SelfAttnRef.U[dtype] * self.habs[name]
        return b

    def outside(self, other, name, dtype):
        """From two references alone: the elements (bool, shaped like want[name]) at which `other` -- a deliberately wrong reference
        of the same call -- leaves this one's bound."""
        return (other.want[name] - self.want[name]).abs() > self.bound(name, dtype)

    def check(self, got, what, group="", dtype=None):
        """Asserts the bound on every element of got = (out, lse, dq, dk, dv) (any may be None: skipped); prints the largest
        err / bound of each and returns them by name."""
        dtype = dtype or got[0].dtype
        ratios, failed = {}, []
        for name, x in zip(SelfAttnRef.NAMES, got):
            if x is None:
                continue
            want = self.want[name]
            assert torch.isfinite(x.float()).all(), f"{what} {name}: non-finite result"
            err, bound = (x.detach().double().reshape(want.shape) - want).abs(), self.bound(name, dtype)
            ratios[name] = (err / bound.clamp_min(1e-300)).max().item()
            print(f"[bound {group}] {what} {name}: max err/bound {ratios[name]:.3f}")
            bad = (err > bound).nonzero()
            if bad.numel():
                # (sample, head, row): lse is [B,H,T], the others [B,rows,heads,D]
                at = bad[:, :3] if name == "lse" else bad[:, [0, 2, 1]]
                failed.append(f"{what} {name}: {bad.shape[0]} of {err.numel()} elements outside the bound (max err/bound "
                              f"{ratios[name]:.2f}); (sample, head, row) {at.unique(dim=0).tolist()[:12]}")
        assert not failed, "\n".join(failed)
        return ratios


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
        return SelfAttnRef.U[dtype] * self.want[name].abs() + SelfAttnRef.C[dtype] * self.mag[name] + n * self.smag[name]


# ------------------------------------------------------------------------------------------ single-query attention (csrc/decode.hip)
DECODE_KERNELS = ("plain", "gqa", "beam", "block", "gqa_block", "q8", "gqa_q8", "relbias")


def _cdiv(a, b):
    return -(-a // b)


def decode_geometry(kernel, dtype, D):
    """(VEC, LPK, KPI, I) of a decode.hip kernel: elements per lane and 16-byte load (8 bf16, 4 fp32; Q8_VEC = 16 codes for the q8
    kernels), lanes per key D / VEC, keys per wave and load instruction 64 / LPK, keys per workgroup loop trip 16 KPI."""
    assert kernel in DECODE_KERNELS, kernel
    vec = 16 if kernel in ("q8", "gqa_q8") else (8 if dtype == torch.bfloat16 else 4)
    lpk = D // vec
    return vec, lpk, 64 // lpk, 16 * (64 // lpk)


def decode_rows_cache(k, v, valid):
    """plain, GQA and relbias kernels: row b reads the S cache rows of sample b.  -> (k, v [B,S,kd], allowed [B,S], uniform [B,S])."""
    ok = valid.bool()
    return k, v, ok, torch.ones_like(ok)


def decode_rows_beam(k_pre, v_pre, valid, W, k_tail=None, v_tail=None, src=None, uniform_tail=True):
    """Beam kernel: row (b, w) reads pre[b] ++ tail[b*W + src[b*W + w, j], j].  A sample whose prefix has no valid key allows nothing
    and is uniform over all S_pre + n_tail keys (uniform_tail=False: over the prefix alone, a wrong reference)."""
    B, S = k_pre.shape[:2]
    R = B * W
    k, v, ok = (t.repeat_interleave(W, 0) for t in (k_pre, v_pre, valid.bool()))
    n = 0 if k_tail is None else k_tail.shape[1]
    uni = torch.ones(R, S + n, dtype=torch.bool, device=k.device)
    if n:
        rows = (torch.arange(R, device=k.device) // W * W)[:, None] + src[:, :n].long()
        cols = torch.arange(n, device=k.device)[None, :].expand(R, -1)
        k, v = torch.cat([k, k_tail[rows, cols]], 1), torch.cat([v, v_tail[rows, cols]], 1)
        ok = torch.cat([ok, ok.any(1, keepdim=True).expand(R, n)], 1)
        uni[:, S:] = uniform_tail
    return k, v, ok, uni


def decode_rows_block(k, v, valid, lens, k_new, v_new, m, strict=False, below_capacity=False):
    """Block kernels: row (b, i) reads the valid cache columns s < lens[b], then the new keys j <= i of its sample (strict: j < i, a
    wrong reference).  k, v [B,cap,kd]; k_new, v_new [B*m,kd].  below_capacity (the GQA block kernel, whose new keys are cache
    columns): new key j exists only where lens[b] + j < cap.  -> N = cap + m keys per row."""
    B, cap, kd = k.shape
    dev = k.device
    L = lens.to(dev).long().clamp(0, cap)
    s = torch.arange(cap, device=dev)
    i = torch.arange(m, device=dev)
    old = ((s[None, :] < L[:, None]) & valid.bool()).repeat_interleave(m, 0)                          # [B*m, cap]
    new = (i[None, :] < i[:, None]) if strict else (i[None, :] <= i[:, None])                         # [i, j]
    new = new[None].expand(B, m, m).clone()
    if below_capacity:
        new &= ((L[:, None] + i[None, :]) < cap)[:, None, :]
    kk = torch.cat([k.repeat_interleave(m, 0), k_new.reshape(B, m, kd).repeat_interleave(m, 0)], 1)
    vv = torch.cat([v.repeat_interleave(m, 0), v_new.reshape(B, m, kd).repeat_interleave(m, 0)], 1)
    ok = torch.cat([old, new.reshape(B * m, m)], 1)
    return kk, vv, ok, torch.ones_like(ok)


def decode_rows_q8(codes, e, valid, k_new, v_new, num_kv_heads):
    """q8 kernels: row b reads the S columns dequantised as tests/kvq_ref.py states the format, then its unquantised new row (always
    valid).  codes uint8 [B,S,2kd], e int8 [B,S,2Hkv] (CPU); -> fp32 k, v [B,S+1,kd] on k_new's device."""
    import kvq_ref
    kc, vc = kvq_ref.dequantize_row(codes, e, num_kv_heads)
    dev = k_new.device
    k = torch.cat([kc.to(dev), k_new.float()[:, None]], 1)
    v = torch.cat([vc.to(dev), v_new.float()[:, None]], 1)
    ok = torch.cat([valid.bool().to(dev), torch.ones(k.shape[0], 1, dtype=torch.bool, device=dev)], 1)
    return k, v, ok, torch.ones_like(ok)


def decode_bias_relbias(bias, S, wrong=None):
    """relbias kernel: key s gets bias[h, S - 1 - s].  -> fp32 [H,S].  wrong: "distance s" | "head h^1" | "no bias"."""
    rows = bias[:, :S].float()
    H = rows.shape[0]
    if wrong == "distance s":
        return rows.clone()
    if wrong == "head h^1":
        return rows[[h ^ 1 if (h ^ 1) < H else h for h in range(H)]].flip(1)
    if wrong == "no bias":
        return torch.zeros_like(rows)
    assert wrong is None, wrong
    return rows.flip(1)


class DecodeAttnRef:
    """fp64 reference of the eight single-query attention entry points of csrc/decode.hip on the device the (storage-rounded)
    operands live on.  Every one of them is softmax attention of one query row over a per-row key list, so the reference takes the
    list EXPANDED (the decode_rows_* builders above gather it): q [R, H*D] (already scaled; raw for the relbias kernel),
    k, v [R, N, Hkv*D], allowed [R, N], an optional fp32 bias [H, N] added to the score, kv_head (h -> key/value head, default
    h // G) and uniform [R, N]: the key set a row WITHOUT an allowed key weighs equally (include/mmgl_hip.h: all S keys for the plain
    and GQA kernels, all S_pre + n_tail keys for the beam kernel; default every key of the list).

    Per (row, head):  want = sum_j p_j v_j,  mag = sum_j p_j |v_j|,  S_i = max over the allowed j of sum_d |q_d| |k_jd| (+ |bias_j|)
    (0 for a row without an allowed key: no score reaches its result).

    Per-element bound (every element is checked), a function of the reference alone, never of the kernel's output:
        |got - want| <= u |want| + (n_s S_i + n_c) 2^-24 mag            u = 2^-8 (bf16), 2^-23 (fp32)
    u |want| is the one round-to-nearest store (SelfAttnRef.U).  The rest is fp32 VALU arithmetic, counted to first order from the
    statements of the kernels in units of one rounding, 2^-24 (the second-order terms are below 2^-12 of the bound at the largest
    count in use).  The computed weight of key j is e^(s_j - M) (1 + eps_j) with M the row's final maximum; a relative error eps of the
    weights moves the result by at most 2 eps mag -- eps mag through the numerator and eps |want| <= eps mag through the normaliser,
    which a common factor does not cancel when the keys err in opposite directions -- so every rounding that reaches a WEIGHT counts
    twice, and a rounding of an accumulator (acc or l) once.

    n_s = 2 (VEC + log2 LPK + 5 [+ 1 relbias]): the roundings of a score that reach p through the exponent, relative to S_i.
      * VEC: the lane's chain dot += q_e k_e; a term passes at most VEC roundings (its product and the sums after it; an fma only
        removes some).  log2 LPK: the xor butterfly (group_sum) over the lanes of the key.  [+ 1: dot + bias, relative to
        |dot + bias| <= S_i, which is why S_i takes |bias_j| in.]  The q8 kernels' 2^e on the dot is exact.
      * 2: the subtraction of the maximum.  |sc - mn| <= 2 S_i, and along the path of a key to the result -- p = e^(sc - mn), then one
        corr = e^(m - mn) per later step of its chain, c1 / c2 per lane-group merge, ci per wave -- the maxima only grow, so the
        magnitudes of ALL these differences telescope to M - s_j <= 2 S_i: two units for the whole path, not two per step.
      * 2 + 1: __expf(x) = exp2(x log2e): the rounded product, relative to the same |x| (telescoping likewise), and the fp32 constant
        log2e itself, 0.22 * 2^-24 off, times 2 S_i: under one unit.
    n_c = sum over the phases of trips (2 U + 6)  +  8 log2 KPI  +  13: the roundings on the weights and accumulators that do not scale
    with the score, along the longest chain a lane group runs.
      * a trip that folds U keys into a state (U = 1: one key of the plain, relbias kernels, a new key of the block and q8 kernels;
        U = AD_UNROLL = 4: the cache / prefix loop of the NQ and q8 kernels; U = TAIL_UNROLL = 2: the beam tail):
        corr and p are v_exp_f32 results, 1 ulp = 2 units each, on disjoint keys (the old state, the trip's keys) and on weights: 4;
        acc: acc * corr, then U sums of p_u v_u: at most 1 + U on the old state, fewer on a new term; l: ps (U - 1), l corr, + ps:
        U + 1.  Together 2 U + 6, i.e. 8 / 14 / 10 for U = 1 / 4 / 2.
        trips: plain, relbias ceil(S / (4 KPI)) at U = 1;  gqa, q8, gqa_q8, beam prefix, block caches ceil(S / (16 KPI)) at U = 4;
        beam tail ceil(n_tail / (8 KPI)) at U = 2;  block, gqa_block new keys and the q8 new row: one trip at U = 1.
      * a lane-group merge (log2 KPI of them): c1, c2 (2 units on a weight: 4), acc c1 + acc' c2 (2), l likewise (2): 8.
      * the waves: ci (4), o += sm_o ci over 4 waves (product and up to 3 sums: 4), ll likewise (4), the division (1): 13.
    The q8 kernels' power-of-two scales (2^e on the dot and on p) are exact, so ONE formula parameterised by the kernel's geometry
    (decode_geometry) serves all eight; the block and q8 kernels add their one extra trip and nothing else.  A p below 2^-126 flushes
    to zero: at most N 2^-126 max|v| against mag, nothing for finite operands.  The constants are derived, not fitted; they grow only
    by a rounding that is found in the kernel and named here.

    inputs() / keys() build edge-weighted operands: q[..., 0] = 1 in every head of every row and k[s, 0] = BOOST on the edge keys, 0
    elsewhere, so an edge key is lifted along EVERY reader's query and carries a few percent of each row at any N."""
    U = SelfAttnRef.U
    BOOST, SPREAD = 4.0, 40.0

    @staticmethod
    def counts(kernel, dtype, D, S, n_tail=0):
        """(n_s, n_c) for a call of `kernel` whose longest cache / prefix phase has S keys (block kernels: the largest lens)."""
        vec, lpk, kpi, I = decode_geometry(kernel, dtype, D)
        lg = lambda x: int(x).bit_length() - 1
        n_s = 2 * (vec + lg(lpk) + 5 + (kernel == "relbias"))
        if kernel in ("plain", "relbias"):
            chain = 8 * _cdiv(S, 4 * kpi)
        else:
            chain = 14 * _cdiv(S, I)
        if kernel == "beam":
            chain += 10 * _cdiv(n_tail, 8 * kpi)
        if kernel in ("block", "gqa_block", "q8", "gqa_q8"):
            chain += 8
        return n_s, chain + 8 * lg(kpi) + 13

    @staticmethod
    def edges(kernel, dtype, D, n, extra=()):
        """The edge positions of a phase of n keys: {0, KPI-1, KPI, 4KPI-1, 4KPI, I-1, I, n-1} and `extra`, where they exist."""
        _, _, kpi, I = decode_geometry(kernel, dtype, D)
        return sorted({e for e in (0, kpi - 1, kpi, 4 * kpi - 1, 4 * kpi, I - 1, I, n - 1) + tuple(extra) if 0 <= e < n})

    @staticmethod
    def inputs(dtype, R, H, D, seed=0):
        """q [R, H*D] in `dtype`: randn D^-0.5 with q[..., 0] = 1 in every head."""
        g = torch.Generator().manual_seed(seed)
        q = torch.randn(R, H, D, generator=g) * D ** -0.5
        q[..., 0] = 1.0
        return q.reshape(R, H * D).to(dtype)

    @staticmethod
    def keys(dtype, lead, n, Hkv, D, edges=(), seed=0, order=None):
        """k, v [*lead, n, Hkv*D] in `dtype`: randn, with k[..., s, :, 0] = BOOST on the edge keys and 0 elsewhere.  order "asc" /
        "desc": k[..., s, :, 0] = SPREAD s / (n - 1) rising / falling instead -- the running maximum moves at every key / never."""
        g = torch.Generator().manual_seed(seed + 7919)
        k, v = torch.randn(*lead, n, Hkv, D, generator=g), torch.randn(*lead, n, Hkv, D, generator=g)
        k[..., 0] = 0.0
        if order is None:
            k[..., list(edges), :, 0] = DecodeAttnRef.BOOST
        else:
            ramp = DecodeAttnRef.SPREAD * torch.arange(n, dtype=torch.float32) / max(n - 1, 1)
            k[..., 0] = (ramp if order == "asc" else ramp.flip(0))[:, None]
        return tuple(t.reshape(*lead, n, Hkv * D).to(dtype) for t in (k, v))

    def __init__(self, q, k, v, allowed, num_heads, num_kv_heads=None, bias=None, kv_head=None, uniform=None, counts=(0, 0)):
        R, d = q.shape
        H, Hkv = num_heads, num_kv_heads or num_heads
        D, G, N = d // H, H // Hkv, k.shape[1]
        assert k.shape == v.shape == (R, N, Hkv * D) and allowed.shape == (R, N), (q.shape, k.shape, v.shape, allowed.shape)
        dev = q.device
        kv_head = kv_head or (lambda h: h // G)
        ok = allowed.to(dev).bool()
        uni = torch.ones_like(ok) if uniform is None else uniform.to(dev).bool()
        live = ok.any(1)
        q3, k4, v4 = q.double().reshape(R, H, D), k.reshape(R, N, Hkv, D), v.reshape(R, N, Hkv, D)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
        self.R, self.H, self.Hkv, self.D, self.N = R, H, Hkv, D, N
        self.n_s, self.n_c = counts
        self.allowed = ok
        self.want, self.mag, self.S = z(R, H, D), z(R, H, D), z(R, H)
        fill = torch.where(uni, 0.0, float("-inf")).double()
        for h in range(H):
            K, V = k4[:, :, kv_head(h)].double(), v4[:, :, kv_head(h)].double()
            sc = torch.einsum("rd,rnd->rn", q3[:, h], K)
            sa = torch.einsum("rd,rnd->rn", q3[:, h].abs(), K.abs())
            if bias is not None:
                sc = sc + bias[h].to(dev).double()[None]
                sa = sa + bias[h].to(dev).double().abs()[None]
            self.S[:, h] = sa.masked_fill(~ok, 0.0).amax(1)
            sc = torch.where(live[:, None], sc.masked_fill(~ok, float("-inf")), fill)
            p = torch.softmax(sc, 1)
            self.want[:, h] = torch.einsum("rn,rnd->rd", p, V)
            self.mag[:, h] = torch.einsum("rn,rnd->rd", p, V.abs())

    def bound(self, dtype):
        """[R,H,D]."""
        return DecodeAttnRef.U[dtype] * self.want.abs() + ((self.n_s * self.S + self.n_c) * 2.0 ** -24)[..., None] * self.mag

    def outside(self, other, dtype):
        """From two references alone: the elements [R,H,D] at which `other` -- a deliberately wrong reference of the same call --
        leaves this one's bound."""
        return (other.want - self.want).abs() > self.bound(dtype)

    def affected(self, other):
        """[R] bool: the rows `other` does not reproduce bit for bit (a wrong reference that cannot reach a row leaves it as it is)."""
        return (other.want != self.want).flatten(1).any(1)

    def check(self, got, what, group="", dtype=None, rows=None):
        """Asserts the bound on every element of got [R, H*D] (rows [R] bool: those rows alone); prints and returns the largest
        err / bound and names (row, head) on failure."""
        dtype = dtype or got.dtype
        keep = torch.ones(self.R, dtype=torch.bool, device=self.want.device) if rows is None else rows.to(self.want.device).bool()
        x = got.detach().double().reshape(self.want.shape)
        assert torch.isfinite(x[keep]).all(), f"{what}: non-finite result"
        err, bound = (x - self.want).abs(), self.bound(dtype)
        ratio = torch.where(keep[:, None, None], err / bound.clamp_min(1e-300), torch.zeros_like(err))
        worst = ratio.max().item() if ratio.numel() else 0.0
        print(f"[bound {group}] {what}: max err/bound {worst:.3f}")
        bad = (ratio > 1.0).nonzero()
        assert not bad.numel(), (f"{what}: {bad.shape[0]} of {int(keep.sum()) * self.H * self.D} elements outside the bound (max err/bound "
                                 f"{worst:.2f}); (row, head) {bad[:, :2].unique(dim=0).tolist()[:12]}")
        return worst


# ------------------------------------------------------------------------------------------ the GEMM family (csrc/gemm*.hip)
class GemmRef:
    """fp64 reference of one product of the GEMM family on the device the (storage-rounded) operands live on (or the CPU):
        forward   want = act((x[:, :K] W[:, :K]^T + bias) * scale), zeroed where zmask <= 0, + residual
                  mag  = (|x| |W|^T + |bias|) * |scale| + |residual|
        dgrad     want = dyp W, zeroed where x_mask <= 0 (mask_dx)          mag = |dyp| |W|
        wgrad     want = dyp^T x + prior (accumulate)                       mag = |dyp|^T |x| + |prior|
        dbias     want = column sums of dyp + prior                         mag = column sums of |dyp| + |prior|
    with dyp = dy * scale * (y > 0) (y: the operand the call is given; None: no activation) in all three.

    Per-element bound (every element is checked; none is weighted out near a ReLU kink: a pre-activation within c mag of zero moves
    the output by at most c mag), a function of the reference alone, never of the kernel's output:
        |got - want| <= u |want| + L c mag + E + staged                     u = 2^-8 (bf16) or 2^-23 (fp32)
      * u |want| is the half ulp of the one round-to-nearest store of the fp32 result; rounding alone reaches it.
      * c = max(2^-16, 2 n 2^-24): n fp32 roundings of 2^-24 on the magnitude sum, with a factor 2 of room.  n is the longest chain
        of the case (GemmRef.chain): contraction length / kb -- the accumulator is rounded once per MFMA k-block; kb = 16 for the bf16
        MFMAs (16x16x32 counts as two, 32x32x16 as one), kb = 4 for mfma_f32_16x16x4f32 -- plus the number of partial tiles or
        partial sums that are folded (K splits of the persistent kernels, row splits of the bias gradient and its 16-slot LDS fold)
        plus 8 for the epilogue: bias add, scale, the activation's own arithmetic (E below counts its evaluation), residual add, the
        accumulate add, the fold's scale.  2^-16 is SkinnyRef's floor: it also covers a rounding decision the summation order flips.
      * L is the activation's Lipschitz constant, through which the pre-activation error passes: 1 for none / ReLU, 1.13 for erf-GELU
        (max of Phi(x) + x phi(x), 1.1290 at x = sqrt 2), 1.10 for quick-GELU x sigmoid(1.702 x) (1.0998, whatever the slope), 1.13
        for tanh-GELU (1.1291).
      * E = 2^-20 (|pre| + |act(pre)|) is the evaluation error of the device function for the three GELUs, 0 otherwise:
          erf-GELU, fused (p8_act / mid_act): Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7 on erf, with v_rcp_f32 (1 ulp) and __expf
            (v_exp_f32, 1 ulp, on an argument product rounded to 2^-24 |z^2|: z^2 e^(-z^2) <= 1 / e keeps that below 2^-23): below
            4e-7 on erf, 2^-22 |pre| on the result.  Composed (mmgl_activation_fwd): erff, 4 ulp = 2^-21 on erf.
          quick-GELU: v * v_rcp_f32(1 + __expf(-1.702 v)): the exponential's relative error 2^-23 + 2 * 1.702 |v| 2^-24 reaches the
            sigmoid through s (1 - s), and t s (1 - s) <= 0.224: below 2^-23 |pre|.  mmgl_activation_fwd divides instead (exact).
          tanh-GELU: tanhf, 2 ulp = 2^-22 absolute, on an argument of four rounded operations where u (1 - tanh^2 u) <= 0.45:
            below 2^-21 on 1 + tanh, 2^-22 |pre| on the result.
        each with a factor 2 or more of room; relative to u = 2^-8 it is nothing, it matters for fp32 on the composed route.
      * staged (composed TILE128 route only: launch_nt128, then an activation pass, a zmask pass, a residual pass, each storing in the
        operand dtype): L u |pre| where the GEMM's store precedes an activation pass, and u |act(pre), masked| where a residual pass
        follows.  The zmask pass stores the value it read or zero: no rounding.
      * the bf16 backward materialises dyp once in bf16 when there is an activation: one more operand rounding, u mag, unless scale
        is a power of two (`dyp_rounded`).
    The constants are counted, not fitted to a GPU run; c may grow by one factor of two for a rounding that is found and counted, no
    further (none was: on an MI355X the largest err / bound is 0.89-0.99 in bf16 -- the store's half ulp, which rounding alone reaches
    -- and 0.004-0.015 in fp32)."""
    U = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -23}
    LIP = {0: 1.0, 1: 1.0, 2: 1.13, 3: 1.10, 4: 1.13}
    ACT = {0: lambda t: t, 1: torch.relu, 2: lambda t: 0.5 * t * (1 + torch.erf(t * 0.5 ** 0.5)), 3: lambda t: t * torch.sigmoid(1.702 * t),
           4: lambda t: 0.5 * t * (1 + torch.tanh(0.7978845608028654 * (t + 0.044715 * t ** 3)))}

    @staticmethod
    def inputs(dtype, M, N, K, seed=0, device="cpu"):
        """Operands of a linear y[M,N] = x[M,K] W[N,K]^T and of its backward, in `dtype`: randn, W scaled by K^-0.5; bias, residual,
        zmask, dy and the accumulate priors of unit scale; y = relu(randn) (half of it exact zeros: the operand of dyp's mask) and
        xr = relu(x) (the operand of mask_dx)."""
        g = torch.Generator(device=device).manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g, device=device)
        t = dict(x=r(M, K), w=r(N, K) * K ** -0.5, bias=r(N), residual=r(M, N), zmask=r(M, N), dy=r(M, N), y=torch.relu(r(M, N)),
                 prior_w=r(N, K), prior_b=r(N))
        t["xr"] = torch.relu(t["x"])
        return {k: v.to(dtype) for k, v in t.items()}

    @staticmethod
    def chain(dtype, contraction, folds=0):
        """n of the docstring: the longest chain of fp32 roundings."""
        return -(-contraction // (16 if dtype == torch.bfloat16 else 4)) + folds + 8

    @staticmethod
    def c(n):
        return max(2.0 ** -16, 2 * n * 2.0 ** -24)

    def __init__(self, want, mag, lip=1.0, evalerr=None, pre=None, masked_act=None):
        self.want, self.mag, self.lip, self.evalerr, self.pre, self.masked_act = want, mag, lip, evalerr, pre, masked_act

    @classmethod
    def forward(cls, x, w, bias=None, act=0, scale=1.0, residual=None, zmask=None, K=None, scale_after=False):
        """scale_after: the scale applied after the activation instead of before (a deliberately wrong reference)."""
        d = lambda t: t.detach().double()
        K = x.shape[1] if K is None else K
        X, W = d(x)[:, :K], d(w)[:, :K]
        pre, mag = X @ W.t(), X.abs() @ W.abs().t()
        if bias is not None:
            pre, mag = pre + d(bias), mag + d(bias).abs()
        mag = mag * abs(scale)
        a = cls.ACT[act](pre) * scale if scale_after else cls.ACT[act](pre * scale)
        pre = pre * scale
        ev = 2.0 ** -20 * (pre.abs() + a.abs()) if act >= 2 else None
        if zmask is not None:
            a = torch.where(d(zmask) > 0, a, torch.zeros_like(a))
        want = a
        if residual is not None:
            want, mag = a + d(residual), mag + d(residual).abs()
        return cls(want, mag, cls.LIP[act], ev, pre, a)

    @staticmethod
    def dyp(dy, y=None, scale=1.0):
        v = dy.detach().double() * scale
        return v if y is None else torch.where(y.detach().double() > 0, v, torch.zeros_like(v))

    @classmethod
    def dgrad(cls, dy, w, y=None, scale=1.0, x_mask=None, mask_ge=False):
        """mask_ge: the mask taken from x >= 0 instead of x > 0 (a deliberately wrong reference)."""
        g, W = cls.dyp(dy, y, scale), w.detach().double()
        want, mag = g @ W, g.abs() @ W.abs()
        if x_mask is not None:
            xm = x_mask.detach().double()
            want = torch.where((xm >= 0) if mask_ge else (xm > 0), want, torch.zeros_like(want))
        return cls(want, mag)

    @classmethod
    def wgrad(cls, dy, x, y=None, scale=1.0, prior=None):
        g, X = cls.dyp(dy, y, scale), x.detach().double()
        want, mag = g.t() @ X, g.abs().t() @ X.abs()
        if prior is not None:
            want, mag = want + prior.detach().double(), mag + prior.detach().double().abs()
        return cls(want, mag)

    @classmethod
    def dbias(cls, dy, y=None, scale=1.0, prior=None):
        g = cls.dyp(dy, y, scale)
        want, mag = g.sum(0), g.abs().sum(0)
        if prior is not None:
            want, mag = want + prior.detach().double(), mag + prior.detach().double().abs()
        return cls(want[None, :], mag[None, :])

    def bound(self, dtype, n, composed=False, has_act_pass=False, has_residual_pass=False, dyp_rounded=False):
        """The bound, shaped like `want`.  n: GemmRef.chain of the case.  composed, has_act_pass, has_residual_pass: the staged stores
        of the TILE128 route.  dyp_rounded: the bf16 backward's materialised dyp with a scale that is no power of two."""
        u = GemmRef.U[dtype]
        b = u * self.want.abs() + self.lip * GemmRef.c(n) * self.mag
        if self.evalerr is not None:
            b = b + self.evalerr
        if composed and has_act_pass:
            b = b + self.lip * u * self.pre.abs()
        if composed and has_residual_pass:
            b = b + u * self.masked_act.abs()
        if dyp_rounded:
            b = b + u * self.mag
        return b

    def outside(self, other, dtype, n, **kw):
        """From two references alone: the elements (bool) at which `other` -- a deliberately wrong reference of the same call -- leaves
        this one's bound."""
        return (other.want - self.want).abs() > self.bound(dtype, n, **kw)

    @staticmethod
    def tiles(bad, tile):
        """The (row tile, column tile) pairs that hold the elements `bad` [k, 2]."""
        return [tuple(t) for t in torch.div(bad, tile, rounding_mode="floor").unique(dim=0).tolist()]

    def check(self, got, what, group="", n=8, **kw):
        """Asserts the bound on every element of `got`; prints and returns the largest err / bound.  A failure names the number of
        elements outside and the (row tile, column tile) pairs that hold them, in the 256 and in the 128 tiling."""
        got = got.detach().reshape(self.want.shape)
        assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
        err, bound = (got.double() - self.want).abs(), self.bound(got.dtype, n, **kw)
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        print(f"[bound {group}] {what}: max err/bound {ratio:.3f}")
        bad = (err > bound).nonzero()
        if bad.numel():
            raise AssertionError(f"{what}: {bad.shape[0]} of {err.numel()} elements outside the bound (max err/bound {ratio:.2f}); "
                                 f"(row tile, column tile) of 256: {GemmRef.tiles(bad, 256)[:24]}; of 128: {GemmRef.tiles(bad, 128)[:24]}")
        return ratio


# ------------------------------------------------------------------------------------------ row kernels (csrc/rownorm.hip, elementwise.hip)
_M64 = (1 << 64) - 1


def hash32_int(seed, i):
    """mmgl_hash32 (csrc/common.h: the splitmix64 finaliser, upper 32 bits) of one (seed, element index) pair in Python integers."""
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return ((z ^ (z >> 31)) & _M64) >> 32


def drop_threshold(p):
    """The kernels' uint32(fminf(p * 2^32, 2^32 - 1)) with p an fp32: an element is dropped when its hash is below it."""
    return min(int(float(np.float32(p)) * 4294967296.0), 4294967295)


def hash_keep(seed, n, p, start=0):
    """Keep mask (numpy bool [n]) of elements start ... start + n - 1 under (seed, p): mmgl_hash32 restated in numpy uint64, whose
    array arithmetic wraps around like the device's, against the kernels' threshold."""
    i = np.arange(n, dtype=np.uint64) + np.uint64(start)
    z = np.uint64(seed & _M64) + (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)) >= np.uint64(drop_threshold(p))


def _keep_scale(p):
    """The kernels' fp32 1.f / (1.f - p), as a Python float."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def _report(err, bound, what, group):
    """Shared tail of the row references' check(): prints the largest err / bound, names the rows and columns outside."""
    assert torch.isfinite(err).all(), f"{what}: non-finite output"
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print(f"[bound {group}] {what}: max err/bound {ratio:.3f}")
    bad = (err > bound).nonzero()
    if bad.numel():
        where = (f"rows {bad[:, 0].unique().tolist()[:16]}, columns {bad[:, 1].unique().tolist()[:16]}" if bad.shape[1] == 2
                 else f"indices {bad[:, 0].tolist()[:16]}")
        raise AssertionError(f"{what}: {bad.shape[0]} of {err.numel()} elements outside the bound (max err/bound {ratio:.2f}); {where}")
    return ratio


class Slab:
    """A tensor (.v) carved out of the middle of a buffer filled with `fill`: NaN around operands, a canary around and inside
    outputs.  64 elements of guard on either side keep the 16-byte alignment."""
    PAD = 64

    def __init__(self, shape, dtype, fill, src=None, device="cuda"):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * Slab.PAD,), fill, dtype=dtype, device=device)
        self.v = self.buf[Slab.PAD:Slab.PAD + n].view(shape)
        self.n, self.fill = n, fill
        if src is not None:
            self.v.copy_(src)

    def same(self, t):
        return bool(torch.isnan(t).all()) if isinstance(self.fill, float) and self.fill != self.fill else bool((t == self.fill).all())

    def guards_ok(self):
        return self.same(self.buf[:Slab.PAD]) and self.same(self.buf[Slab.PAD + self.n:])

    def untouched(self):
        return self.same(self.buf)


class ByteSlab:
    """A workspace of nbytes of 0xFF (fp32 NaN) between two 256-byte guards of 0xA5."""

    def __init__(self, nbytes, device="cuda"):
        self.buf = torch.full((nbytes + 512,), 0xA5, dtype=torch.uint8, device=device)
        self.buf[256:256 + nbytes] = 0xFF
        self.nbytes = nbytes

    def ptr(self):
        import ctypes
        return ctypes.c_void_p(self.buf.data_ptr() + 256)

    def guards_ok(self):
        return bool((self.buf[:256] == 0xA5).all()) and bool((self.buf[256 + self.nbytes:] == 0xA5).all())

    def untouched(self):
        return self.guards_ok() and bool((self.buf[256:256 + self.nbytes] == 0xFF).all())


U_STORE = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -23}
VEC = {torch.bfloat16: 8, torch.float32: 4}      # elements of a 16-byte chunk


class NormRef:
    """fp64 reference of the LayerNorm / RMSNorm entry points of csrc/rownorm.hip, forward and backward over s (s = x, or the sum the
    fused pairs store), on the device the storage-rounded operands live on.

    s.  p = 0: (x + r) in fp32 rounded to the operand dtype.  p > 0: fma(fp32(1 / (1 - p)), keep x, r) rounded once to fp32, then to the
    dtype, keep = hash_keep(seed, rows cols, p) at element index row cols + col.  The kernel's stored sum is compared bit for bit
    (check_sum) and everything below is taken from it.  (The fma is formed in fp64 and rounded: a 32-bit product plus a bf16 is exact
    there; in fp32 storage it is a double rounding that differs from the device's single one at a tie of about 2^-29 probability.)

    Forward, with mu, rs = (var + eps)^-1/2, d = s - mu, A = mean|s| per row, kappa = A rs (RMSNorm: mu = 0):
        want y = d rs gamma + beta                 mag y = (|d| + A) rs |gamma| + |beta|
        |mean - mu| <= 2^-18 A                     |rstd - rs| <= 2^-17 rs
    Backward, with gy = dy gamma, h = d rs, m1 = mean(gy) (RMSNorm: 0), m2 = mean(gy h):
        want dx = rs (gy - m1 - h m2) + dres       mag dx = rs (1 + kappa) (|gy| + mean|gy| + |h| mean(|gy| |h|)) + |dres|
        want dx_drop = keep / (1 - p) dx           (p > 0: the gradient of the dropped branch, one more store)
        want dgamma = sum_r dy h                   mag = sum_r |dy| (|h| + kappa_r)
        want dbeta  = sum_r dy                     mag = sum_r |dy|
    Bounds, functions of the reference alone (every element is checked):
        y, dx            |got - want| <= u |want| + 2^-16 mag                 u = 2^-8 (bf16) / 2^-23 (fp32)
        dx_drop          keep / (1 - p) times dx's bound, + u |want dx_drop|
        dgamma, dbeta    |got - want| <= 2^-24 |want| + max(2^-16, 2 n 2^-24) mag,   n = NormRef.chain(rows, tpr)
    The count of roundings:
      * mean: a thread adds at most NV VN = 32 elements, the wave sum is 6 shuffle steps, the block adds 4 wave sums (3), one
        division: about 41 roundings of 2^-24 relative to A, counted as 64 = 2^-18 A.
      * rstd: the variance takes the same chain on d^2 (all terms positive: a relative error), d carries its own rounding and the
        mean's error delta, which enters the sum as delta^2 only; rsqrtf is 1 ulp.  Half of 64 + 4 roundings on var, + 2^-23: 2^-17.
      * y: the mean's error reaches it as delta rs gamma <= 2^-18 A rs |gamma|, rstd's as 2^-17 |d| rs |gamma|, then three rounded
        operations: all inside 2^-16 mag -- SkinnyRef's floor of 256 roundings; the chains above are under 64.
      * dx: m1 and m2 take the mean's chain on gy and gy h; the kernel forms h from the SAVED fp32 mean and rstd, whose errors
        (2^-18 A rs = 2^-18 kappa on h, 2^-17 |h|) are what the factor (1 + kappa) carries.
      * dgamma / dbeta: chain(rows, tpr) = rows per partial row + partial rows / 8 (norm_param_reduce_kernel's lane) + 8 (its LDS
        fold) + 8 (h, the product, the two stores); partial rows = blocks x rows per block with blocks capped at 512 (bwd_blocks).
    Nothing is fitted to a run.  Keyword arguments build deliberately wrong references: stat_cols (bool [cols]: the columns that
    enter the statistics, or m1 / m2, still divided by cols), grad_rows (bool [rows]: the rows that enter dgamma / dbeta), no_dres,
    mask_row_shift (the mask's element index offset by that many rows)."""

    @staticmethod
    def edges(cols, vn):
        """The columns scaled by 16: chunk, lane-trip and row ends."""
        nch = cols // vn
        e = [0, vn - 1, vn, (nch // 2) * vn, 64 * vn - 1, 64 * vn, 256 * vn - 1, 256 * vn, cols - vn - 1, cols - vn, cols - 1]
        return sorted({c for c in e if 0 <= c < cols})

    @staticmethod
    def edge_rows(rows, seams=()):
        e = [0, 3, 4, rows - 2, rows - 1] + [r + o for r in seams for o in (-1, 0)]
        return sorted({r for r in e if 0 <= r < rows})

    @staticmethod
    def inputs(dtype, rows, cols, seed=0, device="cpu", seams=()):
        """x = 2 randn + 0.5, res, dy, dres, gamma = 1 + randn / 2, beta = randn / 2 in `dtype`; x and dy times 16 on the edge columns,
        dy times 16 on the edge rows (0, 3, 4, rows - 2, rows - 1 and both sides of every grid-stride seam).  Drawn on the CPU (the same
        numbers whatever the device), then moved."""
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g)
        t = dict(x=2 * r(rows, cols) + 0.5, res=r(rows, cols), dy=r(rows, cols), dres=r(rows, cols), gamma=1 + 0.5 * r(cols), beta=0.5 * r(cols))
        ec = NormRef.edges(cols, VEC[dtype])
        t["x"][:, ec] *= 16
        t["dy"][:, ec] *= 16
        t["dy"][NormRef.edge_rows(rows, seams)] *= 16
        return {k: v.to(dtype).to(device) for k, v in t.items()}

    @staticmethod
    def chain(rows, tpr):
        """n of the dgamma / dbeta bound; restates bwd_blocks (csrc/rownorm.hip)."""
        rpb = 256 // tpr
        blocks = min(-(-rows // rpb), 512)
        parts = blocks * rpb
        return -(-rows // parts) + -(-parts // 8) + 8 + 8

    @staticmethod
    def c(n):
        return max(2.0 ** -16, 2 * n * 2.0 ** -24)

    @staticmethod
    def keep(seed, rows, cols, p, device, row_shift=0):
        k = hash_keep(seed, rows * cols, p, start=row_shift * cols)
        return torch.from_numpy(k).view(rows, cols).to(device)

    def __init__(self, x, gamma=None, beta=None, rms=False, eps=1e-5, res=None, p=0.0, seed=0, s=None, stat_cols=None, mask_row_shift=0):
        d = lambda t: t.detach().double()
        rows, cols = x.shape
        self.rows, self.cols, self.dtype, self.rms, self.p = rows, cols, x.dtype, rms, p
        self.keep = None
        if res is None:
            self.s = x.detach()
        elif p > 0:
            self.keep = NormRef.keep(seed, rows, cols, p, x.device, mask_row_shift)
            self.s = (_keep_scale(p) * torch.where(self.keep, d(x), torch.zeros_like(d(x))) + d(res)).float().to(x.dtype)
        else:
            self.s = (x.detach().float() + res.detach().float()).to(x.dtype)
        S = d(self.s if s is None else s)          # s: the kernel's stored sum, once check_sum has held it against self.s
        w = torch.ones(cols, dtype=torch.float64, device=x.device) if stat_cols is None else stat_cols.to(x.device).double()
        self.w = w
        mu = torch.zeros(rows, 1, dtype=torch.float64, device=x.device) if rms else (S * w).sum(1, keepdim=True) / cols
        dd = S - mu
        rs = ((dd * dd * w).sum(1, keepdim=True) / cols + float(np.float32(eps))).rsqrt()
        A = S.abs().mean(1, keepdim=True)
        self.mu, self.rs, self.A, self.kappa, self.d = mu, rs, A, A * rs, dd
        self.gamma = None if gamma is None else d(gamma)
        y, mag = dd * rs, (dd.abs() + A) * rs
        if gamma is not None:
            y, mag = y * d(gamma), mag * d(gamma).abs()
        if beta is not None:
            y, mag = y + d(beta), mag + d(beta).abs()
        self.want = dict(y=y, mean=mu[:, 0], rstd=rs[:, 0])
        self.mag = dict(y=mag, mean=A[:, 0], rstd=rs[:, 0])

    def backward(self, dy, dres=None, grad_rows=None, no_dres=False):
        """Adds dx, dx_drop (p > 0), dgamma and dbeta to want / mag; returns self."""
        d = lambda t: t.detach().double()
        DY, h, rs, w, cols = d(dy), self.d * self.rs, self.rs, self.w, self.cols
        gy = DY if self.gamma is None else DY * self.gamma
        mean = lambda t: (t * w).sum(1, keepdim=True) / cols
        m1 = torch.zeros_like(rs) if self.rms else mean(gy)
        m2 = mean(gy * h)
        dx = rs * (gy - m1 - h * m2)
        mag = rs * (1 + self.kappa) * (gy.abs() + gy.abs().mean(1, keepdim=True) + h.abs() * (gy.abs() * h.abs()).mean(1, keepdim=True))
        if dres is not None:
            mag = mag + d(dres).abs()
            if not no_dres:
                dx = dx + d(dres)
        self.want["dx"], self.mag["dx"] = dx, mag
        if self.keep is not None:
            self.want["dx_drop"] = torch.where(self.keep, dx * _keep_scale(self.p), torch.zeros_like(dx))
            self.mag["dx_drop"] = torch.where(self.keep, mag * _keep_scale(self.p), torch.zeros_like(mag))
        r = torch.ones(self.rows, 1, dtype=torch.float64, device=DY.device) if grad_rows is None else grad_rows.to(DY.device).double()[:, None]
        self.want["dgamma"], self.mag["dgamma"] = (DY * h * r).sum(0), (DY.abs() * (h.abs() + self.kappa) * r).sum(0)
        self.want["dbeta"], self.mag["dbeta"] = (DY * r).sum(0), (DY.abs() * r).sum(0)
        return self

    def bound(self, name, tpr=64):
        want, mag, u = self.want[name], self.mag[name], U_STORE[self.dtype]
        if name == "mean":
            return 2.0 ** -18 * mag
        if name == "rstd":
            return 2.0 ** -17 * mag
        if name in ("dgamma", "dbeta"):
            return 2.0 ** -24 * want.abs() + NormRef.c(NormRef.chain(self.rows, tpr)) * mag
        if name == "dx_drop":                # mag is already keep / (1 - p) times dx's: the first store's half ulp passes through the scale
            return u * want.abs() + (u * want.abs() + 2.0 ** -16 * mag)
        return u * want.abs() + 2.0 ** -16 * mag

    def outside(self, other, name, tpr=64):
        """From two references alone: the elements at which `other` (a deliberately wrong reference) leaves this one's bound."""
        return (other.want[name] - self.want[name]).abs() > self.bound(name, tpr)

    def check_sum(self, got, what):
        assert torch.equal(got, self.s), f"{what}: the stored sum is not the reference's, bit for bit ({(got != self.s).sum().item()} elements differ)"

    def check(self, got, name, what, group="", tpr=64):
        """Asserts the bound of output `name` on every element of `got`; prints and returns the largest err / bound."""
        want = self.want[name]
        got = got.detach().reshape(want.shape).double()
        err, bound = (got - want).abs(), self.bound(name, tpr)
        if err.dim() == 1:                   # per-row outputs are reported as rows, the parameter gradients as columns
            err, bound = (err[None, :], bound[None, :]) if name in ("dgamma", "dbeta") else (err[:, None], bound[:, None])
        return _report(err, bound, f"{what} {name}", group)


class CrossEntropyRef:
    """fp64 reference of mmgl_cross_entropy_fwd / bwd (csrc/elementwise.hip) from the storage-rounded logits, on their device.

    With max_r, lse_r = log sum_j exp x_j, p = exp(x - lse), H_r = sum_j p_j (max_r - x_j), live rows those whose label is not the
    ignore index and lies in [0, V), count = their number, scale = dloss / max(count, 1) (`count` overrides the divisor: the LM head
    scores a chunk of rows against the count of the whole batch):
        row_lse    |got - lse| <= 2^-23 (|max| + |lse|) + n 2^-24 (1 + H) =: b_lse,      n = 3 ceil(V / (256 VN)) + VN + 16
        row_loss   want lse - x_label, bound b_lse + 2^-24 (|lse| + |x_label|); exactly 0 on ignored rows
        count      exact;   loss_sum  within the sum of the live rows' bounds + (rows / 256 + 16) 2^-24 sum|row_loss|
        dlogits    want (p - onehot) scale;  |got - want| <= u |want| + |scale| (p_j (b_lse + 2^-22 (1 + |x_j - lse|)) + 2^-24),
                   every element; exactly 0 on ignored rows and at -inf logits.        u = 2^-8 (bf16) / 2^-23 (fp32)
    The count of roundings: n is the folds of one thread (ceil(V / (256 VN)) of them, three roundings each: the rescale of the
    running sum, its product, the add), the sum inside a 16-byte vector (VN), and the block merge with logf (rescale, 6 shuffle
    steps, 3 adds of wave sums, logf at 2 ulp, the final add: 16).  H is how the rounding |a| 2^-24 of __expf's argument a = x - m
    reaches the sum: sum_j p_j |x_j - max| 2^-24 relative to the sum, times the same n.  2^-23 (|max| + |lse|) is the rounding of
    the running maximum's differences and of the final gm + logf(gs).  In dlogits, b_lse is the saved lse's error in the exponent,
    2^-22 (1 + |x - lse|) is v_exp_f32 at 1 ulp plus the rounded argument difference and its product with log2 e, and 2^-24 is the
    subtraction of the one-hot; the division dloss / count and the product with it are inside u |want| in fp32 (2 x 2^-24).
    Nothing is fitted to a run.  Keyword arguments build deliberately wrong references: lse_cols (bool [V]: the columns that enter
    lse), label_shift (the one-hot offset by that many columns), by_rows (division by rows instead of count), live_row (an ignored
    row treated as live: its gradient is p scale, its loss lse)."""

    @staticmethod
    def edges(V, vn):
        e = [0, vn - 1, vn, 256 * vn - 1, 256 * vn, 768 * vn - 1, 768 * vn, 1024 * vn - 1, 1024 * vn, V - vn - 1, V - vn, V - 1]
        return sorted({c for c in e if 0 <= c < V})

    @staticmethod
    def inputs(dtype, V, seed=0, device="cpu", ignore=-100):
        """Six rows of unit randn logits with the edge columns at max(2, ln(0.165 V)) (each edge holds about 4.5 % of its row's mass
        at any V), labels 0, V - 1, ignore, an edge, V / 2, 7 (clamped to V - 1).  Drawn on the CPU, then moved."""
        import math
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(6, V, generator=g)
        ec = CrossEntropyRef.edges(V, VEC[dtype])
        x[:, ec] = max(2.0, math.log(0.165 * V))
        lab = torch.tensor([0, V - 1, ignore, ec[len(ec) // 2], V // 2, min(7, V - 1)], dtype=torch.int64)
        return x.to(dtype).to(device), lab.to(device)

    def __init__(self, logits, labels, ignore=-100, dloss=1.0, count=None, lse_cols=None, label_shift=0, by_rows=False, live_row=None):
        X = logits.detach().double()
        rows, V = X.shape
        self.rows, self.V, self.dtype, self.x = rows, V, logits.dtype, X
        vn = VEC[logits.dtype]
        neg = torch.full_like(X, float("-inf"))
        Xs = X if lse_cols is None else torch.where(lse_cols.to(X.device)[None, :], X, neg)
        mx = Xs.amax(1, keepdim=True)
        lse = torch.logsumexp(Xs, 1, keepdim=True)
        p = torch.exp(X - lse)
        ps = torch.exp(Xs - lse)
        H = torch.where(ps > 0, ps * (mx - Xs), torch.zeros_like(ps)).sum(1, keepdim=True)
        n = 3 * -(-V // (256 * vn)) + vn + 16
        b_lse = 2.0 ** -23 * (mx.abs() + lse.abs()) + n * 2.0 ** -24 * (1 + H)
        lab = labels.detach().to(X.device)
        live = (lab != ignore) & (lab >= 0) & (lab < V)
        self.live, self.p = live, p
        safe = torch.where(live, lab, torch.zeros_like(lab))
        xl = X.gather(1, safe[:, None])
        row_loss = torch.where(live[:, None], lse - xl, torch.zeros_like(lse))
        b_loss = torch.where(live[:, None], b_lse + 2.0 ** -24 * (lse.abs() + xl.abs()), torch.zeros_like(lse))
        cnt = float(live.sum().item())
        div = float(rows) if by_rows else (cnt if count is None else float(count))
        scale = float(np.float32(dloss)) / max(div, 1.0)
        onehot = torch.zeros_like(X)
        tgt = safe + label_shift
        tgt = torch.where(tgt >= V, safe - label_shift, tgt).clamp(0, V - 1)
        onehot.scatter_(1, tgt[:, None], 1.0)
        g = torch.where(live[:, None], (p - onehot) * scale, torch.zeros_like(p))
        b_g = abs(scale) * (p * (b_lse + 2.0 ** -22 * (1 + torch.where(p > 0, (X - lse).abs(), torch.zeros_like(p)))) + 2.0 ** -24)
        if live_row is not None:
            g[live_row] = p[live_row] * scale
            row_loss[live_row] = lse[live_row]
        self.exact0 = (~live[:, None]) | torch.isneginf(X)              # where dlogits must be exactly zero
        self.want = dict(row_lse=lse[:, 0], row_loss=row_loss[:, 0], loss_sum=row_loss.sum().reshape(1), dlogits=g,
                         count=torch.tensor([cnt], dtype=torch.float64, device=X.device))
        self.mag = dict(row_lse=mx.abs()[:, 0] + lse.abs()[:, 0], row_loss=row_loss.abs()[:, 0], dlogits=abs(scale) * p)
        self._bound = dict(row_lse=b_lse[:, 0], row_loss=b_loss[:, 0], count=torch.zeros(1, dtype=torch.float64, device=X.device),
                           loss_sum=(b_loss.sum() + (rows / 256 + 16) * 2.0 ** -24 * row_loss.abs().sum()).reshape(1),
                           dlogits=U_STORE[logits.dtype] * g.abs() + torch.where(self.exact0, torch.zeros_like(b_g), b_g))

    def bound(self, name):
        return self._bound[name]

    def outside(self, other, name):
        return (other.want[name] - self.want[name]).abs() > self.bound(name)

    def check(self, got, name, what, group=""):
        want = self.want[name]
        got = got.detach().reshape(want.shape).double()
        err, bound = (got - want).abs(), self.bound(name)
        if err.dim() == 1:
            err, bound = err[:, None], bound[:, None]
        return _report(err, bound, f"{what} {name}", group)


class GatedRef:
    """fp64 reference of mmgl_gated_residual_fwd / bwd (csrc/elementwise.hip) over n elements, on the operands' device.

    With tg = tanh(gate) (1 without a gate), keep = hash_keep(seed, n, p), inv = 1 / (1 - p):
        want y  = r + (tg inv) keep x              one fma, one store:   |got - want| <= u |want| + 2^-22 (|r| + |tg inv keep x|)
        want dx = tg keep inv dy                   |got - want| <= u |want| + 2^-21 |want|
        want dgate = (1 - tg^2) sum dy keep inv x  |got - want| <= 2^-23 |want| + max(2^-16, 2 n 2^-24) mag,   mag = (1 - tg^2) sum|dy keep inv x|
    2^-22 carries tanhf at 2 ulp and the scale's own rounding (the fp32 1 - p, the division).  dx is two rounded products of three
    rounded factors -- tanhf at 2 ulp (2^-22), 1 - p and the division (2 x 2^-24), the products (2 x 2^-24): 2^-21 -- then the store.
    n = elements per thread (VN per grid-stride trip, + the n % VN tail elements of thread 0) + 6 (wave shuffle) + 4 (block) +
    blocks / 256 (gate_grad_kernel's thread) + 8 (its block sum, tanhf, 1 - tg^2, the product); blocks = min(ceil(nvec / 256), 2048).
    `index_shift` (a deliberately wrong reference) offsets the mask's element index."""

    @staticmethod
    def blocks(n, vn):
        return min(max(-(-(n // vn) // 256), 1), 2048)

    @staticmethod
    def chain(n, vn):
        b = GatedRef.blocks(n, vn)
        return -(-(n // vn) // (b * 256)) * vn + n % vn + 6 + 4 + -(-b // 256) + 8

    def __init__(self, res, x, gate=None, p=0.0, seed=0, index_shift=0):
        import math
        d = lambda t: t.detach().double().reshape(-1)
        self.dtype, self.n = x.dtype, x.numel()
        self.tg = 1.0 if gate is None else math.tanh(float(gate))
        self.inv = _keep_scale(p)
        keep = torch.from_numpy(hash_keep(seed, self.n, p, start=index_shift)).to(x.device) if p > 0 else torch.ones(self.n, dtype=torch.bool, device=x.device)
        self.kx = torch.where(keep, d(x), torch.zeros_like(d(x))) * self.inv
        self.keep = keep
        term = self.tg * self.kx
        u = U_STORE[x.dtype]
        self.want = dict(y=d(res) + term)
        self.mag = dict(y=d(res).abs() + term.abs())
        self._bound = dict(y=u * self.want["y"].abs() + 2.0 ** -22 * self.mag["y"])

    def backward(self, dy):
        DY, u = dy.detach().double().reshape(-1), U_STORE[self.dtype]
        dx = torch.where(self.keep, DY, torch.zeros_like(DY)) * (self.tg * self.inv)
        c = max(2.0 ** -16, 2 * GatedRef.chain(self.n, VEC[self.dtype]) * 2.0 ** -24)
        t2 = 1 - self.tg * self.tg
        self.want.update(dx=dx, dgate=(t2 * (DY * self.kx).sum()).reshape(1))
        self.mag.update(dx=dx.abs(), dgate=(abs(t2) * (DY * self.kx).abs().sum()).reshape(1))
        self._bound.update(dx=(u + 2.0 ** -21) * dx.abs(), dgate=2.0 ** -23 * self.want["dgate"].abs() + c * self.mag["dgate"])
        return self

    def bound(self, name):
        return self._bound[name]

    def outside(self, other, name):
        return (other.want[name] - self.want[name]).abs() > self.bound(name)

    def check(self, got, name, what, group=""):
        want = self.want[name]
        got = got.detach().reshape(want.shape).double()
        return _report((got - want).abs()[:, None], self.bound(name)[:, None], f"{what} {name}", group)


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
        n, u = (self.D + 8) * 2.0 ** -24, SelfAttnRef.U[dtype]
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
        ratios, failed = {}, []
        U = self.uni_rows
        for name in GeneralAttnRef.NAMES + ("probs",):
            x = got.get(name)
            if x is None:
                continue
            want = self.want[name]
            x = x.detach().reshape(want.shape)
            if name == "lse":
                assert bool((x[U[:, None, :].expand_as(x)] == float("inf")).all()), f"{what} lse: a row without an allowed key is not +inf"
                xs = torch.where(torch.isinf(want), torch.zeros_like(want), x.double())
                assert torch.isfinite(xs).all(), f"{what} lse: non-finite on a row with an allowed key"
                err = (xs - torch.where(torch.isinf(want), torch.zeros_like(want), want)).abs()
            else:
                assert torch.isfinite(x.float()).all(), f"{what} {name}: non-finite result"
                err = (x.double() - want).abs()
            if name == "probs" and bool(U.any()):
                ex = self.exact_probs(dtype)[None, :, None, None].expand_as(x)
                sel = U[:, None, :, None].expand_as(x)
                assert torch.equal(x[sel], ex[sel]), f"{what} probs: a row without an allowed key is not exactly fp32(1/S) hm"
                err = err.masked_fill(sel, 0.0)
            bound = self.bound(name, dtype)
            sel = None
            if rows is not None and name in ("out", "dq"):
                sel = rows[:, :, None, None].expand_as(err)
            elif rows is not None and name == "lse":
                sel = rows[:, None, :].expand_as(err)
            elif rows is not None and name == "probs":
                sel = rows[:, None, :, None].expand_as(err)
            elif keys is not None and name in ("dk", "dv"):
                sel = keys[:, :, None, None].expand_as(err)
            elif rows is not None or keys is not None:
                continue
            if sel is not None:
                err, bound = err[sel], bound[sel]
                if not err.numel():
                    continue
            ratios[name] = (err / bound.clamp_min(1e-300)).max().item() if bool((err > 0).any()) else 0.0
            print(f"[bound {group}] {what} {name}: max err/bound {ratios[name]:.3f}")
            bad = (err > bound).nonzero()
            if bad.numel():
                failed.append(f"{what} {name}: {bad.shape[0]} of {err.numel()} elements outside the bound (max err/bound "
                              f"{ratios[name]:.2f}); first indices {bad[:8].tolist()}")
        assert not failed, "\n".join(failed)
        return ratios


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
        want = self.want["out"]
        r = self.rows(q_rows)
        x = got.detach().reshape(want.shape)[r]
        assert torch.isfinite(x.float()).all(), f"{what} out: non-finite result"
        err, bound = (x.double() - want[r]).abs(), self.bound("out", self.dtype)[r]
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        print(f"[bound {group}] {what} out: max err/bound {ratio:.3f}")
        bad = (err > bound).nonzero()
        assert not bad.numel(), (f"{what} out: {bad.shape[0]} of {err.numel()} elements outside the bound (max err/bound {ratio:.2f}); "
                                 f"(row among the written, head) {bad[:, :2].unique(dim=0).tolist()[:12]}")
        return ratio


# ------------------------------------------------------------------------------------------ streaming ops (csrc/llama_ops.hip, elementwise.hip)
TINY = 2.0 ** -126      # the smallest normal fp32: what a result flushed to zero, or an overflowed __expf's sigmoid of 0, can lose


class RopeRef:
    """fp64 reference of mmgl_rope_inplace / mmgl_rope (csrc/llama_ops.hip) over buf [rows, ld], on the operands' device: the row is
    `nall` column blocks of `unit` heads x D, the first `nblk` are rotated, the rest copied.  For pair (i, i + D/2) of a rotated head,
    with (c, s) the fp32 table entry cos_sin[row % T, i] and sigma = +1 forward / -1 backward:
        lo' = x0 c - sigma x1 s        mag = |x0 c| + |x1 s|
        hi' = x1 c + sigma x0 s        mag = |x1 c| + |x0 s|
        |got - want| <= u |want| + 3 * 2^-24 mag
    u |want| is the store's half ulp (bf16) or the last add's rounding counted once more (fp32); 3: the two products and the add (two
    with the contraction to an fma), each at most 2^-24 of mag.  The operands and the table are exact in fp32.  The unrotated blocks are
    compared bit for bit by the caller (`rotated` names the columns).
    Deliberately wrong references: `partner_shift` (the pair partner one 16-byte vector off, inside the head's half), `t_shift` (the
    position one off), backward not flipped (pass the other `backward`), the v block rotated (pass nblk = nall), `flat_table` (the table
    offset c * VN of the thread's chunk ignored: entry i % VN)."""

    @staticmethod
    def table(T, D, device="cpu"):
        """cos_sin fp32 [T, D/2, 2] of the usual angles t 10000^(-2i/D); T = 1 is the angle 0: (1, 0) exactly."""
        i = torch.arange(D // 2, dtype=torch.float64, device=device)
        ang = torch.arange(T, dtype=torch.float64, device=device)[:, None] * 10000.0 ** (-2 * i / D)[None, :]
        return torch.stack([ang.cos(), ang.sin()], -1).float().contiguous()

    @staticmethod
    def inputs(dtype, rows, ld, seed=0, device="cpu"):
        g = torch.Generator(device=device).manual_seed(seed)
        return torch.randn(rows, ld, generator=g, device=device).to(dtype)

    def __init__(self, x, cos_sin, T, unit, D, nblk, nall, backward=False, partner_shift=0, t_shift=0, flat_table=False):
        rows, half, vn = x.shape[0], D // 2, VEC[x.dtype]
        self.dtype, self.width = x.dtype, nall * unit * D
        X = x.detach()[:, :self.width].double().view(rows, nall * unit, 2, half)
        x0, x1 = X[:, :, 0], X[:, :, 1]
        p0, p1 = (x1, x0) if not partner_shift else (torch.roll(x1, -partner_shift * vn, -1), torch.roll(x0, -partner_shift * vn, -1))
        t = (torch.arange(rows, device=x.device) + t_shift) % T
        i = torch.arange(half, device=x.device)
        cs = cos_sin.detach().double()[t][:, i % vn if flat_table else i]          # [rows, half, 2]
        c, s = cs[:, None, :, 0], cs[:, None, :, 1] * (-1.0 if backward else 1.0)
        rot = (torch.arange(nall * unit, device=x.device) < nblk * unit)[None, :, None]
        want = torch.stack([torch.where(rot, x0 * c - p0 * s, x0), torch.where(rot, x1 * c + p1 * s, x1)], 2)
        mag = torch.stack([(x0 * c).abs() + (p0 * s).abs(), (x1 * c).abs() + (p1 * s).abs()], 2)
        self.want, self.mag = want.reshape(rows, self.width), torch.where(rot[:, :, None], mag, torch.zeros_like(mag)).reshape(rows, self.width)
        self.rotated = rot[:, :, None].expand(1, nall * unit, 2, half).reshape(self.width)

    def bound(self):
        return U_STORE[self.dtype] * self.want.abs() + 3 * 2.0 ** -24 * self.mag

    def outside(self, other):
        return (other.want - self.want).abs() > self.bound()

    def check(self, got, what, group=""):
        got = got.detach()[:, :self.width]
        r = _report((got.double() - self.want).abs(), self.bound(), what, group)
        assert torch.equal(got[:, ~self.rotated], self.want[:, ~self.rotated].to(got.dtype)), f"{what}: an unrotated block is no bit-for-bit copy"
        return r


class SwigluRef:
    """fp64 reference of mmgl_swiglu_fwd / mmgl_swiglu_bwd (csrc/llama_ops.hip) over gu [M, 2F] = [gate | up] and dy [M, F], with
    s = sigmoid(g):
        y = g s u        du = dy g s        dg = dy u s (1 + g (1 - s))
    The kernel forms s = 1 / (1 + __expf(-g)) in fp32.  __expf is v_exp_f32 (1 ulp, 2^-23) on the product g log2(e) rounded to fp32
    (2^-24 |g| on the result); with a factor 2 of room, rel_e = 2^-22 + |g| 2^-23.  It reaches s through ds / s = -(1 - s) de / e; the
    add 1 + e and the division round s twice more.  Per element:
        y, du:  |got - want| <= u |want| + (4 * 2^-24 + (1 - s) rel_e) |want| + floor
                4: the two roundings of s and the two products.
        dg:     |got - want| <= u |want| + (8 * 2^-24 + 2 (1 - s) rel_e) mag + 2 * 2^-24 |g| |dy u| s + floor
                mag = |dy u| s (1 + |g| (1 - s)) >= |want|: at the root of silu' (g = -1.27846) want cancels and only mag is left.
                8: the three products and the two roundings of s on the result (5), the rounding of 1 - s, of g (1 - s) and of the sum
                (3, each at most 2^-24 (1 + |g| (1 - s))).  rel_e twice: through s and through 1 - s.
                2 * 2^-24 |g| |dy u| s: the cancellation.  For g in about [6, 20] s is within 2^-24 of 1, its two roundings are an
                ABSOLUTE 2 * 2^-24 s on 1 - s = e^-g, whatever its size, and the factor g multiplies them.
        floor = 2^-126 (1 + P): for g < -87 __expf(-g) overflows, s is 0 where sigmoid(g) < 2^-126, and a product below the smallest
                normal may be flushed.  P = |g u| + |u| (y), |dy g| + |dy| (du), |dy u| (1 + |g|) (dg).
    Deliberately wrong references: `swap` (gate and up exchanged), `no_gterm` (silu' without g (1 - s)), `up_pitch_f` (up read at row
    pitch F instead of 2F)."""

    ROOT = -1.2784645                       # silu'(g) = 0
    PLANTED_G = [ROOT] + [float(k) for k in range(6, 21)] + [float(k) for k in range(-104, -59, 4)] + [0.0, -0.0]

    @staticmethod
    def inputs(dtype, M, F, seed=0, device="cpu"):
        """gu [M, 2F] and dy [M, F] = randn * 4 with planted values, all finite, at evenly spread elements: the gates of PLANTED_G (the
        root of silu', a grid over [6, 20], a grid over [-104, -60], +0 and -0), then two zeros of u and two of dy.  A case with fewer
        than 68 elements plants half of its elements (the rest stay random), starting at planted value number M F + seed; every case
        from 68 elements on holds the whole list."""
        g = torch.Generator(device=device).manual_seed(seed)
        gu = torch.randn(M, 2 * F, generator=g, device=device) * 4
        dy = torch.randn(M, F, generator=g, device=device) * 4
        vals = SwigluRef.PLANTED_G + ["u", "u", "dy", "dy"]
        n = M * F
        k = min(max(n // 2, 1), len(vals))
        for j in range(k):
            e = j * (n // k)
            r, c = e // F, e % F
            val = vals[(j + (n + seed if k < len(vals) else 0)) % len(vals)]
            if val == "u":
                gu[r, F + c] = 0.0
            elif val == "dy":
                dy[r, c] = 0.0
            else:
                gu[r, c] = val
        return gu.to(dtype), dy.to(dtype)

    def __init__(self, gu, dy=None, swap=False, no_gterm=False, up_pitch_f=False):
        M, F = gu.shape[0], gu.shape[1] // 2
        self.dtype = gu.dtype
        G = gu.detach().double()
        g, u = G[:, :F], G[:, F:]
        if up_pitch_f:
            idx = torch.arange(M, device=gu.device)[:, None] * F + F + torch.arange(F, device=gu.device)[None, :]
            u = G.reshape(-1)[idx]
        if swap:
            g, u = u, g
        s = torch.sigmoid(g)
        one_s = torch.sigmoid(-g)                              # 1 - s without the cancellation
        rel_e = 2.0 ** -22 + g.abs() * 2.0 ** -23
        uu, r = U_STORE[self.dtype], 2.0 ** -24
        y = g * s * u
        self.want = dict(y=y)
        self._bound = dict(y=(uu + 4 * r + one_s * rel_e) * y.abs() + TINY * (1 + (g * u).abs() + u.abs()))
        if dy is not None:
            d = dy.detach().double()
            du = d * g * s
            fac = 1 + (0 if no_gterm else 1) * g * one_s
            dg = d * u * s * fac
            du_s = (d * u).abs() * s
            mag = du_s * (1 + g.abs() * one_s)
            self.want.update(du=du, dg=dg)
            self._bound.update(du=(uu + 4 * r + one_s * rel_e) * du.abs() + TINY * (1 + (d * g).abs() + d.abs()),
                               dg=uu * dg.abs() + (8 * r + 2 * one_s * rel_e) * mag + 2 * r * g.abs() * du_s + TINY * (1 + (d * u).abs() * (1 + g.abs())))

    def bound(self, name):
        return self._bound[name]

    def outside(self, other, name):
        return (other.want[name] - self.want[name]).abs() > self.bound(name)

    def err(self, got, name):
        return (got.detach().reshape(self.want[name].shape).double() - self.want[name]).abs()

    def check(self, got, name, what, group=""):
        return _report(self.err(got, name), self.bound(name), f"{what} {name}", group)


class ActRef:
    """fp64 reference of mmgl_activation_fwd (csrc/elementwise.hip) over n elements: GemmRef.ACT[act], within u |want| + E with
    GemmRef's evaluation term E = 2^-20 (|x| + |act(x)|) of the composed route for the three GELUs (0 for ReLU: a select).  `fn`
    replaces the activation (a deliberately wrong reference)."""

    PLANTED = [s * a for a in (0.0, 1e-30, 5.0, 9.0, 30.0, 100.0, 1e13, 1e20) for s in (1.0, -1.0)]

    @staticmethod
    def inputs(dtype, n, seed=0, device="cpu"):
        """randn * 3 with PLANTED (rounded to the dtype) over the leading elements, as many as fit, starting at value number n: the
        1 + erf cancellation (-5, -9), the cube overflowing inside tanh-GELU (1e13, 1e20), __expf overflowing inside quick-GELU (-100)."""
        g = torch.Generator(device=device).manual_seed(seed)
        x = torch.randn(n, generator=g, device=device) * 3
        k = min(n, len(ActRef.PLANTED))
        x[:k] = torch.tensor([ActRef.PLANTED[(j + (n if k < len(ActRef.PLANTED) else 0)) % len(ActRef.PLANTED)] for j in range(k)], device=device)
        return x.to(dtype)

    def __init__(self, x, act, fn=None):
        pre = x.detach().double().reshape(-1)
        self.dtype = x.dtype
        self.want = (fn or GemmRef.ACT[act])(pre)
        self._bound = U_STORE[x.dtype] * self.want.abs() + (2.0 ** -20 * (pre.abs() + self.want.abs()) if act >= 2 else 0.0)

    def bound(self):
        return self._bound

    def outside(self, other):
        return (other.want - self.want).abs() > self.bound()

    def check(self, got, what, group=""):
        return _report((got.detach().reshape(-1).double() - self.want).abs()[:, None], self.bound()[:, None], what, group)


class AdamWRef:
    """fp64 reference of ONE step of mmgl_adamw_step (csrc/elementwise.hip) from the state the kernel was handed -- p (the fp32 master
    where there is one, else the parameter), m, v, g -- over the hyperparameters rounded to float32 as the C ABI receives them; the bias
    corrections bc1 = 1 - b1^step, bc2 = 1 - b2^step are the exact functions of those floats.  With gs = g grad_scale:
        m' = b1 m + (1 - b1) gs                            mag_m = |b1 m| + |(1 - b1) gs|
        v' = b2 v + (1 - b2) gs^2                          (no cancellation: v >= 0)
        p' = p (1 - lr wd) - upd,  upd = (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)
    Bounds, roundings of 2^-24 counted from adamw_kernel (`floor` = 2^-126, a result flushed below the smallest normal):
        m': 4 mag_m + floor     gs, 1 - b1, its product, the sum (b1 m: the product and the sum)
        v': 6 v' + floor        gs twice, 1 - b2, two products, the sum
        p': 4 |p| + 16 U + u_store |want| (+ U sqrt(floor) / (sqrt(bc2) den))
            U = (lr / bc1) mag_m / den, den = sqrt(v') / sqrt(bc2) + eps: the update with m' at its magnitude, because the 4 roundings of
            m' are relative to mag_m and pass through unchanged.  4 |p|: lr wd, 1 - lr wd, the product, the final subtraction.  16 U: bc1
            as a correctly rounded fp32 (1) and lr / bc1 (1), its product with m' (1), m' (4), the denominator (7: v' halved by the
            square root 3, sqrtf 1, bc2s as a correctly rounded fp32 1, the division 1, + eps 1), the division (1), the final
            subtraction (1).  u_store |want|: only for a bf16 parameter without a master (the one bf16 store); a master is fp32 and
            the bf16 parameter is its rounding, bit for bit (the caller compares).
    Deliberately wrong references: `decay_after`, `bc_step` (the bias corrections of another step), `no_bc2`, `no_grad_scale`,
    `eps_inside`, `bc` = (bc1, bc2s) given (the host's fp32 powf arithmetic)."""

    @staticmethod
    def f32(x):
        return float(np.float32(x))

    @staticmethod
    def bc_fp32(b1, b2, step):
        """bc1 and bc2s as 1.f - powf(beta, step) and sqrtf(1.f - powf(beta, step)) give them, restated in numpy float32."""
        one, st = np.float32(1), np.float32(step)
        return float(one - np.power(np.float32(b1), st)), float(np.sqrt(one - np.power(np.float32(b2), st)))

    PLANTED_G = (0.0, 1e-20, 1e4)

    @staticmethod
    def inputs(dtype, n, step, p_zero, seed=0, device="cpu"):
        """The state before step `step`: p fp32 (zeros, or randn), m and v zeros before step 1, else randn * 0.1 and rand * 0.01, g
        randn in `dtype` with PLANTED_G over its leading elements (as many as fit, starting at value number `step`)."""
        gen = torch.Generator(device=device).manual_seed(seed)
        r = lambda: torch.randn(n, generator=gen, device=device)
        p, m, v, g = r(), r() * 0.1, torch.rand(n, generator=gen, device=device) * 0.01, r()
        if p_zero:
            p.zero_()
        if step == 1:
            m.zero_(), v.zero_()
        k = min(n, 3)
        g[:k] = torch.tensor([AdamWRef.PLANTED_G[(j + step) % 3] for j in range(k)], device=device)
        return p, m, v, g.to(dtype)

    def __init__(self, p, m, v, g, lr, b1, b2, eps, wd, step, grad_scale=1.0, store_bf16=False, decay_after=False, bc_step=None,
                 no_bc2=False, no_grad_scale=False, eps_inside=False, bc=None):
        import math
        f = AdamWRef.f32
        lr, b1, b2, eps, wd, gsc = f(lr), f(b1), f(b2), f(eps), f(wd), f(grad_scale)
        d = lambda t: t.detach().double().reshape(-1)
        P, M, V, G = d(p), d(m), d(v), d(g)
        st = step if bc_step is None else bc_step
        bc1, bc2s = (1 - b1 ** st, math.sqrt(1 - b2 ** st)) if bc is None else bc
        if no_bc2:
            bc2s = 1.0
        gs = G if no_grad_scale else G * gsc
        t1, t2 = b1 * M, (1 - b1) * gs
        mn, mag_m = t1 + t2, t1.abs() + t2.abs()
        vn = b2 * V + (1 - b2) * gs * gs
        den = torch.sqrt(vn + eps) / bc2s if eps_inside else torch.sqrt(vn) / bc2s + eps
        upd, U = (lr / bc1) * mn / den, (lr / bc1) * mag_m / den
        want = (P - upd) * (1 - lr * wd) if decay_after else P * (1 - lr * wd) - upd
        r = 2.0 ** -24
        self.want = dict(m=mn, v=vn, p=want)
        self._bound = dict(m=4 * r * mag_m + TINY, v=6 * r * vn + TINY,
                           p=4 * r * P.abs() + 16 * r * U + U * math.sqrt(TINY) / (bc2s * den) + (2.0 ** -8 * want.abs() if store_bf16 else 0.0))

    def bound(self, name):
        return self._bound[name]

    def outside(self, other, name):
        return (other.want[name] - self.want[name]).abs() > self.bound(name)

    def err(self, got, name):
        return (got.detach().reshape(-1).double() - self.want[name]).abs()


# ------------------------------------------------------------------------------------------ tiny model builders
def tiny_opt_config(pre_ln=True, proj=None, dropout=0.1):
    from transformers import OPTConfig
    return OPTConfig(vocab_size=128, hidden_size=64, num_attention_heads=4, ffn_dim=128, num_hidden_layers=4,
                     max_position_embeddings=64, word_embed_proj_dim=proj or 64, do_layer_norm_before=pre_ln,
                     dropout=dropout, attention_dropout=0.0, pad_token_id=1, bos_token_id=2, eos_token_id=2, init_std=0.08)


def tiny_roberta_config():
    from transformers import RobertaConfig
    return RobertaConfig(vocab_size=128, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                         max_position_embeddings=40, pad_token_id=1, type_vocab_size=1, hidden_dropout_prob=0.0,
                         attention_probs_dropout_prob=0.0)


def tiny_clip_vision_config():
    from transformers import CLIPVisionConfig
    return CLIPVisionConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2, image_size=32,
                            patch_size=16)


def mpt_args(**kw):
    from types import SimpleNamespace
    a = dict(context="all", neighbor_mode="cross_attention", n_text_tokens=2, n_visual_tokens=2, text_model="roberta-tiny",
             visual_model="clip-vit-tiny", max_output_length=8, freeze_lm=False, model_name_or_path="opt-tiny",
             peft_type="flamingo", lora_r=4, lora_alpha=1.0, lora_dropout=0.0, neighbor_layer_wise=2, decoder_only=True,
             position_type="none", max_text_neighbors=3, max_image_neighbors=2)
    a.update(kw)
    return SimpleNamespace(**a)


def load_exact(module, state, prefix=""):
    """load_state_dict(strict) from a fixture group, ignoring fixture keys outside `prefix`."""
    sd = {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}
    missing, unexpected = module.load_state_dict(sd, strict=False)
    missing = [k for k in missing if "position_ids" not in k]
    assert not missing, f"missing keys: {missing[:5]}"
    assert not [k for k in unexpected if "position_ids" not in k], f"unexpected keys: {unexpected[:5]}"
