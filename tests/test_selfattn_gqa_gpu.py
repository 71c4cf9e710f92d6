"""-m gpu: grouped-query causal self-attention (mmgl_selfattn_gqa_fwd / _bwd, ops.selfattn_core / selfattn_core_fused / rope_qk_ with
num_kv_heads < num_heads).  Query head h reads key / value head h // G, G = H / Hkv (transformers' repeat_kv).

Two references.  (a) The multi-head kernels of this library on K / V expanded with repeat_interleave(G): out, lse and dq must be
BITWISE equal (the same arithmetic per head, only addresses differ), dk / dv must be the group's sum within one rounding plus an
fp32 sum of G terms.  (b) The CPU oracle's additive-mask attention (oracle/lm_ref.py) on the expanded K / V, gradients summed over the
group by autograd.  Both comparisons are also run against the WRONG mapping h % Hkv and must fail there."""
import functools

import pytest
import torch

from helpers import assert_close, rel_err

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
# dtype, D, H, Hkv, T  (B = 2 everywhere)
SA32_CASES = [(BF16, D, H, Hkv, T) for D in (64, 128) for (H, Hkv) in ((8, 2), (8, 1), (6, 3)) for T in (64, 130, 200)]
GENERIC_CASES = [(dt, D, H, Hkv, 70) for (dt, D) in ((F32, 16), (F32, 32), (BF16, 32)) for (H, Hkv) in ((4, 2), (4, 1))]
CASES = SA32_CASES + GENERIC_CASES
B = 2
ORACLE_TOL = {F32: 1e-3, BF16: 2e-2}           # tests/test_selfattn_gpu.py
U = {F32: 2.0 ** -23, BF16: 2.0 ** -8}         # decode_ref.SkinnyRef


def _id(c):
    return f"{'bf16' if c[0] == BF16 else 'f32'}-D{c[1]}-H{c[2]}-Hkv{c[3]}-T{c[4]}"


def _expand(x, Hkv, G, D, wrong=False):
    """[B,T,Hkv*D] -> [B,T,H*D]: head h = kv head h // G (repeat_kv); wrong = True: head h = kv head h % Hkv."""
    Bx, T = x.shape[:2]
    x4 = x.reshape(Bx, T, Hkv, D)
    x4 = x4.repeat(1, 1, G, 1) if wrong else x4.repeat_interleave(G, dim=2)
    return x4.reshape(Bx, T, Hkv * G * D).contiguous()


def _inputs(dtype, D, H, Hkv, T):
    gen = torch.Generator().manual_seed(1000 * H + 100 * Hkv + T + D)
    q = (torch.randn(B, T, H * D, generator=gen) * (D ** -0.5) * 2).to(dtype).cuda()
    k = torch.randn(B, T, Hkv * D, generator=gen).to(dtype).cuda()
    v = torch.randn(B, T, Hkv * D, generator=gen).to(dtype).cuda()
    w = torch.randn(B, T, H * D, generator=gen).to(dtype).cuda()
    am = torch.ones(B, T, dtype=torch.uint8)
    am[1, T - T // 4:] = 0                           # right-padded; column 0 stays valid
    return q, k, v, w, am.cuda()


def _gqa_raw(q, k, v, w, am, H, Hkv):
    """out, lse, dq, dk, dv of the GQA entry points over separate packed tensors."""
    from mmgl_amd import ops
    from mmgl_amd._lib import ptr
    Bq, T, d = q.shape
    D = d // H
    out, lse = ops._gqa_fwd(q, ptr(q), ptr(k), ptr(v), am, Bq, T, H, Hkv, D, 0, 0)
    dq, dk, dv = torch.full_like(q, float("nan")), torch.full_like(k, float("nan")), torch.full_like(v, float("nan"))
    ops._gqa_bwd(q, w, ptr(q), ptr(k), ptr(v), out, lse, am, ptr(dq), ptr(dk), ptr(dv), Bq, T, H, Hkv, D, 0, 0, 0, 0)
    return out, lse, dq, dk, dv


def _mha_raw(q, k, v, w, am, H):
    """out, lse, dq, dk, dv of mmgl_selfattn_fwd / _bwd (k, v [B,T,H*D])."""
    from mmgl_amd import ops
    from mmgl_amd._lib import ptr
    Bq, T, d = q.shape
    out, lse = ops._selfattn_fwd(q, ptr(q), ptr(k), ptr(v), am, Bq, T, d, H, None, 0)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ops._selfattn_bwd(q, w, ptr(q), ptr(k), ptr(v), out, lse, am, ptr(dq), ptr(dk), ptr(dv), Bq, T, d, H, None, 0, 0)
    return out, lse, dq, dk, dv


def _oracle(q, k, v, w, am, H, Hkv, wrong):
    from oracle import lm_ref
    D, G = q.shape[2] // H, H // Hkv
    q, k, v = (t.detach().float().cpu().requires_grad_() for t in (q, k, v))
    mask = lm_ref.decoder_self_mask(am.cpu().long(), torch.float32)
    out = lm_ref.attention_core(q, _expand(k, Hkv, G, D, wrong), _expand(v, Hkv, G, D, wrong), mask, H)
    (out * w.float().cpu()).sum().backward()          # autograd sums the group's gradients into k.grad / v.grad
    return out.detach(), q.grad, k.grad, v.grad


@functools.lru_cache(maxsize=None)
def _run(case):
    """Everything the tests of one case compare, computed once and left unchanged."""
    dtype, D, H, Hkv, T = case
    G = H // Hkv
    q, k, v, w, am = _inputs(*case)
    r = dict(inputs=(q, k, v, w, am), gqa=_gqa_raw(q, k, v, w, am, H, Hkv),
             mha=_mha_raw(q, _expand(k, Hkv, G, D), _expand(v, Hkv, G, D), w, am, H),
             oracle=_oracle(q, k, v, w, am, H, Hkv, False))
    if Hkv > 1:                                        # (Hkv = 1: both mappings are the same)
        r["mha_wrong_out"] = _mha_raw(q, _expand(k, Hkv, G, D, True), _expand(v, Hkv, G, D, True), w, am, H)[0]
        r["oracle_wrong"] = _oracle(q, k, v, w, am, H, Hkv, True)
    torch.cuda.synchronize()
    return r


def _group_bound(x, Hkv, G, D, dtype, wrong=False):
    """x: the multi-head route's per-head gradient [B,T,H*D].  Returns (S, bound): the fp64 sum over each group and
    u |S| + G 2^-23 sum_g |x_g| -- one rounding of the result plus an fp32 sum of G terms."""
    Bx, T = x.shape[:2]
    x = x.double()
    x5 = x.reshape(Bx, T, G, Hkv, D).transpose(2, 3) if wrong else x.reshape(Bx, T, Hkv, G, D)
    S, A = x5.sum(3), x5.abs().sum(3)
    return S.reshape(Bx, T, Hkv * D), (U[dtype] * S.abs() + G * 2.0 ** -23 * A).reshape(Bx, T, Hkv * D)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gqa_equals_multihead_on_expanded_kv(case):
    dtype, D, H, Hkv, T = case
    G = H // Hkv
    r = _run(case)
    out, lse, dq, dk, dv = r["gqa"]
    mo, ml, mq, mk, mv = r["mha"]
    for t in (out, lse, dq, dk, dv):
        assert torch.isfinite(t).all()
    assert torch.equal(out, mo), "out"
    assert torch.equal(lse, ml), "lse"
    assert torch.equal(dq, mq), "dq"
    for name, got, x in (("dk", dk, mk), ("dv", dv, mv)):
        S, bound = _group_bound(x, Hkv, G, D, dtype)
        err = (got.double() - S).abs()
        print(f"[gqa {_id(case)}] {name}: max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
        bad = int((err > bound).sum())
        assert bad == 0, f"{name}: {bad} of {err.numel()} elements outside u|S| + G 2^-23 sum|x_g|"
    # padded keys get exactly zero gradient, as in the multi-head kernels
    pad = ~r["inputs"][4].bool()
    assert (dk[pad] == 0).all() and (dv[pad] == 0).all()
    if Hkv > 1:                                        # the comparison can fail: the mapping h % Hkv is not this one
        assert not torch.equal(out, r["mha_wrong_out"])
        for name, got, x in (("dk", dk, mk), ("dv", dv, mv)):
            S, bound = _group_bound(x, Hkv, G, D, dtype, wrong=True)
            frac = ((got.double() - S).abs() > bound).double().mean().item()
            assert frac > 0.25, f"{name}: regrouping the heads as h % Hkv leaves {1 - frac:.0%} of the elements inside the bound"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gqa_vs_oracle_on_expanded_kv(case):
    dtype, D, H, Hkv, T = case
    r = _run(case)
    out, _, dq, dk, dv = r["gqa"]
    tol = ORACLE_TOL[dtype]
    for name, got, want in zip(("out", "dq", "dk", "dv"), (out, dq, dk, dv), r["oracle"]):
        print(f"[gqa {_id(case)}] {name} vs oracle: rel err {rel_err(got.float(), want):.3e} (tol {tol:.0e})")
    for name, got, want in zip(("out", "dq", "dk", "dv"), (out, dq, dk, dv), r["oracle"]):
        assert_close(got.float(), want, tol, name)
    if Hkv > 1:                                        # the same check against the mapping h % Hkv must fail
        for name, got, want in zip(("out", "dq", "dk", "dv"), (out, dq, dk, dv), r["oracle_wrong"]):
            e = rel_err(got.float(), want)
            assert e > tol, f"{name}: the wrong head mapping passes too (rel err {e:.3e})"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gqa_fused_layout_is_bitwise_the_separate_call(case):
    """q | k | v as column slices of ONE [B, T, ld] buffer with 16 padding columns, gradients into one NaN-filled buffer of the same
    layout: the payload is written (finite), the padding is not touched, and every value equals the separate-tensor call's."""
    from mmgl_amd import ops
    from mmgl_amd._lib import ptr, ptr_off
    dtype, D, H, Hkv, T = case
    r = _run(case)
    q, k, v, w, am = r["inputs"]
    n = (H + 2 * Hkv) * D
    ld = n + 16
    es = q.element_size()
    buf = torch.zeros(B, T, ld, dtype=dtype, device="cuda")
    buf[..., :n] = torch.cat([q, k, v], -1)
    grad = torch.full_like(buf, float("nan"))
    ko, vo = H * D * es, (H + Hkv) * D * es
    out, lse = ops._gqa_fwd(buf, ptr(buf), ptr_off(buf, ko), ptr_off(buf, vo), am, B, T, H, Hkv, D, ld, ld)
    ops._gqa_bwd(buf, w, ptr(buf), ptr_off(buf, ko), ptr_off(buf, vo), out, lse, am, ptr(grad), ptr_off(grad, ko), ptr_off(grad, vo),
                 B, T, H, Hkv, D, ld, ld, ld, ld)
    so, sl, sq, sk, sv = r["gqa"]
    assert torch.isfinite(grad[..., :n]).all(), "a payload column was not written"
    assert torch.isnan(grad[..., n:]).all(), "a padding column was written"
    assert torch.equal(out, so) and torch.equal(lse, sl)
    assert torch.equal(grad[..., :n], torch.cat([sq, sk, sv], -1))
    # the autograd ops over the unpadded fused buffer and over separate tensors: the same values again
    qkv = torch.cat([q, k, v], -1).requires_grad_()
    of = ops.selfattn_core_fused(qkv, am, H, Hkv)
    (gf,) = torch.autograd.grad((of * w).sum(), qkv)
    q2, k2, v2 = (t.clone().requires_grad_() for t in (q, k, v))
    os_ = ops.selfattn_core(q2, k2, v2, am, H, Hkv)
    gs = torch.autograd.grad((os_ * w).sum(), (q2, k2, v2))
    assert torch.equal(of, so) and torch.equal(os_, so)
    assert torch.equal(gf, torch.cat([sq, sk, sv], -1)) and torch.equal(torch.cat(gs, -1), gf)


@pytest.mark.parametrize("dtype,D,H,T", [(BF16, 64, 4, 130), (BF16, 128, 2, 200), (F32, 16, 4, 70), (F32, 32, 4, 70), (BF16, 32, 4, 70)])
def test_gqa_entry_points_with_all_heads_are_the_multihead_ones(dtype, D, H, T):
    """Hkv == H through mmgl_selfattn_gqa_* is mmgl_selfattn_fwd / _bwd: bitwise, and through the ops the multi-head code path."""
    from mmgl_amd import ops
    q, k, v, w, am = _inputs(dtype, D, H, H, T)
    for a, b in zip(_gqa_raw(q, k, v, w, am, H, H), _mha_raw(q, k, v, w, am, H)):
        assert torch.equal(a, b)
    assert torch.equal(ops.selfattn_core(q, k, v, am, H, H), ops.selfattn_core(q, k, v, am, H))
    qkv = torch.cat([q, k, v], -1)
    assert torch.equal(ops.selfattn_core_fused(qkv, am, H, H), ops.selfattn_core_fused(qkv, am, H))


def _rot_half(x):
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], -1)


def _rot_half_t(x):                                    # the transpose of rotate_half
    h = x.shape[-1] // 2
    return torch.cat([x[..., h:], -x[..., :h]], -1)


@pytest.mark.parametrize("dtype,tol", [(F32, 1e-5), (BF16, 2e-2)])          # tests/test_llama_gpu.py
@pytest.mark.parametrize("Bx,T,H,Hkv,D", [(2, 24, 4, 2, 16), (1, 70, 8, 1, 64), (1, 130, 6, 3, 128), (2, 33, 8, 2, 32)])
def test_rope_qk_grouped_matches_rotate_half(Bx, T, H, Hkv, D, dtype, tol):
    """rope_qk_ on a [q: H heads | k: Hkv heads | v: Hkv heads] buffer against the fp64 definition x cos + rotate_half(x) sin on
    every q and k head; v bitwise untouched; the gradient is the transpose rotation (and passes v's through bitwise)."""
    from mmgl_amd import ops
    g = torch.Generator().manual_seed(T + H)
    n, nq, nk = (H + 2 * Hkv) * D, H * D, Hkv * D
    x = torch.randn(Bx, T, n, generator=g).to(dtype).cuda().requires_grad_()
    w = torch.randn(Bx, T, n, generator=g).to(dtype).cuda()
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).double() / D))
    ang = torch.arange(T).double()[:, None] * inv[None]
    cos_sin = torch.stack([ang.cos(), ang.sin()], -1).float()
    y = ops.rope_qk_(x * 1.0, cos_sin.cuda(), H, Hkv)       # (x * 1.0: a fresh buffer, as the GEMM output is)
    (gx,) = torch.autograd.grad(y, x, w)
    cs = cos_sin.double()                                   # the table the kernel reads, in fp64
    cos = torch.cat([cs[..., 0], cs[..., 0]], -1)[None, :, None, :]
    sin = torch.cat([cs[..., 1], cs[..., 1]], -1)[None, :, None, :]
    xd, wd = x.detach().double().cpu(), w.double().cpu()
    rot = xd[..., :nq + nk].reshape(Bx, T, H + Hkv, D)
    want = torch.cat([(rot * cos + _rot_half(rot) * sin).reshape(Bx, T, nq + nk), xd[..., nq + nk:]], -1)
    gr = wd[..., :nq + nk].reshape(Bx, T, H + Hkv, D)
    gwant = torch.cat([(gr * cos + _rot_half_t(gr * sin)).reshape(Bx, T, nq + nk), wd[..., nq + nk:]], -1)
    for name, lo, hi in (("q", 0, nq), ("k", nq, nq + nk)):
        assert_close(y[..., lo:hi].float(), want[..., lo:hi], tol, f"rope fwd {name}")
        assert_close(gx[..., lo:hi].float(), gwant[..., lo:hi], tol, f"rope bwd {name}")
    assert torch.equal(y[..., nq + nk:], x.detach()[..., nq + nk:]), "v was touched"
    assert torch.equal(gx[..., nq + nk:], w[..., nq + nk:]), "v's gradient was touched"
    # per head, so that one unrotated (or doubly rotated) head cannot hide behind the tensor's maximum
    e = ((y.detach().double().cpu() - want)[..., :nq + nk].reshape(Bx, T, H + Hkv, D).abs().amax(dim=(0, 1, 3))
         / want[..., :nq + nk].reshape(Bx, T, H + Hkv, D).abs().amax(dim=(0, 1, 3)))
    assert (e <= tol).all(), e
