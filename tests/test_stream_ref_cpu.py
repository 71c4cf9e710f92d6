"""CPU: the comparisons of tests/test_llama_ops_bounds_gpu.py and tests/test_stream_bounds_gpu.py can fail, and do not fail an honest
kernel.  From stream_ref.RopeRef, SwigluRef, ActRef and AdamWRef alone (fp64, no kernel), at the small cases of the GPU files, their
inputs and their seed:

  * the same operations in torch's fp32 arithmetic, in the kernels' operation order (the exponential as an exact 2^x of the argument
    product rounded to fp32, overflowing to inf as v_exp_f32 does), stored in the operand dtype, leave no element outside any bound;
  * a deliberately wrong reference of each defect the kernels could have puts at least one element outside the bound of the right
    one in every case it applies to (the share is printed): RoPE -- the pair partner one vector off, the position one off, the
    backward sign not flipped, the v block rotated, the table offset of the thread's chunk ignored; SwiGLU -- gate and up swapped,
    silu' without g (1 - s), up read at row pitch F; AdamW -- decay after the update, the bias corrections of step - 1, sqrt(bc2)
    dropped, grad_scale ignored, eps inside the square root, the host's fp32 powf bias corrections at (0.999, step 2) with p = 0;
    activation in fp32 -- tanh-GELU for erf-GELU, quick-GELU's slope 1.7 for 1.702."""
import itertools

import numpy as np
import pytest
import torch

from bounds import BF16, F32, NAME, VEC, check_bound
from gemm_ref import GemmRef
from stream_ref import ActRef, AdamWRef, RopeRef, SwigluRef

SEED = 0
LOG2E = np.float32(1.4426950408889634)
ROPE_LAYOUTS = [(2, 3), (5, 6)]                         # (nblk, nall): multi-head / G = 1, and grouped-query with G = 4
ADAM = dict(lr=1e-2, eps=1e-8)


def _outside(mask, what, applies=True):
    frac = mask.double().mean().item()
    print(f"[can fail] {what}: {frac:.1%} of the elements leave the bound")
    assert not applies or mask.any(), f"{what}: no element leaves the bound"
    return frac


def _exp32(arg):
    """exp of an fp32 tensor the way the kernels' __expf forms it: the argument times log2(e) rounded to fp32, then 2^x (here exactly,
    rounded once), inf past 2^128."""
    return torch.exp2((arg * float(LOG2E)).double()).float()


# ------------------------------------------------------------------------------------------ RoPE
def _rope32(x, cs, T, unit, D, nblk, nall, backward):
    rows, half = x.shape[0], D // 2
    X = x.float()[:, :nall * unit * D].reshape(rows, nall * unit, 2, half).clone()
    x0, x1 = X[:, :nblk * unit, 0].clone(), X[:, :nblk * unit, 1].clone()
    t = torch.arange(rows) % T
    c, s = cs[t][:, None, :, 0], cs[t][:, None, :, 1] * (-1.0 if backward else 1.0)
    X[:, :nblk * unit, 0] = x0 * c - x1 * s
    X[:, :nblk * unit, 1] = x1 * c + x0 * s
    return X.reshape(rows, -1).to(x.dtype)


@pytest.mark.parametrize("layout", ROPE_LAYOUTS, ids=lambda l: f"{l[0]}of{l[1]}")
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("dk", [2, 4, 0], ids=["D2vn", "D4vn", "D128"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_rope(dtype, dk, H, layout):
    vn = VEC[dtype]
    D, (nblk, nall), T, B = dk * vn or 128, layout, 7, 3
    rows, ld = B * T, nall * H * D
    x, cs = RopeRef.inputs(dtype, rows, ld, seed=SEED), RopeRef.table(T, D)
    what = f"{NAME[dtype]} D={D} H={H} {nblk}of{nall}"
    for backward in (False, True):
        ref = RopeRef(x, cs, T, H, D, nblk, nall, backward=backward)
        assert ref.check(_rope32(x, cs, T, H, D, nblk, nall, backward), f"torch fp32 {what} {'bwd' if backward else 'fwd'}", "cpu") <= 1.0
        w = lambda **kw: RopeRef(x, cs, T, H, D, kw.pop("nblk", nblk), nall, backward=kw.pop("backward", backward), **kw)
        _outside(ref.outside(w(partner_shift=1)), f"{what}: pair partner one vector off", applies=D > 2 * vn)
        _outside(ref.outside(w(t_shift=1)), f"{what}: position one off")
        _outside(ref.outside(w(backward=not backward)), f"{what}: backward sign not flipped")
        out = ref.outside(w(nblk=nall))
        _outside(out, f"{what}: v block rotated")
        assert not out[:, ref.rotated].any() and out[:, ~ref.rotated].any()
        _outside(ref.outside(w(flat_table=True)), f"{what}: table offset of the chunk ignored", applies=D > 2 * vn)
    one = RopeRef(x[:B], RopeRef.table(1, D), 1, H, D, nblk, nall)                 # T = 1: the angle 0
    assert torch.equal(one.want, x[:B].double()) and not one.bound().lt(0).any()


# ------------------------------------------------------------------------------------------ SwiGLU
def _swiglu32(gu, dy):
    F = gu.shape[1] // 2
    g, u, d = gu.float()[:, :F], gu.float()[:, F:], dy.float()
    s = 1.0 / (1.0 + _exp32(-g))
    return (g * s * u).to(gu.dtype), (d * u * s * (1.0 + g * (1.0 - s))).to(gu.dtype), (d * g * s).to(gu.dtype)


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("fk", [1, 3, 13])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_swiglu(dtype, fk, M):
    F = fk * VEC[dtype]
    gu, dy = SwigluRef.inputs(dtype, M, F, seed=SEED)
    assert torch.isfinite(gu.float()).all() and torch.isfinite(dy.float()).all()
    ref = SwigluRef(gu, dy)
    y, dg, du = _swiglu32(gu, dy)
    what = f"{NAME[dtype]} {M}x{F}"
    for name, v in dict(y=y, dg=dg, du=du).items():
        assert ref.check(v, name, f"torch fp32 {what}", "cpu") <= 1.0
    wrong = SwigluRef(gu, dy, swap=True)
    for name in ("y", "dg", "du"):
        _outside(ref.outside(wrong, name), f"{what}: gate and up swapped ({name})")
    out = ref.outside(SwigluRef(gu, dy, no_gterm=True), "dg")
    _outside(out, f"{what}: silu' without g (1 - s) (dg)")
    assert not ref.outside(SwigluRef(gu, dy, no_gterm=True), "du").any()
    wrong = SwigluRef(gu, dy, up_pitch_f=True)
    for name in ("y", "dg"):
        out = ref.outside(wrong, name)
        _outside(out, f"{what}: up read at row pitch F ({name})", applies=M > 1)
        assert not out[0].any()                                                   # row 0 is at the same place under both pitches


def test_swiglu_planted_values_and_the_terms_that_carry_them():
    """Every planted value is reached by the small cases between them; without the cancellation term torch's fp32 arithmetic leaves
    the dg bound for g in [6, 20], without the floor y and du leave theirs for g < -87 (the two terms are needed, not decoration)."""
    seen = set()
    for dtype, fk, M in itertools.product((F32,), (1, 3, 13), (1, 5)):
        gu, dy = SwigluRef.inputs(dtype, M, fk * 4, seed=SEED)
        seen |= {float(np.float32(v)) for v in SwigluRef.PLANTED_G if (gu[:, :fk * 4] == v).any()}
        if M * fk * 4 >= 68:
            assert (gu[:, fk * 4:] == 0).sum() >= 2 and (dy == 0).sum() >= 2
            assert (gu[:, :fk * 4].view(torch.int32) == -2 ** 31).any(), "-0 is planted"
    assert seen == {float(np.float32(v)) for v in SwigluRef.PLANTED_G}
    g = torch.cat([torch.linspace(6, 20, 4001), torch.linspace(-104, -87.5, 4001)])
    gu = torch.stack([g, torch.full_like(g, 3.0)], 1)                             # F = 1: [g | u = 3]
    dy = torch.full((g.numel(), 1), 2.0)
    ref = SwigluRef(gu, dy)
    y, dg, du = _swiglu32(gu, dy)
    assert not (ref.err(y, "y") > ref.bound("y")).any() and not (ref.err(dg, "dg") > ref.bound("dg")).any()
    G, s1 = g.double()[:, None], torch.sigmoid(-g.double())[:, None]
    without_cancel = ref.bound("dg") - 2 * 2.0 ** -24 * G.abs() * 6.0 * torch.sigmoid(G)
    assert (ref.err(dg, "dg") > without_cancel)[:4001].any(), "the cancellation term is not needed on [6, 20]"
    without_floor = (2.0 ** -23 + 4 * 2.0 ** -24 + s1 * (2.0 ** -22 + G.abs() * 2.0 ** -23)) * ref.want["y"].abs()
    assert (ref.err(y, "y") > without_floor)[4001:].any(), "the floor is not needed below -87"


# ------------------------------------------------------------------------------------------ activation
def _act32(x, act):
    a = x.float()
    if act == 1:
        y = torch.relu(a)
    elif act == 2:
        y = 0.5 * a * (1.0 + torch.erf(a * float(np.float32(0.70710678118654752440))))
    elif act == 3:
        y = a / (1.0 + _exp32(float(np.float32(-1.702)) * a))
    else:
        y = 0.5 * a * (1.0 + torch.tanh(float(np.float32(0.79788456080286535588)) * (a + float(np.float32(0.044715)) * a * a * a)))
    return y.to(x.dtype)


@pytest.mark.parametrize("act", [1, 2, 3, 4], ids=["relu", "gelu", "quick_gelu", "gelu_tanh"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_activation(dtype, act):
    vn = VEC[dtype]
    for n in (1, vn - 1, vn, vn + 1, 65 * vn + 3):
        x = ActRef.inputs(dtype, n, seed=SEED)
        ref = ActRef(x, act)
        got = _act32(x, act)
        assert torch.isfinite(got.float()).all()
        assert ref.check(got, f"torch fp32 {NAME[dtype]} act{act} n={n}", "cpu") <= 1.0
    if dtype == F32 and act == 2:
        _outside(ref.outside(ActRef(x, 2, fn=GemmRef.ACT[4])), "f32: tanh-GELU in place of erf-GELU")
    if dtype == F32 and act == 3:
        _outside(ref.outside(ActRef(x, 3, fn=lambda t: t * torch.sigmoid(1.7 * t))), "f32: quick-GELU slope 1.7 in place of 1.702")


# ------------------------------------------------------------------------------------------ AdamW
def _adamw32(p, m, v, g, lr, b1, b2, eps, wd, step, gsc, bc=None):
    """adamw_kernel's operation order in torch fp32; bc1 and bc2s correctly rounded from the exact function of the float betas
    (what the bound counts) unless `bc` gives them."""
    f = lambda x: float(np.float32(x))
    lr, b1, b2, eps, wd, gsc = (f(x) for x in (lr, b1, b2, eps, wd, gsc))
    bc1, bc2s = (f(1 - b1 ** step), f((1 - b2 ** step) ** 0.5)) if bc is None else bc
    one = np.float32(1)
    gs = g.float() * gsc
    p = p.float() * float(one - np.float32(lr) * np.float32(wd))
    mi = b1 * m + float(one - np.float32(b1)) * gs
    vi = b2 * v + float(one - np.float32(b2)) * gs * gs
    p = p - float(np.float32(lr) / np.float32(bc1)) * mi / (torch.sqrt(vi) / bc2s + eps)
    return p, mi, vi


ADAM_HYPER = [(b, s, wd, gs) for b in ((0.9, 0.95), (0.9, 0.999)) for s in (1, 2, 3, 1000) for wd in (0.0, 0.01) for gs in (1.0, 0.125, 1 / 3)]


@pytest.mark.parametrize("layout", ["f32", "master", "bf16"])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_adamw(n, layout):
    gdt = F32 if layout == "f32" else BF16
    shares = {}
    for (b1, b2), step, wd, gsc in ADAM_HYPER:
        for p_zero in (True, False):
            p, m, v, g = AdamWRef.inputs(gdt, n, step, p_zero, seed=SEED)
            if layout == "bf16":
                p = p.to(BF16).float()                                            # the state handed in is the bf16 parameter
            kw = dict(lr=ADAM["lr"], b1=b1, b2=b2, eps=ADAM["eps"], wd=wd, step=step, grad_scale=gsc, store_bf16=layout == "bf16")
            ref = AdamWRef(p, m, v, g, **kw)
            pn, mn, vn = _adamw32(p, m, v, g, ADAM["lr"], b1, b2, ADAM["eps"], wd, step, gsc)
            if layout == "bf16":
                pn = pn.to(BF16)
            what = f"torch fp32 {layout} n={n} betas=({b1},{b2}) step={step} wd={wd} gs={gsc:.3f} {'p=0' if p_zero else 'p~1'}"
            for name, got in dict(m=mn, v=vn, p=pn).items():
                assert check_bound(ref.err(got, name)[:, None], None, ref.bound(name)[:, None], f"{what} {name}", "cpu") <= 1.0
            if n < 255 or layout == "bf16":                                       # the wrong references: the fp32 layouts at a few hundred elements
                continue
            live = 1 - AdamWRef.f32(b2) ** (step - 1) < 0.999                       # (0.95 at step 1000: both corrections are 1 to 1e-22, nothing to tell apart)
            wrongs = dict(decay_after=(wd > 0, dict(decay_after=True)), bc_step=(step > 1 and live, dict(bc_step=step - 1)), no_bc2=(live, dict(no_bc2=True)),
                          no_grad_scale=(gsc != 1.0, dict(no_grad_scale=True)), eps_inside=(True, dict(eps_inside=True)))
            for name, (applies, knob) in wrongs.items():
                if applies:
                    out = ref.outside(AdamWRef(p, m, v, g, **kw, **knob), "p")
                    assert out.any(), f"{what}: {name} leaves no element outside the bound"
                    shares.setdefault(name, []).append(out.double().mean().item())
            if (b2, step, p_zero) == (0.999, 2, True):
                bc = AdamWRef.bc_fp32(b1, b2, step)
                out = ref.outside(AdamWRef(p, m, v, g, **kw, bc=bc), "p")
                assert out.any(), f"{what}: the fp32 powf bias corrections leave no element outside the bound"
                shares.setdefault("fp32 powf bc at (0.999, 2), p = 0", []).append(out.double().mean().item())
                pn, _, _ = _adamw32(p, m, v, g, ADAM["lr"], b1, b2, ADAM["eps"], wd, step, gsc, bc=bc)
                r = (ref.err(pn, "p") / ref.bound("p").clamp_min(1e-300)).max().item()
                print(f"[can fail] {what}: adamw_kernel's arithmetic with the host's fp32 powf corrections: max err/bound {r:.2f}")
                assert r > 1.0
    for name, s in shares.items():
        print(f"[can fail] adamw {layout} n={n}: {name}: {min(s):.1%} - {max(s):.1%} of p over {len(s)} cases")


def test_adamw_bias_corrections_in_fp32_lose_bits():
    """1.f - powf(beta, step) cancels: at (0.999, step 2) the fp32 form is 6.7e-6 off, the correctly rounded value below 2^-24."""
    exact = 1 - AdamWRef.f32(0.999) ** 2
    bc1, bc2s = AdamWRef.bc_fp32(0.9, 0.999, 2)
    assert abs(bc2s ** 2 / exact - 1) > 5e-6 and abs(float(np.float32(exact ** 0.5)) / exact ** 0.5 - 1) <= 2.0 ** -24
    assert abs(bc1 / (1 - AdamWRef.f32(0.9) ** 2) - 1) < 4 * 2.0 ** -24
