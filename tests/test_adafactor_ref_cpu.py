"""No GPU: what tests/test_adafactor_bounds_gpu.py stands on.  From adafactor_ref.AdafactorRef alone:
  * the fp64 formula is transformers' Adafactor (beta1 None, no relative step, no parameter scaling) run on float64 parameters, steps 1-3
    chained on the shared shapes (the all-zero gradients among them), to 1e-12 relative, with and without weight decay and grad_scale;
  * each deliberately wrong reference leaves the bound on at least a quarter of the elements it reaches, on inputs planted so that it
    does (no_clip: rms(u) > 1; clip_always: rms(u) < 1; no_eps1: a zero gradient), and a second correct reference leaves it nowhere;
  * the kernel's arithmetic restated in torch (adafactor_ref.emulate_fp32: fp32 elementwise, every sum and moving average in double,
    rounded to fp32 where the kernel stores a float) stays inside the bound everywhere."""
import pytest
import torch
from transformers.optimization import Adafactor

from adafactor_ref import SHAPES, WRONG, ZERO_GRAD, AdafactorRef, emulate_fp32, f32, inputs
from bounds import BF16, F32, NAME, check_bound

LR = 2.0 ** -7                   # exact in fp32, as the ABI passes it


def _state_names(shape):
    return ("row", "col") if len(shape) == 2 else ("v",)


@pytest.mark.parametrize("wd, gs", [(0.0, 1.0), (2.0 ** -6, 0.5)], ids=["plain", "wd-gs"])
def test_reference_is_transformers_adafactor_in_fp64(wd, gs):
    cases = inputs(F32, 1, seed=1)
    params = [torch.nn.Parameter(c["p"].double()) for c in cases]
    # eps1 as the float32 the ABI passes and torch's fp32 arithmetic uses (1e-30 is no fp32 number: 3.2e-9 off)
    opt = Adafactor(params, scale_parameter=False, relative_step=False, warmup_init=False, lr=LR, weight_decay=wd, eps=(f32(1e-30), 1e-3))
    state = [tuple(s.double() for s in c["state"]) for c in cases]
    worst = 0.0
    for step in (1, 2, 3):
        grads = [c["g"] for c in inputs(F32, step, seed=10 + step)]
        refs = [AdafactorRef(p.detach(), g, st, LR, step, gs, wd) for p, g, st in zip(params, grads, state)]
        before = [p.detach().clone() for p in params]
        for p, g in zip(params, grads):
            p.grad = g.double() * f32(gs)
        opt.step()
        for i, (p, ref) in enumerate(zip(params, refs)):
            st = opt.state[p]
            got = dict(p=p.detach(), row=st.get("exp_avg_sq_row"), col=st.get("exp_avg_sq_col"), v=st.get("exp_avg_sq"))
            for name in ("p",) + _state_names(SHAPES[i]):
                # relative to the result; for p to |p| + |update|, the terms of the subtraction (an element may cancel to nearly zero)
                scale = ref.want[name].abs() if name != "p" else before[i].abs() + (before[i] - ref.want[name]).abs()
                rel = ((got[name] - ref.want[name]).abs() / scale.clamp_min(1e-300)).max().item()
                worst = max(worst, rel)
                assert rel <= 1e-12, f"step {step} tensor {SHAPES[i]} {name}: {rel:.3e}"
                assert torch.isfinite(ref.want[name]).all()
            if i in ZERO_GRAD and wd == 0.0:
                assert torch.equal(ref.want["p"], before[i]), "a zero gradient moved the parameter"
        state = [tuple(opt.state[p][k].clone() for k in (("exp_avg_sq_row", "exp_avg_sq_col") if p.dim() == 2 else ("exp_avg_sq",))) for p in params]
    print(f"[adafactor ref] fp64 reference against transformers' Adafactor, steps 1-3: largest relative difference {worst:.3e}")


# wrong reference -> (shape, step, state_scale, grad_scale, zero gradient, outputs it reaches)
PLANTS = {
    "no_eps1": [((24, 24), 1, 1.0, 1.0, True, ("row", "col")), ((40,), 1, 1.0, 1.0, True, ("v",))],
    "mean_as_sum": [((24, 24), 2, 1.0, 1.0, False, ("row", "col", "p"))],
    "row_col_swapped": [((24, 24), 2, 1.0, 1.0, False, ("row", "col", "p"))],
    "no_clip": [((24, 24), 1000, 0.01, 1.0, False, ("p",)), ((40,), 1000, 0.01, 1.0, False, ("p",))],
    "clip_always": [((24, 24), 1000, 4.0, 1.0, False, ("p",)), ((40,), 1000, 4.0, 1.0, False, ("p",))],
    "beta_of_other_step": [((24, 24), 2, 1.0, 1.0, False, ("row", "col", "p")), ((40,), 2, 1.0, 1.0, False, ("v", "p"))],
    "no_grad_scale": [((24, 24), 2, 1.0, 0.5, False, ("row", "col", "p")), ((40,), 2, 1.0, 0.5, False, ("v", "p"))],
    "row_mean_dropped": [((24, 24), 1000, 4.0, 1.0, False, ("p",))],
}


@pytest.mark.parametrize("wrong", WRONG)
def test_every_wrong_reference_leaves_the_bound(wrong):
    assert set(PLANTS) == set(WRONG)
    for shape, step, scale, gs, zero, names in PLANTS[wrong]:
        (c,) = inputs(F32, step, seed=2, state_scale=scale, shapes=[shape])
        g = torch.zeros_like(c["g"]) if zero else c["g"]
        ref = AdafactorRef(c["p"], g, c["state"], LR, step, gs)
        again = AdafactorRef(c["p"], g, c["state"], LR, step, gs)
        other = AdafactorRef(c["p"], g, c["state"], LR, step, gs, wrong=wrong)
        if wrong == "no_clip":
            assert ref.rms > 1.5, ref.rms
        if wrong == "clip_always":
            assert ref.rms < 0.75, ref.rms
        for name in names:
            share = ref.outside(other, name).double().mean().item()
            print(f"[can fail] adafactor {wrong} {shape} {name}: {share:.1%} of the elements outside the bound")
            assert share >= 0.25, f"{wrong} {shape} {name}: only {share:.1%} outside"
            assert not ref.outside(again, name).any()


@pytest.mark.parametrize("gdt", [F32, BF16], ids=NAME.get)
def test_fp32_arithmetic_in_the_kernels_order_stays_inside(gdt):
    for steps, scale, wd, gs in (((1, 2, 3), 1.0, 0.0, 1.0), ((1000,), 0.01, 0.01, 0.5), ((1000,), 4.0, 0.0, 1.0)):
        cases = inputs(gdt, steps[0], seed=3, state_scale=scale)
        for step in steps:
            grads = cases if step == steps[0] else inputs(gdt, step, seed=3 + step)
            for i, (c, gc) in enumerate(zip(cases, grads)):
                ref = AdafactorRef(c["p"], gc["g"], c["state"], LR, step, gs, wd)
                got = emulate_fp32(c["p"], gc["g"], c["state"], LR, step, gs, wd)
                for name in ("p",) + _state_names(c["shape"]):
                    check_bound(got[name], ref.want[name], ref.bound(name), f"fp32 emulation step {step} {c['shape']} {name}", f"emulation {NAME[gdt]}")
                c["p"], c["state"] = got["p"], tuple(got[k] for k in _state_names(c["shape"]))
