"""-m gpu: DataParallelEngine(optimizer="adafactor_fused") on the tiny T5 of tests/test_t5_hip_gpu.py under SelfAttentionModel, bf16 and fp32:
two training steps against the stock kind ("adafactor", transformers' optimizer) from the same seed, both measured against an fp64 run
of the same two steps -- the fused arm within twice the stock arm's own distance, per tensor, the rule of the T5 model test --; the step
is one ops.adafactor_step_ call and leaves the flat gradient alone; a checkpoint taken after step 1 reproduces step 2 bit for bit.

The learning rate is the trainer's default (Arguments.learning_rate, 1e-3).  What the rule can resolve depends on it: after step 1 the two
arms differ in the last bit of a few parameters (their reductions run in different orders), and step 2's gradient of a badly
conditioned element -- one that is a small difference of large sums in the fp32 backward -- answers such a bit with a relative change of
1e-5 and more.  That change reaches the parameter multiplied by lr: at lr = 1e-2 it is several fp32 units of a layer-norm weight near 1
and was measured on an MI355X as a ratio of 2.36 on one tensor (fused 5.06e-07, stock 2.14e-07 of the tensor's scale; the other 1-D
tensors 1.00, the 2-D ones 0.71-1.45) in one build of the kernel and below 1.5 everywhere in two earlier builds whose sums were less
accurate -- the backward's conditioning, not the optimizer's arithmetic, which tests/test_adafactor_bounds_gpu.py holds to twice the
stock optimizer's error element by element from identical inputs.  Measured in fp32 with the fused arm's parameters overwritten by the
stock arm's after step 1 (only the optimizers' second steps differ) and without: worst ratio 1.94 / 2.36 at lr = 1e-2, 1.00 / 1.14 at
1e-3, 1.00 / 1.14 at 1e-4.  At the rate a run uses, that amplified bit stays below the two fp32 stores both arms share, while an
optimizer that dropped a factor would still be off by about lr, four orders of magnitude above them."""
import pytest
import torch
from transformers.optimization import Adafactor

from helpers import mpt_args, tiny_clip_vision_config, tiny_roberta_config
from test_t5_hip_gpu import _batch, _cfg, _wrapper

pytestmark = pytest.mark.gpu

LR = 1e-3                                # = run_generation.Arguments().learning_rate (asserted below)


def _step(model, eng, batch):
    ids, labels, mask = batch
    eng.zero_grad()
    model(ids, mask, labels).loss.backward()
    eng.finish_backward()
    eng.step()


def _fp64_two_steps(state):
    from mmgl_amd.model import SelfAttentionModel
    args = mpt_args(neighbor_mode="raw", context="text_only", model_name_or_path="t5-tiny", decoder_only=False, peft_type="none")
    ref = SelfAttentionModel(args, None, lm_config=_cfg(), text_config=tiny_roberta_config(), visual_config=tiny_clip_vision_config()).double().train()
    ref.load_state_dict({k: v.detach().double().cpu() for k, v in state.items()})
    opt = Adafactor([p for p in ref.parameters() if p.requires_grad], scale_parameter=False, relative_step=False, warmup_init=False, lr=LR)
    ids, labels, mask = _batch()
    for _ in range(2):
        opt.zero_grad()
        ref(ids, mask, labels).loss.backward()
        opt.step()
    return {n: p.detach() for n, p in ref.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_two_steps_within_twice_the_stock_kind(dtype, monkeypatch):
    from mmgl_amd import ops
    from mmgl_amd.distributed import DataParallelEngine
    from mmgl_amd.language_modelling.run_generation import Arguments
    assert Arguments().learning_rate == LR
    batch = tuple(t.cuda() for t in _batch())
    arms = {}
    calls = {"n": 0}
    real = ops.adafactor_step_

    def counted(*a, **k):
        calls["n"] += 1
        return real(*a, **k)
    monkeypatch.setattr(ops, "adafactor_step_", counted)
    for kind in ("adafactor_fused", "adafactor"):
        model = _wrapper(dtype)
        if kind == "adafactor_fused":
            want = _fp64_two_steps(model.state_dict())
        eng = DataParallelEngine(model, lr=LR, optimizer=kind, master_weights=False)
        for s in range(2):
            if kind == "adafactor_fused":
                ids, labels, mask = batch
                eng.zero_grad()
                model(ids, mask, labels).loss.backward()
                eng.finish_backward()
                grad, version, n = eng.flat_grad.clone(), eng.flat_grad._version, calls["n"]
                eng.step()
                assert calls["n"] == n + 1, "the step is one ops.adafactor_step_ call"
                assert eng.flat_grad._version == version and torch.equal(eng.flat_grad, grad), "the step wrote the flat gradient"
            else:
                _step(model, eng, batch)
        torch.cuda.synchronize()
        arms[kind] = {n: p.detach().double().cpu() for n, p in model.named_parameters() if p.requires_grad}
        if kind == "adafactor_fused":
            assert not hasattr(eng, "exp_avg") and eng.torch_optimizer is None
    assert calls["n"] == 2 and set(arms["adafactor_fused"]) == set(want)
    failed = []
    for name in sorted(want):
        scale = want[name].abs().max().item()
        e_fused = (arms["adafactor_fused"][name] - want[name]).abs().max().item() / scale
        e_stock = (arms["adafactor"][name] - want[name]).abs().max().item() / scale
        print(f"[adafactor engine {dtype}] {name}: fused {e_fused:.3e} stock {e_stock:.3e} ratio {e_fused / max(e_stock, 1e-300):.2f}")
        assert torch.isfinite(arms["adafactor_fused"][name]).all(), name
        if e_fused > 2.0 * e_stock:
            failed.append(f"{name}: fused {e_fused:.3e} > 2 x stock {e_stock:.3e}")
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_checkpoint_after_step_one_reproduces_step_two(dtype):
    from mmgl_amd.distributed import DataParallelEngine
    batch = tuple(t.cuda() for t in _batch())
    model = _wrapper(dtype)
    eng = DataParallelEngine(model, lr=LR, optimizer="adafactor_fused", master_weights=False)
    _step(model, eng, batch)
    weights = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ckpt = eng.state_dict()
    assert all(st["step"] == 1 for st in ckpt["state"].values()) and len(ckpt["state"]) == len(eng.params)
    _step(model, eng, batch)

    again = _wrapper(dtype, seed=1)                      # other initial weights: everything must come from the checkpoint
    again.load_state_dict(weights)
    eng2 = DataParallelEngine(again, lr=LR, optimizer="adafactor_fused", master_weights=False)
    eng2.load_state_dict(ckpt)
    assert eng2.step_count == 1
    _step(again, eng2, batch)
    torch.cuda.synchronize()
    for (n, a), b in zip(model.named_parameters(), again.parameters()):
        assert torch.equal(a, b), f"{n}: step 2 from the checkpoint differs"
    assert torch.equal(eng.adafactor_state, eng2.adafactor_state)
