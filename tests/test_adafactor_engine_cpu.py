"""No GPU: DataParallelEngine(optimizer="adafactor_fused", fused=False) -- the plain-torch restatement of the fused step -- on the tiny T5
of tests/test_t5_hip_gpu.py: three steps against a stock transformers Adafactor on a copy of the model, the checkpoint layout through a
stock Adafactor and back, the buffers that are not allocated, the refusals, the trainer's flag."""
import copy

import pytest
import torch
from transformers import T5Config
from transformers.optimization import Adafactor

from helpers import mpt_args, tiny_clip_vision_config, tiny_roberta_config

LR = 1e-2


def _model(dtype=torch.float32, seed=0):
    from mmgl_amd.model import SelfAttentionModel
    torch.manual_seed(seed)
    cfg = T5Config(vocab_size=128, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, dropout_rate=0.0,
                   decoder_start_token_id=0, pad_token_id=0)
    args = mpt_args(neighbor_mode="raw", context="text_only", model_name_or_path="t5-tiny", decoder_only=False, peft_type="none")
    m = SelfAttentionModel(args, None, lm_config=cfg, text_config=tiny_roberta_config(), visual_config=tiny_clip_vision_config())
    return m.to(dtype).train()


def _batch():
    g = torch.Generator().manual_seed(3)
    return torch.randint(1, 128, (2, 20), generator=g), torch.ones(2, 20, dtype=torch.long), torch.randint(1, 128, (2, 6), generator=g)


def _engine(model, **kw):
    from mmgl_amd.distributed import DataParallelEngine
    return DataParallelEngine(model, lr=LR, optimizer="adafactor_fused", fused=False, **kw)


def _train(model, stepper, steps):
    ids, mask, labels = _batch()
    for _ in range(steps):
        stepper.zero_grad()
        model(ids, mask, labels).loss.backward()
        if hasattr(stepper, "finish_backward"):
            stepper.finish_backward()
        stepper.step()


def _stock(model):
    return Adafactor(model.parameters(), scale_parameter=False, relative_step=False, warmup_init=False, lr=LR)


def test_three_steps_match_stock_adafactor():
    """Both fp32 arms against an fp64 run of the same three steps.  The tolerance is measured: per tensor the engine's largest distance to
    fp64 is at most twice the stock arm's, or one fp32 store unit of the tensor's scale where the stock arm is closer than that (the rule
    of the GPU tests).  An arm that skipped a step or a factor would be off by about lr = 1e-2."""
    m_engine, m_stock, m_ref = _model(), _model(), _model(torch.float64)
    _train(m_engine, _engine(m_engine), 3)
    _train(m_stock, _stock(m_stock), 3)
    _train(m_ref, _stock(m_ref), 3)
    worst = 0.0
    for (n, a), b, r in zip(m_engine.named_parameters(), m_stock.parameters(), m_ref.parameters()):
        a, b, r = a.detach().double(), b.detach().double(), r.detach()
        e_a, e_b, unit = (a - r).abs().max().item(), (b - r).abs().max().item(), 2.0 ** -23 * r.abs().max().item()
        worst = max(worst, e_a / max(e_b, unit))
        assert e_a <= max(2 * e_b, unit), f"{n}: to fp64: engine {e_a:.3e}, stock {e_b:.3e}"
    print(f"[adafactor engine cpu] largest engine / stock distance to fp64 over the tensors: {worst:.2f}")


def test_state_dict_round_trips_through_stock_adafactor():
    m = _model()
    e = _engine(m)
    assert e.state_dict()["state"] == {}                       # nothing before the first step, as in torch
    _train(m, e, 2)
    sd = e.state_dict()
    names = [n for n, _ in m.named_parameters()]
    assert sd["param_names"] == names and set(sd["state"]) == {i for i, (n, p) in enumerate(m.named_parameters()) if p.requires_grad}
    g = sd["param_groups"][0]
    assert set(g) == {"lr", "eps", "clip_threshold", "decay_rate", "beta1", "weight_decay", "scale_parameter", "relative_step", "warmup_init", "params"}
    assert g["params"] == list(range(len(names))) and g["beta1"] is None and g["weight_decay"] == 0.0 and not g["relative_step"]
    for i, p in enumerate(m.parameters()):
        st = sd["state"][i]
        want = {"step", "RMS"} | ({"exp_avg_sq_row", "exp_avg_sq_col"} if p.dim() == 2 else {"exp_avg_sq"})
        assert set(st) == want and st["step"] == 2
        if p.dim() == 2:
            assert st["exp_avg_sq_row"].shape == p.shape[:1] and st["exp_avg_sq_col"].shape == p.shape[1:]
        else:
            assert st["exp_avg_sq"].shape == p.shape

    # a stock Adafactor over model.parameters() loads it and continues exactly as the engine does
    m2 = copy.deepcopy(m)
    stock = _stock(m2)
    stock.load_state_dict(copy.deepcopy(sd))
    _train(m2, stock, 1)
    sd_stock = stock.state_dict()

    # and back: a fresh engine loads the stock optimizer's state_dict (no param_names: model order) and holds the stock state
    m3 = copy.deepcopy(m2)
    e3 = _engine(m3)
    e3.load_state_dict(sd_stock)
    assert e3.step_count == 3
    back = e3.state_dict()
    for i in sd_stock["state"]:
        for k in ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq"):
            if k in sd_stock["state"][i]:
                assert torch.equal(back["state"][i][k], sd_stock["state"][i][k].float()), (i, k)

    # the engine's own third step from its own checkpoint: the same second moments as the stock optimizer's third step, to fp32 rounding
    _train(m, e, 1)
    mine = e.state_dict()
    for i in sd_stock["state"]:
        for k in ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq"):
            if k in sd_stock["state"][i]:
                torch.testing.assert_close(mine["state"][i][k], sd_stock["state"][i][k].float(), rtol=1e-5, atol=1e-30)

    # a checkpoint loaded into a fresh engine reproduces the next step bit for bit
    m4 = copy.deepcopy(m2)                                      # m2 after step 3 == the parameters e3 was built over
    _train(m3, e3, 1)
    e4 = _engine(m4)
    e4.load_state_dict(sd_stock)
    _train(m4, e4, 1)
    for a, b in zip(m3.parameters(), m4.parameters()):
        assert torch.equal(a, b)


def test_adamw_moments_are_not_allocated():
    m = _model()
    e = _engine(m)
    assert not hasattr(e, "exp_avg") and not hasattr(e, "exp_avg_sq") and e.torch_optimizer is None and e.master is None
    want = sum(sum(p.shape) if p.dim() == 2 else p.numel() for p in e.params)
    assert want <= e.adafactor_state.numel() <= want + 32 * len(e.params) < e.numel
    assert _engine(_model(torch.bfloat16), master_weights=True).master.dtype == torch.float32


def test_refusals():
    from mmgl_amd.distributed import DataParallelEngine
    m = _model()
    adamw = DataParallelEngine(copy.deepcopy(m), lr=LR, fused=False).state_dict()
    e = _engine(m)
    with pytest.raises(ValueError, match="AdamW state"):
        e.load_state_dict(adamw)
    torch_adamw = torch.optim.AdamW(copy.deepcopy(m).parameters(), lr=LR).state_dict()       # no state yet: the group's betas give it away
    with pytest.raises(ValueError, match="AdamW state"):
        e.load_state_dict(torch_adamw)

    class ThreeD(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.randn(2, 3, 4))
            self.b = torch.nn.Parameter(torch.randn(4))
    with pytest.raises(ValueError, match=r"shape \(2, 3, 4\).*optimizer='adafactor'"):
        _engine(ThreeD())
    for opts in (dict(beta1=0.9), dict(relative_step=True), dict(scale_parameter=True), dict(warmup_init=True)):
        with pytest.raises(ValueError, match="use optimizer='adafactor'"):
            _engine(_model(), adafactor=opts)
    with pytest.raises(ValueError, match="unknown optimizer"):
        DataParallelEngine(_model(), optimizer="adafactor_fussed", fused=False)
    assert _engine(_model(), adafactor=dict(weight_decay=0.01, clip_threshold=2.0)).weight_decay == 0.01


def test_trainer_flag_defaults_off():
    from mmgl_amd.language_modelling.run_generation import Arguments
    assert Arguments().fused_adafactor is False
