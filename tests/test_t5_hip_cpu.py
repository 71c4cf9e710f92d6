"""CPU side of the native T5 forward (mmgl_amd/model/t5_hip.py, ops.attn_relbias): what supports() covers, the bucket table against
HuggingFace's compute_bias along every diagonal, the CPU path of SelfAttentionModel (stock HuggingFace, the runner never entered), the
new symbols in the header and the binding, and the argument checks of the entry points (refused before any launch: no GPU here)."""
import ctypes
import os
import re

import pytest
import torch
from transformers import T5Config, T5ForConditionalGeneration
from transformers.models.t5.modeling_t5 import T5Attention

from helpers import mpt_args, tiny_clip_vision_config, tiny_roberta_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mmgl_attn_relbias_fwd", "mmgl_attn_relbias_bwd_workspace", "mmgl_attn_relbias_bwd")


def _cfg(**kw):
    base = dict(vocab_size=128, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, dropout_rate=0.0,
                decoder_start_token_id=0, pad_token_id=0)
    base.update(kw)
    return T5Config(**base)


def test_supports_decisions():
    from mmgl_amd.model.t5_hip import T5HipRunner
    from mmgl_amd.model.modelling_self_attention import inject_lora
    mk = lambda **kw: T5ForConditionalGeneration(_cfg(**kw))
    assert T5HipRunner.supports(mk())
    assert T5HipRunner.supports(mk(tie_word_embeddings=False))
    assert not T5HipRunner.supports(mk(feed_forward_proj="gated-gelu"))
    assert not T5HipRunner.supports(mk(feed_forward_proj="gelu"))
    assert not T5HipRunner.supports(mk(d_kv=32))
    assert not T5HipRunner.supports(mk(d_kv=48))
    assert not T5HipRunner.supports(mk(d_model=132))
    assert not T5HipRunner.supports(mk(d_ff=252))
    lora = mk()
    inject_lora(lora, 4, 1.0, 0.0)
    assert not T5HipRunner.supports(lora)                       # LoRA modules in place of q / v: the stock call
    assert not T5HipRunner.supports(torch.nn.Linear(4, 4))
    with pytest.raises(ValueError):
        T5HipRunner(mk(d_kv=32))


@pytest.mark.parametrize("bidirectional", [True, False])
def test_bucket_table_rebuilds_compute_bias_bitwise(bidirectional):
    from mmgl_amd import ops
    cfg = _cfg(is_decoder=not bidirectional, num_heads=3, d_model=192)
    att = T5Attention(cfg, has_relative_attention_bias=True, layer_idx=0)
    for T, S in ((1, 1), (17, 40), (130, 70), (200, 200)):
        bucket_of = ops.t5_bucket_table(T, S, bidirectional, cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance, "cpu")
        assert bucket_of.dtype == torch.int32 and tuple(bucket_of.shape) == (T + S - 1,)
        assert ops.t5_bucket_table(T, S, bidirectional, cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance, "cpu") is bucket_of
        want = att.compute_bias(T, S)[0]                        # [H, T, S]
        idx = torch.arange(S)[None, :] - torch.arange(T)[:, None] + T - 1
        got = att.relative_attention_bias.weight[bucket_of.long()[idx]].permute(2, 0, 1)
        assert torch.equal(got, want)


def test_cpu_call_of_the_wrapper_stays_stock(monkeypatch):
    from mmgl_amd.model import SelfAttentionModel
    from mmgl_amd.model.t5_hip import T5HipRunner
    assert SelfAttentionModel.t5_native is True
    args = mpt_args(neighbor_mode="raw", context="text_only", model_name_or_path="t5-tiny", decoder_only=False, peft_type="none")
    torch.manual_seed(0)
    model = SelfAttentionModel(args, None, lm_config=_cfg(), text_config=tiny_roberta_config(), visual_config=tiny_clip_vision_config())
    assert T5HipRunner.supports(model.lm) and model.can_generate() is False

    def boom(*a, **k):
        raise AssertionError("the native runner was entered on CPU tensors")
    monkeypatch.setattr(T5HipRunner, "__call__", boom)
    before = T5HipRunner.calls
    ids = torch.randint(1, 128, (2, 9))
    out = model(ids, torch.ones_like(ids), torch.randint(1, 128, (2, 5)))
    assert torch.isfinite(out.loss) and out.logits.shape == (2, 5, 128)
    assert T5HipRunner.calls == before and "_t5_runner" not in model.__dict__


def test_symbols_declared_and_bound():
    from mmgl_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmgl_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/mmgl_hip.h"
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().mmgl_version() == _lib.ABI_VERSION


def test_unsupported_arguments_are_refused_before_any_launch():
    from mmgl_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(256)              # never dereferenced: every check below fails on the host
    def fwd(T, S, D, causal, ld):
        return L.mmgl_attn_relbias_fwd(one, one, one, None, None, None, one, one, 2, 3, T, S, D, 0, ld, ld, causal, 0.0, 0, _lib.BF16, None)
    assert fwd(17, 40, 64, 1, 192) == _lib._ERR_UNSUPPORTED     # causal needs T == S
    assert fwd(17, 17, 48, 0, 144) == _lib._ERR_UNSUPPORTED     # head_dim 48
    assert fwd(17, 17, 32, 0, 96) == _lib._ERR_UNSUPPORTED
    assert fwd(17, 17, 64, 0, 100) == _lib._ERR_INVALID         # pitch below H * D
    assert L.mmgl_attn_relbias_bwd_workspace(2, 3, 17, 40) > 0 and L.mmgl_attn_relbias_bwd_workspace(0, 3, 17, 40) == 0
    rc = L.mmgl_attn_relbias_bwd(one, one, one, one, one, one, None, None, None, one, one, one, None, one, 16, 2, 3, 17, 40, 64, 0, 192, 192,
                                 0, 0.0, 0, _lib.BF16, None)
    assert rc == _lib._ERR_INVALID                              # workspace too small
