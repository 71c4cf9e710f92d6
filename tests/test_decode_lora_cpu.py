"""CPU tests of the LoRA decode boundary (no compute: there is no GPU here): mmgl_gemm_skinny_lora is declared, exported and bound
and validates its arguments before any launch; ops.decode_lora_linear and SelfAttentionModel.generate() fail loudly on CPU tensors;
SelfAttentionModel.can_generate() says which language models generate() serves."""
import os

import pytest
import torch

from helpers import mpt_args, tiny_clip_vision_config, tiny_opt_config, tiny_roberta_config


def test_lora_decode_symbol_is_bound():
    from mmgl_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 107 and L.mmgl_version() == _lib.ABI_VERSION
    assert "mmgl_gemm_skinny_lora" in _lib.SIGNATURES and hasattr(L, "mmgl_gemm_skinny_lora")
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "mmgl_hip.h")).read()
    assert "int mmgl_gemm_skinny_lora(" in header and "workspace" in header


def _call(L, M=4, N=64, K=64, r=8, dtype=1, null=True, act=0):
    # mmgl_gemm_skinny_lora(x, ldx, W, ldw, bias, residual, y, ldy, A, lda, B, ldb, r, lora_scale, workspace, M, N, K, act, scale, dtype, stream)
    p = None if null else 64        # a non-null address that is never dereferenced: every check below fails before a launch
    return L.mmgl_gemm_skinny_lora(p, K, p, K, None, None, p, N, p, K, p, max(r, 1), r, 2.0, p, M, N, K, act, 1.0, dtype, None)


def test_lora_decode_argument_validation():
    from mmgl_amd import _lib
    L = _lib.lib()
    assert _call(L) == 1                                   # null pointers
    assert b"null" in L.mmgl_last_error()
    assert _call(L, M=65) == 2                             # M > 64: the caller chunks
    assert _call(L, M=65, dtype=0) == 2
    assert _call(L, M=0) == 1
    assert _call(L, r=0) == 1
    assert _call(L, r=257) == 2
    assert b"rank" in L.mmgl_last_error()
    assert _call(L, dtype=7) == 1                          # dtype
    assert _call(L, dtype=7, null=False) == 1
    assert _call(L, act=5, null=False) == 1                # activation, with every pointer set
    assert b"activation" in L.mmgl_last_error()


def test_decode_lora_linear_has_no_cpu_path():
    from mmgl_amd import ops
    x, w, A, B = torch.randn(2, 64), torch.randn(8, 64), torch.randn(4, 64), torch.randn(8, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.decode_lora_linear(x, w, None, A, B, 2.0)
    from mmgl_amd.model.modelling_self_attention import LoRALinear
    with pytest.raises(RuntimeError, match="no CPU path"):
        LoRALinear(torch.nn.Linear(64, 8), 4, 8.0).decode(x)


def _wrapper(**kw):
    from mmgl_amd.model import SelfAttentionModel
    name = kw.pop("name", "opt-tiny")
    lm_config = kw.pop("lm_config", None) or tiny_opt_config(dropout=0.0)
    args = mpt_args(neighbor_mode="raw", context="text_only", model_name_or_path=name, **kw)
    return SelfAttentionModel(args, None, lm_config=lm_config, text_config=tiny_roberta_config(), visual_config=tiny_clip_vision_config()).eval()


def test_self_attention_model_can_generate_truth_table():
    from transformers import T5Config
    for peft in ("none", "lora", "prompt"):
        assert _wrapper(peft_type=peft).can_generate() is True, peft
    assert _wrapper(peft_type="prefix").can_generate() is False
    t5 = T5Config(vocab_size=128, d_model=32, d_kv=8, d_ff=64, num_layers=1, num_decoder_layers=1, num_heads=4, decoder_start_token_id=0)
    for peft in ("none", "lora", "prompt", "prefix"):
        assert _wrapper(name="t5-tiny", lm_config=t5, decoder_only=False, peft_type=peft).can_generate() is False, peft


def test_self_attention_generate_refusals():
    ids = torch.randint(3, 128, (2, 6))
    for peft in ("none", "lora", "prompt"):
        with pytest.raises(RuntimeError, match="no CPU path"):
            _wrapper(peft_type=peft).generate(ids, torch.ones_like(ids), max_new_tokens=4)
    with pytest.raises(ValueError, match="prefix"):
        _wrapper(peft_type="prefix").generate(ids, torch.ones_like(ids), max_new_tokens=4)
    lm = _wrapper(peft_type="none").lm
    with pytest.raises(ValueError, match="exactly one"):
        lm.generate(ids, torch.ones_like(ids), inputs_embeds=torch.zeros(2, 6, 64))
    with pytest.raises(ValueError, match="exactly one"):
        lm.generate(attention_mask=torch.ones_like(ids))
    with pytest.raises(RuntimeError, match="no CPU path"):
        lm.generate(inputs_embeds=torch.zeros(2, 6, 64), attention_mask=torch.ones_like(ids), max_new_tokens=4)
