"""CPU tests of the Llama-family generation boundary (no compute: there is no GPU here): LlamaNeighborLM says it can generate and fails
loudly on CPU tensors; the two entry points of its decode step (mmgl_attn_decode_gqa_fwd, mmgl_rope_kv_append) are declared, exported and
bound, and validate their arguments before any launch."""
import pytest
import torch

from helpers import mpt_args


def _tiny_lm(n_kv=2):
    from transformers import LlamaConfig
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    cfg = LlamaConfig(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=4, num_attention_heads=4,
                      num_key_value_heads=n_kv, max_position_embeddings=256, pad_token_id=1, bos_token_id=2, eos_token_id=2,
                      attention_dropout=0.0)
    return LlamaNeighborLM(mpt_args(model_name_or_path="llama-tiny", neighbor_layer_wise=2), cfg)


def test_llama_lm_can_generate_and_has_no_cpu_path():
    lm = _tiny_lm().eval()
    assert lm.can_generate() is True
    ids = torch.randint(3, 128, (2, 6))
    with pytest.raises(RuntimeError, match="no CPU path"):
        lm.generate(ids, torch.ones_like(ids), max_new_tokens=4)
    with pytest.raises(ValueError, match="max_new_tokens"):
        lm.generate(ids, torch.ones_like(ids), max_new_tokens=0)


def test_llama_cache_refusals():
    lm = _tiny_lm()
    ids = torch.randint(3, 128, (2, 6))
    with pytest.raises(ValueError, match="training mode"):
        lm.train()(input_ids=ids, attention_mask=torch.ones_like(ids), use_cache=True)
    lm.eval()
    with pytest.raises(ValueError, match="capacity"):           # a cache larger than the rotary table may grow
        lm(input_ids=ids, attention_mask=torch.ones_like(ids), use_cache=True, cache_capacity=257)
    with pytest.raises(ValueError, match="capacity"):           # a prompt wider than the cache
        lm(input_ids=ids, attention_mask=torch.ones_like(ids), use_cache=True, cache_capacity=5)
    with pytest.raises(ValueError, match="DecodeCache"):
        lm(input_ids=ids[:, :1], past_key_values=((None, None),))
    from mmgl_amd.model.modelling_cross_attention import DecodeCache
    cache = DecodeCache(4, 2, 8, 2 * 16, torch.float32, "cpu")
    assert cache.kv[0].shape == (2, 8, 2 * 2 * 16)
    with pytest.raises(ValueError, match="not been filled"):
        lm(input_ids=ids[:, :1], past_key_values=cache)
    with pytest.raises(ValueError, match="one new token"):
        lm(input_ids=ids, past_key_values=cache)
    with pytest.raises(ValueError, match="labels"):
        lm(input_ids=ids[:, :1], labels=ids[:, :1], past_key_values=cache)


def test_gqa_decode_symbols_are_bound():
    from mmgl_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 109 and L.mmgl_version() == _lib.ABI_VERSION
    import os
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "mmgl_hip.h")).read()
    for name in ("mmgl_attn_decode_gqa_fwd", "mmgl_rope_kv_append"):
        assert name in _lib.SIGNATURES and hasattr(L, name) and f"int {name}(" in header


def test_gqa_decode_argument_validation():
    from mmgl_amd import _lib
    L = _lib.lib()
    # mmgl_attn_decode_gqa_fwd(q, ldq, k, v, ldkv, batch_stride_kv, key_valid, ld_valid, out, B, H, Hkv, S, D, dtype, stream)
    assert L.mmgl_attn_decode_gqa_fwd(None, 256, None, None, 256, 2560, None, 10, None, 2, 4, 2, 10, 64, 1, None) == 1
    assert b"null" in L.mmgl_last_error()
    assert L.mmgl_attn_decode_gqa_fwd(None, 256, None, None, 256, 2560, None, 10, None, 2, 4, 3, 10, 64, 1, None) == 1     # H % Hkv
    assert b"multiple" in L.mmgl_last_error()
    assert L.mmgl_attn_decode_gqa_fwd(None, 192, None, None, 192, 1920, None, 10, None, 2, 4, 2, 10, 48, 1, None) == 2     # head_dim
    assert L.mmgl_attn_decode_gqa_fwd(None, 256, None, None, 256, 2560, None, 10, None, 2, 4, 0, 10, 64, 1, None) == 1     # no kv head
    assert L.mmgl_attn_decode_gqa_fwd(None, 256, None, None, 256, 2560, None, 10, None, 2, 4, 2, 0, 64, 1, None) == 1      # no keys
    assert L.mmgl_attn_decode_gqa_fwd(None, 256, None, None, 260, 2600, None, 10, None, 2, 4, 2, 10, 64, 1, None) == 2     # rows not 16-byte multiples
    assert L.mmgl_attn_decode_gqa_fwd(None, 256, None, None, 256, 2560, None, 10, None, 2, 4, 2, 10, 64, 7, None) == 1     # dtype
    # mmgl_rope_kv_append(qkv, ldqkv, cos_sin_row, kv_col, batch_stride_kv, B, H, Hkv, D, dtype, stream)
    assert L.mmgl_rope_kv_append(None, 512, None, None, 2560, 2, 4, 2, 64, 1, None) == 1
    assert b"null" in L.mmgl_last_error()
    assert L.mmgl_rope_kv_append(None, 512, None, None, 2560, 2, 4, 3, 64, 1, None) == 1                                   # H % Hkv
    assert b"multiple" in L.mmgl_last_error()
    assert L.mmgl_rope_kv_append(None, 384, None, None, 2560, 2, 4, 2, 48, 1, None) == 2                                   # head_dim
    assert L.mmgl_rope_kv_append(None, 516, None, None, 2560, 2, 4, 2, 64, 1, None) == 2                                   # rows not 16-byte multiples
    assert L.mmgl_rope_kv_append(None, 512, None, None, 2560, 0, 4, 2, 64, 1, None) == 1                                   # no rows


def test_gqa_decode_ops_have_no_cpu_path():
    from mmgl_amd import ops
    q, k = torch.randn(2, 64), torch.randn(2, 4, 32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.attn_decode(q, k, k.clone(), torch.ones(2, 4, dtype=torch.bool), 4, num_kv_heads=2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rope_kv_append(torch.randn(2, 128), torch.zeros(8, 2), torch.zeros(2, 64), 4, 2)
