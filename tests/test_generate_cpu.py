"""CPU tests of the generation boundary (no compute: there is no GPU here): the two decode entry points are declared, exported and
bound; they validate their arguments before any launch; ops.decode_linear / ops.attn_decode / generate() fail loudly on CPU tensors;
the decode cache refuses what it does not implement."""
import pytest
import torch

from helpers import mpt_args, tiny_opt_config


def test_decode_symbols_are_bound():
    from mmgl_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 106 and L.mmgl_version() == _lib.ABI_VERSION
    for name in ("mmgl_gemm_skinny", "mmgl_attn_decode_fwd"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    header = open(__import__("os").path.join(__import__("os").path.dirname(_lib.__file__), "..", "include", "mmgl_hip.h")).read()
    for cite in ("run_generation.py:597-603", "modelling_cross_attention.py:372", ":629", ":851-870"):
        assert cite in header, cite


def test_decode_argument_validation():
    from mmgl_amd import _lib
    L = _lib.lib()
    # mmgl_gemm_skinny(x, ldx, W, ldw, bias, residual, y, ldy, M, N, K, act, scale, dtype, stream)
    assert L.mmgl_gemm_skinny(None, 64, None, 64, None, None, None, 64, 4, 64, 64, 0, 1.0, 1, None) == 1
    assert b"null" in L.mmgl_last_error()
    assert L.mmgl_gemm_skinny(None, 64, None, 64, None, None, None, 64, 65, 64, 64, 0, 1.0, 1, None) == 2      # M > 64
    assert L.mmgl_gemm_skinny(None, 64, None, 64, None, None, None, 64, 65, 64, 64, 0, 1.0, 0, None) == 2
    assert L.mmgl_gemm_skinny(None, 64, None, 64, None, None, None, 64, 0, 64, 64, 0, 1.0, 1, None) == 1
    assert L.mmgl_gemm_skinny(None, 64, None, 64, None, None, None, 64, 4, 64, 64, 0, 1.0, 7, None) == 1       # dtype
    # mmgl_attn_decode_fwd(q, ldq, k, v, ldkv, batch_stride_kv, key_valid, ld_valid, out, B, H, S, D, dtype, stream)
    assert L.mmgl_attn_decode_fwd(None, 64, None, None, 128, 1280, None, 10, None, 2, 1, 10, 64, 1, None) == 1
    assert b"null" in L.mmgl_last_error()
    assert L.mmgl_attn_decode_fwd(None, 48, None, None, 96, 960, None, 10, None, 2, 1, 10, 48, 1, None) == 2   # head_dim
    assert L.mmgl_attn_decode_fwd(None, 64, None, None, 128, 1280, None, 10, None, 2, 1, 0, 64, 1, None) == 1  # no keys
    assert L.mmgl_attn_decode_fwd(None, 64, None, None, 132, 1320, None, 10, None, 2, 1, 10, 64, 1, None) == 2  # rows not 16-byte multiples
    # any key count: the cross call site's S <= 256 limit does not apply
    assert L.mmgl_attn_decode_fwd(None, 64, None, None, 128, 128 * 672, None, 672, None, 2, 1, 672, 64, 1, None) == 1


def test_decode_ops_have_no_cpu_path():
    from mmgl_amd import ops
    x, w = torch.randn(2, 64), torch.randn(8, 64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.decode_linear(x, w)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.attn_decode(x, torch.randn(2, 4, 64), torch.randn(2, 4, 64), torch.ones(2, 4, dtype=torch.bool), 1)


def _tiny_lm():
    from mmgl_amd.model.modelling_cross_attention import MPTConfig, MPTForCausalLM
    return MPTForCausalLM(MPTConfig(mpt_args(neighbor_mode="raw", peft_type="none"), tiny_opt_config(dropout=0.0))).eval()


def test_generate_has_no_cpu_path():
    from mmgl_amd.model import CrossAttentionModel
    from helpers import tiny_clip_vision_config, tiny_roberta_config
    lm = _tiny_lm()
    ids = torch.randint(3, 128, (2, 6))
    with pytest.raises(RuntimeError, match="no CPU path"):
        lm.generate(ids, torch.ones_like(ids), max_new_tokens=4)
    w = CrossAttentionModel(mpt_args(), tokenizer=None, lm_config=tiny_opt_config(dropout=0.0), text_config=tiny_roberta_config(),
                            visual_config=tiny_clip_vision_config()).eval()
    assert w.can_generate() and lm.can_generate()
    with pytest.raises(RuntimeError, match="no CPU path"):
        w.generate(ids, torch.ones_like(ids), max_new_tokens=4)


def test_decode_cache_refusals():
    from mmgl_amd.model.modelling_cross_attention import DecodeCache
    lm = _tiny_lm()
    dec = lm.model.decoder
    cfg = lm.config
    ids = torch.randint(3, 128, (2, 6))
    table = torch.zeros(3, 2 * cfg.num_hidden_layers * cfg.hidden_size)
    with pytest.raises(ValueError, match="prefix"):           # a prefix table AND a request for a decode cache
        dec(input_ids=ids, attention_mask=torch.ones_like(ids), past_key_values=table, use_cache=True)
    cache = DecodeCache(cfg.num_hidden_layers, 2, 8, cfg.hidden_size, torch.float32, "cpu")
    assert cache.kv[0].shape == (2, 8, 2 * cfg.hidden_size) and cache.mask.shape == (2, 8) and cache.col == 0
    with pytest.raises(ValueError, match="layer_head_mask"):
        dec(input_ids=ids[:, :1], past_key_values=cache, head_mask=torch.ones(cfg.num_hidden_layers, cfg.num_attention_heads))
    with pytest.raises(ValueError, match="output_attentions"):
        dec(input_ids=ids[:, :1], past_key_values=cache, output_attentions=True)
    with pytest.raises(ValueError, match="not been filled"):
        dec(input_ids=ids[:, :1], past_key_values=cache)
    with pytest.raises(ValueError, match="one new token"):
        cache.next_pos = torch.full((2,), 2)
        dec(input_ids=ids, past_key_values=cache)
    cache.col = 8
    with pytest.raises(ValueError, match="full"):
        dec(input_ids=ids[:, :1], past_key_values=cache)
    with pytest.raises(ValueError, match="capacity"):          # a cache larger than the position table
        dec(input_ids=ids, attention_mask=torch.ones_like(ids), use_cache=True, cache_capacity=cfg.max_position_embeddings + 1)
    from mmgl_amd.model.modelling_cross_attention import MPTConfig, MPTForCausalLM
    hot = MPTForCausalLM(MPTConfig(mpt_args(neighbor_mode="raw", peft_type="none"), tiny_opt_config(dropout=0.1))).train()
    with pytest.raises(ValueError, match="training mode"):
        hot.model.decoder(input_ids=ids, attention_mask=torch.ones_like(ids), use_cache=True)
    # the prefix table alone keeps its meaning: it is not mistaken for a cache (fails later, on the CPU tensors)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dec(input_ids=ids, attention_mask=torch.ones(2, 9), past_key_values=table)


def test_llama_wrapper_cannot_generate():
    """The Llama-family wrapper (a real one, tiny, on the CPU) has no generate(): can_generate() is false and generate() says so."""
    from transformers import LlamaConfig
    from helpers import tiny_clip_vision_config, tiny_roberta_config
    from mmgl_amd.model import CrossAttentionModel
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    llama = LlamaConfig(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=4, num_attention_heads=4,
                        num_key_value_heads=4, max_position_embeddings=256, pad_token_id=1, bos_token_id=2, eos_token_id=2,
                        attention_dropout=0.0)
    w = CrossAttentionModel(mpt_args(model_name_or_path="llama-tiny", context="text_only", neighbor_layer_wise=2), None, lm_config=llama,
                            text_config=tiny_roberta_config(), visual_config=tiny_clip_vision_config())
    assert isinstance(w.lm, LlamaNeighborLM) and w.can_generate() is False
    ids = torch.randint(3, 128, (2, 6))
    with pytest.raises(ValueError, match="OPT fork"):
        w.generate(ids, torch.ones_like(ids), max_new_tokens=4)
