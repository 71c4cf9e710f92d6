"""CPU tests of the FP8 key/value cache of the Llama-family LM (no compute: there is no GPU here).  The grouped-query
entry point is declared, exported and bound and validates its arguments before any launch; ops.attn_decode_q8(num_kv_heads=) has no
CPU path and its one operand check refuses a cache of H-head rows; LlamaNeighborLM.generate takes kv_cache_dtype through its **lookup
catch-all and refuses what sampling.check_kv_cache refuses before any device work (the prompts are CPU tensors: an accepted call ends
at "no CPU path"); a DecodeCache of Hkv heads has the shapes and the byte ratio of section 4.19."""
import inspect
import os

import pytest
import torch

from helpers import mpt_args

NAME = "mmgl_attn_decode_gqa_q8_fwd"


def test_symbol_is_declared_exported_and_bound():
    from mmgl_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION == 110 and L.mmgl_version() == 110
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "mmgl_hip.h")).read()
    assert NAME in _lib.SIGNATURES and hasattr(L, NAME) and f"int {NAME}(" in header
    # the signature of mmgl_attn_decode_q8_fwd with Hkv after H
    mha = list(_lib.SIGNATURES["mmgl_attn_decode_q8_fwd"][1])
    assert list(_lib.SIGNATURES[NAME][1]) == mha[:19] + [mha[18]] + mha[19:]


def test_argument_validation():
    if torch.cuda.is_available():
        pytest.skip("runs where no GPU is visible: a missing check would launch on a made-up address")
    from mmgl_amd import _lib
    L = _lib.lib()
    err = lambda: L.mmgl_last_error()
    A = 0x10000                                                     # a made-up, 16-byte aligned address: nothing is launched on a refusal
    # (q, ldq, k_new, v_new, ld_new, k_codes, v_codes, ld_code, bs_code, k_scale, v_scale, ld_scale, bs_scale, capacity, key_valid, ld_valid,
    #  out, B, H, Hkv, S, D, dtype, stream): H = 4 query heads on Hkv = 2 heads of D = 64 -- q rows of 256, cache rows of 2 * 128 codes
    attn = lambda q=A, ldq=256, kn=A, vn=A + 256, ld_new=256, kc=A, vc=A + 128, ld_code=256, bs_code=2560, ks=A, vs=A + 2, ld_scale=4, \
        bs_scale=40, cap=10, valid=A, ld_valid=10, out=A, B=2, H=4, Hkv=2, S=5, D=64, dtype=1: getattr(L, NAME)(
            q, ldq, kn, vn, ld_new, kc, vc, ld_code, bs_code, ks, vs, ld_scale, bs_scale, cap, valid, ld_valid, out, B, H, Hkv, S, D, dtype, None)
    for name in ("q", "kn", "vn", "kc", "vc", "ks", "vs", "valid", "out"):
        assert attn(**{name: None}) == 1 and b"null" in err(), name
    assert attn(S=0) == 1 and b"bad sizes" in err()
    assert attn(B=0) == 1 and attn(H=0) == 1
    assert attn(Hkv=0) == 1 and b"bad sizes" in err()
    assert attn(Hkv=3) == 1 and b"no multiple" in err()
    assert attn(H=6, Hkv=4, ldq=384) == 1 and b"no multiple" in err()
    assert attn(S=10) == 1 and b"capacity" in err()                 # capacity = S: no column for the new token
    assert attn(S=11, ld_valid=11) == 1 and b"capacity" in err()
    assert attn(D=48, ldq=192, ld_new=96) == 2 and b"head_dim" in err()
    assert attn(ldq=260) == 2 and b"16 bytes" in err()
    assert attn(ld_new=260) == 2 and attn(ld_code=264) == 2 and attn(bs_code=2568) == 2
    assert attn(ldq=128) == 1 and b"smaller than the rows" in err()  # q rows hold H heads ...
    assert attn(ld_new=64) == 1 and attn(ld_code=64) == 1 and attn(ld_scale=1) == 1 and attn(ld_valid=4) == 1
    assert attn(ld_new=120) == 1 and attn(ld_code=112) == 1        # ... the new rows and the cache rows hold Hkv of them
    assert attn(bs_code=2048) == 1 and attn(bs_scale=32) == 1
    assert attn(q=A + 8) == 2 and b"aligned" in err()
    assert attn(kc=A + 8) == 2 and attn(vc=A + 8) == 2
    assert attn(kn=A + 4) == 2 and b"aligned" in err()             # a misaligned k_new
    assert attn(vn=A + 4) == 2
    assert attn(B=1, cap=(1 << 23) + 1) == 2 and b"2 GiB" in err()
    assert attn(dtype=7) == 1 and b"dtype" in err()


def test_ops_have_no_cpu_path_and_one_operand_check():
    from mmgl_amd import ops
    B, H, Hkv, D, cap = 2, 4, 2, 16, 6
    kvq, scale = torch.zeros(B, cap, 2 * Hkv * D, dtype=torch.uint8).view(torch.float8_e4m3fn), torch.zeros(B, cap, 2 * Hkv, dtype=torch.int8)
    q, new, ok = torch.randn(B, H * D), torch.randn(B, 2 * Hkv * D), torch.ones(B, 5, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.attn_decode_q8(q, new[:, :Hkv * D], new[:, Hkv * D:], kvq, scale, ok, H, num_kv_heads=Hkv)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.kv_quantize(torch.randn(B, 5, Hkv * D), torch.randn(B, 5, Hkv * D), kvq, scale, Hkv)
    # the operand check of the q8 family, as attn_decode_q8 calls it for a grouped-query cache: rows of Hkv heads
    assert ops._q8_cache_operands("attn_decode_q8", kvq, scale, B, Hkv * D, Hkv, q) == (cap, D)
    wide = torch.zeros(B, cap, 2 * H * D, dtype=torch.uint8).view(torch.float8_e4m3fn)
    with pytest.raises(ValueError, match="attn_decode_q8: incompatible codes"):       # kvq with 2*H*D columns
        ops._q8_cache_operands("attn_decode_q8", wide, scale, B, Hkv * D, Hkv, q)
    with pytest.raises(ValueError, match="attn_decode_q8: incompatible codes"):       # scale with 2H
        ops._q8_cache_operands("attn_decode_q8", kvq, torch.zeros(B, cap, 2 * H, dtype=torch.int8), B, Hkv * D, Hkv, q)
    assert [n for n in dir(ops) if n.startswith("_q8") and n.endswith("operands")] == ["_q8_cache_operands"]      # no second checker
    sig = inspect.signature(ops.attn_decode_q8).parameters
    assert list(sig)[-2:] == ["out", "num_kv_heads"] and sig["num_kv_heads"].default is None


def _lm(n_kv=2):
    from transformers import LlamaConfig
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=4, num_attention_heads=4,
                      num_key_value_heads=n_kv, max_position_embeddings=256, pad_token_id=1, bos_token_id=2, eos_token_id=2, attention_dropout=0.0)
    return LlamaNeighborLM(mpt_args(model_name_or_path="llama-tiny", neighbor_layer_wise=2), cfg).eval()


@pytest.fixture(scope="module")
def lm():
    return _lm()


def _call(model, **kw):
    ids = torch.randint(3, 128, (2, 6))
    return model.generate(ids, torch.ones_like(ids), max_new_tokens=4, **kw)


def test_the_keyword_arrives_through_the_catch_all(lm):
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    params = inspect.signature(LlamaNeighborLM.generate).parameters
    assert "kv_cache_dtype" not in params and params["lookup"].kind is inspect.Parameter.VAR_KEYWORD
    with pytest.raises(TypeError, match="unexpected keyword argument 'foo'"):
        _call(lm, foo=1)
    with pytest.raises(TypeError, match="unexpected keyword argument 'foo'"):
        _call(lm, kv_cache_dtype="fp8", foo=1)


@pytest.mark.parametrize("kw,message", [
    (dict(kv_cache_dtype="int8"), r"LlamaNeighborLM\.generate\(\): kv_cache_dtype = 'int8' is unknown"),
    (dict(kv_cache_dtype=torch.bfloat16), r"kv_cache_dtype = torch\.bfloat16 is unknown"),
    (dict(kv_cache_dtype="fp8", prompt_lookup_num_tokens=3), r"FP8 key/value cache\) with prompt_lookup_num_tokens = 3"),
    (dict(kv_cache_dtype=torch.float8_e4m3fn, prompt_lookup_num_tokens=3), r"FP8 key/value cache\) with prompt_lookup_num_tokens = 3"),
    (dict(kv_cache_dtype="fp8", num_beams=2), r"num_beams = 2 is not implemented \(beam search runs on the OPT fork only\)"),
], ids=["int8", "bf16", "lookup", "lookup-dtype", "beams"])
def test_refusals(lm, kw, message):
    with pytest.raises(ValueError, match=message):
        _call(lm, **kw)


def test_num_return_sequences_keeps_the_llama_refusal(lm):
    for kw in (dict(), dict(kv_cache_dtype="fp8")):
        with pytest.raises(ValueError) as today:
            _call(lm, do_sample=True, num_return_sequences=2, **kw)
        assert "FP8 key/value cache" not in str(today.value)


@pytest.mark.parametrize("name", ["q_proj", "o_proj"])
def test_adapted_projections_are_refused(name):
    from mmgl_amd.model.modelling_self_attention import LoRALinear
    model = _lm()
    attn = model.llama.model.layers[1].self_attn
    setattr(attn, name, LoRALinear(getattr(attn, name), 4, 8.0))
    with pytest.raises(ValueError, match=r"FP8 key/value cache\) runs plain nn\.Linear q / k / v / out projections only"):
        _call(model, kv_cache_dtype="fp8")


def test_accepted_calls_reach_the_device_check(lm):
    for kw in (dict(), dict(kv_cache_dtype=None), dict(kv_cache_dtype="fp8"), dict(kv_cache_dtype=torch.float8_e4m3fn),
               dict(kv_cache_dtype="fp8", return_step_logits=True), dict(kv_cache_dtype="fp8", do_sample=True, top_k=5, seed=3),
               dict(kv_cache_dtype="fp8", repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[5])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            _call(lm, **kw)
    ids = torch.randint(3, 128, (2, 6))
    with pytest.raises(RuntimeError, match="no CPU path"):
        lm(input_ids=ids, attention_mask=torch.ones_like(ids), use_cache=True, kv_cache_dtype="fp8")
    with pytest.raises(ValueError, match="belongs to the prefill"):
        lm(input_ids=ids, attention_mask=torch.ones_like(ids), kv_cache_dtype="fp8")
    with pytest.raises(ValueError, match="is unknown"):
        lm(input_ids=ids, attention_mask=torch.ones_like(ids), use_cache=True, kv_cache_dtype="int8")


def test_the_wrapper_over_a_llama_lm_still_does_not_generate():
    from mmgl_amd.model import CrossAttentionModel
    from helpers import tiny_clip_vision_config, tiny_roberta_config
    w = CrossAttentionModel(mpt_args(model_name_or_path="llama-tiny", context="text_only", neighbor_layer_wise=2), None,
                            lm_config=_lm().config, text_config=tiny_roberta_config(), visual_config=tiny_clip_vision_config())
    assert w.can_generate() is False and w.lm.can_generate() is True


@pytest.mark.parametrize("Hkv,D", [(2, 16), (1, 64), (8, 128)])
def test_decode_cache_of_key_value_heads(Hkv, D):
    from mmgl_amd import ops
    from mmgl_amd.model.modelling_cross_attention import DecodeCache
    B, cap = 3, 9
    plain = DecodeCache(2, B, cap, Hkv * D, torch.bfloat16, "cpu")
    c = DecodeCache(2, B, cap, Hkv * D, torch.bfloat16, "cpu", kv_dtype=ops.KV_FP8, num_heads=Hkv)
    assert len(c.kv) == len(c.kv_scale) == 2
    assert all(t.shape == (B, cap, 2 * Hkv * D) and t.dtype == torch.float8_e4m3fn for t in c.kv)
    assert all(t.shape == (B, cap, 2 * Hkv) and t.dtype == torch.int8 for t in c.kv_scale)
    assert c.kv_new.shape == (B, 2 * Hkv * D) and c.kv_new.dtype == torch.bfloat16 and c.kv_new.is_contiguous()
    assert c.kv_out(1) == (c.kv[1], c.kv_scale[1]) and plain.kv_out(1) is plain.kv[1]
    nbytes = lambda cache: sum(t.numel() * t.element_size() for t in cache.kv + (cache.kv_scale or []))
    assert nbytes(c) / nbytes(plain) == (D + 1) / (2 * D)
