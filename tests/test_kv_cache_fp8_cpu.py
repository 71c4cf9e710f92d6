"""CPU tests of the FP8 key/value cache (no compute: there is no GPU here).  The two entry points are declared,
exported and bound and validate their arguments before any launch; the ops have no CPU path; generate(kv_cache_dtype=...) refuses
what sampling.check_kv_cache refuses before any device work (the prompts are CPU tensors: an accepted call ends at "no CPU path");
and the torch restatement of the format, tests/kvq_ref.py, has the properties the GPU tests rest on."""
import inspect
import os

import pytest
import torch

import kvq_ref
from helpers import mpt_args, tiny_clip_vision_config, tiny_opt_config, tiny_roberta_config

NAMES = ("mmgl_kv_quantize", "mmgl_attn_decode_q8_fwd")


def test_symbols_are_declared_exported_and_bound():
    from mmgl_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION == 110 and L.mmgl_version() == 110
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "mmgl_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(L, name) and f"int {name}(" in header


def test_argument_validation():
    if torch.cuda.is_available():
        pytest.skip("runs where no GPU is visible: a missing check would launch on a made-up address")
    from mmgl_amd import _lib
    L = _lib.lib()
    err = lambda: L.mmgl_last_error()
    A = 0x10000                                                     # a made-up, 16-byte aligned address: nothing is launched on a refusal
    # mmgl_kv_quantize(k, v, ld_src, bs_src, codes, ld_code, bs_code, scale, ld_scale, bs_scale, B, n, H, D, dtype, stream)
    quant = lambda k=A, v=A, ld_src=384, bs_src=1920, codes=A, ld_code=256, bs_code=2560, scale=A, ld_scale=4, bs_scale=40, B=2, n=5, H=2, D=64, \
        dtype=1: L.mmgl_kv_quantize(k, v, ld_src, bs_src, codes, ld_code, bs_code, scale, ld_scale, bs_scale, B, n, H, D, dtype, None)
    assert quant(k=None) == 1 and b"null" in err()
    assert quant(codes=None) == 1 and quant(scale=None) == 1 and quant(v=None) == 1
    assert quant(B=0) == 1 and b"bad sizes" in err()
    assert quant(n=0) == 1 and quant(H=0) == 1
    assert quant(D=48) == 2 and b"head_dim" in err()
    assert quant(ld_src=388) == 2 and b"16 bytes" in err()
    assert quant(bs_src=1924) == 2 and quant(ld_code=264) == 2 and quant(bs_code=2568) == 2
    assert quant(ld_src=64) == 1 and b"smaller than the rows" in err()
    assert quant(ld_code=128) == 1 and quant(ld_scale=3) == 1 and quant(bs_code=1024) == 1 and quant(bs_scale=16) == 1
    assert quant(k=A + 8) == 2 and b"aligned" in err()
    assert quant(codes=A + 4) == 2
    assert quant(dtype=7) == 1 and b"dtype" in err()
    # mmgl_attn_decode_q8_fwd(q, ldq, k_new, v_new, ld_new, k_codes, v_codes, ld_code, bs_code, k_scale, v_scale, ld_scale, bs_scale, capacity,
    #                         key_valid, ld_valid, out, B, H, S, D, dtype, stream)
    attn = lambda q=A, ldq=128, kn=A, vn=A, ld_new=256, kc=A, vc=A + 128, ld_code=256, bs_code=2560, ks=A, vs=A + 2, ld_scale=4, bs_scale=40, \
        cap=10, valid=A, ld_valid=10, out=A, B=2, H=2, S=5, D=64, dtype=1: L.mmgl_attn_decode_q8_fwd(
            q, ldq, kn, vn, ld_new, kc, vc, ld_code, bs_code, ks, vs, ld_scale, bs_scale, cap, valid, ld_valid, out, B, H, S, D, dtype, None)
    for name in ("q", "kn", "vn", "kc", "vc", "ks", "vs", "valid", "out"):
        assert attn(**{name: None}) == 1 and b"null" in err(), name
    assert attn(S=0) == 1 and b"bad sizes" in err()
    assert attn(B=0) == 1 and attn(H=0) == 1
    assert attn(S=10) == 1 and b"capacity" in err()                 # no column for the new token
    assert attn(D=48, ldq=96, ld_new=192) == 2 and b"head_dim" in err()
    assert attn(ldq=132) == 2 and b"16 bytes" in err()
    assert attn(ld_new=260) == 2 and attn(ld_code=264) == 2 and attn(bs_code=2568) == 2
    assert attn(ldq=64) == 1 and b"smaller than the rows" in err()
    assert attn(ld_new=64) == 1 and attn(ld_code=64) == 1 and attn(ld_scale=1) == 1 and attn(ld_valid=4) == 1
    assert attn(bs_code=2048) == 1 and attn(bs_scale=32) == 1
    assert attn(q=A + 8) == 2 and b"aligned" in err()
    assert attn(kc=A + 8) == 2 and attn(kn=A + 4) == 2
    assert attn(B=1, cap=(1 << 23) + 1) == 2 and b"2 GiB" in err()
    assert attn(dtype=7) == 1 and b"dtype" in err()


def test_ops_have_no_cpu_path():
    from mmgl_amd import ops
    kvq, scale = torch.zeros(2, 6, 128, dtype=torch.uint8).view(torch.float8_e4m3fn), torch.zeros(2, 6, 4, dtype=torch.int8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.kv_quantize(torch.randn(2, 5, 64), torch.randn(2, 5, 64), kvq, scale, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.attn_decode_q8(torch.randn(2, 64), torch.randn(2, 64), torch.randn(2, 64), kvq, scale, torch.ones(2, 5, dtype=torch.bool), 2)


def _lm():
    from mmgl_amd.model.modelling_cross_attention import MPTConfig, MPTForCausalLM
    return MPTForCausalLM(MPTConfig(mpt_args(neighbor_mode="raw", peft_type="none"), tiny_opt_config(dropout=0.0))).eval()


def _wrapper():
    from mmgl_amd.model import CrossAttentionModel
    return CrossAttentionModel(mpt_args(), tokenizer=None, lm_config=tiny_opt_config(dropout=0.0), text_config=tiny_roberta_config(),
                               visual_config=tiny_clip_vision_config()).eval()


@pytest.fixture(scope="module", params=["MPTForCausalLM", "CrossAttentionModel"])
def model(request):
    return _lm() if request.param == "MPTForCausalLM" else _wrapper()


def _call(model, **kw):
    ids = torch.randint(3, 128, (2, 6))
    return model.generate(ids, torch.ones_like(ids), max_new_tokens=4, **kw)


@pytest.mark.parametrize("kw,message", [
    (dict(kv_cache_dtype="int8"), r"kv_cache_dtype = 'int8' is unknown"),
    (dict(kv_cache_dtype=torch.float8_e5m2), r"kv_cache_dtype = torch\.float8_e5m2 is unknown"),
    (dict(kv_cache_dtype=torch.bfloat16), r"kv_cache_dtype = torch\.bfloat16 is unknown"),
    (dict(kv_cache_dtype="fp8", num_beams=2), r"FP8 key/value cache\) with num_beams = 2 is not implemented"),
    (dict(kv_cache_dtype=torch.float8_e4m3fn, num_beams=4), r"FP8 key/value cache\) with num_beams = 4 is not implemented"),
    (dict(kv_cache_dtype="fp8", do_sample=True, num_return_sequences=2), r"FP8 key/value cache\) with num_return_sequences = 2"),
    (dict(kv_cache_dtype="fp8", prompt_lookup_num_tokens=3), r"FP8 key/value cache\) with prompt_lookup_num_tokens = 3"),
    (dict(kv_cache_dtype="fp8", penalty_alpha=0.6, top_k=4), r"FP8 key/value cache\) with penalty_alpha = 0\.6"),
], ids=lambda v: None if isinstance(v, str) and "cache" in v else str(v))
def test_refusals_name_the_fp8_cache_and_the_option(model, kw, message):
    with pytest.raises(ValueError, match=message):
        _call(model, **kw)


def test_adapted_projections_are_refused():
    from mmgl_amd.model.modelling_self_attention import LoRALinear
    for make, lm_of in ((_lm, lambda m: m), (_wrapper, lambda m: m.lm)):
        for name in ("q_proj", "k_proj", "v_proj", "out_proj"):
            model = make()
            attn = lm_of(model).model.decoder.layers[1].self_attn
            setattr(attn, name, LoRALinear(getattr(attn, name), 4, 8.0))
            with pytest.raises(ValueError, match=r"FP8 key/value cache\) runs plain nn\.Linear q / k / v / out projections only"):
                _call(model, kv_cache_dtype="fp8")
            with pytest.raises((RuntimeError, ValueError), match="no CPU path|plain nn.Linear"):     # without the keyword: today's path
                _call(model)


def test_prefix_tuning_is_refused():
    from mmgl_amd.model import sampling
    with pytest.raises(ValueError, match=r"FP8 key/value cache\) with a prefix-tuning past_key_values"):
        sampling.check_kv_cache("generate()", "fp8", past_key_values=torch.zeros(3, 8))
    lm = _lm()
    cfg = lm.config
    ids = torch.randint(3, 128, (2, 6))
    table = torch.zeros(3, 2 * cfg.num_hidden_layers * cfg.hidden_size)
    with pytest.raises(ValueError, match=r"FP8 key/value cache\) with a prefix-tuning past_key_values"):
        lm.model.decoder(input_ids=ids, attention_mask=torch.ones_like(ids), past_key_values=table, use_cache=True, kv_cache_dtype="fp8")
    with pytest.raises(ValueError, match="belongs to the prefill"):
        lm.model.decoder(input_ids=ids, attention_mask=torch.ones_like(ids), kv_cache_dtype="fp8")


def test_accepted_calls_reach_the_device_check(model):
    from mmgl_amd.model import sampling
    assert sampling.check_kv_cache("generate()", None, num_beams=4, penalty_alpha=0.5) is None            # off: nothing to refuse
    assert sampling.check_kv_cache("generate()", "fp8") is torch.float8_e4m3fn
    assert sampling.check_kv_cache("generate()", torch.float8_e4m3fn) is torch.float8_e4m3fn
    for kw in (dict(kv_cache_dtype=None), dict(kv_cache_dtype="fp8"), dict(kv_cache_dtype=torch.float8_e4m3fn),
               dict(kv_cache_dtype="fp8", return_step_logits=True), dict(kv_cache_dtype="fp8", do_sample=True, top_k=5, seed=3),
               dict(kv_cache_dtype="fp8", repetition_penalty=1.3, no_repeat_ngram_size=2)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            _call(model, **kw)
    with pytest.raises(ValueError, match="num_beams = 2"):                                                  # the other checks still hold
        _call(model, kv_cache_dtype="fp8", num_beams=2, do_sample=True)


def test_the_other_generators_do_not_take_the_keyword():
    from mmgl_amd.model import CrossAttentionModel, SelfAttentionModel
    from mmgl_amd.model.modelling_cross_attention import MPTForCausalLM
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    for cls in (MPTForCausalLM, CrossAttentionModel):
        p = inspect.signature(cls.generate).parameters["kv_cache_dtype"]
        assert p.default is None
    for cls in (SelfAttentionModel, LlamaNeighborLM):
        assert "kv_cache_dtype" not in inspect.signature(cls.generate).parameters


def test_decode_cache_shapes_and_arguments():
    from mmgl_amd import ops
    from mmgl_amd.language_modelling.run_generation import Arguments
    from mmgl_amd.model.modelling_cross_attention import DecodeCache
    plain = DecodeCache(3, 2, 9, 64, torch.bfloat16, "cpu")
    assert plain.kv_dtype is None and plain.kv_scale is None and plain.kv_new is None and plain.kv[0].dtype == torch.bfloat16
    assert plain.kv_out(1) is plain.kv[1]
    c = DecodeCache(3, 2, 9, 64, torch.bfloat16, "cpu", kv_dtype=ops.KV_FP8, num_heads=4)
    assert ops.KV_FP8 is torch.float8_e4m3fn and len(c.kv) == 3 and len(c.kv_scale) == 3
    assert all(t.shape == (2, 9, 128) and t.dtype == torch.float8_e4m3fn for t in c.kv)
    assert all(t.shape == (2, 9, 8) and t.dtype == torch.int8 for t in c.kv_scale)
    assert c.kv_new.shape == (2, 128) and c.kv_new.dtype == torch.bfloat16 and c.kv_out(2) == (c.kv[2], c.kv_scale[2]) and c.cross == []
    nbytes = lambda cache: sum(t.numel() * t.element_size() for t in cache.kv + (cache.kv_scale or []))
    assert nbytes(c) / nbytes(plain) == (2 * 64 + 2 * 4) / (4 * 64)
    with pytest.raises(ValueError, match="kv_dtype"):
        DecodeCache(3, 2, 9, 64, torch.bfloat16, "cpu", kv_dtype=torch.float8_e5m2, num_heads=4)
    with pytest.raises(ValueError, match="num_heads"):
        DecodeCache(3, 2, 9, 64, torch.bfloat16, "cpu", kv_dtype=ops.KV_FP8)
    assert Arguments().kv_cache_dtype is None


# ------------------------------------------------------------------------------------------ the restatement
def _rows(seed, n, H, D, dtype):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, H, D, generator=g) * torch.exp2(torch.randint(-20, 21, (n, H, 1), generator=g).float())
    return x.reshape(n, H * D).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [16, 64, 128])
def test_restatement_scaled_amax_and_exactness(D, dtype):
    H = 3
    x = _rows(D, 200, H, D, dtype)
    x[7, D:2 * D] = 0                                               # an all-zero head
    codes, e = kvq_ref.quantize(x, H)
    assert codes.dtype == torch.uint8 and e.dtype == torch.int8 and codes.shape == x.shape and e.shape == (200, H)
    a = x.float().reshape(200, H, D).abs().amax(-1)
    scaled = torch.ldexp(a, -e.to(torch.int32))
    nz = a > 0
    assert ((scaled[nz] > 224) & (scaled[nz] <= 448)).all() and (e[~nz] == 0).all() and int((~nz).sum()) == 1
    assert (torch.ldexp(a[nz], -(e[nz].to(torch.int32) - 1)) > 448).all()            # e is the smallest exponent that fits
    assert not (codes & 0x7F == 0x7F).any()                                          # no NaN code
    v = kvq_ref.dequantize(codes, e, H)
    assert torch.equal(v.bfloat16().float(), v) and torch.isfinite(v).all()          # exact in bf16, hence in fp32
    assert torch.equal(v[7, D:2 * D], torch.zeros(D))
    # requantising the dequantised values gives the same codes: the format is a fixed point
    c2, e2 = kvq_ref.quantize(v, H)
    assert torch.equal(kvq_ref.dequantize(c2, e2, H), v)
    # e4m3 keeps 3 mantissa bits: relative error at most 2^-4 on elements that stay normal (|scaled| >= 2^-6)
    big = x.float().abs() >= torch.ldexp(torch.tensor(2.0 ** -6), e.to(torch.int32)).repeat_interleave(D, dim=1)
    rel = ((v - x.float()).abs() / x.float().abs().clamp_min(1e-30))[big]
    assert rel.max() <= 2.0 ** -4
    k, vv = kvq_ref.dequantize_row(*kvq_ref.quantize_row(x, x.flip(0), H), H)
    assert torch.equal(k, v) and torch.equal(vv, kvq_ref.dequantize(*kvq_ref.quantize(x.flip(0), H), H))


def test_restatement_boundary_of_the_mantissa():
    """m = 0.875 exactly (a = 448 * 2^k) takes e = X - 9 and the top code; one ulp above takes e = X - 8."""
    for k in (-30, -3, 0, 5, 40):
        for dtype, ulp in ((torch.float32, 2.0 ** -23), (torch.bfloat16, 2.0 ** -7)):
            at = torch.tensor([[448.0 * 2.0 ** k, 1.0 * 2.0 ** k]]).to(dtype)
            above = torch.tensor([[448.0 * 2.0 ** k * (1 + ulp * 4 / 7), 1.0 * 2.0 ** k]]).to(dtype)
            assert above[0, 0].float() > at[0, 0].float()
            c, e = kvq_ref.quantize(at, 1)
            assert int(e) == k and c[0, 0] == 0x7E and kvq_ref.dequantize(c, e, 1)[0, 0] == at[0, 0].float()
            c, e = kvq_ref.quantize(above, 1)
            assert int(e) == k + 1 and c[0, 0] == 0x76                                  # 224 * 2^(k+1) after rounding to even
    z = torch.zeros(1, 16)
    c, e = kvq_ref.quantize(z, 1)
    assert int(e) == 0 and not c.any()
    tiny, huge = torch.full((1, 16), 2.0 ** -140), torch.full((1, 16), 2.0 ** 127)
    assert int(kvq_ref.exponents(tiny, 1)) == -120 and int(kvq_ref.exponents(huge, 1)) == 119


def test_restatement_attention_matches_softmax():
    g = torch.Generator().manual_seed(0)
    B, H, D, S = 2, 2, 16, 7
    q, kn, vn = (torch.randn(B, H * D, generator=g) for _ in range(3))
    kc, vc = torch.randn(B, S, H * D, generator=g), torch.randn(B, S, H * D, generator=g)
    ok = torch.rand(B, S, generator=g) > 0.4
    ok[1] = False
    out = kvq_ref.attention(q, kc, vc, ok, kn, vn, H)
    assert torch.allclose(out[1], vn[1].double())                  # every cached key masked: the new value row
    from decode_ref import attn_decode_ref
    full_k, full_v = torch.cat([kc, kn[:, None]], 1), torch.cat([vc, vn[:, None]], 1)
    ref = attn_decode_ref(q, full_k, full_v, torch.cat([ok, torch.ones(B, 1, dtype=torch.bool)], 1), H)
    assert torch.allclose(out, ref.double(), atol=1e-5)
