"""CPU: FP8 frozen weights -- the format as tests/w8_ref.py states it, the two exports and their refusals (nothing is
launched), and the weight_dtype keyword of the three generate() that take it.

Format bounds.  With s = 2^e the row's scale, a code is the e4m3 rounding of w / s: normal codes (|w| >= 2^-6 s) carry 3 mantissa bits,
so |deq - w| <= 2^-4 |w| (half an ulp); below 2^-6 s the codes are subnormal with step 2^-9 s, so |deq - w| <= 2^-10 s."""
import inspect

import pytest
import torch

import w8_ref
from helpers import mpt_args, tiny_opt_config

P = 64        # a non-null, 16-byte aligned address that is never dereferenced


def _rows(dtype):
    g = torch.Generator().manual_seed(11)
    w = torch.randn(24, 200, generator=g) * torch.logspace(-3, 3, 24)[:, None]
    w[:, ::7] *= 2.0 ** -9                                   # values deep in the subnormal codes of their row
    names, edges = w8_ref.edge_rows(200, dtype)
    return torch.cat([w.to(dtype), edges]), names


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_format_bounds_and_fixed_point(dtype):
    w, names = _rows(dtype)
    codes, exps = w8_ref.quantize(w)
    assert codes.dtype == torch.uint8 and codes.shape == w.shape and exps.dtype == torch.int8 and exps.shape == (w.shape[0],)
    deq = w8_ref.dequantize(codes, exps)
    assert torch.isfinite(deq).all()
    assert torch.equal(deq.to(torch.bfloat16).float(), deq), "a dequantised value is not exact in bf16"
    wf = w.float().double()
    s = torch.ldexp(torch.ones(w.shape[0], dtype=torch.float64), exps.to(torch.int32))[:, None]
    err = (deq.double() - wf).abs()
    normal = wf.abs() >= 2.0 ** -6 * s
    assert (err[normal] <= 2.0 ** -4 * wf.abs()[normal]).all()
    assert (err[~normal] <= (2.0 ** -10 * s).expand_as(err)[~normal]).all()
    assert (~normal).sum() > 100 and normal.sum() > 1000      # both regimes are visited
    # nothing saturates: the scaled maximum is at most 448, and above 224 unless the row is zero or its exponent clamped
    scaled = (wf.abs() / s).amax(1)
    assert (scaled <= 448).all()
    free = (wf.abs().amax(1) > 0) & (exps.abs() < 120)
    assert (scaled[free] > 224).all()
    # quantising a dequantised row gives the same values again (not always the same codes: a maximum that rounded down to 224 * 2^e
    # is 448 * 2^(e-1) of the second pass)
    c2, e2 = w8_ref.quantize(deq)
    assert torch.equal(w8_ref.dequantize(c2, e2), deq)
    assert ((e2 == exps) | (e2 == exps - 1)).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_edge_rows(dtype):
    names, rows = w8_ref.edge_rows(72, dtype)
    codes, exps = w8_ref.quantize(rows)
    e = dict(zip(names, exps.tolist()))
    assert e["zero row"] == 0 and not codes[0].any()
    assert e["max = 448 * 2^-3"] == -3 and e["max one step above 448 * 2^-3"] == -2 and e["max = 448 (e = 0)"] == 0
    assert e["low clamp"] == -120 and e["high clamp"] == 120 and e["negative exponent"] < 0 < e["large exponent"]
    top = codes.view(w8_ref.FP8).float().abs().amax(1)
    assert top[names.index("max = 448 * 2^-3")] == 448 and top[names.index("max one step above 448 * 2^-3")] == 224
    assert top[names.index("low clamp")] == 32               # 2^-115 * 2^120: the clamp leaves the row below 224
    import kvq_ref
    assert w8_ref.FP8 is kvq_ref.FP8 and torch.equal(exps.to(torch.int32), kvq_ref.exponents(rows, 1)[:, 0])      # one exponent rule


# ------------------------------------------------------------------------------------------ the exports
def test_the_exports_are_declared_and_bound_at_abi_110():
    import os
    from mmgl_amd import _lib
    assert _lib.ABI_VERSION == 110 and _lib.lib().mmgl_version() == 110
    header = open(os.path.join(os.path.dirname(_lib.__file__), os.pardir, "include", "mmgl_hip.h")).read()
    for name, n_args in (("mmgl_weight_quantize", 9), ("mmgl_gemm_skinny_w8", 16)):
        assert f"int {name}(" in header and len(_lib.SIGNATURES[name][1]) == n_args
        assert getattr(_lib.lib(), name).argtypes == _lib.SIGNATURES[name][1]


QUANT = dict(w=P, ldw=64, codes=P, ldc=64, exps=P, N=8, K=64, dtype=1)
GEMM = dict(x=P, ldx=64, codes=P, ldc=64, exps=P, bias=None, residual=None, y=P, ldy=64, M=4, N=64, K=64, act=0, scale=1.0, dtype=1)
ENTRY = {
    "mmgl_weight_quantize": (QUANT, "w ldw codes ldc exps N K dtype"),
    "mmgl_gemm_skinny_w8": (GEMM, "x ldx codes ldc exps bias residual y ldy M N K act scale dtype"),
}
# (entry point, the one condition violated, the arguments changed for it, return code, mmgl_last_error())
REFUSALS = [
    ("mmgl_weight_quantize", "sizes N", dict(N=0), 1, "mmgl_weight_quantize: bad sizes N=0 K=64"),
    ("mmgl_weight_quantize", "sizes K", dict(K=0), 1, "mmgl_weight_quantize: bad sizes N=8 K=0"),
    ("mmgl_weight_quantize", "dtype", dict(dtype=7), 1, "mmgl_weight_quantize: bad dtype 7"),
    ("mmgl_weight_quantize", "null w", dict(w=None), 1, "mmgl_weight_quantize: null pointer"),
    ("mmgl_weight_quantize", "null codes", dict(codes=None), 1, "mmgl_weight_quantize: null pointer"),
    ("mmgl_weight_quantize", "null exps", dict(exps=None), 1, "mmgl_weight_quantize: null pointer"),
    ("mmgl_weight_quantize", "ldw", dict(ldw=63), 1, "mmgl_weight_quantize: leading dimensions (63, 64) smaller than the rows (K=64)"),
    ("mmgl_weight_quantize", "ld_codes", dict(ldc=63), 1, "mmgl_weight_quantize: leading dimensions (64, 63) smaller than the rows (K=64)"),
    ("mmgl_gemm_skinny_w8", "sizes", dict(M=0), 1, "mmgl_gemm_skinny_w8: bad sizes M=0 N=64 K=64"),
    ("mmgl_gemm_skinny_w8", "M = 65", dict(M=65), 2, "mmgl_gemm_skinny_w8: M=65 > 64 rows (chunk the rows)"),
    ("mmgl_gemm_skinny_w8", "dtype", dict(dtype=7), 1, "mmgl_gemm_skinny_w8: bad dtype 7"),
    ("mmgl_gemm_skinny_w8", "null x", dict(x=None), 1, "mmgl_gemm_skinny_w8: null pointer"),
    ("mmgl_gemm_skinny_w8", "null codes", dict(codes=None), 1, "mmgl_gemm_skinny_w8: null pointer"),
    ("mmgl_gemm_skinny_w8", "null exps", dict(exps=None), 1, "mmgl_gemm_skinny_w8: null pointer"),
    ("mmgl_gemm_skinny_w8", "null y", dict(y=None), 1, "mmgl_gemm_skinny_w8: null pointer"),
    ("mmgl_gemm_skinny_w8", "activation", dict(act=5), 1, "mmgl_gemm_skinny_w8: unknown activation 5"),
    ("mmgl_gemm_skinny_w8", "ldx", dict(ldx=63), 1, "mmgl_gemm_skinny_w8: leading dimensions (63, 64, 64) smaller than the rows (K=64, N=64)"),
    ("mmgl_gemm_skinny_w8", "ld_codes", dict(ldc=63), 1, "mmgl_gemm_skinny_w8: leading dimensions (64, 63, 64) smaller than the rows (K=64, N=64)"),
    ("mmgl_gemm_skinny_w8", "ldy", dict(ldy=63), 1, "mmgl_gemm_skinny_w8: leading dimensions (64, 64, 63) smaller than the rows (K=64, N=64)"),
]


@pytest.mark.parametrize("fn,what,change,code,text", REFUSALS, ids=[f"{r[0]}-{r[1]}" for r in REFUSALS])
def test_entry_point_refuses(fn, what, change, code, text):
    if torch.cuda.is_available():
        pytest.skip("runs where no GPU is visible: a missing check would launch on a made-up address")
    from mmgl_amd import _lib
    L = _lib.lib()
    valid, order = ENTRY[fn]
    assert set(change) <= set(valid)
    args = dict(valid, **change)
    assert getattr(L, fn)(*[args[name] for name in order.split()], None) == code
    assert L.mmgl_last_error().decode() == text


def test_ops_have_no_cpu_path_and_check_their_operands():
    from mmgl_amd import ops
    w, x = torch.randn(16, 64), torch.randn(3, 64)
    codes, exps = w8_ref.quantize(w)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.quantize_weight_fp8(w)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.decode_linear_w8(x, codes.view(w8_ref.FP8), exps)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.gemm_skinny_w8(x, codes, exps)
    for bad in (dict(codes=codes[:, :32]), dict(exps=exps[:8]), dict(exps=exps.to(torch.int32)), dict(codes=codes.float())):
        kw = dict(dict(codes=codes, exps=exps), **bad)
        with pytest.raises(ValueError, match="decode_linear_w8: shapes"):
            ops._w8_operands("decode_linear_w8", x, kw["codes"], kw["exps"])
    assert list(inspect.signature(ops.decode_linear_w8).parameters) == ["x", "codes", "exps", "bias", "act", "out_scale", "residual", "out"]
    assert list(inspect.signature(ops.decode_linear).parameters) == ["x", "weight", "bias", "act", "out_scale", "residual", "out"]


# ------------------------------------------------------------------------------------------ the keyword
def _llama():
    from transformers import LlamaConfig
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=4, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=256, pad_token_id=1, bos_token_id=2, eos_token_id=2, attention_dropout=0.0)
    return LlamaNeighborLM(mpt_args(model_name_or_path="llama-tiny", neighbor_layer_wise=2), cfg).eval()


def _fork():
    from mmgl_amd.model.modelling_cross_attention import MPTConfig, MPTForCausalLM
    torch.manual_seed(0)
    return MPTForCausalLM(MPTConfig(mpt_args(neighbor_mode="raw", peft_type="none"), tiny_opt_config(dropout=0.0))).eval()


def _call(model, **kw):
    ids = torch.randint(3, 128, (2, 6))
    return model.generate(ids, torch.ones_like(ids), max_new_tokens=4, **kw)


def test_where_the_keyword_is_named():
    from mmgl_amd.model import CrossAttentionModel, SelfAttentionModel
    from mmgl_amd.model.modelling_cross_attention import MPTForCausalLM
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    for cls in (MPTForCausalLM, CrossAttentionModel):
        p = inspect.signature(cls.generate).parameters
        assert p["weight_dtype"].default is None and p["weight_dtype"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    llama = inspect.signature(LlamaNeighborLM.generate).parameters
    assert "weight_dtype" not in llama and llama["lookup"].kind is inspect.Parameter.VAR_KEYWORD
    assert "weight_dtype" not in inspect.signature(SelfAttentionModel.generate).parameters
    from mmgl_amd.language_modelling.run_generation import Arguments
    assert Arguments.__dataclass_fields__["weight_dtype"].default is None


def test_llama_takes_the_keyword_through_the_catch_all():
    lm = _llama()
    with pytest.raises(TypeError, match="unexpected keyword argument 'foo'"):
        _call(lm, foo=1)
    with pytest.raises(TypeError, match="unexpected keyword argument 'foo'"):
        _call(lm, weight_dtype="fp8", foo=1)
    for bad, shown in (("int8", "'int8'"), (torch.bfloat16, r"torch\.bfloat16"), ("bf16", "'bf16'")):
        with pytest.raises(ValueError, match=rf"LlamaNeighborLM\.generate\(\): weight_dtype = {shown} is unknown"):
            _call(lm, weight_dtype=bad)
    for kw in (dict(weight_dtype=None), dict(weight_dtype="fp8"), dict(weight_dtype=torch.float8_e4m3fn),
               dict(weight_dtype="fp8", kv_cache_dtype="fp8"), dict(weight_dtype="fp8", prompt_lookup_num_tokens=3),
               dict(weight_dtype="fp8", do_sample=True, top_k=5, seed=3), dict(weight_dtype="fp8", return_step_logits=True)):
        with pytest.raises(RuntimeError, match="no CPU path"):          # accepted: the call reaches the device check
            _call(lm, **kw)
    assert all("_w8_codes" not in fr.__dict__ for fr in lm._frozen)                      # nothing was quantised on the way


@pytest.mark.parametrize("name", ["q_proj", "o_proj", "down_proj"])
def test_llama_refuses_adapted_linears(name):
    from mmgl_amd.model.modelling_self_attention import LoRALinear
    lm = _llama()
    layer = lm.llama.model.layers[1]
    holder = layer.mlp if name == "down_proj" else layer.self_attn
    setattr(holder, name, LoRALinear(getattr(holder, name), 4, 8.0))
    with pytest.raises(ValueError, match=r"weight_dtype = 'fp8' \(FP8 frozen weights\) runs plain nn\.Linear projections and FFN layers only"):
        _call(lm, weight_dtype="fp8")


def test_fork_validates_and_refuses():
    from mmgl_amd.model.modelling_self_attention import LoRALinear
    lm = _fork()
    for bad, shown in (("int8", "'int8'"), (torch.bfloat16, r"torch\.bfloat16")):
        with pytest.raises(ValueError, match=rf"generate\(\): weight_dtype = {shown} is unknown"):
            _call(lm, weight_dtype=bad)
    for kw in (dict(weight_dtype=None), dict(weight_dtype="fp8"), dict(weight_dtype=torch.float8_e4m3fn), dict(weight_dtype="fp8", num_beams=2),
               dict(weight_dtype="fp8", kv_cache_dtype="fp8"), dict(weight_dtype="fp8", prompt_lookup_num_tokens=3),
               dict(weight_dtype="fp8", penalty_alpha=0.6, top_k=4), dict(weight_dtype="fp8", do_sample=True, num_return_sequences=2, seed=1)):
        with pytest.raises(RuntimeError, match="no CPU path|GPU only"):
            _call(lm, **kw)
    for holder, name in ((lm.model.decoder.layers[1].self_attn, "v_proj"), (lm.model.decoder.layers[0], "fc1")):
        plain = getattr(holder, name)
        setattr(holder, name, LoRALinear(plain, 4, 8.0))
        with pytest.raises(ValueError, match=r"weight_dtype = 'fp8' \(FP8 frozen weights\) runs plain nn\.Linear"):
            _call(lm, weight_dtype="fp8")
        setattr(holder, name, plain)


def test_wrapper_validates_and_refuses():
    """CrossAttentionModel.generate checks the keyword itself, in front of the neighbor encoders."""
    from helpers import tiny_clip_vision_config, tiny_roberta_config
    from mmgl_amd.model import CrossAttentionModel
    from mmgl_amd.model.modelling_self_attention import LoRALinear
    torch.manual_seed(0)
    w = CrossAttentionModel(mpt_args(context="all"), tokenizer=None, lm_config=tiny_opt_config(dropout=0.0), text_config=tiny_roberta_config(),
                            visual_config=tiny_clip_vision_config()).eval()
    encoded = []
    w._neighbor_tokens = lambda *a, **kw: encoded.append(1)
    for bad, shown in (("int8", "'int8'"), (torch.bfloat16, r"torch\.bfloat16")):
        with pytest.raises(ValueError, match=rf"generate\(\): weight_dtype = {shown} is unknown"):
            _call(w, weight_dtype=bad)
    for kw in (dict(weight_dtype=None), dict(weight_dtype="fp8"), dict(weight_dtype=torch.float8_e4m3fn), dict(weight_dtype="fp8", num_beams=2),
               dict(weight_dtype="fp8", guidance_scale=None)):
        with pytest.raises(RuntimeError, match="GPU only"):            # accepted: the call reaches the device check
            _call(w, **kw)
    dec = w.lm.model.decoder
    for holder, name in ((dec.layers[1].self_attn, "q_proj"), (dec.layers[2].self_attn, "out_proj"), (dec.layers[0], "fc2")):
        plain = getattr(holder, name)
        setattr(holder, name, LoRALinear(plain, 4, 8.0))
        with pytest.raises(ValueError, match=r"weight_dtype = 'fp8' \(FP8 frozen weights\) runs plain nn\.Linear"):
            _call(w, weight_dtype="fp8")
        setattr(holder, name, plain)
    gated = dec.neighbor_layers[0]                                       # a gated layer is not quantised: its adapters are not the keyword's business
    gated.fc1 = LoRALinear(gated.fc1, 4, 8.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        _call(w, weight_dtype="fp8")
    assert not encoded, "the neighbor encoders ran before the keyword was checked"


def test_check_weight_dtype():
    from mmgl_amd import ops
    from mmgl_amd.model.sampling import check_weight_dtype
    lin = torch.nn.Linear(4, 4)
    assert check_weight_dtype("generate()", None, [object()]) is None          # off: nothing is looked at
    assert check_weight_dtype("generate()", "fp8", [lin]) is ops.KV_FP8 and check_weight_dtype("generate()", torch.float8_e4m3fn) is ops.KV_FP8
    with pytest.raises(ValueError, match="is unknown: None"):
        check_weight_dtype("generate()", "FP8")
    with pytest.raises(ValueError, match="plain nn.Linear"):
        check_weight_dtype("generate()", "fp8", [lin, torch.nn.Sequential(lin)])
