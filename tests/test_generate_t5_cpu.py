"""CPU side of generate() for a T5 (T5HipRunner.generate, ops.attn_decode_relbias; no GPU here): the new symbol in the header and the
binding, its refusals before any launch, the bias rows against transformers' compute_bias bitwise, the fp64 reference
(tests/t5_decode_ref.py) against transformers' T5Attention, that the reference can tell three wrong kernels from the right one on the
kernel test's main case, and the wrapper's decisions (can_generate() unchanged, can_generate_seq2seq(), the refusals of generate())."""
import ctypes
import os
import re

import pytest
import torch
from transformers import T5Config, T5ForConditionalGeneration
from transformers.models.t5.modeling_t5 import T5Attention

import t5_decode_ref as R
from helpers import mpt_args, tiny_clip_vision_config, tiny_opt_config, tiny_roberta_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mmgl_attn_decode_relbias_fwd"


def _cfg(**kw):
    base = dict(vocab_size=128, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, dropout_rate=0.0,
                decoder_start_token_id=0, pad_token_id=0, eos_token_id=1)
    base.update(kw)
    return T5Config(**base)


def test_symbol_declared_bound_and_version_110():
    from mmgl_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmgl_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint %s\s*\(" % NAME, text), f"{NAME} is not declared in include/mmgl_hip.h"
    # the signature of mmgl_attn_decode_fwd: the bias rows and their pitch stand where the mask and its pitch do
    assert _lib.SIGNATURES[NAME] == _lib.SIGNATURES["mmgl_attn_decode_fwd"]
    assert hasattr(_lib.lib(), NAME)
    assert _lib.ABI_VERSION == 110 and _lib.lib().mmgl_version() == 110


def test_refused_before_any_launch():
    from mmgl_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(256)                # never dereferenced: every check below fails on the host
    # (q, ldq, k, v, ldkv, batch_stride_kv, bias, ld_bias, out, B, H, S, D, dtype, stream)
    call = lambda ldq=128, ldkv=256, bs=2560, ld_bias=10, H=2, S=10, D=64, dtype=_lib.BF16, bias=p: getattr(L, NAME)(
        p, ldq, p, p, ldkv, bs, bias, ld_bias, p, 2, H, S, D, dtype, None)
    assert call(ldq=96, ldkv=192, bs=1920, D=48) == _lib._ERR_UNSUPPORTED           # head_dim 48
    assert b"head_dim 48" in L.mmgl_last_error()
    assert call(ldq=120) == _lib._ERR_INVALID                                       # pitch below H * D
    assert call(ldkv=120) == _lib._ERR_INVALID
    assert call(ld_bias=9) == _lib._ERR_INVALID                                     # ld_bias < S
    assert b"smaller than the rows" in L.mmgl_last_error()
    assert call(S=0) == _lib._ERR_INVALID
    assert call(ldkv=260, bs=2600) == _lib._ERR_UNSUPPORTED                         # rows no multiples of 16 bytes
    assert call(bias=None) == _lib._ERR_INVALID
    assert call(bias=ctypes.c_void_p(258)) == _lib._ERR_UNSUPPORTED                 # bias not 4-byte aligned
    assert call(dtype=7) == _lib._ERR_INVALID


@pytest.mark.parametrize("S", [1, 16, 17, 33, 128, 129, 200])        # both sides of the exact / log boundary (16) and of max_distance (128)
def test_decode_bias_rows_are_compute_bias_reversed_bitwise(S):
    from mmgl_amd import ops
    cfg = _cfg(is_decoder=True, num_heads=3, d_model=192)
    torch.manual_seed(S)
    att = T5Attention(cfg, has_relative_attention_bias=True, layer_idx=0)
    want = att.compute_bias(S, S)[0, :, -1, :].flip(-1)               # [H, S]: the last query's row, by distance
    got = ops.t5_decode_bias(att.relative_attention_bias.weight, S, cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, S) and got.stride() == (S, 1) and not got.requires_grad
    assert torch.equal(got, want.detach())
    if S > 1:                                                         # a longer cache has the shorter one's rows in front
        assert torch.equal(got[:, :S - 1], ops.t5_decode_bias(att.relative_attention_bias.weight, S - 1, cfg.relative_attention_num_buckets,
                                                              cfg.relative_attention_max_distance))


@pytest.mark.parametrize("S", [1, 17, 140])
def test_reference_is_transformers_attention_in_fp64(S):
    """The last row of an uncached T5Attention call attends every key (no mask is needed for it): what a cached call computes."""
    from mmgl_amd import ops
    cfg = _cfg(is_decoder=True, num_heads=3, d_model=96)
    torch.manual_seed(S)
    att = T5Attention(cfg, has_relative_attention_bias=True, layer_idx=0).double().eval()
    with torch.no_grad():
        att.relative_attention_bias.weight.normal_(0, 2.0)
        hidden = torch.randn(2, S, cfg.d_model, dtype=torch.float64)
        want = att(hidden)[0][:, -1]
        bias = ops.t5_decode_bias(att.relative_attention_bias.weight, S + 3, cfg.relative_attention_num_buckets,
                                  cfg.relative_attention_max_distance)
        got = att.o(R.attn_decode_relbias_ref(att.q(hidden[:, -1]), att.k(hidden), att.v(hidden), bias, cfg.num_heads))
    # the bias rows are fp32 (what the kernel reads): 2^-24 relative on a word of magnitude <= 8
    assert (got - want).abs().max().item() <= 1e-5 * want.abs().max().item()
    with torch.no_grad():
        exact = att.o(R.attn_decode_relbias_ref(att.q(hidden[:, -1]), att.k(hidden), att.v(hidden),
                                                att.compute_bias(S, S)[0, :, -1, :].flip(-1), cfg.num_heads))
    assert (exact - want).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1.0)


@pytest.mark.parametrize("wrong", R.WRONG)
def test_reference_tells_wrong_kernels_apart_on_the_main_case(wrong):
    """Each deliberately wrong reference leaves the bf16 tolerance on EVERY sample of the kernel test's main case."""
    S, q, cache, bias, _ = R.main_case()
    k, v = R.slabs(cache, S, q.shape[1])
    want = R.attn_decode_relbias_ref(q, k, v, bias, 2)
    gap = R.per_sample(R.attn_decode_relbias_ref(q, k, v, bias, 2, wrong), want)
    assert (gap > R.TOL[R.BF16]).all(), f"{wrong}: {gap.tolist()}"


def _wrapper(**kw):
    from mmgl_amd.model import SelfAttentionModel
    name = kw.pop("name", "t5-tiny")
    lm_config = kw.pop("lm_config", None) or _cfg()
    kw.setdefault("decoder_only", name != "t5-tiny")
    args = mpt_args(neighbor_mode="raw", context="text_only", model_name_or_path=name, **kw)
    return SelfAttentionModel(args, None, lm_config=lm_config, text_config=tiny_roberta_config(), visual_config=tiny_clip_vision_config()).eval()


def test_can_generate_stays_false_and_seq2seq_truth_table():
    plain = _wrapper(peft_type="none")
    assert plain.can_generate() is False
    assert plain.can_generate_seq2seq() is True
    assert _wrapper(peft_type="none", lm_config=_cfg(tie_word_embeddings=False)).can_generate_seq2seq() is True
    assert _wrapper(peft_type="none", lm_config=_cfg(feed_forward_proj="gated-gelu")).can_generate_seq2seq() is False
    assert _wrapper(peft_type="none", lm_config=_cfg(d_kv=32)).can_generate_seq2seq() is False
    lora = _wrapper(peft_type="lora")
    assert lora.can_generate_seq2seq() is False and lora.can_generate() is False
    opt = _wrapper(name="opt-tiny", lm_config=tiny_opt_config(dropout=0.0), peft_type="none")
    assert opt.can_generate_seq2seq() is False and opt.can_generate() is True
    assert "_t5_runner" not in plain.__dict__                          # decided without building a runner


def test_generate_refusals():
    from mmgl_amd.model.t5_hip import T5HipRunner
    model = _wrapper(peft_type="none")
    ids = torch.randint(3, 128, (2, 6))
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.generate(ids, torch.ones_like(ids), max_new_tokens=4)
    with pytest.raises(ValueError, match="num_beams"):
        model.generate(ids, torch.ones_like(ids), max_new_tokens=4, num_beams=2)
    runner = T5HipRunner(model.lm)
    with pytest.raises(RuntimeError, match="no CPU path"):
        runner.generate(input_ids=ids, max_new_tokens=4)
    with pytest.raises(ValueError, match="num_beams"):
        runner.generate(input_ids=ids, max_new_tokens=4, num_beams=2)
    with pytest.raises(ValueError, match="num_return_sequences"):
        runner.generate(input_ids=ids, max_new_tokens=4, num_return_sequences=2)
    with pytest.raises(ValueError, match="num_return_sequences"):
        runner.generate(input_ids=ids, max_new_tokens=4, do_sample=True, num_return_sequences=2)
    with pytest.raises(ValueError, match="exactly one"):
        runner.generate(max_new_tokens=4)
    with pytest.raises(ValueError):
        T5HipRunner(T5ForConditionalGeneration(_cfg(feed_forward_proj="gated-gelu")))
    with pytest.raises(RuntimeError, match="no CPU path"):
        from mmgl_amd import ops
        ops.attn_decode_relbias(torch.zeros(2, 128), torch.zeros(2, 3, 128), torch.zeros(2, 3, 128), torch.zeros(2, 3), 2)


def test_generate_seq2seq_flag_defaults_to_off():
    from mmgl_amd.language_modelling.run_generation import Arguments
    assert Arguments().generate_seq2seq is False
