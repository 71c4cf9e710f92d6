"""CPU: the sampling surface without a GPU -- the yardstick of the GPU tests itself (tests/sample_ref.py's fp64 restatement of the
mmgl_sample_tokens contract against transformers' Temperature / TopK / TopP logits warpers), the symbol and its argument validation,
and the refusals of the three generate() methods and of ops.sample_tokens that need no device."""
import os

import numpy as np
import pytest
import torch

from helpers import mpt_args, tiny_clip_vision_config, tiny_opt_config, tiny_roberta_config
from sample_ref import scaled, warp_row

SETTINGS = [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.0, 0, 0.9), (0.8, 50, 0.95), (1.3, 8, 0.5)]


# ------------------------------------------------------------------------------------------ the restatement against transformers
# top-p alone at V = 50272 is left out: nearly every row has a token within 1e-5 of the boundary, nothing could be compared
HF_CASES = [(V, sigma, T, k, p) for V in (128, 1003, 50272) for sigma in (1.0, 3.0) for (T, k, p) in SETTINGS
            if not (V == 50272 and k == 0 and p < 1.0)]


@pytest.mark.parametrize("V,sigma,T,k,p", HF_CASES)
def test_restatement_agrees_with_transformers(V, sigma, T, k, p):
    """The kept set of sample_ref.warp_row equals the set transformers' warpers leave finite, on every row where no survivor's
    mass-above lies within 1e-5 of top_p (there the two sides' fp32 / fp64 cumulative sums may fall on different sides).  Continuous
    logits: no ties.  V = 50272 with top-p alone has so many tokens within 1e-5 of the boundary that it cannot be compared."""
    from transformers import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    rows = 16
    g = torch.Generator().manual_seed(1000 + V + int(10 * sigma))
    logits = torch.randn(rows, V, generator=g) * sigma
    scores = logits.clone()
    if T != 1.0:
        scores = TemperatureLogitsWarper(T)(None, scores)
    if k > 0:
        scores = TopKLogitsWarper(k)(None, scores)
    if p < 1.0:
        scores = TopPLogitsWarper(p)(None, scores)
    hf_kept = torch.isfinite(scores).numpy()
    x = scaled(logits, T)
    clear = 0
    for r in range(rows):
        surv, above, kept = warp_row(x[r], k, p)
        if p < 1.0 and bool((surv & (np.abs(above - p) <= 1e-5)).any()):
            continue
        clear += 1
        assert np.array_equal(kept, hf_kept[r]), f"row {r}: {int(kept.sum())} kept, transformers keeps {int(hf_kept[r].sum())}"
    print(f"V={V} sigma={sigma} T={T} k={k} p={p}: {clear} of {rows} rows clear, all equal to transformers")
    assert clear >= 13, f"only {clear} of {rows} rows are clear: the comparison shows too little"


def test_restatement_ties_and_draw():
    """Ties at the k-th value and at the top-p boundary are all kept; the draw walks the kept set in index order."""
    from sample_ref import cdf, draw_ok, top_set
    x = np.array([0.0, 2.0, 1.0, 2.0, 1.0, 1.0, -1.0, 0.0])
    surv, above, kept = warp_row(x, 3, 1.0)                     # the 3rd largest is 1.0: all three 1.0s survive
    assert kept.tolist() == [False, True, True, True, True, True, False, False] and np.array_equal(surv, kept)
    z = 2 * np.exp(2.0) + 3 * np.exp(1.0) + 2 * np.exp(0.0) + np.exp(-1.0)
    surv, above, kept = warp_row(x, 0, 2 * np.exp(2.0) / z + 1e-9)      # the boundary falls on the group of 1.0s: all in, the 0.0s out
    assert kept.tolist() == [False, True, True, True, True, True, False, False]
    assert abs(above[2] - 2 * np.exp(2.0) / z) < 1e-12 and above[1] == 0.0
    surv, above, kept = warp_row(x, 0, 1e-6)                    # the largest logit is always kept, with its tie
    assert kept.tolist() == [False, True, False, True, False, False, False, False]
    mask, whole = top_set(x, 5)
    assert np.array_equal(mask, kept | (x == 1.0)) and whole and not top_set(x, 4)[1]
    c = cdf(x, kept)
    assert draw_ok(c, kept, 0.0, 1, 0.0) and draw_ok(c, kept, 0.49, 1, 0.0) and draw_ok(c, kept, 0.5, 3, 0.0)
    assert not draw_ok(c, kept, 0.5, 1, 0.0) and not draw_ok(c, kept, 0.2, 2, 1.0)


# ------------------------------------------------------------------------------------------ the symbol
def test_sample_tokens_symbol_and_argument_validation():
    from mmgl_amd import _lib
    L = _lib.lib()
    assert L.mmgl_version() == _lib.ABI_VERSION
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "mmgl_hip.h")).read()
    assert "mmgl_sample_tokens" in _lib.SIGNATURES and hasattr(L, "mmgl_sample_tokens") and "int mmgl_sample_tokens(" in header

    def call(V=128, n_draws=1, T=1.0, k=0, p=1.0, dtype=1, ld=None, stride=1, rows=2, ptrs=64):
        # (logits, ld, u, tokens, token_stride, finished, kept, rows, n_draws, V, temperature, top_k, top_p, eos, pad, dtype, stream);
        # a non-null address that is never dereferenced: every check below fails before a launch
        return L.mmgl_sample_tokens(ptrs, V if ld is None else ld, ptrs, ptrs, stride, None, None, rows, n_draws, V, T, k, p, -1, 0, dtype, None)

    assert call(ptrs=None) == 1 and b"null" in L.mmgl_last_error()
    assert call(V=131073) == 2 and call(n_draws=9) == 2
    assert call(T=0.0) == 1 and b"temperature" in L.mmgl_last_error()
    assert call(T=float("inf")) == 1 and call(T=float("nan")) == 1 and call(T=-1.0) == 1
    assert call(p=0.0) == 1 and b"top_p" in L.mmgl_last_error()
    assert call(p=1.5) == 1 and call(p=float("nan")) == 1
    assert call(k=-1) == 1 and call(dtype=7) == 1 and call(ld=100) == 1 and call(stride=0) == 1 and call(rows=0) == 1 and call(n_draws=0) == 1


def test_ops_sample_tokens_has_no_cpu_path():
    from mmgl_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sample_tokens(torch.zeros(2, 64), torch.zeros(2, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sample_tokens(torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(2), temperature=0.7, top_k=5, top_p=0.9)


# ------------------------------------------------------------------------------------------ generate()'s refusals
def _mpt():
    from mmgl_amd.model.modelling_cross_attention import MPTConfig, MPTForCausalLM
    return MPTForCausalLM(MPTConfig(mpt_args(neighbor_mode="raw", peft_type="none"), tiny_opt_config(dropout=0.0))).eval()


def _self_wrapper():
    from mmgl_amd.model import SelfAttentionModel
    args = mpt_args(neighbor_mode="raw", context="text_only", model_name_or_path="opt-tiny", peft_type="none")
    return SelfAttentionModel(args, None, lm_config=tiny_opt_config(dropout=0.0), text_config=tiny_roberta_config(),
                              visual_config=tiny_clip_vision_config()).eval()


def _cross_wrapper():
    from mmgl_amd.model import CrossAttentionModel
    return CrossAttentionModel(mpt_args(context="all"), tokenizer=None, lm_config=tiny_opt_config(dropout=0.0),
                               text_config=tiny_roberta_config(), visual_config=tiny_clip_vision_config()).eval()


def _llama():
    from transformers import LlamaConfig
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    cfg = LlamaConfig(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=4, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=256, pad_token_id=1, bos_token_id=2, eos_token_id=2,
                      attention_dropout=0.0)
    return LlamaNeighborLM(mpt_args(model_name_or_path="llama-tiny", neighbor_layer_wise=2), cfg).eval()


@pytest.mark.parametrize("make", [_mpt, _cross_wrapper, _self_wrapper, _llama])
def test_generate_sampling_refusals_without_a_device(make):
    m = make()
    ids = torch.randint(3, 128, (2, 6))
    mask = torch.ones_like(ids)
    for knob in (dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9), dict(seed=3), dict(sample_u=torch.zeros(4, 2))):
        with pytest.raises(ValueError, match="do_sample"):      # a knob without do_sample would be silently ignored
            m.generate(ids, mask, max_new_tokens=4, **knob)
    for bad in (dict(temperature=0.0), dict(temperature=float("inf")), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            m.generate(ids, mask, max_new_tokens=4, do_sample=True, **bad)
    with pytest.raises(ValueError, match="not both"):
        m.generate(ids, mask, max_new_tokens=4, do_sample=True, seed=1, sample_u=torch.zeros(4, 2))
    with pytest.raises(ValueError, match="num_beams"):          # sampling with beams
        m.generate(ids, mask, max_new_tokens=4, do_sample=True, num_beams=2)
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.generate(ids, mask, max_new_tokens=4, num_return_sequences=2)                         # greedy
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.generate(ids, mask, max_new_tokens=4, do_sample=True, num_return_sequences=9)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.generate(ids, mask, max_new_tokens=4, do_sample=True, top_k=5)


def test_num_return_sequences_outside_its_conditions():
    ids = torch.randint(3, 128, (2, 6))
    mask = torch.ones_like(ids)
    for make in (_self_wrapper, _llama):                        # R > 1 needs the beam-shared cache of the OPT fork
        with pytest.raises(ValueError, match="num_return_sequences"):
            make().generate(ids, mask, max_new_tokens=4, do_sample=True, num_return_sequences=2)
    m = _mpt()
    with pytest.raises(ValueError, match="inputs_embeds"):
        m.generate(inputs_embeds=torch.zeros(2, 6, 64), attention_mask=mask, max_new_tokens=4, do_sample=True, num_return_sequences=2)
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.generate(ids, mask, max_new_tokens=4, num_beams=2, num_return_sequences=2)
    with pytest.raises(RuntimeError, match="no CPU path"):      # inside its conditions only the device is missing
        m.generate(ids, mask, max_new_tokens=4, do_sample=True, num_return_sequences=2)


def test_arguments_default_to_greedy():
    from mmgl_amd.language_modelling.run_generation import Arguments
    a = Arguments()
    assert a.do_sample is False and a.temperature == 1.0 and a.top_k == 0 and a.top_p == 1.0 and a.num_beams == 1
