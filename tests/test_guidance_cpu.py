"""CPU tests of neighbor guidance (generate(guidance_scale); no GPU needed):
  * sampling.check_guidance refuses, in front of the device check and in words that name guidance_scale, what is not implemented;
    None and 1.0 are off and reach the error a call without the keyword reaches;
  * mmgl_guidance_logits is declared, bound and refuses every bad argument before a launch (the method of
    tests/test_decode_refusals_cpu.py: addresses that are never dereferenced);
  * the yardstick of tests/test_guidance_kernel_gpu.py bites: guidance_ref.reference is the formula (checked against a plain-Python
    fsum evaluation and, where it imports, transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor arithmetic), and each wrong
    variant of guidance_ref.VARIANTS leaves the bf16 bound -- the looser one -- on at least 90 % of the elements, for every g of the
    GPU file at which the variant is wrong at all (g = 0.5 is symmetric in lc and lu), from the references alone."""
import math
import os

import pytest
import torch

import guidance_ref
from helpers import mpt_args, tiny_clip_vision_config, tiny_opt_config, tiny_roberta_config

G_VALUES = (0.0, 0.5, 1.5, 3.0)
SHARE = 0.90


# ------------------------------------------------------------------------------------------ the checks
def _lm(**kw):
    from mmgl_amd.model.modelling_cross_attention import MPTConfig, MPTForCausalLM
    return MPTForCausalLM(MPTConfig(mpt_args(**kw), tiny_opt_config(dropout=0.0))).eval()


def _wrapper(**kw):
    from mmgl_amd.model import CrossAttentionModel
    return CrossAttentionModel(mpt_args(**kw), tokenizer=None, lm_config=tiny_opt_config(dropout=0.0), text_config=tiny_roberta_config(),
                               visual_config=tiny_clip_vision_config()).eval()


IDS = torch.randint(3, 128, (2, 6), generator=torch.Generator().manual_seed(0))
NE = torch.zeros(2, 4, 64)

REFUSED = [
    (dict(guidance_scale=-0.5), "finite number >= 0"),
    (dict(guidance_scale=float("inf")), "finite number >= 0"),
    (dict(guidance_scale=float("nan")), "finite number >= 0"),
    (dict(guidance_scale="2"), "finite number >= 0"),
    (dict(guidance_scale=True), "finite number >= 0"),
    (dict(guidance_scale=1.5, num_beams=2), r"num_beams = 2 is not implemented"),
    (dict(guidance_scale=1.5, do_sample=True, num_return_sequences=2), r"num_return_sequences = 2 is not implemented"),
    (dict(guidance_scale=1.5, prompt_lookup_num_tokens=3), r"prompt_lookup_num_tokens = 3 is not implemented"),
    (dict(guidance_scale=1.5, penalty_alpha=0.6, top_k=4), r"penalty_alpha = 0.6 is not implemented"),
    (dict(guidance_scale=1.5, kv_cache_dtype="fp8"), r"kv_cache_dtype = 'fp8' is not implemented"),
]


@pytest.mark.parametrize("kw,text", REFUSED, ids=[",".join(f"{k}={v}" for k, v in r[0].items()) for r in REFUSED])
def test_generate_refuses_in_front_of_the_device_check(kw, text):
    """CPU tensors: a refusal that came after the device check would be the RuntimeError 'no CPU path' instead."""
    lm = _lm()
    with pytest.raises(ValueError, match="guidance_scale.*" + text):
        lm.generate(IDS, torch.ones_like(IDS), neighbor_embeds=NE, max_new_tokens=4, **kw)
    w = _wrapper()
    with pytest.raises(ValueError, match="guidance_scale.*" + text):
        w.generate(IDS, torch.ones_like(IDS), neighbor_input_ids=torch.zeros(2, 3, 4, dtype=torch.long), max_new_tokens=4, **kw)


def test_generate_refuses_embeddings_prompts_and_nothing_to_contrast():
    lm = _lm()
    with pytest.raises(ValueError, match=r"guidance_scale = 1.5 .*inputs_embeds is not implemented"):
        lm.generate(inputs_embeds=torch.zeros(2, 6, 64), neighbor_embeds=NE, max_new_tokens=4, guidance_scale=1.5)
    with pytest.raises(ValueError, match=r"guidance_scale = 1.5 .*without neighbor tokens.*not implemented: there is nothing to contrast"):
        lm.generate(IDS, torch.ones_like(IDS), max_new_tokens=4, guidance_scale=1.5)
    plain = _lm(neighbor_mode="raw", peft_type="none")                                    # a decoder without gated layers
    assert len(plain.model.decoder.neighbor_layers) == 0
    with pytest.raises(ValueError, match=r"guidance_scale = 2 .*without gated layers.*nothing to contrast"):
        plain.generate(IDS, torch.ones_like(IDS), neighbor_embeds=NE, max_new_tokens=4, guidance_scale=2)
    w = _wrapper()
    with pytest.raises(ValueError, match=r"guidance_scale = 0 .*nothing to contrast"):   # g = 0 is on: the LM without neighbors
        w.generate(IDS, torch.ones_like(IDS), max_new_tokens=4, guidance_scale=0)
    raw = _wrapper(neighbor_mode="raw", peft_type="none")
    with pytest.raises(ValueError, match=r"guidance_scale = 1.5 .*nothing to contrast"):
        raw.generate(IDS, torch.ones_like(IDS), neighbor_input_ids=torch.zeros(2, 3, 4, dtype=torch.long), max_new_tokens=4, guidance_scale=1.5)


@pytest.mark.parametrize("g", [None, 1.0, 1])
def test_off_reaches_the_error_of_a_call_without_the_keyword(g):
    lm, w = _lm(), _wrapper()
    for call in (lambda **kw: lm.generate(IDS, torch.ones_like(IDS), max_new_tokens=4, **kw),
                 lambda **kw: lm.generate(IDS, torch.ones_like(IDS), max_new_tokens=4, num_beams=2, kv_cache_dtype=None, **kw),
                 lambda **kw: w.generate(IDS, torch.ones_like(IDS), max_new_tokens=4, **kw)):
        with pytest.raises(RuntimeError, match="no CPU path") as without:
            call()
        with pytest.raises(RuntimeError, match="no CPU path") as with_g:
            call(guidance_scale=g)
        assert str(with_g.value) == str(without.value)


def test_check_guidance_returns():
    from mmgl_amd.model.sampling import check_guidance
    assert check_guidance("generate()", None) is None and check_guidance("generate()", 1.0) is None
    assert check_guidance("generate()", 0) == 0.0 and check_guidance("generate()", 2.5) == 2.5
    assert check_guidance("generate()", None, num_beams=4, kv_cache_dtype="fp8", neighbors=False) is None     # off: nothing to refuse


def test_other_generators_keep_their_signature():
    import inspect
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    from mmgl_amd.model.modelling_self_attention import SelfAttentionModel
    from mmgl_amd.model.modelling_cross_attention import CrossAttentionModel, MPTForCausalLM
    for cls in (LlamaNeighborLM, SelfAttentionModel):
        assert "guidance_scale" not in inspect.signature(cls.generate).parameters
    for cls in (CrossAttentionModel, MPTForCausalLM):
        assert inspect.signature(cls.generate).parameters["guidance_scale"].default is None


def test_arguments_and_abi():
    from mmgl_amd import _lib
    from mmgl_amd.language_modelling.run_generation import Arguments
    assert Arguments().guidance_scale == 1.0
    assert _lib.ABI_VERSION == 110 and _lib.lib().mmgl_version() == 110


def test_ops_wrapper_refuses():
    from mmgl_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.guidance_logits(torch.zeros(4, 8), 2, 1.5)


# ------------------------------------------------------------------------------------------ the entry point
P = 64        # a non-null address that is never dereferenced
VALID = dict(logits=P, ld=10, batch=2, V=10, g=1.5, dtype=1)
ORDER = "logits ld batch V g dtype"
ENTRY_REFUSALS = [
    ("null pointer", dict(logits=None), 1, "mmgl_guidance_logits: null pointer"),
    ("batch = 0", dict(batch=0), 1, "mmgl_guidance_logits: bad sizes batch=0 V=10"),
    ("batch < 0", dict(batch=-3), 1, "mmgl_guidance_logits: bad sizes batch=-3 V=10"),
    ("V = 0", dict(V=0), 1, "mmgl_guidance_logits: bad sizes batch=2 V=0"),
    ("ld < V", dict(ld=9), 1, "mmgl_guidance_logits: row stride 9 smaller than V=10"),
    ("V > 131072", dict(V=131073, ld=131073), 2, "mmgl_guidance_logits: V=131073 (at most 131072)"),
    ("dtype", dict(dtype=7), 1, "mmgl_guidance_logits: bad dtype 7"),
    ("g = nan", dict(g=float("nan")), 1, "mmgl_guidance_logits: guidance_scale nan must be finite and not negative"),
    ("g = inf", dict(g=float("inf")), 1, "mmgl_guidance_logits: guidance_scale inf must be finite and not negative"),
    ("g < 0", dict(g=-0.5), 1, "mmgl_guidance_logits: guidance_scale -0.5 must be finite and not negative"),
]


def test_symbol_is_declared_and_bound():
    from mmgl_amd import _lib
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "mmgl_hip.h")).read()
    assert "int mmgl_guidance_logits(void* logits, size_t ld_logits, int batch, int V, float guidance_scale, int dtype, void* stream);" in header
    assert "A row without any finite logit is outside the contract" in header
    assert "mmgl_guidance_logits" in _lib.SIGNATURES and hasattr(_lib.lib(), "mmgl_guidance_logits")
    assert len(_lib.SIGNATURES["mmgl_guidance_logits"][1]) == len(ORDER.split()) + 1


@pytest.mark.parametrize("what,change,code,text", ENTRY_REFUSALS, ids=[r[0] for r in ENTRY_REFUSALS])
def test_entry_point_refuses(what, change, code, text):
    if torch.cuda.is_available():
        pytest.skip("runs where no GPU is visible: a missing check would launch on a made-up address")
    from mmgl_amd import _lib
    L = _lib.lib()
    assert set(change) <= set(VALID)
    args = dict(VALID, **change)
    assert L.mmgl_guidance_logits(*[args[n] for n in ORDER.split()], None) == code
    assert L.mmgl_last_error().decode() == text


# ------------------------------------------------------------------------------------------ the yardstick
def test_reference_is_the_formula():
    B, V = 3, 37
    x = guidance_ref.kernel_inputs(B, V, torch.float32, seed=3)
    for g in G_VALUES:
        ref = guidance_ref.reference(x, B, g)["score"]
        for b in range(B):
            want = torch.tensor(guidance_ref.guided_row_python(x[b].double().tolist(), x[B + b].double().tolist(), g), dtype=torch.float64)
            assert (ref[b] - want).abs().max().item() <= 1e-12 * want.abs().max().item(), (g, b)
    # the -inf / NaN rules
    y = x.clone()
    y[0, 5] = -math.inf          # conditional -inf -> -inf
    y[B + 0, 7] = -math.inf      # unconditional -inf under a finite conditional -> lc
    y[1, 9] = math.nan           # NaN counts as -inf
    y[B + 1, 9] = -math.inf      # both -inf -> -inf
    r = guidance_ref.reference(y, B, 1.5)
    assert r["score"][0, 5] == -math.inf and r["score"][1, 9] == -math.inf
    assert r["score"][0, 7] == r["lc"][0, 7] and math.isfinite(r["score"][0, 7])
    assert torch.isfinite(r["score"]).sum() == B * V - 2
    bd = guidance_ref.bound(r, 1.5, V, torch.float32)
    assert bd[0, 5] == 0 and (bd[torch.isfinite(r["score"])] > 0).all() and torch.isfinite(bd).all()


def test_reference_is_transformers_guidance_arithmetic():
    """UnbatchedClassifierFreeGuidanceLogitsProcessor.__call__: log_softmax of both, scale * (cond - uncond) + uncond."""
    hf = pytest.importorskip("transformers.generation.logits_process")
    cls = getattr(hf, "UnbatchedClassifierFreeGuidanceLogitsProcessor", None)
    if cls is None:
        pytest.skip("this transformers has no UnbatchedClassifierFreeGuidanceLogitsProcessor")
    B, V = 3, 53
    x = guidance_ref.kernel_inputs(B, V, torch.float64, seed=4)

    class Out(dict):
        logits = property(lambda self: self["logits"])

    class Uncond:                                                    # the processor's unconditional model: rows B .. 2B - 1
        config = type("C", (), dict(is_encoder_decoder=False))()

        def __call__(self, input_ids, **kw):
            return Out(logits=x[B:, None, :], past_key_values=None)

    for g in (0.5, 1.5, 3.0):
        proc = cls(g, Uncond(), unconditional_ids=torch.zeros(B, 1, dtype=torch.long), use_cache=False)
        got = proc(torch.zeros(B, 1, dtype=torch.long), x[:B].clone())
        want = guidance_ref.reference(x, B, g)["score"]
        assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item(), g


# B = 1 has one pair: pair-adjacent then reads row 1 = row B + 0, the right one, and is no wrong variant there
MUTANT_CASES = [(v, B, V) for B, V in [(3, 7), (3, 1025), (1, 4097)] for v in guidance_ref.VARIANTS if not (v == "pair-adjacent" and B == 1)]


@pytest.mark.parametrize("variant,B,V", MUTANT_CASES)
def test_wrong_variants_leave_the_bound(variant, B, V):
    """From the references alone, on the inputs of the GPU file (guidance_ref.kernel_inputs): the share of elements whose wrong value
    lies outside the bf16 bound around the right one."""
    x = guidance_ref.kernel_inputs(B, V, torch.bfloat16, seed=V)
    for g in G_VALUES:
        if variant == "swapped" and g == 0.5:              # lu + (lc - lu) / 2 is symmetric in the two: swapping them changes nothing
            continue
        ref = guidance_ref.reference(x, B, g)
        bd = guidance_ref.bound(ref, g, V, torch.bfloat16)
        bad = guidance_ref.reference(x, B, g, variant)["score"]
        share = ((bad - ref["score"]).abs() > bd).double().mean().item()
        print(f"{variant} B={B} V={V} g={g}: {share * 100:.1f} % of the elements leave the bf16 bound")
        assert share >= SHARE, (variant, g, share)
