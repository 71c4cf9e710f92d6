"""Contrastive search without a GPU: the keyword checks of generate(penalty_alpha, top_k, return_contrastive_trace), which come before
any device work, the refusals of mmgl_contrastive_select (the method of tests/test_decode_refusals_cpu.py: addresses that are never
dereferenced, skipped where a GPU is visible) and the near-tie share of the reference restatement on the seed the GPU suite uses."""
import pytest
import torch

from contrastive_ref import search_ref
from test_generate_contrastive_gpu import ALPHA, B, BF16_TOL, N_NEW, NEAR_TIE_CAP, TAU32, WRAPPER_SEED, _closure
from test_generate_gpu import SEED, T, _fork, _prompt, _wrapper


def _cpu_models():
    _, lm = _fork()
    w, nb, _ = _wrapper()
    return lm, w, {k: v[:B] for k, v in nb.items()}


REFUSED = [
    (dict(top_k=1), "top_k"),
    (dict(top_k=9), "top_k"),
    (dict(top_k=0), "top_k"),
    (dict(penalty_alpha=1.0), "penalty_alpha"),
    (dict(penalty_alpha=-0.1), "penalty_alpha"),
    (dict(do_sample=True), "do_sample"),
    (dict(num_beams=2), "num_beams"),
    (dict(do_sample=True, num_return_sequences=2), "do_sample"),
    (dict(num_return_sequences=2), "num_return_sequences"),
    (dict(prompt_lookup_num_tokens=3), "prompt_lookup_num_tokens"),
    (dict(return_beam_trace=True), "return_beam_trace"),
    (dict(return_sequences_scores=True), "return_sequences_scores"),
    (dict(penalty_alpha=0.0, top_k=0, return_contrastive_trace=True), "return_contrastive_trace"),
]


@pytest.mark.parametrize("change,word", REFUSED, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in REFUSED])
def test_keyword_refusals_come_before_device_work(change, word):
    lm, w, nb = _cpu_models()
    ids, am = _prompt(SEED, batch=B)
    kw = dict(dict(penalty_alpha=ALPHA, top_k=4, max_new_tokens=N_NEW), **change)
    with pytest.raises(ValueError, match=word):
        lm.generate(ids, am, **kw)
    with pytest.raises(ValueError, match=word):
        w.generate(ids, am, **nb, **kw)


def test_inputs_embeds_is_refused():
    lm, _, _ = _cpu_models()
    with pytest.raises(ValueError, match="inputs_embeds"):
        lm.generate(inputs_embeds=torch.zeros(B, T, 64), attention_mask=torch.ones(B, T, dtype=torch.long), penalty_alpha=ALPHA, top_k=4)


def test_defaults_and_top_k_alone_are_unchanged():
    lm, w, nb = _cpu_models()
    ids, am = _prompt(SEED, batch=B)
    for gen, extra in ((lm.generate, {}), (w.generate, nb)):
        with pytest.raises(RuntimeError, match="no CPU path"):                  # today's greedy error, the new keywords at their defaults
            gen(ids, am, **extra, max_new_tokens=N_NEW, penalty_alpha=0.0, return_contrastive_trace=False)
        with pytest.raises(RuntimeError, match="no CPU path"):                  # a valid contrastive call gets as far as the device check
            gen(ids, am, **extra, max_new_tokens=N_NEW, penalty_alpha=ALPHA, top_k=4)
        with pytest.raises(ValueError, match="belong to do_sample=True"):
            gen(ids, am, **extra, max_new_tokens=N_NEW, top_k=4)


def test_signatures_of_the_other_generators_are_unchanged():
    import inspect
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    from mmgl_amd.model.modelling_self_attention import SelfAttentionModel
    for cls in (LlamaNeighborLM, SelfAttentionModel):
        assert not {"penalty_alpha", "return_contrastive_trace"} & set(inspect.signature(cls.generate).parameters)


def test_abi_version_and_chunk_constant():
    from mmgl_amd import _lib, ops
    L = _lib.lib()
    assert L.mmgl_version() == _lib.ABI_VERSION == 110
    assert L.mmgl_contrastive_chunk() == ops.CONTRASTIVE_CTX_CHUNK
    C = ops.CONTRASTIVE_CTX_CHUNK
    assert L.mmgl_contrastive_workspace(3, 5, 3 * C + 5) == 3 * 4 * 5 * 4
    assert L.mmgl_contrastive_workspace(0, 5, 8) == 0


P = 64        # a non-null, 16-byte aligned address that is never dereferenced
VALID = dict(cand=P, ld_cand=64, ctx=P, ld_ctx=64, bs=512, valid=P, ld_valid=8, n_cap=8, cs=P, ci=P, ld_pair=8, alpha=0.5, n_ctx=3, step=0,
             src=P, ld_src=4, ids=P, ld_ids=20, finished=P, eos=5, pad=1, hout=P, sel=P, tp=None, tpen=None, tsc=None, ws=P, ws_bytes=1024,
             B=2, k=4, d=64, V=128, dtype=1)
ORDER = ("cand ld_cand ctx ld_ctx bs valid ld_valid n_cap cs ci ld_pair alpha n_ctx step src ld_src ids ld_ids finished eos pad hout sel tp "
         "tpen tsc ws ws_bytes B k d V dtype").split()
INVALID, UNSUPPORTED = 1, 2
C_REFUSALS = [
    ("null cand_hidden", dict(cand=None), INVALID, "null pointer"),
    ("null ctx", dict(ctx=None), INVALID, "null pointer"),
    ("null ctx_valid", dict(valid=None), INVALID, "null pointer"),
    ("null cand_score", dict(cs=None), INVALID, "null pointer"),
    ("null src", dict(src=None), INVALID, "null pointer"),
    ("null ids", dict(ids=None), INVALID, "null pointer"),
    ("null hidden_out", dict(hout=None), INVALID, "null pointer"),
    ("null selected", dict(sel=None), INVALID, "null pointer"),
    ("null workspace", dict(ws=None), INVALID, "null pointer"),
    ("null finished with eos", dict(finished=None), INVALID, "null pointer"),
    ("one trace pointer", dict(tp=P), INVALID, "come together"),
    ("k = 1", dict(k=1), UNSUPPORTED, "k=1 candidates"),
    ("k = 9", dict(k=9, ld_pair=16), UNSUPPORTED, "k=9 candidates"),
    ("d no vector multiple", dict(d=60), UNSUPPORTED, "16-byte vector"),
    ("d no vector multiple, fp32", dict(d=62, dtype=0), UNSUPPORTED, "16-byte vector"),
    ("ld_cand smaller than the row", dict(ld_cand=56), INVALID, "smaller than the rows"),
    ("ld_ctx smaller than the row", dict(ld_ctx=56), INVALID, "smaller than the rows"),
    ("sample stride smaller than its rows", dict(bs=256), INVALID, "smaller than the rows"),
    ("mask stride smaller than the row", dict(ld_valid=7), INVALID, "smaller than the rows"),
    ("pair stride smaller than k", dict(ld_pair=3), INVALID, "smaller than the rows"),
    ("step outside src", dict(step=4), INVALID, "smaller than the rows"),
    ("ld_cand no 16-byte multiple", dict(ld_cand=68), UNSUPPORTED, "multiples of 16 bytes"),
    ("ld_ctx no 16-byte multiple, fp32", dict(ld_ctx=66, bs=1024, dtype=0), UNSUPPORTED, "multiples of 16 bytes"),
    ("sample stride no 16-byte multiple", dict(bs=516), UNSUPPORTED, "multiples of 16 bytes"),
    ("misaligned cand_hidden", dict(cand=72), UNSUPPORTED, "16-byte aligned"),
    ("misaligned ctx", dict(ctx=72), UNSUPPORTED, "16-byte aligned"),
    ("misaligned hidden_out", dict(hout=72), UNSUPPORTED, "16-byte aligned"),
    ("misaligned selected", dict(sel=66), INVALID, "4-byte aligned"),
    ("misaligned ids", dict(ids=68), INVALID, "ids 8-byte"),
    ("n_ctx = -1", dict(n_ctx=-1), INVALID, "n_ctx=-1 outside"),
    ("n_ctx = n_cap", dict(n_ctx=8), INVALID, "n_ctx=8 outside"),
    ("dtype", dict(dtype=7), INVALID, "bad dtype 7"),
    ("alpha", dict(alpha=1.5), INVALID, "alpha="),
    ("pad outside the vocabulary", dict(pad=128), INVALID, "pad_token_id"),
    ("candidate rows beyond the LDS", dict(k=8, ld_pair=8, d=8192, ld_cand=8192, ld_ctx=8192, bs=65536), UNSUPPORTED, "LDS"),
    ("workspace too small", dict(ws_bytes=16), INVALID, "workspace"),
    ("sizes", dict(B=0), INVALID, "bad sizes"),
]


@pytest.mark.parametrize("what,change,code,text", C_REFUSALS, ids=[r[0] for r in C_REFUSALS])
def test_entry_point_refuses(what, change, code, text):
    if torch.cuda.is_available():
        pytest.skip("runs where no GPU is visible: a missing check would launch on a made-up address")
    from mmgl_amd import _lib
    L = _lib.lib()
    assert set(change) <= set(VALID)
    args = dict(VALID, **change)
    assert L.mmgl_contrastive_select(*[args[name] for name in ORDER], None) == code
    msg = L.mmgl_last_error().decode()
    assert msg.startswith("mmgl_contrastive_select: ") and text in msg, msg


@pytest.mark.parametrize("k", [2, 4, 5])
def test_reference_near_tie_share_on_the_gpu_suites_seed(k):
    """The GPU suite excludes the (sample, step) pairs whose reference margin is below twice its tolerance and caps their share at
    5 % (fp32).  Here the reference alone, on its own tokens, on the HF fork of that suite: the share at that margin (tolerance
    2 TAU32 max|logit|: tests/test_generate_contrastive_gpu.py), and the search differs from greedy (the penalty is live) -- both before
    anything runs on a GPU."""
    hf, _ = _fork()
    ids, am = _prompt(SEED, batch=B)
    with torch.no_grad():
        hidden = lambda i, m: hf.model.decoder(input_ids=i, attention_mask=m).last_hidden_state
        new, steps = search_ref(hidden, hf.lm_head, ids, am, N_NEW, k, ALPHA)
        greedy = hf.generate(input_ids=ids, attention_mask=am, do_sample=False, num_beams=1, max_new_tokens=N_NEW, min_new_tokens=N_NEW,
                             pad_token_id=1, eos_token_id=None)[:, T:]
    tol = 2 * TAU32 * max(float(st["logits"].abs().max()) for st in steps)
    margins = torch.stack([st["margin"] for st in steps], 1)
    share = float((margins < 2 * tol).float().mean())
    print(f"k={k}: tolerance {tol:.3e}, smallest margin {float(margins.min()):.3e}, near-tie share {share:.3f}")
    assert share <= NEAR_TIE_CAP[torch.float32], share
    assert not torch.equal(new, greedy) and any(int(st["selected"].max()) > 0 for st in steps)


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_oracle_near_tie_share_on_the_wrapper_seed(dtype, k):
    """The same for the CrossAttentionModel cases: the oracle alone, on its own tokens (bf16: on the rounded weights, at the margin
    2 BF16_TOL and the 40 % cap)."""
    import torch.nn.functional as F
    from oracle import lm_ref
    _, _, oracle = _wrapper(seed=WRAPPER_SEED, round_bf16=dtype == torch.bfloat16)
    c = _closure(oracle)
    ids, am = _prompt(WRAPPER_SEED, batch=B)
    with torch.no_grad():
        _, steps = search_ref(lambda i, m: lm_ref.decoder_forward(c["lm"], c["cfg"], i, m, c["ne"][:B], c["nm"][:B]),
                              lambda h: F.linear(h, c["lm"]["lm_head.weight"]), ids, am, N_NEW, k, ALPHA)
    tol = BF16_TOL if dtype == torch.bfloat16 else 2 * TAU32 * max(float(st["logits"].abs().max()) for st in steps)
    share = float((torch.stack([st["margin"] for st in steps], 1) < 2 * tol).float().mean())
    print(f"wrapper oracle {dtype} k={k}: tolerance {tol:.3e}, near-tie share {share:.3f}")
    assert share <= NEAR_TIE_CAP[dtype], share
