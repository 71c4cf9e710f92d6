"""-m gpu: generate(weight_dtype="fp8") -- the decode steps of the frozen layers on e4m3fn codes of their weights.

The reference of every comparison is the SAME generate() call with ops.decode_linear_w8 replaced by "dequantise, then ops.decode_linear":
the same prefill, the same cache, the same codes; only the kernel under test is swapped (tests/test_gemm_skinny_w8_gpu.py checks that
kernel element by element).  Rule:
  * the step logits agree within the tolerance the model's existing test of cached against uncached step logits uses (max-norm relative
    error, helpers.rel_err): OPT fork tests/test_generate_gpu.py TAU = 1e-3 fp32 / 2e-2 bf16; Llama LM tests/test_generate_llama_gpu.py
    test_cached_equals_uncached_inside_the_product, 1e-3 fp32 / BF16_LOGITS_TOL = 2.5e-2 bf16;
  * the tokens are equal on every (sample, step) whose top-1 minus top-2 margin in the reference exceeds that tolerance times the
    reference's largest |logit| (stricter than the 2 tau rule of those modules);
  * the share of (sample, step) pairs at or below the margin is computed from the reference alone and asserted <= 5 % BEFORE any
    comparison.  A sample whose token differs at such a pair has another history afterwards: its later steps are not compared, and the
    share of pairs lost that way is capped at 5 % as well.
Random tiny models have flat logits: at the bf16 tolerances 15-40 % of their steps are below the margin, whatever the seed.  The bf16
models here are therefore built to be decided: tied heads (the Llama config ties lm_head to the embedding; the OPT fork always does), a
residual stream the token embedding leads (Llama: initializer_range 0.05; OPT fork: the embedding rows doubled), layers that still move
it -- each case asserts that the FP8 weights move the logits at least 4 times as far from the unquantised run as the kernel under
test is from its reference, so a case in which the frozen layers' GEMMs did not matter would fail.  The seeds are not free: shares per
seed are in SEEDS' comment.  In the post-LN fork with project_in / project_out the projections sit between the embedding and the head:
there project_out is also set to the pseudo-inverse of project_in (embedding width 64, hidden 128), so that the way out undoes the way
in.  That case runs in bf16 -- the MFMA kernel behind word_embed_proj_dim 64 and in front of the LayerNorms that follow the residual
epilogues -- and once more in fp32 as it is initialised.

Sizes: hidden 128 (FFN 256) so that every GEMM of a step has K % 128 == 0 and takes the MFMA kernel; the fp32 case takes the generic one.
Calls per step, counted: 4 w8 calls per frozen Llama layer (q|k|v, o_proj, gate|up, down_proj); per OPT layer 5 where the LM is frozen
and its q|k|v weight fused (the wrapper: q and k|v of the fused weight, out_proj, fc1, fc2) and 6 where q, k and v are parameters that
still require gradients and are multiplied one by one (the bare fork of these tests); ops.decode_linear only for the gated layers (4
each), project_in / project_out and the head."""
import pytest
import torch

from helpers import mpt_args, rel_err, tiny_clip_vision_config, tiny_roberta_config
from test_generate_gpu import TAU as OPT_TAU
from test_generate_gpu import _neighbors as _wrapper_neighbors
from test_generate_llama_gpu import BF16_LOGITS_TOL, _open_gates, _prompt

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
B, T, N_NEW, S = 8, 12, 16, 10
HIDDEN, FFN, VOCAB = 128, 256, 128
TOL = {"llama": {F32: 1e-3, BF16: BF16_LOGITS_TOL}, "opt": OPT_TAU}
CAP = 0.05
# seed per case.  Share of reference pairs at or below the margin, measured for seeds 0..7 with the construction above:
SEEDS = {
    "llama Hkv=H": 2,                 # 6.2 7.8 4.7 7.0 11.7 14.1 8.6 14.8 %
    "llama Hkv<H": 2,                 # 9.4 10.9 4.7 9.4 8.6 7.0 7.0 7.8 %
    "llama neighbors": 6,             # 10.2 14.1 7.0 11.7 12.5 10.2 3.1 17.2 %
    "opt pre-LN": 0,                  # 1.6 7.0 7.0 2.3 2.3 8.6 15.6 5.5 %
    "opt post-LN proj": 1,            # 3.1 2.3 5.5 3.9 4.7 5.5 0.0 0.0 %
    "opt post-LN proj fp32": 0,       # 0.8 1.6 0.0 0.0 0.0 4.7 1.6 1.6 %
    "wrapper": 5,                     # 7.8 0.8 7.8 3.9 3.9 2.3 5.5 10.2 %
}


# ------------------------------------------------------------------------------------------ models
def _llama(seed, n_kv, dtype=BF16):
    from transformers import LlamaConfig
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    torch.manual_seed(seed)
    cfg = LlamaConfig(vocab_size=VOCAB, hidden_size=HIDDEN, intermediate_size=FFN, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=n_kv, max_position_embeddings=256, pad_token_id=1, bos_token_id=2, eos_token_id=2,
                      attention_dropout=0.0, initializer_range=0.05, tie_word_embeddings=True)
    lm = LlamaNeighborLM(mpt_args(model_name_or_path="llama-tiny", neighbor_layer_wise=1), cfg)
    _open_gates(lm, HIDDEN)
    return lm.eval().to(dtype).cuda()


def _llama_neighbors(seed, dtype=BF16):
    g = torch.Generator().manual_seed(seed + 100)
    ne = torch.randn(B, S, HIDDEN, generator=g)
    valid = torch.rand(B, S, generator=g) > 0.3
    valid[5] = False
    return dict(neighbor_embeds=ne.to(dtype).cuda(), neighbor_attention_mask=valid.cuda())


def _opt_config(pre_ln=True, proj=None):
    from transformers import OPTConfig
    return OPTConfig(vocab_size=VOCAB, hidden_size=HIDDEN, num_attention_heads=4, ffn_dim=FFN, num_hidden_layers=2, max_position_embeddings=64,
                     word_embed_proj_dim=proj or HIDDEN, do_layer_norm_before=pre_ln, dropout=0.0, attention_dropout=0.0, pad_token_id=1,
                     bos_token_id=2, eos_token_id=2, init_std=0.08)


def _lead(lm, by=2.0):
    with torch.no_grad():
        lm.model.decoder.embed_tokens.weight.mul_(by)      # tied to lm_head: the token embedding leads the residual stream


def _fork(seed, pre_ln=True, proj=None, dtype=BF16):
    from mmgl_amd.model.modelling_cross_attention import MPTConfig, MPTForCausalLM
    torch.manual_seed(seed)
    lm = MPTForCausalLM(MPTConfig(mpt_args(neighbor_mode="raw", peft_type="none"), _opt_config(pre_ln, proj)))
    if dtype == BF16:
        _lead(lm)
        if proj:                                           # the way back from the hidden to the embedding width undoes the way in
            dec = lm.model.decoder
            with torch.no_grad():
                dec.project_out.weight.copy_(torch.linalg.pinv(dec.project_in.weight.float()))
    return lm.eval().to(dtype).cuda()


def _wrapper(seed, dtype=BF16):
    from mmgl_amd.model import CrossAttentionModel
    torch.manual_seed(seed)
    w = CrossAttentionModel(mpt_args(context="all", neighbor_layer_wise=1), tokenizer=None, lm_config=_opt_config(), text_config=tiny_roberta_config(),
                            visual_config=tiny_clip_vision_config()).eval()
    with torch.no_grad():
        gates = [p for n_, p in w.named_parameters() if n_.endswith(("gating1", "gating2"))]
        assert len(gates) == 4
        for p, v in zip(gates, (0.6, -0.8, 0.9, 0.5)):
            p.fill_(v)
    _lead(w.lm)
    nb = {k: v.cuda() for k, v in _wrapper_neighbors(seed + 100).items()}
    return w.to(dtype).cuda(), nb


def _case(name, seed=None):
    """(model, the keyword arguments of its generate() besides the prompt, tolerance, frozen layers, gated layers that run, w8 calls
    per frozen layer, ops.decode_linear calls per step outside the gated layers and the head)."""
    seed = SEEDS[name] if seed is None else seed
    if name.startswith("llama"):
        lm = _llama(seed, 4 if name == "llama Hkv=H" else 2)
        kw = _llama_neighbors(seed) if name == "llama neighbors" else {}
        return lm, kw, TOL["llama"][BF16], len(lm._frozen), len(lm.neighbor_layers) if kw else 0, 4, 0
    if name == "opt pre-LN":
        lm = _fork(seed)
        return lm, {}, TOL["opt"][BF16], 2, 0, 6, 0
    if name == "opt post-LN proj":
        lm = _fork(seed, False, 64)
        return lm, {}, TOL["opt"][BF16], 2, 0, 6, 2
    if name == "opt post-LN proj fp32":
        lm = _fork(seed, False, 64, F32)
        return lm, {}, TOL["opt"][F32], 2, 0, 6, 2
    w, nb = _wrapper(seed)
    dec = w.lm.model.decoder
    return w, nb, TOL["opt"][BF16], len(dec.layers), len(dec.neighbor_layers), 5, 0


# ------------------------------------------------------------------------------------------ the swap and the rule
def _dequantise_then_decode_linear(real):
    def ref(x, codes, exps, bias=None, act="none", out_scale=1.0, residual=None, out=None):
        w = (codes.float() * torch.exp2(exps.float())[:, None]).to(x.dtype)        # exact: every value is a bf16 number
        return real(x, w, bias, act=act, out_scale=out_scale, residual=residual, out=out)
    return ref


class _Counter:
    def __init__(self, fn):
        self.fn, self.n, self.rows = fn, 0, []

    def __call__(self, *a, **kw):
        self.n += 1
        self.rows.append(a[0].shape[0])
        return self.fn(*a, **kw)


def _generate(model, seed, kw, **more):
    ids, am = _prompt(seed, vocab=VOCAB)
    return model.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, **kw, **more)


def _reference(monkeypatch, model, seed, kw, **more):
    """The same call with the kernel under test swapped out."""
    from mmgl_amd import ops
    with monkeypatch.context() as m:
        m.setattr(ops, "decode_linear_w8", _dequantise_then_decode_linear(ops.decode_linear))
        return _generate(model, seed, kw, weight_dtype="fp8", **more)


def _low_margin(ref_steps, tol):
    ref = ref_steps.float().cpu()
    top2 = ref.topk(2, dim=-1).values
    return (top2[..., 0] - top2[..., 1]) <= tol * ref.abs().max().item()


def _compare(what, out, steps, ref_out, ref_steps, tol):
    """The rule of the module docstring; returns the error."""
    low = _low_margin(ref_steps, tol)
    share = low.float().mean().item()
    print(f"{what}: {share * 100:.1f} % of the {low.numel()} reference (sample, step) pairs are at or below the margin")
    assert share <= CAP, f"{what}: {share:.3f} of the steps are near-ties of the reference itself"
    n = steps.shape[1]
    tok, ref_tok = out[:, -n:].cpu(), ref_out[:, -n:].cpu()
    differs = tok != ref_tok
    same_history = torch.cat([torch.ones(tok.shape[0], 1, dtype=torch.bool), differs.cumsum(1)[:, :-1] == 0], dim=1)
    lost = 1.0 - same_history.float().mean().item()
    assert lost <= CAP, f"{what}: {lost:.3f} of the steps follow a token that differed at a near-tie"
    wrong = differs & same_history & ~low
    assert not wrong.any(), f"{what}: {int(wrong.sum())} tokens differ from the reference at a clear margin: {wrong.nonzero().tolist()[:8]}"
    a, b = steps.float().cpu()[same_history], ref_steps.float().cpu()[same_history]
    err = (a - b).abs().max().item() / ref_steps.float().abs().max().item()
    print(f"{what}: step logits rel err {err:.3e} (tolerance {tol:.1e}); {int(differs.sum())} tokens differ, {lost * 100:.1f} % of the steps lost")
    assert err <= tol, f"{what}: step logits rel err {err:.3e} > {tol:.1e}"
    return err


# ------------------------------------------------------------------------------------------ greedy, every model
@pytest.mark.parametrize("name", list(SEEDS))
def test_steps_run_on_codes_and_match_the_swapped_reference(name, monkeypatch):
    from mmgl_amd import ops
    model, kw, tol, frozen, gated, per_layer, extra = _case(name)
    seed = SEEDS[name]
    ref_out, ref_steps = _reference(monkeypatch, model, seed, kw, return_step_logits=True)
    assert _low_margin(ref_steps, tol).float().mean().item() <= CAP                      # first, from the reference alone
    w8, dense = _Counter(ops.decode_linear_w8), _Counter(ops.decode_linear)
    with monkeypatch.context() as m:
        m.setattr(ops, "decode_linear_w8", w8)
        m.setattr(ops, "decode_linear", dense)
        out, steps = _generate(model, seed, kw, weight_dtype="fp8", return_step_logits=True)
    assert out.shape == (B, T + N_NEW) and steps.shape == (B, N_NEW, VOCAB)
    # the steps really run on codes: per step per_layer w8 calls per frozen layer; ops.decode_linear only for the gated layers, the
    # projections in / out and the head (which also runs once on the prefill's last row)
    assert w8.n == (N_NEW - 1) * frozen * per_layer and set(w8.rows) == {B}, (w8.n, set(w8.rows))
    assert dense.n == (N_NEW - 1) * (4 * gated + extra) + N_NEW, dense.n
    err = _compare(name, out, steps, ref_out, ref_steps, tol)
    # the quantised weights are live: the unquantised run lies much further away than the kernel under test from its reference
    plain_out, plain_steps = _generate(model, seed, kw, return_step_logits=True)
    first = (plain_out[:, T:] != out[:, T:]).int().cumsum(1) == 0                        # steps on the same history
    first = torch.cat([torch.ones_like(first[:, :1]), first[:, :-1]], dim=1).cpu()
    dist = (plain_steps.float().cpu() - steps.float().cpu())[first].abs().max().item() / ref_steps.float().abs().max().item()
    print(f"{name}: FP8 weights move the step logits by {dist:.3e} of the largest logit")
    assert dist >= 4 * err and dist >= 1e-3, (dist, err)
    # the two spellings of the keyword are one
    assert torch.equal(_generate(model, seed, kw, weight_dtype=torch.float8_e4m3fn), out)


# ------------------------------------------------------------------------------------------ what it combines with
def _holders(model):
    """The objects that keep a model's WeightCodes."""
    if hasattr(model, "_frozen"):
        mods = model._frozen
    else:
        dec = (model.lm if hasattr(model, "lm") else model).model.decoder
        mods = [m for layer in dec.layers for m in (layer, layer.self_attn)]
    return [m.__dict__["_w8_codes"] for m in mods if "_w8_codes" in m.__dict__]


def _code_tensors(model):
    return [t for h in _holders(model) for pair in h.tensors().values() for t in pair]


@pytest.mark.parametrize("name", ["llama Hkv<H", "opt pre-LN", "wrapper"])
def test_off_is_the_call_without_the_keyword_and_keeps_no_codes(name, monkeypatch):
    from mmgl_amd import ops
    model, kw, *_ = _case(name)
    seed = SEEDS[name]
    w8 = _Counter(ops.decode_linear_w8)
    with monkeypatch.context() as m:
        m.setattr(ops, "decode_linear_w8", w8)
        a, sa = _generate(model, seed, kw, return_step_logits=True)
        b, sb = _generate(model, seed, kw, return_step_logits=True, weight_dtype=None)
    assert torch.equal(a, b) and torch.equal(sa, sb) and w8.n == 0
    assert _code_tensors(model) == [], "weight_dtype=None left code tensors behind"


@pytest.mark.parametrize("name", ["llama Hkv<H", "opt pre-LN"])
def test_codes_are_cached_until_a_weight_changes(name):
    model, kw, *_ = _case(name)
    seed = SEEDS[name]
    first = _generate(model, seed, kw, weight_dtype="fp8")
    ptrs = sorted(t.data_ptr() for t in _code_tensors(model))
    n_weights = {"llama Hkv<H": 4, "opt pre-LN": 6}[name] * 2
    assert len(ptrs) == 2 * n_weights and len(set(ptrs)) == len(ptrs)                   # a (codes, exps) pair per quantised weight
    again = _generate(model, seed, kw, weight_dtype="fp8")
    assert torch.equal(first, again) and sorted(t.data_ptr() for t in _code_tensors(model)) == ptrs, "the second call quantised again"
    # an in-place change of one frozen weight: its codes are new, and they are the codes of the new weight
    if name.startswith("llama"):
        weight, holder, key = model.llama.model.layers[1].mlp.down_proj.weight, model._frozen[1].__dict__["_w8_codes"], "down_proj"
    else:
        layer = model.model.decoder.layers[1]
        weight, holder, key = layer.fc2.weight, layer.__dict__["_w8_codes"], "fc2"
    old = holder.tensors()[key]
    old_codes = old[0].view(torch.uint8).clone()
    with torch.no_grad():
        weight.mul_(-1.5)
    _generate(model, seed, kw, weight_dtype="fp8")
    new = holder.tensors()[key]
    assert new[0] is not old[0] and not torch.equal(new[0].view(torch.uint8), old_codes)
    import w8_ref
    want_c, want_e = w8_ref.quantize(weight.detach().cpu())
    assert torch.equal(new[0].view(torch.uint8).cpu(), want_c) and torch.equal(new[1].cpu(), want_e)


def test_an_embeddings_prompt_gives_the_tokens_of_the_ids_prompt():
    lm, kw, *_ = _case("opt pre-LN")
    seed = SEEDS["opt pre-LN"]
    ids, am = _prompt(seed, vocab=VOCAB)
    greedy = _generate(lm, seed, kw, weight_dtype="fp8")
    emb = lm.model.decoder.embed_tokens(ids.cuda())
    new = lm.generate(inputs_embeds=emb, attention_mask=am.cuda(), max_new_tokens=N_NEW, weight_dtype="fp8")
    assert new.shape == (B, N_NEW) and torch.equal(new, greedy[:, T:])


@pytest.mark.parametrize("name", ["llama neighbors", "opt pre-LN"])
def test_sampled_with_fixed_draws(name, monkeypatch):
    model, kw, tol, *_ = _case(name)
    seed = SEEDS[name]
    u = torch.rand(N_NEW, B, generator=torch.Generator().manual_seed(seed + 7)).cuda()
    more = dict(do_sample=True, top_k=8, temperature=0.8, sample_u=u, return_step_logits=True)
    ref_out, ref_steps = _reference(monkeypatch, model, seed, kw, **more)
    out, steps = _generate(model, seed, kw, weight_dtype="fp8", **more)
    # a sampled token moves only where a draw lies within the kernel's noise of a boundary of the CDF: none for these draws
    assert torch.equal(out, ref_out), f"{name}: sampled tokens differ at {(out != ref_out).nonzero().tolist()[:8]}"
    assert rel_err(steps, ref_steps) <= tol


@pytest.mark.parametrize("name", ["llama Hkv<H", "opt pre-LN"])
def test_with_the_fp8_key_value_cache(name, monkeypatch):
    model, kw, tol, *_ = _case(name)
    seed = SEEDS[name]
    more = dict(kv_cache_dtype="fp8", return_step_logits=True)
    ref_out, ref_steps = _reference(monkeypatch, model, seed, kw, **more)
    out, steps = _generate(model, seed, kw, weight_dtype="fp8", **more)
    _compare(f"{name} + FP8 key/value cache", out, steps, ref_out, ref_steps, tol)


@pytest.mark.parametrize("name", ["llama Hkv<H", "opt pre-LN"])
def test_prompt_lookup_gives_the_greedy_result(name, monkeypatch):
    from mmgl_amd import ops
    model, kw, *_ = _case(name)
    seed = SEEDS[name]
    greedy = _generate(model, seed, kw, weight_dtype="fp8")
    w8 = _Counter(ops.decode_linear_w8)
    with monkeypatch.context() as m:
        m.setattr(ops, "decode_linear_w8", w8)
        out, stats = _generate(model, seed, kw, weight_dtype="fp8", prompt_lookup_num_tokens=3, return_lookup_stats=True)
    assert set(w8.rows) == {B * 4} and w8.n > 0 and stats["steps"] < N_NEW - 1           # verify steps of B (K + 1) rows, fewer of them
    assert torch.equal(out, greedy), f"{name}: prompt lookup differs from greedy at {(out != greedy).nonzero().tolist()[:8]}"


@pytest.mark.parametrize("more", [dict(num_beams=2), dict(guidance_scale=1.5)], ids=["beams", "guidance"])
def test_fork_modes_of_more_rows(more, monkeypatch):
    from mmgl_amd import ops
    model, kw, tol, *_ = _case("wrapper")
    seed = SEEDS["wrapper"]
    ref_out = _reference(monkeypatch, model, seed, kw, **more)
    w8 = _Counter(ops.decode_linear_w8)
    with monkeypatch.context() as m:
        m.setattr(ops, "decode_linear_w8", w8)
        out = _generate(model, seed, kw, weight_dtype="fp8", **more)
    assert set(w8.rows) == {2 * B} and w8.n > 0
    assert torch.equal(out, ref_out), f"{more}: tokens differ at {(out != ref_out).nonzero().tolist()[:8]}"


def test_evaluate_loop_passes_the_argument(tmp_path):
    from torch.utils.data import DataLoader, Subset
    from mmgl_amd.language_modelling.run_generation import Arguments, build_datasets, build_model, evaluate_loop
    from mmgl_amd.wikiweb2m.synthetic import synthetic_tokenizer
    torch.manual_seed(0)
    tokenizer = synthetic_tokenizer()
    args = Arguments(model_name_or_path="mpt-tiny", dataset="synthetic", context="all", neighbor_mode="embedding", peft_type="flamingo",
                     max_input_length=32, max_output_length=12, max_text_neighbors=5, max_image_neighbors=2, n_text_tokens=2,
                     n_visual_tokens=2, per_device_val_batch_size=4, dataloader_num_workers=0, val_steps_per_epoch=2, print_freq=100,
                     log_dir=str(tmp_path), seed=0)
    args.image_size = 32
    assert args.weight_dtype is None
    model = build_model(args, tokenizer, offline=True).float().cuda().eval()
    _, val_ds, _ = build_datasets(args, tokenizer)
    loader = lambda: DataLoader(Subset(val_ds, list(range(4))), batch_size=4, shuffle=False, num_workers=0, drop_last=True)
    seen, real = [], model.generate

    def spy(**kw):
        seen.append(kw.get("weight_dtype", "absent"))
        return real(**kw)
    model.generate = spy
    try:
        evaluate_loop(loader(), model, tokenizer, 0, args, prefix="test")
        n = len(seen)
        assert n >= 1 and set(seen) == {"absent"}                                   # the default: today's call
        args.weight_dtype = "fp8"
        evaluate_loop(loader(), model, tokenizer, 0, args, prefix="test")
        assert len(seen) == 2 * n and set(seen[n:]) == {"fp8"}
        assert _code_tensors(model), "the generations of the second pass did not run on codes"
    finally:
        del model.generate
