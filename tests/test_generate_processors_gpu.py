"""-m gpu: the logits processors of generate() -- repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens -- on the
three generators (MPTForCausalLM / CrossAttentionModel, SelfAttentionModel, LlamaNeighborLM), DESIGN.md 4.14.  Tiny models, prompts
and comparison rule of tests/test_generate_gpu.py (its helpers are imported).

Rule.  At step s the reference runs UNCACHED on the product's own tokens; transformers' chain RepetitionPenalty -> NoRepeatNGram ->
MinNewTokensLength -> SuppressTokens is then applied per row to those logits with the row's COMPACTED history (the prompt without its
masked columns, then the new tokens).  Against that:
  * first, the processors must have changed at least one chosen token against the reference's raw argmax (else the case shows nothing);
  * the share of (sample, step) pairs whose processed top-1 minus top-2 margin is at most twice the bound below comes from the reference
    alone and is asserted (<= the cap of the model's own test file) BEFORE any comparison;
  * the -inf pattern of the returned step logits equals the reference's exactly;
  * finite logits agree within bound = tau max(p, 1/p) max|raw logit| (tau: the model's own tolerance, 1e-3 in fp32; a penalised
    logit scales the error by at most max(p, 1/p));
  * the token equals the reference's argmax wherever the margin exceeds 2 bound (rows that have emitted EOS hold pad_token_id instead).
The structural checks need no tolerance."""
import pytest
import torch

from logits_ref import compact, hf_chain, process_row
from test_generate_gpu import B, LOW_MARGIN_SHARE, N_NEW, SEED, T, TAU, _fork, _prompt, _reference_steps, _wrapper

pytestmark = pytest.mark.gpu

V = 128
# (repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens); EOS = 2 where min_new_tokens is on
FORK_SETTINGS = [(1.3, 0, 0, ()), (1.0, 2, 0, ()), (1.3, 3, 4, (5, 77)), (0.8, 1, 0, ())]
WRAPPER_SETTING = (1.3, 2, 0, ())


def _kw(p, n, m, suppress):
    kw = dict(repetition_penalty=p, no_repeat_ngram_size=n, min_new_tokens=m, suppress_tokens=list(suppress) or None)
    if m:
        kw.update(eos_token_id=2, pad_token_id=1)
    return kw


def chain_steps(raw, ids, am, p, n, m, suppress):
    """transformers' chain on the reference's raw step logits [B, n_new, V], per row on the compacted history of ids [B, T + n_new]."""
    out = torch.empty_like(raw)
    width = am.shape[1]
    for b in range(raw.shape[0]):
        for s in range(raw.shape[1]):
            h = compact(ids[b, :width + s].tolist(), am[b].tolist())
            out[b, s] = hf_chain(raw[b, s], h, p, n, suppress, eos=2 if m else None, min_new=m, n_generated=s)
    return out


def bound_of(raw, p, tau):
    return tau * max(p, 1.0 / p) * raw.abs().max().item()


def low_margin(proc, bound):
    top2 = proc.topk(2, dim=-1).values
    return ~((top2[..., 0] - top2[..., 1]) > 2 * bound)


def _compare(steps, ids, am, raw, setting, tau, cap, what, greedy=True):
    p, n, m, suppress = setting
    proc = chain_steps(raw, ids, am, p, n, m, suppress)
    changed = int((proc.argmax(-1) != raw.argmax(-1)).sum())
    print(f"{what}: the processors change {changed} of the {raw.shape[0] * raw.shape[1]} reference tokens")
    assert changed >= 1, f"{what}: the processors changed no token of the reference: the case shows nothing"
    bound = bound_of(raw, p, tau)
    low = low_margin(proc, bound)
    share = low.float().mean().item()
    print(f"{what}: {share * 100:.1f} % of the (sample, step) pairs are below the margin 2 bound = {2 * bound:.3e}")
    assert share <= cap, f"{what}: {share:.3f} of the steps are near-ties of the reference itself"
    got = steps.float().cpu()
    assert torch.equal(got == float("-inf"), proc == float("-inf")), f"{what}: the -inf pattern differs from the reference's"
    assert not torch.isnan(got).any() and not (got == float("inf")).any()
    finite = torch.isfinite(proc)
    err = (got[finite] - proc[finite]).abs().max().item()
    print(f"{what}: finite step logits differ by at most {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: step logits differ by {err:.3e} > {bound:.3e}"
    if greedy:
        tokens = ids[:, -raw.shape[1]:].cpu()
        free = torch.ones_like(tokens, dtype=torch.bool)        # False from the step after a row's EOS on: those hold the pad
        if m:
            for b in range(tokens.shape[0]):
                hit = (tokens[b] == 2).nonzero()
                if len(hit):
                    free[b, int(hit[0]) + 1:] = False
            assert bool((tokens[~free] == 1).all())
        assert torch.equal(tokens[free], got.argmax(-1)[free]), f"{what}: the returned ids are not the argmax of the returned step logits"
        wrong = (tokens != proc.argmax(-1)) & ~low & free
        assert not wrong.any(), f"{what}: {int(wrong.sum())} tokens differ from the reference at a clear margin: {wrong.nonzero().tolist()[:8]}"
    return proc


def _no_repeated_ngram(ids, am, n, n_new):
    """No n-gram that ends in a new token occurs twice in a row's compacted sequence."""
    for b in range(ids.shape[0]):
        h = compact(ids[b].tolist(), am[b].tolist())
        first_new = len(h) - n_new
        for j in range(max(first_new, n - 1), len(h)):
            gram = h[j - n + 1:j + 1]
            for i in range(n - 1, j):
                assert h[i - n + 1:i + 1] != gram, f"row {b}: the {n}-gram {gram} ending at new token {j - first_new} occurred at {i} already"


# ------------------------------------------------------------------------------------------ the fork against HF OPT + transformers' chain
@pytest.mark.parametrize("setting", FORK_SETTINGS, ids=lambda s: f"p{s[0]}-n{s[1]}-min{s[2]}-sup{len(s[3])}")
def test_fp32_fork_vs_hf_opt_and_transformers_chain(setting):
    """Ragged prompts, SEED = 1; the cap on the share below the margin is 5 %.  Shares by THIS file's rule (low_margin at 2 bound_of:
    the margin 2 tau max(p, 1/p) max|raw logit| over all steps), on HF OPT's own greedy tokens under transformers' chain, CPU, for the
    four settings: 0.0 / 2.3 / 1.6 / 3.9 % at SEED = 1; seeds 0 and 2 give 1.6-3.9 %, seed 3 gives 3.9 / 0.0 / 5.5 / 7.8 % and would
    fail the cap.  On the product's tokens, which is what the assertion below sees, the shares are the same 0.0 / 2.3 / 1.6 / 3.9 %;
    3.9 % is 5 pairs of 128 against a cap of 6."""
    hf, lm = _fork()
    ids, am = _prompt(SEED)
    lm = lm.cuda()
    out, steps = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, return_step_logits=True, **_kw(*setting))
    assert out.shape == (B, T + N_NEW) and steps.shape == (B, N_NEW, V) and torch.equal(out[:, :T].cpu(), ids)
    with torch.no_grad():
        raw = _reference_steps(lambda i, m: hf(input_ids=i, attention_mask=m).logits[:, -1], out.cpu(), am, N_NEW)
    _compare(steps, out.cpu(), am, raw, setting, TAU[torch.float32], LOW_MARGIN_SHARE[torch.float32], f"fork fp32 {setting}")
    p, n, m, suppress = setting
    new = out[:, T:].cpu()
    if n:
        _no_repeated_ngram(out.cpu(), am, n, N_NEW)
    if m:
        assert not (new[:, :m] == 2).any()
    for t in suppress:
        assert not (new == t).any()
    plain = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW)
    assert not torch.equal(plain, out), "the processors left the greedy run as it was"


def test_structural_checks_bite():
    """no_repeat_ngram_size = 1 / 2 / 3; min_new_tokens with an EOS the plain greedy run emits before step m; suppressed tokens that the
    plain run emits."""
    _, lm = _fork()
    lm = lm.cuda()
    ids, am = _prompt(SEED)
    run = lambda **kw: lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, **kw).cpu()
    plain = run()
    for n in (1, 2, 3):
        with pytest.raises(AssertionError):                     # the plain run of this random model does repeat
            _no_repeated_ngram(plain, am, n, N_NEW)
        _no_repeated_ngram(run(no_repeat_ngram_size=n), am, n, N_NEW)
    m = 6
    eos = int(plain[0, T + 2])                                  # the plain run emits it in row 0 at step 2 < m
    early = run(eos_token_id=eos, pad_token_id=1)
    assert (early[0, T + 3:] == 1).all()                        # without the ban row 0 ends there
    held = run(eos_token_id=eos, pad_token_id=1, min_new_tokens=m)
    assert not (held[:, T:T + m] == eos).any() and not (held[0, T:T + m] == 1).any()
    for b in range(B):                                          # the ban moves the EOS logit alone: up to a row's first EOS the run is the plain one
        hit = (plain[b, T:] == eos).nonzero()
        first = int(hit[0]) if len(hit) else N_NEW
        assert torch.equal(held[b, :T + first], plain[b, :T + first]), b
    banned = sorted(set(plain[:, T:T + 3].flatten().tolist()))
    out = run(suppress_tokens=banned)
    assert len(banned) >= 3 and not torch.isin(out[:, T:], torch.tensor(banned)).any()
    # defaults: bitwise the call without the keywords
    assert torch.equal(run(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=None), plain)
    assert torch.equal(run(suppress_tokens=[]), plain)
    with pytest.raises(ValueError, match="beam search"):
        run(num_beams=2, no_repeat_ngram_size=2)


# ------------------------------------------------------------------------------------------ sampling
def test_sampling_draws_from_the_processed_logits():
    from mmgl_amd import ops
    hf, lm = _fork()
    lm = lm.cuda()
    ids, am = _prompt(SEED)
    setting = (1.3, 3, 4, (5, 77))
    u = torch.rand(N_NEW, B, generator=torch.Generator().manual_seed(11)).cuda()
    knobs = dict(temperature=0.8, top_k=20, top_p=0.9)
    out, steps = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, return_step_logits=True, do_sample=True, sample_u=u, **knobs,
                             **_kw(*setting))
    with torch.no_grad():
        raw = _reference_steps(lambda i, m: hf(input_ids=i, attention_mask=m).logits[:, -1], out.cpu(), am, N_NEW)
    _compare(steps, out.cpu(), am, raw, setting, TAU[torch.float32], LOW_MARGIN_SHARE[torch.float32], "fork fp32 sampled", greedy=False)
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    for s in range(N_NEW):                                      # every ids column is the draw from the returned (processed) step logits
        tok = ops.sample_tokens(steps[:, s].contiguous(), u[s], finished=done, eos_token_id=2, pad_token_id=1, **knobs)
        assert torch.equal(tok, out[:, T + s]), f"step {s}"
    new = out[:, T:].cpu()
    assert not (new[:, :4] == 2).any() and not torch.isin(new, torch.tensor([5, 77])).any()
    _no_repeated_ngram(out.cpu(), am, 3, N_NEW)


def test_num_return_sequences_share_the_prompt_as_history():
    """R = 3, no_repeat_ngram_size = 1: at step 0 the R rows of a prompt see the prompt as common history, afterwards their own
    tokens -- no row repeats a token of its prompt or one of its own."""
    _, lm = _fork()
    lm = lm.cuda()
    ids, am = _prompt(SEED)
    R = 3
    u = torch.rand(N_NEW, B * R, generator=torch.Generator().manual_seed(12)).cuda()
    out, steps = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, do_sample=True, sample_u=u, num_return_sequences=R,
                             no_repeat_ngram_size=1, return_step_logits=True)
    out, steps = out.cpu(), steps.float().cpu()
    assert out.shape == (B * R, T + N_NEW) and torch.equal(out[:, :T], ids.repeat_interleave(R, dim=0))
    am_r = am.repeat_interleave(R, dim=0)
    _no_repeated_ngram(out, am_r, 1, N_NEW)
    for r in range(B * R):
        for s in range(N_NEW):                                  # the -inf pattern is the restatement's on the row's own history
            h = compact(out[r, :T + s].tolist(), am_r[r].tolist())
            want = process_row(torch.zeros(V), h, 1.0, 1) == float("-inf")
            assert torch.equal(steps[r, s] == float("-inf"), want), (r, s)
    assert len({tuple(out[r, T:].tolist()) for r in range(R)}) > 1
    plain = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, do_sample=True, sample_u=u, num_return_sequences=R).cpu()
    with pytest.raises(AssertionError):
        _no_repeated_ngram(plain, am_r, 1, N_NEW)


# ------------------------------------------------------------------------------------------ the wrappers and the Llama LM
def test_cross_attention_model_vs_oracle_loop():
    """Context `all`, ragged prompts, setting (1.3, 2, 0).  On the CPU oracle's own greedy tokens under this setting seeds 0-5 give
    4.7 / 3.9 / 3.9 / 1.6 / 3.1 / 3.1 % below the margin (the chain changes 57-68 of the 128 tokens); seed 3 sits at 1.6 %, cap 5 %."""
    w, nb, oracle = _wrapper(seed=3)
    ids, am = _prompt(3)
    w = w.cuda()
    out, steps = w.generate(ids.cuda(), am.cuda(), **{k: v.cuda() for k, v in nb.items()}, max_new_tokens=N_NEW, return_step_logits=True,
                            **_kw(*WRAPPER_SETTING))
    raw = _reference_steps(oracle, out.cpu(), am, N_NEW)
    _compare(steps, out.cpu(), am, raw, WRAPPER_SETTING, TAU[torch.float32], LOW_MARGIN_SHARE[torch.float32], "CrossAttentionModel fp32")
    _no_repeated_ngram(out.cpu(), am, 2, N_NEW)


def test_self_attention_model_raw_mode():
    """Raw mode, text only, no adapter: the LM input is input_ids, the reference the wrapper's own uncached forward.  On the CPU (HF
    OPT on the wrapper's LM weights, its own greedy tokens under (1.3, 2, 0)) seeds 0-5 give 2.3 / 2.3 / 5.5 / 3.9 / 6.2 / 3.1 % below
    the margin; seed 1 sits at 2.3 %, cap 5 %."""
    from test_generate_selfattn_gpu import _sa, _uncached
    w = _sa(seed=1).cuda()
    ids, am = _prompt(1)
    out, steps = w.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, return_step_logits=True, **_kw(*WRAPPER_SETTING))
    assert out.shape == (B, T + N_NEW) and torch.equal(out[:, :T].cpu(), ids)
    raw = _reference_steps(_uncached(w), out.cpu(), am, N_NEW)
    _compare(steps, out.cpu(), am, raw, WRAPPER_SETTING, TAU[torch.float32], LOW_MARGIN_SHARE[torch.float32], "SelfAttentionModel raw")
    _no_repeated_ngram(out.cpu(), am, 2, N_NEW)


def test_self_attention_model_embedding_mode_history_is_the_prompt_ids():
    """Embedding mode, context `all`: the LM runs on embeddings [prompt | neighbor tokens | new tokens], the history is input_ids
    (history_ids / history_mask) and then the new tokens -- the neighbor slots are no part of it.  Reference: w.lm uncached on the
    embeddings of the shared helper.  Shares below the margin, from the reference alone on the product's tokens (the LM input of this
    scenario exists on the device only): seeds 0-5 give 3.9 / 2.3 / 3.9 / 3.9 / 3.1 / 7.0 %; seed 1 sits at 2.3 %, cap 5 %."""
    from test_generate_gpu import _neighbors
    from test_generate_selfattn_gpu import _embeds_reference, _sa
    w = _sa(seed=1, neighbor_mode="embedding", context="all").cuda()
    ids, am = _prompt(1)
    nb = {k: v.cuda() for k, v in _neighbors(1 + 100).items()}
    out, steps = w.generate(ids.cuda(), am.cuda(), **nb, max_new_tokens=N_NEW, return_step_logits=True, **_kw(*WRAPPER_SETTING))
    assert out.shape == (B, T + N_NEW) and torch.equal(out[:, :T].cpu(), ids)
    with torch.no_grad():
        lm_in, lm_mask = w._lm_inputs(ids.cuda(), am.cuda(), **nb)
    raw = _embeds_reference(w, lm_in, lm_mask, out, N_NEW)
    _compare(steps, out.cpu(), am, raw, WRAPPER_SETTING, TAU[torch.float32], LOW_MARGIN_SHARE[torch.float32], "SelfAttentionModel embedding")
    _no_repeated_ngram(out.cpu(), am, 2, N_NEW)
    # without history_ids the LM's history of an embeddings prompt is the new tokens alone
    new, steps2 = w.lm.generate(inputs_embeds=lm_in, attention_mask=lm_mask, max_new_tokens=N_NEW, return_step_logits=True,
                                **_kw(*WRAPPER_SETTING))
    assert new.shape == (B, N_NEW) and new.is_contiguous()
    for b in range(B):
        for s in range(N_NEW):
            want = process_row(torch.zeros(V), new[b, :s].tolist(), 1.0, 2) == float("-inf")
            assert torch.equal(steps2[b, s].float().cpu() == float("-inf"), want), (b, s)


def test_llama_neighbor_lm_vs_oracle_loop():
    """The tiny GQA config (Hkv = 2) of tests/test_generate_llama_gpu.py, gates open, ragged prompts, setting (1.3, 2, 0).  On the CPU
    oracle's own greedy tokens under this setting seeds 0-5 give 1.6 / 3.1 / 3.1 / 3.9 / 3.1 / 2.3 % below the margin; SEED = 0 (the seed
    of that file) sits at 1.6 %, cap 5 %."""
    import test_generate_llama_gpu as tl
    lm = tl._lm("tiny", 2, seed=0)
    ne, valid = tl._neighbors(0, 64)
    ref_fn = tl._oracle_last_logits(lm, "tiny", ne, valid)
    ids, am = tl._prompt(0)
    out, steps = tl._generate(lm.cuda(), ids, am, ne, valid, return_step_logits=True, **_kw(*WRAPPER_SETTING))
    raw = tl._reference_steps(ref_fn, out.cpu(), am, N_NEW)
    _compare(steps, out.cpu(), am, raw, WRAPPER_SETTING, tl.TAU[torch.float32], tl.LOW_MARGIN_SHARE[torch.float32], "LlamaNeighborLM fp32")
    _no_repeated_ngram(out.cpu(), am, 2, N_NEW)
    u = torch.rand(N_NEW, B, generator=torch.Generator().manual_seed(13)).cuda()
    sampled = tl._generate(lm, ids, am, ne, valid, do_sample=True, sample_u=u, no_repeat_ngram_size=1).cpu()
    _no_repeated_ngram(sampled, am, 1, N_NEW)


# ------------------------------------------------------------------------------------------ bf16
def test_bf16_fork_structure_and_minus_infinity_pattern():
    """bf16: the structural checks, and the -inf pattern of the step logits equals the restatement on the returned ids (the numerical
    accuracy of the bf16 rewrite is the kernel test's job)."""
    _, lm = _fork()
    lm = lm.bfloat16().cuda()
    ids, am = _prompt(SEED)
    p, n, m, suppress = 1.3, 3, 4, (5, 77)
    out, steps = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, return_step_logits=True, **_kw(p, n, m, suppress))
    out, steps = out.cpu(), steps.float().cpu()
    assert steps.shape == (B, N_NEW, V) and not torch.isnan(steps).any()
    new = out[:, T:]
    _no_repeated_ngram(out, am, n, N_NEW)
    assert not (new[:, :m] == 2).any() and not torch.isin(new, torch.tensor(suppress)).any()
    for b in range(B):
        for s in range(N_NEW):
            h = compact(out[b, :T + s].tolist(), am[b].tolist())
            want = process_row(torch.zeros(V), h, 1.0, n, suppress + ((2,) if s < m else ())) == float("-inf")
            assert torch.equal(steps[b, s] == float("-inf"), want), (b, s)


# ------------------------------------------------------------------------------------------ the trainer
def test_evaluate_loop_passes_the_processor_arguments(tmp_path):
    from torch.utils.data import DataLoader, Subset
    from mmgl_amd.language_modelling.run_generation import Arguments, build_datasets, build_model, evaluate_loop
    from mmgl_amd.wikiweb2m.synthetic import synthetic_tokenizer
    torch.manual_seed(0)
    tokenizer = synthetic_tokenizer()
    base = dict(model_name_or_path="mpt-tiny", dataset="synthetic", context="all", neighbor_mode="embedding", peft_type="flamingo",
                max_input_length=32, max_output_length=12, max_text_neighbors=5, max_image_neighbors=2, n_text_tokens=2, n_visual_tokens=2,
                per_device_val_batch_size=4, dataloader_num_workers=0, val_steps_per_epoch=2, print_freq=100, log_dir=str(tmp_path), seed=0)
    args = Arguments(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3, **base)
    plain = Arguments(**base)
    args.image_size = plain.image_size = 32
    model = build_model(args, tokenizer, offline=True).float().cuda().eval()
    _, val_ds, _ = build_datasets(args, tokenizer)
    loader = lambda: DataLoader(Subset(val_ds, list(range(8))), batch_size=4, shuffle=False, num_workers=0, drop_last=True)
    names = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens")
    calls, real = [], model.generate

    def recording(**kw):
        calls.append({k: kw.get(k) for k in names})
        return real(**kw)
    model.generate = recording
    try:
        evaluate_loop(loader(), model, tokenizer, 0, args, prefix="test")
        n = len(calls)
        assert n >= 1 and all(c == dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3) for c in calls), calls
        evaluate_loop(loader(), model, tokenizer, 0, plain, prefix="test")
        assert len(calls) > n and all(c == dict.fromkeys(names) for c in calls[n:]), calls[n:]
    finally:
        del model.generate
