"""-m gpu: prompt-lookup decoding, generate(prompt_lookup_num_tokens=K).  The result is the greedy result in fewer steps:

(a) against the uncached reference run on the product's own tokens, under the rule of tests/test_generate_gpu.py: the low-margin share
    of the reference is asserted first (<= 5 % fp32, <= 25 % bf16), then every returned token equals the reference's argmax wherever
    the reference's margin exceeds 2 tau max|logit|.  There are no step logits to compare: a verify step scores K + 1 rows per sample
    and returns none of them.  HF OPT for the fork (for bf16: on the bf16-rounded weights), the CPU oracle for the wrapper with open
    gates; pre-LN and post-LN; K = 1, 3, 7.  On HF's own greedy tokens the reference's share is 0.8 % / 10.2 % (pre-LN fp32 / bf16) and
    0 % / 4.7 % (post-LN) for this layout and SEED; tests/test_generate_gpu.py records 1.6 % / 14.8 % for the wrapper.
(b) the ids equal the K = 0 ids of the same model up to each row's first low-margin step.
(c) a successor model -- out_proj and fc2 zeroed, positions zeroed, lm_head row v = embedding row v - 1, so that every greedy token
    is the previous one + 1; the relative top-2 margin of this file's embedding draw is 0.38 in fp32 and on bf16-rounded weights
    (HF OPT on the CPU; another draw of the same construction gave 0.47), and _successor asserts >= 0.3 from the weights -- on prompts that
    give a full accept, a partial accept, rejected drafts, no drafts, an EOS inside an accepted block and ragged right padding.  Each
    case is established with the CPU simulation (tests/lookup_ref.py) first; then ids are exact and `emitted` is the simulated trace.
(d) the cache after generation against the cache of a K = 0 run, (e) the limits and refusals, (f) evaluate_loop(prefix="test")."""
import pytest
import torch
import torch.nn as nn

from helpers import rel_err
from lookup_ref import emitted_matrix, simulate
from test_generate_gpu import B, LOW_MARGIN_SHARE, N_NEW, SEED, T, TAU, _fork, _neighbors, _prompt, _reference_steps, _wrapper

pytestmark = pytest.mark.gpu

KS = [1, 3, 7]


def _low_margin(ref, dtype, what):
    """The (sample, step) pairs below the margin, from the reference alone; their share is asserted here, before any comparison."""
    scale = ref.abs().max().item()
    top2 = ref.topk(2, dim=-1).values
    low = (top2[..., 0] - top2[..., 1]) <= 2 * TAU[dtype] * scale
    share = low.float().mean().item()
    print(f"{what}: {share * 100:.1f} % of the {low.numel()} (sample, step) pairs are below the margin")
    assert share <= LOW_MARGIN_SHARE[dtype], f"{what}: {share:.3f} of the steps are near-ties of the reference itself"
    return low


def _check_against_reference(out, stats, greedy, ref, dtype, n_new, width, what):
    """(a) and (b) for one generation `out` [rows, width + n_new] with its K = 0 twin `greedy`."""
    low = _low_margin(ref, dtype, what)
    tokens = out[:, width:].cpu()
    wrong = (tokens != ref.argmax(-1)) & ~low
    assert not wrong.any(), f"{what}: {int(wrong.sum())} tokens differ from the reference argmax at a clear margin: {wrong.nonzero().tolist()[:8]}"
    same = 0
    for b in range(out.shape[0]):
        first_low = int(low[b].nonzero()[0]) if low[b].any() else n_new
        assert torch.equal(out[b, :width + first_low], greedy[b, :width + first_low]), (what, b, first_low)
        same += first_low
    # (b) must compare something: at the fp32 margin at least half of the positions, as tests/test_generate_gpu.py asks of HF's own
    # loop; at the bf16 margin one early near-tie ends a row's comparison (up to a quarter of the pairs may be near-ties), so the
    # count is printed and only has to be positive
    print(f"{what}: {same} of {out.shape[0] * n_new} positions lie in front of a row's first near-tie and equal the K = 0 ids")
    assert same >= (out.shape[0] * n_new // 2 if dtype == torch.float32 else 1), f"{what}: only {same} positions were compared"
    em = stats["emitted"].cpu()
    assert em.shape == (stats["steps"] + 1, out.shape[0]) and em.dtype == torch.int32
    assert (em.sum(0) == n_new).all() and (em[0] == 1).all() and 1 <= stats["steps"] <= n_new - 1, (em.tolist(), stats["steps"])


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("pre_ln", [True, False], ids=["pre-LN", "post-LN"])
def test_fork_vs_hf_uncached(pre_ln, dtype, K):
    from mmgl_amd.model.modelling_cross_attention import copy_opt_weights
    hf, lm = _fork(pre_ln)
    if dtype == torch.bfloat16:                                # the reference sees the weights the bf16 product computes with
        with torch.no_grad():
            for p in hf.parameters():
                p.copy_(p.bfloat16().float())
        copy_opt_weights(hf, lm)
    ids, am = _prompt(SEED)
    lm = lm.to(dtype).cuda()
    out, stats = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, prompt_lookup_num_tokens=K, return_lookup_stats=True)
    greedy = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW)
    assert out.shape == (B, T + N_NEW) and out.dtype == ids.dtype and torch.equal(out[:, :T].cpu(), ids)
    with torch.no_grad():
        ref = _reference_steps(lambda i, m: hf(input_ids=i, attention_mask=m).logits[:, -1], out.cpu(), am, N_NEW)
    _check_against_reference(out, stats, greedy, ref, dtype, N_NEW, T, f"fork {'pre' if pre_ln else 'post'}-LN {dtype} K={K} vs HF OPT")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_wrapper_vs_oracle_uncached(dtype, K):
    """Open gates: the gated layers run m = K + 1 queries per sample on the neighbour tokens (ops.attn_decode_beam)."""
    w, nb, oracle = _wrapper(round_bf16=dtype == torch.bfloat16)
    ids, am = _prompt(SEED)
    w = w.to(dtype).cuda()
    dev = {k: v.cuda() for k, v in nb.items()}
    out, stats = w.generate(ids.cuda(), am.cuda(), **dev, max_new_tokens=N_NEW, prompt_lookup_num_tokens=K, max_matching_ngram_size=3,
                            return_lookup_stats=True)
    greedy = w.generate(ids.cuda(), am.cuda(), **dev, max_new_tokens=N_NEW)
    assert out.shape == (B, T + N_NEW)
    ref = _reference_steps(oracle, out.cpu(), am, N_NEW)
    _check_against_reference(out, stats, greedy, ref, dtype, N_NEW, T, f"CrossAttentionModel {dtype} K={K} vs oracle loop")


# ------------------------------------------------------------------------------------------ (c) the successor model
def _successor(dtype=torch.float32, pre_ln=True):
    """The fork whose greedy token is always the previous token + 1 (mod 128): the residual stream carries the token's embedding
    alone (attention and FFN outputs zeroed, no positions), and lm_head row v is the embedding of v - 1."""
    _, lm = _fork(pre_ln)
    dec = lm.model.decoder
    with torch.no_grad():
        for layer in dec.layers:
            for mod in (layer.self_attn.out_proj, layer.fc2):
                mod.weight.zero_()
                mod.bias.zero_()
        dec.embed_positions.weight.zero_()
        E = torch.randn(128, 64, generator=torch.Generator().manual_seed(SEED))
        dec.embed_tokens.weight.copy_(E)
        lm.lm_head = nn.Linear(64, 128, bias=False)            # untied from embed_tokens
        lm.lm_head.weight.copy_(torch.roll(E, 1, 0))
        # the property the traces rest on, from the weights alone: the stream is the token's embedding, then the final LayerNorm and lm_head
        fln = dec.final_layer_norm
        lg = torch.nn.functional.layer_norm(E, (64,), fln.weight, fln.bias, fln.eps) @ lm.lm_head.weight.t()
        top2 = lg.topk(2, dim=-1).values
        assert torch.equal(lg.argmax(-1), (torch.arange(128) + 1) % 128) and float(((top2[:, 0] - top2[:, 1]) / lg.abs().max()).min()) >= 0.3
    return lm.to(dtype).cuda().eval()


S_T, S_NEW, S_EOS = 24, 16, 84


def _successor_prompts():
    """ids, mask [6, 24] and the role of each row.  The first new token follows column T - 1 (generate()'s right-padded layout), so
    a padded row continues from the pad token 1."""
    up = lambda a, n: list(range(a, a + n))
    rows = [
        ("full accept", up(40, 23) + [40], 24),                               # new 41 .. 56, all of it in the prompt behind (40, 41)
        ("partial accept", up(5, 4) + up(90, 19) + [5], 24),                  # behind (5, 6): 7, 8 hold, 90 is not 9
        ("rejected drafts", [60, 20, 21, 50, 62, 64, 66, 68] + list(range(100, 70, -2)) + [20], 24),   # behind (20, 21): 50, not 22
        ("no drafts", list(range(126, 80, -2)) + [10], 24),                   # nothing in 11 .. 26 occurs earlier
        ("EOS inside a block", up(80, 23) + [80], 24),                        # new 81, 82, 83, 84 = EOS
        ("ragged right padding", up(2, 10) + [70, 2], 12),                    # 12 valid columns, then pads: new 2, 3, ... behind the pad
    ]
    ids = torch.ones(len(rows), S_T, dtype=torch.int64)
    am = torch.zeros(len(rows), S_T, dtype=torch.int64)
    for b, (_, toks, n) in enumerate(rows):
        assert len(toks) == n
        ids[b, :n] = torch.tensor(toks)
        am[b, :n] = 1
    return ids, am, [r[0] for r in rows]


def _successor_expectation(ids, am, K, N, eos, pad=1):
    """Expected new tokens [rows, S_NEW] by the successor rule and the per-row traces by simulation."""
    new, traces = [], []
    for b in range(ids.shape[0]):
        toks = [(int(ids[b, -1]) + 1 + s) % 128 for s in range(S_NEW)]
        if eos in toks:
            cut = toks.index(eos) + 1
            toks = toks[:cut] + [pad] * (S_NEW - cut)
        new.append(toks)
        traces.append(simulate([int(t) for t, a in zip(ids[b], am[b]) if a], toks, K, N, eos))
    return torch.tensor(new), traces


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K", [3, 7])
def test_successor_model_traces(K, dtype):
    N = 2
    ids, am, roles = _successor_prompts()
    new, traces = _successor_expectation(ids, am, K, N, S_EOS)
    tr = dict(zip(roles, traces))
    # the cases, established on the CPU before anything runs on the GPU
    assert any(c["k"] == K + 1 for c in tr["full accept"]) and len(tr["full accept"]) - 1 < S_NEW - 1
    assert any(0 < c["k"] - 1 < c["nd"] for c in tr["partial accept"])
    assert any(c["nd"] > 0 and c["k"] == 1 for c in tr["rejected drafts"])
    assert all(c["nd"] == 0 and c["k"] == 1 for c in tr["no drafts"]) and len(tr["no drafts"]) == S_NEW
    eos_call = tr["EOS inside a block"][-1]
    assert eos_call["eos_at"] is not None and 0 < eos_call["eos_at"] < eos_call["nd"] and sum(c["k"] for c in tr["EOS inside a block"]) < S_NEW
    assert any(c["k"] == K + 1 for c in tr["ragged right padding"]) and new[5, 0] == 2
    lm = _successor(dtype)
    out, stats = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=S_NEW, eos_token_id=S_EOS, pad_token_id=1, prompt_lookup_num_tokens=K,
                             max_matching_ngram_size=N, return_lookup_stats=True)
    assert torch.equal(out.cpu(), torch.cat([ids, new], 1)), out[:, S_T:].tolist()
    assert torch.equal(out, lm.generate(ids.cuda(), am.cuda(), max_new_tokens=S_NEW, eos_token_id=S_EOS, pad_token_id=1))
    steps = max(len(t) for t in traces) - 1
    assert stats["steps"] == steps == S_NEW - 1                                        # the row without drafts needs every step
    assert torch.equal(stats["emitted"].cpu(), emitted_matrix(traces, steps)), stats["emitted"].tolist()
    # the rows whose drafts are accepted, on their own: fewer steps than tokens
    pick = [roles.index(r) for r in ("full accept", "EOS inside a block", "ragged right padding")]
    out2, stats2 = lm.generate(ids[pick].cuda(), am[pick].cuda(), max_new_tokens=S_NEW, eos_token_id=S_EOS, pad_token_id=1,
                               prompt_lookup_num_tokens=K, max_matching_ngram_size=N, return_lookup_stats=True)
    steps2 = max(len(traces[b]) for b in pick) - 1
    assert torch.equal(out2, out[pick]) and stats2["steps"] == steps2 < S_NEW - 1
    assert torch.equal(stats2["emitted"].cpu(), emitted_matrix([traces[b] for b in pick], steps2))
    print(f"successor K={K} {dtype}: {steps} steps for the batch, {steps2} for the accepting rows, {S_NEW - 1} greedy")


def test_successor_model_more_than_64_rows():
    """B (K + 1) = 72 rows: every GEMM of a verify step goes through ops.decode_linear's chunks of 64 rows."""
    K, N, rows = 7, 2, 9
    ids = torch.tensor([list(range(3 + 11 * b, 26 + 11 * b)) + [3 + 11 * b] for b in range(rows)])
    am = torch.ones_like(ids)
    new, traces = _successor_expectation(ids, am, K, N, None)
    assert all([c["k"] for c in t] == [1, 8, 7] for t in traces)                      # every draft accepted, then the row is full
    lm = _successor(torch.bfloat16)
    out, stats = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=S_NEW, prompt_lookup_num_tokens=K, max_matching_ngram_size=N,
                             return_lookup_stats=True)
    assert torch.equal(out.cpu(), torch.cat([ids, new], 1)), out[:, S_T:].tolist()
    assert torch.equal(out, lm.generate(ids.cuda(), am.cuda(), max_new_tokens=S_NEW))
    assert stats["steps"] == 2 and torch.equal(stats["emitted"].cpu(), emitted_matrix(traces, 2))


# ------------------------------------------------------------------------------------------ (d) the cache
def _generate_with_cache(lm, ids, am, **kw):
    caches = []
    hook = lm.model.decoder.register_forward_hook(lambda mod, args, out: caches.append(out.past_key_values))
    try:
        out = lm.generate(ids, am, **kw)
    finally:
        hook.remove()
    return out, caches[0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_cache_after_generation_matches_the_greedy_cache(dtype):
    """Rows whose ids agree in both runs: every frozen layer's keys and values at columns [T, len) are the projections of the same
    tokens' layer inputs, computed by the same GEMM kernel at another row count: equal to TAU of the file's comparison rule."""
    _, lm = _fork()
    lm = lm.to(dtype).cuda()
    ids, am = _prompt(SEED)
    out, cache = _generate_with_cache(lm, ids.cuda(), am.cuda(), max_new_tokens=N_NEW, prompt_lookup_num_tokens=3)
    ref, ref_cache = _generate_with_cache(lm, ids.cuda(), am.cuda(), max_new_tokens=N_NEW)
    assert cache.lookup is not None and ref_cache.lookup is None and ref_cache.col == T + N_NEW - 1 == cache.capacity
    lens = cache.lookup.len.cpu()
    assert (lens == T + N_NEW - 1).all() and (cache.lookup.gen.cpu() == N_NEW).all()
    rows = [b for b in range(B) if torch.equal(out[b], ref[b])]
    assert len(rows) >= B // 2, rows
    assert (cache.mask[:, T:] == 1).all() and torch.equal(cache.mask[:, :T], ref_cache.mask[:, :T])
    for idx, (kv, kv_ref) in enumerate(zip(cache.kv, ref_cache.kv)):
        assert rel_err(kv[:, :T].float(), kv_ref[:, :T].float()) <= TAU[dtype]        # the prefill is the same code
        err = rel_err(kv[rows, T:].float(), kv_ref[rows, T:].float())
        print(f"cache layer {idx} {dtype}: rel err of the generated columns {err:.3e}")
        assert err <= TAU[dtype], (idx, err)


# ------------------------------------------------------------------------------------------ (e) limits and refusals
def test_last_position_of_the_table_clamp_and_skip():
    """T + n_new - 1 == max_position_embeddings with K = 7: the drafts behind the last token have positions past the table (clamped by
    ops.lookup_accept) and cache columns past the capacity (dropped by ops.attn_decode_block); the ids are the greedy ids."""
    lm = _successor()
    width, n_new = 49, 16
    assert width + n_new - 1 == lm.model.decoder.max_target_positions
    ids = torch.tensor([list(range(40, 88)) + [40], list(range(30, 60)) + list(range(90, 108)) + [30]])
    am = torch.ones_like(ids)
    out, stats = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=n_new, prompt_lookup_num_tokens=7, return_lookup_stats=True)
    want = torch.stack([ids[:, -1] + 1 + s for s in range(n_new)], 1)
    assert torch.equal(out.cpu(), torch.cat([ids, want], 1))
    assert torch.equal(out, lm.generate(ids.cuda(), am.cuda(), max_new_tokens=n_new))
    traces = [simulate(ids[b].tolist(), want[b].tolist(), 7, 2) for b in range(2)]
    assert traces[0][-1]["nd"] > traces[0][-1]["k"] - 1                               # drafts reached behind token n_new - 1
    assert torch.equal(stats["emitted"].cpu(), emitted_matrix(traces, stats["steps"])) and stats["steps"] < n_new - 1
    with pytest.raises(ValueError, match="max_position_embeddings"):
        lm.generate(ids.cuda(), am.cuda(), max_new_tokens=n_new + 1, prompt_lookup_num_tokens=7)


def test_refusals_and_the_default_path():
    _, lm = _fork()
    lm = lm.cuda()
    ids, am = _prompt(SEED)
    ids, am = ids.cuda(), am.cuda()
    base = lm.generate(ids, am, max_new_tokens=4)
    assert torch.is_tensor(base)
    assert torch.equal(lm.generate(ids, am, max_new_tokens=4, prompt_lookup_num_tokens=0, max_matching_ngram_size=2), base)
    with pytest.raises(ValueError, match="return_lookup_stats"):
        lm.generate(ids, am, max_new_tokens=4, return_lookup_stats=True)
    for kw in (dict(do_sample=True), dict(num_beams=2), dict(repetition_penalty=1.3), dict(min_new_tokens=2, eos_token_id=2),
               dict(return_step_logits=True), dict(max_matching_ngram_size=5), dict(prompt_lookup_num_tokens=8)):
        with pytest.raises(ValueError):
            lm.generate(ids, am, max_new_tokens=4, **{**dict(prompt_lookup_num_tokens=3), **kw})
    with pytest.raises(ValueError, match="inputs_embeds"):
        lm.generate(inputs_embeds=torch.randn(2, 5, 64, device="cuda"), max_new_tokens=4, prompt_lookup_num_tokens=3)
    # a decode step still takes one token per sample, and a verify step needs the LookupState
    dec = lm.model.decoder
    with torch.no_grad():
        o = lm(input_ids=ids, attention_mask=am, use_cache=True, cache_capacity=T + 4)
        with pytest.raises(ValueError, match="one new token"):
            lm(input_ids=ids[:, :2], past_key_values=o.past_key_values)
        with pytest.raises(ValueError, match="LookupState"):
            dec._verify_step(o.past_key_values)

    class Adapted(nn.Linear):                                  # stands for any adapted projection: not a plain nn.Linear
        pass
    v = dec.layers[1].self_attn.v_proj
    ad = Adapted(64, 64).cuda()
    ad.load_state_dict(v.state_dict())
    dec.layers[1].self_attn.v_proj = ad
    with pytest.raises(ValueError, match="nn.Linear"):
        lm.generate(ids, am, max_new_tokens=4, prompt_lookup_num_tokens=3)
    # one new token: the prefill's row is the whole generation, no verify step runs
    dec.layers[1].self_attn.v_proj = v
    one, stats = lm.generate(ids, am, max_new_tokens=1, prompt_lookup_num_tokens=3, return_lookup_stats=True)
    assert torch.equal(one, base[:, :T + 1]) and stats["steps"] == 0 and stats["emitted"].cpu().tolist() == [[1] * B]
    # int32 prompts come back as int32
    assert lm.generate(ids.int(), am, max_new_tokens=4, prompt_lookup_num_tokens=3).dtype == torch.int32


# ------------------------------------------------------------------------------------------ (f) the test protocol
def test_evaluate_loop_passes_prompt_lookup(tmp_path):
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
    model = build_model(args, tokenizer, offline=True).float().cuda().eval()
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if n_.endswith(("gating1", "gating2")):
                p.fill_(0.5)
    _, val_ds, _ = build_datasets(args, tokenizer)
    loader = lambda: DataLoader(Subset(val_ds, list(range(8))), batch_size=4, shuffle=False, num_workers=0, drop_last=True)
    calls, real = [], model.generate

    def recording(**kw):
        out = real(**kw)
        calls.append((kw.get("prompt_lookup_num_tokens", 0), kw.get("max_matching_ngram_size"), out.clone()))
        return out
    model.generate = recording
    try:
        evaluate_loop(loader(), model, tokenizer, 0, args, prefix="test")
        plain, plain_meters = list(calls), dict(evaluate_loop.last)
        del calls[:]
        args.prompt_lookup_num_tokens = 3
        evaluate_loop(loader(), model, tokenizer, 0, args, prefix="test")
        looked, looked_meters = list(calls), dict(evaluate_loop.last)
        del calls[:]
        args.num_beams = 2                                                             # not a plain greedy run: the keyword stays away
        evaluate_loop(loader(), model, tokenizer, 0, args, prefix="test")
        beams = list(calls)
    finally:
        del model.generate
    assert len(plain) == len(looked) >= 1 and all(c[0] == 0 for c in plain) and all(c[0] == 3 and c[1] == 2 for c in looked)
    for a, b in zip(plain, looked):
        assert torch.equal(a[2], b[2])                                                 # the same ids: the same captions
    assert plain_meters == looked_meters
    assert all(c[0] == 0 for c in beams)
