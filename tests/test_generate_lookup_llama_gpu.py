"""-m gpu: prompt-lookup decoding on the Llama-family LM, LlamaNeighborLM.generate(prompt_lookup_num_tokens=K).  The
result is the greedy result in fewer steps.  Models, prompts, neighbors and SEED are those of tests/test_generate_llama_gpu.py.

(a) against the uncached reference run on the product's own tokens, under that file's rule: the low-margin share of the reference is
    asserted first at its caps (<= 5 % fp32, <= 40 % bf16; margin 2 tau max|logit|), then every returned token equals the reference's
    argmax outside the low-margin pairs.  There are no step logits to compare.  HF LlamaForCausalLM at gates 0 (fp32 tiny, Hkv = 4, 2,
    1 = H, D = 16), the oracle loop at open gates (the same, and the bf16 models A: Hkv = 2, D = 64 and B: Hkv = 1, D = 128); K = 1,
    3, 7.  The shares of these inputs on the reference's own greedy tokens, recomputed on the CPU: gates 0 2.3 / 3.1 / 1.6 %, gates
    open 1.6 / 0.8 / 3.1 % (Hkv 4 / 2 / 1), A 31.2 %, B 26.6 % -- the figures tests/test_generate_llama_gpu.py records.
(b) the ids equal the K = 0 ids of the same model up to each row's first low-margin step; at least half of the positions are compared
    in fp32 and at least one in bf16.
(c) a successor Llama -- o_proj and down_proj zeroed in every frozen layer (gates 0: the gated layers add nothing), so that the
    residual stream is the token's embedding; lm_head row v = embedding row v - 1, so that every greedy token is the previous one + 1.
    _successor asserts the relative top-2 margin >= 0.3 from the weights on the CPU (this file's embedding draw, SUCC_SEED: 0.375 in fp32
    and 0.376 on bf16-rounded weights).  The prompts of tests/test_generate_lookup_gpu.py: full accept, partial accept, rejected
    drafts, no drafts, EOS inside an accepted block, ragged right padding.  The ids are exact and `emitted` is the simulated trace.
(d) the cache after generation against the cache of a K = 0 run: this pins the rotary position len[b] + i of every filed key.
(e) the limits: the last position of the table with K = 7, B (K + 1) = 72 rows, K = 0 bitwise, the cache row width."""
import pytest
import torch

from helpers import rel_err
from lookup_ref import emitted_matrix, simulate
from test_generate_llama_gpu import (B, BF16_LOGITS_TOL, LOW_MARGIN_SHARE, MODELS, N_NEW, SEED, T, TAU, _generate, _hf_last_logits, _lm,
                                     _neighbors, _oracle_last_logits, _prompt, _reference_steps, low_margin)
from test_generate_lookup_gpu import S_EOS, S_NEW, S_T, _successor_expectation, _successor_prompts

pytestmark = pytest.mark.gpu

KS = [1, 3, 7]
SUCC_SEED = 1              # seeds 0 and 2 draw embeddings with margins 0.24 and 0.26: the seed is not free to change


def _check_against_reference(out, stats, greedy, ref, dtype, n_new, width, what):
    """(a) and (b) for one generation `out` [rows, width + n_new] with its K = 0 twin `greedy`."""
    low = low_margin(ref, TAU[dtype])
    share = low.float().mean().item()
    print(f"{what}: {share * 100:.1f} % of the {low.numel()} (sample, step) pairs are below the margin 2 tau max|logit|")
    assert share <= LOW_MARGIN_SHARE[dtype], f"{what}: {share:.3f} of the steps are near-ties of the reference itself"
    tokens = out[:, width:].cpu()
    wrong = (tokens != ref.argmax(-1)) & ~low
    assert not wrong.any(), f"{what}: {int(wrong.sum())} tokens differ from the reference argmax at a clear margin: {wrong.nonzero().tolist()[:8]}"
    same = 0
    for b in range(out.shape[0]):
        first_low = int(low[b].nonzero()[0]) if low[b].any() else n_new
        assert torch.equal(out[b, :width + first_low], greedy[b, :width + first_low]), (what, b, first_low)
        same += first_low
    print(f"{what}: {same} of {out.shape[0] * n_new} positions lie in front of a row's first near-tie and equal the K = 0 ids")
    assert same >= (out.shape[0] * n_new // 2 if dtype == torch.float32 else 1), f"{what}: only {same} positions were compared"
    em = stats["emitted"].cpu()
    assert em.shape == (stats["steps"] + 1, out.shape[0]) and em.dtype == torch.int32
    assert (em.sum(0) == n_new).all() and (em[0] == 1).all() and 1 <= stats["steps"] <= n_new - 1, (em.tolist(), stats["steps"])
    print(f"{what}: {stats['steps']} verify steps for {n_new} tokens")


def _run_pair(lm, ids, am, ne, valid, K, N):
    out, stats = _generate(lm, ids, am, ne, valid, prompt_lookup_num_tokens=K, max_matching_ngram_size=N, return_lookup_stats=True)
    greedy = _generate(lm, ids, am, ne, valid)
    assert out.shape == (B, T + N_NEW) and out.dtype == ids.dtype and torch.equal(out[:, :T].cpu(), ids)
    return out, stats, greedy


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n_kv", [4, 2, 1])
def test_fp32_gates_zero_vs_hf_llama(n_kv, K):
    lm = _lm("tiny", n_kv, gates=False)
    ref_fn = _hf_last_logits(lm)
    ids, am = _prompt(SEED, ragged=False)
    ne, valid = _neighbors(SEED, 64)
    out, stats, greedy = _run_pair(lm.cuda(), ids, am, ne, valid, K, 2)
    ref = _reference_steps(ref_fn, out.cpu(), am, N_NEW)
    _check_against_reference(out, stats, greedy, ref, torch.float32, N_NEW, T, f"Hkv={n_kv} fp32 gates 0 K={K} vs HF Llama")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n_kv", [4, 2, 1])
def test_fp32_gates_open_vs_oracle_loop(n_kv, K):
    """Open gates and ragged prompts: the gated layers run K + 1 queries per sample on the neighbor tokens (ops.attn_decode_beam); N = 1
    drafts behind every repeated token, so the blocks are seldom empty."""
    lm = _lm("tiny", n_kv)
    ne, valid = _neighbors(SEED, 64)
    ref_fn = _oracle_last_logits(lm, "tiny", ne, valid)
    ids, am = _prompt(SEED)
    out, stats, greedy = _run_pair(lm.cuda(), ids, am, ne, valid, K, 1)
    ref = _reference_steps(ref_fn, out.cpu(), am, N_NEW)
    _check_against_reference(out, stats, greedy, ref, torch.float32, N_NEW, T, f"Hkv={n_kv} fp32 gates open K={K} vs oracle loop")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("kind", ["A", "B"])
def test_bf16_vs_fp32_oracle_of_the_rounded_weights(kind, K):
    lm = _lm(kind).bfloat16()
    ne, valid = _neighbors(SEED, MODELS[kind]["hidden"])
    ne = ne.bfloat16()
    ref_fn = _oracle_last_logits(lm, kind, ne, valid)
    ids, am = _prompt(SEED)
    out, stats, greedy = _run_pair(lm.cuda(), ids, am, ne, valid, K, 1)
    ref = _reference_steps(ref_fn, out.cpu(), am, N_NEW)
    _check_against_reference(out, stats, greedy, ref, torch.bfloat16, N_NEW, T, f"model {kind} bf16 K={K} vs fp32 oracle loop")


# ------------------------------------------------------------------------------------------ (c) the successor model
def _successor(dtype=torch.float32, n_kv=2, max_pos=256):
    """The Llama whose greedy token is always the previous token + 1 (mod 128): attention and MLP outputs zeroed, gates 0, so the
    residual stream carries the token's embedding alone, and lm_head row v is the embedding of v - 1.  The margin is asserted from the
    weights the product computes with (for bf16: the rounded ones), on the CPU, before the model moves."""
    lm = _lm("tiny", n_kv, gates=False, max_pos=max_pos)
    with torch.no_grad():
        for layer in lm.llama.model.layers:
            layer.self_attn.o_proj.weight.zero_()
            layer.mlp.down_proj.weight.zero_()
        E = torch.randn(128, 64, generator=torch.Generator().manual_seed(SUCC_SEED))
        lm.llama.model.embed_tokens.weight.copy_(E)
        lm.llama.lm_head.weight.copy_(torch.roll(E, 1, 0))
        assert lm.llama.lm_head.weight.data_ptr() != lm.llama.model.embed_tokens.weight.data_ptr()       # an untied head
        lm = lm.to(dtype)
        Er, Wr, g = lm.llama.model.embed_tokens.weight.float(), lm.llama.lm_head.weight.float(), lm.llama.model.norm.weight.float()
        x = Er * torch.rsqrt(Er.pow(2).mean(-1, keepdim=True) + lm.config.rms_norm_eps) * g
        lg = x @ Wr.t()
        top2 = lg.topk(2, dim=-1).values
        margin = float(((top2[:, 0] - top2[:, 1]) / lg.abs().max()).min())
        print(f"successor Llama {dtype}: relative top-2 margin {margin:.3f}")
        assert torch.equal(lg.argmax(-1), (torch.arange(128) + 1) % 128) and margin >= 0.3
    return lm.cuda().eval()


@pytest.mark.parametrize("dtype,n_kv", [(torch.float32, 2), (torch.bfloat16, 1), (torch.float32, 4)], ids=["fp32-Hkv2", "bf16-Hkv1", "fp32-Hkv4"])
@pytest.mark.parametrize("K", [3, 7])
def test_successor_model_traces(K, dtype, n_kv):
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
    lm = _successor(dtype, n_kv)
    kw = dict(max_new_tokens=S_NEW, eos_token_id=S_EOS, pad_token_id=1)
    out, stats = lm.generate(ids.cuda(), am.cuda(), prompt_lookup_num_tokens=K, max_matching_ngram_size=N, return_lookup_stats=True, **kw)
    assert torch.equal(out.cpu(), torch.cat([ids, new], 1)), out[:, S_T:].tolist()
    assert torch.equal(out, lm.generate(ids.cuda(), am.cuda(), **kw))
    steps = max(len(t) for t in traces) - 1
    assert stats["steps"] == steps == S_NEW - 1                                        # the row without drafts needs every step
    assert torch.equal(stats["emitted"].cpu(), emitted_matrix(traces, steps)), stats["emitted"].tolist()
    # the rows whose drafts are accepted, on their own: fewer steps than tokens
    pick = [roles.index(r) for r in ("full accept", "EOS inside a block", "ragged right padding")]
    out2, stats2 = lm.generate(ids[pick].cuda(), am[pick].cuda(), prompt_lookup_num_tokens=K, max_matching_ngram_size=N,
                               return_lookup_stats=True, **kw)
    steps2 = max(len(traces[b]) for b in pick) - 1
    assert torch.equal(out2, out[pick]) and stats2["steps"] == steps2 < S_NEW - 1
    assert torch.equal(stats2["emitted"].cpu(), emitted_matrix([traces[b] for b in pick], steps2))
    print(f"successor Llama K={K} {dtype} Hkv={n_kv}: {steps} steps for the batch, {steps2} for the accepting rows, {S_NEW - 1} greedy")


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
def _generate_with_cache(lm, ids, am, ne, valid, **kw):
    caches, real = [], lm._hidden

    def recording(*a, **k):
        out = real(*a, **k)
        caches.append(out[1])
        return out
    lm._hidden = recording
    try:
        out = _generate(lm, ids, am, ne, valid, **kw)
    finally:
        del lm._hidden
    return out, caches[0]


@pytest.mark.parametrize("dtype,n_kv,K", [(torch.float32, 2, 3), (torch.float32, 1, 7), (torch.bfloat16, 2, 3)], ids=["fp32-Hkv2-K3", "fp32-Hkv1-K7", "bf16-Hkv2-K3"])
def test_cache_after_generation_matches_the_greedy_cache(dtype, n_kv, K):
    """Cache column c of a frozen layer holds the rotated key and the value of the token at ids column c, computed from the layer
    input of that token: where the two runs agree on the ids up to column c, the columns are the same quantities computed by the same
    GEMM kernel at another row count and rotated at position c by another kernel -- equal to the tolerance the file of the K = 0 path
    holds cached against uncached logits to (1e-3 fp32, 2.5e-2 bf16 max-norm relative; DESIGN.md 4.11 measured 4e-7 / 7e-3).  A key
    rotated at another position is a rotation of O(1) radians away.  N = 1: most blocks carry drafts, so i > 0 is exercised."""
    tol = 1e-3 if dtype == torch.float32 else BF16_LOGITS_TOL
    lm = _lm("tiny", n_kv).to(dtype).cuda()
    ne, valid = _neighbors(SEED, 64)
    ne = ne.to(dtype)
    ids, am = _prompt(SEED)
    (out, stats), cache = _generate_with_cache(lm, ids, am, ne, valid, prompt_lookup_num_tokens=K, max_matching_ngram_size=1,
                                               return_lookup_stats=True)
    ref, ref_cache = _generate_with_cache(lm, ids, am, ne, valid)
    cap = T + N_NEW - 1
    assert cache.lookup is not None and cache.lookup.scratch is None and ref_cache.lookup is None
    assert ref_cache.col == cap == cache.capacity and cache.col == T
    assert (cache.lookup.len.cpu() == cap).all() and (cache.lookup.gen.cpu() == N_NEW).all()
    assert all(kv.shape == (B, cap, 2 * n_kv * 16) for kv in cache.kv) and len(cache.kv) == 4          # 2 Hkv D columns per row
    assert (cache.mask[:, T:] == 1).all() and torch.equal(cache.mask[:, :T], ref_cache.mask[:, :T])
    assert (stats["emitted"].cpu() > 1).any(), "no draft was accepted: every key was filed as token 0 of its block"
    # columns [T, T + f) of row b, f = the first new token the two runs disagree on (all N_NEW - 1 filed columns when they agree)
    agree = (out[:, T:] == ref[:, T:]).cpu()
    upto = [int((~agree[b]).nonzero()[0]) if not agree[b].all() else N_NEW - 1 for b in range(B)]
    upto = [min(f, N_NEW - 1) for f in upto]
    compared = sum(upto)
    print(f"cache {dtype} Hkv={n_kv} K={K}: {compared} of {B * (N_NEW - 1)} generated columns compared, {stats['steps']} verify steps")
    assert compared >= (B * (N_NEW - 1) // 2 if dtype == torch.float32 else 1)
    for idx, (kv, kv_ref) in enumerate(zip(cache.kv, ref_cache.kv)):
        assert rel_err(kv[:, :T].float(), kv_ref[:, :T].float()) <= tol                # the prefill is the same code
        got = torch.cat([kv[b, T:T + f] for b, f in enumerate(upto)]).float()
        want = torch.cat([kv_ref[b, T:T + f] for b, f in enumerate(upto)]).float()
        err = rel_err(got, want)
        print(f"cache layer {idx} {dtype}: rel err of the generated columns {err:.3e}")
        assert err <= tol, (idx, err)
        # the check can fail: the reference's own next column is not within 10 tolerances of a column
        if compared > B:
            nxt = torch.cat([kv_ref[b, T + 1:T + f] for b, f in enumerate(upto)]).float()
            assert rel_err(nxt, torch.cat([kv_ref[b, T:T + max(f - 1, 0)] for b, f in enumerate(upto)]).float()) > 10 * tol


# ------------------------------------------------------------------------------------------ (e) limits
def test_last_position_of_the_table_clamp_and_drop():
    """T + n_new - 1 == max_position_embeddings with K = 7: the drafts behind the last token have positions past the rotary table (read
    at its last row) and cache columns past the capacity (dropped by ops.rope_kv_append_block); the ids are the greedy ids."""
    width, n_new = 49, 16
    lm = _successor(max_pos=width + n_new - 1)
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


def test_last_position_on_a_random_model_gives_the_greedy_ids():
    """The same limit where attention matters: the tiny random Llama with open gates at T + n_new - 1 == max_position_embeddings = 32,
    K = 7, N = 1, against its K = 0 ids up to each row's first low-margin step of the oracle."""
    lm = _lm("tiny", 2, max_pos=32)
    ne, valid = _neighbors(SEED, 64)
    ref_fn = _oracle_last_logits(lm, "tiny", ne, valid)
    ids, am = _prompt(SEED)
    n_new = 21
    lm = lm.cuda()
    out, stats = _generate(lm, ids, am, ne, valid, n_new=n_new, prompt_lookup_num_tokens=7, max_matching_ngram_size=1, return_lookup_stats=True)
    greedy = _generate(lm, ids, am, ne, valid, n_new=n_new)
    ref = _reference_steps(ref_fn, out.cpu(), am, n_new)
    _check_against_reference(out, stats, greedy, ref, torch.float32, n_new, T, "tiny fp32 at the table's last position, K=7")


def test_default_path_and_small_generations():
    lm = _lm("tiny", 2).cuda()
    ne, valid = _neighbors(SEED, 64)
    ids, am = _prompt(SEED)
    base, base_steps = _generate(lm, ids, am, ne, valid, n_new=4, return_step_logits=True)
    out, steps = _generate(lm, ids, am, ne, valid, n_new=4, return_step_logits=True, prompt_lookup_num_tokens=0, max_matching_ngram_size=2,
                           return_lookup_stats=False)
    assert torch.equal(out, base) and torch.equal(steps, base_steps)                   # K = 0: bitwise the call without the keywords
    with pytest.raises(ValueError, match="return_lookup_stats"):
        _generate(lm, ids, am, ne, valid, n_new=4, return_lookup_stats=True)
    # one new token: the prefill's row is the whole generation, no verify step runs
    one, stats = _generate(lm, ids, am, ne, valid, n_new=1, prompt_lookup_num_tokens=3, return_lookup_stats=True)
    assert torch.equal(one, base[:, :T + 1]) and stats["steps"] == 0 and stats["emitted"].cpu().tolist() == [[1] * B]
    # int32 prompts come back as int32
    assert lm.generate(ids.int().cuda(), am.cuda(), max_new_tokens=4, prompt_lookup_num_tokens=3).dtype == torch.int32
    # a decode step still takes one token per sample, and a verify step needs the LookupState
    with torch.no_grad():
        o = lm(input_ids=ids.cuda(), attention_mask=am.cuda(), use_cache=True, cache_capacity=T + 4)
        with pytest.raises(ValueError, match="one new token"):
            lm(input_ids=ids[:, :2].cuda(), past_key_values=o.past_key_values)
        with pytest.raises(ValueError, match="LookupState"):
            lm._verify_step(o.past_key_values)
