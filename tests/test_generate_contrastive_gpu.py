"""-m gpu: generate(penalty_alpha, top_k) of MPTForCausalLM / CrossAttentionModel -- contrastive search on the beam-shared cache
(DESIGN.md 4.17).

Comparison rule (the beam suite): at every step the restatement of tests/contrastive_ref.py runs UNCACHED on the
product's own tokens and candidates, so one near-tie cannot cascade.  p / penalty / score of the trace lie within a tolerance of it;
`selected` equals the restatement's wherever its margin (best minus second score) is at least twice that tolerance, and the share of
(sample, step) pairs below that margin is asserted from the restatement alone before anything is compared (<= 5 % fp32, <= 40 % bf16).

fp32 tolerance.  The beam suite's, 2 tau max|logit| with tau = 1e-3, is 4e-3 .. 6e-3 here, and the score margins of the tiny random
models are of that size (median 5e-3 .. 3e-2: p is at most 0.1): at that tolerance 17 - 75 % of the restatement's own steps are
near-ties on every seed 0 .. 7, far above the 5 % cap, and nothing would be compared.  The tests use a hundredth of it, tau = 1e-5 --
the relative score error the beam suite asserts for the fp32 fork against transformers -- which asks more on both counts: closer
values, and equal selections at more steps.  tests/test_contrastive_cpu.py holds the share at that margin on the CPU.

bf16 tolerance.  Measured on an MI355X against the fp32 oracle of the bf16-rounded weights, doubled (the kernels are deterministic;
the factor covers other seeds).  Largest |p, penalty, score| deviation of the CrossAttentionModel trace, k = 2 / k = 4:
seed 1: 1.56e-3 / 1.54e-3, seed 2: 2.97e-3 / 2.02e-3, seed 3: 1.53e-3 / 2.07e-3, seed 4: 1.71e-3 / 2.02e-3 (the penalty leads; fp32 on the
same cases: 1.5e-7 .. 2.2e-7).  The wrapper cases run seed 4, where 2.021e-3 was measured: BF16_TOL = 4.042e-3, and 25 % (k = 2) and
33 % (k = 4) of the restatement's steps lie below the margin 2 BF16_TOL.  At the suites' usual seed 1 that share is 41.7 % for k = 4,
above the 40 % cap, so the seed was picked as for the fp32 cases."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from contrastive_ref import penalty_ref, step_ref
from helpers import mpt_args
from test_generate_gpu import SEED, T, TAU, _fork, _prompt, _wrapper

pytestmark = pytest.mark.gpu

B, N_NEW, V, ALPHA = 3, 8, 128, 0.6
TAU32 = 1e-5                      # see the module docstring
BF16_TOL = 2 * 2.021e-3            # 2 x the largest |p, penalty, score| deviation measured (module docstring)
WRAPPER_SEED = 4
NEAR_TIE_CAP = {torch.float32: 0.05, torch.bfloat16: 0.40}


def _closure(fn):
    """The variables a nested function captured, by name (the oracle of test_generate_gpu._wrapper keeps its weights there)."""
    return dict(zip(fn.__code__.co_freevars, (c.cell_contents for c in fn.__closure__)))


def _check_trace(trace, out, hidden_fn, head_fn, ids, am, k, tol, dtype, what):
    """The comparison rule of the module docstring; tol None: 2 TAU32 max|logit| of the restatement.  Returns the largest deviation."""
    new = out[:, T:].cpu()
    assert len(trace) == N_NEW and out.shape == (B, T + N_NEW) and torch.equal(out[:, :T].cpu(), ids)
    refs = []
    for s, st in enumerate(trace):
        cands, sel = st["candidates"].cpu().long(), st["selected"].cpu().long()
        assert cands.shape == (B, k) and all(len(set(r)) == k for r in cands.tolist()), (what, s)
        score = st["score"].cpu()
        assert all(int(sel[b]) == int(torch.nonzero(score[b] == score[b].max())[0]) for b in range(B)), (what, s, "selected is not the lowest argmax")
        assert torch.equal(new[:, s], cands.gather(1, sel[:, None])[:, 0]), (what, s, "the ids column is not the selected candidate")
        refs.append(step_ref(hidden_fn, head_fn, ids, am, new[:, :s], cands, ALPHA))
    if tol is None:
        tol = 2 * TAU32 * max(float(r["logits"].abs().max()) for r in refs)
    near = torch.stack([r["margin"] for r in refs], 1) < 2 * tol
    share = float(near.float().mean())
    print(f"{what}: tolerance {tol:.3e}, {share * 100:.1f} % of the {near.numel()} (sample, step) pairs are near-ties of the restatement")
    assert share <= NEAR_TIE_CAP[dtype], f"{what}: {share:.3f} of the steps are near-ties of the restatement itself"
    worst = 0.0
    for s, (st, r) in enumerate(zip(trace, refs)):
        for key in ("p", "penalty", "score"):
            err = float((st[key].double().cpu() - r[key]).abs().max())
            worst = max(worst, err)
            assert err <= tol, f"{what} step {s}: {key} err {err:.3e} > {tol:.3e}"
        # the candidates are the restatement's top k, up to logits closer than the tolerance of the suite (2 tau max|logit|)
        top = r["logits"].topk(k, dim=-1).values[:, -1:]
        assert (r["logits"].gather(1, st["candidates"].cpu().long()) >= top - 2 * TAU[dtype] * float(r["logits"].abs().max())).all()
        wrong = (st["selected"].cpu().long() != r["selected"]) & ~near[:, s]
        assert not wrong.any(), f"{what} step {s}: selected {st['selected'].tolist()} vs {r['selected'].tolist()} at margins {r['margin'].tolist()}"
    print(f"{what}: largest |p, penalty, score| deviation {worst:.3e}")
    return worst


def _hf_fns(hf):
    return (lambda i, m: hf.model.decoder(input_ids=i, attention_mask=m).last_hidden_state), hf.lm_head


@contextlib.contextmanager
def _spy(dec):
    """Records (input_ids shape, cache) of every decoder call."""
    calls, real = [], dec.forward

    def spy(*a, **kw):
        o = real(*a, **kw)
        calls.append((tuple(kw["input_ids"].shape), o.past_key_values))
        return o
    dec.forward = spy
    try:
        yield calls
    finally:
        del dec.forward


# ------------------------------------------------------------------------------------------ numerics against the uncached restatement
@pytest.mark.parametrize("k", [2, 4, 5])
def test_fork_fp32_against_the_uncached_restatement(k):
    hf, lm = _fork()
    ids, am = _prompt(SEED, batch=B)                                          # ragged right padding
    lm = lm.cuda()
    out, trace = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, penalty_alpha=ALPHA, top_k=k, return_contrastive_trace=True)
    with torch.no_grad():
        _check_trace(trace, out, *_hf_fns(hf), ids, am, k, None, torch.float32, f"fork fp32 k={k}")
    # the penalty is live: not the greedy ids, and some step does not take the most likely candidate
    greedy = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW)
    assert not torch.equal(out, greedy) and any(int(st["selected"].max()) > 0 for st in trace)
    assert torch.equal(out, lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, penalty_alpha=ALPHA, top_k=k))      # deterministic


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cross_attention_model_against_the_oracle(dtype, k):
    """Context `all`, open gates, ragged prompts; bf16 against the fp32 oracle of the rounded weights.  The k candidates of a sample
    read its neighbor tokens once: cache.cross stays at B rows."""
    from oracle import lm_ref
    w, nb, oracle = _wrapper(seed=WRAPPER_SEED, round_bf16=dtype == torch.bfloat16)
    c = _closure(oracle)
    hidden_fn = lambda i, m: lm_ref.decoder_forward(c["lm"], c["cfg"], i, m, c["ne"][:B], c["nm"][:B])
    head_fn = lambda h: F.linear(h, c["lm"]["lm_head.weight"])
    ids, am = _prompt(WRAPPER_SEED, batch=B)
    w = w.to(dtype).cuda()
    dev = {key: v[:B].cuda() for key, v in nb.items()}
    with _spy(w.lm.model.decoder) as calls:
        out, trace = w.generate(ids.cuda(), am.cuda(), **dev, max_new_tokens=N_NEW, penalty_alpha=ALPHA, top_k=k, return_contrastive_trace=True)
    cache = calls[0][1]
    assert [cl[0] for cl in calls] == [(B, T)] + [(B * k, 1)] * N_NEW
    assert len(cache.cross) == 2 and all(t.shape[0] == B for kv in cache.cross for t in kv) and cache.cross_valid.shape[0] == B
    with torch.no_grad():
        worst = _check_trace(trace, out, hidden_fn, head_fn, ids, am, k, None if dtype == torch.float32 else BF16_TOL, dtype,
                             f"CrossAttentionModel {dtype} k={k}")
    if dtype == torch.bfloat16:
        print(f"bf16 bound {BF16_TOL:.3e} = 2 x the deviation measured when it was set; this run: {worst:.3e}")
    plain = w.lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, penalty_alpha=ALPHA, top_k=k)
    assert not torch.equal(plain, out), "the neighbors do not move the result"


# ------------------------------------------------------------------------------------------ a model whose greedy choice must survive
def test_successor_model_equals_greedy():
    """lm_head row v = embedding row v - 1 and nothing else in the stream: p_0 is nearly 1, so with alpha = 0.2
    (1 - alpha)(p_0 - p_1) exceeds 2 alpha, the largest difference two penalties can have, and every selection is candidate 0."""
    from test_generate_lookup_gpu import _successor
    alpha, k = 0.2, 4
    lm = _successor()
    dec = lm.model.decoder
    with torch.no_grad():
        E, fln = dec.embed_tokens.weight.float(), dec.final_layer_norm
        lg = F.layer_norm(E, (64,), fln.weight.float(), fln.bias.float(), fln.eps) @ lm.lm_head.weight.float().t()
        p = torch.softmax(lg.double(), -1).topk(2, dim=-1).values
    assert float(((1 - alpha) * (p[:, 0] - p[:, 1])).min()) > 2 * alpha
    ids = torch.tensor([list(range(5, 5 + T)), list(range(60, 60 + T)), [9] * T])
    am = torch.ones_like(ids)
    am[2, 4:] = 0
    ids = torch.where(am.bool(), ids, torch.ones_like(ids))
    out, trace = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, penalty_alpha=alpha, top_k=k, return_contrastive_trace=True)
    assert torch.equal(out, lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW))
    assert torch.equal(out[:, T:].cpu(), torch.stack([ids[:, -1] + 1 + s for s in range(N_NEW)], 1))
    assert all(st["selected"].tolist() == [0] * 3 for st in trace)


# ------------------------------------------------------------------------------------------ structure
def test_one_prefill_and_cache_shapes():
    _, lm = _fork()
    lm = lm.cuda()
    ids, am = _prompt(SEED, batch=B)
    k, dec, d = 4, lm.model.decoder, lm.config.hidden_size
    with _spy(dec) as calls:
        lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, penalty_alpha=ALPHA, top_k=k)
    assert [c[0] for c in calls] == [(B, T)] + [(B * k, 1)] * N_NEW                 # ONE prefill, of B rows; every step forwards k candidates
    cache = calls[0][1]
    assert all(kv.shape == (B, T, 2 * d) for kv in cache.kv) and cache.mask.shape == (B, T) and cache.col == T
    assert len(cache.beam.tail) == len(cache.kv) and all(t.shape == (B * k, N_NEW, 2 * d) for t in cache.beam.tail)
    assert cache.beam.book.src.shape == (B * k, N_NEW) and cache.beam.n_tail == N_NEW and cache.beam.book.cur == 0


def test_eos_rows_are_padded():
    _, lm = _fork()
    lm = lm.cuda()
    ids, am = _prompt(SEED, batch=B)
    kw = dict(max_new_tokens=N_NEW, penalty_alpha=ALPHA, top_k=4)
    free = lm.generate(ids.cuda(), am.cuda(), **kw).cpu()
    eos = int(free[0, T + 2])                                                  # row 0 emits it at step 2
    assert eos not in free[0, T:T + 2].tolist()
    out = lm.generate(ids.cuda(), am.cuda(), **kw, eos_token_id=eos, pad_token_id=1).cpu()
    assert out[0, T:].tolist() == free[0, T:T + 3].tolist() + [1] * (N_NEW - 3)
    others = 0
    for b in range(1, B):
        row = free[b, T:].tolist()
        if eos in row:
            e = row.index(eos)
            assert out[b, T:].tolist() == row[:e + 1] + [1] * (N_NEW - e - 1)
        else:
            others += 1
            assert torch.equal(out[b], free[b])
    assert others >= 1


def test_position_limit():
    _, lm = _fork()
    lm = lm.cuda()
    width = lm.model.decoder.max_target_positions - N_NEW
    ids, am = _prompt(SEED, width=width, batch=B)
    out = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, penalty_alpha=ALPHA, top_k=4)       # T + n_new == max_position_embeddings
    assert out.shape == (B, width + N_NEW)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW + 1, penalty_alpha=ALPHA, top_k=4)
    assert lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW + 1).shape == (B, width + N_NEW + 1)   # greedy needs one position less


def test_processors_rewrite_the_logits_in_front_of_the_top_k():
    _, lm = _fork()
    lm = lm.cuda()
    ids, am = _prompt(SEED, batch=B)
    k = 4
    kw = dict(max_new_tokens=N_NEW, penalty_alpha=ALPHA, top_k=k)
    out, steps, trace = lm.generate(ids.cuda(), am.cuda(), **kw, repetition_penalty=1.3, return_step_logits=True, return_contrastive_trace=True)
    assert steps.shape == (B, N_NEW, V)
    plain, plain_steps = lm.generate(ids.cuda(), am.cuda(), **kw, return_step_logits=True)
    assert not torch.equal(steps[:, 0], plain_steps[:, 0])                     # the processor did rewrite the prompt's tokens
    for s, st in enumerate(trace):
        want = torch.sort(steps[:, s].float(), dim=-1, descending=True, stable=True).indices[:, :k]
        assert torch.equal(st["candidates"].long(), want), s
        logp = torch.log_softmax(steps[:, s].double(), -1).gather(1, want)
        assert float((st["p"].double() - logp.exp()).abs().max()) <= 1e-5


def test_evaluate_loop_test_prefix_generates_with_contrastive_search(tmp_path):
    from torch.utils.data import DataLoader, Subset
    from mmgl_amd.language_modelling.run_generation import Arguments, build_datasets, build_model, evaluate_loop
    from mmgl_amd.wikiweb2m.synthetic import synthetic_tokenizer
    torch.manual_seed(0)
    tokenizer = synthetic_tokenizer()
    args = Arguments(model_name_or_path="mpt-tiny", dataset="synthetic", context="all", neighbor_mode="embedding", peft_type="flamingo",
                     max_input_length=32, max_output_length=12, max_text_neighbors=5, max_image_neighbors=2, n_text_tokens=2,
                     n_visual_tokens=2, per_device_val_batch_size=4, dataloader_num_workers=0, val_steps_per_epoch=2, print_freq=100,
                     log_dir=str(tmp_path), seed=0, penalty_alpha=0.6, top_k=4, prompt_lookup_num_tokens=3)
    assert Arguments(model_name_or_path="mpt-tiny").penalty_alpha == 0.0         # the default stays greedy
    args.image_size = 32
    model = build_model(args, tokenizer, offline=True).float().cuda().eval()
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if n_.endswith(("gating1", "gating2")):
                p.fill_(0.5)
    _, val_ds, _ = build_datasets(args, tokenizer)
    loader = DataLoader(Subset(val_ds, list(range(8))), batch_size=4, shuffle=False, num_workers=0, drop_last=True)
    calls, real = [], model.generate

    def counting(**kw):
        out = real(**kw)
        calls.append((kw.get("penalty_alpha"), kw.get("top_k"), kw.get("prompt_lookup_num_tokens"), tuple(kw["input_ids"].shape), tuple(out.shape)))
        return out
    model.generate = counting
    try:
        evaluate_loop(loader, model, tokenizer, 0, args, prefix="test")
    finally:
        del model.generate
    assert len(calls) >= 1 and sum(c[3][0] for c in calls) == 8, calls
    for alpha, k, lookup, shape_in, shape_out in calls:
        assert alpha == 0.6 and k == 4 and lookup is None and shape_out == (shape_in[0], args.max_input_length + 32), calls


# ------------------------------------------------------------------------------------------ the real widths
@pytest.mark.parametrize("batch", [2, 16])
def test_full_width_trace_is_consistent_with_the_products_own_hidden_rows(batch):
    """OPT-1.3B layer width (d = 2048, 32 heads, vocab 50272), random weights, 2 frozen + 1 gated layer, prompt 64, 4 new tokens,
    k = 4, bf16: B*k = 8 and 64 rows.  `selected` is the argmax of `score`; `penalty` is within the derived bound 4 d 2^-24 of an fp64
    recompute from the hidden rows the select call was given (its operands are recorded on the way in)."""
    from transformers import OPTConfig
    from mmgl_amd import ops
    from mmgl_amd.model import generation
    from mmgl_amd.model.modelling_cross_attention import MPTConfig, MPTForCausalLM
    torch.manual_seed(11)
    oc = OPTConfig(vocab_size=50272, hidden_size=2048, num_attention_heads=32, ffn_dim=8192, num_hidden_layers=2, max_position_embeddings=2048,
                   word_embed_proj_dim=2048, do_layer_norm_before=True, dropout=0.1, attention_dropout=0.0, pad_token_id=1, bos_token_id=2,
                   eos_token_id=2)
    with torch.device("cuda"):
        lm = MPTForCausalLM(MPTConfig(mpt_args(neighbor_mode="embedding", neighbor_layer_wise=2), oc))
    with torch.no_grad():
        for n_, p in lm.named_parameters():
            if n_.endswith(("gating1", "gating2")):
                p.fill_(0.5)
    lm = lm.bfloat16().eval()
    assert len(lm.model.decoder.neighbor_layers) == 1
    width, n_new, S, k, d = 64, 4, 16, 4, 2048
    ids, am = _prompt(3, width=width, batch=batch, vocab=50272)
    g = torch.Generator().manual_seed(5)
    ne = torch.randn(batch, S, d, generator=g).bfloat16().cuda()
    nv = torch.ones(batch, S, dtype=torch.bool).cuda()
    seen, real = [], ops.contrastive_select

    def recording(cand_hidden, ctx, ctx_valid, *a, **kw):
        seen.append((cand_hidden.clone(), ctx, ctx_valid, a[3]))               # a[3]: n_ctx
        return real(cand_hidden, ctx, ctx_valid, *a, **kw)
    generation.ops.contrastive_select = recording
    try:
        out, trace = lm.generate(ids.cuda(), am.cuda(), neighbor_embeds=ne, neighbor_attention_mask=nv, max_new_tokens=n_new, penalty_alpha=ALPHA,
                                 top_k=k, return_contrastive_trace=True)
    finally:
        generation.ops.contrastive_select = real
    assert out.shape == (batch, width + n_new) and len(seen) == n_new
    tol, worst = 4 * d * 2.0 ** -24, 0.0
    for s, (st, (cand, ctx, valid, n_ctx)) in enumerate(zip(trace, seen)):
        assert n_ctx == width + s
        score, sel = st["score"].cpu(), st["selected"].cpu()
        assert torch.isfinite(score).all()
        assert all(int(sel[b]) == int(torch.nonzero(score[b] == score[b].max())[0]) for b in range(batch)), s
        cand, ctx, valid = cand.cpu().float(), ctx[:, :n_ctx].cpu().float(), valid[:, :n_ctx].cpu()
        if s > 0:                                                              # the rows the earlier steps appended are the selected rows
            prev = seen[s - 1][0].cpu().float().view(batch, k, d)
            assert torch.equal(ctx[:, n_ctx - 1], prev[torch.arange(batch), trace[s - 1]["selected"].cpu().long()])
        for b in range(batch):
            pen = penalty_ref(cand[b * k:(b + 1) * k], ctx[b], valid[b])
            err = float((st["penalty"][b].double().cpu() - pen).abs().max())
            worst = max(worst, err)
            assert err <= tol, (s, b, err)
    print(f"full width B={batch}: largest penalty deviation from the fp64 recompute {worst:.3e} (bound {tol:.3e})")
