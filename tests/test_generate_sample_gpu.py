"""-m gpu: generate(do_sample=True) of the three generators (MPTForCausalLM / CrossAttentionModel, SelfAttentionModel, LlamaNeighborLM)
and num_return_sequences on the beam-shared cache.  Tiny models of the existing generate tests, B = 3, T = 12, 8 new
tokens.

Rules.  top_k = 1 is greedy decoding, exactly, once the greedy run's own step logits show no tie at the maximum (a tie is kept whole by
the sampler and cut by argmax; the prompt seed is the first of a few whose greedy run has none).  Replay: every token of a sampled run
satisfies the kernel criterion of tests/test_sample_kernels_gpu.py on the step logits the product returned, and the product's uncached
forward over its own ids reproduces those logits within the tolerance the existing generate tests of that model use.  Where the replay
runs on logits of an UNCACHED forward (num_return_sequences returns no step logits per row), the two sides' logits differ by up to
d = tau max|logit|, every unnormalised mass by a factor within e^(+-d) and every CDF value by at most e^(2d) - 1: that is added to
the draw's bound, and the case samples without filters so that the kept set is the vocabulary on both sides."""
import math

import numpy as np
import pytest
import torch

from helpers import rel_err
from sample_ref import cdf, draw_ok, eps_u, scaled
from test_generate_gpu import BF16_LOGITS_TOL, TAU, _fork, _neighbors, _prompt, _reference_steps, _uncached_last_logits, _wrapper
from test_generate_llama_gpu import _generate as _llama_generate
from test_generate_llama_gpu import _lm as _llama_lm
from test_generate_llama_gpu import _neighbors as _llama_neighbors
from test_generate_llama_gpu import _uncached_last_logits as _llama_uncached
from test_generate_selfattn_gpu import _sa, _uncached
from test_sample_kernels_gpu import _check

pytestmark = pytest.mark.gpu

B, T, N_NEW, V = 3, 12, 8, 128
DTYPES = [pytest.param(torch.float32, id="fp32"), pytest.param(torch.bfloat16, id="bf16")]
GENERATORS = ["fork", "selfattn-lora", "selfattn-prompt", "llama"]
KNOBS = dict(temperature=0.8, top_k=20, top_p=0.9)


def _generator(kind, dtype):
    """(run(ids, am, **kw) -> generate()'s result, uncached(ids, mask) -> last-position logits fp32 on the CPU, logits tolerance)."""
    if kind == "fork":
        lm = _fork()[1].to(dtype).cuda()
        return (lambda ids, am, **kw: lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, **kw),
                lambda i, m: _uncached_last_logits(lm, i, m), TAU[dtype])
    if kind.startswith("selfattn"):
        w = _sa(peft_type=kind.split("-")[1]).to(dtype).cuda()
        return lambda ids, am, **kw: w.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, **kw), _uncached(w), TAU[dtype]
    lm = _llama_lm("tiny", 2).to(dtype).cuda()
    ne, valid = _llama_neighbors(0, 64, batch=B, empty=1)
    ne = ne.to(dtype)
    return (lambda ids, am, **kw: _llama_generate(lm, ids, am, ne, valid, n_new=N_NEW, **kw), _llama_uncached(lm, ne, valid),
            1e-3 if dtype == torch.float32 else BF16_LOGITS_TOL)


def _u(seed, rows=B):
    return torch.rand(N_NEW, rows, generator=torch.Generator().manual_seed(seed)).cuda()


def _untied_prompt(run):
    """The first prompt seed whose GREEDY run has no tie at the maximum of any step's logits; (ids, am, greedy ids, step logits)."""
    for seed in range(1, 9):
        ids, am = _prompt(seed, batch=B)
        out, steps = run(ids, am, return_step_logits=True)
        top2 = steps.float().topk(2, dim=-1).values
        if bool((top2[..., 0] > top2[..., 1]).all()):
            return ids, am, out, steps
    raise AssertionError("every prompt seed has a tie at the maximum of some step: top_k = 1 cannot be compared with argmax")


def _replay(steps, out, u, knobs):
    """Every generated token against the kernel criterion on the step logits the product returned."""
    from mmgl_amd import ops
    tokens = out[:, -N_NEW:]
    for s in range(N_NEW):
        lg, us = steps[:, s].contiguous(), u[s].view(-1, 1)
        tok, kept = ops.sample_tokens(lg, us, return_kept=True, **knobs)
        assert torch.equal(tok, tokens[:, s]), f"step {s}: the ids are not what ops.sample_tokens draws from the returned step logits"
        _check(lg.cpu(), us.cpu(), knobs["temperature"], knobs["top_k"], knobs["top_p"], tok.tolist(), kept.tolist())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", GENERATORS)
def test_top_k_1_is_greedy_and_sampled_runs_replay(kind, dtype):
    run, uncached, tol = _generator(kind, dtype)
    ids, am, greedy, _ = _untied_prompt(run)
    out = run(ids, am, do_sample=True, top_k=1, sample_u=_u(1))
    assert torch.equal(out, greedy)
    out = run(ids, am, do_sample=True, top_k=1, temperature=0.5, top_p=0.3, seed=4)
    assert torch.equal(out, greedy)
    # a sampled run: replay on the returned step logits (the raw logits, before the temperature), which the uncached forward reproduces
    u = _u(2)
    out, steps = run(ids, am, do_sample=True, sample_u=u, return_step_logits=True, **KNOBS)
    assert out.shape == (B, T + N_NEW) and steps.shape == (B, N_NEW, V) and steps.dtype == dtype and torch.equal(out[:, :T].cpu(), ids)
    assert not torch.equal(out, greedy), "the sampled run is the greedy run: the case shows nothing"
    _replay(steps, out, u, KNOBS)
    ref = _reference_steps(uncached, out.cpu(), am, N_NEW)
    for s in range(N_NEW):
        err = rel_err(steps[:, s].float().cpu(), ref[:, s])
        assert err <= tol, f"{kind} {dtype} step {s}: cached vs uncached logits rel err {err:.3e} > {tol:.1e}"
    assert torch.equal(run(ids, am, do_sample=True, sample_u=u, **KNOBS), out)


def test_seeding():
    run, _, _ = _generator("fork", torch.float32)
    ids, am = _prompt(1, batch=B)
    a = run(ids, am, do_sample=True, seed=5)
    state = torch.cuda.get_rng_state()
    assert torch.equal(run(ids, am, do_sample=True, seed=5), a)
    assert torch.equal(torch.cuda.get_rng_state(), state), "a call that passes seed advanced the global generator"
    b = run(ids, am, do_sample=True, seed=6)                     # 24 draws from near-flat random-model distributions over 128 tokens
    assert not torch.equal(a[:, T:], b[:, T:]) and torch.equal(a[:, :T], b[:, :T])
    # seed=None: torch's global device generator, which the call advances
    torch.manual_seed(7)
    c = run(ids, am, do_sample=True)
    assert not torch.equal(torch.cuda.get_rng_state(), state)
    torch.manual_seed(7)
    assert torch.equal(run(ids, am, do_sample=True), c)
    # the numbers are torch.rand(max_new_tokens, rows) on a generator seeded with seed
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    assert torch.equal(run(ids, am, do_sample=True, sample_u=torch.rand(N_NEW, B, generator=g, device="cuda")), a)
    for bad in (torch.rand(N_NEW, B), torch.rand(N_NEW, B + 1).cuda(), torch.rand(N_NEW, B).double().cuda(), torch.rand(B, N_NEW).cuda().t()):
        with pytest.raises(ValueError, match="sample_u"):
            run(ids, am, do_sample=True, sample_u=bad)


@pytest.mark.parametrize("kind", ["fork", "llama"])
def test_eos_rows_are_padded(kind):
    run, _, _ = _generator(kind, torch.float32)
    ids, am, free, _ = _untied_prompt(run)
    free = free.cpu()
    eos = int(free[0, T + 2])                                    # top_k = 1 emits it in row 0 at step 2 at the latest
    out = run(ids, am, do_sample=True, top_k=1, sample_u=_u(3), eos_token_id=eos, pad_token_id=1).cpu()
    hit = 0
    for b in range(B):
        new, ref = out[b, T:], free[b, T:]
        pos = (ref == eos).nonzero()
        if len(pos) == 0:
            assert torch.equal(new, ref)                         # the other rows are unaffected
            continue
        p = int(pos[0])
        hit += 1
        assert torch.equal(new[:p + 1], ref[:p + 1]) and (new[p + 1:] == 1).all(), (b, new.tolist(), ref.tolist())
    assert hit >= 1 and int((free[0, T:] == eos).nonzero()[0]) <= 2 and (out[0, T + 3:] == 1).all()
    assert torch.equal(run(ids, am, do_sample=True, top_k=1, seed=1, eos_token_id=eos).cpu(), out)      # the default pad is the config's


@pytest.mark.parametrize("R", [2, 4])
def test_num_return_sequences_on_one_prefill(R):
    lm = _fork()[1].cuda()
    dec, d = lm.model.decoder, lm.config.hidden_size
    ids, am = _prompt(1, batch=B)
    run = lambda **kw: lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, do_sample=True, **kw)
    calls, real = [], dec.forward

    def spy(*a, **kw):
        o = real(*a, **kw)
        calls.append((tuple(kw["input_ids"].shape), o.past_key_values))
        return o
    u = _u(10 + R, B * R)
    dec.forward = spy
    try:
        out = run(num_return_sequences=R, sample_u=u, temperature=0.9)
    finally:
        del dec.forward
    # shape and row order: rows b*R .. b*R + R - 1 belong to prompt b; one prefill of B rows, steps of B*R rows
    assert out.shape == (B * R, T + N_NEW) and torch.equal(out[:, :T].cpu(), ids.repeat_interleave(R, dim=0))
    assert [c[0] for c in calls] == [(B, T)] + [(B * R, 1)] * (N_NEW - 1)
    cache = calls[0][1]
    assert all(kv.shape == (B, T, 2 * d) for kv in cache.kv) and cache.mask.shape == (B, T) and cache.col == T
    assert all(t.shape == (B * R, N_NEW - 1, 2 * d) for t in cache.beam.tail) and cache.beam.n_tail == N_NEW - 1
    ident = (torch.arange(B * R, device="cuda") % R).int()[:, None].expand(B * R, N_NEW - 1)
    assert torch.equal(cache.beam.book.src, ident), "somebody moved the parent table: the R rows are no longer independent"
    # distinct u: each row replays against the uncached forward over ITS OWN ids (the bound: module docstring)
    rows_am = am.repeat_interleave(R, dim=0)
    ref = _reference_steps(lambda i, m: _uncached_last_logits(lm, i, m), out.cpu(), rows_am, N_NEW)
    delta = TAU[torch.float32] * ref.abs().max().item()
    eps = eps_u(V) + math.expm1(2 * delta)
    everything = np.ones(V, dtype=bool)
    for s in range(N_NEW):
        x = scaled(ref[:, s], 0.9)
        for r in range(B * R):
            t, uu = int(out[r, T + s]), float(u[s, r])
            assert draw_ok(cdf(x[r], everything), everything, uu, t, eps), f"row {r} step {s}: token {t} for u = {uu} (eps {eps:.2e})"
    assert len({tuple(out[r, T:].tolist()) for r in range(R)}) > 1, "the R rows of prompt 0 are one text: distinct u showed nothing"
    # every draw of a prompt with the same u: its R rows are identical, and equal the R = 1 run on that u
    same = _u(20, B)
    tied = run(num_return_sequences=R, sample_u=same.repeat_interleave(R, dim=1).contiguous(), **KNOBS)
    single = run(sample_u=same, **KNOBS)
    assert torch.equal(tied, single.repeat_interleave(R, dim=0))
    assert torch.equal(run(num_return_sequences=1, sample_u=same, **KNOBS), single)
    # EOS bookkeeping per row, seeds, and the refusals that need the device
    eos = int(tied[0, T + 1])
    padded = run(num_return_sequences=R, sample_u=same.repeat_interleave(R, dim=1).contiguous(), eos_token_id=eos, pad_token_id=1, **KNOBS)
    first = int((tied[0, T:] == eos).nonzero()[0])
    assert torch.equal(padded[:R, :T + first + 1], tied[:R, :T + first + 1]) and bool((padded[:R, T + first + 1:] == 1).all())
    assert torch.equal(run(num_return_sequences=R, seed=3), run(num_return_sequences=R, seed=3))
    with pytest.raises(ValueError, match="sample_u"):
        run(num_return_sequences=R, sample_u=same)
    with pytest.raises(ValueError, match="inputs_embeds"):
        lm.generate(inputs_embeds=torch.zeros(B, T, 64, device="cuda"), attention_mask=am.cuda(), do_sample=True, num_return_sequences=R)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_attention_model_samples_with_neighbors(dtype):
    """The wrapper passes the sampling keywords through; R rows of a prompt read its neighbor tokens once (they stay at 8 rows)."""
    w, nb, _ = _wrapper(round_bf16=dtype == torch.bfloat16)
    ids, am = _prompt(1)
    w = w.to(dtype).cuda()
    nbd = {k: v.cuda() for k, v in nb.items()}
    run = lambda **kw: w.generate(ids.cuda(), am.cuda(), **nbd, max_new_tokens=N_NEW, do_sample=True, **kw)
    rows = ids.shape[0]
    u = _u(5, rows)
    out, steps = run(sample_u=u, return_step_logits=True, **KNOBS)
    assert out.shape == (rows, T + N_NEW)
    _replay(steps, out, u, KNOBS)
    R = 2
    tied = run(num_return_sequences=R, sample_u=u.repeat_interleave(R, dim=1).contiguous(), **KNOBS)
    assert tied.shape == (rows * R, T + N_NEW) and torch.equal(tied[:, :T + 1], out[:, :T + 1].repeat_interleave(R, dim=0))
    assert torch.equal(tied[0::R], tied[1::R]), "the same u on the same cache rows gave two texts"
    plain = w.lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, do_sample=True, sample_u=u, **KNOBS)
    assert not torch.equal(plain, out), "the neighbors do not reach the sampled steps"


def test_refusals_on_the_device():
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    from mmgl_amd.model.modelling_self_attention import SelfAttentionModel
    lm = _fork()[1].cuda()
    ids, am = _prompt(1, batch=B)
    ids, am = ids.cuda(), am.cuda()
    with pytest.raises(ValueError, match="do_sample"):
        lm.generate(ids, am, temperature=0.7)
    with pytest.raises(ValueError, match="num_beams"):
        lm.generate(ids, am, do_sample=True, num_beams=2)
    with pytest.raises(ValueError, match="num_return_sequences"):
        lm.generate(ids, am, num_return_sequences=2)
    with pytest.raises(ValueError, match="num_return_sequences"):
        lm.generate(ids, am, num_beams=2, num_return_sequences=2)
    with pytest.raises(ValueError, match="num_return_sequences"):
        SelfAttentionModel.generate(None, ids, am, do_sample=True, num_return_sequences=2)
    with pytest.raises(ValueError, match="num_return_sequences"):
        LlamaNeighborLM.generate(None, ids, am, do_sample=True, num_return_sequences=2)
    with pytest.raises(ValueError, match="beam search"):
        lm.generate(ids, am, do_sample=True, return_beam_trace=True)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        lm.generate(ids, am, do_sample=True, max_new_tokens=64)


def test_evaluate_loop_passes_the_sampling_knobs(tmp_path):
    from torch.utils.data import DataLoader, Subset
    from mmgl_amd.language_modelling.run_generation import Arguments, build_datasets, build_model, evaluate_loop
    from mmgl_amd.wikiweb2m.synthetic import synthetic_tokenizer
    torch.manual_seed(0)
    tokenizer = synthetic_tokenizer()
    base = dict(model_name_or_path="mpt-tiny", dataset="synthetic", context="all", neighbor_mode="embedding", peft_type="flamingo",
                max_input_length=32, max_output_length=12, max_text_neighbors=5, max_image_neighbors=2, n_text_tokens=2, n_visual_tokens=2,
                per_device_val_batch_size=4, dataloader_num_workers=0, val_steps_per_epoch=2, print_freq=100, log_dir=str(tmp_path), seed=0)
    args = Arguments(do_sample=True, temperature=0.7, top_k=5, top_p=0.9, **base)
    greedy = Arguments(**base)
    assert (greedy.do_sample, greedy.temperature, greedy.top_k, greedy.top_p) == (False, 1.0, 0, 1.0)       # the default stays greedy
    args.image_size = greedy.image_size = 32
    model = build_model(args, tokenizer, offline=True).float().cuda().eval()
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if n_.endswith(("gating1", "gating2")):
                p.fill_(0.5)
    _, val_ds, _ = build_datasets(args, tokenizer)
    loader = lambda: DataLoader(Subset(val_ds, list(range(8))), batch_size=4, shuffle=False, num_workers=0, drop_last=True)
    calls, real = [], model.generate

    def counting(**kw):
        out = real(**kw)
        calls.append(({k: kw.get(k) for k in ("do_sample", "temperature", "top_k", "top_p", "seed")}, tuple(kw["input_ids"].shape), tuple(out.shape)))
        return out
    model.generate = counting
    try:
        evaluate_loop(loader(), model, tokenizer, 0, args, prefix="test")
        n = len(calls)
        assert n >= 1 and sum(c[1][0] for c in calls) == 8, calls
        for knobs, shape_in, shape_out in calls:
            assert knobs == dict(do_sample=True, temperature=0.7, top_k=5, top_p=0.9, seed=0), knobs
            assert shape_out == (shape_in[0], args.max_input_length + 32)
        evaluate_loop(loader(), model, tokenizer, 0, greedy, prefix="test")
        assert len(calls) > n and all(c[0] == dict(do_sample=None, temperature=None, top_k=None, top_p=None, seed=None) for c in calls[n:])
    finally:
        del model.generate
