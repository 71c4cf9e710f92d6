"""-m gpu: generate(kv_cache_dtype="fp8") -- the FP8 key/value cache of the frozen layers -- on the tiny fork, prompts
and seed of tests/test_generate_gpu.py (B = 8, prompt width 12 with ragged right padding, 16 new tokens).

(a) Replay: a decode step on the FP8 cache equals a plain step on a cache that holds the dequantised columns (exact up to summation
    order; asserted at TAU).  (b) The prompt columns of the FP8 cache are the restatement (tests/kvq_ref.py) of a plain run's cache,
    bitwise.  (c) An independent reference, fp32: HF OPT on the CPU with its own cache, whose columns are quantised and dequantised by
    the restatement -- the prompt's after the prefill, each appended one after its step -- on the product's tokens.  Its distance
    `dist` from the unquantised HF reference on the same tokens says how much the FP8 cache moves the logits (asserted >= 1e-2, or the
    case shows nothing); the product lies within dist / 4 of it, so a product that ignores the keyword fails.  (d) Structure.

Measured on the CPU with the construction of (c), on the reference's own greedy tokens: seeds 0-3 give dist 2.2e-2 / 2.0e-2 / 1.9e-2 /
2.1e-2 and a share of low-margin (sample, step) pairs of 1.6 / 0.8 / 7.8 / 2.3 %; seed 2 is over the 5 % cap, so the seed is not free.
Relative noise of 1e-6 on the quantiser's inputs (rounding flips from fp32 GEMM differences, about ten times what fp32 should give)
moved the logits by at most 9e-4, well inside dist / 4."""
import pytest
import torch

import kvq_ref
from helpers import rel_err
from test_generate_gpu import B, N_NEW, SEED, T, TAU, _fork, _neighbors, _prompt, _wrapper

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn


def _spy_cache(dec, run):
    """Runs `run()` with dec.forward spied on; returns (what run returned, the DecodeCache of the prefill, the input shapes)."""
    calls, real = [], dec.forward

    def spy(*a, **kw):
        o = real(*a, **kw)
        calls.append((tuple(kw["input_ids"].shape), o.past_key_values))
        return o
    dec.forward = spy
    try:
        res = run()
    finally:
        del dec.forward
    return res, calls[0][1], [c[0] for c in calls]


def _grown(cache, lm, fp8):
    """A DecodeCache with one more column than `cache` (an FP8 cache after its last step: full) and the same state: an FP8 one with
    the same codes and exponents, or a plain one that holds the dequantised columns."""
    from mmgl_amd.model.modelling_cross_attention import DecodeCache
    cfg = lm.config
    Hh, d, col = cfg.num_attention_heads, cfg.hidden_size, cache.col
    dtype, dev = cache.kv_new.dtype, cache.mask.device
    new = DecodeCache(len(cache.kv), cache.mask.shape[0], cache.capacity + 1, d, dtype, dev, FP8 if fp8 else None, Hh if fp8 else None)
    for l in range(len(cache.kv)):
        if fp8:
            new.kv[l].view(torch.uint8)[:, :col] = cache.kv[l].view(torch.uint8)[:, :col]
            new.kv_scale[l][:, :col] = cache.kv_scale[l][:, :col]
        else:
            k, v = kvq_ref.dequantize_row(cache.kv[l].view(torch.uint8)[:, :col], cache.kv_scale[l][:, :col], Hh)
            assert torch.equal(k.to(dtype).float(), k) and torch.equal(v.to(dtype).float(), v)          # exact in the model's dtype
            new.kv[l][:, :col] = torch.cat([k, v], dim=-1).to(dtype).to(dev)
    new.mask[:, :col] = cache.mask[:, :col]
    new.col, new.next_pos, new.cross, new.cross_valid = col, cache.next_pos.clone(), cache.cross, cache.cross_valid
    return new


def _replay(lm, cache, tok, dtype, what):
    """One more step on the FP8 cache and on the plain cache of its dequantised columns: the same token at the same column."""
    dec = lm.model.decoder
    a, b = _grown(cache, lm, True), _grown(cache, lm, False)
    assert a.kv[0].dtype == FP8 and b.kv[0].dtype == dtype and b.kv_scale is None
    with torch.no_grad():
        la = lm._last_logits(dec(input_ids=tok, past_key_values=a).last_hidden_state[:, 0])
        lb = lm._last_logits(dec(input_ids=tok, past_key_values=b).last_hidden_state[:, 0])
    assert a.col == b.col == cache.col + 1
    err = rel_err(la, lb)
    print(f"{what}: FP8 step vs plain step on the dequantised columns, rel err {err:.3e} (tau {TAU[dtype]:.0e})")
    assert err <= TAU[dtype], err
    # layer 0 projects the same rows in both steps (the embedding and a LayerNorm in front of it): the FP8 step filed the restatement
    # of the column the plain step filed, bitwise.  Deeper layers see attention outputs that differ in summation order.
    d, Hh = b.kv[0].shape[-1] // 2, lm.config.num_attention_heads
    codes, e = kvq_ref.quantize_row(b.kv[0][:, cache.col, :d], b.kv[0][:, cache.col, d:], Hh)
    assert torch.equal(a.kv[0].view(torch.uint8)[:, cache.col].cpu(), codes) and torch.equal(a.kv_scale[0][:, cache.col].cpu(), e)
    return la


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_replay_a_step_equals_a_plain_step_on_the_dequantised_columns(dtype):
    _, lm = _fork()
    lm = lm.to(dtype).cuda()
    ids, am = _prompt(SEED)
    dec = lm.model.decoder
    (out, steps), cache, shapes = _spy_cache(dec, lambda: lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, return_step_logits=True,
                                                                       kv_cache_dtype="fp8"))
    assert shapes == [(B, T)] + [(B, 1)] * (N_NEW - 1) and out.shape == (B, T + N_NEW) and steps.shape == (B, N_NEW, 128)
    assert cache.col == cache.capacity == T + N_NEW - 1 and cache.kv[0].dtype == FP8
    assert torch.equal(out[:, T:], steps.float().argmax(-1))
    _replay(lm, cache, out[:, -1:], dtype, f"fork {dtype}")
    # and the step the loop itself made last: its logits are those of a plain step on the columns it read
    with torch.no_grad():
        plain = _grown(cache, lm, False)
        plain.col -= 1
        plain.next_pos = plain.next_pos - 1
        again = lm._last_logits(dec(input_ids=out[:, -2:-1], past_key_values=plain).last_hidden_state[:, 0])
    err = rel_err(steps[:, -1], again)
    print(f"fork {dtype}: the loop's last step vs a plain step on the dequantised columns, rel err {err:.3e}")
    assert err <= TAU[dtype], err


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_prefill_columns_are_the_restatement_of_a_plain_cache(dtype):
    _, lm = _fork()
    lm = lm.to(dtype).cuda()
    ids, am = _prompt(SEED)
    Hh, d = lm.config.num_attention_heads, lm.config.hidden_size
    with torch.no_grad():
        plain = lm(input_ids=ids.cuda(), attention_mask=am.cuda(), use_cache=True, cache_capacity=T + 1).past_key_values
        q8 = lm(input_ids=ids.cuda(), attention_mask=am.cuda(), use_cache=True, cache_capacity=T + 1, kv_cache_dtype=FP8).past_key_values
    assert plain.kv_scale is None and q8.col == plain.col == T and torch.equal(q8.mask, plain.mask)
    for l in range(len(plain.kv)):
        codes, e = kvq_ref.quantize_row(plain.kv[l][:, :T, :d], plain.kv[l][:, :T, d:], Hh)
        assert torch.equal(q8.kv[l].view(torch.uint8)[:, :T].cpu(), codes), l
        assert torch.equal(q8.kv_scale[l][:, :T].cpu(), e), l


def _qdq(x):
    """[..., D] of one head -> its dequantised FP8 restatement."""
    return kvq_ref.dequantize(*kvq_ref.quantize(x, 1), 1).to(x.dtype)


def _hf_cached_steps(hf, ids, am, out, n_new, quantised):
    """[B, n_new, V]: HF OPT with its own cache on the tokens `out`; quantised: every cached column goes through the restatement --
    the prompt's after the prefill, each appended one after the step that used it as projected."""
    width = ids.shape[1]
    with torch.no_grad():
        o = hf(input_ids=ids, attention_mask=am, use_cache=True)
        pkv = o.past_key_values
        if quantised:
            for layer in pkv.layers:
                layer.keys, layer.values = _qdq(layer.keys), _qdq(layer.values)
        logits = [o.logits[:, -1]]
        for s in range(n_new - 1):
            mask = torch.cat([am, torch.ones(am.shape[0], s + 1, dtype=am.dtype)], dim=1)
            o = hf(input_ids=out[:, width + s:width + s + 1], attention_mask=mask, past_key_values=pkv, use_cache=True)
            pkv = o.past_key_values
            if quantised:
                for layer in pkv.layers:
                    assert layer.keys.shape[2] == width + s + 1
                    layer.keys[:, :, -1], layer.values[:, :, -1] = _qdq(layer.keys[:, :, -1]), _qdq(layer.values[:, :, -1])
            logits.append(o.logits[:, -1])
    return torch.stack(logits, dim=1).float()


def test_fp32_against_hf_opt_with_a_quantised_cache():
    hf, lm = _fork()
    ids, am = _prompt(SEED)
    lm = lm.cuda()
    out, steps = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, return_step_logits=True, kv_cache_dtype="fp8")
    out, steps = out.cpu(), steps.float().cpu()
    ref = _hf_cached_steps(hf, ids, am, out, N_NEW, quantised=True)
    unq = _hf_cached_steps(hf, ids, am, out, N_NEW, quantised=False)
    dist = rel_err(ref, unq)
    print(f"HF OPT with a quantised cache vs HF OPT, the product's tokens: dist {dist:.3e}")
    assert dist >= 1e-2, f"the FP8 cache moves the reference's logits by {dist:.3e} only: the case shows nothing"
    assert torch.equal(ref[:, 0], unq[:, 0])                                       # the prefill's own attention is untouched
    tol = dist / 4
    scale = ref.abs().max().item()
    top2 = ref.topk(2, dim=-1).values
    low = (top2[..., 0] - top2[..., 1]) <= 2 * tol * scale
    share = low.float().mean().item()
    print(f"{share * 100:.1f} % of the {low.numel()} (sample, step) pairs are below the margin 2 tol max|logit| = {2 * tol * scale:.3e}")
    assert share <= 0.05, f"{share:.3f} of the steps are near-ties of the reference itself"
    err = rel_err(steps, ref)
    print(f"product vs the quantised reference: rel err {err:.3e} (tol dist / 4 = {tol:.3e}); vs the unquantised one: {rel_err(steps, unq):.3e}")
    assert err <= tol, f"step logits rel err {err:.3e} > {tol:.3e}"
    assert torch.equal(out[:, T:], steps.argmax(-1))
    wrong = (out[:, T:] != ref.argmax(-1)) & ~low
    assert not wrong.any(), f"{int(wrong.sum())} tokens differ from the reference argmax at a clear margin: {wrong.nonzero().tolist()[:8]}"


# ------------------------------------------------------------------------------------------ (d) structure
def test_cache_dtypes_shapes_and_bytes():
    w, nb, _ = _wrapper()
    ids, am = _prompt(SEED)
    w = w.bfloat16().cuda()
    dec, cfg = w.lm.model.decoder, w.lm.config
    dev = {k: v.cuda() for k, v in nb.items()}
    caches = {}
    for key in (None, "fp8"):
        _, caches[key], _ = _spy_cache(dec, lambda: w.generate(ids.cuda(), am.cuda(), **dev, max_new_tokens=N_NEW, kv_cache_dtype=key))
    plain, q8 = caches[None], caches["fp8"]
    d, Hh, cap, L = cfg.hidden_size, cfg.num_attention_heads, T + N_NEW - 1, cfg.num_hidden_layers
    assert plain.kv_scale is None and plain.kv_new is None and all(t.dtype == torch.bfloat16 and t.shape == (B, cap, 2 * d) for t in plain.kv)
    assert len(q8.kv) == len(q8.kv_scale) == L
    assert all(t.dtype == FP8 and t.shape == (B, cap, 2 * d) for t in q8.kv)
    assert all(t.dtype == torch.int8 and t.shape == (B, cap, 2 * Hh) for t in q8.kv_scale)
    assert q8.kv_new.dtype == torch.bfloat16 and q8.kv_new.shape == (B, 2 * d)
    assert len(q8.cross) == len(plain.cross) == len(dec.neighbor_layers) > 0
    for (k8, v8), (kp, vp) in zip(q8.cross, plain.cross):                          # the neighbor tokens stay in the model's dtype, untouched
        assert k8.dtype == v8.dtype == torch.bfloat16 and torch.equal(k8, kp) and torch.equal(v8, vp)
    nbytes = lambda c: sum(t.numel() * t.element_size() for t in c.kv + (c.kv_scale or []))
    assert nbytes(q8) / nbytes(plain) == (2 * d + 2 * Hh) / (4 * d)
    assert all((s.cpu().abs() <= 120).all() for s in q8.kv_scale)                  # every column was filed


def test_a_decode_step_makes_the_launches_of_the_plain_step(monkeypatch):
    from mmgl_amd import _lib
    _, lm = _fork()
    lm = lm.cuda()
    ids, am = _prompt(SEED)
    names, real = [], _lib.call

    def counting(name, *a):
        names.append(name)
        return real(name, *a)
    counts = {}
    for key in (None, "fp8"):
        with torch.no_grad():
            cache = lm(input_ids=ids.cuda(), attention_mask=am.cuda(), use_cache=True, cache_capacity=T + 2, kv_cache_dtype=key).past_key_values
            monkeypatch.setattr(_lib, "call", counting)
            del names[:]
            lm(input_ids=ids[:, :1].cuda(), past_key_values=cache)
            monkeypatch.setattr(_lib, "call", real)
        counts[key] = sorted(names)
    L = lm.config.num_hidden_layers
    print(f"C-ABI calls of a decode step: {len(counts[None])} plain, {len(counts['fp8'])} with the FP8 cache")
    assert len(counts["fp8"]) == len(counts[None])
    assert counts["fp8"].count("mmgl_attn_decode_q8_fwd") == counts[None].count("mmgl_attn_decode_fwd") == L
    assert "mmgl_attn_decode_fwd" not in counts["fp8"] and "mmgl_kv_quantize" not in counts["fp8"]
    swap = lambda n: "mmgl_attn_decode_fwd" if n == "mmgl_attn_decode_q8_fwd" else n
    assert sorted(map(swap, counts["fp8"])) == counts[None]


def test_none_is_the_call_without_the_keyword_bitwise():
    _, lm = _fork()
    lm = lm.cuda()
    ids, am = _prompt(SEED)
    a, sa = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, return_step_logits=True)
    b, sb = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, return_step_logits=True, kv_cache_dtype=None)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    c, sc = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, return_step_logits=True, kv_cache_dtype="fp8")
    assert torch.equal(sc[:, 0], sa[:, 0]) and not torch.equal(sc[:, 1:], sa[:, 1:])         # the prefill is untouched, the steps are not
    c2, sc2 = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, return_step_logits=True, kv_cache_dtype=torch.float8_e4m3fn)
    assert torch.equal(c, c2) and torch.equal(sc, sc2)                                        # two runs, and the two spellings


def test_sampling_processors_embeds_and_eos():
    _, lm = _fork()
    lm = lm.cuda()
    ids, am = _prompt(SEED)
    g = torch.Generator().manual_seed(3)
    u = torch.rand(N_NEW, B, generator=g).cuda()
    kw = dict(max_new_tokens=N_NEW, do_sample=True, sample_u=u, top_k=20, top_p=0.9, temperature=0.8, repetition_penalty=1.2,
              no_repeat_ngram_size=2, suppress_tokens=[5, 9], return_step_logits=True, kv_cache_dtype="fp8")
    out, steps = lm.generate(ids.cuda(), am.cuda(), **kw)
    out2, steps2 = lm.generate(ids.cuda(), am.cuda(), **kw)
    assert out.shape == (B, T + N_NEW) and torch.equal(out, out2) and torch.equal(steps, steps2) and torch.equal(out[:, :T].cpu(), ids)
    new = out[:, T:].cpu()
    assert ((new >= 0) & (new < 128)).all() and not ((new == 5) | (new == 9)).any()
    assert torch.isinf(steps[:, :, 5]).all() and (steps[:, :, 5] < 0).all()                   # the processed logits came back
    # an embeddings prompt
    emb = lm.model.decoder.embed_tokens(ids.cuda())
    new_e = lm.generate(inputs_embeds=emb, attention_mask=am.cuda(), max_new_tokens=N_NEW, kv_cache_dtype="fp8")
    greedy = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, kv_cache_dtype="fp8")
    assert new_e.shape == (B, N_NEW) and torch.equal(new_e, greedy[:, T:])
    # EOS rows are padded
    free = greedy.cpu()
    eos = int(free[0, T + 3])
    padded = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, eos_token_id=eos, pad_token_id=1, kv_cache_dtype="fp8").cpu()
    hit = 0
    for b in range(B):
        row, ref = padded[b, T:], free[b, T:]
        pos = (ref == eos).nonzero()
        if len(pos) == 0:
            assert torch.equal(row, ref)
            continue
        p = int(pos[0])
        hit += 1
        assert torch.equal(row[:p + 1], ref[:p + 1]) and (row[p + 1:] == 1).all(), (b, row.tolist(), ref.tolist())
    assert hit >= 1


def test_cross_attention_model_bf16_replay():
    w, nb, _ = _wrapper(round_bf16=True)
    ids, am = _prompt(SEED)
    w = w.bfloat16().cuda()
    dev = {k: v.cuda() for k, v in nb.items()}
    dec = w.lm.model.decoder
    (out, steps), cache, shapes = _spy_cache(dec, lambda: w.generate(ids.cuda(), am.cuda(), **dev, max_new_tokens=N_NEW, return_step_logits=True,
                                                                     kv_cache_dtype="fp8"))
    assert shapes == [(B, T)] + [(B, 1)] * (N_NEW - 1) and steps.dtype == torch.bfloat16 and len(cache.cross) > 0
    _replay(w.lm, cache, out[:, -1:], torch.bfloat16, "CrossAttentionModel bf16")
    with torch.no_grad():
        plain = _grown(cache, w.lm, False)
        plain.col -= 1
        plain.next_pos = plain.next_pos - 1
        again = w.lm._last_logits(dec(input_ids=out[:, -2:-1], past_key_values=plain).last_hidden_state[:, 0])
    err = rel_err(steps[:, -1], again)
    print(f"CrossAttentionModel bf16: the loop's last step vs a plain step on the dequantised columns, rel err {err:.3e}")
    assert err <= TAU[torch.bfloat16], err


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
    model = build_model(args, tokenizer, offline=True).float().cuda().eval()
    _, val_ds, _ = build_datasets(args, tokenizer)
    loader = lambda: DataLoader(Subset(val_ds, list(range(4))), batch_size=4, shuffle=False, num_workers=0, drop_last=True)
    seen, real = [], model.generate

    def spy(**kw):
        seen.append(kw.get("kv_cache_dtype", "absent"))
        return real(**kw)
    model.generate = spy
    try:
        evaluate_loop(loader(), model, tokenizer, 0, args, prefix="test")
        n = len(seen)
        assert n >= 1 and set(seen) == {"absent"}                                   # the default: today's call
        args.kv_cache_dtype = "fp8"
        evaluate_loop(loader(), model, tokenizer, 0, args, prefix="test")
        assert len(seen) == 2 * n and set(seen[n:]) == {"fp8"}
    finally:
        del model.generate
