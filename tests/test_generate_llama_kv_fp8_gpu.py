"""-m gpu: LlamaNeighborLM.generate(kv_cache_dtype="fp8") -- the FP8 cache of the Hkv key/value heads -- on the tiny
models, prompts, neighbors and seed of tests/test_generate_llama_gpu.py (B = 8, prompt width 12, 16 new tokens).

(a) Replay: a decode step on the FP8 cache equals a plain step on a cache that holds the dequantised columns (exact up to summation
    order; asserted at TAU), and layer 0 files the restatement of the plain step's column, bitwise.  (b) The prompt columns of the FP8
    cache are the restatement (tests/kvq_ref.py, Hkv heads) of a plain run's cache, bitwise, for every layer.  (c) An independent
    reference, fp32, gates 0: HF LlamaForCausalLM on the CPU with its own cache, whose rows go through the restatement per (kv head, D)
    -- the prompt's after the prefill, each appended column after the step that used it -- on the product's tokens.  `dist` is its
    distance from unquantised HF on the same tokens (asserted >= 8e-3, or the case shows nothing); the tolerance is dist / 8, never
    below the fp32 tau of 1e-3, and a product that ignores the keyword sits 8 tolerances away.  The share of (sample, step) pairs whose
    top-1 minus top-2 margin is within 2 tol max|logit| is computed from the reference alone and asserted <= 10 % before any
    comparison: a condition, not a measurement.  (d) Structure.

Measured on the CPU with the construction of (c) on the reference's OWN greedy tokens, seed 0 (tol = dist / 8):
  equal-length prompts  Hkv 4 / 2 / 1: dist 1.05e-2 / 1.59e-2 / 1.43e-2, share below the margin 3.1 / 5.5 / 5.5 %
  ragged prompts        Hkv 4 / 2:     dist 2.12e-2 / 1.50e-2,           share below the margin 3.9 / 7.0 %
Ragged Hkv = 1 gives 8.6 % and is left out; other seeds reach 7 % on these cases, so the seed is not free.  The cap is 10 %, not the
OPT fork's 5 %: a random untied-head Llama has flatter logits (tests/test_generate_llama_gpu.py), and this margin is 2-3 times wider
than that file's.  Relative noise of 1e-6 on the quantiser's inputs moved the logits by at most 4e-4, inside every dist / 8.
Measured on the product's tokens on one MI355X (what test_fp32_against_hf_llama_with_a_quantised_cache prints): the same dist, shares
3.1 / 5.5 / 5.5 % (equal-length, Hkv 4 / 2 / 1) and 3.9 / 7.0 % (ragged, Hkv 4 / 2); the product lies 2.5e-6 / 3.6e-7 / 3.9e-7 / 3.3e-7 /
3.7e-7 from the quantised reference and dist from the unquantised one.  Replay: 1.6e-7 - 2.6e-7 in fp32, 0 in bf16."""
import copy

import pytest
import torch

import kvq_ref
from helpers import rel_err
from test_generate_llama_gpu import B, MODELS, N_NEW, SEED, T, TAU, _generate, _lm, _neighbors, _prompt

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn


def _spy_cache(lm, run):
    """Runs `run()` with lm._hidden spied on; returns (what run returned, the DecodeCache of the prefill)."""
    caches, real = [], lm._hidden

    def spy(*a, **kw):
        o = real(*a, **kw)
        caches.append(o[1])
        return o
    lm._hidden = spy
    try:
        res = run()
    finally:
        del lm._hidden
    assert len(caches) == 1
    return res, caches[0]


def _grown(cache, lm, fp8):
    """A DecodeCache with one more column than `cache` (an FP8 cache after its last step: full) and the same state: an FP8 one with
    the same codes and exponents, or a plain one that holds the dequantised columns."""
    from mmgl_amd.model.modelling_cross_attention import DecodeCache
    fr = lm._frozen[0]
    Hkv, kd, col = fr.Hkv, fr.Hkv * fr.D, cache.col
    dtype, dev = cache.kv_new.dtype, cache.mask.device
    new = DecodeCache(len(cache.kv), cache.mask.shape[0], cache.capacity + 1, kd, dtype, dev, FP8 if fp8 else None, Hkv if fp8 else None)
    for l in range(len(cache.kv)):
        if fp8:
            new.kv[l].view(torch.uint8)[:, :col] = cache.kv[l].view(torch.uint8)[:, :col]
            new.kv_scale[l][:, :col] = cache.kv_scale[l][:, :col]
        else:
            k, v = kvq_ref.dequantize_row(cache.kv[l].view(torch.uint8)[:, :col], cache.kv_scale[l][:, :col], Hkv)
            assert torch.equal(k.to(dtype).float(), k) and torch.equal(v.to(dtype).float(), v)          # exact in the model's dtype
            new.kv[l][:, :col] = torch.cat([k, v], dim=-1).to(dtype).to(dev)
    new.mask[:, :col] = cache.mask[:, :col]
    new.col, new.cross, new.cross_valid, new.cross_gu = col, cache.cross, cache.cross_valid, cache.cross_gu
    new.cos_sin = lm._cos_sin(new.capacity, dev).clone()
    assert torch.equal(new.cos_sin[:cache.capacity], cache.cos_sin)
    return new


def _replay(lm, cache, tok, dtype, what):
    """One more step on the FP8 cache and on the plain cache of its dequantised columns: the same token at the same column."""
    a, b = _grown(cache, lm, True), _grown(cache, lm, False)
    assert a.kv[0].dtype == FP8 and b.kv[0].dtype == dtype and b.kv_scale is None
    la, lb = lm._last_logits(lm._decode_step(tok, a)), lm._last_logits(lm._decode_step(tok, b))
    assert a.col == b.col == cache.col + 1
    err = rel_err(la, lb)
    print(f"{what}: FP8 step vs plain step on the dequantised columns, rel err {err:.3e} (tau {TAU[dtype]:.0e})")
    assert err <= TAU[dtype], err
    # layer 0 projects and rotates the same rows in both steps (the embedding and an RMSNorm in front): the FP8 step filed the
    # restatement of the column the plain step filed, bitwise.  Deeper layers see attention outputs that differ in summation order.
    fr = lm._frozen[0]
    kd = fr.Hkv * fr.D
    codes, e = kvq_ref.quantize_row(b.kv[0][:, cache.col, :kd], b.kv[0][:, cache.col, kd:], fr.Hkv)
    assert torch.equal(a.kv[0].view(torch.uint8)[:, cache.col].cpu(), codes) and torch.equal(a.kv_scale[0][:, cache.col].cpu(), e)


@pytest.mark.parametrize("kind,n_kv,dtype", [("tiny", 2, torch.float32), ("tiny", 1, torch.float32), ("A", None, torch.bfloat16),
                                             ("B", None, torch.bfloat16)], ids=["fp32-Hkv2", "fp32-Hkv1", "bf16-A", "bf16-B"])
def test_replay_a_step_equals_a_plain_step_on_the_dequantised_columns(kind, n_kv, dtype):
    lm = _lm(kind, n_kv).to(dtype).cuda()
    ne, valid = _neighbors(SEED, MODELS[kind]["hidden"])
    ne = ne.to(dtype)
    ids, am = _prompt(SEED)
    (out, steps), cache = _spy_cache(lm, lambda: _generate(lm, ids, am, ne, valid, return_step_logits=True, kv_cache_dtype="fp8"))
    assert out.shape == (B, T + N_NEW) and steps.shape == (B, N_NEW, 128) and steps.dtype == dtype
    assert cache.col == cache.capacity == T + N_NEW - 1 and cache.kv[0].dtype == FP8 and len(cache.cross) > 0
    assert torch.equal(out[:, T:], steps.float().argmax(-1))
    _replay(lm, cache, out[:, -1:], dtype, f"model {kind} {dtype}")
    # and the step the loop itself made last: its logits are those of a plain step on the columns it read
    plain = _grown(cache, lm, False)
    plain.col -= 1
    again = lm._last_logits(lm._decode_step(out[:, -2:-1], plain))
    err = rel_err(steps[:, -1], again)
    print(f"model {kind} {dtype}: the loop's last step vs a plain step on the dequantised columns, rel err {err:.3e}")
    assert err <= TAU[dtype], err


def _prefill(lm, ids, am, ne, valid, **kw):
    with torch.no_grad():
        return lm(input_ids=ids.cuda(), attention_mask=am.cuda(), neighbor_embeds=ne.cuda(), neighbor_attention_mask=valid.cuda(), use_cache=True,
                  return_logits=True, **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_prefill_columns_are_the_restatement_of_a_plain_cache(dtype):
    lm = _lm("tiny", 2).to(dtype).cuda()
    ne, valid = _neighbors(SEED, 64)
    ne = ne.to(dtype)
    ids, am = _prompt(SEED)
    fr = lm._frozen[0]
    Hkv, kd = fr.Hkv, fr.Hkv * fr.D
    po = _prefill(lm, ids, am, ne, valid, cache_capacity=T + 1)
    qo = _prefill(lm, ids, am, ne, valid, cache_capacity=T + 1, kv_cache_dtype=FP8)
    plain, q8 = po.past_key_values, qo.past_key_values
    assert torch.equal(po.logits, qo.logits)                                        # the prefill's own attention is untouched
    assert plain.kv_scale is None and q8.col == plain.col == T and torch.equal(q8.mask, plain.mask) and len(plain.kv) == 4
    for l in range(len(plain.kv)):
        codes, e = kvq_ref.quantize_row(plain.kv[l][:, :T, :kd], plain.kv[l][:, :T, kd:], Hkv)
        assert torch.equal(q8.kv[l].view(torch.uint8)[:, :T].cpu(), codes), l
        assert torch.equal(q8.kv_scale[l][:, :T].cpu(), e), l


# ------------------------------------------------------------------------------------------ (c) the independent reference
def _qdq(x):
    """[..., D] of one kv head -> its dequantised FP8 restatement."""
    return kvq_ref.dequantize(*kvq_ref.quantize(x, 1), 1).to(x.dtype)


def hf_of(lm):
    hf = copy.deepcopy(lm.llama).float().cpu().eval()
    hf.model.rotary_emb.inv_freq.copy_(lm._inv_freq)
    return hf


def hf_cached_steps(hf, ids, am, out, n_new, quantised):
    """[B, n_new, V]: HF Llama with its own cache ([B, Hkv, S, D] per layer) on the tokens `out`; quantised: every cached row goes
    through the restatement per (kv head, D) -- the prompt's after the prefill, each appended one after the step that used it."""
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


def reference_condition(ref, unq, what):
    """(tol, the mask of pairs below the margin) from the two references alone; asserts dist >= 8e-3 and a share <= 10 %."""
    dist = rel_err(ref, unq)
    print(f"{what}: HF Llama with a quantised cache vs HF Llama, the same tokens: dist {dist:.3e}")
    assert dist >= 8e-3, f"the FP8 cache moves the reference's logits by {dist:.3e} only: the case shows nothing"
    tol = dist / 8
    assert tol >= TAU[torch.float32]
    scale = ref.abs().max().item()
    top2 = ref.topk(2, dim=-1).values
    low = (top2[..., 0] - top2[..., 1]) <= 2 * tol * scale
    share = low.float().mean().item()
    print(f"{what}: {share * 100:.1f} % of the {low.numel()} (sample, step) pairs are below the margin 2 tol max|logit| = {2 * tol * scale:.3e}")
    assert share <= 0.10, f"{share:.3f} of the steps are near-ties of the reference itself"
    return tol, low


@pytest.mark.parametrize("ragged,n_kv", [(False, 4), (False, 2), (False, 1), (True, 4), (True, 2)],
                         ids=["equal-Hkv4", "equal-Hkv2", "equal-Hkv1", "ragged-Hkv4", "ragged-Hkv2"])
def test_fp32_against_hf_llama_with_a_quantised_cache(ragged, n_kv):
    lm = _lm("tiny", n_kv, gates=False)
    hf = hf_of(lm)
    ids, am = _prompt(SEED, ragged=ragged)
    ne, valid = _neighbors(SEED, 64)
    out, steps = _generate(lm.cuda(), ids, am, ne, valid, return_step_logits=True, kv_cache_dtype="fp8")
    out, steps = out.cpu(), steps.float().cpu()
    what = f"{'ragged' if ragged else 'equal-length'} Hkv={n_kv}"
    ref = hf_cached_steps(hf, ids, am, out, N_NEW, quantised=True)
    unq = hf_cached_steps(hf, ids, am, out, N_NEW, quantised=False)
    assert torch.equal(ref[:, 0], unq[:, 0])                                       # the prefill's own attention is untouched
    tol, low = reference_condition(ref, unq, what)
    err = rel_err(steps, ref)
    print(f"{what}: product vs the quantised reference: rel err {err:.3e} (tol dist / 8 = {tol:.3e}); vs the unquantised one: {rel_err(steps, unq):.3e}")
    assert err <= tol, f"step logits rel err {err:.3e} > {tol:.3e}"
    assert torch.equal(out[:, T:], steps.argmax(-1))
    wrong = (out[:, T:] != ref.argmax(-1)) & ~low
    assert not wrong.any(), f"{int(wrong.sum())} tokens differ from the reference argmax at a clear margin: {wrong.nonzero().tolist()[:8]}"


# ------------------------------------------------------------------------------------------ (d) structure
def test_cache_dtypes_shapes_and_bytes():
    lm = _lm("A").bfloat16().cuda()
    ne, valid = _neighbors(SEED, MODELS["A"]["hidden"])
    ne = ne.bfloat16()
    ids, am = _prompt(SEED)
    caches = {}
    for key in (None, "fp8"):
        _, caches[key] = _spy_cache(lm, lambda: _generate(lm, ids, am, ne, valid, kv_cache_dtype=key))
    plain, q8 = caches[None], caches["fp8"]
    Hkv, D, cap, L = 2, 64, T + N_NEW - 1, 2
    assert plain.kv_scale is None and plain.kv_new is None and all(t.dtype == torch.bfloat16 and t.shape == (B, cap, 2 * Hkv * D) for t in plain.kv)
    assert len(q8.kv) == len(q8.kv_scale) == L
    assert all(t.dtype == FP8 and t.shape == (B, cap, 2 * Hkv * D) for t in q8.kv)
    assert all(t.dtype == torch.int8 and t.shape == (B, cap, 2 * Hkv) for t in q8.kv_scale)
    assert q8.kv_new.dtype == torch.bfloat16 and q8.kv_new.shape == (B, 2 * Hkv * D)
    assert len(q8.cross) == len(plain.cross) == len(lm.neighbor_layers) == 2
    for (k8, v8), (kp, vp) in zip(q8.cross, plain.cross):                          # the neighbor tokens stay in the model's dtype, untouched
        assert k8.dtype == v8.dtype == torch.bfloat16 and torch.equal(k8, kp) and torch.equal(v8, vp)
    nbytes = lambda c: sum(t.numel() * t.element_size() for t in c.kv + (c.kv_scale or []))
    assert nbytes(q8) / nbytes(plain) == (D + 1) / (2 * D)
    assert all((s.cpu().abs() <= 120).all() for s in q8.kv_scale)                  # every column was filed


@pytest.mark.parametrize("n_kv", [2, 4])
def test_a_decode_step_makes_the_launches_of_the_plain_step(monkeypatch, n_kv):
    from mmgl_amd import _lib
    lm = _lm("tiny", n_kv).cuda()
    ne, valid = _neighbors(SEED, 64)
    ids, am = _prompt(SEED)
    names, real = [], _lib.call

    def counting(name, *a):
        names.append(name)
        return real(name, *a)
    calls = {}
    for key in (None, "fp8"):
        cache = _prefill(lm, ids, am, ne, valid, cache_capacity=T + 2, kv_cache_dtype=key).past_key_values
        with torch.no_grad():
            monkeypatch.setattr(_lib, "call", counting)
            del names[:]
            lm(input_ids=ids[:, :1].cuda(), past_key_values=cache)
            monkeypatch.setattr(_lib, "call", real)
        calls[key] = list(names)
    # Hkv = H runs the multi-head pair of entry points, as ops.attn_decode does
    old, new = ("mmgl_attn_decode_gqa_fwd", "mmgl_attn_decode_gqa_q8_fwd") if n_kv < 4 else ("mmgl_attn_decode_fwd", "mmgl_attn_decode_q8_fwd")
    print(f"C-ABI calls of a decode step: {len(calls[None])} plain, {len(calls['fp8'])} with the FP8 cache")
    # (the two gated layers attend over their neighbor tokens through mmgl_attn_decode_fwd in both runs)
    assert calls["fp8"].count(new) == 4 and new not in calls[None] and calls[None].count(old) - calls["fp8"].count(old) == 4
    assert "mmgl_attn_decode_gqa_fwd" not in calls["fp8"] and "mmgl_kv_quantize" not in calls["fp8"]
    assert [old if n == new else n for n in calls["fp8"]] == calls[None]            # name for name, in order


def test_none_is_the_call_without_the_keyword_bitwise():
    lm = _lm("tiny", 2).cuda()
    ne, valid = _neighbors(SEED, 64)
    ids, am = _prompt(SEED)
    a, sa = _generate(lm, ids, am, ne, valid, return_step_logits=True)
    b, sb = _generate(lm, ids, am, ne, valid, return_step_logits=True, kv_cache_dtype=None)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    c, sc = _generate(lm, ids, am, ne, valid, return_step_logits=True, kv_cache_dtype="fp8")
    assert torch.equal(sc[:, 0], sa[:, 0]) and not torch.equal(sc[:, 1:], sa[:, 1:])         # the prefill is untouched, the steps are not
    c2, sc2 = _generate(lm, ids, am, ne, valid, return_step_logits=True, kv_cache_dtype=torch.float8_e4m3fn)
    assert torch.equal(c, c2) and torch.equal(sc, sc2)                                        # two runs, and the two spellings
    with pytest.raises(ValueError, match=r"FP8 key/value cache\) with prompt_lookup_num_tokens = 3"):
        _generate(lm, ids, am, ne, valid, kv_cache_dtype="fp8", prompt_lookup_num_tokens=3)


def test_sampling_processors_and_eos():
    lm = _lm("tiny", 2).cuda()
    ne, valid = _neighbors(SEED, 64)
    ids, am = _prompt(SEED)
    g = torch.Generator().manual_seed(3)
    u = torch.rand(N_NEW, B, generator=g).cuda()
    kw = dict(do_sample=True, sample_u=u, top_k=20, top_p=0.9, temperature=0.8, repetition_penalty=1.2, no_repeat_ngram_size=2,
              suppress_tokens=[5, 9], return_step_logits=True, kv_cache_dtype="fp8")
    out, steps = _generate(lm, ids, am, ne, valid, **kw)
    out2, steps2 = _generate(lm, ids, am, ne, valid, **kw)
    assert out.shape == (B, T + N_NEW) and torch.equal(out, out2) and torch.equal(steps, steps2) and torch.equal(out[:, :T].cpu(), ids)
    new = out[:, T:].cpu()
    assert ((new >= 0) & (new < 128)).all() and not ((new == 5) | (new == 9)).any()
    assert torch.isinf(steps[:, :, 5]).all() and (steps[:, :, 5] < 0).all()                   # the processed logits came back
    # EOS rows are padded
    free = _generate(lm, ids, am, ne, valid, kv_cache_dtype="fp8").cpu()
    eos = int(free[0, T + 3])
    padded = _generate(lm, ids, am, ne, valid, eos_token_id=eos, pad_token_id=1, kv_cache_dtype="fp8").cpu()
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
