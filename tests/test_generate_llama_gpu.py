"""-m gpu: greedy generation of the Llama-family neighbor LM with a grouped-query key/value cache (LlamaNeighborLM.generate).

Comparison rule (that of tests/test_generate_gpu.py, restated here because the cap on near-ties differs): at step s the reference runs
UNCACHED on the tokens the product has produced so far, so one near-tie cannot cascade.  The step logits must lie within tau of the
reference (max-norm relative error: 1e-3 fp32, 2e-2 bf16) and the product's token must equal the reference's argmax wherever the
reference's top-1 minus top-2 margin exceeds 2 tau max|logit|.  The share of (sample, step) pairs below that margin is computed from the
reference alone and asserted BEFORE any comparison: <= 5 % fp32, <= 40 % bf16 (a random Llama with an untied head has flatter logits
than the tied-head OPT fork, whose bf16 cap is 25 %).  A cap is a condition, not a measurement.

Layout: B = 8, prompt width 12 with ragged right padding, 16 new tokens, S = 10 neighbor tokens, sample 5 without a valid neighbor.
Construction: model under torch.manual_seed(seed), prompts _prompt(seed), neighbors from Generator(seed + 100): randn(B, S, hidden), then
rand(B, S) > 0.3; gates opened as tests/test_llama_gqa_gpu.py does.

Shares measured on the CPU with the reference's OWN greedy tokens, for the seeds used below (SEED = 0):
  fp32 tiny (hidden 64, H = 4, 4 layers, wise 2), gates 0, equal prompts, HF Llama:   Hkv 4 / 2 / 1: 2.3 / 3.1 / 1.6 %
  fp32 tiny, gates open, ragged prompts, oracle:                                      Hkv 4 / 2 / 1: 1.6 / 0.8 / 3.1 %
  bf16 A (hidden 256, H = 4, Hkv = 2, D = 64, inter 512, 2 layers, wise 1):           31.2 %
  bf16 B (hidden 512, H = 4, Hkv = 1, D = 128, inter 1024, 2 layers, wise 1):         26.6 %
all at or below 0.8 of their caps (4 % / 32 %).  Seeds 1 and 2 give 0-3.9 % fp32 and 30-43 % bf16: model A is over its cap there, so the
seed is not free to change.  On the product's tokens (what the tests assert) the same seed measured 0.8-3.1 % fp32, 31.2 % (A), 28.1 % (B)."""
import copy

import pytest
import torch

from helpers import mpt_args, rel_err, tiny_clip_vision_config, tiny_roberta_config

pytestmark = pytest.mark.gpu

B, T, N_NEW, S = 8, 12, 16, 10
TAU = {torch.float32: 1e-3, torch.bfloat16: 2e-2}
LOW_MARGIN_SHARE = {torch.float32: 0.05, torch.bfloat16: 0.40}
BF16_LOGITS_TOL = 2.5e-2          # tests/test_generate_gpu.py: the project's bound on bf16 logits
SEED = 0
MODELS = {"tiny": dict(hidden=64, H=4, inter=128, layers=4, wise=2), "A": dict(hidden=256, H=4, Hkv=2, inter=512, layers=2, wise=1),
          "B": dict(hidden=512, H=4, Hkv=1, inter=1024, layers=2, wise=1)}


def _prompt(seed, width=T, ragged=True, batch=B, vocab=128):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab, (batch, width), generator=g)
    am = torch.ones_like(ids)
    if ragged:
        for b in range(1, batch):                       # sample 0 fills the width; every sample keeps its first token
            am[b, int(torch.randint(1, width + 1, (1,), generator=g)):] = 0
    return torch.where(am.bool(), ids, torch.ones_like(ids)), am


def _neighbors(seed, hidden, batch=B, empty=5):
    g = torch.Generator().manual_seed(seed + 100)
    ne = torch.randn(batch, S, hidden, generator=g)
    valid = torch.rand(batch, S, generator=g) > 0.3
    if empty is not None:
        valid[empty] = False                            # a sample without any valid neighbor
    return ne, valid


def _open_gates(lm, hidden):
    with torch.no_grad():
        for i, layer in enumerate(lm.neighbor_layers):
            layer.gating1.fill_(0.5 + 0.1 * i)
            layer.gating2.fill_(-0.3 - 0.1 * i)
            layer.input_layernorm.add_(0.1 * torch.randn(hidden).to(layer.input_layernorm.device))


def _config(kind, n_kv=None, max_pos=256, vocab=128):
    from transformers import LlamaConfig
    m = MODELS[kind]
    return LlamaConfig(vocab_size=vocab, hidden_size=m["hidden"], intermediate_size=m["inter"], num_hidden_layers=m["layers"],
                       num_attention_heads=m["H"], num_key_value_heads=n_kv or m["Hkv"], max_position_embeddings=max_pos, pad_token_id=1,
                       bos_token_id=2, eos_token_id=2, attention_dropout=0.0)


def _lm(kind, n_kv=None, seed=SEED, gates=True, max_pos=256):
    """The LM on the CPU in fp32, in eval mode."""
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    torch.manual_seed(seed)
    lm = LlamaNeighborLM(mpt_args(model_name_or_path="llama-tiny", neighbor_layer_wise=MODELS[kind]["wise"]), _config(kind, n_kv, max_pos))
    if gates:
        _open_gates(lm, MODELS[kind]["hidden"])
    return lm.eval()


def _hf_last_logits(lm):
    hf = copy.deepcopy(lm.llama).float().eval()
    hf.model.rotary_emb.inv_freq.copy_(lm._inv_freq)        # a bf16 cast rounds HF's frequency buffer too (see LlamaNeighborLM.__init__)

    def last_logits(ids, mask):
        with torch.no_grad():
            return hf(input_ids=ids, attention_mask=mask).logits[:, -1]
    return last_logits


def _oracle_last_logits(lm, kind, ne, valid):
    """The fp32 CPU oracle of lm's present weights (for a bf16 model: the rounded ones)."""
    from oracle import llama_ref
    hf = copy.deepcopy(lm.llama).float().eval()
    hf.model.rotary_emb.inv_freq.copy_(lm._inv_freq)
    p = {k: v.detach().clone().float() for k, v in lm.state_dict().items() if k.startswith("neighbor_layers.")}
    ne = ne.float()

    def last_logits(ids, mask):
        with torch.no_grad():
            return llama_ref.llama_neighbor_lm_forward(hf, p, MODELS[kind]["wise"], ids, mask, ids, ne, valid)[0][:, -1]
    return last_logits


def _reference_steps(ref_last_logits, ids, am, n_new):
    """[B, n_new, V] fp32: the uncached reference on the product's own tokens, one run per step."""
    width = am.shape[1]
    out = []
    for s in range(n_new):
        mask = torch.cat([am, torch.ones(am.shape[0], s, dtype=am.dtype)], dim=1)
        out.append(ref_last_logits(ids[:, :width + s], mask).float())
    return torch.stack(out, dim=1)


def low_margin(ref, tau):
    top2 = ref.topk(2, dim=-1).values
    return (top2[..., 0] - top2[..., 1]) <= 2 * tau * ref.abs().max().item()


def _compare(step_logits, ids, ref, dtype, what):
    """The comparison rule of the module docstring.  Returns the mask of (sample, step) pairs below the margin."""
    tau = TAU[dtype]
    n_new = ref.shape[1]
    low = low_margin(ref, tau)
    share = low.float().mean().item()
    print(f"{what}: {share * 100:.1f} % of the {low.numel()} (sample, step) pairs are below the margin 2 tau max|logit|")
    assert share <= LOW_MARGIN_SHARE[dtype], f"{what}: {share:.3f} of the steps are near-ties of the reference itself"
    err = rel_err(step_logits.float().cpu(), ref)
    print(f"{what}: step logits rel err {err:.3e} (tau {tau:.1e})")
    assert err <= tau, f"{what}: step logits rel err {err:.3e} > {tau:.1e}"
    tokens = ids[:, -n_new:].cpu()
    assert torch.equal(tokens, step_logits.float().argmax(-1).cpu()), f"{what}: the returned ids are not the argmax of the returned step logits"
    wrong = (tokens != ref.argmax(-1)) & ~low
    assert not wrong.any(), f"{what}: {int(wrong.sum())} tokens differ from the reference argmax at a clear margin: {wrong.nonzero().tolist()[:8]}"
    return low


def _generate(lm, ids, am, ne, valid, n_new=N_NEW, **kw):
    return lm.generate(ids.cuda(), am.cuda(), neighbor_embeds=None if ne is None else ne.cuda(),
                       neighbor_attention_mask=None if valid is None else valid.cuda(), max_new_tokens=n_new, **kw)


@pytest.mark.parametrize("n_kv", [4, 2, 1])
def test_fp32_gates_zero_equal_length_prompts_vs_hf_llama(n_kv):
    lm = _lm("tiny", n_kv, gates=False)
    ref_fn = _hf_last_logits(lm)
    ids, am = _prompt(SEED, ragged=False)
    ne, valid = _neighbors(SEED, 64)
    out, steps = _generate(lm.cuda(), ids, am, ne, valid, return_step_logits=True)
    assert out.shape == (B, T + N_NEW) and steps.shape == (B, N_NEW, 128) and torch.equal(out[:, :T].cpu(), ids)
    ref = _reference_steps(ref_fn, out.cpu(), am, N_NEW)
    _compare(steps, out, ref, torch.float32, f"Hkv={n_kv} fp32 gates 0 vs HF Llama (uncached, product tokens)")


@pytest.mark.parametrize("n_kv", [4, 2, 1])
def test_fp32_gates_open_ragged_prompts_vs_oracle_loop(n_kv):
    lm = _lm("tiny", n_kv)
    ne, valid = _neighbors(SEED, 64)
    assert not valid[5].any()
    ref_fn = _oracle_last_logits(lm, "tiny", ne, valid)
    ids, am = _prompt(SEED)
    out, steps = _generate(lm.cuda(), ids, am, ne, valid, return_step_logits=True)
    ref = _reference_steps(ref_fn, out.cpu(), am, N_NEW)
    _compare(steps, out, ref, torch.float32, f"Hkv={n_kv} fp32 gates open vs oracle loop")


@pytest.mark.parametrize("kind", ["A", "B"])
def test_bf16_vs_fp32_oracle_of_the_rounded_weights(kind):
    lm = _lm(kind).bfloat16()
    ne, valid = _neighbors(SEED, MODELS[kind]["hidden"])
    ne = ne.bfloat16()
    ref_fn = _oracle_last_logits(lm, kind, ne, valid)
    ids, am = _prompt(SEED)
    out, steps = _generate(lm.cuda(), ids, am, ne, valid, return_step_logits=True)
    assert steps.dtype == torch.bfloat16
    ref = _reference_steps(ref_fn, out.cpu(), am, N_NEW)
    _compare(steps, out, ref, torch.bfloat16, f"model {kind} bf16 vs fp32 oracle loop")


def _uncached_last_logits(lm, ne, valid):
    def last_logits(ids, mask):
        with torch.no_grad():
            return lm(input_ids=ids.cuda(), attention_mask=mask.cuda(), neighbor_embeds=ne.cuda(), neighbor_attention_mask=valid.cuda(),
                      return_logits=True).logits[:, -1].float().cpu()
    return last_logits


@pytest.mark.parametrize("width", [T, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cached_equals_uncached_inside_the_product(dtype, width):
    tol = 1e-3 if dtype == torch.float32 else BF16_LOGITS_TOL
    lm = _lm("tiny", 2).to(dtype).cuda()
    ne, valid = _neighbors(SEED, 64)
    ne = ne.to(dtype)
    ids, am = _prompt(SEED + 1, width=width)
    out, steps = _generate(lm, ids, am, ne, valid, return_step_logits=True)
    ref = _reference_steps(_uncached_last_logits(lm, ne, valid), out.cpu(), am, N_NEW)
    for s in range(N_NEW):
        err = rel_err(steps[:, s].float().cpu(), ref[:, s])
        assert err <= tol, f"{dtype} width={width} step {s}: rel err {err:.3e} > {tol:.1e}"
    print(f"cached vs uncached {dtype} width={width}: rel err {rel_err(steps.float().cpu(), ref):.3e}")
    # the forward() surface: prefill with use_cache, then single steps on the cache
    kw = dict(neighbor_embeds=ne.cuda(), neighbor_attention_mask=valid.cuda())
    with torch.no_grad():
        o = lm(input_ids=ids.cuda(), attention_mask=am.cuda(), use_cache=True, cache_capacity=width + 2, return_logits=True, **kw)
        assert o.past_key_values.col == width and rel_err(o.logits[:, -1], steps[:, 0]) <= tol
        o2 = lm(input_ids=out[:, width:width + 1], past_key_values=o.past_key_values)
        assert o2.logits.shape == (B, 1, 128) and rel_err(o2.logits[:, 0], steps[:, 1]) <= tol and o2.past_key_values.col == width + 1
        lm(input_ids=out[:, width + 1:width + 2], past_key_values=o.past_key_values)
        with pytest.raises(ValueError, match="full"):
            lm(input_ids=out[:, width + 2:width + 3], past_key_values=o.past_key_values)
        # without the new arguments the forward returns no cache
        assert lm(input_ids=ids.cuda(), attention_mask=am.cuda(), **kw).past_key_values is None


@pytest.mark.parametrize("n_kv", [2, 1])
def test_cache_rows_hold_the_key_value_heads_only(n_kv):
    lm = _lm("tiny", n_kv).cuda()
    ne, valid = _neighbors(SEED, 64)
    ids, am = _prompt(SEED)
    with torch.no_grad():
        cache = lm(input_ids=ids.cuda(), attention_mask=am.cuda(), neighbor_embeds=ne.cuda(), neighbor_attention_mask=valid.cuda(),
                   use_cache=True, cache_capacity=T + 4).past_key_values
    D = 16
    assert len(cache.kv) == 4 and all(kv.shape == (B, T + 4, 2 * n_kv * D) for kv in cache.kv)
    assert len(cache.cross) == 2 and all(k.shape == (B, S, 64) and v.shape == (B, S, 64) for k, v in cache.cross)
    assert cache.col == T and torch.equal(cache.mask[:, :T].cpu(), am.to(torch.uint8)) and not cache.mask[:, T:].any()
    assert torch.equal(cache.cross_valid.cpu().bool(), valid)


def _forced_steps(lm, ids, am, ne, valid, tokens):
    """[B, 1 + n, V]: the prefill's last logits, then one decode step per forced token column of `tokens` [B, n]."""
    with torch.no_grad():
        o = lm(input_ids=ids.cuda(), attention_mask=am.cuda(), neighbor_embeds=ne.cuda(), neighbor_attention_mask=valid.cuda(), use_cache=True,
               cache_capacity=ids.shape[1] + tokens.shape[1], return_logits=True)
        logits = [o.logits[:, -1]]
        for s in range(tokens.shape[1]):
            logits.append(lm(input_ids=tokens[:, s:s + 1].cuda(), past_key_values=o.past_key_values).logits[:, 0])
    return torch.stack(logits, dim=1)


def test_neighbor_cache_is_live():
    ne, valid = _neighbors(SEED, 64)
    ids, am = _prompt(SEED)
    g = torch.Generator().manual_seed(9)
    other = torch.randn(ne.shape, generator=g)
    masked_only = torch.where(valid[..., None], ne, other)               # differs at masked neighbor tokens alone ...
    masked_only[5] = ne[5]                                               # ... of samples that have a valid one (none valid: uniform over all)
    assert (masked_only != ne).any()
    lm = _lm("tiny", 2).cuda()
    out, steps = _generate(lm, ids, am, ne, valid, return_step_logits=True)
    # open gates: the same tokens forced through a cache of other neighbor embeddings give other logits, at the prefill and at every step
    forced = out[:, T:T + 4]
    mine, theirs = _forced_steps(lm, ids, am, ne, valid, forced), _forced_steps(lm, ids, am, other, valid, forced)
    assert rel_err(mine[:, :4], steps[:, :4]) <= TAU[torch.float32]
    per_step = [(mine[:, s] - theirs[:, s]).abs().max().item() / mine.abs().max().item() for s in range(5)]
    print(f"step logits under other neighbor embeddings, same tokens: rel diff per step {per_step}")
    assert min(per_step) > 10 * TAU[torch.float32], per_step
    _, steps_masked = _generate(lm, ids, am, masked_only, valid, return_step_logits=True)
    assert torch.equal(steps_masked, steps), "a masked neighbor's embedding changed the logits"
    shut = _lm("tiny", 2, gates=False).cuda()
    _, a = _generate(shut, ids, am, ne, valid, return_step_logits=True)
    _, b = _generate(shut, ids, am, other, valid, return_step_logits=True)
    assert torch.equal(a, b), "at gates 0 the neighbors changed the logits"


def test_eos_rows_are_padded():
    lm = _lm("tiny", 2).cuda()
    ne, valid = _neighbors(SEED, 64)
    ids, am = _prompt(SEED)
    free = _generate(lm, ids, am, ne, valid).cpu()
    eos = int(free[0, T + 3])                                            # a token the model does emit
    out = _generate(lm, ids, am, ne, valid, eos_token_id=eos, pad_token_id=1).cpu()
    assert out.shape == (B, T + N_NEW) and torch.equal(out[:, :T], ids)
    hit = 0
    for b in range(B):
        new, ref = out[b, T:], free[b, T:]
        pos = (ref == eos).nonzero()
        if len(pos) == 0:
            assert torch.equal(new, ref)
            continue
        p = int(pos[0])
        hit += 1
        assert torch.equal(new[:p + 1], ref[:p + 1]) and (new[p + 1:] == 1).all(), (b, new.tolist(), ref.tolist())
    assert hit >= 1 and int((free[0, T:] == eos).nonzero()[0]) <= 3
    assert torch.equal(_generate(lm, ids, am, ne, valid, eos_token_id=eos).cpu(), out)       # the default pad is the config's
    assert torch.equal(_generate(lm, ids, am, ne, valid, eos_token_id=None, pad_token_id=1).cpu(), free)


def test_wrapper_composition_over_a_gqa_llama():
    """CrossAttentionModel keeps teacher-forcing a Llama LM (can_generate() is False); its LM generates from the wrapper's own neighbor
    tokens, and that equals the uncached loop over the wrapper's forward on the same ids."""
    from mmgl_amd.model import CrossAttentionModel
    torch.manual_seed(SEED)
    w = CrossAttentionModel(mpt_args(model_name_or_path="llama-tiny", context="text_only", neighbor_layer_wise=2), None,
                            lm_config=_config("tiny", 2), text_config=tiny_roberta_config(), visual_config=tiny_clip_vision_config())
    _open_gates(w.lm, 64)
    w = w.cuda().eval()
    assert w.can_generate() is False and w.lm.can_generate() is True
    g = torch.Generator().manual_seed(1)
    ids, am = _prompt(SEED)
    ids, am = ids.cuda(), am.cuda()
    nb = dict(neighbor_input_ids=torch.randint(3, 128, (B, 3, 12), generator=g).cuda(),
              neighbor_attention_mask=torch.ones(B, 3, 12, dtype=torch.long).cuda(),
              neighbor_pos_ids=torch.tensor([[1, 2, 0], [1, 0, 0], [1, 2, 3], [0, 0, 0]] * 2).cuda())
    n_new = 6
    with torch.no_grad():
        ne, valid = w._neighbor_tokens(nb["neighbor_input_ids"], nb["neighbor_attention_mask"], nb["neighbor_pos_ids"], None, None, None,
                                       None, None)
        out, steps = w.lm.generate(ids, am, neighbor_embeds=ne, neighbor_attention_mask=valid, max_new_tokens=n_new, return_step_logits=True)
        for s in range(n_new):
            mask = torch.cat([am, torch.ones(B, s, dtype=am.dtype, device="cuda")], dim=1)
            cur = out[:, :T + s]
            ref = w(cur, mask, cur, **nb).logits[:, -1]
            err = rel_err(steps[:, s], ref)
            assert err <= 1e-3, f"step {s}: rel err {err:.3e} against the wrapper's forward"


def test_limits():
    lm = _lm("tiny", 2, max_pos=32).cuda()
    ne, valid = _neighbors(SEED, 64)
    ids, am = _prompt(SEED)
    out = _generate(lm, ids, am, ne, valid, n_new=21)                     # the last token read sits at position 31
    assert out.shape == (B, T + 21)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        _generate(lm, ids, am, ne, valid, n_new=22)


@pytest.mark.parametrize("batch", [2, 64])
def test_full_width_steps_match_the_uncached_forward(batch):
    """Llama-3.2-1B layer dimensions (hidden 2048, H = 32, Hkv = 8, D = 64, inter 8192, vocab 32000), random weights, 2 frozen layers and
    one gated layer, prompt 64, bf16: prefill plus 3 steps against the product's own uncached forward on the same tokens.  Reaches the
    MFMA skinny routes at K = 2048 and K = 8192, the lm_head route and the 64-row limit."""
    from transformers import LlamaConfig
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    torch.manual_seed(11)
    cfg = LlamaConfig(vocab_size=32000, hidden_size=2048, intermediate_size=8192, num_hidden_layers=2, num_attention_heads=32,
                      num_key_value_heads=8, max_position_embeddings=256, pad_token_id=1, bos_token_id=2, eos_token_id=2, attention_dropout=0.0)
    with torch.device("cuda"):
        lm = LlamaNeighborLM(mpt_args(model_name_or_path="llama-tiny", neighbor_layer_wise=2), cfg)
    _open_gates(lm, 2048)
    lm = lm.bfloat16().eval()
    assert len(lm.neighbor_layers) == 1 and lm._frozen[0].Hkv == 8 and lm._frozen[0].D == 64
    width, n_new, ns = 64, 4, 16
    ids, am = _prompt(3, width=width, batch=batch, vocab=32000)
    g = torch.Generator().manual_seed(5)
    ne = torch.randn(batch, ns, 2048, generator=g).bfloat16()
    nv = torch.rand(batch, ns, generator=g) > 0.3
    nv[:, 0] = True
    nv[batch - 1] = False                                               # a sample without any valid neighbor
    out, steps = _generate(lm, ids, am, ne, nv, n_new=n_new, return_step_logits=True)
    assert out.shape == (batch, width + n_new) and torch.isfinite(steps.float()).all()
    ref = _reference_steps(_uncached_last_logits(lm, ne, nv), out.cpu(), am, n_new)
    for s in range(n_new):
        err = rel_err(steps[:, s].float().cpu(), ref[:, s])
        print(f"full width B={batch} step {s}: rel err {err:.3e}")
        assert err <= BF16_LOGITS_TOL, (batch, s, err)
