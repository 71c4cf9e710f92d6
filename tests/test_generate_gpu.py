"""-m gpu: greedy generation with a key/value cache (MPTForCausalLM.generate / CrossAttentionModel.generate on the HIP decode path).

Comparison rule of every test that has a reference: at step s the reference runs UNCACHED on the tokens the product has produced so
far, so one near-tie cannot cascade.  The step logits are compared at tau (max-norm relative error: 1e-3 fp32 -- BASELINE.json --,
2e-2 bf16 -- DESIGN.md 2), and the product's token must equal the reference's argmax wherever the reference's top-1 minus top-2 margin
exceeds 2 tau max|logit| (two implementations within tau of each other cannot disagree there).  The share of (sample, step) pairs
below that margin is computed from the reference alone and asserted BEFORE any comparison (<= 5 % fp32, <= 25 % bf16).  On the
CPU oracle's own greedy tokens, with tiny_opt_config(dropout=0), this layout and these gates, seeds 0-5 give 0-1.6 % at the fp32
margin and 15-25 % at the bf16 margin for the wrapper (0-3.1 % fp32 for the plain fork); SEED = 1 sits at 1.6 % / 14.8 % (fork
0.8 %), so an unlucky change fails loudly instead of hiding cases.

Layout: B = 8, prompt width 12 with ragged right padding, 16 new tokens, tiny models of tests/helpers.py, gates set to non-zero
values (at their initial 0 the cross layers are inert and a test of them shows nothing)."""
import pytest
import torch

from helpers import mpt_args, rel_err, tiny_clip_vision_config, tiny_opt_config, tiny_roberta_config

pytestmark = pytest.mark.gpu

B, T, N_NEW = 8, 12, 16
TAU = {torch.float32: 1e-3, torch.bfloat16: 2e-2}
LOW_MARGIN_SHARE = {torch.float32: 0.05, torch.bfloat16: 0.25}
SEED = 1
BF16_LOGITS_TOL = 2.5e-2          # tests/test_model_gpu.py: bf16 logits at full size


def _prompt(seed, width=T, ragged=True, batch=B, vocab=128):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab, (batch, width), generator=g)
    am = torch.ones_like(ids)
    if ragged:
        for b in range(1, batch):                       # sample 0 fills the width; every sample keeps its first token
            am[b, int(torch.randint(1, width + 1, (1,), generator=g)):] = 0
    return torch.where(am.bool(), ids, torch.ones_like(ids)), am


def _neighbors(seed, batch=B, Nt=3, Ni=2, L=12, image=32, empty=5):
    """Neighbor fields of a context-`all` batch: ragged neighbor counts, a random interleave of the valid slots, padding slots
    last; sample `empty` has no valid neighbor at all."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    nids = torch.randint(3, 128, (batch, Nt, L), generator=g)
    nam = torch.ones(batch, Nt, L, dtype=torch.long)
    npos, ipos = torch.zeros(batch, Nt, dtype=torch.long), torch.zeros(batch, Ni, dtype=torch.long)
    tloc, iloc = torch.zeros(batch, Nt, dtype=torch.long), torch.zeros(batch, Ni, dtype=torch.long)
    imgs = torch.zeros(batch, Ni, 3, image, image)
    for b in range(batch):
        nt, ni = (0, 0) if b == empty else (ri(1, Nt), ri(0, Ni))
        for j in range(Nt):
            ln = ri(3, L) if j < nt else 2
            nids[b, j, 0] = 0
            nids[b, j, ln - 1] = 2
            nids[b, j, ln:] = 1
            nam[b, j, ln:] = 0
            npos[b, j] = j + 1 if j < nt else 0
        for j in range(ni):
            imgs[b, j] = torch.randn(3, image, image, generator=g)
            ipos[b, j] = j + 1
        kinds = ["t"] * nt + ["i"] * ni
        order = [kinds[q] for q in torch.randperm(len(kinds), generator=g).tolist()]
        ti = ii = 0
        for loc, kd in enumerate(order):
            if kd == "t":
                tloc[b, ti] = loc
                ti += 1
            else:
                iloc[b, ii] = loc
                ii += 1
        loc = len(order)
        for j in range(nt, Nt):
            tloc[b, j] = loc
            loc += 1
        for j in range(ni, Ni):
            iloc[b, j] = loc
            loc += 1
    return dict(neighbor_input_ids=nids, neighbor_attention_mask=nam, neighbor_pos_ids=npos, text_locations=tloc, neighbor_images=imgs,
                neighbor_images_pos_ids=ipos, image_locations=iloc)


def _reference_steps(ref_last_logits, ids, am, n_new):
    """[B, n_new, V] fp32: the uncached reference on the product's own tokens, one run per step."""
    width = am.shape[1]
    out = []
    for s in range(n_new):
        mask = torch.cat([am, torch.ones(am.shape[0], s, dtype=am.dtype)], dim=1)
        out.append(ref_last_logits(ids[:, :width + s], mask).float())
    return torch.stack(out, dim=1)


def _compare(step_logits, ids, ref, dtype, what, tau=None):
    """The comparison rule of the module docstring.  Returns the mask of (sample, step) pairs below the margin."""
    tau = TAU[dtype] if tau is None else tau
    n_new = ref.shape[1]
    scale = ref.abs().max().item()
    top2 = ref.topk(2, dim=-1).values
    low = (top2[..., 0] - top2[..., 1]) <= 2 * tau * scale
    share = low.float().mean().item()
    print(f"{what}: {share * 100:.1f} % of the {low.numel()} (sample, step) pairs are below the margin 2 tau max|logit| = {2 * tau * scale:.3e}")
    assert share <= LOW_MARGIN_SHARE[dtype], f"{what}: {share:.3f} of the steps are near-ties of the reference itself"
    err = rel_err(step_logits.float().cpu(), ref)
    print(f"{what}: step logits rel err {err:.3e} (tau {tau:.1e})")
    assert err <= tau, f"{what}: step logits rel err {err:.3e} > {tau:.1e}"
    tokens = ids[:, -n_new:].cpu()
    assert torch.equal(tokens, step_logits.float().argmax(-1).cpu()), f"{what}: the returned ids are not the argmax of the returned step logits"
    wrong = (tokens != ref.argmax(-1)) & ~low
    assert not wrong.any(), f"{what}: {int(wrong.sum())} tokens differ from the reference argmax at a clear margin: {wrong.nonzero().tolist()[:8]}"
    return low


def _fork(pre_ln=True, proj=None, seed=SEED):
    from transformers import OPTForCausalLM
    from mmgl_amd.model.modelling_cross_attention import MPTConfig, MPTForCausalLM, copy_opt_weights
    torch.manual_seed(seed)
    oc = tiny_opt_config(pre_ln=pre_ln, proj=proj, dropout=0.0)
    hf = OPTForCausalLM(oc).eval()
    lm = MPTForCausalLM(MPTConfig(mpt_args(neighbor_mode="raw", peft_type="none"), oc))
    copy_opt_weights(hf, lm)
    return hf, lm.eval()


def test_fp32_fork_equal_length_prompts_vs_hf_generate():
    hf, lm = _fork()
    ids, am = _prompt(SEED, ragged=False)
    lm = lm.cuda()
    out, steps = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, return_step_logits=True)
    assert out.shape == (B, T + N_NEW) and steps.shape == (B, N_NEW, 128) and torch.equal(out[:, :T].cpu(), ids)
    with torch.no_grad():
        ref = _reference_steps(lambda i, m: hf(input_ids=i, attention_mask=m).logits[:, -1], out.cpu(), am, N_NEW)
        low = _compare(steps, out, ref, torch.float32, "fork fp32 vs HF OPT (uncached, product tokens)")
        hf.generation_config.eos_token_id = None                        # all N_NEW steps, as the product runs them
        hf_ids = hf.generate(input_ids=ids, attention_mask=am, do_sample=False, num_beams=1, max_new_tokens=N_NEW, min_new_tokens=N_NEW,
                             pad_token_id=1)
    assert hf_ids.shape == out.shape
    # HF's own greedy loop: identical up to each sample's first near-tie (after one the two continuations are different texts)
    for b in range(B):
        first_low = int(low[b].nonzero()[0]) if low[b].any() else N_NEW
        assert torch.equal(hf_ids[b, :T + first_low], out[b, :T + first_low].cpu()), (b, first_low)
    assert sum(int(low[b].nonzero()[0]) if low[b].any() else N_NEW for b in range(B)) >= B * N_NEW // 2


def _wrapper(seed=SEED, round_bf16=False):
    """(wrapper on the CPU in fp32, its neighbor batch, the uncached oracle's last-position logits as a function of (ids, mask))."""
    from oracle import lm_ref, wrapper_ref
    from mmgl_amd.model import CrossAttentionModel
    torch.manual_seed(seed)
    oc = tiny_opt_config(dropout=0.0)
    w = CrossAttentionModel(mpt_args(context="all"), tokenizer=None, lm_config=oc, text_config=tiny_roberta_config(),
                            visual_config=tiny_clip_vision_config()).eval()
    with torch.no_grad():
        gates = [p for n_, p in w.named_parameters() if n_.endswith(("gating1", "gating2"))]
        assert len(gates) == 4
        for p, v in zip(gates, (0.6, -0.8, 0.9, 0.5)):
            p.fill_(v)
        if round_bf16:                                                  # the oracle sees the weights the bf16 product computes with
            for p in w.parameters():
                p.copy_(p.bfloat16().float())
    nb = _neighbors(seed + 100)
    sd = {k: v.detach().float() for k, v in w.state_dict().items()}
    with torch.no_grad():
        L = nb["neighbor_input_ids"].shape[-1]
        tl = w.text_model(input_ids=nb["neighbor_input_ids"].reshape(-1, L), attention_mask=nb["neighbor_attention_mask"].reshape(-1, L)).last_hidden_state
        vp = w.visual_model(nb["neighbor_images"].reshape(-1, 3, 32, 32)).pooler_output
        te = wrapper_ref.project_neighbors(sd, "text", wrapper_ref.text_pooler(sd, tl), nb["neighbor_pos_ids"], B, 2)
        ve = wrapper_ref.project_neighbors(sd, "visual", vp, nb["neighbor_images_pos_ids"], B, 2)
        ne, nm = wrapper_ref.interleave_neighbors(te, ve, nb["neighbor_pos_ids"], nb["neighbor_images_pos_ids"], nb["text_locations"],
                                                  nb["image_locations"])
    assert not nm[5].any() and nm[:5].any(dim=1).all()                  # one sample without any valid neighbor
    lm = {k[3:]: v for k, v in sd.items() if k.startswith("lm.")}
    cfg = lm_ref.LMConfig(vocab_size=oc.vocab_size, hidden_size=oc.hidden_size, num_attention_heads=oc.num_attention_heads, ffn_dim=oc.ffn_dim,
                          num_hidden_layers=oc.num_hidden_layers, word_embed_proj_dim=oc.word_embed_proj_dim, neighbor_layer_wise=2)

    def last_logits(ids, mask):
        with torch.no_grad():
            return lm_ref.causal_lm_forward(lm, cfg, ids, mask, None, ne, nm)[0][:, -1]
    return w, nb, last_logits


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cross_attention_model_vs_oracle_loop(dtype):
    """Context `all`, text and image neighbors, one sample with no valid neighbor, ragged prompts; fp32, and bf16 against the oracle
    on the bf16-rounded weights."""
    w, nb, oracle = _wrapper(round_bf16=dtype == torch.bfloat16)
    ids, am = _prompt(SEED)
    w = w.to(dtype).cuda()
    out, steps = w.generate(ids.cuda(), am.cuda(), **{k: v.cuda() for k, v in nb.items()}, max_new_tokens=N_NEW, return_step_logits=True)
    assert out.shape == (B, T + N_NEW) and steps.dtype == dtype
    ref = _reference_steps(oracle, out.cpu(), am, N_NEW)
    _compare(steps, out, ref, dtype, f"CrossAttentionModel {dtype} vs oracle loop")
    # the same through host_meta (no device->host synchronisation in the neighbor encoders): the same tokens
    from mmgl_amd.model.modelling_cross_attention import host_metadata
    meta = host_metadata(dict(nb, attention_mask=am))
    out2 = w.generate(ids.cuda(), am.cuda(), **{k: v.cuda() for k, v in nb.items()}, host_meta=meta, max_new_tokens=N_NEW)
    assert torch.equal(out2, out)


def _uncached_last_logits(lm, ids, mask, **kw):
    with torch.no_grad():
        return lm(input_ids=ids.cuda(), attention_mask=mask.cuda(), return_logits=True, **kw).logits[:, -1].float().cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("pre_ln,proj,width", [(True, None, T), (False, 32, T), (True, None, 1), (False, None, 1)])
def test_cached_equals_uncached_inside_the_product(pre_ln, proj, width, dtype):
    """Step logits of the cache path against forward(..., return_logits=True) on the full prefix: pre-LN, post-LN (with
    project_in / project_out), and a prompt of width 1."""
    _, lm = _fork(pre_ln, proj)
    lm = lm.to(dtype).cuda()
    ids, am = _prompt(SEED + 1, width=width)
    out, steps = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, return_step_logits=True)
    ref = _reference_steps(lambda i, m: _uncached_last_logits(lm, i, m), out.cpu(), am, N_NEW)
    err = rel_err(steps.float().cpu(), ref)
    print(f"cached vs uncached pre_ln={pre_ln} proj={proj} width={width} {dtype}: rel err {err:.3e}")
    assert err <= TAU[dtype], err
    # and the forward() surface gives the same logits (the prefill's own lm_head runs the full-sequence GEMM route: same numbers to tau)
    with torch.no_grad():
        o = lm(input_ids=ids.cuda(), attention_mask=am.cuda(), use_cache=True, cache_capacity=width + 2, return_logits=True)
        assert o.past_key_values.col == width and rel_err(o.logits[:, -1], steps[:, 0]) <= TAU[dtype]
        o2 = lm(input_ids=out[:, width:width + 1], past_key_values=o.past_key_values)
        assert o2.logits.shape == (B, 1, 128) and rel_err(o2.logits[:, 0], steps[:, 1]) <= TAU[dtype] and o2.past_key_values.col == width + 1
        lm(input_ids=out[:, width + 1:width + 2], past_key_values=o.past_key_values)
        with pytest.raises(ValueError, match="full"):
            lm(input_ids=out[:, width + 2:width + 3], past_key_values=o.past_key_values)


def test_neighbor_cache_is_live():
    w, nb, _ = _wrapper()
    ids, am = _prompt(SEED)
    w = w.cuda()
    dev = {k: v.cuda() for k, v in nb.items()}
    out, steps = w.generate(ids.cuda(), am.cuda(), **dev, max_new_tokens=N_NEW, return_step_logits=True)
    # the plain LM forced along the same tokens: feed them step by step without neighbors
    with torch.no_grad():
        o = w.lm(input_ids=ids.cuda(), attention_mask=am.cuda(), use_cache=True, cache_capacity=T + N_NEW, return_logits=True)
        plain = [o.logits[:, -1]]
        for s in range(N_NEW - 1):
            plain.append(w.lm(input_ids=out[:, T + s:T + s + 1], past_key_values=o.past_key_values).logits[:, 0])
    plain = torch.stack(plain, dim=1)
    diff = rel_err(steps, plain)
    print(f"step logits with vs without neighbors: rel diff {diff:.3e}")
    assert diff > 10 * TAU[torch.float32]
    per_step = [(steps[:, s] - plain[:, s]).abs().max().item() / plain.abs().max().item() for s in range(N_NEW)]
    assert min(per_step[1:]) > 10 * TAU[torch.float32], per_step          # decode steps too, not only the prefill
    # and with other neighbor content the decode steps move: the cached neighbor keys are what the steps attend to
    dev2 = dict(dev, neighbor_images=torch.randn_like(dev["neighbor_images"]))
    _, steps2 = w.generate(ids.cuda(), am.cuda(), **dev2, max_new_tokens=2, return_step_logits=True)
    assert (steps2[:, 0] - steps[:, 0]).abs().max() > 0


def test_eos_rows_are_padded():
    _, lm = _fork()
    lm = lm.cuda()
    ids, am = _prompt(SEED)
    free = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW).cpu()
    eos = int(free[0, T + 3])                                            # a token the model does emit
    out = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, eos_token_id=eos, pad_token_id=1).cpu()
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
    # the default pad is the config's
    out2 = lm.generate(ids.cuda(), am.cuda(), max_new_tokens=N_NEW, eos_token_id=eos).cpu()
    assert torch.equal(out2, out)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        lm.generate(ids.cuda(), am.cuda(), max_new_tokens=64)


def test_evaluate_loop_test_prefix_generates(tmp_path):
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
    assert model.can_generate()
    calls, real = [], model.generate

    def counting(**kw):
        out = real(**kw)
        calls.append((tuple(kw["input_ids"].shape), tuple(out.shape), kw.get("host_meta") is not None, "neighbor_input_ids" in kw))
        return out
    model.generate = counting
    try:
        evaluate_loop(loader(), model, tokenizer, 0, args, prefix="test")
        generated = dict(evaluate_loop.last)
        assert len(calls) >= 1 and sum(c[0][0] for c in calls) == 8, calls
        for shape_in, shape_out, has_meta, has_neighbors in calls:
            assert shape_in[1] == args.max_input_length and shape_out == (shape_in[0], args.max_input_length + 32)
            assert has_meta and has_neighbors
        n_calls = len(calls)
        evaluate_loop(loader(), model, tokenizer, 0, args, prefix="val")               # every other prefix: the argmax path
        assert len(calls) == n_calls
        argmax = dict(evaluate_loop.last)
        assert generated["loss"] == argmax["loss"]                                      # the meter stays the teacher-forced one
        model.can_generate = lambda: False                                              # e.g. the Llama-family LM
        evaluate_loop(loader(), model, tokenizer, 0, args, prefix="test")
        assert len(calls) == n_calls and dict(evaluate_loop.last) == argmax
    finally:
        del model.generate
        model.__dict__.pop("can_generate", None)


@pytest.mark.parametrize("batch", [2, 64])
def test_full_width_steps_match_the_uncached_forward(batch):
    """Config-3 dimensions (d = 2048, 32 heads of 64, ffn 8192, vocab 50272), random weights, 4 frozen + 2 gated layers (the
    kernels see the real shapes; the layer count only repeats them), prompt 512, 64 neighbor tokens, bf16: prefill plus 3 steps
    against the product's own uncached forward on the same tokens."""
    from transformers import OPTConfig
    from mmgl_amd.model.modelling_cross_attention import MPTConfig, MPTForCausalLM, _lin
    torch.manual_seed(11)
    oc = OPTConfig(vocab_size=50272, hidden_size=2048, num_attention_heads=32, ffn_dim=8192, num_hidden_layers=4, max_position_embeddings=2048,
                   word_embed_proj_dim=2048, do_layer_norm_before=True, dropout=0.1, attention_dropout=0.0, pad_token_id=1, bos_token_id=2,
                   eos_token_id=2)
    with torch.device("cuda"):
        lm = MPTForCausalLM(MPTConfig(mpt_args(neighbor_mode="embedding", neighbor_layer_wise=2), oc))
    with torch.no_grad():
        for n_, p in lm.named_parameters():
            if n_.endswith(("gating1", "gating2")):
                p.fill_(0.5)
    lm = lm.bfloat16().eval()
    assert len(lm.model.decoder.neighbor_layers) == 2
    width, n_new, S = 512, 4, 64
    ids, am = _prompt(3, width=width, batch=batch, vocab=50272)
    g = torch.Generator().manual_seed(5)
    ne = torch.randn(batch, S, 2048, generator=g).bfloat16().cuda()
    nv = torch.rand(batch, S, generator=g) > 0.3
    nv[:, 0] = True
    nv[batch - 1] = False                                               # a sample without any valid neighbor
    nv = nv.cuda()
    out, steps = lm.generate(ids.cuda(), am.cuda(), neighbor_embeds=ne, neighbor_attention_mask=nv, max_new_tokens=n_new, return_step_logits=True)
    assert out.shape == (batch, width + n_new) and torch.isfinite(steps.float()).all()
    dec = lm.model.decoder
    for s in range(n_new):
        mask = torch.cat([am, torch.ones(batch, s, dtype=am.dtype)], dim=1).cuda()
        with torch.no_grad():
            h = dec(input_ids=out[:, :width + s], attention_mask=mask, neighbor_embeds=ne, neighbor_attention_mask=nv).last_hidden_state
            ref = _lin(lm.lm_head, h[:, -1:].contiguous())[:, 0].float()
        err = rel_err(steps[:, s].float(), ref)
        print(f"full width B={batch} step {s}: rel err {err:.3e}")
        assert err <= BF16_LOGITS_TOL, (batch, s, err)
