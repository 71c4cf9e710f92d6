"""-m gpu: cached generation of a T5 (T5HipRunner.generate, SelfAttentionModel.generate over a T5, evaluate_loop(generate_seq2seq)).

Comparison rule (that of tests/test_generate_llama_gpu.py, restated): at step s the reference runs UNCACHED -- HuggingFace
T5ForConditionalGeneration on the CPU in fp32 (for a bf16 model: on the bf16-rounded weights), decoder_input_ids = the product's own
tokens so far, .logits[:, -1] -- so one near-tie cannot cascade.  The step logits must lie within tau of the reference by helpers.rel_err
(1e-3 fp32, 2e-2 bf16), the returned ids must be the argmax of the returned step logits, and the token must equal the reference's argmax
wherever the reference's top-1 minus top-2 margin exceeds 2 tau max|logit|.  The share of (sample, step) pairs below that margin comes
from the reference alone and is asserted FIRST: <= 5 % fp32, <= 40 % bf16.  A cap is a condition, not a measurement.

Construction: T5Config(vocab 128, dropout 0, decoder_start_token_id 0, pad 0, eos 1, tie_word_embeddings=False), "small" = d_model 128 / d_kv 64 /
d_ff 256 / 2 + 2 layers / 2 heads, "mid" = 256 / 64 / 512 / 2 + 2 / 4, built under torch.manual_seed(seed); then from
Generator(seed + 100), in this order, lm_head.weight = randn d_model^-0.5, the encoder table = 2 randn, the decoder table = 2 randn.
Prompts: B = 8, width 12, ragged right padding (the Llama test's _prompt with pad id 0); 24 new tokens, so the distances cross the
exact / log bucket boundary at 16.  With the reference's own greedy tokens, seed 0 gave on the CPU: small fp32 1.0 % below the margin (26
distinct tokens), mid on bf16-rounded weights 25.0 % at tau 2e-2 (22 distinct tokens) -- both at or below 0.8 of the cap; seeds 1 and 2
likewise.  On that construction zeroing the decoder table moves the step logits by >= 0.24 of max|logit| on every sample, ignoring the
encoder mask by >= 0.096 on every ragged sample: the comparison sees both.  A default-initialised tiny T5 with the tied head is NOT
usable here: it emits one single token at every step of every sample and the decoder table then has no effect on its logits.

Measured on an MI355X: docs/t5_generate_mi355x.md."""
import copy

import pytest
import torch
from transformers import T5Config, T5ForConditionalGeneration

from helpers import mpt_args, rel_err, tiny_clip_vision_config, tiny_roberta_config

pytestmark = pytest.mark.gpu

B, T, N_NEW, V = 8, 12, 24, 128
TAU = {torch.float32: 1e-3, torch.bfloat16: 2e-2}
LOW_MARGIN_SHARE = {torch.float32: 0.05, torch.bfloat16: 0.40}
BF16_LOGITS_TOL = 2.5e-2          # tests/test_generate_gpu.py: the project's bound on bf16 logits
SEED = 0
SIZES = {"small": dict(d_model=128, d_kv=64, d_ff=256, num_heads=2), "mid": dict(d_model=256, d_kv=64, d_ff=512, num_heads=4)}


def _cfg(size, tie=False, vocab=V, **kw):
    return T5Config(vocab_size=vocab, dropout_rate=0.0, decoder_start_token_id=0, pad_token_id=0, eos_token_id=1, tie_word_embeddings=tie,
                    num_layers=2, num_decoder_layers=2, **SIZES[size], **kw)


def _randomise(lm, seed):
    """The draws of the module docstring.  Where transformers ties lm_head to `shared` whatever the config says (tie_word_embeddings=False
    then only drops the d_model^-0.5 scale of the decoder output), the head's draw is the embedding's too."""
    g = torch.Generator().manual_seed(seed + 100)
    d = lm.config.d_model
    with torch.no_grad():
        lm.lm_head.weight.copy_(torch.randn(lm.lm_head.weight.shape, generator=g) * d ** -0.5)
        for stack in (lm.encoder, lm.decoder):
            table = stack.block[0].layer[0].SelfAttention.relative_attention_bias.weight
            table.copy_(torch.randn(table.shape, generator=g) * 2.0)
    return lm


def _model(size, seed=SEED, tie=False):
    torch.manual_seed(seed)
    return _randomise(T5ForConditionalGeneration(_cfg(size, tie)), seed).eval()


def _prompt(seed, width=T, batch=B, vocab=V):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab, (batch, width), generator=g)
    am = torch.ones_like(ids)
    for b in range(1, batch):                           # sample 0 fills the width; every sample keeps its first token
        am[b, int(torch.randint(1, width + 1, (1,), generator=g)):] = 0
    return torch.where(am.bool(), ids, torch.zeros_like(ids)), am


def _reference(lm):
    """The fp32 CPU copy of lm's present weights (of a bf16 model: the rounded ones)."""
    return copy.deepcopy(lm).float().cpu().eval()


def _reference_steps(ref, out, n_new, rows=None, **enc):
    """[rows, n_new, V] fp32: the uncached reference on the product's own decoder row out [B, 1 + n_new], one run per step."""
    out = out.cpu()
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])
    enc = {k: pick(v.detach().float().cpu() if v.is_floating_point() else v.cpu()) for k, v in enc.items()}
    steps = []
    with torch.no_grad():
        for s in range(n_new):
            steps.append(ref(decoder_input_ids=pick(out)[:, :1 + s], **enc).logits[:, -1].float())
    return torch.stack(steps, dim=1)


def _compare(step_logits, out, ref, dtype, what):
    tau = TAU[dtype]
    top2 = ref.topk(2, dim=-1).values
    low = (top2[..., 0] - top2[..., 1]) <= 2 * tau * ref.abs().max().item()
    share = low.float().mean().item()
    print(f"{what}: {share * 100:.1f} % of the {low.numel()} (sample, step) pairs are below the margin 2 tau max|logit|")
    assert share <= LOW_MARGIN_SHARE[dtype], f"{what}: {share:.3f} of the steps are near-ties of the reference itself"
    err = rel_err(step_logits.float().cpu(), ref)
    print(f"{what}: step logits rel err {err:.3e} (tau {tau:.1e})")
    assert err <= tau, f"{what}: step logits rel err {err:.3e} > {tau:.1e}"
    tokens = out[:, 1:].cpu()
    assert torch.equal(tokens, step_logits.float().argmax(-1).cpu()), f"{what}: the returned ids are not the argmax of the returned step logits"
    wrong = (tokens != ref.argmax(-1)) & ~low
    assert not wrong.any(), f"{what}: {int(wrong.sum())} tokens differ from the reference argmax at a clear margin: {wrong.nonzero().tolist()[:8]}"
    print(f"{what}: {tokens.unique().numel()} distinct tokens")


def _runner(lm):
    from mmgl_amd.model.t5_hip import T5HipRunner
    return T5HipRunner(lm)


@pytest.fixture(scope="module")
def small():
    """The fp32 small model on the GPU, its runner, its CPU reference, the prompts and the plain greedy run with its reference steps."""
    lm = _model("small")
    ref = _reference(lm)
    ids, am = _prompt(SEED)
    run = _runner(lm.cuda())
    out, steps = run.generate(input_ids=ids.cuda(), attention_mask=am.cuda(), max_new_tokens=N_NEW, return_step_logits=True)
    want = _reference_steps(ref, out, N_NEW, input_ids=ids, attention_mask=am)
    return dict(lm=lm, ref=ref, ids=ids, am=am, run=run, out=out, steps=steps, want=want)


def test_fp32_small_from_input_ids(small):
    out, steps = small["out"], small["steps"]
    assert out.shape == (B, 1 + N_NEW) and out.dtype == torch.int64 and bool((out[:, 0] == 0).all())
    assert steps.shape == (B, N_NEW, V) and steps.dtype == torch.float32
    _compare(steps, out, small["want"], torch.float32, "small fp32 from input_ids")
    again = small["run"].generate(input_ids=small["ids"].cuda(), attention_mask=small["am"].cuda(), max_new_tokens=N_NEW)
    assert torch.equal(again, out), "two runs differ"
    one = small["run"].generate(input_ids=small["ids"].cuda(), attention_mask=small["am"].cuda(), max_new_tokens=1)
    assert torch.equal(one, out[:, :2]), "a single new token (a cache of one column) differs from the first of 24"


def test_encode_is_the_encoder_half(small):
    ids, am = small["ids"], small["am"]
    with torch.no_grad():
        got = small["run"].encode(input_ids=ids.cuda(), attention_mask=am.cuda())
        same = small["run"].encode(inputs_embeds=small["lm"].shared(ids.cuda()), attention_mask=am.cuda())
        want = small["ref"].encoder(input_ids=ids, attention_mask=am).last_hidden_state
    assert got.shape == (B, T, 128) and torch.equal(got, same)
    keep = am.bool()                                            # the rows of pad tokens are no key of any later attention
    err = rel_err(got.float().cpu()[keep], want[keep])
    print(f"encode fp32: rel err {err:.3e} on the valid rows")
    assert err <= TAU[torch.float32], err


def test_bf16_mid_from_input_ids():
    lm = _model("mid").bfloat16()
    ref = _reference(lm)
    ids, am = _prompt(SEED)
    out, steps = _runner(lm.cuda()).generate(input_ids=ids.cuda(), attention_mask=am.cuda(), max_new_tokens=N_NEW, return_step_logits=True)
    assert out.shape == (B, 1 + N_NEW) and steps.dtype == torch.bfloat16
    _compare(steps, out, _reference_steps(ref, out, N_NEW, input_ids=ids, attention_mask=am), torch.bfloat16, "mid bf16 from input_ids")


def test_fp32_small_from_inputs_embeds(small):
    ids, am, lm = small["ids"], small["am"], small["lm"]
    with torch.no_grad():
        emb = lm.shared(ids.cuda())
    out, steps = small["run"].generate(inputs_embeds=emb, attention_mask=am.cuda(), max_new_tokens=N_NEW, return_step_logits=True)
    assert torch.equal(out, small["out"]), "shared(ids) passed as embeddings gives other tokens than the ids"
    _compare(steps, out, _reference_steps(small["ref"], out, N_NEW, inputs_embeds=emb, attention_mask=am), torch.float32,
             "small fp32 from inputs_embeds")


def test_tied_head_scale_at_teacher_forced_level():
    """A tied head multiplies the decoder output by d_model^-0.5 in front of lm_head: the step logits against the reference within tau
    (without the scale they are 11 times too large).  No token claim rests on this model (module docstring)."""
    lm = _model("small", tie=True)
    assert getattr(lm.config, "scale_decoder_outputs", lm.config.tie_word_embeddings)
    ref = _reference(lm)
    ids, am = _prompt(SEED)
    out, steps = _runner(lm.cuda()).generate(input_ids=ids.cuda(), attention_mask=am.cuda(), max_new_tokens=N_NEW, return_step_logits=True)
    want = _reference_steps(ref, out, N_NEW, input_ids=ids, attention_mask=am)
    err = rel_err(steps.float().cpu(), want)
    print(f"tied head fp32: step logits rel err {err:.3e}")
    assert err <= TAU[torch.float32], err


def test_batch_of_70_rows_bf16():
    """decode_linear chunks its rows at 64: rows 0-2 and 67-69 against the uncached reference, 8 new tokens."""
    n_new, rows = 8, [0, 1, 2, 67, 68, 69]
    lm = _model("mid").bfloat16()
    ref = _reference(lm)
    ids, am = _prompt(SEED + 1, batch=70)
    out, steps = _runner(lm.cuda()).generate(input_ids=ids.cuda(), attention_mask=am.cuda(), max_new_tokens=n_new, return_step_logits=True)
    assert out.shape == (70, 1 + n_new)
    want = _reference_steps(ref, out, n_new, rows=rows, input_ids=ids, attention_mask=am)
    err = rel_err(steps[rows].float().cpu(), want)
    print(f"70 rows bf16: step logits of rows {rows} rel err {err:.3e}")
    assert err <= BF16_LOGITS_TOL, err
    assert torch.equal(out[:, 1:].cpu(), steps.float().argmax(-1).cpu())


def test_cache_buffers_have_max_new_tokens_columns(small, monkeypatch):
    from mmgl_amd.model import decode_cache
    made = []

    class Recording(decode_cache.DecodeCache):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(decode_cache, "DecodeCache", Recording)
    n_new = 5
    out = small["run"].generate(input_ids=small["ids"].cuda(), attention_mask=small["am"].cuda(), max_new_tokens=n_new)
    assert len(made) == 1 and torch.equal(out, small["out"][:, :1 + n_new])
    cache, inner = made[0], 2 * 64
    assert len(cache.kv) == 2 and all(tuple(kv.shape) == (B, n_new, 2 * inner) for kv in cache.kv)
    assert cache.col == n_new and tuple(cache.rel_bias.shape) == (2, n_new) and cache.rel_bias.dtype == torch.float32
    assert len(cache.cross) == 2
    for k, v in cache.cross:                                    # the two slabs of one [B, S_enc, 2 inner] buffer
        assert tuple(k.shape) == tuple(v.shape) == (B, T, inner) and k.stride() == v.stride() == (T * 2 * inner, 2 * inner, 1)
        assert v.data_ptr() - k.data_ptr() == inner * k.element_size()
    assert torch.equal(cache.cross_valid.cpu().bool(), small["am"].bool())


def test_eos_rows_are_padded(small):
    free = small["out"].cpu()
    eos = int(free[0, 1 + 2])                                   # the plain run emits it in row 0 at step 2 at the latest
    out = small["run"].generate(input_ids=small["ids"].cuda(), attention_mask=small["am"].cuda(), max_new_tokens=N_NEW, eos_token_id=eos).cpu()
    hit = 0
    for b in range(B):
        new, ref = out[b, 1:], free[b, 1:]
        pos = (ref == eos).nonzero()
        if len(pos) == 0:
            assert torch.equal(new, ref), b                     # the other rows are unaffected
            continue
        p = int(pos[0])
        hit += 1
        assert torch.equal(new[:p + 1], ref[:p + 1]) and (new[p + 1:] == 0).all(), (b, new.tolist(), ref.tolist())   # pad_token_id from the config
    assert hit >= 1


def test_sampled_run_replays_on_the_returned_step_logits(small):
    from mmgl_amd import ops
    from test_sample_kernels_gpu import _check
    knobs = dict(temperature=0.8, top_k=20, top_p=0.9)
    u = torch.rand(N_NEW, B, generator=torch.Generator().manual_seed(2)).cuda()
    ids, am = small["ids"], small["am"]
    out, steps = small["run"].generate(input_ids=ids.cuda(), attention_mask=am.cuda(), max_new_tokens=N_NEW, return_step_logits=True,
                                       do_sample=True, sample_u=u, **knobs)
    assert out.shape == (B, 1 + N_NEW) and not torch.equal(out, small["out"]), "the sampled run is the greedy run: the case shows nothing"
    for s in range(N_NEW):
        lg, us = steps[:, s].contiguous(), u[s].view(-1, 1)
        tok, kept = ops.sample_tokens(lg, us, return_kept=True, **knobs)
        assert torch.equal(tok, out[:, 1 + s]), f"step {s}: the ids are not what ops.sample_tokens draws from the returned step logits"
        _check(lg.cpu(), us.cpu(), knobs["temperature"], knobs["top_k"], knobs["top_p"], tok.tolist(), kept.tolist())
    err = rel_err(steps.float().cpu(), _reference_steps(small["ref"], out, N_NEW, input_ids=ids, attention_mask=am))
    assert err <= TAU[torch.float32], err
    assert torch.equal(small["run"].generate(input_ids=ids.cuda(), attention_mask=am.cuda(), max_new_tokens=N_NEW, do_sample=True, sample_u=u,
                                             **knobs), out)


def test_processors_see_the_decoder_row_with_its_start_token(small):
    """repetition_penalty 1.3, no_repeat_ngram_size 2 against transformers' chain on the uncached reference's logits; the history is the
    decoder row so far, start token included (transformers' processors see decoder_input_ids of an encoder-decoder).  The rule and the
    bound are tests/test_generate_processors_gpu.py's."""
    from test_generate_processors_gpu import _compare as compare_processed
    from test_generate_processors_gpu import _no_repeated_ngram
    setting = (1.3, 2, 0, ())
    ids, am = small["ids"], small["am"]
    out, steps = small["run"].generate(input_ids=ids.cuda(), attention_mask=am.cuda(), max_new_tokens=N_NEW, return_step_logits=True,
                                       repetition_penalty=1.3, no_repeat_ngram_size=2)
    assert not torch.equal(out, small["out"]), "the processors left the greedy run as it was"
    raw = _reference_steps(small["ref"], out, N_NEW, input_ids=ids, attention_mask=am)
    start = torch.ones(B, 1, dtype=torch.long)                  # the one column in front of the new tokens: always history
    compare_processed(steps, out.cpu(), start, raw, setting, TAU[torch.float32], LOW_MARGIN_SHARE[torch.float32], "T5 small fp32 processors")
    _no_repeated_ngram(out.cpu(), start, 2, N_NEW)


# ------------------------------------------------------------------------------------------ the wrapper and the trainer
def _wrapper(seed=SEED, **kw):
    from mmgl_amd.model import SelfAttentionModel
    torch.manual_seed(seed)
    args = mpt_args(model_name_or_path="t5-tiny", decoder_only=False, peft_type="none", **kw)
    w = SelfAttentionModel(args, None, lm_config=_cfg("small"), text_config=tiny_roberta_config(), visual_config=tiny_clip_vision_config())
    _randomise(w.lm, seed)
    return w.eval()


def test_wrapper_generates_from_its_own_lm_inputs():
    """Embedding mode, context `all`: text and image neighbor tokens behind the prompt's embeddings, one sample without a neighbor."""
    from test_generate_gpu import _neighbors
    w = _wrapper(neighbor_mode="embedding", context="all").cuda()
    assert w.can_generate_seq2seq() and not w.can_generate()
    ids, am = _prompt(SEED)
    nb = {k: v.cuda() for k, v in _neighbors(SEED + 100).items()}
    out, steps = w.generate(ids.cuda(), am.cuda(), **nb, max_new_tokens=N_NEW, return_step_logits=True)
    assert out.shape == (B, 1 + N_NEW) and out.dtype == torch.int64 and bool((out[:, 0] == 0).all())
    with torch.no_grad():
        lm_in, lm_mask = w._lm_inputs(ids.cuda(), am.cuda(), **nb)
    S = (3 + 2) * 2
    assert lm_in.shape == (B, T + S, 128) and lm_mask.shape == (B, T + S) and not bool(lm_mask[5, T:].any())
    want, want_steps = _runner(w.lm).generate(inputs_embeds=lm_in, attention_mask=lm_mask, max_new_tokens=N_NEW, return_step_logits=True)
    assert torch.equal(out, want) and torch.equal(steps, want_steps)
    ref = _reference_steps(_reference(w.lm), out, N_NEW, inputs_embeds=lm_in, attention_mask=lm_mask)
    _compare(steps, out, ref, torch.float32, "wrapper, embedding mode")
    # the neighbors reach the output: without them the step logits move
    _, plain = _runner(w.lm).generate(inputs_embeds=lm_in[:, :T], attention_mask=lm_mask[:, :T], max_new_tokens=N_NEW, return_step_logits=True)
    assert rel_err(plain[:, 0], steps[:, 0]) > 10 * TAU[torch.float32]


def _trainer(tmp_path, **kw):
    from torch.utils.data import DataLoader, Subset
    from mmgl_amd.language_modelling.run_generation import Arguments, build_datasets
    from mmgl_amd.model import SelfAttentionModel
    from mmgl_amd.wikiweb2m.synthetic import synthetic_tokenizer
    torch.manual_seed(0)
    tokenizer = synthetic_tokenizer()
    args = Arguments(model_name_or_path="t5-tiny", dataset="synthetic", context="section_only", neighbor_mode="raw", peft_type="none",
                     max_input_length=32, max_output_length=12, per_device_val_batch_size=4, dataloader_num_workers=0, val_steps_per_epoch=2,
                     print_freq=100, log_dir=str(tmp_path), seed=0, **kw)
    args.decoder_only = False
    txt, vis = tiny_roberta_config(), tiny_clip_vision_config()
    txt.vocab_size = len(tokenizer)
    lm_cfg = T5Config(vocab_size=len(tokenizer), dropout_rate=0.0, decoder_start_token_id=1, pad_token_id=1, eos_token_id=2, num_layers=2,
                      num_decoder_layers=2, **SIZES["small"])
    model = SelfAttentionModel(args, tokenizer, lm_config=lm_cfg, text_config=txt, visual_config=vis).float().cuda().eval()
    _, val_ds, _ = build_datasets(args, tokenizer)
    loader = DataLoader(Subset(val_ds, list(range(8))), batch_size=4, shuffle=False, num_workers=0, drop_last=True)
    return args, model, tokenizer, loader


@pytest.mark.parametrize("flag", [True, False], ids=["generate_seq2seq", "default"])
def test_evaluate_loop_generates_only_with_the_flag(flag, tmp_path):
    from mmgl_amd.language_modelling.run_generation import evaluate_loop
    args, model, tokenizer, loader = _trainer(tmp_path, **(dict(generate_seq2seq=True) if flag else {}))
    assert model.can_generate_seq2seq() and not model.can_generate()
    calls, real = [], model.generate

    def recording(**kw):
        calls.append(kw)
        out = real(**kw)
        assert out.shape == (kw["input_ids"].shape[0], 1 + 32) and bool((out[:, 0] == 1).all())
        return out
    model.generate = recording
    try:
        bleu4 = evaluate_loop(loader, model, tokenizer, 0, args, prefix="test")
        if flag:
            assert len(calls) >= 1 and all(c["max_new_tokens"] == 32 and "attention_mask" in c for c in calls), calls
        else:
            assert calls == []
        assert all(torch.isfinite(torch.tensor(float(v))) for v in evaluate_loop.last.values()) and bleu4 >= 0.0
        n = len(calls)
        evaluate_loop(loader, model, tokenizer, 0, args, prefix="val")      # only the test protocol generates
        assert len(calls) == n
    finally:
        del model.generate
