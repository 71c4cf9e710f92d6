"""CPU tests of prompt-lookup decoding: the reference rules of tests/lookup_ref.py on hand-written cases, the ValueErrors of the new
generate() keywords (they come before the device check), and the refusals of ops.attn_decode_block / ops.lookup_accept and of their
C entry points (arguments are rejected before any launch: safe without a GPU)."""
import pytest
import torch

from helpers import mpt_args, tiny_opt_config
from lookup_ref import accept, draft, emitted_matrix, lookup_accept_ref, simulate


# ------------------------------------------------------------------------------------------ the draft rule
def test_draft_no_match():
    assert draft([5, 6, 7, 8], 3, 2) == []
    assert draft([5], 3, 2) == [] and draft([], 3, 2) == []


def test_draft_bigram_preferred_over_unigram():
    # (7, 8) occurred at p = 1 -> [20, 21]; the later single 8 at p = 5 (-> 30) only counts for n = 1
    hist = [1, 7, 8, 20, 21, 8, 30, 7, 8]
    assert draft(hist, 2, 2) == [20, 21]
    assert draft(hist, 2, 1) == [30, 7]


def test_draft_latest_occurrence_wins():
    hist = [7, 8, 10, 7, 8, 11, 7, 8]
    assert draft(hist, 1, 2) == [11]
    assert draft(hist, 3, 2) == [11, 7, 8]


def test_draft_cut_at_the_history_end_and_at_least_one():
    assert draft([3, 4, 3], 7, 2) == [4, 3]                  # n = 1 (len - 1 = 2 bounds n; the bigram has no earlier start)
    assert draft([9, 9], 7, 4) == [9]                        # p = len - n - 1: the match may end right in front of the pattern
    assert draft([4, 5, 6, 4, 5], 7, 4) == [6, 4, 5]


def test_draft_longer_ngrams_first():
    hist = [1, 2, 3, 4, 50, 2, 3, 4, 60, 3, 4, 70, 1, 2, 3, 4]
    assert draft(hist, 1, 4) == [50] and draft(hist, 1, 3) == [60] and draft(hist, 1, 2) == [70]


# ------------------------------------------------------------------------------------------ the accept rule
def test_accept_prefix_rule():
    assert accept([10, 11, 12, 13], [10, 11, 12], 1, 16) == ([10, 11, 12, 13], False)           # full accept: K + 1 tokens
    assert accept([10, 11, 12, 13], [10, 99, 12], 1, 16) == ([10, 11], False)                   # partial
    assert accept([10, 11, 12, 13], [99, 11, 12], 1, 16) == ([10], False)                       # rejected
    assert accept([10, 11, 12, 13], [], 1, 16) == ([10], False)                                 # no drafts
    assert accept([10, 11, 12, 13], [10], 1, 16) == ([10, 11], False)                           # filler behind nd is never accepted


def test_accept_eos_inside_a_block_and_row_full():
    assert accept([10, 2, 12, 13], [10, 2, 12], 1, 16, eos=2) == ([10, 2], True)
    assert accept([10, 11, 12, 13], [10, 11, 12], 13, 16) == ([10, 11, 12], True)               # n_new reached inside the block
    assert accept([10, 11, 12, 13], [10, 11, 12], 15, 16) == ([10], True)


def _state(B, K, T, n_new, prompt, mask, gen, new=None, block=None, nd=None, fin=None):
    ids = torch.full((B, T + n_new), -7, dtype=torch.int64)
    ids[:, :T] = torch.tensor(prompt)
    for b in range(B):
        if new is not None:
            ids[b, T:T + len(new[b])] = torch.tensor(new[b], dtype=torch.int64)
    return dict(ids=ids, prompt_mask=torch.tensor(mask, dtype=torch.uint8), gen=torch.tensor(gen, dtype=torch.int32),
                lens=torch.tensor([T + max(g - 1, 0) for g in gen], dtype=torch.int32),
                finished=torch.tensor(fin or [0] * B, dtype=torch.uint8),
                block=torch.tensor(block or [[0] * (K + 1)] * B, dtype=torch.int64), n_draft=torch.tensor(nd or [0] * B, dtype=torch.int32))


def _logits(rows, V=32):
    """One row per entry: the entry is the argmax."""
    x = torch.arange(V, dtype=torch.float32).repeat(len(rows), 1) * 0.01
    for r, a in enumerate(rows):
        x[r, a] = 5.0
    return x


def test_reference_call_prefill_row_masked_prompt_columns_skipped():
    # row 0: the hole at column 2 makes (7, 8) adjacent in the history; row 1: right padding is no history
    st = _state(2, 3, 6, 4, [[7, 8, 9, 20, 21, 7], [7, 8, 7, 1, 1, 1]], [[1, 1, 0, 1, 1, 1], [1, 1, 1, 0, 0, 0]], [0, 0])
    out = lookup_accept_ref(_logits([8, 8]), 1, **st, n_new=4, N=2, pos_offset=2, pos_max=65)
    assert out["emitted"].tolist() == [1, 1] and out["gen"].tolist() == [1, 1] and out["lens"].tolist() == [6, 6]
    assert out["ids"][:, 6].tolist() == [8, 8]
    assert out["block"].tolist() == [[8, 20, 21, 7], [8, 7, 8, 8]] and out["n_draft"].tolist() == [3, 2]
    assert out["positions"].tolist() == [[7, 8, 9, 10], [5, 6, 7, 8]]           # valid prompt tokens + 2 + gen - 1 + i


def test_reference_call_eos_pads_at_once_and_positions_clamp():
    st = _state(2, 3, 4, 6, [[3, 4, 5, 6]] * 2, [[1] * 4] * 2, [2, 5], new=[[10, 11], [10, 11, 12, 13, 14]],
                block=[[11, 12, 13, 14], [14, 15, 16, 17]], nd=[3, 3])
    out = lookup_accept_ref(_logits([12, 2, 14, 15, 15, 16, 17, 18]), 4, **st, n_new=6, N=2, eos=2, pad=1, pos_offset=2, pos_max=10)
    assert out["emitted"].tolist() == [2, 1]                                   # row 0: EOS as the second token; row 1: full at n_new
    assert out["ids"][0, 4:].tolist() == [10, 11, 12, 2, 1, 1] and out["gen"].tolist() == [6, 6] and out["finished"].tolist() == [1, 1]
    assert out["lens"].tolist() == [7, 9]                                       # len grows by the tokens emitted, never by the pads
    assert out["n_draft"].tolist() == [0, 0] and out["block"].tolist() == [[2] * 4, [15] * 4]
    assert out["positions"][0].tolist() == [10, 10, 10, 10]                    # 4 + 2 + 6 - 1 = 11 and beyond: clamped to the table
    again = lookup_accept_ref(_logits([12, 2, 14, 15, 15, 16, 17, 18]), 4, out["block"], out["n_draft"], out["ids"], st["prompt_mask"],
                              out["gen"], out["lens"], out["finished"], n_new=6, N=2, eos=2, pad=1, pos_offset=2, pos_max=10)
    for key in ("block", "n_draft", "positions", "ids", "gen", "lens", "finished"):          # a finished row is frozen
        assert torch.equal(again[key], out[key]), key
    assert again["emitted"].tolist() == [0, 0]


def test_simulated_trace():
    prompt = [50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 50]
    new = list(range(51, 67))
    tr = simulate(prompt, new, 7, 2)
    # call 1 verifies 52 .. 58 (all accepted); call 2 drafts [60, 50, 51, ...] behind (58, 59): 60 holds, 50 is not 61
    assert [c["k"] for c in tr] == [1, 8, 2, 1, 1, 1, 1, 1] and [c["nd"] for c in tr] == [0, 7, 7, 0, 0, 0, 0, 0]
    assert sum(c["k"] for c in tr) == 16
    tr = simulate(prompt, new[:5] + [1] * 11, 3, 2, eos=55)
    assert [c["k"] for c in tr] == [1, 4] and tr[1]["eos_at"] == 3
    other = simulate(prompt, new, 3, 2)
    em = emitted_matrix([tr, other], len(other) - 1)                            # a finished row emits 0 while the others run on
    assert em[:, 0].tolist() == [1, 4] + [0] * (len(other) - 2) and em[:, 1].tolist() == [c["k"] for c in other]


# ------------------------------------------------------------------------------------------ generate()'s keywords, on CPU tensors
def _lm():
    from mmgl_amd.model.modelling_cross_attention import MPTConfig, MPTForCausalLM
    torch.manual_seed(0)
    return MPTForCausalLM(MPTConfig(mpt_args(neighbor_mode="raw", peft_type="none"), tiny_opt_config(dropout=0.0))).eval()


@pytest.mark.parametrize("kw,match", [
    (dict(prompt_lookup_num_tokens=8), "prompt_lookup_num_tokens"),
    (dict(prompt_lookup_num_tokens=-1), "prompt_lookup_num_tokens"),
    (dict(prompt_lookup_num_tokens=3, max_matching_ngram_size=0), "max_matching_ngram_size"),
    (dict(prompt_lookup_num_tokens=3, max_matching_ngram_size=5), "max_matching_ngram_size"),
    (dict(prompt_lookup_num_tokens=3, do_sample=True), "do_sample"),
    (dict(prompt_lookup_num_tokens=3, num_beams=2), "num_beams"),
    (dict(prompt_lookup_num_tokens=3, do_sample=True, num_return_sequences=2), "prompt_lookup_num_tokens"),
    (dict(prompt_lookup_num_tokens=3, repetition_penalty=1.2), "repetition_penalty"),
    (dict(prompt_lookup_num_tokens=3, no_repeat_ngram_size=2), "no_repeat_ngram_size"),
    (dict(prompt_lookup_num_tokens=3, suppress_tokens=[5]), "suppress_tokens"),
    (dict(prompt_lookup_num_tokens=3, return_step_logits=True), "return_step_logits"),
    (dict(return_lookup_stats=True), "return_lookup_stats"),
])
def test_generate_keyword_refusals_come_before_the_device_check(kw, match):
    lm = _lm()
    ids = torch.randint(3, 128, (2, 6))
    with pytest.raises(ValueError, match=match):
        lm.generate(ids, torch.ones_like(ids), max_new_tokens=4, **kw)


def test_generate_refuses_embeds_prompts_and_then_the_cpu():
    lm = _lm()
    with pytest.raises(ValueError, match="inputs_embeds"):
        lm.generate(inputs_embeds=torch.randn(2, 6, 64), max_new_tokens=4, prompt_lookup_num_tokens=3)
    ids = torch.randint(3, 128, (2, 6))
    with pytest.raises(RuntimeError, match="no CPU path"):                      # valid keywords reach the device check
        lm.generate(ids, torch.ones_like(ids), max_new_tokens=4, prompt_lookup_num_tokens=3, return_lookup_stats=True)


def test_generate_refuses_adapted_projections_before_any_work():
    """With the other refusals, on CPU tensors; K = 0 with the same module gets as far as the device check."""
    import torch.nn as nn

    class Adapted(nn.Linear):                                  # stands for any adapted projection: not a plain nn.Linear
        pass
    lm = _lm()
    lm.model.decoder.layers[2].self_attn.v_proj = Adapted(64, 64)
    ids = torch.randint(3, 128, (2, 6))
    with pytest.raises(ValueError, match="plain nn.Linear"):
        lm.generate(ids, torch.ones_like(ids), max_new_tokens=4, prompt_lookup_num_tokens=3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        lm.generate(ids, torch.ones_like(ids), max_new_tokens=4)


def test_evaluate_loop_leaves_the_keyword_out_for_adapted_models():
    import torch.nn as nn
    from mmgl_amd.language_modelling.run_generation import _plain_projections
    lm = _lm()
    assert _plain_projections(lm)
    lm.model.decoder.layers[0].self_attn.q_proj.lora_A = nn.Parameter(torch.zeros(4, 64))
    assert not _plain_projections(lm)


def test_wrapper_passes_the_keywords_and_other_generators_lack_them():
    import inspect
    from mmgl_amd.model import CrossAttentionModel
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    from mmgl_amd.model.modelling_self_attention import SelfAttentionModel
    from mmgl_amd.language_modelling.run_generation import Arguments
    names = ("prompt_lookup_num_tokens", "max_matching_ngram_size", "return_lookup_stats")
    sig = inspect.signature(CrossAttentionModel.generate).parameters
    assert [sig[n].default for n in names] == [0, 2, False]
    for other in (SelfAttentionModel, LlamaNeighborLM):
        assert not set(names) & set(inspect.signature(other.generate).parameters)
    a = Arguments()
    assert a.prompt_lookup_num_tokens == 0 and a.max_matching_ngram_size == 2


# ------------------------------------------------------------------------------------------ the ops and their entry points
def test_ops_have_no_cpu_path():
    from mmgl_amd import ops
    q, kv = torch.zeros(4, 64), torch.zeros(2, 9, 128)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.attn_decode_block(q, q, q, kv[:, :, :64], kv[:, :, 64:], torch.ones(2, 9, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32), 4, 2)
    i32 = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lookup_accept(torch.zeros(2, 32), 1, torch.zeros(2, 4, dtype=torch.int64), i32, torch.zeros(2, 4, dtype=torch.int64),
                          torch.zeros(2, 10, dtype=torch.int64), torch.ones(2, 6, dtype=torch.uint8), i32, i32, torch.zeros(2, dtype=torch.uint8),
                          i32, 4, 2)


def test_entry_points_refuse_before_any_launch():
    import ctypes
    from mmgl_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(256)              # a non-null, 16-byte aligned address that no refused call dereferences
    blk = lambda **kw: L.mmgl_attn_decode_block_fwd(*[{**dict(q=p, ldq=256, kn=p, vn=p, ld_new=512, k=p, v=p, ldkv=512, bs=512 * 40, cap=40,
                                                              valid=p, ld_valid=40, len=p, out=p, B=2, m=4, H=4, D=64, dtype=1, st=None), **kw}[n]
                                                      for n in ("q", "ldq", "kn", "vn", "ld_new", "k", "v", "ldkv", "bs", "cap", "valid", "ld_valid",
                                                                "len", "out", "B", "m", "H", "D", "dtype", "st")])
    assert blk(m=9) == 2 and b"new tokens" in L.mmgl_last_error()
    assert blk(m=0) == 1 and blk(cap=0) == 1 and blk(B=0) == 1
    assert blk(D=48) == 2 and blk(dtype=7) == 1
    assert blk(len=None) == 1 and blk(kn=None) == 1 and blk(q=None) == 1
    assert blk(ld_new=260) == 2 and blk(ldkv=260) == 2 and blk(kn=ctypes.c_void_p(264)) == 2
    assert blk(ld_new=128) == 1 and blk(bs=512) == 1 and blk(ld_valid=8) == 1
    acc = lambda **kw: L.mmgl_lookup_accept(*[{**dict(logits=p, ld=128, m_in=4, block=p, nd=p, pos=p, ids=p, ld_ids=40, mask=p, ld_mask=8, gen=p,
                                                      len=p, fin=p, emitted=p, B=2, T=8, n_new=32, V=128, K=3, N=2, eos=2, pad=1, off=2, pmax=65,
                                                      dtype=0, st=None), **kw}[n]
                                              for n in ("logits", "ld", "m_in", "block", "nd", "pos", "ids", "ld_ids", "mask", "ld_mask", "gen", "len",
                                                        "fin", "emitted", "B", "T", "n_new", "V", "K", "N", "eos", "pad", "off", "pmax", "dtype", "st")])
    assert acc(K=8, m_in=9) == 2 and acc(K=0, m_in=1) == 2 and acc(N=5) == 2 and acc(N=0) == 2
    assert acc(m_in=2) == 1 and b"m_in" in L.mmgl_last_error()
    assert acc(T=8161, ld_ids=9000, ld_mask=9000) == 2 and b"8192" in L.mmgl_last_error()       # the LDS history: T + n_new <= 8192
    assert acc(T=2048, ld_ids=2080, ld_mask=2048, gen=None) == 1                                 # 2048 + 32 fits; the null pointer is next
    assert acc(ld=100) == 1 and acc(ld_ids=39) == 1 and acc(ld_mask=7) == 1
    assert acc(pad=128) == 1 and acc(eos=-1, pad=128, logits=None) == 1 and acc(dtype=3) == 1 and acc(B=0) == 1
