"""CPU tests of prompt-lookup decoding on the Llama-family LM (no compute: there is no GPU here).
LlamaNeighborLM.generate takes the prompt-lookup keywords of MPTForCausalLM.generate and refuses what sampling.check_lookup refuses, with
its messages, before any device work: the prompts below are CPU tensors, so a call that got past the keyword checks would end in the
RuntimeError of generation.check_prompt ("no CPU path") instead.  The two entry points of the verify step are declared, exported and
bound, and validate their arguments before any launch."""
import pytest
import torch

from test_generate_llama_cpu import _tiny_lm


@pytest.fixture(scope="module")
def lm():
    return _tiny_lm().eval()


def _call(lm, **kw):
    ids = torch.randint(3, 128, (2, 6))
    return lm.generate(ids, torch.ones_like(ids), max_new_tokens=4, **kw)


@pytest.mark.parametrize("kw,message", [
    (dict(prompt_lookup_num_tokens=8), r"prompt_lookup_num_tokens = 8 \(0: off, 1\.\.7\)"),
    (dict(prompt_lookup_num_tokens=-1), r"prompt_lookup_num_tokens = -1 \(0: off, 1\.\.7\)"),
    (dict(prompt_lookup_num_tokens=3, max_matching_ngram_size=0), r"max_matching_ngram_size = 0 \(1\.\.4\)"),
    (dict(prompt_lookup_num_tokens=3, max_matching_ngram_size=5), r"max_matching_ngram_size = 5 \(1\.\.4\)"),
    (dict(prompt_lookup_num_tokens=3, do_sample=True), r"prompt_lookup_num_tokens = 3 with do_sample=True is not implemented"),
    (dict(prompt_lookup_num_tokens=3, do_sample=True, num_return_sequences=2), r"prompt_lookup_num_tokens = 3 with do_sample=True"),
    (dict(prompt_lookup_num_tokens=3, repetition_penalty=1.3), r"prompt_lookup_num_tokens = 3 is not implemented with repetition_penalty"),
    (dict(prompt_lookup_num_tokens=3, no_repeat_ngram_size=2), r"prompt_lookup_num_tokens = 3 is not implemented with repetition_penalty"),
    (dict(prompt_lookup_num_tokens=3, suppress_tokens=[5]), r"prompt_lookup_num_tokens = 3 is not implemented with repetition_penalty"),
    (dict(prompt_lookup_num_tokens=3, return_step_logits=True), r"prompt_lookup_num_tokens = 3 has no per-step logits"),
    (dict(prompt_lookup_num_tokens=3, num_return_sequences=2), r"prompt_lookup_num_tokens = 3 with num_beams = 1 / num_return_sequences = 2"),
    (dict(return_lookup_stats=True), r"return_lookup_stats belongs to prompt_lookup_num_tokens > 0"),
    (dict(prompt_lookup_num_tokens=0, return_lookup_stats=True), r"return_lookup_stats belongs to prompt_lookup_num_tokens > 0"),
], ids=lambda v: None if isinstance(v, str) else "-".join(f"{k}={x}" for k, x in v.items()))
def test_refusals_carry_check_lookups_message(lm, kw, message):
    with pytest.raises(ValueError, match=r"LlamaNeighborLM\.generate\(\): " + message):
        _call(lm, **kw)


def test_accepted_keywords_reach_the_prompt_check(lm):
    """K = 0 with the keywords is today's call, and K in 1..7 with N in 1..4 passes every keyword check: both end at the device check."""
    for kw in (dict(), dict(prompt_lookup_num_tokens=0, max_matching_ngram_size=2), dict(prompt_lookup_num_tokens=1, max_matching_ngram_size=1),
               dict(prompt_lookup_num_tokens=7, max_matching_ngram_size=4, return_lookup_stats=True)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            _call(lm, **kw)
    with pytest.raises(ValueError, match="num_beams = 2 is not implemented"):          # beam search stays refused, with or without K
        _call(lm, prompt_lookup_num_tokens=3, num_beams=2)
    with pytest.raises(TypeError, match="unexpected keyword argument 'prompt_lookup'"):   # the three names and no other
        _call(lm, prompt_lookup=3)


def test_lookup_state_can_skip_the_projection_scratch():
    """LlamaNeighborLM files a block's keys from its fused q|k|v rows and needs no [B*W, 2d] scratch per layer; the OPT path gets its own."""
    from mmgl_amd.model.modelling_cross_attention import DecodeCache, LookupState
    cache = DecodeCache(3, 2, 9, 16, torch.float32, "cpu")
    cache.col = 5
    own = LookupState(cache, 3, 2, 4)
    assert len(own.scratch) == 3 and all(s.shape == (2 * 4, 32) for s in own.scratch)
    cache.mask[:, 5:] = 0
    bare = LookupState(cache, 3, 2, 4, scratch=False)
    assert bare.scratch is None and bare.W == 4 and bare.len.tolist() == [5, 5] and bare.block.shape == (2, 4)
    assert bare.emitted.shape == (4, 2) and (cache.mask[:, 5:] == 1).all() and not cache.mask[:, :5].any()


def test_verify_step_needs_a_lookup_state(lm):
    from mmgl_amd.model.modelling_cross_attention import DecodeCache
    with pytest.raises(ValueError, match="LookupState"):
        lm._verify_step(DecodeCache(4, 2, 8, 2 * 16, torch.float32, "cpu"))


def test_block_symbols_are_bound():
    import os
    from mmgl_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 110 and L.mmgl_version() == _lib.ABI_VERSION
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "mmgl_hip.h")).read()
    for name in ("mmgl_rope_kv_append_block", "mmgl_attn_decode_gqa_block_fwd"):
        assert name in _lib.SIGNATURES and hasattr(L, name) and f"int {name}(" in header


def test_block_argument_validation():
    from mmgl_amd import _lib
    L = _lib.lib()
    err = lambda: L.mmgl_last_error()
    # mmgl_rope_kv_append_block(qkv, ldqkv, cos_sin, n_pos, kv, ldkv, batch_stride_kv, capacity, len, B, m, H, Hkv, D, dtype, stream)
    rope = lambda ldqkv=512, n_pos=32, ldkv=256, bs=2560, cap=10, B=2, m=4, H=4, Hkv=2, D=64, dtype=1: L.mmgl_rope_kv_append_block(
        None, ldqkv, None, n_pos, None, ldkv, bs, cap, None, B, m, H, Hkv, D, dtype, None)
    assert rope() == 1 and b"null" in err()
    assert rope(m=9) == 2 and b"1..8" in err()
    assert rope(m=0) == 1 and rope(B=0) == 1 and rope(cap=0) == 1 and rope(n_pos=0) == 1 and rope(Hkv=0) == 1
    assert rope(Hkv=3) == 1 and b"multiple" in err()
    assert rope(ldqkv=384, D=48) == 2 and b"head_dim" in err()
    assert rope(ldqkv=516) == 2 and rope(bs=2564) == 2                                  # rows not 16-byte multiples
    assert rope(dtype=7) == 1
    # mmgl_attn_decode_gqa_block_fwd(q, ldq, k, v, ldkv, batch_stride_kv, capacity, key_valid, ld_valid, len, out, B, m, H, Hkv, D, dtype, stream)
    attn = lambda ldq=512, ldkv=256, bs=2560, cap=10, ldv=10, B=2, m=4, H=4, Hkv=2, D=64, dtype=1: L.mmgl_attn_decode_gqa_block_fwd(
        None, ldq, None, None, ldkv, bs, cap, None, ldv, None, None, B, m, H, Hkv, D, dtype, None)
    assert attn() == 1 and b"null" in err()
    assert attn(m=9) == 2 and b"1..8" in err()
    assert attn(m=0) == 1 and attn(B=0) == 1 and attn(cap=0) == 1 and attn(Hkv=0) == 1
    assert attn(Hkv=3) == 1 and b"multiple" in err()
    assert attn(ldq=192, ldkv=192, bs=1920, D=48) == 2 and b"head_dim" in err()
    assert attn(ldkv=260, bs=2600) == 2                                                 # rows not 16-byte multiples
    assert attn(dtype=7) == 1


def test_block_ops_have_no_cpu_path():
    from mmgl_amd import ops
    lens = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rope_kv_append_block(torch.randn(4, 128), torch.zeros(8, 8, 2), torch.zeros(2, 5, 64), lens, 4, 2, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.attn_decode_gqa_block(torch.randn(4, 64), torch.randn(2, 5, 32), torch.randn(2, 5, 32), torch.ones(2, 5, dtype=torch.bool), lens, 4, 2, 2)
