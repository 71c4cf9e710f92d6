"""CPU tests of the decode-mode dispatch of DecodeCache (mmgl_amd/model/decode_cache.py; no compute: there is no GPU here).
new_kv / file_rotated / attend_self / attend_cross are the one place that knows the modes of a decode step: plain, FP8, beam, verify
with and without scratch.  The attention and filing ops are replaced by recorders; for every mode the test pins which op is called,
exactly once, that each tensor argument is the expected view of the cache (same data_ptr, shape and strides) and where new_kv points.
The two FP8 refusals fire before any op is reached."""
import pytest
import torch

from mmgl_amd import ops
from mmgl_amd.model.decode_cache import BeamState, DecodeCache, LookupState

B, CAP, T, D_MODEL, H, HKV, W, N_CAP, K = 2, 5, 3, 32, 2, 1, 2, 2, 1
HEAD = D_MODEL // H
N_GQA = HKV * HEAD                                              # key width of the grouped-query rows
OPS = ("attn_decode", "attn_decode_q8", "attn_decode_beam", "attn_decode_block", "attn_decode_gqa_block", "rope_kv_append", "rope_kv_append_block")


@pytest.fixture
def calls(monkeypatch):
    """Every attention / filing op the dispatch may reach, replaced by a recorder; the list of (name, args, kwargs) it saw."""
    seen = []

    def recorder(name):
        def op(*args, **kwargs):
            seen.append((name, args, kwargs))
            return args[0] if name.startswith("rope") else ("out of", name)
        return op
    for name in OPS:
        monkeypatch.setattr(ops, name, recorder(name))
    return seen


def _cache(n, fp8=False, heads=H):
    """A two-layer cache of key width n whose prompt of T columns is filed: what a prefill leaves."""
    c = DecodeCache(2, B, CAP, n, torch.float32, "cpu", ops.KV_FP8 if fp8 else None, heads if fp8 else None)
    c.col = T
    c.mask[:, :T] = 1
    c.next_pos = torch.full((B,), T + 2)
    c.cos_sin = torch.zeros(CAP, HEAD // 2, 2)
    return c


def _same(got, want):
    return (torch.is_tensor(got) and got.data_ptr() == want.data_ptr() and got.shape == want.shape and got.stride() == want.stride()
            and got.dtype == want.dtype)


def _check(calls, name, args, **kwargs):
    """The recorders saw exactly one call, of op `name`, with these arguments: tensors as the same views, the rest equal."""
    assert [c[0] for c in calls] == [name]
    got_args, got_kwargs = calls[0][1], calls[0][2]
    assert len(got_args) == len(args) and got_kwargs.keys() == kwargs.keys()
    pairs = list(zip(got_args, args)) + [(got_kwargs[k], kwargs[k]) for k in kwargs]
    for i, (got, want) in enumerate(pairs):
        assert _same(got, want) if torch.is_tensor(want) else (not torch.is_tensor(got) and got == want), f"{name}: argument {i}"
    calls.clear()


def test_plain(calls):
    c, n, idx = _cache(D_MODEL), D_MODEL, 1
    kv, q = c.kv[idx], torch.zeros(B, D_MODEL)
    new = c.new_kv(idx)
    assert _same(new, kv[:, T]) and c.plain and not calls
    assert c.attend_self(idx, q, new, H) == ("out of", "attn_decode")
    _check(calls, "attn_decode", (q, kv[:, :T + 1, :n], kv[:, :T + 1, n:], c.mask[:, :T + 1], H), num_kv_heads=None)


def test_plain_grouped_query(calls):
    c, n, idx = _cache(N_GQA), N_GQA, 0
    kv, qkv = c.kv[idx], torch.zeros(B, (H + 2 * HKV) * HEAD)
    new = c.file_rotated(idx, qkv, H, HKV)
    assert _same(new, kv[:, T]) and _same(new, c.new_kv(idx))
    _check(calls, "rope_kv_append", (qkv, c.cos_sin[T], kv[:, T], H, HKV))
    c.attend_self(idx, qkv[:, :D_MODEL], new, H, HKV)
    _check(calls, "attn_decode", (qkv[:, :D_MODEL], kv[:, :T + 1, :n], kv[:, :T + 1, n:], c.mask[:, :T + 1], H), num_kv_heads=HKV)


def test_fp8(calls):
    c, n, idx = _cache(D_MODEL, fp8=True), D_MODEL, 1
    q = torch.zeros(B, D_MODEL)
    new = c.new_kv(idx)
    assert _same(new, c.kv_new) and not c.plain and not calls
    assert c.attend_self(idx, q, new, H) == ("out of", "attn_decode_q8")
    _check(calls, "attn_decode_q8", (q, c.kv_new[:, :n], c.kv_new[:, n:], c.kv[idx], c.kv_scale[idx], c.mask[:, :T], H), num_kv_heads=None)


def test_fp8_grouped_query(calls):
    c, n, idx = _cache(N_GQA, fp8=True, heads=HKV), N_GQA, 1
    qkv = torch.zeros(B, (H + 2 * HKV) * HEAD)
    new = c.file_rotated(idx, qkv, H, HKV)
    assert _same(new, c.kv_new)
    _check(calls, "rope_kv_append", (qkv, c.cos_sin[T], c.kv_new, H, HKV))
    c.attend_self(idx, qkv[:, :D_MODEL], new, H, HKV)
    _check(calls, "attn_decode_q8", (qkv[:, :D_MODEL], c.kv_new[:, :n], c.kv_new[:, n:], c.kv[idx], c.kv_scale[idx], c.mask[:, :T], H),
           num_kv_heads=HKV)


def test_beam(calls):
    c, n, idx = _cache(D_MODEL), D_MODEL, 1
    c.beam = beam = BeamState(c, W, N_CAP)
    beam.n_tail = 1                                             # the second step: one tail column is filled, this step writes the next
    kv, tail, q = c.kv[idx], beam.tail[idx], torch.zeros(B * W, D_MODEL)
    new = c.new_kv(idx)
    assert tail.shape == (B * W, N_CAP, 2 * n) and _same(new, tail[:, 1]) and not c.plain and not calls
    assert c.attend_self(idx, q, new, H) == ("out of", "attn_decode_beam")
    _check(calls, "attn_decode_beam", (q, kv[:, :T, :n], kv[:, :T, n:], c.mask[:, :T], H, W, tail[:, :2, :n], tail[:, :2, n:], beam.book.src))
    with pytest.raises(ValueError, match="no beam step"):       # the rotary filing has no tail form
        c.file_rotated(idx, torch.zeros(B * W, 2 * D_MODEL), H, HKV)
    assert not calls


def test_verify_with_scratch(calls):
    c, n, idx = _cache(D_MODEL), D_MODEL, 1
    c.lookup = lookup = LookupState(c, K, 2, 4)
    kv, q = c.kv[idx], torch.zeros(B * lookup.W, D_MODEL)
    new = c.new_kv(idx)
    assert lookup.W == K + 1 and new.shape == (B * lookup.W, 2 * n) and _same(new, lookup.scratch[idx]) and not c.plain and not calls
    assert c.attend_self(idx, q, new, H) == ("out of", "attn_decode_block")
    _check(calls, "attn_decode_block", (q, new[:, :n], new[:, n:], kv[:, :, :n], kv[:, :, n:], c.mask, lookup.len, H, lookup.W))


def test_verify_without_scratch(calls):
    c, n, idx = _cache(N_GQA), N_GQA, 1
    c.lookup = lookup = LookupState(c, K, 2, 4, scratch=False)
    kv, qkv = c.kv[idx], torch.zeros(B * lookup.W, (H + 2 * HKV) * HEAD)
    assert c.new_kv(idx) is None and not calls
    assert c.file_rotated(idx, qkv, H, HKV) is None
    _check(calls, "rope_kv_append_block", (qkv, c.cos_sin, kv, lookup.len, H, HKV, lookup.W))
    assert c.attend_self(idx, qkv[:, :D_MODEL], None, H, HKV) == ("out of", "attn_decode_gqa_block")
    _check(calls, "attn_decode_gqa_block", (qkv[:, :D_MODEL], kv[:, :, :n], kv[:, :, n:], c.mask, lookup.len, H, HKV, lookup.W))


@pytest.mark.parametrize("state", ["none", "beam", "lookup"])
def test_cross(calls, state):
    """One row per sample: ops.attn_decode.  W rows per sample (beams, or the tokens of a verify step): ops.attn_decode_beam without a
    tail -- the neighbor tokens stay at B rows."""
    c = _cache(D_MODEL)
    c.cross = [(torch.zeros(B, 4, D_MODEL), torch.zeros(B, 4, D_MODEL)) for _ in range(2)]
    c.cross_valid = torch.ones(B, 4, dtype=torch.uint8)
    if state == "beam":
        c.beam = BeamState(c, W, N_CAP)
    elif state == "lookup":
        c.lookup = LookupState(c, K, 2, 4)
    rows = 1 if state == "none" else W
    q = torch.zeros(B * rows, D_MODEL)
    k, v = c.cross[1]
    c.attend_cross(1, q, H)
    if rows == 1:
        _check(calls, "attn_decode", (q, k, v, c.cross_valid, H))
    else:
        _check(calls, "attn_decode_beam", (q, k, v, c.cross_valid, H, W))


@pytest.mark.parametrize("state,message", [("beam", "the FP8 key/value cache has no beam step"), ("lookup", "the FP8 key/value cache has no verify step")])
def test_fp8_refusals_come_before_any_op(calls, state, message):
    c = _cache(D_MODEL, fp8=True)
    if state == "beam":
        c.beam = BeamState(c, W, N_CAP)
    else:
        c.lookup = LookupState(c, K, 2, 4)
    q = torch.zeros(B * W, D_MODEL)
    for call in (lambda: c.new_kv(0), lambda: c.file_rotated(0, torch.zeros(B * W, 2 * D_MODEL), H, HKV),
                 lambda: c.attend_self(0, q, c.kv_new, H)):
        with pytest.raises(ValueError, match=message):
            call()
    assert not calls and not c.plain


def test_declared_fields_and_reexports():
    """cos_sin and cross_gu are fields of every cache (the Llama prefill fills them), and the three classes are importable from the
    OPT fork's module, where tests and tools have always found them."""
    from mmgl_amd.model import modelling_cross_attention as mca, modelling_llama_cross_attention as mlca
    c = DecodeCache(1, B, CAP, D_MODEL, torch.float32, "cpu")
    assert c.cos_sin is None and c.cross_gu == [] and c.beam is None and c.lookup is None and c.plain
    assert mca.DecodeCache is DecodeCache and mca.LookupState is LookupState and mca.BeamState is BeamState
    assert mlca.DecodeCache is DecodeCache and mlca.LookupState is LookupState
