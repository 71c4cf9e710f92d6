"""-m gpu: the packed bidirectional encoder attention mmgl_encattn_fwd (encattn_fwd_kernel of csrc/selfattn.hip, sa32_enc_fwd of
csrc/selfattn32.hip) against attn_ref.EncAttnRef -- per sequence an fp64 all-valid attention of the storage-rounded operands --
element by element, within u |want| + (c + n 2^-24 (S_i + ln len)) mag (XAttnRef's count).  tests/test_attn_general_ref_cpu.py shows
on the CPU that this comparison fails for a key leaking in from the next sequence, a dropped last key and a shifted head mapping.
The raw entry point is called (ld_out is free there); `out` holds a canary before every call.

Routes (mmgl_encattn_fwd's dispatch, restated in _route):
  R32      bf16, D 64 / 128, max_len <= 4096: sa32_enc_fwd, query blocks of 128 rows
  R16      fp32 D 16 / 32 / 64 / 128 and bf16 D 16 / 32: encattn_fwd_kernel, query blocks of 128 rows (fp32 D = 128: 64)
  R16big   bf16, D 64 / 128, max_len > 4096: encattn_fwd_kernel's bf16 D 64 / 128 instantiations

  A  lengths: one packed batch per route with sequences of 1, 15, 16, 17, 63, 64, 65, 127, 128, 129 and 257 tokens, short next to
     long; sequences x heads x blocks is no multiple of 8 (xcd_remap's remainder path)
  B  q_rows in {1, 2, 16, 17, QB - 1, QB, QB + 1, more than the longest}: rows at and past q_rows keep the canary, the written rows
     are the full call's bit for bit
  C  the dispatch edge: max_len 4096 and 4097 over the same short batch (an upper bound: it selects the route and sizes the grid,
     nothing else), and one true sequence of 4097 tokens
  D  layouts: q / k / v as column slices of one fused [ntok, 3 H D] buffer, as three buffers of a padded pitch, ld_out > H D with
     canaries in the pad columns
  E  memory: the packed buffers between NaN guards, a neighbouring sequence of NaN and of +Inf, two launches
  F  refusals: an error code and nothing written
  Z  a sequence of no tokens between two others (both kernels return before any load when a sequence has no query row): nothing
     written, the neighbours' rows bit-equal to the batch without it"""
import ctypes
import functools

import pytest
import torch

from attn_ref import EncAttnRef
from bounds import BF16, CANARY, F32, NAME, NAN, Slab

pytestmark = pytest.mark.gpu

SEED = 0
LENS = (1, 129, 15, 64, 17, 63, 16, 128, 65, 257, 127)
H = 3
R32, R16, R16BIG = "R32", "R16", "R16big"
ROUTES = ([(R32, BF16, D, 257) for D in (64, 128)] + [(R16, F32, D, 257) for D in (16, 32, 64, 128)] + [(R16, BF16, D, 257) for D in (16, 32)]
          + [(R16BIG, BF16, D, 4097) for D in (64, 128)])


def _route(dtype, D, max_len):
    """mmgl_encattn_fwd: sa32_supported(dtype, D, max_len) ? sa32_enc_fwd : encattn_fwd_kernel."""
    if dtype == BF16 and D in (64, 128):
        return R32 if max_len <= 4096 else R16BIG
    return R16


def _qb(dtype, D, max_len):
    """Query rows per workgroup: 128 for sa32; 4 * 16 * SC<T, D>::QT for the 16x16 kernel (QT = 2 while 4 (D / 16) (sizeof(T) / 2) <= 32)."""
    if _route(dtype, D, max_len) == R32:
        return 128
    return 128 if 4 * (D // 16) * (2 if dtype == F32 else 1) <= 32 else 64


def _rid(r):
    return f"{r[0]}-{NAME[r[1]]}-D{r[2]}"


@functools.lru_cache(maxsize=None)
def _batch(dtype, D, lens=LENS, heads=H):
    """(q, k, v, cu, reference) of the packed batch, built once per (dtype, D) and left unchanged."""
    q, k, v = EncAttnRef.inputs(dtype, lens, heads, D, seed=SEED, device="cuda")
    cu = EncAttnRef.cu(lens, "cuda")
    return q, k, v, cu, EncAttnRef(q, k, v, cu, heads)


def _enc(q, k, v, cu, out, nseq, heads, D, ld_in, ld_out, max_len, q_rows, dtype):
    from mmgl_amd import _lib
    p = lambda x: x if (x is None or isinstance(x, ctypes.c_void_p)) else _lib.ptr(x)
    code = dtype if isinstance(dtype, int) else _lib.dtype_code(torch.empty(0, dtype=dtype))
    _lib.call("mmgl_encattn_fwd", None, p(q), p(k), p(v), p(cu), p(out), nseq, heads, D, ld_in, ld_out, max_len, q_rows, code, _lib.stream_ptr())


def _run(dtype, D, max_len, q_rows=None, lens=LENS, heads=H, qkv=None):
    q, k, v, cu, ref = _batch(dtype, D, lens, heads)
    if qkv is not None:
        q, k, v = qkv
    so = Slab((q.shape[0], heads * D), dtype, CANARY)
    _enc(q, k, v, cu, so.v, len(lens), heads, D, q.stride(0), heads * D, max_len, max_len if q_rows is None else q_rows, dtype)
    torch.cuda.synchronize()
    return so.v, ref


# ------------------------------------------------------------------------------------------ A: lengths
def test_A_routes_and_grids():
    assert [_route(dt, D, ml) for _, dt, D, ml in ROUTES] == [r for r, *_ in ROUTES]
    assert {(dt, D) for r, dt, D, _ in ROUTES if r == R16} == {(F32, 16), (F32, 32), (F32, 64), (F32, 128), (BF16, 16), (BF16, 32)}
    assert {_qb(dt, D, ml) for r, dt, D, ml in ROUTES if r == R16} == {64, 128}
    for r, dt, D, ml in ROUTES:
        nqb = -(-ml // _qb(dt, D, ml))
        assert (len(LENS) * H * nqb) % 8, f"{_rid((r, dt, D))}: the grid is a multiple of 8"
    assert set(LENS) == {1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257}
    assert all(min(a, b) <= 17 or abs(a - b) >= 63 for a, b in zip(LENS, LENS[1:])), "short next to long"


@pytest.mark.parametrize("route", ROUTES, ids=_rid)
def test_A_lengths(route):
    r, dtype, D, max_len = route
    out, ref = _run(dtype, D, max_len)
    ref.check(out, _rid(route), f"A {r} {NAME[dtype]}")


@pytest.mark.parametrize("route", [ROUTES[0], ROUTES[3], ROUTES[6], ROUTES[8]], ids=_rid)
def test_A_ops_encoder_attention_is_the_raw_call(route):
    from mmgl_amd import ops
    r, dtype, D, max_len = route
    q, k, v, cu, ref = _batch(dtype, D)
    for q_rows in (None, 1):
        raw, _ = _run(dtype, D, max_len, q_rows)
        got = ops.encoder_attention(q, k, v, cu, H, max_len, q_rows=q_rows)
        rows = ref.rows(q_rows)
        assert torch.equal(got[rows], raw[rows]), f"q_rows={q_rows}: ops.encoder_attention is not the raw entry point's result"


# ------------------------------------------------------------------------------------------ B: q_rows
REPS_B = [ROUTES[0], ROUTES[5], ROUTES[4], ROUTES[6], ROUTES[9]]       # R32 D64 | fp32 D128 (QB 64) | fp32 D64 | bf16 D16 | R16big D128


def test_B_representatives():
    assert [(r, _qb(dt, D, ml)) for r, dt, D, ml in REPS_B] == [(R32, 128), (R16, 64), (R16, 128), (R16, 128), (R16BIG, 128)]


@pytest.mark.parametrize("which", ["1", "2", "16", "17", "QB-1", "QB", "QB+1", "past-the-longest"])
@pytest.mark.parametrize("route", REPS_B, ids=_rid)
def test_B_q_rows(route, which):
    r, dtype, D, max_len = route
    QB = _qb(dtype, D, max_len)
    q_rows = {"QB-1": QB - 1, "QB": QB, "QB+1": QB + 1, "past-the-longest": max(LENS) + 44}.get(which) or int(which)
    full, ref = _run(dtype, D, max_len)
    out, _ = _run(dtype, D, max_len, q_rows)
    rows = ref.rows(q_rows)
    assert bool((out[~rows] == CANARY).all()), "a row at or past q_rows was written"
    assert torch.equal(out[rows], full[rows]), "the rows written with q_rows are not the full call's"
    ref.check(out, f"{_rid(route)} q_rows={q_rows}", f"B {r} {NAME[dtype]}", q_rows=q_rows)


# ------------------------------------------------------------------------------------------ C: the dispatch edge
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("max_len", [4096, 4097])
def test_C_max_len_is_an_upper_bound(D, max_len):
    out, ref = _run(BF16, D, max_len)
    ref.check(out, f"bf16-D{D} max_len={max_len}", f"C {_route(BF16, D, max_len)} bf16")
    tight, _ = _run(BF16, D, 257 if max_len == 4096 else 4200)
    assert torch.equal(out, tight), "max_len changed the result inside one route"


def test_C_one_sequence_of_4097_tokens():
    lens, heads, D = (4097,), 2, 64
    out, ref = _run(BF16, D, 4097, lens=lens, heads=heads)
    ref.check(out, "bf16-D64 len=4097", "C R16big bf16")


# ------------------------------------------------------------------------------------------ D: layouts
LAYOUT_REPS = [ROUTES[0], ROUTES[1], ROUTES[2], ROUTES[5], ROUTES[7], ROUTES[8]]


@pytest.mark.parametrize("route", LAYOUT_REPS, ids=_rid)
def test_D_layouts(route):
    r, dtype, D, max_len = route
    q, k, v, cu, ref = _batch(dtype, D)
    plain, _ = _run(dtype, D, max_len)
    hd, n = H * D, q.shape[0]
    fused = torch.cat([q, k, v], 1).contiguous()
    out, _ = _run(dtype, D, max_len, qkv=(fused[:, :hd], fused[:, hd:2 * hd], fused[:, 2 * hd:]))
    assert torch.equal(out, plain), "column slices of a fused [ntok, 3 H D] buffer"
    pitch = hd + 8
    out, _ = _run(dtype, D, max_len, qkv=tuple(Slab((n, hd), dtype, NAN, t, ld=pitch).v for t in (q, k, v)))
    assert torch.equal(out, plain), "three buffers of a padded pitch (NaN in the pad columns)"
    wide = Slab((n, hd), dtype, CANARY, ld=hd + 16)
    _enc(q, k, v, cu, wide.v, len(LENS), H, D, hd, hd + 16, max_len, max_len, dtype)
    torch.cuda.synchronize()
    assert wide.untouched(), "ld_out > H D: a pad column was written"
    assert torch.equal(wide.v, plain)
    ref.check(wide.v, _rid(route) + " ld_out", f"D {r} {NAME[dtype]}")


# ------------------------------------------------------------------------------------------ E: memory
@pytest.mark.parametrize("route", LAYOUT_REPS, ids=_rid)
def test_E_isolation_and_determinism(route):
    r, dtype, D, max_len = route
    q, k, v, cu, ref = _batch(dtype, D)
    plain, _ = _run(dtype, D, max_len)
    slabs = [Slab(t.shape, dtype, NAN, t) for t in (q, k, v)]
    so = Slab(plain.shape, dtype, CANARY)
    _enc(slabs[0].v, slabs[1].v, slabs[2].v, cu, so.v, len(LENS), H, D, H * D, H * D, max_len, max_len, dtype)
    torch.cuda.synchronize()
    assert so.untouched() and all(s.untouched() for s in slabs), "bytes next to a buffer were written"
    assert torch.isfinite(so.v.float()).all() and torch.equal(so.v, plain), "the guards reached the result"
    again, _ = _run(dtype, D, max_len)
    assert torch.equal(again, plain), "two launches differ"
    # a neighbour of NaN, then of +Inf: sequences 1 (129 tokens, after the 1-token one) and 9 (257 tokens) are the neighbours
    cul = ref.cu_list
    for fill in (float("nan"), float("inf")):
        for nb in (1, 9):
            q2, k2, v2 = q.clone(), k.clone(), v.clone()
            for t in (q2, k2, v2):
                t[cul[nb]:cul[nb + 1]] = fill
            out, _ = _run(dtype, D, max_len, qkv=(q2, k2, v2))
            others = torch.ones(q.shape[0], dtype=torch.bool, device="cuda")
            others[cul[nb]:cul[nb + 1]] = False
            assert torch.isfinite(out[others].float()).all(), f"sequence {nb} of {fill} reached another sequence"
            assert torch.equal(out[others], plain[others]), f"sequence {nb} of {fill} changed another sequence"


# ------------------------------------------------------------------------------------------ F: refusals
BAD = [("q_rows-0", dict(q_rows=0)), ("ld_in-below-HD", dict(ld_in=H * 64 - 8)), ("ld_out-below-HD", dict(ld_out=H * 64 - 8)),
       ("ld_in-not-multiple-of-8", dict(ld_in=H * 64 + 4)), ("ld_out-not-multiple-of-8", dict(ld_out=H * 64 + 4)), ("dtype", dict(dtype=99)),
       ("D20", dict(D=20)), ("max_len-0", dict(max_len=0)), ("nseq-0", dict(nseq=0))] + \
      [(f"null-{n}", {n: ctypes.c_void_p(None)}) for n in ("q", "k", "v", "cu", "out")]


@pytest.mark.parametrize("what,over", BAD, ids=[b[0] for b in BAD])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_F_refusals(dtype, what, over):
    D = 64
    q, k, v, cu, _ = _batch(dtype, D)
    so = Slab((q.shape[0], H * D), dtype, CANARY)
    a = dict(q=q, k=k, v=v, cu=cu, out=so.v, nseq=len(LENS), heads=H, D=D, ld_in=H * D, ld_out=H * D, max_len=257, q_rows=257, dtype=dtype)
    a.update(over)
    with pytest.raises(ValueError):
        _enc(**a)
    torch.cuda.synchronize()
    assert so.unwritten(), "written by a refused call"


# ------------------------------------------------------------------------------------------ Z: a sequence without tokens
@pytest.mark.parametrize("route", [ROUTES[0], ROUTES[2], ROUTES[7], ROUTES[8]], ids=_rid)
def test_Z_zero_length_sequence(route):
    r, dtype, D, max_len = route
    lens_z, lens = (65, 0, 17, 0, 129), (65, 17, 129)
    with_z, ref_z = _run(dtype, D, max_len, lens=lens_z)
    without, ref = _run(dtype, D, max_len, lens=lens)
    assert torch.equal(with_z, without), "a sequence of no tokens changed its neighbours"
    ref.check(with_z, _rid(route) + " zero-length", f"Z {r} {NAME[dtype]}")
    q, k, v, cu, _ = _batch(dtype, D, lens_z)
    so = Slab(without.shape, dtype, CANARY)
    _enc(q, k, v, cu, so.v, len(lens_z), H, D, H * D, H * D, max_len, max_len, dtype)
    torch.cuda.synchronize()
    assert so.untouched() and torch.equal(so.v, without)
