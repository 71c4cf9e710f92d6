"""-m gpu: the masked cross-attention core (csrc/xattn.hip) against attn_ref.XAttnRef -- an fp64 reference of the storage-rounded
operands -- element by element: out, lse, dq, dk, dv each within u |want| + (c + n 2^-24 (S_i + ln S)) mag (the count is in the
docstrings of XAttnRef and SelfAttnRef; tests/test_xattn_ref_cpu.py shows on the CPU that this comparison fails for a dropped key, a
shifted mask, a wrong head, a lost query row or the wrong rule for a sample without a valid key).  mmgl_xattn_fwd / mmgl_xattn_bwd are
called directly, so lse is seen; every output buffer holds NaN before the call.  Inputs: XAttnRef.inputs (edge keys carry several
percent of every row, dout is 16 times larger on the edge rows).  Masks: XAttnRef.mask -- sample 0 all valid, sample 1 holed (edge
keys and key S - 1 among the holes), sample 2 without a valid key.

The plans of csrc/xattn.hip are restated here (_route, _bwd_plan, _fwd_geometry, _workspace) and the restated workspace size is held
against mmgl_xattn_bwd_workspace for every case, so a change to the plans fails loudly instead of quietly moving the cases off the
paths they were chosen for.

  A  every (dtype, D, key block) instantiation, both sides of S = 32 / 33, 64 / 65, 128 / 129, S = 1, 17 and 256; the one that cannot
     be launched (fp32, D = 128, S > 128: 256 KiB of LDS) is refused before any launch.  One sample without a valid key on its own.
     A handful also through ops.xattn_core under autograd, bit for bit.
  B  query rows: T on either side of the 16- / 32-row tile and the 64-row trip, one representative per backward route
  C  chunk plans: per backward route one chunk with T > 64, several chunks, a chunk of an odd number of 32-row tiles followed by
     another chunk, a last chunk of one row; forward chunks that are no whole number of 4-wave rounds.  Asserted on the case list.
  D  isolation and determinism: operands carved out of NaN slabs, results and an exactly sized workspace out of canary slabs; huge
     finite K / V on the masked keys; two launches"""
import pytest
import torch

from attn_ref import XAttnRef
from bounds import BF16, CANARY_BYTE, F32, NAME, NAN, NAN_BYTE, ByteSlab, Slab, esz, nan

pytestmark = pytest.mark.gpu

SEED = 0                    # tests/test_xattn_ref_cpu.py: every wrong reference leaves the bound on >= 25 % at this seed
ONE_WAVE, MULTI_WAVE, TWO_KERNEL = "one-wave", "multi-wave", "two-kernel"
MAX_LDS = 160 * 1024        # mmgl_set_lds


# ------------------------------------------------------------------------------------------ csrc/xattn.hip's plans, restated
def _nsb(S):
    """DISPATCH_NSB: 16-key blocks of the instantiation that serves S keys."""
    return 2 if S <= 32 else 4 if S <= 64 else 8 if S <= 128 else 16


def _qt(dtype, D, S, work=1):
    """XC::QT: 16-row query tiles per iteration (work = 1 forward, 2 dQ)."""
    return 2 if work * _nsb(S) * (D // 16) * (esz(dtype) // 2) <= 32 else 1


def _route(dtype, D, S):
    """bwd_route."""
    if dtype != BF16:
        return TWO_KERNEL
    if D <= 64 and S <= 64:
        return ONE_WAVE
    if D in (64, 128) and S <= 128:
        return MULTI_WAVE
    return TWO_KERNEL


def _bwd_plan(dtype, B, H, T, S, D):
    """bwd_plan: (route, nchunk, rows_per_chunk)."""
    route = _route(dtype, D, S)
    units = B * H * (1 if route == MULTI_WAVE else (S + 31) // 32)
    if route == MULTI_WAVE:
        nchunk = 1 if units >= 256 else (512 + units - 1) // units
    else:
        nchunk = (2048 + units - 1) // units
    nchunk = max(1, min(nchunk, (T + 63) // 64))
    rows = ((T + nchunk - 1) // nchunk + 31) // 32 * 32
    return route, (T + rows - 1) // rows, rows


def _fwd_geometry(B, H, T, tile):
    """fwd_geometry at its defaults (512 workgroups aimed at, two chunks from 8 tiles on): (rows_per_wg, nchunk)."""
    bh = B * H
    nc = (512 + bh // 2) // bh
    if nc < 2 and T >= 8 * tile:
        nc = 2
    nc = max(1, min(nc, (T + tile - 1) // tile))
    rows = ((T + nc - 1) // nc + tile - 1) // tile * tile
    return rows, (T + rows - 1) // rows


def _workspace(B, H, T, S, D):
    """mmgl_xattn_bwd_workspace: the row dots and two sets of per-chunk fp32 partials, the larger of the two dtypes' plans."""
    up = lambda n: (n + 255) // 256 * 256
    return max(up(B * H * T * 4) + 2 * up(_bwd_plan(dt, B, H, T, S, D)[1] * B * S * H * D * 4) for dt in (BF16, F32))


def _lds_fwd(dtype, D, S):
    """launch_fwd / the dQ kernel: XC::KV_BYTES + SPAD."""
    spad, dpad = 16 * _nsb(S), (D + 31) // 32 * 32
    return esz(dtype) * (spad * dpad + (spad * (dpad + 16) if dtype == BF16 else spad * dpad)) + spad


# ------------------------------------------------------------------------------------------ cases
def _case(group, dtype, D, S, T=70, B=3, H=3, first=0):
    return (group, dtype, D, S, T, B, H, first)


def _id(c):
    group, dtype, D, S, T, B, H, first = c
    return f"{NAME[dtype]}-D{D}-S{S}-T{T}-B{B}H{H}" + ("-masked" if first == 2 else "")


GRID = [(dt, D, S) for dt in (F32, BF16) for D in (16, 32, 64, 128) for S in (1, 17, 32, 33, 64, 65, 128, 129, 256)]
REFUSED = [g for g in GRID if _lds_fwd(*g) > MAX_LDS]
CASES_A = ([_case("A", dt, D, S) for dt, D, S in GRID if (dt, D, S) not in REFUSED]
           + [_case("A", dt, D, S, B=1, first=2) for dt in (F32, BF16) for D, S in ((64, 100), (32, 200))])
AUTOGRAD = [_case("A", *g) for g in ((BF16, 64, 33), (BF16, 128, 128), (BF16, 32, 129), (BF16, 16, 65), (F32, 64, 65), (F32, 16, 17))]
REPS_B = [(BF16, 64, 40), (BF16, 128, 100), (BF16, 64, 100), (BF16, 32, 100), (F32, 64, 40)]
CASES_B = [_case("B", dt, D, S, T=T, H=2) for dt, D, S in REPS_B for T in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)]
CASES_C = [
    # one chunk with more than one 64-row trip: the direct bf16 store of dK / dV
    _case("C", BF16, 16, 33, T=65, B=32, H=32),       # one-wave: B H nsg = 2048
    _case("C", BF16, 128, 33, T=65, B=8, H=32),       # multi-wave (2 waves): B H = 256
    # three chunks of 96, 96 and 1 rows: an odd number of 32-row tiles followed by another chunk, and a last chunk of one row
    _case("C", BF16, 16, 33, T=193, B=18, H=19),      # one-wave: B H nsg = 684
    _case("C", BF16, 128, 33, T=193, B=9, H=19),      # multi-wave: B H = 171
    _case("C", BF16, 16, 65, T=193, B=12, H=19),      # two-kernel: B H nsg = 684
    _case("C", F32, 16, 33, T=193, B=18, H=19),       # two-kernel, fp32
    # forward: four chunks of two 32-row tiles, half a 4-wave round
    _case("C", BF16, 16, 17, T=200, B=4, H=32),
] + [_case("C", dt, D, S, T=T, B=2) for dt, D, S in REPS_B for T in (65, 129)]      # chunks of 64 (, 64) and 1 rows
CASES_D = [_case("D", dt, D, S, T=T, H=2) for dt, D, S in ((BF16, 64, 40), (BF16, 128, 100), (BF16, 32, 100), (F32, 64, 40)) for T in (40, 70)]
EVERY = CASES_A + CASES_B + CASES_C + CASES_D


def _inputs(c):
    group, dtype, D, S, T, B, H, first = c
    q, k, v, dout = XAttnRef.inputs(dtype, B, T, S, H, D, seed=SEED, device="cuda")
    return q, k, v, dout, XAttnRef.mask(B, S, first).cuda()


def _fwd(c, q, k, v, am, out, lse):
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr
    group, dtype, D, S, T, B, H, first = c
    _lib.call("mmgl_xattn_fwd", None, ptr(q), ptr(k), ptr(v), ptr(am), ptr(out), ptr(lse), B, H, T, S, D, _lib.dtype_code(q), _lib.stream_ptr())


def _bwd(c, q, k, v, dout, am, lse, dq, dk, dv, ws):
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr
    group, dtype, D, S, T, B, H, first = c
    _lib.call("mmgl_xattn_bwd", None, ptr(dout), ptr(q), ptr(k), ptr(v), ptr(lse), ptr(am), ptr(dq), ptr(dk), ptr(dv), ptr(ws), ws.numel(),
              B, H, T, S, D, _lib.dtype_code(q), _lib.stream_ptr())


def _call(c, q, k, v, dout, am):
    """out, lse, dq, dk, dv of the raw entry points; every result buffer holds NaN before the call, the workspace NaN bit patterns."""
    from mmgl_amd import _lib
    group, dtype, D, S, T, B, H, first = c
    out, lse = nan(B, T, H * D, dtype=dtype), nan(B, H, T, dtype=F32)
    _fwd(c, q, k, v, am, out, lse)
    nws = _lib.lib().mmgl_xattn_bwd_workspace(B, H, T, S, D)
    assert nws == _workspace(B, H, T, S, D), "mmgl_xattn_bwd_workspace is not the restated plan's: the cases may have left their paths"
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device="cuda")
    dq, dk, dv = nan(B, T, H * D, dtype=dtype), nan(B, S, H * D, dtype=dtype), nan(B, S, H * D, dtype=dtype)
    _bwd(c, q, k, v, dout, am, lse, dq, dk, dv, ws)
    torch.cuda.synchronize()
    return out, lse, dq, dk, dv


def _group(c):
    group, dtype, D, S, T, B, H, first = c
    return f"{group} {_route(dtype, D, S)} {NAME[dtype]}"


def _check(c):
    group, dtype, D, S, T, B, H, first = c
    q, k, v, dout, am = _inputs(c)
    got = _call(c, q, k, v, dout, am)
    XAttnRef(q, k, v, am, dout, H).check(got, _id(c), _group(c))
    return (q, k, v, dout, am), got


# ------------------------------------------------------------------------------------------ A: the instantiation grid
def test_A_grid_covers_every_instantiation():
    """All 16 (D, key block) pairs of either dtype are launched or asserted refused; the refused set is the one INTEGRATION.md states."""
    assert sorted(REFUSED, key=str) == sorted([(F32, 128, 129), (F32, 128, 256)], key=str)
    for dt in (F32, BF16):
        seen = {(D, _nsb(S)) for _, dtype, D, S, *_ in CASES_A if dtype == dt} | {(D, _nsb(S)) for dtype, D, S in REFUSED if dtype == dt}
        assert seen == {(D, n) for D in (16, 32, 64, 128) for n in (2, 4, 8, 16)}
    assert {_route(dt, D, S) for _, dt, D, S, *_ in CASES_A if dt == BF16} == {ONE_WAVE, MULTI_WAVE, TWO_KERNEL}


@pytest.mark.parametrize("case", CASES_A, ids=_id)
def test_A_instantiation_grid(case):
    _check(case)


@pytest.mark.parametrize("dtype,D,S", REFUSED, ids=lambda x: NAME.get(x, str(x)))
def test_A_refused_before_any_launch(dtype, D, S):
    """fp32, D = 128, S > 128: K and V of 256 keys are 256 KiB of LDS.  Both entry points return an error through _lib.call and
    launch nothing: every result buffer still holds its NaN."""
    c = _case("A", dtype, D, S)
    group, dtype, D, S, T, B, H, first = c
    q, k, v, dout, am = _inputs(c)
    out, lse = nan(B, T, H * D, dtype=dtype), nan(B, H, T, dtype=F32)
    with pytest.raises(ValueError, match="LDS"):
        _fwd(c, q, k, v, am, out, lse)
    from mmgl_amd import _lib
    ws = torch.full((_lib.lib().mmgl_xattn_bwd_workspace(B, H, T, S, D),), 0xFF, dtype=torch.uint8, device="cuda")
    dq, dk, dv = nan(B, T, H * D, dtype=dtype), nan(B, S, H * D, dtype=dtype), nan(B, S, H * D, dtype=dtype)
    with pytest.raises(ValueError, match="LDS"):
        _bwd(c, q, k, v, dout, am, torch.zeros_like(lse), dq, dk, dv, ws)
    torch.cuda.synchronize()
    for name, x in zip(XAttnRef.NAMES, (out, lse, dq, dk, dv)):
        assert torch.isnan(x).all(), f"{name}: written by a refused call"
    assert bool((ws == 0xFF).all()), "workspace: written by a refused call"


@pytest.mark.parametrize("case", AUTOGRAD, ids=_id)
def test_A_ops_under_autograd_is_the_raw_call(case):
    from mmgl_amd import ops
    group, dtype, D, S, T, B, H, first = case
    (q, k, v, dout, am), got = _check(case)
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    out = ops.xattn_core(qg, kg, vg, am, H)
    grads = torch.autograd.grad(out, (qg, kg, vg), dout)
    for name, a, b in zip(("out", "dq", "dk", "dv"), (out,) + grads, (got[0],) + got[2:]):
        assert torch.equal(a, b), f"{name}: ops.xattn_core under autograd is not the raw entry point's result"


# ------------------------------------------------------------------------------------------ B: query-row edges
def test_B_representatives():
    """One representative per backward route, and a 16-row and a 32-row forward tile."""
    assert [_route(*r) for r in REPS_B] == [ONE_WAVE, MULTI_WAVE, MULTI_WAVE, TWO_KERNEL, TWO_KERNEL]
    assert {_qt(*r) for r in REPS_B} == {1, 2} and _qt(BF16, 128, 100) == 1 and _qt(BF16, 64, 40) == 2


@pytest.mark.parametrize("case", CASES_B, ids=_id)
def test_B_query_row_edges(case):
    _check(case)


# ------------------------------------------------------------------------------------------ C: chunk plans
def test_C_case_list_has_the_plan_properties():
    plans = {}
    for c in CASES_A + CASES_B + CASES_C:
        group, dtype, D, S, T, B, H, first = c
        route, nchunk, rows = _bwd_plan(dtype, B, H, T, S, D)
        plans.setdefault((NAME[dtype], route), []).append((T, nchunk, rows))
    assert set(plans) == {("bf16", ONE_WAVE), ("bf16", MULTI_WAVE), ("bf16", TWO_KERNEL), ("f32", TWO_KERNEL)}
    for key, ps in plans.items():
        assert any(n > 1 for T, n, r in ps), f"{key}: no case with several chunks"
        assert any(n > 1 and (r // 32) % 2 == 1 for T, n, r in ps), f"{key}: no chunk of an odd number of 32-row tiles followed by another"
        assert any(n > 1 and T - (n - 1) * r == 1 for T, n, r in ps), f"{key}: no last chunk of one row"
        if key[1] != TWO_KERNEL:            # the direct store of dK / dV in the operand dtype, over more than one 64-row trip
            assert any(n == 1 and T > 64 for T, n, r in ps), f"{key}: no single chunk with T > 64"
            assert any(n == 1 and T <= 64 for T, n, r in ps)
    fwd = []
    for c in CASES_A + CASES_B + CASES_C:
        group, dtype, D, S, T, B, H, first = c
        tile = 16 * _qt(dtype, D, S)
        rows, nchunk = _fwd_geometry(B, H, T, tile)
        fwd.append((tile, rows, nchunk))
    assert any(n >= 2 and r > t and r % (4 * t) for t, r, n in fwd), "forward: no chunk of several tiles that is no whole 4-wave round"
    assert any(n >= 2 and r == t for t, r, n in fwd) and any(n == 1 and r >= 4 * t for t, r, n in fwd)
    assert {t for t, r, n in fwd} == {16, 32}


def test_C_restated_workspace_is_the_library_s():
    from mmgl_amd import _lib
    for c in EVERY + [_case("A", *g) for g in REFUSED]:
        group, dtype, D, S, T, B, H, first = c
        assert _lib.lib().mmgl_xattn_bwd_workspace(B, H, T, S, D) == _workspace(B, H, T, S, D), _id(c)


@pytest.mark.parametrize("case", CASES_C, ids=_id)
def test_C_chunk_plans(case):
    _check(case)


# ------------------------------------------------------------------------------------------ D: isolation and determinism
def _carved_call(c, q, k, v, dout, am):
    """The two calls with every operand carved out of a slab of 0xFF bytes (NaN in either dtype, 255 in the mask) and every result,
    and a workspace of exactly mmgl_xattn_bwd_workspace bytes, out of canary slabs.  lse is a result of the forward and an operand of
    the backward: its slab is 0xFF.  Returns the results and the names of the slabs whose margins changed."""
    from mmgl_amd import _lib
    group, dtype, D, S, T, B, H, first = c
    ins = dict(zip(("q", "k", "v", "dout", "key_valid"), (Slab(t.shape, t.dtype, NAN_BYTE, t) for t in (q, k, v, dout, am))))
    qc, kc, vc, gc, ac = (s.v for s in ins.values())
    nws = _lib.lib().mmgl_xattn_bwd_workspace(B, H, T, S, D)
    outs = dict(out=Slab((B, T, H * D), dtype, CANARY_BYTE), lse=Slab((B, H, T), F32, NAN_BYTE), dq=Slab((B, T, H * D), dtype, CANARY_BYTE),
                dk=Slab((B, S, H * D), dtype, CANARY_BYTE), dv=Slab((B, S, H * D), dtype, CANARY_BYTE), workspace=ByteSlab(nws))
    for name in ("out", "dq", "dk", "dv"):
        outs[name].v.fill_(NAN)
    _fwd(c, qc, kc, vc, ac, outs["out"].v, outs["lse"].v)
    _bwd(c, qc, kc, vc, gc, ac, outs["lse"].v, outs["dq"].v, outs["dk"].v, outs["dv"].v, outs["workspace"].v)
    torch.cuda.synchronize()
    touched = [name for name, s in list(outs.items()) + list(ins.items()) if not s.untouched()]
    return tuple(outs[n].v for n in XAttnRef.NAMES), touched


@pytest.mark.parametrize("case", CASES_D, ids=_id)
def test_D_isolation_and_determinism(case):
    group, dtype, D, S, T, B, H, first = case
    (q, k, v, dout, am), plain = _check(case)
    # nothing but the operands is read, nothing but the results is written
    got, touched = _carved_call(case, q, k, v, dout, am)
    assert not touched, f"bytes next to {touched} were written"
    XAttnRef(q, k, v, am, dout, H).check(got, _id(case), _group(case) + " carved")
    for name, a, b in zip(XAttnRef.NAMES, got, plain):
        assert torch.equal(a, b), f"{name}: the carved call differs from the plain one"
    # two launches are bit-equal
    for name, a, b in zip(XAttnRef.NAMES, _call(case, q, k, v, dout, am), plain):
        assert torch.equal(a, b), f"{name}: two calls differ"
    # a masked key of a sample that has a valid key contributes nothing, whatever it holds (huge and finite: 0 * NaN is NaN in the
    # reference too); a sample without a valid key reads all its keys
    dead = (am == 0) & (am != 0).any(1, keepdim=True)
    assert bool(dead.any())
    k2, v2 = k.clone(), v.clone()
    k2[dead], v2[dead] = 1e30, -1e30
    for name, a, b in zip(XAttnRef.NAMES, _call(case, q, k2, v2, dout, am), plain):
        assert torch.isfinite(a.float()).all(), f"{name}: a masked key's value reached the result"
        assert torch.equal(a, b), f"{name}: differs from the run with ordinary values on the masked keys"
