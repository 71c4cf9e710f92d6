"""-m gpu: mmgl_rope_inplace / mmgl_rope and mmgl_swiglu_fwd / mmgl_swiglu_bwd (csrc/llama_ops.hip) against stream_ref.RopeRef and
SwigluRef -- fp64 references of the storage-rounded operands -- element by element (tests/test_stream_ref_cpu.py shows that the
comparisons can fail and that torch's fp32 arithmetic stays inside).  The entry points are called directly; operands in NaN slabs,
outputs in canary slabs with intact guards, two launches bit-equal, both dtypes (VN = 8 elements of a 16-byte vector in bf16, 4 in fp32).

  RoPE     D in {2 VN (one vector per half), 4 VN, 128}, H in {1, 3}, layouts (unit, nblk, nall) = (H, 2, 3) -- multi-head, and
           grouped-query with G = 1 -- and (H, 5, 6) -- G = 4; T = 1 (the angle 0: bit-equal) and T = 7 with B = 3 (row % T wraps);
           in place (the columns past the nblk blocks keep their values), out of place forward and backward (the source untouched, the
           unrotated block a bit-for-bit copy); a row pitch one vector wider than the blocks (the padding keeps the canary); past the
           4096-block grid cap with a ragged second trip (349,531 rows, 1,048,593 work items, both entry points); ops.rope_qk_
           forward and autograd backward in the multi-head and one grouped-query layout; the refusals; rows = 0.
  SwiGLU   F in {VN, 3 VN, 13 VN}, M in {1, 5}, and M = 349,531 at F = 3 VN (the same ragged second trip), forward and backward;
           inputs randn * 4 with the root of silu', grids over [6, 20] and [-104, -60], +-0, u = 0 and dy = 0 planted
           (SwigluRef.inputs); ops.swiglu forward and backward with a non-contiguous dy; the refusals; M = 0."""
import pytest
import torch

from bounds import BF16, CANARY, F32, NAME, NAN, VEC, Slab, same
from stream_ref import RopeRef, SwigluRef

pytestmark = pytest.mark.gpu

SEED = 0
BIG_ROWS = 349531                                       # 49,933 x 7: with 3 work items per row 17 past 4096 x 256
LAYOUTS = [(2, 3), (5, 6)]                              # (nblk, nall)


def _rope(src, dst, cs, rows, T, unit, D, ld, nblk, nall, backward, code=None):
    """dst None: mmgl_rope_inplace over src's first nblk blocks; else mmgl_rope."""
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr
    code = _lib.dtype_code(src) if code is None else code
    if dst is None:
        _lib.call("mmgl_rope_inplace", None, ptr(src), ptr(cs), rows, T, unit, D, ld, nblk, int(backward), code, _lib.stream_ptr())
    else:
        _lib.call("mmgl_rope", None, ptr(src), ptr(dst), ptr(cs), rows, T, unit, D, ld, nblk, nall, int(backward), code, _lib.stream_ptr())


def _rope_case(dtype, rows, T, H, D, nblk, nall, pad, what, group):
    """All three calls of one geometry; prints one line each."""
    vn = VEC[dtype]
    width, ld = nall * H * D, nall * H * D + pad * vn
    x = RopeRef.inputs(dtype, rows, ld, seed=SEED).cuda()
    x[:, width:] = CANARY                                                       # the padding columns are no operand
    cs = Slab((T, D // 2, 2), F32, NAN, RopeRef.table(T, D).cuda())
    # in place: blocks 0 .. nblk-1 rotated, every later column as it was
    buf = Slab((rows, ld), dtype, CANARY, x)
    _rope(buf.v, None, cs.v, rows, T, H, D, ld, nblk, nall, False)
    first = buf.v.clone()
    ref = RopeRef(x, cs.v, T, H, D, nblk, nblk)
    ref.check(buf.v, f"{what} inplace", group)
    assert same(buf.v[:, ref.width:], x[:, ref.width:]), f"{what}: in place changed a column past the rotated blocks"
    assert buf.untouched() and cs.untouched()
    buf.v.copy_(x)
    _rope(buf.v, None, cs.v, rows, T, H, D, ld, nblk, nall, False)
    assert same(buf.v, first), f"{what}: two in-place launches differ"
    if T == 1:
        assert same(buf.v, x), f"{what}: the angle 0 changed a value"
    # out of place, forward and backward
    src = Slab((rows, ld), dtype, NAN, x)
    for backward in (False, True):
        dst, dst2 = Slab((rows, ld), dtype, CANARY), Slab((rows, ld), dtype, CANARY)
        _rope(src.v, dst.v, cs.v, rows, T, H, D, ld, nblk, nall, backward)
        _rope(src.v, dst2.v, cs.v, rows, T, H, D, ld, nblk, nall, backward)
        ref = RopeRef(x, cs.v, T, H, D, nblk, nall, backward=backward)
        ref.check(dst.v, f"{what} {'bwd' if backward else 'fwd'}", group)
        assert same(dst.v[:, :width][:, ~ref.rotated], x[:, :width][:, ~ref.rotated]), f"{what}: the unrotated block is no bit-for-bit copy"
        assert bool((dst.v[:, width:] == CANARY).all()), f"{what}: the padding columns were written"
        assert same(dst.v, dst2.v), f"{what}: two launches differ"
        assert same(src.v, x) and src.untouched() and dst.untouched() and cs.untouched(), f"{what}: the source or a guard changed"
        if T == 1:
            assert same(dst.v[:, :width], x[:, :width]), f"{what}: the angle 0 changed a value"


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l[0]}of{l[1]}")
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("dk", [2, 4, 0], ids=["D2vn", "D4vn", "D128"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_rope_bounds(dtype, dk, H, layout):
    D, (nblk, nall) = dk * VEC[dtype] or 128, layout
    per_head = D // 2 // VEC[dtype]
    for T, B in ((1, 3), (7, 3)):
        for pad in (0, 1):
            what = f"{NAME[dtype]}-D{D}-H{H}-{nblk}of{nall}-T{T}-B{B}-pad{pad}"
            group = f"{'one vector per half' if per_head == 1 else f'{per_head} vectors per half'}{', angle 0' if T == 1 else ', row % T wraps'}{', wide pitch' if pad else ''} {NAME[dtype]}"
            _rope_case(dtype, B * T, T, H, D, nblk, nall, pad, what, group)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_rope_past_the_grid_cap(dtype):
    vn = VEC[dtype]
    rows, T, H, D, nblk, nall = BIG_ROWS, 7, 1, 2 * vn, 2, 3
    assert rows % T == 0 and rows * nall * H * (D // 2 // vn) == 4096 * 256 + 17
    _rope_case(dtype, rows, T, H, D, nblk, nall, 0, f"{NAME[dtype]}-D{D}-H1-2of3-T7-rows{rows}", f"capped, ragged second trip {NAME[dtype]}")


@pytest.mark.parametrize("gqa", [False, True], ids=["mha", "gqa"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_rope_ops_route(dtype, gqa):
    from mmgl_amd import ops
    B, T, D = 3, 7, 4 * VEC[dtype]
    H, Hkv = (4, 2) if gqa else (3, None)
    unit, nblk, nall = (Hkv, H // Hkv + 1, H // Hkv + 2) if gqa else (H, 2, 3)
    ld = nall * unit * D
    x = RopeRef.inputs(dtype, B * T, ld, seed=SEED).cuda()
    dy = RopeRef.inputs(dtype, B * T, ld, seed=SEED + 1).cuda()
    cs = RopeRef.table(T, D).cuda()
    leaf = x.clone().view(B, T, ld).requires_grad_()
    y = ops.rope_qk_(leaf * 1.0, cs, H, Hkv)
    y.backward(dy.view(B, T, ld))
    what = f"ops.rope_qk_ {NAME[dtype]} {'gqa' if gqa else 'mha'}"
    RopeRef(x, cs, T, unit, D, nblk, nall).check(y.view(B * T, ld), f"{what} fwd", f"ops route {NAME[dtype]}")
    RopeRef(dy, cs, T, unit, D, nblk, nall, backward=True).check(leaf.grad.view(B * T, ld), f"{what} bwd", f"ops route {NAME[dtype]}")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_rope_refusals(dtype):
    from mmgl_amd import _lib
    vn = VEC[dtype]
    rows, T, H, D, nblk, nall = 6, 3, 2, 2 * vn, 2, 3
    ld = nall * H * D
    src = Slab((rows, ld), dtype, NAN, RopeRef.inputs(dtype, rows, ld, seed=SEED).cuda())
    buf, dst = Slab((rows, ld), dtype, CANARY), Slab((rows, ld), dtype, CANARY)
    cs = RopeRef.table(T, D).cuda()
    ok = dict(cs=cs, rows=rows, T=T, unit=H, D=D, ld=ld, nblk=nblk, nall=nall, backward=False, code=_lib.dtype_code(src.v))
    # (D + VN: a multiple of VN, not of 2 VN, with a pitch that holds it.  Every refusal happens on the host, before any launch.)
    both = [(dict(D=D + vn, ld=nall * H * (D + vn)), "must be multiples"), (dict(ld=ld + 1), "must be multiples"), (dict(nblk=0), "bad sizes"),
            (dict(T=0), "bad sizes"), (dict(cs=None), "null pointer"), (dict(code=7), "bad dtype")]
    for kw, msg in both + [(dict(ld=ld - vn), "bad sizes"), (dict(nblk=nall + 1), "bad sizes")]:
        with pytest.raises(ValueError, match=msg):
            _rope(src.v, dst.v, **dict(ok, **kw))
    for kw, msg in both + [(dict(ld=nblk * H * D - vn), "bad sizes")]:          # in place the row is its nblk blocks
        with pytest.raises(ValueError, match=msg):
            _rope(buf.v, None, **dict(ok, **kw))
    for s_, d_ in ((None, dst.v), (src.v, None)):
        with pytest.raises(ValueError, match="null pointer"):
            _lib.call("mmgl_rope", None, _lib.ptr(s_), _lib.ptr(d_), _lib.ptr(cs), rows, T, H, D, ld, nblk, nall, 0, ok["code"], _lib.stream_ptr())
    with pytest.raises(ValueError, match="null pointer"):
        _lib.call("mmgl_rope_inplace", None, None, _lib.ptr(cs), rows, T, H, D, ld, nblk, 0, ok["code"], _lib.stream_ptr())
    with pytest.raises(ValueError, match="src == dst"):
        _rope(buf.v, buf.v, **ok)
    _rope(src.v, dst.v, **dict(ok, rows=0))                                     # rows = 0: OK, nothing written
    _rope(buf.v, None, **dict(ok, rows=0))
    torch.cuda.synchronize()
    assert buf.unwritten() and dst.unwritten() and src.untouched()


# ------------------------------------------------------------------------------------------ SwiGLU
def _swiglu_fwd(gu, y, M, F, code=None):
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr
    _lib.call("mmgl_swiglu_fwd", None, ptr(gu), ptr(y), M, F, _lib.dtype_code(y) if code is None else code, _lib.stream_ptr())


def _swiglu_bwd(dy, gu, dgu, M, F, code=None):
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr
    _lib.call("mmgl_swiglu_bwd", None, ptr(dy), ptr(gu), ptr(dgu), M, F, _lib.dtype_code(dgu) if code is None else code, _lib.stream_ptr())


SWIGLU_CASES = [(fk, M) for fk in (1, 3, 13) for M in (1, 5)] + [(3, BIG_ROWS)]


@pytest.mark.parametrize("case", SWIGLU_CASES, ids=lambda c: f"F{c[0]}vn-M{c[1]}")
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_swiglu_bounds(dtype, case):
    vn = VEC[dtype]
    F, M = case[0] * vn, case[1]
    if M == BIG_ROWS:
        assert M * (F // vn) == 4096 * 256 + 17
    gu, dy = (t.cuda() for t in SwigluRef.inputs(dtype, M, F, seed=SEED))
    assert torch.isfinite(gu.float()).all() and torch.isfinite(dy.float()).all()
    gus, dys = Slab((M, 2 * F), dtype, NAN, gu), Slab((M, F), dtype, NAN, dy)
    out = [(Slab((M, F), dtype, CANARY), Slab((M, 2 * F), dtype, CANARY)) for _ in range(2)]
    for y, dgu in out:
        _swiglu_fwd(gus.v, y.v, M, F)
        _swiglu_bwd(dys.v, gus.v, dgu.v, M, F)
    (y, dgu), (y2, dgu2) = out
    what = f"{NAME[dtype]}-{M}x{F}"
    group = f"{'capped, ragged second trip' if M == BIG_ROWS else 'one vector per row' if F == vn else f'{F // vn} vectors per row'} {NAME[dtype]}"
    ref = SwigluRef(gu, dy)
    ref.check(y.v, "y", what, group)
    ref.check(dgu.v[:, :F], "dg", what, group)
    ref.check(dgu.v[:, F:], "du", what, group)
    assert same(y.v, y2.v) and same(dgu.v, dgu2.v), f"{what}: two launches differ"
    assert same(gus.v, gu) and same(dys.v, dy), f"{what}: an operand changed"
    for name, s in dict(gu=gus, dy=dys, y=y, dgu=dgu).items():
        assert s.untouched(), f"{what}: written outside {name}"


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_swiglu_ops_route(dtype):
    from mmgl_amd import ops
    M, F = 5, 13 * VEC[dtype]
    gu, dy = (t.cuda() for t in SwigluRef.inputs(dtype, M, F, seed=SEED))
    wide = torch.full((M, 2 * F), NAN, dtype=dtype, device="cuda")
    wide[:, ::2] = dy                                                           # dy as every second column: non-contiguous
    leaf = gu.clone().requires_grad_()
    y = ops.swiglu(leaf)
    assert not wide[:, ::2].is_contiguous()
    y.backward(wide[:, ::2])
    ref, what, group = SwigluRef(gu, dy), f"ops.swiglu {NAME[dtype]} {M}x{F}", f"ops route {NAME[dtype]}"
    ref.check(y, "y", what, group)
    ref.check(leaf.grad[:, :F], "dg", what, group)
    ref.check(leaf.grad[:, F:], "du", what, group)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_swiglu_refusals(dtype):
    vn = VEC[dtype]
    M, F = 5, 3 * vn
    gu, dy = (t.cuda() for t in SwigluRef.inputs(dtype, M, F, seed=SEED))
    gus, dys = Slab((M, 2 * F), dtype, NAN, gu), Slab((M, F), dtype, NAN, dy)
    y, dgu = Slab((M, F), dtype, CANARY), Slab((M, 2 * F), dtype, CANARY)
    for kw, msg in [(dict(F=F - 1), "must be a multiple"), (dict(F=0), "bad arguments"), (dict(F=-vn), "bad arguments"), (dict(code=7), "bad dtype")]:
        with pytest.raises(ValueError, match=msg):
            _swiglu_fwd(gus.v, y.v, M, **dict(dict(F=F), **kw))
        with pytest.raises(ValueError, match=msg):
            _swiglu_bwd(dys.v, gus.v, dgu.v, M, **dict(dict(F=F), **kw))
    from mmgl_amd import _lib
    code = _lib.dtype_code(gu)
    for args in ((None, y.v), (gus.v, None)):
        with pytest.raises(ValueError, match="bad arguments"):
            _swiglu_fwd(*args, M, F, code=code)
    for args in ((None, gus.v, dgu.v), (dys.v, None, dgu.v), (dys.v, gus.v, None)):
        with pytest.raises(ValueError, match="bad arguments"):
            _swiglu_bwd(*args, M, F, code=code)
    _swiglu_fwd(gus.v, y.v, 0, F)                                               # M = 0: OK, nothing written
    _swiglu_bwd(dys.v, gus.v, dgu.v, 0, F)
    torch.cuda.synchronize()
    assert y.unwritten() and dgu.unwritten() and gus.untouched() and dys.untouched()
