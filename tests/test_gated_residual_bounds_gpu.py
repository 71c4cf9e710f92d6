"""-m gpu: mmgl_gated_residual_fwd / bwd (csrc/elementwise.hip) against row_ref.GatedRef -- an fp64 reference of the storage-rounded
operands -- element by element, with the dropout mask taken from bounds.hash_keep, an independent restatement of mmgl_hash32 (the
existing tests compare the kernels' masks with each other only; tests/test_row_ref_cpu.py holds hash_keep against a big-integer
restatement and shows that a mask one element off leaves the bound on 42 % of the elements).  The entry points are called directly.

  n in {5, 8, 65, 256 * 8 * 2048 + 3}: nothing but the tail loop, one whole chunk, chunks and a tail, and past the 2048-block cap
  (a second grid-stride trip in bf16, every block's second trip in fp32) with a tail; both dtypes; gate given and NULL; p in {0, 0.3}.
  y, dx and dgate within the bound; the gradient of the residual is dy itself, bit for bit, through ops.gated_residual (the entry
  point does not write it: the caller aliases it); operands in NaN slabs, outputs and the workspace in canary slabs; a short workspace
  and p = 1 are refused before any launch."""
import pytest
import torch

from bounds import BF16, CANARY, F32, NAME, VEC, ByteSlab, Slab
from row_ref import GatedRef

pytestmark = pytest.mark.gpu

SEED = 0
DROP_SEED = 0x9E3779B97F4A7C15          # a seed with its top bit set: the hash's 64-bit wrap-around
BIG = 256 * 8 * 2048 + 3
WS_BYTES = 2048 * 4


def _inputs(dtype, n):
    g = torch.Generator().manual_seed(SEED)
    res, x, dy = (torch.randn(n, generator=g).to(dtype).cuda() for _ in range(3))
    return res, x, dy, torch.tensor([0.7], device="cuda")


def _fwd(res, x, gate, y, n, p):
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr
    _lib.call("mmgl_gated_residual_fwd", None, ptr(res.v), ptr(x.v), ptr(gate), ptr(y.v), n, p, DROP_SEED, _lib.dtype_code(x.v), _lib.stream_ptr())


def _bwd(dy, x, gate, dx, dgate, ws, nbytes, n, p):
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr
    _lib.call("mmgl_gated_residual_bwd", None, ptr(dy.v), ptr(x.v), ptr(gate), ptr(dx.v), ptr(None if dgate is None else dgate.v), ws.ptr(), nbytes, n, p,
              DROP_SEED, _lib.dtype_code(x.v), _lib.stream_ptr())


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("gated", [True, False], ids=["gate", "nogate"])
@pytest.mark.parametrize("n", [5, 8, 65, BIG])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_gated_residual_bounds(dtype, n, gated, p):
    from mmgl_amd import _lib
    assert _lib.lib().mmgl_gated_residual_bwd_workspace(n) == WS_BYTES
    assert GatedRef.blocks(n, VEC[dtype]) * 4 <= WS_BYTES
    res, x, dy, gate = _inputs(dtype, n)
    gate = gate if gated else None
    rs, xs, dys = (Slab(t.shape, dtype, float("nan"), t) for t in (res, x, dy))
    y, dx = Slab((n,), dtype, CANARY), Slab((n,), dtype, CANARY)
    dgate = Slab((1,), F32, CANARY)
    ws = ByteSlab(WS_BYTES)
    _fwd(rs, xs, gate, y, n, p)
    _bwd(dys, xs, gate, dx, dgate if gated else None, ws, WS_BYTES, n, p)
    torch.cuda.synchronize()
    what = f"{NAME[dtype]}-n{n}-{'gate' if gated else 'nogate'}-p{p}"
    group = f"{'tail' if n < VEC[dtype] else 'capped' if n == BIG else 'chunks'} {NAME[dtype]}"
    ref = GatedRef(res, x, None if gate is None else gate.item(), p, seed=DROP_SEED).backward(dy)
    ref.check(y.v, "y", what, group)
    ref.check(dx.v, "dx", what, group)
    if gated:
        ref.check(dgate.v, "dgate", what, group)
    else:
        assert dgate.unwritten()
    if p > 0:
        assert bool((dx.v[~ref.keep] == 0).all()), f"{what}: a dropped element has a gradient"
        assert n < 100 or 0.69 < ref.keep.double().mean().item() < 0.71
    for name, s in dict(res=rs, x=xs, dy=dys, y=y, dx=dx, dgate=dgate, ws=ws).items():
        assert s.untouched(), f"{what}: written outside {name}"


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_residual_gradient_is_dy(dtype):
    from mmgl_amd import ops
    res, x, dy, gate = _inputs(dtype, 4099)
    res.requires_grad_(), x.requires_grad_()
    ops.gated_residual(res, x, gate[0], 0.3, True).backward(dy)
    assert torch.equal(res.grad, dy)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_refusals(dtype):
    n = 65
    res, x, dy, gate = _inputs(dtype, n)
    rs, xs, dys = (Slab(t.shape, dtype, float("nan"), t) for t in (res, x, dy))
    y, dx, dgate, ws = Slab((n,), dtype, CANARY), Slab((n,), dtype, CANARY), Slab((1,), F32, CANARY), ByteSlab(WS_BYTES)
    with pytest.raises(ValueError, match="outside"):
        _fwd(rs, xs, gate, y, n, 1.0)
    with pytest.raises(ValueError, match="outside"):
        _bwd(dys, xs, gate, dx, dgate, ws, WS_BYTES, n, 1.0)
    with pytest.raises(ValueError, match="workspace too small"):
        _bwd(dys, xs, gate, dx, dgate, ws, WS_BYTES - 1, n, 0.0)
    torch.cuda.synchronize()
    for s in (y, dx, dgate, ws):
        assert s.unwritten()
