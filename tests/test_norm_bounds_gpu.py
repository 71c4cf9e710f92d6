"""-m gpu: the ten norm entry points of csrc/rownorm.hip against row_ref.NormRef -- an fp64 reference of the storage-rounded operands --
element by element: y and dx within u |want| + 2^-16 mag, the saved mean and rstd within 2^-18 A and 2^-17 rs, dgamma and dbeta within
2^-24 |want| + max(2^-16, 2 n 2^-24) mag, the stored sum and the dropout mask bit for bit against bounds.hash_keep (the count is in
NormRef's docstring; tests/test_row_ref_cpu.py shows on the CPU that this comparison fails for a chunk lost from the statistics, a row
lost from the parameter gradients, dres left out, a mask index one row off).  The entry points are called directly.

geometry(), bwd_blocks() and mmgl_norm_bwd_workspace of csrc/rownorm.hip are restated here.  Every case holds the restated workspace size
against the entry point, and the backward runs with exactly the bytes the restated grid uses (blocks x rows per block partial rows):
one byte less is refused (F), so a change to the dispatch fails loudly instead of quietly moving the cases off their branches.

  A  every dispatch branch, first and last cols of each: 1, 64 | 65, 128 | 129, 192 | 193, 256 | 257, 512 | 513, 768 | 769, 1024 chunks
     of 16 bytes (bf16 cols 8 ... 8192, fp32 4 ... 4096), 5 rows, LayerNorm and RMSNorm, forward and backward, the combinations of
     gamma / beta present or NULL in turn, dgamma / dbeta NULL (the uncapped grid, no reduce launch) on three of them
  B  rows: 1 and 3 (less than a block of four: dead rows must still write zero partial rows), 125, 2053 on a TPR = 64 shape and 517 on
     a TPR = 256 shape (the backward's 512-block cap and its stride seam), 32773 x 8 and 8197 x 2056 in bf16 (the forward's 8192-block
     cap, and the frozen-affine backward's)
  C  the fused pairs mmgl_add_layernorm_fwd / bwd and mmgl_add_rmsnorm_fwd / bwd: dsum given and NULL, p_drop 0 and 0.3 with the sum,
     dres and dx held against hash_keep at element indices past the first row, sum_out / mean / rstd NULL (inference).  One forward
     case whose element index passes 2^31 (262147 x 8192 bf16, p_drop 0.3), checked on row slices: under a second
  D  the compact copy (mmgl_layernorm_tiles_fwd, mmgl_add_layernorm_tiles_fwd): yc rows bit-equal to the mapped rows of y, unmapped
     rows of yc and map entries -1 and >= crows leave the canary
  E  isolation and determinism: in every case the operands are carved out of NaN slabs and the outputs out of canary slabs whose
     guards come back untouched, the workspace is pre-filled with NaN (a dead row that skipped its zero partial row would show in
     dgamma) between guard bytes; E runs one case of each kernel twice, bit-equal
  F  refusals before any launch, outputs untouched: cols 1004 / 1002 (no whole chunks), 8200 / 4100 (past the register-resident row),
     a workspace one byte short, p_drop = 1, crows > rows"""
import pytest
import torch

from bounds import BF16, CANARY, F32, NAME, VEC, ByteSlab, Slab
from row_ref import NormRef

pytestmark = pytest.mark.gpu

SEED = 0                    # tests/test_row_ref_cpu.py: every wrong reference leaves the bound on >= 25 % at this seed
DROP_SEED = 11
EPS = 1e-5
MAXBLK, FWD_MAXBLK, NVMAX = 512, 8192, 4


# ------------------------------------------------------------------------------------------ the plans, restated
def geometry(dtype, cols):
    """(threads per row, 16-byte chunks per thread, rows per block) of csrc/rownorm.hip's geometry(); ValueError where it refuses."""
    vn = VEC[dtype]
    if cols % vn:
        raise ValueError("no whole chunks")
    nch = cols // vn
    tpr = 64 if nch <= 64 * 4 else 256
    nv = -(-nch // tpr)
    if nv > NVMAX:
        raise ValueError("past the register-resident row")
    return tpr, nv, 256 // tpr


def bwd_blocks(rows, rpb):
    return min(-(-rows // rpb), MAXBLK)


def workspace_bytes(rows, cols):
    """mmgl_norm_bwd_workspace: the partial rows of either geometry."""
    return min(-(-rows // 4) * 4, 4 * MAXBLK) * cols * 2 * 4


def used_bytes(dtype, rows, cols):
    """What norm_bwd asks of the workspace: one partial row of 2 cols floats per (block, row in block)."""
    _, _, rpb = geometry(dtype, cols)
    return bwd_blocks(rows, rpb) * rpb * cols * 2 * 4


# ------------------------------------------------------------------------------------------ slabs
def operand(t):
    return None if t is None else Slab(t.shape, t.dtype, float("nan"), t)


def output(shape, dtype):
    return Slab(shape, dtype, CANARY)


Workspace = ByteSlab


def P(s):
    from mmgl_amd._lib import ptr
    return ptr(None if s is None else s.v)


# ------------------------------------------------------------------------------------------ one case
class Case:
    def __init__(self, group, kind, dtype, rows, cols, gamma=True, beta=True, grads=True, fused=False, dsum=True, p=0.0, seams=(), saved=True):
        self.group, self.kind, self.dtype, self.rows, self.cols, self.gamma, self.grads = group, kind, dtype, rows, cols, gamma, grads
        self.beta, self.fused, self.dsum, self.p, self.seams, self.saved = beta and kind == "ln", fused, dsum and fused, p, seams, saved
        self.rms = kind == "rms"

    @property
    def id(self):
        f = ("g" if self.gamma else "") + ("b" if self.beta else "") + ("" if self.grads else "-frozen")
        a = ("+add" + ("-dsum" if self.dsum else "") + (f"-p{self.p}" if self.p else "") + ("" if self.saved else "-inference")) if self.fused else ""
        return f"{self.group}-{self.kind}{a}-{NAME[self.dtype]}-{self.rows}x{self.cols}-{f or 'plain'}"


def _forward(c, o, y, mean, rstd, s):
    from mmgl_amd import _lib
    code, st, rows, cols = _lib.dtype_code(o["x"].v), _lib.stream_ptr(), c.rows, c.cols
    g, b = P(o["gamma"]), P(o["beta"])
    if c.fused and c.rms:
        _lib.call("mmgl_add_rmsnorm_fwd", None, P(o["x"]), P(o["res"]), g, P(s), P(y), P(rstd), rows, cols, EPS, code, st)
    elif c.fused:
        _lib.call("mmgl_add_layernorm_fwd", None, P(o["x"]), P(o["res"]), g, b, P(s), P(y), P(mean), P(rstd), rows, cols, EPS, c.p, DROP_SEED, code, st)
    elif c.rms:
        _lib.call("mmgl_rmsnorm_fwd", None, P(o["x"]), g, P(y), P(rstd), rows, cols, EPS, code, st)
    else:
        _lib.call("mmgl_layernorm_fwd", None, P(o["x"]), g, b, P(y), P(mean), P(rstd), rows, cols, EPS, code, st)


def _backward(c, o, s, mean, rstd, dx, dd, dg, db, ws, nbytes):
    """s: the forward's input (x, or the stored sum).  dx: LayerNorm'(dy) + dsum; dd: the dropped branch's gradient (p > 0)."""
    from mmgl_amd import _lib
    code, st, rows, cols = _lib.dtype_code(o["x"].v), _lib.stream_ptr(), c.rows, c.cols
    g, wp = P(o["gamma"]), (ws.ptr() if ws is not None else None)
    dsum = P(o["dres"]) if c.dsum else None
    if c.fused and c.rms:
        _lib.call("mmgl_add_rmsnorm_bwd", None, P(o["dy"]), dsum, P(s), g, P(rstd), P(dx), P(dg), wp, nbytes, rows, cols, code, st)
    elif c.fused:
        _lib.call("mmgl_add_layernorm_bwd", None, P(o["dy"]), dsum, P(s), g, P(mean), P(rstd), P(dx), P(dd), P(dg), P(db), wp, nbytes, rows, cols,
                  c.p, DROP_SEED, code, st)
    elif c.rms:
        _lib.call("mmgl_rmsnorm_bwd", None, P(o["dy"]), P(s), g, P(rstd), P(dx), P(dg), wp, nbytes, rows, cols, code, st)
    else:
        _lib.call("mmgl_layernorm_bwd", None, P(o["dy"]), P(s), g, P(mean), P(rstd), P(dx), P(dg), P(db), wp, nbytes, rows, cols, code, st)


def _operands(c):
    t = NormRef.inputs(c.dtype, c.rows, c.cols, seed=SEED, device="cuda", seams=c.seams)
    o = {k: operand(t[k]) for k in ("x", "dy")}
    o["gamma"] = operand(t["gamma"]) if c.gamma else None
    o["beta"] = operand(t["beta"]) if c.beta else None
    o["res"] = operand(t["res"]) if c.fused else None
    o["dres"] = operand(t["dres"]) if c.dsum else None
    return o


def _run(c, check=True):
    """Forward and backward of one case on slabs; the bounds, the guards, the restated plan.  Returns the outputs."""
    from mmgl_amd import _lib
    tpr, nv, rpb = geometry(c.dtype, c.cols)
    rows, cols = c.rows, c.cols
    nws = workspace_bytes(rows, cols)
    assert _lib.lib().mmgl_norm_bwd_workspace(rows, cols) == nws, f"{c.id}: mmgl_norm_bwd_workspace is not the restated size"
    used = used_bytes(c.dtype, rows, cols)
    assert used <= nws, f"{c.id}: the restated grid needs more partial rows than mmgl_norm_bwd_workspace promises"
    o = _operands(c)
    val = lambda k: None if o[k] is None else o[k].v
    y = output((rows, cols), c.dtype)
    mean = output((rows,), F32) if c.saved and not c.rms else None
    rstd = output((rows,), F32) if c.saved else None
    s = output((rows, cols), c.dtype) if c.fused and c.saved else None
    _forward(c, o, y, mean, rstd, s)
    torch.cuda.synchronize()
    ref = NormRef(val("x"), val("gamma"), val("beta"), rms=c.rms, eps=EPS, res=val("res"), p=c.p, seed=DROP_SEED)
    grp = f"{c.group} tpr{tpr} nv{nv} {NAME[c.dtype]}"
    outs = dict(y=y, mean=mean, rstd=rstd, s=s)
    if s is not None:
        ref.check_sum(s.v, c.id)
    if check:
        for name in ("y", "mean", "rstd"):
            if outs[name] is not None:
                ref.check(outs[name].v, name, c.id, grp)
    if c.saved:
        dx = output((rows, cols), c.dtype)
        dd = output((rows, cols), c.dtype) if c.p > 0 else None
        dg = output((cols,), F32) if c.grads else None
        db = output((cols,), F32) if c.grads and not c.rms else None
        ws = Workspace(used) if c.grads else None
        _backward(c, o, s if c.fused else o["x"], mean, rstd, dx, dd, dg, db, ws, used if c.grads else 0)
        torch.cuda.synchronize()
        ref.backward(val("dy"), val("dres"))
        outs.update(dx=dx, dx_drop=dd, dgamma=dg, dbeta=db)
        if check:
            for name in ("dx", "dx_drop", "dgamma", "dbeta"):
                if outs[name] is not None:
                    ref.check(outs[name].v, name, c.id, grp, tpr)
        assert ws is None or ws.untouched(), f"{c.id}: written past the workspace"
    for k, sl in list(o.items()) + list(outs.items()):
        assert sl is None or sl.untouched(), f"{c.id}: written outside {k}"
    return outs, ref


# ------------------------------------------------------------------------------------------ cases
CHUNKS = (1, 64, 65, 128, 129, 192, 193, 256, 257, 512, 513, 768, 769, 1024)
AFFINE = ((True, True), (True, False), (False, True), (False, False))
CASES_A = [Case("A", kind, dt, 5, n * VEC[dt], gamma=AFFINE[(i + j) % 4][0], beta=AFFINE[(i + j) % 4][1])
           for j, kind in enumerate(("ln", "rms")) for dt in (BF16, F32) for i, n in enumerate(CHUNKS)]
CASES_A += [Case("A", kind, dt, 5, n * VEC[dt], grads=False) for kind in ("ln", "rms") for dt in (BF16, F32) for n in (1, 257, 1024)]
S64, S256 = (4 * MAXBLK, 4 * FWD_MAXBLK), (MAXBLK, FWD_MAXBLK)          # grid-stride seams of the two geometries: backward, forward
CASES_B = ([Case("B", kind, dt, rows, 65 * VEC[dt]) for kind in ("ln", "rms") for dt in (BF16, F32) for rows in (1, 3, 125)]
           + [Case("B", kind, dt, rows, 257 * VEC[dt]) for kind in ("ln", "rms") for dt in (BF16, F32) for rows in (1, 3)]
           + [Case("B", kind, dt, 2053, 65 * VEC[dt], seams=S64) for kind in ("ln", "rms") for dt in (BF16, F32)]
           + [Case("B", kind, dt, 517, 257 * VEC[dt], seams=S256) for kind in ("ln", "rms") for dt in (BF16, F32)]
           + [Case("B", kind, BF16, 32773, 8, seams=S64, grads=gr) for kind in ("ln", "rms") for gr in (True, False)]
           + [Case("B", "ln", BF16, 8197, 2056, seams=S256, grads=False), Case("B", "rms", BF16, 8197, 2056, seams=S256)])
CASES_C = ([Case("C", kind, dt, rows, cols * VEC[dt] // 8, fused=True, dsum=ds)
            for kind in ("ln", "rms") for dt in (BF16, F32) for rows, cols in ((5, 520), (37, 2056)) for ds in (True, False)]
           + [Case("C", "ln", dt, rows, cols * VEC[dt] // 8, fused=True, dsum=ds, p=0.3, gamma=ga)
              for dt in (BF16, F32) for (rows, cols), ds, ga in (((5, 520), True, True), ((37, 2056), False, True), ((125, 8), True, False))]
           + [Case("C", "ln", dt, 37, 2056 * VEC[dt] // 8, fused=True, p=p, saved=False) for dt in (BF16, F32) for p in (0.0, 0.3)])
EVERY = CASES_A + CASES_B + CASES_C


def test_case_list_reaches_every_branch():
    """On the case list itself (the per-case checks hold the restated plan against the library)."""
    seen = {(c.dtype, c.kind) + geometry(c.dtype, c.cols)[:2] for c in CASES_A if c.grads}
    for dt in (BF16, F32):
        for kind in ("ln", "rms"):
            assert {k[2:] for k in seen if k[:2] == (dt, kind)} == {(64, 1), (64, 2), (64, 3), (64, 4), (256, 2), (256, 3), (256, 4)}
    for kind in ("ln", "rms"):
        a = [c for c in CASES_A if c.kind == kind and c.grads]
        assert {(c.gamma, c.beta) for c in a} == ({(True, False), (False, False)} if kind == "rms" else set(AFFINE))
    assert any(not c.grads and geometry(c.dtype, c.cols)[0] == t for c in CASES_A for t in (64,)) and any(not c.grads and geometry(c.dtype, c.cols)[0] == 256 for c in CASES_A)
    b = CASES_B
    assert any(c.rows < 4 and geometry(c.dtype, c.cols)[2] == 4 for c in b) and any(c.rows % 4 for c in b)
    for t in (64, 256):
        rpb = 256 // t
        assert any(geometry(c.dtype, c.cols)[0] == t and c.grads and -(-c.rows // rpb) > MAXBLK and c.rows % (MAXBLK * rpb) for c in b)      # capped, ragged second trip
        assert any(geometry(c.dtype, c.cols)[0] == t and -(-c.rows // rpb) > FWD_MAXBLK for c in b)
        assert any(geometry(c.dtype, c.cols)[0] == t and not c.grads and -(-c.rows // rpb) > FWD_MAXBLK for c in b)
    assert {(c.kind, c.dsum) for c in CASES_C if c.saved and not c.p} == {("ln", True), ("ln", False), ("rms", True), ("rms", False)}
    assert any(c.p > 0 and c.rows * c.cols > c.cols for c in CASES_C) and any(not c.saved for c in CASES_C)
    assert len({c.id for c in EVERY}) == len(EVERY)
    # the chain of the parameter gradients' bound restates the same grid
    for c in EVERY:
        tpr, _, rpb = geometry(c.dtype, c.cols)
        parts = bwd_blocks(c.rows, rpb) * rpb
        assert NormRef.chain(c.rows, tpr) == -(-c.rows // parts) + -(-parts // 8) + 16, c.id


@pytest.mark.parametrize("case", CASES_A, ids=lambda c: c.id)
def test_A_every_dispatch_branch(case):
    _run(case)


@pytest.mark.parametrize("case", CASES_B, ids=lambda c: c.id)
def test_B_rows(case):
    _run(case)


@pytest.mark.parametrize("case", CASES_C, ids=lambda c: c.id)
def test_C_fused_pairs(case):
    outs, ref = _run(case)
    if case.p > 0:
        keep = ref.keep
        assert 0.6 < keep.double().mean().item() < 0.8
        if case.saved:              # the dropped branch's gradient is zero exactly where the independent mask says so
            assert bool((outs["dx_drop"].v[~keep] == 0).all()), f"{case.id}: a dropped element has a gradient"


def test_C_element_index_past_2_31():
    """mmgl_add_layernorm_fwd with p_drop = 0.3 over 262147 x 8192 bf16 elements (33 grid-stride trips of 8192 blocks): the stored sum,
    bit for bit against hash_keep, and y, mean, rstd on the first rows, across the first grid-stride seam and on the rows either side of element index 2^31
    (the reference of a slice takes its mask from the slice's first element index).  Forward only, operands drawn on the device:
    four 4 GiB tensors, a fraction of a second."""
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr
    rows, cols = 262147, 8192
    assert rows * cols > 2 ** 31 + 2 * cols and geometry(BF16, cols) == (256, 4, 1)
    g = torch.Generator(device="cuda").manual_seed(SEED)
    x = torch.randn(rows, cols, generator=g, device="cuda", dtype=BF16)
    res = torch.randn(rows, cols, generator=g, device="cuda", dtype=BF16)
    gamma, beta = torch.randn(cols, generator=g, device="cuda", dtype=BF16), torch.randn(cols, generator=g, device="cuda", dtype=BF16)
    s, y = torch.full_like(x, CANARY), torch.full_like(x, CANARY)
    mean, rstd = output((rows,), F32), output((rows,), F32)
    _lib.call("mmgl_add_layernorm_fwd", None, ptr(x), ptr(res), ptr(gamma), ptr(beta), ptr(s), ptr(y), P(mean), P(rstd), rows, cols, EPS, 0.3, DROP_SEED,
              _lib.dtype_code(x), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert mean.untouched() and rstd.untouched()
    for r0, r1 in ((0, 3), (8191, 8194), (262143, 262147)):
        ref = NormRef(x[r0:r1], gamma, beta, eps=EPS, res=res[r0:r1], p=0.3, seed=DROP_SEED, mask_row_shift=r0)
        what = f"C-ln+add-p0.3-bf16-{rows}x{cols}-rows{r0}:{r1}"
        ref.check_sum(s[r0:r1], what)
        for name, got in (("y", y[r0:r1]), ("mean", mean.v[r0:r1]), ("rstd", rstd.v[r0:r1])):
            ref.check(got, name, what, "C tpr256 nv4 bf16")
    assert not bool((s[::4099] == CANARY).all(1).any()) and not bool((y[::4099] == CANARY).all(1).any())       # every sampled row was written


# ------------------------------------------------------------------------------------------ D: the compact copy
@pytest.mark.parametrize("fused,p", [(False, 0.0), (True, 0.0), (True, 0.3)], ids=["tiles", "add-tiles", "add-tiles-p0.3"])
@pytest.mark.parametrize("dtype,cols", [(BF16, 520), (F32, 1028)], ids=["bf16-520", "f32-1028"])
def test_D_compact_copy(dtype, cols, fused, p):
    from mmgl_amd import _lib
    rows, crows = 9, 6
    tpr, nv, _ = geometry(dtype, cols)
    t = NormRef.inputs(dtype, rows, cols, seed=SEED, device="cuda")
    o = {k: operand(t[k]) for k in ("x", "gamma", "beta", "res")}
    rowmap = torch.tensor([2, -1, 0, 6, 4, -1, 100, 1, -5], dtype=torch.int32, device="cuda")       # -1, >= crows: no copy; yc rows 3, 5 unnamed
    y, yc, s = output((rows, cols), dtype), output((crows, cols), dtype), output((rows, cols), dtype)
    mean, rstd = output((rows,), F32), output((rows,), F32)
    code, st = _lib.dtype_code(t["x"]), _lib.stream_ptr()
    if fused:
        _lib.call("mmgl_add_layernorm_tiles_fwd", None, P(o["x"]), P(o["res"]), P(o["gamma"]), P(o["beta"]), P(s), P(y), P(yc), _lib.ptr(rowmap),
                  P(mean), P(rstd), rows, cols, crows, EPS, p, DROP_SEED, code, st)
    else:
        _lib.call("mmgl_layernorm_tiles_fwd", None, P(o["x"]), P(o["gamma"]), P(o["beta"]), P(y), P(yc), _lib.ptr(rowmap), P(mean), P(rstd), rows, cols,
                  crows, EPS, code, st)
    torch.cuda.synchronize()
    what = f"D-{'add-' if fused else ''}tiles-{NAME[dtype]}-{rows}x{cols}" + (f"-p{p}" if p else "")
    ref = NormRef(o["x"].v, o["gamma"].v, o["beta"].v, eps=EPS, res=o["res"].v if fused else None, p=p, seed=DROP_SEED)
    if fused:
        ref.check_sum(s.v, what)
    else:
        assert s.unwritten()
    for name, got in (("y", y), ("mean", mean), ("rstd", rstd)):
        ref.check(got.v, name, what, f"D tpr{tpr} nv{nv} {NAME[dtype]}")
    named = {}
    for r, cr in enumerate(rowmap.tolist()):
        if 0 <= cr < crows:
            named[cr] = r
    assert sorted(named) == [0, 1, 2, 4]
    for cr in range(crows):
        if cr in named:
            assert torch.equal(yc.v[cr], y.v[named[cr]]), f"{what}: compact row {cr} is not y row {named[cr]}"
        else:
            assert bool((yc.v[cr] == CANARY).all()), f"{what}: compact row {cr} is named by no map entry and was written"
    for sl in list(o.values()) + [y, yc, s, mean, rstd]:
        assert sl.untouched(), what


# ------------------------------------------------------------------------------------------ E: determinism
@pytest.mark.parametrize("case", [Case("E", "ln", BF16, 517, 2056, seams=S256), Case("E", "rms", F32, 2053, 260, seams=S64),
                                  Case("E", "ln", BF16, 125, 520, fused=True, p=0.3), Case("E", "rms", BF16, 3, 1032, fused=True),
                                  Case("E", "ln", F32, 5, 4096, grads=False)], ids=lambda c: c.id)
def test_E_two_launches_bit_equal(case):
    a, _ = _run(case)
    b, _ = _run(case, check=False)
    for k in a:
        assert (a[k] is None) == (b[k] is None)
        if a[k] is not None:
            assert torch.equal(a[k].buf, b[k].buf), f"{case.id}: {k} differs between two launches"


# ------------------------------------------------------------------------------------------ F: refusals
def _refused(c, match, forward=True, backward=True, nbytes=None, p=None):
    """Both directions of case c are refused with `match` before any launch: every output keeps its canary."""
    o = _operands(c)
    rows, cols = c.rows, c.cols
    y, s, dx, dd = (output((rows, cols), c.dtype) for _ in range(4))
    mean, rstd, dg, db = output((rows,), F32), output((rows,), F32), output((cols,), F32), output((cols,), F32)
    mean.v.zero_(), rstd.v.fill_(1.0)
    ws = Workspace(workspace_bytes(rows, cols))
    if p is not None:
        c.p = p
    if forward:
        with pytest.raises(ValueError, match=match):
            _forward(c, o, y, mean if not c.rms else None, rstd, s if c.fused else None)
    if backward:
        with pytest.raises(ValueError, match=match):
            _backward(c, o, o["x"], mean if not c.rms else None, rstd, dx, dd if c.p > 0 else None, dg, db if not c.rms else None, ws,
                      ws.nbytes if nbytes is None else nbytes)
    torch.cuda.synchronize()
    for name, sl in dict(y=y, s=s, dx=dx, dd=dd, dg=dg, db=db, ws=ws).items():
        assert sl.unwritten(), f"{c.id}: {name} written by a refused call"
    assert mean.untouched() and rstd.untouched()


@pytest.mark.parametrize("kind,fused", [("ln", False), ("rms", False), ("ln", True), ("rms", True)])
@pytest.mark.parametrize("dtype,cols,match", [(BF16, 1004, "multiple of 8"), (F32, 1002, "multiple of 4"), (BF16, 8200, "register-resident"),
                                             (F32, 4100, "register-resident")], ids=["bf16-1004", "f32-1002", "bf16-8200", "f32-4100"])
def test_F_cols_refused(dtype, cols, match, kind, fused):
    with pytest.raises(ValueError):
        geometry(dtype, cols)
    _refused(Case("F", kind, dtype, 5, cols, fused=fused), match)


@pytest.mark.parametrize("kind,fused", [("ln", False), ("rms", False), ("ln", True), ("rms", True)])
@pytest.mark.parametrize("dtype,rows,cols", [(BF16, 5, 520), (BF16, 5, 2056), (F32, 7, 1028), (F32, 2053, 260)])
def test_F_workspace_one_byte_short(dtype, rows, cols, kind, fused):
    """One byte less than blocks x rows per block partial rows of the restated grid; that size itself is what every other case runs with.
    (5 rows on a TPR = 256 shape use 5 partial rows where mmgl_norm_bwd_workspace promises 8: a wrong restated geometry shows here.)"""
    _refused(Case("F", kind, dtype, rows, cols, fused=fused), "workspace too small", forward=False, nbytes=used_bytes(dtype, rows, cols) - 1)


def test_F_p_drop_1_and_crows_past_rows():
    from mmgl_amd import _lib
    _refused(Case("F", "ln", BF16, 5, 520, fused=True), "outside", p=1.0)
    rows, cols = 5, 520
    t = NormRef.inputs(BF16, rows, cols, seed=SEED, device="cuda")
    rowmap = torch.zeros(rows, dtype=torch.int32, device="cuda")
    y, yc, s, mean, rstd = output((rows, cols), BF16), output((rows + 1, cols), BF16), output((rows, cols), BF16), output((rows,), F32), output((rows,), F32)
    code, st = _lib.dtype_code(t["x"]), _lib.stream_ptr()
    with pytest.raises(ValueError, match="crows"):
        _lib.call("mmgl_layernorm_tiles_fwd", None, _lib.ptr(t["x"]), _lib.ptr(t["gamma"]), _lib.ptr(t["beta"]), P(y), P(yc), _lib.ptr(rowmap), P(mean),
                  P(rstd), rows, cols, rows + 1, EPS, code, st)
    with pytest.raises(ValueError, match="crows"):
        _lib.call("mmgl_add_layernorm_tiles_fwd", None, _lib.ptr(t["x"]), _lib.ptr(t["res"]), _lib.ptr(t["gamma"]), _lib.ptr(t["beta"]), P(s), P(y), P(yc),
                  _lib.ptr(rowmap), P(mean), P(rstd), rows, cols, rows + 1, EPS, 0.0, DROP_SEED, code, st)
    torch.cuda.synchronize()
    for sl in (y, yc, s, mean, rstd):
        assert sl.unwritten()
