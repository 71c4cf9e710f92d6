"""-m gpu: mmgl_gemm_nt and the mask-bits pair (csrc/gemm8p.hip, gemm_mid.hip, gemm.hip) against gemm_ref.GemmRef -- an fp64 reference of
the storage-rounded operands -- element by element: |got - want| <= u |want| + L c mag + E + staged (the count is in GemmRef's
docstring; tests/test_gemm_ref_cpu.py shows on the CPU that this comparison fails for a lost or doubled K unit or K split, a bias line
of another tile, a tail-row offset, a scale on the wrong side of the activation, a transposed operand).  The entry points are called
directly, with a workspace of exactly mmgl_gemm_nt_workspace bytes.

The plans of csrc/gemm.hip and csrc/gemm8p.hip are restated in tests/gemm_ref.py (nt_route, gemm8p_plan, gemm8p_row_split,
gemm8p_use_splits, gemm8p_supported, gemm_mid_supported; the CU count from the device properties) and every case holds the restated
route and scratch size against mmgl_gemm_nt_fast, mmgl_gemm_nt_workspace and mmgl_gemm_nt_relu_bits_bytes, so a change to the plans fails loudly instead
of quietly moving the cases off the routes they were chosen for.  The shapes are the smallest that reach each route on 256 CUs:

  A  whole 256x256 tiles on the persistent kernel: two and three K units, ragged last tile row / column (240 and 16 columns), every
     workgroup's second tile (352 tiles), strided x, W and y, every instantiated (activation, zmask / residual) epilogue; erf-GELU
     with zmask / residual is refused before any launch
  B  row split: whole rounds on the persistent kernel, the tail rows on the 128x128 kernel, bias + zmask + residual so that the tail's
     offsets matter; a ragged tail; two rounds; a ragged last column tile in both parts (N = 8176: the 33 tile columns of N = 8208
     divide no round, that shape stays on whole tiles and is checked as such)
  C  remainder of a round as K splits (264 tiles: 256 whole, 8 as 3 splits of 4 units), ragged M, every epilogue stage in the finish
     kernel; K = 1408, one unit short, does not split
  D  few-tile K splits: 24 tiles as 8 splits of 3 units, 80 tiles as 3 uneven splits of 32 units, a ragged last column tile with the
     zmask in the finish kernel; 23 tiles, K = 2944 and 64 tiles at K = 3072 go to the 128x128 kernel; without scratch the
     persistent kernel runs unsplit (mmgl_gemm_nt plans with K splits for every caller; the route without them is mmgl_linear_fwd's:
     tests/test_linear_bwd_bounds_gpu.py)
  E  128x128 kernel: M in {127, 128, 129} x N in {120, 128, 136} (N = 127 / 129 are no multiple of 4: refused), N = 8, K = 64, 128,
     192, strided operands
  F  composed route (launch_nt128 + activation, zmask and residual passes: the staged bound): bf16 with K = 72 and 200, an [M, N] that
     is no whole number of 16-byte chunks, fp32 at 300 x 96 x 64 and 129 x 132 x 100, every activation; a strided operand is refused
  G  padded contraction on the persistent kernel: x rows of 304 elements (a row stride must be a multiple of 8), K = 384 against
     zero columns of W, NaN right after x's last row
  H  mask bits: mmgl_gemm_nt_relu_bits with the bound, mmgl_gemm_nt_masked of a second operand pair against where(y > 0, want, 0)
     with y the first call's stored output; both refused for a few-tile shape
  I  isolation and determinism: operands carved out of NaN slabs with ld > K, outputs (ldy > N) and the exactly sized workspace out of
     canary slabs that come back untouched, two launches bit-equal
  J  dynamic tile schedule: one case each of A, B and C bit-equal to the static result, counters left at zero"""
import pytest
import torch

from bounds import BF16, CANARY_BYTE, F32, NAME, NAN, NAN_BYTE, Slab
from gemm_ref import (FAST, MID, P8, P8_FEW, P8_REM, P8_ROWS, TILE128, GemmRef, bits_bytes, cdiv, detail, gemm8p_plan, gemm8p_row_split, nt_route,
                      num_cu, workspace_bytes)

pytestmark = pytest.mark.gpu

SEED = 0                    # tests/test_gemm_ref_cpu.py: every wrong reference leaves the bound on >= 25 % at this seed


# ------------------------------------------------------------------------------------------ cases
class Case:
    def __init__(self, group, route, M, N, K, act=0, bias=False, resid=False, zmask=False, scale=1.0, dtype=BF16, pad=(0, 0, 0), scratch=True):
        self.group, self.route, self.M, self.N, self.K, self.act, self.bias, self.resid, self.zmask = group, route, M, N, K, act, bias, resid, zmask
        self.scale, self.dtype, self.pad, self.scratch = scale, dtype, pad, scratch
        self.ld = (K + pad[0], K + pad[1], N + pad[2])

    @property
    def id(self):
        e = f"a{self.act}" + ("b" if self.bias else "") + ("z" if self.zmask else "") + ("r" if self.resid else "") + (f"-s{self.scale}" if self.scale != 1 else "")
        return (f"{self.group}-{NAME[self.dtype]}-{self.M}x{self.N}x{self.K}-{e}" + ("-strided" if any(self.pad) else "")
                + ("" if self.scratch else "-noscratch"))


C = Case
ALL = dict(bias=True, zmask=True, resid=True)
A0 = (2560, 4096, 256)
CASES_A = [
    C("A", P8, *A0), C("A", P8, *A0, act=0, bias=True, zmask=True, scale=0.125), C("A", P8, *A0, act=0, bias=True, resid=True),
    C("A", P8, *A0, act=1, bias=True), C("A", P8, *A0, act=1, bias=True, resid=True), C("A", P8, *A0, act=1, scale=0.125, **ALL),
    C("A", P8, *A0, act=2, bias=True, scale=0.125), C("A", P8, *A0, act=3, bias=True), C("A", P8, *A0, act=3, zmask=True),
    C("A", P8, *A0, act=3, scale=0.125, **ALL), C("A", P8, *A0, act=4, bias=True), C("A", P8, *A0, act=4, scale=0.125),
    C("A", P8, *A0, act=4, bias=True, zmask=True), C("A", P8, *A0, act=4, **ALL),
    C("A", P8, 2560, 4096, 384, act=3, bias=True, resid=True),                      # an odd number of K units
    C("A", P8, 2500, 4080, 256, act=0, bias=True, zmask=True, scale=0.125),         # ragged last tile row, last tile 240 columns wide
    C("A", P8, 2500, 3856, 256, act=2, bias=True),                                  # 16 columns in the last tile
    C("A", P8, 2816, 8192, 256, act=4, bias=True, scale=0.125),                     # 352 tiles: every workgroup's second tile, rem = 96
    C("A", P8, 2816, 8192, 256, act=1, **ALL),
    C("A", P8, 2560, 8208, 256, act=0, **ALL),                                      # 330 tiles, 33 tile columns: no row split
    C("A", P8, *A0, act=0, pad=(64, 128, 64), **ALL), C("A", P8, 2500, 4080, 384, act=1, bias=True, pad=(8, 8, 8)),
]
CASES_B = [
    C("B", P8_ROWS, 2560, 8192, 256, act=1, scale=0.125, **ALL),                    # 2048 rows + 512 on the 128x128 kernel
    C("B", P8_ROWS, 2400, 8192, 256, act=0, **ALL),                                 # ragged tail of 352 rows
    C("B", P8_ROWS, 4352, 8192, 256, act=3, **ALL),                                 # two rounds + 256 rows
    C("B", P8_ROWS, 2560, 8176, 256, act=4, scale=0.125, **ALL),                    # last column tile 240 wide in both parts
    C("B", P8_ROWS, 2400, 8192, 384, act=0, pad=(8, 16, 16), **ALL),
]
C0 = (5632, 3072, 1536)
CASES_C = [
    C("C", P8_REM, *C0, act=0, bias=True), C("C", P8_REM, 5400, 3072, 1536, act=1, resid=True),
    C("C", P8_REM, *C0, act=3, scale=0.125, **ALL), C("C", P8_REM, 5400, 3072, 1536, act=4, bias=True, scale=0.125),
    C("C", P8, 5632, 3072, 1408, act=1, **ALL),                                     # 11 units: one short of 3 splits of 4
    C("C", P8, *C0, act=0, bias=True, scratch=False),                               # no scratch: nothing is split
]
CASES_D = [
    C("D", P8_FEW, 1536, 1024, 3072, act=1, bias=True), C("D", P8_FEW, 1536, 1024, 3072, act=2, scale=0.125, **ALL),
    C("D", P8_FEW, 2560, 2048, 4096, act=3, bias=True, resid=True),                 # 32 units over 3 splits: 11, 11, 10
    C("D", P8_FEW, 2560, 2064, 4096, act=0, zmask=True),
    C("D", P8_FEW, 2500, 2064, 4096, act=4, scale=0.125, **ALL),
    C("D", MID, 5888, 256, 3072, act=1, bias=True),                                 # 23 tiles
    C("D", MID, 1536, 1024, 2944, act=0, **ALL),                                    # 23 units
    C("D", MID, 2048, 2048, 3072, act=3, bias=True),                                # 64 tiles below 32 units
    C("D", P8, 1536, 1024, 3072, act=1, bias=True, scratch=False),                  # no scratch: the persistent kernel, unsplit
]
EPI_E = [dict(act=1, **ALL), dict(act=0, bias=True), dict(act=2, zmask=True, scale=0.125), dict(act=3, resid=True), dict(act=4, bias=True, scale=0.125),
         dict(act=0), dict(act=4, **ALL), dict(act=2, bias=True), dict(act=3, bias=True, zmask=True, scale=0.125)]
CASES_E = ([C("E", MID, M, N, 128, **EPI_E[(3 * i + j) % len(EPI_E)]) for i, M in enumerate((127, 128, 129)) for j, N in enumerate((120, 128, 136))]
           + [C("E", MID, 300, 8, 64, act=1, **ALL), C("E", MID, 129, 136, 64, act=2, **ALL), C("E", MID, 129, 136, 192, act=3, **ALL),
              C("E", MID, 300, 136, 192, act=4, pad=(8, 72, 24), **ALL), C("E", MID, 129, 120, 64, act=0, bias=True, pad=(64, 0, 8))])
CASES_F = ([C("F", TILE128, 129, 132, K, act=a, scale=0.125, **ALL) for K in (72, 200) for a in (0, 1, 2, 3, 4)]
           + [C("F", TILE128, 129, 132, 72, act=0, zmask=True), C("F", TILE128, 300, 96, 200, act=2, bias=True), C("F", TILE128, 300, 96, 72, act=3, resid=True)]
           + [C("F", TILE128, M, N, K, act=a, scale=0.125, dtype=F32, **ALL) for M, N, K in ((300, 96, 64), (129, 132, 100)) for a in (0, 1, 2, 3, 4)]
           + [C("F", TILE128, 129, 132, 100, act=4, bias=True, dtype=F32), C("F", TILE128, 300, 96, 64, act=1, zmask=True, dtype=F32)])
EVERY = CASES_A + CASES_B + CASES_C + CASES_D + CASES_E + CASES_F


def _alloc(rows, cols, ld, dtype, src=None):
    """[rows, cols] with row stride ld; what lies between the rows is NaN."""
    buf = torch.full((rows, ld), float("nan"), dtype=dtype, device="cuda")
    v = buf[:, :cols]
    if src is not None:
        v.copy_(src)
    return v


def _operands(c):
    t = GemmRef.inputs(c.dtype, c.M, c.N, c.K, seed=SEED, device="cuda")
    ldx, ldw, ldy = c.ld
    x, w = _alloc(c.M, c.K, ldx, c.dtype, t["x"]), _alloc(c.N, c.K, ldw, c.dtype, t["w"])
    r = _alloc(c.M, c.N, ldy, c.dtype, t["residual"]) if c.resid else None
    z = _alloc(c.M, c.N, ldy, c.dtype, t["zmask"]) if c.zmask else None
    return x, w, (t["bias"] if c.bias else None), r, z


def _plan_checks(c):
    """The restated plan against the ABI's answers; returns (route detail, K splits, workspace bytes)."""
    from mmgl_amd import _lib
    L, G, code = _lib.lib(), num_cu(), _lib.BF16 if c.dtype == BF16 else _lib.F32
    dims = (c.M, c.N, c.K) + c.ld
    route, s = detail(*dims, c.dtype, c.scratch, G)
    assert route == c.route, f"{c.id}: the restated plan sends this case to {route}, it was chosen for {c.route}"
    assert L.mmgl_gemm_nt_fast(*dims, code) == FAST[route], f"{c.id}: mmgl_gemm_nt_fast is not the restated route's"
    nws = workspace_bytes(*dims, c.dtype, G)
    assert L.mmgl_gemm_nt_workspace(*dims, code) == nws, f"{c.id}: mmgl_gemm_nt_workspace is not the restated plan's"
    assert L.mmgl_gemm_nt_relu_bits_bytes(*dims, code) == bits_bytes(*dims, c.dtype, G), f"{c.id}: mmgl_gemm_nt_relu_bits_bytes"
    assert (nws > 0) == (route in (P8_REM, P8_FEW) or (route == P8 and not c.scratch and gemm8p_plan(c.M, c.N, c.K, G)[1] > 0)), c.id
    return route, s, nws if c.scratch else 0


def _gemm(c, x, w, b, r, z, y, ws, nws):
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr
    _lib.call("mmgl_gemm_nt", None, ptr(x), x.stride(0), ptr(w), w.stride(0), ptr(b), ptr(r), ptr(z), ptr(y), y.stride(0), c.M, c.N, c.K, c.act,
              float(c.scale), ptr(ws), nws, _lib.dtype_code(x), _lib.stream_ptr())


def _bound_kw(c, route, s):
    kw = dict(n=GemmRef.chain(c.dtype, c.K, s))
    if route == TILE128:
        kw.update(composed=True, has_act_pass=c.act > 1, has_residual_pass=c.resid)
    return kw


def _check(c):
    route, s, nws = _plan_checks(c)
    x, w, b, r, z = _operands(c)
    y = _alloc(c.M, c.N, c.ld[2], c.dtype)
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device="cuda") if nws else None
    _gemm(c, x, w, b, r, z, y, ws, nws)
    torch.cuda.synchronize()
    ref = GemmRef.forward(x, w, b, c.act, c.scale, r, z)
    ref.check(y, c.id, f"{c.group} {route} {NAME[c.dtype]}", **_bound_kw(c, route, s))
    return (x, w, b, r, z), y, ref


def test_case_list_reaches_every_route_and_threshold_side():
    """On the case list itself (the per-case checks hold each restated route against the library)."""
    G = num_cu()
    assert G == 256, f"the shapes were derived for 256 CUs, this device has {G}"
    seen = {}
    for c in EVERY:
        route, s = detail(c.M, c.N, c.K, *c.ld, c.dtype, c.scratch, G)
        assert route == c.route, c.id
        seen.setdefault(route, []).append((c, s))
    assert set(seen) == {P8, P8_ROWS, P8_REM, P8_FEW, MID, TILE128}
    # every (route, epilogue stage) pair; erf-GELU with zmask / residual is not instantiated on the persistent kernel's whole tiles
    for route, cs in seen.items():
        acts = {c.act for c, _ in cs}
        assert acts >= ({0, 1, 3, 4} if route in (P8_ROWS, P8_REM) else {0, 1, 2, 3, 4}), (route, acts)
        for stage in ("bias", "zmask", "resid"):
            assert any(getattr(c, stage) for c, _ in cs) and any(not getattr(c, stage) for c, _ in cs) or route in (P8_ROWS,), (route, stage)
    for act in (1, 3, 4):
        assert any(c.act == act and (c.zmask or c.resid) for c, _ in seen[P8]) and any(c.act == act and not (c.zmask or c.resid) for c, _ in seen[P8])
    # the plan properties the shapes were chosen for
    p8 = [c for c, _ in seen[P8]]
    assert any(c.K == 256 for c in p8) and any(c.K // 128 % 2 for c in p8)
    assert any(c.M % 256 and c.N % 256 == 240 for c in p8) and any(c.N % 256 == 16 for c in p8)
    assert any(cdiv(c.M, 256) * cdiv(c.N, 256) > G and gemm8p_plan(c.M, c.N, c.K, G)[1] == 0 for c in p8)           # second tiles, nothing split
    assert any(any(c.pad) for c in p8) and any(any(c.pad) for c, _ in seen[P8_ROWS]) and any(any(c.pad) for c, _ in seen[MID])
    rows = {c.id: gemm8p_row_split(c.M, c.N, c.K, *c.ld, G) for c, _ in seen[P8_ROWS]}
    assert set(rows.values()) == {2048, 4096}
    assert any((c.M - gemm8p_row_split(c.M, c.N, c.K, *c.ld, G)) % 128 for c, _ in seen[P8_ROWS]) and any(c.N % 256 for c, _ in seen[P8_ROWS])
    assert {(gemm8p_plan(c.M, c.N, c.K, G), s) for c, s in seen[P8_REM]} == {((256, 3), 3)} and any(c.M % 256 for c, _ in seen[P8_REM])
    assert {(cdiv(c.M, 256) * cdiv(c.N, 256), c.K // 128, s) for c, s in seen[P8_FEW]} == {(24, 24, 8), (80, 32, 3), (90, 32, 3)}
    sides = {(cdiv(c.M, 256) * cdiv(c.N, 256), c.K // 128) for c, _ in seen[MID] if c.group == "D"}
    assert sides == {(23, 24), (24, 23), (64, 24)}
    assert any(c.K == 1408 and c.route == P8 for c in CASES_C) and any(not c.scratch for c in CASES_C + CASES_D)
    f = [c for c, _ in seen[TILE128]]
    assert {c.K for c in f if c.dtype == BF16} == {72, 200} and {(c.M, c.N, c.K) for c in f if c.dtype == F32} == {(300, 96, 64), (129, 132, 100)}
    assert any(c.dtype == BF16 and c.zmask and (c.M * c.N) % 8 for c in f)


@pytest.mark.parametrize("case", CASES_A, ids=lambda c: c.id)
def test_A_whole_tiles(case):
    _check(case)


@pytest.mark.parametrize("zmask,resid", [(True, False), (False, True)])
def test_A_erf_gelu_with_zmask_or_residual_is_refused(zmask, resid):
    """Not instantiated on the persistent kernel: an error before any launch, the output untouched."""
    c = Case("A", P8, *A0, act=2, bias=True, zmask=zmask, resid=resid)
    _plan_checks(c)
    x, w, b, r, z = _operands(c)
    y = _alloc(c.M, c.N, c.N, c.dtype)
    with pytest.raises(ValueError, match="not instantiated"):
        _gemm(c, x, w, b, r, z, y, None, 0)
    torch.cuda.synchronize()
    assert torch.isnan(y).all(), "written by a refused call"


@pytest.mark.parametrize("case", CASES_B, ids=lambda c: c.id)
def test_B_row_split(case):
    _check(case)


@pytest.mark.parametrize("case", CASES_C, ids=lambda c: c.id)
def test_C_remainder_of_a_round_as_k_splits(case):
    _check(case)


@pytest.mark.parametrize("case", CASES_D, ids=lambda c: c.id)
def test_D_few_tile_k_splits(case):
    _check(case)


@pytest.mark.parametrize("case", CASES_E, ids=lambda c: c.id)
def test_E_128_kernel(case):
    _check(case)


@pytest.mark.parametrize("N", [127, 129])
def test_E_columns_no_multiple_of_4_are_refused(N):
    c = Case("E", TILE128, 128, N, 128, bias=True)
    x, w, b, r, z = _operands(c)
    y = _alloc(c.M, c.N, c.N, c.dtype)
    with pytest.raises(ValueError, match="multiple"):
        _gemm(c, x, w, b, r, z, y, None, 0)
    torch.cuda.synchronize()
    assert torch.isnan(y).all(), "written by a refused call"


@pytest.mark.parametrize("case", CASES_F, ids=lambda c: c.id)
def test_F_composed_route(case):
    _check(case)


@pytest.mark.parametrize("dtype,K", [(BF16, 72), (F32, 64)], ids=["bf16", "f32"])
def test_F_strided_operand_is_refused(dtype, K):
    c = Case("F", TILE128, 129, 132, K, act=3, dtype=dtype, pad=(8, 0, 0), **ALL)
    assert nt_route(c.M, c.N, c.K, *c.ld, dtype, True, num_cu()) == TILE128
    x, w, b, r, z = _operands(c)
    y = _alloc(c.M, c.N, c.N, c.dtype)
    with pytest.raises(ValueError, match="strided"):
        _gemm(c, x, w, b, r, z, y, None, 0)
    torch.cuda.synchronize()
    assert torch.isnan(y).all(), "written by a refused call"


# ------------------------------------------------------------------------------------------ G: padded contraction
def test_G_padded_contraction_on_the_persistent_kernel():
    """K past x's row length against zero columns of W (mmgl_gemm_nt's contract, the lm_head dgrad's trick): a row's tail reads the
    head of the next row (times zero), the LAST row's tail must not read past the tensor (NaN planted there)."""
    M, N, K0, K = 2560, 4096, 304, 384
    G = num_cu()
    assert detail(M, N, K, K0, K, N, BF16, True, G) == (P8, 0)
    t = GemmRef.inputs(BF16, M, N, K0, seed=SEED, device="cuda")
    buf = torch.full((M + 1, K0), float("nan"), device="cuda", dtype=BF16)
    buf[:M] = t["x"]
    x = buf[:M]
    w = torch.zeros(N, K, device="cuda", dtype=BF16)
    w[:, :K0] = t["w"]
    c = Case("G", P8, M, N, K, act=1, bias=True)
    y = _alloc(M, N, N, BF16)
    _gemm(c, x, w, t["bias"], None, None, y, None, 0)
    torch.cuda.synchronize()
    GemmRef.forward(x, w, t["bias"], 1, K=K0).check(y, f"G-{M}x{N}x{K}-rows-of-{K0}", f"G {P8} bf16", n=GemmRef.chain(BF16, K))


# ------------------------------------------------------------------------------------------ H: mask bits
def _bits_calls(M, N, K, K2, x, w, b, dy, w2, y, dh, bits):
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr
    _lib.call("mmgl_gemm_nt_relu_bits", None, ptr(x), x.stride(0), ptr(w), w.stride(0), ptr(b), ptr(y), y.stride(0), ptr(bits), M, N, K, 1.0,
              _lib.BF16, _lib.stream_ptr())
    _lib.call("mmgl_gemm_nt_masked", None, ptr(dy), dy.stride(0), ptr(w2), w2.stride(0), ptr(bits), ptr(dh), dh.stride(0), M, N, K2, 1.0,
              _lib.BF16, _lib.stream_ptr())


@pytest.mark.parametrize("M,N", [(2560, 4096), (2500, 4080)])
def test_H_mask_bits(M, N):
    from mmgl_amd import _lib
    K, K2, G = 256, 384, num_cu()
    nb = bits_bytes(M, N, K, K, K, N, BF16, G)
    assert nb == cdiv(M, 256) * cdiv(N, 256) * 8192 == _lib.lib().mmgl_gemm_nt_relu_bits_bytes(M, N, K, K, K, N, _lib.BF16)
    assert bits_bytes(M, N, K2, K2, K2, N, BF16, G) == nb
    t, t2 = GemmRef.inputs(BF16, M, N, K, seed=SEED, device="cuda"), GemmRef.inputs(BF16, M, N, K2, seed=SEED + 1, device="cuda")
    y, dh = _alloc(M, N, N, BF16), _alloc(M, N, N, BF16)
    bits = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    _bits_calls(M, N, K, K2, t["x"], t["w"], t["bias"], t2["x"], t2["w"], y, dh, bits)
    torch.cuda.synchronize()
    GemmRef.forward(t["x"], t["w"], t["bias"], 1).check(y, f"H-{M}x{N}x{K}-relu-bits", "H P8 bf16", n=GemmRef.chain(BF16, K))
    assert 0.3 < (y > 0).float().mean().item() < 0.7
    GemmRef.forward(t2["x"], t2["w"], zmask=y).check(dh, f"H-{M}x{N}x{K2}-masked", "H P8 bf16", n=GemmRef.chain(BF16, K2))


def test_H_mask_bits_are_refused_for_a_few_tile_shape():
    from mmgl_amd import _lib
    M, N, K = 1536, 1024, 3072           # the persistent kernel only through K splits: no bits
    assert bits_bytes(M, N, K, K, K, N, BF16, num_cu()) == 0 == _lib.lib().mmgl_gemm_nt_relu_bits_bytes(M, N, K, K, K, N, _lib.BF16)
    t = GemmRef.inputs(BF16, M, N, K, seed=SEED, device="cuda")
    y, dh = _alloc(M, N, N, BF16), _alloc(M, N, N, BF16)
    bits = torch.full((24 * 8192,), 0xA5, dtype=torch.uint8, device="cuda")
    from mmgl_amd._lib import ptr
    with pytest.raises(ValueError, match="whole tiles"):
        _lib.call("mmgl_gemm_nt_relu_bits", None, ptr(t["x"]), K, ptr(t["w"]), K, ptr(t["bias"]), ptr(y), N, ptr(bits), M, N, K, 1.0, _lib.BF16, _lib.stream_ptr())
    with pytest.raises(ValueError, match="whole tiles"):
        _lib.call("mmgl_gemm_nt_masked", None, ptr(t["x"]), K, ptr(t["w"]), K, ptr(bits), ptr(dh), N, M, N, K, 1.0, _lib.BF16, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(dh).all() and bool((bits == 0xA5).all()), "written by a refused call"


# ------------------------------------------------------------------------------------------ I: isolation and determinism
CASES_I = [
    C("I", P8, 2500, 4080, 256, act=1, pad=(64, 8, 16), **ALL), C("I", P8_ROWS, 2400, 8176, 256, act=3, pad=(8, 64, 16), **ALL),
    C("I", P8_REM, 5400, 3072, 1536, act=0, pad=(8, 8, 8), **ALL), C("I", P8_FEW, 2500, 2064, 4096, act=1, scale=0.125, pad=(8, 8, 48), **ALL),
    C("I", MID, 129, 136, 192, act=4, pad=(8, 16, 8), **ALL), C("I", TILE128, 129, 132, 72, act=3, **ALL),
    C("I", TILE128, 129, 132, 100, act=2, dtype=F32, **ALL),
]


@pytest.mark.parametrize("case", CASES_I, ids=lambda c: c.id)
def test_I_isolation_and_determinism(case):
    c = case
    route, s, nws = _plan_checks(c)
    t = GemmRef.inputs(c.dtype, c.M, c.N, c.K, seed=SEED, device="cuda")
    ldx, ldw, ldy = c.ld
    x, w = Slab((c.M, c.K), c.dtype, NAN_BYTE, t["x"], ld=ldx), Slab((c.N, c.K), c.dtype, NAN_BYTE, t["w"], ld=ldw)
    b = Slab((c.N,), c.dtype, NAN_BYTE, t["bias"])
    r, z = Slab((c.M, c.N), c.dtype, NAN_BYTE, t["residual"], ld=ldy), Slab((c.M, c.N), c.dtype, NAN_BYTE, t["zmask"], ld=ldy)
    ys = [Slab((c.M, c.N), c.dtype, CANARY_BYTE, ld=ldy, extra=3) for _ in range(2)]
    ws = Slab((max(nws, 1),), torch.uint8, CANARY_BYTE)
    for y in ys:
        y.v.fill_(NAN)
        ws.v.fill_(NAN_BYTE)
        _gemm(c, x.v, w.v, b.v, r.v, z.v, y.v, ws.v if nws else None, nws)
        torch.cuda.synchronize()
        assert y.untouched(), "bytes next to the output (rows past M, columns past N) were written"
        assert ws.untouched(), "bytes past the workspace were written"
    assert all(o.untouched() for o in (x, w, b, r, z))
    ref = GemmRef.forward(x.v, w.v, b.v, c.act, c.scale, r.v, z.v)
    ref.check(ys[0].v, c.id, f"I {route} {NAME[c.dtype]}", **_bound_kw(c, route, s))
    assert torch.equal(ys[0].v, ys[1].v), "two launches differ"


# ------------------------------------------------------------------------------------------ J: dynamic tile schedule
CASES_J = [CASES_A[18], CASES_B[1], CASES_C[2]]


@pytest.mark.parametrize("case", CASES_J, ids=lambda c: c.id)
def test_J_dynamic_schedule_is_bitwise_the_static_one(case):
    from mmgl_amd import ops
    c = case
    assert (c.M, c.N, c.route) in ((2816, 8192, P8), (2400, 8192, P8_ROWS), (5632, 3072, P8_REM))
    ops_, y0, ref = _check(c)
    route, s, nws = _plan_checks(c)
    outs = []
    ctr = ops.gemm_dynamic_schedule(True)
    try:
        for _ in range(2):
            y = _alloc(c.M, c.N, c.ld[2], c.dtype)
            ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device="cuda") if nws else None
            _gemm(c, *ops_, y, ws, nws)
            torch.cuda.synchronize()
            assert int(ctr.abs().sum()) == 0, ctr.tolist()
            outs.append(y)
    finally:
        ops.gemm_dynamic_schedule(False)
    assert all(torch.equal(y0, y) for y in outs), "the dynamic schedule's result differs from the static one"
