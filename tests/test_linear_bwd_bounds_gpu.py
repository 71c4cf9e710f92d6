"""-m gpu: mmgl_linear_fwd / mmgl_linear_bwd through the C ABI against gemm_ref.GemmRef, element by element (the bound's count is in
GemmRef's docstring; tests/test_gemm_ref_cpu.py shows on the CPU that the comparison fails for contraction rows lost from a weight
gradient, `accumulate` ignored or applied twice, a row split lost from a bias gradient and mask_dx taken from x >= 0).  The backward
is called directly, so y, `accumulate`, mask_dx and the NULL-able outputs are the test's to choose; the workspace has exactly
mmgl_linear_bwd_workspace bytes and sits, like every output, in a canary slab that must come back untouched.

gemm8p_tt_splits, colsum_splits, big_tile_shape and the workspace layout of csrc/gemm.hip are restated in tests/gemm_ref.py, beside
the NT plans; the restated size is held against mmgl_linear_bwd_workspace for every case and the case list asserts
the route of every case.

  dgrad   NT against W^T on the 128x128 kernel (300 x 128 x 192), NT on the persistent kernel with K splits (1536 x 1024, N = 3072),
          gemm_tx NN with LDS-DMA staging (N = 192, K_in = 128) and without (N = 136; K_in = 72); each with and without mask_dx and
          with act = relu (the dyp pass)
  wgrad   gemm8p_tt unsplit (M = 256, N = K = 4096), split by 4 plus the fp32 fold (M = 2048, N = K = 1024), ragged unsplit
          (N = 3080), gemm_tx TN with LDS-DMA (M = 192, N = K = 128) and without (100 x 136 x 72); M one 128-row step on either side
          of each gemm8p_tt shape (the route changes, the result must not); each with accumulate 0 and 1 (the output prefilled with
          randn: mag gains |prior|)
  dbias   N = 8, 136, 2048 x M = 5, 129, 2560 (fewer rows than row splits, then many), with and without the ReLU mask, accumulate
  fp32    every product at 129 x 132 x 100 and 300 x 200 x 136 on the transpose path, dbias from the transpose kernel
  scale   0.125 everywhere but one bf16 case with 0.3 and an activation: dyp is then rounded once more, u mag, counted in the bound
  forward mmgl_linear_fwd at the same shapes; it plans without K splits, so 1536 x 1024 x 3072 runs on the 128x128 kernel"""
import pytest
import torch

from bounds import BF16, CANARY_BYTE, F32, NAME, NAN, NAN_BYTE, Slab
from gemm_ref import (MID, NT_FEW, NT_MID, P8, TILE128, TRANSPOSE, TT1, TT4, TX, TX_GLDS, GemmRef, bwd_workspace, cdiv, colsum_splits, dgrad_route,
                      gemm8p_tt_splits, nt_route, num_cu, wgrad_route)

pytestmark = pytest.mark.gpu

SEED = 0                    # tests/test_gemm_ref_cpu.py: every wrong reference leaves the bound on >= 25 % at this seed


# ------------------------------------------------------------------------------------------ cases
class Case:
    def __init__(self, M, N, K, dx=None, dw=None, db=False, act=0, scale=0.125, accumulate=0, mask_dx=False, dtype=BF16):
        """dx / dw: the expected route of that product (None: the output is NULL); db: the bias gradient is asked for."""
        self.M, self.N, self.K, self.dx, self.dw, self.db, self.act, self.scale = M, N, K, dx, dw, db, act, scale
        self.accumulate, self.mask_dx, self.dtype = accumulate, mask_dx, dtype

    @property
    def id(self):
        return (f"{NAME[self.dtype]}-{self.M}x{self.N}x{self.K}-" + "+".join(n for n, v in (("dx", self.dx), ("dW", self.dw), ("db", self.db)) if v)
                + ("-relu" if self.act else "") + ("-mask_dx" if self.mask_dx else "") + ("-acc" if self.accumulate else "")
                + (f"-s{self.scale}" if self.scale != 0.125 else ""))


DGRAD = [Case(M, N, K, dx=r, act=a, mask_dx=m)
         for M, N, K, r in ((300, 128, 192, NT_MID), (1536, 3072, 1024, NT_FEW), (300, 192, 128, TX_GLDS), (300, 136, 128, TX), (300, 192, 72, TX))
         for a, m in ((0, False), (0, True), (1, False), (1, True))]
WGRAD = [Case(M, N, K, dw=r, act=a, accumulate=acc)
         for M, N, K, r in ((256, 4096, 4096, TT1), (128, 4096, 4096, TX_GLDS), (384, 4096, 4096, TT1),
                            (2048, 1024, 1024, TT4), (1920, 1024, 1024, TX_GLDS), (2176, 1024, 1024, TX_GLDS),
                            (256, 3080, 4096, TT1), (128, 3080, 4096, TX), (384, 3080, 4096, TT1),
                            (192, 128, 128, TX_GLDS), (100, 136, 72, TX))
         for a, acc in ((0, 0), (1, 1))]
WGRAD += [Case(2048, 1024, 1024, dw=TT4, act=0, accumulate=1), Case(256, 3080, 4096, dw=TT1, act=1, accumulate=0), Case(100, 136, 72, dw=TX, act=0, accumulate=1)]
DBIAS = [Case(M, N, 8, db=True, act=a, accumulate=acc) for N in (8, 136, 2048) for M in (5, 129, 2560) for a, acc in ((0, 0), (1, 1))]
DBIAS += [Case(2560, 2048, 8, db=True, act=1, accumulate=0), Case(129, 136, 8, db=True, act=0, accumulate=1),
          Case(2560, 8192, 8, db=True, act=1, accumulate=1)]              # 64 column blocks: the fewest row splits, 16
ROUNDED = [Case(300, 192, 128, dx=TX_GLDS, dw=TX, db=True, act=1, scale=0.3, mask_dx=True),                 # the one case with a scale that is no power of two
           Case(2048, 1024, 1024, dx=NT_MID, dw=TT4, db=True, act=1, accumulate=1, mask_dx=True)]            # all three outputs of one call
FP32 = [Case(M, N, K, dx=TRANSPOSE, dw=TRANSPOSE, db=True, act=a, accumulate=acc, mask_dx=m, dtype=F32)
        for M, N, K in ((129, 132, 100), (300, 200, 136)) for a, acc, m in ((0, 0, False), (1, 1, True))]
FP32 += [Case(129, 132, 100, dx=TRANSPOSE, act=1, dtype=F32), Case(300, 200, 136, dw=TRANSPOSE, dtype=F32)]
EVERY = DGRAD + WGRAD + DBIAS + ROUNDED + FP32


def test_case_list_reaches_every_route():
    G = num_cu()
    assert G == 256, f"the shapes were derived for 256 CUs, this device has {G}"
    for c in EVERY:
        if c.dtype == BF16:
            assert c.dx is None or dgrad_route(c.M, c.N, c.K, G)[0] == c.dx, (c.id, dgrad_route(c.M, c.N, c.K, G))
            assert c.dw is None or wgrad_route(c.M, c.N, c.K, G)[0] == c.dw, (c.id, wgrad_route(c.M, c.N, c.K, G))
    for route in (NT_MID, NT_FEW, TX_GLDS, TX):
        got = {(c.act, c.mask_dx) for c in DGRAD if c.dx == route}
        assert got == {(0, False), (0, True), (1, False), (1, True)}, route
    assert dgrad_route(1536, 3072, 1024, G) == (NT_FEW, 8)
    for route in (TT1, TT4, TX_GLDS, TX):
        assert {c.accumulate for c in WGRAD if c.dw == route} == {0, 1}, route
    assert gemm8p_tt_splits(4096, 3080, 256, G) == 1 and gemm8p_tt_splits(1024, 1024, 2048, G) == 4
    # one 128-row step on either side of every gemm8p_tt shape
    for N, K, M in ((4096, 4096, 256), (1024, 1024, 2048), (3080, 4096, 256)):
        assert {c.M for c in WGRAD if (c.N, c.K) == (N, K)} == {M - 128, M, M + 128}
        assert len({wgrad_route(m, N, K, G)[0] for m in (M - 128, M, M + 128)}) >= 2
    assert {colsum_splits(c.M, c.N, 8) for c in DBIAS} == {1, 16, 20} and colsum_splits(5, 8, 8) == 1 and colsum_splits(2560, 2048, 8) == 20
    assert {(c.act, c.accumulate) for c in DBIAS} == {(0, 0), (1, 1), (1, 0), (0, 1)}
    assert [c.scale for c in EVERY if c.scale != 0.125] == [0.3]


def _bwd(c, dy, y, x, w, dx, dw, db, ws, nws):
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr
    _lib.call("mmgl_linear_bwd", None, ptr(dy), ptr(y), ptr(x), ptr(w), ptr(dx), ptr(dw), ptr(db), ptr(ws), nws, c.M, c.N, c.K, c.act, float(c.scale),
              c.accumulate, int(c.mask_dx), _lib.dtype_code(dy), _lib.stream_ptr())


def _run(c):
    from mmgl_amd import _lib
    G = num_cu()
    t = GemmRef.inputs(c.dtype, c.M, c.N, c.K, seed=SEED, device="cuda")
    x = t["xr"] if c.mask_dx else t["x"]             # mask_dx: x is the output of a ReLU
    y = t["y"] if c.act else None
    nws = bwd_workspace(c.M, c.N, c.K, c.act, c.dtype, G)
    assert _lib.lib().mmgl_linear_bwd_workspace(c.M, c.N, c.K, c.act, _lib.BF16 if c.dtype == BF16 else _lib.F32) == nws, \
        f"{c.id}: mmgl_linear_bwd_workspace is not the restated layout's"
    ws = Slab((nws,), torch.uint8, CANARY_BYTE)
    ws.v.fill_(NAN_BYTE)
    dx = Slab((c.M, c.K), c.dtype, CANARY_BYTE) if c.dx else None
    dw = Slab((c.N, c.K), c.dtype, CANARY_BYTE) if c.dw else None
    db = Slab((c.N,), c.dtype, CANARY_BYTE) if c.db else None
    for o, fill in ((dx, None), (dw, t["prior_w"]), (db, t["prior_b"])):
        if o is not None:
            o.v.copy_(fill) if (fill is not None and c.accumulate) else o.v.fill_(NAN)
    v = lambda o: None if o is None else o.v
    _bwd(c, t["dy"], y, x, t["w"], v(dx), v(dw), v(db), ws.v, nws)
    torch.cuda.synchronize()
    for name, o in (("dx", dx), ("dW", dw), ("dbias", db), ("workspace", ws)):
        assert o is None or o.untouched(), f"{c.id}: bytes next to {name} were written"
    bf = c.dtype == BF16
    rounded = bf and c.act == 1 and c.scale not in (0.125, 1.0)
    group = f"bwd {NAME[c.dtype]}"
    if dx is not None:
        route, s = dgrad_route(c.M, c.N, c.K, G) if bf else (TRANSPOSE, 0)
        ref = GemmRef.dgrad(t["dy"], t["w"], y, c.scale, x_mask=x if c.mask_dx else None)
        ref.check(dx.v, f"{c.id} dx", f"{group} dgrad {route}", n=GemmRef.chain(c.dtype, c.N, s), dyp_rounded=rounded)
        if c.mask_dx:
            assert bool((dx.v[x <= 0] == 0).all()) and 0.3 < (x <= 0).float().mean().item() < 0.7
    prior = c.accumulate == 1
    if dw is not None:
        route, s = wgrad_route(c.M, c.N, c.K, G) if bf else (TRANSPOSE, 0)
        ref = GemmRef.wgrad(t["dy"], x, y, c.scale, prior=t["prior_w"] if prior else None)
        ref.check(dw.v, f"{c.id} dW", f"{group} wgrad {route}", n=GemmRef.chain(c.dtype, c.M, s), dyp_rounded=rounded)
    if db is not None:
        if bf:      # colsum_kernel: rows of a split in 16 strides, the 16-slot LDS fold, colsum_finish_kernel's fold of the splits
            sp = colsum_splits(c.M, c.N, 8)
            n, route = cdiv(cdiv(c.M, sp), 16) + 16 + sp + 8, f"colsum/{sp}"
        else:       # transpose_kernel: one thread adds every fourth row of its column, four partial sums
            n, route = cdiv(c.M, 4) + 4 + 8, TRANSPOSE
        ref = GemmRef.dbias(t["dy"], y, c.scale, prior=t["prior_b"] if prior else None)
        ref.check(db.v, f"{c.id} dbias", f"{group} dbias {route}", n=n, dyp_rounded=rounded)
    return t, (v(dx), v(dw), v(db))


@pytest.mark.parametrize("case", DGRAD, ids=lambda c: c.id)
def test_dgrad(case):
    _run(case)


@pytest.mark.parametrize("case", WGRAD, ids=lambda c: c.id)
def test_wgrad(case):
    _run(case)


@pytest.mark.parametrize("case", DBIAS, ids=lambda c: c.id)
def test_dbias(case):
    _run(case)


@pytest.mark.parametrize("case", ROUNDED, ids=lambda c: c.id)
def test_all_outputs_of_one_call(case):
    """dx, dW and dbias of one call; two calls are bit-equal."""
    _, a = _run(case)
    _, b = _run(case)
    for name, p, q in zip(("dx", "dW", "dbias"), a, b):
        assert torch.equal(p, q), f"{name}: two calls differ"


@pytest.mark.parametrize("case", FP32, ids=lambda c: c.id)
def test_fp32_transpose_path(case):
    _run(case)


def test_fp32_dbias_needs_dw():
    """include/mmgl_hip.h: the fp32 path forms dbias in the transpose of dy that the weight gradient needs; alone it is refused."""
    c = Case(129, 132, 100, db=True, dtype=F32)
    t = GemmRef.inputs(F32, c.M, c.N, c.K, seed=SEED, device="cuda")
    nws = bwd_workspace(c.M, c.N, c.K, 0, F32, num_cu())
    ws, db = torch.empty(nws, dtype=torch.uint8, device="cuda"), torch.full((c.N,), float("nan"), device="cuda")
    with pytest.raises(ValueError, match="needs dW"):
        _bwd(c, t["dy"], None, t["x"], t["w"], None, None, db, ws, nws)
    torch.cuda.synchronize()
    assert torch.isnan(db).all()


# ------------------------------------------------------------------------------------------ forward
FWD = [(BF16, 300, 128, 192, MID), (BF16, 1536, 3072, 1024, MID), (BF16, 1536, 1024, 3072, MID), (BF16, 300, 136, 72, TILE128),
       (BF16, 256, 4096, 4096, MID), (BF16, 2560, 4096, 256, P8), (F32, 129, 132, 100, TILE128), (F32, 300, 200, 136, TILE128)]


@pytest.mark.parametrize("act,bias,scale", [(0, True, 1.0), (1, True, 0.125), (1, False, 1.0)])
@pytest.mark.parametrize("dtype,M,N,K,route", FWD, ids=lambda v: NAME.get(v, str(v)))
def test_linear_fwd(dtype, M, N, K, route, act, bias, scale):
    """mmgl_linear_fwd plans without K splits (nt_route's k_splits = false): a few-tile shape with a long contraction -- the persistent
    kernel's under mmgl_gemm_nt -- runs on the 128x128 kernel.  mmgl_gemm_nt_relu_bits_bytes answers with that same plan."""
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr
    G = num_cu()
    assert nt_route(M, N, K, K, K, N, dtype, False, G) == route
    if dtype == BF16:
        assert (_lib.lib().mmgl_gemm_nt_relu_bits_bytes(M, N, K, K, K, N, _lib.BF16) > 0) == (route == P8)
    if (M, N, K) == (1536, 1024, 3072):
        assert nt_route(M, N, K, K, K, N, dtype, True, G) == P8
    t = GemmRef.inputs(dtype, M, N, K, seed=SEED, device="cuda")
    y = Slab((M, N), dtype, CANARY_BYTE, extra=1)
    y.v.fill_(NAN)
    b = t["bias"] if bias else None
    _lib.call("mmgl_linear_fwd", None, ptr(t["x"]), ptr(t["w"]), ptr(b), ptr(y.v), M, N, K, act, float(scale), _lib.dtype_code(t["x"]), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert y.untouched(), "bytes next to the output were written"
    GemmRef.forward(t["x"], t["w"], b, act, scale).check(y.v, f"{NAME[dtype]}-{M}x{N}x{K}-a{act}{'b' if bias else ''}-s{scale}", f"fwd {route} {NAME[dtype]}",
                                                        n=GemmRef.chain(dtype, K), composed=route == TILE128)
