"""-m gpu: the kernels of FP8 frozen weights (csrc/decode.hip).

mmgl_weight_quantize -- codes and exponents bitwise equal to the restatement tests/w8_ref.py, bf16 and fp32 weights: random rows, the
edge rows of the exponent rule, K at the 16-element vector width's edges (8, 64, 72; 16, 1024 = one trip of a wave, 1040, 2064) and
N = 1 and 9 (4 rows per workgroup); source and destination as windows of buffers that hold NaN / a marker everywhere else.

mmgl_gemm_skinny_w8 -- every element within decode_ref.SkinnyRef's bound  u |want| + 2^-16 mag  of fp64 on the dequantised weight, with
bias, residual, ReLU and scale together, two runs bitwise equal.  tests/test_weight_fp8_ref_cpu.py shows from the references alone that
the mistakes such a kernel can make leave that bound; here SkinnyRef.assert_can_fail repeats it for the dropped K columns.  The codes
come from the restatement, not from the kernel under test, and the weight rows span exponents from negative to large, so the
epilogue's power of two is never 1 throughout.  The states are those tests/test_decode_edges_gpu.py group B visits, restated for the
K unit of 128 codes (a W ring of 4 units per lane; 4 K slots in 16-row workgroups, 8 in 8-row ones):
  B  fewer units than slots, a ragged last trip, a partial second round of the ring; 16-row (N = 16 x compute units) and 8-row (768)
     workgroups; widths 8, 24, N16 - 16, N16 + 8; M = 1, 16, 17, 32, 33, 64.
  C  operands as windows of NaN buffers with free ldx / ld_codes / ldy: aligned (MFMA kernel), 8-byte-aligned bases or odd strides
     (generic kernel); nothing outside the output window changes.
  D  the generic kernel's grid edges, bf16 and fp32 x (fp32 has this route only), and K = 64 / N % 8 shapes of bf16.
  E  a refused call leaves y alone."""
import pytest
import torch

import w8_ref
from decode_ref import SkinnyRef

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="fp32")]
NAN = float("nan")
MARK = 0xAB


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _window(g, rows, cols, dtype, scale=1.0, ld=None, col0=0, row0=0, pad_rows=0, fill=NAN):
    """A random [rows, cols] window at (row0, col0) of a [row0 + rows + pad_rows, ld] buffer that holds `fill` everywhere else."""
    buf = torch.full((row0 + rows + pad_rows, ld or cols), fill, device="cuda", dtype=dtype)
    win = buf[row0:row0 + rows, col0:col0 + cols]
    win.copy_((torch.randn(rows, cols, device="cuda", generator=g) * scale).to(dtype))
    return win


# ------------------------------------------------------------------------------------------ mmgl_weight_quantize
def _weight(g, N, K, dtype):
    """Rows whose magnitudes span 2^-12 .. 2^12, some elements deep in the subnormal codes."""
    w = torch.randn(N, K, device="cuda", generator=g) * torch.logspace(-3.6, 3.6, N, device="cuda")[:, None]
    w[:, ::5] *= 2.0 ** -9
    return w.to(dtype)


def _check_quantize(w, what, out=None):
    from mmgl_amd import ops
    codes, exps = ops.quantize_weight_fp8(w, out=out)
    assert codes.shape == w.shape and exps.shape == (w.shape[0],) and exps.dtype == torch.int8
    want_c, want_e = w8_ref.quantize(w.cpu())
    assert torch.equal(exps.cpu(), want_e), f"{what}: exponents differ from the restatement"
    got = codes.view(torch.uint8).cpu()
    bad = (got != want_c).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} codes differ from the restatement, first at {bad[0].tolist()}"
    c2, e2 = ops.quantize_weight_fp8(w)
    assert torch.equal(c2.view(torch.uint8).cpu(), got) and torch.equal(e2, exps), f"{what}: two runs differ"
    return codes, exps


@pytest.mark.parametrize("K", [8, 16, 64, 72, 1024, 1040, 2064])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_matches_the_restatement(dtype, K):
    for N in (1, 9, 130):
        codes, exps = _check_quantize(_weight(_gen(K + N), N, K, dtype), f"{dtype} {N}x{K}")
        assert codes.dtype == torch.float8_e4m3fn
        if N > 1:
            assert exps.min() < 0 < exps.max()


@pytest.mark.parametrize("K", [64, 72])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_edge_rows(dtype, K):
    names, rows = w8_ref.edge_rows(K, dtype)
    _, exps = _check_quantize(rows.cuda(), f"edge rows {dtype} K={K}")
    e = dict(zip(names, exps.tolist()))
    assert e["zero row"] == 0 and e["low clamp"] == -120 and e["high clamp"] == 120 and e["max one step above 448 * 2^-3"] == e["max = 448 * 2^-3"] + 1


@pytest.mark.parametrize("how", ["aligned", "source off 16 bytes", "codes at column 8", "ld_codes = K + 8", "K = 72"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_windows_of_nan_buffers(dtype, how):
    """The first case takes the 16-element path, every other one the element path; nothing outside the windows is read (a NaN would
    poison a row's maximum) or written."""
    N, K = 9, 72 if how == "K = 72" else 80
    g = _gen(3)
    col = 2 if how == "source off 16 bytes" else 8
    w = _window(g, N, K, dtype, ld=K + 24, col0=col, row0=1, pad_rows=2)
    w.mul_(torch.logspace(-3, 3, N, device="cuda")[:, None].to(dtype))
    ldc = K + 8 if how == "ld_codes = K + 8" else K + 48
    ccol = {"codes at column 8": 8, "ld_codes = K + 8": 0}.get(how, 16)
    cbuf = torch.full((N + 3, ldc), MARK, dtype=torch.uint8, device="cuda")
    ebuf = torch.full((N + 9,), 77, dtype=torch.int8, device="cuda")
    codes, exps = cbuf[2:2 + N, ccol:ccol + K], ebuf[5:5 + N]
    vec = K % 16 == 0 and w.data_ptr() % 16 == 0 and codes.data_ptr() % 16 == 0 and ldc % 16 == 0 and (w.stride(0) * w.element_size()) % 16 == 0
    assert vec == (how == "aligned")
    _check_quantize(w, f"windows {dtype} {how}", out=(codes, exps))
    keep = torch.ones_like(cbuf, dtype=torch.bool)
    keep[2:2 + N, ccol:ccol + K] = False
    assert (cbuf[keep] == MARK).all(), "code bytes outside the window changed"
    assert (ebuf[:5] == 77).all() and (ebuf[5 + N:] == 77).all(), "exponent bytes outside the window changed"


# ------------------------------------------------------------------------------------------ mmgl_gemm_skinny_w8
def _codes(g, N, K, ld=None, col0=0, pad_rows=0):
    """A weight [N, K] with row magnitudes from 1e-2 to 1e6 around K^-1/2, quantised by the restatement: (codes uint8 window on the
    GPU -- the rest of its buffer holds the NaN code 0x7f --, exps, the dequantised weight fp32 on the GPU)."""
    w = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5 * torch.logspace(-2, 6, N, device="cuda")[:, None]
    c, e = w8_ref.quantize(w.to(BF16).cpu())
    buf = torch.full((N + pad_rows, ld or K), 0x7F, dtype=torch.uint8, device="cuda")
    win = buf[:N, col0:col0 + K]
    win.copy_(c)
    if N >= 8:
        assert e.min() < 0 < e.max()                        # the epilogue's power of two on both sides of 1
    return win, e.cuda(), w8_ref.dequantize(c, e).cuda()


def _operands(g, M, N, K, dtype):
    x = _window(g, M, K, dtype)
    b = (torch.randn(N, device="cuda", generator=g) * torch.logspace(-2, 6, N, device="cuda")).to(dtype)
    res = _window(g, M, N, dtype)
    return x, b, res


def _states(N, K, rows, group, dtype=BF16, relu=True):
    from mmgl_amd import ops
    codes, exps, deq = _codes(_gen(K * 7 + N), N, K)
    cases = [_operands(_gen(K * 100 + M), M, N, K, dtype) for M in rows]
    refs = [SkinnyRef(x, deq, b, relu, 0.5, res) for x, b, res in cases]
    SkinnyRef.assert_can_fail(refs, dtype, f"M in {rows}, {N}x{K}")
    for M, (x, b, res), ref in zip(rows, cases, refs):
        y = ops.gemm_skinny_w8(x, codes, exps, b, res, act=int(relu), out_scale=0.5)
        ref.check(y, f"w8 {M}x{N}x{K}", group, can_fail=False)
        assert torch.equal(y, ops.gemm_skinny_w8(x, codes.view(torch.float8_e4m3fn), exps, b, res, act=int(relu), out_scale=0.5)), \
            f"{M}x{N}x{K}: two runs differ"


def _rows(K, more_at):
    return [1, 17, 33, 64] + ([16, 32] if K in more_at else [])


@pytest.mark.parametrize("K", [128, 256, 384, 512, 640, 2176, 2688, 3584])           # units 1, 2, 3, 4, 5, 17, 21, 28: K-loop trips 1 x 4, 2, 5, 6, 7
def test_mfma_16_row_workgroups(K):
    N16 = 16 * torch.cuda.get_device_properties(0).multi_processor_count              # the narrowest N whose workgroups take 16 rows
    _states(N16, K, _rows(K, (640, 2688)), "B")


@pytest.mark.parametrize("K", [128, 640, 1024, 1152, 4224, 6272, 7296])              # units 1, 5, 8, 9, 33, 49, 57: K-loop trips 1, 1, 1, 2, 5, 7, 8
def test_mfma_8_row_workgroups(K):
    _states(768, K, _rows(K, (640, 4224)), "B")


@pytest.mark.parametrize("N", [8, 24, "N16 - 16", "N16 + 8"])
def test_mfma_width_edges(N):
    N16 = 16 * torch.cuda.get_device_properties(0).multi_processor_count
    N = {"N16 - 16": N16 - 16, "N16 + 8": N16 + 8}.get(N, N)
    _states(N, 1152, [1, 33], "B")


C_SHAPE = (33, 768, 1152)


@pytest.mark.parametrize("how", ["aligned", "bases at 8 bytes", "ldx = K + 4", "ld_codes = K + 8"])
def test_windows_of_nan_buffers(how):
    from mmgl_amd import ops
    M, N, K = C_SHAPE
    g = _gen(31)
    xcol, ccol = (4, 8) if how == "bases at 8 bytes" else (8, 16)
    x = _window(g, M, K, BF16, ld=K + 4 if how == "ldx = K + 4" else K + 24, col0=0 if how == "ldx = K + 4" else xcol, pad_rows=3)
    codes, exps, deq = _codes(g, N, K, ld=K + 8 if how == "ld_codes = K + 8" else K + 48, col0=0 if how == "ld_codes = K + 8" else ccol,
                              pad_rows=5)
    b = _window(g, 1, N, BF16, ld=N + 16, col0=8)[0]
    res = _window(g, M, N, BF16, ld=N + 24, col0=8, row0=1, pad_rows=1)
    outbuf = torch.full((M + 2, N + 24), 7.0, device="cuda", dtype=BF16)
    out = outbuf[1:1 + M, 8:8 + N]
    mfma = x.data_ptr() % 16 == 0 and codes.data_ptr() % 16 == 0 and x.stride(0) % 8 == 0 and codes.stride(0) % 16 == 0
    assert mfma == (how == "aligned") and x.stride(0) > K and codes.stride(0) > K and res.stride(0) == out.stride(0)
    ref = SkinnyRef(x, deq, b, True, 0.5, res)
    ops.gemm_skinny_w8(x, codes, exps, b, res, act=1, out_scale=0.5, out=out)
    ref.check(out, f"w8 windows, {how}", "C")
    keep = torch.ones_like(outbuf, dtype=torch.bool)
    keep[1:1 + M, 8:8 + N] = False
    assert torch.equal(outbuf[keep], torch.full_like(outbuf, 7.0)[keep]), "bytes outside the output window changed"
    first = out.clone()
    ops.gemm_skinny_w8(x, codes, exps, b, res, act=1, out_scale=0.5, out=out)
    assert torch.equal(first, out), "two runs differ"


@pytest.mark.parametrize("K", [1, 63, 65, 1088])
@pytest.mark.parametrize("dtype", DTYPES)
def test_generic_kernel_grid_edges(dtype, K):
    """4 output columns and 8 rows of x per workgroup: N = 3, 4, 5 and M = 8, 9, 64; K below, at and above a wave's 64 lanes.  No ReLU
    (24 elements are too few to count on the share it leaves)."""
    for M in (8, 9, 64):
        for N in (3, 4, 5):
            _states(N, K, [M], "D", dtype, relu=False)


@pytest.mark.parametrize("dtype,N,K", [(F32, 768, 1152), (F32, 24, 128), (BF16, 768, 64), (BF16, 772, 1152), (BF16, 24, 1160)],
                         ids=["fp32 768x1152", "fp32 24x128", "bf16 K=64", "bf16 N%8", "bf16 K%128"])
def test_generic_kernel_takes_what_the_mfma_kernel_does_not(dtype, N, K):
    _states(N, K, [1, 17, 64], "D", dtype)


def test_decode_linear_w8_chunks_rows_and_writes_a_strided_out():
    """130 rows: chunks of 64, 64 and 2 into a cache column (row stride 3 N), with the kernel's own quantiser in front."""
    from mmgl_amd import ops
    M, N, K = 130, 768, 256
    g = _gen(9)
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(BF16)
    codes, exps = ops.quantize_weight_fp8(w)
    x, b, _ = _operands(g, M, N, K, BF16)
    cache = torch.full((M, 3, N), 7.0, device="cuda", dtype=BF16)
    res = torch.randn(M, 3, N, device="cuda", generator=g).to(BF16)[:, 1]
    out = ops.decode_linear_w8(x, codes, exps, b, act="relu", out_scale=0.5, residual=res, out=cache[:, 1])
    assert out.data_ptr() == cache[:, 1].data_ptr()
    SkinnyRef(x, w8_ref.dequantize(codes.view(torch.uint8).cpu(), exps.cpu()).cuda(), b, True, 0.5, res).check(out, "decode_linear_w8 130 rows", "C")
    assert (cache[:, 0] == 7).all() and (cache[:, 2] == 7).all()


def test_a_refused_call_leaves_y_alone():
    from mmgl_amd import ops
    g = _gen(2)
    codes, exps, _ = _codes(g, 64, 128)
    for M, act in ((65, 0), (4, 5)):
        y = torch.full((M, 64), 7.0, device="cuda", dtype=BF16)
        with pytest.raises(ValueError, match="mmgl_gemm_skinny_w8"):
            ops.gemm_skinny_w8(torch.ones(M, 128, device="cuda", dtype=BF16), codes, exps, act=act, out=y)
        torch.cuda.synchronize()
        assert torch.equal(y, torch.full_like(y, 7.0))
