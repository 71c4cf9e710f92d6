"""-m gpu: mmgl_gemm_skinny_lora (csrc/decode.hip) through ops.decode_lora_linear / ops.gemm_skinny_lora:
    y = act((x W^T + bias + s (x A^T) B^T) * out_scale) + residual
against an fp32 torch reference on the same (bf16-rounded) operands, with the bound of tests/test_decode_kernels_gpu.py::_check
(2e-2 * max|want| + 1e-2 on the largest absolute error).  B is scaled so that the rank-r term is of the size of the base product: every
comparison first asserts, from the reference alone, that dropping the term would miss the bound tenfold, and then holds element by
element against the fp64 reference within decode_ref.SkinnyRef's bound (which the reference without the term, or without its last 64 K
columns, leaves on a quarter of the elements or more).  Also: the epilogue options
one by one and together; a strided output inside a larger buffer whose other bytes stay untouched; two runs bitwise equal; agreement
with the training forward ops.lora_linear on the same operands (2e-2 bf16, 1e-3 fp32, max-norm relative: DESIGN.md 2)."""
import pytest
import torch

from decode_ref import SkinnyRef
from helpers import rel_err

pytestmark = pytest.mark.gpu

# (4096, 2048): 16-row workgroups; (2048, 2048), (768, 768): the 8-row HALF path; (72, 40): the generic kernel, nothing aligned
SHAPES = [(4096, 2048), (2048, 2048), (768, 768), (72, 40)]
ROWS = [1, 7, 16, 33, 64, 65]            # 65: two chunks in the op
RANKS = [4, 8, 16, 64]
SCALING = 2.0


def _operands(M, N, K, r, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x = rn(M, K).to(dtype)
    w = (rn(N, K) * K ** -0.5).to(dtype)
    b = rn(N).to(dtype)
    res = rn(M, N).to(dtype)
    A = (rn(r, K) * K ** -0.5).to(dtype)          # t = x A^T ~ N(0, 1)
    Bm = (rn(N, r) * r ** -0.5).to(dtype)         # t B^T ~ N(0, 1): with SCALING = 2 the term is twice the base product's size
    return x, w, b, res, A, Bm


def _want(x, w, A, Bm, bias=None, relu=False, scale=1.0, residual=None, lora=True):
    y = x.float() @ w.float().t()
    if lora:
        y = y + SCALING * ((x.float() @ A.float().t()) @ Bm.float().t())
    if bias is not None:
        y = y + bias.float()
    y = y * scale
    if relu:
        y = torch.relu(y)
    if residual is not None:
        y = y + residual.float()
    return y


def _ref(x, w, A, Bm, bias=None, relu=False, scale=1.0, residual=None):
    """(fp32 reference, the same without the rank-r term, the fp64 reference of the per-element bound), on the GPU."""
    return (_want(x, w, A, Bm, bias, relu, scale, residual), _want(x, w, A, Bm, bias, relu, scale, residual, lora=False),
            SkinnyRef(x, w, bias, relu, scale, residual, A, Bm, SCALING))


def _check(got, want, want_plain, ref64, what):
    bound = 2e-2 * want.abs().max().item() + 1e-2
    live = (want - want_plain).abs().max().item()
    assert live > 10 * bound, f"{what}: the rank-r term ({live:.3e}) is not visible at the bound {bound:.3e}"
    err = (got.float() - want).abs().max().item()
    print(f"{what}: max abs err {err:.3e} (bound {bound:.3e}, rank-r term {live:.3e})")
    assert torch.isfinite(got.float()).all(), what
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"
    ref64.check(got, what, "F")


@pytest.mark.parametrize("N,K", SHAPES)
def test_decode_lora_linear_bf16_shapes(N, K):
    from mmgl_amd import ops
    for r in RANKS:
        for M in ROWS:
            x, w, b, _, A, Bm = _operands(M, N, K, r, torch.bfloat16, 1000 * r + M)
            y = ops.decode_lora_linear(x, w, b, A, Bm, SCALING)
            assert y.shape == (M, N) and y.dtype == torch.bfloat16
            _check(y, *_ref(x, w, A, Bm, b), f"lora {M}x{N}x{K} r={r}")
            assert torch.equal(y, ops.decode_lora_linear(x, w, b, A, Bm, SCALING)), f"{M}x{N}x{K} r={r}: two runs differ"


def test_decode_lora_linear_fp32():
    from mmgl_amd import ops
    N = K = 768
    for r in RANKS:
        for M in ROWS:
            x, w, b, _, A, Bm = _operands(M, N, K, r, torch.float32, 2000 * r + M)
            y = ops.decode_lora_linear(x, w, b, A, Bm, SCALING)
            want, plain, ref64 = _ref(x, w, A, Bm, b)
            _check(y, want, plain, ref64, f"lora fp32 {M}x{N}x{K} r={r}")
            e = rel_err(y, want)
            assert e <= 1e-3, (M, r, e)
            assert torch.equal(y, ops.decode_lora_linear(x, w, b, A, Bm, SCALING))


@pytest.mark.parametrize("r", [1, 3, 12, 100, 256])
def test_every_rank_from_one(r):
    """Ranks outside the vector path of the epilogue (r % 8) and up to the limit, on the MFMA and the generic kernel."""
    from mmgl_amd import ops
    for (N, K) in [(768, 768), (72, 40)]:
        x, w, b, _, A, Bm = _operands(9, N, K, r, torch.bfloat16, 77 + r)
        y = ops.decode_lora_linear(x, w, b, A, Bm, SCALING)
        _check(y, *_ref(x, w, A, Bm, b), f"lora 9x{N}x{K} r={r}")
    with pytest.raises(ValueError):
        ops.decode_lora_linear(x, w, b, torch.zeros(257, K, device="cuda", dtype=torch.bfloat16),
                               torch.zeros(N, 257, device="cuda", dtype=torch.bfloat16), SCALING)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("N,K", [(768, 768), (72, 40)])
def test_epilogue_order_one_by_one_and_together(dtype, N, K):
    """bias, then out_scale on the whole sum (base, bias and rank-r term), then ReLU, then the residual."""
    from mmgl_amd import ops
    M, r = 7, 8
    x, w, b, res, A, Bm = _operands(M, N, K, r, dtype, 7)
    run = lambda **kw: ops.gemm_skinny_lora(x, w, A, Bm, SCALING, **kw)
    ref = lambda **kw: _ref(x, w, A, Bm, **kw)
    _check(run(), *ref(), "plain")
    _check(run(bias=b), *ref(bias=b), "bias")
    _check(run(act=1), *ref(relu=True), "relu")
    assert (run(act=1) >= 0).all()
    _check(run(residual=res), *ref(residual=res), "residual")
    # the scale multiplies the rank-r term too: at 0.125 the reference's term is an eighth, and so must the kernel's be
    got, (want, plain, ref64) = run(out_scale=0.125), ref(scale=0.125)
    ref64.check(got, "scale", "F")
    bound = 2e-2 * want.abs().max().item() + 1e-2
    assert (got.float() - want).abs().max().item() <= bound
    assert (want - plain).abs().max().item() > 3 * bound             # an eighth of the term: still visible, less than tenfold
    unscaled_term = _want(x, w, A, Bm, lora=False, scale=0.125) + SCALING * ((x.float() @ A.float().t()) @ Bm.float().t())
    assert (got.float() - unscaled_term).abs().max().item() > bound   # a kernel that scales only the base product fails
    got = run(bias=b, residual=res, act=1, out_scale=0.125)
    want = _want(x, w, A, Bm, b, True, 0.125, res)
    assert (got.float() - want).abs().max().item() <= 2e-2 * want.abs().max().item() + 1e-2
    SkinnyRef(x, w, b, True, 0.125, res, A, Bm, SCALING).check(got, "bias, scale, relu, residual", "F")
    wrong_order = torch.relu(_want(x, w, A, Bm, b, False, 0.125, res))                   # residual in front of the ReLU
    assert (want - wrong_order).abs().max().item() > 10 * (2e-2 * want.abs().max().item() + 1e-2)
    if dtype == torch.float32:
        assert rel_err(got, want) <= 1e-3


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M", [2, 16, 64])
def test_writes_the_value_columns_of_a_cache_row_in_place(dtype, M):
    """out = the v columns of column `col` of a [M, cap, 2d + 16] buffer: every other byte stays as it was."""
    from mmgl_amd import ops
    d, cap, col, r = 256, 5, 3, 8
    x, w, b, _, A, Bm = _operands(M, d, d, r, dtype, 11)
    cache = torch.full((M, cap, 2 * d + 16), 7.0, device="cuda", dtype=dtype)
    before = cache.clone()
    out = cache[:, col, 8 + d:8 + 2 * d]
    assert out.stride(0) == cap * (2 * d + 16)
    ops.decode_lora_linear(x, w, b, A, Bm, SCALING, out=out)
    _check(cache[:, col, 8 + d:8 + 2 * d], *_ref(x, w, A, Bm, b), f"strided out M={M}")
    keep = torch.ones_like(cache, dtype=torch.bool)
    keep[:, col, 8 + d:8 + 2 * d] = False
    assert torch.equal(cache[keep], before[keep]), "bytes outside the written slab changed"


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 2e-2), (torch.float32, 1e-3)])
@pytest.mark.parametrize("M,N,K,r", [(16, 768, 768, 8), (64, 2048, 2048, 16), (33, 768, 768, 64)])
def test_agrees_with_the_training_forward(dtype, tol, M, N, K, r):
    """The decode step computes the function the adapter was trained through: ops.lora_linear on the same operands."""
    from mmgl_amd import ops
    x, w, b, _, A, Bm = _operands(M, N, K, r, dtype, 5)
    with torch.no_grad():
        train = ops.lora_linear(x[None], w, b, A, Bm, SCALING, 0.125)[0]
    got = ops.decode_lora_linear(x, w, b, A, Bm, SCALING, out_scale=0.125)
    e = rel_err(got, train.float())
    print(f"decode vs training forward {M}x{N}x{K} r={r} {dtype}: rel err {e:.3e}")
    assert e <= tol, e
    plain = ops.decode_linear(x, w, b, out_scale=0.125)
    assert rel_err(plain, train.float()) > 10 * tol                 # the adapter is live in the comparison


def test_refuses_gradients_and_bad_shapes():
    from mmgl_amd import ops
    x, w, b, _, A, Bm = _operands(4, 768, 768, 8, torch.bfloat16, 5)
    Ag = A.clone().requires_grad_()
    with pytest.raises(ValueError, match="forward only"):
        ops.decode_lora_linear(x, w, b, Ag, Bm, SCALING)
    with torch.no_grad():
        ops.decode_lora_linear(x, w, b, Ag, Bm, SCALING)
    with pytest.raises(ValueError, match="shapes"):
        ops.decode_lora_linear(x, w, b, A[:, :64], Bm, SCALING)
    with pytest.raises(ValueError):
        ops.gemm_skinny_lora(torch.cat([x] * 17)[:65], w, A, Bm, SCALING)           # the kernel itself stops at 64 rows
