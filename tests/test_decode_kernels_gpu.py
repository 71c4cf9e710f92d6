"""-m gpu: the two kernels of the decode step (csrc/decode.hip) at the C-ABI level of mmgl_amd.ops.
  * mmgl_gemm_skinny against an fp32 torch GEMM of the same (bf16-rounded) operands, bound as in tests/test_gemm_nt_gpu.py
    (2e-2 * max|want| + 1e-2 on the largest absolute error); every epilogue option; a strided output inside a larger buffer whose
    other bytes must stay untouched; two runs bitwise equal (the K partials are folded in a fixed order).  Every comparison also
    holds element by element against the fp64 reference, within decode_ref.SkinnyRef's bound (half an ulp of the store plus 256 fp32
    roundings on the magnitude sum), which a dropped 64-wide K unit leaves on a quarter of the elements or more.
  * mmgl_attn_decode_fwd against oracle.lm_ref.attention_core with one query row: random key masks, a sample without any valid key
    (uniform over its keys), K and V addressed in place as column slabs of wider cache rows.  Tolerances of tests/test_xattn_gpu.py:
    1e-3 fp32, 2e-2 bf16 (relative to the largest reference magnitude)."""
import pytest
import torch

from decode_ref import SkinnyRef
from helpers import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(2048, 2048), (4096, 2048), (8192, 2048), (2048, 8192), (50272, 2048), (768, 768), (3072, 768)]
ROWS = [1, 2, 7, 16, 17, 32, 33, 64]            # 16 | 17 and 32 | 33: the kernel's 1, 2 and 4 x-tile variants


def _operands(M, N, K, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(M, K, device="cuda", generator=g).to(dtype)
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(dtype)
    b = torch.randn(N, device="cuda", generator=g).to(dtype)
    r = torch.randn(M, N, device="cuda", generator=g).to(dtype)
    return x, w, b, r


def _want(x, w, bias=None, relu=False, scale=1.0, residual=None):
    y = x.float() @ w.float().t()
    if bias is not None:
        y = y + bias.float()
    y = y * scale
    if relu:
        y = torch.relu(y)
    if residual is not None:
        y = y + residual.float()
    return y


def _ref(x, w, bias=None, relu=False, scale=1.0, residual=None):
    """The fp32 reference of the max-norm bound and the fp64 one of the per-element bound, both on the GPU."""
    return _want(x, w, bias, relu, scale, residual), SkinnyRef(x, w, bias, relu, scale, residual)


def _check(got, ref, what, can_fail=True):
    want, ref64 = ref
    err = (got.float() - want).abs().max().item()
    bound = 2e-2 * want.abs().max().item() + 1e-2
    print(f"{what}: max abs err {err:.3e} (bound {bound:.3e})")
    assert torch.isfinite(got.float()).all(), what
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"
    ref64.check(got, what, "F", can_fail)


@pytest.mark.parametrize("N,K", SHAPES)
def test_skinny_gemm_bf16_shapes(N, K):
    from mmgl_amd import ops
    for M in ROWS:
        x, w, b, r = _operands(M, N, K, torch.bfloat16, 1000 + M)
        y = ops.gemm_skinny(x, w)
        _check(y, _ref(x, w), f"skinny {M}x{N}x{K}")
        assert torch.equal(y, ops.gemm_skinny(x, w)), f"{M}x{N}x{K}: two runs differ"
        y = ops.gemm_skinny(x, w, b, r, act=1, out_scale=0.5)
        _check(y, _ref(x, w, b, True, 0.5, r), f"skinny {M}x{N}x{K} +bias*0.5+relu+residual")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_skinny_gemm_epilogue_options_one_by_one(dtype):
    from mmgl_amd import ops
    M, N, K = 7, 768, 768
    x, w, b, r = _operands(M, N, K, dtype, 7)
    _check(ops.gemm_skinny(x, w, bias=b), _ref(x, w, bias=b), "bias")
    _check(ops.gemm_skinny(x, w, act=1), _ref(x, w, relu=True), "relu")
    _check(ops.gemm_skinny(x, w, residual=r), _ref(x, w, residual=r), "residual")
    _check(ops.gemm_skinny(x, w, out_scale=0.125), _ref(x, w, scale=0.125), "scale")
    assert (ops.gemm_skinny(x, w, act=1) >= 0).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M", [2, 16, 64])
def test_skinny_gemm_writes_a_cache_column_in_place(dtype, M):
    """ldy = a whole cache row: the k|v projection of a decode step writes column `col` of [B, capacity, 2d]; every other byte of the
    buffer, the rows around the written ones included, stays as it was."""
    from mmgl_amd import ops
    d, cap, col = 256, 5, 3
    x, w, b, _ = _operands(M, 2 * d, d, dtype, 11)
    cache = torch.full((M, cap, 2 * d + 16), 7.0, device="cuda", dtype=dtype)
    before = cache.clone()
    out = cache[:, col, 8:8 + 2 * d]
    assert out.stride(0) == cap * (2 * d + 16)
    ops.decode_linear(x, w, b, out=out)
    _check(cache[:, col, 8:8 + 2 * d], _ref(x, w, b), f"strided ldy M={M}")
    keep = torch.ones_like(cache, dtype=torch.bool)
    keep[:, col, 8:8 + 2 * d] = False
    assert torch.equal(cache[keep], before[keep]), "bytes outside the written slab changed"
    # the residual shares the output's row stride
    res = torch.randn(M, cap, 2 * d + 16, device="cuda").to(dtype)
    ops.decode_linear(x, w, None, residual=res[:, col, 8:8 + 2 * d], out=out)
    _check(cache[:, col, 8:8 + 2 * d], _ref(x, w, residual=res[:, col, 8:8 + 2 * d]), "strided residual")


def test_skinny_gemm_fp32_and_odd_shapes():
    """fp32 and shapes outside the MFMA kernel's alignment (K % 64, N % 8) run the plain kernel: same contract."""
    from mmgl_amd import ops
    for dtype, (M, N, K) in [(torch.float32, (5, 128, 64)), (torch.float32, (64, 2048, 2048)), (torch.bfloat16, (3, 50, 72)),
                             (torch.bfloat16, (9, 128, 100)), (torch.float32, (1, 7, 13))]:
        x, w, b, r = _operands(M, N, K, dtype, 3)
        y = ops.gemm_skinny(x, w, b, r, act=1)
        want, ref64 = _ref(x, w, b, True, 1.0, r)
        if dtype == torch.float32:
            assert rel_err(y, want) <= 1e-3, (M, N, K, rel_err(y, want))
            ref64.check(y, f"generic fp32 {M}x{N}x{K}", "F", can_fail=M * N >= 64)      # 1 x 7 under a ReLU: too few elements to count on
        else:
            _check(y, (want, ref64), f"generic {M}x{N}x{K}")
        assert torch.equal(y, ops.gemm_skinny(x, w, b, r, act=1))


def test_decode_linear_chunks_rows_and_refuses_gradients():
    from mmgl_amd import ops
    x, w, b, _ = _operands(150, 768, 768, torch.bfloat16, 5)
    _check(ops.decode_linear(x, w, b, act="relu"), _ref(x, w, b, True), "150 rows in chunks of 64")
    with pytest.raises(ValueError):
        ops.gemm_skinny(x[:65], w)                       # the kernel itself stops at 64 rows
    wg = w.clone().requires_grad_()
    with pytest.raises(ValueError, match="forward only"):
        ops.decode_linear(x[:4], wg)
    with torch.no_grad():
        ops.decode_linear(x[:4], wg)
    with pytest.raises(ValueError, match="forward only"):
        ops.attn_decode(x[:2, :64].clone().requires_grad_(), x[:8, :64].reshape(2, 4, 64), x[:8, :64].reshape(2, 4, 64),
                        torch.ones(2, 4, dtype=torch.bool, device="cuda"), 1)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-3), (torch.bfloat16, 2e-2)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [1, 33, 64, 128, 544, 672])
def test_attn_decode_against_the_oracle(S, D, dtype, tol):
    from mmgl_amd import ops
    from oracle import lm_ref
    B, H = 3, 4
    d = H * D
    g = torch.Generator().manual_seed(S * 1000 + D)
    q = (torch.randn(B, d, generator=g) * D ** -0.5).to(dtype)
    cap = S + 5
    cache = torch.randn(B, cap, 2 * d + 8, generator=g).to(dtype)        # K|V slabs inside wider rows: strided, addressed in place
    valid = torch.rand(B, S, generator=g) > 0.3
    valid[0] = True
    valid[1, 0] = True
    valid[2] = False                                                     # no valid key: uniform over the S keys
    k, v = cache[:, :S, :d], cache[:, :S, d:2 * d]
    want = lm_ref.attention_core(q.float()[:, None], k.float(), v.float(), lm_ref.expand_mask(valid, torch.float32, 1), H)[:, 0]
    assert torch.allclose(want[2], v.float()[2].mean(0), atol=1e-5)      # the oracle's own uniform row
    cg = cache.cuda()
    got = ops.attn_decode(q.cuda(), cg[:, :S, :d], cg[:, :S, d:2 * d], valid.cuda(), H)
    assert got.shape == (B, d) and got.dtype == dtype
    e = rel_err(got, want)
    print(f"attn_decode S={S} D={D} {dtype}: rel err {e:.3e}")
    assert e <= tol, f"S={S} D={D} {dtype}: {e:.3e} > {tol:.1e}"
    per_sample = [(got[b].float().cpu() - want[b]).abs().max().item() / want.abs().max().item() for b in range(B)]
    assert max(per_sample) <= tol, per_sample
    # the running mask of a cache: a uint8 view with a row stride
    mask = torch.zeros(B, cap, dtype=torch.uint8)
    mask[:, :S] = valid
    got2 = ops.attn_decode(q.cuda(), cg[:, :S, :d], cg[:, :S, d:2 * d], mask.cuda()[:, :S], H)
    assert torch.equal(got, got2)


@pytest.mark.parametrize("D", [16, 32])
def test_attn_decode_small_heads(D):
    from mmgl_amd import ops
    from oracle import lm_ref
    B, H, S = 2, 4, 19
    g = torch.Generator().manual_seed(D)
    for dtype, tol in ((torch.float32, 1e-3), (torch.bfloat16, 2e-2)):
        q, k, v = (torch.randn(B, n, H * D, generator=g).to(dtype) for n in (1, S, S))
        valid = torch.rand(B, S, generator=g) > 0.4
        valid[:, 0] = True
        q = (q.float() * D ** -0.5).to(dtype)
        want = lm_ref.attention_core(q.float(), k.float(), v.float(), lm_ref.expand_mask(valid, torch.float32, 1), H)[:, 0]
        got = ops.attn_decode(q[:, 0].cuda(), k.cuda(), v.cuda(), valid.cuda(), H)
        assert rel_err(got, want) <= tol, (D, dtype, rel_err(got, want))
