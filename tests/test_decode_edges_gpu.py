"""-m gpu: the kernels of csrc/decode.hip at the states and addresses tests/test_decode_kernels_gpu.py and tests/test_decode_lora_gpu.py
do not visit, against fp64 references of the same storage-rounded operands computed on the GPU (decode_ref.SkinnyRef, decode_ref.attn_decode_ref).

GEMM groups -- every element within  u |want| + 2^-16 mag  (decode_ref.SkinnyRef: the half ulp of the one rounding store plus 256 fp32
roundings on the magnitude sum), after asserting from the reference alone that a dropped 64-wide K unit, and a dropped rank-r term, leave
that bound on >= 25 % of the elements:
  B  the MFMA kernel's K loop: a W ring of 4 units per lane, 4 (16-row workgroups) or 8 (8-row) K slots -- fewer units than slots, a ragged
     last trip, a partial second round of the ring -- times the 1 / 2 / 4 x-tile variants (M around 16 and 32); N = 8, 8 x odd, and
     either side of the width at which workgroups take 16 rows (N / 16 >= compute units).  Bias, residual, ReLU and scale together.
  C  operands as windows of larger buffers that hold NaN everywhere else (free ldx / ldw / lda / ldb, the output and the residual inside
     a buffer whose other bytes must not change): nothing outside a window is read or written.  Aligned windows run the MFMA kernel;
     8-byte-aligned bases, ldx % 8 or ldw % 8 fall to the plain kernel.  With an adapter: the vector and the scalar paths of stage 1 and
     of the epilogue term, and the workspace (holds t = x A^T on return, nothing past M r floats is written).
  D  the plain kernel's and stage 1's grid edges (4 columns / adapter rows and 8 rows of x per workgroup), bf16 and fp32.
Attention groups (E) -- 1e-3 fp32 / 2e-2 bf16 of the largest reference magnitude, the tolerances of tests/test_decode_kernels_gpu.py,
per sample.  I = 1024 VEC / D keys per workgroup loop trip, KPI = 64 VEC / D keys per wave and load (VEC = 8 bf16, 4 fp32):
  E1 one valid key per sample, at every position of two trips and a tail: the output is that key's value row, bitwise (masked keys weigh
     exp(-FLT_MAX - m) = 0, the valid one exp(0) = 1, the division is by 1).
  E2 only the keys one wave / one lane group / the tail owns are valid; E3 scores spanning +-12 with the maximum last or first (the
     online-softmax rescale); E4 NaN in every key row past S, pad column and q pad, mask bytes past S set; E5 refusals leave `out` alone.
  Each E2 / E3 case first asserts from the reference that the all-valid and the uniform result lie more than 10 tolerances away."""
import pytest
import torch

from decode_ref import SkinnyRef, attn_decode_ref

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="fp32")]
NAN = float("nan")
SCALING = 2.0


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _window(g, rows, cols, dtype, scale=1.0, ld=None, col0=0, row0=0, pad_rows=0, fill=NAN):
    """A random [rows, cols] window at (row0, col0) of a [row0 + rows + pad_rows, ld] buffer that holds `fill` everywhere else."""
    buf = torch.full((row0 + rows + pad_rows, ld or cols), fill, device="cuda", dtype=dtype)
    win = buf[row0:row0 + rows, col0:col0 + cols]
    win.copy_((torch.randn(rows, cols, device="cuda", generator=g) * scale).to(dtype))
    return win


def _dense(g, M, N, K, dtype, r=None):
    x = _window(g, M, K, dtype)
    w = _window(g, N, K, dtype, K ** -0.5)
    b = _window(g, 1, N, dtype)[0]
    res = _window(g, M, N, dtype)
    if r is None:
        return x, w, b, res
    return x, w, b, res, _window(g, r, K, dtype, K ** -0.5), _window(g, N, r, dtype, r ** -0.5)     # t ~ N(0, 1), t B^T ~ N(0, 1)


# ------------------------------------------------------------------------------------------ B: the MFMA kernel's ring and tail states
def _mfma_states(N, K, rows, group):
    from mmgl_amd import ops
    cases = [_dense(_gen(K * 100 + M), M, N, K, BF16) for M in rows]
    refs = [SkinnyRef(x, w, b, True, 0.5, res) for x, w, b, res in cases]
    SkinnyRef.assert_can_fail(refs, BF16, f"M in {rows}, {N}x{K}")         # pooled: at N = 8 one call has 8 elements, half of them under the ReLU
    for M, (x, w, b, res), ref in zip(rows, cases, refs):
        y = ops.gemm_skinny(x, w, b, res, act=1, out_scale=0.5)
        ref.check(y, f"{M}x{N}x{K}", group, can_fail=False)
        assert torch.equal(y, ops.gemm_skinny(x, w, b, res, act=1, out_scale=0.5)), f"{M}x{N}x{K}: two runs differ"


def _rows(K, more_at):
    return [1, 17, 33, 64] + ([16, 32] if K in more_at else [])


@pytest.mark.parametrize("K", [64, 128, 192, 256, 320, 1088, 1344, 1792])            # K-loop trips 1, 1, 1, 1, 2, 5, 6, 7
def test_mfma_16_row_workgroups(K):
    N16 = 16 * torch.cuda.get_device_properties(0).multi_processor_count              # the narrowest N whose workgroups take 16 rows
    _mfma_states(N16, K, _rows(K, (320, 1344)), "B")


@pytest.mark.parametrize("K", [64, 320, 512, 576, 2112, 3136, 3648])                 # K-loop trips 1, 1, 1, 2, 5, 7, 8
def test_mfma_8_row_workgroups(K):
    _mfma_states(768, K, _rows(K, (320, 2112)), "B")


@pytest.mark.parametrize("N", [8, 24, "N16 - 16", "N16 + 8"])
def test_mfma_width_edges(N):
    """One workgroup, 8 x odd, and the widths just below / just above 16 x compute units (8-row workgroups on either side: N16 + 8 is
    no multiple of 16; N16 itself is test_mfma_16_row_workgroups)."""
    N16 = 16 * torch.cuda.get_device_properties(0).multi_processor_count
    N = {"N16 - 16": N16 - 16, "N16 + 8": N16 + 8}.get(N, N)
    _mfma_states(N, 576, [1, 33], "B")


# ------------------------------------------------------------------------------------------ C: strides, alignment fallback, NaN outside
C_SHAPE = (33, 768, 576)


def _windows(g, dtype, xcol=8, wcol=8, ldx=None, ldw=None):
    M, N, K = C_SHAPE
    x = _window(g, M, K, dtype, ld=ldx or K + 24, col0=xcol, pad_rows=3)
    w = _window(g, N, K, dtype, K ** -0.5, ld=ldw or K + 40, col0=wcol, pad_rows=5)
    b = _window(g, 1, N, dtype, ld=N + 16, col0=8)[0]
    res = _window(g, M, N, dtype, ld=N + 24, col0=8, row0=1, pad_rows=1)
    outbuf = torch.full((M + 2, N + 24), 7.0, device="cuda", dtype=dtype)
    return x, w, b, res, outbuf, outbuf[1:1 + M, 8:8 + N]


def _outside_unchanged(outbuf):
    M, N, _ = C_SHAPE
    keep = torch.ones_like(outbuf, dtype=torch.bool)
    keep[1:1 + M, 8:8 + N] = False
    assert torch.equal(outbuf[keep], torch.full_like(outbuf, 7.0)[keep]), "bytes outside the output window changed"


@pytest.mark.parametrize("how", ["aligned", "bases at column 4", "ldx = K + 4", "ldw = K + 4"])
def test_windows_of_nan_buffers(how):
    from mmgl_amd import ops
    M, N, K = C_SHAPE
    kw = {"aligned": {}, "bases at column 4": dict(xcol=4, wcol=4), "ldx = K + 4": dict(xcol=0, ldx=K + 4),
          "ldw = K + 4": dict(wcol=0, ldw=K + 4)}[how]
    x, w, b, res, outbuf, out = _windows(_gen(31), BF16, **kw)
    mfma = x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0 and x.stride(0) % 8 == 0 and w.stride(0) % 8 == 0
    assert mfma == (how == "aligned") and x.stride(0) > K and w.stride(0) > K and res.stride(0) == out.stride(0)
    ref = SkinnyRef(x, w, b, True, 0.5, res)
    ops.gemm_skinny(x, w, b, res, act=1, out_scale=0.5, out=out)
    ref.check(out, f"windows, {how}", "C")
    _outside_unchanged(outbuf)
    first = out.clone()
    ops.gemm_skinny(x, w, b, res, act=1, out_scale=0.5, out=out)
    assert torch.equal(first, out), "two runs differ"


@pytest.mark.parametrize("abcol", [8, 4])                    # 8: the 8-element vector loads of stage 1 and of the epilogue term; 4: scalar
@pytest.mark.parametrize("r", [8, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lora_windows_of_nan_buffers(dtype, r, abcol):
    """bf16: column 8 is 16-byte aligned, column 4 is not.  fp32: column 8 is 32-byte aligned (the vector path), column 4 16-byte."""
    from mmgl_amd import ops
    M, N, K = C_SHAPE
    g = _gen(37 + r)
    x, w, b, res, outbuf, out = _windows(g, dtype)
    A = _window(g, r, K, dtype, K ** -0.5, ld=K + 24, col0=abcol, pad_rows=2)
    Bm = _window(g, N, r, dtype, r ** -0.5, ld=r + 8, col0=abcol, pad_rows=3)
    assert A.stride(0) > K and Bm.stride(0) > r and Bm.data_ptr() % (8 * Bm.element_size()) == (0 if abcol == 8 else 4 * Bm.element_size())
    ws = torch.full((M * r + 64,), -3.0, device="cuda")
    ref = SkinnyRef(x, w, b, True, 0.5, res, A, Bm, SCALING)
    ops.gemm_skinny_lora(x, w, A, Bm, SCALING, b, res, act=1, out_scale=0.5, out=out, workspace=ws)
    ref.check(out, f"lora windows {dtype} r={r} A, B at column {abcol}", "C")
    _outside_unchanged(outbuf)
    # the workspace: t = x A^T in fp32 on return, nothing behind it written
    assert torch.equal(ws[M * r:], torch.full((64,), -3.0, device="cuda")), "the workspace was written past M * r floats"
    t, t_mag = x.double() @ A.double().t(), x.double().abs() @ A.double().abs().t()
    t_err = (ws[:M * r].view(M, r).double() - t).abs()
    print(f"[bound C] workspace t {dtype} r={r} column {abcol}: max err/bound {(t_err / (2.0 ** -16 * t_mag)).max().item():.3f}")
    assert (t_err <= 2.0 ** -16 * t_mag).all(), "the workspace does not hold x A^T"
    first = out.clone()
    ops.gemm_skinny_lora(x, w, A, Bm, SCALING, b, res, act=1, out_scale=0.5, out=out, workspace=ws)
    assert torch.equal(first, out), "two runs differ"


# ------------------------------------------------------------------------------------------ D: the plain kernel's and stage 1's grid edges
@pytest.mark.parametrize("K", [1, 63, 65, 1088])
@pytest.mark.parametrize("dtype", DTYPES)
def test_plain_kernel_grid_edges(dtype, K):
    """4 output columns and 8 rows of x per workgroup: N = 3, 4, 5 and M = 8, 9, 64; K below, at and above a wave's 64 lanes.  No ReLU
    here (tests/test_decode_kernels_gpu.py runs it on this kernel): 24 elements are too few to count on the share a ReLU leaves."""
    from mmgl_amd import ops
    for M in (8, 9, 64):
        for N in (3, 4, 5):
            x, w, b, res = _dense(_gen(K * 1000 + M * 10 + N), M, N, K, dtype)
            ref = SkinnyRef(x, w, b, False, 0.5, res)
            y = ops.gemm_skinny(x, w, b, res, out_scale=0.5)
            ref.check(y, f"plain {dtype} {M}x{N}x{K}", "D")
            assert torch.equal(y, ops.gemm_skinny(x, w, b, res, out_scale=0.5))


@pytest.mark.parametrize("r", [1, 4, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lora_stage_one_grid_edges(dtype, r):
    from mmgl_amd import ops
    N, K = 72, 40
    for M in (8, 9):
        x, w, b, res, A, Bm = _dense(_gen(r * 100 + M), M, N, K, dtype, r)
        ref = SkinnyRef(x, w, b, False, 0.5, res, A, Bm, SCALING)
        y = ops.gemm_skinny_lora(x, w, A, Bm, SCALING, b, res, out_scale=0.5)
        ref.check(y, f"plain lora {dtype} {M}x{N}x{K} r={r}", "D")
        assert torch.equal(y, ops.gemm_skinny_lora(x, w, A, Bm, SCALING, b, res, out_scale=0.5))


# ------------------------------------------------------------------------------------------ E: single-query attention
TOL = {F32: 1e-3, BF16: 2e-2}
H = 2


def _trip(dtype, D):
    vec = 8 if dtype == BF16 else 4
    return 1024 * vec // D, 64 * vec // D             # I: keys per workgroup loop trip; KPI: keys per wave and load instruction


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _per_sample(a, want):
    """max|a[b] - want[b]| / max|want[b]| for every sample b: the tolerances' measure, per sample."""
    return ((a.double() - want).abs().amax(1) / want.abs().amax(1)).cpu()


def _attn_check(got, want, dtype, what, group):
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    e = _per_sample(got, want)
    print(f"[attn {group}] {what}: max rel err {e.max().item():.3e}")
    assert (e <= TOL[dtype]).all(), f"{what}: per-sample rel err {[f'{v:.2e}' for v in e.tolist()]} > {TOL[dtype]:.0e}"


@pytest.mark.parametrize("D", [16, 32, 64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_valid_key_at_every_position_bitwise(dtype, D):
    """Sample b attends key b alone; k and v are one sample expanded over the batch (batch stride 0)."""
    from mmgl_amd import ops
    I, KPI = _trip(dtype, D)
    S = 2 * I + KPI + 3
    g = torch.Generator().manual_seed(D)
    q = (_randn(g, S, H * D) * D ** -0.5).to(dtype).cuda()
    k, v = (_randn(g, 1, S, H * D).to(dtype).cuda() for _ in range(2))
    valid = torch.eye(S, dtype=torch.bool, device="cuda")
    out = ops.attn_decode(q, k.expand(S, S, H * D), v.expand(S, S, H * D), valid, H)
    wrong = (out != v[0]).any(1).nonzero().flatten().tolist()
    assert not wrong, f"{dtype} D={D} S={S}: the output is not the value row of key {wrong[:32]} ({len(wrong)} keys)"
    assert torch.equal(out, v[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_valid_key_in_cache_slabs_bitwise(dtype):
    """The same with every sample's own keys and values, as column slabs of wider cache rows."""
    from mmgl_amd import ops
    B = S = 40
    D = 64
    d = H * D
    g = torch.Generator().manual_seed(5)
    q = (_randn(g, B, d) * D ** -0.5).to(dtype).cuda()
    cache = _randn(g, B, S + 5, 2 * d + 16).to(dtype).cuda()
    k, v = cache[:, :S, 8:8 + d], cache[:, :S, 8 + d:8 + 2 * d]
    out = ops.attn_decode(q, k, v, torch.eye(S, dtype=torch.bool, device="cuda"), H)
    want = v[torch.arange(B), torch.arange(B)]
    wrong = (out != want).any(1).nonzero().flatten().tolist()
    assert not wrong, f"{dtype}: the output is not the value row of key {wrong}"


def _ownership_patterns(S, I, KPI):
    s = torch.arange(S)
    pats = {f"the keys of wave {w}": (s // KPI) % 4 == w for w in range(4)}
    pats["the keys of lane group 0"] = s % KPI == 0
    pats[f"the keys of lane group {KPI - 1}"] = s % KPI == KPI - 1
    pats["the tail behind two trips"] = s >= 2 * I
    pats["all but the first trip"] = s >= I
    pats["the last key"] = s == S - 1
    return pats


def ownership_case(dtype, D):
    """CPU tensors of E2: one sample per pattern.  q has norm 2 per head (scores ~ N(0, 4)): a few keys carry each row, so that the
    result over a subset of the keys lies far from the result over all of them."""
    I, KPI = _trip(dtype, D)
    S = 2 * I + KPI + 3
    pats = _ownership_patterns(S, I, KPI)
    B = len(pats)
    g = torch.Generator().manual_seed(1000 + D)
    q = _randn(g, B, H, D)
    q = (2.0 * q / q.norm(dim=-1, keepdim=True)).reshape(B, H * D).to(dtype)
    k, v = (_randn(g, B, S, H * D).to(dtype) for _ in range(2))
    return q, k, v, torch.stack(list(pats.values())), list(pats)


def assert_far(want, other, dtype, what):
    gap = _per_sample(other, want)
    assert (gap > 10 * TOL[dtype]).all(), f"{what}: only {gap.min().item():.3f} of the largest magnitude away (10 x tolerance = {10 * TOL[dtype]})"


@pytest.mark.parametrize("D,dtype", [(128, BF16), (64, F32), (16, BF16)], ids=["128-bf16", "64-fp32", "16-bf16"])
def test_keys_owned_by_one_wave_lane_group_or_trip(D, dtype):
    from mmgl_amd import ops
    q, k, v, valid, names = (t.cuda() if torch.is_tensor(t) else t for t in ownership_case(dtype, D))
    want = attn_decode_ref(q, k, v, valid, H)
    assert_far(want, attn_decode_ref(q, k, v, torch.ones_like(valid), H), dtype, "from the result over every key")
    assert_far(want, v.double().mean(1), dtype, "from the uniform mean")
    got = ops.attn_decode(q, k, v, valid, H)
    for b, name in enumerate(names):
        _attn_check(got[b:b + 1], want[b:b + 1], dtype, f"{dtype} D={D}, valid: {name}", "E2")


def wide_score_case(dtype, D):
    """CPU tensors of E3: q of norm 4 per head; sample 0 holds the keys of every head by ascending score, sample 1 by descending."""
    I, _ = _trip(dtype, D)
    S = 3 * I + 5
    g = torch.Generator().manual_seed(2000 + D)
    q = _randn(g, 1, H, D)
    q = (4.0 * q / q.norm(dim=-1, keepdim=True)).to(dtype)
    k, v = (_randn(g, S, H, D).to(dtype) for _ in range(2))
    order = torch.einsum("hd,shd->hs", q[0].double(), k.double()).argsort(dim=1)        # [H, S] ascending
    idx = torch.stack([order, order.flip(1)])                                            # [2, H, S]
    pick = lambda t: torch.stack([torch.stack([t[idx[b, h], h] for h in range(H)], 1) for b in range(2)]).reshape(2, S, H * D)
    return q.reshape(1, H * D).expand(2, H * D).contiguous(), pick(k), pick(v)


@pytest.mark.parametrize("D,dtype", [(64, BF16), (128, BF16), (64, F32), (128, F32), (16, BF16)],
                         ids=["64-bf16", "128-bf16", "64-fp32", "128-fp32", "16-bf16"])
def test_wide_scores_with_the_maximum_last_and_first(D, dtype):
    from mmgl_amd import ops
    q, k, v = (t.cuda() for t in wide_score_case(dtype, D))
    valid = torch.ones(2, k.shape[1], dtype=torch.bool, device="cuda")
    want = attn_decode_ref(q, k, v, valid, H)
    assert (want[0] - want[1]).abs().max().item() < 1e-12                                # the same keys in two orders
    assert_far(want, v.double().mean(1), dtype, "from the uniform mean")
    got = ops.attn_decode(q, k, v, valid, H)
    for b, name in enumerate(("ascending", "descending")):
        _attn_check(got[b:b + 1], want[b:b + 1], dtype, f"{dtype} D={D} S={k.shape[1]}, scores {name}", "E3")


@pytest.mark.parametrize("D", [32, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_nothing_past_the_keys_or_outside_the_slabs(dtype, D):
    """NaN in the cache rows past S, in the pad columns around the K|V slabs and around q; the mask bytes past S are 1.  Sample 0 attends
    every key, sample 1 a random subset, sample 2 none (uniform over exactly S keys)."""
    from mmgl_amd import ops
    I, KPI = _trip(dtype, D)
    B, d = 3, H * D
    for S in sorted({1, KPI - 1, KPI, I + 1}):
        g = torch.Generator().manual_seed(S * 10 + D)
        qbuf = torch.full((B, d + 16), NAN, dtype=dtype)
        qbuf[:, 8:8 + d] = (_randn(g, B, d) * D ** -0.5).to(dtype)
        cache = torch.full((B, S + 5, 2 * d + 16), NAN, dtype=dtype)
        cache[:, :S, 8:8 + 2 * d] = _randn(g, B, S, 2 * d).to(dtype)
        mask = torch.ones(B, S + 5, dtype=torch.uint8)
        mask[1, :S] = torch.rand(S, generator=g) > 0.3
        mask[1, 0] = 1
        mask[2, :S] = 0
        qbuf, cache, mask = qbuf.cuda(), cache.cuda(), mask.cuda()
        q, k, v, valid = qbuf[:, 8:8 + d], cache[:, :S, 8:8 + d], cache[:, :S, 8 + d:8 + 2 * d], mask[:, :S]
        assert q.stride(0) > d and k.stride(1) > 2 * d and valid.stride(0) > S
        want = attn_decode_ref(q, k, v, valid, H)
        assert (want[2] - v[2].double().mean(0)).abs().max().item() < 1e-12
        _attn_check(ops.attn_decode(q, k, v, valid, H), want, dtype, f"{dtype} D={D} S={S}, NaN outside", "E4")


def test_refused_calls_leave_the_output_alone():
    from mmgl_amd import ops
    B, S = 2, 9
    valid = torch.ones(B, S, dtype=torch.bool, device="cuda")

    def refused(q, k, v):
        out = torch.full((B, q.shape[1]), 7.0, device="cuda", dtype=q.dtype)
        with pytest.raises(ValueError):
            ops.attn_decode(q, k, v, valid, H, out=out)
        torch.cuda.synchronize()
        assert torch.equal(out, torch.full_like(out, 7.0))

    ones = lambda *shape: torch.ones(*shape, device="cuda", dtype=BF16)
    refused(ones(B, H * 48), ones(B, S, H * 48), ones(B, S, H * 48))                    # head_dim 48
    d = H * 64
    cache = ones(B, S, 2 * d + 16)
    refused(ones(B, d), cache[:, :, 4:4 + d], cache[:, :, 4 + d:4 + 2 * d])             # slabs at column 4: 8-byte aligned
    refused(ones(B, d + 4)[:, :d], cache[:, :, :d], cache[:, :, d:2 * d])               # ldq = d + 4: rows not 16-byte aligned
    out = torch.full((B, d), 7.0, device="cuda", dtype=BF16)
    assert ops.attn_decode(ones(B, d), cache[:, :, :d], cache[:, :, d:2 * d], valid, H, out=out) is out   # the accepted twin of the three
    assert torch.equal(out, torch.ones_like(out))
