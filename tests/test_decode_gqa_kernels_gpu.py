"""-m gpu: the two kernels of the Llama-family decode step (csrc/decode.hip): mmgl_attn_decode_gqa_fwd through ops.attn_decode(...,
num_kv_heads) and mmgl_rope_kv_append through ops.rope_kv_append.

Attention -- the fp64 reference is decode_ref.attn_decode_ref on K / V expanded to H heads (repeat_interleave(G) over the head axis:
transformers' repeat_kv), the bounds are those of tests/test_decode_edges_gpu.py: per sample 1e-3 (fp32) / 2e-2 (bf16) of the sample's
largest reference magnitude.  The kernel keeps attn_decode_kernel's lane layout: I = 1024 VEC / D keys per workgroup loop trip, KPI =
64 VEC / D keys per wave and load (VEC = 8 bf16, 4 fp32); a workgroup serves up to 8 query heads of one key/value head, G = 12 takes
two blocks of 6.

Rotary -- the reference is the fp64 rotate_half formula on the table row: out_lo = x cos - y sin, out_hi = y cos + x sin.  With
a = |x cos| + |y sin| (resp. |y cos| + |x sin|) every element must satisfy |got - want| <= 2^-21 a in fp32 (two products and one
sum, each rounded once at 2^-24 relative, leave 3 x 2^-24 a < 2^-22 a; 2^-21 a allows a few roundings) and 2^-8 a in bf16 (the one
rounding to bf16 is 2^-9 relative of |want| <= a; the fp32 arithmetic in front of it is 2^-22 a; the rest is margin)."""
import pytest
import torch

from decode_ref import attn_decode_ref

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="fp32")]
NAN = float("nan")
TOL = {F32: 1e-3, BF16: 2e-2}
GROUPS = [(4, 2), (4, 1), (6, 2), (8, 1), (12, 1)]           # G = 2, 4, 3 (a block of 4 with one idle slot), 8, 12 (two blocks of 6)


def _trip(dtype, D):
    vec = 8 if dtype == BF16 else 4
    return 1024 * vec // D, 64 * vec // D             # I: keys per workgroup loop trip; KPI: keys per wave and load instruction


def _expand(t, H, Hkv):
    """[B, S, Hkv*D] -> [B, S, H*D]: key/value head j serves query heads j G .. j G + G - 1."""
    B, S, kd = t.shape
    return t.reshape(B, S, Hkv, kd // Hkv).repeat_interleave(H // Hkv, dim=2).reshape(B, S, -1)


def _ref(q, k, v, valid, H, Hkv):
    return attn_decode_ref(q, _expand(k, H, Hkv), _expand(v, H, Hkv), valid, H)


def _per_sample(a, want):
    return ((a.double() - want).abs().amax(1) / want.abs().amax(1)).cpu()


def _check(got, want, dtype, what):
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    e = _per_sample(got, want)
    print(f"[gqa decode] {what}: max rel err {e.max().item():.3e}")
    assert (e <= TOL[dtype]).all(), f"{what}: per-sample rel err {[f'{x:.2e}' for x in e.tolist()]} > {TOL[dtype]:.0e}"


def _case(seed, B, S, H, Hkv, D, dtype, qnorm=None):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, D, generator=g)
    q = q * D ** -0.5 if qnorm is None else qnorm * q / q.norm(dim=-1, keepdim=True)
    k, v = (torch.randn(B, S, Hkv * D, generator=g).to(dtype).cuda() for _ in range(2))
    return q.reshape(B, H * D).to(dtype).cuda(), k, v, g


@pytest.mark.parametrize("D", [16, 64, 128])
@pytest.mark.parametrize("H,Hkv", GROUPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_mapping(dtype, H, Hkv, D):
    """q of norm 2 per head (scores ~ N(0, 4)): a few keys carry each row, so a query head that read another key/value head lands far
    from its reference -- asserted from the reference alone, against the result of the NEXT key/value head, where there is one."""
    from mmgl_amd import ops
    I, KPI = _trip(dtype, D)
    B, S = 3, KPI + 5
    q, k, v, g = _case(H * 1000 + Hkv * 100 + D, B, S, H, Hkv, D, dtype, qnorm=2.0)
    valid = (torch.rand(B, S, generator=g) > 0.2).cuda()
    valid[:, 0] = True
    want = _ref(q, k, v, valid, H, Hkv)
    if Hkv > 1:
        roll = lambda t: t.reshape(B, S, Hkv, D).roll(1, dims=2).reshape(B, S, Hkv * D)
        gap = _per_sample(_ref(q, roll(k), roll(v), valid, H, Hkv), want)
        assert (gap > 10 * TOL[dtype]).all(), f"the wrong key/value head is only {gap.min().item():.3f} away"
    got = ops.attn_decode(q, k, v, valid, H, num_kv_heads=Hkv)
    assert got.shape == (B, H * D) and got.dtype == dtype
    _check(got, want, dtype, f"{dtype} H={H} Hkv={Hkv} D={D} S={S}")
    assert torch.equal(got, ops.attn_decode(q, k, v, valid, H, num_kv_heads=Hkv)), "two runs differ"


@pytest.mark.parametrize("H,Hkv,D", [(4, 2, 64), (12, 1, 16), (8, 1, 128), (6, 2, 32)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_valid_key_at_every_position_bitwise(dtype, H, Hkv, D):
    """Sample b attends key b alone (k and v are one sample expanded over the batch, batch stride 0): out[b, h] is the value row of
    key/value head h // G at key b, bitwise -- masked keys weigh exp(-FLT_MAX - m) = 0, the valid one exp(0) = 1, the division is by 1."""
    from mmgl_amd import ops
    I, KPI = _trip(dtype, D)
    S = I + KPI + 3
    g = torch.Generator().manual_seed(D + H)
    q = (torch.randn(S, H * D, generator=g) * D ** -0.5).to(dtype).cuda()
    k, v = (torch.randn(1, S, Hkv * D, generator=g).to(dtype).cuda() for _ in range(2))
    valid = torch.eye(S, dtype=torch.bool, device="cuda")
    out = ops.attn_decode(q, k.expand(S, S, Hkv * D), v.expand(S, S, Hkv * D), valid, H, num_kv_heads=Hkv)
    want = _expand(v, H, Hkv)[0]
    wrong = (out != want).any(1).nonzero().flatten().tolist()
    assert not wrong, f"{dtype} H={H} Hkv={Hkv} D={D} S={S}: the output is not the value row of key {wrong[:32]} ({len(wrong)} keys)"
    per_head = (out != want).reshape(S, H, D).any(2).any(0)
    assert not per_head.any(), per_head.tolist()


@pytest.mark.parametrize("H,Hkv,D", [(4, 2, 64), (8, 1, 128), (12, 1, 16)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_trip_boundaries(dtype, H, Hkv, D):
    from mmgl_amd import ops
    I, KPI = _trip(dtype, D)
    for S in sorted({1, KPI - 1, KPI, KPI + 1, 4 * KPI - 1, 4 * KPI, 4 * KPI + 1, I - 1, I, I + 1}):
        q, k, v, g = _case(S * 7 + D, 2, S, H, Hkv, D, dtype)
        valid = torch.ones(2, S, dtype=torch.bool, device="cuda")
        valid[1] = (torch.rand(S, generator=g) > 0.3).cuda()
        valid[1, S - 1] = True                                                   # the last key of the tail counts
        _check(ops.attn_decode(q, k, v, valid, H, num_kv_heads=Hkv), _ref(q, k, v, valid, H, Hkv), dtype, f"{dtype} H={H} Hkv={Hkv} D={D} S={S}")


@pytest.mark.parametrize("H,Hkv,D", [(4, 2, 64), (8, 1, 128), (6, 2, 16)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_cache_slabs_masking_and_untouched_memory(dtype, H, Hkv, D):
    """K and V as the two column slabs of NaN-filled cache rows [B, capacity > S, 2*Hkv*D], q as a window of a NaN-filled fused row,
    mask bytes past S set.  Sample 1 has a random mask, sample 2 no valid key (uniform over exactly S keys).  The result is finite, equals
    the call on dense copies bitwise, and nothing but `out` is written."""
    from mmgl_amd import ops
    I, KPI = _trip(dtype, D)
    B, kd = 3, Hkv * D
    for S in (KPI + 1, I + 3):
        g = torch.Generator().manual_seed(S + D)
        qbuf = torch.full((B, (H + 2 * Hkv) * D + 16), NAN, dtype=dtype)
        qbuf[:, :H * D] = (torch.randn(B, H * D, generator=g) * D ** -0.5).to(dtype)
        cache = torch.full((B, S + 5, 2 * kd), NAN, dtype=dtype)
        cache[:, :S] = torch.randn(B, S, 2 * kd, generator=g).to(dtype)
        mask = torch.ones(B, S + 5, dtype=torch.uint8)
        mask[1, :S] = torch.rand(S, generator=g) > 0.3
        mask[1, 0] = 1
        mask[2, :S] = 0
        qbuf, cache, mask = qbuf.cuda(), cache.cuda(), mask.cuda()
        q, k, v, valid = qbuf[:, :H * D], cache[:, :S, :kd], cache[:, :S, kd:], mask[:, :S]
        assert q.stride(0) > H * D and k.stride(1) == 2 * kd and k.stride(0) > S * 2 * kd and valid.stride(0) > S
        before = [t.clone() for t in (qbuf, cache, mask)]
        outbuf = torch.full((B + 2, H * D), 7.0, dtype=dtype, device="cuda")
        out = ops.attn_decode(q, k, v, valid, H, out=outbuf[1:1 + B], num_kv_heads=Hkv)
        want = _ref(q, k, v, valid, H, Hkv)
        assert (want[2] - _expand(v, H, Hkv)[2].double().mean(0)).abs().max().item() < 1e-12
        _check(out, want, dtype, f"{dtype} H={H} Hkv={Hkv} D={D} S={S}, slabs of a NaN cache")
        dense = ops.attn_decode(q.contiguous(), k.contiguous(), v.contiguous(), valid.contiguous(), H, num_kv_heads=Hkv)
        assert torch.equal(out, dense), "the strided call differs from the dense one"
        for t, b4 in zip((qbuf, cache, mask), before):
            assert torch.equal(t.view(torch.uint8), b4.view(torch.uint8)), "an input buffer changed"
        assert (outbuf[0] == 7).all() and (outbuf[B + 1] == 7).all(), "rows around `out` changed"


def test_refused_calls_leave_the_output_alone():
    from mmgl_amd import ops
    B, S, H, D = 2, 9, 4, 64
    valid = torch.ones(B, S, dtype=torch.bool, device="cuda")
    ones = lambda *shape, dtype=BF16: torch.ones(*shape, device="cuda", dtype=dtype)

    def refused(q, k, v, Hkv, heads=H):
        out = torch.full((B, q.shape[1]), 7.0, device="cuda", dtype=q.dtype)
        with pytest.raises(ValueError):
            ops.attn_decode(q, k, v, valid, heads, out=out, num_kv_heads=Hkv)
        torch.cuda.synchronize()
        assert torch.equal(out, torch.full_like(out, 7.0))

    refused(ones(B, H * D), ones(B, S, 3 * D), ones(B, S, 3 * D), 3)                          # 3 key/value heads for 4 query heads
    refused(ones(B, H * D), ones(B, S, 2 * D), ones(B, S, 2 * D), 1)                          # rows of 2 heads, 1 announced
    refused(ones(B, H * D), ones(B, S, 2 * D, dtype=F32), ones(B, S, 2 * D, dtype=F32), 2)    # dtype mismatch
    refused(ones(B, H * 48), ones(B, S, 2 * 48), ones(B, S, 2 * 48), 2)                       # head_dim 48
    cache = ones(B, S, 4 * D + 16)
    refused(ones(B, H * D), cache[:, :, 4:4 + 2 * D], cache[:, :, 4 + 2 * D:4 + 4 * D], 2)    # slabs at column 4: 8-byte aligned
    refused(ones(B, H * D + 4)[:, :H * D], cache[:, :, :2 * D], cache[:, :, 2 * D:4 * D], 2)  # ldq = d + 4: rows not 16-byte aligned
    refused(ones(B, H * D), cache[:, :, :2 * D], cache[:, :, 2 * D:4 * D + 8], 2)             # k and v of different widths
    out = torch.full((B, H * D), 7.0, device="cuda", dtype=BF16)
    assert ops.attn_decode(ones(B, H * D), cache[:, :, :2 * D], cache[:, :, 2 * D:4 * D], valid, H, out=out, num_kv_heads=2) is out
    assert torch.equal(out, torch.ones_like(out))                                             # the accepted twin


# ------------------------------------------------------------------------------------------ rope_kv_append
ROPE_BOUND = {F32: 2.0 ** -21, BF16: 2.0 ** -8}
CAP = 5


def _rope_case(dtype, H, Hkv, D, B, col, seed, identity=False):
    g = torch.Generator().manual_seed(seed)
    width = (H + 2 * Hkv) * D
    qkv = torch.randn(B, width, generator=g).to(dtype).cuda()
    if identity:
        row = torch.stack([torch.ones(D // 2), torch.zeros(D // 2)], dim=-1)
    else:
        ang = torch.rand(D // 2, generator=g) * 6.0
        row = torch.stack([ang.cos(), ang.sin()], dim=-1)
    cache = torch.full((B, CAP, 2 * Hkv * D), -3.0, dtype=dtype, device="cuda")                # the sentinel
    return qkv, row.float().contiguous().cuda(), cache


def _rotate_ref(x, row, heads, D):
    """fp64 rotate_half of [B, heads*D] by the table row; returns (want, a): the value and the magnitude sum of its two products."""
    B = x.shape[0]
    xd = x.double().reshape(B, heads, D)
    lo, hi = xd[..., :D // 2], xd[..., D // 2:]
    co, si = row[:, 0].double(), row[:, 1].double()
    want = torch.cat([lo * co - hi * si, hi * co + lo * si], dim=-1)
    a = torch.cat([(lo * co).abs() + (hi * si).abs(), (hi * co).abs() + (lo * si).abs()], dim=-1)
    return want.reshape(B, heads * D), a.reshape(B, heads * D)


@pytest.mark.parametrize("col", [0, 4])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D", [16, 64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2), (8, 1)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rope_kv_append(dtype, H, Hkv, D, B, col):
    from mmgl_amd import ops
    qkv, row, cache = _rope_case(dtype, H, Hkv, D, B, col, seed=H * 100 + Hkv * 10 + D + B + col)
    src = qkv.clone()
    nq, nkv = H * D, Hkv * D
    ret = ops.rope_kv_append(qkv, row, cache[:, col], H, Hkv)
    assert ret is qkv
    for name, got, x, heads in (("q", qkv[:, :nq], src[:, :nq], H), ("k", cache[:, col, :nkv], src[:, nq:nq + nkv], Hkv)):
        want, a = _rotate_ref(x, row, heads, D)
        err = (got.double() - want).abs()
        ratio = (err / (ROPE_BOUND[dtype] * a).clamp_min(1e-300)).max().item()
        print(f"[rope_kv_append] {dtype} H={H} Hkv={Hkv} D={D} B={B} col={col} {name}: max err / bound {ratio:.3f}")
        assert (err <= ROPE_BOUND[dtype] * a).all(), f"{name}: {int((err > ROPE_BOUND[dtype] * a).sum())} elements over the bound (max ratio {ratio:.3f})"
        assert (want - x.double()).abs().max().item() > 0.1, "the rotation is no identity: the check can fail"
    assert torch.equal(cache[:, col, nkv:], src[:, nq + nkv:]), "v did not arrive bitwise"
    assert torch.equal(qkv[:, nq:], src[:, nq:]), "the k | v blocks of qkv changed"
    keep = torch.ones(CAP, dtype=torch.bool)
    keep[col] = False
    assert (cache[:, keep] == -3.0).all(), "cache columns other than `col` changed"


@pytest.mark.parametrize("H,Hkv,D", [(4, 2, 64), (8, 1, 16), (4, 4, 128)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rope_kv_append_identity_row_is_bitwise(dtype, H, Hkv, D):
    """Position 0 (cos 1, sin 0): q and k come back bitwise; the cache column is a window of wider rows (pad columns keep the sentinel)."""
    from mmgl_amd import ops
    B, col = 3, 2
    qkv, row, _ = _rope_case(dtype, H, Hkv, D, B, col, seed=D, identity=True)
    src = qkv.clone()
    wide = torch.full((B, CAP, 2 * Hkv * D + 16), -3.0, dtype=dtype, device="cuda")
    ops.rope_kv_append(qkv, row, wide[:, col, 8:8 + 2 * Hkv * D], H, Hkv)
    assert torch.equal(qkv, src), "q changed under the identity rotation"
    assert torch.equal(wide[:, col, 8:8 + 2 * Hkv * D], src[:, H * D:]), "k | v did not arrive bitwise"
    assert (wide[:, col, :8] == -3.0).all() and (wide[:, col, 8 + 2 * Hkv * D:] == -3.0).all(), "pad columns changed"


def test_rope_kv_append_refusals_leave_everything_alone():
    from mmgl_amd import ops
    H, Hkv, D, B = 4, 2, 64, 2
    qkv, row, cache = _rope_case(BF16, H, Hkv, D, B, 0, seed=1)
    src = qkv.clone()
    wide = torch.full((B, CAP, 2 * Hkv * D + 16), -3.0, dtype=BF16, device="cuda")
    for args in ((qkv, row, cache[:, 0], 4, 3),                                 # no divisor
                 (qkv, row, cache[:, 0, :D], H, Hkv),                           # a column of the wrong width
                 (qkv, row.double(), cache[:, 0], H, Hkv),                      # the table row is fp32
                 (qkv, row, cache.float()[:, 0], H, Hkv),                       # dtype mismatch
                 (qkv, row, wide[:, 0, 4:4 + 2 * Hkv * D], H, Hkv),             # the column 8-byte aligned
                 (torch.ones(B, (H + 2 * Hkv) * 48, device="cuda", dtype=BF16), torch.zeros(24, 2, device="cuda"),
                  torch.full((B, 4 * 48), -3.0, device="cuda", dtype=BF16), H, Hkv)):      # head_dim 48
        with pytest.raises(ValueError):
            ops.rope_kv_append(*args)
    torch.cuda.synchronize()
    assert torch.equal(qkv, src) and (cache == -3.0).all() and (wide == -3.0).all()
