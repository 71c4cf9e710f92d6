"""-m gpu: mmgl_attn_decode_relbias_fwd through ops.attn_decode_relbias against the fp64 reference of the storage-rounded operands
(tests/t5_decode_ref.py).  Tolerances: the project's for single-query attention (tests/test_decode_edges_gpu.py), per sample -- 1e-3 of
the largest reference magnitude in fp32, 2e-2 in bf16.  I = 1024 VEC / D keys per workgroup loop trip, KPI = 64 VEC / D keys per wave and
load (VEC = 8 bf16, 4 fp32).
  a  sample b has bias -1e30 at every distance but S - 1 - b: the output is the value row of key b, bitwise, at every position of two
     trips and a tail (the other keys weigh exp(-1e30 - m) = 0, the chosen one exp(0) = 1, the division is by 1).
  b  random operands, a table drawn N(0, 2), H = 2 and 3, S from 1 to two trips and a tail, k and v as slabs of wider cache rows,
     ld_bias > S.  For S > 2 the case first asserts from the reference alone that the three wrong references (the distance taken as s, no
     bias, head h ^ 1's bias row) lie more than 10 tolerances away on every sample.  Not for S = 1 and 2: over one key the softmax is 1
     whatever the score, over two only the difference of two bias words counts, so a wrong reference can coincide with the right one.
  c  NaN in every key row past S, in the pad columns, around q and in bias past S; out sits inside a NaN buffer that must not change.
  d  refused calls leave out alone."""
import pytest
import torch

import t5_decode_ref as R
from bounds import Slab

pytestmark = pytest.mark.gpu

BF16, F32 = R.BF16, R.F32
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="fp32")]
NAN = float("nan")


def _check(got, want, dtype, what, group):
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    e = R.per_sample(got, want.to(got.device))
    print(f"[relbias {group}] {what}: max rel err {e.max().item():.3e}")
    assert (e <= R.TOL[dtype]).all(), f"{what}: per-sample rel err {[f'{v:.2e}' for v in e.tolist()]} > {R.TOL[dtype]:.0e}"


@pytest.mark.parametrize("D", [64, 32])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_distance_per_sample_bitwise(dtype, D):
    """k and v are one sample expanded over the batch (batch stride 0); every head of sample b keeps the key at distance S - 1 - b."""
    from mmgl_amd import ops
    H = 2
    I, KPI = R.trip(dtype, D)
    S = 2 * I + KPI + 3
    g = torch.Generator().manual_seed(D)
    q = torch.randn(S, H * D, generator=g).to(dtype).cuda()
    k, v = (torch.randn(1, S, H * D, generator=g).to(dtype).cuda() for _ in range(2))
    for b0 in range(0, S, 64):                       # the bias rows are per call, not per sample: one call per sample, 64 checked per sync
        outs = []
        for b in range(b0, min(S, b0 + 64)):
            bias = torch.full((H, S + 3), -1e30, device="cuda")
            bias[:, S - 1 - b] = 0.25 * (b % 5)
            outs.append(ops.attn_decode_relbias(q[b:b + 1], k, v, bias, H)[0])
        got = torch.stack(outs)
        wrong = (got != v[0, b0:b0 + got.shape[0]]).any(1).nonzero().flatten().tolist()
        assert not wrong, f"{dtype} D={D} S={S}: the output is not the value row of key {[b0 + w for w in wrong][:32]}"


def test_one_distance_per_sample_bitwise_over_a_batch():
    """The bias rows are per head and shared by the samples of a launch, so the batched form of the case varies the heads: head h of
    every sample keeps key (shift + h) % S, each sample with its own keys and values."""
    from mmgl_amd import ops
    dtype, D, H = BF16, 64, 4
    I, KPI = R.trip(dtype, D)
    S = I + KPI + 3
    g = torch.Generator().manual_seed(7)
    q = torch.randn(3, H * D, generator=g).to(dtype).cuda()
    k, v = (torch.randn(3, S, H * D, generator=g).to(dtype).cuda() for _ in range(2))
    for shift in (0, 1, KPI, I - 1, I, S - 4):
        bias = torch.full((H, S), -1e30, device="cuda")
        keep = [(shift + h) % S for h in range(H)]                     # the key index head h keeps
        for h, s in enumerate(keep):
            bias[h, S - 1 - s] = 0.0
        got = ops.attn_decode_relbias(q, k, v, bias, H).view(3, H, D)
        want = torch.stack([v[:, s].view(3, H, D)[:, h] for h, s in enumerate(keep)], dim=1)
        assert torch.equal(got, want), f"shift {shift}: heads keep keys {keep}"


def _sizes(dtype, D=64):
    I, KPI = R.trip(dtype, D)
    return sorted({1, 2, 17, KPI + 1, I - 1, I, I + 1, 2 * I + KPI + 3})


@pytest.mark.parametrize("H", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_random_operands_in_cache_slabs(dtype, H):
    from mmgl_amd import ops
    D = 64
    d = H * D
    for S in _sizes(dtype):
        q, cache, bias, _ = R.random_case(dtype, H, S, D)
        k, v = R.slabs(cache, S, d)
        want = R.attn_decode_relbias_ref(q, k, v, bias, H)
        if S > 2:
            for wrong in R.WRONG:
                gap = R.per_sample(R.attn_decode_relbias_ref(q, k, v, bias, H, wrong), want)
                assert (gap > 10 * R.TOL[dtype]).all(), f"S={S} {wrong}: only {gap.min().item():.3f} away (10 x tolerance = {10 * R.TOL[dtype]})"
        qc, cc, bc = q.cuda(), cache.cuda(), bias.cuda()
        kc, vc = R.slabs(cc, S, d)
        assert bc.stride(0) > S and kc.stride(1) > 2 * d
        got = ops.attn_decode_relbias(qc, kc, vc, bc, H)
        _check(got, want, dtype, f"{dtype} H={H} S={S}", "b")
        assert torch.equal(got, ops.attn_decode_relbias(qc, kc, vc, bc, H)), f"S={S}: two runs differ"


@pytest.mark.parametrize("D", [64, 128, 16])
@pytest.mark.parametrize("dtype", DTYPES)
def test_nothing_past_the_keys_or_outside_the_slabs(dtype, D):
    from mmgl_amd import ops
    H = 2
    I, KPI = R.trip(dtype, D)
    B, d = 3, H * D
    for S in sorted({1, KPI - 1, KPI, I + 1}):
        g = torch.Generator().manual_seed(S * 10 + D)
        qbuf = torch.full((B, d + 16), NAN, dtype=dtype)
        qbuf[:, 8:8 + d] = (torch.randn(B, d, generator=g) * D ** -0.5).to(dtype)
        cache = torch.full((B, S + 5, 2 * d + 16), NAN, dtype=dtype)
        cache[:, :S, 8:8 + 2 * d] = torch.randn(B, S, 2 * d, generator=g).to(dtype)
        bias = torch.full((H, S + 7), NAN)
        bias[:, :S] = torch.randn(H, S, generator=g) * 2.0
        qbuf, cache, bias = qbuf.cuda(), cache.cuda(), bias.cuda()
        q, (k, v) = qbuf[:, 8:8 + d], R.slabs(cache, S, d)
        want = R.attn_decode_relbias_ref(q, k, v, bias, H)
        out = Slab((B, d), dtype, NAN)
        assert ops.attn_decode_relbias(q, k, v, bias, H, out=out.v) is out.v
        _check(out.v, want, dtype, f"{dtype} D={D} S={S}, NaN outside", "c")
        assert out.untouched(), f"{dtype} D={D} S={S}: bytes around the output changed"


def test_refused_calls_leave_the_output_alone():
    from mmgl_amd import ops
    B, S, H = 2, 9, 2

    def refused(q, k, v, bias):
        out = torch.full((B, q.shape[1]), 7.0, device="cuda", dtype=q.dtype)
        with pytest.raises(ValueError):
            ops.attn_decode_relbias(q, k, v, bias, H, out=out)
        torch.cuda.synchronize()
        assert torch.equal(out, torch.full_like(out, 7.0))

    ones = lambda *shape: torch.ones(*shape, device="cuda", dtype=BF16)
    zeros = torch.zeros(H, S + 3, device="cuda")
    refused(ones(B, H * 48), ones(B, S, H * 48), ones(B, S, H * 48), zeros)                    # head_dim 48
    d = H * 64
    cache = ones(B, S, 2 * d + 16)
    refused(ones(B, d), cache[:, :, 4:4 + d], cache[:, :, 4 + d:4 + 2 * d], zeros)             # slabs at column 4: 8-byte aligned
    refused(ones(B, d + 4)[:, :d], cache[:, :, :d], cache[:, :, d:2 * d], zeros)               # ldq = d + 4: rows not 16-byte aligned
    refused(ones(B, d), cache[:, :, :d], cache[:, :, d:2 * d], zeros[:, :S - 1])               # fewer bias words than keys
    refused(ones(B, d), cache[:, :, :d], cache[:, :, d:2 * d], zeros.double())                 # bias not fp32
    out = torch.full((B, d), 7.0, device="cuda", dtype=BF16)
    assert ops.attn_decode_relbias(ones(B, d), cache[:, :, :d], cache[:, :, d:2 * d], zeros, H, out=out) is out   # the accepted twin
    assert torch.equal(out, torch.ones_like(out))
