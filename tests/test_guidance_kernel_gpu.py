"""-m gpu: ops.guidance_logits (mmgl_guidance_logits, csrc/guidance.hip) against the fp64 reference of tests/guidance_ref.py on the
stored inputs, under that module's per-element bound: half an ulp of the storage type at the result plus the fp32 evaluation term
  2 eps32 (g (|lc| + |lu|) + |lu|) + (eps32 / 2) ((1 + g)(L(V) + |lse_u|) + g (L(V) + |lse_c|)),   L(V) = 3 ln V + ceil(V / 1024) + 25
derived there by counting roundings (DESIGN.md 4.20 has the derivation and the largest measured error / bound ratio).  A reference
-inf must be met exactly.  tests/test_guidance_cpu.py shows that the bound catches wrong pairings and wrong formulas.

Addressing, in every case: the [2B, V] logits are carved from a slab of NaN canaries with row stride V + 3 and a base one element off
16-byte alignment; after the call the canaries and rows B .. 2B - 1 hold their bits."""
import math

import pytest
import torch

import guidance_ref

pytestmark = pytest.mark.gpu

G_VALUES = (0.0, 0.5, 1.5, 3.0)
DTYPES = [torch.bfloat16, torch.float32]


def _carve(x):
    """x [rows, V] on the CPU -> (slab, view): a NaN slab on the GPU and the [rows, V] view of it that holds x, row stride V + 3, its
    first element one element past a 16-byte boundary."""
    rows, V = x.shape
    ld = V + 3
    per16 = 16 // x.element_size()
    slab = torch.full((per16 + 1 + rows * ld + 8,), math.nan, dtype=x.dtype, device="cuda")
    off = (-(slab.data_ptr() // x.element_size()) % per16) + 1
    view = slab[off:off + rows * ld].view(rows, ld)[:, :V]
    assert view.data_ptr() % 16 == x.element_size() and view.stride() == (ld, 1)
    view.copy_(x)
    return slab, view


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _check(x, B, g, what):
    """One call on the carved copy of x [2B, V]; every element against the bound; the untouched bytes.  Returns the largest
    error / bound ratio and the result."""
    from mmgl_amd import ops
    V = x.shape[1]
    slab, view = _carve(x)
    before = slab.clone()
    out = ops.guidance_logits(view, B, g)
    assert out.data_ptr() == view.data_ptr() and out.shape == (B, V)
    got = view[:B].cpu().to(torch.float64)
    ref = guidance_ref.reference(x, B, g)
    bd = guidance_ref.bound(ref, g, V, x.dtype)
    want = ref["score"]
    dead = torch.isinf(want)
    assert torch.equal(got[dead], want[dead]), f"{what}: a -inf of the reference is not met exactly"
    assert torch.isfinite(got[~dead]).all(), f"{what}: a non-finite result where the reference is finite"
    err = (got - want).abs()[~dead]
    ratio = (err / bd[~dead]).max().item() if err.numel() else 0.0
    print(f"{what}: max error / bound {ratio:.3f} (max error {err.max().item() if err.numel() else 0.0:.3e})")
    assert ratio <= 1.0, f"{what}: error / bound {ratio:.3f}"
    # everything but the [B, V] window keeps its bits: rows B .. 2B - 1, the columns behind V, the slab around the view
    keep = torch.ones_like(slab, dtype=torch.bool)
    off = (view.data_ptr() - slab.data_ptr()) // x.element_size()
    win = keep[off:off + 2 * B * (V + 3)].view(2 * B, V + 3)
    win[:B, :V] = False
    assert torch.equal(_bits(slab)[keep], _bits(before)[keep]), f"{what}: bytes outside the [B, V] window changed"
    assert torch.equal(_bits(view[B:]), _bits(x.cuda()[B:]))
    return ratio, view[:B].clone()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", [7, 1023, 1024, 1025, 4097])
def test_against_the_fp64_reference(V, B, dtype):
    x = guidance_ref.kernel_inputs(B, V, dtype, seed=V)
    for g in G_VALUES:
        _check(x, B, g, f"V={V} B={B} {dtype} g={g}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_vocabulary_of_the_flagship_model(dtype):
    x = guidance_ref.kernel_inputs(3, 50272, dtype, seed=1)
    _check(x, 3, 1.5, f"V=50272 B=3 {dtype} g=1.5")


@pytest.mark.parametrize("dtype", DTYPES)
def test_largest_vocabulary_accepted_and_the_next_refused(dtype):
    from mmgl_amd import ops
    x = guidance_ref.kernel_inputs(1, 131072, dtype, seed=2)
    _check(x, 1, 1.5, f"V=131072 B=1 {dtype} g=1.5")
    y = torch.zeros(2, 131073, dtype=dtype, device="cuda")
    with pytest.raises(ValueError, match="131072"):
        ops.guidance_logits(y, 1, 1.5)
    assert not y.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_infinities_nans_and_large_logits(dtype):
    """The -inf / NaN rules, and logits of +-1e4: exp of either overflows or vanishes unless the row maximum is taken out first."""
    B, V = 3, 1025
    x = guidance_ref.kernel_inputs(B, V, dtype, seed=9)
    x[0, 5] = -math.inf              # conditional -inf -> -inf
    x[B + 0, 7] = -math.inf          # unconditional -inf under a finite conditional -> lc
    x[1, 9] = math.nan               # NaN counts as -inf ...
    x[B + 1, 11] = math.nan          # ... on either side
    x[1, 13] = x[B + 1, 13] = -math.inf
    x[2, 1000:] = -math.inf          # a banned tail, e.g. suppressed tokens, with neighbors only
    x[B + 2, 3] = -math.inf
    for g in G_VALUES:
        _, out = _check(x, B, g, f"inf / NaN rules {dtype} g={g}")
        out = out.cpu()
        assert out[0, 5] == -math.inf and out[1, 9] == -math.inf and out[1, 13] == -math.inf and (out[2, 1000:] == -math.inf).all()
        assert torch.isfinite(out[0, 7]) and torch.isfinite(out[1, 11]) and torch.isfinite(out[2, 3])
        assert torch.isfinite(out).sum() == B * V - 3 - 25
    big = guidance_ref.kernel_inputs(B, V, dtype, seed=10)
    big[:, ::2] += 1e4
    big[:, 1::2] -= 1e4
    big[B:, :] = big[B:, :].flip(1)
    for g in G_VALUES:
        _, out = _check(big, B, g, f"logits of +-1e4 {dtype} g={g}")
        assert torch.isfinite(out).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_are_bitwise_equal(dtype):
    from mmgl_amd import ops
    x = guidance_ref.kernel_inputs(3, 50272, dtype, seed=5).cuda()
    a, b = x.clone(), x.clone()
    ops.guidance_logits(a, 3, 1.5)
    ops.guidance_logits(b, 3, 1.5)
    assert torch.equal(_bits(a), _bits(b)) and not torch.equal(_bits(a[:3]), _bits(x[:3]))


def test_refused_calls_leave_the_tensor_alone():
    from mmgl_amd import ops
    x = guidance_ref.kernel_inputs(2, 33, torch.float32, seed=6).cuda()
    keep = x.clone()
    refused = [(lambda: ops.guidance_logits(x, 3, 1.5), "4 rows for batch = 3"),
               (lambda: ops.guidance_logits(x, 0, 1.5), "4 rows for batch = 0"),
               (lambda: ops.guidance_logits(x[:3], 1, 1.5), "3 rows for batch = 1"),
               (lambda: ops.guidance_logits(x, 2, -1.0), "finite and not negative"),
               (lambda: ops.guidance_logits(x, 2, math.nan), "finite and not negative"),
               (lambda: ops.guidance_logits(x, 2, math.inf), "finite and not negative"),
               (lambda: ops.guidance_logits(x[:, ::2], 2, 1.5), "unit column stride"),
               (lambda: ops.guidance_logits(x[:, :1].expand(4, 33), 2, 1.5), "unit column stride"),
               (lambda: ops.guidance_logits(torch.as_strided(x, (4, 33), (16, 1)), 2, 1.5), "row stride must be at least V")]
    for call, text in refused:
        with pytest.raises(ValueError, match=text):
            call()
        assert torch.equal(_bits(x), _bits(keep)), text
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        ops.guidance_logits(x.half(), 2, 1.5)
