"""ops.relu_ffn, the fc1 + ReLU / fc2 pair as one call (reference :352-355): the frozen route on a strided input and at a shape
without mask bits, the route taken when only one of the two linears is frozen, and the refusals.  The pair at the bench shapes:
tests/test_gemm_nt_gpu.py (frozen), tests/test_kernels_gpu.py and tests/test_bench_shapes_gpu.py (trainable)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _operands(M, d, ffn, dtype, seed=11):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda *s, scale=1.0: (torch.randn(*s, device="cuda", generator=g) * scale).to(dtype)
    return mk(M, d), mk(ffn, d, scale=d ** -0.5), mk(ffn, scale=0.1), mk(d, ffn, scale=ffn ** -0.5), mk(d, scale=0.1), mk(M, d)


def test_frozen_route_strided_input_equals_contiguous():
    """x as a column slice of a wider buffer (rows not contiguous) at (2560, 2048, 8192) bf16 -- 2048 rows with mask bits and a
    512-row tail: output and dx equal, bit for bit, to the call on a contiguous copy."""
    from mmgl_amd import ops
    M, d, ffn = 2560, 2048, 8192
    x, W1, b1, W2, b2, dy = _operands(M, d, ffn, torch.bfloat16)
    wide = torch.zeros(M, d + 256, device="cuda", dtype=torch.bfloat16)
    wide[:, 128:128 + d] = x
    xs = wide[:, 128:128 + d].detach().requires_grad_()
    xc = x.requires_grad_()
    assert not xs.is_contiguous() and torch.equal(xs, xc)
    ys = ops.relu_ffn(xs, W1, b1, W2, b2)
    yc = ops.relu_ffn(xc, W1, b1, W2, b2)
    assert ys.grad_fn.mask_bits[2] == yc.grad_fn.mask_bits[2] == 2048
    ys.backward(dy)
    yc.backward(dy)
    assert torch.equal(ys, yc) and torch.equal(xs.grad, xc.grad)
    assert float(xc.grad.float().abs().max()) > 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_frozen_route_without_mask_bits(dtype):
    """(200, 64, 128): no mask bits in either dtype, the activation is the mask.  Forward and dx against fp32 torch autograd; bf16 at
    the bound of test_frozen_ffn_pair_mask_dx, fp32 at 1e-5 of the tensor's maximum (test_linear_relu_pair_with_folded_mask's)."""
    from mmgl_amd import ops
    M, d, ffn = 200, 64, 128
    x, W1, b1, W2, b2, w = _operands(M, d, ffn, dtype)
    x.requires_grad_()
    y, h = ops.relu_ffn(x, W1, b1, W2, b2, return_hidden=True)
    assert type(y.grad_fn).__name__ == "_FrozenReluFFNBackward" and y.grad_fn.mask_bits is None and not h.requires_grad
    y.backward(w)
    xr = x.detach().float().requires_grad_()
    # the kernel masks with the h it stored: reproduce that mask in the reference (sign flips at pre-activation ~ 0)
    hr = torch.relu(F.linear(xr, W1.float(), b1.float())) * (h.float() > 0)
    yr = F.linear(hr, W2.float(), b2.float())
    yr.backward(w.float())
    ey = (y.float() - yr).abs().max().item() / yr.abs().max().item()
    ex = (x.grad.float() - xr.grad).abs().max().item() / xr.grad.abs().max().item()
    print(f"[relu_ffn] frozen (200, 64, 128) {dtype}: max err / max|ref|  y {ey:.3e}  dx {ex:.3e}")
    if dtype == torch.float32:
        assert ey <= 1e-5 and ex <= 1e-5
    else:
        assert (y.float() - yr).abs().max().item() <= 3e-2 * yr.abs().max().item() + 1e-2
        assert (x.grad.float() - xr.grad).abs().max().item() <= 3e-2 * xr.grad.abs().max().item() + 1e-2


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_mixed_freezing_takes_the_trainable_route(dtype):
    """fc1 frozen, fc2 trainable: frozen=None must pick the trainable route (the frozen node has no weight gradients).  y and fc2's
    weight and bias gradients equal those of relu_ffn(frozen=False) with all four parameters trainable, bit for bit."""
    from mmgl_amd import ops
    x, W1, b1, W2, b2, dy = _operands(200, 64, 128, dtype)
    got = []
    for fc1_trains in (False, True):
        ps = [t.clone().requires_grad_(r) for t, r in zip((x, W1, b1, W2, b2), (True, fc1_trains, fc1_trains, True, True))]
        y = ops.relu_ffn(*ps) if not fc1_trains else ops.relu_ffn(*ps, frozen=False)
        assert type(y.grad_fn).__name__ == "_LinearBackward"
        y.backward(dy)
        got.append([y.detach()] + [p.grad for p in ps])
    assert got[0][2] is None and got[0][3] is None and got[1][2] is not None
    for i, name in ((0, "y"), (4, "dW2"), (5, "db2")):
        assert torch.equal(got[0][i], got[1][i]), name
    assert float(got[0][4].float().abs().max()) > 0 and float(got[0][5].float().abs().max()) > 0


def test_refusals_and_removed_keywords():
    from mmgl_amd import ops
    x, W1, b1, W2, b2, _ = _operands(8, 64, 128, torch.float32)
    with pytest.raises(ValueError, match=r"relu_ffn: weight and bias must be frozen \(requires_grad=False\)"):
        ops.relu_ffn(x, W1, b1, W2.clone().requires_grad_(), b2, frozen=True)
    with pytest.raises(TypeError, match="mask_dx"):
        ops.linear(x, W1, b1, mask_dx=True)
    with pytest.raises(TypeError, match="bwd_premasked"):
        ops.frozen_linear(x, W1, b1, act="relu", bwd_premasked=True)
