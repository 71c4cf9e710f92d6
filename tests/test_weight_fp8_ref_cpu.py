"""CPU: the comparison tests/test_gemm_skinny_w8_gpu.py makes can fail.  From the references alone (decode_ref.SkinnyRef on the dequantised
weight against the same reference of a wrong kernel), each of the mistakes a kernel on FP8 codes can make moves at least 25 % of the
elements out of the per-element bound  u |want| + 2^-16 mag:
  a dropped K unit (the last 128 codes of every row), an exponent off by one, codes read as e5m2, the two halves of a 32-bit code word
  swapped, the row scale applied after the bias instead of before.
Shapes and epilogue are the GPU test's: bias, residual, ReLU and scale together, bf16 and fp32 bounds."""
import pytest
import torch

import w8_ref
from decode_ref import SkinnyRef

SHAPES = [(17, 768, 1152), (33, 24, 640), (8, 5, 200)]


def _case(M, N, K, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + K)
    x = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) * K ** -0.5 * torch.logspace(-3, 5, N)[:, None]).to(dtype)     # row exponents from negative to large
    b = (torch.randn(N, generator=g) * torch.logspace(-3, 5, N)).to(dtype)
    res = torch.randn(M, N, generator=g).to(dtype)
    codes, exps = w8_ref.quantize(w)
    return x, codes, exps, b, res


def _mutants(x, codes, exps, b, res):
    """name -> SkinnyRef of the wrong kernel."""
    N, K = codes.shape
    deq = w8_ref.dequantize(codes, exps)
    unit = 128 if K >= 256 else 64
    dropped = deq.clone()
    dropped[:, K - unit:] = 0
    e5m2 = torch.ldexp(codes.view(torch.float8_e5m2).float(), exps.to(torch.int32)[:, None])
    k4 = K // 4 * 4
    swapped = deq.clone()
    swapped[:, :k4] = deq[:, :k4].reshape(N, -1, 2, 2).flip(2).reshape(N, k4)
    s = torch.ldexp(torch.ones(N), exps.to(torch.int32))
    late = SkinnyRef(x, codes.view(w8_ref.FP8).float(), None, True, 0.5, res)      # act(((acc + bias) * 2^e) * scale) + residual
    pre = (x.double() @ codes.view(w8_ref.FP8).double().t() + b.double()) * s.double()
    late.want = torch.relu(pre * 0.5) + res.double()
    return {
        "a dropped K unit": SkinnyRef(x, dropped, b, True, 0.5, res),
        "an exponent off by one": SkinnyRef(x, w8_ref.dequantize(codes, exps + 1), b, True, 0.5, res),
        "codes read as e5m2": SkinnyRef(x, e5m2, b, True, 0.5, res),
        "code word halves swapped": SkinnyRef(x, swapped, b, True, 0.5, res),
        "row scale after the bias": late,
    }


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_mistake_leaves_the_bound(shape, dtype):
    x, codes, exps, b, res = _case(*shape, dtype)
    assert exps.min() < 0 < exps.max()
    ref = SkinnyRef(x, w8_ref.dequantize(codes, exps), b, True, 0.5, res)
    bound = ref.bound(dtype)
    for name, wrong in _mutants(x, codes, exps, b, res).items():
        frac = ((wrong.want - ref.want).abs() > bound).double().mean().item()
        print(f"{shape} {dtype} {name}: {frac:.0%} of the elements leave the bound")
        assert frac >= 0.25, f"{name}: only {frac:.0%} of the elements leave the bound"
