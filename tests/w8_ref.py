"""The FP8 frozen-weight format (include/mmgl_hip.h) restated in torch on the CPU, for the tests of mmgl_weight_quantize,
mmgl_gemm_skinny_w8 and generate(weight_dtype="fp8").

It is the FP8 key/value cache's format with a weight row in the place of a head: kvq_ref.exponents / quantize / dequantize with
num_heads = 1 on the rows of W [N, K] -- the exponent rule is that module's function, not a second copy.
    exps[n] = kvq_ref exponent of max_k |W[n, k]|;   codes[n, k] = e4m3fn(W[n, k] * 2^-exps[n]) (round to nearest even);
    value   = codes[n, k] * 2^exps[n], exact in bf16 and fp32."""
import torch

import kvq_ref

FP8 = kvq_ref.FP8
FP8_MAX = kvq_ref.FP8_MAX


def quantize(w):
    """w [N, K] (bf16 or fp32, storage-rounded) -> (codes uint8 [N, K], exps int8 [N]) on the CPU."""
    codes, e = kvq_ref.quantize(w, 1)
    return codes, e[:, 0].contiguous()


def dequantize(codes, exps):
    """(codes uint8 / e4m3fn [N, K], exps int8 [N]) -> fp32 [N, K] on the CPU (exact)."""
    return kvq_ref.dequantize(codes, exps.detach().cpu()[:, None], 1)


def edge_rows(K, dtype=torch.float32):
    """Rows [R, K] that sit on the edges of the exponent rule, named: zero row; a maximum exactly at 448 * 2^e and one step of `dtype`
    above it (the exponent moves by one); magnitudes at both exponent clamps (2^-115: e = -123 clamped to
    -120; 0.9375 * 2^128, the top of the finite range: e = 120); a negative and a large exponent in between.  Every row also holds small values, so that the subnormal codes are visited."""
    g = torch.Generator().manual_seed(5)
    fill = torch.rand(K, generator=g) * 2 - 1
    eps = torch.finfo(dtype).eps
    names, rows = [], []

    def add(name, amax, scale=None):
        r = fill * (amax if scale is None else scale) * 0.75
        r[K // 2] = -amax
        names.append(name)
        rows.append(r)

    names.append("zero row")
    rows.append(torch.zeros(K))
    add("max = 448 * 2^-3", 448.0 * 2.0 ** -3)
    add("max one step above 448 * 2^-3", 448.0 * 2.0 ** -3 * (1 + eps))
    add("max = 448 (e = 0)", 448.0)
    add("low clamp", 2.0 ** -115)
    add("high clamp", 0.9375 * 2.0 ** 128)
    add("negative exponent", 3.0e-4)
    add("large exponent", 7.0e6)
    return names, torch.stack(rows).to(dtype)
