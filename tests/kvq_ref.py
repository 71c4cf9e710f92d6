"""The FP8 key/value cache format (include/mmgl_hip.h) restated in torch on the CPU, for the tests of the kernels and of
generate(kv_cache_dtype="fp8").

For the D storage-rounded elements x of one head of one key or value row, a = max |x|:  e = 0 if a = 0, else with a = m * 2^X,
m in [0.5, 1) (torch.frexp):  e = X - 9 if m <= 0.875 else X - 8 -- the smallest integer with a * 2^-e <= 448 -- clamped to
[-120, 120];  code = e4m3fn(x * 2^-e), round to nearest even (torch's CPU cast);  value = code * 2^e.  The scale is a power of two and
e4m3 has 3 mantissa bits, so every value is exact in bf16 and fp32."""
import torch

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def exponents(x, num_heads):
    """x [..., H*D] (any float dtype, storage-rounded) -> int32 [..., H]: the exponent of every head."""
    xf = x.detach().float().cpu()
    a = xf.reshape(*xf.shape[:-1], num_heads, -1).abs().amax(dim=-1)
    m, X = torch.frexp(a)
    e = torch.where(m <= 0.875, X - 9, X - 8)
    e = torch.where(a == 0, torch.zeros_like(e), e)
    return e.clamp(-120, 120).to(torch.int32)


def quantize(x, num_heads):
    """x [..., H*D] -> (codes uint8 [..., H*D], exponents int8 [..., H])."""
    xf = x.detach().float().cpu()
    e = exponents(xf, num_heads)
    D = xf.shape[-1] // num_heads
    scaled = torch.ldexp(xf.reshape(*xf.shape[:-1], num_heads, D), -e[..., None])       # exact: a power of two
    assert scaled.abs().max().item() <= FP8_MAX
    codes = scaled.to(FP8).view(torch.uint8).reshape(xf.shape)
    return codes, e.to(torch.int8)


def dequantize(codes, e, num_heads):
    """codes uint8 / e4m3fn [..., H*D], exponents int8 [..., H] -> fp32 values [..., H*D] (exact)."""
    c = codes.detach().cpu()
    c = (c.view(FP8) if c.dtype == torch.uint8 else c).float()
    D = c.shape[-1] // num_heads
    v = torch.ldexp(c.reshape(*c.shape[:-1], num_heads, D), e.detach().cpu().to(torch.int32)[..., None])
    return v.reshape(c.shape)


def quantize_row(k, v, num_heads):
    """A cache row as the kernels file it: k, v [..., H*D] -> (codes uint8 [..., 2*H*D], exponents int8 [..., 2H]), key heads first."""
    kc, ke = quantize(k, num_heads)
    vc, ve = quantize(v, num_heads)
    return torch.cat([kc, vc], dim=-1), torch.cat([ke, ve], dim=-1)


def dequantize_row(codes, e, num_heads):
    """(codes [..., 2*H*D], exponents [..., 2H]) -> (k, v) fp32 [..., H*D]."""
    d = codes.shape[-1] // 2
    return dequantize(codes[..., :d], e[..., :num_heads], num_heads), dequantize(codes[..., d:], e[..., num_heads:], num_heads)


def attention(q, k_cached, v_cached, key_valid, k_new, v_new, num_heads):
    """fp64 single-query attention over [the S cached columns ++ the new row]: q, k_new, v_new [B, H*D], k_cached, v_cached
    [B, S, H*D] (dequantised values), key_valid [B, S] (the new key is always valid).  Returns fp64 [B, H*D]."""
    B, d = q.shape
    H, D = num_heads, d // num_heads
    qd = q.detach().double().cpu().reshape(B, H, 1, D)
    k = torch.cat([k_cached.detach().double().cpu(), k_new.detach().double().cpu()[:, None]], dim=1).reshape(B, -1, H, D).transpose(1, 2)
    v = torch.cat([v_cached.detach().double().cpu(), v_new.detach().double().cpu()[:, None]], dim=1).reshape(B, -1, H, D).transpose(1, 2)
    ok = torch.cat([key_valid.detach().cpu().bool(), torch.ones(B, 1, dtype=torch.bool)], dim=1)
    s = (qd @ k.transpose(-1, -2)).masked_fill(~ok[:, None, None, :], float("-inf"))
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, d)
