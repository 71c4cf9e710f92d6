"""-m gpu: the two kernels of the FP8 key/value cache against tests/kvq_ref.py.

ops.kv_quantize is compared BITWISE with the restatement (codes and exponents): the format has one answer.  ops.attn_decode_q8 is
compared with an fp64 attention over [the dequantised cached columns ++ the new row] at the tolerance of tests/test_beam_kernels_gpu.py
(per sample, max-norm relative: 1e-3 fp32, 2e-2 bf16), after a sensitivity check computed from the reference alone: reading the
exponents wrongly (all 0, key and value swapped, the neighbouring head's) moves every sample by at least 10 tolerances, so the
comparison can tell.  The heads of a row differ in magnitude by 2^6 and keys and values of a head by 2^6 the other way, which is what
makes a wrong exponent visible.  B = 2 or 3, H = 2, D in {16, 64, 128}."""
import pytest
import torch

import kvq_ref

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
TOL = {F32: 1e-3, BF16: 2e-2}                      # tests/test_beam_kernels_gpu.py
DEV = "cuda"
H = 2
NAN_CODE, FILL_EXP = 0x7F, 0x55                     # 0x7F is NaN in e4m3fn; an exponent no head of these tests has


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.uint8)


def _head_scale(D, flip=False):
    """[H*D] multipliers: head 0 times 8, head 1 times 1/8 (flip: the other way round)."""
    s = torch.tensor([8.0, 0.125]).repeat_interleave(D)
    return s.flip(0) if flip else s


# ------------------------------------------------------------------------------------------ the quantiser
def _special_rows(seed, B, D, dtype):
    """k, v [B, 5, H*D] fp32 values that are exact in `dtype`: row 0 a zero head, row 1 amax = 448 * 2^k exactly and one ulp above,
    row 2 a ladder down to amax * 2^-12 with ties of the fp8 grid, rows 3-4 random; heads differ by 2^6."""
    g = torch.Generator().manual_seed(seed)
    d = H * D
    ulp = 2.0 ** -23 if dtype == F32 else 2.0 ** -7
    out = []
    for flip in (False, True):
        x = (torch.randn(B, 5, d, generator=g) * _head_scale(D, flip)).to(dtype).float()
        x[:, 0, :D] = 0                                                              # an all-zero head
        for b in range(B):
            k = b - 3
            x[b, 1, :D] = (torch.randn(D, generator=g) * 8).clamp(-50, 50) * 2.0 ** k
            x[b, 1, 0] = -448.0 * 2.0 ** k                                            # m = 0.875 exactly: the top code
            x[b, 1, D:] = (torch.randn(D, generator=g) * 8).clamp(-50, 50) * 2.0 ** k
            x[b, 1, D + 3] = 448.0 * 2.0 ** k * (1 + ulp * 4 / 7)                     # one ulp above: the next exponent
            # scaled amax 256 (e = k), then values on and between the steps of the fp8 grid: subnormals (step 2^-9), round to zero, ties
            ladder = torch.tensor([256.0, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -9, 5 * 2.0 ** -10, 2.0 ** -12, 2.0 ** -4, 17.0, 19.0, 15.5, 14.5,
                                   0.0146484375, 0.0166015625, 1.0625, 1.1875, 240.0])
            sign = torch.where(torch.rand(16, generator=g) < 0.5, -1.0, 1.0)
            x[b, 2, :D] = (ladder * sign).repeat(D // 16) * 2.0 ** k
        x = x.to(dtype)
        assert torch.equal(x.float()[:, 1, 0].abs(), 448.0 * 2.0 ** (torch.arange(B) - 3.0))
        out.append(x)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [16, 64, 128])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("fused", [True, False], ids=["qkv-view", "two-tensors"])
def test_quantiser_is_the_restatement_bitwise(fused, n, D, dtype):
    from mmgl_amd import ops
    B, d = 3, H * D
    k, v = _special_rows(D + n, B, D, dtype)
    if n == 1:
        k, v = k[:, 2:3], torch.cat([v[:1, 1:2], v[1:, 0:1]])                          # the ladder; the boundary row and the zero head
    ref_codes, ref_e = kvq_ref.quantize_row(k, v, H)
    assert set(ref_e.flatten().tolist()) - {0} and FILL_EXP not in ref_e.flatten().tolist()
    if fused:                                                                        # the k and v columns of a [B, n, 3d + pad] projection output
        buf = torch.full((B, n, 3 * d + 16), float("nan"), dtype=dtype)
        buf[..., d:2 * d], buf[..., 2 * d:3 * d] = k, v
        buf = buf.to(DEV)
        ks, vs, keep = buf[..., d:2 * d], buf[..., 2 * d:3 * d], [buf]
    else:
        ks, vs = k.to(DEV), v.to(DEV)
        keep = [ks, vs]
    before = [_bits(t).clone() for t in keep]
    cap = n + 2
    kvq = torch.full((B, cap, 2 * d), NAN_CODE, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)
    scale = torch.full((B, cap, 2 * H), FILL_EXP, dtype=torch.int8, device=DEV)
    ops.kv_quantize(ks, vs, kvq, scale, H)
    torch.cuda.synchronize()
    codes, e = kvq.view(torch.uint8).cpu(), scale.cpu()
    assert torch.equal(e[:, :n], ref_e), (e[:, :n] - ref_e).nonzero()[:8].tolist()
    bad = (codes[:, :n] != ref_codes).nonzero()
    assert len(bad) == 0, [(i, int(codes[:, :n][tuple(i)]), int(ref_codes[tuple(i)])) for i in bad[:8].tolist()]
    assert (codes[:, n:] == NAN_CODE).all() and (e[:, n:] == FILL_EXP).all()           # nothing outside the n columns
    assert all(torch.equal(_bits(t), b0) for t, b0 in zip(keep, before))               # the inputs, NaN columns included
    # a refused call writes nothing
    with pytest.raises(ValueError, match="rows for a cache"):
        ops.kv_quantize(ks.repeat(1, cap + 1, 1), vs.repeat(1, cap + 1, 1), kvq, scale, H)
    with pytest.raises(ValueError, match="incompatible"):
        ops.kv_quantize(ks, vs, kvq, scale[..., :2 * H - 1], H)
    assert torch.equal(kvq.view(torch.uint8).cpu(), codes) and torch.equal(scale.cpu(), e)


# ------------------------------------------------------------------------------------------ attention over the quantised cache
def _lengths(D):
    """As tests/test_beam_kernels_gpu.py builds them, for this kernel's 16 codes per lane: kpi = keys per wave and load instruction;
    a workgroup loads 4 kpi keys at once and a loop trip covers 16 kpi."""
    kpi = 64 * 16 // D
    return [1, kpi - 1, kpi + 1, 4 * kpi + 1, 16 * kpi - 1, 16 * kpi + 3]


def _case(seed, B, D, S, dtype, valid="ragged"):
    """Operands of one call.  Scores stay of order 1 (q carries the inverse of the key heads' scale), so the softmax is soft and
    every cached value counts."""
    g = torch.Generator().manual_seed(seed)
    d, cap = H * D, S + 2
    rn = lambda *s: torch.randn(*s, generator=g)
    ksc, vsc = _head_scale(D), _head_scale(D, flip=True)
    q = (rn(B, d) * D ** -0.5 / ksc).to(dtype)
    k_new, v_new = (rn(B, d) * ksc * 0.25).to(dtype), (rn(B, d) * vsc).to(dtype)
    kc, vc = rn(B, S, d) * ksc, (rn(B, S, d) * vsc).to(dtype)
    qh = q.float().reshape(B, 1, H, D)
    kc = (kc.reshape(B, S, H, D) + 2 * qh / (qh * qh).sum(-1, keepdim=True)).reshape(B, S, d).to(dtype)     # cached scores around +2, the new key's
    ok = torch.ones(B, S, dtype=torch.bool)                                                                  # around 0: also at S = 1 the cache counts
    if valid == "ragged":
        ok = torch.rand(B, S, generator=g) > 0.3
        ok[:, 0] = True
    elif valid == "one-masked":
        ok = torch.rand(B, S, generator=g) > 0.3
        ok[:, 0] = True
        ok[1] = False                                                                  # every cached key of sample 1
    codes, e = kvq_ref.quantize_row(kc, vc, H)
    return dict(B=B, D=D, d=d, S=S, cap=cap, dtype=dtype, q=q, k_new=k_new, v_new=v_new, ok=ok, codes=codes, e=e)


def _reference(c, e=None):
    k, v = kvq_ref.dequantize_row(c["codes"], c["e"] if e is None else e, H)
    return kvq_ref.attention(c["q"], k, v, c["ok"], c["k_new"], c["v_new"], H)


def _per_sample(a, ref):
    return ((a.double() - ref).abs().amax(dim=1) / ref.abs().amax(dim=1)).tolist()


def _device_cache(c):
    B, S, cap, d = c["B"], c["S"], c["cap"], c["d"]
    kvq = torch.full((B, cap, 2 * d), NAN_CODE, dtype=torch.uint8)
    scale = torch.full((B, cap, 2 * H), FILL_EXP, dtype=torch.int8)
    kvq[:, :S], scale[:, :S] = c["codes"], c["e"]
    return kvq.to(DEV).view(torch.float8_e4m3fn), scale.to(DEV)


def _run(c, kvq, scale, out=None):
    from mmgl_amd import ops
    S, d = c["S"], c["d"]
    new = torch.cat([c["k_new"], c["v_new"]], dim=1).to(DEV)                            # the dense [B, 2d] projection output of the model
    mask = torch.zeros(c["B"], c["cap"], dtype=torch.bool)
    mask[:, :S] = c["ok"]
    mask = mask.to(DEV)
    return ops.attn_decode_q8(c["q"].to(DEV), new[:, :d], new[:, d:], kvq, scale, mask[:, :S], H, out=out)


def _check_filing(c, kvq, scale, kvq0, scale0):
    """Column S holds the restatement of the new row, bitwise; every other byte of the cache is as it was."""
    S = c["S"]
    new_codes, new_e = kvq_ref.quantize_row(c["k_new"], c["v_new"], H)
    codes, e = kvq.view(torch.uint8).cpu(), scale.cpu()
    assert torch.equal(codes[:, S], new_codes) and torch.equal(e[:, S], new_e), (S, e[:, S].tolist(), new_e.tolist())
    want_c, want_e = kvq0.view(torch.uint8).cpu(), scale0.cpu()
    want_c[:, S], want_e[:, S] = new_codes, new_e
    assert torch.equal(codes, want_c) and torch.equal(e, want_e)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [16, 64, 128])
def test_attention_against_the_fp64_reference(D, dtype):
    tol, B = TOL[dtype], 2
    for i, S in enumerate(_lengths(D)):
        c = _case(100 * D + i, B, D, S, dtype)
        ref = _reference(c)
        # sensitivity, from the reference alone: a kernel that reads the exponents wrongly is outside the tolerance by a wide margin
        e = c["e"]
        wrong = {"all exponents 0": torch.zeros_like(e),
                 "key and value exponents swapped": torch.cat([e[..., H:], e[..., :H]], dim=-1),
                 "the neighbouring head's exponent": torch.cat([e[..., :H].flip(-1), e[..., H:].flip(-1)], dim=-1)}
        for what, ew in wrong.items():
            moved = _per_sample(_reference(c, ew), ref)
            print(f"D={D} S={S} {dtype}: {what} moves the samples by {['%.2e' % m for m in moved]}")
            assert min(moved) >= 10 * tol, (what, S, moved)
        kvq, scale = _device_cache(c)
        kvq0, scale0 = kvq.clone(), scale.clone()
        out = _run(c, kvq, scale)
        torch.cuda.synchronize()
        assert out.dtype == dtype and out.shape == (B, c["d"])
        err = _per_sample(out.cpu(), ref)
        print(f"D={D} S={S} {dtype}: per-sample rel err {['%.2e' % x for x in err]} (tol {tol:.0e})")
        assert max(err) <= tol, (S, err)
        _check_filing(c, kvq, scale, kvq0, scale0)
        # two runs are bitwise equal: the output, and the column filed
        kvq2, scale2 = kvq0.clone(), scale0.clone()
        out2 = _run(c, kvq2, scale2)
        assert torch.equal(_bits(out2), _bits(out)) and torch.equal(kvq2.view(torch.uint8), kvq.view(torch.uint8)) and torch.equal(scale2, scale)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [16, 64, 128])
def test_a_sample_of_masked_keys_returns_the_new_value_row(D, dtype):
    B = 3
    for S in (1, _lengths(D)[3]):
        c = _case(7 * D + S, B, D, S, dtype, valid="one-masked")
        ref = _reference(c)
        kvq, scale = _device_cache(c)
        kvq0, scale0 = kvq.clone(), scale.clone()
        out = _run(c, kvq, scale).cpu()
        assert torch.equal(_bits(out[1]), _bits(c["v_new"][1])), (out[1] - c["v_new"][1]).abs().max()     # bitwise: the only key that counts
        err = _per_sample(out, ref)
        assert max(err) <= TOL[dtype], (S, err)
        _check_filing(c, kvq, scale, kvq0, scale0)


def test_refused_calls_leave_out_and_the_cache_untouched():
    from mmgl_amd import ops
    D, S, B = 64, 9, 2
    c = _case(3, B, D, S, BF16)
    kvq, scale = _device_cache(c)
    kvq0, scale0 = kvq.clone(), scale.clone()
    d = c["d"]
    q, new = c["q"].to(DEV), torch.cat([c["k_new"], c["v_new"]], dim=1).to(DEV)
    ok = c["ok"].to(DEV)
    out = torch.full((B, d), 7.0, dtype=BF16, device=DEV)
    with pytest.raises(ValueError, match="full"):
        ops.attn_decode_q8(q, new[:, :d], new[:, d:], kvq[:, :S], scale[:, :S], ok, H, out=out)
    with pytest.raises(ValueError, match="no cached columns"):
        ops.attn_decode_q8(q, new[:, :d], new[:, d:], kvq, scale, ok[:, :0], H, out=out)
    with pytest.raises(ValueError, match="incompatible"):
        ops.attn_decode_q8(q, new[:, :d], new[:, d:].float(), kvq, scale, ok, H, out=out)
    with pytest.raises(ValueError, match="incompatible codes"):
        ops.attn_decode_q8(q, new[:, :d], new[:, d:], kvq.view(torch.uint8).to(torch.int16), scale, ok, H, out=out)
    with pytest.raises(ValueError, match="out"):
        ops.attn_decode_q8(q, new[:, :d], new[:, d:], kvq, scale, ok, H, out=out.float())
    with pytest.raises(ValueError, match="divisible"):
        ops.attn_decode_q8(q, new[:, :d], new[:, d:], kvq, scale, ok, 3, out=out)
    with pytest.raises(ValueError, match="head_dim"):                                   # the C side: D = 8
        ops.attn_decode_q8(q, new[:, :d], new[:, d:], kvq, torch.zeros(B, S + 2, 32, dtype=torch.int8, device=DEV), ok, 16, out=out)
    with pytest.raises(ValueError, match="forward only"):
        with torch.enable_grad():
            ops.attn_decode_q8(q.clone().requires_grad_(), new[:, :d], new[:, d:], kvq, scale, ok, H, out=out)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and torch.equal(kvq.view(torch.uint8), kvq0.view(torch.uint8)) and torch.equal(scale, scale0)
