"""-m gpu: mmgl_attn_decode_gqa_q8_fwd -- grouped-query single-query attention over a cache of e4m3fn codes -- through
ops.attn_decode_q8(..., num_kv_heads) against tests/kvq_ref.py.

The reference dequantises the cached columns with Hkv heads (kvq_ref.dequantize_row), expands K and V to H heads with
repeat_interleave (query head h reads key/value head h // G, transformers' repeat_kv) and runs kvq_ref.attention in fp64 over [the
cached columns ++ the new row].  Bounds: per sample, max-norm relative, 1e-3 fp32 / 2e-2 bf16 (the project's TOL).  Before any device
comparison the reference alone shows that the comparison can tell: all exponents 0, key and value exponents swapped, the neighbouring
kv head's exponent (Hkv > 1) and the head mapping h % Hkv (where it differs from h // G) each move every sample by at least 10
tolerances.  The kv heads of a row alternate in magnitude by 2^6, and keys and values of a head by 2^6 the other way.

Groups (H, Hkv): G = 1, 2, 4, 3 (a block of 4 with an idle slot), 8 (two blocks of 4) and 12 (three blocks of 4: the single-writer rule).
Lengths come from the kernel's constants: KPI = 1024 / D keys per wave and load instruction, 4 KPI per workgroup load, 16 KPI per trip.
The column filed is compared BITWISE with kvq_ref.quantize_row(k_new, v_new, Hkv): the format has one answer."""
import pytest
import torch

import kvq_ref

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16")]
TOL = {F32: 1e-3, BF16: 2e-2}
DEV = "cuda"
GROUPS = [(4, 4), (4, 2), (4, 1), (6, 2), (8, 1), (12, 1)]
NAN_CODE, FILL_EXP = 0x7F, 0x55                     # 0x7F is NaN in e4m3fn; an exponent no head of these tests has


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.uint8)


def _lengths(D):
    """As tests/test_kv_quant_kernels_gpu.py builds them: kpi keys per wave and load instruction; a workgroup loads 4 kpi keys at once
    and a loop trip covers 16 kpi."""
    kpi = 64 * 16 // D
    return [1, kpi - 1, kpi + 1, 4 * kpi + 1, 16 * kpi - 1, 16 * kpi + 3]


def _head_scale(Hkv, D, flip=False):
    """[Hkv*D] multipliers: even kv heads times 8, odd ones times 1/8 (flip: the other way round)."""
    s = torch.tensor([8.0, 0.125] * Hkv)[:Hkv]
    return (1.0 / s if flip else s).repeat_interleave(D)


def _expand(t, H, Hkv, mapping="group"):
    """[..., Hkv*D] -> [..., H*D]: query head h reads kv head h // G ("group") or, the wrong way, h % Hkv ("modulo")."""
    D = t.shape[-1] // Hkv
    th = t.reshape(*t.shape[:-1], Hkv, D)
    idx = torch.arange(H) // (H // Hkv) if mapping == "group" else torch.arange(H) % Hkv
    return th[..., idx, :].reshape(*t.shape[:-1], H * D)


def _case(seed, B, H, Hkv, D, S, dtype, valid="ragged", cap=None):
    """Operands of one call.  Scores stay of order 1 (a query head carries the inverse of its kv head's key scale) and the cached
    scores sit around +2, the new key's around 0: every cached value counts, also at S = 1."""
    g = torch.Generator().manual_seed(seed)
    G, kd = H // Hkv, Hkv * D
    rn = lambda *s: torch.randn(*s, generator=g)
    ksc, vsc = _head_scale(Hkv, D), _head_scale(Hkv, D, flip=True)
    q = (rn(B, H * D) * D ** -0.5 / _expand(ksc, H, Hkv)).to(dtype)
    k_new, v_new = (rn(B, kd) * ksc * 0.25).to(dtype), (rn(B, kd) * vsc).to(dtype)
    kc, vc = rn(B, S, kd) * ksc, (rn(B, S, kd) * vsc).to(dtype)
    qh = q.float().reshape(B, Hkv, G, D)
    shift = (2 * qh / (qh * qh).sum(-1, keepdim=True)).sum(2)                            # + 2 on the score of every query head of the group,
    kc = (kc.reshape(B, S, Hkv, D) + shift[:, None]).reshape(B, S, kd).to(dtype)        # up to the small products between its queries
    ok = torch.ones(B, S, dtype=torch.bool)
    if valid in ("ragged", "one-masked"):
        ok = torch.rand(B, S, generator=g) > 0.3
        ok[:, 0] = True
    if valid == "one-masked":
        ok[1] = False                                                                  # every cached key of sample 1
    codes, e = kvq_ref.quantize_row(kc, vc, Hkv)
    return dict(B=B, H=H, Hkv=Hkv, D=D, d=H * D, kd=kd, S=S, cap=S + 2 if cap is None else cap, dtype=dtype, q=q, k_new=k_new, v_new=v_new,
                ok=ok, codes=codes, e=e)


def _reference(c, e=None, mapping="group"):
    H, Hkv = c["H"], c["Hkv"]
    k, v = kvq_ref.dequantize_row(c["codes"], c["e"] if e is None else e, Hkv)
    ex = lambda t: _expand(t, H, Hkv, mapping)
    return kvq_ref.attention(c["q"], ex(k), ex(v), c["ok"], ex(c["k_new"]), ex(c["v_new"]), H)


def _per_sample(a, ref):
    return ((a.double() - ref).abs().amax(dim=1) / ref.abs().amax(dim=1)).tolist()


def sensitivity(c, ref):
    """{what: per-sample movement of the reference under a wrong reading}, from the reference alone."""
    H, Hkv, e = c["H"], c["Hkv"], c["e"]
    wrong = {"all exponents 0": dict(e=torch.zeros_like(e)),
             "key and value exponents swapped": dict(e=torch.cat([e[..., Hkv:], e[..., :Hkv]], dim=-1))}
    if Hkv > 1:
        wrong["the neighbouring kv head's exponent"] = dict(e=torch.cat([e[..., :Hkv].roll(1, -1), e[..., Hkv:].roll(1, -1)], dim=-1))
    if Hkv > 1 and H > Hkv:
        wrong["the head mapping h % Hkv"] = dict(mapping="modulo")
    return {what: _per_sample(_reference(c, **kw), ref) for what, kw in wrong.items()}


def _device_cache(c):
    B, S, cap, kd, Hkv = c["B"], c["S"], c["cap"], c["kd"], c["Hkv"]
    kvq = torch.full((B, cap, 2 * kd), NAN_CODE, dtype=torch.uint8)
    scale = torch.full((B, cap, 2 * Hkv), FILL_EXP, dtype=torch.int8)
    kvq[:, :S], scale[:, :S] = c["codes"], c["e"]
    return kvq.to(DEV).view(torch.float8_e4m3fn), scale.to(DEV)


def _run(c, kvq, scale, out=None, q=None):
    from mmgl_amd import ops
    S, kd = c["S"], c["kd"]
    new = torch.cat([c["k_new"], c["v_new"]], dim=1).to(DEV)                            # the dense [B, 2*Hkv*D] row of DecodeCache.kv_new
    mask = torch.zeros(c["B"], c["cap"], dtype=torch.bool)
    mask[:, :S] = c["ok"]
    mask = mask.to(DEV)
    return ops.attn_decode_q8(c["q"].to(DEV) if q is None else q, new[:, :kd], new[:, kd:], kvq, scale, mask[:, :S], c["H"], out=out,
                              num_kv_heads=c["Hkv"])


def _check_filing(c, kvq, scale, kvq0, scale0):
    """Column S holds the restatement of the new row, bitwise; every other byte of the cache is as it was."""
    S = c["S"]
    new_codes, new_e = kvq_ref.quantize_row(c["k_new"], c["v_new"], c["Hkv"])
    codes, e = kvq.view(torch.uint8).cpu(), scale.cpu()
    assert torch.equal(codes[:, S], new_codes) and torch.equal(e[:, S], new_e), (S, e[:, S].tolist(), new_e.tolist())
    want_c, want_e = kvq0.view(torch.uint8).cpu(), scale0.cpu()
    want_c[:, S], want_e[:, S] = new_codes, new_e
    assert torch.equal(codes, want_c) and torch.equal(e, want_e)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [16, 64, 128])
@pytest.mark.parametrize("H,Hkv", GROUPS)
def test_attention_against_the_fp64_reference(H, Hkv, D, dtype):
    tol, B = TOL[dtype], 2
    for i, S in enumerate(_lengths(D)):
        c = _case(1000 * H + 100 * Hkv + D + i, B, H, Hkv, D, S, dtype)
        ref = _reference(c)
        for what, moved in sensitivity(c, ref).items():
            print(f"H={H} Hkv={Hkv} D={D} S={S} {dtype}: {what} moves the samples by {['%.2e' % m for m in moved]}")
            assert min(moved) >= 10 * tol, (what, S, moved)
        kvq, scale = _device_cache(c)
        kvq0, scale0 = kvq.clone(), scale.clone()
        out = torch.full((B, c["d"]), float("nan"), dtype=dtype, device=DEV)
        assert _run(c, kvq, scale, out=out) is out
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all()                                       # the rows are complete: every query head was stored
        err = _per_sample(out.cpu(), ref)
        print(f"H={H} Hkv={Hkv} D={D} S={S} {dtype}: per-sample rel err {['%.2e' % x for x in err]} (tol {tol:.0e})")
        assert max(err) <= tol, (S, err)
        _check_filing(c, kvq, scale, kvq0, scale0)
        # two runs are bitwise equal: the output, and the column filed
        kvq2, scale2 = kvq0.clone(), scale0.clone()
        out2 = _run(c, kvq2, scale2)
        assert torch.equal(_bits(out2), _bits(out)) and torch.equal(kvq2.view(torch.uint8), kvq.view(torch.uint8)) and torch.equal(scale2, scale)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [16, 64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (6, 2), (12, 1)])
def test_a_sample_of_masked_keys_returns_the_new_value_row(H, Hkv, D, dtype):
    B = 3
    for S in (1, _lengths(D)[5]):
        c = _case(7 * D + S + H, B, H, Hkv, D, S, dtype, valid="one-masked")
        ref = _reference(c)
        kvq, scale = _device_cache(c)
        kvq0, scale0 = kvq.clone(), scale.clone()
        out = _run(c, kvq, scale).cpu()
        want = _expand(c["v_new"][1], H, Hkv)                                           # the kv head's row for each query head of its group
        assert torch.equal(_bits(out[1]), _bits(want)), (out[1] - want).abs().max()
        err = _per_sample(out, ref)
        assert max(err) <= TOL[dtype], (S, err)
        _check_filing(c, kvq, scale, kvq0, scale0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,Hkv,D", [(4, 2, 64), (12, 1, 16), (8, 1, 128)])
def test_strided_views(H, Hkv, D, dtype):
    """q as the first columns of a fused q|k|v row (as the model passes it), k_new / v_new the halves of one dense buffer, a cache with
    spare columns behind S + 1."""
    B, S = 3, _lengths(D)[2]
    c = _case(11 * D + H, B, H, Hkv, D, S, dtype, cap=S + 5)
    ref = _reference(c)
    kvq, scale = _device_cache(c)
    kvq0, scale0 = kvq.clone(), scale.clone()
    qkv = torch.full((B, (H + 2 * Hkv) * D), float("nan"), dtype=dtype)
    qkv[:, :H * D] = c["q"]
    qkv = qkv.to(DEV)
    out = _run(c, kvq, scale, q=qkv[:, :H * D])
    err = _per_sample(out.cpu(), ref)
    assert max(err) <= TOL[dtype], err
    _check_filing(c, kvq, scale, kvq0, scale0)
    assert torch.equal(_bits(out), _bits(_run(c, kvq0.clone(), scale0.clone())))       # the same bits as from a dense q


def test_refused_calls_leave_out_and_the_cache_untouched():
    from mmgl_amd import ops
    H, Hkv, D, S, B = 4, 2, 64, 9, 2
    c = _case(3, B, H, Hkv, D, S, BF16)
    kvq, scale = _device_cache(c)
    kvq0, scale0 = kvq.clone(), scale.clone()
    d, kd = c["d"], c["kd"]
    q, new = c["q"].to(DEV), torch.cat([c["k_new"], c["v_new"]], dim=1).to(DEV)
    ok = c["ok"].to(DEV)
    out = torch.full((B, d), 7.0, dtype=BF16, device=DEV)
    call = lambda **kw: ops.attn_decode_q8(**{**dict(q=q, k_new=new[:, :kd], v_new=new[:, kd:], kvq=kvq, scale=scale, key_valid=ok, num_heads=H,
                                                     out=out, num_kv_heads=Hkv), **kw})
    with pytest.raises(ValueError, match="full"):
        call(kvq=kvq[:, :S], scale=scale[:, :S])
    with pytest.raises(ValueError, match="no cached columns"):
        call(key_valid=ok[:, :0])
    with pytest.raises(ValueError, match="incompatible codes"):                        # the scale rows of H heads
        call(scale=torch.zeros(B, S + 2, 2 * H, dtype=torch.int8, device=DEV))
    with pytest.raises(ValueError, match="incompatible codes"):                        # the code rows of H heads
        call(kvq=torch.zeros(B, S + 2, 2 * d, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="incompatible q"):                            # k_new / v_new of H heads
        call(k_new=q, v_new=q)
    with pytest.raises(ValueError, match="multiple of num_kv_heads"):
        call(num_kv_heads=3)
    with pytest.raises(ValueError, match="float32 or bfloat16"):                       # fp16
        call(q=q.half(), k_new=new[:, :kd].half(), v_new=new[:, kd:].half(), out=out.half())
    with pytest.raises(ValueError, match="out"):
        call(out=out.float())
    torch.cuda.synchronize()
    assert (out == 7.0).all() and torch.equal(kvq.view(torch.uint8), kvq0.view(torch.uint8)) and torch.equal(scale, scale0)
