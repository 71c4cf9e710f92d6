"""-m gpu: the causal self-attention kernels (csrc/selfattn32.hip, csrc/selfattn.hip) against attn_ref.SelfAttnRef -- an fp64 reference of
the storage-rounded operands -- element by element: out, lse, dq, dk, dv each within u |want| + (c + n 2^-24 S) mag (the count is in
SelfAttnRef's docstring; tests/test_selfattn_ref_cpu.py shows on the CPU that this comparison fails for a mask or head mapping that is
off by one).  Every case uses the recency-ramp inputs (the newest allowed key carries ~40 % of a row), and the forward also a plain
randn set (the flat-softmax regime).  Gradient buffers hold NaN before the call.  B = 2, H = 3 unless stated: an odd H exercises the
split of the grid index into (sample, head, query block).

Masks (key 0 always valid): M0 all valid; M1 the last sample right-padded to L of {1, 63, 64, 65, 128, T - 1} where L < T; M2 the
WikiWeb2M layout prompt | pad | summary | pad with hole edges at 70 and T - T // 5, no tile multiple.

  A  the 32x32 route (bf16, D 64 / 128, at most 4096 key rows) at T around the 64-key tile and the 128-row blocks
  B  the 16x16 route (fp32 any D, bf16 D 16 / 32) at the same edges and either side of its query block 4 * 16 * QT
  C  the dispatch boundary: 4096 key rows (32x32, the 64-entry valid-word table full), 4097 and 4160 (the bf16 D 64 / 128
     instantiations of the 16x16 forward, dQ and dK/dV kernels, which nothing else reaches), with and without a 20-key prefix
  D  prefix keys, P on either side of a tile, through the raw entry points and ops.selfattn_core_prefix under autograd
  E  grouped-query heads: the first comparison of the GQA gradients with an independent reference at a per-element bound
  F  nothing outside the tensors is read into a result or written: NaN / Inf behind the last sample and in the pad columns of
     free row strides, sentinels behind every output
  G  two calls of every A and C case are bitwise equal"""
import pytest
import torch

from attn_ref import SelfAttnRef
from bounds import BF16, F32, NAME, NAN, Slab

pytestmark = pytest.mark.gpu

SEED = 2                    # tests/test_selfattn_ref_cpu.py: the seed at which every wrong reference leaves the bound on >= 40 %


def _case(group, dtype, D, T, layout="M0", L=None, B=2, H=3, Hkv=None, P=0):
    return (group, dtype, D, T, layout, L, B, H, Hkv or H, P)


def _id(c):
    group, dtype, D, T, layout, L, B, H, Hkv, P = c
    return (f"{NAME[dtype]}-D{D}-T{T}" + (f"-P{P}" if P else "") + (f"-H{H}kv{Hkv}" if Hkv != H else "")
            + (f"-B{B}H{H}" if (B, H) != (2, 3) and Hkv == H else "") + f"-{layout}" + (f"L{L}" if L else ""))


def _masks(T, m2=False):
    """(layout, L) of M0, every M1 that fits T, and M2 where asked for."""
    fit = sorted({L for L in (1, 63, 64, 65, 128, T - 1) if 1 <= L < T})
    return [("M0", None)] + [("M1", L) for L in fit] + ([("M2", None)] if m2 else [])


def _query_block(dtype, D):
    """4 * 16 * QT of the 16x16 forward kernel, QT from XC<T, D, 4, 1> (csrc/attn_common.h):
    QT = 2 if 1 * 4 * (D / 16) * (sizeof(T) / 2) <= 32 else 1 -- 128 rows everywhere but fp32 D = 128 (64 rows)."""
    es = 4 if dtype == F32 else 2
    return 4 * 16 * (2 if 4 * (D // 16) * (es // 2) <= 32 else 1)


ROUTE32 = [(BF16, 64), (BF16, 128)]
ROUTE16 = [(F32, 16), (F32, 32), (F32, 64), (F32, 128), (BF16, 16), (BF16, 32)]
CASES_A = [_case("A", dt, D, T, lay, L) for dt, D in ROUTE32 for T in (1, 63, 64, 65, 127, 128, 129, 193, 257)
           for lay, L in _masks(T, m2=T == 257)]
CASES_B = [_case("B", dt, D, T, lay, L) for dt, D in ROUTE16
           for T in sorted({1, 63, 65, 129, 257, _query_block(dt, D) - 1, _query_block(dt, D), _query_block(dt, D) + 1})
           for lay, L in _masks(T, m2=T == 257)]
# The dK / dV launcher of selfattn.hip picks PAR from lds_for(2) <= 160 KiB (XC<T, D, 2>: 4 row images of 32 x DPAD plus 8 tiles of
# 32 x (DPAD + 16), or the 2 x 2 fp32 reduction buffers if larger): bf16 D = 64 -> 56 KiB, bf16 D = 128 -> 104 KiB, fp32 D = 16 / 32 /
# 64 -> 64 / 64 / 112 KiB: PAR = 2; fp32 D = 128 -> 208 KiB: PAR = 1, the only one.  So the bf16 cases here run PAR = 2, and PAR = 1 is
# covered by group B's fp32 D = 128 cases.
CASES_C = ([_case("C", BF16, D, T, lay, L, B=1, H=H) for D, H in ((64, 2), (128, 1)) for T in (4096, 4097, 4160)
            for lay, L in (("M0", None), ("M1", 4033))]          # L = 4033: the last 64-key tile dead, the one before it partly live
           + [_case("C", BF16, 64, Tk - 20, lay, L, B=1, H=2, P=20) for Tk in (4096, 4097) for lay, L in (("M0", None), ("M1", 4033 - 20))])
CASES_D = [_case("D", dt, D, T, "M1", L, P=P) for dt, D in ((BF16, 64), (F32, 32)) for P in (1, 20, 64, 65, 130) for T in (63, 129)
           for _, L in _masks(T)[1:]]
CASES_E = [_case("E", dt, D, T, lay, L, H=H, Hkv=Hkv) for dt, D in ((BF16, 64), (BF16, 128), (F32, 32)) for H, Hkv in ((6, 3), (4, 1))
           for T in (65, 129) for lay, L in _masks(T)]
CASES_F = [_case("F", dt, D, T, lay, L) for dt, D in ((BF16, 64), (F32, 32)) for T in (65, 129, 193) for lay, L in (("M0", None), ("M1", 64))]


def _inputs(c, ramp=True):
    group, dtype, D, T, layout, L, B, H, Hkv, P = c
    q, k, v, dout = SelfAttnRef.inputs(dtype, B, T, H, D, Hkv, P, seed=SEED, ramp=ramp, device="cuda")
    return q, k, v, dout, SelfAttnRef.mask(B, T, layout, L, P).cuda()


def _forward(c, q, k, v, am):
    from mmgl_amd import ops
    from mmgl_amd._lib import ptr
    group, dtype, D, T, layout, L, B, H, Hkv, P = c
    if Hkv != H:
        return ops._gqa_fwd(q, ptr(q), ptr(k), ptr(v), am, B, T, H, Hkv, D, 0, 0)
    return ops._selfattn_fwd(q, ptr(q), ptr(k), ptr(v), am, B, T, H * D, H, P if (P or group == "D") else None, 0)


def _call(c, q, k, v, dout, am):
    """out, lse, dq, dk, dv of the raw entry points; the gradient buffers hold NaN before the call."""
    from mmgl_amd import ops
    from mmgl_amd._lib import ptr
    group, dtype, D, T, layout, L, B, H, Hkv, P = c
    out, lse = _forward(c, q, k, v, am)
    dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))
    if Hkv != H:
        ops._gqa_bwd(q, dout, ptr(q), ptr(k), ptr(v), out, lse, am, ptr(dq), ptr(dk), ptr(dv), B, T, H, Hkv, D, 0, 0, 0, 0)
    else:
        ops._selfattn_bwd(q, dout, ptr(q), ptr(k), ptr(v), out, lse, am, ptr(dq), ptr(dk), ptr(dv), B, T, H * D, H,
                          P if (P or group == "D") else None, 0, 0)
    torch.cuda.synchronize()
    return out, lse, dq, dk, dv


def _check(c):
    group, dtype, D, T, layout, L, B, H, Hkv, P = c
    q, k, v, dout, am = _inputs(c)
    got = _call(c, q, k, v, dout, am)
    SelfAttnRef(q, k, v, am, dout, H, Hkv, P).check(got, _id(c), group)
    # the forward once more on plain randn inputs: a flat softmax, every key of a row carries about the same weight
    q, k, v, dout, am = _inputs(c, ramp=False)
    out, lse = _forward(c, q, k, v, am)
    torch.cuda.synchronize()
    SelfAttnRef(q, k, v, am, dout, H, Hkv, P).check((out, lse, None, None, None), _id(c), group + " randn")
    return got


@pytest.mark.parametrize("case", CASES_A, ids=_id)
def test_A_route_32x32(case):
    _check(case)


@pytest.mark.parametrize("case", CASES_B, ids=_id)
def test_B_route_16x16(case):
    _check(case)


@pytest.mark.parametrize("case", CASES_C, ids=_id)
def test_C_dispatch_boundary(case):
    _check(case)


@pytest.mark.parametrize("case", CASES_D, ids=_id)
def test_D_prefix(case):
    from mmgl_amd import ops
    group, dtype, D, T, layout, L, B, H, Hkv, P = case
    got = _check(case)
    q, k, v, dout, am = _inputs(case)
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    out = ops.selfattn_core_prefix(qg, kg, vg, am, H, P)
    grads = torch.autograd.grad(out, (qg, kg, vg), dout)
    for name, a, b in zip(("out", "dq", "dk", "dv"), (out,) + grads, (got[0],) + got[2:]):
        assert torch.equal(a, b), f"{name}: ops.selfattn_core_prefix under autograd is not the raw entry point's result"


@pytest.mark.parametrize("case", CASES_E, ids=_id)
def test_E_grouped_query(case):
    _check(case)


# ------------------------------------------------------------------------------------------ F: nothing outside the tensors
TAIL = 128                 # rows behind the last sample
SENTINEL = 777.0


def _windowed(c, fill):
    """The call through mmgl_selfattn_prefix_fwd / _bwd (P = 0: they take separate row strides for q and k / v) with every operand a
    window of a larger buffer: TAIL rows behind the last sample and the pad columns of the free row strides hold `fill` on the
    inputs and SENTINEL on the outputs, as do the guards of each Slab; the key mask has TAIL more bytes, all 1.  Returns the payloads
    and the output slabs."""
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr
    group, dtype, D, T, layout, L, B, H, Hkv, P = c
    HD, rows = H * D, B * T
    ldq, ldk, ldgq, ldgk = HD + 24, HD + 40, HD + 8, HD + 56
    q, k, v, dout, am = _inputs(c)

    def window(x, ld):
        return Slab((rows, HD), dtype, fill, x.reshape(rows, HD), ld=ld, extra=TAIL).v

    def target(ld):
        s = Slab((rows, HD), dtype, SENTINEL, ld=ld, extra=TAIL)
        s.v.fill_(NAN)
        return s

    qb, kb, vb, gb = window(q, ldq), window(k, ldk), window(v, ldk), window(dout, HD)
    amb = torch.ones(rows + TAIL, dtype=torch.uint8, device="cuda")
    amb[:rows] = am.reshape(-1)
    outs = dict(out=target(HD), lse=Slab((B * H * T,), F32, SENTINEL), dq=target(ldgq), dk=target(ldgk), dv=target(ldgk))
    outb, lseb, dqb, dkb, dvb = (outs[n].v for n in SelfAttnRef.NAMES)
    code, st = _lib.dtype_code(qb), _lib.stream_ptr()
    _lib.call("mmgl_selfattn_prefix_fwd", None, ptr(qb), ptr(kb), ptr(vb), ptr(amb), ptr(outb), ptr(lseb), B, H, T, 0, D, ldq, ldk, code, st)
    nbytes = _lib.lib().mmgl_selfattn_bwd_workspace(B, H, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.call("mmgl_selfattn_prefix_bwd", None, ptr(gb), ptr(qb), ptr(kb), ptr(vb), ptr(outb), ptr(lseb), ptr(amb), ptr(dqb), ptr(dkb),
              ptr(dvb), ptr(ws), nbytes, B, H, T, 0, D, ldq, ldk, ldgq, ldgk, code, st)
    torch.cuda.synchronize()
    payload = tuple(b.reshape(B, T, HD) for b in (outb, dqb, dkb, dvb))
    got = (payload[0], lseb.view(B, H, T)) + payload[1:]
    return (q, k, v, dout, am), got, outs


@pytest.mark.parametrize("case", CASES_F, ids=_id)
def test_F_nothing_outside_the_tensors(case):
    group, dtype, D, T, layout, L, B, H, Hkv, P = case
    (q, k, v, dout, am), clean, _ = _windowed(case, 0.0)
    SelfAttnRef(q, k, v, am, dout, H).check(clean, _id(case), "F")
    for fill in (float("nan"), float("inf")):
        _, got, outs = _windowed(case, fill)
        for name, a, b in zip(SelfAttnRef.NAMES, got, clean):
            assert torch.isfinite(a.float()).all(), f"{name}: {fill} behind the last sample or in a pad column reached the result"
            assert torch.equal(a, b), f"{name}: differs from the run with zeros outside the tensors (fill {fill})"
        for name, s in outs.items():
            assert s.untouched(), f"{name}: rows behind the last sample (lse: the last row) or a pad column were written"


# ------------------------------------------------------------------------------------------ G: determinism
@pytest.mark.parametrize("case", CASES_A + CASES_C, ids=lambda c: c[0] + "-" + _id(c))
def test_G_two_calls_are_bitwise_equal(case):
    q, k, v, dout, am = _inputs(case)
    first, second = _call(case, q, k, v, dout, am), _call(case, q, k, v, dout, am)
    for name, a, b in zip(SelfAttnRef.NAMES, first, second):
        assert torch.isfinite(a.float()).all(), name
        assert torch.equal(a, b), f"{name}: two calls differ"
