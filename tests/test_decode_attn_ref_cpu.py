"""decode_ref.DecodeAttnRef, the fp64 reference behind tests/test_decode_attn_bounds_gpu.py, on the CPU (no GPU needed):

(a) it IS the four references the decode tests have used so far -- decode_ref.attn_decode_ref, beam_ref.attn_beam_ref, kvq_ref.attention,
    t5_decode_ref.attn_decode_relbias_ref (its three wrong variants included) -- to 1e-12 of the largest magnitude, on cases of
    tests/decode_attn_cases.py: the new reference is the old ones, generalised;
(b) the comparison it carries can fail: for each of the eight entry points and both dtypes, EVERY deliberately wrong reference the case
    can tell apart reaches at least one row and leaves the bound on at least 25 % of the elements of the rows it reaches, from the
    references alone.  What a case cannot tell apart by construction it names (Case.blind, Case.wrongs): S = 1 -- one key has weight 1
    with or without it --, S = 2 for the relbias kernel, a dropped key that no row is allowed, a key/value head without a neighbour ...
    never a threshold.  The kernel-specific names of the issue are asserted to be among the ones tested;
(c) the bound's constants cover the arithmetic they were counted from: a float32 numpy emulation of the kernels' order -- the lane's
    VEC-long chain, the xor butterfly, one online-softmax chain per lane group (per key: plain, relbias; per trip of AD_UNROLL or
    TAIL_UNROLL keys: the NQ kernels), the butterfly merge of the lane groups, the waves in order, exp as exp2(fl(x log2e)) -- stays
    inside the bound at the longest chain the GPU cases use (S = 2 I + KPI + 3; the beam tail 16 KPI + 3), with keys in ascending score
    order (the running maximum moves at every step), descending, and edge-weighted.  The worst err / bound is printed: a record, not a
    fitted threshold.  If the emulation left the bound the count would be wrong, not the emulation."""
import numpy as np
import pytest
import torch

import beam_ref
import kvq_ref
import t5_decode_ref
from decode_attn_cases import BF16, CAP, F32, BeamCase, BlockCase, CacheCase, Q8Case, RelbiasCase, gqa_plan, trip
from decode_ref import DecodeAttnRef, attn_decode_ref, decode_geometry

DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="fp32")]


def _close(a, b, what):
    e = (a.double().reshape(b.shape) - b).abs().max().item() / max(b.abs().max().item(), 1e-300)
    assert e <= 1e-12, f"{what}: {e:.2e}"


# ------------------------------------------------------------------------------------------ (a) the old references, generalised
@pytest.mark.parametrize("dtype", DTYPES)
def test_ref_is_the_old_references(dtype):
    for S in (1, 9, 70):                                                        # plain: all three mask layouts in every case
        c = CacheCase(dtype, 32, S, H=3)
        r = c.ref()
        _close(attn_decode_ref(c.q, c.k, c.v, c.valid, c.H), r.want, c.what)
        assert (r.mag >= r.want.abs() * (1 - 1e-12)).all()
        assert float(r.S[~c.valid.any(1)].abs().max()) == 0.0, "a row without an allowed key forms no score"
    for W, n_tail, pat, valid in ((1, 0, "perm", "ragged"), (3, 7, "history", "ragged"), (2, 5, "perm", "none"), (4, 0, "one", "none")):
        c = BeamCase(dtype, 32, W, 21, n_tail, pat, valid)
        n = c.n_tail
        want = beam_ref.attn_beam_ref(c.q, c.k, c.v, c.valid, c.H, W, c.kt[:, :n] if n else None, c.vt[:, :n] if n else None, c.src)
        _close(want, c.ref().want, c.what)
    for S, valid in ((1, "layouts"), (37, "layouts"), (20, "one-masked")):
        c = Q8Case(dtype, 32, S, valid=valid)
        kc, vc = kvq_ref.dequantize_row(c.codes, c.e, c.Hkv)
        _close(kvq_ref.attention(c.q, kc, vc, c.valid, c.k_new, c.v_new, c.H), c.ref().want, c.what)
    for S in (1, 2, 40):
        c = RelbiasCase(dtype, 32, S, H=3)
        for mine, theirs in ((None, None), ("distance s", t5_decode_ref.WRONG[0]), ("no bias", t5_decode_ref.WRONG[1]),
                             ("head h^1", t5_decode_ref.WRONG[2])):
            _close(t5_decode_ref.attn_decode_relbias_ref(c.q, c.k, c.v, c.bias, c.H, wrong=theirs), c.ref(mine).want, f"{c.what} {mine}")


# ------------------------------------------------------------------------------------------ (b) the comparison can fail
def _long(kernel, dtype, D):
    I, KPI, _ = trip(kernel, dtype, D)
    return 2 * I + KPI + 3


def _fail_cases(dtype):
    """kernel -> (cases, the kernel's own wrong names that must be among the tested ones)."""
    I, KPI, TAIL = trip("beam", dtype, 128)
    Ib, Kb, _ = trip("block", dtype, 64)
    Ig, Kg, _ = trip("gqa_block", dtype, 16)
    Iq, Kq, _ = trip("q8", dtype, 64)
    return {
        "plain": ([CacheCase(dtype, 64, _long("plain", dtype, 64)), CacheCase(dtype, 16, 4 * trip("plain", dtype, 16)[1] + 1, huge=True)], ()),
        "gqa": ([CacheCase(dtype, 128, trip("gqa", dtype, 128)[0] + 3, H=6, Hkv=2), CacheCase(dtype, 64, 2, H=9, Hkv=1, first=0)], ()),
        "relbias": ([RelbiasCase(dtype, 64, trip("relbias", dtype, 64)[0] + 1, H=3), RelbiasCase(dtype, 32, 40, few=True)], RelbiasCase.OWN),
        "beam": ([BeamCase(dtype, 128, 3, 4 * KPI + 1, 2 * TAIL + 3, "history"), BeamCase(dtype, 128, 2, I + 3, TAIL + 1, "perm", "none"),
                  BeamCase(dtype, 64, 5, 21, 0, "one")], BeamCase.OWN),
        "block": ([BlockCase(dtype, 64, 5, [0, Kb + 1, Ib + 3], Ib + 3 + 5), BlockCase(dtype, 128, 8, [3, 10], 10 + 8 - 2 + 0)], BlockCase.OWN),
        "gqa_block": ([BlockCase(dtype, 16, 3, [0, Kg + 1, Ig + 3], Ig + 3 + 3, G=3, gqa=True),
                       BlockCase(dtype, 64, 5, [2, 20], 20 + 5 - 2, G=2, gqa=True)], BlockCase.OWN),
        "q8": ([Q8Case(dtype, 64, 4 * Kq + 1), Q8Case(dtype, 16, 70, valid="one-masked")], Q8Case.OWN),
        "gqa_q8": ([Q8Case(dtype, 128, trip("gqa_q8", dtype, 128)[0] + 3, G=5), Q8Case(dtype, 64, 9, G=2)], Q8Case.OWN),
    }


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", ["plain", "gqa", "relbias", "beam", "block", "gqa_block", "q8", "gqa_q8"])
def test_wrong_references_leave_the_bound(kernel, dtype):
    cases, own = _fail_cases(dtype)[kernel]
    tested = set()
    for c in cases:
        assert c.kernel == kernel
        right = c.ref()
        names = c.wrongs(right)
        for name in names:
            share, rows = c.share(right, name)
            print(f"[can fail] {c.what} | {name}: {share:.2f} of the elements of {rows} rows outside the bound")
            assert rows > 0, f"{c.what}: the wrong reference '{name}' reaches no row and is not named in blind()"
            assert share >= CAP, f"{c.what}: '{name}' leaves the bound on only {share:.2f} of the elements of its {rows} rows"
        for name, why in c.blind().items():
            print(f"[can fail] {c.what} | {name}: not told apart -- {why}")
        tested |= set(names)
    generic = {"lane group", "wave", "kv head"} | ({"mask+1"} if kernel != "relbias" else set())     # the relbias kernel has no mask
    assert any(n.startswith("drop@") for n in tested)
    missing = (set(own) | generic) - tested
    assert not missing, f"{kernel}: no case tests the wrong references {sorted(missing)}"


def test_what_a_case_cannot_tell_apart_is_so_by_construction():
    """S = 1: dropping the only key leaves a row uniform over that same key -- the wrong reference IS the right one, bit for bit."""
    c = CacheCase(F32, 64, 1)
    right = c.ref()
    assert "drop@0" in c.blind() and not bool(right.affected(c.ref("drop@0")).any())
    r = RelbiasCase(F32, 64, 1)
    right = r.ref()
    for name in RelbiasCase.OWN:
        assert name in r.blind() and not bool(right.affected(r.ref(name)).any())
    assert set(RelbiasCase.OWN) <= set(RelbiasCase(F32, 64, 2).blind())


def test_the_restated_plans():
    """The GQA block plan of attn_decode_gqa_nq (8 heads per block) and of attn_decode_gqa_q8_nq (4)."""
    assert gqa_plan(9) == (2, 5, 8, [5, 4]) and gqa_plan(12) == (2, 6, 8, [6, 6]) and gqa_plan(16) == (2, 8, 8, [8, 8])
    assert [gqa_plan(G)[2] for G in (1, 2, 3, 4, 5, 7, 8)] == [1, 2, 4, 4, 8, 8, 8]
    assert gqa_plan(5, 4) == (2, 3, 4, [3, 2]) and gqa_plan(8, 4) == (2, 4, 4, [4, 4]) and gqa_plan(4, 4) == (1, 4, 4, [4])
    assert decode_geometry("q8", BF16, 64) == (16, 4, 16, 256) and decode_geometry("plain", BF16, 128) == (8, 16, 4, 64)
    assert decode_geometry("plain", F32, 128) == (4, 32, 2, 32)


# ------------------------------------------------------------------------------------------ (c) the count covers the arithmetic
f32 = np.float32
LOG2E = f32(1.4426950408889634)
NEG = f32(-3.4028234663852886e38)


def _exp(x):
    """__expf: v_exp_f32 of the rounded product x log2e."""
    return np.exp2((x.astype(f32) * LOG2E).astype(f32)).astype(f32)


def emulate(q, phases, VEC):
    """One (row, head) in float32, in the order of the kernels.  q [D]; phases: (k [n,D], v [n,D], ok [n], U, bias [n] or None) -- the
    cache / prefix loop (U = 1: attn_decode_kernel, a state update per key; U = 4: the NQ kernels' trip) and the beam tail (U = 2) run
    through the same 4 KPI lane-group states."""
    D = q.size
    LPK = D // VEC
    KPI = 64 // LPK
    NG = 4 * KPI
    g = np.arange(NG)
    m, l, acc = np.full(NG, NEG, f32), np.zeros(NG, f32), np.zeros((NG, D), f32)
    qc = q.astype(f32).reshape(LPK, VEC)
    with np.errstate(all="ignore"):
        for k, v, ok, U, bias in phases:
            n = k.shape[0]
            if n == 0:
                continue
            kc, v = k.astype(f32).reshape(n, LPK, VEC), v.astype(f32)
            part = np.zeros((n, LPK), f32)
            for e in range(VEC):                                                   # the lane's chain
                part = (part + (qc[None, :, e] * kc[:, :, e]).astype(f32)).astype(f32)
            o = 1
            while o < LPK:                                                         # xor butterfly over the lanes of a key
                part = (part + part[:, np.arange(LPK) ^ o]).astype(f32)
                o <<= 1
            sc = part[:, 0]
            if bias is not None:
                sc = (sc + bias.astype(f32)).astype(f32)
            sc = np.where(ok, sc, NEG).astype(f32)
            for t in range(-(-n // (NG * U))):
                idx = g[None, :] + (t * U + np.arange(U))[:, None] * NG                # [U, NG]: lane group g's keys of the trip
                inn, idc = idx < n, np.minimum(idx, n - 1)
                su = sc[idc]
                mn = m.copy()
                for u in range(U):
                    mn = np.where(inn[u], np.maximum(mn, su[u]), mn)
                corr = _exp(m - mn)
                pu = np.where(inn, _exp(su - mn[None]), f32(0))
                ps = np.zeros(NG, f32)
                for u in range(U):
                    ps = (ps + pu[u]).astype(f32)
                l = ((l * corr).astype(f32) + ps).astype(f32)
                a = (acc * corr[:, None]).astype(f32)
                for u in range(U):
                    a = (a + (pu[u][:, None] * v[idc[u]]).astype(f32)).astype(f32)
                acc, m = a, mn
        o = 1
        while o < KPI:                                                             # butterfly merge of a wave's lane groups
            pg = (g // KPI) * KPI + ((g % KPI) ^ o)
            m2, l2, a2 = m[pg], l[pg], acc[pg]
            mn = np.maximum(m, m2)
            c1, c2 = _exp(m - mn), _exp(m2 - mn)
            l = ((l * c1).astype(f32) + (l2 * c2).astype(f32)).astype(f32)
            acc = ((acc * c1[:, None]).astype(f32) + (a2 * c2[:, None]).astype(f32)).astype(f32)
            m = mn
            o <<= 1
        mw, lw, aw = m[::KPI], l[::KPI], acc[::KPI]                                # the waves in order
        mm = mw.max()
        ll, out = f32(0), np.zeros(D, f32)
        for i in range(4):
            ci = _exp(mw[i:i + 1] - mm)[0]
            ll = f32(ll + f32(lw[i] * ci))
            out = (out + (aw[i] * ci).astype(f32)).astype(f32)
        return (out / ll).astype(f32)


def _emulate_case(c, U, U2=None):
    """Every (row, head) of the case through emulate(); -> got [R, H*D] in the case's dtype."""
    x = c.expand(None, "cpu")
    R, N = x["allowed"].shape
    VEC = decode_geometry(c.kernel, c.dtype, c.D)[0]
    q = x["q"].float().reshape(R, c.H, c.D).numpy()
    k, v = (x[n].float().reshape(R, N, c.Hkv, c.D).numpy() for n in ("k", "v"))
    ok = x["allowed"].numpy()
    bias = None if x.get("bias") is None else x["bias"].float().numpy()
    out = np.zeros((R, c.H, c.D), f32)
    for r in range(R):
        for h in range(c.H):
            hk, b = h // c.G, None if bias is None else bias[h]
            ph = [(k[r, :c.S1, hk], v[r, :c.S1, hk], ok[r, :c.S1], U, b)]
            if N > c.S1:
                ph.append((k[r, c.S1:, hk], v[r, c.S1:, hk], ok[r, c.S1:], U2, None))
            out[r, h] = emulate(q[r, h], ph, VEC)
    return torch.from_numpy(out).reshape(R, -1).to(c.dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [16, 64, 128])
def test_the_emulated_arithmetic_stays_inside_the_bound(D, dtype):
    worst = {}
    for order in ("asc", "desc", None):
        _, KPI, TAIL = trip("beam", dtype, D)
        cases = [(CacheCase(dtype, D, _long("plain", dtype, D), H=2, B=3 if order is None else 1, order=order), 1, None),
                 (RelbiasCase(dtype, D, _long("relbias", dtype, D), H=2, B=1, order=order), 1, None),
                 (CacheCase(dtype, D, _long("gqa", dtype, D), H=4, Hkv=2, B=3 if order is None else 1, order=order), 4, None),
                 (BeamCase(dtype, D, 2, _long("beam", dtype, D), 2 * TAIL + 3, "history", B=1 if order else 2, order=order), 4, 2)]
        for c, U, U2 in cases:
            assert c.counts == DecodeAttnRef.counts(c.kernel, dtype, D, c.S1, getattr(c, "n_tail", 0))
            ratio = c.ref().check(_emulate_case(c, U, U2), f"{c.what} (fp32 emulation)", "emulation")
            worst[c.kernel] = max(worst.get(c.kernel, 0.0), ratio)
    print(f"[emulation] D={D} {dtype}: worst err/bound {worst}")
