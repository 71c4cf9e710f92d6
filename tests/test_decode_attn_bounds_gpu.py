"""-m gpu: the eight single-query attention entry points of csrc/decode.hip, every element against decode_ref.DecodeAttnRef:

    |got - want| <= u |want| + (n_s S_i + n_c) 2^-24 mag          u = 2^-8 (bf16), 2^-23 (fp32)

with n_s, n_c counted from the kernels' statements (the class docstring has the count; tests/test_decode_attn_ref_cpu.py shows without a
GPU that the bound covers an fp32 emulation of the kernels' order and that wrong references leave it).  The cases are
tests/decode_attn_cases.py's: edge-weighted operands in the kernels' own layouts, through the ops wrappers, `out` pre-filled with NaN.
Before a case compares anything it asserts from the references alone that at least 25 % of what one wrong reference of its kind
reaches lies outside the bound, and for bf16 that the bound is nowhere below the store's half ulp.

The trip constants are restated (decode_attn_cases.trip, gqa_plan, pair_plan; KPI keys per wave and load, 4 KPI per workgroup and load,
I = 16 KPI per loop trip, 8 KPI per trip of the beam tail) and every case list asserts that the states it is there for are reached:
  plain      S on both sides of KPI, 4 KPI and I, two trips and a tail; all-valid / holed / no-valid-key samples in every call; keys in
             ascending and descending score order at the longest chain; 1e30 on the masked keys
  GQA        G in {1 .. 16}: NQ = 1, 2, 4, 8, surplus slots of the 8-wide instantiation (G = 5, 7), G = 9 -> blocks of 5 and 4 through
             the min(j, nq - 1) clamp, G = 12 -> 6 + 6; G = 1 through the GQA entry itself (the wrapper routes Hkv = H to the plain kernel)
  beam       W in {1 .. 8}, three prefix straddles, n_tail up to 16 KPI + 3: the SECOND tail trip (n_tail > 8 KPI) in both dtypes,
             the three src patterns, a fully masked prefix with and without a tail
  block      m in {1, 2, 5, 8}, ragged lens with 0, KPI + 1, I + 3 and capacity - m + 2 (rows at or past the capacity: unspecified,
             excluded, counted exactly); fp32 D = 128 m = 8: every one of the 4 KPI = 8 lane groups holds a new key; the filed columns
             bitwise and no other cache byte changed
  GQA block  (m, G) in {(1,1), (2,4), (8,1), (3,3), (5,2), (8,3)} at a small batch (the plan shrinks to one pair per block) and at a
             batch sized from the device's CU count so that the plan keeps blocks of up to 8 pairs: pairs of more than one token and
             head in a block, a short last block
  q8, GQA q8 D in {16, 64, 128} around the kernels' own trips (16 codes per lane: KPI = 1024 / D), heads differing by 2^6 and keys
             against values by 2^6 the other way, G in {1, 2, 4, 5, 8} (blocks of 4 heads: 5 -> 3 + 2, 8 -> 4 + 4), a sample of masked
             cached keys -> the new value row bitwise, column S filed bitwise and no other byte changed
  relbias    H in {2, 3}, D in {32, 64}, S from 1 to two trips and a tail, a T5 table drawn N(0, 2) with ld_bias > S, and -1e30 on all
             but a few distances
One `[bound <kernel>] <case>: max err/bound` line per case with -s; docs/decode_attn_bounds_mi355x.md keeps the worst of a run."""
import pytest
import torch

from decode_attn_cases import BF16, F32, BeamCase, BlockCase, CacheCase, Q8Case, RelbiasCase, gqa_plan, pair_plan, trip

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="fp32")]


def _check(c):
    """The case's can-fail assertion from the references alone, then the kernel against the bound on every specified element."""
    right = c.ref(dev=DEV)
    c.assert_can_fail(right, DEV)
    return right.check(c.run(DEV), c.what, c.kernel, rows=c.rows())


def _worst(kernel, dtype, ratios):
    print(f"[bound {kernel}] worst of {len(ratios)} {'bf16' if dtype == BF16 else 'fp32'} cases: {max(ratios):.3f}")


def _lengths(kernel, dtype, D):
    I, KPI, _ = trip(kernel, dtype, D)
    return sorted({1, 2, KPI - 1, KPI, KPI + 1, 4 * KPI - 1, 4 * KPI + 1, I - 1, I, I + 1, 2 * I + KPI + 3} - {0})


# ------------------------------------------------------------------------------------------ plain
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_plain(D, dtype):
    I, KPI, _ = trip("plain", dtype, D)
    lengths = _lengths("plain", dtype, D)
    for edge in (KPI, 4 * KPI, I):
        assert any(S < edge for S in lengths) and any(S > edge for S in lengths) and (edge in lengths or edge + 1 in lengths)
    assert -(-max(lengths) // I) == 3 and max(lengths) % I, "two workgroup trips and a tail"
    cases = [CacheCase(dtype, D, S, first=i) for i, S in enumerate(lengths)]
    assert all(len({int(v.any()) + int(v.all()) for v in c.valid}) == 3 for c in cases if c.S1 > 1), "all valid | holed | no valid key in every call"
    cases += [CacheCase(dtype, D, S, huge=True) for S in (4 * KPI + 1, max(lengths))]
    _worst("plain", dtype, [_check(c) for c in cases])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ["asc", "desc"])
def test_plain_long_chain_in_score_order(order, dtype):
    D = 64
    I, KPI, _ = trip("plain", dtype, D)
    c = CacheCase(dtype, D, 2 * I + KPI + 3, order=order)
    s = torch.einsum("bhd,bshd->bhs", c.q.double().reshape(3, 2, D), c.k.double().reshape(3, c.S1, 2, D))
    step = (s[..., 4 * KPI:] - s[..., :-4 * KPI])                     # a lane group's next key lies 4 KPI further
    assert (step > 0).double().mean() > 0.9 if order == "asc" else (step < 0).double().mean() > 0.9, "the running maximum moves at every step / never"
    _check(c)


# ------------------------------------------------------------------------------------------ GQA
GROUPS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gqa(dtype):
    assert gqa_plan(9) == (2, 5, 8, [5, 4]), "G = 9: a short last block through the min(j, nq - 1) clamp of the 8-wide instantiation"
    assert gqa_plan(12)[3] == [6, 6] and gqa_plan(16)[3] == [8, 8]
    assert {gqa_plan(G)[2] for G in GROUPS} == {1, 2, 4, 8} and [gqa_plan(G)[3] for G in (5, 7)] == [[5], [7]], "surplus slots of NQ = 8"
    grid = [(G, 128 if dtype == BF16 else 64) for G in GROUPS] + [(G, D) for G in (3, 9) for D in (16, 128)]
    ratios = []
    for i, (G, D) in enumerate(grid):
        I, KPI, _ = trip("gqa", dtype, D)
        for S in (KPI + 5, I + 3):
            c = CacheCase(dtype, D, S, H=2 * G, Hkv=2, first=i, force_gqa=True)
            assert c.kernel == "gqa"
            ratios.append(_check(c))
    _worst("gqa", dtype, ratios)


# ------------------------------------------------------------------------------------------ beam
PATTERNS = ("perm", "one", "history")


def _beam_grid(dtype, D):
    I, KPI, TAIL = trip("beam", dtype, D)
    tails = [0, 1, KPI - 1, KPI + 1, 4 * KPI + 1, TAIL - 1, TAIL + 1, 2 * TAIL + 3]
    return [(S, n) for S in (KPI + 1, 4 * KPI + 1, I + 3) for n in tails]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("W", [1, 2, 3, 4, 5, 8])
def test_beam(W, dtype):
    D = 128
    I, KPI, TAIL = trip("beam", dtype, D)
    assert TAIL == (32 if dtype == BF16 else 16)
    grid = _beam_grid(dtype, D)
    assert sum(n > TAIL for _, n in grid) >= 6 and any(n == TAIL - 1 for _, n in grid), "the second tail trip, and the last key of the first"
    cases = [BeamCase(dtype, D, W, S, n, PATTERNS[i % 3], seed=i) for i, (S, n) in enumerate(grid)]
    assert {c.pattern for c in cases if c.n_tail > TAIL} == set(PATTERNS)
    cases += [BeamCase(dtype, D, W, 4 * KPI + 1, n, "history", valid="none") for n in (0, TAIL + 1)]       # a fully masked prefix
    _worst("beam", dtype, [_check(c) for c in cases])


@pytest.mark.parametrize("D,dtype", [(64, BF16), (16, BF16), (64, F32), (16, F32)], ids=["64-bf16", "16-bf16", "64-fp32", "16-fp32"])
def test_beam_tail_edges_at_the_other_head_dims(D, dtype):
    I, KPI, TAIL = trip("beam", dtype, D)
    assert TAIL == {(64, BF16): 64, (16, BF16): 256, (64, F32): 32, (16, F32): 128}[(D, dtype)]
    cases = [BeamCase(dtype, D, W, KPI + 1, n, pat, seed=W) for W, n, pat in ((3, TAIL - 1, "history"), (5, TAIL + 1, "perm"), (2, 2 * TAIL + 3, "one"))]
    _worst("beam", dtype, [_check(c) for c in cases])


# ------------------------------------------------------------------------------------------ block
def _lens(kernel, dtype, D, m):
    """Ragged lens [0, KPI + 1, I + 3, capacity - m + 2 (at most the capacity)] and the capacity."""
    I, KPI, _ = trip(kernel, dtype, D)
    cap = I + 3 + m + 1
    return [0, KPI + 1, I + 3, min(cap - m + 2, cap)], cap


def _excluded(c, m):
    """Exactly the rows of the last sample whose own column is at or past the capacity are left out, and no others."""
    gone = (~c.rows()).nonzero().flatten().tolist()
    R = c.q.shape[0]
    assert gone == list(range(R - min(2, m), R)), (c.what, gone)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 2, 5, 8])
def test_block(m, dtype):
    ratios = []
    for D in ((64, 128) if dtype == BF16 else (32, 128)):
        lens, cap = _lens("block", dtype, D, m)
        c = BlockCase(dtype, D, m, lens, cap)
        _excluded(c, m)
        if dtype == F32 and D == 128 and m == 8:
            assert 4 * c.KPI == 8 == m, "every lane group of the workgroup holds a new key"
        ratios.append(_check(c))
    _worst("block", dtype, ratios)


# ------------------------------------------------------------------------------------------ GQA block
PAIRS = ((1, 1), (2, 4), (8, 1), (3, 3), (5, 2), (8, 3))


@pytest.mark.parametrize("dtype", DTYPES)
def test_gqa_block_small_batch(dtype):
    assert [m * G for m, G in PAIRS] == [1, 8, 8, 9, 10, 24]
    ratios = []
    for D in ((64, 16) if dtype == BF16 else (128, 16)):
        for m, G in PAIRS:
            lens, cap = _lens("gqa_block", dtype, D, m)
            c = BlockCase(dtype, D, m, lens, cap, G=G, Hkv=2, gqa=True)
            _excluded(c, m)
            ratios.append(_check(c))
    _worst("gqa_block", dtype, ratios)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,G", [(2, 4), (8, 1), (3, 3), (5, 2), (8, 3)])
def test_gqa_block_blocks_of_pairs(m, G, dtype):
    """A batch large enough for the plan to keep blocks of up to 8 pairs: B Hkv cdiv(P, 4) workgroups exceed two per CU."""
    D, Hkv, P = 16, 8, m * G
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * num_cu // (Hkv * -(-P // 4)) + 1
    nblk, ppb, nq, sizes = pair_plan(B, Hkv, m, G, num_cu)
    assert nq == 8 and ppb > 4 and sum(sizes) == P, (B, nblk, ppb, sizes)
    first = [(p // G, p % G) for p in range(sizes[0])]
    assert len({t for t, _ in first}) > 1 and (G == 1 or len({g for _, g in first}) > 1), "pairs of more than one token and head in a block"
    if (m, G) in ((3, 3), (5, 2)):
        assert {(3, 3): [5, 4], (5, 2): [5, 5]}[(m, G)] == sizes
    lens4, cap = _lens("gqa_block", dtype, D, m)
    c = BlockCase(dtype, D, m, [lens4[b % 4] for b in range(B)], cap, G=G, Hkv=Hkv, gqa=True)
    assert int((~c.rows()).sum()) == min(2, m) * sum(1 for b in range(B) if b % 4 == 3)
    _check(c)


# ------------------------------------------------------------------------------------------ q8, GQA q8
def _q8_lengths(D):
    I, KPI, _ = trip("q8", BF16, D)
    assert (KPI, I) == (1024 // D, 16 * 1024 // D), "Q8_VEC = 16 codes per lane: LPK = D / 16"
    return [1, KPI - 1, KPI + 1, 4 * KPI + 1, I - 1, I + 3]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [16, 64, 128])
def test_q8(D, dtype):
    cases = [Q8Case(dtype, D, S, valid=("layouts", "one-masked")[i % 2], seed=i) for i, S in enumerate(_q8_lengths(D))]
    assert all(c.kernel == "q8" for c in cases) and {c.valid_kind for c in cases} == {"layouts", "one-masked"}
    _worst("q8", dtype, [_check(c) for c in cases])


@pytest.mark.parametrize("dtype", DTYPES)
def test_gqa_q8(dtype):
    assert gqa_plan(5, 4) == (2, 3, 4, [3, 2]) and gqa_plan(8, 4) == (2, 4, 4, [4, 4]) and gqa_plan(4, 4) == (1, 4, 4, [4]), "blocks of 4 query heads"
    assert [gqa_plan(G, 4)[2] for G in (2, 4, 5, 8)] == [2, 4, 4, 4]
    grid = [(G, 64, S) for G in (2, 4, 5, 8) for S in _q8_lengths(64)] + [(G, D, S) for G in (5, 8) for D in (16, 128) for S in _q8_lengths(D)[2::3]]
    cases = [Q8Case(dtype, D, S, G=G, valid=("layouts", "one-masked")[i % 2], seed=i) for i, (G, D, S) in enumerate(grid)]
    assert all(c.kernel == "gqa_q8" for c in cases)
    _worst("gqa_q8", dtype, [_check(c) for c in cases])


# ------------------------------------------------------------------------------------------ relbias
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,D", [(2, 32), (3, 64), (3, 32), (2, 64)])
def test_relbias(H, D, dtype):
    I, KPI, _ = trip("relbias", dtype, D)
    lengths = sorted({1, 2, 17, KPI + 1, I - 1, I, I + 1, 2 * I + KPI + 3})
    cases = [RelbiasCase(dtype, D, S, H=H, seed=S) for S in lengths]
    assert all(c.bias.stride(0) > c.S1 for c in cases), "ld_bias > S"
    cases += [RelbiasCase(dtype, D, S, H=H, few=True) for S in (17, 2 * I + KPI + 3)]
    _worst("relbias", dtype, [_check(c) for c in cases])
