"""-m gpu: mmgl_logits_process (csrc/logits.hip) through ops.process_logits, BITWISE against the restatement of its contract in
tests/logits_ref.py (itself held bitwise against transformers' processors by tests/test_logits_process_cpu.py); fp32 rows whose
history lies in [0, V) are also compared with transformers' chain directly.  For bf16 the restatement runs in fp32 on the upcast
logits and rounds once.

Every case embeds the logits in a larger NaN-filled allocation -- two guard rows in front, two behind, 24 guard columns behind V (the
row stride is V + 24) -- and compares the WHOLE allocation bit for bit with the expected one: the targets hold the restatement's bits,
every other element its own.  Every case runs twice on equal inputs and compares the two results bit for bit."""
import pytest
import torch

from logits_ref import compact, hf_chain, process

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="fp32")]
DEV = "cuda"
GUARD_ROWS, GUARD_COLS = 2, 24


def _ops():
    from mmgl_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _embedded(rows, V, dtype, g):
    """(the NaN-filled allocation on the CPU, the slice of it that is the logits [rows, V] with row stride V + 24)."""
    buf = torch.full((rows + 2 * GUARD_ROWS, V + GUARD_COLS), float("nan"), dtype=dtype)
    buf[GUARD_ROWS:GUARD_ROWS + rows, :V] = (torch.randn(rows, V, generator=g) * 3.0).to(dtype)
    return buf


def _history(rows, L, V, g, alphabet=6):
    """Duplicate-heavy: two columns of three from a small alphabet (n-grams repeat), the third from the whole vocabulary, and the two
    ends of the vocabulary in every row that has room."""
    h = torch.randint(0, V, (rows, L), generator=g)
    small = torch.randint(7, 7 + alphabet, (rows, L), generator=g)
    pick = torch.arange(L) % 3 != 2
    h[:, pick] = small[:, pick]
    if L >= 8:
        h[:, 2] = 0
        h[:, 5] = V - 1
    return h


def _valid(rows, n_masked, g, all_masked_row=None):
    v = torch.rand(rows, n_masked, generator=g) < 0.6          # gaps
    if all_masked_row is not None and all_masked_row < rows:
        v[all_masked_row] = False
    return v


def _run_and_check(buf, rows, V, hist, valid, p, n, ban, what, hist_dev=None, valid_dev=None, with_hf=True):
    """One call (twice, on equal inputs) against the restatement over the whole allocation.  hist / valid: CPU tensors the reference
    reads; hist_dev / valid_dev: the device views handed to the op (default: plain copies)."""
    ops = _ops()
    dtype = buf.dtype
    sl = (slice(GUARD_ROWS, GUARD_ROWS + rows), slice(0, V))
    want = buf.clone()
    want[sl] = process(buf[sl], hist, valid, p, n, ban)
    if with_hf and dtype == F32 and rows <= 3:
        for r in range(rows):
            h = [] if hist is None else compact(hist[r].tolist(), None if valid is None else valid[r].tolist())
            if all(0 <= t < V for t in h):
                assert torch.equal(_bits(want[sl][r]), _bits(hf_chain(buf[sl][r], h, p, n, suppress=ban))), f"{what}: row {r} vs transformers"
    hist_dev = (None if hist is None else hist.to(DEV)) if hist_dev is None else hist_dev
    valid_dev = (None if valid is None else valid.to(DEV)) if valid_dev is None else valid_dev
    ban_dev = torch.tensor(list(ban), dtype=torch.int32, device=DEV) if len(ban) else None
    got = []
    for _ in range(2):
        dev = buf.to(DEV)
        logits = dev[sl]
        assert logits.stride() == (V + GUARD_COLS, 1)
        out = ops.process_logits(logits, hist_dev, valid_dev, None, p, n, ban_dev)
        assert out.data_ptr() == logits.data_ptr()
        got.append(_bits(dev.cpu()))
    assert torch.equal(got[0], got[1]), f"{what}: two runs differ"
    diff = got[0] != _bits(want)
    if diff.any():
        where = diff.nonzero()[:6].tolist()
        raise AssertionError(f"{what}: {int(diff.sum())} elements differ from the restatement, first (row, col) of the allocation: {where}; "
                             f"{int((diff[sl]).sum())} of them inside the logits")
    changed = int((_bits(want) != _bits(buf)).sum())
    return changed


# ------------------------------------------------------------------------------------------ history lengths across every boundary
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025, 8192])
def test_history_lengths(L, dtype):
    """rows = 3, V = 128, penalty 1.3, n = 3 (> L, = L + 1 and < L along the sweep), one ban; n_masked = L / 2 with gaps, row 1 all
    masked.  Wave (64), compaction chunk (1024) and per-thread loop (8 x 1024) boundaries."""
    rows, V = 3, 128
    g = torch.Generator().manual_seed(100 + L)
    buf = _embedded(rows, V, dtype, g)
    hist = _history(rows, L, V, g)
    valid = _valid(rows, L // 2, g, all_masked_row=1)
    changed = _run_and_check(buf, rows, V, hist, valid if L // 2 else None, 1.3, 3, (9,), f"L={L}")
    assert changed >= rows                                       # the ban at least


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,n,p,n_masked,n_ban", [(65, 2, 0.8, 0, 0), (257, 0, 1.3, 257, 1), (1025, 5, 1.3, 512, 64), (8192, 1, 1.0, 4096, 0),
                                                  (8192, 2, 0.8, 8192, 1), (40, 1, 0.8, 20, 0), (40, 5, 1.0, 0, 0), (4, 5, 1.3, 2, 0)])
def test_full_vocabulary(L, n, p, n_masked, n_ban, dtype):
    """rows = 3, V = 50272 (row stride 50296), tokens 0 and V - 1 in every history, n_masked in {0, L/2, L}, n_ban in {0, 1, 64}."""
    rows, V = 3, 50272
    g = torch.Generator().manual_seed(L + 10 * n + n_ban)
    buf = _embedded(rows, V, dtype, g)
    hist = _history(rows, L, V, g)
    if n >= 2 and L >= 10 + 2 * n:
        hist[:, L - (n - 1):] = hist[:, 10:10 + n - 1]           # the last n-1 tokens occurred before: a ban wherever both are valid
    valid = _valid(rows, n_masked, g, all_masked_row=2) if n_masked else None
    ban = tuple(torch.randperm(V, generator=g)[:n_ban].tolist())
    changed = _run_and_check(buf, rows, V, hist, valid, p, n, ban, f"V={V} L={L} n={n} p={p}")
    assert changed > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V,L,n,p,n_ban", [(128, 257, 2, 1.3, 1), (50272, 64, 3, 0.8, 64)])
def test_512_rows(V, L, n, p, n_ban, dtype):
    rows = 512
    g = torch.Generator().manual_seed(V + L)
    buf = _embedded(rows, V, dtype, g)
    hist = _history(rows, L, V, g)
    valid = _valid(rows, L // 2, g, all_masked_row=7)
    ban = tuple(torch.randperm(V, generator=g)[:n_ban].tolist())
    assert _run_and_check(buf, rows, V, hist, valid, p, n, ban, f"rows=512 V={V}") >= rows


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_row_short_histories_and_bans_alone(dtype):
    V = 128
    g = torch.Generator().manual_seed(5)
    for L, n, p, n_ban in [(0, 0, 1.0, 1), (0, 2, 1.3, 64), (1, 1, 1.3, 0), (2, 3, 0.8, 0), (2, 5, 1.0, 1), (3, 3, 1.0, 0), (1, 0, 0.8, 0)]:
        buf = _embedded(1, V, dtype, g)
        hist = torch.randint(7, 10, (1, L), generator=g)
        ban = tuple(torch.randperm(V, generator=g)[:n_ban].tolist())
        _run_and_check(buf, 1, V, hist, None, p, n, ban, f"rows=1 L={L} n={n} p={p} n_ban={n_ban}")
        _run_and_check(buf, 1, V, None if L == 0 else hist, None, p, n, ban, f"rows=1 L={L}, history None when empty")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R", [2, 3])
def test_strided_history_view(R, dtype):
    """history = ids[::R], mask = mask[::R]: the first step of num_return_sequences, R draws share one prefill row."""
    rows, V, L = 3, 128, 70
    g = torch.Generator().manual_seed(R)
    buf = _embedded(rows, V, dtype, g)
    full = _history(rows * R, L, V, g)
    vfull = _valid(rows * R, 30, g)
    hd, vd = full.to(DEV)[::R], vfull.to(DEV)[::R]
    assert hd.stride(0) == R * L and not hd.is_contiguous()
    _run_and_check(buf, rows, V, full[::R], vfull[::R], 1.3, 2, (), f"history[::{R}]", hist_dev=hd, valid_dev=vd)
    # a history that is the leading columns of a wider ids tensor, as every step of generate() passes it
    wide = torch.cat([full[:rows], torch.full((rows, 9), -7, dtype=torch.int64)], dim=1).to(DEV)
    _run_and_check(buf, rows, V, full[:rows], vfull[:rows], 0.8, 3, (4,), "ids[:, :L]", hist_dev=wide[:, :L], valid_dev=vfull[:rows].to(DEV))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [128, 50272])
def test_tokens_outside_the_vocabulary_are_never_an_address(V, dtype):
    rows, L = 3, 66
    g = torch.Generator().manual_seed(V + 1)
    buf = _embedded(rows, V, dtype, g)
    outside = torch.tensor([-1, V, V + GUARD_COLS - 1, -V, 1 << 40, -(1 << 62), (1 << 32) + 5, -(1 << 32) + 5])
    hist = outside[torch.randint(0, len(outside), (rows, L), generator=g)]
    for p, n in ((1.3, 1), (0.8, 2), (1.3, 3)):                  # nothing moves: the contract
        assert _run_and_check(buf, rows, V, hist, None, p, n, (), f"outside only, p={p} n={n}") == 0
    mixed = _history(rows, L, V, g)
    mixed[:, ::4] = hist[:, ::4]
    mixed[:, -1] = torch.tensor([-1, V, 8])[:rows]               # the prefix of rows 0 and 1 ends in such a token: no n-gram ban there
    for p, n in ((1.3, 1), (0.8, 2), (1.0, 3)):
        assert _run_and_check(buf, rows, V, mixed, _valid(rows, 20, g), p, n, (3,), f"mixed, p={p} n={n}") > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_minus_infinity_beats_the_penalty(dtype):
    V = 128
    buf = _embedded(1, V, dtype, torch.Generator().manual_seed(3))
    hist = torch.tensor([[30, 40, 50, 30]])                      # n = 2: 40 followed 30 before; 50 is seen and banned
    _run_and_check(buf, 1, V, hist, None, 2.0, 2, (50, 60), "seen and banned")
    dev = buf.to(DEV)
    x = _ops().process_logits(dev[GUARD_ROWS:GUARD_ROWS + 1, :V], hist.to(DEV), None, None, 2.0, 2, torch.tensor([50, 60], dtype=torch.int32, device=DEV))[0]
    orig = buf[GUARD_ROWS, :V].float()
    assert x[40] == float("-inf") and x[50] == float("-inf") and x[60] == float("-inf")
    want30 = (orig[30] * 2.0 if orig[30] < 0 else orig[30] / 2.0).to(dtype)
    assert x[30].cpu() == want30 and int(torch.isinf(x.float()).sum()) == 3


def test_everything_off_launches_nothing_and_bad_arguments_raise():
    ops = _ops()
    x = torch.randn(2, 128, device=DEV)
    keep = x.clone()
    h = torch.randint(0, 128, (2, 9), device=DEV)
    assert ops.process_logits(x, h) is x and ops.process_logits(x, None, repetition_penalty=1.3, no_repeat_ngram_size=2) is x
    assert ops.process_logits(x, h[:, :0], repetition_penalty=1.3) is x and torch.equal(x, keep)
    for bad in (dict(history=h.int()), dict(history=h[:1]), dict(history=h.t().contiguous().t()), dict(history=h, history_valid=h > 5, n_masked=10),
                dict(history=h, history_valid=(h > 5).long()), dict(history=h, n_masked=3), dict(history=h, ban=torch.zeros(2, device=DEV)),
                dict(history=h, ban=torch.zeros(65, dtype=torch.int32, device=DEV)), dict(history=h, repetition_penalty=0.0),
                dict(history=h, no_repeat_ngram_size=-1), dict(history=torch.zeros(2, 8193, dtype=torch.int64, device=DEV))):
        with pytest.raises(ValueError, match="process_logits"):
            ops.process_logits(x, **{"repetition_penalty": 1.3, **bad})
    with pytest.raises(ValueError, match="unit column stride"):
        ops.process_logits(x.t().contiguous().t(), h, repetition_penalty=1.3)
    assert torch.equal(x, keep)                                  # a refused call writes nothing
