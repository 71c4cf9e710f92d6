"""-m gpu: mmgl_sample_tokens (csrc/sample.hip) through ops.sample_tokens, against the fp64 restatement of its contract in
tests/sample_ref.py (itself held against transformers' warpers by tests/test_sample_cpu.py).

Kept set: the kernel's `kept` lies between #{above < top_p - eps_p} and #{above < top_p + eps_p}, is a whole number of tie groups, and
is exactly #{x >= k-th} when only top-k filters.  eps_p = sample_ref.eps_p(V) is derived from the kernel's arithmetic (DESIGN.md 4.13:
integer masses, so only the subtraction, expf and the truncation err), 1.9e-6 at V = 50272; it is not tuned to the result.
Draw: the reference rebuilds the set from `kept` (the top-`kept` by logit); the token is in it and C_{v-1}/Z - eps <= u < C_v/Z + eps
for the fp64 index-order CDF, eps = eps_p + 2^-30 (the kernel's floor(u 2^32)).
Measured on one MI355X over every case of this file: the kept count equalled the fp64 count in every row, and the largest distance of
u outside its fp64 interval was 0 (DESIGN.md 4.13 keeps the figures)."""
import numpy as np
import pytest
import torch

from sample_ref import cdf, draw_ok, eos_ref, eps_p, eps_u, kept_bounds, scaled, top_set, warp_row

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="fp32")]
DEV = "cuda"
SETTINGS = [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.0, 0, 0.9), (0.8, 50, 0.95), (1.3, 8, 0.5)]
WORST = dict(kept_off=0, draw_out=0.0)          # measured over the session, printed by every case


def _ops():
    from mmgl_amd import ops
    return ops


def _logits(seed, rows, V, sigma, dtype):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, V, generator=g) * sigma).to(dtype)


def _u(seed, rows, n_draws):
    g = torch.Generator().manual_seed(seed + 7)
    return torch.rand(rows, n_draws, generator=g)


def _check(logits, u, T, k, p, tok, kept):
    """Every row of one call against the restatement; logits / u on the CPU, tok [rows * n_draws] and kept [rows] as lists."""
    rows, V = logits.shape
    n_draws = u.shape[1]
    x = scaled(logits, T)
    ep, eu = eps_p(V), eps_u(V)
    for r in range(rows):
        surv, above, exact = warp_row(x[r], k, p)
        n = kept[r]
        if p < 1.0:
            lo, hi = kept_bounds(surv, above, p, ep)
            assert lo <= n <= hi, f"row {r}: kept {n} outside [{lo}, {hi}] (fp64 count {int(exact.sum())})"
        else:
            assert n == int(surv.sum()), f"row {r}: kept {n}, the top-k survivors are {int(surv.sum())}"
        WORST["kept_off"] = max(WORST["kept_off"], abs(n - int(exact.sum())))
        mask, whole = top_set(x[r], n)
        assert whole, f"row {r}: kept {n} splits a group of tied logits"
        c = cdf(x[r], mask)
        for j in range(n_draws):
            t, uu = tok[r * n_draws + j], float(u[r, j])
            assert 0 <= t < V and draw_ok(c, mask, uu, t, eu), f"row {r} draw {j}: token {t} for u = {uu}"
            WORST["draw_out"] = max(WORST["draw_out"], (c[t - 1] if t else 0.0) - uu, uu - c[t] if uu >= c[t] else 0.0)


def _run(logits, u, T, k, p):
    ops = _ops()
    tok, kept = ops.sample_tokens(logits.to(DEV), u.to(DEV), T, k, p, return_kept=True)
    tok2, kept2 = ops.sample_tokens(logits.to(DEV), u.to(DEV), T, k, p, return_kept=True)
    assert torch.equal(tok, tok2) and torch.equal(kept, kept2), "two runs differ"
    return tok.tolist(), kept.tolist()


@pytest.mark.parametrize("sigma", [1.0, 3.0])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_draws", [1, 8])
@pytest.mark.parametrize("rows", [1, 3, 64])
@pytest.mark.parametrize("V", [128, 1003, 4097])
def test_kept_set_and_draw(V, rows, n_draws, dtype, sigma):
    logits = _logits(V + rows, rows, V, sigma, dtype)
    u = _u(V + rows + n_draws, rows, n_draws)
    for T, k, p in SETTINGS:
        tok, kept = _run(logits, u, T, k, p)
        _check(logits, u, T, k, p, tok, kept)
    print(f"measured so far: kept count off the fp64 count by at most {WORST['kept_off']}, u outside its fp64 interval by at most "
          f"{WORST['draw_out']:.3e} (eps_p = {eps_p(V):.3e})")


@pytest.mark.parametrize("dtype", DTYPES)
def test_full_vocabulary_once(dtype):
    V, rows = 50272, 2
    logits = _logits(5, rows, V, 1.0, dtype)
    u = _u(6, rows, 8)
    for T, k, p in SETTINGS:
        tok, kept = _run(logits, u, T, k, p)
        _check(logits, u, T, k, p, tok, kept)
    print(f"V = {V}: kept off by at most {WORST['kept_off']}, u outside by at most {WORST['draw_out']:.3e} (eps_p = {eps_p(V):.3e})")


def test_forced_ties_are_all_in():
    """bf16 logits on a grid of 0.25: ties at the k-th value and at the top-p boundary.  The reference says, before the kernel runs,
    that the boundary group has several members and that the bounds leave one admissible count."""
    V, rows = 1003, 3
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(rows, V, generator=g) * 1.5 * 4).round().div(4).to(BF16)
    x = scaled(logits, 1.0)
    u = _u(12, rows, 8)
    k = 50
    for r in range(rows):
        kth = np.sort(x[r])[V - k]
        assert (x[r] == kth).sum() > 1 and (x[r] >= kth).sum() > k, "no tie at the k-th value: the case shows nothing"
    tok, kept = _run(logits, u, 1.0, k, 1.0)
    assert kept == [int((x[r] >= np.sort(x[r])[V - k]).sum()) for r in range(rows)]
    _check(logits, u, 1.0, k, 1.0, tok, kept)
    p = 0.6
    for r in range(rows):
        surv, above, exact = warp_row(x[r], 0, p)
        edge = x[r][exact].min()
        assert (x[r] == edge).sum() > 1, "no tie at the top-p boundary: the case shows nothing"
        lo, hi = kept_bounds(surv, above, p, eps_p(V))
        assert lo == hi == int(exact.sum()), "the boundary is too close to a group's edge for an exact statement"
    tok, kept = _run(logits, u, 1.0, 0, p)
    assert kept == [int(warp_row(x[r], 0, p)[2].sum()) for r in range(rows)]
    _check(logits, u, 1.0, 0, p, tok, kept)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [128, 1003])
def test_coverage_every_kept_token_is_reachable(V, dtype):
    """u at the midpoint of a kept token's fp64 interval returns that token (intervals wider than 4 eps); a grid of 4096 u values
    never leaves the set."""
    ops = _ops()
    T, k, p = 0.8, 50, 0.95
    row = _logits(V, 1, V, 1.0, dtype)
    x = scaled(row, T)[0]
    _, kept1 = ops.sample_tokens(row.to(DEV), torch.zeros(1, 1, device=DEV), T, k, p, return_kept=True)
    mask, whole = top_set(x, int(kept1[0]))
    assert whole
    c = cdf(x, mask)
    lo = np.concatenate([[0.0], c[:-1]])
    want = [v for v in range(V) if mask[v] and c[v] - lo[v] > 4 * eps_u(V)]
    assert len(want) >= min(int(mask.sum()), 20) // 2, "too few wide intervals: the case shows nothing"
    mid = np.array([(lo[v] + c[v]) / 2 for v in want] + [0.5] * (-len(want) % 8), dtype=np.float32).reshape(-1, 8)
    tok = ops.sample_tokens(row.expand(mid.shape[0], V).contiguous().to(DEV), torch.from_numpy(mid).to(DEV), T, k, p).tolist()
    assert tok[:len(want)] == want
    grid = ((torch.arange(4096, dtype=torch.float64) + 0.5) / 4096).float().reshape(512, 8)
    tok = ops.sample_tokens(row.expand(512, V).contiguous().to(DEV), grid.to(DEV), T, k, p).tolist()
    assert all(mask[t] for t in tok)
    assert all(draw_ok(c, mask, float(uu), t, eps_u(V)) for uu, t in zip(grid.reshape(-1), tok))
    assert tok == sorted(tok), "a larger u returned an earlier token"


@pytest.mark.parametrize("dtype", DTYPES)
def test_edges(dtype):
    ops = _ops()
    V, rows = 1003, 3
    logits = _logits(21, rows, V, 1.0, dtype)
    x = scaled(logits, 1.0)
    dl = logits.to(DEV)
    top = np.sort(x, axis=1)
    assert (top[:, -1] > top[:, -2]).all(), "a tie at the maximum: the arg-max statements below would not hold"
    amax = x.argmax(axis=1).tolist()
    one = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    u = torch.tensor([[0.0, one, 0.3, 0.999, 0.5, 0.25, 0.75, 0.125]] * rows)
    # u = 0: the first kept token; u just below 1: a kept token
    for T, k, p in SETTINGS:
        tok, kept = ops.sample_tokens(dl, u.to(DEV), T, k, p, return_kept=True)
        tok = tok.view(rows, 8).tolist()
        xs = scaled(logits, T)
        for r in range(rows):
            mask, _ = top_set(xs[r], int(kept[r]))
            assert tok[r][0] == int(np.flatnonzero(mask)[0]) and mask[tok[r][1]]
    # top_k = 1 and a top_p that admits one token: the arg-max for every u, kept = 1
    for kw in (dict(top_k=1), dict(top_p=1e-6), dict(top_k=1, top_p=0.5, temperature=0.5)):
        tok, kept = ops.sample_tokens(dl, u.to(DEV), return_kept=True, **kw)
        assert kept.tolist() == [1] * rows and tok.view(rows, 8).tolist() == [[a] * 8 for a in amax], kw
    # filters that are off equal the unfiltered call bitwise
    base, kept = ops.sample_tokens(dl, u.to(DEV), 0.9, return_kept=True)
    assert kept.tolist() == [V] * rows
    for kw in (dict(top_k=V), dict(top_k=V + 5), dict(top_k=0, top_p=1.0), dict(top_k=V, top_p=1.0)):
        tok, kept = ops.sample_tokens(dl, u.to(DEV), 0.9, return_kept=True, **kw)
        assert torch.equal(tok, base) and kept.tolist() == [V] * rows, kw
    # V equal logits: all kept, the draw is floor(u V) within one
    flat = torch.full((1, V), 0.5, dtype=dtype, device=DEV)
    for kw in (dict(), dict(top_k=7), dict(top_p=0.3), dict(top_k=7, top_p=0.3)):
        tok, kept = ops.sample_tokens(flat, u[:1].to(DEV), return_kept=True, **kw)
        assert kept.tolist() == [V], kw
        assert all(abs(t - int(float(uu) * V)) <= 1 and 0 <= t < V for t, uu in zip(tok.tolist(), u[0])), kw
    # NaN logits count as -inf: the same tokens as with -inf in their place, never outside [0, V); an all-NaN row is uniform
    bad = logits.clone()
    bad[:, ::7] = float("nan")
    ninf = logits.clone()
    ninf[:, ::7] = float("-inf")
    for T, k, p in SETTINGS:
        a, ka = ops.sample_tokens(bad.to(DEV), u.to(DEV), T, k, p, return_kept=True)
        b, kb = ops.sample_tokens(ninf.to(DEV), u.to(DEV), T, k, p, return_kept=True)
        assert torch.equal(a, b) and torch.equal(ka, kb) and int(a.min()) >= 0 and int(a.max()) < V
        assert not bool((a % 7 == 0).any())
    tok = ops.sample_tokens(torch.full((1, V), float("nan"), dtype=dtype, device=DEV), u[:1].to(DEV))
    assert all(abs(t - int(float(uu) * V)) <= 1 and 0 <= t < V for t, uu in zip(tok.tolist(), u[0]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_addressing(dtype):
    ops = _ops()
    V, rows, n_draws = 4097, 3, 8
    logits = _logits(31, rows, V, 1.0, dtype)
    u = _u(32, rows, n_draws).to(DEV)
    T, k, p = 0.8, 50, 0.95
    want, kept = ops.sample_tokens(logits.to(DEV), u, T, k, p, return_kept=True)
    # a strided, misaligned window of a NaN-filled buffer
    buf = torch.full((rows + 2, V + 37), float("nan"), dtype=dtype, device=DEV)
    buf[1:1 + rows, 5:5 + V] = logits.to(DEV)
    win = buf[1:1 + rows, 5:5 + V]
    assert win.stride() == (V + 37, 1) and not win.is_contiguous()
    got, kept2 = ops.sample_tokens(win, u, T, k, p, return_kept=True)
    assert torch.equal(got, want) and torch.equal(kept, kept2)
    # tokens into a column of a wider int64 tensor: the other columns stay as they were
    ids = torch.arange(rows * n_draws * 5, dtype=torch.int64, device=DEV).view(rows * n_draws, 5) - 1000
    before = ids.clone()
    ret = ops.sample_tokens(win, u, T, k, p, out=ids[:, 3])
    assert ret.data_ptr() == ids[:, 3].data_ptr() and torch.equal(ids[:, 3], want)
    keep = [0, 1, 2, 4]
    assert torch.equal(ids[:, keep], before[:, keep])
    # finished / eos / pad, as the greedy loops keep them
    toks = want.tolist()
    eos, pad = toks[2], 1
    fin0 = [0] * len(toks)
    fin0[4] = fin0[9] = 1
    fin = torch.tensor(fin0, dtype=torch.uint8, device=DEV)
    got = ops.sample_tokens(win, u, T, k, p, finished=fin, eos_token_id=eos, pad_token_id=pad)
    ref_tok, ref_fin = eos_ref(toks, fin0, eos, pad)
    assert got.tolist() == ref_tok and fin.tolist() == ref_fin and ref_fin[2] == 1 and sum(ref_fin) >= 3
    finb = torch.tensor(fin0, dtype=torch.bool, device=DEV)                  # a bool buffer is updated in place as well
    got = ops.sample_tokens(win, u, T, k, p, finished=finb, eos_token_id=eos, pad_token_id=pad)
    assert got.tolist() == ref_tok and finb.to(torch.uint8).tolist() == ref_fin
    fin = torch.tensor(fin0, dtype=torch.uint8, device=DEV)                  # no eos: finished draws are padded, nobody finishes
    got = ops.sample_tokens(win, u, T, k, p, finished=fin, pad_token_id=pad)
    assert got.tolist() == eos_ref(toks, fin0, None, pad)[0] and fin.tolist() == fin0


def test_refused_calls_leave_out_untouched():
    ops = _ops()
    V = 128
    logits = torch.randn(2, V, device=DEV)
    u = torch.rand(2, 1, device=DEV)
    out = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    fin = torch.zeros(2, dtype=torch.uint8, device=DEV)
    calls = [
        lambda: ops.sample_tokens(torch.zeros(1, 131073, device=DEV), u[:1], out=out[:1]),
        lambda: ops.sample_tokens(logits, u, temperature=0.0, out=out),
        lambda: ops.sample_tokens(logits, u, temperature=float("nan"), out=out),
        lambda: ops.sample_tokens(logits, u, top_p=0.0, out=out),
        lambda: ops.sample_tokens(logits, u, top_p=1.5, out=out),
        lambda: ops.sample_tokens(logits, u, top_k=-1, out=out),
        lambda: ops.sample_tokens(logits.half(), u, out=out),
        lambda: ops.sample_tokens(logits, u.double(), out=out),
        lambda: ops.sample_tokens(logits, torch.rand(2, 9, device=DEV)),
        lambda: ops.sample_tokens(logits, torch.rand(3, 1, device=DEV), out=out),
        lambda: ops.sample_tokens(logits.t(), u, out=out),
        lambda: ops.sample_tokens(logits, u, out=out.int()),
        lambda: ops.sample_tokens(logits, u, out=torch.zeros(3, dtype=torch.int64, device=DEV)),
        lambda: ops.sample_tokens(logits, u, eos_token_id=5, out=out),
        lambda: ops.sample_tokens(logits, u, finished=fin, eos_token_id=5, out=out),
        lambda: ops.sample_tokens(logits, u, finished=fin[:1], eos_token_id=5, pad_token_id=1, out=out),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert out.tolist() == [-7, -7] and fin.tolist() == [0, 0], f"refused call {i} wrote its outputs"
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sample_tokens(logits.cpu(), u.cpu())
