"""-m gpu: the beam-search kernels (mmgl_attn_decode_beam_fwd in csrc/decode.hip; mmgl_beam_topk, mmgl_beam_advance in csrc/beam.hip).

Attention: against tests/beam_ref.attn_beam_ref, an fp64 reference that EXPANDS the cache (row (b, w) reads pre[b] ++
tail[b*W + src[b, w, j], j]), per sample at the bounds of tests/test_decode_edges_gpu.py: 1e-3 fp32 / 2e-2 bf16 of the sample's largest
reference magnitude.  KPI = 64 VEC / D keys per wave and load, 4 KPI per workgroup and load, 16 KPI per loop trip (VEC = 8 bf16, 4
fp32); prefix lengths straddle all three, n_tail in {0, 1, 5, 31}, src a permutation / one slot for everybody / a history that changes
slot at every step.  Before a case compares anything it asserts FROM THE REFERENCE ALONE that the result under the identity src, and the
result of reading the neighbouring sample's prefix, lie at least 10 tolerances away in every sample: the scores are spread (sigma 4: a few keys
hold the weight) and the tail keys carry a component along their reader's query, sized so that through the case's table a row's tail
holds exactly the softmax mass of its prefix -- under any other table, or with another prefix, the mass moves.
beam_topk: against torch in fp64 on the same logits (scores within 1e-5 max|score|, indices wherever the fp64 gap to the next candidate
exceeds twice that, on both sides of the position; an exact fp64 tie is decided by the tie rule and counts as clear).  beam_advance: against the plain-Python restatement tests/beam_ref.advance_ref, exactly."""
import numpy as np
import pytest
import torch

from beam_ref import BookRef, advance_ref, attn_beam_ref, topk_ref

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="fp32")]
TOL = {F32: 1e-3, BF16: 2e-2}
NAN = float("nan")
DEV = "cuda"
H, B = 2, 2


def _case(seed, W, D, S, n_tail, dtype, n_cap=None, pattern="perm", valid="ragged"):
    """Operands of one call (storage-rounded, on DEV).  The tail lives in a [B*W, n_cap, 2d] buffer as in the model."""
    g = torch.Generator().manual_seed(seed)
    d, R = H * D, B * W
    n_cap = max(n_tail, 1) if n_cap is None else n_cap
    rn = lambda *s: torch.randn(*s, generator=g)
    q = rn(R, d)
    kv_pre = rn(B, S, 2 * d)
    kv_pre[..., :d] *= 4.0 * D ** -0.5                                          # prefix scores ~ N(0, 16): a few keys hold the weight
    tail = rn(R, n_cap, 2 * d)
    tail[..., :d] *= 4.0 * D ** -0.5
    ok = torch.ones(B, S, dtype=torch.uint8)
    if valid == "ragged" and S > 2:
        ok[1, S - max(S // 5, 1):] = 0
    elif valid == "none":
        ok[0] = 0
    src = torch.zeros(R, n_cap, dtype=torch.int32)
    for b in range(B):
        if pattern == "perm":
            p = torch.roll(torch.arange(W), 1) if W > 1 else torch.zeros(1, dtype=torch.long)
            src[b * W:(b + 1) * W] = p[:, None].int()
        elif pattern == "one":
            src[b * W:(b + 1) * W] = W - 1
        elif pattern == "history":
            for j in range(n_cap):
                src[b * W:(b + 1) * W, j] = ((torch.arange(W) + 1 + (j + b) % max(W - 1, 1)) % W).int()      # never the identity
        else:
            src[b * W:(b + 1) * W] = torch.arange(W)[:, None].int()
    # a component along the READER's query lifts the tail keys a row reads through src to exactly the softmax mass of its prefix:
    # under the identity table (or with another prefix) the mass moves, so a wrong row or a wrong prefix shows in the result
    if n_tail:
        qh = q.double().reshape(R, H, D)
        s_pre = torch.einsum("rhd,rshd->rhs", qh, kv_pre[..., :d].double().reshape(B, S, H, D).repeat_interleave(W, 0))
        s_pre = s_pre.masked_fill(~ok.bool().repeat_interleave(W, 0)[:, None, :], float("-inf"))
        rows = (torch.arange(R) // W * W)[:, None] + src[:, :n_tail].long()
        cols = torch.arange(n_tail)[None, :].expand(R, -1)
        s_tail = torch.einsum("rhd,rjhd->rhj", qh, tail[..., :d].double()[rows, cols].reshape(R, n_tail, H, D))
        lift = torch.logsumexp(s_pre, -1) - torch.logsumexp(s_tail, -1)                           # [R, H]
        lift = torch.where(torch.isfinite(lift), lift, torch.zeros_like(lift))
        along = (qh * (lift / qh.pow(2).sum(-1))[..., None]).reshape(R, d).float()
        seen = set()
        for r in range(R):
            for j in range(n_tail):
                if (int(rows[r, j]), j) not in seen:                                               # the first reader of a key sizes it
                    seen.add((int(rows[r, j]), j))
                    tail[rows[r, j], j, :d] += along[r]
    to = lambda t: t.to(dtype).to(DEV)
    return dict(q=to(q), kv_pre=to(kv_pre), tail=to(tail), ok=ok.to(DEV), src=src.to(DEV), W=W, D=D, S=S, n_tail=n_tail, d=d)


def _ref(c, src=None, swap_prefix=False):
    d, n = c["d"], c["n_tail"]
    kv = c["kv_pre"].flip(0) if swap_prefix else c["kv_pre"]
    ok = c["ok"].flip(0) if swap_prefix else c["ok"]
    return attn_beam_ref(c["q"], kv[..., :d], kv[..., d:], ok, H, c["W"], c["tail"][:, :n, :d] if n else None,
                         c["tail"][:, :n, d:] if n else None, c["src"] if src is None else src)


def _run(c, out=None):
    from mmgl_amd import ops
    d, n = c["d"], c["n_tail"]
    return ops.attn_decode_beam(c["q"], c["kv_pre"][..., :d], c["kv_pre"][..., d:], c["ok"], H, c["W"],
                                c["tail"][:, :n, :d] if n else None, c["tail"][:, :n, d:] if n else None, c["src"] if n else None, out=out)


def _per_sample(a, b, W):
    """max|a - b| / max|b| per sample (its W rows)."""
    a, b = a.double().reshape(B, -1), b.double().reshape(B, -1)
    return (a - b).abs().amax(1) / b.abs().amax(1)


def _sensitive(c, dtype, what):
    """From the reference alone: the identity table and the neighbouring sample's prefix give results >= 10 tolerances away."""
    want = _ref(c)
    far = _per_sample(_ref(c, swap_prefix=True), want, c["W"])
    assert (far >= 10 * TOL[dtype]).all(), f"{what}: the other sample's prefix moves the result by only {far.tolist()}"
    if c["n_tail"] and c["W"] > 1:
        ident = (torch.arange(B * c["W"], device=c["src"].device) % c["W"]).int()[:, None].expand_as(c["src"]).contiguous()
        far = _per_sample(_ref(c, src=ident), want, c["W"])
        assert (far >= 10 * TOL[dtype]).all(), f"{what}: the identity table moves the result by only {far.tolist()}"
    return want


def _lengths(D, dtype):
    kpi = 64 * (8 if dtype == BF16 else 4) // D
    return [kpi - 1, kpi + 1, 4 * kpi + 1, 16 * kpi - 1, 16 * kpi + 3]


def _grid(W, D, dtype):
    """(S, n_tail, pattern) of one (W, D, dtype): every length with every tail, the three tables dealt over them."""
    pats = ["perm", "one", "history"]
    cases, i = [], 0
    for S in _lengths(D, dtype):
        for n_tail in (0, 1, 5, 31):
            for pat in (pats if (n_tail == 31 and S == _lengths(D, dtype)[2]) else [pats[i % 3]]):
                cases.append((S, n_tail, pat))
            i += 1
    return cases


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [16, 64, 128])
@pytest.mark.parametrize("W", [1, 2, 3, 4, 8])
def test_attention_against_the_expanded_cache(W, D, dtype):
    worst = 0.0
    for i, (S, n_tail, pat) in enumerate(_grid(W, D, dtype)):
        what = f"W={W} D={D} S={S} n_tail={n_tail} {pat}"
        c = _case(1000 * W + D + i, W, D, S, n_tail, dtype, n_cap=max(n_tail, 1) + 3, pattern=pat)
        want = _sensitive(c, dtype, what)
        got = _run(c)
        assert torch.isfinite(got.float()).all(), what
        err = _per_sample(got, want, W)
        worst = max(worst, float(err.max()))
        assert (err <= TOL[dtype]).all(), f"{what}: per-sample err {err.tolist()} > {TOL[dtype]}"
    print(f"W={W} D={D} {dtype}: worst per-sample err {worst:.3e}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_valid_key_at_each_position_of_a_trip(dtype):
    """One valid prefix key per sample and no tail: the output of every beam row is that key's value row, bitwise."""
    W, D = 4, 64
    trip = 16 * 64 * (8 if dtype == BF16 else 4) // D
    S = trip + 5
    c = _case(7, W, D, S, 0, dtype, valid="all")
    d = c["d"]
    for pos in list(range(0, trip, max(trip // 32, 1))) + [trip - 1, trip, S - 1]:
        c["ok"].zero_()
        c["ok"][0, pos] = 1
        c["ok"][1, S - 1 - pos] = 1
        got = _run(c)
        for b, p in ((0, pos), (1, S - 1 - pos)):
            assert torch.equal(got[b * W:(b + 1) * W], c["kv_pre"][b, p, d:].expand(W, d)), (pos, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_tail", [0, 5])
def test_fully_masked_prefix_is_uniform_over_all_keys(n_tail, dtype):
    """include/mmgl_hip.h: a sample whose prefix has no valid key weighs all its S_pre + n_tail keys equally (n_tail = 0: the uniform
    distribution of mmgl_attn_decode_fwd); the other sample is unaffected.  The fp64 reference implements exactly that."""
    W, D, S = 4, 64, 37
    c = _case(11, W, D, S, n_tail, dtype, pattern="history", valid="none")
    d = c["d"]
    want = _ref(c)
    vals = c["kv_pre"][0, :, d:].double().sum(0, keepdim=True).expand(W, d).clone()
    for w in range(W):
        for j in range(n_tail):
            vals[w] += c["tail"][int(c["src"][w, j]), j, d:].double()
    assert torch.allclose(want[:W], vals / (S + n_tail), rtol=1e-12, atol=1e-12)              # the reference is the stated rule
    got = _run(c)
    err = _per_sample(got, want, W)
    assert (err <= TOL[dtype]).all(), err.tolist()


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_outside_the_views_and_inputs_untouched(dtype):
    """Prefix rows past S_pre, tail columns past n_tail, q pad columns and the rows around q / out hold NaN: bitwise the dense call."""
    from mmgl_amd import ops
    W, D, S, n_tail, n_cap = 3, 64, 70, 5, 9
    c = _case(13, W, D, S, n_tail, dtype, n_cap=n_cap, pattern="history")
    d, R = c["d"], B * W
    dense = _run(c)
    big_pre = torch.full((B, S + 4, 2 * d), NAN, dtype=dtype, device=DEV)
    big_pre[:, :S] = c["kv_pre"]
    big_tail = c["tail"].clone()
    big_tail[:, n_tail:] = NAN
    big_q = torch.full((R + 2, d + 16), NAN, dtype=dtype, device=DEV)
    big_q[1:R + 1, :d] = c["q"]
    big_out = torch.full((R + 2, d), NAN, dtype=dtype, device=DEV)
    big_ok = torch.ones(B, S + 4, dtype=torch.uint8, device=DEV)
    big_ok[:, :S] = c["ok"]
    src = c["src"].clone()
    src[:, n_tail:] = 7 * W                                                      # columns the call must not read
    snap = [t.clone() for t in (big_pre, big_tail, big_q, big_ok, src)]
    got = ops.attn_decode_beam(big_q[1:R + 1, :d], big_pre[:, :S, :d], big_pre[:, :S, d:], big_ok[:, :S], H, W, big_tail[:, :n_tail, :d],
                               big_tail[:, :n_tail, d:], src, out=big_out[1:R + 1])
    assert torch.equal(got, dense)
    assert torch.isnan(big_out[0]).all() and torch.isnan(big_out[R + 1]).all()
    for t, s in zip((big_pre, big_tail, big_q, big_ok, src), snap):
        assert torch.equal(t.view(torch.uint8), s.view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_leave_out_untouched_and_runs_are_bitwise_equal(dtype):
    from mmgl_amd import ops
    c = _case(17, 8, 64, 131, 31, dtype, pattern="history")
    a, b2 = _run(c), _run(c)
    assert torch.equal(a, b2)
    # W = 9
    d = c["d"]
    q9 = torch.randn(B * 9, d, device=DEV).to(dtype)
    out = torch.full((B * 9, d), 3.0, dtype=dtype, device=DEV)
    with pytest.raises(ValueError, match="beams"):
        ops.attn_decode_beam(q9, c["kv_pre"][..., :d], c["kv_pre"][..., d:], c["ok"], H, 9, out=out)
    assert (out == 3.0).all()
    # D = 48
    q48 = torch.randn(B * 2, 96, device=DEV).to(dtype)
    kv48 = torch.randn(B, 20, 192, device=DEV).to(dtype)
    out = torch.full((B * 2, 96), 3.0, dtype=dtype, device=DEV)
    with pytest.raises(ValueError, match="head_dim"):
        ops.attn_decode_beam(q48, kv48[..., :96], kv48[..., 96:], torch.ones(B, 20, dtype=torch.uint8, device=DEV), 2, 2, out=out)
    assert (out == 3.0).all()
    with pytest.raises(ValueError, match="src"):
        ops.attn_decode_beam(c["q"], c["kv_pre"][..., :d], c["kv_pre"][..., d:], c["ok"], H, 8, c["tail"][:, :31, :d], c["tail"][:, :31, d:],
                             c["src"].long())


# ------------------------------------------------------------------------------------------ beam_topk
def _logits(seed, rows, V, dtype, ld=None):
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((rows, ld or V), NAN, dtype=dtype, device=DEV)
    buf[:, :V] = (torch.randn(rows, V, generator=g) * 3.0).to(dtype).to(DEV)
    return buf[:, :V]


def _check_topk(logits, score, W, rows_in, what):
    from mmgl_amd import ops
    K = 2 * W
    cs, ci = ops.beam_topk(logits, score, W, rows_in=rows_in)
    cs2, ci2 = ops.beam_topk(logits, score, W, rows_in=rows_in)
    assert torch.equal(cs, cs2) and torch.equal(ci, ci2), f"{what}: two runs differ"
    ref = topk_ref(logits, score, W, rows_in)                                   # fp64 [B, rows_in * V]
    top = torch.sort(ref, dim=1, descending=True, stable=True)                  # an exact tie: the lower flat index first
    tv, ti = top.values[:, :K + 1], top.indices[:, :K + 1]
    tol = 1e-5 * float(tv.abs().max())                                          # of the candidates' own scores, not of the row's tail
    gap = tv[:, :K] - tv[:, 1:]
    sure = (gap > 2 * tol) | (gap == 0)                                         # decided by the scores, or by the tie rule
    clear = sure & torch.cat([torch.ones_like(sure[:, :1]), sure[:, :-1]], 1)   # on both sides of the position
    share = 1.0 - clear.double().mean().item()
    assert share <= 0.02, f"{what}: {share:.3f} of the positions are near-ties of the reference itself"
    assert (cs[:, :-1] >= cs[:, 1:]).all(), f"{what}: not sorted"
    assert ci.min() >= 0 and ci.max() < ref.shape[1]
    own = ref.gather(1, ci.long())                                              # the reference's score of the product's index
    err = (cs.double() - own).abs().max().item()
    assert err <= tol, f"{what}: score err {err:.3e} > {tol:.3e}"
    assert ((cs.double() - tv[:, :K]).abs() <= tol).all(), f"{what}: rank-by-rank scores"
    wrong = (ci.long() != ti[:, :K]) & clear
    assert not wrong.any(), f"{what}: {int(wrong.sum())} indices differ at a clear gap"
    return cs, ci


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("W", [1, 2, 4, 8])
@pytest.mark.parametrize("V", [128, 1003])
def test_topk_against_fp64(V, W, dtype):
    Bs = 32
    for rows_in in sorted({1, W}):
        rows = Bs * rows_in
        g = torch.Generator().manual_seed(V + W)
        score = (-torch.rand(rows, generator=g) * 5.0).to(DEV)
        _check_topk(_logits(V * 10 + W + rows_in, rows, V, dtype, ld=V + 5), score, W, rows_in, f"V={V} W={W} rows_in={rows_in}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_topk_full_vocabulary(dtype):
    """V = 50272: 13 chunks of 4096 with a ragged last one; W = 4 rows per sample, and the single-row first step."""
    W, Bs, V = 4, 8, 50272
    for rows_in in (W, 1):
        rows = Bs * rows_in
        score = (-torch.arange(rows, dtype=torch.float32) * 0.37).to(DEV)
        _check_topk(_logits(5 + rows_in, rows, V, dtype), score, W, rows_in, f"V={V} rows_in={rows_in}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_topk_exact_ties_go_to_the_lower_flat_index(dtype):
    from mmgl_amd import ops
    W, V = 4, 1003
    # duplicated values inside a row: the row's maximum sits at four columns, two of them in different 256-lanes of the chunk
    x = _logits(3, W, V, dtype).clone()
    x[:, :] = x[0]                                                               # identical rows ...
    top = float(x[0].float().max()) + 1.0
    for col in (900, 17, 513, 18):
        x[:, col] = top
    score = torch.zeros(W, device=DEV)                                           # ... with equal beam scores
    cs, ci = ops.beam_topk(x, score, W, rows_in=W)
    want = [r * V + col for r in range(2) for col in (17, 18, 513, 900)]         # 2W = 8: rows 0 and 1, columns ascending
    assert ci[0].tolist() == want, ci[0].tolist()
    assert (cs[0] == cs[0, 0]).all()
    # a better beam score moves its row in front, the tie rule holds inside it
    score[2] = 0.5
    cs, ci = ops.beam_topk(x, score, W, rows_in=W)
    assert ci[0].tolist() == [2 * V + col for col in (17, 18, 513, 900)] + [col for col in (17, 18, 513, 900)], ci[0].tolist()
    # rows_in = 1 and a full vocabulary: ties across chunks
    y = _logits(4, 1, 50272, dtype).clone()
    top = float(y.float().max()) + 1.0
    for col in (50271, 4096, 4095, 0, 30000, 8191, 12288, 45056):
        y[0, col] = top
    cs, ci = ops.beam_topk(y, torch.zeros(1, device=DEV), W, rows_in=1)
    assert ci[0].tolist() == sorted((50271, 4096, 4095, 0, 30000, 8191, 12288, 45056)), ci[0].tolist()


def test_topk_refusals():
    from mmgl_amd import ops
    x = torch.randn(4, 64, device=DEV)
    with pytest.raises(ValueError, match="beams"):
        ops.beam_topk(x, torch.zeros(4, device=DEV), 9)
    with pytest.raises(ValueError, match="2W"):
        ops.beam_topk(x[:, :6], torch.zeros(4, device=DEV), 4)
    with pytest.raises(ValueError, match="rows_in"):
        ops.beam_topk(x, torch.zeros(4, device=DEV), 4, rows_in=2)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        ops.beam_topk(x.half(), torch.zeros(4, device=DEV), 4)


# ------------------------------------------------------------------------------------------ beam_advance
def _book_equal(book, ref, what):
    W, Bn = ref.W, ref.B
    assert book.tokens.view(Bn, W).tolist() == ref.tokens, what
    assert book.parents.view(Bn, W).tolist() == ref.parents, what
    assert book.beam_score.view(Bn, W).cpu().numpy().tolist() == [[float(s) for s in row] for row in ref.scores], what
    assert book.src.view(Bn, W, -1).tolist() == ref.src, what
    score, length, anc, tok = (t.view(Bn, W, *t.shape[1:]).cpu() for t in book.pool)
    for b in range(Bn):
        for i in range(W):
            if i < len(ref.pool[b]):
                e = ref.pool[b][i]
                assert float(score[b, i]) == float(e["score"]) and int(length[b, i]) == e["len"] and int(tok[b, i]) == e["tok"], (what, b, i)
                assert anc[b, i, :len(e["anc"])].tolist() == e["anc"], (what, b, i)
            else:
                assert int(length[b, i]) == 0 and float(score[b, i]) == float("-inf"), (what, b, i)
    assert [bool(x) for x in book.done.tolist()] == ref.done, what


@pytest.mark.parametrize("early_stopping", [False, True])
@pytest.mark.parametrize("length_penalty", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("W", [1, 2, 4, 8])
def test_advance_against_the_python_restatement(W, length_penalty, early_stopping):
    """Hand-built sorted candidate lists over 6 steps and 5 samples: sample 0 never meets EOS; 1 has EOS inside the first W at
    steps 1 and 3; 2 has EOS only outside the first W; 3 has all of its first W on EOS at step 2 (and again later, so its pool
    fills and it freezes); 4 meets EOS from step 0 on with rising scores (a pool that keeps being displaced, then the heuristic)."""
    from mmgl_amd import ops
    Bn, V, EOS, n_new = 5, 50, 7, 6
    K = 2 * W
    book, ref = ops.BeamBook(Bn, W, n_new - 1, DEV), BookRef(Bn, W, n_new - 1)
    g = np.random.default_rng(W * 10 + int(length_penalty))
    for s in range(n_new):
        rows_in = 1 if s == 0 else W
        cs = np.zeros((Bn, K), np.float32)
        ci = np.zeros((Bn, K), np.int64)
        for b in range(Bn):
            base = -1.5 * (s + 1) + (0.9 * s if b == 4 else 0.0)
            cs[b] = np.sort((base - g.random(K) * 2.0).astype(np.float32))[::-1]
            toks = g.permutation(np.array([t for t in range(V) if t != EOS]))[:K]
            par = g.integers(0, rows_in, K)
            where = []
            if b == 1 and s in (1, 3):
                where = [W // 2]
            if b == 2:
                where = [K - 1] if W > 1 or s % 2 else []
                where = [w_ for w_ in where if w_ >= W]
            if b == 3 and s >= 2:
                where = list(range(W))
            if b == 4:
                where = [0] if rows_in == 1 else list(range(0, W, 2))
            used = set()
            for r in where:                                                   # an EOS candidate per distinct parent only
                if rows_in == 1 and used:
                    break
                p = next(p for p in range(rows_in) if p not in used)
                used.add(p)
                toks[r], par[r] = EOS, p
            ci[b] = par * V + toks
        last = s == n_new - 1
        div = float(s + 1) ** length_penalty
        ops.beam_advance(torch.from_numpy(cs).to(DEV), torch.from_numpy(ci).int().to(DEV), book, s, V, EOS, last, early_stopping, div)
        advance_ref(ref, cs, ci, s, V, EOS, last, early_stopping, div)
        _book_equal(book, ref, f"W={W} step {s}")
    assert all(len(p) >= 1 for p in ref.pool)
    if W > 1:
        assert any(ref.done) and not all(ref.done), ref.done                   # a frozen sample and a live one
        assert any(row != list(range(W)) for b in range(Bn) for row in [[ref.src[b][w][0] for w in range(W)]])
