"""-m gpu: the streaming entry points of csrc/elementwise.hip that stood on max-norm or small-shape parity tests, element by element
(tests/test_stream_ref_cpu.py shows that the comparisons can fail and that torch's fp32 arithmetic stays inside).  Called directly;
operands in NaN slabs, outputs in canary slabs with intact guards; VN = 8 elements of a 16-byte vector in bf16, 4 in fp32.

  activation  mmgl_activation_fwd against stream_ref.ActRef: 4 activations x 2 dtypes, n in {1, VN - 1, VN, VN + 1, 65 VN + 3,
              2048 * 256 VN + 3 VN + (VN - 1)} (nothing but the tail loop, one vector, vectors and a tail, past the 2048-block cap with a
              tail); randn * 3 with +-{0, 1e-30, 5, 9, 30, 100, 1e13, 1e20} planted; finite in, finite out; in place bit-equal.
  scale       mmgl_scale, the same n, s in {1/3, 0, 1, -2^-20}: bit-equal to torch's fp32 product, in place and out of place.
  AdamW       mmgl_adamw_step against stream_ref.AdamWRef, one step from the state handed in: n in {1, 255, 257, 10007, 2048 * 256 + 259},
              an fp32 parameter / bf16 + fp32 master / bf16 alone, betas (0.9, 0.95) and (0.9, 0.999), step in {1, 2, 3, 1000},
              wd in {0, 0.01}, grad_scale in {1, 1/8, 1/3}, p = 0 and p = randn, gradients 0, 1e-20, 1e4 planted.
  interleave  mmgl_neighbor_interleave_fwd / bwd, bit-exact against torch indexing: B = 2, Nt in {1, 3}, Ni in {0, 2}, one 16-byte
              chunk and 257 chunks per neighbor at n_tok 1 and 2, n_tok = 256; permutations and dropped locations (-1, N).
  position ids  mmgl_position_ids against cumsum: T in {1, 63, 64, 65, 128, 129, 700}, B in {1, 5}, all-ones / all-zeros / left-padded /
              right-padded / holed rows, bool and int64 masks through ops.position_ids, the direct call into a canary slab.
  Every refusal is checked to leave the canaries as they were."""
import pytest
import torch

from bounds import BF16, CANARY, F32, NAME, NAN, VEC, Slab, bits, check_bound, code, same
from stream_ref import ActRef, AdamWRef

pytestmark = pytest.mark.gpu

SEED = 0
ACTS = {1: "relu", 2: "gelu", 3: "quick_gelu", 4: "gelu_tanh"}


def _sizes(dtype):
    vn = VEC[dtype]
    return [1, vn - 1, vn, vn + 1, 65 * vn + 3, 2048 * 256 * vn + 3 * vn + (vn - 1)]


def _group(dtype, n):
    vn = VEC[dtype]
    return f"{'tail only' if n < vn else 'one vector' if n == vn else 'capped, tail' if n > 2048 * 256 * vn else 'vectors, tail'} {NAME[dtype]}"


def _call(name, *args):
    from mmgl_amd import _lib
    _lib.call(name, None, *[_lib.ptr(a) if a is None or isinstance(a, torch.Tensor) else a for a in args], _lib.stream_ptr())


# ------------------------------------------------------------------------------------------ activation
@pytest.mark.parametrize("act", list(ACTS), ids=ACTS.get)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_activation_bounds(dtype, act):
    for n in _sizes(dtype):
        x = ActRef.inputs(dtype, n, seed=SEED).cuda()
        assert torch.isfinite(x.float()).all()
        xs, y, z = Slab((n,), dtype, NAN, x), Slab((n,), dtype, CANARY), Slab((n,), dtype, CANARY, x)
        _call("mmgl_activation_fwd", xs.v, y.v, n, act, code(dtype))
        _call("mmgl_activation_fwd", z.v, z.v, n, act, code(dtype))            # in place, as ops.activation_ calls it
        what = f"{NAME[dtype]}-{ACTS[act]}-n{n}"
        ActRef(x, act).check(y.v, what, _group(dtype, n))
        assert same(y.v, z.v), f"{what}: in place differs from out of place"
        assert same(xs.v, x) and xs.untouched() and y.untouched() and z.untouched(), f"{what}: the operand or a guard changed"


def test_activation_ops_route_and_refusals():
    from mmgl_amd import ops
    x = ActRef.inputs(F32, 263, seed=SEED).cuda()
    ActRef(x, 2).check(ops.activation_(x.clone(), "gelu"), "ops.activation_ f32 gelu n263", "ops route f32")
    xs, y = Slab((263,), F32, NAN, x), Slab((263,), F32, CANARY)
    for args, msg in [((xs.v, y.v, 263, 0, 0), "not in"), ((xs.v, y.v, 263, 5, 0), "not in"), ((None, y.v, 263, 2, 0), "null pointer"),
                      ((xs.v, None, 263, 2, 0), "null pointer"), ((xs.v, y.v, 263, 2, 7), "bad dtype")]:
        with pytest.raises(ValueError, match=msg):
            _call("mmgl_activation_fwd", *args)
    _call("mmgl_activation_fwd", xs.v, y.v, 0, 2, 0)                            # n = 0: OK, nothing written
    torch.cuda.synchronize()
    assert y.unwritten() and xs.untouched()


# ------------------------------------------------------------------------------------------ scale
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_scale_is_torchs_fp32_product(dtype):
    for n in _sizes(dtype):
        x = torch.randn(n, generator=torch.Generator().manual_seed(SEED)).to(dtype).cuda()
        for s in (1 / 3, 0.0, 1.0, -2.0 ** -20):
            st = Slab((1,), F32, NAN, torch.tensor([s], device="cuda"))
            xs, y, z = Slab((n,), dtype, NAN, x), Slab((n,), dtype, CANARY), Slab((n,), dtype, CANARY, x)
            _call("mmgl_scale", xs.v, st.v, y.v, n, code(dtype))
            _call("mmgl_scale", z.v, st.v, z.v, n, code(dtype))
            want = (x.float() * st.v[0]).to(dtype)
            what = f"{NAME[dtype]}-n{n}-s{s:.3g}"
            bad = int((bits(y.v) != bits(want)).sum())
            print(f"[bound {_group(dtype, n)}] scale {what}: {bad} of {n} elements differ from torch's fp32 product")
            assert bad == 0 and same(z.v, want), f"{what}: {bad} elements differ, or in place differs"
            assert same(xs.v, x) and all(t.untouched() for t in (xs, y, z, st))
    xs, y = Slab((9,), dtype, NAN, torch.ones(9, dtype=dtype, device="cuda")), Slab((9,), dtype, CANARY)
    st = torch.ones(1, device="cuda")
    for args, msg in [((None, st, y.v, 9, code(dtype)), "null pointer"), ((xs.v, None, y.v, 9, code(dtype)), "null pointer"),
                      ((xs.v, st, None, 9, code(dtype)), "null pointer"), ((xs.v, st, y.v, 9, 7), "bad dtype")]:
        with pytest.raises(ValueError, match=msg):
            _call("mmgl_scale", *args)
    _call("mmgl_scale", xs.v, st, y.v, 0, code(dtype))
    torch.cuda.synchronize()
    assert y.unwritten()


# ------------------------------------------------------------------------------------------ AdamW
LR, EPS = 1e-2, 1e-8
ADAM_N = [1, 255, 257, 10007, 2048 * 256 + 259]
VARIANTS = [(wd, gs, pz) for wd in (0.0, 0.01) for gs in (1.0, 0.125, 1 / 3) for pz in (True, False)]


def _adam_state(layout, n, step, p_zero):
    """(param slab, master slab or None, m, v, grad slab, p: the fp32 state the kernel reads)."""
    pdt = F32 if layout == "f32" else BF16
    p, m, v, g = (t.cuda() for t in AdamWRef.inputs(pdt, n, step, p_zero, seed=SEED))
    if layout == "bf16":
        p = p.to(BF16).float()
    return (Slab((n,), pdt, CANARY, p.to(pdt)), Slab((n,), F32, CANARY, p) if layout == "master" else None, Slab((n,), F32, CANARY, m),
            Slab((n,), F32, CANARY, v), Slab((n,), pdt, NAN, g), p, m, v, g)


def _adam_call(param, master, grad, m, v, n, b1, b2, wd, step, gs, dtype):
    _call("mmgl_adamw_step", param, master, grad, m, v, n, LR, b1, b2, EPS, wd, step, gs, code(dtype))


@pytest.mark.parametrize("step", [1, 2, 3, 1000])
@pytest.mark.parametrize("betas", [(0.9, 0.95), (0.9, 0.999)], ids=["b95", "b999"])
@pytest.mark.parametrize("n", ADAM_N)
@pytest.mark.parametrize("layout", ["f32", "master", "bf16"])
def test_adamw_one_step(layout, n, betas, step):
    """Each (wd, grad_scale, p = 0 | randn) variant is one launch from its own state; the rows of a failure message are the variants in
    VARIANTS' order.  The largest err / bound over the twelve is printed per output."""
    errs, bounds = {k: [] for k in "mvp"}, {k: [] for k in "mvp"}
    for wd, gs, pz in VARIANTS:
        ps, ms, m_, v_, gsl, p, m, v, g = _adam_state(layout, n, step, pz)
        _adam_call(ps.v, None if ms is None else ms.v, gsl.v, m_.v, v_.v, n, *betas, wd, step, gs, ps.v.dtype)
        ref = AdamWRef(p, m, v, g, LR, *betas, EPS, wd, step, gs, store_bf16=layout == "bf16")
        for k, got in dict(m=m_.v, v=v_.v, p=ps.v if ms is None else ms.v).items():
            errs[k].append(ref.err(got, k))
            bounds[k].append(ref.bound(k))
        if ms is not None:
            assert same(ps.v, ms.v.to(BF16)), f"wd={wd} gs={gs} p0={pz}: the bf16 parameter is not the rounded master"
        assert same(gsl.v, g) and all(s.untouched() for s in (ps, m_, v_, gsl) + (() if ms is None else (ms,))), "an operand or a guard changed"
    what = f"{layout}-n{n}-betas{betas[1]}-step{step}"
    group = f"{'one block' if n <= 256 else 'capped, second trip' if n > 2048 * 256 else 'blocks'} {layout}"
    for k in "mvp":
        check_bound(torch.stack(errs[k]), None, torch.stack(bounds[k]), f"adamw {what} {k}", group)


def test_adamw_refusals():
    n = 257
    ps, ms, m_, v_, gsl, *_ = _adam_state("master", n, 2, False)
    keep = [s.buf.clone() for s in (ps, ms, m_, v_)]
    a = dict(param=ps.v, master=ms.v, grad=gsl.v, m=m_.v, v=v_.v, n=n, b1=0.9, b2=0.95, wd=0.0, step=2, gs=1.0, dtype=BF16)
    for kw in (dict(step=0), dict(step=-1), dict(param=None), dict(grad=None), dict(m=None), dict(v=None)):
        with pytest.raises(ValueError, match="bad arguments"):
            _adam_call(**dict(a, **kw))
    with pytest.raises(ValueError, match="bad dtype"):
        _call("mmgl_adamw_step", ps.v, ms.v, gsl.v, m_.v, v_.v, n, LR, 0.9, 0.95, EPS, 0.0, 2, 1.0, 7)
    _adam_call(**dict(a, n=0))                                                  # n = 0: OK, nothing written
    torch.cuda.synchronize()
    assert all(torch.equal(s.buf, k) for s, k in zip((ps, ms, m_, v_), keep)), "a refused call wrote"


# ------------------------------------------------------------------------------------------ neighbor interleave
def _locations(B, Nt, Ni, kind, gen):
    """kind 'perm': every batch row maps its N neighbors onto a permutation of the N slots.  'drop': neighbor 0 of each row goes to
    -1 (even rows) or N (odd rows) and the rest to distinct slots; no two neighbors share a slot."""
    N = Nt + Ni
    loc = torch.stack([torch.randperm(N, generator=gen) for _ in range(B)])
    if kind == "drop":
        loc[0::2, 0], loc[1::2, 0] = -1, N
    pos = torch.tensor([-1, 0, 1, 5])[torch.randint(0, 4, (B, N), generator=gen)]
    return loc[:, :Nt].contiguous(), loc[:, Nt:].contiguous(), pos[:, :Nt].contiguous(), pos[:, Nt:].contiguous()


def _interleave_want(text, vis, tl, il, tp, ip, dout):
    """Plain indexing: (out, valid, dtext, dvis)."""
    B, Nt, n_tok, d = text.shape
    Ni = 0 if vis is None else vis.shape[1]
    N = Nt + Ni
    src = text if vis is None else torch.cat([text, vis], 1)
    loc, pos = (tl, tp) if vis is None else (torch.cat([tl, il], 1), torch.cat([tp, ip], 1))
    out, valid, dsrc = torch.zeros(B, N, n_tok, d, dtype=text.dtype, device=text.device), torch.zeros(B, N, n_tok, dtype=torch.uint8, device=text.device), torch.zeros_like(src)
    for b in range(B):
        for j in range(N):
            l = int(loc[b, j])
            if 0 <= l < N:
                out[b, l] = src[b, j]
                valid[b, l] = 1 if int(pos[b, j]) > 0 else 0
                dsrc[b, j] = dout[b, l]
    return out, valid, dsrc[:, :Nt], (dsrc[:, Nt:] if Ni else None)


def _interleave_shapes(dtype):
    vn = VEC[dtype]
    return [(1, vn, "one chunk"), (2, vn // 2, "one chunk"), (1, 257 * vn, "257 chunks: second trip"), (2, 257 * vn // 2, "257 chunks: second trip"),
            (256, vn + 1, "n_tok 256")]


@pytest.mark.parametrize("kind", ["perm", "drop"])
@pytest.mark.parametrize("Ni", [0, 2])
@pytest.mark.parametrize("Nt", [1, 3])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_interleave_is_exact(dtype, Nt, Ni, kind):
    B, N = 2, Nt + Ni
    for n_tok, d, seam in _interleave_shapes(dtype):
        gen = torch.Generator().manual_seed(SEED)
        r = lambda *s: torch.randn(*s, generator=gen).to(dtype).cuda()
        text, vis, dout = r(B, Nt, n_tok, d), (r(B, Ni, n_tok, d) if Ni else None), r(B, N, n_tok, d)
        tl, il, tp, ip = (t.cuda() for t in _locations(B, Nt, Ni, kind, gen))
        if not Ni:
            il = ip = None
        ts, vs, ds = Slab(text.shape, dtype, NAN, text), (Slab(vis.shape, dtype, NAN, vis) if Ni else None), Slab(dout.shape, dtype, NAN, dout)
        out, valid = Slab((B, N, n_tok, d), dtype, CANARY), Slab((B, N, n_tok), torch.uint8, 0xA5)
        dtext, dvis = Slab(text.shape, dtype, CANARY), (Slab(vis.shape, dtype, CANARY) if Ni else None)
        _call("mmgl_neighbor_interleave_fwd", ts.v, vs.v if Ni else None, tl, il, tp, ip, out.v, valid.v, B, Nt, Ni, n_tok, d, code(dtype))
        _call("mmgl_neighbor_interleave_bwd", ds.v, tl, il, dtext.v, dvis.v if Ni else None, B, Nt, Ni, n_tok, d, code(dtype))
        w_out, w_valid, w_dt, w_dv = _interleave_want(text, vis, tl, il, tp, ip, dout)
        what = f"{NAME[dtype]}-Nt{Nt}-Ni{Ni}-{kind}-{n_tok}x{d}"
        bad = [int((bits(a) != bits(b)).sum()) for a, b in ((out.v, w_out), (valid.v, w_valid), (dtext.v, w_dt))] + ([int((bits(dvis.v) != bits(w_dv)).sum())] if Ni else [])
        print(f"[bound {seam} {NAME[dtype]}] interleave {what}: elements that differ (out, valid, dtext, dvis) {bad}")
        assert not any(bad), f"{what}: elements that differ from plain indexing (out, valid, dtext, dvis): {bad}"
        slabs = [ts, ds, out, valid, dtext] + ([vs, dvis] if Ni else [])
        assert all(s.untouched() for s in slabs), f"{what}: a guard changed"
        assert same(ts.v, text) and same(ds.v, dout)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_interleave_refusals(dtype):
    B, Nt, Ni, vn = 2, 1, 0, VEC[dtype]
    tl = tp = torch.zeros(B, Nt, dtype=torch.int64, device="cuda")
    for n_tok, d, msg in [(257, vn, "n_tok > 256"), (1, vn + 1, "16-byte"), (3, vn // 2, "16-byte"), (0, vn, "bad sizes"), (1, 0, "bad sizes")]:
        size = (B, Nt, max(n_tok, 1), max(d, 1))
        text, out, valid, dtext = Slab(size, dtype, NAN), Slab(size, dtype, CANARY), Slab(size[:3], torch.uint8, 0xA5), Slab(size, dtype, CANARY)
        with pytest.raises(ValueError, match=msg):
            _call("mmgl_neighbor_interleave_fwd", text.v, None, tl, None, tp, None, out.v, valid.v, B, Nt, Ni, n_tok, d, code(dtype))
        with pytest.raises(ValueError, match=msg):
            _call("mmgl_neighbor_interleave_bwd", out.v, tl, None, dtext.v, None, B, Nt, Ni, n_tok, d, code(dtype))
        torch.cuda.synchronize()
        assert out.unwritten() and valid.unwritten() and dtext.unwritten(), f"a refused call ({n_tok} x {d}) wrote"
    size = (B, Nt, 1, vn)
    text, out, valid, dtext = Slab(size, dtype, NAN), Slab(size, dtype, CANARY), Slab(size[:3], torch.uint8, 0xA5), Slab(size, dtype, CANARY)
    with pytest.raises(ValueError, match="bad dtype"):                          # refused before the forward clears its outputs
        _call("mmgl_neighbor_interleave_fwd", text.v, None, tl, None, tp, None, out.v, valid.v, B, Nt, Ni, 1, vn, 7)
    with pytest.raises(ValueError, match="bad dtype"):
        _call("mmgl_neighbor_interleave_bwd", out.v, tl, None, dtext.v, None, B, Nt, Ni, 1, vn, 7)
    with pytest.raises(ValueError, match="null pointer"):
        _call("mmgl_neighbor_interleave_fwd", text.v, None, tl, None, tp, None, None, valid.v, B, Nt, Ni, 1, vn, code(dtype))
    with pytest.raises(ValueError, match="null pointer"):
        _call("mmgl_neighbor_interleave_bwd", out.v, tl, None, None, None, B, Nt, Ni, 1, vn, code(dtype))
    torch.cuda.synchronize()
    assert out.unwritten() and valid.unwritten() and dtext.unwritten()


# ------------------------------------------------------------------------------------------ position ids
def _mask_rows(T, gen):
    """all ones, all zeros, left-padded, right-padded, holes: int64 [5, T]."""
    pad = min(max(T // 3, 1), T - 1) if T > 1 else 0
    m = torch.ones(5, T, dtype=torch.int64)
    m[1] = 0
    m[2, :pad] = 0
    m[3, T - pad:] = 0
    m[4] = torch.randint(0, 2, (T,), generator=gen)
    return m


@pytest.mark.parametrize("T", [1, 63, 64, 65, 128, 129, 700])
def test_position_ids_are_the_cumsum(T):
    from mmgl_amd import ops
    rows = _mask_rows(T, torch.Generator().manual_seed(SEED)).cuda()
    seam = "one partial chunk" if T < 64 else "whole chunks" if T % 64 == 0 else "carry into a partial chunk"
    for B, masks in ((1, [rows[i:i + 1] for i in range(5)]), (5, [rows])):
        for k, m in enumerate(masks):
            want = torch.cumsum(m, 1) * m + 1
            ms, out = Slab(m.shape, torch.int64, -1, m), Slab(m.shape, torch.int64, -77)
            _call("mmgl_position_ids", ms.v, out.v, B, T)
            bad = [int((out.v != want).sum()), int((ops.position_ids(m) != want).sum()), int((ops.position_ids(m.bool()) != want).sum())]
            print(f"[bound {seam}] position_ids T{T}-B{B}-{'all rows' if B == 5 else ['ones', 'zeros', 'left', 'right', 'holes'][k]}: elements that differ (direct, int64, bool) {bad}")
            assert not any(bad), f"T={T} B={B}: elements that differ from cumsum (direct, int64 mask, bool mask): {bad}"
            assert ms.untouched() and out.untouched() and torch.equal(ms.v, m)


def test_position_ids_refusals():
    m, out = torch.ones(2, 65, dtype=torch.int64, device="cuda"), Slab((2, 65), torch.int64, -77)
    for args in ((m, out.v, 0, 65), (m, out.v, 2, 0), (None, out.v, 2, 65), (m, None, 2, 65)):
        with pytest.raises(ValueError, match="bad arguments"):
            _call("mmgl_position_ids", *args)
    torch.cuda.synchronize()
    assert out.unwritten()
