"""-m gpu: the general attention core (csrc/attn_general.hip: attention dropout, layer_head_mask, output_attentions) against
attn_ref.GeneralAttnRef -- an fp64 reference of the storage-rounded operands -- element by element: out, lse, dq, dk, dv and probs each
within the bound of the class docstring, lse exactly +inf and probs exactly fp32(1 / S) hm on a row without an allowed key, exact
zeros where the mask kills everything.  The keep mask of the reference is bounds.hash_keep, never mmgl_attn_dropout_mask (which is
held bit for bit against hash_keep on its own).  tests/test_attn_general_ref_cpu.py shows on the CPU that this comparison fails for a
wrong keep index, scale, head mask, tie factor, causal edge, dropped key or lost row chunk.  mmgl_attn_general_fwd / _bwd are called
directly, so lse and the workspace are seen; every result buffer holds NaN before the call.

  A  seams: T in {1, 31, 32, 33, 63, 64, 65, 129} against S in {1, 63, 64, 65, 129, 200} (cross) and T = S in the T set (causal) --
     AG_RB = 32, AG_ROWS = AG_KC = 64 on either side --, D in {1, 16, 20, 63, 64, 65, 96, 127, 128} (lanes past D, the second
     accumulator, one live lane in it), head mask [1, 0, 0.5, 2] and none, p_drop 0 and 0.3, probs requested and not.  A handful also
     through ops.attn_general under autograd, bit for bit.
  B  rows without an allowed key: a cross sample without a valid key on its own; causal left padding of 5 rows (the first row block
     only) and of 70 rows (two row blocks with such rows, the others without: the per-block chunk count differs inside one launch),
     padded keys in their future (doubly masked); each plain and with dropout and head mask.  Those rows and keys also on their own.
  C  dropout: p in {0.3, 0.5} and one so small that the threshold is 0, a seed with its top bit set, mmgl_attn_dropout_mask against
     hash_keep for every case's (B, H, T, S) and for one mask of more than 4096 x 256 elements, eval mode and p = 0 bit-equal.
  D  memory: operands as windows of NaN and then +Inf buffers, results, probs and an exactly sized NaN workspace between canaries;
     two launches.
  E  refusals: an error code and nothing written."""
import collections
import ctypes

import pytest
import torch

from attn_ref import GeneralAttnRef, XAttnRef
from bounds import BF16, F32, NAME, ByteSlab, Slab, code, hash_keep, nan

pytestmark = pytest.mark.gpu

SEED = 0                              # tests/test_attn_general_ref_cpu.py: every wrong reference leaves the bound on >= 40 % at this seed
DSEED = 0x9E3779B97F4A7C15            # the dropout seed: top bit set
HM = (1.0, 0.0, 0.5, 2.0)
TS = (1, 31, 32, 33, 63, 64, 65, 129)
SS = (1, 63, 64, 65, 129, 200)
DS = (1, 16, 20, 63, 64, 65, 96, 127, 128)

Case = collections.namedtuple("Case", "group dtype D T S B H causal left first hm p probs")


def _id(c):
    return (f"{NAME[c.dtype]}-D{c.D}-T{c.T}-S{c.S}-B{c.B}H{c.H}" + ("-causal" if c.causal else f"-m{c.first}") + (f"-left{c.left}" if c.left else "")
            + ("-hm" if c.hm else "") + (f"-p{c.p}" if c.p else "") + ("-probs" if c.probs else ""))


def _cases_A(dtype):
    shapes = [(T, SS[i % len(SS)], False) for i, T in enumerate(TS)] + [(129, 200, False), (64, 64, False), (1, 200, False)]
    shapes += [(T, T, True) for T in TS]
    out = []
    for i, (T, S, causal) in enumerate(shapes):
        D = DS[(i + (4 if dtype == BF16 else 0)) % len(DS)]
        out.append(Case("A", dtype, D, T, S, 3 if causal else 2, 3 if causal else 4, causal, 0, i % 3, i % 2 == 0, 0.3 if i % 3 else 0.0, i % 4 < 2))
    return out


CASES_A = _cases_A(F32) + _cases_A(BF16)
AUTOGRAD = [c for c in CASES_A if (c.T, c.S) in ((33, 65), (129, 200), (65, 65), (129, 129))]
CASES_B = [Case("B", dt, D, T, S, B, 3, causal, left, first, opt, 0.3 if opt else 0.0, opt)
           for dt in (F32, BF16) for opt in (False, True)
           for D, T, S, B, causal, left, first in ((16, 70, 130, 1, False, 0, 2), (65, 130, 130, 3, True, 5, 0), (16, 200, 200, 3, True, 70, 0))]
CASES_C = [Case("C", dt, 20, 65, 129, 2, 4, False, 0, 0, True, p, False) for dt in (F32, BF16) for p in (0.5, 1e-12)] + \
          [Case("C", dt, 64, 129, 129, 3, 3, True, 5, 0, True, 0.5, True) for dt in (F32, BF16)]
CASES_D = [Case("D", dt, D, T, S, 2, 3, causal, 5 if causal else 0, 0, True, 0.3, True)
           for dt in (F32, BF16) for D, T, S, causal in ((20, 33, 65, False), (65, 70, 70, True))]
EVERY = CASES_A + CASES_B + CASES_C + CASES_D


def _hm(c, device="cuda"):
    return torch.tensor(HM[:c.H], device=device) if c.hm else None


def _inputs(c):
    q, k, v, dout = GeneralAttnRef.inputs(c.dtype, c.B, c.T, c.S, c.H, c.D, c.causal, seed=SEED, device="cuda")
    am = GeneralAttnRef.causal_mask(c.B, c.T, c.left) if c.causal else XAttnRef.mask(c.B, c.S, c.first)
    return q, k, v, dout, am.cuda()


def _fwd(c, q, k, v, am, hm, out, probs, lse, over=None):
    from mmgl_amd import _lib
    a = dict(q=q, k=k, v=v, am=am, hm=hm, out=out, probs=probs, lse=lse, B=c.B, H=c.H, T=c.T, S=c.S, D=c.D, causal=int(c.causal), p=c.p,
             dtype=code(c.dtype))
    a.update(over or {})
    p = lambda x: x if (x is None or isinstance(x, ctypes.c_void_p)) else _lib.ptr(x)
    _lib.call("mmgl_attn_general_fwd", None, p(a["q"]), p(a["k"]), p(a["v"]), p(a["am"]), p(a["hm"]), p(a["out"]), p(a["probs"]), p(a["lse"]),
              a["B"], a["H"], a["T"], a["S"], a["D"], a["causal"], float(a["p"]), DSEED, a["dtype"], _lib.stream_ptr())


def _bwd(c, dout, q, k, v, lse, am, hm, dq, dk, dv, ws, nws, over=None):
    from mmgl_amd import _lib
    a = dict(dout=dout, q=q, k=k, v=v, lse=lse, am=am, hm=hm, dq=dq, dk=dk, dv=dv, ws=ws, nws=nws, B=c.B, H=c.H, T=c.T, S=c.S, D=c.D,
             causal=int(c.causal), p=c.p, dtype=code(c.dtype))
    a.update(over or {})
    p = lambda x: x if (x is None or isinstance(x, ctypes.c_void_p)) else _lib.ptr(x)
    _lib.call("mmgl_attn_general_bwd", None, p(a["dout"]), p(a["q"]), p(a["k"]), p(a["v"]), p(a["lse"]), p(a["am"]), p(a["hm"]), p(a["dq"]),
              p(a["dk"]), p(a["dv"]), p(a["ws"]), a["nws"], a["B"], a["H"], a["T"], a["S"], a["D"], a["causal"], float(a["p"]), DSEED,
              a["dtype"], _lib.stream_ptr())


def _buffers(c):
    return dict(out=nan(c.B, c.T, c.H * c.D, dtype=c.dtype), lse=nan(c.B, c.H, c.T, dtype=F32),
                probs=nan(c.B, c.H, c.T, c.S, dtype=c.dtype) if c.probs else None, dq=nan(c.B, c.T, c.H * c.D, dtype=c.dtype),
                dk=nan(c.B, c.S, c.H * c.D, dtype=c.dtype), dv=nan(c.B, c.S, c.H * c.D, dtype=c.dtype))


def _call(c, q, k, v, dout, am):
    """dict of out, lse, probs, dq, dk, dv of the raw entry points; every buffer holds NaN before the call, the workspace too."""
    from mmgl_amd import _lib
    r, hm = _buffers(c), _hm(c)
    _fwd(c, q, k, v, am, hm, r["out"], r["probs"], r["lse"])
    nws = _lib.lib().mmgl_attn_general_bwd_workspace(c.B, c.H, c.T)
    assert nws == (c.B * c.H * c.T * 4 + 255) // 256 * 256
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device="cuda")
    _bwd(c, dout, q, k, v, r["lse"], am, hm, r["dq"], r["dk"], r["dv"], ws, nws)
    torch.cuda.synchronize()
    return r


def _ref(c, q, k, v, dout, am):
    return GeneralAttnRef(q, k, v, am, dout, c.H, causal=c.causal, head_mask=_hm(c), p_drop=c.p, seed=DSEED)


def _group(c):
    return f"{c.group} {NAME[c.dtype]}"


def _check(c):
    ins = _inputs(c)
    got = _call(c, *ins)
    ref = _ref(c, *ins)
    ref.check(got, _id(c), _group(c))
    return ins, got, ref


# ------------------------------------------------------------------------------------------ A: seams
def test_A_case_list_covers_every_seam_and_head_dim_class():
    for dt in (F32, BF16):
        cs = [c for c in CASES_A if c.dtype == dt]
        assert {c.T for c in cs if not c.causal} >= set(TS) and {c.S for c in cs if not c.causal} >= set(SS)
        assert {c.T for c in cs if c.causal} >= set(TS)
        assert {c.D for c in cs} == set(DS), "every head dim"
        cls = lambda D: "below64" if D < 64 else "64" if D == 64 else "65..127" if D < 128 else "128"
        for sub in (cs, [c for c in cs if c.causal], [c for c in cs if not c.causal]):
            assert {cls(c.D) for c in sub} == {"below64", "64", "65..127", "128"}
        assert {(c.hm, c.p > 0, c.probs) for c in cs} == {(a, b, d) for a in (True, False) for b in (True, False) for d in (True, False)}
        assert {c.first % 3 for c in cs if not c.causal} == {0, 1, 2}


@pytest.mark.parametrize("case", CASES_A, ids=_id)
def test_A_seams(case):
    _check(case)


@pytest.mark.parametrize("case", AUTOGRAD, ids=_id)
def test_A_ops_under_autograd_is_the_raw_call(case):
    from mmgl_amd import ops
    c = case
    q, k, v, dout, am = _inputs(c)
    got = _call(c, q, k, v, dout, am)
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    out, probs = ops.attn_general(qg, kg, vg, am, c.H, causal=c.causal, head_mask=_hm(c), p_drop=c.p, training=True, seed=DSEED,
                                  output_attentions=c.probs)
    grads = torch.autograd.grad(out, (qg, kg, vg), dout)
    for name, a in zip(("out", "dq", "dk", "dv"), (out,) + grads):
        assert torch.equal(a, got[name]), f"{name}: ops.attn_general under autograd is not the raw entry point's result"
    assert (probs is None) == (got["probs"] is None) and (probs is None or torch.equal(probs, got["probs"]))


# ------------------------------------------------------------------------------------------ B: rows without an allowed key
def test_B_case_list_has_the_row_block_properties():
    for c in CASES_B:
        if c.causal:
            blocks = {t // 64 for t in range(c.left)}
            nrb = (c.T + 63) // 64
            assert blocks and len(blocks) < nrb, "a row block without such rows next to one with them"
            assert (len(blocks) == 1) == (c.left == 5) and (c.left != 70 or blocks == {0, 1} and nrb >= 4)
    assert {c.left for c in CASES_B if c.causal} == {5, 70} and any(not c.causal and c.B == 1 and c.first == 2 for c in CASES_B)


@pytest.mark.parametrize("case", CASES_B, ids=_id)
def test_B_rows_without_an_allowed_key(case):
    c = case
    ins, got, ref = _check(c)
    uni = ref.uni_rows
    assert bool(uni.any())
    assert bool((got["lse"][uni[:, None, :].expand_as(got["lse"])] == float("inf")).all())
    ref.check(got, _id(c) + " [rows without a key]", _group(c), rows=uni)
    if c.causal:
        dkeys = (ref.double & uni[:, :, None]).any(1)
        assert bool(dkeys.any()), "no doubly-masked key"
        ref.check(got, _id(c) + " [doubly-masked keys]", _group(c), keys=dkeys)
        # a padded key that no such row reaches holds exact zeros (sample 1: right padding)
        dead = ~ref.valid & ~uni.any(1)[:, None]
        assert bool(dead.any())
        for name in ("dk", "dv"):
            assert float(got[name].reshape(c.B, c.S, c.H, c.D)[dead].float().abs().max()) == 0.0, f"{name}: a dead key is not exactly zero"


# ------------------------------------------------------------------------------------------ C: dropout
@pytest.mark.parametrize("case", CASES_C, ids=_id)
def test_C_dropout(case):
    c = case
    ins, got, ref = _check(c)
    if c.p < 1e-6:                       # threshold 0 and fp32(1 / (1 - p)) = 1: nothing dropped, the p = 0 result bit for bit
        plain = _call(c._replace(p=0.0), *ins)
        for name in ("out", "lse", "dq", "dk", "dv"):
            assert torch.equal(got[name], plain[name]), f"{name}: p = {c.p} differs from p = 0"


def test_C_dropout_mask_is_hash_keep_for_every_case():
    from mmgl_amd import ops
    shapes = sorted({(c.B, c.H, c.T, c.S, c.p) for c in EVERY if c.p > 0} | {(2, 3, 257, 700, 0.3)})
    assert any(B * H * T * S > 4096 * 256 for B, H, T, S, p in shapes), "the mask kernel's grid-stride loop never takes a second trip"
    for B, H, T, S, p in shapes:
        for seed in (DSEED, 7):
            m = ops.attn_dropout_mask(B, H, T, S, p, seed, "cuda").cpu()
            want = torch.from_numpy(hash_keep(seed, B * H * T * S, p)).view(B, H, T, S)
            assert torch.equal(m.bool(), want), f"{(B, H, T, S, p, seed)}: {(m.bool() != want).sum().item()} mask elements differ"
            assert bool(((m == 0) | (m == 1)).all())


def test_C_eval_mode_and_p0_are_bit_equal():
    from mmgl_amd import ops
    c = CASES_C[0]
    q, k, v, dout, am = _inputs(c)
    outs = []
    for kw in (dict(p_drop=0.3, training=False), dict(p_drop=0.0, training=True)):
        qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
        out, probs = ops.attn_general(qg, kg, vg, am, c.H, head_mask=_hm(c), seed=DSEED, output_attentions=True, **kw)
        outs.append((out, probs) + torch.autograd.grad(out, (qg, kg, vg), dout))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ D: memory
@pytest.mark.parametrize("case", CASES_D, ids=_id)
def test_D_isolation_and_determinism(case):
    from mmgl_amd import _lib
    c = case
    (q, k, v, dout, am), plain, ref = _check(c)
    hm = _hm(c)
    nws = _lib.lib().mmgl_attn_general_bwd_workspace(c.B, c.H, c.T)
    for fill in (float("nan"), float("inf")):
        ins = [Slab(t.shape, t.dtype, fill, t) for t in (q, k, v, dout)] + [Slab(am.shape, torch.uint8, 255, am), Slab(hm.shape, F32, fill, hm)]
        qs, ks, vs, gs, ms, hs = ins
        canary = 1536.0            # exact in bf16
        outs = {n: Slab(plain[n].shape, plain[n].dtype, canary) for n in ("out", "lse", "probs", "dq", "dk", "dv")}
        ws = ByteSlab(nws)
        _fwd(c, qs.v, ks.v, vs.v, ms.v, hs.v, outs["out"].v, outs["probs"].v, outs["lse"].v)
        _bwd(c, gs.v, qs.v, ks.v, vs.v, outs["lse"].v, ms.v, hs.v, outs["dq"].v, outs["dk"].v, outs["dv"].v, ws.ptr(), nws)
        torch.cuda.synchronize()
        assert ws.untouched(), "bytes next to the workspace were written"
        for n, s in outs.items():
            assert s.untouched(), f"bytes next to {n} were written"
            assert torch.isfinite(s.v.float()).all() or n == "lse", f"{n}: a value from outside the operands reached the result"
            assert torch.equal(s.v, plain[n]), f"{n}: differs from the run on plain tensors"
        for n, s in zip(("q", "k", "v", "dout", "key_valid", "head_mask"), ins):
            assert s.untouched(), f"bytes next to {n} were written"
    again = _call(c, q, k, v, dout, am)
    for n in plain:
        assert torch.equal(again[n], plain[n]), f"{n}: two launches differ"


# ------------------------------------------------------------------------------------------ E: refusals
def _refused(c, fwd_over=None, bwd_over=None):
    from mmgl_amd import _lib
    q, k, v, dout, am = _inputs(c)
    r, hm = _buffers(c), _hm(c)
    nws = _lib.lib().mmgl_attn_general_bwd_workspace(c.B, c.H, c.T)
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device="cuda")
    if fwd_over is not None:
        with pytest.raises(ValueError):
            _fwd(c, q, k, v, am, hm, r["out"], r["probs"], r["lse"], fwd_over)
    if bwd_over is not None:
        lse = torch.zeros(c.B, c.H, c.T, device="cuda")
        with pytest.raises(ValueError):
            _bwd(c, dout, q, k, v, lse, am, hm, r["dq"], r["dk"], r["dv"], ws, nws, bwd_over)
    torch.cuda.synchronize()
    for n, x in r.items():
        assert x is None or bool(torch.isnan(x).all()), f"{n}: written by a refused call"
    assert bool((ws == 0xFF).all()), "workspace: written by a refused call"


BASE_E = Case("E", F32, 16, 33, 33, 2, 2, False, 0, 0, True, 0.3, True)


@pytest.mark.parametrize("what,over", [("D129", dict(D=129)), ("causal-S-not-T", dict(causal=1, S=32)), ("p1", dict(p=1.0)), ("p-negative", dict(p=-0.1)),
                                       ("dtype", dict(dtype=99)), ("D0", dict(D=0))])
def test_E_bad_arguments_are_refused(what, over):
    _refused(BASE_E, over, over)


@pytest.mark.parametrize("name", ["q", "k", "v", "am", "out", "lse"])
def test_E_forward_null_pointer_is_refused(name):
    _refused(BASE_E, {name: ctypes.c_void_p(None)}, None)


@pytest.mark.parametrize("name", ["dout", "q", "k", "v", "lse", "am", "dq", "dk", "dv", "ws"])
def test_E_backward_null_pointer_is_refused(name):
    _refused(BASE_E, None, {name: ctypes.c_void_p(None)})


def test_E_workspace_one_byte_short_is_refused():
    from mmgl_amd import _lib
    nws = _lib.lib().mmgl_attn_general_bwd_workspace(BASE_E.B, BASE_E.H, BASE_E.T)
    _refused(BASE_E, None, dict(nws=nws - 1))
