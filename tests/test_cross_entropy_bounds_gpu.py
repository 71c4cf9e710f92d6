"""-m gpu: mmgl_cross_entropy_fwd / bwd (csrc/elementwise.hip) against row_ref.CrossEntropyRef -- an fp64 reference of the
storage-rounded logits -- row_lse, row_loss, loss_sum and count, and every element of dlogits (the count of roundings is in
CrossEntropyRef's docstring; tests/test_row_ref_cpu.py shows on the CPU that the comparison fails for a 16-byte chunk lost from lse, a
label one column off, a mean over rows instead of live rows, an ignored row treated as live).  The entry points are called directly,
operands carved out of NaN slabs, outputs out of canary slabs.

Six rows (labels 0, V - 1, ignored, an edge, V / 2, 7), unit randn logits with the edge columns raised so that each holds about 4.5 %
of its row's mass: 0, VN - 1, VN, both sides of vectors 256, 768 and 1024 (the second, fourth and fifth load of a thread), V - VN - 1,
V - VN, V - 1.  dloss = 1.7 unless said otherwise.

  A  V sweep, both dtypes: 1, 3, VN; 1001 and 8191 (rows that are no whole number of 16-byte chunks: the element-wise path); nvec =
     768, 1023, 1024, 1025 (either side of the four-loads-in-flight loop's condition i + 768 < nvec) and 2056; 50272 once; logits
     shifted by 1e4; a row with one dominant logit (loss ~ 0)
  B  -inf logits: a row whose first VN logits are -inf (thread 0's first vector, while its running maximum is still -inf), an odd-V
     row with logit 5 at -inf (the element-wise path), one -inf inside an otherwise finite vector: a finite lse within the bound,
     dlogits exactly 0 there.  Before ce_fwd_kernel's guard the first two gave a NaN lse
  C  in place, as lm_head_cross_entropy calls it: dlogits == logits, dloss = 1, the count of a larger total; bit-equal to the
     out-of-place call
  D  all rows ignored (loss_sum 0, count 0, dlogits all zero), labels < 0 and >= V count as ignored, two launches bit-equal"""
import pytest
import torch

from bounds import BF16, CANARY, F32, NAME, VEC, Slab
from row_ref import CrossEntropyRef

pytestmark = pytest.mark.gpu

SEED = 0                    # tests/test_row_ref_cpu.py's seed
IGNORE = -100
NVECS = (768, 1023, 1024, 1025, 2056)


def _call(x, lab, dloss, count=None, inplace=False):
    """fwd then bwd on slabs.  count: the divisor the backward is given instead of the forward's own (the LM head's whole-batch count).
    Returns the outputs (dlogits is the logits buffer itself when inplace)."""
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr
    rows, V = x.shape
    xs = Slab(x.shape, x.dtype, float("nan"), x)
    labs = Slab(lab.shape, torch.int64, -1, lab)
    lse, loss, lsum, cnt = (Slab(s, F32, CANARY) for s in ((rows,), (rows,), (1,), (1,)))
    dl = Slab((1,), F32, float("nan"), torch.tensor([dloss]))
    code, st = _lib.dtype_code(x), _lib.stream_ptr()
    _lib.call("mmgl_cross_entropy_fwd", None, ptr(xs.v), ptr(labs.v), ptr(lse.v), ptr(loss.v), ptr(lsum.v), ptr(cnt.v), rows, V, IGNORE, code, st)
    torch.cuda.synchronize()
    fwd_cnt = cnt.v.clone()
    div = cnt if count is None else Slab((1,), F32, float("nan"), torch.tensor([float(count)]))
    g = xs if inplace else Slab(x.shape, x.dtype, CANARY)
    _lib.call("mmgl_cross_entropy_bwd", None, ptr(xs.v), ptr(labs.v), ptr(lse.v), ptr(div.v), ptr(dl.v), ptr(g.v), rows, V, IGNORE, code, st)
    torch.cuda.synchronize()
    for name, s in dict(logits=xs, labels=labs, row_lse=lse, row_loss=loss, loss_sum=lsum, count=cnt, dloss=dl, dlogits=g).items():
        assert s.untouched(), f"written outside {name}"
    if not inplace:
        assert torch.equal(xs.v.view(torch.int16 if x.dtype == BF16 else torch.int32), x.view(torch.int16 if x.dtype == BF16 else torch.int32))
    return dict(row_lse=lse.v, row_loss=loss.v, loss_sum=lsum.v, count=fwd_cnt, dlogits=g.v)


def _check(x, lab, what, group, dloss=1.7, count=None):
    got = _call(x, lab, dloss, count)
    ref = CrossEntropyRef(x, lab, ignore=IGNORE, dloss=dloss, count=count)
    for name in ("row_lse", "row_loss", "loss_sum", "count", "dlogits"):
        ref.check(got[name], name, what, group)
    z = got["dlogits"][ref.exact0]
    assert bool((z == 0).all()), f"{what}: {int((z != 0).sum())} gradient elements of ignored rows or -inf logits are not exactly zero"
    assert bool((got["row_loss"][~ref.live] == 0).all())
    return got, ref


def _path(dtype, V):
    vn = VEC[dtype]
    nvec = V // vn if V % vn == 0 else 0
    return "scalar" if nvec == 0 else ("4-in-flight" if nvec > 768 else "vector")


def _v_list(dtype):
    vn = VEC[dtype]
    return [1, 3, vn, 1001, 8191] + [n * vn for n in NVECS]


def test_case_list_reaches_both_paths_and_loop_sides():
    for dt in (BF16, F32):
        vs = _v_list(dt)
        assert {_path(dt, V) for V in vs} == {"scalar", "vector", "4-in-flight"}
        nv = {V // VEC[dt] for V in vs if _path(dt, V) != "scalar"}
        assert {768, 1023, 1024, 1025} <= nv                 # i + 768 < nvec: thread 0 enters at 769, thread 255 at 1024, a second trip never below 1793
        assert any(V % VEC[dt] and V > 256 for V in vs)
    assert _path(BF16, 50272) == "4-in-flight"


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
@pytest.mark.parametrize("k", range(10))
def test_A_vocabulary_sweep(k, dtype):
    V = _v_list(dtype)[k]
    x, lab = CrossEntropyRef.inputs(dtype, V, seed=SEED, device="cuda", ignore=IGNORE)
    _check(x, lab, f"A-{NAME[dtype]}-V{V}", f"A {_path(dtype, V)} {NAME[dtype]}")


def test_A_full_vocabulary():
    x, lab = CrossEntropyRef.inputs(BF16, 50272, seed=SEED, device="cuda", ignore=IGNORE)
    _check(x, lab, "A-bf16-V50272", "A 4-in-flight bf16")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
@pytest.mark.parametrize("V", [1001, 1025], ids=["odd", "vec"])
def test_A_shifted_and_dominant(V, dtype):
    V = V if V % 2 else V * VEC[dtype]
    x, lab = CrossEntropyRef.inputs(dtype, V, seed=SEED, device="cuda", ignore=IGNORE)
    shifted = (x.float() + 1e4).to(dtype)
    _check(shifted, lab, f"A-{NAME[dtype]}-V{V}-shift1e4", f"A {_path(dtype, V)} {NAME[dtype]}")
    x[4, V // 2] = 30.0                                               # row 4's label: loss ~ 0, the gradient row ~ 0
    got, ref = _check(x, lab, f"A-{NAME[dtype]}-V{V}-dominant", f"A {_path(dtype, V)} {NAME[dtype]}")
    assert ref.want["row_loss"][4].item() < 1e-6
    _check(x, lab, f"A-{NAME[dtype]}-V{V}-dloss1", f"A {_path(dtype, V)} {NAME[dtype]}", dloss=1.0)


# ------------------------------------------------------------------------------------------ B
LIVE_ROWS = (1, 3, 4)       # labels V - 1, an edge in the middle, V / 2: none of them on a -inf below


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
@pytest.mark.parametrize("where", ["first-vector", "odd-element-5", "inside-a-vector", "first-1024-vectors"])
def test_B_minus_inf_logits(where, dtype):
    vn = VEC[dtype]
    V = 1001 if where == "odd-element-5" else 2056 * vn
    x, lab = CrossEntropyRef.inputs(dtype, V, seed=SEED, device="cuda", ignore=IGNORE)
    ninf = float("-inf")
    rows = (1, 4) if where == "first-1024-vectors" else LIVE_ROWS     # (row 3's label, the edge 768 VN, lies inside that stretch)
    for r in rows:
        if where == "first-vector":
            x[r, :vn] = ninf
        elif where == "odd-element-5":
            x[r, 5] = ninf
        elif where == "inside-a-vector":
            x[r, vn + 2] = ninf
        else:
            x[r, :1024 * vn] = ninf                                   # every thread's first four vectors: the whole first trip folds nothing
    assert all(torch.isfinite(x[r, lab[r]].float()) for r in range(6) if lab[r] >= 0)
    got, ref = _check(x, lab, f"B-{NAME[dtype]}-V{V}-{where}", f"B {_path(dtype, V)} {NAME[dtype]}")
    assert bool(torch.isfinite(got["row_lse"]).all())
    assert ref.exact0[list(rows)].sum().item() >= len(rows)


# ------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
@pytest.mark.parametrize("V", [1001, 1025, 2056], ids=["odd", "1025-vectors", "2056-vectors"])
def test_C_in_place(V, dtype):
    V = V if V == 1001 else V * VEC[dtype]
    x, lab = CrossEntropyRef.inputs(dtype, V, seed=SEED, device="cuda", ignore=IGNORE)
    what = f"C-{NAME[dtype]}-V{V}-inplace"
    out, ref = _check(x, lab, what, f"C {_path(dtype, V)} {NAME[dtype]}", dloss=1.0, count=37)
    inp = _call(x, lab, 1.0, count=37, inplace=True)
    view = torch.int16 if dtype == BF16 else torch.int32
    assert torch.equal(inp["dlogits"].view(view), out["dlogits"].view(view)), f"{what}: in place differs from out of place"
    for name in ("row_lse", "row_loss", "loss_sum", "count"):
        assert torch.equal(inp[name], out[name])


# ------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_D_ignored_rows_and_determinism(dtype):
    V = 1025 * VEC[dtype]
    x, lab = CrossEntropyRef.inputs(dtype, V, seed=SEED, device="cuda", ignore=IGNORE)
    none = torch.full_like(lab, IGNORE)
    got, _ = _check(x, none, f"D-{NAME[dtype]}-V{V}-all-ignored", f"D {NAME[dtype]}")
    assert got["loss_sum"].item() == 0 and got["count"].item() == 0 and bool((got["dlogits"] == 0).all())
    odd = lab.clone()
    odd[0], odd[1], odd[4] = -5, V, V + 3                             # out of range: ignored, never an index
    got, ref = _check(x, odd, f"D-{NAME[dtype]}-V{V}-labels-out-of-range", f"D {NAME[dtype]}")
    assert got["count"].item() == 2 and ref.live.tolist() == [False, False, False, True, False, True]
    again = _call(x, odd, 1.7)
    view = torch.int16 if dtype == BF16 else torch.int32
    for name in got:
        assert torch.equal(again[name].view(view if name == "dlogits" else torch.int32), got[name].view(view if name == "dlogits" else torch.int32)), name
