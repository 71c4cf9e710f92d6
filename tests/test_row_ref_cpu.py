"""CPU: the comparisons of tests/test_norm_bounds_gpu.py, tests/test_cross_entropy_bounds_gpu.py and
tests/test_gated_residual_bounds_gpu.py can fail, and do not fail an honest kernel.  From row_ref.NormRef, CrossEntropyRef, GatedRef and
hash_keep alone (fp64, no kernel), at the inputs and the seed of the GPU files:

  * a deliberately wrong reference of each defect the row kernels could have -- a 16-byte chunk lost from the norm statistics or from
    m1 / m2, a row lost from dgamma / dbeta, dres left out, the dropout mask's element index one row (one element) off, a chunk lost
    from lse, the label one column off, the mean taken over rows instead of live rows, an ignored row treated as live -- leaves the
    bound of the right reference on at least 25 % of the elements of the tensor it should move; where the move is confined by
    construction (the label's two elements per row, the one ignored row) on exactly those elements;
  * hash_keep is a plain Python big-integer restatement of mmgl_hash32, bit for bit, element indices at and past 2^32 included;
  * the same operations in torch's fp32 arithmetic, stored in the operand dtype, stay inside every bound."""
import math

import numpy as np
import pytest
import torch

from bounds import BF16, F32, NAME, VEC, drop_threshold, hash32_int, hash_keep
from row_ref import CrossEntropyRef, GatedRef, NormRef

SEED = 0                                    # the GPU files' seed
NORM_SHAPES = [(BF16, 5, 512), (BF16, 5, 1032), (BF16, 5, 4104), (BF16, 5, 8192), (BF16, 125, 2056), (F32, 5, 260), (F32, 5, 4096), (F32, 125, 1028)]
CE_V = [(BF16, 1001), (BF16, 8192), (BF16, 16448), (F32, 1001), (F32, 4096), (F32, 8224)]
EPS = 1e-5


def _assert(frac, what, floor=0.25):
    print(f"[can fail] {what}: {frac:.1%} of the touched elements leave the bound")
    assert frac >= floor, f"{what}: only {frac:.1%} of the touched elements leave the bound"


def _frac(mask):
    return mask.double().mean().item()


def _tpr(dtype, cols):
    return 64 if cols // VEC[dtype] <= 256 else 256


def _middle_chunk_dropped(dtype, cols):
    vn = VEC[dtype]
    keep = torch.ones(cols, dtype=torch.bool)
    c0 = (cols // vn // 2) * vn
    keep[c0:c0 + vn] = False
    return keep


def _ids(v):
    return "-".join(NAME.get(x, str(x)) for x in v) if isinstance(v, tuple) else None


# ------------------------------------------------------------------------------------------ the hash
def test_hash_keep_is_the_big_integer_hash():
    for seed in (0, 1, 0x1234, 2 ** 63 + 12345, 2 ** 64 - 1):
        for start in (0, 1, 4095, 2 ** 31 - 2, 2 ** 32 - 2, 2 ** 32 + 7, 2 ** 40 + 3):
            for p in (0.3, 0.1, 0.999):
                want = [hash32_int(seed, start + k) >= drop_threshold(p) for k in range(5)]
                assert hash_keep(seed, 5, p, start=start).tolist() == want, (seed, start, p)
    assert drop_threshold(0.0) == 0 and drop_threshold(0.5) == 2 ** 31 and drop_threshold(0.3) == int(float(np.float32(0.3)) * 2 ** 32)
    assert hash_keep(7, 64, 0.0).all()
    k = hash_keep(7, 1 << 16, 0.3)
    assert abs(k.mean() - 0.7) < 0.01                       # (the density; the bits are held by the restatement above)


# ------------------------------------------------------------------------------------------ norms
def _norm_refs(dtype, rows, cols, rms, p=0.0, **kw):
    t = NormRef.inputs(dtype, rows, cols, seed=SEED)
    fwd = {k: kw.pop(k) for k in ("stat_cols", "mask_row_shift") if k in kw}
    ref = NormRef(t["x"], t["gamma"], None if rms else t["beta"], rms=rms, eps=EPS, res=t["res"] if p > 0 else None, p=p, seed=11, **fwd)
    return t, ref.backward(t["dy"], t["dres"], **kw)


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("shape", NORM_SHAPES, ids=_ids)
def test_norm_chunk_lost_from_the_statistics(shape, rms):
    dtype, rows, cols = shape
    _, ref = _norm_refs(dtype, rows, cols, rms)
    _, wrong = _norm_refs(dtype, rows, cols, rms, stat_cols=_middle_chunk_dropped(dtype, cols))
    what = f"{NAME[dtype]} {rows}x{cols} {'rms' if rms else 'ln'}: middle chunk lost from"
    _assert(_frac(ref.outside(wrong, "y")), f"{what} the statistics (y)")
    _assert(_frac(ref.outside(wrong, "rstd")), f"{what} the statistics (rstd)")
    if not rms:
        _assert(_frac(ref.outside(wrong, "mean")), f"{what} the statistics (mean)")
    _assert(_frac(ref.outside(wrong, "dx")), f"{what} m1 / m2 (dx)")


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("shape", NORM_SHAPES, ids=_ids)
def test_norm_row_lost_from_the_parameter_gradients(shape, rms):
    dtype, rows, cols = shape
    tpr = _tpr(dtype, cols)
    _, ref = _norm_refs(dtype, rows, cols, rms)
    for lost in (0, rows - 1):
        rows_in = torch.ones(rows, dtype=torch.bool)
        rows_in[lost] = False
        _, wrong = _norm_refs(dtype, rows, cols, rms, grad_rows=rows_in)
        for name in ("dgamma",) if rms else ("dgamma", "dbeta"):
            _assert(_frac(ref.outside(wrong, name, tpr)), f"{NAME[dtype]} {rows}x{cols} {'rms' if rms else 'ln'}: row {lost} lost from {name}")


@pytest.mark.parametrize("shape", NORM_SHAPES, ids=_ids)
def test_norm_dres_left_out_and_mask_one_row_off(shape):
    dtype, rows, cols = shape
    _, ref = _norm_refs(dtype, rows, cols, False, p=0.3)
    _, wrong = _norm_refs(dtype, rows, cols, False, p=0.3, no_dres=True)
    _assert(_frac(ref.outside(wrong, "dx")), f"{NAME[dtype]} {rows}x{cols}: dres left out (dx)")
    _, wrong = _norm_refs(dtype, rows, cols, False, p=0.3, mask_row_shift=1)
    _assert(_frac(wrong.s != ref.s), f"{NAME[dtype]} {rows}x{cols}: mask one row off (s, bit for bit)")
    _assert(_frac(ref.outside(wrong, "dx_drop")), f"{NAME[dtype]} {rows}x{cols}: mask one row off (dx_drop)")


def _norm_fp32(t, rms, p, seed, dtype):
    """The norm pair in torch's fp32 arithmetic with the kernels' stores: (s, y, mean, rstd, dx, dx_drop, dgamma, dbeta)."""
    x, res, g, b, dy, dres = (t[k].float() for k in ("x", "res", "gamma", "beta", "dy", "dres"))
    rows, cols = x.shape
    keep = None
    if p > 0:
        keep = torch.from_numpy(hash_keep(seed, rows * cols, p)).view(rows, cols)
        ks = float(np.float32(1) / (np.float32(1) - np.float32(p)))
        s = (ks * torch.where(keep, x, torch.zeros_like(x)).double() + res.double()).float().to(dtype)       # one fma
    else:
        s = (x + res).to(dtype)
    s32 = s.float()
    mu = torch.zeros(rows, 1) if rms else s32.mean(1, keepdim=True)
    rs = torch.rsqrt(((s32 - mu) ** 2).mean(1, keepdim=True) + EPS)
    y = (s32 - mu) * rs * g
    y = (y if rms else y + b).to(dtype)
    h, gy = (s32 - mu) * rs, dy * g
    m1 = torch.zeros(rows, 1) if rms else gy.mean(1, keepdim=True)
    dx = (rs * (gy - m1 - h * (gy * h).mean(1, keepdim=True)) + dres).to(dtype)
    dd = None if keep is None else torch.where(keep, dx.float() * ks, torch.zeros_like(x)).to(dtype)
    return s, y, mu[:, 0], rs[:, 0], dx, dd, (dy * h).sum(0), dy.sum(0)


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("shape", NORM_SHAPES, ids=_ids)
def test_norm_bound_holds_for_fp32_arithmetic(shape, rms, p):
    dtype, rows, cols = shape
    t = NormRef.inputs(dtype, rows, cols, seed=SEED)
    s, y, mu, rs, dx, dd, dg, db = _norm_fp32(t, rms, p, 11, dtype)
    ref = NormRef(t["x"], t["gamma"], None if rms else t["beta"], rms=rms, eps=EPS, res=t["res"], p=p, seed=11)
    ref.check_sum(s, "fp32 arithmetic")
    ref.backward(t["dy"], t["dres"])
    what, tpr = f"torch fp32 {NAME[dtype]} {rows}x{cols} {'rms' if rms else 'ln'} p={p}", _tpr(dtype, cols)
    got = dict(y=y, rstd=rs, dx=dx, dgamma=dg)
    if not rms:
        got.update(mean=mu, dbeta=db)
    if p > 0:
        got["dx_drop"] = dd
    for name, v in got.items():
        assert ref.check(v, name, what, "cpu", tpr) <= 1.0


def test_norm_chain_restates_the_backward_grid():
    assert NormRef.chain(5, 64) == 1 + 1 + 16 and NormRef.chain(5, 256) == 1 + 1 + 16
    assert NormRef.chain(2053, 64) == 2 + 256 + 16              # 512 blocks of 4 rows: 2048 partial rows, the last 5 rows a second trip
    assert NormRef.chain(517, 256) == 2 + 64 + 16 and NormRef.chain(512, 256) == 1 + 64 + 16
    assert NormRef.c(18) == 2.0 ** -16 and NormRef.c(274) == 548 * 2.0 ** -24


# ------------------------------------------------------------------------------------------ cross-entropy
@pytest.mark.parametrize("case", CE_V, ids=_ids)
def test_cross_entropy_wrong_references(case):
    dtype, V = case
    vn = VEC[dtype]
    x, lab = CrossEntropyRef.inputs(dtype, V, seed=SEED)
    ref = CrossEntropyRef(x, lab, dloss=1.7)
    what = f"{NAME[dtype]} V={V}"
    live = ref.live
    # a 16-byte chunk lost from lse: the first one (an edge at both of its ends)
    cols = torch.ones(V, dtype=torch.bool)
    cols[:vn] = False
    wrong = CrossEntropyRef(x, lab, dloss=1.7, lse_cols=cols)
    _assert(_frac(ref.outside(wrong, "row_lse")), f"{what}: first chunk lost from lse (row_lse)")
    _assert(_frac(ref.outside(wrong, "dlogits")[live]), f"{what}: first chunk lost from lse (dlogits of the live rows)")
    _assert(_frac(ref.outside(wrong, "row_loss")[live]), f"{what}: first chunk lost from lse (row_loss of the live rows)")
    # the label one column off: exactly the two elements of every live row
    wrong = CrossEntropyRef(x, lab, dloss=1.7, label_shift=1)
    out = ref.outside(wrong, "dlogits")
    touched = torch.zeros_like(out)
    for r in range(6):
        if live[r]:
            l = int(lab[r])
            touched[r, l] = touched[r, l + 1 if l + 1 < V else l - 1] = True
    assert torch.equal(out, touched), f"{what}: a label one column off must move its two elements per live row and nothing else"
    # the mean over rows instead of live rows
    wrong = CrossEntropyRef(x, lab, dloss=1.7, by_rows=True)
    assert not ref.outside(wrong, "dlogits")[~live].any()
    _assert(_frac(ref.outside(wrong, "dlogits")[live]), f"{what}: divided by rows instead of count (dlogits of the live rows)")
    # the ignored row treated as live: that row, and only it
    wrong = CrossEntropyRef(x, lab, dloss=1.7, live_row=2)
    out = ref.outside(wrong, "dlogits")
    assert not out[[0, 1, 3, 4, 5]].any() and ref.outside(wrong, "row_loss").tolist() == [False, False, True, False, False, False]
    _assert(_frac(out[2]), f"{what}: ignored row treated as live (its dlogits)", floor=0.99)


def _ce_fp32(x, lab, dloss, dtype, ignore=-100):
    x32 = x.float()
    V = x.shape[1]
    lse = torch.logsumexp(x32, 1)
    live = (lab != ignore) & (lab >= 0) & (lab < V)
    safe = torch.where(live, lab, torch.zeros_like(lab))
    loss = torch.where(live, lse - x32.gather(1, safe[:, None])[:, 0], torch.zeros_like(lse))
    scale = np.float32(dloss) / np.float32(max(int(live.sum()), 1))
    g = torch.exp(x32 - lse[:, None])
    g[torch.arange(6), safe] -= 1.0
    g = torch.where(live[:, None], g * float(scale), torch.zeros_like(g)).to(dtype)
    return lse, loss, loss.sum().reshape(1), live.sum().float().reshape(1), g


@pytest.mark.parametrize("case", [c + (False,) for c in CE_V + [(BF16, 3), (F32, 1)]] + [c + (True,) for c in CE_V], ids=_ids)
def test_cross_entropy_bound_holds_for_fp32_arithmetic(case):
    dtype, V, ninf = case
    x, lab = CrossEntropyRef.inputs(dtype, V, seed=SEED)
    if ninf:
        x[:, 8:16] = float("-inf")
        x[1, 33] = float("-inf")
    lse, loss, lsum, cnt, g = _ce_fp32(x, lab, 1.7, dtype)
    ref = CrossEntropyRef(x, lab, dloss=1.7)
    what = f"torch fp32 {NAME[dtype]} V={V}{' -inf' if ninf else ''}"
    for name, v in dict(row_lse=lse, row_loss=loss, loss_sum=lsum, count=cnt, dlogits=g).items():
        assert ref.check(v, name, what, "cpu") <= 1.0
    assert (g[ref.exact0] == 0).all()


# ------------------------------------------------------------------------------------------ gated residual
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_gated_mask_one_element_off_and_fp32_arithmetic(dtype):
    n = 4099
    g = torch.Generator().manual_seed(SEED)
    res, x, dy = (torch.randn(n, generator=g).to(dtype) for _ in range(3))
    gate = torch.tensor(0.7)
    for p in (0.0, 0.3):
        ref = GatedRef(res, x, gate, p, seed=5).backward(dy)
        tg = torch.tanh(gate).item()
        inv = float(np.float32(1) / (np.float32(1) - np.float32(p))) if p else 1.0
        keep = torch.from_numpy(hash_keep(5, n, p))
        kx = torch.where(keep, x.float(), torch.zeros(n))
        y = (res.float() + np.float32(np.float32(tg) * np.float32(inv)).item() * kx).to(dtype)
        dx = (torch.where(keep, dy.float(), torch.zeros(n)) * (tg * inv)).to(dtype)
        dgate = ((1 - tg * tg) * (dy.float() * kx * inv).sum()).reshape(1)
        for name, v in dict(y=y, dx=dx, dgate=dgate).items():
            assert ref.check(v, name, f"torch fp32 {NAME[dtype]} n={n} p={p}", "cpu") <= 1.0
    wrong = GatedRef(res, x, gate, 0.3, seed=5, index_shift=1).backward(dy)
    _assert(_frac(ref.outside(wrong, "y")), f"{NAME[dtype]}: mask one element off (y)")
    _assert(_frac(ref.outside(wrong, "dx")), f"{NAME[dtype]}: mask one element off (dx)")
    assert GatedRef.blocks(5, 8) == 1 and GatedRef.blocks(256 * 8 * 2048 + 3, 8) == 2048 and GatedRef.blocks(256 * 4 * 2048 + 3, 4) == 2048
    assert GatedRef.chain(256 * 8 * 2048 + 3, 8) == 8 + 3 + 6 + 4 + 8 + 8 and GatedRef.chain(5, 8) == 0 + 5 + 6 + 4 + 1 + 8


# ------------------------------------------------------------------------------------------ the report
def test_check_names_rows_and_columns():
    t = NormRef.inputs(BF16, 5, 512, seed=SEED)
    ref = NormRef(t["x"], t["gamma"], t["beta"], eps=EPS)
    got = ref.want["y"].clone()
    assert ref.check(got.to(BF16), "y", "rounded reference") <= 1.0
    got[3, 77] += 1.0
    with pytest.raises(AssertionError, match=r"1 of 2560 elements outside the bound.*rows \[3\], columns \[77\]"):
        ref.check(got.to(BF16), "y", "planted")
    got[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        ref.check(got.to(BF16), "y", "nan")
    with pytest.raises(AssertionError, match="bit for bit"):
        ref.check_sum(t["x"] + 1, "sum")
    assert math.isclose(ref.bound("mean")[0].item(), 2.0 ** -18 * t["x"][0].double().abs().mean().item())
