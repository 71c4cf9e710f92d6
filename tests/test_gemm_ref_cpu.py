"""CPU: the comparison of tests/test_gemm_bounds_gpu.py and tests/test_linear_bwd_bounds_gpu.py can fail.  From gemm_ref.GemmRef alone
(fp64, no kernel): a deliberately wrong reference of each defect the GEMM family could have -- a K unit or a K split lost or folded
twice, a bias line of another tile, a residual or zmask row offset lost in the tail rows of a row split, the scale on the wrong side
of the activation, a transposed operand, contraction rows lost from a weight gradient, `accumulate` ignored or applied twice, a row
split lost from a bias gradient, mask_dx taken from x >= 0 -- leaves the bound of the right reference on at least 25 % of the
elements the defect touches, at the seed and the contraction lengths of the GPU cases (M and N cut to a few tiles: the per-element
statistics depend on the contraction length only).  The bound is taken in bf16, the wider of the two."""
import pytest
import torch

from bounds import BF16
from gemm_ref import GemmRef

SEED = 0                                    # the GPU files' seed
KS = (256, 384, 1536, 3072, 4096)           # contraction lengths of the forward GPU cases on the fused routes
M, N, M1 = 384, 512, 256                    # two tile rows (the second one the "tail" of a row split), two 256-column tiles


def _frac(ref, wrong, n, touched=None, **kw):
    out = ref.outside(wrong, BF16, n, **kw)
    if touched is not None:
        out = out[touched.expand_as(out)]
    return out.double().mean().item()


def _assert(frac, what):
    print(f"[can fail] {what}: {frac:.1%} of the touched elements leave the bound")
    assert frac >= 0.25, f"{what}: only {frac:.1%} of the touched elements leave the bound"


def _split(K, s, sp):
    """K range of split sp of s (gemm8p_kernel's item_origin: whole 128-wide units, the first K / 128 % s splits one unit longer)."""
    units = K // 128
    base, rem = units // s, units % s
    k0 = (sp * base + min(sp, rem)) * 128
    return k0, k0 + (base + (1 if sp < rem else 0)) * 128


@pytest.fixture(scope="module")
def ops():
    return {K: GemmRef.inputs(BF16, M, N, K, seed=SEED) for K in KS}


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("drop", [64, 128])
@pytest.mark.parametrize("K", KS)
def test_dropped_k_columns(ops, K, drop, act):
    t = ops[K]
    kw = dict(bias=t["bias"], act=act, residual=t["residual"])
    ref = GemmRef.forward(t["x"], t["w"], **kw)
    wrong = GemmRef.forward(t["x"], t["w"], K=K - drop, **kw)
    _assert(_frac(ref, wrong, GemmRef.chain(BF16, K)), f"K={K} act={act}: the last {drop} K columns dropped")


@pytest.mark.parametrize("K,s,sp", [(1536, 3, 1), (3072, 8, 7), (4096, 3, 0), (4096, 3, 2)])
@pytest.mark.parametrize("times", [0.0, 2.0], ids=["missing", "twice"])
def test_k_split_missing_or_counted_twice(ops, K, s, sp, times):
    t = ops[K]
    k0, k1 = _split(K, s, sp)
    x2 = t["x"].clone()
    x2[:, k0:k1] *= times                      # exact in bf16
    kw = dict(bias=t["bias"], act=1, scale=0.125, zmask=t["zmask"], residual=t["residual"])
    ref, wrong = GemmRef.forward(t["x"], t["w"], **kw), GemmRef.forward(x2, t["w"], **kw)
    touched = (t["zmask"].double() > 0)        # the finish kernel zeroes the others whatever the sum was
    _assert(_frac(ref, wrong, GemmRef.chain(BF16, K, s), touched), f"K={K}: split {sp} of {s} {'missing' if not times else 'counted twice'}")


@pytest.mark.parametrize("shift", [256, -256], ids=["shifted-one-tile", "other-parity"])
@pytest.mark.parametrize("K", KS)
def test_bias_of_another_tile(ops, K, shift):
    t = ops[K]
    ref = GemmRef.forward(t["x"], t["w"], bias=t["bias"], scale=0.125)
    wrong = GemmRef.forward(t["x"], t["w"], bias=t["bias"].roll(shift), scale=0.125)
    _assert(_frac(ref, wrong, GemmRef.chain(BF16, K)), f"K={K}: bias of columns n {'-' if shift > 0 else '+'} 256")


@pytest.mark.parametrize("which", ["residual", "zmask"])
@pytest.mark.parametrize("K", KS)
def test_tail_rows_read_one_row_off(ops, K, which):
    t = ops[K]
    # (no ReLU here: with one, half of the elements are zero under either mask and a wrong zmask row shows on a quarter of the rest)
    kw = dict(bias=t["bias"], act=0, scale=0.125, zmask=t["zmask"], residual=t["residual"])
    off = t[which].clone()
    off[M1:] = t[which][M1:].roll(-1, 0)
    ref, wrong = GemmRef.forward(t["x"], t["w"], **kw), GemmRef.forward(t["x"], t["w"], **{**kw, which: off})
    touched = (torch.arange(M) >= M1)[:, None]
    assert not ref.outside(wrong, BF16, GemmRef.chain(BF16, K))[:M1].any()
    _assert(_frac(ref, wrong, GemmRef.chain(BF16, K), touched), f"K={K}: {which} one row off in the tail rows")


@pytest.mark.parametrize("act", [2, 3, 4])
@pytest.mark.parametrize("scale", [0.125, 0.3])
def test_scale_after_the_activation(ops, act, scale):
    t = ops[1536]
    ref = GemmRef.forward(t["x"], t["w"], bias=t["bias"], act=act, scale=scale)
    wrong = GemmRef.forward(t["x"], t["w"], bias=t["bias"], act=act, scale=scale, scale_after=True)
    _assert(_frac(ref, wrong, GemmRef.chain(BF16, 1536)), f"act={act} scale={scale}: scale applied after the activation")


def test_operand_transposed():
    t = GemmRef.inputs(BF16, 256, 256, 256, seed=SEED)
    ref = GemmRef.forward(t["x"], t["w"], bias=t["bias"])
    wrong = GemmRef.forward(t["x"], t["w"].t().contiguous(), bias=t["bias"])
    _assert(_frac(ref, wrong, GemmRef.chain(BF16, 256)), "W read transposed")


# ------------------------------------------------------------------------------------------ backward
ROWS = (256, 2048, 2560)                    # contraction lengths (rows M) of the weight / bias gradient GPU cases
NB, KB = 256, 128                           # out / in features


@pytest.fixture(scope="module")
def bops():
    return {m: GemmRef.inputs(BF16, m, NB, KB, seed=SEED) for m in ROWS}


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("rows", ROWS)
def test_wgrad_missing_the_last_128_rows(bops, rows, relu):
    t = bops[rows]
    y = t["y"] if relu else None
    ref = GemmRef.wgrad(t["dy"], t["x"], y, 0.125)
    wrong = GemmRef.wgrad(t["dy"][:-128], t["x"][:-128], None if y is None else y[:-128], 0.125)
    _assert(_frac(ref, wrong, GemmRef.chain(BF16, rows, 4)), f"M={rows} relu={relu}: weight gradient without its last 128 rows")


@pytest.mark.parametrize("times", [0.0, 2.0], ids=["ignored", "twice"])
@pytest.mark.parametrize("rows", ROWS)
def test_accumulate_ignored_or_applied_twice(bops, rows, times):
    t = bops[rows]
    ref = GemmRef.wgrad(t["dy"], t["x"], t["y"], 0.125, prior=t["prior_w"])
    wrong = GemmRef.wgrad(t["dy"], t["x"], t["y"], 0.125, prior=t["prior_w"].double() * times)
    _assert(_frac(ref, wrong, GemmRef.chain(BF16, rows, 4)), f"M={rows}: weight gradient, accumulate {'ignored' if not times else 'applied twice'}")
    ref = GemmRef.dbias(t["dy"], t["y"], 0.125, prior=t["prior_b"])
    wrong = GemmRef.dbias(t["dy"], t["y"], 0.125, prior=t["prior_b"].double() * times)
    _assert(_frac(ref, wrong, GemmRef.chain(BF16, rows, 64)), f"M={rows}: bias gradient, accumulate {'ignored' if not times else 'applied twice'}")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("rows,splits", [(256, 2), (2560, 20)])
def test_dbias_missing_one_row_split(bops, rows, splits, relu):
    t = bops[rows]
    y = t["y"] if relu else None
    per = -(-rows // splits)
    dy2 = t["dy"].clone()
    dy2[(splits - 1) * per:] = 0
    ref, wrong = GemmRef.dbias(t["dy"], y, 0.125), GemmRef.dbias(dy2, y, 0.125)
    _assert(_frac(ref, wrong, GemmRef.chain(BF16, rows, 16 + splits)), f"M={rows} relu={relu}: bias gradient without its last row split of {splits}")


@pytest.mark.parametrize("relu", [False, True])
def test_mask_dx_from_x_ge_0(bops, relu):
    t = bops[256]
    y = t["y"] if relu else None
    ref = GemmRef.dgrad(t["dy"], t["w"], y, 0.125, x_mask=t["xr"])
    wrong = GemmRef.dgrad(t["dy"], t["w"], y, 0.125, x_mask=t["xr"], mask_ge=True)
    touched = t["xr"].double() == 0
    assert 0.3 < touched.double().mean().item() < 0.7
    _assert(_frac(ref, wrong, GemmRef.chain(BF16, NB), touched), f"relu={relu}: mask_dx from x >= 0")


# ------------------------------------------------------------------------------------------ the bound itself
def test_bound_terms():
    """What bound() is made of: the constants of the docstring, the staged terms only on the composed route, and a tile report that
    names the tile of a planted error."""
    assert GemmRef.chain(BF16, 4096, 3) == 256 + 3 + 8 and GemmRef.chain(torch.float32, 100) == 25 + 8
    assert GemmRef.c(8) == 2.0 ** -16 and GemmRef.c(267) == 534 * 2.0 ** -24
    t = GemmRef.inputs(BF16, 300, 264, 64, seed=SEED)
    ref = GemmRef.forward(t["x"], t["w"], bias=t["bias"], act=3, residual=t["residual"], zmask=t["zmask"])
    n = GemmRef.chain(BF16, 64)
    plain, staged = ref.bound(BF16, n), ref.bound(BF16, n, composed=True, has_act_pass=True, has_residual_pass=True)
    assert torch.allclose(staged - plain, 2.0 ** -8 * (1.10 * ref.pre.abs() + ref.masked_act.abs()), rtol=1e-9, atol=0)
    assert torch.allclose(ref.bound(BF16, n, dyp_rounded=True) - plain, 2.0 ** -8 * ref.mag, rtol=1e-9, atol=0)
    got = ref.want.clone()
    assert ref.check(got.to(BF16), "rounded reference") <= 1.0
    got[299, 260] += 1.0
    with pytest.raises(AssertionError, match=r"1 of 79200 elements.*of 256: \[\(1, 1\)\]; of 128: \[\(2, 2\)\]"):
        ref.check(got.to(BF16), "planted")
    got[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        ref.check(got.to(BF16), "nan")
