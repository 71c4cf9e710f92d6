"""tests/bounds.py on the CPU: check_bound fails for exactly the element pushed outside and names it, and a strided Slab tells a write
into its view from one into a pad column, an extra row or a guard."""
import pytest
import torch

from bounds import BF16, CANARY_BYTE, PAD, Slab, check_bound

ROW, COL = 1, 3


def _case(factor):
    g = torch.Generator().manual_seed(0)
    want = torch.randn(3, 5, generator=g, dtype=torch.float64)
    bound = torch.rand(3, 5, generator=g, dtype=torch.float64) + 0.5
    got = want + 0.25 * bound
    got[ROW, COL] = want[ROW, COL] + factor * bound[ROW, COL]
    return got, want, bound


def test_one_element_outside_is_named():
    got, want, bound = _case(1.01)
    with pytest.raises(AssertionError, match=rf"1 of 15 elements outside the bound \(max err/bound 1\.01\); rows \[{ROW}\], columns \[{COL}\]"):
        check_bound(got, want, bound, "case", "cpu")


def test_the_same_element_inside_passes():
    got, want, bound = _case(0.99)
    assert check_bound(got, want, bound, "case", "cpu") == pytest.approx(0.99, rel=1e-12)
    assert check_bound((got - want).abs(), None, bound, "case, error given", "cpu") == pytest.approx(0.99, rel=1e-12)


def test_nan_is_refused():
    got, want, bound = _case(0.99)
    got[2, 0] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        check_bound(got, want, bound, "case", "cpu")


def test_select_leaves_the_bad_element_out():
    got, want, bound = _case(1.01)
    got[0, 0] = float("nan")
    select = torch.ones(3, 5, dtype=torch.bool)
    select[ROW, COL] = select[0, 0] = False
    assert check_bound(got, want, bound, "case", "cpu", select=select) == pytest.approx(0.25, rel=1e-9)
    with pytest.raises(AssertionError, match="1 of 14 elements"):
        check_bound(got, want, bound, "case", "cpu", select=select | (torch.arange(5) == COL))


def test_strided_slab_tells_its_view_from_everything_around_it():
    rows, cols, ld, extra = 3, 5, 8, 2
    s = Slab((rows, cols), BF16, CANARY_BYTE, ld=ld, extra=extra, device="cpu")
    assert s.v.shape == (rows, cols) and s.v.stride() == (ld, 1) and s.buf.numel() == 2 * PAD + (rows + extra) * ld * 2
    assert s.unwritten() and s.untouched()
    s.v.fill_(1.0)
    assert s.untouched() and not s.unwritten()
    body = s.buf[PAD:-PAD].view(BF16).view(rows + extra, ld)
    for where, at in (("a pad column", body[1, cols:cols + 1]), ("an extra row", body[rows, :1]), ("the last extra row", body[rows + extra - 1, ld - 1:]),
                      ("the guard in front", s.buf[PAD - 1:PAD]), ("the guard behind", s.buf[-PAD:-PAD + 1])):
        kept = at.clone()
        at.zero_()
        assert not s.untouched(), where
        at.copy_(kept)
        assert s.untouched(), where
