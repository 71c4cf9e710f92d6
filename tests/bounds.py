"""What every per-element bound test shares: the store units, the one check of a bound on every element, the dropout hash of the
kernels restated, and tensors carved out of guarded buffers.  The references themselves are in the *_ref.py modules."""
import ctypes

import numpy as np
import torch

BF16, F32 = torch.bfloat16, torch.float32
NAME = {BF16: "bf16", F32: "f32"}
U = {BF16: 2.0 ** -8, F32: 2.0 ** -23}           # the half ulp of one round-to-nearest store
VEC = {BF16: 8, F32: 4}                          # elements of a 16-byte chunk
NAN = float("nan")
CANARY = -77.0                                   # exact in bf16
NAN_BYTE, CANARY_BYTE = 0xFF, 0xA5               # byte fills: 0xFF is NaN in both dtypes
PAD = 512                                        # bytes of guard on either side of a carved tensor (keeps the 16-byte alignment)


# ------------------------------------------------------------------------------------------ the check
def rows_columns(bad):
    if bad.shape[1] != 2:
        return f"indices {bad[:, 0].tolist()[:16]}"
    return f"rows {bad[:, 0].unique().tolist()[:16]}, columns {bad[:, 1].unique().tolist()[:16]}"


def tiles(bad):
    """The (row tile, column tile) pairs that hold the elements `bad` [k, 2], in the 256 and in the 128 tiling."""
    of = lambda tile: [tuple(t) for t in torch.div(bad, tile, rounding_mode="floor").unique(dim=0).tolist()][:24]
    return f"(row tile, column tile) of 256: {of(256)}; of 128: {of(128)}"


def sample_head_row(bad):
    """Of a [B,rows,heads,D] tensor, or of lse [B,H,T]."""
    return f"(sample, head, row) {(bad if bad.shape[1] == 3 else bad[:, [0, 2, 1]]).unique(dim=0).tolist()[:12]}"


def row_head(bad):
    return f"(row, head) {bad[:, :2].unique(dim=0).tolist()[:12]}"


def first_indices(bad):
    return f"first indices {bad[:8].tolist()}"


def check_bound(got, want, bound, what, group, where=None, select=None):
    """Asserts |got - want| <= bound on every element (select, bool: on those alone; want None: `got` already is the error) and that
    they are finite; prints and returns the largest err / bound.  A failure gives the count, the total, the worst ratio and
    where(bad), bad [k, ndim] the indices outside."""
    x = got.detach().double()
    if want is not None:
        x = x.reshape(want.shape)
    if select is not None:
        select = select.expand_as(x)
        x = torch.where(select, x, torch.zeros_like(x))
    assert torch.isfinite(x).all(), f"{what}: non-finite result"
    err = x.abs() if want is None else (x - want).abs()
    if select is not None:
        err = torch.where(select, err, torch.zeros_like(err))
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print(f"[bound {group}] {what}: max err/bound {ratio:.3f}")
    bad = (err > bound).nonzero()
    if bad.numel():
        total = err.numel() if select is None else int(select.sum())
        raise AssertionError(f"{what}: {bad.shape[0]} of {total} elements outside the bound (max err/bound {ratio:.2f}); "
                             f"{(where or rows_columns)(bad)}")
    return ratio


def check_bounds(items, what, group):
    """check_bound on every (name, got, want, bound, where, select) of `items`, as `what name`: the failures of all of them are
    collected before raising.  Returns the largest err / bound by name."""
    ratios, failed = {}, []
    for name, got, want, bound, where, select in items:
        try:
            ratios[name] = check_bound(got, want, bound, f"{what} {name}", group, where, select)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)
    return ratios


def outside(want, other_want, bound):
    """From two references alone: the elements (bool) at which `other_want` -- a deliberately wrong reference of the same call --
    leaves the bound around `want`."""
    return (other_want - want).abs() > bound


# ------------------------------------------------------------------------------------------ the kernels' dropout hash
_M64 = (1 << 64) - 1


def hash32_int(seed, i):
    """mmgl_hash32 (csrc/common.h: the splitmix64 finaliser, upper 32 bits) of one (seed, element index) pair in Python integers."""
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return ((z ^ (z >> 31)) & _M64) >> 32


def drop_threshold(p):
    """The kernels' uint32(fminf(p * 2^32, 2^32 - 1)) with p an fp32: an element is dropped when its hash is below it."""
    return min(int(float(np.float32(p)) * 4294967296.0), 4294967295)


def hash_keep(seed, n, p, start=0):
    """Keep mask (numpy bool [n]) of elements start ... start + n - 1 under (seed, p): mmgl_hash32 restated in numpy uint64, whose
    array arithmetic wraps around like the device's, against the kernels' threshold."""
    i = np.arange(n, dtype=np.uint64) + np.uint64(start)
    z = np.uint64(seed & _M64) + (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)) >= np.uint64(drop_threshold(p))


def _keep_scale(p):
    """The kernels' fp32 1.f / (1.f - p), as a Python float."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


# ------------------------------------------------------------------------------------------ carved buffers
def esz(dtype):
    return torch.empty((), dtype=dtype).element_size()


def code(dtype):
    """The ABI's dtype code."""
    from mmgl_amd import _lib
    return _lib.BF16 if dtype == BF16 else _lib.F32


def nan(*shape, dtype, device="cuda"):
    return torch.full(shape, NAN, dtype=dtype, device=device)


def bits(t):
    """The bit patterns of a bf16 / fp32 tensor as integers (NaN == NaN, -0 != +0); any other tensor as it is."""
    return t.contiguous().view({BF16: torch.int16, F32: torch.int32}.get(t.dtype, t.dtype))


def same(a, b):
    return torch.equal(bits(a), bits(b))


class Slab:
    """A tensor (.v) of `shape` carved out of a byte buffer (.buf) filled with `fill`: NaN around operands, a canary around and
    between outputs.  PAD bytes of guard lie on either side; with a row stride `ld` (elements) above the last dimension every row
    has pad columns, and `extra` more rows of ld follow the last.  `fill` is a value of `dtype`, or -- an int with a floating
    dtype -- a byte (NAN_BYTE, CANARY_BYTE).  `src` is copied into the view, which otherwise holds the fill as well."""

    def __init__(self, shape, dtype, fill, src=None, device="cuda", ld=None, extra=0):
        shape = tuple(shape)
        self.cols = shape[-1]
        self.rows = int(np.prod(shape[:-1]))
        self.ld = self.cols if ld is None else ld
        assert self.ld >= self.cols
        e = esz(dtype)
        byte = isinstance(fill, int) and dtype.is_floating_point
        self.unit = (torch.full((e,), fill, dtype=torch.uint8) if byte else torch.tensor([fill], dtype=dtype).view(torch.uint8)).to(device)
        self.nbytes = self.rows * self.ld * e
        self.buf = self.unit.repeat((self.nbytes + extra * self.ld * e + 2 * PAD) // e)
        self.v = self.buf[PAD:PAD + self.nbytes].view(dtype).view(*shape[:-1], self.ld)[..., :self.cols]
        if src is not None:
            self.v.copy_(src)

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + PAD)

    def _holds_fill(self, *parts):
        return bool((torch.cat([p.reshape(-1) for p in parts]).view(-1, self.unit.numel()) == self.unit).all())

    def untouched(self):
        """Nothing but the view's own elements differs from the fill: the guards, the pad columns, the extra rows."""
        e = self.unit.numel()
        body = self.buf[PAD:PAD + self.nbytes].view(self.rows, self.ld * e)
        return self._holds_fill(self.buf[:PAD], body[:, self.cols * e:], self.buf[PAD + self.nbytes:])

    def unwritten(self):
        """untouched(), and the view still holds the fill as well."""
        return self._holds_fill(self.buf)


class ByteSlab(Slab):
    """A workspace of nbytes of 0xFF (fp32 NaN) between two guards of 0xA5."""

    def __init__(self, nbytes, device="cuda"):
        super().__init__((nbytes,), torch.uint8, CANARY_BYTE, device=device)
        self.v.fill_(NAN_BYTE)

    def unwritten(self):
        return self.untouched() and bool((self.v == NAN_BYTE).all())
