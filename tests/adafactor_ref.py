"""fp64 reference of the fused Adafactor step (csrc/adafactor.hip, mmgl_adafactor_step), its per-element bound, deliberately wrong
references, the shared test shapes and an emulation of the kernel's arithmetic (fp32 elementwise, sums and moving averages in double)."""
import math

import numpy as np
import torch

from bounds import BF16, F32, U, outside

TINY = 2.0 ** -126
R24 = 2.0 ** -24                 # one fp32 rounding
TR, TC = 64, 256                 # the kernel's tile: rows, columns (a 1-D tensor: runs of TR * TC elements)
WRONG = ("no_eps1", "mean_as_sum", "row_col_swapped", "no_clip", "clip_always", "beta_of_other_step", "no_grad_scale", "row_mean_dropped")

# the shapes every test shares: the degenerate ones, odd C ragged in both tile directions, one below / at / one above the row tile and
# the column tile, several workgroups in both directions, a 1-D tensor of several workgroups, two all-zero gradients
SHAPES = [(1, 8), (8, 1), (32, 6), (7,), (1,), (257, 131), (TR - 1, 5), (TR, 5), (TR + 1, 5), (3, TC - 1), (3, TC), (3, TC + 1),
          (2 * TR + 2, 2 * TC + 3), (2 * TR * TC + 5,), (16, 12), (9,)]
ZERO_GRAD = {14, 15}             # indices into SHAPES whose gradient is all zero
PLANTED = {5, 13}                # indices whose leading gradients are PLANTED_G
PLANTED_G = (0.0, 1e-20, 1e4)


def cdiv(a, b):
    return (a + b - 1) // b


def f32(x):
    return float(np.float32(x))


def inputs(dtype, step, seed=0, state_scale=1.0, shapes=SHAPES, device="cpu"):
    """Per tensor dict(shape, p fp32, g in `dtype`, state: (row, col) or (v,) fp32): the state before step `step` -- zeros before step 1,
    else (0.5 + rand) * state_scale (positive).  ZERO_GRAD tensors have g = 0, PLANTED ones start with PLANTED_G."""
    gen = torch.Generator(device=device).manual_seed(seed)
    out = []
    for i, shape in enumerate(shapes):
        p = torch.randn(*shape, generator=gen, device=device)
        g = torch.randn(*shape, generator=gen, device=device)
        if shapes is SHAPES and i in ZERO_GRAD:
            g.zero_()
        if shapes is SHAPES and i in PLANTED:
            g.view(-1)[:3] = torch.tensor([PLANTED_G[(j + step) % 3] for j in range(3)], device=device)
        sizes = (shape[0], shape[1]) if len(shape) == 2 else (shape[0],)
        state = tuple(torch.zeros(s, device=device) if step == 1 else (0.5 + torch.rand(s, generator=gen, device=device)) * state_scale
                      for s in sizes)
        out.append(dict(shape=shape, p=p, g=g.to(dtype), state=state))
    return out


class AdafactorRef:
    """fp64 reference of ONE step of mmgl_adafactor_step for ONE tensor from the state the kernel was handed -- p (the fp32 master where
    there is one, else the parameter), the gradient, row | col (2-D) or v (1-D) -- over lr, eps1, clip, weight_decay and grad_scale rounded
    to float32 as the C ABI receives them; decay_rate is a double there.  pw = step^decay_rate, b2 = 1 - pw, gs = g grad_scale,
    x = gs^2 + eps1:
        2-D: row' = b2 row + pw mean_j x     col' = b2 col + pw mean_i x     u = (rsqrt(row'_i / mean(row')) rsqrt(col'_j)) gs
        1-D: v' = b2 v + pw x                u = gs rsqrt(v')
        d = max(1, sqrt(mean u^2) / clip)    upd = lr u / d    p1 = p + (-lr wd) p    p' = p1 - upd

    Bounds: roundings r = 2^-24 counted from the kernel's statements.  The kernel accumulates every sum in double, keeps the partials as
    doubles in the workspace and forms row', col', v' in double from the fp32 operands, rounded to fp32 once; `dbl` = 1 stands for all the
    double operations of one chain (2^-53 each, at most 2^31 of them: far below one fp32 rounding).
        2-D x:  4        gs (1), its square (2 through gs, 1 the product), + eps1 (1), in fp32: 4 in all, rounded up from 1 + 2 + 1
        row':   K_row = 4 + dbl + 1 + 1 = 7     x; the sums, the mean and the moving average in double; pw (or b2) as an fp32; the one store
        col':   K_col = 7                       the same chain over the rows
        v':     K_v = 2 + dbl + 1 + 1 = 5       gs squared in double (2 through gs); as above
                + 2^-126 for a flushed product
        mean(row'): K_mean = K_row + dbl + 1    the sum of the stored rows in double; the mean stored
        u:      K_u = (K_row + K_mean + 1) / 2 + 2 + K_col / 2 + 2 + 3    the quotient, rsqrt halves its argument's error and adds 2 of its
                own (1 ulp); rsqrt(col'); the product of the factors, gs, the product with it.    1-D: K_u = K_v / 2 + 2 + 2
        d:      K_d = (2 K_u + 1 + dbl + 1) / 2 + 1 + 1    u^2 in fp32; its sum in double; sum / numel stored; the square root halves and
                adds 1; / clip 1.  max(1, .) does not enlarge an error.
        upd:    K_upd = K_u + K_d + 2     the quotient and the product with lr
        p':     store |p'| + r (|p1| + 2 |lr wd p|) + K_upd r |upd| + 2^-126      store = bounds.U of the dtype that holds the result (the last
                subtraction IS the fp32 store; a bf16 parameter without a master is rounded once more, which U[bf16] covers); p1's add;
                -lr wd rounded and its product.
    Deliberately wrong references (`wrong`): no_eps1, mean_as_sum (row' and col' from sums), row_col_swapped (square tensors: the means
    over the other axis), no_clip (d = 1), clip_always (d = rms / clip), beta_of_other_step (step + 1), no_grad_scale,
    row_mean_dropped (rsqrt(row'_i) alone)."""

    def __init__(self, p, g, state, lr, step, grad_scale=1.0, weight_decay=0.0, eps1=1e-30, clip=1.0, decay_rate=-0.8, store=F32, wrong=None):
        assert wrong is None or wrong in WRONG
        lr, gsc, wd, eps1, clip = f32(lr), f32(grad_scale), f32(weight_decay), f32(eps1), f32(clip)
        P, G = p.detach().double(), g.detach().double()
        shape = tuple(P.shape)
        pw = float(step + (wrong == "beta_of_other_step")) ** decay_rate
        b2 = 1.0 - pw
        gs = G if wrong == "no_grad_scale" else G * gsc
        x = gs * gs + (0.0 if wrong == "no_eps1" else eps1)
        self.want, self._bound = {}, {}
        if len(shape) == 2:
            R, C = shape
            row0, col0 = (s.detach().double() for s in state)
            mr, mc = (x.sum(-1), x.sum(-2)) if wrong == "mean_as_sum" else (x.mean(-1), x.mean(-2))
            if wrong == "row_col_swapped":
                assert R == C
                mr, mc = mc, mr
            row, col = b2 * row0 + pw * mr, b2 * col0 + pw * mc
            k_row = k_col = 4 + 1 + 1 + 1
            k_mean = k_row + 1 + 1
            k_u = (k_row + k_mean + 1) / 2 + 2 + k_col / 2 + 2 + 3
            rfac = row.rsqrt() if wrong == "row_mean_dropped" else (row / row.mean()).rsqrt()
            u = (rfac[:, None] * col.rsqrt()[None, :]) * gs
            self.want.update(row=row, col=col)
            self._bound.update(row=k_row * R24 * row + TINY, col=k_col * R24 * col + TINY)
        else:
            v = b2 * state[0].detach().double() + pw * x
            k_u = 5 / 2 + 2 + 2
            u = gs * v.rsqrt()
            self.want.update(v=v)
            self._bound.update(v=5 * R24 * v + TINY)
        rms = math.sqrt(float((u * u).mean()))
        self.rms = rms
        self.d = 1.0 if wrong == "no_clip" else rms / clip if wrong == "clip_always" else max(1.0, rms / clip)
        k_d = (2 * k_u + 1 + 1 + 1) / 2 + 1 + 1
        k_upd = k_u + k_d + 2
        upd = lr * u / self.d
        p1 = P - lr * wd * P
        want = p1 - upd
        self.want["p"] = want
        self._bound["p"] = U[store] * want.abs() + R24 * (p1.abs() + 2 * (lr * wd * P).abs()) + k_upd * R24 * upd.abs() + TINY
        self.k = dict(u=k_u, d=k_d, upd=k_upd)

    def bound(self, name):
        return self._bound[name]

    def outside(self, other, name):
        return outside(self.want[name], other.want[name], self.bound(name))

    def err(self, got, name):
        return (got.detach().double().reshape(self.want[name].shape) - self.want[name]).abs()


# ------------------------------------------------------------------------------------------ the kernel's arithmetic in torch
def emulate_fp32(p, g, state, lr, step, grad_scale=1.0, weight_decay=0.0, eps1=1e-30, clip=1.0, decay_rate=-0.8):
    """One tensor's step on the CPU as the kernel computes it: the elementwise arithmetic in torch float32 (products and sums rounded one
    by one: the device may contract some into an fma, which only drops roundings), every sum and the moving averages in double over the
    fp32 operands, rounded to fp32 where the kernel stores a float.  Returns dict(p, row, col) or dict(p, v)."""
    t32 = lambda v: torch.tensor(v, dtype=torch.float32)
    pw = float(step) ** decay_rate
    b2, omb2, lr_, wdlr = t32(1.0 - pw).double(), t32(pw).double(), t32(lr), t32(-float(f32(weight_decay)) * float(f32(lr)))
    gs = g.float() * t32(grad_scale)
    out = {}
    if g.dim() == 2:
        R, C = g.shape
        x = (gs * gs + t32(eps1)).double()
        row = (b2 * state[0].double() + omb2 * (x.sum(1) / C)).float()
        col = (b2 * state[1].double() + omb2 * (x.sum(0) / R)).float()
        mean = (row.double().sum() / R).float()
        u = ((row / mean).rsqrt()[:, None] * col.rsqrt()[None, :]) * gs
        out.update(row=row, col=col)
    else:
        v = (b2 * state[0].double() + omb2 * (gs.double() * gs.double() + float(t32(eps1)))).float()
        u = gs * v.rsqrt()
        out.update(v=v)
    d = torch.clamp(((u * u).double().sum() / g.numel()).float().sqrt() / t32(clip), min=1.0)
    pf = p.float()
    if float(wdlr) != 0.0:
        pf = pf + wdlr * pf
    out["p"] = pf - (u / d) * lr_
    return out
