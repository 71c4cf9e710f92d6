"""fp64 references of the streaming ops (csrc/llama_ops.hip, elementwise.hip): RoPE, SwiGLU, the activations, AdamW."""
import numpy as np
import torch

from bounds import U, VEC, check_bound, outside
from gemm_ref import GemmRef


# ------------------------------------------------------------------------------------------ streaming ops (csrc/llama_ops.hip, elementwise.hip)
TINY = 2.0 ** -126      # the smallest normal fp32: what a result flushed to zero, or an overflowed __expf's sigmoid of 0, can lose


class RopeRef:
    """fp64 reference of mmgl_rope_inplace / mmgl_rope (csrc/llama_ops.hip) over buf [rows, ld], on the operands' device: the row is
    `nall` column blocks of `unit` heads x D, the first `nblk` are rotated, the rest copied.  For pair (i, i + D/2) of a rotated head,
    with (c, s) the fp32 table entry cos_sin[row % T, i] and sigma = +1 forward / -1 backward:
        lo' = x0 c - sigma x1 s        mag = |x0 c| + |x1 s|
        hi' = x1 c + sigma x0 s        mag = |x1 c| + |x0 s|
        |got - want| <= u |want| + 3 * 2^-24 mag
    u |want| is the store's half ulp (bf16) or the last add's rounding counted once more (fp32); 3: the two products and the add (two
    with the contraction to an fma), each at most 2^-24 of mag.  The operands and the table are exact in fp32.  The unrotated blocks are
    compared bit for bit by the caller (`rotated` names the columns).
    Deliberately wrong references: `partner_shift` (the pair partner one 16-byte vector off, inside the head's half), `t_shift` (the
    position one off), backward not flipped (pass the other `backward`), the v block rotated (pass nblk = nall), `flat_table` (the table
    offset c * VN of the thread's chunk ignored: entry i % VN)."""

    @staticmethod
    def table(T, D, device="cpu"):
        """cos_sin fp32 [T, D/2, 2] of the usual angles t 10000^(-2i/D); T = 1 is the angle 0: (1, 0) exactly."""
        i = torch.arange(D // 2, dtype=torch.float64, device=device)
        ang = torch.arange(T, dtype=torch.float64, device=device)[:, None] * 10000.0 ** (-2 * i / D)[None, :]
        return torch.stack([ang.cos(), ang.sin()], -1).float().contiguous()

    @staticmethod
    def inputs(dtype, rows, ld, seed=0, device="cpu"):
        g = torch.Generator(device=device).manual_seed(seed)
        return torch.randn(rows, ld, generator=g, device=device).to(dtype)

    def __init__(self, x, cos_sin, T, unit, D, nblk, nall, backward=False, partner_shift=0, t_shift=0, flat_table=False):
        rows, half, vn = x.shape[0], D // 2, VEC[x.dtype]
        self.dtype, self.width = x.dtype, nall * unit * D
        X = x.detach()[:, :self.width].double().view(rows, nall * unit, 2, half)
        x0, x1 = X[:, :, 0], X[:, :, 1]
        p0, p1 = (x1, x0) if not partner_shift else (torch.roll(x1, -partner_shift * vn, -1), torch.roll(x0, -partner_shift * vn, -1))
        t = (torch.arange(rows, device=x.device) + t_shift) % T
        i = torch.arange(half, device=x.device)
        cs = cos_sin.detach().double()[t][:, i % vn if flat_table else i]          # [rows, half, 2]
        c, s = cs[:, None, :, 0], cs[:, None, :, 1] * (-1.0 if backward else 1.0)
        rot = (torch.arange(nall * unit, device=x.device) < nblk * unit)[None, :, None]
        want = torch.stack([torch.where(rot, x0 * c - p0 * s, x0), torch.where(rot, x1 * c + p1 * s, x1)], 2)
        mag = torch.stack([(x0 * c).abs() + (p0 * s).abs(), (x1 * c).abs() + (p1 * s).abs()], 2)
        self.want, self.mag = want.reshape(rows, self.width), torch.where(rot[:, :, None], mag, torch.zeros_like(mag)).reshape(rows, self.width)
        self.rotated = rot[:, :, None].expand(1, nall * unit, 2, half).reshape(self.width)

    def bound(self):
        return U[self.dtype] * self.want.abs() + 3 * 2.0 ** -24 * self.mag

    def outside(self, other):
        return outside(self.want, other.want, self.bound())

    def check(self, got, what, group=""):
        got = got.detach()[:, :self.width]
        r = check_bound(got, self.want, self.bound(), what, group)
        assert torch.equal(got[:, ~self.rotated], self.want[:, ~self.rotated].to(got.dtype)), f"{what}: an unrotated block is no bit-for-bit copy"
        return r


class SwigluRef:
    """fp64 reference of mmgl_swiglu_fwd / mmgl_swiglu_bwd (csrc/llama_ops.hip) over gu [M, 2F] = [gate | up] and dy [M, F], with
    s = sigmoid(g):
        y = g s u        du = dy g s        dg = dy u s (1 + g (1 - s))
    The kernel forms s = 1 / (1 + __expf(-g)) in fp32.  __expf is v_exp_f32 (1 ulp, 2^-23) on the product g log2(e) rounded to fp32
    (2^-24 |g| on the result); with a factor 2 of room, rel_e = 2^-22 + |g| 2^-23.  It reaches s through ds / s = -(1 - s) de / e; the
    add 1 + e and the division round s twice more.  Per element:
        y, du:  |got - want| <= u |want| + (4 * 2^-24 + (1 - s) rel_e) |want| + floor
                4: the two roundings of s and the two products.
        dg:     |got - want| <= u |want| + (8 * 2^-24 + 2 (1 - s) rel_e) mag + 2 * 2^-24 |g| |dy u| s + floor
                mag = |dy u| s (1 + |g| (1 - s)) >= |want|: at the root of silu' (g = -1.27846) want cancels and only mag is left.
                8: the three products and the two roundings of s on the result (5), the rounding of 1 - s, of g (1 - s) and of the sum
                (3, each at most 2^-24 (1 + |g| (1 - s))).  rel_e twice: through s and through 1 - s.
                2 * 2^-24 |g| |dy u| s: the cancellation.  For g in about [6, 20] s is within 2^-24 of 1, its two roundings are an
                ABSOLUTE 2 * 2^-24 s on 1 - s = e^-g, whatever its size, and the factor g multiplies them.
        floor = 2^-126 (1 + P): for g < -87 __expf(-g) overflows, s is 0 where sigmoid(g) < 2^-126, and a product below the smallest
                normal may be flushed.  P = |g u| + |u| (y), |dy g| + |dy| (du), |dy u| (1 + |g|) (dg).
    Deliberately wrong references: `swap` (gate and up exchanged), `no_gterm` (silu' without g (1 - s)), `up_pitch_f` (up read at row
    pitch F instead of 2F)."""

    ROOT = -1.2784645                       # silu'(g) = 0
    PLANTED_G = [ROOT] + [float(k) for k in range(6, 21)] + [float(k) for k in range(-104, -59, 4)] + [0.0, -0.0]

    @staticmethod
    def inputs(dtype, M, F, seed=0, device="cpu"):
        """gu [M, 2F] and dy [M, F] = randn * 4 with planted values, all finite, at evenly spread elements: the gates of PLANTED_G (the
        root of silu', a grid over [6, 20], a grid over [-104, -60], +0 and -0), then two zeros of u and two of dy.  A case with fewer
        than 68 elements plants half of its elements (the rest stay random), starting at planted value number M F + seed; every case
        from 68 elements on holds the whole list."""
        g = torch.Generator(device=device).manual_seed(seed)
        gu = torch.randn(M, 2 * F, generator=g, device=device) * 4
        dy = torch.randn(M, F, generator=g, device=device) * 4
        vals = SwigluRef.PLANTED_G + ["u", "u", "dy", "dy"]
        n = M * F
        k = min(max(n // 2, 1), len(vals))
        for j in range(k):
            e = j * (n // k)
            r, c = e // F, e % F
            val = vals[(j + (n + seed if k < len(vals) else 0)) % len(vals)]
            if val == "u":
                gu[r, F + c] = 0.0
            elif val == "dy":
                dy[r, c] = 0.0
            else:
                gu[r, c] = val
        return gu.to(dtype), dy.to(dtype)

    def __init__(self, gu, dy=None, swap=False, no_gterm=False, up_pitch_f=False):
        M, F = gu.shape[0], gu.shape[1] // 2
        self.dtype = gu.dtype
        G = gu.detach().double()
        g, u = G[:, :F], G[:, F:]
        if up_pitch_f:
            idx = torch.arange(M, device=gu.device)[:, None] * F + F + torch.arange(F, device=gu.device)[None, :]
            u = G.reshape(-1)[idx]
        if swap:
            g, u = u, g
        s = torch.sigmoid(g)
        one_s = torch.sigmoid(-g)                              # 1 - s without the cancellation
        rel_e = 2.0 ** -22 + g.abs() * 2.0 ** -23
        uu, r = U[self.dtype], 2.0 ** -24
        y = g * s * u
        self.want = dict(y=y)
        self._bound = dict(y=(uu + 4 * r + one_s * rel_e) * y.abs() + TINY * (1 + (g * u).abs() + u.abs()))
        if dy is not None:
            d = dy.detach().double()
            du = d * g * s
            fac = 1 + (0 if no_gterm else 1) * g * one_s
            dg = d * u * s * fac
            du_s = (d * u).abs() * s
            mag = du_s * (1 + g.abs() * one_s)
            self.want.update(du=du, dg=dg)
            self._bound.update(du=(uu + 4 * r + one_s * rel_e) * du.abs() + TINY * (1 + (d * g).abs() + d.abs()),
                               dg=uu * dg.abs() + (8 * r + 2 * one_s * rel_e) * mag + 2 * r * g.abs() * du_s + TINY * (1 + (d * u).abs() * (1 + g.abs())))

    def bound(self, name):
        return self._bound[name]

    def outside(self, other, name):
        return outside(self.want[name], other.want[name], self.bound(name))

    def err(self, got, name):
        return (got.detach().reshape(self.want[name].shape).double() - self.want[name]).abs()

    def check(self, got, name, what, group=""):
        return check_bound(got, self.want[name], self.bound(name), f"{what} {name}", group)


class ActRef:
    """fp64 reference of mmgl_activation_fwd (csrc/elementwise.hip) over n elements: GemmRef.ACT[act], within u |want| + E with
    GemmRef's evaluation term E = 2^-20 (|x| + |act(x)|) of the composed route for the three GELUs (0 for ReLU: a select).  `fn`
    replaces the activation (a deliberately wrong reference)."""

    PLANTED = [s * a for a in (0.0, 1e-30, 5.0, 9.0, 30.0, 100.0, 1e13, 1e20) for s in (1.0, -1.0)]

    @staticmethod
    def inputs(dtype, n, seed=0, device="cpu"):
        """randn * 3 with PLANTED (rounded to the dtype) over the leading elements, as many as fit, starting at value number n: the
        1 + erf cancellation (-5, -9), the cube overflowing inside tanh-GELU (1e13, 1e20), __expf overflowing inside quick-GELU (-100)."""
        g = torch.Generator(device=device).manual_seed(seed)
        x = torch.randn(n, generator=g, device=device) * 3
        k = min(n, len(ActRef.PLANTED))
        x[:k] = torch.tensor([ActRef.PLANTED[(j + (n if k < len(ActRef.PLANTED) else 0)) % len(ActRef.PLANTED)] for j in range(k)], device=device)
        return x.to(dtype)

    def __init__(self, x, act, fn=None):
        pre = x.detach().double().reshape(-1)
        self.dtype = x.dtype
        self.want = (fn or GemmRef.ACT[act])(pre)
        self._bound = U[x.dtype] * self.want.abs() + (2.0 ** -20 * (pre.abs() + self.want.abs()) if act >= 2 else 0.0)

    def bound(self):
        return self._bound

    def outside(self, other):
        return outside(self.want, other.want, self.bound())

    def check(self, got, what, group=""):
        return check_bound(got, self.want[:, None], self.bound()[:, None], what, group)


class AdamWRef:
    """fp64 reference of ONE step of mmgl_adamw_step (csrc/elementwise.hip) from the state the kernel was handed -- p (the fp32 master
    where there is one, else the parameter), m, v, g -- over the hyperparameters rounded to float32 as the C ABI receives them; the bias
    corrections bc1 = 1 - b1^step, bc2 = 1 - b2^step are the exact functions of those floats.  With gs = g grad_scale:
        m' = b1 m + (1 - b1) gs                            mag_m = |b1 m| + |(1 - b1) gs|
        v' = b2 v + (1 - b2) gs^2                          (no cancellation: v >= 0)
        p' = p (1 - lr wd) - upd,  upd = (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)
    Bounds, roundings of 2^-24 counted from adamw_kernel (`floor` = 2^-126, a result flushed below the smallest normal):
        m': 4 mag_m + floor     gs, 1 - b1, its product, the sum (b1 m: the product and the sum)
        v': 6 v' + floor        gs twice, 1 - b2, two products, the sum
        p': 4 |p| + 16 U + u_store |want| (+ U sqrt(floor) / (sqrt(bc2) den))
            U = (lr / bc1) mag_m / den, den = sqrt(v') / sqrt(bc2) + eps: the update with m' at its magnitude, because the 4 roundings of
            m' are relative to mag_m and pass through unchanged.  4 |p|: lr wd, 1 - lr wd, the product, the final subtraction.  16 U: bc1
            as a correctly rounded fp32 (1) and lr / bc1 (1), its product with m' (1), m' (4), the denominator (7: v' halved by the
            square root 3, sqrtf 1, bc2s as a correctly rounded fp32 1, the division 1, + eps 1), the division (1), the final
            subtraction (1).  u_store |want|: only for a bf16 parameter without a master (the one bf16 store); a master is fp32 and
            the bf16 parameter is its rounding, bit for bit (the caller compares).
    Deliberately wrong references: `decay_after`, `bc_step` (the bias corrections of another step), `no_bc2`, `no_grad_scale`,
    `eps_inside`, `bc` = (bc1, bc2s) given (the host's fp32 powf arithmetic)."""

    @staticmethod
    def f32(x):
        return float(np.float32(x))

    @staticmethod
    def bc_fp32(b1, b2, step):
        """bc1 and bc2s as 1.f - powf(beta, step) and sqrtf(1.f - powf(beta, step)) give them, restated in numpy float32."""
        one, st = np.float32(1), np.float32(step)
        return float(one - np.power(np.float32(b1), st)), float(np.sqrt(one - np.power(np.float32(b2), st)))

    PLANTED_G = (0.0, 1e-20, 1e4)

    @staticmethod
    def inputs(dtype, n, step, p_zero, seed=0, device="cpu"):
        """The state before step `step`: p fp32 (zeros, or randn), m and v zeros before step 1, else randn * 0.1 and rand * 0.01, g
        randn in `dtype` with PLANTED_G over its leading elements (as many as fit, starting at value number `step`)."""
        gen = torch.Generator(device=device).manual_seed(seed)
        r = lambda: torch.randn(n, generator=gen, device=device)
        p, m, v, g = r(), r() * 0.1, torch.rand(n, generator=gen, device=device) * 0.01, r()
        if p_zero:
            p.zero_()
        if step == 1:
            m.zero_(), v.zero_()
        k = min(n, 3)
        g[:k] = torch.tensor([AdamWRef.PLANTED_G[(j + step) % 3] for j in range(k)], device=device)
        return p, m, v, g.to(dtype)

    def __init__(self, p, m, v, g, lr, b1, b2, eps, wd, step, grad_scale=1.0, store_bf16=False, decay_after=False, bc_step=None,
                 no_bc2=False, no_grad_scale=False, eps_inside=False, bc=None):
        import math
        f = AdamWRef.f32
        lr, b1, b2, eps, wd, gsc = f(lr), f(b1), f(b2), f(eps), f(wd), f(grad_scale)
        d = lambda t: t.detach().double().reshape(-1)
        P, M, V, G = d(p), d(m), d(v), d(g)
        st = step if bc_step is None else bc_step
        bc1, bc2s = (1 - b1 ** st, math.sqrt(1 - b2 ** st)) if bc is None else bc
        if no_bc2:
            bc2s = 1.0
        gs = G if no_grad_scale else G * gsc
        t1, t2 = b1 * M, (1 - b1) * gs
        mn, mag_m = t1 + t2, t1.abs() + t2.abs()
        vn = b2 * V + (1 - b2) * gs * gs
        den = torch.sqrt(vn + eps) / bc2s if eps_inside else torch.sqrt(vn) / bc2s + eps
        upd, U = (lr / bc1) * mn / den, (lr / bc1) * mag_m / den
        want = (P - upd) * (1 - lr * wd) if decay_after else P * (1 - lr * wd) - upd
        r = 2.0 ** -24
        self.want = dict(m=mn, v=vn, p=want)
        self._bound = dict(m=4 * r * mag_m + TINY, v=6 * r * vn + TINY,
                           p=4 * r * P.abs() + 16 * r * U + U * math.sqrt(TINY) / (bc2s * den) + (2.0 ** -8 * want.abs() if store_bf16 else 0.0))

    def bound(self, name):
        return self._bound[name]

    def outside(self, other, name):
        return outside(self.want[name], other.want[name], self.bound(name))

    def err(self, got, name):
        return (got.detach().reshape(-1).double() - self.want[name]).abs()
