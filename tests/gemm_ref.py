"""fp64 reference of the GEMM family (csrc/gemm*.hip) and the dispatch plans of csrc/gemm.hip and csrc/gemm8p.hip, restated."""
import torch

from bounds import BF16, U, check_bound, outside, tiles


# ------------------------------------------------------------------------------------------ the GEMM family (csrc/gemm*.hip)
class GemmRef:
    """fp64 reference of one product of the GEMM family on the device the (storage-rounded) operands live on (or the CPU):
        forward   want = act((x[:, :K] W[:, :K]^T + bias) * scale), zeroed where zmask <= 0, + residual
                  mag  = (|x| |W|^T + |bias|) * |scale| + |residual|
        dgrad     want = dyp W, zeroed where x_mask <= 0 (mask_dx)          mag = |dyp| |W|
        wgrad     want = dyp^T x + prior (accumulate)                       mag = |dyp|^T |x| + |prior|
        dbias     want = column sums of dyp + prior                         mag = column sums of |dyp| + |prior|
    with dyp = dy * scale * (y > 0) (y: the operand the call is given; None: no activation) in all three.

    Per-element bound (every element is checked; none is weighted out near a ReLU kink: a pre-activation within c mag of zero moves
    the output by at most c mag), a function of the reference alone, never of the kernel's output:
        |got - want| <= u |want| + L c mag + E + staged                     u = 2^-8 (bf16) or 2^-23 (fp32)
      * u |want| is the half ulp of the one round-to-nearest store of the fp32 result; rounding alone reaches it.
      * c = max(2^-16, 2 n 2^-24): n fp32 roundings of 2^-24 on the magnitude sum, with a factor 2 of room.  n is the longest chain
        of the case (GemmRef.chain): contraction length / kb -- the accumulator is rounded once per MFMA k-block; kb = 16 for the bf16
        MFMAs (16x16x32 counts as two, 32x32x16 as one), kb = 4 for mfma_f32_16x16x4f32 -- plus the number of partial tiles or
        partial sums that are folded (K splits of the persistent kernels, row splits of the bias gradient and its 16-slot LDS fold)
        plus 8 for the epilogue: bias add, scale, the activation's own arithmetic (E below counts its evaluation), residual add, the
        accumulate add, the fold's scale.  2^-16 is SkinnyRef's floor: it also covers a rounding decision the summation order flips.
      * L is the activation's Lipschitz constant, through which the pre-activation error passes: 1 for none / ReLU, 1.13 for erf-GELU
        (max of Phi(x) + x phi(x), 1.1290 at x = sqrt 2), 1.10 for quick-GELU x sigmoid(1.702 x) (1.0998, whatever the slope), 1.13
        for tanh-GELU (1.1291).
      * E = 2^-20 (|pre| + |act(pre)|) is the evaluation error of the device function for the three GELUs, 0 otherwise:
          erf-GELU, fused (p8_act / mid_act): Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7 on erf, with v_rcp_f32 (1 ulp) and __expf
            (v_exp_f32, 1 ulp, on an argument product rounded to 2^-24 |z^2|: z^2 e^(-z^2) <= 1 / e keeps that below 2^-23): below
            4e-7 on erf, 2^-22 |pre| on the result.  Composed (mmgl_activation_fwd): erff, 4 ulp = 2^-21 on erf.
          quick-GELU: v * v_rcp_f32(1 + __expf(-1.702 v)): the exponential's relative error 2^-23 + 2 * 1.702 |v| 2^-24 reaches the
            sigmoid through s (1 - s), and t s (1 - s) <= 0.224: below 2^-23 |pre|.  mmgl_activation_fwd divides instead (exact).
          tanh-GELU: tanhf, 2 ulp = 2^-22 absolute, on an argument of four rounded operations where u (1 - tanh^2 u) <= 0.45:
            below 2^-21 on 1 + tanh, 2^-22 |pre| on the result.
        each with a factor 2 or more of room; relative to u = 2^-8 it is nothing, it matters for fp32 on the composed route.
      * staged (composed TILE128 route only: launch_nt128, then an activation pass, a zmask pass, a residual pass, each storing in the
        operand dtype): L u |pre| where the GEMM's store precedes an activation pass, and u |act(pre), masked| where a residual pass
        follows.  The zmask pass stores the value it read or zero: no rounding.
      * the bf16 backward materialises dyp once in bf16 when there is an activation: one more operand rounding, u mag, unless scale
        is a power of two (`dyp_rounded`).
    The constants are counted, not fitted to a GPU run; c may grow by one factor of two for a rounding that is found and counted, no
    further (none was: on an MI355X the largest err / bound is 0.89-0.99 in bf16 -- the store's half ulp, which rounding alone reaches
    -- and 0.004-0.015 in fp32)."""
    LIP = {0: 1.0, 1: 1.0, 2: 1.13, 3: 1.10, 4: 1.13}
    ACT = {0: lambda t: t, 1: torch.relu, 2: lambda t: 0.5 * t * (1 + torch.erf(t * 0.5 ** 0.5)), 3: lambda t: t * torch.sigmoid(1.702 * t),
           4: lambda t: 0.5 * t * (1 + torch.tanh(0.7978845608028654 * (t + 0.044715 * t ** 3)))}

    @staticmethod
    def inputs(dtype, M, N, K, seed=0, device="cpu"):
        """Operands of a linear y[M,N] = x[M,K] W[N,K]^T and of its backward, in `dtype`: randn, W scaled by K^-0.5; bias, residual,
        zmask, dy and the accumulate priors of unit scale; y = relu(randn) (half of it exact zeros: the operand of dyp's mask) and
        xr = relu(x) (the operand of mask_dx)."""
        g = torch.Generator(device=device).manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g, device=device)
        t = dict(x=r(M, K), w=r(N, K) * K ** -0.5, bias=r(N), residual=r(M, N), zmask=r(M, N), dy=r(M, N), y=torch.relu(r(M, N)),
                 prior_w=r(N, K), prior_b=r(N))
        t["xr"] = torch.relu(t["x"])
        return {k: v.to(dtype) for k, v in t.items()}

    @staticmethod
    def chain(dtype, contraction, folds=0):
        """n of the docstring: the longest chain of fp32 roundings."""
        return -(-contraction // (16 if dtype == torch.bfloat16 else 4)) + folds + 8

    @staticmethod
    def c(n):
        return max(2.0 ** -16, 2 * n * 2.0 ** -24)

    def __init__(self, want, mag, lip=1.0, evalerr=None, pre=None, masked_act=None):
        self.want, self.mag, self.lip, self.evalerr, self.pre, self.masked_act = want, mag, lip, evalerr, pre, masked_act

    @classmethod
    def forward(cls, x, w, bias=None, act=0, scale=1.0, residual=None, zmask=None, K=None, scale_after=False):
        """scale_after: the scale applied after the activation instead of before (a deliberately wrong reference)."""
        d = lambda t: t.detach().double()
        K = x.shape[1] if K is None else K
        X, W = d(x)[:, :K], d(w)[:, :K]
        pre, mag = X @ W.t(), X.abs() @ W.abs().t()
        if bias is not None:
            pre, mag = pre + d(bias), mag + d(bias).abs()
        mag = mag * abs(scale)
        a = cls.ACT[act](pre) * scale if scale_after else cls.ACT[act](pre * scale)
        pre = pre * scale
        ev = 2.0 ** -20 * (pre.abs() + a.abs()) if act >= 2 else None
        if zmask is not None:
            a = torch.where(d(zmask) > 0, a, torch.zeros_like(a))
        want = a
        if residual is not None:
            want, mag = a + d(residual), mag + d(residual).abs()
        return cls(want, mag, cls.LIP[act], ev, pre, a)

    @staticmethod
    def dyp(dy, y=None, scale=1.0):
        v = dy.detach().double() * scale
        return v if y is None else torch.where(y.detach().double() > 0, v, torch.zeros_like(v))

    @classmethod
    def dgrad(cls, dy, w, y=None, scale=1.0, x_mask=None, mask_ge=False):
        """mask_ge: the mask taken from x >= 0 instead of x > 0 (a deliberately wrong reference)."""
        g, W = cls.dyp(dy, y, scale), w.detach().double()
        want, mag = g @ W, g.abs() @ W.abs()
        if x_mask is not None:
            xm = x_mask.detach().double()
            want = torch.where((xm >= 0) if mask_ge else (xm > 0), want, torch.zeros_like(want))
        return cls(want, mag)

    @classmethod
    def wgrad(cls, dy, x, y=None, scale=1.0, prior=None):
        g, X = cls.dyp(dy, y, scale), x.detach().double()
        want, mag = g.t() @ X, g.abs().t() @ X.abs()
        if prior is not None:
            want, mag = want + prior.detach().double(), mag + prior.detach().double().abs()
        return cls(want, mag)

    @classmethod
    def dbias(cls, dy, y=None, scale=1.0, prior=None):
        g = cls.dyp(dy, y, scale)
        want, mag = g.sum(0), g.abs().sum(0)
        if prior is not None:
            want, mag = want + prior.detach().double(), mag + prior.detach().double().abs()
        return cls(want[None, :], mag[None, :])

    def bound(self, dtype, n, composed=False, has_act_pass=False, has_residual_pass=False, dyp_rounded=False):
        """The bound, shaped like `want`.  n: GemmRef.chain of the case.  composed, has_act_pass, has_residual_pass: the staged stores
        of the TILE128 route.  dyp_rounded: the bf16 backward's materialised dyp with a scale that is no power of two."""
        u = U[dtype]
        b = u * self.want.abs() + self.lip * GemmRef.c(n) * self.mag
        if self.evalerr is not None:
            b = b + self.evalerr
        if composed and has_act_pass:
            b = b + self.lip * u * self.pre.abs()
        if composed and has_residual_pass:
            b = b + u * self.masked_act.abs()
        if dyp_rounded:
            b = b + u * self.mag
        return b

    def outside(self, other, dtype, n, **kw):
        """From two references alone: the elements (bool) at which `other` -- a deliberately wrong reference of the same call -- leaves
        this one's bound."""
        return outside(self.want, other.want, self.bound(dtype, n, **kw))

    def check(self, got, what, group="", n=8, **kw):
        """Asserts the bound on every element of `got`; prints and returns the largest err / bound.  A failure names the number of
        elements outside and the (row tile, column tile) pairs that hold them, in the 256 and in the 128 tiling."""
        return check_bound(got, self.want, self.bound(got.dtype, n, **kw), what, group, tiles)


# ------------------------------------------------------------------------------------------ the plans of csrc/gemm.hip and gemm8p.hip, restated
P8, P8_ROWS, P8_REM, P8_FEW, MID, TILE128 = "P8", "P8+rows", "P8+rem", "P8+few", "MID", "TILE128"
FAST = {P8: 1, P8_ROWS: 1, P8_REM: 1, P8_FEW: 1, MID: 2, TILE128: 0}        # mmgl_gemm_nt_fast
MIN_TILES = 160             # GEMM8P_MIN_TILES
NT_MID, NT_FEW, TX_GLDS, TX, TT1, TT4, TRANSPOSE = "nt-" + MID, "nt-" + P8_FEW, "tx-glds", "tx", "tt1", "tt4", "transpose"
COLSUM_SPLITS = 64


def cdiv(a, b):
    return (a + b - 1) // b


def num_cu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def gemm8p_supported(M, N, K, ldx, ldw, ldy):
    return (M > 0 and N > 0 and K >= 256 and K % 128 == 0 and N % 16 == 0 and ldx % 8 == 0 and ldw % 8 == 0 and ldy % 8 == 0
            and M * ldx * 2 < 0xffffffff and N * ldw * 2 < 0xffffffff)


def gemm_mid_supported(M, N, K, ldx, ldw, ldy):
    return (M > 0 and N > 0 and K >= 64 and K % 64 == 0 and N % 8 == 0 and ldx % 8 == 0 and ldw % 8 == 0 and ldy % 8 == 0
            and ldx + 127 >= K and ldw >= K and ldy >= N and max(ldx, ldw, ldy) * 2 * 128 < 0x7fffffff)


def gemm8p_plan(M, N, K, G):
    """(direct, nsplit): tiles [0, direct) whole, the rest as nsplit K-split work items each (0: none)."""
    tiles, units = cdiv(M, 256) * cdiv(N, 256), K // 128
    if tiles < MIN_TILES:
        if units < 24 or (units < 32 and tiles >= 64):
            return tiles, 0
        s = min(cdiv(224, tiles), 8, units // 2)
        return (0, s) if s >= 2 else (tiles, 0)
    rounds, r = tiles // G, tiles % G
    if rounds < 1 or rounds > 12 or r == 0:
        return tiles, 0
    s = min(G // r, 8, units // 4)
    return (tiles - r, s) if s >= 3 else (tiles, 0)


def gemm8p_split_bytes(M, N, K, G):
    d, s = gemm8p_plan(M, N, K, G)
    return (cdiv(M, 256) * cdiv(N, 256) - d) * s * 256 * 256 * 4 if s else 0


def gemm8p_use_splits(M, N, K, G):
    return cdiv(M, 256) * cdiv(N, 256) >= 24 and gemm8p_plan(M, N, K, G)[1] > 0


def gemm8p_row_split(M, N, K, ldx, ldw, ldy, G):
    tm, tn = cdiv(M, 256), cdiv(N, 256)
    rounds, rem = tm * tn // G, tm * tn % G
    if rounds < 1 or rounds > 3 or rem == 0 or rem > G // 4 or (rounds * G) % tn:
        return 0
    m1 = rounds * G // tn * 256
    return m1 if 0 < m1 < M and gemm_mid_supported(M - m1, N, K, ldx, ldw, ldy) else 0


def nt_route(M, N, K, ldx, ldw, ldy, dtype, k_splits, G):
    if dtype != BF16:
        return TILE128
    if gemm8p_supported(M, N, K, ldx, ldw, ldy) and (cdiv(M, 256) * cdiv(N, 256) >= MIN_TILES or (k_splits and gemm8p_use_splits(M, N, K, G))):
        return P8
    return MID if gemm_mid_supported(M, N, K, ldx, ldw, ldy) else TILE128


def workspace_bytes(M, N, K, ldx, ldw, ldy, dtype, G):
    if nt_route(M, N, K, ldx, ldw, ldy, dtype, True, G) != P8 or not gemm8p_use_splits(M, N, K, G):
        return 0
    return cdiv(gemm8p_split_bytes(M, N, K, G), 256) * 256


def bits_bytes(M, N, K, ldx, ldw, ldy, dtype, G):
    return cdiv(M, 256) * cdiv(N, 256) * 8192 if nt_route(M, N, K, ldx, ldw, ldy, dtype, False, G) == P8 else 0


def detail(M, N, K, ldx, ldw, ldy, dtype, scratch, G):
    """(what launch_nt does, K splits folded): the route of nt_route with the persistent kernel's three plans told apart."""
    r = nt_route(M, N, K, ldx, ldw, ldy, dtype, True, G)
    if r != P8:
        return r, 0
    if gemm8p_row_split(M, N, K, ldx, ldw, ldy, G):
        return P8_ROWS, 0
    d, s = gemm8p_plan(M, N, K, G)
    if s and scratch:
        return (P8_FEW if d == 0 else P8_REM), s
    return P8, 0


def gemm8p_tt_splits(RA, RB, M, G):
    if M % 128:
        return 0
    if RA % 256 or RB % 256:
        return 1 if RA % 8 == 0 and RB % 8 == 0 and M >= 256 and cdiv(RA, 256) * cdiv(RB, 256) >= 192 else 0
    tiles, units = (RA // 256) * (RB // 256), M // 128
    best = best_cost = 0
    for s in range(1, 33):
        if units % s or M // s < 256:
            continue
        cost = cdiv(tiles * s, G) * (units // s + 3) + (3 + tiles * s * 6 // 100 if s > 1 else 0)
        if not best or cost < best_cost:
            best, best_cost = s, cost
    return best if best and tiles * best >= 64 else 0


def colsum_splits(M, N, vn):
    s = min(max(cdiv(1024, cdiv(N, 16 * vn)), 16), COLSUM_SPLITS)
    return min(s, max(M // 128, 1))


def big_tile_shape(M, N, K):
    return K % 64 == 0 and cdiv(M, 256) * cdiv(N, 256) >= 512


def dgrad_route(M, N, K, G):
    """(route, K splits folded) of the bf16 dx[M, K] = dyp[M, N] W[N, K]."""
    route, s = detail(M, K, N, N, N, K, BF16, True, G)
    if big_tile_shape(M, K, N) or (N % 128 == 0 and nt_route(M, K, N, N, N, K, BF16, True, G) != TILE128):
        return "nt-" + route, s
    return (TX_GLDS if N % 64 == 0 and K % 128 == 0 else TX), 0


def wgrad_route(M, N, K, G):
    """(route, K splits folded) of the bf16 dW[N, K] = dyp[M, N]^T x[M, K]."""
    s = gemm8p_tt_splits(K, N, M, G)
    if s:
        return f"tt{s}", s if s > 1 else 0
    return (TX_GLDS if M % 64 == 0 and K % 128 == 0 and N % 128 == 0 else TX), 0


def bwd_workspace(M, N, K, act, dtype, G):
    al = lambda n: cdiv(n, 256) * 256
    if dtype == BF16:         # [dyp] [bias column-sum partials] [W^T] [fp32 split partials of the dgrad / the weight gradient]
        s = gemm8p_tt_splits(K, N, M, G)
        return al(M * N * 2) + al(COLSUM_SPLITS * N * 4) + al(K * N * 2) + max(al(s * K * N * 4) if s > 1 else 0, al(gemm8p_split_bytes(M, K, N, G)))
    Mp, Np = cdiv(M, 8) * 8, cdiv(N, 8) * 8
    return max(al(K * Np * 4) + (al(M * N * 4) if act else 0), al(N * Mp * 4) + al(K * Mp * 4))
