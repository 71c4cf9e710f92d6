"""fp64 references of the row kernels (csrc/rownorm.hip, elementwise.hip): the norms, cross-entropy, the gated residual."""
import numpy as np
import torch

from bounds import U, VEC, _keep_scale, check_bound, hash_keep, outside


class NormRef:
    """fp64 reference of the LayerNorm / RMSNorm entry points of csrc/rownorm.hip, forward and backward over s (s = x, or the sum the
    fused pairs store), on the device the storage-rounded operands live on.

    s.  p = 0: (x + r) in fp32 rounded to the operand dtype.  p > 0: fma(fp32(1 / (1 - p)), keep x, r) rounded once to fp32, then to the
    dtype, keep = hash_keep(seed, rows cols, p) at element index row cols + col.  The kernel's stored sum is compared bit for bit
    (check_sum) and everything below is taken from it.  (The fma is formed in fp64 and rounded: a 32-bit product plus a bf16 is exact
    there; in fp32 storage it is a double rounding that differs from the device's single one at a tie of about 2^-29 probability.)

    Forward, with mu, rs = (var + eps)^-1/2, d = s - mu, A = mean|s| per row, kappa = A rs (RMSNorm: mu = 0):
        want y = d rs gamma + beta                 mag y = (|d| + A) rs |gamma| + |beta|
        |mean - mu| <= 2^-18 A                     |rstd - rs| <= 2^-17 rs
    Backward, with gy = dy gamma, h = d rs, m1 = mean(gy) (RMSNorm: 0), m2 = mean(gy h):
        want dx = rs (gy - m1 - h m2) + dres       mag dx = rs (1 + kappa) (|gy| + mean|gy| + |h| mean(|gy| |h|)) + |dres|
        want dx_drop = keep / (1 - p) dx           (p > 0: the gradient of the dropped branch, one more store)
        want dgamma = sum_r dy h                   mag = sum_r |dy| (|h| + kappa_r)
        want dbeta  = sum_r dy                     mag = sum_r |dy|
    Bounds, functions of the reference alone (every element is checked):
        y, dx            |got - want| <= u |want| + 2^-16 mag                 u = 2^-8 (bf16) / 2^-23 (fp32)
        dx_drop          keep / (1 - p) times dx's bound, + u |want dx_drop|
        dgamma, dbeta    |got - want| <= 2^-24 |want| + max(2^-16, 2 n 2^-24) mag,   n = NormRef.chain(rows, tpr)
    The count of roundings:
      * mean: a thread adds at most NV VN = 32 elements, the wave sum is 6 shuffle steps, the block adds 4 wave sums (3), one
        division: about 41 roundings of 2^-24 relative to A, counted as 64 = 2^-18 A.
      * rstd: the variance takes the same chain on d^2 (all terms positive: a relative error), d carries its own rounding and the
        mean's error delta, which enters the sum as delta^2 only; rsqrtf is 1 ulp.  Half of 64 + 4 roundings on var, + 2^-23: 2^-17.
      * y: the mean's error reaches it as delta rs gamma <= 2^-18 A rs |gamma|, rstd's as 2^-17 |d| rs |gamma|, then three rounded
        operations: all inside 2^-16 mag -- SkinnyRef's floor of 256 roundings; the chains above are under 64.
      * dx: m1 and m2 take the mean's chain on gy and gy h; the kernel forms h from the SAVED fp32 mean and rstd, whose errors
        (2^-18 A rs = 2^-18 kappa on h, 2^-17 |h|) are what the factor (1 + kappa) carries.
      * dgamma / dbeta: chain(rows, tpr) = rows per partial row + partial rows / 8 (norm_param_reduce_kernel's lane) + 8 (its LDS
        fold) + 8 (h, the product, the two stores); partial rows = blocks x rows per block with blocks capped at 512 (bwd_blocks).
    Nothing is fitted to a run.  Keyword arguments build deliberately wrong references: stat_cols (bool [cols]: the columns that
    enter the statistics, or m1 / m2, still divided by cols), grad_rows (bool [rows]: the rows that enter dgamma / dbeta), no_dres,
    mask_row_shift (the mask's element index offset by that many rows)."""

    @staticmethod
    def edges(cols, vn):
        """The columns scaled by 16: chunk, lane-trip and row ends."""
        nch = cols // vn
        e = [0, vn - 1, vn, (nch // 2) * vn, 64 * vn - 1, 64 * vn, 256 * vn - 1, 256 * vn, cols - vn - 1, cols - vn, cols - 1]
        return sorted({c for c in e if 0 <= c < cols})

    @staticmethod
    def edge_rows(rows, seams=()):
        e = [0, 3, 4, rows - 2, rows - 1] + [r + o for r in seams for o in (-1, 0)]
        return sorted({r for r in e if 0 <= r < rows})

    @staticmethod
    def inputs(dtype, rows, cols, seed=0, device="cpu", seams=()):
        """x = 2 randn + 0.5, res, dy, dres, gamma = 1 + randn / 2, beta = randn / 2 in `dtype`; x and dy times 16 on the edge columns,
        dy times 16 on the edge rows (0, 3, 4, rows - 2, rows - 1 and both sides of every grid-stride seam).  Drawn on the CPU (the same
        numbers whatever the device), then moved."""
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g)
        t = dict(x=2 * r(rows, cols) + 0.5, res=r(rows, cols), dy=r(rows, cols), dres=r(rows, cols), gamma=1 + 0.5 * r(cols), beta=0.5 * r(cols))
        ec = NormRef.edges(cols, VEC[dtype])
        t["x"][:, ec] *= 16
        t["dy"][:, ec] *= 16
        t["dy"][NormRef.edge_rows(rows, seams)] *= 16
        return {k: v.to(dtype).to(device) for k, v in t.items()}

    @staticmethod
    def chain(rows, tpr):
        """n of the dgamma / dbeta bound; restates bwd_blocks (csrc/rownorm.hip)."""
        rpb = 256 // tpr
        blocks = min(-(-rows // rpb), 512)
        parts = blocks * rpb
        return -(-rows // parts) + -(-parts // 8) + 8 + 8

    @staticmethod
    def c(n):
        return max(2.0 ** -16, 2 * n * 2.0 ** -24)

    @staticmethod
    def keep(seed, rows, cols, p, device, row_shift=0):
        k = hash_keep(seed, rows * cols, p, start=row_shift * cols)
        return torch.from_numpy(k).view(rows, cols).to(device)

    def __init__(self, x, gamma=None, beta=None, rms=False, eps=1e-5, res=None, p=0.0, seed=0, s=None, stat_cols=None, mask_row_shift=0):
        d = lambda t: t.detach().double()
        rows, cols = x.shape
        self.rows, self.cols, self.dtype, self.rms, self.p = rows, cols, x.dtype, rms, p
        self.keep = None
        if res is None:
            self.s = x.detach()
        elif p > 0:
            self.keep = NormRef.keep(seed, rows, cols, p, x.device, mask_row_shift)
            self.s = (_keep_scale(p) * torch.where(self.keep, d(x), torch.zeros_like(d(x))) + d(res)).float().to(x.dtype)
        else:
            self.s = (x.detach().float() + res.detach().float()).to(x.dtype)
        S = d(self.s if s is None else s)          # s: the kernel's stored sum, once check_sum has held it against self.s
        w = torch.ones(cols, dtype=torch.float64, device=x.device) if stat_cols is None else stat_cols.to(x.device).double()
        self.w = w
        mu = torch.zeros(rows, 1, dtype=torch.float64, device=x.device) if rms else (S * w).sum(1, keepdim=True) / cols
        dd = S - mu
        rs = ((dd * dd * w).sum(1, keepdim=True) / cols + float(np.float32(eps))).rsqrt()
        A = S.abs().mean(1, keepdim=True)
        self.mu, self.rs, self.A, self.kappa, self.d = mu, rs, A, A * rs, dd
        self.gamma = None if gamma is None else d(gamma)
        y, mag = dd * rs, (dd.abs() + A) * rs
        if gamma is not None:
            y, mag = y * d(gamma), mag * d(gamma).abs()
        if beta is not None:
            y, mag = y + d(beta), mag + d(beta).abs()
        self.want = dict(y=y, mean=mu[:, 0], rstd=rs[:, 0])
        self.mag = dict(y=mag, mean=A[:, 0], rstd=rs[:, 0])

    def backward(self, dy, dres=None, grad_rows=None, no_dres=False):
        """Adds dx, dx_drop (p > 0), dgamma and dbeta to want / mag; returns self."""
        d = lambda t: t.detach().double()
        DY, h, rs, w, cols = d(dy), self.d * self.rs, self.rs, self.w, self.cols
        gy = DY if self.gamma is None else DY * self.gamma
        mean = lambda t: (t * w).sum(1, keepdim=True) / cols
        m1 = torch.zeros_like(rs) if self.rms else mean(gy)
        m2 = mean(gy * h)
        dx = rs * (gy - m1 - h * m2)
        mag = rs * (1 + self.kappa) * (gy.abs() + gy.abs().mean(1, keepdim=True) + h.abs() * (gy.abs() * h.abs()).mean(1, keepdim=True))
        if dres is not None:
            mag = mag + d(dres).abs()
            if not no_dres:
                dx = dx + d(dres)
        self.want["dx"], self.mag["dx"] = dx, mag
        if self.keep is not None:
            self.want["dx_drop"] = torch.where(self.keep, dx * _keep_scale(self.p), torch.zeros_like(dx))
            self.mag["dx_drop"] = torch.where(self.keep, mag * _keep_scale(self.p), torch.zeros_like(mag))
        r = torch.ones(self.rows, 1, dtype=torch.float64, device=DY.device) if grad_rows is None else grad_rows.to(DY.device).double()[:, None]
        self.want["dgamma"], self.mag["dgamma"] = (DY * h * r).sum(0), (DY.abs() * (h.abs() + self.kappa) * r).sum(0)
        self.want["dbeta"], self.mag["dbeta"] = (DY * r).sum(0), (DY.abs() * r).sum(0)
        return self

    def bound(self, name, tpr=64):
        want, mag, u = self.want[name], self.mag[name], U[self.dtype]
        if name == "mean":
            return 2.0 ** -18 * mag
        if name == "rstd":
            return 2.0 ** -17 * mag
        if name in ("dgamma", "dbeta"):
            return 2.0 ** -24 * want.abs() + NormRef.c(NormRef.chain(self.rows, tpr)) * mag
        if name == "dx_drop":                # mag is already keep / (1 - p) times dx's: the first store's half ulp passes through the scale
            return u * want.abs() + (u * want.abs() + 2.0 ** -16 * mag)
        return u * want.abs() + 2.0 ** -16 * mag

    def outside(self, other, name, tpr=64):
        """From two references alone: the elements at which `other` (a deliberately wrong reference) leaves this one's bound."""
        return outside(self.want[name], other.want[name], self.bound(name, tpr))

    def check_sum(self, got, what):
        assert torch.equal(got, self.s), f"{what}: the stored sum is not the reference's, bit for bit ({(got != self.s).sum().item()} elements differ)"

    def check(self, got, name, what, group="", tpr=64):
        """Asserts the bound of output `name` on every element of `got`; prints and returns the largest err / bound."""
        want, bound = self.want[name], self.bound(name, tpr)
        if want.dim() == 1:                  # per-row outputs are reported as rows, the parameter gradients as columns
            want, bound = (want[None, :], bound[None, :]) if name in ("dgamma", "dbeta") else (want[:, None], bound[:, None])
        return check_bound(got, want, bound, f"{what} {name}", group)


class CrossEntropyRef:
    """fp64 reference of mmgl_cross_entropy_fwd / bwd (csrc/elementwise.hip) from the storage-rounded logits, on their device.

    With max_r, lse_r = log sum_j exp x_j, p = exp(x - lse), H_r = sum_j p_j (max_r - x_j), live rows those whose label is not the
    ignore index and lies in [0, V), count = their number, scale = dloss / max(count, 1) (`count` overrides the divisor: the LM head
    scores a chunk of rows against the count of the whole batch):
        row_lse    |got - lse| <= 2^-23 (|max| + |lse|) + n 2^-24 (1 + H) =: b_lse,      n = 3 ceil(V / (256 VN)) + VN + 16
        row_loss   want lse - x_label, bound b_lse + 2^-24 (|lse| + |x_label|); exactly 0 on ignored rows
        count      exact;   loss_sum  within the sum of the live rows' bounds + (rows / 256 + 16) 2^-24 sum|row_loss|
        dlogits    want (p - onehot) scale;  |got - want| <= u |want| + |scale| (p_j (b_lse + 2^-22 (1 + |x_j - lse|)) + 2^-24),
                   every element; exactly 0 on ignored rows and at -inf logits.        u = 2^-8 (bf16) / 2^-23 (fp32)
    The count of roundings: n is the folds of one thread (ceil(V / (256 VN)) of them, three roundings each: the rescale of the
    running sum, its product, the add), the sum inside a 16-byte vector (VN), and the block merge with logf (rescale, 6 shuffle
    steps, 3 adds of wave sums, logf at 2 ulp, the final add: 16).  H is how the rounding |a| 2^-24 of __expf's argument a = x - m
    reaches the sum: sum_j p_j |x_j - max| 2^-24 relative to the sum, times the same n.  2^-23 (|max| + |lse|) is the rounding of
    the running maximum's differences and of the final gm + logf(gs).  In dlogits, b_lse is the saved lse's error in the exponent,
    2^-22 (1 + |x - lse|) is v_exp_f32 at 1 ulp plus the rounded argument difference and its product with log2 e, and 2^-24 is the
    subtraction of the one-hot; the division dloss / count and the product with it are inside u |want| in fp32 (2 x 2^-24).
    Nothing is fitted to a run.  Keyword arguments build deliberately wrong references: lse_cols (bool [V]: the columns that enter
    lse), label_shift (the one-hot offset by that many columns), by_rows (division by rows instead of count), live_row (an ignored
    row treated as live: its gradient is p scale, its loss lse)."""

    @staticmethod
    def edges(V, vn):
        e = [0, vn - 1, vn, 256 * vn - 1, 256 * vn, 768 * vn - 1, 768 * vn, 1024 * vn - 1, 1024 * vn, V - vn - 1, V - vn, V - 1]
        return sorted({c for c in e if 0 <= c < V})

    @staticmethod
    def inputs(dtype, V, seed=0, device="cpu", ignore=-100):
        """Six rows of unit randn logits with the edge columns at max(2, ln(0.165 V)) (each edge holds about 4.5 % of its row's mass
        at any V), labels 0, V - 1, ignore, an edge, V / 2, 7 (clamped to V - 1).  Drawn on the CPU, then moved."""
        import math
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(6, V, generator=g)
        ec = CrossEntropyRef.edges(V, VEC[dtype])
        x[:, ec] = max(2.0, math.log(0.165 * V))
        lab = torch.tensor([0, V - 1, ignore, ec[len(ec) // 2], V // 2, min(7, V - 1)], dtype=torch.int64)
        return x.to(dtype).to(device), lab.to(device)

    def __init__(self, logits, labels, ignore=-100, dloss=1.0, count=None, lse_cols=None, label_shift=0, by_rows=False, live_row=None):
        X = logits.detach().double()
        rows, V = X.shape
        self.rows, self.V, self.dtype, self.x = rows, V, logits.dtype, X
        vn = VEC[logits.dtype]
        neg = torch.full_like(X, float("-inf"))
        Xs = X if lse_cols is None else torch.where(lse_cols.to(X.device)[None, :], X, neg)
        mx = Xs.amax(1, keepdim=True)
        lse = torch.logsumexp(Xs, 1, keepdim=True)
        p = torch.exp(X - lse)
        ps = torch.exp(Xs - lse)
        H = torch.where(ps > 0, ps * (mx - Xs), torch.zeros_like(ps)).sum(1, keepdim=True)
        n = 3 * -(-V // (256 * vn)) + vn + 16
        b_lse = 2.0 ** -23 * (mx.abs() + lse.abs()) + n * 2.0 ** -24 * (1 + H)
        lab = labels.detach().to(X.device)
        live = (lab != ignore) & (lab >= 0) & (lab < V)
        self.live, self.p = live, p
        safe = torch.where(live, lab, torch.zeros_like(lab))
        xl = X.gather(1, safe[:, None])
        row_loss = torch.where(live[:, None], lse - xl, torch.zeros_like(lse))
        b_loss = torch.where(live[:, None], b_lse + 2.0 ** -24 * (lse.abs() + xl.abs()), torch.zeros_like(lse))
        cnt = float(live.sum().item())
        div = float(rows) if by_rows else (cnt if count is None else float(count))
        scale = float(np.float32(dloss)) / max(div, 1.0)
        onehot = torch.zeros_like(X)
        tgt = safe + label_shift
        tgt = torch.where(tgt >= V, safe - label_shift, tgt).clamp(0, V - 1)
        onehot.scatter_(1, tgt[:, None], 1.0)
        g = torch.where(live[:, None], (p - onehot) * scale, torch.zeros_like(p))
        b_g = abs(scale) * (p * (b_lse + 2.0 ** -22 * (1 + torch.where(p > 0, (X - lse).abs(), torch.zeros_like(p)))) + 2.0 ** -24)
        if live_row is not None:
            g[live_row] = p[live_row] * scale
            row_loss[live_row] = lse[live_row]
        self.exact0 = (~live[:, None]) | torch.isneginf(X)              # where dlogits must be exactly zero
        self.want = dict(row_lse=lse[:, 0], row_loss=row_loss[:, 0], loss_sum=row_loss.sum().reshape(1), dlogits=g,
                         count=torch.tensor([cnt], dtype=torch.float64, device=X.device))
        self.mag = dict(row_lse=mx.abs()[:, 0] + lse.abs()[:, 0], row_loss=row_loss.abs()[:, 0], dlogits=abs(scale) * p)
        self._bound = dict(row_lse=b_lse[:, 0], row_loss=b_loss[:, 0], count=torch.zeros(1, dtype=torch.float64, device=X.device),
                           loss_sum=(b_loss.sum() + (rows / 256 + 16) * 2.0 ** -24 * row_loss.abs().sum()).reshape(1),
                           dlogits=U[logits.dtype] * g.abs() + torch.where(self.exact0, torch.zeros_like(b_g), b_g))

    def bound(self, name):
        return self._bound[name]

    def outside(self, other, name):
        return outside(self.want[name], other.want[name], self.bound(name))

    def check(self, got, name, what, group=""):
        want, bound = self.want[name], self.bound(name)
        if want.dim() == 1:
            want, bound = want[:, None], bound[:, None]
        return check_bound(got, want, bound, f"{what} {name}", group)


class GatedRef:
    """fp64 reference of mmgl_gated_residual_fwd / bwd (csrc/elementwise.hip) over n elements, on the operands' device.

    With tg = tanh(gate) (1 without a gate), keep = hash_keep(seed, n, p), inv = 1 / (1 - p):
        want y  = r + (tg inv) keep x              one fma, one store:   |got - want| <= u |want| + 2^-22 (|r| + |tg inv keep x|)
        want dx = tg keep inv dy                   |got - want| <= u |want| + 2^-21 |want|
        want dgate = (1 - tg^2) sum dy keep inv x  |got - want| <= 2^-23 |want| + max(2^-16, 2 n 2^-24) mag,   mag = (1 - tg^2) sum|dy keep inv x|
    2^-22 carries tanhf at 2 ulp and the scale's own rounding (the fp32 1 - p, the division).  dx is two rounded products of three
    rounded factors -- tanhf at 2 ulp (2^-22), 1 - p and the division (2 x 2^-24), the products (2 x 2^-24): 2^-21 -- then the store.
    n = elements per thread (VN per grid-stride trip, + the n % VN tail elements of thread 0) + 6 (wave shuffle) + 4 (block) +
    blocks / 256 (gate_grad_kernel's thread) + 8 (its block sum, tanhf, 1 - tg^2, the product); blocks = min(ceil(nvec / 256), 2048).
    `index_shift` (a deliberately wrong reference) offsets the mask's element index."""

    @staticmethod
    def blocks(n, vn):
        return min(max(-(-(n // vn) // 256), 1), 2048)

    @staticmethod
    def chain(n, vn):
        b = GatedRef.blocks(n, vn)
        return -(-(n // vn) // (b * 256)) * vn + n % vn + 6 + 4 + -(-b // 256) + 8

    def __init__(self, res, x, gate=None, p=0.0, seed=0, index_shift=0):
        import math
        d = lambda t: t.detach().double().reshape(-1)
        self.dtype, self.n = x.dtype, x.numel()
        self.tg = 1.0 if gate is None else math.tanh(float(gate))
        self.inv = _keep_scale(p)
        keep = torch.from_numpy(hash_keep(seed, self.n, p, start=index_shift)).to(x.device) if p > 0 else torch.ones(self.n, dtype=torch.bool, device=x.device)
        self.kx = torch.where(keep, d(x), torch.zeros_like(d(x))) * self.inv
        self.keep = keep
        term = self.tg * self.kx
        u = U[x.dtype]
        self.want = dict(y=d(res) + term)
        self.mag = dict(y=d(res).abs() + term.abs())
        self._bound = dict(y=u * self.want["y"].abs() + 2.0 ** -22 * self.mag["y"])

    def backward(self, dy):
        DY, u = dy.detach().double().reshape(-1), U[self.dtype]
        dx = torch.where(self.keep, DY, torch.zeros_like(DY)) * (self.tg * self.inv)
        c = max(2.0 ** -16, 2 * GatedRef.chain(self.n, VEC[self.dtype]) * 2.0 ** -24)
        t2 = 1 - self.tg * self.tg
        self.want.update(dx=dx, dgate=(t2 * (DY * self.kx).sum()).reshape(1))
        self.mag.update(dx=dx.abs(), dgate=(abs(t2) * (DY * self.kx).abs().sum()).reshape(1))
        self._bound.update(dx=(u + 2.0 ** -21) * dx.abs(), dgate=2.0 ** -23 * self.want["dgate"].abs() + c * self.mag["dgate"])
        return self

    def bound(self, name):
        return self._bound[name]

    def outside(self, other, name):
        return outside(self.want[name], other.want[name], self.bound(name))

    def check(self, got, name, what, group=""):
        return check_bound(got, self.want[name][:, None], self.bound(name)[:, None], f"{what} {name}", group)
