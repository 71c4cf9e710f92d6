"""fp64 references of the decode kernels (csrc/decode.hip): the skinny GEMMs and the eight single-query attention entry points."""
import torch

from bounds import U, check_bound, outside, row_head, rows_columns


class SkinnyRef:
    """fp64 reference of mmgl_gemm_skinny / mmgl_gemm_skinny_lora on the device the (storage-rounded) operands live on:
        want = act((x W^T + bias + s (x A^T) B^T) * scale) + residual
        mag  = (|x| |W|^T + |bias| + |s| (|x| |A|^T) |B|^T) * |scale| + |residual|
    and two deliberately wrong references of the same call, for the assertion that a comparison can fail: `drop_k` (the last 64 K
    columns of x left out of both products) and, with an adapter, `no_lora` (the rank-r term left out).

    Per-element bound (every element is checked):  |got - want| <= u |want| + 2^-16 mag,  u = 2^-8 (bf16) or 2^-23 (fp32).
      * u |want| is the half ulp of the one round-to-nearest store of the fp32 result; rounding alone reaches it, so it has no margin.
      * 2^-16 mag is 256 fp32 roundings of 2^-24 on the magnitude sum: the longest summation chain of either kernel at K = 8192 is
        below 100 on the MFMA kernel (64 MFMA steps, the in-MFMA tree, the 8-slot fold) and 128 + 6 on the plain one; it also covers
        a rounding decision, or a ReLU whose pre-activation lies within 2^-16 mag of zero, that the summation order flips.
    The bound is a function of the reference alone, never of the kernel's output."""

    def __init__(self, x, w, bias=None, relu=False, scale=1.0, residual=None, A=None, B=None, s=1.0):
        d = lambda t: t.detach().double()
        X, W = d(x), d(w)
        K = X.shape[1]
        tail = slice(max(K - 64, 0), K)
        pre = X @ W.t()
        mag = X.abs() @ W.abs().t()
        gone = X[:, tail] @ W[:, tail].t()
        lora = None
        if A is not None:
            Ad, Bd = d(A), d(B)
            lora = s * ((X @ Ad.t()) @ Bd.t())
            pre = pre + lora
            mag = mag + abs(s) * ((X.abs() @ Ad.abs().t()) @ Bd.abs().t())
            gone = gone + s * ((X[:, tail] @ Ad[:, tail].t()) @ Bd.t())
        if bias is not None:
            mag = mag + d(bias).abs()
        mag = mag * abs(scale)
        if residual is not None:
            mag = mag + d(residual).abs()

        def epilogue(y):
            if bias is not None:
                y = y + d(bias)
            y = y * scale
            if relu:
                y = torch.relu(y)
            return y if residual is None else y + d(residual)

        self.want, self.mag = epilogue(pre), mag
        self.drop_k = epilogue(pre - gone)
        self.no_lora = None if lora is None else epilogue(pre - lora)

    def bound(self, dtype):
        return U[dtype] * self.want.abs() + 2.0 ** -16 * self.mag

    @staticmethod
    def assert_can_fail(refs, dtype, what):
        """From the references alone: a kernel that drops one 64-wide K unit (or the rank-r term) leaves the bound on >= 25 % of the
        elements (of the pooled `refs`: the calls of one test, where a single call has too few elements to count on)."""
        for name, pick in (("the last 64 K columns", lambda r: r.drop_k), ("the rank-r term", lambda r: r.no_lora)):
            if pick(refs[0]) is not None:
                out = sum(outside(r.want, pick(r), r.bound(dtype)).sum().item() for r in refs)
                frac = out / sum(r.want.numel() for r in refs)
                assert frac >= 0.25, f"{what}: dropping {name} moves only {frac:.0%} of the elements out of the bound"

    def check(self, got, what, group="", can_fail=True):
        """Asserts the bound on every element of `got` (first, unless can_fail is off, that the comparison can fail); prints and
        returns the largest err / bound."""
        if can_fail:
            SkinnyRef.assert_can_fail([self], got.dtype, what)
        return check_bound(got, self.want, self.bound(got.dtype), what, group, rows_columns)


def attn_decode_ref(q, k, v, valid, num_heads):
    """fp64 reference of mmgl_attn_decode_fwd from the storage-rounded operands: q [B, d] (already scaled), k, v [B, S, d],
    valid [B, S]; softmax over the valid keys of each (sample, head), uniform over all S keys where none is valid.  Returns [B, d]."""
    B, S, d = k.shape
    D = d // num_heads
    sc = torch.einsum("bhd,bshd->bhs", q.double().reshape(B, num_heads, D), k.double().reshape(B, S, num_heads, D))
    ok = valid.bool()
    sc = sc.masked_fill(~ok[:, None, :], float("-inf"))
    sc[~ok.any(1)] = 0.0
    return torch.einsum("bhs,bshd->bhd", torch.softmax(sc, -1), v.double().reshape(B, S, num_heads, D)).reshape(B, d)


# ------------------------------------------------------------------------------------------ single-query attention (csrc/decode.hip)
DECODE_KERNELS = ("plain", "gqa", "beam", "block", "gqa_block", "q8", "gqa_q8", "relbias")


def _cdiv(a, b):
    return -(-a // b)


def decode_geometry(kernel, dtype, D):
    """(VEC, LPK, KPI, I) of a decode.hip kernel: elements per lane and 16-byte load (8 bf16, 4 fp32; Q8_VEC = 16 codes for the q8
    kernels), lanes per key D / VEC, keys per wave and load instruction 64 / LPK, keys per workgroup loop trip 16 KPI."""
    assert kernel in DECODE_KERNELS, kernel
    vec = 16 if kernel in ("q8", "gqa_q8") else (8 if dtype == torch.bfloat16 else 4)
    lpk = D // vec
    return vec, lpk, 64 // lpk, 16 * (64 // lpk)


def decode_rows_cache(k, v, valid):
    """plain, GQA and relbias kernels: row b reads the S cache rows of sample b.  -> (k, v [B,S,kd], allowed [B,S], uniform [B,S])."""
    ok = valid.bool()
    return k, v, ok, torch.ones_like(ok)


def decode_rows_beam(k_pre, v_pre, valid, W, k_tail=None, v_tail=None, src=None, uniform_tail=True):
    """Beam kernel: row (b, w) reads pre[b] ++ tail[b*W + src[b*W + w, j], j].  A sample whose prefix has no valid key allows nothing
    and is uniform over all S_pre + n_tail keys (uniform_tail=False: over the prefix alone, a wrong reference)."""
    B, S = k_pre.shape[:2]
    R = B * W
    k, v, ok = (t.repeat_interleave(W, 0) for t in (k_pre, v_pre, valid.bool()))
    n = 0 if k_tail is None else k_tail.shape[1]
    uni = torch.ones(R, S + n, dtype=torch.bool, device=k.device)
    if n:
        rows = (torch.arange(R, device=k.device) // W * W)[:, None] + src[:, :n].long()
        cols = torch.arange(n, device=k.device)[None, :].expand(R, -1)
        k, v = torch.cat([k, k_tail[rows, cols]], 1), torch.cat([v, v_tail[rows, cols]], 1)
        ok = torch.cat([ok, ok.any(1, keepdim=True).expand(R, n)], 1)
        uni[:, S:] = uniform_tail
    return k, v, ok, uni


def decode_rows_block(k, v, valid, lens, k_new, v_new, m, strict=False, below_capacity=False):
    """Block kernels: row (b, i) reads the valid cache columns s < lens[b], then the new keys j <= i of its sample (strict: j < i, a
    wrong reference).  k, v [B,cap,kd]; k_new, v_new [B*m,kd].  below_capacity (the GQA block kernel, whose new keys are cache
    columns): new key j exists only where lens[b] + j < cap.  -> N = cap + m keys per row."""
    B, cap, kd = k.shape
    dev = k.device
    L = lens.to(dev).long().clamp(0, cap)
    s = torch.arange(cap, device=dev)
    i = torch.arange(m, device=dev)
    old = ((s[None, :] < L[:, None]) & valid.bool()).repeat_interleave(m, 0)                          # [B*m, cap]
    new = (i[None, :] < i[:, None]) if strict else (i[None, :] <= i[:, None])                         # [i, j]
    new = new[None].expand(B, m, m).clone()
    if below_capacity:
        new &= ((L[:, None] + i[None, :]) < cap)[:, None, :]
    kk = torch.cat([k.repeat_interleave(m, 0), k_new.reshape(B, m, kd).repeat_interleave(m, 0)], 1)
    vv = torch.cat([v.repeat_interleave(m, 0), v_new.reshape(B, m, kd).repeat_interleave(m, 0)], 1)
    ok = torch.cat([old, new.reshape(B * m, m)], 1)
    return kk, vv, ok, torch.ones_like(ok)


def decode_rows_q8(codes, e, valid, k_new, v_new, num_kv_heads):
    """q8 kernels: row b reads the S columns dequantised as tests/kvq_ref.py states the format, then its unquantised new row (always
    valid).  codes uint8 [B,S,2kd], e int8 [B,S,2Hkv] (CPU); -> fp32 k, v [B,S+1,kd] on k_new's device."""
    import kvq_ref
    kc, vc = kvq_ref.dequantize_row(codes, e, num_kv_heads)
    dev = k_new.device
    k = torch.cat([kc.to(dev), k_new.float()[:, None]], 1)
    v = torch.cat([vc.to(dev), v_new.float()[:, None]], 1)
    ok = torch.cat([valid.bool().to(dev), torch.ones(k.shape[0], 1, dtype=torch.bool, device=dev)], 1)
    return k, v, ok, torch.ones_like(ok)


def decode_bias_relbias(bias, S, wrong=None):
    """relbias kernel: key s gets bias[h, S - 1 - s].  -> fp32 [H,S].  wrong: "distance s" | "head h^1" | "no bias"."""
    rows = bias[:, :S].float()
    H = rows.shape[0]
    if wrong == "distance s":
        return rows.clone()
    if wrong == "head h^1":
        return rows[[h ^ 1 if (h ^ 1) < H else h for h in range(H)]].flip(1)
    if wrong == "no bias":
        return torch.zeros_like(rows)
    assert wrong is None, wrong
    return rows.flip(1)


class DecodeAttnRef:
    """fp64 reference of the eight single-query attention entry points of csrc/decode.hip on the device the (storage-rounded)
    operands live on.  Every one of them is softmax attention of one query row over a per-row key list, so the reference takes the
    list EXPANDED (the decode_rows_* builders above gather it): q [R, H*D] (already scaled; raw for the relbias kernel),
    k, v [R, N, Hkv*D], allowed [R, N], an optional fp32 bias [H, N] added to the score, kv_head (h -> key/value head, default
    h // G) and uniform [R, N]: the key set a row WITHOUT an allowed key weighs equally (include/mmgl_hip.h: all S keys for the plain
    and GQA kernels, all S_pre + n_tail keys for the beam kernel; default every key of the list).

    Per (row, head):  want = sum_j p_j v_j,  mag = sum_j p_j |v_j|,  S_i = max over the allowed j of sum_d |q_d| |k_jd| (+ |bias_j|)
    (0 for a row without an allowed key: no score reaches its result).

    Per-element bound (every element is checked), a function of the reference alone, never of the kernel's output:
        |got - want| <= u |want| + (n_s S_i + n_c) 2^-24 mag            u = 2^-8 (bf16), 2^-23 (fp32)
    u |want| is the one round-to-nearest store (bounds.U).        The rest is fp32 VALU arithmetic, counted to first order from the
    statements of the kernels in units of one rounding, 2^-24 (the second-order terms are below 2^-12 of the bound at the largest
    count in use).  The computed weight of key j is e^(s_j - M) (1 + eps_j) with M the row's final maximum; a relative error eps of the
    weights moves the result by at most 2 eps mag -- eps mag through the numerator and eps |want| <= eps mag through the normaliser,
    which a common factor does not cancel when the keys err in opposite directions -- so every rounding that reaches a WEIGHT counts
    twice, and a rounding of an accumulator (acc or l) once.

    n_s = 2 (VEC + log2 LPK + 5 [+ 1 relbias]): the roundings of a score that reach p through the exponent, relative to S_i.
      * VEC: the lane's chain dot += q_e k_e; a term passes at most VEC roundings (its product and the sums after it; an fma only
        removes some).  log2 LPK: the xor butterfly (group_sum) over the lanes of the key.  [+ 1: dot + bias, relative to
        |dot + bias| <= S_i, which is why S_i takes |bias_j| in.]  The q8 kernels' 2^e on the dot is exact.
      * 2: the subtraction of the maximum.  |sc - mn| <= 2 S_i, and along the path of a key to the result -- p = e^(sc - mn), then one
        corr = e^(m - mn) per later step of its chain, c1 / c2 per lane-group merge, ci per wave -- the maxima only grow, so the
        magnitudes of ALL these differences telescope to M - s_j <= 2 S_i: two units for the whole path, not two per step.
      * 2 + 1: __expf(x) = exp2(x log2e): the rounded product, relative to the same |x| (telescoping likewise), and the fp32 constant
        log2e itself, 0.22 * 2^-24 off, times 2 S_i: under one unit.
    n_c = sum over the phases of trips (2 U + 6)  +  8 log2 KPI  +  13: the roundings on the weights and accumulators that do not scale
    with the score, along the longest chain a lane group runs.
      * a trip that folds U keys into a state (U = 1: one key of the plain, relbias kernels, a new key of the block and q8 kernels;
        U = AD_UNROLL = 4: the cache / prefix loop of the NQ and q8 kernels; U = TAIL_UNROLL = 2: the beam tail):
        corr and p are v_exp_f32 results, 1 ulp = 2 units each, on disjoint keys (the old state, the trip's keys) and on weights: 4;
        acc: acc * corr, then U sums of p_u v_u: at most 1 + U on the old state, fewer on a new term; l: ps (U - 1), l corr, + ps:
        U + 1.  Together 2 U + 6, i.e. 8 / 14 / 10 for U = 1 / 4 / 2.
        trips: plain, relbias ceil(S / (4 KPI)) at U = 1;  gqa, q8, gqa_q8, beam prefix, block caches ceil(S / (16 KPI)) at U = 4;
        beam tail ceil(n_tail / (8 KPI)) at U = 2;  block, gqa_block new keys and the q8 new row: one trip at U = 1.
      * a lane-group merge (log2 KPI of them): c1, c2 (2 units on a weight: 4), acc c1 + acc' c2 (2), l likewise (2): 8.
      * the waves: ci (4), o += sm_o ci over 4 waves (product and up to 3 sums: 4), ll likewise (4), the division (1): 13.
    The q8 kernels' power-of-two scales (2^e on the dot and on p) are exact, so ONE formula parameterised by the kernel's geometry
    (decode_geometry) serves all eight; the block and q8 kernels add their one extra trip and nothing else.  A p below 2^-126 flushes
    to zero: at most N 2^-126 max|v| against mag, nothing for finite operands.  The constants are derived, not fitted; they grow only
    by a rounding that is found in the kernel and named here.

    inputs() / keys() build edge-weighted operands: q[..., 0] = 1 in every head of every row and k[s, 0] = BOOST on the edge keys, 0
    elsewhere, so an edge key is lifted along EVERY reader's query and carries a few percent of each row at any N."""
    BOOST, SPREAD = 4.0, 40.0

    @staticmethod
    def counts(kernel, dtype, D, S, n_tail=0):
        """(n_s, n_c) for a call of `kernel` whose longest cache / prefix phase has S keys (block kernels: the largest lens)."""
        vec, lpk, kpi, I = decode_geometry(kernel, dtype, D)
        lg = lambda x: int(x).bit_length() - 1
        n_s = 2 * (vec + lg(lpk) + 5 + (kernel == "relbias"))
        if kernel in ("plain", "relbias"):
            chain = 8 * _cdiv(S, 4 * kpi)
        else:
            chain = 14 * _cdiv(S, I)
        if kernel == "beam":
            chain += 10 * _cdiv(n_tail, 8 * kpi)
        if kernel in ("block", "gqa_block", "q8", "gqa_q8"):
            chain += 8
        return n_s, chain + 8 * lg(kpi) + 13

    @staticmethod
    def edges(kernel, dtype, D, n, extra=()):
        """The edge positions of a phase of n keys: {0, KPI-1, KPI, 4KPI-1, 4KPI, I-1, I, n-1} and `extra`, where they exist."""
        _, _, kpi, I = decode_geometry(kernel, dtype, D)
        return sorted({e for e in (0, kpi - 1, kpi, 4 * kpi - 1, 4 * kpi, I - 1, I, n - 1) + tuple(extra) if 0 <= e < n})

    @staticmethod
    def inputs(dtype, R, H, D, seed=0):
        """q [R, H*D] in `dtype`: randn D^-0.5 with q[..., 0] = 1 in every head."""
        g = torch.Generator().manual_seed(seed)
        q = torch.randn(R, H, D, generator=g) * D ** -0.5
        q[..., 0] = 1.0
        return q.reshape(R, H * D).to(dtype)

    @staticmethod
    def keys(dtype, lead, n, Hkv, D, edges=(), seed=0, order=None):
        """k, v [*lead, n, Hkv*D] in `dtype`: randn, with k[..., s, :, 0] = BOOST on the edge keys and 0 elsewhere.  order "asc" /
        "desc": k[..., s, :, 0] = SPREAD s / (n - 1) rising / falling instead -- the running maximum moves at every key / never."""
        g = torch.Generator().manual_seed(seed + 7919)
        k, v = torch.randn(*lead, n, Hkv, D, generator=g), torch.randn(*lead, n, Hkv, D, generator=g)
        k[..., 0] = 0.0
        if order is None:
            k[..., list(edges), :, 0] = DecodeAttnRef.BOOST
        else:
            ramp = DecodeAttnRef.SPREAD * torch.arange(n, dtype=torch.float32) / max(n - 1, 1)
            k[..., 0] = (ramp if order == "asc" else ramp.flip(0))[:, None]
        return tuple(t.reshape(*lead, n, Hkv * D).to(dtype) for t in (k, v))

    def __init__(self, q, k, v, allowed, num_heads, num_kv_heads=None, bias=None, kv_head=None, uniform=None, counts=(0, 0)):
        R, d = q.shape
        H, Hkv = num_heads, num_kv_heads or num_heads
        D, G, N = d // H, H // Hkv, k.shape[1]
        assert k.shape == v.shape == (R, N, Hkv * D) and allowed.shape == (R, N), (q.shape, k.shape, v.shape, allowed.shape)
        dev = q.device
        kv_head = kv_head or (lambda h: h // G)
        ok = allowed.to(dev).bool()
        uni = torch.ones_like(ok) if uniform is None else uniform.to(dev).bool()
        live = ok.any(1)
        q3, k4, v4 = q.double().reshape(R, H, D), k.reshape(R, N, Hkv, D), v.reshape(R, N, Hkv, D)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
        self.R, self.H, self.Hkv, self.D, self.N = R, H, Hkv, D, N
        self.n_s, self.n_c = counts
        self.allowed = ok
        self.want, self.mag, self.S = z(R, H, D), z(R, H, D), z(R, H)
        fill = torch.where(uni, 0.0, float("-inf")).double()
        for h in range(H):
            K, V = k4[:, :, kv_head(h)].double(), v4[:, :, kv_head(h)].double()
            sc = torch.einsum("rd,rnd->rn", q3[:, h], K)
            sa = torch.einsum("rd,rnd->rn", q3[:, h].abs(), K.abs())
            if bias is not None:
                sc = sc + bias[h].to(dev).double()[None]
                sa = sa + bias[h].to(dev).double().abs()[None]
            self.S[:, h] = sa.masked_fill(~ok, 0.0).amax(1)
            sc = torch.where(live[:, None], sc.masked_fill(~ok, float("-inf")), fill)
            p = torch.softmax(sc, 1)
            self.want[:, h] = torch.einsum("rn,rnd->rd", p, V)
            self.mag[:, h] = torch.einsum("rn,rnd->rd", p, V.abs())

    def bound(self, dtype):
        """[R,H,D]."""
        return U[dtype] * self.want.abs() + ((self.n_s * self.S + self.n_c) * 2.0 ** -24)[..., None] * self.mag

    def outside(self, other, dtype):
        """From two references alone: the elements [R,H,D] at which `other` -- a deliberately wrong reference of the same call --
        leaves this one's bound."""
        return outside(self.want, other.want, self.bound(dtype))

    def affected(self, other):
        """[R] bool: the rows `other` does not reproduce bit for bit (a wrong reference that cannot reach a row leaves it as it is)."""
        return (other.want != self.want).flatten(1).any(1)

    def check(self, got, what, group="", dtype=None, rows=None):
        """Asserts the bound on every element of got [R, H*D] (rows [R] bool: those rows alone); prints and returns the largest
        err / bound and names (row, head) on failure."""
        select = None if rows is None else rows.to(self.want.device).bool()[:, None, None]
        return check_bound(got, self.want, self.bound(dtype or got.dtype), what, group, row_head, select)
