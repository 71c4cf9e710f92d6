"""The cases of tests/test_decode_attn_bounds_gpu.py, built on the CPU so that tests/test_decode_attn_ref_cpu.py can hold the same
cases' references, deliberately wrong references and fp32 emulation without a GPU.  One class per entry-point family of csrc/decode.hip;
each holds the storage-rounded operands in the kernel's own layout, expands them for decode_ref.DecodeAttnRef (`ref(wrong=None, dev)`) and
calls the kernel through its ops wrapper (`run(dev)`).

A wrong reference is named; `wrongs()` lists the names a case can tell apart from the right one, `blind()` those it cannot BY
CONSTRUCTION, with the reason -- never by a threshold:
  generic      "drop@<e>" (one dropped key at an edge position of the expanded list), "lane group" (the keys of the last lane group of
               the cache phase: s % 4KPI = 4KPI - 1), "wave" (those of the last wave: (s / KPI) % 4 = 3), "mask+1" (the mask shifted by
               one key), "kv head" (the neighbouring key/value head, (h // G + 1) % Hkv)
  beam         "src identity", "src column+1", "other prefix", "uniform prefix"
  block        "j<i", "len+1", "len-1", "slot+1" (a (token, head) pair's query taken from the neighbouring block slot)
  q8           "exps swapped", "exps zero", "exps neighbour head", "new row quantised"
  relbias      "distance s", "head h^1", "no bias" """
import torch

import kvq_ref
from bounds import BF16, F32, NAN
from decode_ref import DecodeAttnRef, decode_bias_relbias, decode_geometry, decode_rows_beam, decode_rows_block, decode_rows_cache, decode_rows_q8

HUGE = 1e30                      # tests/test_xattn_bounds_gpu.py group D: what a masked key may hold
CAP = 0.25                       # the share of the affected elements a wrong reference must push outside the bound
NAN_CODE, FILL_EXP = 0x7F, 77    # an e4m3fn NaN and an exponent no case produces: the unwritten part of a quantised cache


def trip(kernel, dtype, D):
    """(I, KPI, TAIL): keys per workgroup loop trip, per wave and load instruction, per trip of the beam tail (AD_WAVES KPI TAIL_UNROLL)."""
    _, _, kpi, I = decode_geometry(kernel, dtype, D)
    return I, kpi, 8 * kpi


def gqa_plan(G, most=8):
    """attn_decode_gqa_nq / attn_decode_gqa_q8_nq (most = 4): (nblk, qpb, NQ instantiation, heads per block)."""
    nblk = -(-G // most)
    qpb = -(-G // nblk)
    nq = 1 if qpb == 1 else 2 if qpb == 2 else 4 if qpb <= 4 else 8
    return nblk, qpb, nq, [min(qpb, G - b * qpb) for b in range(nblk)]


def pair_plan(B, Hkv, m, G, num_cu):
    """attn_decode_gqa_block_nq: (nblk, ppb, NQ, pairs per block) for P = m G (token, head) pairs; the blocks shrink 8 -> 4 -> 2 -> 1
    while the grid stays within two workgroups per CU."""
    P, room, most = m * G, 2 * num_cu, 8
    while most > 1 and B * Hkv * -(-P // (most // 2)) <= room:
        most //= 2
    nblk = -(-P // most)
    ppb = -(-P // nblk)
    nq = 1 if ppb == 1 else 2 if ppb == 2 else 4 if ppb <= 4 else 8
    return nblk, ppb, nq, [min(ppb, P - b * ppb) for b in range(nblk)]


def mask_layouts(kernel, dtype, D, B, S, first=0):
    """valid [B,S] bool.  Sample b has layout (first + b) % 3:  0 all valid;  1 holed: the edge keys KPI-1, 4KPI, I-1, I, key S-1 and
    every key s % 5 == 3 masked (key 0 stays, and S = 1 keeps its key);  2 no valid key."""
    I, kpi, _ = trip(kernel, dtype, D)
    ok = torch.ones(B, S, dtype=torch.bool)
    s = torch.arange(S)
    for b in range(B):
        lay = (first + b) % 3
        if lay == 1 and S > 1:
            ok[b, (s % 5 == 3) | (s == S - 1) | (s == kpi - 1) | (s == 4 * kpi) | (s == I - 1) | (s == I)] = False
            ok[b, 0] = True
        elif lay == 2:
            ok[b] = False
    return ok


class Case:
    kernel = None
    GENERIC = ("lane group", "wave", "mask+1", "kv head")

    def _init(self, dtype, D, H, Hkv, S, n_tail=0):
        self.dtype, self.D, self.H, self.Hkv, self.G = dtype, D, H, Hkv, H // Hkv
        self.S1 = S                                             # keys of the cache / prefix phase in the expanded list
        self.counts = DecodeAttnRef.counts(self.kernel, dtype, D, S, n_tail)
        self.I, self.KPI, self.TAIL = trip(self.kernel, dtype, D)

    # ---- to be provided: expand(wrong, dev) -> dict(q, k, v, allowed, uniform, bias), edge_positions(), own wrong names
    OWN = ()

    def rows(self):
        """[R] bool: the rows whose output the header specifies."""
        return torch.ones(self.q.shape[0], dtype=torch.bool)

    def ref(self, wrong=None, dev="cpu"):
        generic = wrong is not None and (wrong in Case.GENERIC or wrong.startswith("drop@"))
        x = self.expand(None if generic else wrong, dev)
        ok, kv_head = x["allowed"].clone(), None
        if generic:
            if wrong.startswith("drop@") or wrong in ("lane group", "wave"):
                ok[:, self._keys(wrong, ok.shape[1]).to(ok.device)] = False
            elif wrong == "mask+1":
                ok = torch.roll(ok, 1, 1)
            else:
                kv_head = lambda h: (h // self.G + 1) % self.Hkv
        return DecodeAttnRef(x["q"], x["k"], x["v"], ok, self.H, self.Hkv, bias=x.get("bias"), kv_head=kv_head,
                             uniform=x.get("uniform"), counts=self.counts)

    def _keys(self, wrong, N):
        """[N] bool: the keys of the expanded list that a key-dropping wrong reference drops."""
        s = torch.arange(N)
        if wrong == "lane group":
            return (s < self.S1) & (s % (4 * self.KPI) == 4 * self.KPI - 1)
        if wrong == "wave":
            return (s < self.S1) & ((s // self.KPI) % 4 == 3)
        return s == int(wrong[5:])

    def blind(self):
        """name -> why this case cannot tell that wrong reference from the right one."""
        b = {}
        if self.S1 < 4 * self.KPI:
            b["lane group"] = b["wave"] = "fewer than 4 KPI keys: the last lane group and wave hold none"
        if self.Hkv == 1:
            b["kv head"] = "one key/value head"
        return b

    def wrongs(self, right):
        """The wrong references this case can tell from `right`.  Left out by construction: blind(); dropped keys that no specified
        row is allowed; the shifted mask where the shift maps the mask onto itself."""
        ok = right.allowed[self.rows().to(right.allowed.device)].cpu()
        names = [f"drop@{e}" for e in self.edge_positions()] + list(Case.GENERIC) + list(self.OWN)
        names = [n for n in names if not (n.startswith("drop@") or n in ("lane group", "wave")) or bool(ok[:, self._keys(n, ok.shape[1])].any())]
        if torch.equal(torch.roll(ok, 1, 1), ok):
            names.remove("mask+1")
        return [n for n in names if n not in self.blind()]

    def share(self, right, wrong, dev="cpu", dtype=None):
        """From the references alone: (share of the elements of the affected, specified rows that `wrong` puts outside the bound,
        number of those rows)."""
        other = self.ref(wrong, dev)
        hit = right.affected(other) & self.rows().to(right.want.device)
        n = int(hit.sum())
        return (right.outside(other, dtype or self.dtype)[hit].double().mean().item() if n else 0.0), n

    def assert_can_fail(self, right, dev="cpu"):
        """At least CAP of the affected elements of at least one wrong reference of the case's kind lie outside the bound; for bf16 the
        bound is nowhere tighter than the store's own half ulp.  Returns the name that showed it."""
        if self.dtype == BF16:
            tight = (right.bound(BF16) < 2.0 ** -9 * right.want.abs()).double().mean().item()
            assert tight == 0.0, f"{self.what}: {tight:.3f} of the elements have a bound below the bf16 half ulp"
        seen = {}
        for name in self.wrongs(right):
            seen[name], n = self.share(right, name, dev)
            if n and seen[name] >= CAP:
                return name
        raise AssertionError(f"{self.what}: no wrong reference leaves the bound on {CAP:.0%} of what it reaches: {seen}")


# ------------------------------------------------------------------------------------------ plain, GQA
class CacheCase(Case):
    """mmgl_attn_decode_fwd (Hkv = H) and mmgl_attn_decode_gqa_fwd: B samples of the three mask layouts."""

    def __init__(self, dtype, D, S, H=2, Hkv=None, B=3, first=0, order=None, huge=False, seed=0, force_gqa=False):
        Hkv = Hkv or H
        self.kernel = "gqa" if (Hkv != H or force_gqa) else "plain"
        self._init(dtype, D, H, Hkv, S)
        self.force_gqa = force_gqa
        self.what = f"{self.kernel} {'bf16' if dtype == BF16 else 'fp32'} D={D} S={S} H={H} Hkv={Hkv} B={B}" + (f" {order}" if order else "") + (" huge" if huge else "")
        self.q = DecodeAttnRef.inputs(dtype, B, H, D, seed)
        self.k, self.v = DecodeAttnRef.keys(dtype, (B,), S, Hkv, D, self.edge_positions(), seed, order)
        self.valid = mask_layouts(self.kernel, dtype, D, B, S, first) if order is None else torch.ones(B, S, dtype=torch.bool)
        if huge:
            dead = ~self.valid & self.valid.any(1, keepdim=True)
            self.k[dead], self.v[dead] = HUGE, -HUGE

    def edge_positions(self):
        return DecodeAttnRef.edges(self.kernel, self.dtype, self.D, self.S1)

    def blind(self):
        b = super().blind()
        if self.S1 == 1:
            for n in ("drop@0", "mask+1"):
                b[n] = "S = 1: a row without an allowed key is uniform over the same one key"
        return b

    def expand(self, wrong, dev):
        assert wrong is None, wrong
        k, v, ok, uni = decode_rows_cache(self.k.to(dev), self.v.to(dev), self.valid.to(dev))
        return dict(q=self.q.to(dev), k=k, v=v, allowed=ok, uniform=uni)

    def run(self, dev):
        from mmgl_amd import ops
        kd = self.Hkv * self.D
        cache = torch.cat([self.k, self.v], -1).to(dev)
        q, valid = self.q.to(dev), self.valid.to(dev)
        out = torch.full_like(q, NAN)
        if self.force_gqa and self.Hkv == self.H:               # G = 1 through the GQA entry: the wrapper routes it to the plain kernel
            B = q.shape[0]
            k, v, ok = cache[..., :kd], cache[..., kd:], valid.to(torch.uint8)
            ops._lib.call("mmgl_attn_decode_gqa_fwd", dict(bytes=0.0), ops.ptr(q), q.stride(0), ops.ptr(k), ops.ptr(v), k.stride(1), k.stride(0),
                          ops.ptr(ok), ok.stride(0), ops.ptr(out), B, self.H, self.Hkv, self.S1, self.D, ops.dtype_code(q), ops.stream_ptr())
            return out
        got = ops.attn_decode(q, cache[..., :kd], cache[..., kd:], valid, self.H, out=out, num_kv_heads=None if self.Hkv == self.H else self.Hkv)
        assert got is out
        return out


# ------------------------------------------------------------------------------------------ relbias
class RelbiasCase(Case):
    kernel = "relbias"
    OWN = ("distance s", "head h^1", "no bias")
    NUM_BUCKETS, MAX_DISTANCE = 32, 128

    def __init__(self, dtype, D, S, H=2, B=2, few=False, seed=0, order=None):
        from mmgl_amd import ops
        self._init(dtype, D, H, H, S)
        self.few = few
        self.what = f"relbias {'bf16' if dtype == BF16 else 'fp32'} D={D} S={S} H={H}" + (" few distances" if few else "") + (f" {order}" if order else "")
        self.q = DecodeAttnRef.inputs(dtype, B, H, D, seed)
        self.k, self.v = DecodeAttnRef.keys(dtype, (B,), S, H, D, self.edge_positions(), seed, order)
        g = torch.Generator().manual_seed(seed + 31)
        table = torch.randn(self.NUM_BUCKETS, H, generator=g) * 2.0
        self.bias = ops.t5_decode_bias(table, S + 5, self.NUM_BUCKETS, self.MAX_DISTANCE)           # fp32 [H, S + 5]: ld_bias > S
        self.open = torch.ones(S, dtype=torch.bool)                                                  # by distance
        if few:
            self.open[:] = False
            self.open[[d for d in (0, 1, self.KPI, S - 1) if d < S]] = True
            self.bias[:, :S][:, ~self.open] = -HUGE

    def edge_positions(self):
        return DecodeAttnRef.edges("relbias", self.dtype, self.D, self.S1)

    def blind(self):
        b = super().blind()
        if self.S1 == 1:
            for n in ("drop@0", "mask+1") + self.OWN:
                b[n] = "S = 1: over one key the softmax is 1 whatever the score"
        if self.S1 == 2:
            for n in self.OWN:
                b[n] = "S = 2: only the difference of two bias words counts, so a wrong reference can coincide with the right one"
        if self.few:
            b["distance s"] = b["mask+1"] = "the open distances decide the keys: another test's subject (test_decode_relbias_gpu a)"
        if self.H == 1:
            b["head h^1"] = "one head"
        return b

    def expand(self, wrong, dev):
        k, v, ok, uni = decode_rows_cache(self.k.to(dev), self.v.to(dev), torch.ones(self.k.shape[:2], dtype=torch.bool))
        bias = decode_bias_relbias(self.bias, self.S1, wrong)
        if self.few:            # exp(-1e30 - m) is 0 in fp32 and in fp64: such a key is not allowed, and its bias word reaches nothing
            shut = (~self.open).flip(0)
            ok = ok.clone()
            ok[:, shut.to(ok.device)] = False
            bias = bias.masked_fill(bias <= -HUGE / 2, 0.0)
        return dict(q=self.q.to(dev), k=k, v=v, allowed=ok.to(dev), uniform=uni.to(dev), bias=bias.to(dev))

    def run(self, dev):
        from mmgl_amd import ops
        d = self.H * self.D
        cache = torch.cat([self.k, self.v], -1).to(dev)
        q = self.q.to(dev)
        out = torch.full_like(q, NAN)
        assert ops.attn_decode_relbias(q, cache[..., :d], cache[..., d:], self.bias.to(dev), self.H, out=out) is out
        return out


# ------------------------------------------------------------------------------------------ beam
class BeamCase(Case):
    kernel = "beam"
    OWN = ("src identity", "src column+1", "other prefix", "uniform prefix")

    def __init__(self, dtype, D, W, S, n_tail, pattern="perm", valid="ragged", H=2, B=2, seed=0, order=None):
        self._init(dtype, D, H, H, S, n_tail)
        self.W, self.n_tail, self.pattern, self.valid_kind, self.B = W, n_tail, pattern, valid, B
        self.what = f"beam {'bf16' if dtype == BF16 else 'fp32'} D={D} W={W} S={S} n_tail={n_tail} {pattern} {valid}"
        R = B * W
        self.n_cap = n_cap = max(n_tail, 1) + 3
        self.q = DecodeAttnRef.inputs(dtype, R, H, D, seed)
        self.k, self.v = DecodeAttnRef.keys(dtype, (B,), S, H, D, DecodeAttnRef.edges("beam", dtype, D, S), seed, order)
        te = sorted({e for e in (0, self.KPI - 1, self.KPI, self.TAIL - 1, self.TAIL, n_tail - 1) if 0 <= e < n_tail})
        self.kt, self.vt = DecodeAttnRef.keys(dtype, (R,), n_cap, H, D, te, seed + 1, order)
        self.tail_edges = te
        self.valid = torch.ones(B, S, dtype=torch.bool)
        if valid == "ragged" and S > 2 and B > 1:
            self.valid[1, S - max(S // 5, 1):] = False
        elif valid == "none":
            self.valid[0] = False
        src = torch.zeros(R, n_cap, dtype=torch.int32)
        for b in range(B):
            rows = slice(b * W, (b + 1) * W)
            if pattern == "perm":
                src[rows] = (torch.roll(torch.arange(W), 1) if W > 1 else torch.zeros(1, dtype=torch.long))[:, None].int()
            elif pattern == "one":
                src[rows] = W - 1
            else:
                for j in range(n_cap):
                    src[rows, j] = ((torch.arange(W) + 1 + (j + b) % max(W - 1, 1)) % W).int()      # never the identity
        self.src = src

    def edge_positions(self):
        return DecodeAttnRef.edges("beam", self.dtype, self.D, self.S1) + [self.S1 + e for e in self.tail_edges]

    def blind(self):
        b = super().blind()
        if self.W == 1 or not self.n_tail:
            b["src identity"] = "one beam or no tail: every table reads the same keys"
        if self.W == 1 or self.n_tail < 2 or self.pattern != "history":
            b["src column+1"] = "the table's columns are equal (or there is one)"
        if self.valid_kind != "none" or not self.n_tail:
            b["uniform prefix"] = "no sample without a valid prefix key, or no tail to leave out"
        if self.S1 == 1 and not self.n_tail:
            b["drop@0"] = b["mask+1"] = "one key"
        return b

    def expand(self, wrong, dev):
        n = self.n_tail
        k, v, ok, src = self.k, self.v, self.valid, self.src.clone()
        if wrong == "other prefix":
            k, v, ok = k.flip(0), v.flip(0), ok.flip(0)
        elif wrong == "src identity":
            src[:] = (torch.arange(src.shape[0]) % self.W).int()[:, None]
        elif wrong == "src column+1":
            src[:, :n] = torch.roll(src[:, :n], -1, 1)
        else:
            assert wrong in (None, "uniform prefix"), wrong
        k, v, ok, uni = decode_rows_beam(k.to(dev), v.to(dev), ok.to(dev), self.W, self.kt[:, :n].to(dev) if n else None,
                                         self.vt[:, :n].to(dev) if n else None, src.to(dev), uniform_tail=wrong != "uniform prefix")
        return dict(q=self.q.to(dev), k=k, v=v, allowed=ok, uniform=uni)

    def run(self, dev):
        from mmgl_amd import ops
        d, n = self.H * self.D, self.n_tail
        pre, tail = torch.cat([self.k, self.v], -1).to(dev), torch.cat([self.kt, self.vt], -1).to(dev)
        q = self.q.to(dev)
        out = torch.full_like(q, NAN)
        got = ops.attn_decode_beam(q, pre[..., :d], pre[..., d:], self.valid.to(dev), self.H, self.W, tail[:, :n, :d] if n else None,
                                   tail[:, :n, d:] if n else None, self.src.to(dev) if n else None, out=out)
        assert got is out
        return out


# ------------------------------------------------------------------------------------------ block, GQA block
class BlockCase(Case):
    """mmgl_attn_decode_block_fwd (G = 1 and gqa=False: the new keys come dense and the kernel files them) and
    mmgl_attn_decode_gqa_block_fwd (the cache holds the new columns already).  lens: per sample, in [0, cap]."""
    OWN = ("j<i", "len+1", "len-1", "slot+1")

    def __init__(self, dtype, D, m, lens, cap, G=1, Hkv=2, gqa=False, seed=0):
        self.kernel = "gqa_block" if gqa else "block"
        assert gqa or G == 1
        B, H = len(lens), Hkv * G
        self._init(dtype, D, H, Hkv, cap)
        self.counts = DecodeAttnRef.counts(self.kernel, dtype, D, min(max(lens), cap))
        self.m, self.cap, self.B = m, cap, B
        self.lens = torch.tensor(lens, dtype=torch.int32)
        assert int(self.lens.min()) >= 0 and int(self.lens.max()) <= cap
        self.what = f"{self.kernel} {'bf16' if dtype == BF16 else 'fp32'} D={D} m={m} G={G} Hkv={Hkv} lens={list(lens[:4])}{f' repeated over B={B}' if B > 4 else ''} cap={cap}"
        self.q = DecodeAttnRef.inputs(dtype, B * m, H, D, seed)
        edges = DecodeAttnRef.edges(self.kernel, dtype, D, cap, extra=[l - 1 for l in lens])
        self.k, self.v = DecodeAttnRef.keys(dtype, (B,), cap, Hkv, D, edges, seed)                   # finite everywhere: columns >= len too
        kn, vn = DecodeAttnRef.keys(dtype, (B,), m, Hkv, D, (0, m - 1), seed + 1)
        self.k_new, self.v_new = kn.reshape(B * m, -1), vn.reshape(B * m, -1)
        self.valid = mask_layouts(self.kernel, dtype, D, B, cap, first=0)
        self.valid[self.valid.any(1).logical_not()] = True      # the new keys are always valid: a sample without a valid CACHE key is the lens = 0 case
        if B > 1:
            self.valid[1, ::7] = False
        if gqa:                                                  # rope_kv_append_block ran first: the new columns below the capacity are filed
            for b in range(B):
                for t in range(m):
                    if lens[b] + t < cap:
                        self.k[b, lens[b] + t], self.v[b, lens[b] + t] = self.k_new[b * m + t], self.v_new[b * m + t]

    def edge_positions(self):
        live = [e for e in DecodeAttnRef.edges(self.kernel, self.dtype, self.D, self.cap, extra=[int(l) - 1 for l in self.lens])
                if e < int(self.lens.max())]
        return live + [self.cap, self.cap + self.m - 1][:self.m]

    def rows(self):
        """A row whose own column lens[b] + i is at or past the capacity has an unspecified output."""
        i = torch.arange(self.m)
        return ((self.lens[:, None].long() + i[None, :]) < self.cap).reshape(-1)

    def blind(self):
        b = super().blind()
        if int(self.lens.max()) < 4 * self.KPI:
            b["lane group"] = b["wave"] = "fewer than 4 KPI cached keys"
        if self.m * self.G == 1:
            b["slot+1"] = "one (token, head) pair"
        return b

    def expand(self, wrong, dev):
        lens, q = self.lens.clone(), self.q
        if wrong == "len+1":
            lens = (lens + 1).clamp(max=self.cap)
        elif wrong == "len-1":
            lens = (lens - 1).clamp(min=0)
        elif wrong == "slot+1":                                  # pair p = i G + g of a key/value head reads the query of pair p + 1
            B, m, G, Hkv, D = self.B, self.m, self.G, self.Hkv, self.D
            q5 = q.reshape(B, m, Hkv, G, D).permute(0, 2, 1, 3, 4).reshape(B, Hkv, m * G, D)
            q = torch.roll(q5, -1, 2).reshape(B, Hkv, m, G, D).permute(0, 2, 1, 3, 4).reshape(B * m, -1)
        else:
            assert wrong in (None, "j<i"), wrong
        k, v, ok, uni = decode_rows_block(self.k.to(dev), self.v.to(dev), self.valid.to(dev), lens.to(dev), self.k_new.to(dev), self.v_new.to(dev),
                                          self.m, strict=wrong == "j<i", below_capacity=self.kernel == "gqa_block")
        return dict(q=q.to(dev), k=k, v=v, allowed=ok, uniform=uni)

    def run(self, dev):
        from mmgl_amd import ops
        kd, m = self.Hkv * self.D, self.m
        cache0 = torch.cat([self.k, self.v], -1)
        cache = cache0.to(dev)
        q, valid, lens = self.q.to(dev), self.valid.to(dev), self.lens.to(dev)
        out = torch.full_like(q, NAN)
        if self.kernel == "block":
            new = torch.cat([self.k_new, self.v_new], -1).to(dev)                                  # the dense [B*m, 2d] projection output
            got = ops.attn_decode_block(q, new[:, :kd], new[:, kd:], cache[..., :kd], cache[..., kd:], valid, lens, self.H, m, out=out)
            want = cache0.clone()                                # the filed columns are k_new | v_new bitwise; no other byte changes
            for b in range(self.B):
                for t in range(m):
                    if int(self.lens[b]) + t < self.cap:
                        want[b, int(self.lens[b]) + t] = torch.cat([self.k_new[b * m + t], self.v_new[b * m + t]])
            assert torch.equal(cache.cpu().view(torch.int16 if self.dtype == BF16 else torch.int32),
                               want.view(torch.int16 if self.dtype == BF16 else torch.int32)), f"{self.what}: the cache after the call"
        else:
            got = ops.attn_decode_gqa_block(q, cache[..., :kd], cache[..., kd:], valid, lens, self.H, self.Hkv, m, out=out)
            assert torch.equal(cache.cpu(), cache0), f"{self.what}: the kernel only reads the cache"
        assert got is out
        return out


# ------------------------------------------------------------------------------------------ q8, GQA q8
class Q8Case(Case):
    """mmgl_attn_decode_q8_fwd (G = 1) and mmgl_attn_decode_gqa_q8_fwd.  Key heads differ by 2^6 (8, 1/8, 8, ...), value heads by 2^6
    the other way, q carries the inverse of its key head's scale: scores stay of order 1 and the exponents differ by head and by
    key against value, as in tests/test_kv_quant_kernels_gpu.py.  valid: "layouts" (mask_layouts) | "one-masked" (every cached key of
    sample 1 masked: its output is the new value row, bitwise)."""
    OWN = ("exps swapped", "exps zero", "exps neighbour head", "new row quantised")

    def __init__(self, dtype, D, S, G=1, Hkv=2, B=2, valid="layouts", seed=0):
        self.kernel = "q8" if G == 1 else "gqa_q8"
        H = Hkv * G
        self._init(dtype, D, H, Hkv, S)
        self.B, self.valid_kind = B, valid
        self.what = f"{self.kernel} {'bf16' if dtype == BF16 else 'fp32'} D={D} S={S} G={G} Hkv={Hkv} {valid}"
        ks = torch.tensor([8.0, 0.125] * Hkv)[:Hkv]
        ksc, vsc = ks.repeat_interleave(D), (1.0 / ks).repeat_interleave(D)
        q = DecodeAttnRef.inputs(F32, B, H, D, seed)
        self.q = (q / ks.repeat_interleave(G).repeat_interleave(D)).to(dtype)
        kc, vc = DecodeAttnRef.keys(F32, (B,), S, Hkv, D, self.edge_positions()[:-1], seed)
        kc, vc = (kc * ksc).to(dtype), (vc * vsc).to(dtype)
        kn, vn = DecodeAttnRef.keys(F32, (B,), 1, Hkv, D, (0,), seed + 1)
        self.k_new, self.v_new = (kn[:, 0] * ksc).to(dtype), (vn[:, 0] * vsc).to(dtype)
        self.codes, self.e = kvq_ref.quantize_row(kc, vc, Hkv)
        assert len(set(self.e[0, 0].tolist())) > 1, "the exponents differ by head or by key against value"
        self.valid = mask_layouts(self.kernel, dtype, D, B, S, first=0)
        self.valid[~self.valid.any(1)] = True
        if valid == "one-masked":
            self.valid[1] = False

    def edge_positions(self):
        return DecodeAttnRef.edges(self.kernel, self.dtype, self.D, self.S1) + [self.S1]

    def blind(self):
        b = super().blind()
        if self.Hkv == 1:
            b["exps neighbour head"] = "one key/value head"
        return b

    def expand(self, wrong, dev):
        e, Hkv = self.e, self.Hkv
        k_new, v_new = self.k_new, self.v_new
        if wrong == "exps swapped":
            e = torch.cat([e[..., Hkv:], e[..., :Hkv]], -1)
        elif wrong == "exps zero":
            e = torch.zeros_like(e)
        elif wrong == "exps neighbour head":
            e = torch.cat([torch.roll(e[..., :Hkv], 1, -1), torch.roll(e[..., Hkv:], 1, -1)], -1)
        elif wrong == "new row quantised":
            c1, e1 = kvq_ref.quantize_row(k_new, v_new, Hkv)
            k_new, v_new = kvq_ref.dequantize_row(c1, e1, Hkv)
        else:
            assert wrong is None, wrong
        k, v, ok, uni = decode_rows_q8(self.codes, e, self.valid, k_new.to(dev), v_new.to(dev), Hkv)
        return dict(q=self.q.to(dev), k=k, v=v, allowed=ok, uniform=uni)

    def run(self, dev):
        from mmgl_amd import ops
        B, S, Hkv, kd = self.B, self.S1, self.Hkv, self.Hkv * self.D
        cap = S + 2
        kvq0 = torch.full((B, cap, 2 * kd), NAN_CODE, dtype=torch.uint8)
        sc0 = torch.full((B, cap, 2 * Hkv), FILL_EXP, dtype=torch.int8)
        kvq0[:, :S], sc0[:, :S] = self.codes, self.e
        kvq, scale = kvq0.to(dev).view(torch.float8_e4m3fn), sc0.to(dev)
        new = torch.cat([self.k_new, self.v_new], 1).to(dev)                                      # the dense [B, 2 kd] projection output
        mask = torch.zeros(B, cap, dtype=torch.bool)
        mask[:, :S] = self.valid
        q = self.q.to(dev)
        out = torch.full_like(q, NAN)
        got = ops.attn_decode_q8(q, new[:, :kd], new[:, kd:], kvq, scale, mask.to(dev)[:, :S], self.H, out=out,
                                 num_kv_heads=None if self.G == 1 else Hkv)
        assert got is out
        new_codes, new_e = kvq_ref.quantize_row(self.k_new, self.v_new, Hkv)                     # column S filed as kvq_ref says, bitwise;
        kvq0[:, S], sc0[:, S] = new_codes, new_e                                                  # every other byte as it was
        assert torch.equal(kvq.view(torch.uint8).cpu(), kvq0) and torch.equal(scale.cpu(), sc0), f"{self.what}: the cache after the call"
        dead = ~self.valid.any(1)
        if dead.any():                                           # all cached keys masked: the new value row, bitwise
            vrow = self.v_new.reshape(B, Hkv, 1, self.D).expand(B, Hkv, self.G, self.D).reshape(B, -1)
            assert torch.equal(out.cpu()[dead].float(), vrow[dead].float()), f"{self.what}: a sample of masked cached keys is not its new value row"
        return out
