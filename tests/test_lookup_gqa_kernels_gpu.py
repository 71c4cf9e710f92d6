"""-m gpu: the two kernels of a prompt-lookup verify step on a grouped-query cache, through ops.rope_kv_append_block and
ops.attn_decode_gqa_block.

Shapes follow _block_case of tests/test_lookup_kernels_gpu.py: capacity = one workgroup loop trip (1024 * vec / D keys) + 37, and one
sample per len in {0, 1, cap - m, a value that drops some of the new columns, cap, trip + 1, 5}; the len = 5 sample has a fully masked
prefix.  Operands are windows of NaN-filled buffers with padded strides, so nothing outside them is read.

rope_kv_append_block: every rotated element within 2^-21 a (fp32) / 2^-8 a (bf16) of the fp64 formula at position len[b] + i, with
a = |x cos| + |y sin| -- DESIGN.md 4.11's bounds for rope_kv_append: the products and their sum are formed in fp32 (each rounding at most
2^-24 of a partial result no larger than a, contraction allowed), then one rounding to the storage type (2^-9 |result| <= 2^-9 a in
bf16, 2^-24 a in fp32); the table's own fp32 entries are the reference's inputs.  Everything else is bitwise.

attn_decode_gqa_block: against an fp64 softmax over K / V expanded with repeat_interleave(G), at the per-sample tolerances of
tests/test_decode_edges_gpu.py (TOL: 1e-3 fp32, 2e-2 bf16 of the sample's largest reference magnitude).  Rows whose own column is at or
past the capacity have an unspecified value and are not compared (they must stay in bounds: the buffers around are NaN and nothing
else may change)."""
import pytest
import torch

from test_decode_edges_gpu import TOL, _attn_check, _per_sample
from test_decode_gqa_kernels_gpu import ROPE_BOUND

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _lens(dtype, D, m):
    vec = 8 if dtype == BF16 else 4
    trip = 1024 * vec // D                                      # keys per workgroup loop trip
    cap = trip + 37
    return [0, 1, cap - m, cap - m + (m + 1) // 2, cap, trip + 1, 5], cap


# ------------------------------------------------------------------------------------------ ops.rope_kv_append_block
def _rope_block_case(dtype, H, Hkv, D, m, seed, short_table):
    lens, cap = _lens(dtype, D, m)
    B, width, nkv2 = len(lens), (H + 2 * Hkv) * D, 2 * Hkv * D
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((B * m + 1, width + 16), NAN, dtype=dtype)
    buf[:B * m, 8:8 + width] = torch.randn(B * m, width, generator=g).to(dtype)
    n_pos = cap - 3 if short_table else cap + 8                 # short: the positions of the last columns are clamped to row n_pos - 1
    ang = torch.rand(n_pos, D // 2, generator=g) * 6.0
    table = torch.stack([ang.cos(), ang.sin()], dim=-1).float().contiguous()
    cache = torch.full((B, cap + 3, nkv2 + 16), NAN, dtype=dtype)
    return buf, table, cache, torch.tensor(lens, dtype=torch.int32), cap


def _rotate_ref(x, rows_cs, heads, D):
    """fp64 rotate_half of x [R, heads*D] by the per-row angles rows_cs [R, D/2, 2]; returns (want, a)."""
    R = x.shape[0]
    xd = x.double().reshape(R, heads, D)
    lo, hi = xd[..., :D // 2], xd[..., D // 2:]
    co, si = rows_cs[:, None, :, 0].double(), rows_cs[:, None, :, 1].double()
    want = torch.cat([lo * co - hi * si, hi * co + lo * si], dim=-1)
    a = torch.cat([(lo * co).abs() + (hi * si).abs(), (hi * co).abs() + (lo * si).abs()], dim=-1)
    return want.reshape(R, heads * D), a.reshape(R, heads * D)


@pytest.mark.parametrize("short_table", [False, True], ids=["table-covers", "table-short"])
@pytest.mark.parametrize("H,Hkv,D,m", [(4, 4, 16, 1), (4, 2, 64, 2), (6, 2, 128, 3), (8, 1, 64, 8), (4, 2, 16, 8), (16, 2, 128, 8)])
@DTYPES
def test_rope_kv_append_block(dtype, H, Hkv, D, m, short_table):
    from mmgl_amd import ops
    buf, table, cache, lens, cap = _rope_block_case(dtype, H, Hkv, D, m, 100 * H + 10 * Hkv + D + m, short_table)
    B, nq, nkv = len(lens), H * D, Hkv * D
    width = nq + 2 * nkv
    n_pos = table.shape[0]
    bg, cg = buf.cuda(), cache.cuda()
    before = cg.clone()
    qkv, kv = bg[:B * m, 8:8 + width], cg[:, :cap, 8:8 + 2 * nkv]
    assert qkv.stride(0) > width and kv.stride(1) > 2 * nkv and kv.stride(0) > cap * kv.stride(1)
    assert ops.rope_kv_append_block(qkv, table.cuda(), kv, lens.cuda(), H, Hkv, m) is qkv
    src = buf[:B * m, 8:8 + width]
    pos = torch.tensor([int(lens[b]) + i for b in range(B) for i in range(m)])
    rows_cs = table[pos.clamp(max=n_pos - 1)]
    assert short_table == bool((pos > n_pos - 1).any()), "the table's clamp is (not) exercised as the case says"
    bound = ROPE_BOUND[dtype]

    def check(name, got, x, heads, cs):
        want, a = _rotate_ref(x, cs, heads, D)
        err = (got.double().cpu() - want).abs()
        ratio = (err / (bound * a).clamp_min(1e-300)).max().item()
        print(f"[rope_kv_append_block] {dtype} H={H} Hkv={Hkv} D={D} m={m} n_pos={n_pos} {name}: max err / bound {ratio:.3f}")
        assert (err <= bound * a).all(), f"{name}: {int((err > bound * a).sum())} elements over the bound (max ratio {ratio:.3f})"
        assert (want - x.double()).abs().max().item() > 0.1, "the rotation is no identity: the check can fail"

    check("q", qkv[:, :nq], src[:, :nq], H, rows_cs)
    assert torch.equal(_bits(qkv[:, nq:].cpu()), _bits(src[:, nq:])), "the k | v blocks of qkv changed"
    assert torch.equal(_bits(bg[:, :8].cpu()), _bits(buf[:, :8])) and torch.equal(_bits(bg[:, 8 + width:].cpu()), _bits(buf[:, 8 + width:]))
    assert torch.equal(_bits(bg[B * m:].cpu()), _bits(buf[B * m:])), "a row behind the B*m rows changed"
    # the cache: column len[b] + i holds row (b, i)'s rotated keys and its values bitwise, when it lies below the capacity; every
    # other byte -- the pad columns of a filed row included -- is as before
    filed = [(b, i) for b in range(B) for i in range(m) if int(lens[b]) + i < cap]
    assert 0 < len(filed) < B * m, "no new column was dropped at the capacity"
    r = torch.tensor([b * m + i for b, i in filed])
    bi, ci = torch.tensor([b for b, _ in filed]), torch.tensor([int(lens[b]) + i for b, i in filed])
    got_kv = cg[bi, ci].cpu()
    check("k", got_kv[:, 8:8 + nkv], src[r, nq:nq + nkv], Hkv, rows_cs[r])
    assert torch.equal(_bits(got_kv[:, 8 + nkv:8 + 2 * nkv]), _bits(src[r, nq + nkv:])), "v did not arrive bitwise"
    expect = before.clone()
    expect[bi, ci, 8:8 + 2 * nkv] = cg[bi, ci, 8:8 + 2 * nkv]
    assert torch.equal(_bits(cg), _bits(expect)), "a cache byte outside the filed columns changed"
    # a second run on the inputs as they were: bitwise the same
    bg2, cg2 = buf.cuda(), cache.cuda()
    ops.rope_kv_append_block(bg2[:B * m, 8:8 + width], table.cuda(), cg2[:, :cap, 8:8 + 2 * nkv], lens.cuda(), H, Hkv, m)
    assert torch.equal(_bits(bg2), _bits(bg)) and torch.equal(_bits(cg2), _bits(cg)), "two runs differ"


@pytest.mark.parametrize("H,Hkv,D", [(4, 2, 64), (8, 1, 16), (4, 4, 128)])
@DTYPES
def test_rope_kv_append_block_of_one_token_is_rope_kv_append_bitwise(dtype, H, Hkv, D):
    from mmgl_amd import ops
    B, cap, col = 3, 9, 4
    g = torch.Generator().manual_seed(D + H)
    width = (H + 2 * Hkv) * D
    src = torch.randn(B, width, generator=g).to(dtype).cuda()
    ang = torch.rand(cap, D // 2, generator=g) * 6.0
    table = torch.stack([ang.cos(), ang.sin()], dim=-1).float().contiguous().cuda()
    one, blk = src.clone(), src.clone()
    cache_one = torch.full((B, cap, 2 * Hkv * D), -3.0, dtype=dtype, device="cuda")
    cache_blk = cache_one.clone()
    ops.rope_kv_append(one, table[col], cache_one[:, col], H, Hkv)
    ops.rope_kv_append_block(blk, table, cache_blk, torch.full((B,), col, dtype=torch.int32, device="cuda"), H, Hkv, 1)
    assert not torch.equal(one, src), "nothing was rotated"
    assert torch.equal(_bits(blk), _bits(one)) and torch.equal(_bits(cache_blk), _bits(cache_one))


def test_rope_kv_append_block_refusals_leave_everything_alone():
    from mmgl_amd import ops
    H, Hkv, D, B, m, cap = 4, 2, 64, 2, 4, 9
    width = (H + 2 * Hkv) * D
    qkv = torch.ones(B * m, width, device="cuda", dtype=BF16)
    table = torch.full((cap, D // 2, 2), 0.5, device="cuda")
    wide = torch.full((B, cap, 2 * Hkv * D + 16), -3.0, device="cuda", dtype=BF16)
    kv = wide[:, :, 8:8 + 2 * Hkv * D]
    lens = torch.full((B,), 3, dtype=torch.int32, device="cuda")
    good = dict(qkv=qkv, cos_sin=table, kv=kv, lens=lens, num_heads=H, num_kv_heads=Hkv, m=m)
    for kw in (dict(m=9), dict(m=0), dict(m=3), dict(num_kv_heads=3), dict(lens=lens.long()), dict(lens=lens[:1]), dict(lens=lens.cpu()),
               dict(cos_sin=table.double()), dict(cos_sin=table[:, :16]), dict(cos_sin=table[0]), dict(kv=wide[:, :, 4:4 + 2 * Hkv * D]),
               dict(kv=wide[:, :, 8:8 + Hkv * D]), dict(kv=kv.float()), dict(kv=kv[:1]),
               dict(qkv=torch.ones(B * m, (H + 2 * Hkv) * 48, device="cuda", dtype=BF16), cos_sin=torch.zeros(cap, 24, 2, device="cuda"),
                    kv=torch.full((B, cap, 4 * 48), -3.0, device="cuda", dtype=BF16))):
        with pytest.raises((ValueError, RuntimeError)):
            ops.rope_kv_append_block(**{**good, **kw})
    torch.cuda.synchronize()
    assert (qkv == 1).all() and (wide == -3.0).all()
    ops.rope_kv_append_block(**good)                                                    # the accepted twin writes
    assert not (qkv[:, :H * D] == 1).all() and (wide[:, 3:3 + m, 8:8 + 2 * Hkv * D] != -3.0).all() and (wide[:, :3] == -3.0).all()


# ------------------------------------------------------------------------------------------ ops.attn_decode_gqa_block
def _attn_case(dtype, H, Hkv, D, m, seed):
    """The cache AFTER the append: sample b holds len[b] filed columns (some masked) and its new columns len[b] .. below the capacity,
    whose mask bytes are 0 -- new columns are always valid, the mask is not read there.  Everything else is NaN."""
    lens, cap = _lens(dtype, D, m)
    B, d, nkv = len(lens), H * D, Hkv * D
    g = torch.Generator().manual_seed(seed)
    qbuf = torch.full((B * m + 1, d + 16), NAN, dtype=dtype)
    qbuf[:B * m, 8:8 + d] = (torch.randn(B * m, d, generator=g) * D ** -0.5).to(dtype)
    cache = torch.full((B, cap + 3, 2 * nkv + 16), NAN, dtype=dtype)
    mask = torch.ones(B, cap + 5, dtype=torch.uint8)
    for b, L in enumerate(lens):
        n = min(L + m, cap)
        cache[b, :n, 8:8 + 2 * nkv] = torch.randn(n, 2 * nkv, generator=g).to(dtype)
        if L > 2:
            mask[b, :L] = torch.rand(L, generator=g) > 0.3      # masked prefix keys
            mask[b, 0] = 1
        mask[b, L:] = 0
    mask[6, :5] = 0                                             # a prefix without any valid key: the new keys carry the row
    return qbuf, cache, mask, torch.tensor(lens, dtype=torch.int32), cap


def _attn_ref(q, k, v, mask, lens, m, H, Hkv, cap, shift=0):
    """fp64: row (b, i), query head h, over key/value head (h // G + shift) % Hkv -- the valid cache columns below len[b] and the new
    columns len[b] .. len[b] + i.  Returns (out [B*m, d], the rows whose own column lies below the capacity)."""
    B, d = k.shape[0], q.shape[1]
    D, G = d // H, H // Hkv
    heads = (torch.arange(H) // G + shift) % Hkv
    out = torch.zeros(B * m, d, dtype=torch.float64)
    live = torch.zeros(B * m, dtype=torch.bool)
    for b in range(B):
        L = int(lens[b])
        keep = torch.cat([mask[b, :L].bool(), torch.ones(m, dtype=torch.bool)])
        for i in range(m):
            if L + i >= cap:
                continue
            live[b * m + i] = True
            sel = keep[:L + i + 1]
            kk = k[b, :L + i + 1][sel].double().view(-1, Hkv, D)[:, heads]                # = repeat_interleave(G) at shift 0
            vv = v[b, :L + i + 1][sel].double().view(-1, Hkv, D)[:, heads]
            p = torch.softmax(torch.einsum("hd,shd->hs", q[b * m + i].double().view(H, D), kk), -1)
            out[b * m + i] = torch.einsum("hs,shd->hd", p, vv).reshape(d)
    return out, live


def _check_rows(got, want, live, B, m, dtype, what, group):
    for b in range(B):
        rows = [b * m + i for i in range(m) if live[b * m + i]]
        if rows:
            _attn_check(got[rows].reshape(1, -1), want[rows].reshape(1, -1).to(got.device), dtype, f"{what} sample {b}", group)


# G = H / Hkv in {1, 2, 3, 4, 8}, m in {1, 2, 3, 8}, D in {16, 64, 128}: every value of each.  The launcher cuts the m*G pairs of a
# (sample, key/value head) into blocks of at most 8 / 4 / 2 / 1 pairs, the smallest that keeps the grid within two workgroups per CU
# (512 on the 256 CUs of an MI355X).  With the B = 7 samples of a case the first 16 shapes run blocks of 1 and 2 pairs; the last six
# have the key/value heads to reach the others: 4 pairs (7*8 heads, 24 pairs in 6 blocks), 4 with a surplus pair (7*16 heads, 9 pairs in
# 3 blocks of 3), 8 pairs (64 pairs in 8 blocks; D = 16 and 128) and 8 with a surplus pair (42 pairs in 6 blocks of 7).
GQA_CASES = [(4, 4, 64, 1), (2, 2, 16, 3), (4, 4, 128, 8), (4, 2, 64, 2), (4, 2, 16, 8), (6, 2, 128, 3), (6, 2, 16, 1), (8, 2, 128, 2),
             (8, 2, 64, 8), (16, 2, 128, 1), (16, 2, 128, 8), (16, 2, 64, 3), (16, 2, 16, 2), (6, 2, 64, 8), (8, 2, 16, 3), (8, 1, 64, 1),
             (64, 8, 16, 3), (48, 16, 16, 3), (64, 8, 16, 8), (64, 8, 128, 8), (48, 8, 64, 7), (64, 8, 64, 2)]


@pytest.mark.parametrize("H,Hkv,D,m", GQA_CASES)
@DTYPES
def test_attn_decode_gqa_block(dtype, H, Hkv, D, m):
    from mmgl_amd import ops
    qbuf, cache, mask, lens, cap = _attn_case(dtype, H, Hkv, D, m, 1000 * D + 10 * H + m)
    B, d, nkv, G = len(lens), H * D, Hkv * D, H // Hkv
    q_c, k_c, v_c = qbuf[:B * m, 8:8 + d], cache[:, :cap, 8:8 + nkv], cache[:, :cap, 8 + nkv:8 + 2 * nkv]
    want, live = _attn_ref(q_c, k_c, v_c, mask, lens, m, H, Hkv, cap)
    assert live.any() and not live.all()
    if Hkv > 1:                                                 # from the reference alone: the neighbouring key/value head is far away
        wrong, _ = _attn_ref(q_c, k_c, v_c, mask, lens, m, H, Hkv, cap, shift=1)
        for b in range(B):
            rows = [b * m + i for i in range(m) if live[b * m + i]]
            if rows:
                far = _per_sample(wrong[rows].reshape(1, -1), want[rows].reshape(1, -1)).item()
                assert far >= 10 * TOL[dtype], f"sample {b}: the neighbouring head is only {far:.2e} away"
    qg, cg, mg, lg = qbuf.cuda(), cache.cuda(), mask.cuda(), lens.cuda()
    before = cg.clone()
    q, k, v, valid = qg[:B * m, 8:8 + d], cg[:, :cap, 8:8 + nkv], cg[:, :cap, 8 + nkv:8 + 2 * nkv], mg[:, :cap]
    assert q.stride(0) > d and k.stride(1) > 2 * nkv and valid.stride(0) > cap
    got = ops.attn_decode_gqa_block(q, k, v, valid, lg, H, Hkv, m)
    assert got.shape == (B * m, d) and got.dtype == dtype
    what = f"{dtype} H={H} Hkv={Hkv} D={D} m={m} cap={cap}"
    _check_rows(got, want, live, B, m, dtype, what, "gqa block")
    assert torch.equal(_bits(cg), _bits(before)), "the cache changed"
    assert torch.equal(_bits(ops.attn_decode_gqa_block(q, k, v, valid, lg, H, Hkv, m)), _bits(got)), "two runs differ"
    # the kernels this one generalises, on the same cache against the same reference at the same tolerance.  Bitwise equality is not
    # expected (tests/test_lookup_kernels_gpu.py says why: another rescale rhythm, and here another order of the keys).
    if m == 1:
        ones = torch.ones(B, cap, dtype=torch.uint8, device="cuda")
        seen = torch.where(torch.arange(cap, device="cuda")[None] < lg[:, None], valid, ones)      # the new column counts as valid
        for b in range(B):
            L = int(lens[b])
            if L < cap:
                one = ops.attn_decode(q[b:b + 1], k[b:b + 1, :L + 1], v[b:b + 1, :L + 1], seen[b:b + 1, :L + 1], H, num_kv_heads=Hkv)
                _attn_check(one, want[b:b + 1].cuda(), dtype, f"attn_decode {what} len={L}", "gqa block m=1")
    if G == 1:
        new = torch.zeros(B * m, 2 * d, dtype=dtype)
        for b in range(B):
            n = min(int(lens[b]) + m, cap) - int(lens[b])
            new[b * m:b * m + n] = cache[b, int(lens[b]):int(lens[b]) + n, 8:8 + 2 * d]
        ng = new.cuda()
        blk = ops.attn_decode_block(q, ng[:, :d], ng[:, d:], k, v, valid, lg, H, m)
        _check_rows(blk, want, live, B, m, dtype, f"attn_decode_block {what}", "gqa block G=1")
        assert torch.equal(_bits(cg), _bits(before)), "attn_decode_block filed other bytes than the cache already held"


def test_attn_decode_gqa_block_refusals_leave_out_alone():
    from mmgl_amd import ops
    B, m, H, Hkv, D, cap = 2, 4, 4, 2, 64, 9
    d, nkv = H * D, Hkv * D
    ones = lambda *shape: torch.ones(*shape, device="cuda", dtype=BF16)
    cache, qkv = ones(B, cap, 2 * nkv + 16), ones(B * m, d + 2 * nkv + 16)
    valid, lens = torch.ones(B, cap, dtype=torch.bool, device="cuda"), torch.full((B,), 3, dtype=torch.int32, device="cuda")
    before = cache.clone()
    good = dict(q=qkv[:, :d], k=cache[:, :, :nkv], v=cache[:, :, nkv:2 * nkv], key_valid=valid, lens=lens, num_heads=H, num_kv_heads=Hkv, m=m)

    def refused(**kw):
        out = torch.full((B * m, d), 7.0, device="cuda", dtype=BF16)
        with pytest.raises((ValueError, RuntimeError)):
            ops.attn_decode_gqa_block(**{**good, **kw}, out=out)
        torch.cuda.synchronize()
        assert torch.equal(out, torch.full_like(out, 7.0)) and torch.equal(cache, before)

    refused(m=9)
    refused(m=0)
    refused(m=2)                                                                       # q rows are not B * m
    refused(num_kv_heads=3)                                                            # H % Hkv != 0
    refused(num_kv_heads=4)                                                            # the cache rows hold 2 heads
    wide = ones(B * m, 4 * 48 + 16)                                                    # D = 48
    c48 = ones(B, cap, 4 * 48)
    refused(q=wide[:, :4 * 48], k=c48[:, :, :2 * 48], v=c48[:, :, 2 * 48:])
    refused(q=qkv[:, 4:4 + d])                                                         # q 8-byte aligned
    refused(k=cache[:, :, 4:4 + nkv], v=cache[:, :, 4 + nkv:4 + 2 * nkv])              # k, v 8-byte aligned
    odd = ones(B, cap, 2 * nkv + 4)
    refused(k=odd[:, :, :nkv], v=odd[:, :, nkv:2 * nkv])                               # a row stride of 8 bytes more
    refused(lens=lens.cpu())                                                           # len on the host
    refused(lens=lens.long())
    refused(lens=lens[:1])
    refused(key_valid=valid[:, :5])
    refused(k=cache[:, :, :nkv].float(), v=cache[:, :, nkv:2 * nkv].float())
    out = torch.full((B * m, d), 7.0, device="cuda", dtype=BF16)
    assert ops.attn_decode_gqa_block(**good, out=out) is out
    assert torch.equal(out, torch.ones_like(out)) and torch.equal(cache, before)        # the accepted twin: every value row is ones
