"""-m gpu: the two kernels of prompt-lookup decoding.

ops.lookup_accept against tests/lookup_ref.py, exactly, on every tensor it writes: logits with distinct values (integers in a random
order: exact in bf16 too), ragged prompt masks with a hole, rows in every state (fresh, mid-generation, finished), blocks whose drafts
the logits accept in full, in part or not at all, EOS among the accepted tokens.  Two runs are bitwise equal.

ops.attn_decode_block against an fp64 softmax of the same storage-rounded operands with the tolerance and the per-sample measure of
tests/test_decode_edges_gpu.py (TOL, _attn_check: 1e-3 fp32 / 2e-2 bf16 of the sample's largest reference magnitude).  Operands are
windows of buffers that hold NaN everywhere else -- the cache rows from len[b] on included -- so nothing outside them is read; the
cache afterwards equals the cache before except for the filed columns, which hold k_new / v_new bitwise."""
import pytest
import torch

from lookup_ref import lookup_accept_ref
from test_decode_edges_gpu import _attn_check

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
KEYS = ("block", "n_draft", "positions", "ids", "gen", "lens", "finished", "emitted")


# ------------------------------------------------------------------------------------------ ops.lookup_accept
def _accept_case(seed, B, T, n_new, V, K, N, m_in, dtype, alphabet=9, eos=None):
    """CPU tensors of one call.  Tokens come from a small alphabet so that n-grams repeat; row b's state cycles through: fresh /
    mid-generation with drafts the logits accept in full, in part, not at all / no drafts / finished."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    ids = torch.full((B, T + n_new), -7, dtype=torch.int64)
    ids[:, :T] = torch.randint(3, 3 + alphabet, (B, T), generator=g)
    mask = torch.ones(B, T, dtype=torch.uint8)
    for b in range(1, B):
        mask[b, ri(2, T):] = 0                                  # ragged right padding; row 0 fills the width
    mask[B - 1, 1] = 0                                          # and a hole
    gen, lens = torch.zeros(B, dtype=torch.int32), torch.full((B,), T, dtype=torch.int32)
    finished, n_draft = torch.zeros(B, dtype=torch.uint8), torch.zeros(B, dtype=torch.int32)
    block = torch.randint(3, 3 + alphabet, (B, K + 1), generator=g)
    logits = torch.stack([torch.randperm(V, generator=g).float() - V // 2 for _ in range(B * m_in)])
    top = float(V)
    for r in range(B * m_in):                                   # every greedy token comes from the alphabet, so the next draft finds matches
        logits[r, ri(3, 2 + alphabet)] = top - 1.0
    if m_in > 1:
        for b in range(B):
            kind = b % 6
            gb = ri(1, n_new - 1) if kind != 5 else n_new
            new = torch.randint(3, 3 + alphabet, (gb,), generator=g)
            ids[b, T:T + gb] = new
            gen[b], lens[b] = gb, T + gb - 1
            block[b, 0] = new[-1]
            nd = 0 if kind == 3 else ri(1, K)
            n_draft[b] = nd
            finished[b] = int(kind == 5)
            want = {0: nd, 1: nd // 2, 2: 0}.get(kind, nd)      # drafts the logits confirm: all, some, none
            for i in range(want):
                logits[b * m_in + i, int(block[b, i + 1])] = top
            if eos is not None and kind == 0 and nd >= 2:
                block[b, 2] = eos                               # EOS inside the accepted run
                logits[b * m_in + 1, eos] = top + 1.0
    return dict(logits=logits.to(dtype), block=block, n_draft=n_draft, ids=ids, prompt_mask=mask, gen=gen, lens=lens, finished=finished)


def _run_accept(case, m_in, n_new, N, eos, pad, pos_offset, pos_max, dense=False):
    """dense: the logits rows start at multiples of 16 bytes (the kernel's vector loads); else every operand with a row stride has
    one of its own, the logits' an odd one (element loads)."""
    from mmgl_amd import ops
    dev = {k: v.cuda() for k, v in case.items()}
    for key, extra, fill in (("logits", 5, NAN), ("ids", 3, -9), ("prompt_mask", 7, 1)):
        t = case[key]
        if dense and key == "logits":
            extra = -t.shape[1] % 8                             # rows 16-byte aligned, V itself need not be a multiple
        buf = torch.full((t.shape[0], t.shape[1] + extra), fill, dtype=t.dtype).cuda()
        dev[key] = buf[:, :t.shape[1]]
        dev[key].copy_(t)
    B, M1 = case["block"].shape
    positions = torch.full((B, M1), -5, dtype=torch.int64, device="cuda")
    emitted = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    ops.lookup_accept(dev["logits"], m_in, dev["block"], dev["n_draft"], positions, dev["ids"], dev["prompt_mask"], dev["gen"], dev["lens"],
                      dev["finished"], emitted, n_new, N, eos, pad, pos_offset, pos_max)
    return dict(block=dev["block"], n_draft=dev["n_draft"], positions=positions, ids=dev["ids"], gen=dev["gen"], lens=dev["lens"],
                finished=dev["finished"], emitted=emitted)


def _check_accept(case, m_in, n_new, N, eos=None, pad=None, pos_offset=2, pos_max=10 ** 6, what=""):
    want = lookup_accept_ref(case["logits"], m_in, case["block"], case["n_draft"], case["ids"], case["prompt_mask"], case["gen"],
                             case["lens"], case["finished"], n_new, N, eos, pad, pos_offset, pos_max)
    got = _run_accept(case, m_in, n_new, N, eos, pad, pos_offset, pos_max)
    again = _run_accept(case, m_in, n_new, N, eos, pad, pos_offset, pos_max)
    dense = _run_accept(case, m_in, n_new, N, eos, pad, pos_offset, pos_max, dense=True)
    for key in KEYS:
        assert torch.equal(got[key].cpu(), want[key]), f"{what}: {key}\n got {got[key].cpu().tolist()}\nwant {want[key].tolist()}"
        assert torch.equal(got[key], again[key]), f"{what}: two runs differ in {key}"
        assert torch.equal(dense[key].cpu(), want[key]), f"{what}, dense logits: {key}\n got {dense[key].cpu().tolist()}\nwant {want[key].tolist()}"
    return want


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", [1, 2, 4])
@pytest.mark.parametrize("K", [1, 3, 7])
def test_lookup_accept_verify_call(K, N, dtype):
    B, T, n_new, V = 12, 21, 12, 128
    eos = 5
    case = _accept_case(100 * K + N, B, T, n_new, V, K, N, K + 1, dtype, eos=eos)
    want = _check_accept(case, K + 1, n_new, N, eos, 1, what=f"K={K} N={N} {dtype}")
    k = want["emitted"]
    assert (k == 0).any() and (k == 1).any() and (k > 1).any()                      # finished rows, rejections and accepted drafts
    assert (want["n_draft"] > 0).any() and (want["n_draft"] == 0).any()              # drafted blocks and empty ones
    assert K < 3 or ((want["ids"][:, T:] == 1).any() and (k < case["n_draft"] + 1).any())   # an EOS was hit: pads behind it


@pytest.mark.parametrize("K,N", [(1, 2), (3, 1), (3, 2), (7, 4)])
def test_lookup_accept_prefill_call(K, N):
    """m_in = 1: one logits row per sample, gen = 0; len stays at T; the first block is drafted from the prompt alone."""
    B, T, n_new, V = 12, 21, 12, 128
    case = _accept_case(7 * K + N, B, T, n_new, V, K, N, 1, F32, alphabet=5)
    want = _check_accept(case, 1, n_new, N, what=f"prefill K={K} N={N}")
    assert want["emitted"].tolist() == [1] * B and want["lens"].tolist() == [T] * B and (want["n_draft"] > 0).any()


def test_lookup_accept_row_limits():
    """n_new = 1 (the prefill's token completes every row), positions at the table's end (the clamp), and an EOS as the first token."""
    case = _accept_case(3, 4, 9, 1, 128, 3, 2, 1, F32)
    want = _check_accept(case, 1, 1, 2, what="n_new = 1")
    assert want["finished"].tolist() == [1] * 4 and want["n_draft"].tolist() == [0] * 4
    case = _accept_case(4, 6, 21, 12, 128, 7, 2, 8, F32)
    want = _check_accept(case, 8, 12, 2, pos_max=21 + 2 + 3, what="clamped positions")
    assert (want["positions"] == 26).any() and (want["positions"] < 26).any()
    case = _accept_case(5, 4, 9, 6, 128, 3, 2, 1, F32)
    eos = int(case["logits"][0].argmax())
    want = _check_accept(case, 1, 6, 2, eos=eos, pad=1, what="EOS first")
    assert want["ids"][0, 9:].tolist() == [eos, 1, 1, 1, 1, 1] and want["gen"][0] == 6


def test_lookup_accept_wide_vocabulary():
    """V = 50272 (no multiple of the 1024 threads), fp32 so that all values stay distinct; the maxima sit at the row's ends and at a
    wave boundary."""
    B, T, n_new, V, K = 3, 21, 12, 50272, 3
    case = _accept_case(11, B, T, n_new, V, K, 2, K + 1, F32)
    for r, v in enumerate([0, V - 1, 1023, 1024, 50271, 49152, 63, 64, V - 2, 4097, 2, 31337]):
        case["logits"][r, v] = 2.0 * V
    want = _check_accept(case, K + 1, n_new, 2, what="V = 50272")
    assert want["ids"][0, T + int(case["gen"][0])] == 0


def test_lookup_accept_ties_and_nan():
    """A tie goes to the lowest index; a NaN is never chosen.  V = 2502 in fp32: 625 whole 16-byte vectors and two columns behind
    them, where row 1 has its maximum."""
    B, T, n_new, V, K = 2, 9, 6, 2502, 1
    case = _accept_case(13, B, T, n_new, V, K, 2, 1, F32)
    case["logits"][0, [2047, 1030, 77, 2501]] = 9999.0
    case["logits"][1, 5] = NAN
    case["logits"][1, 2501] = 9999.0
    want = _check_accept(case, 1, n_new, 2, what="ties")
    assert want["ids"][:, T].tolist() == [77, 2501]


def test_lookup_accept_refusals_leave_the_state_alone():
    from mmgl_amd import ops
    case = {k: v.cuda() for k, v in _accept_case(1, 4, 9, 6, 128, 3, 2, 4, F32).items()}
    pos, em = torch.full((4, 4), -5, dtype=torch.int64, device="cuda"), torch.full((4,), -5, dtype=torch.int32, device="cuda")
    before = {k: v.clone() for k, v in case.items()}
    call = lambda **kw: ops.lookup_accept(**{**dict(logits=case["logits"], m_in=4, block=case["block"], n_draft=case["n_draft"], positions=pos,
                                                    ids=case["ids"], prompt_mask=case["prompt_mask"], gen=case["gen"], lens=case["lens"],
                                                    finished=case["finished"], emitted=em, n_new=6, ngram_size=2), **kw})
    for kw in (dict(m_in=2), dict(ngram_size=5), dict(ngram_size=0), dict(gen=case["gen"].long()), dict(lens=case["lens"][:3]),
               dict(block=case["block"].int()), dict(block=torch.zeros(4, 9, dtype=torch.int64, device="cuda")), dict(positions=pos[:, :3]),
               dict(ids=case["ids"].int()), dict(prompt_mask=case["prompt_mask"].long()), dict(logits=case["logits"].half()),
               dict(logits=case["logits"][:15]), dict(eos_token_id=2), dict(eos_token_id=2, pad_token_id=128), dict(n_new=0),
               dict(finished=case["finished"].cpu())):
        with pytest.raises((ValueError, RuntimeError)):
            call(**kw)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(case[k], v), k
    assert (pos == -5).all() and (em == -5).all()


# ------------------------------------------------------------------------------------------ ops.attn_decode_block
H = 4


def _block_case(dtype, D, m, seed):
    """Windows of NaN buffers.  len covers 0, 1, capacity - m, a value that drops some of the new columns, capacity, and one past a loop trip."""
    vec = 8 if dtype == BF16 else 4
    trip = 1024 * vec // D                                      # keys per workgroup loop trip
    cap, d = trip + 37, H * D
    lens = [0, 1, cap - m, cap - m + (m + 1) // 2, cap, trip + 1, 5]
    B = len(lens)
    g = torch.Generator().manual_seed(seed)
    qbuf = torch.full((B * m + 1, d + 16), NAN, dtype=dtype)
    qbuf[:B * m, 8:8 + d] = (torch.randn(B * m, d, generator=g) * D ** -0.5).to(dtype)
    new = torch.full((B * m + 1, 2 * d), NAN, dtype=dtype)
    new[:B * m] = torch.randn(B * m, 2 * d, generator=g).to(dtype)
    cache = torch.full((B, cap + 3, 2 * d + 16), NAN, dtype=dtype)
    mask = torch.ones(B, cap + 5, dtype=torch.uint8)
    for b, L in enumerate(lens):
        cache[b, :L, 8:8 + 2 * d] = torch.randn(L, 2 * d, generator=g).to(dtype)
        if L > 2:
            mask[b, :L] = torch.rand(L, generator=g) > 0.3      # masked prefix keys
            mask[b, 0] = 1
    mask[6, :5] = 0                                             # a prefix without any valid key: the new keys carry the row
    return qbuf, new, cache, mask, torch.tensor(lens, dtype=torch.int32), cap


def _block_ref(q, new, cache_k, cache_v, mask, lens, m):
    """fp64: row (b, i) over the valid cache columns below len[b] and the new keys j <= i."""
    B, d = cache_k.shape[0], q.shape[1]
    D = d // H
    out = torch.zeros(B * m, d, dtype=torch.float64)
    for b in range(B):
        L = int(lens[b])
        keep = mask[b, :L].bool()
        for i in range(m):
            k = torch.cat([cache_k[b, :L][keep], new[b * m:b * m + i + 1, :d]]).double().view(-1, H, D)
            v = torch.cat([cache_v[b, :L][keep], new[b * m:b * m + i + 1, d:]]).double().view(-1, H, D)
            p = torch.softmax(torch.einsum("hd,shd->hs", q[b * m + i].double().view(H, D), k), -1)
            out[b * m + i] = torch.einsum("hs,shd->hd", p, v).reshape(d)
    return out


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


@pytest.mark.parametrize("m", [1, 2, 3, 8])
@pytest.mark.parametrize("D", [16, 64, 128])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_attn_decode_block(dtype, D, m):
    from mmgl_amd import ops
    qbuf, new, cache, mask, lens, cap = _block_case(dtype, D, m, 1000 * D + m)
    d, B = H * D, len(lens)
    q_c, k_c, v_c = qbuf[:B * m, 8:8 + d], cache[:, :cap, 8:8 + d], cache[:, :cap, 8 + d:8 + 2 * d]
    want = _block_ref(q_c, new[:B * m], k_c, v_c, mask, lens, m).cuda()
    qg, ng, cg, mg, lg = qbuf.cuda(), new.cuda(), cache.cuda(), mask.cuda(), lens.cuda()
    before = cg.clone()
    q, k_new, v_new = qg[:B * m, 8:8 + d], ng[:B * m, :d], ng[:B * m, d:]
    k, v, valid = cg[:, :cap, 8:8 + d], cg[:, :cap, 8 + d:8 + 2 * d], mg[:, :cap]
    assert q.stride(0) > d and k.stride(1) > 2 * d and valid.stride(0) > cap and k_new.stride(0) == 2 * d
    got = ops.attn_decode_block(q, k_new, v_new, k, v, valid, lg, H, m)
    assert got.shape == (B * m, d)
    for b in range(B):
        _attn_check(got[b * m:(b + 1) * m].reshape(1, -1), want[b * m:(b + 1) * m].reshape(1, -1), dtype,
                    f"{dtype} D={D} m={m} len={int(lens[b])} of {cap}", "block")
    # the cache: the new keys / values at columns len .. len + m - 1 below the capacity, bitwise; every other byte as before
    expect = before.clone()
    filed = 0
    for b in range(B):
        for j in range(m):
            c = int(lens[b]) + j
            if c < cap:
                expect[b, c, 8:8 + 2 * d] = ng[b * m + j]
                filed += 1
    assert filed < B * m, "no new column was dropped at the capacity"
    assert torch.equal(_bits(cg), _bits(expect)), "the cache differs from: old bytes + the filed columns"
    # a second run on the cache as it was: bitwise the same output
    cg.copy_(before)
    assert torch.equal(_bits(ops.attn_decode_block(q, k_new, v_new, k, v, valid, lg, H, m)), _bits(got)), "two runs differ"
    if m == 1:
        # ops.attn_decode on the cache the call left behind, against the same fp64 reference at the same TOL.  Bitwise equality of the
        # two kernels is not expected: attn_decode rescales its state per key, the block kernel once per trip of 4, so they round
        # differently; each is held to the reference.
        for b in range(B):
            L = int(lens[b])
            if L < cap:
                one = ops.attn_decode(q[b:b + 1], k[b:b + 1, :L + 1], v[b:b + 1, :L + 1], valid[b:b + 1, :L + 1], H)
                _attn_check(one, want[b:b + 1], dtype, f"attn_decode {dtype} D={D} len={L}", "block m=1")


def test_attn_decode_block_refusals_leave_outputs_alone():
    from mmgl_amd import ops
    B, m, D, cap = 2, 4, 64, 9
    d = H * D
    ones = lambda *shape: torch.ones(*shape, device="cuda", dtype=BF16)
    cache, new, q = ones(B, cap, 2 * d + 16), ones(B * m, 2 * d), ones(B * m, d)
    valid, lens = torch.ones(B, cap, dtype=torch.bool, device="cuda"), torch.full((B,), 3, dtype=torch.int32, device="cuda")
    before = cache.clone()

    def refused(**kw):
        a = {**dict(q=q, k_new=new[:, :d], v_new=new[:, d:], k=cache[:, :, :d], v=cache[:, :, d:2 * d], key_valid=valid, lens=lens, num_heads=H, m=m),
             **kw}
        out = torch.full((B * m, d), 7.0, device="cuda", dtype=BF16)
        with pytest.raises(ValueError):
            ops.attn_decode_block(**a, out=out)
        torch.cuda.synchronize()
        assert torch.equal(out, torch.full_like(out, 7.0)) and torch.equal(cache, before)

    refused(m=9)
    refused(m=0)
    refused(m=2)                                                                       # q rows are not B * m
    refused(lens=lens.long())
    refused(lens=lens[:1])
    refused(k_new=new[:, :d].float(), v_new=new[:, d:].float())
    refused(k_new=new[:B, :d], v_new=new[:B, d:])
    wide = ones(B * m, 2 * d + 16)
    refused(k_new=wide[:, 4:4 + d], v_new=wide[:, 4 + d:4 + 2 * d])                    # 8-byte aligned halves
    refused(k=cache[:, :, 4:4 + d], v=cache[:, :, 4 + d:4 + 2 * d])
    refused(key_valid=valid[:, :5])
    refused(num_heads=3)
    out = torch.full((B * m, d), 7.0, device="cuda", dtype=BF16)
    assert ops.attn_decode_block(q, new[:, :d], new[:, d:], cache[:, :, :d], cache[:, :, d:2 * d], valid, lens, H, m, out=out) is out
    assert torch.equal(out, torch.ones_like(out))                                       # the accepted twin: every value row is ones
    assert torch.equal(cache, before)                                                   # the rows filed are rows of ones, too
