"""fp64 reference of mmgl_attn_decode_relbias_fwd (ops.attn_decode_relbias) from the storage-rounded operands, the deliberately wrong
variants the tests must be able to tell from it, and the operands of the kernel test's cases (CPU tensors: tests/test_generate_t5_cpu.py
checks the main case without a GPU, tests/test_decode_relbias_gpu.py runs it).

decode_ref.attn_decode_ref plus the bias, with no mask: the score of key s of (sample b, head h) is q[b, h] . k[b, s, h] + bias[h, S - 1 - s]
-- the query is the newest key s = S - 1, at distance 0 -- with no D^-0.5 anywhere."""
import torch

BF16, F32 = torch.bfloat16, torch.float32
TOL = {F32: 1e-3, BF16: 2e-2}            # tests/test_decode_edges_gpu.py: per sample, of the largest reference magnitude
NUM_BUCKETS, MAX_DISTANCE = 32, 128      # T5's defaults
WRONG = ("distance taken as s", "no bias", "bias row of head h ^ 1")


def trip(dtype, D):
    """I: keys per workgroup loop trip; KPI: keys per wave and load instruction."""
    vec = 8 if dtype == BF16 else 4
    return 1024 * vec // D, 64 * vec // D


def attn_decode_relbias_ref(q, k, v, bias, num_heads, wrong=None):
    """q [B, d] (raw), k, v [B, S, d], bias fp32 [H, >= S] -> [B, d] in fp64.  wrong: one of WRONG, for the can-fail assertions."""
    B, S, d = k.shape
    H, D = num_heads, d // num_heads
    sc = torch.einsum("bhd,bshd->bhs", q.double().reshape(B, H, D), k.double().reshape(B, S, H, D))
    rows = bias.double()[:, :S]
    if wrong is None:
        sc = sc + rows.flip(1)[None]                          # key s sits S - 1 - s behind the query
    elif wrong == WRONG[0]:
        sc = sc + rows[None]
    elif wrong == WRONG[2]:
        other = [h ^ 1 if (h ^ 1) < H else h for h in range(H)]
        sc = sc + rows[other].flip(1)[None]
    elif wrong != WRONG[1]:
        raise ValueError(wrong)
    return torch.einsum("bhs,bshd->bhd", torch.softmax(sc, -1), v.double().reshape(B, S, H, D)).reshape(B, d)


def per_sample(a, want):
    """max|a[b] - want[b]| / max|want[b]| for every sample b: the tolerances' measure."""
    return ((a.double() - want).abs().amax(1) / want.abs().amax(1)).cpu()


def random_case(dtype, H, S, D=64, B=4, seed=0):
    """CPU operands of one random case: q [B, d] with scores q . k ~ N(0, 1), k and v as column slabs of wider cache rows
    [B, S + 3, 2d + 16], a table [NUM_BUCKETS, H] drawn N(0, 2) (standard deviation 2) and its bias rows with ld_bias = S + 5 > S.
    Returns (q, cache, bias, table); the slabs are cache[:, :S, 8:8 + d] and cache[:, :S, 8 + d:8 + 2d]."""
    from mmgl_amd import ops
    d = H * D
    g = torch.Generator().manual_seed(seed * 100003 + S * 131 + H * 17 + D)
    q = (torch.randn(B, d, generator=g) * D ** -0.5).to(dtype)
    cache = torch.randn(B, S + 3, 2 * d + 16, generator=g).to(dtype)
    table = torch.randn(NUM_BUCKETS, H, generator=g) * 2.0
    bias = ops.t5_decode_bias(table, S + 5, NUM_BUCKETS, MAX_DISTANCE)
    return q, cache, bias, table


def slabs(cache, S, d):
    return cache[:, :S, 8:8 + d], cache[:, :S, 8 + d:8 + 2 * d]


def main_case(dtype=BF16, H=2, D=64):
    """The kernel test's main case: two workgroup trips and a tail, S = 2I + KPI + 3."""
    I, KPI = trip(dtype, D)
    S = 2 * I + KPI + 3
    return (S,) + random_case(dtype, H, S, D)
