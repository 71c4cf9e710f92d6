"""mmgl_attn_decode_q8_fwd on an FP8 cache against mmgl_attn_decode_fwd on a bf16 cache of the same shape, alternating in one process,
and mmgl_kv_quantize against the copy it replaces at the prefill.

    python tools/bench_attn_decode_q8.py [--batches 2,16,64] [--keys 512,2048] [--iters 200] [--rounds 5] [--out FILE]

Both attention arms answer one decode step's call for q [B, H*D] bf16, H = 32, D = 64, over S cached columns plus the new token: the
bf16 arm reads cache rows [B, S + 1, 2 H D] bf16 whose last column holds the new token (as MPTAttention.decode_self leaves it in the
plain mode of DecodeCache), the FP8 arm reads S columns of e4m3fn codes [B, S + 1, 2 H D] with their int8 exponents [B, S + 1, 2 H],
takes the new token dense and files it at column S.  A decode step streams gigabytes of weights between two attention calls, so no cache row is in a cache when its
call starts: each timed loop walks a ring of caches larger than the 256 MB Infinity Cache, as tools/bench_attn_decode_gqa.py does.
Rounds alternate fp8 / bf16 / fp8 / ...; the table gives the median microseconds per call of each arm (min..max over the rounds), the
bytes each arm reads over its time, and the ratio.  The prefill table times one ops.kv_quantize launch against the one strided copy of
the k|v columns of a fused qkv output [B, S, 3 H D] that the plain prefill makes, same ring rule.  No threshold is fixed in advance:
the yardstick is the bf16 arm in the same process."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, D = 32, 64
RING_BYTES = 640 << 20


def alternate(arms, iters, rounds):
    times = {name: [] for name in arms}
    for r in range(rounds + 1):
        for name, fn in arms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(iters):
                fn(i)
            e.record()
            torch.cuda.synchronize()
            if r:                                               # round 0 warms both arms up
                times[name].append(s.elapsed_time(e) * 1e3 / iters)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,16,64")
    ap.add_argument("--keys", default="512,2048")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_decode_q8 needs the GPU")
    from mmgl_amd import ops
    d = H * D
    fmt = lambda t: f"{statistics.median(t):8.2f} ({min(t):7.2f}..{max(t):7.2f})"
    lines = [f"# {torch.cuda.get_device_name(0)}; H = {H}, D = {D}; {a.iters} calls per loop over a ring of caches >= {RING_BYTES >> 20} MiB; "
             f"median of {a.rounds} alternating rounds (min..max)",
             f"{'B':>3} {'S':>5} | {'fp8 cache us':>24} | {'bf16 cache us':>24} | {'fp8 TB/s':>8} | {'bf16 TB/s':>9} | bf16 / fp8 time"]
    pre = [f"{'B':>3} {'S':>5} | {'kv_quantize us':>24} | {'copy us':>24} | copy / kv_quantize time"]
    for S in [int(s) for s in a.keys.split(",")]:
        for B in [int(b) for b in a.batches.split(",")]:
            q8_bytes, bf_bytes = B * S * (2 * d + 2 * H), B * (S + 1) * 2 * d * 2
            copies = max(2, -(-RING_BYTES // q8_bytes))
            bf_copies = max(2, -(-RING_BYTES // bf_bytes))
            plain = [(torch.randn(B, S + 1, 2 * d, device="cuda")).bfloat16() for _ in range(bf_copies)]
            codes = [torch.empty(B, S + 1, 2 * d, dtype=ops.KV_FP8, device="cuda") for _ in range(copies)]
            scales = [torch.empty(B, S + 1, 2 * H, dtype=torch.int8, device="cuda") for _ in range(copies)]
            for i in range(copies):
                src = plain[i % bf_copies]
                ops.kv_quantize(src[:, :S, :d], src[:, :S, d:], codes[i], scales[i], H)
            q = (torch.randn(B, d, device="cuda") * D ** -0.5).bfloat16()
            new = torch.randn(B, 2 * d, device="cuda").bfloat16()
            valid = torch.ones(B, S + 1, dtype=torch.uint8, device="cuda")
            valid[:, S - S // 8:S] = torch.rand(B, S // 8, device="cuda") > 0.5
            out = torch.empty(B, d, device="cuda", dtype=torch.bfloat16)
            arms = {"fp8": lambda i: ops.attn_decode_q8(q, new[:, :d], new[:, d:], codes[i % copies], scales[i % copies], valid[:, :S], H, out=out),
                    "bf16": lambda i: ops.attn_decode(q, plain[i % bf_copies][:, :, :d], plain[i % bf_copies][:, :, d:], valid, H, out=out)}
            times = alternate(arms, a.iters, a.rounds)
            t8, tb = statistics.median(times["fp8"]), statistics.median(times["bf16"])
            lines.append(f"{B:>3} {S:>5} | {fmt(times['fp8'])} | {fmt(times['bf16'])} | {q8_bytes / (t8 * 1e-6) / 1e12:8.2f} | "
                         f"{bf_bytes / (tb * 1e-6) / 1e12:9.2f} | {tb / t8:5.2f}")
            print(lines[-1], flush=True)
            del plain
            # the prefill's filing: the fused qkv output of one layer into the cache
            qkv_copies = max(2, -(-RING_BYTES // (B * S * 3 * d * 2)))
            qkv = [torch.randn(B, S, 3 * d, device="cuda").bfloat16() for _ in range(qkv_copies)]
            dst = [torch.empty(B, S + 1, 2 * d, dtype=torch.bfloat16, device="cuda") for _ in range(qkv_copies)]
            arms = {"quant": lambda i: ops.kv_quantize(qkv[i % qkv_copies][..., d:2 * d], qkv[i % qkv_copies][..., 2 * d:], codes[i % copies],
                                                       scales[i % copies], H),
                    "copy": lambda i: dst[i % qkv_copies][:, :S].copy_(qkv[i % qkv_copies][..., d:])}
            times = alternate(arms, max(a.iters // 4, 1), a.rounds)
            pre.append(f"{B:>3} {S:>5} | {fmt(times['quant'])} | {fmt(times['copy'])} | "
                       f"{statistics.median(times['copy']) / statistics.median(times['quant']):5.2f}")
            print(pre[-1], flush=True)
            del qkv, dst, codes, scales
    lines += ["", "# the prefill: one mmgl_kv_quantize launch per layer against the copy of the k|v columns it replaces"] + pre
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    else:
        print("\n".join(lines[:2]))


if __name__ == "__main__":
    main()
