"""mmgl_attn_decode_gqa_q8_fwd on an FP8 cache of Hkv key/value heads against mmgl_attn_decode_gqa_fwd (mmgl_attn_decode_fwd at
Hkv = H) on a bf16 cache of the same shape, alternating in one process.

    python tools/bench_attn_decode_gqa_q8.py [--kv-heads 32,8] [--batches 2,16,64] [--keys 512,2048] [--iters 200] [--rounds 5] [--out FILE]

Both arms answer one decode step's call of the Llama-family LM at config-5 head dimensions, q [B, H*D] bf16 with H = 32, D = 128, over
S cached columns plus the new token: the bf16 arm reads cache rows [B, S + 1, 2 Hkv D] bf16 whose last column holds the new token (as
_FrozenLlamaLayer.decode_step leaves it), the FP8 arm reads S columns of e4m3fn codes [B, S + 1, 2 Hkv D] with their int8 exponents
[B, S + 1, 2 Hkv], takes the new token dense and files it at column S.  Hkv = 32 is config 5 itself (the multi-head pair of entry
points runs: ops.attn_decode and ops.attn_decode_q8 route Hkv = H there); Hkv = 8 is the grouped-query shape of the Llama-3 family,
G = 4 query heads per workgroup.  A decode step streams gigabytes of weights between two attention calls, so no cache row is in a cache
when its call starts: each timed loop walks a ring of caches larger than the 256 MB Infinity Cache, as tools/bench_attn_decode_q8.py
does.  Rounds alternate fp8 / bf16 / fp8 / ...; the table gives the median microseconds per call of each arm (min..max over the
rounds), the bytes each arm reads over its time, and the ratio.  No threshold is fixed in advance: the yardstick is the bf16 arm in the
same process."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_attn_decode_q8 import RING_BYTES, alternate        # noqa: E402

H, D = 32, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kv-heads", default="32,8")
    ap.add_argument("--batches", default="2,16,64")
    ap.add_argument("--keys", default="512,2048")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_decode_gqa_q8 needs the GPU")
    from mmgl_amd import ops
    d = H * D
    fmt = lambda t: f"{statistics.median(t):8.2f} ({min(t):7.2f}..{max(t):7.2f})"
    lines = [f"# {torch.cuda.get_device_name(0)}; H = {H}, D = {D}; {a.iters} calls per loop over a ring of caches >= {RING_BYTES >> 20} MiB; "
             f"median of {a.rounds} alternating rounds (min..max)",
             f"{'Hkv':>3} {'B':>3} {'S':>5} | {'fp8 cache us':>24} | {'bf16 cache us':>24} | {'fp8 TB/s':>8} | {'bf16 TB/s':>9} | bf16 / fp8 time"]
    for Hkv in [int(h) for h in a.kv_heads.split(",")]:
        kd = Hkv * D
        for S in [int(s) for s in a.keys.split(",")]:
            for B in [int(b) for b in a.batches.split(",")]:
                q8_bytes, bf_bytes = B * S * (2 * kd + 2 * Hkv), B * (S + 1) * 2 * kd * 2
                copies = max(2, -(-RING_BYTES // q8_bytes))
                bf_copies = max(2, -(-RING_BYTES // bf_bytes))
                plain = [(torch.randn(B, S + 1, 2 * kd, device="cuda")).bfloat16() for _ in range(bf_copies)]
                codes = [torch.empty(B, S + 1, 2 * kd, dtype=ops.KV_FP8, device="cuda") for _ in range(copies)]
                scales = [torch.empty(B, S + 1, 2 * Hkv, dtype=torch.int8, device="cuda") for _ in range(copies)]
                for i in range(copies):
                    src = plain[i % bf_copies]
                    ops.kv_quantize(src[:, :S, :kd], src[:, :S, kd:], codes[i], scales[i], Hkv)
                q = (torch.randn(B, d, device="cuda") * D ** -0.5).bfloat16()
                new = torch.randn(B, 2 * kd, device="cuda").bfloat16()
                valid = torch.ones(B, S + 1, dtype=torch.uint8, device="cuda")
                valid[:, S - S // 8:S] = torch.rand(B, S // 8, device="cuda") > 0.5
                out = torch.empty(B, d, device="cuda", dtype=torch.bfloat16)
                arms = {"fp8": lambda i: ops.attn_decode_q8(q, new[:, :kd], new[:, kd:], codes[i % copies], scales[i % copies], valid[:, :S], H,
                                                            out=out, num_kv_heads=Hkv),
                        "bf16": lambda i: ops.attn_decode(q, plain[i % bf_copies][:, :, :kd], plain[i % bf_copies][:, :, kd:], valid, H, out=out,
                                                          num_kv_heads=Hkv)}
                times = alternate(arms, a.iters, a.rounds)
                t8, tb = statistics.median(times["fp8"]), statistics.median(times["bf16"])
                lines.append(f"{Hkv:>3} {B:>3} {S:>5} | {fmt(times['fp8'])} | {fmt(times['bf16'])} | {q8_bytes / (t8 * 1e-6) / 1e12:8.2f} | "
                             f"{bf_bytes / (tb * 1e-6) / 1e12:9.2f} | {tb / t8:5.2f}")
                print(lines[-1], flush=True)
                del plain, codes, scales
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    else:
        print("\n".join(lines[:2]))


if __name__ == "__main__":
    main()
