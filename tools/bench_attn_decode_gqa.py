"""mmgl_attn_decode_gqa_fwd against mmgl_attn_decode_fwd on K / V expanded to H heads, alternating in one process.

    python tools/bench_attn_decode_gqa.py [--batches 2,16,64] [--keys 512,2176] [--iters 200] [--rounds 5] [--out FILE]

Both arms compute the same bf16 out[B, H*D]: the grouped-query kernel reads cache rows [B, S, 2*Hkv*D]; the multi-head kernel -- the
only other route there is -- needs the same keys and values repeated over the G = H / Hkv query heads of each group, rows
[B, S, 2*H*D] (the expansion itself is not timed: a cache kept in that layout would simply hold it).  Shapes: H = 32, Hkv = 8,
D = 128 and D = 64.  A decode step streams gigabytes of weights between two attention calls, so no cache row is in a cache when its call
starts: each timed loop walks a ring of caches larger than the 256 MB Infinity Cache.  Rounds alternate gqa /
expanded / gqa / ...; the table gives the median microseconds per call of each arm (min..max over the rounds), the bytes each arm reads
over its time, and the ratio.  There is no adoption threshold: the grouped-query route is the only one that keeps the small cache; the
record says what it costs or gains."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, HKV = 32, 8
RING_BYTES = 640 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,16,64")
    ap.add_argument("--keys", default="512,2176")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_decode_gqa needs the GPU")
    from mmgl_amd import ops
    G = H // HKV
    lines = [f"# {torch.cuda.get_device_name(0)}; bf16; H = {H}, Hkv = {HKV}; {a.iters} calls per loop over a ring of caches >= {RING_BYTES >> 20} MiB; "
             f"median of {a.rounds} alternating rounds (min..max)",
             f"{'D':>3} {'B':>3} {'S':>5} | {'gqa us':>24} | {'expanded multi-head us':>24} | {'gqa TB/s':>8} | {'mha TB/s':>8} | mha / gqa time"]
    for D in (128, 64):
        kd, d = HKV * D, H * D
        for S in [int(s) for s in a.keys.split(",")]:
            for B in [int(b) for b in a.batches.split(",")]:
                small_bytes, big_bytes = B * S * 2 * kd * 2, B * S * 2 * d * 2
                copies = max(2, -(-RING_BYTES // small_bytes))
                small = [torch.randn(B, S, 2 * kd, device="cuda").bfloat16() for _ in range(copies)]
                big_copies = min(copies, max(2, -(-RING_BYTES // big_bytes)))
                expand = lambda t: t.reshape(B, S, 2 * HKV, D).repeat_interleave(G, dim=2).reshape(B, S, 2 * d)
                big = [expand(small[i]) for i in range(big_copies)]
                q = (torch.randn(B, d, device="cuda") * D ** -0.5).bfloat16()
                valid = torch.ones(B, S, dtype=torch.uint8, device="cuda")
                valid[:, S - S // 8:] = torch.rand(B, S // 8, device="cuda") > 0.5
                out = torch.empty(B, d, device="cuda", dtype=torch.bfloat16)
                arms = {"gqa": lambda i: ops.attn_decode(q, small[i % copies][:, :, :kd], small[i % copies][:, :, kd:], valid, H, out=out, num_kv_heads=HKV),
                        "mha": lambda i: ops.attn_decode(q, big[i % big_copies][:, :, :d], big[i % big_copies][:, :, d:], valid, H, out=out)}
                a0, a1 = arms["gqa"](0).clone(), arms["mha"](0).clone()
                assert (a0.float() - a1.float()).abs().max().item() <= 2e-2 * a1.float().abs().max().item(), (D, B, S)
                times = {"gqa": [], "mha": []}
                for r in range(a.rounds + 1):
                    for name, fn in arms.items():
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        for i in range(a.iters):
                            fn(i)
                        e.record()
                        torch.cuda.synchronize()
                        if r:                                   # round 0 warms both arms up
                            times[name].append(s.elapsed_time(e) * 1e3 / a.iters)
                tg, tm = statistics.median(times["gqa"]), statistics.median(times["mha"])
                fmt = lambda t: f"{statistics.median(t):8.2f} ({min(t):7.2f}..{max(t):7.2f})"
                lines.append(f"{D:>3} {B:>3} {S:>5} | {fmt(times['gqa'])} | {fmt(times['mha'])} | {small_bytes / (tg * 1e-6) / 1e12:8.2f} | "
                             f"{big_bytes / (tm * 1e-6) / 1e12:8.2f} | {tm / tg:5.2f}")
                print(lines[-1], flush=True)
                del small, big
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    else:
        print("\n".join(lines[:2]))


if __name__ == "__main__":
    main()
