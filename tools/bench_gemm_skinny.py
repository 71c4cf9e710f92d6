"""mmgl_gemm_skinny against mmgl_gemm_nt on the linears of a decode step, alternating in one process.

    python tools/bench_gemm_skinny.py [--rows 2,16,64] [--iters 200] [--rounds 5] [--out FILE]

For every (N, K) of the step and every M, both entry points compute the same dense bf16 y[M, N] = x[M, K] . W[N, K]^T + bias.  A decode
step streams 2.9 GB of weights, so no weight is in a cache when its GEMM starts: each timed loop walks a ring of weight copies larger
than the 256 MB Infinity Cache.  Rounds alternate skinny / nt / skinny / ...; the table gives the median microseconds per call of each,
the spread over the rounds, the weight bytes over the skinny time, and which entry point ops.decode_linear should take for the shape
(the skinny kernel only where it is not slower)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(2048, 2048), (4096, 2048), (8192, 2048), (2048, 8192), (50272, 2048), (768, 768), (3072, 768)]
RING_BYTES = 640 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="2,16,64")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gemm_skinny needs the GPU")
    from mmgl_amd import ops
    lines = [f"# {torch.cuda.get_device_name(0)}; bf16; {a.iters} calls per loop over a ring of weight copies >= {RING_BYTES >> 20} MiB; "
             f"median of {a.rounds} alternating rounds (min..max)",
             f"{'M':>3} {'N':>6} {'K':>5} | {'skinny us':>22} | {'gemm_nt us':>22} | {'skinny TB/s':>11} | route"]
    for N, K in SHAPES:
        copies = max(2, -(-RING_BYTES // (N * K * 2)))
        ws = [(torch.randn(N, K, device="cuda") * K ** -0.5).bfloat16() for _ in range(copies)]
        bias = torch.randn(N, device="cuda").bfloat16()
        for M in [int(m) for m in a.rows.split(",")]:
            x = torch.randn(M, K, device="cuda").bfloat16()
            y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
            arms = {"skinny": lambda w: ops.gemm_skinny(x, w, bias, out=y), "nt": lambda w: ops.gemm_nt(x, w, bias, out=y)}
            ref = (x.float() @ ws[0].float().t() + bias.float())
            for name, fn in arms.items():
                err = (fn(ws[0]).float() - ref).abs().max().item()
                assert err <= 2e-2 * ref.abs().max().item() + 1e-2, (name, M, N, K, err)
            times = {"skinny": [], "nt": []}
            for r in range(a.rounds + 1):
                for name, fn in arms.items():
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for i in range(a.iters):
                        fn(ws[i % copies])
                    e.record()
                    torch.cuda.synchronize()
                    if r:                                   # round 0 warms both arms up
                        times[name].append(s.elapsed_time(e) * 1e3 / a.iters)
            sk, nt = statistics.median(times["skinny"]), statistics.median(times["nt"])
            fmt = lambda t: f"{statistics.median(t):7.2f} ({min(t):6.2f}..{max(t):6.2f})"
            lines.append(f"{M:>3} {N:>6} {K:>5} | {fmt(times['skinny'])} | {fmt(times['nt'])} | {N * K * 2 / (sk * 1e-6) / 1e12:11.2f} | "
                         f"{'skinny' if sk <= nt else 'gemm_nt'}")
            print(lines[-1], flush=True)
        del ws
    # single-query attention at the call sites of a decode step (self: S cached keys; cross: 64 neighbor tokens), cold caches
    H, D = 32, 64
    lines.append("# mmgl_attn_decode_fwd, H = 32, D = 64, K|V in [B, S, 2 H D] cache rows, a ring of caches >= 640 MiB")
    lines.append(f"{'B':>3} {'S':>5} | {'us':>22} | {'TB/s':>6} | workgroups")
    for B, S in [(2, 544), (16, 544), (64, 544), (2, 64), (64, 64)]:
        d = H * D
        copies = max(2, -(-RING_BYTES // (B * S * 2 * d * 2)))
        copies = min(copies, 256)
        kvs = [torch.randn(B, S, 2 * d, device="cuda").bfloat16() for _ in range(copies)]
        q = (torch.randn(B, d, device="cuda") * D ** -0.5).bfloat16()
        valid = torch.ones(B, S, dtype=torch.uint8, device="cuda")
        t = []
        for r in range(a.rounds + 1):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(a.iters):
                kv = kvs[i % copies]
                ops.attn_decode(q, kv[:, :, :d], kv[:, :, d:], valid, H)
            e.record()
            torch.cuda.synchronize()
            if r:
                t.append(s.elapsed_time(e) * 1e3 / a.iters)
        med = statistics.median(t)
        lines.append(f"{B:>3} {S:>5} | {med:7.2f} ({min(t):6.2f}..{max(t):6.2f}) | {B * S * 2 * d * 2 / (med * 1e-6) / 1e12:6.2f} | {B * H}")
        print(lines[-1], flush=True)
        del kvs
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
