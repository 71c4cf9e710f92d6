"""mmgl_gemm_skinny_w8 (FP8 frozen weights) against mmgl_gemm_skinny on the linears of a decode step, alternating in one process.

    python tools/bench_gemm_skinny_w8.py [--rows 2,16,64] [--iters 200] [--rounds 5] [--out FILE]

For every (N, K) of the step and every M, the two entry points compute y[M, N] = x[M, K] . W^T + bias in bf16: mmgl_gemm_skinny on the
bf16 weight, mmgl_gemm_skinny_w8 on its e4m3fn codes and row exponents (ops.quantize_weight_fp8).  A decode step streams gigabytes of
weights, so no weight is in a cache when its GEMM starts: each timed loop walks a ring of weight copies whose CODES alone are larger
than the 256 MiB last-level cache (the bf16 ring is then twice that); a single resident weight would measure the cache, not the step.
Rounds alternate bf16 / w8 / bf16 / ...; the table gives the median microseconds per call of each with the spread over the rounds,
the bytes of weight each streams per second, and the ratio.  Shapes: config 3 (OPT-1.3B: q|k|v 6144x2048, out_proj 2048x2048, fc1
8192x2048, fc2 2048x8192) and config 5 (Llama-2-7B dimensions: q|k|v 12288x4096 and the Hkv = 8 width 6144x4096, o_proj 4096x4096,
gate|up 22016x4096, down_proj 4096x11008)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("config 3", 6144, 2048), ("config 3", 2048, 2048), ("config 3", 8192, 2048), ("config 3", 2048, 8192),
          ("config 5", 12288, 4096), ("config 5", 6144, 4096), ("config 5", 4096, 4096), ("config 5", 22016, 4096), ("config 5", 4096, 11008)]
RING_BYTES = 320 << 20                  # of codes: above the 256 MiB last-level cache; the bf16 ring is twice this


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="2,16,64")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gemm_skinny_w8 needs the GPU")
    from mmgl_amd import ops
    lines = [f"# {torch.cuda.get_device_name(0)}; x, bias, y bf16; {a.iters} calls per loop over a ring of weight copies (codes >= "
             f"{RING_BYTES >> 20} MiB, bf16 twice that); median of {a.rounds} alternating rounds (min..max)",
             f"# command: python tools/bench_gemm_skinny_w8.py --rows {a.rows} --iters {a.iters} --rounds {a.rounds}",
             f"{'':>8} {'M':>3} {'N':>6} {'K':>5} | {'bf16 us':>22} | {'w8 us':>22} | {'bf16 TB/s':>9} | {'w8 TB/s':>7} | bf16 / w8"]
    for cfg, N, K in SHAPES:
        copies = max(2, -(-RING_BYTES // (N * K)))
        ws = [(torch.randn(N, K, device="cuda") * K ** -0.5).bfloat16() for _ in range(copies)]
        qs = [ops.quantize_weight_fp8(w) for w in ws]
        bias = torch.randn(N, device="cuda").bfloat16()
        for M in [int(m) for m in a.rows.split(",")]:
            x = torch.randn(M, K, device="cuda").bfloat16()
            y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
            arms = {"bf16": lambda i: ops.gemm_skinny(x, ws[i], bias, out=y), "w8": lambda i: ops.gemm_skinny_w8(x, *qs[i], bias, out=y)}
            deq = qs[0][0].float() * torch.exp2(qs[0][1].float())[:, None]
            for name, w in (("bf16", ws[0].float()), ("w8", deq)):
                ref = x.float() @ w.t() + bias.float()
                err = (arms[name](0).float() - ref).abs().max().item()
                assert err <= 2e-2 * ref.abs().max().item() + 1e-2, (name, M, N, K, err)
            times = {"bf16": [], "w8": []}
            for r in range(a.rounds + 1):
                for name, fn in arms.items():
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for i in range(a.iters):
                        fn(i % copies)
                    e.record()
                    torch.cuda.synchronize()
                    if r:                                   # round 0 warms both arms up
                        times[name].append(s.elapsed_time(e) * 1e3 / a.iters)
            b, q = statistics.median(times["bf16"]), statistics.median(times["w8"])
            fmt = lambda t: f"{statistics.median(t):7.2f} ({min(t):6.2f}..{max(t):6.2f})"
            lines.append(f"{cfg:>8} {M:>3} {N:>6} {K:>5} | {fmt(times['bf16'])} | {fmt(times['w8'])} | {N * K * 2 / (b * 1e-6) / 1e12:9.2f} | "
                         f"{N * (K + 1) / (q * 1e-6) / 1e12:7.2f} | {b / q:5.2f}x")
            print(lines[-1], flush=True)
        del ws, qs
    # the quantiser itself, run once per weight
    lines.append("# mmgl_weight_quantize (run once per weight), bf16 source, median of the rounds")
    for N, K in [(8192, 2048), (22016, 4096)]:
        w = (torch.randn(N, K, device="cuda") * K ** -0.5).bfloat16()
        out = ops.quantize_weight_fp8(w)
        t = []
        for r in range(a.rounds + 1):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(20):
                ops.quantize_weight_fp8(w, out=out)
            e.record()
            torch.cuda.synchronize()
            if r:
                t.append(s.elapsed_time(e) * 1e3 / 20)
        lines.append(f"{N:>6} {K:>5} | {statistics.median(t):8.1f} us ({min(t):.1f}..{max(t):.1f})")
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
