"""ops.decode_lora_linear (mmgl_gemm_skinny_lora) against the composition a checkout without it has to run, alternating in one process.

    python tools/bench_gemm_skinny_lora.py [--rows 2,16,64] [--ranks 16,64] [--iters 200] [--rounds 5] [--out FILE]

Both arms compute the bf16 y[M, N] = x W^T + bias + s (x A^T) B^T of a LoRA-adapted q_proj / v_proj in a decode step:
    fused     ops.decode_lora_linear(x, W, bias, A, B, s): two launches (t = x A^T in fp32, then the skinny GEMM with the rank-r term)
    composed  ops.decode_linear(x, W, bias) + s * ops.decode_linear(ops.decode_linear(x, A), B): three skinny GEMMs and an add
As in tools/bench_gemm_skinny.py no weight is in a cache when its GEMM starts: each timed loop walks a ring of (W, A, B) copies larger
than the 256 MB Infinity Cache.  Rounds alternate fused / composed / fused / ...; the table gives the median microseconds per call of
each, the spread over the rounds and the ratio composed / fused (above 1: the fused entry point is faster)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(2048, 2048), (768, 768)]
RING_BYTES = 640 << 20
SCALING = 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="2,16,64")
    ap.add_argument("--ranks", default="16,64")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gemm_skinny_lora needs the GPU")
    from mmgl_amd import ops
    lines = [f"# {torch.cuda.get_device_name(0)}; bf16; {a.iters} calls per loop over a ring of (W, A, B) copies >= {RING_BYTES >> 20} MiB; "
             f"median of {a.rounds} alternating rounds (min..max)",
             f"{'M':>3} {'N':>5} {'K':>5} {'r':>3} | {'fused us':>22} | {'composed us':>22} | composed / fused"]
    rn = lambda *s: torch.randn(*s, device="cuda")
    for N, K in SHAPES:
        for r in [int(v) for v in a.ranks.split(",")]:
            copies = max(2, -(-RING_BYTES // ((N * K + r * K + N * r) * 2)))
            ws = [((rn(N, K) * K ** -0.5).bfloat16(), (rn(r, K) * K ** -0.5).bfloat16(), (rn(N, r) * r ** -0.5).bfloat16()) for _ in range(copies)]
            bias = rn(N).bfloat16()
            for M in [int(m) for m in a.rows.split(",")]:
                x = rn(M, K).bfloat16()
                y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)

                def fused(w):
                    return ops.decode_lora_linear(x, w[0], bias, w[1], w[2], SCALING, out=y)

                def composed(w):
                    ops.decode_linear(x, w[0], bias, out=y)
                    return y.add_(ops.decode_linear(ops.decode_linear(x, w[1]), w[2]), alpha=SCALING)
                arms = {"fused": fused, "composed": composed}
                W, A, Bm = (t.float() for t in ws[0])
                ref = x.float() @ W.t() + bias.float() + SCALING * ((x.float() @ A.t()) @ Bm.t())
                with torch.no_grad():
                    for name, fn in arms.items():
                        err = (fn(ws[0]).float() - ref).abs().max().item()
                        assert err <= 2e-2 * ref.abs().max().item() + 1e-2, (name, M, N, K, r, err)
                    times = {"fused": [], "composed": []}
                    for rd in range(a.rounds + 1):
                        for name, fn in arms.items():
                            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            s.record()
                            for i in range(a.iters):
                                fn(ws[i % copies])
                            e.record()
                            torch.cuda.synchronize()
                            if rd:                                  # round 0 warms both arms up
                                times[name].append(s.elapsed_time(e) * 1e3 / a.iters)
                fu, co = statistics.median(times["fused"]), statistics.median(times["composed"])
                fmt = lambda t: f"{statistics.median(t):7.2f} ({min(t):6.2f}..{max(t):6.2f})"
                lines.append(f"{M:>3} {N:>5} {K:>5} {r:>3} | {fmt(times['fused'])} | {fmt(times['composed'])} | {co / fu:6.2f}")
                print(lines[-1], flush=True)
            del ws
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
