"""mmgl_attn_decode_relbias_fwd against the aten chain a T5 decoder's cached self-attention takes without it, alternating in one process.

    python tools/bench_attn_decode_relbias.py [--batches 2,16,64] [--keys 1,32,128,512] [--iters 200] [--rounds 5] [--out FILE]

Both arms compute out[B, H*D] = softmax_s(q . k_s + bias[h, S - 1 - s]) v for one new token per sample, bf16, over the same cache rows
[B, S, 2 H D] and the same fp32 bias rows [H, S]:
  hip    ops.attn_decode_relbias: one launch, the cache slabs addressed in place
  aten   gather of the bias by distance (flip), matmul(q, k^T) on head-major views, add, softmax in fp32, matmul with v: what
         transformers' T5Attention does with a cache, on views of the same buffers (its own cache is head-major; the permute is a view here)
Shapes: T5-small / T5-base decode (H = 8 / 12, D = 64).  Every timed loop walks a ring of caches (a step streams the layer's weights
between two attention calls, so cache rows are not in a cache when their call starts); at these sizes the ring is capped at 64 copies, so
the smallest shapes do stay in the Infinity Cache -- for both arms alike.  Rounds alternate hip / aten / hip / ...; the table gives the
median microseconds per call of each arm (min..max over the rounds) and the ratio.  No adoption threshold: the record says what the kernel
costs or gains."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D = 64
RING_BYTES = 640 << 20
MAX_COPIES = 64


def aten_chain(q, k, v, bias, H):
    B, S, d = k.shape
    qh = q.view(B, H, 1, D)
    kh, vh = k.view(B, S, H, D).permute(0, 2, 1, 3), v.view(B, S, H, D).permute(0, 2, 1, 3)
    sc = torch.matmul(qh, kh.transpose(2, 3)).float() + bias[:, :S].flip(1)[None, :, None, :]
    return torch.matmul(torch.softmax(sc, dim=-1).to(q.dtype), vh).permute(0, 2, 1, 3).reshape(B, d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,16,64")
    ap.add_argument("--keys", default="1,32,128,512")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_decode_relbias needs the GPU")
    from mmgl_amd import ops
    lines = [f"# {torch.cuda.get_device_name(0)}; bf16; D = {D}; {a.iters} calls per loop over a ring of up to {MAX_COPIES} caches (>= "
             f"{RING_BYTES >> 20} MiB where that many reach it); median of {a.rounds} alternating rounds (min..max)",
             f"{'H':>3} {'B':>3} {'S':>5} | {'hip us':>24} | {'aten chain us':>24} | aten / hip time"]
    for H in (8, 12):
        d = H * D
        for S in [int(s) for s in a.keys.split(",")]:
            for B in [int(b) for b in a.batches.split(",")]:
                copies = min(MAX_COPIES, max(2, -(-RING_BYTES // (B * S * 2 * d * 2))))
                ring = [torch.randn(B, S, 2 * d, device="cuda").bfloat16() for _ in range(copies)]
                q = torch.randn(B, d, device="cuda").mul(D ** -0.5).bfloat16()
                bias = ops.t5_decode_bias(torch.randn(32, H, device="cuda") * 2.0, S, 32, 128)
                out = torch.empty(B, d, device="cuda", dtype=torch.bfloat16)
                arms = {"hip": lambda i: ops.attn_decode_relbias(q, ring[i % copies][:, :, :d], ring[i % copies][:, :, d:], bias, H, out=out),
                        "aten": lambda i: aten_chain(q, ring[i % copies][:, :, :d], ring[i % copies][:, :, d:], bias, H)}
                a0, a1 = arms["hip"](0).clone().float(), arms["aten"](0).float()
                assert (a0 - a1).abs().max().item() <= 2e-2 * a1.abs().max().item(), (H, B, S)
                times = {"hip": [], "aten": []}
                with torch.no_grad():
                    for r in range(a.rounds + 1):
                        for name, fn in arms.items():
                            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            s.record()
                            for i in range(a.iters):
                                fn(i)
                            e.record()
                            torch.cuda.synchronize()
                            if r:                               # round 0 warms both arms up
                                times[name].append(s.elapsed_time(e) * 1e3 / a.iters)
                th, ta = statistics.median(times["hip"]), statistics.median(times["aten"])
                fmt = lambda t: f"{statistics.median(t):8.2f} ({min(t):7.2f}..{max(t):7.2f})"
                lines.append(f"{H:>3} {B:>3} {S:>5} | {fmt(times['hip'])} | {fmt(times['aten'])} | {ta / th:5.2f}")
                print(lines[-1], flush=True)
                del ring
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    else:
        print("\n".join(lines[:2]))


if __name__ == "__main__":
    main()
