"""mmgl_attn_decode_beam_fwd against mmgl_attn_decode_fwd on K / V expanded to B*W rows, alternating in one process.

    python tools/bench_attn_decode_beam.py [--batches 2,16] [--beams 4] [--prefix 512] [--tail 31] [--iters 200] [--rounds 5] [--out FILE]

Both arms compute the same bf16 out[B*W, H*D] (H = 32, D = 64).  The beam kernel reads the sample's prefix rows [B, S_pre, 2d] once for
its W queries and the hypotheses' own keys through the parent table from a tail [B*W, n_tail, 2d]; the multi-head kernel -- the only
other route there is -- needs every hypothesis' S_pre + n_tail keys and values laid out as its own cache rows [B*W, S_pre + n_tail, 2d]
(the expansion and the per-step reordering of those rows are not timed: a cache kept in that layout would pay them elsewhere).  A decode
step streams gigabytes of weights between two attention calls, so no cache row is in a cache when its call starts: each timed loop walks
a ring of caches larger than the 256 MB Infinity Cache.  Rounds alternate beam / expanded / beam / ...; the table gives the median
microseconds per call of each arm (min..max over the rounds), the bytes each arm reads over its time, and the ratio.  There is no
adoption threshold: the beam kernel is the only route that keeps the shared cache; the record says what it costs or gains."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, D = 32, 64
RING_BYTES = 640 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,16")
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--prefix", type=int, default=512)
    ap.add_argument("--tail", type=int, default=31)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_decode_beam needs the GPU")
    from mmgl_amd import ops
    W, S, n, d = a.beams, a.prefix, a.tail, H * D
    lines = [f"# {torch.cuda.get_device_name(0)}; bf16; H = {H}, D = {D}, W = {W}, S_pre = {S}, n_tail = {n}; {a.iters} calls per loop over a ring "
             f"of caches >= {RING_BYTES >> 20} MiB; median of {a.rounds} alternating rounds (min..max)",
             f"{'B':>3} {'rows':>4} | {'beam us':>24} | {'expanded multi-head us':>24} | {'beam TB/s':>9} | {'mha TB/s':>8} | mha / beam time"]
    for B in [int(b) for b in a.batches.split(",")]:
        R = B * W
        beam_bytes, big_bytes = (B * S + R * n) * 2 * d * 2, R * (S + n) * 2 * d * 2
        copies = max(2, -(-RING_BYTES // beam_bytes))
        big_copies = max(2, -(-RING_BYTES // big_bytes))
        pre = [torch.randn(B, S, 2 * d, device="cuda").bfloat16() for _ in range(copies)]
        tail = [torch.randn(R, n, 2 * d, device="cuda").bfloat16() for _ in range(copies)]
        src = torch.stack([(torch.arange(R, device="cuda") + j) % W for j in range(n)], 1).int().contiguous()        # a new slot at every step
        rows = (torch.arange(R, device="cuda") // W * W)[:, None] + src.long()
        cols = torch.arange(n, device="cuda")[None, :].expand(R, -1)
        expand = lambda i: torch.cat([pre[i].repeat_interleave(W, 0), tail[i][rows, cols]], 1).contiguous()
        big = [expand(i) for i in range(big_copies)]
        q = (torch.randn(R, d, device="cuda") * D ** -0.5).bfloat16()
        valid = torch.ones(B, S, dtype=torch.uint8, device="cuda")
        valid[:, S - S // 8:] = torch.rand(B, S // 8, device="cuda") > 0.5
        big_valid = torch.cat([valid.repeat_interleave(W, 0), torch.ones(R, n, dtype=torch.uint8, device="cuda")], 1).contiguous()
        out = torch.empty(R, d, device="cuda", dtype=torch.bfloat16)
        arms = {"beam": lambda i: ops.attn_decode_beam(q, pre[i % copies][:, :, :d], pre[i % copies][:, :, d:], valid, H, W,
                                                       tail[i % copies][:, :, :d], tail[i % copies][:, :, d:], src, out=out),
                "mha": lambda i: ops.attn_decode(q, big[i % big_copies][:, :, :d], big[i % big_copies][:, :, d:], big_valid, H, out=out)}
        a0, a1 = arms["beam"](0).clone(), arms["mha"](0).clone()
        assert (a0.float() - a1.float()).abs().max().item() <= 2e-2 * a1.float().abs().max().item(), B
        times = {"beam": [], "mha": []}
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
        tb, tm = statistics.median(times["beam"]), statistics.median(times["mha"])
        fmt = lambda t: f"{statistics.median(t):8.2f} ({min(t):7.2f}..{max(t):7.2f})"
        lines.append(f"{B:>3} {R:>4} | {fmt(times['beam'])} | {fmt(times['mha'])} | {beam_bytes / (tb * 1e-6) / 1e12:9.2f} | "
                     f"{big_bytes / (tm * 1e-6) / 1e12:8.2f} | {tm / tb:5.2f}")
        print(lines[-1], flush=True)
        del pre, tail, big
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    else:
        print("\n".join(lines[:2]))


if __name__ == "__main__":
    main()
