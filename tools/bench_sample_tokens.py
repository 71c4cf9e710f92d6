"""ops.sample_tokens (one launch: temperature, top-k, top-p, the draw, the EOS bookkeeping and the ids column) against the aten chain
that gives the same kept set, and against the argmax + EOS tail of a greedy step, at the flagship vocabulary (V = 50272, bf16).

    python tools/bench_sample_tokens.py [--rows 2,16,64] [--calls 200] [--rounds 5] [--out profiles/decode_sample_tokens.txt]

Arms, alternated inside every round of one process; the figure is the median over the rounds of (time of `--calls` back-to-back calls,
ended by one device synchronise) / calls, so it holds launch overhead as a decode step pays it:
  hip     ops.sample_tokens(logits, u, T, k, p, finished, eos, pad, out=ids[:, c])
  aten    divide, topk + masked_fill (top-k), sort + softmax + cumsum + mask + scatter (top-p), softmax, multinomial, then where /
          full_like / == / | / setitem -- what a user of return_step_logits runs today
  greedy  torch.argmax + the same EOS ops + setitem: the tail of the greedy loops
The logits are one [rows, V] buffer that stays in L2, as the lm_head leaves them in a decode step."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V = 50272
SETTINGS = [(1.0, 0, 1.0), (0.7, 50, 0.95), (1.0, 0, 0.9)]
EOS, PAD = 2, 1


def aten_chain(logits, T, k, p, finished, col):
    x = logits.float() / T
    if k > 0:
        kth = torch.topk(x, k).values[:, -1:]
        x = x.masked_fill(x < kth, float("-inf"))
    if p < 1.0:
        sx, si = torch.sort(x, descending=True)
        pr = torch.softmax(sx, dim=-1)
        above = pr.cumsum(-1) - pr
        x = torch.full_like(x, float("-inf")).scatter(1, si, sx.masked_fill(above >= p, float("-inf")))
    tok = torch.multinomial(torch.softmax(x, dim=-1), 1)[:, 0]
    tok = torch.where(finished, torch.full_like(tok, PAD), tok)
    finished |= tok == EOS
    col.copy_(tok)


def greedy_tail(logits, finished, col):
    tok = torch.argmax(logits, dim=-1)
    tok = torch.where(finished, torch.full_like(tok, PAD), tok)
    finished |= tok == EOS
    col.copy_(tok)


def loop_us(fn, calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="2,16,64")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample_tokens needs the GPU: a timing taken anywhere else says nothing")
    from mmgl_amd import ops
    fmt = lambda ts: f"{statistics.median(ts):8.2f} ({min(ts):7.2f}..{max(ts):7.2f})"
    lines = [f"# {torch.cuda.get_device_name(0)}; bf16 logits [rows, {V}]; {a.calls} calls per loop, one synchronise per loop; median of "
             f"{a.rounds} alternating rounds (min..max); us per call",
             " rows |   T    k     p |              hip us |             aten us |           greedy us | aten / hip | greedy / hip"]
    for rows in [int(r) for r in a.rows.split(",")]:
        g = torch.Generator().manual_seed(rows)
        logits = (torch.randn(rows, V, generator=g) * 3).bfloat16().cuda()
        u = torch.rand(rows, 1, generator=g).cuda()
        ids = torch.zeros(rows, 8, dtype=torch.int64, device="cuda")
        fin_b = torch.zeros(rows, dtype=torch.bool, device="cuda")
        fin_u = torch.zeros(rows, dtype=torch.uint8, device="cuda")
        for T, k, p in SETTINGS:
            arms = dict(hip=lambda: ops.sample_tokens(logits, u, T, k, p, fin_u, EOS, PAD, out=ids[:, 3]),
                        aten=lambda: aten_chain(logits, T, k, p, fin_b, ids[:, 3]),
                        greedy=lambda: greedy_tail(logits, fin_b, ids[:, 3]))
            for fn in arms.values():                   # warm-up: code objects, the caching allocator
                loop_us(fn, 10)
            times = {n: [] for n in arms}
            for _ in range(a.rounds):
                for n, fn in arms.items():
                    fin_b.zero_()
                    fin_u.zero_()
                    times[n].append(loop_us(fn, a.calls))
            med = {n: statistics.median(t) for n, t in times.items()}
            line = (f" {rows:4d} | {T:3.1f} {k:4d} {p:5.2f} | {fmt(times['hip'])} | {fmt(times['aten'])} | {fmt(times['greedy'])} | "
                    f"{med['aten'] / med['hip']:10.2f} | {med['greedy'] / med['hip']:12.2f}")
            print(line, flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
