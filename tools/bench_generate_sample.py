"""Sampled generation on the flagship language model (config 3: OPT-1.3B dims, 24 frozen + 4 gated layers, 64 neighbor tokens), bf16.

    python tools/bench_generate_sample.py [--do_sample] [--returns 4] [--batches 2,16] [--prompt 512] [--new 32] [--reps 3] [--out FILE]

Without --do_sample: the greedy arm, MPTForCausalLM.generate as it is (the baseline on the same commit).
--do_sample: three more arms per batch size, alternated with the greedy one in every repetition:
  sample      generate(do_sample=True, temperature=0.7, top_k=50, top_p=0.95): the greedy loop with ops.sample_tokens as its tail
  sample_R    generate(..., num_return_sequences=R): one prefill of B rows, then steps of B*R rows on the beam-shared cache
  repeated_R  the prompts repeated R times with num_return_sequences=1: what R continuations per prompt cost without the shared cache
Whole generate() calls are timed and counted, so the selection tail of each loop is in the figures: prefill_ms is generate(1 new token),
step_ms = (generate(--new) - generate(1)) / (--new - 1), launches_per_step = launches of generate(3) - launches of generate(2), counted
as tools/bench_generate.py counts them (C-ABI calls + aten ops that launch).  One JSON line per (batch size, arm)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_generate import DIMS, _Launches, batch_of, build, timed        # noqa: E402
from bench_generate_beam import cache_bytes                               # noqa: E402

KNOBS = dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.95, seed=0)


def launches(gen, n_new):
    with torch.no_grad(), _Launches() as c:
        gen(n_new)
    return c.abi + c.aten


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--do_sample", action="store_true")
    ap.add_argument("--returns", type=int, default=4)
    ap.add_argument("--batches", default="2,16")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=DIMS["num_hidden_layers"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate_sample needs the GPU: a timing taken anywhere else says nothing")
    lm = build(a.layers)
    R, T, lines = a.returns, a.prompt, []
    for B in [int(b) for b in a.batches.split(",")]:
        ids, am, ne, nv = batch_of(B, T)
        rep = lambda t: t.repeat_interleave(R, 0).contiguous()
        one = lambda n, **kw: lm.generate(ids, am, neighbor_embeds=ne, neighbor_attention_mask=nv, max_new_tokens=n, **kw)
        arms = {"greedy": (lambda n: one(n), B, cache_bytes(lm, B, 0, B, T + a.new - 1, 0))}
        if a.do_sample:
            arms["sample"] = (lambda n: one(n, **KNOBS), B, cache_bytes(lm, B, 0, B, T + a.new - 1, 0))
            arms[f"sample_R{R}"] = (lambda n: one(n, num_return_sequences=R, **KNOBS), B * R, cache_bytes(lm, B, B * R, B, T, a.new - 1))
            big = (rep(ids), rep(am), rep(ne), rep(nv))
            arms[f"repeated_R{R}"] = (lambda n: lm.generate(big[0], big[1], neighbor_embeds=big[2], neighbor_attention_mask=big[3],
                                                            max_new_tokens=n, **KNOBS), B * R, cache_bytes(lm, B * R, 0, B * R, T + a.new - 1, 0))
        times = {n: ([], []) for n in arms}
        for gen, _, _ in arms.values():                  # warm-up: code objects, caches of derived weights, every shape of the window
            gen(2)
        for _ in range(a.reps):
            for n, (gen, _, _) in arms.items():
                times[n][0].append(timed(lambda: gen(1))[1])
                times[n][1].append(timed(lambda: gen(a.new))[1])
        for n, (gen, rows, cbytes) in arms.items():
            pre, full = statistics.median(times[n][0]), statistics.median(times[n][1])
            rec = dict(arm=n, model="opt-1.3b", layers=a.layers, dtype="bf16", batch=B, rows=rows, prompt=T, new_tokens=a.new,
                       device=torch.cuda.get_device_name(0), prefill_ms=pre, step_ms=(full - pre) / (a.new - 1), generate_ms=full,
                       generate_ms_all=[round(t, 2) for t in times[n][1]], launches_per_step=launches(gen, 3) - launches(gen, 2),
                       cache_bytes=cbytes, sequences_per_s=rows / (full * 1e-3))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
