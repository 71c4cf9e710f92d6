"""ops.process_logits (one launch: repetition penalty, n-gram ban, token bans, in place) against transformers' own processors run on the
device tensors, at the flagship vocabulary (V = 50272, bf16), and the decode step of generate() with the processors on against off.

    python tools/bench_logits_process.py [--rows 2,16,64,512] [--hist 64,544,2048] [--calls 200] [--rounds 5] [--no-generate]
                                         [--batches 2,16,64] [--out profiles/decode_logits_process.txt]

Kernel part.  Arms, alternated inside every round of one process; the figure is the median over the rounds of (time of N back-to-back
calls, ended by one device synchronise) / N, so it holds launch overhead as a decode step pays it:
  hip   ops.process_logits(logits, history, mask, n_masked, p, n, ban)            N = --calls
  hf    RepetitionPenaltyLogitsProcessor -> NoRepeatNGramLogitsProcessor -> SuppressTokensLogitsProcessor of transformers on the same
        device tensors (out of place; in transformers 5 the n-gram processor is vectorised on the device, older releases loop over
        the batch on the host)                                                      N = --calls / 10, or 3 where rows * L > 64 * 544
Settings (p, n, bans): penalty only (1.3, 0, 0), n-gram only (1, 3, 0), all on (1.3, 3, 3).  The history is a prompt of L - 32 columns,
ragged under a mask, plus 32 new tokens; the hf arm gets the same ids without a mask (it has no notion of one).
Generate part.  Config 3 (tools/bench_generate.py: OPT-1.3B dims, 24 frozen + 4 gated layers, 64 neighbor tokens), prompt 512, 32 new
tokens: step_ms = (generate(32) - generate(1)) / 31 with repetition_penalty = 1.3, no_repeat_ngram_size = 3, min_new_tokens = 4 against the
defaults (both arms with eos_token_id = 2, so both run the EOS tail), alternated, median (min..max) of --reps."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

V = 50272
SETTINGS = [("penalty", 1.3, 0, 0), ("ngram 3", 1.0, 3, 0), ("all on", 1.3, 3, 3)]
ON = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=4, eos_token_id=2, pad_token_id=1)


def loop_us(fn, calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6 / calls


def hf_chain(p, n, ban):
    from transformers import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor, SuppressTokensLogitsProcessor
    procs = []
    if p != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(p))
    if n:
        procs.append(NoRepeatNGramLogitsProcessor(n))
    if ban is not None:
        procs.append(SuppressTokensLogitsProcessor(ban.tolist(), device="cuda"))

    def run(ids, scores):
        for proc in procs:
            scores = proc(ids, scores)
        return scores
    return run


def kernel_part(a, lines):
    from mmgl_amd import ops
    fmt = lambda ts: f"{statistics.median(ts):9.2f} ({min(ts):8.2f}..{max(ts):9.2f})"
    lines += [f"# {torch.cuda.get_device_name(0)}; bf16 logits [rows, {V}]; hip: {a.calls} calls per loop, hf: {a.calls // 10} or 3; one synchronise "
              f"per loop; median of {a.rounds} alternating rounds (min..max); us per call",
              " rows |    L | setting |                   hip us |                        hf us | hf / hip"]
    for rows in [int(r) for r in a.rows.split(",")]:
        for L in [int(x) for x in a.hist.split(",")]:
            g = torch.Generator().manual_seed(rows + L)
            fresh = (torch.randn(rows, V, generator=g) * 3).bfloat16().cuda()
            logits = fresh.clone()
            ids = torch.randint(3, V, (rows, L + 8), generator=g).cuda()           # a history is the leading columns of the ids tensor
            T = L - 32
            mask = (torch.arange(T)[None] < torch.randint(T // 2, T + 1, (rows, 1), generator=g)).to(torch.uint8).cuda()
            hist = ids[:, :L]
            for name, p, n, n_ban in SETTINGS:
                ban = torch.tensor([5, 77, 2][:n_ban], dtype=torch.int32, device="cuda") if n_ban else None
                chain = hf_chain(p, n, ban)
                arms = dict(hip=(lambda: ops.process_logits(logits, hist, mask, None, p, n, ban), a.calls),
                            hf=(lambda: chain(hist, fresh), 3 if rows * L > 64 * 544 else max(a.calls // 10, 3)))
                for fn, _ in arms.values():            # warm-up: code objects, the caching allocator
                    loop_us(fn, 2)
                times = {k: [] for k in arms}
                for _ in range(a.rounds):
                    for k, (fn, calls) in arms.items():
                        logits.copy_(fresh)
                        times[k].append(loop_us(fn, calls))
                med = {k: statistics.median(t) for k, t in times.items()}
                line = f" {rows:4d} | {L:4d} | {name:7s} | {fmt(times['hip'])} | {fmt(times['hf'])} | {med['hf'] / med['hip']:8.1f}"
                print(line, flush=True)
                lines.append(line)


def generate_part(a, lines):
    from bench_generate import DIMS, batch_of, build, timed
    lm = build(DIMS["num_hidden_layers"])
    lines += [f"# generate(), config 3, bf16, prompt {a.prompt}, {a.new} new tokens; step_ms = (generate({a.new}) - generate(1)) / {a.new - 1}; median of "
              f"{a.reps} alternating repetitions; on = {ON}",
              "    B |  off step ms (min..max) |   on step ms (min..max) | on - off us | off generate ms | on generate ms"]
    for B in [int(b) for b in a.batches.split(",")]:
        ids, am, ne, nv = batch_of(B, a.prompt)
        arms = dict(off=lambda n: lm.generate(ids, am, neighbor_embeds=ne, neighbor_attention_mask=nv, max_new_tokens=n, eos_token_id=2,
                                              pad_token_id=1),              # the same EOS tail in both arms
                    on=lambda n: lm.generate(ids, am, neighbor_embeds=ne, neighbor_attention_mask=nv, max_new_tokens=n,
                                             **dict(ON, min_new_tokens=min(ON["min_new_tokens"], n))))
        times = {k: ([], []) for k in arms}
        for gen in arms.values():
            gen(2)
        for _ in range(a.reps):
            for k, gen in arms.items():
                times[k][0].append(timed(lambda: gen(1))[1])
                times[k][1].append(timed(lambda: gen(a.new))[1])
        step, full, spread = {}, {}, {}
        for k in arms:
            pre, full[k] = statistics.median(times[k][0]), statistics.median(times[k][1])
            step[k] = (full[k] - pre) / (a.new - 1)
            each = [(f - p) / (a.new - 1) for p, f in zip(*times[k])]
            spread[k] = f"{step[k]:6.3f} ({min(each):6.3f}..{max(each):6.3f})"
        line = (f" {B:4d} | {spread['off']} | {spread['on']} | {(step['on'] - step['off']) * 1e3:11.1f} | {full['off']:15.2f} | "
                f"{full['on']:14.2f}")
        print(line, flush=True)
        lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="2,16,64,512")
    ap.add_argument("--hist", default="64,544,2048")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-generate", action="store_true")
    ap.add_argument("--batches", default="2,16,64")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_logits_process needs the GPU: a timing taken anywhere else says nothing")
    lines = []
    kernel_part(a, lines)
    if not a.no_generate:
        generate_part(a, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
