"""Greedy generation of a T5 at T5-small dimensions (d_model 512, 8 heads of 64, d_ff 2048, 6 + 6 layers, vocab 32128): the native
T5HipRunner.generate against the stock HuggingFace generate on the same weights, arms alternating in one process.

    python tools/bench_generate_t5.py [--batches 2,16,64] [--dtypes bf16,fp32] [--width 512] [--new 32] [--reps 5] [--out FILE]

native:  T5HipRunner.generate(input_ids, attention_mask, max_new_tokens=N) -- the encoder and the cross keys / values once, then N cached
         decoder steps on csrc/decode.hip (skinny GEMMs, mmgl_attn_decode_relbias_fwd, mmgl_attn_decode_fwd over the encoder's keys).
stock:   lm.generate(input_ids, attention_mask, use_cache=True, do_sample=False, max_new_tokens=N, min_new_tokens=N) of transformers.
Both arms are timed with a host clock around the call and a device synchronise inside the window, for N = --new and for N = 1; every
shape is warmed up first, rounds alternate native / stock, medians are reported.  From the two lengths:
  generate_ms   the whole call at N = --new
  prefill_ms    the call at N = 1: the encoder, the cross keys and values, the start token's step and one selection
  step_ms       (generate_ms - prefill_ms) / (N - 1): one further token
launches_per_step (native only) counts the C-ABI calls and aten ops that N = 3 adds over N = 2.  Prompts are ragged (right-padded to
--width columns).  One JSON line per (dtype, batch) goes to stdout (and to --out).  No speed threshold: the record says what comes out."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_generate import _Launches, timed        # noqa: E402

DIMS = dict(vocab_size=32128, d_model=512, d_kv=64, d_ff=2048, num_layers=6, num_decoder_layers=6, num_heads=8)
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


def build(dtype):
    from transformers import T5Config, T5ForConditionalGeneration
    cfg = T5Config(dropout_rate=0.0, decoder_start_token_id=0, pad_token_id=0, eos_token_id=1, **DIMS)
    torch.manual_seed(0)
    lm = T5ForConditionalGeneration(cfg)
    with torch.no_grad():                                   # HuggingFace's init gives the tables std d_model^-0.5: make the bias matter
        for stack in (lm.encoder, lm.decoder):
            stack.block[0].layer[0].SelfAttention.relative_attention_bias.weight.normal_(0, 0.5)
    return lm.to(dtype).cuda().eval()


def batch_of(B, width, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, DIMS["vocab_size"], (B, width), generator=g)
    am = torch.ones_like(ids)
    for b in range(1, B):
        am[b, int(torch.randint(min(64, width), width + 1, (1,), generator=g)):] = 0
    return torch.where(am.bool(), ids, torch.zeros_like(ids)).cuda(), am.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,16,64")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate_t5 needs the GPU: a timing taken anywhere else says nothing")
    from mmgl_amd.model.t5_hip import T5HipRunner
    lines = []
    for name in a.dtypes.split(","):
        lm = build(DTYPES[name])
        run = T5HipRunner(lm)
        for B in [int(b) for b in a.batches.split(",")]:
            ids, am = batch_of(B, a.width)
            arms = {"native": lambda n: run.generate(input_ids=ids, attention_mask=am, max_new_tokens=n),
                    "stock": lambda n: lm.generate(input_ids=ids, attention_mask=am, use_cache=True, do_sample=False, max_new_tokens=n,
                                                   min_new_tokens=n)}
            times = {(arm, n): [] for arm in arms for n in (1, a.new)}
            with torch.no_grad():
                for r in range(a.reps + 1):
                    for arm, fn in arms.items():
                        for n in (1, a.new):
                            out, t = timed(lambda: fn(n))
                            assert tuple(out.shape) == (B, 1 + n), (arm, tuple(out.shape))
                            if r:                               # round 0 warms every shape of both arms up
                                times[(arm, n)].append(t)
                counts = []
                for n in (2, 3):
                    with _Launches() as c:
                        arms["native"](n)
                    counts.append((c.abi, c.aten))
            rec = dict(model="t5-small dims", dtype=name, batch=B, width=a.width, new_tokens=a.new, device=torch.cuda.get_device_name(0),
                       reps=a.reps)
            for arm in arms:
                gen, pre = statistics.median(times[(arm, a.new)]), statistics.median(times[(arm, 1)])
                rec[arm] = dict(generate_ms=round(gen, 3), prefill_ms=round(pre, 3), step_ms=round((gen - pre) / max(a.new - 1, 1), 4),
                                generate_ms_all=[round(t, 2) for t in times[(arm, a.new)]])
            rec["native"].update(abi_calls_per_step=counts[1][0] - counts[0][0], aten_ops_per_step=counts[1][1] - counts[0][1],
                                 launches_per_step=sum(counts[1]) - sum(counts[0]))
            rec["stock_over_native_generate_ms"] = round(rec["stock"]["generate_ms"] / rec["native"]["generate_ms"], 2)
            rec["stock_over_native_step_ms"] = round(rec["stock"]["step_ms"] / rec["native"]["step_ms"], 2)
            rec["tokens_per_s"] = round(B * a.new / (rec["native"]["generate_ms"] * 1e-3), 1)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del lm, run
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
