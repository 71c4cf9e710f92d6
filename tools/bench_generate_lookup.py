"""Prompt-lookup decoding on the flagship language model (config 3: OPT-1.3B dims, 24 frozen + 4 gated layers, 64 neighbor tokens), bf16.

    python tools/bench_generate_lookup.py [--batches 2,8,16] [--ks 1,3,7] [--ngram 2] [--prompt 512] [--new 32] [--reps 3] [--out FILE]

Per batch size the greedy arm -- generate() with prompt_lookup_num_tokens = 0, the path of a checkout without the keyword -- alternates
with one arm per K in every repetition, in one process.  Whole generate() calls are timed, so the accept kernel and the host's
one read per step are in the figures:
  greedy      step_ms = (generate(--new) - generate(1)) / (--new - 1)
  lookup_K    verify_step_ms = (generate(--new, K) - generate(1, K)) / steps, with `steps` the verify steps the call ran (return_lookup_stats);
              step_ratio = verify_step_ms / the greedy step_ms -- what B*(K+1) rows cost against B rows
  launches per step are the launches of the whole call over its steps, counted as tools/bench_generate.py counts them.
Two workloads bound what the steps buy:
  floor    random weights and random prompts: nothing the model emits occurs in the prompt, drafts are rare and rejected, and `steps`
           stays at --new - 1 (tokens_per_step 1): the arm shows the pure cost of verifying
  ceiling  the successor model of tests/test_generate_lookup_gpu.py at these dimensions (attention and FFN outputs zeroed, no positions,
           gates closed, lm_head row v = embedding row v - 1: every greedy token is the previous one + 1) on ascending prompts: every
           draft is accepted and tokens_per_step reaches K + 1
Acceptance on real summaries lies between the two and needs a trained checkpoint: it is not measured here.  One JSON line per
(workload, batch size, arm)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_generate import DIMS, _Launches, batch_of, build, timed        # noqa: E402


def successor(lm):
    """Turns the random model into the successor model, in place (bf16 on the device)."""
    dec = lm.model.decoder
    with torch.no_grad():
        for layer in list(dec.layers) + list(dec.neighbor_layers):
            for mod in (layer.self_attn.out_proj, layer.fc2):
                mod.weight.zero_()
                mod.bias.zero_()
        for n_, p in lm.named_parameters():
            if n_.endswith(("gating1", "gating2")):
                p.zero_()
        dec.embed_positions.weight.zero_()
        E = torch.randn(DIMS["vocab_size"], DIMS["word_embed_proj_dim"], generator=torch.Generator().manual_seed(1)).bfloat16().cuda()
        dec.embed_tokens.weight.copy_(E)
        lm.lm_head = nn.Linear(E.shape[1], E.shape[0], bias=False, device="cuda", dtype=torch.bfloat16)      # untied from embed_tokens
        lm.lm_head.weight.copy_(torch.roll(E, 1, 0))
    return lm


def ascending(B, width):
    """Prompts whose continuation is in the prompt: start, start + 1, ..., and the start again in the last column."""
    start = 1000 + (DIMS["vocab_size"] - 2000 - width) // max(B, 1) * torch.arange(B)[:, None]
    ids = start + torch.arange(width)[None, :]
    ids[:, -1] = start[:, 0]
    return ids.cuda(), torch.ones_like(ids).cuda()


def launches(gen, n_new):
    with torch.no_grad(), _Launches() as c:
        gen(n_new)
    return c.abi + c.aten


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,8,16")
    ap.add_argument("--ks", default="1,3,7")
    ap.add_argument("--ngram", type=int, default=2)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=DIMS["num_hidden_layers"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate_lookup needs the GPU: a timing taken anywhere else says nothing")
    lm = build(a.layers)
    ks, T, lines = [int(k) for k in a.ks.split(",")], a.prompt, []
    for workload in ("floor", "ceiling"):
        if workload == "ceiling":
            successor(lm)
        for B in [int(b) for b in a.batches.split(",")]:
            _, _, ne, nv = batch_of(B, T)
            ids, am = batch_of(B, T)[:2] if workload == "floor" else ascending(B, T)
            one = lambda n, **kw: lm.generate(ids, am, neighbor_embeds=ne, neighbor_attention_mask=nv, max_new_tokens=n, **kw)
            arms = {"greedy": lambda n: one(n)}
            for K in ks:
                arms[f"lookup_{K}"] = lambda n, K=K: one(n, prompt_lookup_num_tokens=K, max_matching_ngram_size=a.ngram, return_lookup_stats=True)
            times = {n: ([], []) for n in arms}
            for gen in arms.values():                        # warm-up: code objects, caches of derived weights, every shape of the window
                gen(2)
            for _ in range(a.reps):
                for n, gen in arms.items():
                    times[n][0].append(timed(lambda: gen(1))[1])
                    times[n][1].append(timed(lambda: gen(a.new))[1])
            greedy_ids = arms["greedy"](a.new)
            greedy_step = greedy_ms = None
            for n, gen in arms.items():
                pre, full = statistics.median(times[n][0]), statistics.median(times[n][1])
                rec = dict(workload=workload, arm=n, model="opt-1.3b", layers=a.layers, dtype="bf16", batch=B, prompt=T, new_tokens=a.new,
                           device=torch.cuda.get_device_name(0), prefill_ms=pre, generate_ms=full,
                           generate_ms_all=[round(t, 2) for t in times[n][1]], tokens_per_s=B * a.new / (full * 1e-3))
                if n == "greedy":
                    steps = a.new - 1
                    greedy_step, greedy_ms = (full - pre) / steps, full
                    rec["step_ms"] = greedy_step
                else:
                    out, stats = gen(a.new)
                    steps = stats["steps"]
                    rec.update(K=int(n.split("_")[1]), ngram=a.ngram, rows_per_step=B * (int(n.split("_")[1]) + 1), steps=steps,
                               tokens_per_step=(a.new - 1) / max(steps, 1), verify_step_ms=(full - pre) / max(steps, 1),
                               same_ids_as_greedy=bool(torch.equal(out, greedy_ids)))
                    rec["step_ratio"] = rec["verify_step_ms"] / greedy_step
                    rec["speedup"] = greedy_ms / full               # > 1: faster than the greedy arm; the time ratio is its inverse
                rec["launches_per_step"] = (launches(gen, a.new) - launches(gen, 1)) / max(steps, 1)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
