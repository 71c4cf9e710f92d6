"""Prompt-lookup decoding on the Llama-family neighbor LM at the settings of tools/bench_generate_llama.py (config-5 dimensions, 8 frozen +
1 gated layer, 128 neighbor tokens, bf16), multi-head (Hkv = 32) and grouped-query (Hkv = 8).

    python tools/bench_generate_lookup_llama.py [--kv-heads 32,8] [--batches 2,16] [--ks 1,3,7] [--ngram 2] [--prompt 512] [--new 32]
                                                [--reps 3] [--kernels-only] [--out FILE]

The arms, the two workloads and every figure are those of tools/bench_generate_lookup.py (see its docstring): per batch size the greedy
arm -- generate() with prompt_lookup_num_tokens = 0, the path of a checkout without the keyword -- alternates with one arm per K in every
repetition, in one process; whole generate() calls are timed.
  floor    random weights, random prompts: drafts are rare and rejected; the arm shows what a verify step of B*(K+1) rows costs
           against a greedy step of B rows (step_ratio)
  ceiling  the successor Llama of tests/test_generate_lookup_llama_gpu.py at these dimensions (o_proj and down_proj zeroed, gates 0,
           lm_head row v = embedding row v - 1) on ascending prompts: every draft is accepted, tokens_per_step reaches K + 1
Behind them, per Hkv and batch size, the two kernels of a verify step on their own (workload "kernel": mmgl_rope_kv_append_block and
mmgl_attn_decode_gqa_block_fwd at K + 1 rows per sample against mmgl_rope_kv_append and the greedy step's attention at one, over
--prompt cache columns; see kernel_records).  One JSON line per (workload, Hkv, batch size, arm)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_generate import timed                                # noqa: E402
from bench_generate_llama import DIMS, batch_of, build          # noqa: E402
from bench_generate_lookup import launches                      # noqa: E402


def successor(lm):
    """Turns the random model into the successor model, in place (bf16 on the device)."""
    with torch.no_grad():
        for layer in lm.llama.model.layers:
            layer.self_attn.o_proj.weight.zero_()
            layer.mlp.down_proj.weight.zero_()
        for layer in lm.neighbor_layers:
            layer.gating1.zero_()
            layer.gating2.zero_()
        E = torch.randn(DIMS["vocab_size"], DIMS["hidden_size"], generator=torch.Generator().manual_seed(1)).bfloat16().cuda()
        lm.llama.model.embed_tokens.weight.copy_(E)
        lm.llama.lm_head.weight.copy_(torch.roll(E, 1, 0))
    return lm


def ascending(B, width):
    """Prompts whose continuation is in the prompt: start, start + 1, ..., and the start again in the last column."""
    start = 1000 + (DIMS["vocab_size"] - 2000 - width) // max(B, 1) * torch.arange(B)[:, None]
    ids = start + torch.arange(width)[None, :]
    ids[:, -1] = start[:, 0]
    return ids.cuda(), torch.ones_like(ids).cuda()


def kernel_records(kv_heads, B, S, ks, calls=40, ring=8):
    """The two kernels of a verify step on their own against the two of a greedy step, us per call: HIP events around `calls` calls
    that walk a ring of caches (cold keys), the four arms alternating, median of 5 rounds.  len[b] = S for every sample."""
    from mmgl_amd import ops
    H, D = DIMS["num_attention_heads"], DIMS["hidden_size"] // DIMS["num_attention_heads"]
    nq, nkv, cap = H * D, kv_heads * D, S + 8
    g = torch.Generator().manual_seed(0)
    caches = [torch.randn(B, cap, 2 * nkv, generator=g).bfloat16().cuda() for _ in range(ring)]
    mask = torch.ones(B, cap, dtype=torch.uint8, device="cuda")
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
    ang = torch.rand(cap, D // 2, generator=g) * 6.0
    table = torch.stack([ang.cos(), ang.sin()], dim=-1).float().contiguous().cuda()
    rows = lambda m: (torch.randn(B * m, nq + 2 * nkv, generator=g) * D ** -0.5).bfloat16().cuda()

    def us(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(calls):
            fn(caches[i % ring])
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) * 1e3 / calls
    one = rows(1)
    arms = {"attn_greedy": lambda kv: ops.attn_decode(one[:, :nq], kv[:, :S + 1, :nkv], kv[:, :S + 1, nkv:], mask[:, :S + 1], H, num_kv_heads=kv_heads),
            "rope_greedy": lambda kv: ops.rope_kv_append(one, table[S], kv[:, S], H, kv_heads)}
    for K in ks:
        blk = rows(K + 1)
        arms[f"attn_block_{K}"] = lambda kv, blk=blk, K=K: ops.attn_decode_gqa_block(blk[:, :nq], kv[:, :, :nkv], kv[:, :, nkv:], mask, lens, H, kv_heads, K + 1)
        arms[f"rope_block_{K}"] = lambda kv, blk=blk, K=K: ops.rope_kv_append_block(blk, table, kv, lens, H, kv_heads, K + 1)
    times = {n: [] for n in arms}
    for fn in arms.values():
        us(fn)
    for _ in range(5):
        for n, fn in arms.items():
            times[n].append(us(fn))
    return [dict(workload="kernel", arm=n, heads=H, kv_heads=kv_heads, head_dim=D, dtype="bf16", batch=B, cache_columns=S,
                 us_per_call=statistics.median(t), us_all=[round(x, 1) for x in t], device=torch.cuda.get_device_name(0)) for n, t in times.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kv-heads", default="32,8")
    ap.add_argument("--batches", default="2,16")
    ap.add_argument("--ks", default="1,3,7")
    ap.add_argument("--ngram", type=int, default=2)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="skip the generate() arms: only the per-kernel records")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate_lookup_llama needs the GPU: a timing taken anywhere else says nothing")
    ks, T, lines = [int(k) for k in a.ks.split(",")], a.prompt, []
    for kv_heads in [int(h) for h in a.kv_heads.split(",")]:
        lm = None if a.kernels_only else build(a.layers, kv_heads)
        for workload in () if a.kernels_only else ("floor", "ceiling"):
            if workload == "ceiling":
                successor(lm)
            for B in [int(b) for b in a.batches.split(",")]:
                _, _, ne, nv = batch_of(B, T)
                ids, am = batch_of(B, T)[:2] if workload == "floor" else ascending(B, T)
                one = lambda n, **kw: lm.generate(ids, am, neighbor_embeds=ne, neighbor_attention_mask=nv, max_new_tokens=n, **kw)
                arms = {"greedy": lambda n: one(n)}
                for K in ks:
                    arms[f"lookup_{K}"] = lambda n, K=K: one(n, prompt_lookup_num_tokens=K, max_matching_ngram_size=a.ngram,
                                                             return_lookup_stats=True)
                times = {n: ([], []) for n in arms}
                for gen in arms.values():                    # warm-up: code objects, caches of derived weights, every shape of the window
                    gen(2)
                for _ in range(a.reps):
                    for n, gen in arms.items():
                        times[n][0].append(timed(lambda: gen(1))[1])
                        times[n][1].append(timed(lambda: gen(a.new))[1])
                greedy_ids = arms["greedy"](a.new)
                greedy_step = greedy_ms = None
                for n, gen in arms.items():
                    pre, full = statistics.median(times[n][0]), statistics.median(times[n][1])
                    rec = dict(workload=workload, arm=n, model="llama-2-7b dims", layers=a.layers, gated_layers=len(lm.neighbor_layers),
                               heads=DIMS["num_attention_heads"], kv_heads=kv_heads, dtype="bf16", batch=B, prompt=T, new_tokens=a.new,
                               device=torch.cuda.get_device_name(0), prefill_ms=pre, generate_ms=full,
                               generate_ms_all=[round(t, 2) for t in times[n][1]], tokens_per_s=B * a.new / (full * 1e-3))
                    if n == "greedy":
                        steps = a.new - 1
                        greedy_step, greedy_ms = (full - pre) / steps, full
                        rec["step_ms"] = greedy_step
                    else:
                        out, stats = gen(a.new)
                        steps, K = stats["steps"], int(n.split("_")[1])
                        rec.update(K=K, ngram=a.ngram, rows_per_step=B * (K + 1), steps=steps, tokens_per_step=(a.new - 1) / max(steps, 1),
                                   verify_step_ms=(full - pre) / max(steps, 1), same_ids_as_greedy=bool(torch.equal(out, greedy_ids)))
                        rec["step_ratio"] = rec["verify_step_ms"] / greedy_step
                        rec["speedup"] = greedy_ms / full           # > 1: faster than the greedy arm; the time ratio is its inverse
                    rec["launches_per_step"] = (launches(gen, a.new) - launches(gen, 1)) / max(steps, 1)
                    print(json.dumps(rec), flush=True)
                    lines.append(rec)
        del lm
        torch.cuda.empty_cache()
        for B in [int(b) for b in a.batches.split(",")]:
            for rec in kernel_records(kv_heads, B, T, ks):
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
