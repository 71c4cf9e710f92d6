"""Contrastive search on the flagship language model (config 3: OPT-1.3B dims, 24 frozen + 4 gated layers, 64 neighbor tokens), bf16.

    python tools/bench_generate_contrastive.py [--batches 2,16] [--ks 4,8] [--prompt 512] [--new 32] [--reps 3] [--out FILE] [--select-out FILE]

Two measurements, one process:
  * the select call alone: ops.contrastive_select against the aten chain a library implementation runs for the same step (normalise,
    bmm, masked max, score, argmax, gathers, the row copies -- in the model dtype, as transformers did) on the same device tensors, at
    n_ctx = prompt + new - 1, d = 2048.  Device events around `--iters` back-to-back calls; TB/s on the context bytes B n_ctx d 2.
  * a contrastive step against a greedy step: per (B, k) the greedy arm of tools/bench_generate.py and then the loop of
    generation.contrastive_loop (lm_head on B rows, ops.beam_topk, one decode step of B*k rows on the beam-shared cache,
    ops.contrastive_select), ms per step, launches per step, ms per generate(), and the cache bytes -- ours (one prompt cache, a
    [B*k, new, 2d] tail per layer, the context buffer) against the k-fold cache a library implementation holds; that figure is
    arithmetic, not a run."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_generate import DIMS, _Launches, batch_of, build, run_cached, timed        # noqa: E402
from bench_generate_beam import cache_bytes        # noqa: E402

ALPHA = 0.6


def select_case(B, k, n_ctx, seed=0):
    d, V = DIMS["hidden_size"], DIMS["vocab_size"]
    g = torch.Generator().manual_seed(seed)
    t = dict(cand=torch.randn(B * k, d, generator=g).bfloat16(), ctx=torch.randn(B, n_ctx + 1, d, generator=g).bfloat16(),
             valid=(torch.rand(B, n_ctx + 1, generator=g) > 0.1).to(torch.uint8),
             cs=torch.log_softmax(torch.randn(B, 2 * k, generator=g), -1).sort(dim=-1, descending=True).values.contiguous(),
             ci=torch.stack([torch.randperm(V, generator=g)[:2 * k] for _ in range(B)]).int(),
             src=torch.zeros(B * k, 4, dtype=torch.int32), ids=torch.zeros(B, 4, dtype=torch.int64))
    return {key: v.cuda() for key, v in t.items()}


def aten_select(t, B, k, n_ctx, alpha):
    """The same step through aten, as a library implementation ranks: returns (selected, hidden) and writes the same outputs."""
    d = t["cand"].shape[1]
    h = torch.nn.functional.normalize(t["cand"].view(B, k, d), dim=-1)
    c = torch.nn.functional.normalize(t["ctx"][:, :n_ctx], dim=-1)
    cos = torch.bmm(h, c.transpose(1, 2)).float().masked_fill(t["valid"][:, None, :n_ctx] == 0, float("-inf"))
    score = (1.0 - alpha) * t["cs"][:, :k].exp() - alpha * cos.amax(-1)
    sel = score.argmax(-1)
    hidden = t["cand"].view(B, k, d).gather(1, sel[:, None, None].expand(B, 1, d))[:, 0]
    t["ids"][:, 1] = t["ci"][:, :k].gather(1, sel[:, None])[:, 0]
    t["ctx"][:, n_ctx] = hidden
    t["valid"][:, n_ctx] = 1
    t["src"][:, 1] = sel.int().repeat_interleave(k)
    return sel, hidden


def events_us(fn, iters):
    for _ in range(5):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def bench_select(B, k, n_ctx, iters):
    from mmgl_amd import ops
    t = select_case(B, k, n_ctx)
    V = DIMS["vocab_size"]
    hip = lambda: ops.contrastive_select(t["cand"], t["ctx"], t["valid"], t["cs"], t["ci"], ALPHA, n_ctx, 1, t["src"], t["ids"][:, 1], V)
    sel_a, _ = aten_select(t, B, k, n_ctx, ALPHA)
    _, sel_h = hip()
    agree = float((sel_a.int() == sel_h).float().mean())                       # bf16 bmm against fp32 accumulation: near-ties may differ
    us_hip = [events_us(hip, iters) for _ in range(3)]
    us_aten = [events_us(lambda: aten_select(t, B, k, n_ctx, ALPHA), iters) for _ in range(3)]
    nbytes = B * n_ctx * DIMS["hidden_size"] * 2
    return dict(batch=B, k=k, n_ctx=n_ctx, d=DIMS["hidden_size"], select_us=statistics.median(us_hip), select_us_all=[round(u, 2) for u in us_hip],
                context_bytes=nbytes, context_TBps=nbytes / statistics.median(us_hip) / 1e6, aten_us=statistics.median(us_aten),
                aten_us_all=[round(u, 2) for u in us_aten], aten_over_select=statistics.median(us_aten) / statistics.median(us_hip),
                selections_equal=agree)


def run_contrastive(lm, ids, am, ne, nv, n_new, k, reps):
    from mmgl_amd import ops
    from mmgl_amd.model.modelling_cross_attention import BeamState
    dec = lm.model.decoder
    B, T = ids.shape
    d, V = DIMS["hidden_size"], DIMS["vocab_size"]
    start = torch.zeros(B, dtype=torch.float32, device="cuda")

    def prefill():
        o = dec(input_ids=ids, attention_mask=am, neighbor_embeds=ne, neighbor_attention_mask=nv, use_cache=True, cache_capacity=T)
        cache = o.past_key_values
        cache.beam = BeamState(cache, k, n_new)
        st = dict(cache=cache, out=torch.empty(B, T + n_new, dtype=torch.int64, device="cuda"),
                  ctx=torch.empty(B, T + n_new, d, dtype=torch.bfloat16, device="cuda"), valid=torch.zeros(B, T + n_new, dtype=torch.uint8, device="cuda"))
        st["ctx"][:, :T] = o.last_hidden_state
        st["valid"][:, :T] = am != 0
        return st, o.last_hidden_state[:, -1]

    def step(st, hidden, s):
        cs, ci = ops.beam_topk(lm._last_logits(hidden), start, k, rows_in=1)
        h = dec(input_ids=ci[:, :k].reshape(B * k, 1), past_key_values=st["cache"]).last_hidden_state[:, 0]
        return ops.contrastive_select(h, st["ctx"], st["valid"], cs, ci, ALPHA, T + s, s, st["cache"].beam.book.src, st["out"][:, T + s], V)[0]

    def once(count=None):
        with torch.no_grad():
            (st, hidden), t_pre = timed(prefill)

            def steps():
                h = hidden
                for s in range(n_new):
                    if count is not None and s == 2:
                        with _Launches() as c:
                            h = step(st, h, s)
                        count.update(abi=c.abi, aten=c.aten)
                    else:
                        h = step(st, h, s)
                return h
            _, t_steps = timed(steps)
        return t_pre, t_steps / n_new
    count = {}
    once(count)
    runs = [once() for _ in range(reps)]
    gen = lambda: lm.generate(ids, am, neighbor_embeds=ne, neighbor_attention_mask=nv, max_new_tokens=n_new, penalty_alpha=ALPHA, top_k=k)
    _, t_gen = timed(gen)
    return dict(prefill_ms=statistics.median(r[0] for r in runs), step_ms=statistics.median(r[1] for r in runs),
                step_ms_all=[round(r[1], 4) for r in runs], generate_ms=t_gen, launches_per_step=count["abi"] + count["aten"],
                abi_calls_per_step=count["abi"], aten_ops_per_step=count["aten"])


def write(path, lines):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,16")
    ap.add_argument("--ks", default="4,8")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--layers", type=int, default=DIMS["num_hidden_layers"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--select-out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate_contrastive needs the GPU: a timing taken anywhere else says nothing")
    batches, ks = [int(b) for b in a.batches.split(",")], [int(k) for k in a.ks.split(",")]
    dev = torch.cuda.get_device_name(0)
    sel = []
    for B in batches:
        for k in ks:
            rec = dict(bench_select(B, k, a.prompt + a.new - 1, a.iters), dtype="bf16", device=dev)
            print(json.dumps(rec), flush=True)
            sel.append(rec)
    write(a.select_out, sel)
    lm = build(a.layers)
    d, lines = DIMS["hidden_size"], []
    for B in batches:
        ids, am, ne, nv = batch_of(B, a.prompt)
        greedy = run_cached(lm, ids, am, ne, nv, a.new, a.reps)
        for k in ks:
            rec = dict(model="opt-1.3b", layers=a.layers, dtype="bf16", batch=B, k=k, rows=B * k, prompt=a.prompt, new_tokens=a.new, alpha=ALPHA, device=dev)
            rec["greedy"] = greedy
            rec["contrastive"] = c = run_contrastive(lm, ids, am, ne, nv, a.new, k, a.reps)
            rec["step_over_greedy"] = c["step_ms"] / greedy["step_ms"]
            rec["generate_over_greedy"] = c["generate_ms"] / greedy["generate_ms"]
            rec["cache_bytes"] = cache_bytes(lm, B, B * k, B, a.prompt, a.new) + 2 * B * (a.prompt + a.new) * d
            rec["cache_bytes_k_fold"] = cache_bytes(lm, B * k, 0, B * k, a.prompt + a.new, 0) + 2 * B * (a.prompt + a.new) * d
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    write(a.out, lines)


if __name__ == "__main__":
    main()
