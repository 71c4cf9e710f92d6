"""Neighbor guidance (generate(guidance_scale)) on the flagship language model (config 3: OPT-1.3B dims, 24 frozen + 4
gated layers, 64 neighbor tokens), bf16, against the plain greedy path.

    python tools/bench_generate_guidance.py [--batches 2,16,32,64] [--prompt 512] [--new 32] [--reps 3] [--scale 1.5] [--out FILE]
                                            [--kernel-out FILE]

Per batch size B, one JSON line with:
  * the guided decode step (2B rows: every frozen layer on all of them, every gated layer on the leading B, lm_head on 2B rows, one
    ops.guidance_logits call, argmax, the token repeated for both rows) against the plain step of B rows: ms per step (median of
    --reps runs of --new - 1 steps) and launches per step (C-ABI calls + aten ops of one step);
  * generate() with --new new tokens, guided against plain, and the two prefill times;
  * the bytes of the two caches (kv + mask + projected neighbor tokens);
  * ops.guidance_logits on the step's [2B, V] logits against the aten chain log_softmax x 2 + combine on the same tensors (events
    around --kernel-iters calls).
The model and the batches are tools/bench_generate.py's.  --kernel-out: the last arm as a text table."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_generate import DIMS, _Launches, batch_of, build, timed      # noqa: E402


def cache_bytes(cache):
    n = sum(t.numel() * t.element_size() for t in cache.kv) + cache.mask.numel()
    n += sum(k.numel() * k.element_size() + v.numel() * v.element_size() for k, v in cache.cross)
    return n


def run_steps(lm, ids, am, ne, nv, n_new, reps, g):
    """g None: the plain step of B rows; else the guided step of 2B rows.  Returns prefill ms, step ms, launches, cache bytes."""
    from mmgl_amd import ops
    dec = lm.model.decoder
    B, T = ids.shape

    def prefill():
        if g is None:
            o = dec(input_ids=ids, attention_mask=am, neighbor_embeds=ne, neighbor_attention_mask=nv, use_cache=True, cache_capacity=T + n_new - 1)
            hidden, cache = o.last_hidden_state[:, -1], o.past_key_values
        else:
            hidden, cache = dec.prefill_guided(ids, am, ne, nv, cache_capacity=T + n_new - 1)
        return cache, select(hidden)

    def select(hidden):
        logits = lm._last_logits(hidden)
        if g is not None:
            logits = ops.guidance_logits(logits, B, g)
        return logits.argmax(-1)

    def step(tok, cache):
        tok = tok if g is None else tok.repeat(2)
        return select(dec(input_ids=tok[:, None], past_key_values=cache).last_hidden_state[:, 0])

    def once(count=None):
        with torch.no_grad():
            (cache, tok), t_pre = timed(prefill)

            def steps():
                t = tok
                for s in range(n_new - 1):
                    if count is not None and s == 1:
                        with _Launches() as c:
                            t = step(t, cache)
                        count.update(abi=c.abi, aten=c.aten)
                    else:
                        t = step(t, cache)
                return t
            _, t_steps = timed(steps)
        return t_pre, t_steps / (n_new - 1), cache_bytes(cache)
    count = {}
    once(count)
    runs = [once() for _ in range(reps)]
    return dict(prefill_ms=statistics.median(r[0] for r in runs), step_ms=statistics.median(r[1] for r in runs),
                step_ms_all=[round(r[1], 4) for r in runs], launches_per_step=count["abi"] + count["aten"], abi_calls_per_step=count["abi"],
                aten_ops_per_step=count["aten"], cache_bytes=runs[0][2])


def run_generate(lm, ids, am, ne, nv, n_new, reps, g):
    kw = {} if g is None else dict(guidance_scale=g)
    call = lambda: lm.generate(ids, am, neighbor_embeds=ne, neighbor_attention_mask=nv, max_new_tokens=n_new, **kw)
    call()
    return statistics.median(timed(call)[1] for _ in range(reps))


def run_kernel(B, g, iters, seed=0):
    """ops.guidance_logits against log_softmax x 2 + combine (aten, fp32 as transformers computes it, the result cast back) on the
    same [2B, V] bf16 logits; us per call from events around `iters` calls."""
    from mmgl_amd import ops
    V = DIMS["vocab_size"]
    x = (torch.randn(2 * B, V, generator=torch.Generator().manual_seed(seed)) * 3).bfloat16().cuda()
    work = x.clone()

    def hip():
        ops.guidance_logits(work, B, g)

    def aten():
        lc = torch.log_softmax(x[:B].float(), dim=-1)
        lu = torch.log_softmax(x[B:].float(), dim=-1)
        return (lu + g * (lc - lu)).to(x.dtype)

    def us(fn):
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
    with _Launches() as c:
        aten()
    work.copy_(x)
    hip()
    err = (work[:B].float() - aten().float()).abs().max().item()
    return dict(hip_us=us(hip), aten_us=us(aten), aten_launches=c.aten, max_abs_diff_vs_aten=err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,16,32,64")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--layers", type=int, default=DIMS["num_hidden_layers"])
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate_guidance needs the GPU: a timing taken anywhere else says nothing")
    lm = build(a.layers)
    lines = []
    for B in [int(b) for b in a.batches.split(",")]:
        ids, am, ne, nv = batch_of(B, a.prompt)
        rec = dict(model="opt-1.3b", layers=a.layers, dtype="bf16", batch=B, prompt=a.prompt, new_tokens=a.new, guidance_scale=a.scale,
                   device=torch.cuda.get_device_name(0))
        plain, guided = (run_steps(lm, ids, am, ne, nv, a.new, a.reps, g) for g in (None, a.scale))
        rec.update({f"plain_{k}": v for k, v in plain.items()})
        rec.update({f"guided_{k}": v for k, v in guided.items()})
        rec.update(step_ratio=guided["step_ms"] / plain["step_ms"], extra_launches_per_step=guided["launches_per_step"] - plain["launches_per_step"],
                   cache_ratio=guided["cache_bytes"] / plain["cache_bytes"])
        rec.update(plain_generate_ms=run_generate(lm, ids, am, ne, nv, a.new, a.reps, None),
                   guided_generate_ms=run_generate(lm, ids, am, ne, nv, a.new, a.reps, a.scale))
        rec["generate_ratio"] = rec["guided_generate_ms"] / rec["plain_generate_ms"]
        rec["kernel"] = run_kernel(B, a.scale, a.kernel_iters)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    if a.kernel_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.kernel_out)), exist_ok=True)
        with open(a.kernel_out, "w") as f:
            f.write(f"ops.guidance_logits vs aten (log_softmax x 2 in fp32 + combine + cast), logits [2B, {DIMS['vocab_size']}] bf16, g = {a.scale}, "
                    f"{lines[0]['device']}, events around {a.kernel_iters} calls\n")
            f.write(f"{'B':>4} {'hip us':>10} {'aten us':>10} {'aten launches':>14} {'aten / hip':>11} {'max |diff|':>11}\n")
            for rec in lines:
                k = rec["kernel"]
                f.write(f"{rec['batch']:>4} {k['hip_us']:>10.1f} {k['aten_us']:>10.1f} {k['aten_launches']:>14} {k['aten_us'] / k['hip_us']:>11.2f} "
                        f"{k['max_abs_diff_vs_aten']:>11.3e}\n")


if __name__ == "__main__":
    main()
