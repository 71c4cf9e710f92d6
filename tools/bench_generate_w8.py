"""generate() with FP8 frozen weights (weight_dtype="fp8") on the flagship language model (config 3: OPT-1.3B dims, 24
frozen + 4 gated layers, 64 neighbor tokens), bf16, against the model's dtype, in one process.

    python tools/bench_generate_w8.py [--batches 2,16,64] [--guided 64] [--prompt 512] [--new 32] [--reps 3] [--out FILE]

Per batch size B the plain decode step of B rows on the bf16 weights and on their e4m3fn codes, alternating rep by rep: ms per step
(median of --reps runs of --new - 1 steps), launches per step (C-ABI calls + aten ops of one step) and ms per generate() call
(alternating too, median of --reps after a warm-up pass; the codes exist already, quantised once by the warm-up).  --guided B: the same for the guided step of 2B rows
(generate(guidance_scale): every frozen layer on 2B rows, two skinny GEMM calls per linear above 64 rows) -- the step with more than
64 rows.  The model and the
batches are tools/bench_generate.py's: q, k and v are multiplied one by one there (the parameters are not frozen), 6 GEMMs per layer."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_generate import _Launches, batch_of, build, timed      # noqa: E402


def one_run(lm, ids, am, ne, nv, n_new, w8, g, count=None):
    from mmgl_amd import ops
    from mmgl_amd.model.decode_cache import StepCodes
    dec = lm.model.decoder
    B, T = ids.shape

    def select(hidden):
        logits = lm._last_logits(hidden)
        if g is not None:
            logits = ops.guidance_logits(logits, B, g)
        return logits.argmax(-1)

    def prefill():
        if g is None:
            o = dec(input_ids=ids, attention_mask=am, neighbor_embeds=ne, neighbor_attention_mask=nv, use_cache=True, cache_capacity=T + n_new - 1)
            hidden, cache = o.last_hidden_state[:, -1], o.past_key_values
        else:
            hidden, cache = dec.prefill_guided(ids, am, ne, nv, cache_capacity=T + n_new - 1)
        cache.w8 = StepCodes() if w8 else None
        return cache, select(hidden)

    def step(tok, cache):
        tok = tok if g is None else tok.repeat(2)
        return select(dec(input_ids=tok[:, None], past_key_values=cache).last_hidden_state[:, 0])

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
    return t_pre, t_steps / (n_new - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,16,64")
    ap.add_argument("--guided", default="64", help="batch sizes of the guided step of 2B rows (empty: none)")
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate_w8 needs the GPU: a timing taken anywhere else says nothing")
    lm = build(a.layers)
    cases = [(int(b), None) for b in a.batches.split(",") if b] + [(int(b), a.scale) for b in a.guided.split(",") if b]
    lines = []
    for B, g in cases:
        ids, am, ne, nv = batch_of(B, a.prompt)
        arms = {"plain": False, "w8": True}
        counts = {name: {} for name in arms}
        for name, w8 in arms.items():                           # warm-up: code objects, the codes; counts one step's launches
            one_run(lm, ids, am, ne, nv, a.new, w8, g, counts[name])
        runs = {name: [] for name in arms}
        for _ in range(a.reps):
            for name, w8 in arms.items():
                runs[name].append(one_run(lm, ids, am, ne, nv, a.new, w8, g))
        rec = dict(model="opt-1.3b dims", layers=a.layers, gated_layers=len(lm.model.decoder.neighbor_layers), dtype="bf16", batch=B,
                   rows_per_step=B if g is None else 2 * B, mode="greedy" if g is None else f"guidance_scale={g}", prompt=a.prompt,
                   new_tokens=a.new, device=torch.cuda.get_device_name(0),
                   command="python " + " ".join([os.path.relpath(sys.argv[0])] + sys.argv[1:]))
        kw = {} if g is None else dict(guidance_scale=g)
        gen = {name: [] for name in arms}
        for _ in range(a.reps + 1):                             # generate() itself, alternating as well; the first pass warms it up
            for name, w8 in arms.items():
                gen[name].append(timed(lambda: lm.generate(ids, am, neighbor_embeds=ne, neighbor_attention_mask=nv, max_new_tokens=a.new,
                                                           weight_dtype="fp8" if w8 else None, **kw))[1])
        for name, w8 in arms.items():
            t_gen, t_gen_all = statistics.median(gen[name][1:]), [round(t, 3) for t in gen[name][1:]]
            r, c = runs[name], counts[name]
            rec[name] = dict(prefill_ms=statistics.median(x[0] for x in r), step_ms=statistics.median(x[1] for x in r),
                             step_ms_all=[round(x[1], 4) for x in r], generate_ms=t_gen, generate_ms_all=t_gen_all, launches_per_step=c["abi"] + c["aten"],
                             abi_calls_per_step=c["abi"], aten_ops_per_step=c["aten"])
        rec["step_plain_over_w8"] = rec["plain"]["step_ms"] / rec["w8"]["step_ms"]
        rec["generate_plain_over_w8"] = rec["plain"]["generate_ms"] / rec["w8"]["generate_ms"]
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
