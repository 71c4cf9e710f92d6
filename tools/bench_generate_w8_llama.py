"""LlamaNeighborLM.generate() with FP8 frozen weights (weight_dtype="fp8") against the model's dtype at config-5
dimensions (Llama-2-7B: hidden 4096, FFN 11008, 32 heads of 128, 8 frozen + 1 gated layer, 128 neighbor tokens), bf16, in one process.

    python tools/bench_generate_w8_llama.py [--batches 2,16,64] [--kv-heads 32,8] [--prompt 512] [--new 32] [--reps 3] [--out FILE]

Per (kv heads, batch size) the cached arm of tools/bench_generate_llama.py twice -- the decode steps on the bf16 weights and on their
e4m3fn codes, alternating rep by rep: ms per decode step (median of --reps runs of --new - 1 steps), launches per step (C-ABI calls +
aten ops), ms per generate() call (alternating too, median of --reps after a warm-up pass; the codes exist already, quantised once by
the warm-up), and the weight bytes a step streams in either arm.  The prefill is the same code in both arms.  The yardstick of the w8
arm is the plain arm of the same process; nothing is fixed in advance."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_generate import _Launches, timed        # noqa: E402
from bench_generate_llama import DIMS, batch_of, build        # noqa: E402


def one_run(lm, ids, am, ne, nv, n_new, w8, count=None):
    from mmgl_amd.model.decode_cache import StepCodes
    T = ids.shape[1]

    def prefill():
        hidden, cache = lm._hidden(ids, am, ne, nv, False, True, T + n_new - 1, None)
        cache.w8 = StepCodes() if w8 else None
        return cache, lm._last_logits(hidden[:, -1]).argmax(-1)

    def step(tok, cache):
        return lm._last_logits(lm._decode_step(tok[:, None], cache)).argmax(-1)

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


def weight_bytes(lm):
    """(bytes of the frozen layers' weights a step streams in the model's dtype, the same as codes and exponents)."""
    plain = w8 = 0
    for fr in lm._frozen:
        for w in (*fr._fused(), fr.layer.self_attn.o_proj.weight, fr.layer.mlp.down_proj.weight):
            plain += w.numel() * w.element_size()
            w8 += w.numel() + w.shape[0]
    return plain, w8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,16,64")
    ap.add_argument("--kv-heads", default="32,8")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate_w8_llama needs the GPU: a timing taken anywhere else says nothing")
    lines = []
    for kv_heads in [int(h) for h in a.kv_heads.split(",")]:
        lm = build(a.layers, kv_heads)
        for B in [int(b) for b in a.batches.split(",")]:
            ids, am, ne, nv = batch_of(B, a.prompt)
            arms = {"plain": False, "w8": True}
            counts = {name: {} for name in arms}
            for name, w8 in arms.items():                       # warm-up: code objects, the fused weight copies, the codes; counts one step
                one_run(lm, ids, am, ne, nv, a.new, w8, counts[name])
            runs = {name: [] for name in arms}
            for _ in range(a.reps):
                for name, w8 in arms.items():
                    runs[name].append(one_run(lm, ids, am, ne, nv, a.new, w8))
            plain_b, w8_b = weight_bytes(lm)
            rec = dict(model="llama-2-7b dims", layers=a.layers, gated_layers=len(lm.neighbor_layers), heads=DIMS["num_attention_heads"],
                       kv_heads=kv_heads, dtype="bf16", batch=B, prompt=a.prompt, new_tokens=a.new, device=torch.cuda.get_device_name(0),
                       command="python " + " ".join([os.path.relpath(sys.argv[0])] + sys.argv[1:]),
                       frozen_weight_bytes_per_step=dict(plain=plain_b, w8=w8_b))
            gen = {name: [] for name in arms}
            for _ in range(a.reps + 1):                         # generate() itself, alternating as well; the first pass warms it up
                for name, w8 in arms.items():
                    gen[name].append(timed(lambda: lm.generate(ids, am, neighbor_embeds=ne, neighbor_attention_mask=nv, max_new_tokens=a.new,
                                                               weight_dtype="fp8" if w8 else None))[1])
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
        del lm
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
