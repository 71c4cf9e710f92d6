"""LlamaNeighborLM.generate() with the FP8 key/value cache against the plain cache at config-5 dimensions (Llama-2-7B: hidden 4096, 32
heads of 128, 8 frozen + 1 gated layer, 128 neighbor tokens), bf16, in one process.

    python tools/bench_generate_q8_llama.py [--batches 2,16,64] [--kv-heads 32,8] [--prompt 512] [--new 32] [--reps 3] [--out FILE]

Per (kv heads, batch size) the cached arm of tools/bench_generate_llama.py twice -- kv_cache_dtype None and "fp8", alternating rep by
rep: prefill ms, ms per decode step, launches per step (C-ABI calls + aten ops), ms per generate() call, and the bytes of the
self-attention cache (codes plus exponents for the FP8 arm: (D + 1) / 2D of the plain bytes).  The yardstick of the FP8 arm is the
plain arm of the same process; nothing is fixed in advance."""
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


def one_run(lm, ids, am, ne, nv, n_new, kv, count=None):
    from mmgl_amd.model.sampling import check_kv_cache
    T = ids.shape[1]
    kv_dtype = check_kv_cache("bench", kv)

    def prefill():
        hidden, cache = lm._hidden(ids, am, ne, nv, False, True, T + n_new - 1, kv_dtype)
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
    nbytes = sum(t.numel() * t.element_size() for t in cache.kv + (cache.kv_scale or []))
    return t_pre, t_steps / (n_new - 1), nbytes


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
        raise SystemExit("bench_generate_q8_llama needs the GPU: a timing taken anywhere else says nothing")
    lines = []
    for kv_heads in [int(h) for h in a.kv_heads.split(",")]:
        lm = build(a.layers, kv_heads)
        for B in [int(b) for b in a.batches.split(",")]:
            ids, am, ne, nv = batch_of(B, a.prompt)
            arms = {"plain": None, "fp8": "fp8"}
            counts = {name: {} for name in arms}
            for name, kv in arms.items():                       # warm-up: code objects, the fused weight copies; counts one step's launches
                one_run(lm, ids, am, ne, nv, a.new, kv, counts[name])
            runs = {name: [] for name in arms}
            for _ in range(a.reps):
                for name, kv in arms.items():
                    runs[name].append(one_run(lm, ids, am, ne, nv, a.new, kv))
            rec = dict(model="llama-2-7b dims", layers=a.layers, gated_layers=len(lm.neighbor_layers), heads=DIMS["num_attention_heads"],
                       kv_heads=kv_heads, dtype="bf16", batch=B, prompt=a.prompt, new_tokens=a.new, device=torch.cuda.get_device_name(0))
            for name, kv in arms.items():
                _, t_gen = timed(lambda: lm.generate(ids, am, neighbor_embeds=ne, neighbor_attention_mask=nv, max_new_tokens=a.new,
                                                     kv_cache_dtype=kv))
                r, c = runs[name], counts[name]
                rec[name] = dict(prefill_ms=statistics.median(x[0] for x in r), step_ms=statistics.median(x[1] for x in r),
                                 step_ms_all=[round(x[1], 4) for x in r], generate_ms=t_gen, launches_per_step=c["abi"] + c["aten"],
                                 abi_calls_per_step=c["abi"], aten_ops_per_step=c["aten"], cache_bytes=r[0][2])
            rec["step_fp8_over_plain"] = rec["fp8"]["step_ms"] / rec["plain"]["step_ms"]
            rec["prefill_fp8_over_plain"] = rec["fp8"]["prefill_ms"] / rec["plain"]["prefill_ms"]
            rec["cache_bytes_fp8_over_plain"] = rec["fp8"]["cache_bytes"] / rec["plain"]["cache_bytes"]
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
