"""Beam search on the flagship language model (config 3: OPT-1.3B dims, 24 frozen + 4 gated layers, 64 neighbor tokens), bf16.

    python tools/bench_generate_beam.py [--arm beam|repeated] [--batches 2,16] [--beams 4] [--prompt 512] [--new 32] [--reps 3] [--out FILE]

--arm beam: MPTForCausalLM.generate(num_beams=W) -- one prefill of B rows, then per step lm_head, ops.beam_topk, ops.beam_advance and
the decode kernels at B*W rows on the beam-shared cache.
--arm repeated: the only way a checkout without num_beams runs W hypotheses per sample -- every prompt repeated W times through the
greedy cached path (tools/bench_generate.run_cached at B*W rows; no reordering of hypotheses, so it is a lower bound of that route).
This arm uses nothing newer than greedy generate(), so the same file runs in a checkout of the parent commit: that run is the baseline.
Per batch size one JSON line: prefill ms, ms per step, launches per step (C-ABI calls + aten ops, as tools/bench_generate.py counts
them) and the bytes of the key/value cache (prompt rows, beam tails, neighbor tokens)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_generate import DIMS, S_NEIGHBORS, _Launches, batch_of, build, run_cached, timed        # noqa: E402


def cache_bytes(lm, rows_prompt, rows_tail, rows_cross, T, n_cap):
    d = DIMS["hidden_size"]
    dec = lm.model.decoder
    return 2 * (len(dec.layers) * (rows_prompt * T + rows_tail * n_cap) * 2 * d + len(dec.neighbor_layers) * rows_cross * S_NEIGHBORS * 2 * d)


def run_beam(lm, ids, am, ne, nv, n_new, W, reps):
    from mmgl_amd import ops
    from mmgl_amd.model.modelling_cross_attention import BeamState
    dec = lm.model.decoder
    B, T = ids.shape
    V = DIMS["vocab_size"]
    start = torch.zeros(B, dtype=torch.float32, device="cuda")

    def select(hidden, cache, s):
        book = cache.beam.book
        cs, ci = ops.beam_topk(lm._last_logits(hidden), start if s == 0 else book.beam_score, W, rows_in=1 if s == 0 else W)
        ops.beam_advance(cs, ci, book, s, V, None, s == n_new - 1, False, float(s + 1))
        return book.tokens.view(B * W, 1)

    def prefill():
        o = dec(input_ids=ids, attention_mask=am, neighbor_embeds=ne, neighbor_attention_mask=nv, use_cache=True, cache_capacity=T)
        cache = o.past_key_values
        cache.beam = BeamState(cache, W, n_new - 1)
        return cache, select(o.last_hidden_state[:, -1], cache, 0)

    def step(tok, cache, s):
        return select(dec(input_ids=tok, past_key_values=cache).last_hidden_state[:, 0], cache, s)

    def once(count=None):
        with torch.no_grad():
            (cache, tok), t_pre = timed(prefill)

            def steps():
                t = tok
                for s in range(1, n_new):
                    if count is not None and s == 2:
                        with _Launches() as c:
                            t = step(t, cache, s)
                        count.update(abi=c.abi, aten=c.aten)
                    else:
                        t = step(t, cache, s)
                return t
            _, t_steps = timed(steps)
        return t_pre, t_steps / (n_new - 1)
    count = {}
    once(count)
    runs = [once() for _ in range(reps)]
    _, t_gen = timed(lambda: lm.generate(ids, am, neighbor_embeds=ne, neighbor_attention_mask=nv, max_new_tokens=n_new, num_beams=W))
    return dict(prefill_ms=statistics.median(r[0] for r in runs), step_ms=statistics.median(r[1] for r in runs),
                step_ms_all=[round(r[1], 4) for r in runs], generate_ms=t_gen, launches_per_step=count["abi"] + count["aten"],
                abi_calls_per_step=count["abi"], aten_ops_per_step=count["aten"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default="beam", choices=["beam", "repeated"])
    ap.add_argument("--batches", default="2,16")
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=DIMS["num_hidden_layers"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate_beam needs the GPU: a timing taken anywhere else says nothing")
    lm = build(a.layers)
    W, lines = a.beams, []
    for B in [int(b) for b in a.batches.split(",")]:
        ids, am, ne, nv = batch_of(B, a.prompt)
        rec = dict(arm=a.arm, model="opt-1.3b", layers=a.layers, dtype="bf16", batch=B, beams=W, rows=B * W, prompt=a.prompt, new_tokens=a.new,
                   device=torch.cuda.get_device_name(0))
        if a.arm == "beam":
            rec.update(run_beam(lm, ids, am, ne, nv, a.new, W, a.reps))
            rec["cache_bytes"] = cache_bytes(lm, B, B * W, B, a.prompt, a.new - 1)
        else:
            rep = lambda t: t.repeat_interleave(W, 0).contiguous()
            rec.update(run_cached(lm, rep(ids), rep(am), rep(ne), rep(nv), a.new, a.reps))
            rec["cache_bytes"] = cache_bytes(lm, B * W, 0, B * W, a.prompt + a.new - 1, 0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
