"""Greedy generation on the Llama-family neighbor LM at config-5 dimensions (Llama-2-7B: hidden 4096, 32 heads of 128, intermediate 11008,
vocab 32000, one gated layer per 8 frozen ones, 128 neighbor tokens), bf16: cached against uncached, in one process.

    python tools/bench_generate_llama.py [--batches 2,16,64] [--prompt 512] [--new 32] [--layers 8] [--kv-heads 32] [--reps 3] [--out FILE]

cached:   LlamaNeighborLM.generate -- one prefill, then the decode steps on csrc/decode.hip (skinny GEMMs, mmgl_rope_kv_append,
          mmgl_attn_decode_gqa_fwd where --kv-heads < 32).  Reports the prefill ms, ms per decode step, launches per step (C-ABI calls +
          aten ops of one step, each one launch) and the bytes the cache holds per token (2 * layers * Hkv * D * 2 B: what GQA saves).
uncached: the only route there is without the cache -- forward()'s layers over the whole prefix for every new token, lm_head on its
          last row only, argmax.
--layers defaults to 8 frozen layers (+ 1 gated) so that the random initialisation stays short; a step's time scales with the layer
count, the per-layer figures do not change.  --kv-heads 32 is config 5 itself (multi-head); 8 is the grouped-query shape of the
Llama-3 family at the same width.  Prompts are ragged (right-padded to --prompt columns).  One JSON line per batch size goes to stdout
(and to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_generate import _Launches, timed        # noqa: E402

DIMS = dict(vocab_size=32000, hidden_size=4096, intermediate_size=11008, num_attention_heads=32, max_position_embeddings=4096)
WISE, S_NEIGHBORS = 8, 128


def build(layers, kv_heads):
    from types import SimpleNamespace
    from transformers import LlamaConfig
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    cfg = LlamaConfig(pad_token_id=0, bos_token_id=1, eos_token_id=2, attention_dropout=0.0, num_hidden_layers=layers,
                      num_key_value_heads=kv_heads, **DIMS)
    torch.manual_seed(0)
    with torch.device("cuda"), torch.no_grad():
        lm = LlamaNeighborLM(SimpleNamespace(model_name_or_path="llama-2-7b", neighbor_layer_wise=WISE), cfg)
        for layer in lm.neighbor_layers:
            layer.gating1.fill_(0.5)
            layer.gating2.fill_(0.5)
    return lm.bfloat16().eval()


def batch_of(B, width, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, DIMS["vocab_size"], (B, width), generator=g)
    am = torch.ones_like(ids)
    for b in range(1, B):
        am[b, int(torch.randint(min(64, width), width + 1, (1,), generator=g)):] = 0
    ids = torch.where(am.bool(), ids, torch.zeros_like(ids))
    ne = torch.randn(B, S_NEIGHBORS, DIMS["hidden_size"], generator=g).bfloat16()
    nv = torch.rand(B, S_NEIGHBORS, generator=g) > 0.3
    nv[:, 0] = True
    return ids.cuda(), am.cuda(), ne.cuda(), nv.cuda()


def run_cached(lm, ids, am, ne, nv, n_new, reps):
    T = ids.shape[1]

    def prefill():
        hidden, cache = lm._hidden(ids, am, ne, nv, False, True, T + n_new - 1)
        return cache, lm._last_logits(hidden[:, -1]).argmax(-1)

    def step(tok, cache):
        return lm._last_logits(lm._decode_step(tok[:, None], cache)).argmax(-1)

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
        return t_pre, t_steps / (n_new - 1)
    count = {}
    once(count)                                        # warm-up: code objects, the fused weight copies; counts one step's launches
    runs = [once() for _ in range(reps)]
    _, t_gen = timed(lambda: lm.generate(ids, am, neighbor_embeds=ne, neighbor_attention_mask=nv, max_new_tokens=n_new))
    return dict(prefill_ms=statistics.median(r[0] for r in runs), step_ms=statistics.median(r[1] for r in runs),
                step_ms_all=[round(r[1], 4) for r in runs], generate_ms=t_gen, launches_per_step=count["abi"] + count["aten"],
                abi_calls_per_step=count["abi"], aten_ops_per_step=count["aten"])


def run_uncached(lm, ids, am, ne, nv, n_new, reps):
    def once():
        cur, mask = ids, am
        with torch.no_grad():
            for s in range(n_new):
                hidden, _ = lm._hidden(cur, mask, ne, nv)                    # forward() without its [B, T, V] head
                cur = torch.cat([cur, lm._last_logits(hidden[:, -1]).argmax(-1)[:, None]], dim=1)
                mask = torch.cat([mask, torch.ones_like(mask[:, :1])], dim=1)
        return cur
    once()
    times = [timed(once)[1] for _ in range(reps)]
    return dict(generate_ms=statistics.median(times), generate_ms_all=[round(t, 2) for t in times])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,16,64")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--kv-heads", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate_llama needs the GPU: a timing taken anywhere else says nothing")
    lm = build(a.layers, a.kv_heads)
    D = DIMS["hidden_size"] // DIMS["num_attention_heads"]
    lines = []
    for B in [int(b) for b in a.batches.split(",")]:
        ids, am, ne, nv = batch_of(B, a.prompt)
        rec = dict(model="llama-2-7b dims", layers=a.layers, gated_layers=len(lm.neighbor_layers), heads=DIMS["num_attention_heads"],
                   kv_heads=a.kv_heads, dtype="bf16", batch=B, prompt=a.prompt, new_tokens=a.new, device=torch.cuda.get_device_name(0),
                   cache_bytes_per_token=2 * a.layers * a.kv_heads * D * 2,
                   cache_bytes_per_token_multi_head=2 * a.layers * DIMS["num_attention_heads"] * D * 2)
        cached = run_cached(lm, ids, am, ne, nv, a.new, a.reps)
        uncached = run_uncached(lm, ids, am, ne, nv, a.new, max(1, a.reps - 1))
        rec.update(cached=cached, uncached=uncached, speedup_generate_ms=round(uncached["generate_ms"] / cached["generate_ms"], 2),
                   tokens_per_s=B * a.new / (cached["generate_ms"] * 1e-3))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
