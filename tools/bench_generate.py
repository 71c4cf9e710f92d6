"""Greedy generation on the flagship language model (config 3: OPT-1.3B dims, 24 frozen + 4 gated layers, 64 neighbor tokens), bf16.

    python tools/bench_generate.py [--batches 2,16,64] [--prompt 512] [--new 32] [--reps 3] [--uncached] [--out FILE]

Default arm: MPTForCausalLM.generate -- one prefill, then the cached decode steps (csrc/decode.hip).  Reports per batch size the
prefill ms, ms per decode step, generated tokens per second, launches per step (C-ABI calls + aten ops of one step, each one launch)
and the bytes a step has to stream (weights + cached keys / values) over the step time as a fraction of 8 TB/s.

--uncached: generation without a cache, by a full decoder forward over the whole prefix for every new token, lm_head on the last
row and argmax.  It uses only what a checkout without generate() exposes (MPTDecoder.forward, the frozen lm_head linear), so the same
file runs there unchanged: that run is the baseline the cached path is compared with.

The model is built at the LM level with random weights and random neighbor tokens [B, 64, d]: the neighbor encoders run once per
generate() in either arm and are not part of the comparison.  Prompts are ragged (right-padded to --prompt columns).  One JSON line
per batch size goes to stdout (and to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS = dict(vocab_size=50272, hidden_size=2048, num_attention_heads=32, ffn_dim=8192, num_hidden_layers=24, max_position_embeddings=2048,
            word_embed_proj_dim=2048)
WISE, S_NEIGHBORS = 6, 64
HBM_PEAK = 8.0e12


def build(layers):
    from types import SimpleNamespace
    from transformers import OPTConfig
    from mmgl_amd.model.modelling_cross_attention import MPTConfig, MPTForCausalLM
    oc = OPTConfig(do_layer_norm_before=True, dropout=0.1, attention_dropout=0.0, pad_token_id=1, bos_token_id=2, eos_token_id=2,
                   **dict(DIMS, num_hidden_layers=layers))
    args = SimpleNamespace(neighbor_mode="embedding", peft_type="flamingo", neighbor_layer_wise=WISE, lora_r=64, lora_alpha=1, lora_dropout=0.0)
    torch.manual_seed(0)
    with torch.device("cuda"):
        lm = MPTForCausalLM(MPTConfig(args, oc))
    with torch.no_grad():
        for n_, p in lm.named_parameters():
            if n_.endswith(("gating1", "gating2")):
                p.fill_(0.5)
    return lm.bfloat16().eval()


def batch_of(B, width, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, DIMS["vocab_size"], (B, width), generator=g)
    am = torch.ones_like(ids)
    for b in range(1, B):
        am[b, int(torch.randint(64, width + 1, (1,), generator=g)):] = 0
    ids = torch.where(am.bool(), ids, torch.ones_like(ids))
    ne = torch.randn(B, S_NEIGHBORS, DIMS["hidden_size"], generator=g).bfloat16()
    nv = torch.rand(B, S_NEIGHBORS, generator=g) > 0.3
    nv[:, 0] = True
    return ids.cuda(), am.cuda(), ne.cuda(), nv.cuda()


def step_bytes(lm, B, keys):
    """Bytes one decode step has to read: every weight of the step's linears once, plus the cached keys and values."""
    d, ffn, V = DIMS["hidden_size"], DIMS["ffn_dim"], DIMS["vocab_size"]
    dec = lm.model.decoder
    w = len(dec.layers) * (4 * d * d + 2 * d * ffn) + len(dec.neighbor_layers) * (2 * d * d + 2 * d * ffn) + V * d
    kv = len(dec.layers) * B * keys * 2 * d + len(dec.neighbor_layers) * B * S_NEIGHBORS * 2 * d
    return 2.0 * w, 2.0 * kv


_NO_LAUNCH = {"view", "_unsafe_view", "reshape", "slice", "select", "as_strided", "unsqueeze", "squeeze", "detach", "alias", "empty", "empty_like",
              "empty_strided", "expand", "t", "transpose", "permute", "_local_scalar_dense"}       # aten ops that launch nothing


class _Launches:
    """C-ABI calls (each launches its kernels on the stream; one for everything a decode step uses) + aten ops, during a `with`."""

    def __enter__(self):
        from torch.utils._python_dispatch import TorchDispatchMode
        from mmgl_amd import _lib
        self.abi = self.aten = 0
        outer = self

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                name = str(getattr(func, "__name__", func)).split(".")[0]
                if name not in _NO_LAUNCH:
                    outer.aten += 1
                return func(*args, **(kwargs or {}))
        self._lib, self._call = _lib, _lib.call

        def call(name, work, *a):
            outer.abi += 1
            return outer._call(name, work, *a)
        _lib.call = call
        self.mode = Mode()
        self.mode.__enter__()
        return self

    def __exit__(self, *exc):
        self.mode.__exit__(*exc)
        self._lib.call = self._call


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def run_cached(lm, ids, am, ne, nv, n_new, reps):
    dec = lm.model.decoder
    T = ids.shape[1]

    def prefill():
        o = dec(input_ids=ids, attention_mask=am, neighbor_embeds=ne, neighbor_attention_mask=nv, use_cache=True, cache_capacity=T + n_new - 1)
        return o.past_key_values, lm._last_logits(o.last_hidden_state[:, -1]).argmax(-1)

    def step(tok, cache):
        return lm._last_logits(dec(input_ids=tok[:, None], past_key_values=cache).last_hidden_state[:, 0]).argmax(-1)

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
    once(count)                                        # warm-up: code objects, caches of derived weights; counts one step's launches
    runs = [once() for _ in range(reps)]
    _, t_gen = timed(lambda: lm.generate(ids, am, neighbor_embeds=ne, neighbor_attention_mask=nv, max_new_tokens=n_new))
    return dict(prefill_ms=statistics.median(r[0] for r in runs), step_ms=statistics.median(r[1] for r in runs),
                step_ms_all=[round(r[1], 4) for r in runs], generate_ms=t_gen, launches_per_step=count["abi"] + count["aten"],
                abi_calls_per_step=count["abi"], aten_ops_per_step=count["aten"])


def run_uncached(lm, ids, am, ne, nv, n_new, reps):
    from mmgl_amd.model.modelling_cross_attention import _lin
    dec = lm.model.decoder

    def once():
        cur, mask = ids, am
        with torch.no_grad():
            for s in range(n_new):
                h = dec(input_ids=cur, attention_mask=mask, neighbor_embeds=ne, neighbor_attention_mask=nv).last_hidden_state
                tok = _lin(lm.lm_head, h[:, -1:].contiguous())[:, 0].argmax(-1)
                cur = torch.cat([cur, tok[:, None]], dim=1)
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=DIMS["num_hidden_layers"])
    ap.add_argument("--uncached", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate needs the GPU: a timing taken anywhere else says nothing")
    lm = build(a.layers)
    lines = []
    for B in [int(b) for b in a.batches.split(",")]:
        ids, am, ne, nv = batch_of(B, a.prompt)
        rec = dict(arm="uncached" if a.uncached else "cached", model="opt-1.3b", layers=a.layers, dtype="bf16", batch=B, prompt=a.prompt,
                   new_tokens=a.new, device=torch.cuda.get_device_name(0))
        if a.uncached:
            rec.update(run_uncached(lm, ids, am, ne, nv, a.new, a.reps))
        else:
            rec.update(run_cached(lm, ids, am, ne, nv, a.new, a.reps))
            wb, kvb = step_bytes(lm, B, a.prompt + a.new // 2)
            rec.update(weight_bytes_per_step=wb, kv_bytes_per_step=kvb,
                       hbm_fraction=(wb + kvb) / (rec["step_ms"] * 1e-3) / HBM_PEAK)
        rec["tokens_per_s"] = B * a.new / (rec["generate_ms"] * 1e-3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
