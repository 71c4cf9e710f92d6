"""Greedy generation on the LoRA language model of config 4 (OPT-1.3B dims, 24 layers, LoRA r = 16 on q_proj / v_proj), bf16.

    python tools/bench_generate_lora.py [--batches 2,16,64] [--prompt 512] [--new 32] [--reps 3] [--layers 24] [--out FILE]

Three arms per batch size, in one process on the same prompts:
    lora_cached    MPTForCausalLM.generate on the adapted fork: one prefill, then decode steps whose q / v projections run
                   ops.decode_lora_linear (mmgl_gemm_skinny_lora)
    lora_uncached  the same model without a cache: a full decoder forward over the whole prefix for every new token, lm_head on the last
                   row, argmax -- what a checkout without this generate() can do
    plain_cached   the fork without adapters at the same dimensions: its cached step against lora_cached's is the cost of the adapter
Reports prefill ms, ms per decode step, the whole generate() in ms and generated tokens per second; launches per step as
tools/bench_generate.py counts them.  Models are built at the LM level with random weights; lora_B ~ N(0, 0.02^2).  One JSON line per
(batch, arm) goes to stdout (and to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_generate import DIMS, _Launches, batch_of, timed        # noqa: E402

LORA_R, LORA_ALPHA = 16, 32.0


def build(layers, lora):
    from types import SimpleNamespace
    from transformers import OPTConfig
    from mmgl_amd.model.modelling_cross_attention import MPTConfig, MPTForCausalLM
    from mmgl_amd.model.modelling_self_attention import LoRALinear, inject_lora
    oc = OPTConfig(do_layer_norm_before=True, dropout=0.1, attention_dropout=0.0, pad_token_id=1, bos_token_id=2, eos_token_id=2,
                   **dict(DIMS, num_hidden_layers=layers))
    args = SimpleNamespace(neighbor_mode="raw", peft_type="none", neighbor_layer_wise=layers + 1)
    torch.manual_seed(0)
    with torch.device("cuda"):
        lm = MPTForCausalLM(MPTConfig(args, oc))
        if lora:
            inject_lora(lm, LORA_R, LORA_ALPHA, 0.0)
    with torch.no_grad():
        for m in lm.modules():
            if isinstance(m, LoRALinear):
                m.lora_B.normal_(std=0.02)
    return lm.bfloat16().eval()


def run_cached(lm, ids, am, n_new, reps):
    dec = lm.model.decoder
    T = ids.shape[1]

    def prefill():
        o = dec(input_ids=ids, attention_mask=am, use_cache=True, cache_capacity=T + n_new - 1)
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
    once(count)                                        # warm-up; counts one step's launches
    runs = [once() for _ in range(reps)]
    gen = [timed(lambda: lm.generate(ids, am, max_new_tokens=n_new))[1] for _ in range(reps)]
    return dict(prefill_ms=statistics.median(r[0] for r in runs), step_ms=statistics.median(r[1] for r in runs),
                step_ms_all=[round(r[1], 4) for r in runs], generate_ms=statistics.median(gen), generate_ms_all=[round(t, 2) for t in gen],
                launches_per_step=count["abi"] + count["aten"], abi_calls_per_step=count["abi"], aten_ops_per_step=count["aten"])


def run_uncached(lm, ids, am, n_new, reps):
    from mmgl_amd.model.modelling_cross_attention import _lin
    dec = lm.model.decoder

    def once():
        cur, mask = ids, am
        with torch.no_grad():
            for s in range(n_new):
                h = dec(input_ids=cur, attention_mask=mask).last_hidden_state
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate_lora needs the GPU: a timing taken anywhere else says nothing")
    lora, plain = build(a.layers, True), build(a.layers, False)
    lines = []
    for B in [int(b) for b in a.batches.split(",")]:
        ids, am, _, _ = batch_of(B, a.prompt)
        for arm, fn in (("lora_cached", lambda: run_cached(lora, ids, am, a.new, a.reps)),
                        ("plain_cached", lambda: run_cached(plain, ids, am, a.new, a.reps)),
                        ("lora_uncached", lambda: run_uncached(lora, ids, am, a.new, a.reps))):
            rec = dict(arm=arm, model="opt-1.3b-lora", lora_r=LORA_R, layers=a.layers, dtype="bf16", batch=B, prompt=a.prompt, new_tokens=a.new,
                       device=torch.cuda.get_device_name(0))
            rec.update(fn())
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
