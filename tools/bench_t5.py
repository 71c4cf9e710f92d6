#!/usr/bin/env python
"""Training step of BASELINE config 1's model (T5-small dimensions: d_model 512, 8 heads of 64, d_ff 2048, 6 + 6 layers, vocabulary 32128;
512 input / 128 output tokens, random weights and tokens) under SelfAttentionModel: the native forward (model/t5_hip.py) against the
stock HuggingFace call (SelfAttentionModel.t5_native = False) on the same module, arms alternating inside one process.
    python tools/bench_t5.py [--batches 4 32] [--steps 8] [--rounds 3] [--optimizer adafactor adafactor_fused] [--out profiles/train_t5-small.json]
A step = forward + backward + Adafactor (DataParallelEngine(optimizer="adafactor"), as run_generation.py trains T5, or "adafactor_fused",
its --fused_adafactor); forward + backward is timed on its own as well.  An existing --out file keeps its rows: the new ones are appended.  Host clock around a device synchronise; the median of the rounds is reported, every round is kept."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(dtype):
    from transformers import T5Config
    from mmgl_amd.model import SelfAttentionModel
    cfg = T5Config(vocab_size=32128, d_model=512, d_kv=64, d_ff=2048, num_layers=6, num_decoder_layers=6, num_heads=8, dropout_rate=0.1,
                   decoder_start_token_id=0, pad_token_id=0)
    args = SimpleNamespace(context="section_only", neighbor_mode="raw", n_text_tokens=4, n_visual_tokens=4, text_model="", visual_model="",
                           max_output_length=128, freeze_lm=False, model_name_or_path="t5-small", peft_type="none", lora_r=0, lora_alpha=0,
                           lora_dropout=0.0, neighbor_layer_wise=1, decoder_only=False, position_type="none", max_text_neighbors=0,
                           max_image_neighbors=0)
    torch.manual_seed(0)
    return SelfAttentionModel(args, None, lm_config=cfg).to(dtype).cuda().train()


def run(B, dtype, steps, rounds, optimizer="adafactor"):
    from mmgl_amd.distributed import DataParallelEngine
    from mmgl_amd.model.t5_hip import T5HipRunner
    model = build(dtype)
    eng = DataParallelEngine(model, lr=1e-4, optimizer=optimizer, master_weights=False)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, 32128, (B, 512), generator=g).cuda()
    mask = torch.ones_like(ids)
    mask[B // 2:, 400:] = 0                                   # half of the samples right-padded
    labels = torch.randint(1, 32128, (B, 128), generator=g).cuda()
    labels[B // 2:, 100:] = -100

    def fb():
        eng.zero_grad()
        loss = model(ids, mask, labels).loss
        loss.backward()
        eng.finish_backward()
        return loss

    def timed(native, with_opt):
        model.t5_native = native
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fb()
            if with_opt:
                eng.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    before = T5HipRunner.calls
    for native in (True, False):                              # warm up both arms: code objects, library algorithm choices
        for _ in range(2):
            timed(native, True)
    assert T5HipRunner.calls == before + 2 * steps, "the native arm did not run the native forward"
    rec = {"native_fwd_bwd_ms": [], "stock_fwd_bwd_ms": [], "native_step_ms": [], "stock_step_ms": []}
    for _ in range(rounds):
        rec["native_fwd_bwd_ms"].append(timed(True, False))
        rec["stock_fwd_bwd_ms"].append(timed(False, False))
        rec["native_step_ms"].append(timed(True, True))
        rec["stock_step_ms"].append(timed(False, True))
    med = {k: sorted(v)[len(v) // 2] for k, v in rec.items()}
    out = dict(batch=B, dtype=str(dtype)[6:], optimizer=optimizer, steps_per_timing=steps, rounds=rec, median=med,
               speedup_fwd_bwd=med["stock_fwd_bwd_ms"] / med["native_fwd_bwd_ms"], speedup_step=med["stock_step_ms"] / med["native_step_ms"],
               native_samples_per_s=B / med["native_step_ms"] * 1e3, stock_samples_per_s=B / med["stock_step_ms"] * 1e3)
    print(json.dumps({k: v for k, v in out.items() if k != "rounds"}), flush=True)
    del eng, model
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="*", type=int, default=[4, 32])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--optimizer", nargs="*", default=["adafactor"], choices=["adafactor", "adafactor_fused"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_t5 needs a GPU"
    results = [run(B, dtype, a.steps, a.rounds, opt) for dtype in (torch.bfloat16, torch.float32) for B in a.batches for opt in a.optimizer]
    command = (f"python tools/bench_t5.py --batches {' '.join(map(str, a.batches))} --steps {a.steps} --rounds {a.rounds}"
               + ("" if a.optimizer == ["adafactor"] else f" --optimizer {' '.join(a.optimizer)}"))
    doc = dict(command=command, model="T5-small dimensions (random weights), 512 input / 128 output tokens, dropout 0.1, Adafactor", results=results)
    if a.out and os.path.exists(a.out):                       # keep the rows of earlier runs (they carry no `optimizer`: the stock kind)
        with open(a.out) as f:
            old = json.load(f)
        doc = dict(old, results=old["results"] + results, later_commands=old.get("later_commands", []) + [command])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
