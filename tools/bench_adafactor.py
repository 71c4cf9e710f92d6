#!/usr/bin/env python
"""The optimizer call alone: DataParallelEngine.step() of the fused Adafactor kind (mmgl_adafactor_step, four launches over the flat buffers)
against the stock kind (transformers.optimization.Adafactor, a Python loop over the tensors), on the trainable sets of T5-small and
T5-base dimensions (random weights, nothing downloaded), bf16 and fp32.
    python tools/bench_adafactor.py [--calls 20] [--rounds 5] [--out profiles/adafactor_step.txt]
Both engines live in one process over their own copy of the model and the same random gradient; the arms alternate, every arm is warmed
up, a timing is `calls` steps between two device events (the stock arm's host loop is part of its call: the events bracket the enqueue
and the execution), and the median of the rounds is reported with the spread.  The bytes a step must move (gradient read twice for a 2-D
tensor, parameter read and written once) over the fused time give its achieved bandwidth; that is an algorithmic figure, not a trace."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODELS = {"t5-small": dict(d_model=512, d_kv=64, d_ff=2048, num_layers=6, num_decoder_layers=6, num_heads=8),
          "t5-base": dict(d_model=768, d_kv=64, d_ff=3072, num_layers=12, num_decoder_layers=12, num_heads=12)}


def engines(name, dtype):
    from transformers import T5Config, T5ForConditionalGeneration
    from mmgl_amd.distributed import DataParallelEngine
    out = {}
    for kind in ("adafactor_fused", "adafactor"):
        torch.manual_seed(0)
        model = T5ForConditionalGeneration(T5Config(vocab_size=32128, decoder_start_token_id=0, pad_token_id=0, **MODELS[name])).to(dtype).cuda()
        out[kind] = DataParallelEngine(model, lr=1e-4, optimizer=kind, master_weights=False)
    g = torch.randn(out["adafactor"].numel, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 1e-2
    for e in out.values():
        e.flat_grad.copy_(g.to(dtype))
    return out


def timed(eng, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(calls):
        eng.step()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / calls


def run(name, dtype, calls, rounds):
    engs = engines(name, dtype)
    fused = engs["adafactor_fused"]
    for e in engs.values():                                   # warm up: code objects, the stock optimizer's state
        timed(e, 3)
    rec = {k: [] for k in engs}
    for _ in range(rounds):
        for k, e in engs.items():
            rec[k].append(timed(e, calls))
    med = {k: sorted(v)[len(v) // 2] for k, v in rec.items()}
    esz = fused.flat_param.element_size()
    two_d = sum(p.numel() for p in fused.params if p.dim() == 2)
    one_d = sum(p.numel() for p in fused.params if p.dim() == 1)
    nbytes = two_d * (3 * esz + 2 * esz) + one_d * (2 * esz + 2 * esz + 8)       # gradient three (2-D) / two (1-D) times, parameter in and out, v in and out
    line = (f"{name:9s} {str(dtype)[6:]:9s} tensors {len(fused.params):4d}  elements {fused.numel / 1e6:7.2f} M  "
            f"fused {med['adafactor_fused'] * 1e3:8.1f} us (min {min(rec['adafactor_fused']) * 1e3:.1f}, max {max(rec['adafactor_fused']) * 1e3:.1f})  "
            f"stock {med['adafactor'] * 1e3:9.1f} us (min {min(rec['adafactor']) * 1e3:.1f}, max {max(rec['adafactor']) * 1e3:.1f})  "
            f"stock / fused {med['adafactor'] / med['adafactor_fused']:6.1f}x  fused {nbytes / med['adafactor_fused'] / 1e6:7.1f} GB/s algorithmic  "
            f"state {fused.adafactor_state.numel() * 4 / 1e6:.2f} MB  workspace {fused.adafactor_table.workspace_bytes / 1e6:.2f} MB  "
            f"launches 4  tiles {fused.adafactor_table.n_tiles}")
    print(line, flush=True)
    del engs
    torch.cuda.empty_cache()
    return line


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="*", default=list(MODELS))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_adafactor needs a GPU"
    head = (f"# python tools/bench_adafactor.py --calls {a.calls} --rounds {a.rounds}: DataParallelEngine.step() alone, fused against stock Adafactor, "
            f"arms alternating in one process, {a.calls} calls between device events, median of {a.rounds} rounds; {torch.cuda.get_device_name(0)}")
    lines = [head] + [run(m, dt, a.calls, a.rounds) for m in a.models for dt in (torch.bfloat16, torch.float32)]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
