#!/usr/bin/env python
"""Micro-benchmark of the T5 attention kernels (csrc/relbias.hip, raw C-ABI launches) against the aten chain HuggingFace runs
(compute_bias gather, matmul, add, softmax, matmul; backward by autograd), forward and backward, HIP events, arms alternating.
    python tools/bench_attn_relbias.py [--batches 4 32] [--iters 30] [--rounds 3] [--out profiles/attn_relbias.txt]
Shapes: T5-small's three (H = 8, D = 64): encoder 512 x 512 and 576 x 576, decoder 128 x 128 causal, cross 128 x 576 (no table)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmgl_amd import _lib, ops  # noqa: E402
from mmgl_amd._lib import ptr, stream_ptr  # noqa: E402

H, D, NB = 8, 64, 32
SHAPES = [("encoder", 512, 512, False, True), ("encoder", 576, 576, False, True), ("decoder", 128, 128, True, True),
          ("cross", 128, 576, False, False)]


def _timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3           # us


def run(B, kind, T, S, causal, has_table, dtype, iters, rounds):
    L = _lib.lib()
    d = H * D
    q = (torch.randn(B, T, d, device="cuda") * D ** -0.5).to(dtype)
    k, v = torch.randn(B, S, d, device="cuda").to(dtype), torch.randn(B, S, d, device="cuda").to(dtype)
    w = torch.randn(B, T, d, device="cuda").to(dtype)
    table = torch.randn(NB, H, device="cuda") if has_table else None
    bucket_of = ops.t5_bucket_table(T, S, not causal, NB, 128, "cuda") if has_table else None
    out, lse = torch.empty_like(q), torch.empty(B, H, T, dtype=torch.float32, device="cuda")
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    dtab = torch.empty(NB, H, device="cuda") if has_table else None
    nws = L.mmgl_attn_relbias_bwd_workspace(B, H, T, S)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    code, st = _lib.dtype_code(q), stream_ptr()
    fwd = lambda: L.mmgl_attn_relbias_fwd(ptr(q), ptr(k), ptr(v), None, ptr(table), ptr(bucket_of), ptr(out), ptr(lse), B, H, T, S, D,
                                          NB if has_table else 0, d, d, int(causal), 0.0, 0, code, st)
    bwd = lambda: L.mmgl_attn_relbias_bwd(ptr(w), ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse), None, ptr(table), ptr(bucket_of), ptr(dq),
                                          ptr(dk), ptr(dv), ptr(dtab), ptr(ws), nws, B, H, T, S, D, NB if has_table else 0, d, d,
                                          int(causal), 0.0, 0, code, st)

    # the aten chain: what T5Attention's eager path launches for the same call
    qa, ka, va = (t.view(B, -1, H, D).transpose(1, 2).detach().requires_grad_() for t in (q, k, v))
    ta = table.detach().to(dtype).requires_grad_() if has_table else None
    idx = (torch.arange(S, device="cuda")[None, :] - torch.arange(T, device="cuda")[:, None] + T - 1)
    bkt = bucket_of.long()[idx] if has_table else None
    cmask = torch.zeros(T, S, device="cuda", dtype=dtype)
    if causal:
        cmask.masked_fill_(torch.triu(torch.ones(T, S, device="cuda", dtype=torch.bool), 1), torch.finfo(dtype).min)
    wa = w.view(B, T, H, D).transpose(1, 2)

    def aten_fwd():
        s = torch.matmul(qa, ka.transpose(2, 3))
        if has_table:
            s = s + torch.nn.functional.embedding(bkt, ta).permute(2, 0, 1).unsqueeze(0)       # compute_bias: an nn.Embedding lookup
        s = s + cmask
        p = torch.nn.functional.softmax(s.float(), dim=-1).type_as(s)
        return torch.matmul(p, va)

    def aten_fwd_only():
        with torch.no_grad():
            aten_fwd()

    def aten_both():
        o = aten_fwd()
        torch.autograd.grad(o, [qa, ka, va] + ([ta] if has_table else []), wa)

    for _ in range(3):
        assert fwd() == 0 and bwd() == 0
        aten_both()
    torch.cuda.synchronize()
    res = dict(hf=[], hb=[], af=[], ab=[])
    for _ in range(rounds):                       # arms alternate: the pool's boxes and clocks drift between calls, not inside one
        res["hf"].append(_timed(fwd, iters))
        res["af"].append(_timed(aten_fwd_only, iters))
        res["hb"].append(_timed(bwd, iters))
        both = _timed(aten_both, iters)
        res["ab"].append(both - res["af"][-1])    # autograd needs its own forward: backward = (forward + backward) - forward
    med = {n: sorted(x)[len(x) // 2] for n, x in res.items()}
    fl = 4.0 * B * T * S * d * (0.5 if causal else 1.0)
    return (f"{kind:8s} B={B:3d} T={T:4d} S={S:4d} {str(dtype)[6:]:9s} fwd hip {med['hf']:8.1f} us ({fl / med['hf'] / 1e6:6.1f} TF) aten {med['af']:8.1f} us "
            f"x{med['af'] / med['hf']:5.2f} | bwd hip {med['hb']:8.1f} us ({2.5 * fl / med['hb'] / 1e6:6.1f} TF) aten {med['ab']:8.1f} us x{med['ab'] / med['hb']:5.2f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="*", type=int, default=[4, 32])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_attn_relbias needs a GPU"
    torch.manual_seed(0)
    lines = [f"# tools/bench_attn_relbias.py --batches {' '.join(map(str, a.batches))} --iters {a.iters} --rounds {a.rounds}: median of "
             f"{a.rounds} alternating rounds, HIP events, H = {H}, D = {D}; x = aten time / hip time (below 1: the HIP kernel is slower)"]
    for dtype in (torch.bfloat16, torch.float32):
        for B in a.batches:
            for shape in SHAPES:
                lines.append(run(B, *shape, dtype, a.iters, a.rounds))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
