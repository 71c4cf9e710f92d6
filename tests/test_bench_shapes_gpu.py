"""-m gpu parity tests at the shapes the bench runs: the cross-attention core and every trainable linear of one gated cross-attention
block (plus the neighbor projections), for the configs and per-GPU batches of bench.py (the headline step, `batch_sweep` and the
trainer protocols), against an independent float64 reference computed from the same bf16-rounded inputs.

Several kernel plans depend on the batch (bwd_plan's chunk count for the cross-attention backward, gemm8p_tt_splits's K-split count
for the weight gradient), so hand-picked small-batch shapes leave the branches of the measured step unchecked.  The shape table is
derived from bench.CONFIGS, and test_census_matches_model checks it against what the model really launches.

Measures: per-(sample, head) max-norm error of the attention outputs and gradients (helpers.slice_err), element-wise error of every
linear output / gradient (helpers.elementwise_err, floor 1e-2 of the tensor's maximum as in test_model_gpu.py) and the per-256 x 256
tile error of every weight gradient (helpers.tile_err).  A defect that scales one chunk, trip, head or K split by a few percent fails
them; a whole-tensor max|a - b| / max|b| <= 2e-2 does not."""
from dataclasses import dataclass

import pytest
import torch

import bench
from helpers import elementwise_err, slice_err, tile_err

pytestmark = pytest.mark.gpu

# per-GPU batches: bench's headline (64 / 8) and batch_sweep (4 / 16 / 32), the trainer protocols' micro-batches (2 / 4)
BATCHES = {"opt-125m": (2, 4, 16, 32, 64), "opt-1.3b": (2, 4, 16, 32, 64), "llama-2-7b": (4, 8)}

# Plans, by reading the planners (csrc/xattn.hip bwd_plan; csrc/gemm8p_tt.hip gemm8p_tt_splits with 256 CUs), not from a run.
# Cross-attention backward (bf16):
#   opt-125m   H 12, D 64, S 16  -> xattn_bwd_fused_kernel<64, 1>, units = 12 B
#              B 2 / 4 / 16: 10 chunks of 64 rows (1 trip); B 32: 5 chunks of 128 (2 trips); B 64: 3 chunks of 224 (3.5 trips)
#   opt-1.3b   H 32, D 64, S 64  -> xattn_bwd_fused_kernel<64, 4>, units = 64 B
#              B 2: 10 chunks (1 trip); B 4: 7 chunks of 96 (1.5 trips); B 16: 2 chunks of 320 (5 trips);
#              B 32 / 64: ONE chunk of 640 rows (10 trips), dK / dV stored directly in bf16 (the `nchunk == 1` branch)
#   llama-2-7b H 32, D 128, S 128 -> xattn_bwd_fusedw_kernel<128, 8>, units = 32 B
#              B 4: 4 chunks of 544 (8.5 trips); B 8: ONE chunk of 2176 rows (34 trips), dK / dV stored directly
# Weight gradient (contraction over the M rows; "tx" = M no multiple of 128 or too few tiles: the 128 x 128 gemm_tx kernel):
#   opt-125m   q / out_proj 768 x 768:     B 2 / 4 tx, B 16: 10 splits, B 32: 16, B 64: 20
#              fc1 / fc2 768 x 3072:       B 2 tx, B 4: 4 splits, B 16 / 32 / 64: 5 splits
#              k / v_proj, pooler, projections: tx
#   opt-1.3b   q / out_proj 2048 x 2048:   B 2 / 4: unsplit, B 16 / 32 / 64: 4 splits
#              k / v_proj 2048 x 2048:     B 2 tx, B 4 / 16 / 32: unsplit, B 64: 2 splits
#              fc1 / fc2 2048 x 8192:      unsplit (256 tiles) at every B
#              pooler, projections: tx
#   llama-2-7b q / k / v / o_proj, gate|up 4096 x 22016, down 11008 x 4096: unsplit at B 4 and 8; pooler, projections: tx


def core_shape(name, B):
    """(B, H, T, S, D) of the cross-attention core of config `name` at batch B: T = prompt + summary, S = 4 tokens per neighbor."""
    cfg = bench.CONFIGS[name]
    d, H = cfg["lm"]["hidden_size"], cfg["lm"]["num_attention_heads"]
    n_tok = bench.make_args(cfg).n_text_tokens
    return B, H, cfg["lin"] + cfg["lout"], n_tok * (cfg["nt"] + cfg["ni"]), d // H


@dataclass(frozen=True)
class Lin:
    """One trainable linear as the model calls ops.linear.  kind: "plain", "relu_pair" (ops.relu_ffn's trainable route: fc1 with the ReLU
    epilogue feeding fc2, whose dgrad carries fc1's ReLU backward, MPTDecoderLayer._ffn) or "swiglu" (Llama: fused gate|up, ops.swiglu, down_proj)."""
    label: str
    M: int
    K: int                 # in features
    N: int                 # out features (relu_pair / swiglu: the ffn width F)
    bias: bool = True
    out_scale: float = 1.0
    need_dx: bool = True   # the input carries a gradient (the neighbor encoders' outputs do not)
    kind: str = "plain"


def linears(name, B):
    """Every trainable linear of one gated cross-attention block of config `name` at batch B, and the trainable neighbor-side ones
    (text pooler dense, text / visual embeddings: M = B * nt and B * ni rows)."""
    cfg = bench.CONFIGS[name]
    lm = cfg["lm"]
    d, H = lm["hidden_size"], lm["num_attention_heads"]
    _, _, T, S, D = core_shape(name, B)
    enc = bench.hf_configs(cfg)[1].hidden_size
    n_tok = bench.make_args(cfg).n_text_tokens
    llama = cfg["kind"] == "llama"
    bias = not llama
    rows = [Lin("q_proj", B * T, d, d, bias, out_scale=D ** -0.5),
            Lin("k_proj", B * S, d, d, bias),
            Lin("v_proj", B * S, d, d, bias),
            Lin("out_proj", B * T, d, d, bias)]
    if llama:
        rows.append(Lin("gate_up/down", B * T, d, lm["intermediate_size"], False, kind="swiglu"))
    else:
        rows.append(Lin("fc1/fc2", B * T, d, lm["ffn_dim"], True, kind="relu_pair"))
    rows += [Lin("text_pooler", B * cfg["nt"], enc, enc, need_dx=False),
             Lin("text_embeddings", B * cfg["nt"], enc, n_tok * d),
             Lin("visual_embeddings", B * cfg["ni"], enc, n_tok * d, need_dx=False)]
    return rows


CORE_CASES = [(n, B) for n, bs in BATCHES.items() for B in bs]
LINEAR_CASES = [(n, B, r) for n, B in CORE_CASES for r in linears(n, B)]

# Bounds: about 2x the largest value measured over the whole table on the unmodified library (MI355X), within the 3x allowed and
# below the 2e-2 of the older tests.  Measured maxima in the comments.
TOL_XATTN = {"out": 8e-3,       # measured 3.92e-3 (opt-125m B 32)        per-(sample, head) max|d| / max|ref|
             "dq": 1.2e-2,      # measured 6.00e-3 (opt-1.3b B 16)
             "dk": 1.1e-2,      # measured 5.33e-3 (opt-1.3b B 64)
             "dv": 1.0e-2}      # measured 5.11e-3 (opt-1.3b B 64)
TOL_LIN_EL = 8e-3               # measured 3.84e-3 over 400 outputs / gradients: element-wise, floor 1e-2 of the tensor's maximum
TOL_LIN_TILE = 8e-3             # measured 3.89e-3 over 108 weight gradients: per-256 x 256-tile max-norm


# ------------------------------------------------------------------------------------------------ float64 references (no mmgl_amd)
def xattn_ref(q, k, v, valid, H, dout):
    """out, dq, dk, dv of softmax(max(q k^T + M, finfo.min)) v per head in float64, M = finfo.min on masked keys (the reference's
    semantics: a sample with no valid key attends uniformly over all S keys, and autograd's 50 / 50 split at the torch.maximum tie
    halves dScores on masked entries)."""
    B, T, d = q.shape
    S = k.shape[1]
    D = d // H
    qh, kh, vh = (t.double().reshape(B, -1, H, D).transpose(1, 2) for t in (q, k, v))
    gh = dout.double().reshape(B, T, H, D).transpose(1, 2)
    masked = ~valid.bool()[:, None, None, :]
    s = (qh @ kh.transpose(-1, -2)).masked_fill(masked, torch.finfo(torch.float64).min)
    p = torch.softmax(s, dim=-1)
    dp = gh @ vh.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    ds = torch.where(masked, 0.5 * ds, ds)
    merge = lambda t: t.transpose(1, 2).reshape(B, -1, d)
    return merge(p @ vh), merge(ds @ kh), merge(ds.transpose(-1, -2) @ qh), merge(p.transpose(-1, -2) @ gh)


MASK_KINDS = ("random", "last_only", "none_valid", "group_masked", "all_valid")


def key_masks(B, S, gen):
    """[B, S] bool: sample b gets MASK_KINDS[b % 5] (B = 2: random, last key only; B = 4 adds a fully masked sample and a masked
    32-key group; B >= 5 all five).  The group is keys 32 .. 63 (S = 16: keys 0 .. 7, the first half of the only group)."""
    valid = torch.rand(B, S, generator=gen, device="cuda") > 0.35
    for b in range(B):
        kind = MASK_KINDS[b % len(MASK_KINDS)]
        if kind == "random":
            valid[b, 0] = valid[b, 0] | ~valid[b].any()
        elif kind == "last_only":
            valid[b] = False
            valid[b, S - 1] = True
        elif kind == "none_valid":
            valid[b] = False
        elif kind == "group_masked":
            valid[b] = True
            if S > 32:
                valid[b, 32:64] = False
            else:
                valid[b, :S // 2] = False
        else:
            valid[b] = True
    return valid


def test_reference_matches_oracle_attention_core():
    """xattn_ref against oracle.lm_ref.attention_core (autograd through the reference's own formulation) at a small shape with every
    mask kind, a fully masked sample included."""
    from oracle import lm_ref
    B, H, T, S, D = 5, 3, 20, 40, 16
    gen = torch.Generator(device="cuda").manual_seed(5)
    q, k, v, w = (torch.randn(B, n, H * D, generator=gen, device="cuda", dtype=torch.float64) for n in (T, S, S, T))
    valid = key_masks(B, S, gen)
    qc, kc, vc = (t.cpu().requires_grad_() for t in (q, k, v))
    out = lm_ref.attention_core(qc, kc, vc, lm_ref.expand_mask(valid.cpu(), torch.float64, T), H)
    out.backward(w.cpu())
    for a, r in zip(xattn_ref(q, k, v, valid, H, w), (out, qc.grad, kc.grad, vc.grad)):
        torch.testing.assert_close(a.cpu(), r.detach(), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------ cross-attention core
@pytest.mark.parametrize("name,B", CORE_CASES)
def test_xattn_core_at_bench_batch(name, B):
    from mmgl_amd import ops
    B, H, T, S, D = core_shape(name, B)
    d = H * D
    gen = torch.Generator(device="cuda").manual_seed(31 * B + d)
    q = (torch.randn(B, T, d, generator=gen, device="cuda") * (2.0 * D ** -0.5)).bfloat16()
    k, v = (torch.randn(B, S, d, generator=gen, device="cuda").bfloat16() for _ in range(2))
    w = torch.randn(B, T, d, generator=gen, device="cuda").bfloat16()
    valid = key_masks(B, S, gen)
    qd, kd, vd = (t.clone().requires_grad_() for t in (q, k, v))
    out = ops.xattn_core(qd, kd, vd, valid, H)
    out.backward(w)
    ref = xattn_ref(q, k, v, valid, H, w)
    got = (out, qd.grad, kd.grad, vd.grad)
    for t in got:
        assert torch.isfinite(t).all()
    # masked keys of a sample that has a valid key receive exactly zero dK and dV
    for b in range(B):
        if valid[b].any() and not valid[b].all():
            assert float(kd.grad[b][~valid[b]].abs().max()) == 0.0 and float(vd.grad[b][~valid[b]].abs().max()) == 0.0, b
    errs = {}
    for n_, a, r in zip(("out", "dq", "dk", "dv"), got, ref):
        e = slice_err(a.view(B, -1, H, D), r.view(B, -1, H, D), (0, 2))
        errs[n_] = e
    print(f"[bench-shapes] xattn {name} B={B} " + " ".join(f"{n_} {float(e.max()):.3e}" for n_, e in errs.items()))
    for n_, e in errs.items():
        worst = int(e.argmax())
        assert float(e.max()) <= TOL_XATTN[n_], (f"{n_}: per-(sample, head) error {float(e.max()):.3e} > {TOL_XATTN[n_]:.1e} at sample "
                                                f"{worst // H} ({MASK_KINDS[(worst // H) % 5]}), head {worst % H}")


# ------------------------------------------------------------------------------------------------ trainable linears
def _check_linear(what, got, ref, weight_grad=False):
    e = elementwise_err(got, ref, floor_frac=1e-2)
    msg = f"{what} el {e:.3e}"
    ok = e <= TOL_LIN_EL
    if weight_grad:
        et = tile_err(got, ref)
        msg += f" tile {et:.3e}"
        ok = ok and et <= TOL_LIN_TILE
    return ok, msg


@pytest.mark.parametrize("name,B,row", LINEAR_CASES, ids=[f"{n}-B{B}-{r.label.replace('/', '+')}" for n, B, r in LINEAR_CASES])
def test_trainable_linear_at_bench_batch(name, B, row):
    from mmgl_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(row.M + 7 * row.N + row.K)
    M, K, N = row.M, row.K, row.N
    checks = []
    if row.kind == "plain":
        x = torch.randn(M, K, generator=gen, device="cuda").bfloat16()
        W = (torch.randn(N, K, generator=gen, device="cuda") * K ** -0.5).bfloat16()
        b = (torch.randn(N, generator=gen, device="cuda") * 0.3).bfloat16() if row.bias else None
        dy = torch.randn(M, N, generator=gen, device="cuda").bfloat16()
        xd = x.clone().requires_grad_(row.need_dx)
        Wd = W.clone().requires_grad_()
        bd = b.clone().requires_grad_() if b is not None else None
        y = ops.linear(xd, Wd, bd, out_scale=row.out_scale)
        y.backward(dy)
        x64, W64, dy64, s = x.double(), W.double(), dy.double(), row.out_scale
        yr = x64 @ W64.t() + (b.double() if b is not None else 0.0)
        checks += [("y", y, yr * s), ("dW", Wd.grad, (dy64.t() @ x64) * s, True)]
        if row.need_dx:
            checks.append(("dx", xd.grad, (dy64 @ W64) * s))
        if b is not None:
            checks.append(("db", bd.grad, dy64.sum(0) * s))
    elif row.kind == "relu_pair":
        # Each GEMM of a pair against float64 from its own bf16 operands: fc2 from fc1's output h, fc1's backward from the gradient
        # fc2's dgrad hands it (h.grad) -- both checked themselves.  A float64 chain would compare every downstream GEMM with an
        # unrounded intermediate: its 2^-9 rounding, summed over thousands of terms, dominated the element-wise error (up to 5e-2).
        F_ = N
        x = torch.randn(M, K, generator=gen, device="cuda").bfloat16()
        W1 = (torch.randn(F_, K, generator=gen, device="cuda") * K ** -0.5).bfloat16()
        b1 = (torch.randn(F_, generator=gen, device="cuda") * 0.3).bfloat16()
        W2 = (torch.randn(K, F_, generator=gen, device="cuda") * F_ ** -0.5).bfloat16()
        b2 = (torch.randn(K, generator=gen, device="cuda") * 0.3).bfloat16()
        dy = torch.randn(M, K, generator=gen, device="cuda").bfloat16()
        ps = [t.clone().requires_grad_() for t in (x, W1, b1, W2, b2)]
        y, h = ops.relu_ffn(*ps, frozen=False, return_hidden=True)          # exactly as the gated layer's MPTDecoderLayer._ffn
        h.retain_grad()
        y.backward(dy)
        x64, W164, W264, dy64 = x.double(), W1.double(), W2.double(), dy.double()
        hh, dh = h.detach().double(), h.grad.double()
        checks += [("h", h, (x64 @ W164.t() + b1.double()).clamp_min(0)), ("y", y, hh @ W264.t() + b2.double()),
                   ("dW2", ps[3].grad, dy64.t() @ hh, True), ("db2", ps[4].grad, dy64.sum(0)),
                   ("dh", h.grad, (dy64 @ W264) * (hh > 0)),                # fc1's ReLU backward folded into fc2's dgrad
                   ("dx", ps[0].grad, dh @ W164), ("dW1", ps[1].grad, dh.t() @ x64, True), ("db1", ps[2].grad, dh.sum(0))]
    else:
        # Llama: fused gate|up, ops.swiglu, down_proj (modelling_llama_cross_attention.py:50-51); stage by stage as the pair above
        F_ = N
        x = torch.randn(M, K, generator=gen, device="cuda").bfloat16()
        Wgu = (torch.randn(2 * F_, K, generator=gen, device="cuda") * K ** -0.5).bfloat16()
        Wd_ = (torch.randn(K, F_, generator=gen, device="cuda") * F_ ** -0.5).bfloat16()
        dy = torch.randn(M, K, generator=gen, device="cuda").bfloat16()
        ps = [t.clone().requires_grad_() for t in (x, Wgu, Wd_)]
        gu = ops.linear(ps[0], ps[1], None)
        gu.retain_grad()
        mid = ops.swiglu(gu)
        mid.retain_grad()
        y = ops.linear(mid, ps[2], None)
        y.backward(dy)
        x64, Wgu64, Wd64, dy64 = x.double(), Wgu.double(), Wd_.double(), dy.double()
        g_, u_ = gu.detach().double().split(F_, dim=1)
        sg = torch.sigmoid(g_)
        mm, dm = mid.detach().double(), mid.grad.double()
        dgu = gu.grad.double()
        checks += [("gate_up", gu, x64 @ Wgu64.t()), ("swiglu", mid, g_ * sg * u_), ("y", y, mm @ Wd64.t()),
                   ("dW_down", ps[2].grad, dy64.t() @ mm, True), ("d_mid", mid.grad, dy64 @ Wd64),
                   ("d_gate_up", gu.grad, torch.cat([dm * u_ * sg * (1 + g_ * (1 - sg)), dm * g_ * sg], dim=1)),
                   ("dx", ps[0].grad, dgu @ Wgu64), ("dW_gate_up", ps[1].grad, dgu.t() @ x64, True)]
        del g_, u_, sg, dm
    results = [_check_linear(c[0], c[1], c[2], len(c) > 3) for c in checks]
    print(f"[bench-shapes] linear {name} B={B} {row.label} M={M} " + "; ".join(m for _, m in results))
    bad = [m for ok, m in results if not ok]
    assert not bad, f"{row}: " + "; ".join(bad)


# ------------------------------------------------------------------------------------------------ census: the table is what the model launches
def _census(name, B=4):
    """The shape / flag sets of mmgl_xattn_fwd / _bwd and mmgl_linear_fwd / _bwd during one bf16 training step of config `name` at
    batch B (bench's model and batch; 4 decoder layers with a gated cross-attention layer after each one instead of 24 with one after
    every 6th: every gated layer launches the same shapes)."""
    from mmgl_amd import _lib
    from mmgl_amd.model import CrossAttentionModel
    cfg = bench.CONFIGS[name]
    lm_cfg, txt_cfg, vis_cfg = bench.hf_configs(cfg)
    lm_cfg.num_hidden_layers = 4
    torch.manual_seed(1234)
    with torch.device("cuda"):
        model = CrossAttentionModel(bench.make_args(cfg, neighbor_layer_wise=1), tokenizer=None, lm_config=lm_cfg, text_config=txt_cfg,
                                    visual_config=vis_cfg)
    model = model.to(torch.bfloat16).train()
    batch, _ = bench.synthetic_batch(B, cfg, seed=1234, device=torch.device("cuda"))
    seen = set()
    real = _lib.call

    def call(fname, work, *args):
        if fname == "mmgl_xattn_fwd":
            seen.add((fname,) + tuple(args[6:12]))
        elif fname == "mmgl_xattn_bwd":
            seen.add((fname,) + tuple(args[11:17]))
        elif fname == "mmgl_linear_fwd":
            seen.add((fname,) + tuple(args[4:10]) + (args[2] is not None,))
        elif fname == "mmgl_linear_bwd":
            seen.add((fname,) + tuple(args[9:17]) + tuple(a is not None for a in args[4:7]))
        return real(fname, work, *args)

    _lib.call = call
    try:
        T = batch["input_ids"].shape[1]
        out = model(**batch, logits_slice=slice(cfg["lin"], T - 1))
        out.loss.backward()
        torch.cuda.synchronize()
    finally:
        _lib.call = real
    return seen


def _expected(name, B=4):
    """The same records as the table predicts them (bf16 = dtype code 1; relu_ffn's fc1 passes act 0 backward: its ReLU backward is fc2's mask_dx)."""
    Bc, H, T, S, D = core_shape(name, B)
    exp = {("mmgl_xattn_fwd", Bc, H, T, S, D, 1), ("mmgl_xattn_bwd", Bc, H, T, S, D, 1)}
    for r in linears(name, B):
        if r.kind == "relu_pair":
            layers = [(r.M, r.N, r.K, 1, 1.0, 0, 0, True), (r.M, r.K, r.N, 0, 1.0, 0, 1, True)]   # (M, N, K, act, scale, act bwd, mask_dx, dx)
        else:
            layers = [(r.M, r.N, r.K, 0, r.out_scale, 0, 0, r.need_dx)]
        for M, N, K, act, sc, act_b, mdx, ndx in layers:
            exp.add(("mmgl_linear_fwd", M, N, K, act, sc, 1, r.bias))
            exp.add(("mmgl_linear_bwd", M, N, K, act_b, sc, 0, mdx, 1, ndx, True, r.bias))
    return exp


@pytest.mark.parametrize("name", ["opt-1.3b", "opt-125m"])
def test_census_matches_model(name):
    seen = _census(name)
    exp = _expected(name)
    print(f"[bench-shapes] census {name}: {len(seen)} launch signatures")
    assert seen <= exp, f"launched but not in the table: {sorted(seen - exp)}"
    assert exp <= seen, f"in the table but never launched: {sorted(exp - seen)}"
