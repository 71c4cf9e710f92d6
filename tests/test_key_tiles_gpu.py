"""-m gpu: the frozen layers on live key tiles only -- mmgl_selfattn_tiles_*, the LayerNorm entry points with the compact copy,
and one frozen MPTDecoderLayer on the new route against the dense one and the fp32 oracle."""
import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")


def _masks(T):
    """T = 256: all valid | 70 valid, pad to 192, 10 valid from 192 on (tile 2 dead, tiles 1 and 3 partly live) | 64 valid, then pad
    with one valid key at 192.  T = 640: the shape of a padded prompt + summary (ten tiles, dead ones in the middle and at the end)."""
    if T == 256:
        m = torch.zeros(3, T, dtype=torch.uint8)
        m[0] = 1
        m[1, :70] = 1; m[1, 192:202] = 1
        m[2, :64] = 1; m[2, 192] = 1
        return m
    m = torch.zeros(2, T, dtype=torch.uint8)
    m[0, :130] = 1; m[0, 512:530] = 1
    m[1, :512] = 1; m[1, 512:575] = 1
    return m


def _tiles(mask):
    from mmgl_amd import ops
    table, m_live = ops.key_tile_table(mask)
    return ops.KeyTiles(table, m_live, "cuda")


def _nan_buffer(rows, cols, extra=64):
    """[rows, cols] view of a NaN-filled buffer with `extra` rows behind it (the unused tail)."""
    full = torch.full((rows + extra, cols), NAN, dtype=BF, device="cuda")
    return full, full[:rows]


@pytest.mark.parametrize("T", [256, 640])
def test_selfattn_tiles_bitwise_equals_dense(T):
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr, ptr_off, stream_ptr
    H, D = 2, 64
    d = H * D
    mask = _masks(T)
    B = mask.shape[0]
    kt = _tiles(mask)
    live = kt.rowmap >= 0
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(B, T, 3 * d, generator=g).to(BF).cuda()
    qkv[..., :d] *= D ** -0.5
    dout = torch.randn(B, T, d, generator=g).to(BF).cuda()
    valid = mask.cuda()
    # compact K | V gathered from the dense buffer; the tail behind the m_live rows is NaN
    kv_full, kvc = _nan_buffer(kt.m_live, 2 * d)
    kvc[kt.rowmap[live].long()] = qkv.view(-1, 3 * d)[live][:, d:]
    assert not torch.isnan(kvc.float()).any()                     # every compact row belongs to exactly one row of a live tile

    lib, code, st = _lib.lib(), _lib.BF16, stream_ptr()
    out0, out1 = torch.empty(B, T, d, dtype=BF, device="cuda"), torch.full((B, T, d), NAN, dtype=BF, device="cuda")
    lse0, lse1 = torch.empty(B, H, T, device="cuda"), torch.full((B, H, T), NAN, device="cuda")
    _lib.call("mmgl_selfattn_fwd", None, ptr(qkv), ptr_off(qkv, 2 * d), ptr_off(qkv, 4 * d), ptr(valid), ptr(out0), ptr(lse0), B, H, T, D, 3 * d,
              code, st)
    _lib.call("mmgl_selfattn_tiles_fwd", None, ptr(qkv), ptr(kvc), ptr_off(kvc, 2 * d), ptr(valid), ptr(kt.table), ptr(out1), ptr(lse1), B, H, T,
              D, kt.m_live, 3 * d, 2 * d, code, st)
    assert torch.equal(out1, out0) and torch.equal(lse1, lse0)

    nws = lib.mmgl_selfattn_bwd_workspace(B, H, T)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    dqkv = torch.empty_like(qkv)
    _lib.call("mmgl_selfattn_bwd", None, ptr(dout), ptr(qkv), ptr_off(qkv, 2 * d), ptr_off(qkv, 4 * d), ptr(out0), ptr(lse0), ptr(valid), ptr(dqkv),
              ptr_off(dqkv, 2 * d), ptr_off(dqkv, 4 * d), ptr(ws), nws, B, H, T, D, 3 * d, 3 * d, code, st)
    # dQ | dK | dV keep the dense layout (the fused dgrad reads them): every element, the zeros of the dead tiles included
    dqkv1 = torch.full((B, T, 3 * d), NAN, dtype=BF, device="cuda")
    _lib.call("mmgl_selfattn_tiles_bwd", None, ptr(dout), ptr(qkv), ptr(kvc), ptr_off(kvc, 2 * d), ptr(out1), ptr(lse1), ptr(valid), ptr(kt.table),
              ptr(dqkv1), ptr_off(dqkv1, 2 * d), ptr_off(dqkv1, 4 * d), ptr(ws), nws, B, H, T, D, kt.m_live, 3 * d, 2 * d, 3 * d, 3 * d, code, st)
    assert torch.equal(dqkv1.view(torch.int16), dqkv.view(torch.int16))                            # bit patterns: -0.0 counts
    assert not dqkv1.view(-1, 3 * d)[~live][:, d:].float().abs().any()                             # dead tiles: zero dK | dV
    assert torch.isnan(kv_full[kt.m_live:].float()).all()                                          # the tail is untouched

    with pytest.raises((ValueError, RuntimeError)):              # head_dim 128 keeps the dense entry points
        _lib.call("mmgl_selfattn_tiles_fwd", None, ptr(qkv), ptr(kvc), ptr_off(kvc, 2 * d), ptr(valid), ptr(kt.table), ptr(out1), ptr(lse1), B, 1, T,
                  128, kt.m_live, 3 * d, 2 * d, code, st)


def _norm_inputs(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s, scale=1.0, shift=0.0: (torch.randn(*s, generator=g) * scale + shift).to(BF).cuda()
    return dict(x=mk(rows, cols, scale=2.0, shift=0.5), r=mk(rows, cols), gamma=mk(cols, scale=0.2, shift=1.0), beta=mk(cols, scale=0.1),
                dy=mk(rows, cols), dsum=mk(rows, cols))


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_norm_tiles_forward_equals_dense(p):
    from mmgl_amd import ops
    cols, seed = 128, 424242
    kt = _tiles(_masks(256))
    rows = kt.rowmap.numel()
    live = kt.rowmap >= 0
    t = _norm_inputs(rows, cols, 5)
    if p == 0.0:                                                  # mmgl_layernorm_tiles_fwd against mmgl_layernorm_fwd
        full, yc = _nan_buffer(kt.m_live, cols, extra=8)
        _, y1, _, mean1, rstd1 = ops._norm_fwd(False, t["x"], None, t["gamma"], t["beta"], 1e-5, compact=(kt.rowmap, yc))
        _, y0, _, mean0, rstd0 = ops._norm_fwd(False, t["x"], None, t["gamma"], t["beta"], 1e-5)
        assert torch.equal(y1, y0) and torch.equal(mean1, mean0) and torch.equal(rstd1, rstd0)
        assert torch.equal(yc[kt.rowmap[live].long()], y0[live]) and not torch.isnan(yc.float()).any()
        assert torch.isnan(full[kt.m_live:].float()).all()
    # mmgl_add_layernorm_tiles_fwd against mmgl_add_layernorm_fwd, without and with dropout
    full, yc = _nan_buffer(kt.m_live, cols, extra=8)
    s1, y1, _, mean1, rstd1 = ops._norm_fwd(False, t["x"], t["r"], t["gamma"], t["beta"], 1e-5, p, seed, compact=(kt.rowmap, yc))
    s0, y0, _, mean0, rstd0 = ops._norm_fwd(False, t["x"], t["r"], t["gamma"], t["beta"], 1e-5, p, seed)
    assert torch.equal(s1, s0) and torch.equal(y1, y0) and torch.equal(mean1, mean0) and torch.equal(rstd1, rstd0)
    assert torch.equal(yc[kt.rowmap[live].long()], y0[live]) and not torch.isnan(yc.float()).any()
    assert torch.isnan(full[kt.m_live:].float()).all()
    if p > 0.0:
        assert abs((s0 == t["r"]).float().mean().item() - p) < 0.03           # the dropout did drop


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_norm_tiles_backward_is_the_dense_backward(p):
    """The compact copy carries no gradient of its own (the fused dgrad of the QKV projection returns everything on y): with and
    without it the pair's backward is the same kernel on the same operands, bit for bit."""
    from mmgl_amd import ops
    cols, seed = 128, 99
    kt = _tiles(_masks(256))
    rows = kt.rowmap.numel()
    t = _norm_inputs(rows, cols, 6)
    grads = []
    for tiles in (None, kt):
        x, r = t["x"].clone().requires_grad_(), t["r"].clone().requires_grad_()
        if tiles is None:
            s, y = ops.add_layer_norm_pair(x, r, t["gamma"], t["beta"], 1e-5, p, True, seed=seed)
        else:
            s, y, yc = ops.add_layer_norm_tiles(x, r, t["gamma"], t["beta"], 1e-5, tiles, p, True, seed=seed)
            assert not yc.requires_grad
        ((y * t["dy"]).sum() + (s * t["dsum"]).sum()).backward()
        grads.append((x.grad, r.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


def _layer(dropout):
    from transformers import OPTConfig
    from helpers import mpt_args
    from mmgl_amd.model.modelling_cross_attention import MPTConfig, MPTDecoderLayer
    opt = OPTConfig(vocab_size=128, hidden_size=128, num_attention_heads=2, ffn_dim=256, num_hidden_layers=2, max_position_embeddings=700,
                    word_embed_proj_dim=128, do_layer_norm_before=True, dropout=dropout, attention_dropout=0.0, pad_token_id=1,
                    bos_token_id=2, eos_token_id=2, init_std=0.08)
    torch.manual_seed(0)
    layer = MPTDecoderLayer(MPTConfig(mpt_args(), opt), cross_attention=False)
    with torch.no_grad():
        for n, p in layer.named_parameters():                     # biases and LayerNorm affines away from their 0 / 1 initial values
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    layer = layer.to(BF).cuda()
    for p in layer.parameters():
        p.requires_grad_(False)                                  # a frozen OPT layer: the fused QKV projection
    return layer


def _oracle(layer, x, mask, w, drop):
    """fp32 oracle (oracle/lm_ref.py) of the frozen pre-LN layer from the bf16-rounded parameters and input; `drop` = the two
    dropout factors (0 or 1 / (1 - p) per element) of the layer's two residual adds, None in eval mode."""
    from oracle import lm_ref
    p = {k: v.detach().float().cpu() for k, v in layer.state_dict().items()}
    xr = x.detach().float().cpu().requires_grad_()
    add = lm_ref.decoder_self_mask(mask.cpu(), torch.float32)
    H = layer.self_attn.num_heads
    if drop is None:
        cfg = lm_ref.LMConfig(vocab_size=128, hidden_size=x.shape[-1], num_attention_heads=H, ffn_dim=p["fc1.weight"].shape[0],
                              num_hidden_layers=1, word_embed_proj_dim=x.shape[-1])
        out = lm_ref.decoder_layer(p, "", xr, add, cfg)
    else:
        a = lm_ref.attention(p, "self_attn.", lm_ref._ln(p, "self_attn_layer_norm.", xr), add, H)
        h = xr + drop[0] * a
        f = F.linear(F.relu(F.linear(lm_ref._ln(p, "final_layer_norm.", h), p["fc1.weight"], p["fc1.bias"])), p["fc2.weight"], p["fc2.bias"])
        out = h + drop[1] * f
    (out * w.float().cpu()).sum().backward()
    return out.detach(), xr.grad


@pytest.mark.parametrize("train", [False, True])
def test_frozen_layer_on_live_tiles_tracks_the_oracle_like_the_dense_path(train):
    """One frozen MPTDecoderLayer at d = 128, new route against dense route, both against the fp32 oracle.  The new route's error
    may exceed the dense route's by one bf16 rounding of the largest element, 2^-8 max|oracle|: at this toy size the split projection
    may run on another GEMM kernel than the fused one, with another summation order; nothing else differs."""
    from mmgl_amd import ops
    mask = _masks(256)
    B, T = mask.shape
    d, pdrop, seed = 128, 0.1, 1234
    layer = _layer(pdrop)
    layer.train(train)
    kt = _tiles(mask)
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, T, d, generator=g).to(BF).cuda()
    w = torch.randn(B, T, d, generator=g).to(BF).cuda()
    valid = mask.cuda()
    res = {}
    for name, tiles in (("dense", None), ("tiles", kt)):
        xd = x.clone().requires_grad_()
        torch.manual_seed(seed)                                   # the dropout seeds are drawn from torch's host generator
        out = layer(xd * 1.0, attention_mask=valid, key_tiles=tiles)[0]
        (out * w).sum().backward()
        res[name] = (out.detach().float().cpu(), xd.grad.float().cpu())
    drop = None
    if train:
        torch.manual_seed(seed)
        seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(2)]
        one, zero = torch.ones(B, T, d, device="cuda"), torch.zeros(B, T, d, device="cuda")
        drop = [ops.gated_residual(zero, one, None, pdrop, True, seed=s).cpu() for s in seeds]
        assert all(abs((m == 0).float().mean().item() - pdrop) < 0.02 for m in drop)
    ref = _oracle(layer, x, mask, w, drop)
    for i, what in enumerate(("out", "d input")):
        e_dense = (res["dense"][i] - ref[i]).abs().max().item()
        e_tiles = (res["tiles"][i] - ref[i]).abs().max().item()
        slack = 2.0 ** -8 * ref[i].abs().max().item()
        assert e_dense <= 4e-2 * ref[i].abs().max().item(), f"{what}: the dense path itself is off the oracle ({e_dense:.3e})"
        assert e_tiles <= e_dense + slack, f"{what}: error vs oracle, tiles {e_tiles:.4e}, dense {e_dense:.4e}, allowed excess {slack:.4e}"


def test_layer_falls_back_to_the_dense_path():
    """No table, a table of another shape, a decode cache: the dense path, bit for bit."""
    from mmgl_amd import ops
    mask = _masks(256)
    layer = _layer(0.0).eval()
    x = torch.randn(3, 256, 128, generator=torch.Generator().manual_seed(1)).to(BF).cuda()
    valid = mask.cuda()
    with torch.no_grad():
        want = layer(x, attention_mask=valid)[0]
        other = _tiles(_masks(640))
        assert torch.equal(layer(x, attention_mask=valid, key_tiles=other)[0], want)
        kv = torch.empty(3, 256, 256, dtype=BF, device="cuda")
        assert torch.equal(layer(x, attention_mask=valid, key_tiles=_tiles(mask), kv_out=kv)[0], want)
        got = layer(x, attention_mask=valid, key_tiles=_tiles(mask))[0]          # the no-grad route of the new path
    assert_close(got.float(), want.float(), 2e-2, "no-grad tiles route")
    assert not ops.selfattn_tiles_supported(x.float(), 2, _tiles(mask))
