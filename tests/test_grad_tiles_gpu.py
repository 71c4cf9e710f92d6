"""-m gpu: live-first gradient rows of the frozen layers -- mmgl_gemm_nt_rowk (a K extent per 256-row tile), mmgl_selfattn_tiles_rows_bwd
(the attention backward storing dQ | dK | dV with the live key tiles first), mmgl_add_layernorm_rows_bwd (dy through a row map) and the
one autograd node that strings them together, each against the call it replaces.  Comparisons are torch.equal: a sum that is exactly
-0 may come out as +0 once its zero tail is no longer added, nothing else may move."""
import pytest
import torch

from gemm_ref import GemmRef

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")


def _rowk(x, w, K_short, m_full, out=None):
    from mmgl_amd import ops
    return ops.gemm_nt_rowk(x, w, K_short, m_full, out=out)


def _ceil256(m):
    return -(-m // 256) * 256


# ------------------------------------------------------------------------------------------ GEMM
M0, N0, K0, KS0 = 1280, 512, 768, 256                            # 5 x 2 tiles, 6 / 2 K units


@pytest.fixture(scope="module")
def gemm_operands():
    t = GemmRef.inputs(BF, M0, N0, K0, seed=0, device="cuda")
    return t["x"], t["w"]


@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
@pytest.mark.parametrize("m_full", [0, 64, 256, 320, 1280])
def test_rowk_gemm_equals_the_full_k_walk(gemm_operands, m_full, dynamic):
    """(a) bit-equal to the same entry at m_full = M (every tile long: the plain kernel), (b) within the per-element fp64 bound of
    tests/test_gemm_bounds_gpu.py, (c) NaNs behind K_short in the short row tiles reach nothing, (d) all of it under the dynamic
    tile schedule, which leaves its counters at zero."""
    from mmgl_amd import ops
    x0, w = gemm_operands
    x = x0.clone()
    x[m_full:, KS0:] = 0
    want = _rowk(x, w, KS0, M0)
    counter = ops.gemm_dynamic_schedule(True) if dynamic else None
    try:
        slab = torch.full((M0 + 8, N0), NAN, dtype=BF, device="cuda")
        got = _rowk(x, w, KS0, m_full, out=slab[:M0])
        xn = x.clone()
        xn[_ceil256(m_full):, KS0:] = NAN
        got_nan = _rowk(xn, w, KS0, m_full)
        torch.cuda.synchronize()
        if dynamic:
            assert not counter.any(), "the tile counters must be left at zero"
    finally:
        if dynamic:
            ops.gemm_dynamic_schedule(False)
    assert torch.equal(got, want), f"m_full={m_full}: {(got.float() - want.float()).abs().max().item():.3e} off the full-K launch"
    assert torch.isnan(slab[M0:].float()).all()
    GemmRef.forward(x, w).check(got, f"rowk-{m_full}", "P8 rowk bf16", n=GemmRef.chain(BF, K0))
    assert torch.equal(got_nan, want), f"m_full={m_full}: columns behind K_short of a short row tile were read"


def test_rowk_gemm_equals_gemm_nt_on_the_persistent_kernel():
    """160 tiles: mmgl_gemm_nt itself takes the persistent kernel, unsplit; a long -> short boundary inside a workgroup's items."""
    from mmgl_amd import _lib, ops
    M, N, K, KS, m_full = 5120, 2048, 768, 256, 1300
    assert _lib.lib().mmgl_gemm_nt_fast(M, N, K, K, K, N, _lib.BF16) == 1
    t = GemmRef.inputs(BF, M, N, K, seed=1, device="cuda")
    x, w = t["x"], t["w"]
    x[m_full:, KS:] = 0
    want = ops.gemm_nt(x, w, k_splits=False)
    xn = x.clone()
    xn[_ceil256(m_full):, KS:] = NAN
    assert torch.equal(_rowk(xn, w, KS, m_full), want)            # 48 long tiles, 112 short ones
    assert torch.equal(_rowk(x, w, KS, M), want)                  # every tile long
    xs = x.clone()
    xs[:, KS:] = 0
    xsn = xs.clone()
    xsn[:, KS:] = NAN
    assert torch.equal(_rowk(xsn, w, KS, 0), ops.gemm_nt(xs, w, k_splits=False))      # every tile short


def test_rowk_gemm_refuses_what_it_cannot_run():
    x = torch.zeros(512, 768, dtype=BF, device="cuda")
    w = torch.zeros(256, 768, dtype=BF, device="cuda")
    for ks, mf in ((128, 0), (320, 0), (1024, 0), (256, -1), (256, 513)):
        with pytest.raises(ValueError):
            _rowk(x, w, ks, mf)
    with pytest.raises(ValueError):
        _rowk(x.float(), w.float(), 256, 0)


# ------------------------------------------------------------------------------------------ attention backward
def _masks(T):
    """A fully live sample | a dead tile between live ones | a single live tile."""
    m = torch.zeros(3, T, dtype=torch.uint8)
    m[0] = 1
    if T == 256:
        m[1, :70] = 1; m[1, 192:202] = 1
        m[2, :10] = 1
    else:
        m[1, :130] = 1; m[1, 512:530] = 1
        m[2, :40] = 1
    return m


def _tiles(mask):
    from mmgl_amd import ops
    table, m_live = ops.key_tile_table(mask)
    return ops.KeyTiles(table, m_live, "cuda")


@pytest.mark.parametrize("T", [256, 640])
def test_attention_backward_with_live_first_rows(T):
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
    kvc = torch.zeros(kt.m_live, 2 * d, dtype=BF, device="cuda")
    kvc[kt.rowmap[live].long()] = qkv.view(-1, 3 * d)[live][:, d:]
    code, st = _lib.BF16, stream_ptr()
    out, lse = torch.empty(B, T, d, dtype=BF, device="cuda"), torch.empty(B, H, T, device="cuda")
    _lib.call("mmgl_selfattn_tiles_fwd", None, ptr(qkv), ptr(kvc), ptr_off(kvc, 2 * d), ptr(valid), ptr(kt.table), ptr(out), ptr(lse), B, H, T,
              D, kt.m_live, 3 * d, 2 * d, code, st)
    nws = _lib.lib().mmgl_selfattn_bwd_workspace(B, H, T)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    args = lambda buf: (ptr(buf), ptr_off(buf, 2 * d), ptr_off(buf, 4 * d), ptr(ws), nws, B, H, T, D, kt.m_live)
    want = torch.full((B * T, 3 * d), NAN, dtype=BF, device="cuda")
    _lib.call("mmgl_selfattn_tiles_bwd", None, ptr(dout), ptr(qkv), ptr(kvc), ptr_off(kvc, 2 * d), ptr(out), ptr(lse), ptr(valid), ptr(kt.table),
              *args(want), 3 * d, 2 * d, 3 * d, 3 * d, code, st)
    dkv_rows = min(B * T, _ceil256(kt.m_live))
    assert kt.m_live < dkv_rows < B * T or T == 256               # T = 640: dead rows inside the boundary row tile AND rows behind it
    slab = torch.full((B * T + 64, 3 * d), NAN, dtype=BF, device="cuda")
    got = slab[:B * T]
    _lib.call("mmgl_selfattn_tiles_rows_bwd", None, ptr(dout), ptr(qkv), ptr(kvc), ptr_off(kvc, 2 * d), ptr(out), ptr(lse), ptr(valid),
              ptr(kt.table), ptr(kt.dest), *args(got), dkv_rows, 3 * d, 2 * d, 3 * d, 3 * d, code, st)
    torch.cuda.synchronize()
    rows = kt.grad_rows.long()
    assert sorted(rows.tolist()) == list(range(B * T))
    back = got[rows]                                              # row r of the dense layout
    assert torch.equal(back[:, :d], want[:, :d]), "dQ"
    read = rows < dkv_rows                                        # the rows whose dK | dV the short-K dgrad reads
    assert torch.equal(back[read][:, d:], want[read][:, d:]), "dK | dV"
    assert not want[~read][:, d:].float().abs().any() and not want[rows >= kt.m_live][:, d:].float().abs().any()
    assert torch.isnan(back[~read][:, d:].float()).all(), "dK | dV behind the boundary row tile are not stored"
    assert not got[kt.m_live:dkv_rows, d:].float().abs().any()    # dead rows inside the boundary row tile: written, zero
    assert torch.isnan(slab[B * T:].float()).all()


# ------------------------------------------------------------------------------------------ norm backward
@pytest.mark.parametrize("with_dres", [False, True], ids=["nodres", "dres"])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_norm_backward_reads_dy_through_the_row_map(p, with_dres):
    from mmgl_amd import ops
    cols, seed = 128, 77
    kt = _tiles(_masks(256))
    rows = kt.grad_rows.numel()
    g = torch.Generator().manual_seed(9)
    mk = lambda *s, scale=1.0, shift=0.0: (torch.randn(*s, generator=g) * scale + shift).to(BF).cuda()
    x, r, gamma, beta, dy, dsum = mk(rows, cols, scale=2.0, shift=0.5), mk(rows, cols), mk(cols, scale=0.2, shift=1.0), mk(cols, scale=0.1), \
        mk(rows, cols), mk(rows, cols)
    s, _, gk, mean, rstd = ops._norm_fwd(False, x, r, gamma, beta, 1e-5, p, seed)
    dyp = torch.full_like(dy, NAN)
    dyp[kt.grad_rows.long()] = dy
    ds = dsum if with_dres else None
    want = ops._norm_bwd(False, True, dy, ds, s, gk, mean, rstd, (False, False), None, p, seed)
    got = ops._norm_bwd(False, True, dyp, ds, s, gk, mean, rstd, (False, False), None, p, seed, dy_rows=kt.grad_rows)
    assert torch.equal(got[0], want[0])
    assert (got[1] is None and want[1] is None and p == 0.0) or torch.equal(got[1], want[1])
    # with parameter gradients too (the node itself keeps frozen affines; the kernel has the instantiation)
    want = ops._norm_bwd(False, True, dy, ds, s, gk, mean, rstd, (True, True), torch.float32, p, seed)
    got = ops._norm_bwd(False, True, dyp, ds, s, gk, mean, rstd, (True, True), torch.float32, p, seed, dy_rows=kt.grad_rows)
    assert all(torch.equal(a, b) for a, b in zip(got, want) if a is not None)


# ------------------------------------------------------------------------------------------ layer
B_L, T_L, D_L, H_L = 64, 640, 256, 4                              # 40960 rows: the dense dgrad [40960, 768] -> 256 is 160 whole tiles


def _layer(dropout):
    from transformers import OPTConfig
    from helpers import mpt_args
    from mmgl_amd.model.modelling_cross_attention import MPTConfig, MPTDecoderLayer
    opt = OPTConfig(vocab_size=128, hidden_size=D_L, num_attention_heads=H_L, ffn_dim=256, num_hidden_layers=2, max_position_embeddings=700,
                    word_embed_proj_dim=D_L, do_layer_norm_before=True, dropout=dropout, attention_dropout=0.0, pad_token_id=1,
                    bos_token_id=2, eos_token_id=2, init_std=0.08)
    torch.manual_seed(0)
    layer = MPTDecoderLayer(MPTConfig(mpt_args(), opt), cross_attention=False)
    with torch.no_grad():
        for n, p in layer.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    layer = layer.to(BF).cuda()
    for p in layer.parameters():
        p.requires_grad_(False)
    return layer


def _layer_mask():
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(1, T_L + 1, (B_L,), generator=g)
    lens[0], lens[1] = T_L, 1
    m = (torch.arange(T_L)[None, :] < lens[:, None]).to(torch.uint8)
    m[2, :] = 0; m[2, :70] = 1; m[2, 512:530] = 1                 # a dead tile between live ones
    return m


@pytest.fixture(scope="module")
def layer_setup():
    mask = _layer_mask()
    g = torch.Generator().manual_seed(23)
    mk = lambda: torch.randn(B_L, T_L, D_L, generator=g).to(BF).cuda()
    return dict(layer=_layer(0.1).train(), mask=mask, valid=mask.cuda(), kt=_tiles(mask), x=mk(), branch=mk(), w=mk())


def _run(s, deferred, calls=None, monkeypatch=None, supported=None):
    from mmgl_amd import ops
    from mmgl_amd.model.modelling_cross_attention import _Deferred
    if supported is not None:
        monkeypatch.setattr(ops, "frozen_attn_block_supported", lambda *a, **k: supported)
    if calls is not None:
        real = ops.frozen_attn_block_tiles
        monkeypatch.setattr(ops, "frozen_attn_block_tiles", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    x, br = s["x"].clone().requires_grad_(), s["branch"].clone().requires_grad_()
    torch.manual_seed(4321)                                       # the dropout seeds come from torch's host generator
    h = _Deferred(x * 1.0, br * 1.0, 0.1, True) if deferred else x * 1.0
    out = s["layer"](h, attention_mask=s["valid"], key_tiles=s["kt"])[0]
    (out * s["w"]).sum().backward()
    return out.detach(), x.grad, (br.grad if deferred else None)


@pytest.mark.parametrize("deferred", [False, True], ids=["fanout", "add+dropout"])
def test_one_node_block_equals_the_three_node_route(layer_setup, monkeypatch, deferred):
    """A frozen pre-LN layer in train mode with dropout: output and input gradients of the one-node route bit-equal to the present
    tile route (the same layer with the new route switched off)."""
    from mmgl_amd import ops
    s = layer_setup
    assert ops.frozen_attn_block_supported(s["x"], H_L, s["kt"], None, None, s["layer"].self_attn._frozen_qkv()[0])
    calls = []
    new = _run(s, deferred, calls=calls, monkeypatch=monkeypatch)
    assert calls == [1], "the layer did not take the one-node route"
    monkeypatch.undo()
    calls = []
    old = _run(s, deferred, calls=calls, monkeypatch=monkeypatch, supported=False)
    assert calls == []
    for a, b, what in zip(new, old, ("output", "d input", "d branch")):
        assert (a is None and b is None) or torch.equal(a, b), what


def test_fallbacks_take_the_three_node_route(layer_setup, monkeypatch):
    """Trainable LayerNorm parameters, no gradient flowing, and a batch whose dense dgrad is no run of whole tiles on the persistent
    kernel: each keeps the present route."""
    from mmgl_amd import ops
    s = layer_setup
    calls = []
    real = ops.frozen_attn_block_tiles
    monkeypatch.setattr(ops, "frozen_attn_block_tiles", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    layer, kt, valid = s["layer"], s["kt"], s["valid"]
    ln = layer.self_attn_layer_norm
    ln.weight.requires_grad_(True)
    try:
        x = s["x"].clone().requires_grad_()
        layer(x * 1.0, attention_mask=valid, key_tiles=kt)[0].sum().backward()
        assert ln.weight.grad is not None and calls == []
    finally:
        ln.weight.requires_grad_(False)
        ln.weight.grad = None
    with torch.no_grad():
        layer(s["x"], attention_mask=valid, key_tiles=kt)
    layer(s["x"], attention_mask=valid, key_tiles=kt)             # grad mode on, nothing requires a gradient
    assert calls == []
    small = _tiles(s["mask"][:4])
    xs = s["x"][:4].clone().requires_grad_()
    assert not ops.frozen_attn_block_supported(xs, H_L, small, None, None, layer.self_attn._frozen_qkv()[0])
    layer(xs * 1.0, attention_mask=valid[:4], key_tiles=small)[0].sum().backward()
    assert calls == [] and xs.grad is not None
    with pytest.raises(ValueError):
        ops.frozen_attn_block_tiles(xs, None, ln.weight, ln.bias, ln.eps, *layer.self_attn._frozen_qkv(), valid[:4], small, H_L)
