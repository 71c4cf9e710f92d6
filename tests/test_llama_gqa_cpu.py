"""CPU tests of grouped-query attention for the Llama variant: LlamaNeighborLM builds for num_key_value_heads < num_attention_heads
(it refused before), the fused q|k|v weight has (H + 2 Hkv) * D rows with only the q rows scaled, and the mmgl_selfattn_gqa_* entry
points validate their arguments before any launch (no GPU here)."""
import pytest
import torch

from helpers import mpt_args

H, D, HIDDEN = 4, 16, 64


def _cfg(n_kv, heads=H):
    from transformers import LlamaConfig
    return LlamaConfig(vocab_size=128, hidden_size=HIDDEN, intermediate_size=128, num_hidden_layers=2, num_attention_heads=heads,
                       num_key_value_heads=n_kv, max_position_embeddings=256, pad_token_id=1, bos_token_id=2, eos_token_id=2,
                       attention_dropout=0.0)


def _build(n_kv, heads=H):
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    torch.manual_seed(0)
    return LlamaNeighborLM(mpt_args(model_name_or_path="llama-tiny", neighbor_layer_wise=1), _cfg(n_kv, heads))


@pytest.mark.parametrize("n_kv", [2, 1])
def test_llama_neighbor_lm_builds_with_grouped_query_heads(n_kv):
    lm = _build(n_kv)
    assert lm.config.num_key_value_heads == n_kv
    assert all(f.H == H and f.Hkv == n_kv and f.D == D for f in lm._frozen)
    # the HF module owns the weights as loaded: k / v projections have Hkv * D rows, the state-dict keys are HF's
    sd = lm.state_dict()
    assert tuple(sd["llama.model.layers.0.self_attn.k_proj.weight"].shape) == (n_kv * D, HIDDEN)
    assert tuple(sd["llama.model.layers.0.self_attn.v_proj.weight"].shape) == (n_kv * D, HIDDEN)
    # the trainable gated layers keep their own hidden -> hidden multi-head projections
    assert tuple(lm.neighbor_layers[0].k_proj.weight.shape) == (HIDDEN, HIDDEN) and lm.neighbor_layers[0].num_heads == H
    assert {n for n, p in lm.named_parameters() if p.requires_grad} == {n for n, _ in lm.named_parameters() if n.startswith("neighbor_layers.")}


def test_indivisible_head_counts_raise():
    with pytest.raises(ValueError, match="multiple of"):
        _build(3, heads=4)


@pytest.mark.parametrize("n_kv", [4, 2, 1])
def test_fused_weight_layout_scales_only_the_q_rows(n_kv):
    lm = _build(n_kv)
    layer = lm._frozen[0]
    at = layer.layer.self_attn
    w_qkv, w_gu = layer._fused()
    assert tuple(w_qkv.shape) == ((H + 2 * n_kv) * D, HIDDEN)
    assert torch.equal(w_qkv[:H * D], (at.q_proj.weight.float() * D ** -0.5).to(w_qkv.dtype))
    assert torch.equal(w_qkv[H * D:(H + n_kv) * D], at.k_proj.weight)
    assert torch.equal(w_qkv[(H + n_kv) * D:], at.v_proj.weight)
    assert tuple(w_gu.shape) == (2 * 128, HIDDEN)


def test_gqa_entry_points_validate_before_any_launch():
    from mmgl_amd import _lib
    L = _lib.lib()
    B, T = 2, 70
    N = None
    fwd = lambda h, hkv, d, dt=1: L.mmgl_selfattn_gqa_fwd(N, N, N, N, N, N, B, h, hkv, T, d, 0, 0, dt, N)
    bwd = lambda h, hkv, d, dt=1: L.mmgl_selfattn_gqa_bwd(N, N, N, N, N, N, N, N, N, N, N, 0, B, h, hkv, T, d, 0, 0, 0, 0, dt, N)
    for f in (fwd, bwd):
        assert f(8, 2, 64) == 1 and b"null" in L.mmgl_last_error()              # null pointers
        assert f(8, 8, 64) == 1                                                  # ... also on the multi-head route it forwards to
        assert f(8, 3, 64) == 1 and b"multiple" in L.mmgl_last_error()           # H % Hkv
        assert f(8, 0, 64) == 1 and f(8, -2, 64) == 1 and f(2, 4, 64) == 1       # Hkv < 1, Hkv > H
        assert f(8, 2, 48) == 2 and f(8, 2, 48, 0) == 2                          # head_dim
        assert f(0, 1, 64) == 1
    for dt, es in ((0, 4), (1, 2)):
        for (h, d) in ((8, 64), (4, 16), (6, 128)):
            mha = L.mmgl_selfattn_bwd_workspace(B, h, T)
            assert mha > 0 and L.mmgl_selfattn_gqa_bwd_workspace(B, h, h, T, d, dt) == mha
            for hkv in (h // 2, 1):
                got = L.mmgl_selfattn_gqa_bwd_workspace(B, h, hkv, T, d, dt)
                assert got > mha and got - mha >= B * T * 2 * h * d * es            # delta + the expanded dK | dV scratch
    assert L.mmgl_selfattn_gqa_bwd_workspace(B, 8, 3, T, 64, 1) == 0
    # a short workspace is refused (pointers are never dereferenced on the host: any non-null value will do)
    p = _lib.c_void_p(4096)
    rc = L.mmgl_selfattn_gqa_bwd(p, p, p, p, p, p, p, p, p, p, p, L.mmgl_selfattn_bwd_workspace(B, 8, T), B, 8, 2, T, 64, 0, 0, 0, 0, 1, N)
    assert rc == 1 and b"workspace" in L.mmgl_last_error()
    # row strides: q rows hold H*D, k / v rows Hkv*D
    assert L.mmgl_selfattn_gqa_fwd(p, p, p, p, p, p, B, 8, 2, T, 64, 8 * 64 - 8, 0, 1, N) == 1
    assert L.mmgl_selfattn_gqa_fwd(p, p, p, p, p, p, B, 8, 2, T, 64, 0, 2 * 64 - 8, 1, N) == 1


def test_gqa_ops_have_no_cpu_path_and_check_shapes():
    from mmgl_amd import ops
    B, T = 2, 8
    q, kv = torch.randn(B, T, H * D), torch.randn(B, T, 2 * D)
    am = torch.ones(B, T, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.selfattn_core(q, kv, kv, am, H, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.selfattn_core_fused(torch.randn(B, T, (H + 4) * D), am, H, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rope_qk_(torch.randn(B, T, (H + 4) * D), torch.zeros(T, D // 2, 2), H, 2)
    with pytest.raises(ValueError, match="multiple of"):
        ops.selfattn_core(q, kv, kv, am, H, 3)
    with pytest.raises(ValueError, match="incompatible shapes"):
        ops.selfattn_core(q, q, q, am, H, 2)
    with pytest.raises(ValueError, match=r"\(H\+2\*Hkv\)\*D"):
        ops.selfattn_core_fused(torch.randn(B, T, 3 * H * D + 1), am, H, 2)
