"""-m gpu: the Llama variant with grouped-query attention (num_key_value_heads < num_attention_heads), after tests/test_llama_gpu.py:
gates = 0 => logits == the frozen HF LlamaForCausalLM (fp32, CPU; HF's own repeat_kv);  gates != 0 => the CPU oracle block
(oracle/llama_ref.py, which runs HF's attention);  one bf16 model whose shapes reach the 32x32 MFMA attention kernels;  a bf16
training step through CrossAttentionModel."""
import copy

import pytest
import torch

from helpers import assert_close, mpt_args, rel_err, tiny_clip_vision_config, tiny_roberta_config

pytestmark = pytest.mark.gpu

BF16_LOGITS_TOL = 2.5e-2          # tests/test_generate_gpu.py: the project's bound on bf16 logits against an fp32 reference


def _tiny_llama(n_kv):
    from transformers import LlamaConfig
    return LlamaConfig(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=4, num_attention_heads=4,
                       num_key_value_heads=n_kv, max_position_embeddings=256, pad_token_id=1, bos_token_id=2, eos_token_id=2,
                       attention_dropout=0.0)


def _batch(B=2, T=24, S=10, d=64, seed=0, vocab=128):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab, (B, T), generator=g)
    am = torch.ones(B, T, dtype=torch.long)
    am[1, T - 6:] = 0
    ne = torch.randn(B, S, d, generator=g)
    valid = torch.ones(B, S, dtype=torch.bool)
    valid[0, 6:] = False
    valid[1, 1::3] = False
    return ids, am, ne, valid


def _build(cfg, wise=2):
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    torch.manual_seed(0)
    return LlamaNeighborLM(mpt_args(model_name_or_path="llama-tiny", neighbor_layer_wise=wise), cfg)


def _open_gates(lm, hidden):
    with torch.no_grad():
        for i, layer in enumerate(lm.neighbor_layers):
            layer.gating1.fill_(0.5 + 0.1 * i)
            layer.gating2.fill_(-0.3 - 0.1 * i)
            layer.input_layernorm.add_(0.1 * torch.randn(hidden))


@pytest.mark.parametrize("n_kv", [2, 1])
def test_llama_gqa_gates_zero_equals_hf_llama(n_kv):
    lm = _build(_tiny_llama(n_kv))
    hf = copy.deepcopy(lm.llama).float().eval()
    ids, am, ne, valid = _batch()
    with torch.no_grad():
        want = hf(input_ids=ids, attention_mask=am).logits
        got = lm.cuda().eval()(input_ids=ids.cuda(), attention_mask=am.cuda(), labels=ids.cuda(), neighbor_embeds=ne.cuda(),
                               neighbor_attention_mask=valid.cuda()).logits
    assert_close(got, want, 1e-3, f"Hkv={n_kv}: gates=0 logits vs HF Llama")


@pytest.mark.parametrize("n_kv", [2, 1])
def test_llama_gqa_gated_block_vs_oracle_fwd_bwd(n_kv):
    from oracle import llama_ref
    lm = _build(_tiny_llama(n_kv))
    _open_gates(lm, 64)
    hf = copy.deepcopy(lm.llama).float().eval()
    p = {k: v.detach().clone().float().requires_grad_() for k, v in lm.state_dict().items() if k.startswith("neighbor_layers.")}
    ids, am, ne, valid = _batch(seed=3)
    logits, loss = llama_ref.llama_neighbor_lm_forward(hf, p, 2, ids, am, ids, ne, valid)
    loss.backward()
    lm = lm.cuda().eval()
    out = lm(input_ids=ids.cuda(), attention_mask=am.cuda(), labels=ids.cuda(), neighbor_embeds=ne.cuda(), neighbor_attention_mask=valid.cuda())
    assert_close(out.logits, logits, 1e-3, "logits")
    assert_close(out.loss, loss, 1e-3, "loss")
    out.loss.backward()
    trainable = {k for k, q in lm.named_parameters() if q.requires_grad}
    assert trainable == {k for k in p}, "only the gated layers are trainable"
    for k, q in lm.named_parameters():
        if q.requires_grad:
            assert_close(q.grad, p[k].grad, 2e-3, f"d {k}")


def test_llama_gqa_bf16_reaches_the_mfma32_attention_route():
    """hidden 256, H = 4, Hkv = 2 (D = 64), T = 136: bf16 with head_dim 64 is the route of the 32x32 MFMA kernels, two query blocks and
    a ragged second key block.  Logits against the fp32 CPU oracle of the same (bf16-rounded) weights, gates open."""
    from transformers import LlamaConfig
    from oracle import llama_ref
    H, Hkv, D, hidden, T, S = 4, 2, 64, 256, 136, 10
    cfg = LlamaConfig(vocab_size=128, hidden_size=hidden, intermediate_size=512, num_hidden_layers=2, num_attention_heads=H,
                      num_key_value_heads=Hkv, max_position_embeddings=256, pad_token_id=1, bos_token_id=2, eos_token_id=2,
                      attention_dropout=0.0)
    lm = _build(cfg, wise=1)
    _open_gates(lm, hidden)
    lm = lm.bfloat16()
    ids, am, ne, valid = _batch(T=T, S=S, d=hidden, seed=5)
    am[1, T - 6:] = 1
    am[1, T - 40:] = 0
    ne = ne.bfloat16()
    hf = copy.deepcopy(lm.llama).float().eval()
    hf.model.rotary_emb.inv_freq.copy_(lm._inv_freq)        # the bf16 cast rounded HF's frequency buffer too (see LlamaNeighborLM.__init__)
    p = {k: v.detach().clone().float() for k, v in lm.state_dict().items() if k.startswith("neighbor_layers.")}
    with torch.no_grad():
        want, _ = llama_ref.llama_neighbor_lm_forward(hf, p, 1, ids, am, ids, ne.float(), valid)

    def run(model):
        model = model.cuda().eval()
        with torch.no_grad():
            return model(input_ids=ids.cuda(), attention_mask=am.cuda(), neighbor_embeds=ne.cuda(), neighbor_attention_mask=valid.cuda()).logits.float().cpu()

    # for the record: the same model with the K / V weights expanded to multi-head (the route that existed before)
    G = H // Hkv
    cfg_mha = copy.deepcopy(cfg)
    cfg_mha.num_key_value_heads = H
    mha = _build(cfg_mha, wise=1).bfloat16()
    sd = {k: v.clone() for k, v in lm.state_dict().items()}
    for k in list(sd):
        if k.endswith("self_attn.k_proj.weight") and k.startswith("llama.") or k.endswith("self_attn.v_proj.weight") and k.startswith("llama."):
            sd[k] = sd[k].reshape(Hkv, D, hidden).repeat_interleave(G, dim=0).reshape(H * D, hidden)
    mha.load_state_dict(sd)
    mha._inv_freq = lm._inv_freq.clone()
    keep = am.bool()
    got, got_mha = run(lm), run(mha)
    e, e_mha = rel_err(got[keep], want[keep]), rel_err(got_mha[keep], want[keep])
    print(f"[llama gqa bf16] logits vs fp32 oracle: grouped-query {e:.3e}, K/V weights expanded to multi-head {e_mha:.3e} (bound {BF16_LOGITS_TOL})")
    assert torch.isfinite(got).all()
    assert e <= BF16_LOGITS_TOL, e


def test_cross_attention_model_trains_a_gqa_llama_bf16():
    from mmgl_amd.model import CrossAttentionModel
    from mmgl_amd.model.modelling_llama_cross_attention import LlamaNeighborLM
    w = CrossAttentionModel(mpt_args(model_name_or_path="llama-tiny", context="text_only", neighbor_layer_wise=2), None,
                            lm_config=_tiny_llama(2), text_config=tiny_roberta_config(), visual_config=tiny_clip_vision_config())
    assert isinstance(w.lm, LlamaNeighborLM) and w.lm._frozen[0].Hkv == 2
    w = w.cuda().bfloat16().train()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, 128, (2, 24), generator=g).cuda()
    am = torch.ones(2, 24, dtype=torch.long).cuda()
    nids = torch.randint(3, 128, (2, 3, 12), generator=g).cuda()
    nam = torch.ones(2, 3, 12, dtype=torch.long).cuda()
    npos = torch.tensor([[1, 2, 0], [1, 0, 0]]).cuda()
    out = w(input_ids=ids, attention_mask=am, labels=ids, neighbor_input_ids=nids, neighbor_attention_mask=nam, neighbor_pos_ids=npos)
    out.loss.backward()
    assert torch.isfinite(out.loss)
    # inside the language model only the gated layers have gradients (the wrapper's own neighbor-embedding projections train too)
    with_grad = {n for n, p in w.lm.named_parameters() if p.grad is not None}
    gated = {n for n, _ in w.lm.named_parameters() if n.startswith("neighbor_layers.")}
    assert gated and with_grad == gated, sorted(with_grad ^ gated)[:8]
    assert all(torch.isfinite(p.grad).all() for n, p in w.lm.named_parameters() if p.grad is not None)
    assert not any(p.requires_grad for p in w.lm.llama.parameters())
