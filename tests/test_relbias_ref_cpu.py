"""relbias_ref.RelBiasRef -- the fp64 reference the GPU bounds of csrc/relbias.hip are held against -- is itself checked here on the CPU:
  * it equals transformers' T5Attention in fp64 for out, dq, dk, dv and the gradient of the bias table, up to fp64 roundoff, as an encoder
    block, a decoder self-attention block and a cross-attention block;
  * each deliberately wrong reference (bias dropped, t - s in place of s - t, offset shifted by one, the other bucket kind, heads swapped)
    leaves the bf16 bound on at least half of the `out` elements: the comparison the GPU tests make can fail."""
import pytest
import torch
from transformers import T5Config
from transformers.models.t5.modeling_t5 import T5Attention

from relbias_ref import RelBiasRef

H, D = 2, 64


def _bucket(T, S, bidirectional, nb=32, md=128):
    return T5Attention._relative_position_bucket(torch.arange(-(T - 1), S), bidirectional=bidirectional, num_buckets=nb, max_distance=md).to(torch.int32)


@pytest.mark.parametrize("kind", ["encoder", "decoder", "cross"])
def test_reference_equals_hf_t5_attention_fp64(kind):
    torch.manual_seed(0)
    B, T = 2, 23
    S = 37 if kind == "cross" else T
    cfg = T5Config(vocab_size=32, d_model=H * D, d_kv=D, d_ff=64, num_layers=1, num_heads=H, dropout_rate=0.0,
                   is_decoder=(kind != "encoder"), decoder_start_token_id=0)
    cfg._attn_implementation = "eager"
    att = T5Attention(cfg, has_relative_attention_bias=(kind != "cross"), layer_idx=0, is_causal=(kind == "decoder")).double().eval()
    with torch.no_grad():
        att.o.weight.copy_(torch.eye(H * D, dtype=torch.float64))
        for lin in (att.q, att.k, att.v):
            lin.weight.normal_(0, (H * D) ** -0.5)
        att.q.weight.mul_(D ** -0.5)
        if kind != "cross":
            att.relative_attention_bias.weight.normal_(0, 1)
    grabbed = {}
    for name in ("q", "k", "v"):
        def hook(_m, _i, out, name=name):
            out.retain_grad()
            grabbed[name] = out
        getattr(att, name).register_forward_hook(hook)
    x = torch.randn(B, T, H * D, dtype=torch.float64)
    enc = torch.randn(B, S, H * D, dtype=torch.float64) if kind == "cross" else None
    key_valid = torch.ones(B, S, dtype=torch.uint8)
    key_valid[1, S - 9:] = 0                                  # one right-padded sample
    allowed = key_valid.bool()[:, None, :].expand(B, T, S)
    if kind == "decoder":
        allowed = allowed & torch.tril(torch.ones(T, S, dtype=torch.bool))[None]
    mask = torch.zeros(B, 1, T, S, dtype=torch.float64).masked_fill(~allowed[:, None], torch.finfo(torch.float64).min)
    out = att(x, mask=mask, key_value_states=enc)[0]
    G = torch.randn_like(out)
    (out * G).sum().backward()

    table = att.relative_attention_bias.weight.detach() if kind != "cross" else None
    ref = RelBiasRef(grabbed["q"].detach(), grabbed["k"].detach(), grabbed["v"].detach(), key_valid, G, H, table=table,
                     bucket_of=None if table is None else _bucket(T, S, kind == "encoder"), causal=(kind == "decoder"))
    tol = 1e-11
    for name, hf in (("out", out.detach()), ("dq", grabbed["q"].grad), ("dk", grabbed["k"].grad), ("dv", grabbed["v"].grad)):
        want = ref.want[name].reshape(hf.shape)
        assert (want - hf).abs().max().item() <= tol * max(1.0, hf.abs().max().item()), name
    if table is not None:
        hf = att.relative_attention_bias.weight.grad
        assert (ref.want["dtable"] - hf).abs().max().item() <= tol * max(1.0, hf.abs().max().item())


def _case(causal):
    T = S = 40
    q, k, v, dout = RelBiasRef.inputs(torch.bfloat16, 2, T, S, H, D, seed=3)
    key_valid = RelBiasRef.mask(2, S, "M1")
    table = torch.randn(32, H, generator=torch.Generator().manual_seed(5))
    return T, S, q, k, v, dout, key_valid, table


@pytest.mark.parametrize("causal", [False, True])
def test_wrong_references_leave_the_bf16_bound(causal):
    T, S, q, k, v, dout, key_valid, table = _case(causal)
    right = _bucket(T, S, not causal)
    ref = RelBiasRef(q, k, v, key_valid, dout, H, table=table, bucket_of=right, causal=causal)
    shifted = torch.cat([right[1:], right[-1:]])
    mutants = {
        "bias dropped": dict(table=None, bucket_of=None),
        "t - s in place of s - t": dict(table=table, bucket_of=right.flip(0).contiguous()),
        "offset shifted by one": dict(table=table, bucket_of=shifted),
        "the other bucket kind": dict(table=table, bucket_of=_bucket(T, S, causal)),
        "heads swapped": dict(table=table[:, [1, 0]].contiguous(), bucket_of=right),
    }
    for name, kw in mutants.items():
        wrong = RelBiasRef(q, k, v, key_valid, dout, H, causal=causal, **kw)
        frac = ref.outside(wrong, "out", torch.bfloat16).double().mean().item()
        print(f"[mutant causal={causal}] {name}: {100 * frac:.1f} % of out outside the bf16 bound")
        assert frac >= 0.5, (name, frac)
