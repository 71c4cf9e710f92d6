"""Native forward of a HuggingFace T5 (`T5ForConditionalGeneration`) on the HIP kernels.

The HuggingFace module stays the parameter container -- state-dict keys, the tied `shared` / `lm_head` and the two
`relative_attention_bias` tables all stay where HuggingFace has them (the pattern of encoders.PackedTextEncoder); `T5HipRunner`
only replaces its forward for GPU tensors:

  * shared embedding, decoder ids from `model._shift_right(labels)`;
  * per block: `ops.rms_norm` (T5LayerNorm is RMSNorm), q / k / v / o through `ops.linear` (no biases), `ops.attn_relbias`
    (unscaled scores + relative-position bias on the MFMAs; the bias table of block 0 serves every block of its stack and autograd
    sums the per-layer table gradients; the decoder-to-encoder cross-attention runs without a table, under the encoder mask),
    `ops.gated_residual` (residual + dropout), the FFN as `ops.linear(act="relu")`, dropout, `ops.linear`;
  * final norm, the d_model^-0.5 scale of a tied head (folded into the head GEMM's epilogue), `ops.linear` onto the head,
    `ops.cross_entropy(ignore_index=-100)`.
Dropout sits at every place HuggingFace has it (embedding outputs, each sublayer output, the FFN hidden, the final norm outputs, the
attention probabilities) and is inert in eval().  `supports()` names what is covered: the ungated ReLU FFN, d_kv = 64, d_model and
d_ff multiples of 8, plain nn.Linear projections (no LoRA modules).  Everything else stays the stock HuggingFace call.
"""
from types import SimpleNamespace

import torch
import torch.nn as nn

from .. import ops

_HEAD_DIMS = (64,)           # what mmgl_attn_relbias_* serves


def _plain(*mods):
    return all(type(m) is nn.Linear and m.bias is None for m in mods)


class T5HipRunner:
    calls = 0                # forwards served (all instances): lets a test see that the native arm ran

    def __init__(self, model):
        if not T5HipRunner.supports(model):
            raise ValueError(f"{type(model).__name__}: no HIP forward for this T5 variant")
        self.model = model

    @staticmethod
    def supports(model):
        cfg = getattr(model, "config", None)
        if cfg is None or getattr(cfg, "model_type", None) != "t5":
            return False
        if not all(hasattr(model, a) for a in ("shared", "encoder", "decoder", "lm_head", "_shift_right")):
            return False
        if getattr(cfg, "feed_forward_proj", None) != "relu" or getattr(cfg, "is_gated_act", False):
            return False
        if cfg.d_kv not in _HEAD_DIMS or cfg.d_model % 8 or cfg.d_ff % 8:
            return False
        for stack in (model.encoder, model.decoder):
            for i, blk in enumerate(stack.block):
                att = blk.layer[0].SelfAttention
                mods = [att.q, att.k, att.v, att.o]
                if stack is model.decoder:
                    x = blk.layer[1].EncDecAttention
                    mods += [x.q, x.k, x.v, x.o]
                ff = blk.layer[-1].DenseReluDense
                if not (hasattr(ff, "wi") and hasattr(ff, "wo")):
                    return False
                if not _plain(*mods, ff.wi, ff.wo):
                    return False
                if (i == 0) != bool(att.has_relative_attention_bias):
                    return False
        return type(model.lm_head) is nn.Linear and model.lm_head.bias is None

    # ------------------------------------------------------------------------------------------ pieces
    def _drop(self, x):
        """nn.Dropout(dropout_rate) on x: the gated-residual kernel with a zero residual (counter-hash mask, regenerated in backward)."""
        p = self.model.config.dropout_rate
        if not (self.model.training and p > 0.0):
            return x
        return ops.gated_residual(torch.zeros_like(x), x, None, p, True)

    def _attention(self, att, x, kv, key_valid, table, bidirectional, causal):
        cfg = self.model.config
        q = ops.linear(x, att.q.weight)
        k = ops.linear(kv, att.k.weight)
        v = ops.linear(kv, att.v.weight)
        bucket_of = None
        if table is not None:
            bucket_of = ops.t5_bucket_table(x.shape[1], kv.shape[1], bidirectional, cfg.relative_attention_num_buckets,
                                            cfg.relative_attention_max_distance, x.device)
        o = ops.attn_relbias(q, k, v, key_valid, cfg.num_heads, table=table, bucket_of=bucket_of, causal=causal,
                             p_drop=cfg.dropout_rate, training=self.model.training)
        return ops.linear(o, att.o.weight)

    def _residual(self, h, y):
        return ops.gated_residual(h, y, None, self.model.config.dropout_rate, self.model.training)

    def _stack(self, stack, h, key_valid, enc=None, enc_valid=None):
        eps = self.model.config.layer_norm_epsilon
        decoder = enc is not None
        table = stack.block[0].layer[0].SelfAttention.relative_attention_bias.weight
        h = self._drop(h)
        for blk in stack.block:
            sa = blk.layer[0]
            x = ops.rms_norm(h, sa.layer_norm.weight, eps)
            h = self._residual(h, self._attention(sa.SelfAttention, x, x, key_valid, table, not decoder, decoder))
            if decoder:
                ca = blk.layer[1]
                x = ops.rms_norm(h, ca.layer_norm.weight, eps)
                h = self._residual(h, self._attention(ca.EncDecAttention, x, enc, enc_valid, None, True, False))
            ff = blk.layer[-1]
            x = ops.rms_norm(h, ff.layer_norm.weight, eps)
            mid = self._drop(ops.linear(x, ff.DenseReluDense.wi.weight, act="relu"))
            h = self._residual(h, ops.linear(mid, ff.DenseReluDense.wo.weight))
        return self._drop(ops.rms_norm(h, stack.final_layer_norm.weight, eps))

    # ------------------------------------------------------------------------------------------ forward
    def __call__(self, input_ids=None, inputs_embeds=None, attention_mask=None, labels=None):
        m = self.model
        cfg = m.config
        if (input_ids is None) == (inputs_embeds is None):
            raise ValueError("You must specify exactly one of input_ids or inputs_embeds")
        if labels is None:
            raise ValueError("T5HipRunner: the native forward is the training forward and needs labels (decoder ids = shift_right(labels))")
        T5HipRunner.calls += 1
        dtype = m.shared.weight.dtype
        h = m.shared(input_ids) if inputs_embeds is None else inputs_embeds.to(dtype)
        B, S = h.shape[:2]
        enc_valid = None if attention_mask is None else (attention_mask != 0)
        if enc_valid is not None and tuple(enc_valid.shape) != (B, S):
            raise ValueError(f"Attention mask should be of size {(B, S)}, but is {tuple(enc_valid.shape)}")
        enc = self._stack(m.encoder, h.contiguous(), enc_valid)
        dec_in = m.shared(m._shift_right(labels)).contiguous()
        dec = self._stack(m.decoder, dec_in, None, enc, enc_valid)
        scale = cfg.d_model ** -0.5 if getattr(cfg, "scale_decoder_outputs", cfg.tie_word_embeddings) else 1.0
        logits = ops.linear(dec, m.lm_head.weight, out_scale=scale)
        loss = ops.cross_entropy(logits.reshape(-1, logits.shape[-1]), labels.reshape(-1), ignore_index=-100)
        return SimpleNamespace(loss=loss, logits=logits, encoder_last_hidden_state=enc)
