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

`T5HipRunner.generate` is the same module's cached decoding: `encode`, the encoder's keys and values projected once per
decoder layer, then one decoder step per new token on the decode kernels -- `ops.decode_linear`, `ops.attn_decode_relbias` over the
tokens so far, `ops.attn_decode` over the encoder's keys -- through the one loop of generation.py.
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

    # ------------------------------------------------------------------------------------------ generation
    def _encoder_inputs(self, input_ids, inputs_embeds, attention_mask):
        m = self.model
        if (input_ids is None) == (inputs_embeds is None):
            raise ValueError("You must specify exactly one of input_ids or inputs_embeds")
        h = m.shared(input_ids) if inputs_embeds is None else inputs_embeds.to(m.shared.weight.dtype)
        B, S = h.shape[:2]
        enc_valid = None if attention_mask is None else (attention_mask != 0)
        if enc_valid is not None and tuple(enc_valid.shape) != (B, S):
            raise ValueError(f"Attention mask should be of size {(B, S)}, but is {tuple(enc_valid.shape)}")
        return h.contiguous(), enc_valid

    def encode(self, input_ids=None, inputs_embeds=None, attention_mask=None):
        """The encoder half of __call__: the last hidden state [B, S, d_model] of the encoder stack under attention_mask."""
        h, enc_valid = self._encoder_inputs(input_ids, inputs_embeds, attention_mask)
        return self._stack(self.model.encoder, h, enc_valid)

    def _kv_weights(self):
        """Per decoder layer the concatenated [k; v] weights [2 inner, d_model] of SelfAttention and of EncDecAttention, built once per
        runner and again when a weight changed (its data pointer, _version, dtype or device: the key of decode_cache.WeightCodes)."""
        atts = [(blk.layer[0].SelfAttention, blk.layer[1].EncDecAttention) for blk in self.model.decoder.block]
        key = tuple((w.data_ptr(), w._version, w.dtype, w.device) for sa, ca in atts for w in (sa.k.weight, sa.v.weight, ca.k.weight, ca.v.weight))
        hit = self.__dict__.get("_kv_cat")
        if hit is None or hit[0] != key:
            cat = lambda a: torch.cat((a.k.weight.detach(), a.v.weight.detach()), dim=0)
            hit = self.__dict__["_kv_cat"] = (key, [cat(sa) for sa, _ in atts], [cat(ca) for _, ca in atts])
        return hit[1], hit[2]

    def _decode_step(self, tok, cache, w_self):
        """One cached decoder step: tokens [B, 1] -> the final-norm hidden row [B, d_model]; files the token's keys and values at
        column cache.col of every layer and advances it."""
        m = self.model
        cfg = m.config
        eps, H = cfg.layer_norm_epsilon, cfg.num_heads
        h = m.shared(tok[:, 0]).contiguous()
        for l, blk in enumerate(m.decoder.block):
            sa, ca, ff = blk.layer[0], blk.layer[1], blk.layer[2]
            x = ops.rms_norm(h, sa.layer_norm.weight, eps)
            q = ops.decode_linear(x, sa.SelfAttention.q.weight)
            new = ops.decode_linear(x, w_self[l], out=cache.new_kv(l))
            h = ops.decode_linear(cache.attend_self(l, q, new, H), sa.SelfAttention.o.weight, residual=h)
            x = ops.rms_norm(h, ca.layer_norm.weight, eps)
            q = ops.decode_linear(x, ca.EncDecAttention.q.weight)
            h = ops.decode_linear(cache.attend_cross(l, q, H), ca.EncDecAttention.o.weight, residual=h)
            x = ops.rms_norm(h, ff.layer_norm.weight, eps)
            mid = ops.decode_linear(x, ff.DenseReluDense.wi.weight, act="relu")
            h = ops.decode_linear(mid, ff.DenseReluDense.wo.weight, residual=h)
        cache.col += 1
        return ops.rms_norm(h, m.decoder.final_layer_norm.weight, eps)

    def _last_logits(self, hidden):
        cfg = self.model.config
        scale = cfg.d_model ** -0.5 if getattr(cfg, "scale_decoder_outputs", cfg.tie_word_embeddings) else 1.0
        return ops.decode_linear(hidden.contiguous(), self.model.lm_head.weight, out_scale=scale)

    @torch.no_grad()
    def generate(self, input_ids=None, inputs_embeds=None, attention_mask=None, max_new_tokens=32, eos_token_id=None, pad_token_id=None,
                 decoder_start_token_id=None, return_step_logits=False, num_beams=1, num_return_sequences=1, do_sample=False,
                 temperature=1.0, top_k=0, top_p=1.0, seed=None, sample_u=None, repetition_penalty=1.0, no_repeat_ngram_size=0,
                 min_new_tokens=0, suppress_tokens=None):
        """generate(input_ids, attention_mask, max_new_tokens) of a T5 with a key/value cache: the encoder once (encode), per decoder
        layer one GEMM of its output onto the concatenated EncDecAttention [k; v] weight (cache.cross), then max_new_tokens cached
        decoder steps on the skinny GEMMs, ops.attn_decode_relbias over the tokens so far (the bias rows of block 0's table serve every
        layer, as in training) and ops.attn_decode over the encoder's keys under its mask.  The decoder has no prompt: its row is
        decoder_start_token_id (default config.decoder_start_token_id) and then the new tokens, so the result is
        [B, 1 + max_new_tokens] int64 with the start token in column 0 -- what transformers returns for an encoder-decoder.  The loop
        and the semantics of eos_token_id / pad_token_id, do_sample with its knobs, the logits processors (their history is the decoder
        row so far, start token included) and return_step_logits are generation.decode_loop's: see that module.  Refused: num_beams > 1,
        num_return_sequences > 1, CPU tensors."""
        from .decode_cache import DecodeCache
        from .generation import decode_loop, make_select
        from .sampling import check_processors, check_sampling
        who = "T5HipRunner.generate()"
        m = self.model
        cfg = m.config
        if int(num_beams) != 1:
            raise ValueError(f"{who}: num_beams = {num_beams} is not implemented (beam search runs on the OPT fork only); this path is greedy "
                             "or sampled")
        check_sampling(who, do_sample, temperature, top_k, top_p, seed, sample_u, 1, num_return_sequences)
        proc = check_processors(who, repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens, eos_token_id, max_new_tokens,
                                cfg.vocab_size, 1, torch.int64)
        if (input_ids is None) == (inputs_embeds is None):
            raise ValueError("generate() takes exactly one of input_ids and inputs_embeds")
        prompt = input_ids if input_ids is not None else inputs_embeds
        n_new = int(max_new_tokens)
        if n_new < 1:
            raise ValueError(f"max_new_tokens must be positive, got {max_new_tokens}")
        if not prompt.is_cuda:
            raise RuntimeError(f"generate() runs on the GPU only (the prompt is on {prompt.device}); there is no CPU path")
        if prompt.dim() != (2 if input_ids is not None else 3):
            raise ValueError(f"generate(): input_ids [B, T] or inputs_embeds [B, T, d_model], got {tuple(prompt.shape)}")
        start_id = cfg.decoder_start_token_id if decoder_start_token_id is None else decoder_start_token_id
        if start_id is None:
            raise ValueError(f"{who}: decoder_start_token_id is not set (argument or config)")
        if eos_token_id is not None and pad_token_id is None:
            pad_token_id = cfg.pad_token_id
            if pad_token_id is None:
                raise ValueError("generate(): eos_token_id needs a pad_token_id")
        dev, dtype = prompt.device, m.shared.weight.dtype
        if dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"{who}: the model is {dtype}; the decode kernels take bfloat16 or float32")
        B = prompt.shape[0]
        if proc is not None:
            proc.upload(dev)                                   # in front of the prefill: see LogitsProcessors
        select = make_select(who, do_sample, n_new, B, 1, dev, seed, sample_u, temperature, top_k, top_p, eos_token_id, pad_token_id)
        T5HipRunner.calls += 1
        # prefill: the encoder, then every layer's keys and values of its output
        h, enc_valid = self._encoder_inputs(input_ids, inputs_embeds, attention_mask)
        enc = self._stack(m.encoder, h, enc_valid)
        w_self, w_cross = self._kv_weights()
        inner = cfg.num_heads * cfg.d_kv
        cache = DecodeCache(len(m.decoder.block), B, n_new, inner, dtype, dev)
        for w in w_cross:
            kv = ops.linear(enc, w)                            # [B, S_enc, 2 inner]: the two column slabs are the layer's k and v
            cache.cross.append((kv[:, :, :inner], kv[:, :, inner:]))
        cache.cross_valid = torch.ones(enc.shape[:2], dtype=torch.uint8, device=dev) if enc_valid is None else enc_valid
        table = m.decoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
        cache.rel_bias = ops.t5_decode_bias(table, n_new, cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance)
        start = torch.full((B, 1), int(start_id), dtype=torch.int64, device=dev)
        hidden = self._decode_step(start, cache, w_self)
        return decode_loop(self._last_logits, lambda tok: self._decode_step(tok, cache, w_self), hidden, select, n_new, start,
                           proc=proc, return_step_logits=return_step_logits)

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
