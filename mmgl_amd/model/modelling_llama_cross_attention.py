"""Llama-family variant of the gated neighbor cross-attention LM (BASELINE.json configs[4]: Llama-2-7B decoder,
flamingo, 32 neighbors).  The reference's fork is OPT-specific (learned positions, LayerNorm, ReLU FFN, biases --
model/modelling_cross_attention.py:278-375); this is the same Flamingo-style block in Llama's conventions -- RMSNorm
pre-norm, bias-free projections, SwiGLU FFN, scalar tanh gates initialised at 0 -- inserted after every
`neighbor_layer_wise`-th layer of a frozen LlamaForCausalLM.  The HF object is loaded through the same HF API and owns the
weights (state-dict keys `llama.*`); its forward is replaced by the HIP path: RMSNorm kernel, ONE fused q|k|v GEMM
(ping-pong MFMA kernel, D^-1/2 folded into the q rows), rotary embedding in place on that buffer, causal flash attention
reading Q/K/V in place (multi-head or grouped-query: num_key_value_heads <= num_attention_heads, query head h reads key / value
head h // G as in transformers' repeat_kv), ONE fused gate|up GEMM + SwiGLU kernel, down projection; dgrads against cached W^T copies.
No reference counterpart exists: parity is UNPINNED vs MMGL; it is pinned (tests/test_llama_gpu.py) to HF Llama itself
when the gates are 0 and to the CPU oracle (oracle/llama_ref.py) otherwise.
Greedy generation (LlamaNeighborLM.generate) keeps a cache of the Hkv key/value heads only -- rows [B, capacity, 2*Hkv*D] -- and runs
each new token on the decode kernels: one skinny GEMM on the fused q|k|v weight, ops.rope_kv_append (q rotated in place, k rotated and
v copied into the token's cache column), ops.attn_decode with num_kv_heads (one read of a cached key serves its G query heads),
residual adds in the GEMM epilogues.  The new token's position is its COLUMN, as in forward() and in HF's default position_ids.
generate(kv_cache_dtype="fp8") keeps those Hkv heads as e4m3fn codes with one power-of-two scale per (sample, column, key-or-value,
kv head): the prefill files the prompt with one ops.kv_quantize launch per layer, a step rotates k|v into the cache's dense kv_new row
and ops.attn_decode_q8 with num_kv_heads reads the codes, counts the new row unquantised and files it.
Prompt-lookup decoding (generate(prompt_lookup_num_tokens=K)) verifies K drafted tokens per step: B*(K+1) rows through the same
GEMMs, ops.rope_kv_append_block (the position of row (b, i) is its column len[b] + i, per sample and on the device) and
ops.attn_decode_gqa_block (causal over the Hkv-head cache); the loop and the accept kernel are the OPT fork's.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from transformers.modeling_outputs import CausalLMOutputWithPast

from .. import ops
from .decode_cache import DecodeCache, LookupState, StepCodes
from .generation import check_prompt, decode_loop, lookup_loop, make_select
from .sampling import check_kv_cache, check_lookup, check_processors, check_sampling, check_weight_dtype


class LlamaGatedCrossAttentionLayer(nn.Module):
    def __init__(self, hidden_size, num_heads, intermediate_size, rms_norm_eps=1e-6, dropout=0.0):
        super().__init__()
        if hidden_size % num_heads:
            raise ValueError(f"embed_dim must be divisible by num_heads (got `embed_dim`: {hidden_size} and `num_heads`: {num_heads}).")
        self.num_heads, self.head_dim, self.eps, self.dropout = num_heads, hidden_size // num_heads, rms_norm_eps, dropout
        self.input_layernorm = nn.Parameter(torch.ones(hidden_size))
        self.post_attention_layernorm = nn.Parameter(torch.ones(hidden_size))
        self.q_proj = nn.Linear(hidden_size, hidden_size, bias=False)
        self.k_proj = nn.Linear(hidden_size, hidden_size, bias=False)
        self.v_proj = nn.Linear(hidden_size, hidden_size, bias=False)
        self.o_proj = nn.Linear(hidden_size, hidden_size, bias=False)
        self.gate_proj = nn.Linear(hidden_size, intermediate_size, bias=False)
        self.up_proj = nn.Linear(hidden_size, intermediate_size, bias=False)
        self.down_proj = nn.Linear(intermediate_size, hidden_size, bias=False)
        self.gating1 = nn.Parameter(torch.tensor(0.0))
        self.gating2 = nn.Parameter(torch.tensor(0.0))

    def forward(self, hidden_states, neighbor_embeds, key_valid, kv_out=None):
        h = hidden_states
        x = ops.rms_norm(h, self.input_layernorm, self.eps)
        q = ops.linear(x, self.q_proj.weight, None, out_scale=self.head_dim ** -0.5)
        k = ops.linear(neighbor_embeds, self.k_proj.weight, None)
        v = ops.linear(neighbor_embeds, self.v_proj.weight, None)
        if kv_out is not None:               # prefill of generate(): the projected neighbor tokens are constant over the decode steps
            kv_out.append((k, v))
        a = ops.linear(ops.xattn_core(q, k, v, key_valid, self.num_heads), self.o_proj.weight, None)
        h = ops.gated_residual(h, a, self.gating1, self.dropout, self.training)
        x = ops.rms_norm(h, self.post_attention_layernorm, self.eps)
        # gate and up are separate trainable parameters (state-dict names of LlamaMLP): their WEIGHTS are concatenated per call (180 MB
        # at 7B dims) so that one GEMM writes the [gate | up] buffer the SwiGLU kernel reads and one dgrad / one wgrad GEMM run backward --
        # concatenating the two activations cost 1.5 GB of traffic per layer and a contiguous copy of each gradient half
        gu = ops.linear(x, torch.cat([self.gate_proj.weight, self.up_proj.weight], dim=0), None)
        m = ops.linear(ops.swiglu(gu), self.down_proj.weight, None)
        return ops.gated_residual(h, m, self.gating2, self.dropout, self.training)

    def decode_step(self, h, cache, k):
        """The layer on the rows of a decode or verify step, h [rows, hidden], against the neighbor keys and values projected at the
        prefill (cache.cross[k], at B rows in every mode: DecodeCache.attend_cross) with cache.cross_gu[k], the [gate | up] weight
        concatenated once per generation."""
        x = ops.rms_norm(h, self.input_layernorm, self.eps)
        q = ops.decode_linear(x, self.q_proj.weight, None, out_scale=self.head_dim ** -0.5)
        a = ops.decode_linear(cache.attend_cross(k, q, self.num_heads), self.o_proj.weight, None)
        h = ops.gated_residual(h, a, self.gating1, 0.0, False)
        x = ops.rms_norm(h, self.post_attention_layernorm, self.eps)
        m = ops.decode_linear(ops.swiglu(ops.decode_linear(x, cache.cross_gu[k], None)), self.down_proj.weight, None)
        return ops.gated_residual(h, m, self.gating2, 0.0, False)


class _FrozenLlamaLayer:
    """Functional forward of one frozen HF LlamaDecoderLayer on the HIP kernels (derived fused weights are cached copies; the
    module's own parameters and state_dict stay as loaded)."""

    def __init__(self, layer, cfg):
        self.layer, self.cfg = layer, cfg
        self.H = cfg.num_attention_heads
        self.Hkv = getattr(cfg, "num_key_value_heads", None) or self.H      # < H: grouped-query attention (Hkv = 1: multi-query)
        self.D = getattr(cfg, "head_dim", None) or cfg.hidden_size // self.H
        self._cache = None

    def _fused(self):
        at, mlp = self.layer.self_attn, self.layer.mlp
        ps = (at.q_proj.weight, at.k_proj.weight, at.v_proj.weight, mlp.gate_proj.weight, mlp.up_proj.weight)
        key = tuple((p.data_ptr(), p._version, p.dtype, p.device) for p in ps)
        if self._cache is None or self._cache[0] != key:
            with torch.no_grad():
                qkv = torch.cat([ps[0].float() * self.D ** -0.5, ps[1].float(), ps[2].float()], 0).to(ps[0].dtype).contiguous()
                gu = torch.cat([ps[3], ps[4]], 0).contiguous()
            self._cache = (key, qkv, gu)
        return self._cache[1], self._cache[2]

    def __call__(self, h, pending, key_valid, cos_sin, kv_out=None):
        """(h, pending) -> (h', pending'): the residual stream and the MLP output NOT yet added to it -- the add runs inside the
        RMSNorm kernel of whoever consumes the sum next (this layer's successor, the final norm), forward and backward.
        kv_out: the layer's [B, capacity, 2*Hkv*D] rows of a DecodeCache -- the prefill copies its rotated keys and its values there --
        or the (codes, scale) pair of an FP8 cache (DecodeCache.kv_out), which one ops.kv_quantize launch fills instead of the copy."""
        ly, eps = self.layer, self.cfg.rms_norm_eps
        w_qkv, w_gu = self._fused()
        if pending is None:
            x = ops.rms_norm(h, ly.input_layernorm.weight, eps)
        else:
            h, x = ops.add_rms_norm_pair(pending, h, ly.input_layernorm.weight, eps)
        # w_qkv is [(H + 2 Hkv) * D, hidden]: the HF q | k | v weights as loaded, so k and v come out with Hkv heads
        qkv = ops.rope_qk_(ops.frozen_linear(x, w_qkv, None), cos_sin, self.H, self.Hkv)
        if isinstance(kv_out, tuple):
            nq, nkv = self.H * self.D, self.Hkv * self.D
            ops.kv_quantize(qkv[:, :, nq:nq + nkv], qkv[:, :, nq + nkv:], kv_out[0], kv_out[1], self.Hkv)
        elif kv_out is not None:
            kv_out[:, :qkv.shape[1]].copy_(qkv[:, :, self.H * self.D:])
        a = ops.frozen_linear(ops.selfattn_core_fused(qkv, key_valid, self.H, self.Hkv), ly.self_attn.o_proj.weight, None)
        h, x = ops.add_rms_norm_pair(a, h, ly.post_attention_layernorm.weight, eps)
        m = ops.frozen_linear(ops.swiglu(ops.frozen_linear(x, w_gu, None)), ly.mlp.down_proj.weight, None)
        return h, m

    def decode_step(self, h, cache, l):
        """The layer on the rows of a decode or verify step, h [rows, hidden] -> [rows, hidden]: the rows' q|k|v from one skinny GEMM
        (per 64 rows) on w_qkv, rotated and filed by one kernel, the attention over layer l's Hkv-head cache, both residual adds in
        GEMM epilogues.  Where the keys go, at which rotary positions, and which attention op reads them is the cache's mode
        (decode_cache.DecodeCache: file_rotated, attend_self); every mode makes the launches of the plain step."""
        ly, eps = self.layer, self.cfg.rms_norm_eps
        w_qkv, w_gu = self._fused()
        if cache.w8 is None:
            mm = lambda name, w, x, residual=None: ops.decode_linear(x, w, None, residual=residual)
        else:                                 # the four GEMMs on codes: only the kernel differs
            fused = self._cache[0]            # the fused copies follow their sources: so do their codes
            mm = lambda name, w, x, residual=None: ops.decode_linear_w8(
                x, *cache.w8.get(self, name, w, fused if name in ("w_qkv", "w_gu") else None), residual=residual)
        x = ops.rms_norm(h, ly.input_layernorm.weight, eps)
        qkv = mm("w_qkv", w_qkv, x)
        new = cache.file_rotated(l, qkv, self.H, self.Hkv)
        a = cache.attend_self(l, qkv[:, :self.H * self.D], new, self.H, self.Hkv)
        h = mm("o_proj", ly.self_attn.o_proj.weight, a, h)
        x = ops.rms_norm(h, ly.post_attention_layernorm.weight, eps)
        return mm("down_proj", ly.mlp.down_proj.weight, ops.swiglu(mm("w_gu", w_gu, x)), h)


class LlamaNeighborLM(nn.Module):
    """Frozen LlamaForCausalLM (HF loading API, weights owned by the HF module) + trainable gated cross-attention layers;
    same call contract as MPTForCausalLM."""

    def __init__(self, args, llama_config=None):
        super().__init__()
        from transformers import AutoConfig, AutoModelForCausalLM, LlamaForCausalLM
        if llama_config is not None:
            self.llama = LlamaForCausalLM(llama_config)
        else:
            cfg = AutoConfig.from_pretrained(args.model_name_or_path)
            self.llama = AutoModelForCausalLM.from_pretrained(args.model_name_or_path, config=cfg)
        cfg = self.llama.config
        self.config = cfg
        n_kv = getattr(cfg, "num_key_value_heads", None) or cfg.num_attention_heads
        if n_kv < 1 or cfg.num_attention_heads % n_kv:
            raise ValueError(f"LlamaNeighborLM: num_attention_heads = {cfg.num_attention_heads} must be a multiple of "
                             f"num_key_value_heads = {n_kv}")
        if getattr(cfg, "attention_bias", False) or getattr(cfg, "mlp_bias", False):
            raise ValueError("LlamaNeighborLM: biased projections are not implemented")
        for p in self.llama.parameters():
            p.requires_grad = False
        n_layers = cfg.num_hidden_layers
        wise = getattr(args, "neighbor_layer_wise", None) or max(1, n_layers // max(1, int(getattr(args, "num_neighbor_layers", 4))))
        self.neighbor_layer_wise = int(wise)
        self.neighbor_layers = nn.ModuleList(
            LlamaGatedCrossAttentionLayer(cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size, cfg.rms_norm_eps)
            for l in range(n_layers) if (l + 1) % self.neighbor_layer_wise == 0)
        std = getattr(cfg, "initializer_range", 0.02)
        for m in self.neighbor_layers.modules():
            if isinstance(m, nn.Linear):
                m.weight.data.normal_(mean=0.0, std=std)
        self._frozen = [_FrozenLlamaLayer(layer, cfg) for layer in self.llama.model.layers]
        self._rope = None
        # The rotary frequencies, kept OUT of the module's buffers: `model.bfloat16()` / `.to(torch.bfloat16)` (what run_generation.py
        # does to the whole model, reference :304-307) casts HF's non-persistent `inv_freq` buffer as well, and positions x
        # frequencies rounded to 8 bits are radians off at T = 2176 (a 4-layer model then drifts 6 % per layer from its fp32 self:
        # tests/test_full_size_gpu.py found it).  A plain attribute is not touched by dtype casts.
        self._inv_freq = self.llama.model.rotary_emb.inv_freq.detach().to(torch.float32).clone()

    def get_input_embeddings(self):
        return self.llama.get_input_embeddings()

    def _cos_sin(self, T, device):
        """fp32 [T, D/2, 2] table of (cos, sin) for positions 0..T-1 from the HF rotary module's own inv_freq / scaling."""
        rot = self.llama.model.rotary_emb
        key = (T, device)
        if self._rope is None or self._rope[0] != key:
            inv = self._inv_freq.to(device=device)
            ang = torch.arange(T, device=device, dtype=torch.float32)[:, None] * inv[None, :]
            sc = float(getattr(rot, "attention_scaling", 1.0))
            self._rope = (key, torch.stack([ang.cos() * sc, ang.sin() * sc], dim=-1).contiguous())
        return self._rope[1]

    def forward(self, input_ids=None, attention_mask=None, labels=None, neighbor_embeds=None, neighbor_attention_mask=None,
                first_key_valid=False, return_logits=None, logits_slice=None, use_cache=False, cache_capacity=None, past_key_values=None,
                kv_cache_dtype=None, **kw):
        """use_cache=True: the prefill of greedy generation -- the same kernels as any forward, plus a copy of every frozen layer's
        rotated keys and its values into a DecodeCache with rows [B, capacity, 2*Hkv*D] (capacity `cache_capacity` columns, default
        max_position_embeddings) and of every gated layer's projected neighbor tokens; returned as past_key_values.
        past_key_values=DecodeCache with input_ids [B, 1]: one decode step (see _decode_step), logits [B, 1, V].
        kv_cache_dtype ("fp8" / torch.float8_e4m3fn, with use_cache=True): that cache keeps the frozen layers' keys and values as
        e4m3fn codes [B, capacity, 2*Hkv*D] with int8 exponents [B, capacity, 2*Hkv]; the gated layers' neighbor tokens stay in the
        model's dtype.  A decode step follows its cache."""
        kv_dtype = check_kv_cache("LlamaNeighborLM.forward()", kv_cache_dtype,
                                  projections=() if kv_cache_dtype is None else self._self_attn_projections())
        if kv_dtype is not None and (past_key_values is not None or not use_cache):
            raise ValueError("LlamaNeighborLM.forward(): kv_cache_dtype belongs to the prefill (use_cache=True); a decode step follows its cache")
        if past_key_values is not None:
            if not isinstance(past_key_values, DecodeCache):
                raise ValueError("LlamaNeighborLM: past_key_values must be the DecodeCache of a forward(use_cache=True)")
            if labels is not None:
                raise ValueError("a decode step takes no labels")
            logits = self._last_logits(self._decode_step(input_ids, past_key_values))[:, None]
            return CausalLMOutputWithPast(loss=None, logits=logits, past_key_values=past_key_values)
        hidden, cache = self._hidden(input_ids, attention_mask, neighbor_embeds, neighbor_attention_mask, first_key_valid, use_cache,
                                     cache_capacity, kv_dtype)
        nxt = None
        if labels is not None:
            nxt = torch.full_like(labels, -100)
            nxt[:, :-1] = labels[:, 1:]
        from .modelling_cross_attention import lm_head_loss_and_logits
        loss, logits = lm_head_loss_and_logits(self, self.llama.lm_head, hidden, nxt, return_logits, logits_slice)
        return CausalLMOutputWithPast(loss=loss, logits=logits, past_key_values=cache)

    def _self_attn_projections(self):
        """What check_kv_cache looks at: the q / k / v / o projections of the frozen layers."""
        return [getattr(ly.self_attn, n) for ly in self.llama.model.layers for n in ("q_proj", "k_proj", "v_proj", "o_proj")]

    def _frozen_linears(self):
        """What check_weight_dtype looks at: every linear of the frozen layers."""
        return self._self_attn_projections() + [getattr(ly.mlp, n) for ly in self.llama.model.layers
                                                for n in ("gate_proj", "up_proj", "down_proj")]

    def _hidden(self, input_ids, attention_mask, neighbor_embeds, neighbor_attention_mask, first_key_valid=False, use_cache=False,
                cache_capacity=None, kv_dtype=None):
        """(final-norm hidden states [B, T, hidden], the filled DecodeCache or None).  kv_dtype: None, or ops.KV_FP8 as
        check_kv_cache returned it -- the cache then holds codes and exponents of the Hkv heads (DecodeCache)."""
        emb = self.llama.get_input_embeddings()
        B, T = input_ids.shape
        cache = None
        table = T                                 # rows of the rotary table
        if use_cache:
            if self.training:
                raise ValueError("a decode cache in training mode: generation is deterministic, call eval() first")
            limit = self.config.max_position_embeddings
            capacity = limit if cache_capacity is None else int(cache_capacity)
            if T > capacity or capacity > limit:
                raise ValueError(f"decode cache: a prompt of {T} columns, capacity {capacity}, max_position_embeddings {limit}")
            ops.require_cuda(input_ids)
            fr = self._frozen[0]
            cache = DecodeCache(len(self._frozen), B, capacity, fr.Hkv * fr.D, emb.weight.dtype, input_ids.device, kv_dtype=kv_dtype,
                                num_heads=None if kv_dtype is None else fr.Hkv)
            table = capacity
        h = emb(input_ids)
        if attention_mask is None:
            attention_mask = torch.ones(B, T, dtype=torch.long, device=h.device)
        if not first_key_valid:                   # same precondition (and device-side check) as MPTDecoder.forward
            torch._assert_async((attention_mask[:, 0] != 0).all(), "LlamaNeighborLM: attention_mask[:, 0] must be 1 for every sample")
        key_mask = (attention_mask != 0).to(torch.uint8).contiguous()
        ne = valid = None
        if neighbor_embeds is not None:
            valid = neighbor_attention_mask
            if valid is None:
                valid = torch.ones(neighbor_embeds.shape[:2], dtype=torch.uint8, device=neighbor_embeds.device)
            ne, valid = neighbor_embeds.to(emb.weight.dtype), valid.to(torch.uint8).contiguous()
        # with a cache the table is built once at the cache's capacity: its first T rows are bitwise the table of T positions
        cos_sin = self._cos_sin(table, h.device)[:T]
        k = 0
        pending = None                            # a frozen layer's MLP output, added inside the next RMSNorm kernel
        for l, layer in enumerate(self._frozen):
            h, pending = layer(h, pending, key_mask, cos_sin, None if cache is None else cache.kv_out(l))
            if (l + 1) % self.neighbor_layer_wise == 0:
                if ne is not None:
                    h, pending = ops.gated_residual(h, pending), None
                    h = self.neighbor_layers[k](h, ne, valid, None if cache is None else cache.cross)
                k += 1
        if pending is None:
            hidden = ops.rms_norm(h, self.llama.model.norm.weight, self.config.rms_norm_eps)
        else:
            hidden = ops.add_rms_norm_pair(pending, h, self.llama.model.norm.weight, self.config.rms_norm_eps)[1]
        if cache is not None:
            cache.mask[:, :T] = key_mask
            cache.col = T
            cache.cross_valid = valid if cache.cross else None
            cache.cos_sin = self._cos_sin(table, h.device)
            # the gated layers' [gate | up] weights, concatenated once per generation instead of once per step
            cache.cross_gu = [torch.cat([ly.gate_proj.weight, ly.up_proj.weight], dim=0) for ly in self.neighbor_layers] if cache.cross else []
        return hidden, cache

    def _decode_step(self, input_ids, cache):
        """One new token per sample against the cache, input_ids [B, 1] -> final-norm hidden [B, hidden].  The token is appended at
        column cache.col of every sample and that column is its rotary position: forward() (mmgl_rope_inplace: row r % T) and HF's
        default position_ids count columns, not valid tokens, so cached generation equals the uncached forward on the same ids."""
        if input_ids is None or input_ids.dim() != 2 or input_ids.shape[1] != 1 or input_ids.shape[0] != cache.mask.shape[0]:
            raise ValueError(f"a decode step takes one new token per cached sample ([{cache.mask.shape[0]}, 1]), "
                             f"got {None if input_ids is None else tuple(input_ids.shape)}")
        if cache.cos_sin is None:
            raise ValueError("the DecodeCache has not been filled: run the prompt with use_cache=True first")
        if cache.col >= cache.capacity:
            raise ValueError(f"decode cache is full: column {cache.col} of capacity {cache.capacity}")
        ops.require_cuda(cache.mask, input_ids)
        with torch.no_grad():
            cache.mask[:, cache.col] = 1
            h = self._decode_rows(input_ids[:, 0], cache)
            cache.col += 1
        return h

    def _verify_step(self, cache):
        """A verify step of prompt-lookup decoding: the W = K + 1 tokens cache.lookup.block [B, W] of every sample -- its last token,
        then the drafts -- causally against the sample's lookup.len cache columns.  The layers run at B*W rows and file the block's
        keys and values at columns lookup.len .. lookup.len + W - 1 (below the capacity); which of them count is decided afterwards
        by ops.lookup_accept, which advances lookup.len.  A token's position is its column, so lookup.positions is not read, and
        cache.col stands still at the prompt's width.  Returns the final-norm hidden rows [B*W, hidden]."""
        if cache.lookup is None or cache.cos_sin is None:
            raise ValueError("a verify step needs a prefilled DecodeCache with a LookupState (cache.lookup)")
        ops.require_cuda(cache.mask)
        with torch.no_grad():
            return self._decode_rows(cache.lookup.block.view(-1), cache)

    def _decode_rows(self, tokens, cache):
        """The walk of a decode or verify step: tokens [rows] -> final-norm hidden [rows, hidden] through every frozen layer's
        decode_step, the gated layers interleaved."""
        h = self.llama.get_input_embeddings()(tokens)
        k = 0
        for l, layer in enumerate(self._frozen):
            h = layer.decode_step(h, cache, l)
            if (l + 1) % self.neighbor_layer_wise == 0:
                if cache.cross:
                    h = self.neighbor_layers[k].decode_step(h, cache, k)
                k += 1
        return ops.rms_norm(h, self.llama.model.norm.weight, self.config.rms_norm_eps)

    def _last_logits(self, hidden):
        """lm_head on one row per sample, hidden [B, hidden] (any row stride): the [V, hidden] head is read once for the B rows."""
        head = self.llama.lm_head
        if type(head) is not nn.Linear:
            raise ValueError("generate(): lm_head must be a plain nn.Linear")
        return ops.decode_linear(hidden.contiguous(), head.weight, head.bias)

    def can_generate(self):
        return True

    @torch.no_grad()
    def generate(self, input_ids, attention_mask=None, neighbor_embeds=None, neighbor_attention_mask=None, max_new_tokens=32,
                 eos_token_id=None, pad_token_id=None, return_step_logits=False, first_key_valid=False, num_beams=1,
                 num_return_sequences=1, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=None, sample_u=None,
                 repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=None, **lookup):
        """The contract of MPTForCausalLM.generate for input_ids prompts: one prefill over the right-padded prompts [B, T] -- the
        kernels of forward(), plus the copy of every layer's Hkv key/value heads into a DecodeCache -- then max_new_tokens - 1 decode
        steps; lm_head runs on the last row only.  Every new token is appended at the same column for all samples (its rotary
        position), the pad keys stay masked.  The loop and the semantics of eos_token_id / pad_token_id, do_sample with its knobs,
        the logits processors and return_step_logits are generation.decode_loop's: see that module.  Refused here: num_beams > 1
        (beam search is implemented for the OPT fork only), num_return_sequences > 1 (it needs the beam-shared cache of the OPT
        fork) and do_sample=True on prompts that are not int64.
        **lookup takes exactly five keywords, prompt_lookup_num_tokens=0, max_matching_ngram_size=2, return_lookup_stats=False,
        kv_cache_dtype=None and weight_dtype=None (any other name is the TypeError of an unknown keyword).  They are not named
        parameters: the parameter list above is the greedy and sampled contract, which tests/test_lookup_accept_cpu.py pins by
        inspecting this signature.
        prompt_lookup_num_tokens = K (1..7; 0: off, today's loop) with max_matching_ngram_size = N (1..4): prompt-lookup decoding
        with the keywords, semantics and refusals of MPTForCausalLM.generate -- each step drafts up to K tokens from the row's own
        text and verifies them in one step of B*(K+1) rows (_verify_step, generation.lookup_loop).  The result is the
        greedy result in fewer steps.  return_lookup_stats: also the dict of `steps` and `emitted` lookup_loop describes.
        kv_cache_dtype = "fp8" (or torch.float8_e4m3fn; None: off, every call as without it): the frozen layers keep the Hkv cached
        key/value heads as e4m3fn codes with power-of-two scales, (D + 1) / 2D of the bf16 cache's bytes; the steps read them through
        ops.attn_decode_q8 with num_kv_heads.  Greedy, do_sample, the processors, return_step_logits and EOS handling
        combine with it; prompt_lookup_num_tokens > 0 is refused (the verify kernel has no FP8 form), adapted projections too.
        weight_dtype = "fp8" (or torch.float8_e4m3fn; None: off, every call as without it): the decode and verify steps multiply
        e4m3fn codes of the frozen layers' weights -- the fused q|k|v and gate|up weights, o_proj and down_proj, one power-of-two scale
        per weight row, quantised once on the first such call and kept on the layer until a weight changes -- through
        ops.decode_linear_w8: half the bytes a step streams.  The gated layers, lm_head and the whole prefill keep the
        model's dtype: the prompt's keys come from the exact weights, only the steps run on codes, and the weights stay resident
        beside their codes (N K + N more bytes per weight: this saves bandwidth, not memory).  It is only another GEMM: greedy,
        do_sample, the processors, return_step_logits, EOS handling, kv_cache_dtype and prompt_lookup_num_tokens combine with it;
        adapted (non-nn.Linear) projections are refused."""
        who = "LlamaNeighborLM.generate()"
        prompt_lookup_num_tokens = lookup.pop("prompt_lookup_num_tokens", 0)
        max_matching_ngram_size = lookup.pop("max_matching_ngram_size", 2)
        return_lookup_stats = lookup.pop("return_lookup_stats", False)
        kv_cache_dtype = lookup.pop("kv_cache_dtype", None)
        weight_dtype = lookup.pop("weight_dtype", None)
        if lookup:
            raise TypeError(f"{who} got an unexpected keyword argument '{next(iter(lookup))}'")
        if int(num_beams) != 1:
            raise ValueError(f"{who}: num_beams = {num_beams} is not implemented (beam search runs on the OPT fork only); this path is greedy")
        # num_beams and num_return_sequences keep this model's own refusals (above, and check_sampling's)
        kv_dtype = check_kv_cache(who, kv_cache_dtype, prompt_lookup_num_tokens=prompt_lookup_num_tokens,
                                  projections=() if kv_cache_dtype is None else self._self_attn_projections())
        w8 = check_weight_dtype(who, weight_dtype, () if weight_dtype is None else self._frozen_linears())
        if int(prompt_lookup_num_tokens) != 0:                 # its refusals of do_sample / num_return_sequences come before check_sampling's
            check_lookup(who, prompt_lookup_num_tokens, max_matching_ngram_size, return_lookup_stats, do_sample, 1, num_return_sequences)
        check_sampling(who, do_sample, temperature, top_k, top_p, seed, sample_u, 1, num_return_sequences)
        proc = check_processors(who, repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens, eos_token_id, max_new_tokens,
                                self.config.vocab_size, 1, input_ids.dtype)
        K, N = check_lookup(who, prompt_lookup_num_tokens, max_matching_ngram_size, return_lookup_stats, do_sample, 1, num_return_sequences,
                            proc is not None, return_step_logits)
        if do_sample and input_ids.dtype != torch.int64:
            raise ValueError(f"generate(do_sample=True): input_ids must be int64, got {input_ids.dtype}")
        B, T, n_new, pad_token_id, attention_mask = check_prompt(input_ids, None, attention_mask, max_new_tokens, eos_token_id,
                                                                 pad_token_id, self.config, self.config.max_position_embeddings)
        dev = input_ids.device
        if proc is not None:
            proc.upload(dev)                                   # in front of the prefill: see LogitsProcessors
        select = make_select(who, do_sample, n_new, B, 1, dev, seed, sample_u, temperature, top_k, top_p, eos_token_id, pad_token_id)
        hidden, cache = self._hidden(input_ids, attention_mask, neighbor_embeds, neighbor_attention_mask, first_key_valid, True,
                                     T + n_new - 1, kv_dtype)
        cache.w8 = None if w8 is None else StepCodes()
        if K > 0:
            cache.lookup = LookupState(cache, K, N, n_new, scratch=False)
            return lookup_loop(self._last_logits, lambda: self._verify_step(cache), hidden[:, -1], cache.lookup, input_ids, attention_mask,
                               n_new, eos_token_id, pad_token_id, 0, self.config.max_position_embeddings - 1, return_lookup_stats)
        return decode_loop(self._last_logits, lambda tok: self._decode_step(tok, cache), hidden[:, -1], select, n_new, input_ids,
                           attention_mask, proc=proc, return_step_logits=return_step_logits)
