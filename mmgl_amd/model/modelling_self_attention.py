"""Self-attention fusion wrapper: neighbor embeddings are concatenated into the LM's input sequence.

Mirrors reference model/modelling_self_attention.py (constructor, forward kwargs, state-dict names of the
wrapper-level modules).  T5 (config 1) is the stock HuggingFace model on CPU tensors and runs the native forward of t5_hip.py on the
GPU (same module, same parameters); a decoder-only OPT is loaded through
the same HF API and then runs as this build's OPT fork (modelling_cross_attention.MPTForCausalLM without cross-attention
layers, identical state-dict keys) on the HIP kernels.  What else this build owns here:
  * LoRA injection without `peft` (absent in this image, unpinned in the reference's requirements.txt:8):
    q/v projections of every attention block become LoRALinear modules whose forward/backward are the fused
    MFMA kernel `ops.lora_linear` (y = xW^T + b + (alpha/r) (xA^T)B^T), base weights frozen, `lm_head` kept
    trainable (peft's modules_to_save=["lm_head"], reference :80-87).  The reference's target_modules
    ["query","value"] are BERT names that match nothing in OPT/T5; the evident intent
    (q_proj/v_proj for OPT, q/v for T5) is implemented.  Parity vs peft is UNPINNED.
  * prompt tuning (20 virtual tokens, random init) as a learned prefix of input embeddings; prefix tuning of the decoder-only
    OPT as peft's per-layer key/value prefix (a [20, 2 * n_layers * d] table fed to every layer's attention as fixed
    past_key_values: ops.selfattn_core_prefix); for T5 (stock HF model, CPU plumbing) it stays the learned input prefix.
  * the neighbor encoders, interleave scatter (HIP), Laplacian-PE linear and GCN PE exactly as :282-332, with the
    reference's "session" typos read as "section" (SURVEY.md 3.4).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F
from transformers import AutoConfig, AutoModelForCausalLM, AutoModelForSeq2SeqLM, CLIPVisionModel, RobertaModel

from .. import ops
from .encoders import PackedTextEncoder, PackedVisionEncoder
from .graph import GCN
from .modelling_cross_attention import TextPooler
from .sampling import check_processors, check_sampling
from .t5_hip import T5HipRunner

NUM_VIRTUAL_TOKENS = 20


class LoRALinear(nn.Module):
    """Frozen nn.Linear + trainable low-rank update, one fused kernel call (GPU) per forward."""

    def __init__(self, base: nn.Linear, r: int, alpha: float, dropout: float = 0.0):
        super().__init__()
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"lora_dropout must be in [0, 1), got {dropout}")
        self.lora_dropout = float(dropout)          # peft: dropout on the INPUT of the low-rank branch only, in training
        self.base_layer = base
        for p in self.base_layer.parameters():
            p.requires_grad = False
        self.r, self.scaling = r, alpha / r
        self.lora_A = nn.Parameter(torch.empty(r, base.in_features))
        self.lora_B = nn.Parameter(torch.zeros(base.out_features, r))
        nn.init.kaiming_uniform_(self.lora_A, a=math.sqrt(5))

    @property
    def weight(self):
        return self.base_layer.weight

    @property
    def bias(self):
        return self.base_layer.bias

    def forward(self, x, out_scale=1.0):
        """out_scale: a constant factor on the whole output (attention's D^-1/2 on an adapted q_proj), applied in the GEMM epilogues
        instead of a separate pass over [B, T, d]."""
        if self.training and self.lora_dropout > 0.0:
            # lora_dropout > 0 (reference model/modelling_self_attention.py:80-87 -> peft: result = base(x) + B(A(dropout(x))) * scaling;
            # the reference's default is 0.0 and no BASELINE config sets it): the branch sees a dropped copy of x, so the one-call fused
            # kernel (one x for both products) does not apply -- frozen base GEMM + the two skinny GEMMs, all on the HIP kernels;
            # dropout(x) = the gated-residual kernel with a zero residual and no gate (counter-hash mask, regenerated in backward)
            xd = ops.gated_residual(torch.zeros_like(x), x, None, self.lora_dropout, True)
            base = ops.frozen_linear(x, self.base_layer.weight, self.base_layer.bias)
            low = ops.linear(ops.linear(xd, self.lora_A, None), self.lora_B, None)
            y = torch.add(base, low, alpha=self.scaling)
            return y if out_scale == 1.0 else y * out_scale
        return ops.lora_linear(x, self.base_layer.weight, self.base_layer.bias, self.lora_A, self.lora_B, self.scaling, out_scale)

    def decode(self, x, out_scale=1.0, out=None):
        """The layer on the rows of a decode step, x [B, in_features]: ops.decode_lora_linear -- the same function as forward (the
        rank-r term kept apart from the bf16 weight, in fp32), never a merged weight.  `out`: a strided [B, out_features] view."""
        return ops.decode_lora_linear(x, self.base_layer.weight, self.base_layer.bias, self.lora_A, self.lora_B, self.scaling, out_scale, out)


def inject_lora(model: nn.Module, r: int, alpha: float, dropout: float, targets=("q_proj", "v_proj", "q", "v")):
    """Freeze `model`, swap every attention q/v nn.Linear for LoRALinear, keep lm_head trainable.  Returns #swapped."""
    for p in model.parameters():
        p.requires_grad = False
    swapped = 0
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if name in targets and isinstance(child, nn.Linear):
                setattr(parent, name, LoRALinear(child, r, alpha, dropout))
                swapped += 1
    if swapped == 0:
        raise ValueError("LoRA: no target modules (q_proj/v_proj/q/v) found in the base model")
    head = getattr(model, "lm_head", None)
    if head is not None:                       # modules_to_save=["lm_head"]: an untied, trainable copy
        new_head = nn.Linear(head.in_features, head.out_features, bias=head.bias is not None)
        new_head.load_state_dict(head.state_dict())
        model.lm_head = new_head
        if hasattr(model.config, "tie_word_embeddings"):
            model.config.tie_word_embeddings = False
    return swapped


class SelfAttentionModel(nn.Module):
    """SelfAttentionModel(args, tokenizer): T5 (encoder-decoder) or OPT (decoder-only) with neighbor tokens
    concatenated into the sequence (reference :48-335).  `lm_config`/`text_config`/`visual_config` build random-init
    models instead of from_pretrained (synthetic benchmarks / tests)."""

    t5_native = True         # a T5 on the GPU runs t5_hip.T5HipRunner; False selects the stock HuggingFace call (tools/bench_t5.py)

    def __init__(self, args, tokenizer, lm_config=None, text_config=None, visual_config=None):
        super().__init__()
        self.args = args
        self.context = args.context
        self.decoder_only = args.decoder_only
        self.neighbor_mode = args.neighbor_mode
        self.position_type = args.position_type
        self.n_text_tokens = args.n_text_tokens
        self.n_visual_tokens = args.n_visual_tokens
        self.tokenizer = tokenizer

        name = args.model_name_or_path
        if "t5" in name:
            if lm_config is not None:
                model = AutoModelForSeq2SeqLM.from_config(lm_config)
            else:
                model = AutoModelForSeq2SeqLM.from_pretrained(name, config=AutoConfig.from_pretrained(name))
        elif "opt" in name:
            # decoder-only: the same HF loading API (reference :66-72), the weights copied into this build's OPT fork without
            # cross-attention layers (state-dict keys = HF's; fixture G3: fork == HF OPT), so the LM runs on the HIP path --
            # fused-QKV / ping-pong GEMMs, causal flash attention, fused add+LayerNorm, lm_head + token cross-entropy
            from types import SimpleNamespace
            from .modelling_cross_attention import MPTConfig, MPTForCausalLM, copy_opt_weights
            opt_config = lm_config if lm_config is not None else AutoConfig.from_pretrained(name)
            hf = None if lm_config is not None else AutoModelForCausalLM.from_pretrained(name, config=opt_config)
            plain = SimpleNamespace(neighbor_mode="raw", peft_type="none", neighbor_layer_wise=opt_config.num_hidden_layers + 1)
            model = MPTForCausalLM(MPTConfig(plain, opt_config))
            if hf is not None:
                copy_opt_weights(hf, model)
        else:
            raise ValueError(f"SelfAttentionModel does not support {name}.")

        self.prompt_embeddings = None
        self.prefix_encoder = None
        if args.peft_type == "none":
            pass
        elif args.peft_type == "lora":
            inject_lora(model, args.lora_r, args.lora_alpha, args.lora_dropout)
        elif args.peft_type in ("prefix", "prompt"):
            for p in model.parameters():
                p.requires_grad = False
            d = model.get_input_embeddings().embedding_dim
            if args.peft_type == "prefix" and "opt" in name:
                # peft's PrefixEncoder without projection: one table [P, 2 * n_layers * d]; layer i takes columns
                # [2i d, (2i+1) d) as its key prefix and the next d as its value prefix (heads x head_dim inside d), handed
                # to the decoder as a fixed per-layer past_key_values (mmgl_selfattn_prefix_fwd/_bwd)
                n_layers = model.config.num_hidden_layers
                self.prefix_encoder = nn.Embedding(NUM_VIRTUAL_TOKENS, 2 * n_layers * model.config.hidden_size)
            else:
                self.prompt_embeddings = nn.Embedding(NUM_VIRTUAL_TOKENS, d)
        else:
            raise ValueError(f"SelfAttentionModel does not support {args.peft_type}.")
        self.lm = model
        self.input_embeddings = self.lm.get_input_embeddings()
        d_lm = self.input_embeddings.embedding_dim

        self.text_model = None
        if self.neighbor_mode == "embedding":
            embedding_dim = d_lm * args.n_text_tokens
            if text_config is not None:
                self.text_model = RobertaModel(text_config, add_pooling_layer=False)
            else:
                self.text_model = RobertaModel.from_pretrained(args.text_model, config=AutoConfig.from_pretrained(args.text_model))
            self.text_pooler = TextPooler(self.text_model.config)
            self.text_embeddings = nn.Linear(self.text_model.config.hidden_size, embedding_dim)
            if args.position_type != "none":
                self.text_position_embeddings = nn.Embedding(args.max_output_length + 1, embedding_dim)
            self.text_model.eval()
            for p in self.text_model.parameters():
                p.requires_grad = False

        self.visual_model = None
        if self.context in ("section_all", "all"):
            embedding_dim = d_lm * args.n_visual_tokens
            self.visual_model = (CLIPVisionModel(visual_config) if visual_config is not None
                                 else CLIPVisionModel.from_pretrained(args.visual_model))
            self.visual_embeddings = nn.Linear(self.visual_model.config.hidden_size, embedding_dim)
            if args.position_type != "none":
                self.visual_position_embeddings = nn.Embedding(args.max_output_length + 1, embedding_dim)
            self.visual_model.eval()
            for p in self.visual_model.parameters():
                p.requires_grad = False
            from .modelling_cross_attention import _conv_patch_embed_as_gemm
            _conv_patch_embed_as_gemm(self.visual_model)     # CLIP's stride == kernel patch Conv2d as a GEMM (MIOpen falls back to naive_conv)

        if self.position_type == "laplacian":
            if self.context in ("section_only", "section_all", "text_only") or self.neighbor_mode == "raw":
                raise ValueError(f"[Laplacian PE] neighbor mode: {self.neighbor_mode} and context: {self.context} are not supported.")
            k = 1 + args.max_text_neighbors + args.max_image_neighbors - 5
            self.lpe_embeddings = nn.Linear(k, d_lm * args.n_text_tokens)
        if self.position_type == "gnn":
            embedding_dim = d_lm * args.n_text_tokens
            self.gnn = GCN(input_dim=embedding_dim, output_dim=embedding_dim, hidden_dim=self.text_model.config.hidden_size)

        if self.args.freeze_lm:
            print("Freezing the LM.")
            self.lm.eval()
            for p in self.lm.parameters():
                p.requires_grad = False
        else:
            self.lm.train()

    # ------------------------------------------------------------------------------------------ encoders
    def _packed(self, model, cls):
        """Padding-free HIP forward of a frozen encoder (encoders.py) -- the only forward it has here: an architecture `cls` does
        not cover raises (no HuggingFace / library-GEMM forward in the product)."""
        cache = self.__dict__.setdefault("_packed_cache", {})
        if id(model) not in cache:
            if not cls.supports(model):
                raise ValueError(f"{type(model).__name__}: no HIP forward for this encoder architecture ({cls.__name__} does not cover it)")
            cache[id(model)] = cls(model)
        return cache[id(model)]

    def _project(self, pooled, linear, pos_emb, pos_ids, batch_size, n_tokens):
        embs = ops.linear(pooled.to(linear.weight.dtype).contiguous(), linear.weight, linear.bias)
        if pos_emb is not None and pos_ids is not None:
            embs = embs + pos_emb(pos_ids.reshape(-1))
        return embs.reshape(batch_size, -1, n_tokens, embs.shape[-1] // n_tokens)

    def get_text_embs(self, input_ids, attention_mask, pos_ids=None):
        batch_size, neighbor_num, seq_len = input_ids.shape
        ids, am = input_ids.reshape(-1, seq_len), attention_mask.reshape(-1, seq_len)
        with torch.no_grad():
            cls = self._packed(self.text_model, PackedTextEncoder).cls(ids, am)
        pooled = self.text_pooler(cls.unsqueeze(1))
        pos = getattr(self, "text_position_embeddings", None) if self.position_type != "none" else None
        return self._project(pooled, self.text_embeddings, pos, pos_ids, batch_size, self.n_text_tokens)

    def get_visual_embs(self, pixel_values, pos_ids=None):
        batch_size, neighbor_num, pixel, width, height = pixel_values.shape
        with torch.no_grad():
            pv = pixel_values.reshape(-1, pixel, width, height).to(next(self.visual_model.parameters()).dtype)
            pooled = self._packed(self.visual_model, PackedVisionEncoder).pooled(pv)
        pos = getattr(self, "visual_position_embeddings", None) if self.position_type != "none" else None
        return self._project(pooled, self.visual_embeddings, pos, pos_ids, batch_size, self.n_visual_tokens)

    def train(self, mode=True):
        super().train(mode=mode)
        if self.args.freeze_lm:
            self.lm.eval()
        if self.text_model is not None:
            self.text_model.eval()
        if self.visual_model is not None:
            self.visual_model.eval()
        return self

    # ------------------------------------------------------------------------------------------ LM call
    def _lm_inputs(self, input_ids, attention_mask, images=None, image_positions=None, neighbor_input_ids=None,
                   neighbor_attention_mask=None, neighbor_pos_ids=None, text_locations=None, neighbor_images=None,
                   neighbor_images_pos_ids=None, image_locations=None, lpe=None, graph=None):
        """What the LM is fed for a batch, shared by forward and generate: (lm_input, attention_mask).  lm_input is the [B, T] ids
        when the sequence is text alone, else the [B, T', d] input embeddings
            [virtual tokens (prompt tuning) | token embeddings, image tokens scattered in (raw + images) | neighbor tokens (embedding mode)]
        and attention_mask [B, T'] covers the same columns (virtual tokens always valid, padded neighbor slots masked)."""
        input_embs = None
        if self.neighbor_mode == "raw" and self.context in ("section_only", "text_only"):
            pass
        elif self.neighbor_mode == "raw" and self.context in ("section_all", "all"):
            input_embs = self.input_embeddings(input_ids.clamp_min(0)).clone()
            visual_embs = self.get_visual_embs(images)
            B, _, hidden_dim = input_embs.shape
            batch_idx = torch.arange(B, device=input_embs.device)[:, None]
            input_embs[batch_idx, image_positions] = visual_embs.reshape(B, -1, hidden_dim).to(input_embs.dtype)
        else:
            if self.neighbor_mode == "embedding" and self.context in ("section_only", "text_only"):
                text = self.get_text_embs(neighbor_input_ids, neighbor_attention_mask, neighbor_pos_ids)
                B, Nt = text.shape[:2]
                loc = torch.arange(Nt, device=text.device).expand(B, -1).contiguous()
                neighbor_embeds, key_valid = ops.neighbor_interleave(text, None, loc, None, neighbor_pos_ids, None)
            elif self.neighbor_mode == "embedding" and self.context in ("section_all", "all"):
                text = self.get_text_embs(neighbor_input_ids, neighbor_attention_mask, neighbor_pos_ids)
                visual = self.get_visual_embs(neighbor_images, neighbor_images_pos_ids)
                B, Nt, n_tokens, hidden_dim = text.shape
                total = Nt + visual.shape[1]
                neighbor_embeds, key_valid = ops.neighbor_interleave(text, visual, text_locations, image_locations,
                                                                     neighbor_pos_ids, neighbor_images_pos_ids)
                if self.context == "all":
                    if self.position_type == "laplacian":
                        lpe_emb = ops.linear(lpe.to(neighbor_embeds.dtype), self.lpe_embeddings.weight, self.lpe_embeddings.bias)
                        lpe_emb = lpe_emb.reshape(B, total + 1, n_tokens, hidden_dim)
                        neighbor_embeds = neighbor_embeds + lpe_emb[:, 1:].reshape(B, -1, hidden_dim)
                    elif self.position_type == "gnn":
                        flat = neighbor_embeds.reshape(B, total, n_tokens * hidden_dim)
                        neighbor_embeds = (flat + self.gnn(flat, graph)).reshape(B, -1, hidden_dim)
            else:
                raise ValueError(f"Neighbor mode: {self.neighbor_mode} and context: {self.context} are not supported.")
            # neighbors go AFTER the token embeddings (reference :323-325)
            input_embs = torch.cat((self.input_embeddings(input_ids), neighbor_embeds.to(self.input_embeddings.weight.dtype)), dim=1)
            attention_mask = torch.cat((attention_mask, key_valid.to(attention_mask.dtype)), dim=1)
        if self.prompt_embeddings is not None:
            if input_embs is None:
                input_embs = self.input_embeddings(input_ids)
            B = input_embs.shape[0]
            prompt = self.prompt_embeddings.weight.to(input_embs.dtype)[None].expand(B, -1, -1)
            input_embs = torch.cat([prompt, input_embs], dim=1)
            attention_mask = torch.cat([attention_mask.new_ones(B, NUM_VIRTUAL_TOKENS), attention_mask], dim=1)
        return (input_ids if input_embs is None else input_embs), attention_mask

    def _run_lm(self, lm_input, attention_mask, labels=None):
        """lm_input: the ids or the embeddings of _lm_inputs."""
        kw = {}
        opts = getattr(self, "_logit_opts", None)
        if opts and hasattr(self.lm, "model") and "t5" not in self.args.model_name_or_path:
            # the OPT fork: a training step with a frozen head never builds [B, T, V] logits unless asked (lm_head_loss_and_logits)
            rl, sl = opts
            if sl is not None and self.prompt_embeddings is not None:               # virtual tokens sit in front of the sequence
                shift = lambda v: v + NUM_VIRTUAL_TOKENS if (v is not None and v >= 0) else v
                sl = slice(shift(sl.start if sl.start is not None else 0), shift(sl.stop), sl.step)
            kw.update(return_logits=rl, logits_slice=sl)
        if self.prefix_encoder is not None:
            # labels and logits keep the sequence length: the prefix lives in the attention of every layer, not in the sequence
            kw["past_key_values"] = self.prefix_encoder.weight.to(self.input_embeddings.weight.dtype)
        if self.t5_native and lm_input.is_cuda and labels is not None and not kw and "t5" in self.args.model_name_or_path:
            # T5 on the GPU: the native forward over the HuggingFace module (t5_hip.py: relative-position-bias attention and every
            # GEMM on the HIP kernels); a variant it does not cover, CPU tensors and t5_native = False stay the stock call below
            runner = self._t5()
            if runner:
                ids, embeds = (None, lm_input) if lm_input.dim() == 3 else (lm_input, None)
                return runner(input_ids=ids, inputs_embeds=embeds, attention_mask=attention_mask, labels=labels)
        if lm_input.dim() == 3:
            return self.lm(inputs_embeds=lm_input, attention_mask=attention_mask, labels=labels, **kw)
        return self.lm(input_ids=lm_input, attention_mask=attention_mask, labels=labels, **kw)

    def forward(self, input_ids, attention_mask, labels, images=None, image_positions=None, neighbor_input_ids=None,
                neighbor_attention_mask=None, neighbor_pos_ids=None, text_locations=None, neighbor_images=None,
                neighbor_images_pos_ids=None, image_locations=None, lpe=None, graph=None, host_meta=None, return_logits=None,
                logits_slice=None):
        # return_logits / logits_slice: see modelling_cross_attention.lm_head_loss_and_logits (decoder-only OPT fork only)
        self._logit_opts = (return_logits, logits_slice) if (return_logits is not None or logits_slice is not None) else None
        # host_meta (optional, see modelling_cross_attention.host_metadata): accepted for a uniform trainer call; this wrapper
        # encodes every neighbor slot (the concatenated sequence keeps padded slots as masked keys), so it has no use for it
        lm_input, lm_mask = self._lm_inputs(input_ids, attention_mask, images, image_positions, neighbor_input_ids, neighbor_attention_mask,
                                            neighbor_pos_ids, text_locations, neighbor_images, neighbor_images_pos_ids, image_locations,
                                            lpe, graph)
        if self.decoder_only and labels is not None:
            # labels follow the layout of _lm_inputs: -100 on image tokens, on the neighbor tokens behind the text (reference :327-330)
            # and on the virtual tokens in front of it
            if self.neighbor_mode == "raw" and self.context in ("section_all", "all"):
                labels = labels.clone()
                labels[torch.arange(labels.shape[0], device=labels.device)[:, None], image_positions] = -100
            front = NUM_VIRTUAL_TOKENS if self.prompt_embeddings is not None else 0
            back = lm_mask.shape[1] - front - labels.shape[1]
            if back:
                labels = torch.cat((labels, labels.new_full((labels.shape[0], back), -100)), dim=1)
            if front:
                labels = torch.cat([labels.new_full((labels.shape[0], front), -100), labels], dim=1)
        return self._run_lm(lm_input, lm_mask, labels)

    def can_generate(self):
        """Whether generate() exists for this wrapper: the decoder-only OPT fork without adapters, with LoRA or with prompt tuning.
        Not T5 (the stock HuggingFace model) and not OPT prefix tuning (a key/value prefix has no decode cache)."""
        from .modelling_cross_attention import MPTForCausalLM
        return isinstance(self.lm, MPTForCausalLM) and self.args.peft_type in ("none", "lora", "prompt")

    def can_generate_seq2seq(self):
        """Whether generate() runs the cached T5 decoding of t5_hip.T5HipRunner.generate: the LM is a T5 variant its supports()
        covers (can_generate() stays False over a T5: the trainer's default test protocol is unchanged).  Decided from the module
        alone, without touching the device."""
        return self.prefix_encoder is None and bool(T5HipRunner.supports(self.lm))

    def _t5(self):
        runner = self.__dict__.get("_t5_runner")
        if runner is None:                   # decided once: the architecture is fixed at construction (False: not covered)
            runner = self.__dict__["_t5_runner"] = T5HipRunner(self.lm) if T5HipRunner.supports(self.lm) else False
        return runner

    @torch.no_grad()
    def generate(self, input_ids, attention_mask, images=None, image_positions=None, neighbor_input_ids=None,
                 neighbor_attention_mask=None, neighbor_pos_ids=None, text_locations=None, neighbor_images=None,
                 neighbor_images_pos_ids=None, image_locations=None, lpe=None, graph=None, host_meta=None, max_new_tokens=32,
                 eos_token_id=None, pad_token_id=None, return_step_logits=False, num_beams=1, num_return_sequences=1, do_sample=False,
                 temperature=1.0, top_k=0, top_p=1.0, seed=None, sample_u=None, repetition_penalty=1.0, no_repeat_ngram_size=0,
                 min_new_tokens=0, suppress_tokens=None):
        """Greedy generation from the prompt `input_ids` [B, T] (right-padded).  The LM input is built exactly as forward builds it
        (_lm_inputs), then MPTForCausalLM.generate runs the prefill and the cached decode steps (LoRA-adapted q / v projections on
        ops.decode_lora_linear).  New tokens are appended behind the whole LM input:
            [virtual tokens | prompt, image tokens scattered in | neighbor tokens | new tokens ...]
        so in embedding mode they follow the neighbor tokens and see them; padded neighbor slots stay masked keys, and position ids
        count the valid keys, as the cache does.  Returns [B, T + max_new_tokens] ids -- input_ids followed by the new tokens -- and the
        [B, max_new_tokens, V] step logits with return_step_logits=True.  num_beams > 1 is refused: beam search takes input_ids
        prompts and plain projections (CrossAttentionModel / MPTForCausalLM), this wrapper generates from embeddings.
        do_sample, temperature, top_k, top_p, seed and sample_u are MPTForCausalLM.generate's sampling keywords, passed through;
        num_return_sequences > 1 is refused for the same reason as beams.  So are its logits processors repetition_penalty,
        no_repeat_ngram_size, min_new_tokens and suppress_tokens; in either mode their history is the returned row so far, input_ids
        without the masked columns and then the new tokens (embedding mode hands input_ids / attention_mask over as history_ids /
        history_mask: virtual, image and neighbor tokens are no part of it).
        Over a T5 (can_generate_seq2seq()) the same call runs T5HipRunner.generate on the encoder input _lm_inputs builds and returns
        [B, 1 + max_new_tokens]: decoder_start_token_id, then the new tokens (transformers' shape for an encoder-decoder; input_ids
        are the encoder's and are not repeated).  The processors' history is then that decoder row."""
        if int(num_beams) != 1:
            raise ValueError(f"SelfAttentionModel.generate(): num_beams = {num_beams} is not implemented (beam search runs on "
                             "CrossAttentionModel / MPTForCausalLM with input_ids prompts); this path is greedy")
        check_sampling("SelfAttentionModel.generate()", do_sample, temperature, top_k, top_p, seed, sample_u, 1, num_return_sequences)
        if self.can_generate_seq2seq():
            # a T5: the encoder input is built as forward builds it (neighbor tokens and their mask included), the decoder row starts
            # at decoder_start_token_id.  Returns [B, 1 + max_new_tokens] -- the start token, then the new tokens -- as transformers does
            if not input_ids.is_cuda:
                raise RuntimeError(f"generate() runs on the GPU only (input_ids is on {input_ids.device}); there is no CPU path")
            lm_input, lm_mask = self._lm_inputs(input_ids, attention_mask, images, image_positions, neighbor_input_ids,
                                                neighbor_attention_mask, neighbor_pos_ids, text_locations, neighbor_images,
                                                neighbor_images_pos_ids, image_locations, lpe, graph)
            ids, embeds = (None, lm_input) if lm_input.dim() == 3 else (lm_input, None)
            return self._t5().generate(input_ids=ids, inputs_embeds=embeds, attention_mask=lm_mask, max_new_tokens=max_new_tokens,
                                       eos_token_id=eos_token_id, pad_token_id=pad_token_id, return_step_logits=return_step_logits,
                                       do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, sample_u=sample_u,
                                       repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                       min_new_tokens=min_new_tokens, suppress_tokens=suppress_tokens)
        if not self.can_generate():
            raise ValueError(f"generate() is implemented for the decoder-only OPT fork with peft_type none / lora / prompt, not for "
                             f"{type(self.lm).__name__} with peft_type {self.args.peft_type!r}")
        proc = check_processors("SelfAttentionModel.generate()", repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens,
                                eos_token_id, max_new_tokens, self.lm.config.vocab_size, 1, input_ids.dtype)
        if not input_ids.is_cuda:
            raise RuntimeError(f"generate() runs on the GPU only (input_ids is on {input_ids.device}); there is no CPU path")
        T = input_ids.shape[1]
        if image_positions is not None and self.neighbor_mode == "raw" and self.context in ("section_all", "all"):
            if bool((image_positions >= T).any()):          # one host read per call: the scatter below would write out of bounds
                raise ValueError(f"generate(): image_positions must lie inside the {T} prompt columns")
        lm_input, lm_mask = self._lm_inputs(input_ids, attention_mask, images, image_positions, neighbor_input_ids, neighbor_attention_mask,
                                            neighbor_pos_ids, text_locations, neighbor_images, neighbor_images_pos_ids, image_locations,
                                            lpe, graph)
        # key 0 is a virtual token under prompt tuning (always valid); otherwise the collate may vouch for the prompt's first column
        first = self.prompt_embeddings is not None or bool(host_meta and host_meta.get("first_key_valid"))
        kw = dict(max_new_tokens=max_new_tokens, eos_token_id=eos_token_id, pad_token_id=pad_token_id, return_step_logits=return_step_logits,
                  first_key_valid=first)
        if do_sample:
            kw.update(do_sample=True, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, sample_u=sample_u)
        if proc is not None:
            kw.update(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_new_tokens=min_new_tokens,
                      suppress_tokens=suppress_tokens)
        if lm_input.dim() == 2:
            return self.lm.generate(lm_input, lm_mask, **kw)
        if proc is not None:
            kw.update(history_ids=input_ids, history_mask=attention_mask)
        out = self.lm.generate(inputs_embeds=lm_input, attention_mask=lm_mask, **kw)
        new, logits = out if return_step_logits else (out, None)
        ids = torch.cat([input_ids, new.to(input_ids.dtype)], dim=1)
        return (ids, logits) if return_step_logits else ids
