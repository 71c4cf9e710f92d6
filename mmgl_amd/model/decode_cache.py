"""The state of generation with a key/value cache, and the one place that knows its decode modes.

A DecodeCache is built by a prefill (MPTDecoder.forward(use_cache=True), LlamaNeighborLM._hidden) and advanced by the LM's decode and
verify steps.  The layers of a step never ask which mode is on: they project, hand the result to the cache's dispatch -- new_kv /
file_rotated say where the new token's key and value go, attend_self / attend_cross pick the attention op and the views it reads --
and carry on.  A new mode is a new row of the table in DecodeCache's docstring and a new branch in these four methods."""
import torch

from .. import ops


class DecodeCache:
    """State of generation with a key/value cache:
      kv          per frozen layer one preallocated [B, capacity, 2n] buffer: columns [0, n) of a row are that position's key, [n, 2n) its
                  value (the project's [B, S, H*D] layout, never head-transposed; the kernels address the two slabs in place).  n is the
                  hidden size of the OPT fork, Hkv*D of the Llama LM (the key/value heads only)
      cross       per gated layer the neighbor tokens' (k_proj, v_proj) outputs [B, S, d], projected once at prefill; cross_valid their [B, S] mask
      mask        the running [B, capacity] uint8 key mask: the prompt's attention mask (pad keys stay masked), then 1 per new token
      col         the column the next token is written to -- the same for every sample (prompts are right-padded to a common width)
      next_pos    [B] position id of the next token, counted from the mask as HF does (valid tokens so far + OPT's offset 2)
      cos_sin     None, or the Llama LM's fp32 rotary table [capacity, D/2, 2]; cross_gu its gated layers' [gate | up] weights, concatenated
                  once per generation
      beam, lookup, kv_dtype    what selects the mode of a step, below
      pairs       None, or the pair count B of a guided generation: batch_size is then 2B (the mode `guided`, below)
      rel_bias    None, or the T5 decoder's fp32 bias rows [H, capacity] (ops.t5_decode_bias; the mode `relbias`, below)
      w8          None, or a StepCodes (generate(weight_dtype="fp8")): the frozen layers' decode_step then multiplies e4m3fn codes of its
                  weights (ops.decode_linear_w8 on what w8.get returns) instead of the weights.  It is only another GEMM: it selects
                  no attention kernel and is no mode below

    The modes.  x is the layer input of a step's rows, q|k|v its projection, n the key width as above:
      plain       beam, lookup and kv_dtype None; rows = B.  k|v go into kv[l][:, col] -- the GEMM (OPT fork) or ops.rope_kv_append (Llama)
                  writes the cache column in place -- and ops.attn_decode reads columns 0..col (all at or before the query: no causal
                  test).  The one mode in which q_proj and v_proj may be LoRA-adapted.
      beam        beam = a BeamState: rows = B*W.  kv / mask / cross / cross_valid / next_pos stay at B rows -- the prompt is prefilled once
                  per sample and col stays at the prompt width.  k|v go into column beam.n_tail of the layer's tail [B*W, n_cap, 2n]; the
                  rows attend over the sample's `col` prompt columns (shared, never copied) plus their own n_tail + 1 tail keys,
                  addressed through beam.book.src (ops.attn_decode_beam).  OPT fork only.
      verify      lookup = a LookupState (prompt-lookup decoding): rows = B*W, W = K + 1 new tokens per sample, against per-sample cache
                  lengths lookup.len; col / next_pos stand still at the prompt's.  OPT fork: k|v go into the dense lookup.scratch[l]
                  [B*W, 2n], and ops.attn_decode_block attends causally and files them at columns lookup.len .. of kv[l].  Llama
                  (scratch=False): ops.rope_kv_append_block rotates at positions lookup.len[b] + i and files them, then
                  ops.attn_decode_gqa_block reads the cache.
      FP8         kv_dtype = ops.KV_FP8 (with num_heads = the key/value heads): kv[l] holds e4m3fn codes [B, capacity, 2n], kv_scale[l]
                  their int8 exponents [B, capacity, 2*heads] -- one power of two per (sample, column, key-or-value, head), key heads
                  first.  k|v of every layer go into the one dense kv_new [B, 2n] in the model's dtype, and ops.attn_decode_q8 attends
                  over the `col` cached columns plus the new row and files it, quantised, at column `col` -- the launches of the plain
                  step.  cross stays in the model's dtype.  No beams and no verify step.
      guided      pairs = B (neighbor guidance, generate(guidance_scale)): the plain mode over 2B rows.  kv / mask / next_pos have 2B rows
                  -- rows [0, B) are the prompts with neighbors, rows [B, 2B) the same prompts prefilled without the gated layers --
                  and every frozen layer runs the plain step on all of them; cross / cross_valid keep B rows and the gated layers run
                  on the leading B rows only (MPTDecoder._decode_rows).  No new branch below: pairs selects no kernel.  OPT fork only.
      relbias     rel_bias set (T5HipRunner.generate): the plain mode of a T5 decoder -- k|v go into kv[l][:, col] in place, and
                  ops.attn_decode_relbias reads columns 0..col with the raw q, rel_bias and no mask (a decoder row has no padding).
                  cross[l] / cross_valid are the encoder's projected keys / values and its mask.  No beams, verify step or FP8 cache.
    The gated layers attend over cross[k] in every mode: ops.attn_decode, or with a BeamState / LookupState ops.attn_decode_beam without a
    tail -- the W rows of a sample read its neighbor tokens once."""

    def __init__(self, num_layers, batch_size, capacity, hidden_size, dtype, device, kv_dtype=None, num_heads=None):
        self.capacity = int(capacity)
        self.kv_dtype = kv_dtype
        self.kv_scale = self.kv_new = None
        if kv_dtype is not None:
            if kv_dtype is not ops.KV_FP8 or not num_heads or hidden_size % int(num_heads):
                raise ValueError(f"DecodeCache: kv_dtype = {kv_dtype!r} with num_heads = {num_heads} (None, or torch.float8_e4m3fn with the "
                                 "number of heads)")
            self.kv_scale = [torch.empty(batch_size, self.capacity, 2 * int(num_heads), dtype=torch.int8, device=device) for _ in range(num_layers)]
            self.kv_new = torch.empty(batch_size, 2 * hidden_size, dtype=dtype, device=device)
        self.kv = [torch.empty(batch_size, self.capacity, 2 * hidden_size, dtype=kv_dtype or dtype, device=device) for _ in range(num_layers)]
        self.mask = torch.zeros(batch_size, self.capacity, dtype=torch.uint8, device=device)
        self.cross = []
        self.cross_valid = None
        self.cross_gu = []
        self.cos_sin = None
        self.col = 0
        self.next_pos = None
        self.beam = None
        self.lookup = None
        self.pairs = None
        self.rel_bias = None
        self.w8 = None

    def kv_out(self, idx):
        """What layer idx's prefill files its keys and values into (MPTAttention._file_kv)."""
        return self.kv[idx] if self.kv_scale is None else (self.kv[idx], self.kv_scale[idx])

    # -- the dispatch of a decode / verify step
    def _mode(self):
        if self.lookup is not None:
            if self.kv_scale is not None:
                raise ValueError("the FP8 key/value cache has no verify step")
            return "verify"
        if self.kv_scale is not None:
            if self.beam is not None:
                raise ValueError("the FP8 key/value cache has no beam step")
            return "fp8"
        return "plain" if self.beam is None else "beam"

    @property
    def plain(self):
        """Whether a step runs in the plain mode: the one with a decode path for LoRA-adapted q / v projections."""
        return self.beam is None and self.lookup is None and self.kv_scale is None

    def new_kv(self, idx):
        """Where layer idx's k|v projection of this step writes, [rows, 2n] with unit column stride (None: a verify step without
        scratch -- file_rotated files from the q|k|v rows)."""
        mode = self._mode()
        if mode == "plain":
            return self.kv[idx][:, self.col]
        if mode == "beam":
            return self.beam.tail[idx][:, self.beam.n_tail]
        if mode == "fp8":
            return self.kv_new
        return None if self.lookup.scratch is None else self.lookup.scratch[idx]

    def file_rotated(self, idx, qkv, num_heads, num_kv_heads):
        """The Llama filing: rotates the query heads of the step's fused q|k|v rows in place and files the rotated keys and the values
        of layer idx -- at new_kv(idx) with the rotary row of column `col`, or on a verify step at columns lookup.len .. of kv[idx]
        with the row of each token's own column.  Returns new_kv(idx), what attend_self takes."""
        mode = self._mode()
        if mode == "beam":
            raise ValueError("the rotary key/value cache has no beam step")
        if mode == "verify":
            ops.rope_kv_append_block(qkv, self.cos_sin, self.kv[idx], self.lookup.len, num_heads, num_kv_heads, self.lookup.W)
            return None
        new = self.new_kv(idx)
        ops.rope_kv_append(qkv, self.cos_sin[self.col], new, num_heads, num_kv_heads)
        return new

    def attend_self(self, idx, q, new, num_heads, num_kv_heads=None):
        """Self-attention of the step's rows q [rows, H*D] (scaled) over layer idx's cache; new: what new_kv(idx) / file_rotated
        returned, filled.  num_kv_heads: the grouped-query cache of the Llama LM."""
        mode = self._mode()
        kv, mask, col = self.kv[idx], self.mask, self.col
        n = kv.shape[-1] // 2
        if mode == "plain" and self.rel_bias is not None:
            return ops.attn_decode_relbias(q, kv[:, :col + 1, :n], kv[:, :col + 1, n:], self.rel_bias, num_heads)
        if mode == "plain":
            return ops.attn_decode(q, kv[:, :col + 1, :n], kv[:, :col + 1, n:], mask[:, :col + 1], num_heads, num_kv_heads=num_kv_heads)
        if mode == "fp8":
            return ops.attn_decode_q8(q, new[:, :n], new[:, n:], kv, self.kv_scale[idx], mask[:, :col], num_heads, num_kv_heads=num_kv_heads)
        if mode == "beam":
            beam, tail = self.beam, self.beam.tail[idx]
            t = beam.n_tail + 1
            return ops.attn_decode_beam(q, kv[:, :col, :n], kv[:, :col, n:], mask[:, :col], num_heads, beam.W, tail[:, :t, :n], tail[:, :t, n:],
                                        beam.book.src)
        lookup = self.lookup
        if new is None:                       # filed already (file_rotated): the call only reads
            return ops.attn_decode_gqa_block(q, kv[:, :, :n], kv[:, :, n:], mask, lookup.len, num_heads, num_kv_heads, lookup.W)
        return ops.attn_decode_block(q, new[:, :n], new[:, n:], kv[:, :, :n], kv[:, :, n:], mask, lookup.len, num_heads, lookup.W)

    def attend_cross(self, idx, q, num_heads):
        """Gated layer idx's attention of the step's rows q over the sample's projected neighbor tokens, which stay at B rows."""
        k, v = self.cross[idx]
        rows = self.beam if self.lookup is None else self.lookup
        if rows is None:
            return ops.attn_decode(q, k, v, self.cross_valid, num_heads)
        return ops.attn_decode_beam(q, k, v, self.cross_valid, num_heads, rows.W)


class WeightCodes:
    """A frozen layer's weights as FP8 codes (ops.quantize_weight_fp8: e4m3fn codes [N, K] and int8 exponents [N]), quantised on first
    use and kept beside the layer's fused-weight cache: get(name, w) returns the pair for the weight the decode step would multiply and
    quantises again when `key` changed -- by default the weight's (data pointer, _version, dtype, device), for a derived fused weight
    the key of the cache it came from (a rebuilt copy may land on the old address).  The weights themselves stay resident: the prefill
    multiplies them."""

    def __init__(self):
        self._codes = {}

    def get(self, name, w, key=None):
        key = (w.data_ptr(), w._version, w.dtype, w.device) if key is None else key
        hit = self._codes.get(name)
        if hit is None or hit[0] != key:
            hit = (key, ops.quantize_weight_fp8(w))
            self._codes[name] = hit
        return hit[1]

    def tensors(self):
        """Every (codes, exps) pair held, by name."""
        return {name: hit[1] for name, hit in self._codes.items()}

    @staticmethod
    def of(holder):
        """The WeightCodes of a frozen layer (or of its attention), kept in the holder's __dict__ beside its fused-weight cache: no
        parameter, no buffer, nothing in a state_dict."""
        codes = holder.__dict__.get("_w8_codes")
        if codes is None:
            codes = holder.__dict__["_w8_codes"] = WeightCodes()
        return codes


class StepCodes:
    """What DecodeCache.w8 holds during one generation with FP8 frozen weights: the (codes, exps) pairs its steps multiply, looked up
    once.  get(holder, name, w) asks the holder's WeightCodes on the first step -- which quantises, or finds the weight unchanged --
    and answers every later step of the generation from a dict: the weights are frozen, so a step does not look at them again."""

    def __init__(self):
        self._pairs = {}

    def get(self, holder, name, w, key=None):
        k = (id(holder), name)
        pair = self._pairs.get(k)
        if pair is None:
            pair = self._pairs[k] = WeightCodes.of(holder).get(name, w, key)
        return pair


class LookupState:
    """What prompt-lookup decoding adds to a prefilled DecodeCache (cache.lookup): per sample a cache length of its own and the block
    of W = K + 1 tokens the next verify step feeds.  All of it lives on the device and is advanced by ops.lookup_accept.
      len        int32 [B] cache columns filed (starts at the prompt width T: pad keys stay masked), gen int32 [B] tokens the row has,
                 finished uint8 [B], n_draft int32 [B] drafts in the block
      block      int64 [B, W] = [last token, drafts, filler], positions int64 [B, W] its position ids (clamped to the table)
      scratch    per frozen layer the dense [B*W, 2d] output of the k|v projection; ops.attn_decode_block files it into the cache
                 (scratch=False: None -- LlamaNeighborLM files the block's keys from its fused q|k|v rows, ops.rope_kv_append_block)
      emitted    int32 [n_new, B]: row c holds the tokens call c of ops.lookup_accept appended (call 0: the prefill's row)"""

    def __init__(self, cache, num_tokens, ngram_size, n_new, scratch=True):
        B, _, two_d = cache.kv[0].shape
        dev = cache.mask.device
        self.K, self.N, self.W = int(num_tokens), int(ngram_size), int(num_tokens) + 1
        self.len = torch.full((B,), cache.col, dtype=torch.int32, device=dev)
        self.gen = torch.zeros(B, dtype=torch.int32, device=dev)
        self.finished = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.n_draft = torch.zeros(B, dtype=torch.int32, device=dev)
        self.block = torch.zeros(B, self.W, dtype=torch.int64, device=dev)
        self.positions = torch.zeros(B, self.W, dtype=torch.int64, device=dev)
        self.scratch = [torch.empty(B * self.W, two_d, dtype=kv.dtype, device=dev) for kv in cache.kv] if scratch else None
        self.emitted = torch.zeros(max(int(n_new), 1), B, dtype=torch.int32, device=dev)
        cache.mask[:, cache.col:] = 1                            # once: lookup.len bounds what a sample reads


class BeamState:
    """What a beam search adds to a prefilled DecodeCache (cache.beam): W hypotheses per sample that share the sample's cache rows.
      tail    per frozen layer one [B*W, n_cap, 2d] buffer of the keys | values the hypotheses generated themselves: decode step j
              writes column j of row b*W + w in place (the k|v projection's ldy), as a greedy step writes its cache column
      book    ops.BeamBook: the running beams, the two parent tables that say which tail row holds a hypothesis' key of step j
              (reordering the beams rewrites these few int32, never a cache row) and the pool of finished hypotheses
      n_tail  tail columns filled so far = decode steps done"""

    def __init__(self, cache, num_beams, n_cap):
        B, _, two_d = cache.kv[0].shape
        self.W = int(num_beams)
        self.n_cap = max(int(n_cap), 1)
        self.tail = [torch.empty(B * self.W, self.n_cap, two_d, dtype=kv.dtype, device=kv.device) for kv in cache.kv]
        self.book = ops.BeamBook(B, self.W, self.n_cap, cache.mask.device)
        self.n_tail = 0
