"""The sampling, logits-processor, prompt-lookup, contrastive-search, key/value-cache and neighbor-guidance arguments shared by the three generate()
methods (MPTForCausalLM / CrossAttentionModel, SelfAttentionModel, LlamaNeighborLM): their checks, which need no device, the uniform numbers a sampled generation consumes and the
per-generation state of the processors.  The selection itself is ops.sample_tokens, the processors are ops.process_logits, one launch
per decode step each; the loop that makes those calls is generation.decode_loop."""
import math

import torch

from .. import ops


def check_sampling(who, do_sample, temperature, top_k, top_p, seed, sample_u, num_beams=1, num_return_sequences=1, multi=False):
    """Validates generate()'s sampling keywords; returns R = the sequences returned per prompt (1 unless do_sample with
    num_return_sequences).  do_sample=False: the other five must be at their defaults (the greedy and beam paths ignore them, and a
    silently ignored temperature is a wrong result).  `multi`: whether this generator implements num_return_sequences > 1."""
    if not do_sample:
        if float(temperature) != 1.0 or int(top_k) != 0 or float(top_p) != 1.0 or seed is not None or sample_u is not None:
            raise ValueError(f"{who}: temperature / top_k / top_p / seed / sample_u belong to do_sample=True; with do_sample=False they "
                             "must stay at their defaults")
        if num_return_sequences != 1:
            raise ValueError(f"{who}: num_return_sequences = {num_return_sequences} is not implemented without do_sample=True (the best "
                             "hypothesis per sample is returned)")
        return 1
    if int(num_beams) != 1:
        raise ValueError(f"{who}: do_sample=True with num_beams = {num_beams} (sampling combined with beam search) is not implemented")
    if not (0.0 < float(temperature) < float("inf")):
        raise ValueError(f"{who}: temperature = {temperature} must be positive and finite")
    if int(top_k) < 0:
        raise ValueError(f"{who}: top_k = {top_k} must not be negative (0: off)")
    if not (0.0 < float(top_p) <= 1.0):
        raise ValueError(f"{who}: top_p = {top_p} outside (0, 1]")
    if seed is not None and sample_u is not None:
        raise ValueError(f"{who}: pass seed or sample_u, not both")
    R = int(num_return_sequences)
    if not 1 <= R <= ops.MAX_BEAMS:
        raise ValueError(f"{who}: num_return_sequences = {num_return_sequences} (1..{ops.MAX_BEAMS})")
    if R > 1 and not multi:
        raise ValueError(f"{who}: num_return_sequences = {R} is implemented for MPTForCausalLM / CrossAttentionModel with input_ids prompts "
                         "and plain projections only (the continuations share the prompt's cache rows)")
    return R


def sampling_u(who, n_new, rows, device, seed, sample_u):
    """The uniform numbers of one sampled generation, fp32 [n_new, rows] in [0, 1): `sample_u` itself when given, else one torch.rand
    before the loop -- on a fresh device generator seeded with `seed`, or on torch's global device generator (seed=None).  Nothing is
    drawn per step."""
    if sample_u is not None:
        if (not torch.is_tensor(sample_u) or sample_u.dtype != torch.float32 or tuple(sample_u.shape) != (n_new, rows)
                or sample_u.device != device or not sample_u.is_contiguous()):
            raise ValueError(f"{who}: sample_u must be a dense fp32 [max_new_tokens = {n_new}, rows = {rows}] tensor on {device}")
        return sample_u
    gen = None
    if seed is not None:
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed))
    return torch.rand(n_new, rows, generator=gen, device=device, dtype=torch.float32)


def check_lookup(who, prompt_lookup_num_tokens, max_matching_ngram_size, return_lookup_stats, do_sample=False, num_beams=1,
                 num_return_sequences=1, processors=False, return_step_logits=False, inputs_embeds=None):
    """Validates generate()'s prompt-lookup keywords; returns (K, N).  K = prompt_lookup_num_tokens = 0: off -- the
    greedy loop runs exactly as without the keywords.  K > 0 verifies K drafted tokens per step and returns the greedy result, so it
    combines with nothing that changes or observes the per-step selection."""
    K, N = int(prompt_lookup_num_tokens), int(max_matching_ngram_size)
    if not 0 <= K <= ops.MAX_LOOKUP_TOKENS:
        raise ValueError(f"{who}: prompt_lookup_num_tokens = {prompt_lookup_num_tokens} (0: off, 1..{ops.MAX_LOOKUP_TOKENS})")
    if K == 0:
        if return_lookup_stats:
            raise ValueError(f"{who}: return_lookup_stats belongs to prompt_lookup_num_tokens > 0")
        return 0, N
    if not 1 <= N <= ops.MAX_LOOKUP_NGRAM:
        raise ValueError(f"{who}: max_matching_ngram_size = {max_matching_ngram_size} (1..{ops.MAX_LOOKUP_NGRAM})")
    if do_sample:
        raise ValueError(f"{who}: prompt_lookup_num_tokens = {K} with do_sample=True is not implemented (the drafts are verified against "
                         "the greedy choice)")
    if int(num_beams) != 1 or int(num_return_sequences) != 1:
        raise ValueError(f"{who}: prompt_lookup_num_tokens = {K} with num_beams = {num_beams} / num_return_sequences = "
                         f"{num_return_sequences} is not implemented")
    if processors:
        raise ValueError(f"{who}: prompt_lookup_num_tokens = {K} is not implemented with repetition_penalty / no_repeat_ngram_size / "
                         "min_new_tokens / suppress_tokens (they rewrite each step's logits from the tokens before it)")
    if return_step_logits:
        raise ValueError(f"{who}: prompt_lookup_num_tokens = {K} has no per-step logits to return (return_step_logits)")
    if inputs_embeds is not None:
        raise ValueError(f"{who}: prompt_lookup_num_tokens = {K} takes input_ids prompts, not inputs_embeds (the drafts are looked up in the ids)")
    return K, N


def check_contrastive(who, penalty_alpha, top_k, return_contrastive_trace, do_sample=False, num_beams=1, num_return_sequences=1,
                      prompt_lookup_num_tokens=0, inputs_embeds=None, return_beam_trace=False, return_sequences_scores=False):
    """Validates generate()'s contrastive-search keywords; returns k, the candidates ranked per step (0: off -- then
    every other path and check runs exactly as without the keywords, top_k stays a sampling knob).  penalty_alpha in (0, 1) turns it
    on and makes top_k its k (2..ops.MAX_BEAMS).  It is a decoding mode of its own: it combines with the logits processors and
    return_step_logits, and with nothing else that selects tokens."""
    alpha = float(penalty_alpha)
    if alpha == 0.0:
        if return_contrastive_trace:
            raise ValueError(f"{who}: return_contrastive_trace belongs to penalty_alpha > 0")
        return 0
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"{who}: penalty_alpha = {penalty_alpha} outside [0, 1) (0: off)")
    k = int(top_k)
    if not 2 <= k <= ops.MAX_BEAMS:
        raise ValueError(f"{who}: penalty_alpha = {penalty_alpha} (contrastive search) needs top_k in 2..{ops.MAX_BEAMS}, got {top_k}")
    if do_sample:
        raise ValueError(f"{who}: penalty_alpha = {penalty_alpha} with do_sample=True is not implemented (contrastive search is deterministic)")
    if int(num_beams) != 1 or int(num_return_sequences) != 1:
        raise ValueError(f"{who}: penalty_alpha = {penalty_alpha} with num_beams = {num_beams} / num_return_sequences = "
                         f"{num_return_sequences} is not implemented")
    if int(prompt_lookup_num_tokens) != 0:
        raise ValueError(f"{who}: penalty_alpha = {penalty_alpha} with prompt_lookup_num_tokens = {prompt_lookup_num_tokens} is not implemented "
                         "(the drafts are verified against the greedy choice)")
    if inputs_embeds is not None:
        raise ValueError(f"{who}: penalty_alpha = {penalty_alpha} takes input_ids prompts, not inputs_embeds")
    if return_beam_trace or return_sequences_scores:
        raise ValueError(f"{who}: return_sequences_scores / return_beam_trace belong to beam search; contrastive search has "
                         "return_contrastive_trace")
    return k


def check_kv_cache(who, kv_cache_dtype, num_beams=1, num_return_sequences=1, prompt_lookup_num_tokens=0, penalty_alpha=0.0, projections=(),
                   past_key_values=None):
    """Validates generate()'s kv_cache_dtype; returns None (off: every path runs exactly as without the keyword) or
    ops.KV_FP8.  "fp8" / torch.float8_e4m3fn keeps the frozen layers' self-attention cache as e4m3fn codes with power-of-two scales.
    It belongs to the greedy and sampled loop of one row per prompt (generation.decode_loop: the processors and return_step_logits
    combine with it); the beam, block and candidate steps read the cache through kernels that have no FP8 form.  `projections`: the
    q / k / v / out projections of the frozen layers, which must be plain nn.Linear."""
    if kv_cache_dtype is None:
        return None
    if not (kv_cache_dtype == "fp8" or kv_cache_dtype is ops.KV_FP8):
        raise ValueError(f"{who}: kv_cache_dtype = {kv_cache_dtype!r} is unknown: None (the model's dtype), 'fp8' or torch.float8_e4m3fn "
                         "(the FP8 key/value cache)")
    fp8 = f"{who}: kv_cache_dtype = 'fp8' (the FP8 key/value cache)"
    if int(num_beams) != 1:
        raise ValueError(f"{fp8} with num_beams = {num_beams} is not implemented (the beam steps read the cache through a kernel of their own)")
    if int(num_return_sequences) != 1:
        raise ValueError(f"{fp8} with num_return_sequences = {num_return_sequences} is not implemented (the continuations share the "
                         "prompt's cache rows through the beam kernel)")
    if int(prompt_lookup_num_tokens) != 0:
        raise ValueError(f"{fp8} with prompt_lookup_num_tokens = {prompt_lookup_num_tokens} is not implemented (the verify steps read the "
                         "cache through the block kernel)")
    if float(penalty_alpha) != 0.0:
        raise ValueError(f"{fp8} with penalty_alpha = {penalty_alpha} is not implemented (contrastive search runs on the beam-shared cache)")
    if any(type(m) is not torch.nn.Linear for m in projections):
        raise ValueError(f"{fp8} runs plain nn.Linear q / k / v / out projections only (adapted projections, e.g. LoRA, are not implemented)")
    if past_key_values is not None:
        raise ValueError(f"{fp8} with a prefix-tuning past_key_values (a key/value prefix) is not implemented")
    return ops.KV_FP8


def check_weight_dtype(who, weight_dtype, linears=()):
    """Validates generate()'s weight_dtype; returns None (off: every path runs exactly as without the keyword) or
    ops.KV_FP8.  "fp8" / torch.float8_e4m3fn runs the decode steps' GEMMs of the frozen layers on e4m3fn codes of their weights with
    one power-of-two scale per weight row (ops.decode_linear_w8).  It is only another GEMM, so it selects no decoding mode and
    combines with all of them.  `linears`: the modules whose weights the frozen layers' steps multiply, which must be plain nn.Linear
    (a LoRA-adapted projection runs the skinny GEMM with the rank-r term, which has no form on codes)."""
    if weight_dtype is None:
        return None
    if not (weight_dtype == "fp8" or weight_dtype is ops.KV_FP8):
        raise ValueError(f"{who}: weight_dtype = {weight_dtype!r} is unknown: None (the model's dtype), 'fp8' or torch.float8_e4m3fn "
                         "(FP8 frozen weights for the decode steps)")
    if any(type(m) is not torch.nn.Linear for m in linears):
        raise ValueError(f"{who}: weight_dtype = 'fp8' (FP8 frozen weights) runs plain nn.Linear projections and FFN layers only (adapted "
                         "projections, e.g. LoRA, are not implemented)")
    return ops.KV_FP8


def check_guidance(who, guidance_scale, num_beams=1, num_return_sequences=1, prompt_lookup_num_tokens=0, penalty_alpha=0.0,
                   kv_cache_dtype=None, inputs_embeds=None, neighbors=True, gated_layers=True):
    """Validates generate()'s guidance_scale; returns None (off: None or 1.0 -- every path runs exactly as without the
    keyword) or g as a float.  Any other finite g >= 0 contrasts each step's next-token distribution with neighbors against the one
    of the LM without its gated layers: score = lu + g (lc - lu) on log-probabilities.  It belongs to the greedy and sampled loop of
    one row per prompt (generation.decode_loop: the processors and return_step_logits combine with it) on a cache of 2B rows.
    `neighbors`: whether the call has neighbor tokens; `gated_layers`: whether the decoder has layers that read them."""
    if guidance_scale is None:
        return None
    if isinstance(guidance_scale, bool) or not isinstance(guidance_scale, (int, float)):
        raise ValueError(f"{who}: guidance_scale = {guidance_scale!r} must be a finite number >= 0 (None or 1: off)")
    g = float(guidance_scale)
    if not (0.0 <= g < math.inf):
        raise ValueError(f"{who}: guidance_scale = {guidance_scale} must be a finite number >= 0 (None or 1: off)")
    if g == 1.0:
        return None
    on = f"{who}: guidance_scale = {guidance_scale} (neighbor guidance)"
    if int(num_beams) != 1:
        raise ValueError(f"{on} with num_beams = {num_beams} is not implemented (beam search scores hypotheses on the beam-shared cache)")
    if int(num_return_sequences) != 1:
        raise ValueError(f"{on} with num_return_sequences = {num_return_sequences} is not implemented (the continuations share the "
                         "prompt's cache rows through the beam kernel)")
    if int(prompt_lookup_num_tokens) != 0:
        raise ValueError(f"{on} with prompt_lookup_num_tokens = {prompt_lookup_num_tokens} is not implemented (the drafts are verified "
                         "against the unguided greedy choice)")
    if float(penalty_alpha) != 0.0:
        raise ValueError(f"{on} with penalty_alpha = {penalty_alpha} is not implemented (contrastive search ranks its candidates on the "
                         "beam-shared cache)")
    if kv_cache_dtype is not None:
        raise ValueError(f"{on} with kv_cache_dtype = {kv_cache_dtype!r} is not implemented (the FP8 cache has no step of paired rows)")
    if inputs_embeds is not None:
        raise ValueError(f"{on} with inputs_embeds is not implemented (it takes input_ids prompts)")
    if not neighbors or not gated_layers:
        raise ValueError(f"{on} without neighbor tokens, or on a decoder without gated layers, is not implemented: there is nothing to "
                         "contrast")
    return g


MAX_SUPPRESS = ops.MAX_BAN - 1        # the ban array of a generation is suppress_tokens followed by the EOS entry


def check_processors(who, repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens, eos_token_id, max_new_tokens,
                     vocab_size, num_beams=1, ids_dtype=None):
    """Validates generate()'s logits-processor keywords.  Returns None when all four are at their defaults -- the
    loop then runs exactly as without them -- else a LogitsProcessors that generation.decode_loop binds and calls once per step."""
    p, n, m = float(repetition_penalty), int(no_repeat_ngram_size), int(min_new_tokens)
    if not (0.0 < p < math.inf):
        raise ValueError(f"{who}: repetition_penalty = {repetition_penalty} must be positive and finite (1: off)")
    if n < 0:
        raise ValueError(f"{who}: no_repeat_ngram_size = {no_repeat_ngram_size} must not be negative (0: off)")
    if m < 0:
        raise ValueError(f"{who}: min_new_tokens = {min_new_tokens} must not be negative")
    suppress = [] if suppress_tokens is None else [int(t) for t in suppress_tokens]
    if len(suppress) > MAX_SUPPRESS:
        raise ValueError(f"{who}: {len(suppress)} suppress_tokens (at most {MAX_SUPPRESS})")
    for t in suppress:
        if not 0 <= t < int(vocab_size):
            raise ValueError(f"{who}: suppress_tokens entry {t} outside [0, {int(vocab_size)})")
    if m > 0:
        if eos_token_id is None:
            raise ValueError(f"{who}: min_new_tokens = {m} needs an eos_token_id")
        if m > int(max_new_tokens):
            raise ValueError(f"{who}: min_new_tokens = {m} exceeds max_new_tokens = {max_new_tokens}")
    if p == 1.0 and n == 0 and m == 0 and not suppress:
        return None
    if int(num_beams) != 1:
        raise ValueError(f"{who}: repetition_penalty / no_repeat_ngram_size / min_new_tokens / suppress_tokens are not implemented with "
                         f"beam search (num_beams = {num_beams}): there they act on log-probabilities along each hypothesis' ancestry")
    if ids_dtype is not None and ids_dtype != torch.int64:
        raise ValueError(f"{who}: with a logits processor on, input_ids must be int64, got {ids_dtype}")
    return LogitsProcessors(p, n, m, suppress, eos_token_id)


class LogitsProcessors:
    """The processors of one generate() call.  The device state is built once: upload() copies the ban array (suppress_tokens
    followed by EOS; the EOS entry counts only while s < min_new_tokens, decided on the host from the step index), bind() makes the
    uint8 mask of the prompt columns.  Step s then makes one ops.process_logits call on the [rows, V] logits with the row so far as
    history.  upload() is the one host-to-device copy of a generation, and such a copy waits for the work queued before it: every
    generate() calls it in FRONT of its prefill, where nothing of this generation is queued yet (behind the prefill it cost the host its
    head start over the device, 15 ms per call at B = 16 on the flagship model)."""

    def __init__(self, penalty, ngram, min_new, suppress, eos_token_id):
        self.penalty, self.ngram, self.min_new, self.suppress, self.eos = penalty, ngram, min_new, suppress, eos_token_id
        self.ban = self.mask = None

    def upload(self, device):
        ban = self.suppress + ([int(self.eos)] if self.min_new > 0 else [])
        if ban and self.ban is None:
            self.ban = torch.tensor(ban, dtype=torch.int32, device=device)
        return self

    def bind(self, device, prompt_mask=None, repeat=1):
        """prompt_mask [B, T] (any integer / bool dtype, None: every prompt column is history); repeat = R rows per prompt."""
        self.upload(device)
        if prompt_mask is not None and prompt_mask.shape[1] > 0:
            mask = (prompt_mask != 0).to(torch.uint8)
            self.mask = mask if repeat == 1 else mask.repeat_interleave(repeat, dim=0)
        return self

    def __call__(self, logits, history, s, stride=1):
        """Step s, in place on logits; history = the ids in front of the column being chosen.  stride = R on the first step of
        num_return_sequences = R, where history (and logits) has one row per prompt."""
        n_ban = len(self.suppress) + (1 if s < self.min_new else 0)
        mask = self.mask if self.mask is None or stride == 1 else self.mask[::stride]
        return ops.process_logits(logits, history, mask, None, self.penalty, self.ngram, self.ban[:n_ban] if n_ban else None)
