"""The sampling arguments shared by the three generate() methods (MPTForCausalLM / CrossAttentionModel, SelfAttentionModel,
LlamaNeighborLM): their checks, which need no device, and the uniform numbers a sampled generation consumes.  The selection itself is
ops.sample_tokens, one launch per decode step."""
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
