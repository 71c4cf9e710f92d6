"""generation.decode_loop with the greedy tail, and generation.check_prompt, without a GPU.  The language model is a stub: a fixed fp32
table [V, V] holds "the logits given the last token", the hidden state IS the last token and a decode step returns the token it was
fed.  Everything is compared with a plain Python restatement of the loop.  Sampled and processor runs need ops.sample_tokens /
ops.process_logits, which have no CPU path: the GPU tests of generate() hold them."""
import pytest
import torch

from mmgl_amd.model.generation import GreedyTail, check_prompt, decode_loop

V, EOS, PAD, N_NEW = 16, 2, 1, 6
# the chain of argmax successors: 3 -> 4 -> ... -> 15 -> 3 never meets EOS, except through 7 -> EOS; 0, 1 (PAD) and 2 (EOS) lead to 3
NEXT = [3, 3, 3] + [t + 1 for t in range(3, 15)] + [3]
NEXT[7] = EOS
TABLE = torch.randn(V, V, generator=torch.Generator().manual_seed(0))
TABLE[torch.arange(V), torch.tensor(NEXT)] = 10.0
# the last prompt tokens: row 0 emits EOS at step 2, row 1 never, row 2 at step 0
PROMPT = torch.tensor([[9, 4, 5], [3, 11, 8], [14, 6, 7]])


class _Stub:
    def __init__(self):
        self.calls = 0

    def last_logits(self, hidden):
        return TABLE[hidden]

    def step(self, tok):
        assert tok.shape == (PROMPT.shape[0], 1)
        self.calls += 1
        return tok[:, 0]


def _restated(n_new, eos):
    """Per row: the new tokens and the token each step's logits were read for."""
    new, fed = [], []
    for last in PROMPT[:, -1].tolist():
        row, seen, done = [], [], False
        for _ in range(n_new):
            seen.append(last)
            tok = PAD if done else NEXT[last]
            done = done or (eos is not None and tok == eos)
            row.append(tok)
            last = tok
        new.append(row)
        fed.append(seen)
    return torch.tensor(new), torch.tensor(fed)


def _run(n_new=N_NEW, eos=EOS, input_ids=PROMPT, **kw):
    lm = _Stub()
    out = decode_loop(lm.last_logits, lm.step, PROMPT[:, -1], GreedyTail(PROMPT.shape[0], "cpu", eos, None if eos is None else PAD), n_new,
                      input_ids, None if input_ids is None else torch.ones_like(input_ids), **kw)
    return out, lm.calls


def test_ids_and_eos_padding():
    want, _ = _restated(N_NEW, EOS)
    assert want[0].tolist() == [6, 7, EOS, PAD, PAD, PAD] and EOS not in want[1].tolist() and want[2].tolist() == [EOS] + [PAD] * 5
    ids, calls = _run()
    assert ids.dtype == PROMPT.dtype and ids.is_contiguous() and calls == N_NEW - 1
    assert torch.equal(ids, torch.cat([PROMPT, want], dim=1))


def test_without_eos_every_row_runs_on():
    want, _ = _restated(N_NEW, None)
    assert want[0].tolist() == [6, 7, EOS, 3, 4, 5]
    ids, _ = _run(eos=None)
    assert torch.equal(ids, torch.cat([PROMPT, want], dim=1))


def test_the_result_keeps_the_prompts_dtype():
    ids, _ = _run(input_ids=PROMPT.to(torch.int32))
    assert ids.dtype == torch.int32 and torch.equal(ids.long(), torch.cat([PROMPT, _restated(N_NEW, EOS)[0]], dim=1))


def test_step_logits_are_the_tables_rows():
    want, fed = _restated(N_NEW, EOS)
    (ids, logits), _ = _run(return_step_logits=True)
    assert logits.shape == (PROMPT.shape[0], N_NEW, V) and logits.dtype == torch.float32
    assert torch.equal(logits, TABLE[fed]) and torch.equal(ids[:, PROMPT.shape[1]:], want)


def test_embeddings_prompt_returns_the_new_tokens_only():
    ids, calls = _run(input_ids=None)
    assert ids.shape == (PROMPT.shape[0], N_NEW) and ids.dtype == torch.int64 and ids.is_contiguous() and calls == N_NEW - 1
    assert torch.equal(ids, _restated(N_NEW, EOS)[0])


def test_one_new_token_runs_no_decode_step():
    (ids, logits), calls = _run(n_new=1, return_step_logits=True)
    assert calls == 0 and logits.shape == (PROMPT.shape[0], 1, V)
    assert torch.equal(ids, torch.cat([PROMPT, _restated(1, EOS)[0]], dim=1))


class _OnGpu:
    """What check_prompt reads of a prompt, for what lies behind the device check (the default mask is built on `device`)."""
    is_cuda, device = True, torch.device("cpu")

    def __init__(self, *shape):
        self.shape = shape

    def dim(self):
        return len(self.shape)


class _Config:
    pad_token_id = None


def test_check_prompt_refusals_and_defaults():
    ids, emb, mask = _OnGpu(3, 5), _OnGpu(3, 5, 8), object()
    for pair in ((None, None), (ids, emb)):
        with pytest.raises(ValueError, match="exactly one of input_ids and inputs_embeds"):
            check_prompt(*pair, mask, 4, None, None, _Config, 16)
    with pytest.raises(ValueError, match="max_new_tokens must be positive, got 0"):
        check_prompt(PROMPT, None, mask, 0, None, None, _Config, 16)              # in front of the device check
    with pytest.raises(RuntimeError, match=r"runs on the GPU only \(the prompt is on cpu\); there is no CPU path"):
        check_prompt(PROMPT, None, mask, 4, None, None, _Config, 16)
    for pair in ((emb, None), (None, ids)):                                       # ids of rank 3, embeddings of rank 2
        with pytest.raises(ValueError, match=r"input_ids \[B, T\] or inputs_embeds \[B, T, d_embed\], got"):
            check_prompt(*pair, mask, 4, None, None, _Config, 16)
    with pytest.raises(ValueError, match="5 prompt columns \\+ 13 new tokens exceed max_position_embeddings 16"):
        check_prompt(ids, None, mask, 13, None, None, _Config, 16)
    with pytest.raises(ValueError, match="eos_token_id needs a pad_token_id"):
        check_prompt(ids, None, mask, 4, EOS, None, _Config, 16)

    class WithPad:
        pad_token_id = 7
    assert check_prompt(ids, None, mask, 12, None, None, _Config, 16) == (3, 5, 12, None, mask)       # 5 + 12 - 1 positions fit
    assert check_prompt(None, emb, mask, "4", EOS, None, WithPad, 16) == (3, 5, 4, 7, mask)
    assert check_prompt(ids, None, mask, 4, EOS, PAD, WithPad, 16)[3] == PAD
    assert check_prompt(ids, None, mask, 4, None, None, WithPad, 16)[3] is None  # no EOS: nothing to pad
    default = check_prompt(None, emb, None, 4, None, None, _Config, 16)[4]
    assert default.dtype == torch.int64 and torch.equal(default, torch.ones(3, 5, dtype=torch.int64))
