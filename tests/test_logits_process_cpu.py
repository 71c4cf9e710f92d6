"""CPU: the logits-processor surface without a GPU -- the yardstick of the GPU tests itself (tests/logits_ref.py's restatement of the
mmgl_logits_process contract, bitwise against transformers' RepetitionPenalty / NoRepeatNGram / MinNewTokensLength / SuppressTokens
processors), the symbol and its argument validation, and the refusals of the generate() methods and of ops.process_logits that need
no device."""
import os

import pytest
import torch

from logits_ref import compact, hf_chain, process, process_row
from test_sample_cpu import _cross_wrapper, _llama, _mpt, _self_wrapper


def _bits(t):
    return t.contiguous().view(torch.int32)


def _histories(V, n, g):
    """Named histories for one (V, n): the lengths 0, 1, n-1, n, 40, a 4-token alphabet, and the two ends of the vocabulary."""
    out = {f"L{L}": torch.randint(0, V, (L,), generator=g).tolist() for L in sorted({0, 1, max(n - 1, 0), n, 40})}
    out["alphabet4"] = torch.randint(5, 9, (40,), generator=g).tolist()
    out["ends"] = [0, V - 1, 0, V - 1, 3, 0, V - 1] * 3
    return out


@pytest.mark.parametrize("V", [128, 50272])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("p", [0.8, 1.3])
def test_restatement_is_bitwise_transformers(V, n, p):
    g = torch.Generator().manual_seed(V + 10 * n + int(10 * p))
    for name, h in _histories(V, n, g).items():
        x = torch.randn(V, generator=g) * 3.0
        for t in h[:2]:
            x[t] = -abs(x[t])                                   # both signs among the penalised logits
        for kw in (dict(penalty=p), dict(ngram=n), dict(penalty=p, ngram=n)):
            want = hf_chain(x, h, **kw)
            got = process_row(x, h, **kw)
            assert torch.equal(_bits(got), _bits(want)), f"{name} {kw}"
        # the whole chain with the bans: suppress + EOS below min_new_tokens (3 of the history's tokens count as generated)
        gen = min(3, len(h))
        want = hf_chain(x, h, p, n, suppress=(5, 77), eos=2, min_new=4, n_generated=gen)
        got = process_row(x, h, p, n, ban=(5, 77, 2))
        assert torch.equal(_bits(got), _bits(want)), f"{name} chain"
        want = hf_chain(x, h, p, n, suppress=(5,), eos=2, min_new=2, n_generated=gen)
        got = process_row(x, h, p, n, ban=(5, 2) if gen < 2 else (5,))
        assert torch.equal(_bits(got), _bits(want)), f"{name} chain past min_new_tokens"


@pytest.mark.parametrize("V", [128, 50272])
def test_restatement_masked_rows_equal_the_chain_on_the_compacted_row(V):
    g = torch.Generator().manual_seed(7 + V)
    rows, L, T = 6, 40, 24
    hist = torch.randint(0, V, (rows, L), generator=g)
    hist[:, ::3] = torch.randint(5, 9, (rows, len(range(0, L, 3))), generator=g)
    valid = torch.rand(rows, T, generator=g) < 0.6
    valid[0] = True
    valid[1] = False                                            # only the new tokens are history
    x = torch.randn(rows, V, generator=g) * 3.0
    for p, n in ((1.3, 2), (0.8, 3), (1.3, 0), (1.0, 1)):
        got = process(x, hist, valid, p, n, ban=(5, 77))
        for r in range(rows):
            h = compact(hist[r].tolist(), valid[r].tolist())
            assert len(h) == L - T + int(valid[r].sum())
            want = hf_chain(x[r], h, p, n, suppress=(5, 77))
            assert torch.equal(_bits(got[r]), _bits(want)), f"row {r} p={p} n={n}"


def test_restatement_edges():
    x = torch.arange(-4.0, 4.0)                                 # V = 8
    out = process_row(x, [1, 1, 1, 6, 6], penalty=2.0)          # once per distinct token
    assert out[1] == -6.0 and out[6] == 1.0 and torch.equal(out[[0, 2, 3, 4, 5, 7]], x[[0, 2, 3, 4, 5, 7]])
    assert torch.equal(process_row(x, [-1, 8, 1 << 40], 2.0, 1), x)                     # outside [0, V): nothing moves
    assert torch.equal(process_row(x, [3, -1, 5, 3, -1], ngram=3), x)                   # an n-gram holding such a token never matches
    assert torch.equal(process_row(x, [3, 4], ngram=3), x)                              # L < n
    out = process_row(x, [3, 4, 3], ngram=2, penalty=2.0)       # -inf beats the penalty on token 4, seen and banned
    assert out[4] == float("-inf") and out[3] == -2.0               # x[3] = -1: multiplied
    out = process(x[None].bfloat16(), torch.tensor([[1, 6]]), None, 1.3)
    assert out.dtype == torch.bfloat16 and out[0, 1] == (x[1] * torch.tensor(1.3)).bfloat16() and out[0, 6] == (x[6] / torch.tensor(1.3)).bfloat16()


# ------------------------------------------------------------------------------------------ the symbol
def test_logits_process_symbol_and_argument_validation():
    from mmgl_amd import _lib
    L = _lib.lib()
    assert L.mmgl_version() == _lib.ABI_VERSION == 110
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "mmgl_hip.h")).read()
    assert "mmgl_logits_process" in _lib.SIGNATURES and hasattr(L, "mmgl_logits_process") and "int mmgl_logits_process(" in header

    def call(logits=64, ld=None, hist=64, valid=None, n_masked=0, hist_len=8, ban=None, n_ban=0, rows=2, V=128, p=1.3, n=2, dtype=1):
        # (logits, ld_logits, history, ld_history, hist_valid, ld_valid, n_masked, hist_len, ban, n_ban, rows, V, p, n, dtype, stream);
        # non-null addresses that are never dereferenced: every check below fails before a launch
        return L.mmgl_logits_process(logits, V if ld is None else ld, hist, max(hist_len, 0), valid, 8, n_masked, hist_len, ban, n_ban, rows, V,
                                     p, n, dtype, None)

    assert call(logits=None) == 1 and b"null" in L.mmgl_last_error()
    assert call(hist=None) == 1 and call(n_masked=4) == 1 and call(n_ban=1) == 1                # each names a buffer that is NULL
    assert call(hist_len=8193) == 2 and b"hist_len" in L.mmgl_last_error()
    assert call(ban=64, n_ban=65) == 2 and call(V=131073) == 2
    assert call(p=0.0) == 1 and b"repetition_penalty" in L.mmgl_last_error()
    assert call(p=-1.0) == 1 and call(p=float("inf")) == 1 and call(p=float("nan")) == 1
    assert call(n=-1) == 1 and call(ban=64, n_ban=-1) == 1 and call(hist_len=-1) == 1 and call(valid=64, n_masked=-1) == 1
    assert call(valid=64, n_masked=9) == 1 and b"n_masked" in L.mmgl_last_error()
    assert call(dtype=7) == 1 and call(ld=100) == 1 and call(rows=0) == 1 and call(rows=-3) == 1 and call(V=0) == 1
    assert call(p=1.0, n=0) == 0 and call(hist=None, hist_len=0) == 0                           # everything off: no launch either


def test_ops_process_logits_has_no_cpu_path():
    from mmgl_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.process_logits(torch.zeros(2, 64), torch.zeros(2, 4, dtype=torch.int64), repetition_penalty=1.3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.process_logits(torch.zeros(2, 64, dtype=torch.bfloat16), None, ban=torch.zeros(1, dtype=torch.int32))


# ------------------------------------------------------------------------------------------ generate()'s refusals
@pytest.mark.parametrize("make", [_mpt, _cross_wrapper, _self_wrapper, _llama])
def test_generate_processor_refusals_without_a_device(make):
    m = make()
    ids = torch.randint(3, 128, (2, 6))
    mask = torch.ones_like(ids)
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf")),
                dict(repetition_penalty=float("nan")), dict(no_repeat_ngram_size=-1)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            m.generate(ids, mask, max_new_tokens=4, **bad)
    with pytest.raises(ValueError, match="eos_token_id"):
        m.generate(ids, mask, max_new_tokens=4, min_new_tokens=2)
    with pytest.raises(ValueError, match="max_new_tokens"):
        m.generate(ids, mask, max_new_tokens=4, min_new_tokens=5, eos_token_id=2)
    for bad in ([128], [-1], [5, 200]):
        with pytest.raises(ValueError, match="suppress_tokens"):
            m.generate(ids, mask, max_new_tokens=4, suppress_tokens=bad)
    with pytest.raises(ValueError, match="suppress_tokens"):
        m.generate(ids, mask, max_new_tokens=4, suppress_tokens=list(range(64)))
    with pytest.raises(ValueError, match="int64"):
        m.generate(ids.int(), mask, max_new_tokens=4, repetition_penalty=1.3)
    for on in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(min_new_tokens=2, eos_token_id=2),
               dict(suppress_tokens=list(range(63)))):
        with pytest.raises(RuntimeError, match="no CPU path"):  # accepted: only the device is missing
            m.generate(ids, mask, max_new_tokens=4, **on)
        with pytest.raises(RuntimeError, match="no CPU path"):
            m.generate(ids, mask, max_new_tokens=4, do_sample=True, **on)


@pytest.mark.parametrize("make", [_mpt, _cross_wrapper, _self_wrapper, _llama])
def test_processors_with_beam_search_are_refused(make):
    m = make()
    ids = torch.randint(3, 128, (2, 6))
    for on in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(min_new_tokens=2, eos_token_id=2), dict(suppress_tokens=[5])):
        with pytest.raises(ValueError, match="beam search"):
            m.generate(ids, torch.ones_like(ids), max_new_tokens=4, num_beams=2, **on)


def test_history_ids_belong_to_embeddings_prompts():
    m = _mpt()
    ids = torch.randint(3, 128, (2, 6))
    with pytest.raises(ValueError, match="history_ids"):
        m.generate(ids, torch.ones_like(ids), max_new_tokens=4, repetition_penalty=1.3, history_ids=ids)


def test_arguments_default_to_no_processors():
    from mmgl_amd.language_modelling.run_generation import Arguments
    a = Arguments()
    assert a.repetition_penalty == 1.0 and a.no_repeat_ngram_size == 0 and a.min_new_tokens == 0
