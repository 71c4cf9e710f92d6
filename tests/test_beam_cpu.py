"""CPU: the beam-search surface without a GPU -- ABI 110 and its symbols, the refusals that need no device, and the yardstick of the GPU
tests itself: the plain-Python bookkeeping of tests/beam_ref.py against transformers' generate(num_beams=W) on a CPU OPT model."""
import pytest
import torch

from beam_ref import beam_search_ref
from helpers import mpt_args, tiny_opt_config

EOS = 116


def test_abi_110_and_symbols():
    from mmgl_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION == 110 and L.mmgl_version() == 110
    for name in ("mmgl_attn_decode_beam_fwd", "mmgl_beam_topk", "mmgl_beam_topk_workspace", "mmgl_beam_advance"):
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    # 4 (2 + 4W) bytes per (row, chunk of 4096 logits)
    assert L.mmgl_beam_topk_workspace(64, 50272, 4) == 64 * 13 * 18 * 4
    assert L.mmgl_beam_topk_workspace(1, 128, 1) == 6 * 4


def test_cpu_tensors_are_refused():
    from mmgl_amd import ops
    q, k, m = torch.zeros(4, 32), torch.zeros(2, 3, 32), torch.ones(2, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.attn_decode_beam(q, k, k, m, 2, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.beam_topk(torch.zeros(4, 64), torch.zeros(4), 2)
    book = ops.BeamBook(2, 2, 3, "cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.beam_advance(torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int32), book, 0, 64)
    with pytest.raises(ValueError, match="beams"):
        ops.BeamBook(2, 9, 3, "cpu")


def test_generate_refuses_beam_options_without_a_device():
    from mmgl_amd.model.modelling_cross_attention import MPTConfig, MPTForCausalLM
    m = MPTForCausalLM(MPTConfig(mpt_args(neighbor_mode="raw", peft_type="none"), tiny_opt_config(dropout=0.0))).eval()
    ids = torch.ones(2, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="never"):
        m.generate(ids, num_beams=2, early_stopping="never")
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.generate(ids, num_beams=2, num_return_sequences=2)
    with pytest.raises(ValueError, match="inputs_embeds"):
        m.generate(inputs_embeds=torch.zeros(2, 4, 64), num_beams=2)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(ids, num_beams=0)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.generate(ids, num_beams=2)


@pytest.fixture(scope="module")
def hf_model():
    from transformers import OPTForCausalLM
    torch.manual_seed(1)
    return OPTForCausalLM(tiny_opt_config(dropout=0.0)).eval()


@pytest.mark.parametrize("early_stopping", [False, True])
@pytest.mark.parametrize("length_penalty", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("eos", [None, EOS])
def test_bookkeeping_restatement_agrees_with_transformers(hf_model, W, length_penalty, early_stopping, eos):
    """beam_ref.beam_search_ref fed with the HF model's own uncached log-probs returns what hf.generate returns, for every sample
    whose search met no near-tie (the two sides round their log-probs differently: cached vs uncached forward)."""
    B, T, n_new, V = 8, 12, 8, 128
    g = torch.Generator().manual_seed(1)
    prompt = torch.randint(3, V, (B, T), generator=g)

    def step_logits(hyps):
        rows = len(hyps)
        ids = torch.cat([prompt.repeat_interleave(rows // B, 0), torch.tensor(hyps, dtype=torch.int64).reshape(rows, -1)], 1)
        with torch.no_grad():
            lp = torch.log_softmax(hf_model(ids).logits[:, -1].float(), -1)
        return lp.numpy()

    new, scores, book = beam_search_ref(step_logits, B, W, V, n_new, eos, 1, length_penalty, early_stopping)
    hf_model.generation_config.eos_token_id = eos                       # None: all n_new steps (the config's own EOS is 2)
    with torch.no_grad():
        out = hf_model.generate(prompt, num_beams=W, do_sample=False, early_stopping=early_stopping, length_penalty=length_penalty,
                                max_new_tokens=n_new, min_new_tokens=0, eos_token_id=eos, pad_token_id=1, return_dict_in_generate=True,
                                output_scores=True)
    got = out.sequences[:, T:]
    agree = 0
    for b in range(B):
        want = new[b][:got.shape[1]]
        if got[b].tolist() == want and all(t == 1 for t in new[b][got.shape[1]:]):
            agree += 1
            assert abs(float(out.sequences_scores[b]) - float(scores[b])) <= 1e-4 * max(1.0, abs(float(scores[b])))
    print(f"W={W} lp={length_penalty} es={early_stopping} eos={eos}: {agree} of {B} samples agree")
    assert agree == B, f"{agree} of {B} samples agree with transformers"
    if eos is not None:
        assert any(len(p) and p[0]["len"] < n_new for p in book.pool), "no hypothesis ended on EOS: the case shows nothing"
