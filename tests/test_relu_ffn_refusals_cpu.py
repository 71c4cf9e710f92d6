"""The feature-count refusals of ops.relu_ffn (CPU only: nothing is launched).  Every row of REFUSALS changes the valid call in
exactly one operand; the call must raise ValueError with the whole text below, relu_ffn's name included, on the frozen and on the
trainable route alike -- and before anything reaches the library: lib() and _lib.call are replaced by a function that fails."""
import pytest
import torch

D_IN, FFN, D_OUT = 8, 16, 24      # three different widths: a transposed or swapped operand cannot pass by accident
VALID = dict(x=(3, 5, D_IN), w1=(FFN, D_IN), b1=(FFN,), w2=(D_OUT, FFN), b2=(D_OUT,))

# (the one operand changed, its shape, the text of the ValueError)
REFUSALS = [
    ("x", (3, 5, FFN), "relu_ffn: x has 16 features, fc1 maps 8 to 16, fc2 expects 16"),
    ("x", (D_IN + 1,), "relu_ffn: x has 9 features, fc1 maps 8 to 16, fc2 expects 16"),
    ("w1", (FFN, D_IN - 1), "relu_ffn: x has 8 features, fc1 maps 7 to 16, fc2 expects 16"),
    ("w1", (FFN + 8, D_IN), "relu_ffn: x has 8 features, fc1 maps 8 to 24, fc2 expects 16"),
    ("w2", (D_OUT, FFN - 8), "relu_ffn: x has 8 features, fc1 maps 8 to 16, fc2 expects 8"),
    ("w2", (FFN, D_OUT), "relu_ffn: x has 8 features, fc1 maps 8 to 16, fc2 expects 24"),          # fc2 handed over transposed
]


@pytest.mark.parametrize("frozen", [None, True, False], ids=["auto", "frozen", "trainable"])
@pytest.mark.parametrize("operand,shape,text", REFUSALS, ids=[f"{r[0]}-{'x'.join(map(str, r[1]))}" for r in REFUSALS])
def test_relu_ffn_refuses_before_the_library(monkeypatch, operand, shape, text, frozen):
    from mmgl_amd import _lib, ops

    def reached(*a, **k):
        raise AssertionError("relu_ffn reached the library with mismatched feature counts")
    monkeypatch.setattr(ops, "lib", reached)
    monkeypatch.setattr(_lib, "lib", reached)
    monkeypatch.setattr(_lib, "call", reached)
    t = {k: torch.zeros(dict(VALID, **{operand: shape})[k]) for k in VALID}
    with pytest.raises(ValueError) as e:
        ops.relu_ffn(t["x"].requires_grad_(), t["w1"], t["b1"], t["w2"], t["b2"], frozen=frozen)
    assert str(e.value) == text
    if frozen is not True:                # the same call with a trainable fc2: the other route, the same words
        with pytest.raises(ValueError) as e:
            ops.relu_ffn(t["x"], t["w1"], t["b1"], t["w2"].requires_grad_(), t["b2"], frozen=frozen)
        assert str(e.value) == text
