"""Fixture loading + comparison helpers shared by the test modules."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_FIXTURE_BYTES = 1 << 20    # every committed file stays below 1 MiB: a larger fixture is <stem>.npz + <stem>.part1.npz + ...


def load_golden(name):
    """The arrays of the fixture tests/golden/<name> (<stem>.npz) and of its continuation files <stem>.part1.npz, .part2.npz, ..."""
    out, k, path = {}, 0, os.path.join(GOLDEN, name)
    while os.path.exists(path):
        with np.load(path, allow_pickle=False) as z:
            out.update((n, z[n]) for n in z.files)
        k += 1
        path = os.path.join(GOLDEN, f"{name[:-4]}.part{k}.npz")
    if not out:
        raise FileNotFoundError(os.path.join(GOLDEN, name))
    return out


def save_golden(path, flat):
    """np.savez_compressed of `flat` as <stem>.npz plus as many continuation files as keep every file below MAX_FIXTURE_BYTES
    (consecutive runs of keys, in order); returns the paths written"""
    import glob
    stem = path[:-4]
    for n in range(1, len(flat) + 1):
        for old in glob.glob(stem + ".part*.npz"):
            os.remove(old)
        keys = list(flat)
        chunks = [keys[i * len(keys) // n:(i + 1) * len(keys) // n] for i in range(n)]
        paths = [path] + [f"{stem}.part{k}.npz" for k in range(1, n)]
        for p, ks in zip(paths, chunks):
            np.savez_compressed(p, **{key: flat[key] for key in ks})
        if all(os.path.getsize(p) < MAX_FIXTURE_BYTES for p in paths):
            return paths
    raise ValueError(f"{path}: a single array is larger than {MAX_FIXTURE_BYTES} bytes compressed")


class Fixture:
    def __init__(self, name):
        z = load_golden(name)
        self.meta = json.loads(str(z["meta"]))
        self.groups = {}
        for k in z:
            if k == "meta":
                continue
            g, n = k.split("/", 1)
            self.groups.setdefault(g, {})[n] = torch.from_numpy(np.array(z[k]))

    def __getattr__(self, g):
        try:
            return self.__dict__["groups"][g]
        except KeyError:
            raise AttributeError(g)

    @property
    def inp(self):
        return self.groups["in"]


def rel_err(a: torch.Tensor, b: torch.Tensor, floor: float = 1e-6) -> float:
    """max|a-b| / max(max|b|, floor) -- the 'relative fp32' measure BASELINE.json's 1e-3 tolerance is stated in.
    The floor keeps analytically-zero tensors (e.g. d k_proj.bias: softmax is invariant to a per-row score shift)
    from turning 1e-10 round-off into a relative error."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), floor)


def elementwise_err(a: torch.Tensor, b: torch.Tensor, floor_frac: float = 1e-3, abs_floor: float = 1e-6) -> float:
    """max over elements of |a - b| / (|b| + floor_frac * max|b|): an element-wise relative error (rel_err above is a max-norm measure:
    a small element of a tensor with a large maximum can be wrong by many times its own size and pass).  The floor -- a fraction of the
    tensor's largest magnitude -- keeps elements that are analytically ~0 from dividing round-off by nothing."""
    a = a.detach().double()
    b = b.detach().double().to(a.device)      # on the device `a` lives on: a [40960, 8192] gradient is checked where it was computed
    floor = max(floor_frac * b.abs().max().item(), abs_floor)      # abs_floor: analytically-zero tensors (d k_proj.bias) are round-off on both sides
    return ((a - b).abs() / (b.abs() + floor)).max().item()


def slice_err(a: torch.Tensor, b: torch.Tensor, keep, floor_frac: float = 1e-3) -> torch.Tensor:
    """Per-slice max-norm relative error: for every index along the dims in `keep` (e.g. (0, 2) of a [B, T, H, D] tensor: one
    (sample, head) slice), max|a - b| / max|b| over the slice's other elements.  Returns the errors indexed by the `keep` dims.
    A whole-tensor maximum hides a defect confined to one chunk, trip, head or split; this measure does not.  The floor -- a fraction
    of the WHOLE tensor's largest magnitude -- keeps an analytically-zero slice (dQ of a sample with one valid key) from dividing
    round-off by nothing."""
    a = a.detach().double()
    b = b.detach().double().to(a.device)
    red = [i for i in range(b.dim()) if i not in keep]
    d = (a - b).abs().amax(dim=red)
    m = b.abs().amax(dim=red)
    return (d / m.clamp_min(max(floor_frac * float(m.max()), 1e-30))).cpu()


def tile_err(a: torch.Tensor, b: torch.Tensor, tile: int = 256, floor_frac: float = 1e-3) -> float:
    """Largest slice_err over the tile x tile blocks of a 2-D tensor (ragged edge blocks included): a weight gradient whose one
    output tile or one K split is off shows here even when the tensor's maximum lies in another tile."""
    R, C = b.shape
    pr, pc = (-R) % tile, (-C) % tile
    pad = lambda t: torch.nn.functional.pad(t.detach().double(), (0, pc, 0, pr))
    a, b = pad(a), pad(b.to(a.device))
    return float(slice_err(a.view(-1, tile, a.shape[1] // tile, tile), b.view(-1, tile, b.shape[1] // tile, tile), (0, 2), floor_frac).max())


def assert_close(a, b, tol, what="", floor=1e-6):
    e = rel_err(a, b, floor)
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"
    return e


# ------------------------------------------------------------------------------------------ tiny model builders
def tiny_opt_config(pre_ln=True, proj=None, dropout=0.1):
    from transformers import OPTConfig
    return OPTConfig(vocab_size=128, hidden_size=64, num_attention_heads=4, ffn_dim=128, num_hidden_layers=4,
                     max_position_embeddings=64, word_embed_proj_dim=proj or 64, do_layer_norm_before=pre_ln,
                     dropout=dropout, attention_dropout=0.0, pad_token_id=1, bos_token_id=2, eos_token_id=2, init_std=0.08)


def tiny_roberta_config():
    from transformers import RobertaConfig
    return RobertaConfig(vocab_size=128, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                         max_position_embeddings=40, pad_token_id=1, type_vocab_size=1, hidden_dropout_prob=0.0,
                         attention_probs_dropout_prob=0.0)


def tiny_clip_vision_config():
    from transformers import CLIPVisionConfig
    return CLIPVisionConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2, image_size=32,
                            patch_size=16)


def mpt_args(**kw):
    from types import SimpleNamespace
    a = dict(context="all", neighbor_mode="cross_attention", n_text_tokens=2, n_visual_tokens=2, text_model="roberta-tiny",
             visual_model="clip-vit-tiny", max_output_length=8, freeze_lm=False, model_name_or_path="opt-tiny",
             peft_type="flamingo", lora_r=4, lora_alpha=1.0, lora_dropout=0.0, neighbor_layer_wise=2, decoder_only=True,
             position_type="none", max_text_neighbors=3, max_image_neighbors=2)
    a.update(kw)
    return SimpleNamespace(**a)


def load_exact(module, state, prefix=""):
    """load_state_dict(strict) from a fixture group, ignoring fixture keys outside `prefix`."""
    sd = {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}
    missing, unexpected = module.load_state_dict(sd, strict=False)
    missing = [k for k in missing if "position_ids" not in k]
    assert not missing, f"missing keys: {missing[:5]}"
    assert not [k for k in unexpected if "position_ids" not in k], f"unexpected keys: {unexpected[:5]}"
