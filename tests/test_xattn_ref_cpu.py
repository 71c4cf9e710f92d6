"""attn_ref.XAttnRef, the fp64 reference behind tests/test_xattn_bounds_gpu.py, on the CPU (no GPU needed):

(a) it IS the oracle's attention: oracle.lm_ref.expand_mask + attention_core under autograd in fp64, to 1e-12, on out, lse, dq, dk, dv
    (lse of a sample without a valid key excepted: the kernel's convention is log S, the oracle's finfo.min + log S);
(b) the comparison it carries can fail: for the mask layouts of the GPU file (all valid | holed | no valid key) every deliberately
    wrong reference leaves the bf16 bound -- the looser one -- on at least 25 % of the elements it reaches, from the references alone;
(c) with plain randn inputs the same wrong references stay below that at S >= 129: why every case uses the edge-key / edge-row inputs.

What a wrong reference reaches: the samples and tensors it can alter at all.
  * a dropped key (S - 1, the first key of the last 32-key group, key 0): the samples where that key is valid or that have no valid
    key; out, lse, dq on every row, dk, dv on the keys that are valid there (all S keys of a sample without a valid key);
  * a masked edge key read as valid (the first masked edge key of a holed sample), the mask shifted by one key: the samples whose
    set of valid keys changes; the same tensors, dk / dv on the keys valid on either side;
  * head h reading head h + 1's keys: every sample; lse only where a sample has a valid key (log S does not depend on the head);
  * a query row missing from dK / dV (row T - 1, row 32): dk, dv of every sample, on the valid keys;
  * tie factor 1: dq, dk of the samples without a valid key; uniform over the padded key block: all five tensors of those samples,
    where S is no multiple of the block (S = 256 pads to itself: nothing changes, not counted).
The 25 % is asserted per wrong reference and shape with its tensors pooled; each tensor's own fraction is printed.  A sample without
a valid key on its own (the GPU file's B = 1 case) has p = 1 / S whatever the inputs hold: there a dropped key is held to the cap under
the fp32 bound from S = 128 on (see that test).  DESIGN.md 4.9c has the table."""
import functools

import pytest
import torch

from attn_ref import XAttnRef
from bounds import BF16

CAP = 0.25
B, H, T = 3, 3, 130
SEED = 0
SHAPES = [(S, D) for S in (33, 65, 129, 200, 256) for D in (16, 64, 128)]


# ------------------------------------------------------------------------------------------ (a) the reference is the oracle
@pytest.mark.parametrize("Hh,S,first", [(1, 40, 0), (3, 33, 0), (4, 70, 1), (2, 129, 2), (3, 1, 0)])
def test_ref_is_the_oracle_in_fp64(Hh, S, first):
    from oracle import lm_ref
    Tq, D, Bq = 37, 16, 4
    q, k, v, dout = XAttnRef.inputs(torch.float64, Bq, Tq, S, Hh, D, seed=5 + Hh)
    am = XAttnRef.mask(Bq, S, first)
    live = am.bool().any(1)
    assert live.any() and not live.all(), "a fully masked sample next to live ones"
    ref = XAttnRef(q, k, v, am, dout, Hh)
    qr, kr, vr = (t.clone().requires_grad_() for t in (q, k, v))
    add = lm_ref.expand_mask(am, torch.float64, Tq)
    out = lm_ref.attention_core(qr, kr, vr, add, Hh)
    (out * dout).sum().backward()
    sc = q.reshape(Bq, Tq, Hh, D).permute(0, 2, 1, 3) @ k.reshape(Bq, S, Hh, D).permute(0, 2, 3, 1)
    lse = torch.logsumexp(torch.maximum(sc + add, torch.tensor(torch.finfo(torch.float64).min, dtype=torch.float64)), -1)
    got = dict(out=out.detach(), lse=lse, dq=qr.grad, dk=kr.grad, dv=vr.grad)
    for name in XAttnRef.NAMES:
        want, x = ref.want[name], got[name].reshape(ref.want[name].shape)
        if name == "lse":               # the oracle's finfo.min + log S is another convention: the tie excludes those samples
            assert torch.equal(want[~live], torch.full_like(want[~live], float(torch.log(torch.tensor(float(S), dtype=torch.float64)))))
            want, x = want[live], x[live]
        e = (x - want).abs().max().item() / max(want.abs().max().item(), 1e-300)
        assert e <= 1e-12, f"{name}: {e:.2e}"
        if name != "lse":
            assert (ref.mag[name] >= ref.want[name].abs() * (1 - 1e-12)).all(), f"{name}: mag below |want|"
    if S > 1:                           # the holed sample: a masked key gets exactly zero dk and dv
        dead = ~am.bool() & live[:, None]
        assert dead.any() and float(ref.want["dk"][dead].abs().max()) == 0.0 and float(ref.want["dv"][dead].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ (b) the comparison can fail
ALL5, GRADS_KV = ("out", "lse", "dq", "dk", "dv"), ("dk", "dv")


def _mutants(am, S):
    """name -> (XAttnRef keyword arguments, {tensor: samples reached [B] bool}, keys reached for dk / dv [B,S] bool)."""
    ok = am.bool()
    Bq = ok.shape[0]
    live = ok.any(1)
    every = torch.ones(Bq, dtype=torch.bool)
    keys0 = ok | ~live[:, None]                      # the keys that carry a gradient at all
    m = {}
    for name, j in (("key-last-dropped", S - 1), ("key-first-of-last-group-dropped", 32 * ((S - 1) // 32)), ("key0-dropped", 0)):
        hit = ok[:, j] | ~live
        bad, ex = ok.clone(), torch.ones_like(ok)
        bad[:, j] = False
        ex[:, j] = False
        m[name] = (dict(allowed=bad, exists=ex), {t: hit for t in ALL5}, keys0)
    bad, hit = ok.clone(), torch.zeros(Bq, dtype=torch.bool)
    for b in range(Bq):
        masked_edges = [e for e in XAttnRef.edges(S) if live[b] and not ok[b, e]]
        if masked_edges:
            bad[b, masked_edges[0]] = True
            hit[b] = True
    m["masked-edge-key-valid"] = (dict(allowed=bad), {t: hit for t in ALL5}, keys0 | bad)
    bad = ok.clone()
    bad[:, 1:] = ok[:, :-1]
    m["mask-shifted"] = (dict(allowed=bad), {t: (bad != ok).any(1) for t in ALL5}, keys0 | bad)
    m["head-plus-one"] = (dict(kv_head=lambda h: (h + 1) % H), {t: (live if t == "lse" else every) for t in ALL5}, keys0)
    for name, row in (("row-last-missing", T - 1), ("row32-missing", 32)):
        rows = torch.ones(T, dtype=torch.bool)
        rows[row] = False
        m[name] = (dict(rows_kv=rows), {t: every for t in GRADS_KV}, keys0)
    m["tie-factor-1"] = (dict(tie=1.0), {t: ~live for t in ("dq", "dk")}, keys0)
    spad = 32 if S <= 32 else 64 if S <= 64 else 128 if S <= 128 else 256          # DISPATCH_NSB's key blocks
    m["uniform-over-padded-block"] = (dict(uniform_n=lambda b: spad), {t: ~live & (spad != S) for t in ALL5}, keys0)
    return m


@functools.lru_cache(maxsize=None)
def _fractions(S, D, edge, first=0, Bq=B, dtype=BF16):
    """{(mutant, tensor): fraction of the reached elements outside the `dtype` bound}, from the references alone (the operands are
    bf16-rounded either way)."""
    q, k, v, dout = XAttnRef.inputs(BF16, Bq, T, S, H, D, seed=SEED, edge=edge)
    am = XAttnRef.mask(Bq, S, first)
    ref = XAttnRef(q, k, v, am, dout, H)
    res = {}
    for name, (kw, reach, keys) in _mutants(am, S).items():
        wrong = XAttnRef(q, k, v, am, dout, H, **kw)
        n_out = n_all = 0
        for tensor, samples in reach.items():
            o = ref.outside(wrong, tensor, dtype)
            o = o[samples] if tensor in ("out", "lse", "dq") else o[samples[:, None] & keys]
            if o.numel():
                res[name, tensor] = o.double().mean().item()
                n_out, n_all = n_out + int(o.sum()), n_all + o.numel()
        if n_all:
            res[name, "all"] = n_out / n_all
    return res


NAMES = ("key-last-dropped", "key-first-of-last-group-dropped", "key0-dropped", "masked-edge-key-valid", "mask-shifted", "head-plus-one",
         "row-last-missing", "row32-missing", "tie-factor-1", "uniform-over-padded-block")


def _report(tag, res):
    low = []
    for (name, tensor), frac in res.items():
        print(f"[can-fail {tag}] {name} {tensor}: {frac:.0%}")
        if tensor == "all" and frac < CAP:
            low.append(f"{name}: {frac:.0%} (" + ", ".join(f"{t} {res[name, t]:.0%}" for t in ALL5 if (name, t) in res) + ")")
    return low


@pytest.mark.parametrize("S,D", SHAPES)
def test_wrong_references_leave_the_bound(S, D):
    res = _fractions(S, D, True)
    low = _report(f"S{S} D{D}", res)
    seen = {name for (name, _) in res}
    want = set(NAMES) - ({"uniform-over-padded-block"} if S == 256 else set())
    assert want <= seen, f"mutants never exercised: {want - seen}"
    assert not low, f"S={S} D={D}: a wrong reference stays inside the bf16 bound on more than {1 - CAP:.0%} of what it reaches:\n" + "\n".join(low)


KEY_DROPS = ("key-last-dropped", "key-first-of-last-group-dropped", "key0-dropped")


@pytest.mark.parametrize("S,D", [(33, 64), (200, 16), (129, 128), (256, 64)])
def test_wrong_references_leave_the_bound_single_masked_sample(S, D):
    """The GPU file's B = 1 case: one sample, no valid key.  Its probabilities are 1 / S whatever the operands hold, so no input can
    make one key carry more than 1 / S of a row: a dropped key moves an element by about mag / S, under the bf16 bound (2^-7 mag)
    from S = 128 on whatever the kernel does (measured: 53 % at S = 33, 14 % at S = 129, 7 % at S = 200).  The three dropped-key
    references are therefore held to the cap under the fp32 bound there -- the GPU case runs in both dtypes -- and every other wrong
    reference under the bf16 bound as everywhere."""
    res = _fractions(S, D, True, first=2, Bq=1)
    res32 = _fractions(S, D, True, first=2, Bq=1, dtype=torch.float32)
    if S >= 128:
        res = {k: (res32[k] if k[0] in KEY_DROPS else x) for k, x in res.items()}
    low = _report(f"B1 S{S} D{D}", res)
    want = {"tie-factor-1", "row-last-missing", "row32-missing", "head-plus-one", *KEY_DROPS} | ({"uniform-over-padded-block"} if S != 256 else set())
    assert want <= {n for (n, _) in res}
    assert not low, "\n".join(low)


def test_plain_randn_inputs_do_not_meet_the_cap():
    """Why the recipe exists: on plain randn inputs at S >= 129 a key carries under 1 % of a row and one of ~130 query rows as
    little of a key's gradient, so the dropped keys, the masked key read as valid and the missing rows stay inside the bound (3-19 %)."""
    for S in (129, 200, 256):
        res = _fractions(S, 64, False)
        for name in KEY_DROPS + ("masked-edge-key-valid", "row-last-missing", "row32-missing"):
            frac = res[name, "all"]
            print(f"[randn S{S} D64] {name}: {frac:.0%}")
            assert frac < CAP, f"plain randn already shows {name} on {frac:.0%}"
