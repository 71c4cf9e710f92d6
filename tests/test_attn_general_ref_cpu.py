"""attn_ref.GeneralAttnRef and attn_ref.EncAttnRef, the fp64 references behind tests/test_attn_general_bounds_gpu.py and
tests/test_encattn_bounds_gpu.py, on the CPU (no GPU needed), with the GPU files' inputs and seed:

(a) GeneralAttnRef IS the oracle's attention: oracle.lm_ref.attention_core under autograd in fp64 with expand_mask /
    decoder_self_mask, the reference's own keep mask and head mask, to 1e-12 on out, probs, dq, dk, dv (lse against the logsumexp of the
    clamped scores on the rows with an allowed key; the others carry the kernel's +inf marker) -- cross and causal, holed masks, samples
    and rows without an allowed key, doubly-masked keys;  EncAttnRef is a plain per-sequence fp64 softmax;
(b) hash_keep at this kernel's element index ((b H + h) T + t) S + s is hash32_int (Python integers) on a sample of indices;
(c) the comparison can fail: every deliberately wrong reference, built from the classes alone, leaves the bf16 bound on at least 40 %
    of the elements it reaches, its tensors pooled;
(d) the same operations in torch fp32 arithmetic with the store rounded to the dtype stay inside every bound.

What a wrong reference reaches: the tensors it can alter at all, on the rows / keys / heads named with each one below, and of those
only the elements that can be non-zero in either reference (mag > 0: a head with head_mask 0, a masked key of a sample whose rows
all have an allowed key hold exact zeros on both sides and no bound can tell the references apart).  For a key dropped or added under
the causal ramp the window is SelfAttnRef's: the query rows within 8 after the key, the key rows within 8 before it.  DESIGN.md 4.9f
has the table."""
import functools

import numpy as np
import pytest
import torch

from attn_ref import EncAttnRef, GeneralAttnRef, XAttnRef
from bounds import BF16, F32, drop_threshold, hash32_int, hash_keep

F64 = torch.float64
CAP = 0.40
SEED = 0
P_DROP, DSEED = 0.3, 0x9E3779B97F4A7C15          # the GPU files' dropout seed: its top bit is set
HM = (1.0, 0.0, 0.5, 2.0)


def _hm(H):
    return torch.tensor(HM[:H])


# ------------------------------------------------------------------------------------------ (a) the references are the oracle
ORACLE = [
    # causal, H, T, S, left padding, first mask layout, p_drop, head mask
    (False, 3, 37, 40, 0, 0, 0.0, False),
    (False, 3, 37, 70, 0, 1, 0.5, True),
    (False, 2, 20, 129, 0, 2, 0.75, True),
    (False, 3, 5, 1, 0, 0, 0.0, False),
    (True, 3, 70, 70, 0, 0, 0.0, False),
    (True, 3, 70, 70, 5, 0, 0.5, True),
    (True, 2, 90, 90, 70, 0, 0.75, True),
    (True, 2, 33, 33, 33, 0, 0.5, False),         # sample 0: every key padded
]


@pytest.mark.parametrize("causal,H,T,S,left,first,p,use_hm", ORACLE)
def test_general_ref_is_the_oracle_in_fp64(causal, H, T, S, left, first, p, use_hm):
    from oracle import lm_ref
    Bq, D = 3, 16
    q, k, v, dout = GeneralAttnRef.inputs(F64, Bq, T, S, H, D, causal, seed=5 + H)
    am = GeneralAttnRef.causal_mask(Bq, T, left) if causal else XAttnRef.mask(Bq, S, first)
    hm = _hm(H).double() if use_hm else None
    keep = GeneralAttnRef.keep(DSEED, Bq, H, T, S, p) if p > 0 else None
    # p = 0.5, 0.75: 1 / (1 - p) is the same number in fp32 and fp64
    ref = GeneralAttnRef(q, k, v, am, dout, H, causal=causal, head_mask=hm, p_drop=p, seed=DSEED)
    qr, kr, vr = (t.clone().requires_grad_() for t in (q, k, v))
    add = lm_ref.decoder_self_mask(am.bool(), F64) if causal else lm_ref.expand_mask(am.bool(), F64, T)
    out, probs = lm_ref.attention_core(qr, kr, vr, add, H, head_mask=hm, keep=keep, p_drop=p, return_probs=True)
    (out * dout).sum().backward()
    sc = q.reshape(Bq, T, H, D).permute(0, 2, 1, 3) @ k.reshape(Bq, S, H, D).permute(0, 2, 3, 1)
    lse = torch.logsumexp(torch.maximum(sc + add, torch.tensor(torch.finfo(F64).min, dtype=F64)), -1)
    got = dict(out=out.detach(), lse=lse, dq=qr.grad, dk=kr.grad, dv=vr.grad, probs=probs.detach())
    uni = ref.uni_rows
    for name in GeneralAttnRef.NAMES + ("probs",):
        want, x = ref.want[name], got[name].reshape(ref.want[name].shape)
        if name == "lse":
            sel = uni[:, None, :].expand_as(want)
            assert bool(torch.isinf(want[sel]).all()) and bool((want[sel] > 0).all())
            want, x = want[~sel], x[~sel]
        e = (x - want).abs().max().item() / max(want.abs().max().item(), 1e-300)
        assert e <= 1e-12, f"{name}: {e:.2e}"
        if name in ref.mag:
            assert (ref.mag[name] >= ref.want[name].abs() * (1 - 1e-12)).all(), f"{name}: mag below |want|"
    if left:
        assert bool(uni[0, :left].all()) and not bool(uni[1:].any())
        dbl = ref.double[0] & uni[0][:, None]
        assert left >= T or bool(dbl.any()), "no doubly-masked key"
    # a masked key that no row without an allowed key reaches holds exact zeros
    dead = ~am.bool() & ~uni.any(1)[:, None]
    if bool(dead.any()):
        assert float(ref.want["dk"][dead].abs().max()) == 0.0 and float(ref.want["dv"][dead].abs().max()) == 0.0
        assert float(ref.want["probs"].permute(0, 3, 1, 2)[dead].abs().max()) == 0.0


def test_oracle_cases_cover_the_semantics():
    kinds = set()
    for causal, H, T, S, left, first, p, use_hm in ORACLE:
        am = GeneralAttnRef.causal_mask(3, T, left) if causal else XAttnRef.mask(3, S, first)
        none = ~am.bool().any(1)
        kinds |= {("causal" if causal else "cross", "sample-without-key" if x else "live") for x in none.tolist()}
        if not causal and bool((~am.bool() & ~none[:, None]).any()):
            kinds.add("holed")
        if causal and 0 < left < T:
            kinds.add("rows-without-key")
        if p > 0 and use_hm:
            kinds.add("dropout+head-mask")
    assert kinds >= {("cross", "live"), ("cross", "sample-without-key"), ("causal", "live"), ("causal", "sample-without-key"),
                     "rows-without-key", "dropout+head-mask", "holed"}


ENC_LENS = (1, 129, 15, 64, 17, 63, 16, 128, 65, 257, 127)


@pytest.mark.parametrize("H,D", [(2, 16), (3, 64)])
def test_enc_ref_is_a_per_sequence_softmax(H, D):
    q, k, v = EncAttnRef.inputs(F64, ENC_LENS, H, D, seed=SEED)
    cu = EncAttnRef.cu(ENC_LENS)
    ref = EncAttnRef(q, k, v, cu, H)
    n = q.shape[0]
    q3, k3, v3 = (t.reshape(n, H, D) for t in (q, k, v))
    a = 0
    for L in ENC_LENS:
        for h in range(H):
            s = q3[a:a + L, h] @ k3[a:a + L, h].t()
            e = (s - s.amax(1, keepdim=True)).exp()
            o = (e / e.sum(1, keepdim=True)) @ v3[a:a + L, h]
            assert (ref.want["out"][a:a + L, h] - o).abs().max().item() <= 1e-12
            assert (ref.mag["out"][a:a + L, h] >= o.abs() * (1 - 1e-12)).all()
        a += L
    assert bool(ref.rows(1).sum() == len(ENC_LENS)) and bool(ref.rows().all()) and int(ref.rows(16).sum()) == sum(min(L, 16) for L in ENC_LENS)


# ------------------------------------------------------------------------------------------ (b) the keep mask's index layout
def test_hash_keep_at_this_kernels_index_is_hash32_int():
    Bq, H, T, S, p = 3, 3, 70, 130, P_DROP
    for seed in (DSEED, 12345):
        kp = GeneralAttnRef.keep(seed, Bq, H, T, S, p)
        flat = hash_keep(seed, Bq * H * T * S, p)
        thr = drop_threshold(p)
        rng = np.random.default_rng(1)
        picks = [(0, 0, 0, 0), (Bq - 1, H - 1, T - 1, S - 1), (1, 2, 63, 64), (2, 0, 64, 129), (0, 1, 69, 0)]
        picks += [tuple(int(x) for x in (rng.integers(Bq), rng.integers(H), rng.integers(T), rng.integers(S))) for _ in range(300)]
        for b, h, t, s in picks:
            i = ((b * H + h) * T + t) * S + s
            want = hash32_int(seed, i) >= thr
            assert bool(kp[b, h, t, s]) == want == bool(flat[i]), (seed, b, h, t, s)
        # the shifted / transposed masks of (c) are really other masks
        for kw in (dict(dkey=1), dict(drow=1), dict(swap=True)):
            other = GeneralAttnRef.keep(seed, Bq, H, T, S, p, **kw)
            assert 0.3 < float((other != kp).double().mean()) < 0.55       # 2 p (1 - p) = 0.42
        assert bool((GeneralAttnRef.keep(seed, Bq, H, T, S, p, dkey=1).flatten()[:-1] == kp.flatten()[1:]).all())
        assert bool((GeneralAttnRef.keep(seed, Bq, H, T, S, p, drow=1)[:, :, :-1] == kp[:, :, 1:])[0, 0].all())
    assert abs(float(kp.double().mean()) - (1 - p)) < 0.01


# ------------------------------------------------------------------------------------------ (c) the comparison can fail
ROWT, KEYT = ("out", "lse", "dq", "probs"), ("dk", "dv")
CASES = {
    # name: (causal, B, H, T, S, left)
    "cross": (False, 3, 3, 70, 130, 0),
    "causal-left5": (True, 3, 3, 130, 130, 5),
    "causal-left70": (True, 3, 3, 150, 150, 70),
}


def _setup(case, D):
    causal, Bq, H, T, S, left = CASES[case]
    q, k, v, dout = GeneralAttnRef.inputs(BF16, Bq, T, S, H, D, causal, seed=SEED)
    am = GeneralAttnRef.causal_mask(Bq, T, left) if causal else XAttnRef.mask(Bq, S, 0)
    kw = dict(causal=causal, head_mask=_hm(H), p_drop=P_DROP, seed=DSEED)
    return (q, k, v, am, dout, H), kw


def _mutants(case, ref):
    """name -> (keyword arguments, tensors, rows [B,T], keys [B,S], heads [H]) of the wrong references of `case`."""
    causal, Bq, H, T, S, left = CASES[case]
    hm = _hm(H)
    every_r, every_k, every_h = torch.ones(Bq, T, dtype=torch.bool), torch.ones(Bq, S, dtype=torch.bool), torch.ones(H, dtype=torch.bool)
    nz = hm != 0
    uni, ok, valid, dbl = ref.uni_rows, ref.true_ok, ref.valid, ref.double
    has_uni = uni.any(1)
    GR = ("out", "dq", "dk", "dv")
    m = {}
    for name, kw in (("keep-T-S-swapped", dict(swap=True)), ("keep-one-key-off", dict(dkey=1)), ("keep-one-row-off", dict(drow=1))):
        m[name] = (dict(keep=GeneralAttnRef.keep(DSEED, Bq, H, T, S, P_DROP, **kw)), GR, every_r, every_k, nz)
    m["keep-scale-missing"] = (dict(keep_scale=1.0), GR, every_r, every_k, nz)
    m["head-mask-of-h+1"] = (dict(hm_of=lambda h: (h + 1) % H), GR + ("probs",), every_r, every_k, hm != hm.roll(-1))
    m["head-mask-missing-from-delta"] = (dict(hm_in_delta=False), ("dq", "dk"), every_r, every_k, hm != 1)
    # rows without an allowed key: the samples that have them
    mixed = has_uni & valid.any(1)                      # ... next to valid keys: uniform over the valid keys only is another thing
    if bool(mixed.any()):
        uk = torch.where(mixed[:, None], valid, torch.ones_like(valid))
        m["uniform-over-valid-keys-only"] = (dict(uniform_keys=uk), ("out", "probs", "dq"), uni & mixed[:, None], every_k, nz)
    if bool(has_uni.any()):
        m["tie-1.0"] = (dict(tie=1.0), ("dq", "dk"), uni, has_uni[:, None] & every_k, nz)
    dkeys = (dbl & uni[:, :, None]).any(1)              # keys doubly masked for some row without an allowed key
    if bool(dkeys.any()):
        m["tie-0.5-on-doubly-masked"] = (dict(tie_double=0.5), ("dk",), uni & (dbl & uni[:, :, None]).any(2), dkeys, nz)
    t, s = torch.arange(T)[:, None], torch.arange(S)[None, :]
    win = lambda j: (((torch.arange(T) >= j) & (torch.arange(T) <= j + 8))[None].expand(Bq, T),
                     ((torch.arange(S) >= j - 8) & (torch.arange(S) <= j))[None].expand(Bq, S))
    ALL = ROWT + KEYT

    def masked(name, bad, rows, keys, j=None):
        bad = torch.where(bad.any(2, keepdim=True), bad, ok)                # a row never loses its last key: it keeps the true mask
        changed = (bad != ok).any(2) & ~uni & rows
        if j is not None:               # no more key rows than query rows changed (one changed row moves the dropped key's gradient only)
            back = (changed.sum(1, keepdim=True) - 1).clamp(0, 8)
            keys = keys & (torch.arange(S)[None, :] >= j - back)
        if bool(changed.any()):
            m[name] = (dict(allowed=bad), ALL, changed, keys & (valid | has_uni[:, None]), nz)

    if causal:
        masked("diagonal-missed", ok & (s != t)[None], every_r, every_k)
        masked("next-visible", (valid[:, None, :] & (s <= t + 1)[None]), every_r, every_k)
    for name, j in (("key63-dropped", 63), ("key64-dropped", 64), ("keylast-dropped", S - 1)):
        bad = ok.clone()
        bad[:, :, j] = False
        rows, keys = win(j) if causal else (every_r, every_k)
        masked(name, bad, rows, keys, j if causal else None)
    r0 = 32 * ((T - 1) // 32)
    rk = torch.ones(T, dtype=torch.bool)
    rk[r0:] = False
    # under the causal ramp the missing rows read the keys next to them: the window again, 8 keys before the chunk and the chunk itself
    kwin = (torch.arange(S)[None, :] >= r0 - 8) if causal else every_k
    m["last-row-chunk-missing"] = (dict(rows_kv=rk), KEYT, every_r, kwin & (valid | has_uni[:, None]), nz)
    return m


def _select(name, x, rows, keys, heads):
    """The reached elements of tensor `name` (shaped like want[name])."""
    if name in ("out", "dq"):
        sel = rows[:, :, None, None] & heads[None, None, :, None]
    elif name == "lse":
        sel = rows[:, None, :] & heads[None, :, None]
    elif name == "probs":
        sel = rows[:, None, :, None] & heads[None, :, None, None]
    else:
        sel = keys[:, :, None, None] & heads[None, None, :, None]
    return sel.expand_as(x)


@functools.lru_cache(maxsize=None)
def _fractions(case, D):
    """{(mutant, tensor): fraction of the reached elements outside the bf16 bound}, from the references alone."""
    args, kw = _setup(case, D)
    ref = GeneralAttnRef(*args, **kw)
    res = {}
    for name, (mkw, tensors, rows, keys, heads) in _mutants(case, ref).items():
        wrong = GeneralAttnRef(*args, **{**kw, **mkw})
        n_out = n_all = 0
        for tn in tensors:
            if tn == "lse" and "allowed" not in mkw:
                continue
            sel = _select(tn, ref.want[tn], rows, keys, heads)
            if tn in ref.mag:
                sel = sel & ((ref.mag[tn] > 0) | (wrong.mag[tn] > 0))
            elif tn == "probs":
                sel = sel & ((ref.want[tn] != 0) | (wrong.want[tn] != 0))
            else:
                sel = sel & torch.isfinite(ref.want[tn])
            o = ref.outside(wrong, tn, BF16)[sel]
            if o.numel():
                res[name, tn] = o.double().mean().item()
                n_out, n_all = n_out + int(o.sum()), n_all + o.numel()
        if n_all:
            res[name, "all"] = n_out / n_all
    return res


EVERYWHERE = {"keep-T-S-swapped", "keep-one-key-off", "keep-one-row-off", "keep-scale-missing", "head-mask-of-h+1",
              "head-mask-missing-from-delta", "key63-dropped", "key64-dropped", "keylast-dropped", "last-row-chunk-missing"}
EXPECTED = {
    "cross": EVERYWHERE | {"tie-1.0"},
    "causal-left5": EVERYWHERE | {"uniform-over-valid-keys-only", "tie-1.0", "tie-0.5-on-doubly-masked", "diagonal-missed", "next-visible"},
    "causal-left70": EVERYWHERE | {"uniform-over-valid-keys-only", "tie-1.0", "tie-0.5-on-doubly-masked", "diagonal-missed", "next-visible"},
}


@pytest.mark.parametrize("D", [16, 65, 128])
@pytest.mark.parametrize("case", list(CASES))
def test_wrong_references_leave_the_bound(case, D):
    res = _fractions(case, D)
    low = []
    for (name, tn), frac in res.items():
        print(f"[can-fail {case} D{D}] {name} {tn}: {frac:.0%}")
        if tn == "all" and frac < CAP:
            low.append(f"{name}: {frac:.0%} (" + ", ".join(f"{t} {res[name, t]:.0%}" for t in ROWT + KEYT if (name, t) in res) + ")")
    seen = {name for (name, _) in res}
    assert EXPECTED[case] <= seen, f"mutants never exercised: {EXPECTED[case] - seen}"
    assert not low, f"{case} D={D}: a wrong reference stays inside the bf16 bound on more than {1 - CAP:.0%} of what it reaches:\n" + "\n".join(low)


ENC_MUTANTS = {"next-sequence-first-key-visible": dict(next_key=True), "last-key-dropped": dict(drop_last=True), "head-plus-one": None}


@pytest.mark.parametrize("D", [16, 64, 128])
def test_wrong_encoder_references_leave_the_bound(D):
    H = 3
    q, k, v = EncAttnRef.inputs(BF16, ENC_LENS, H, D, seed=SEED)
    cu = EncAttnRef.cu(ENC_LENS)
    ref = EncAttnRef(q, k, v, cu, H)
    bound = ref.bound("out", BF16)
    low = []
    for name, kw in ENC_MUTANTS.items():
        wrong = EncAttnRef(q, k, v, cu, H, **(kw or dict(kv_head=lambda h: (h + 1) % H)))
        reach = torch.ones(q.shape[0], dtype=torch.bool)
        if name == "next-sequence-first-key-visible":       # the last sequence has no next one
            reach[int(cu[-2]):] = False
        if name == "last-key-dropped":                      # a sequence of one token keeps its key
            for i, L in enumerate(ENC_LENS):
                if L == 1:
                    reach[int(cu[i]):int(cu[i + 1])] = False
        frac = ((wrong.want["out"] - ref.want["out"]).abs() > bound)[reach].double().mean().item()
        print(f"[can-fail enc D{D}] {name}: {frac:.0%}")
        if frac < CAP:
            low.append(f"{name}: {frac:.0%}")
    assert not low, "\n".join(low)


# ------------------------------------------------------------------------------------------ (d) fp32 arithmetic stays inside
def _emulate(q, k, v, am, dout, H, causal, hm, p, seed, dtype):
    """The operations of csrc/attn_general.hip in torch fp32 (not its order of summation), outputs rounded once to `dtype`."""
    Bq, T, d = q.shape
    S, D = k.shape[1], d // H
    f = lambda x, n: x.float().reshape(Bq, n, H, D).permute(0, 2, 1, 3)
    Q, K, V, G = f(q, T), f(k, S), f(v, S), f(dout, T)
    t, s = torch.arange(T)[:, None], torch.arange(S)[None, :]
    valid = am.bool()
    past = (s <= t) if causal else torch.ones(T, S, dtype=torch.bool)
    ok = (valid[:, None, :] & past[None])[:, None]                          # [B,1,T,S]
    uni = ~ok.any(3, keepdim=True)
    sc = (Q @ K.transpose(2, 3)).masked_fill(~ok, float("-inf")).masked_fill(uni, 0.0)
    lse = torch.logsumexp(sc, 3, keepdim=True)
    P = torch.where(uni, torch.full_like(sc, 1.0) * (torch.ones((), dtype=F32) / torch.tensor(float(S), dtype=F32)), (sc - lse).exp())
    hmv = (torch.ones(H) if hm is None else hm.float()).view(1, H, 1, 1)
    ks = torch.ones(Bq, H, T, S)
    if p > 0:
        ks = GeneralAttnRef.keep(seed, Bq, H, T, S, p).float() * (torch.ones((), dtype=F32) / (1 - torch.tensor(p, dtype=F32)))
    W = hmv * P
    Wd = W * ks
    O = Wd @ V
    dWd = G @ V.transpose(2, 3)
    delta = (dWd * Wd).sum(3, keepdim=True)
    fac = torch.where(uni, torch.where((~valid[:, None, None, :] & ~past[None, None]), torch.zeros(()), torch.full((), 0.5)), torch.ones(()))
    dS = fac * P * (hmv * ks * dWd - delta)
    back = lambda x: x.permute(0, 2, 1, 3).reshape(Bq, -1, d).to(dtype)
    return dict(out=back(O), lse=lse[..., 0].masked_fill(uni[..., 0], float("inf")), dq=back(dS @ K), dk=back(dS.transpose(2, 3) @ Q),
                dv=back(Wd.transpose(2, 3) @ G), probs=W.to(dtype))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("D", [1, 20, 65, 128])
def test_fp32_arithmetic_stays_inside_the_bound(case, D, dtype):
    """Largest err / bound over the cases (torch fp32 on the CPU; recorded in DESIGN.md 4.9f): far below 1 for every output."""
    causal, Bq, H, T, S, left = CASES[case]
    q, k, v, dout = GeneralAttnRef.inputs(dtype, Bq, T, S, H, D, causal, seed=SEED)
    am = GeneralAttnRef.causal_mask(Bq, T, left) if causal else XAttnRef.mask(Bq, S, 0)
    for hm, p in ((_hm(H), P_DROP), (None, 0.0)):
        ref = GeneralAttnRef(q, k, v, am, dout, H, causal=causal, head_mask=hm, p_drop=p, seed=DSEED)
        ref.check(_emulate(q, k, v, am, dout, H, causal, hm, p, DSEED, dtype), f"{case} D{D} p{p}", "emulated")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_fp32_encoder_arithmetic_stays_inside_the_bound(dtype):
    H, D = 3, 64
    q, k, v = EncAttnRef.inputs(dtype, ENC_LENS, H, D, seed=SEED)
    cu = EncAttnRef.cu(ENC_LENS)
    n = q.shape[0]
    out = torch.empty(n, H, D)
    q3, k3, v3 = (t.float().reshape(n, H, D) for t in (q, k, v))
    for i, L in enumerate(ENC_LENS):
        a = int(cu[i])
        for h in range(H):
            out[a:a + L, h] = torch.softmax(q3[a:a + L, h] @ k3[a:a + L, h].t(), 1) @ v3[a:a + L, h]
    EncAttnRef(q, k, v, cu, H).check(out.to(dtype), f"D{D}", "emulated")
