"""-m gpu: ops.contrastive_select (csrc/contrastive.hip) against the fp64 restatement of tests/contrastive_ref.py.

Tolerances, derived and not measured.  The inputs are the same bf16 / fp32 values on both sides and a product of two bf16 values is exact
in fp32, so what differs is the fp32 accumulation of d terms in the dot product and the two squared norms: |d cos| <= 4 d 2^-24
(1.5e-5 at d = 64, 4.9e-4 at d = 2048).  p is within 4 ulp of exp of the given log-probability.  score is within the cosine bound plus
2^-22.  `selected` is the lowest argmax of the returned score row, exactly; every case's inputs carry a planted context row at a chosen
angle to one candidate so that the reference's margin between best and second score is at least 10 tolerances -- asserted from the
reference before anything is compared -- and there `selected` equals the reference's."""
import numpy as np
import pytest
import torch

from contrastive_ref import rank_ref
from mmgl_amd import ops

pytestmark = pytest.mark.gpu

C = ops.CONTRASTIVE_CTX_CHUNK
V = 1000
ALPHA = 0.6


def cos_tol(d):
    return 4 * d * 2.0 ** -24


def _case(B, k, d, n_ctx, dtype, seed, n_cap=None, plant=None, angle=0.95):
    """CPU tensors of one call.  plant: per sample (candidate, context row): that row is set at cosine `angle` to that candidate,
    every other row is random (cosines ~ N(0, 1/d)), so the candidate's penalty sits on that row."""
    g = torch.Generator().manual_seed(seed)
    n_cap = n_ctx + 1 if n_cap is None else n_cap
    cand = torch.randn(B * k, d, generator=g)
    ctx = torch.randn(B, n_cap, d, generator=g)
    if plant is None:
        plant = [(b % k, (7 * b + n_ctx // 2) % n_ctx) for b in range(B)] if n_ctx else []
    for b, (c, j) in enumerate(plant):
        h = cand[b * k + c]
        u = torch.randn(d, generator=g)
        u = u - (u @ h) / (h @ h) * h
        ctx[b, j] = 3.0 * (angle * h / h.norm() + (1 - angle ** 2) ** 0.5 * u / u.norm())
    # log-probabilities of 2k candidates that fall by 0.9 per rank (p = 0.53, 0.22, 0.09 ...: the likelihood term separates the
    # candidates the planted row leaves alone by far more than their random cosines differ), distinct random tokens
    cs = torch.log_softmax(-0.9 * torch.arange(2 * k).float() + 0.05 * torch.randn(B, 2 * k, generator=g), -1) + float(np.log(0.9))
    cs = cs.sort(dim=-1, descending=True).values
    ci = torch.stack([torch.randperm(V, generator=g)[:2 * k] for _ in range(B)])
    return dict(B=B, k=k, d=d, n_ctx=n_ctx, n_cap=n_cap, dtype=dtype, plant=plant, cand=cand.to(dtype), ctx=ctx.to(dtype),
                valid=torch.ones(B, n_cap, dtype=torch.uint8), cs=cs.float().contiguous(), ci=ci.int().contiguous(),
                src=(torch.arange(B * k, dtype=torch.int32) % k)[:, None].repeat(1, 5).contiguous(), step=2,
                ids=torch.full((B, 7), -7, dtype=torch.int64), col=4, finished=None, eos=None, pad=None)


def _ref(case, alpha=ALPHA):
    k, n = case["k"], case["n_ctx"]
    return [rank_ref(case["cs"][b, :k], case["cand"][b * k:(b + 1) * k].float(), case["ctx"][b, :n].float(), case["valid"][b, :n], alpha)
            for b in range(case["B"])]


def _run(case, alpha=ALPHA, trace=True):
    """The call on device copies of the case's tensors; returns the device tensors after it (inputs included)."""
    dev = {key: (v.cuda() if torch.is_tensor(v) else v) for key, v in case.items()}
    res = ops.contrastive_select(dev["cand"], dev["ctx"], dev["valid"], dev["cs"], dev["ci"], alpha, case["n_ctx"], case["step"], dev["src"],
                                 dev["ids"][:, case["col"]], V, dev["finished"], case["eos"], case["pad"], trace=trace)
    dev["hidden_out"], dev["selected"] = res[0], res[1]
    if trace:
        dev["p"], dev["penalty"], dev["score"] = res[2]
    torch.cuda.synchronize()
    return dev


def _check_numerics(case, out, refs, what):
    d, k = case["d"], case["k"]
    tol = cos_tol(d)
    for b, r in enumerate(refs):
        assert r["margin"] >= 10 * (tol + 2.0 ** -22), f"{what} sample {b}: the reference's own margin {r['margin']:.3e} is below 10 tolerances"
    worst = [0.0, 0.0]
    for b, r in enumerate(refs):
        p, pen, sc = (out[key][b].double().cpu() for key in ("p", "penalty", "score"))
        ulp = torch.from_numpy(np.spacing(r["p"].numpy().astype(np.float32))).double()
        assert ((p - r["p"]).abs() <= 4 * ulp).all(), (what, b, p.tolist(), r["p"].tolist())
        e_pen, e_sc = float((pen - r["penalty"]).abs().max()), float((sc - r["score"]).abs().max())
        worst = [max(worst[0], e_pen), max(worst[1], e_sc)]
        assert e_pen <= tol, f"{what} sample {b}: penalty err {e_pen:.3e} > {tol:.3e}"
        assert e_sc <= tol + 2.0 ** -22, f"{what} sample {b}: score err {e_sc:.3e} > {tol + 2.0 ** -22:.3e}"
        score = out["score"][b].cpu()
        assert int(out["selected"][b]) == int(torch.nonzero(score == score.max())[0]) == r["selected"], (what, b, score.tolist(), r["score"].tolist())
    print(f"{what}: penalty err {worst[0]:.3e}, score err {worst[1]:.3e} (tolerance {tol:.3e})")


def _check_bookkeeping(case, out, what):
    """Row n_ctx of ctx and hidden_out are bitwise the selected row, the flag is set, src column `step` names the selection, the ids
    column holds the token -- and nothing else moved."""
    B, k, n, step, col = case["B"], case["k"], case["n_ctx"], case["step"], case["col"]
    sel = out["selected"].cpu().long()
    rows = torch.arange(B) * k + sel
    picked = case["cand"][rows]
    assert torch.equal(out["hidden_out"].cpu().view(torch.uint8), picked.view(torch.uint8)), what
    ctx = out["ctx"].cpu()
    assert torch.equal(ctx[:, n].view(torch.uint8), picked.view(torch.uint8)), what
    keep = torch.ones(case["n_cap"], dtype=torch.bool)
    keep[n] = False
    assert torch.equal(ctx[:, keep].view(torch.uint8), case["ctx"][:, keep].view(torch.uint8)), what
    valid = case["valid"].clone()
    valid[:, n] = 1
    assert torch.equal(out["valid"].cpu(), valid), what
    src = case["src"].clone()
    src[:, step] = sel.int().repeat_interleave(k)
    assert torch.equal(out["src"].cpu(), src), what
    if case["eos"] is None:
        ids = case["ids"].clone()
        ids[:, col] = case["ci"].long().gather(1, sel[:, None])[:, 0]
        assert torch.equal(out["ids"].cpu(), ids), what
    for key in ("cand", "cs", "ci"):
        assert torch.equal(out[key].cpu().view(torch.uint8), case[key].view(torch.uint8)), (what, key)


GROUND = [(torch.float32, 16, 2, 1, 1), (torch.bfloat16, 16, 8, 3, C + 1), (torch.bfloat16, 64, 3, 3, 2), (torch.float32, 64, 5, 3, C - 1),
          (torch.bfloat16, 768, 8, 1, C), (torch.float32, 768, 3, 3, C + 1), (torch.bfloat16, 2048, 5, 3, 3 * C + 5),
          (torch.float32, 2048, 8, 1, 3 * C + 5), (torch.float32, 64, 2, 3, 3 * C + 5), (torch.bfloat16, 2048, 8, 3, C)]


@pytest.mark.parametrize("dtype,d,k,B,n_ctx", GROUND, ids=[f"{str(g[0])[6:]}-d{g[1]}-k{g[2]}-B{g[3]}-n{g[4]}" for g in GROUND])
def test_numerics_bookkeeping_and_determinism(dtype, d, k, B, n_ctx):
    what = f"{dtype} d={d} k={k} B={B} n_ctx={n_ctx}"
    case = _case(B, k, d, n_ctx, dtype, seed=d + k + n_ctx, n_cap=n_ctx + 3)
    refs = _ref(case)
    out = _run(case)
    _check_numerics(case, out, refs, what)
    _check_bookkeeping(case, out, what)
    again = _run(case)
    for key in ("p", "penalty", "score", "selected", "hidden_out", "ctx", "src", "ids", "valid"):
        assert torch.equal(out[key].view(torch.uint8), again[key].view(torch.uint8)), (what, key)
    assert refs[0]["selected"] != 0, "the penalty does not change sample 0's selection: the case shows nothing"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_the_maximum_at_the_ends_and_on_both_sides_of_every_chunk_boundary(dtype):
    """n_ctx = 3 chunks + 5: the context row that holds candidate 0's maximum sits at row 0, at row n_ctx - 1 and at rows m C - 1 and
    m C.  A row the kernel skipped or read twice at a boundary moves that penalty from 0.95 to a random row's cosine."""
    n, d, k, B = 3 * C + 5, 64, 4, 3
    spots = [0, n - 1] + [m * C + o for m in (1, 2, 3) for o in (-1, 0)]
    spots += [spots[0]] * (-len(spots) % B)
    for i in range(0, len(spots), B):
        plant = [(0, j) for j in spots[i:i + B]]
        case = _case(B, k, d, n, dtype, seed=100 + i, plant=plant)
        refs = _ref(case)
        for b, r in enumerate(refs):
            assert abs(float(r["penalty"][0]) - 0.95) < 1e-2, (plant, r["penalty"])      # the planted row is the maximum, in the reference
        out = _run(case)
        _check_numerics(case, out, refs, f"{dtype} maxima at rows {spots[i:i + B]}")
        _check_bookkeeping(case, out, f"{dtype} maxima at rows {spots[i:i + B]}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_all_negative_cosines_zero_norms_and_masked_context(dtype):
    B, k, d, n = 3, 3, 64, C + 3
    case = _case(B, k, d, n, dtype, seed=5, plant=[])
    case["cand"] = case["cand"].float().abs().add(0.1).to(dtype)
    case["ctx"] = (-case["ctx"].float().abs() - 0.1).to(dtype)
    # -- every cosine negative: a running max that starts at 0 reports 0
    refs = _ref(case)
    assert all(float(r["penalty"].max()) < -0.1 for r in refs)
    out = _run(case)
    for b, r in enumerate(refs):
        assert float((out["penalty"][b].double().cpu() - r["penalty"]).abs().max()) <= cos_tol(d), (b, out["penalty"][b].tolist())
        assert (out["penalty"][b] < 0).all()
    # -- a zero-norm context row has cosine 0, the maximum here; a zero-norm candidate has penalty 0
    zero = {key: (v.clone() if torch.is_tensor(v) else v) for key, v in case.items()}
    zero["ctx"][1, C] = 0
    zero["cand"][2 * k + 1] = 0
    refs = _ref(zero)
    out = _run(zero)
    assert out["penalty"][1].tolist() == [0.0] * k and float(out["penalty"][2, 1]) == 0.0 and float(out["penalty"][2, 0]) < 0
    for b, r in enumerate(refs):
        assert float((out["penalty"][b].double().cpu() - r["penalty"]).abs().max()) <= cos_tol(d)
        assert float((out["score"][b].double().cpu() - r["score"]).abs().max()) <= cos_tol(d) + 2.0 ** -22
    # -- every context row masked (sample 0), an empty context (n_ctx = 0): penalty 0, score (1 - alpha) p, candidate 0 selected
    masked = {key: (v.clone() if torch.is_tensor(v) else v) for key, v in case.items()}
    masked["valid"][0, :n] = 0
    out = _run(masked)
    assert out["penalty"][0].tolist() == [0.0] * k and int(out["selected"][0]) == 0 and (out["penalty"][1:] < 0).all()
    _check_bookkeeping(masked, out, "masked context")
    empty = dict(case, n_ctx=0)
    out = _run(empty)
    assert out["penalty"].tolist() == [[0.0] * k] * B and out["selected"].tolist() == [0] * B
    assert torch.equal(out["score"], (1 - torch.tensor(ALPHA, dtype=torch.float32).cuda()) * out["p"])
    _check_bookkeeping(empty, out, "empty context")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_nan_in_everything_that_must_not_be_read(dtype):
    """NaN in masked rows, in rows at and past n_ctx and in the padding of strided cand_hidden / ctx / ids / src / candidate buffers:
    the results are bitwise those of the dense call on the compacted context."""
    B, k, d, n = 3, 4, 64, 2 * C + 3
    case = _case(B, k, d, n, dtype, seed=9, n_cap=n + 2)
    g = torch.Generator().manual_seed(1)
    case["valid"][:, :n] = (torch.rand(B, n, generator=g) > 0.4).to(torch.uint8)
    case["valid"][0, :C] = 0                                                   # a whole chunk without a live row
    for b, (c, j) in enumerate(case["plant"]):
        case["valid"][b, j] = 1
    live = int(case["valid"][:, :n].sum(1).min())
    # the dense call: per sample the live rows first (each sample padded to the same count with masked finite rows)
    dense = {key: (v.clone() if torch.is_tensor(v) else v) for key, v in case.items()}
    for b in range(B):
        order = torch.argsort(1 - case["valid"][b, :n].int(), stable=True)
        dense["ctx"][b, :n] = case["ctx"][b, :n][order]
        dense["valid"][b, :n] = case["valid"][b, :n][order]
    want = _run(dense)
    assert live >= 3 and any(r["selected"] != 0 for r in _ref(case))
    # the strided, NaN-riddled call
    nan = float("nan")
    pad = 8 if dtype == torch.bfloat16 else 4
    cand = torch.full((B * k, d + pad), nan).to(dtype).cuda()
    cand[:, :d] = case["cand"].cuda()
    ctx = torch.full((B, case["n_cap"] + 1, d + 2 * pad), nan).to(dtype).cuda()
    ctx[:, :n, :d] = torch.where(case["valid"][:, :n, None].bool(), case["ctx"][:, :n].float(), torch.full((1,), nan)).to(dtype).cuda()
    valid = torch.zeros(B, case["n_cap"] + 5, dtype=torch.uint8).cuda()
    valid[:, :case["n_cap"]] = case["valid"].cuda()
    cs = torch.full((B, 2 * k + 3), nan).cuda()
    cs[:, :2 * k] = case["cs"].cuda()
    ci = torch.full((B, 2 * k + 3), -1, dtype=torch.int32).cuda()
    ci[:, :2 * k] = case["ci"].cuda()
    src = torch.full((B * k, 9), -3, dtype=torch.int32).cuda()
    ids = torch.full((B, 11), -7, dtype=torch.int64).cuda()
    tr = tuple(torch.empty(B, k, device="cuda") for _ in range(3))
    ho, sel, _ = ops.contrastive_select(cand[:, :d], ctx[:, :case["n_cap"], :d], valid[:, :case["n_cap"]], cs[:, :2 * k], ci[:, :2 * k], ALPHA, n,
                                        3, src[:, :6], ids[:, 5], V, trace=tr)
    torch.cuda.synchronize()
    for key, got in (("p", tr[0]), ("penalty", tr[1]), ("score", tr[2]), ("selected", sel), ("hidden_out", ho)):
        assert torch.equal(got.view(torch.uint8), want[key].view(torch.uint8)), key
    assert torch.equal(ctx[:, n, :d].view(torch.uint8), ho.view(torch.uint8)) and torch.isnan(ctx[:, n, d:].float()).all()
    assert torch.isnan(ctx[:, n + 1:].float()).all() and torch.isnan(cand[:, d:].float()).all()
    assert valid[:, n].tolist() == [1] * B and torch.equal(valid[:, n + 1:case["n_cap"]].cpu(), case["valid"][:, n + 1:])
    assert valid[:, case["n_cap"]:].sum() == 0
    assert torch.equal(src[:, 3], sel.repeat_interleave(k)) and (src[:, :3] == -3).all() and (src[:, 4:] == -3).all()
    assert torch.equal(ids[:, 5], ci.long().gather(1, sel.long()[:, None])[:, 0]) and (ids[:, :5] == -7).all() and (ids[:, 6:] == -7).all()


def test_finished_rows_get_pad_and_eos_sets_finished():
    B, k, d, n = 3, 3, 64, 5
    case = _case(B, k, d, n, torch.float32, seed=3)
    refs = _ref(case)
    tokens = [int(case["ci"][b, r["selected"]]) for b, r in enumerate(refs)]
    case.update(eos=tokens[1], pad=1, finished=torch.tensor([1, 0, 0], dtype=torch.uint8))
    assert tokens[2] != tokens[1]
    out = _run(case)
    assert out["ids"][:, case["col"]].tolist() == [1, tokens[1], tokens[2]] and out["finished"].tolist() == [1, 1, 0]
    assert out["selected"].tolist() == [r["selected"] for r in refs]              # a finished row still selects: its cache stays defined
    _check_bookkeeping(case, out, "eos")


def test_a_refused_call_writes_nothing():
    B, k, d, n = 2, 4, 64, C + 2
    case = _case(B, k, d, n, torch.bfloat16, seed=4)
    dev = {key: (v.cuda() if torch.is_tensor(v) else v) for key, v in case.items()}
    ho, sel = torch.full((B, d), 5.0, dtype=torch.bfloat16).cuda(), torch.full((B,), -9, dtype=torch.int32).cuda()
    tr = tuple(torch.full((B, k), 7.0).cuda() for _ in range(3))
    shifted = torch.zeros(B * k, d + 8, dtype=torch.bfloat16).cuda()[:, 1:d + 1]      # rows 2 bytes off the 16-byte grid

    def call(**kw):
        a = dict(cand=dev["cand"], ctx=dev["ctx"], n_ctx=n, step=case["step"], alpha=ALPHA)
        a.update(kw)
        return ops.contrastive_select(a["cand"], a["ctx"], dev["valid"], dev["cs"], dev["ci"], a["alpha"], a["n_ctx"], a["step"], dev["src"],
                                      dev["ids"][:, case["col"]], V, hidden_out=ho, selected=sel, trace=tr)
    for kw, word in ((dict(cand=shifted), "16-byte"), (dict(n_ctx=case["n_cap"]), "n_ctx"), (dict(step=5), "step"), (dict(alpha=1.5), "alpha"),
                     (dict(ctx=dev["ctx"].float()), "incompatible"), (dict(cand=dev["cand"][:B * k - 1]), "cand_hidden")):
        with pytest.raises(ValueError, match=word):
            call(**kw)
    torch.cuda.synchronize()
    assert (ho == 5).all() and (sel == -9).all() and all((t == 7).all() for t in tr)
    for key in ("ctx", "valid", "src", "ids"):
        assert torch.equal(dev[key].cpu().view(torch.uint8), case[key].view(torch.uint8)), key
    call()                                                                           # and the valid call goes through
    torch.cuda.synchronize()
    assert (sel >= 0).all() and not (ho == 5).all()
