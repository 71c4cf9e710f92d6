"""-m gpu: mmgl_adafactor_step (csrc/adafactor.hip) through the raw entry point, element by element against adafactor_ref.AdafactorRef
(tests/test_adafactor_ref_cpu.py shows that the comparison can fail and that fp32 arithmetic in the kernel's order stays inside).

One flat buffer holds adafactor_ref.SHAPES together, each tensor on a 128-element boundary: [1, 8], [8, 1], [32, 6], [7], [1],
[257, 131] (odd C, ragged in both tile directions), 63 / 64 / 65 rows (the row tile), 255 / 256 / 257 columns (the column tile),
[130, 515] (3 x 3 tiles), a 1-D tensor of three tiles, a 2-D and a 1-D tensor whose gradient is all zero; gradients 0, 1e-20, 1e4
planted.  The parameter, master, state and table are carved out of canary slabs, the gradient out of a NaN slab (its padding is NaN: a
lane that read it would poison a sum), the workspace out of a NaN byte slab between canaries.

Cases: bf16 / fp32 x with / without master x (grad_scale 1, weight_decay 0) / (0.5, 0.01) x {steps 1, 2, 3 chained from zero state; step
1000 from a random positive state with the clip idle on at least three tensors in four; the same with the clip active on all but
at most two of the tensors that have a gradient}.  Per step: every element
of param / master / row / col / v inside the counted bound; with a master the bf16 parameter is its rounding bit for bit; the padding
between tensors, every guard, the gradient and the table unchanged; a second run on the same inputs bit-equal; and -- a yardstick that does
not rest on the counted constants -- per tensor and output the fused result's largest error against fp64 is at most twice that of
transformers' Adafactor on the same GPU from the same state, or one store unit of the tensor's largest value where the stock error is
smaller."""
import ctypes

import pytest
import torch
from transformers.optimization import Adafactor

from adafactor_ref import SHAPES, ZERO_GRAD, AdafactorRef, inputs
from bounds import BF16, CANARY, F32, NAME, NAN, ByteSlab, Slab, U, bits, check_bound, code, same

pytestmark = pytest.mark.gpu

LR = 2.0 ** -7
SCENARIOS = {"steps123": ((1, 2, 3), 1.0), "step1000-idle": ((1000,), 4.0), "step1000-active": ((1000,), 0.01)}


def _names(shape):
    return ("row", "col") if len(shape) == 2 else ("v",)


def _table():
    from mmgl_amd import ops
    offs, off = [], 0
    for s in SHAPES:
        offs.append(off)
        off += (torch.Size(s).numel() + 127) // 128 * 128
    return ops.AdafactorTable(list(zip(offs, SHAPES))), off


class Buffers:
    """The operands of one call, carved; `tensors`: per tensor dict(p fp32 as the kernel reads it, g, state)."""

    def __init__(self, table, numel, dtype, with_master, tensors):
        self.table, self.numel, self.dtype = table, numel, dtype
        self.param, self.grad = Slab((numel,), dtype, CANARY), Slab((numel,), dtype, NAN)
        self.master = Slab((numel,), F32, CANARY) if with_master else None
        self.state = Slab((table.state_numel,), F32, CANARY)
        self.tab = Slab((len(table.host),), torch.int64, -77, torch.tensor(list(table.host), dtype=torch.int64))
        self.ws = ByteSlab(table.workspace_bytes)
        self.live, self.live_state = torch.zeros(numel, dtype=torch.bool, device="cuda"), torch.zeros(table.state_numel, dtype=torch.bool, device="cuda")
        for t, off, so in zip(tensors, table.offsets, table.state_offsets):
            k = t["p"].numel()
            self.param.v[off:off + k] = t["p"].reshape(-1).to(dtype)
            self.grad.v[off:off + k] = t["g"].reshape(-1)
            if with_master:
                self.master.v[off:off + k] = t["p"].reshape(-1)
            st = torch.cat([s.reshape(-1) for s in t["state"]])
            self.state.v[so:so + st.numel()] = st
            self.live[off:off + k], self.live_state[so:so + st.numel()] = True, True
        self.before = {k: s.buf.clone() for k, s in self._slabs().items()}

    def _slabs(self):
        d = dict(param=self.param, grad=self.grad, state=self.state, tab=self.tab)
        if self.master is not None:
            d["master"] = self.master
        return d

    def call(self, step, gs, wd):
        from mmgl_amd import _lib
        _lib.call("mmgl_adafactor_step", None, self.param.ptr(), None if self.master is None else self.master.ptr(), self.grad.ptr(),
                  self.state.ptr(), self.tab.ptr(), self.table.host, self.table.n, self.ws.ptr(), self.table.workspace_bytes, LR, 1e-30, 1.0,
                  -0.8, wd, step, gs, code(self.dtype), _lib.stream_ptr())
        torch.cuda.synchronize()

    def out(self, i):
        """dict(p fp32 -- the master where there is one --, row, col | v) of tensor i."""
        shape, off, so = SHAPES[i], self.table.offsets[i], self.table.state_offsets[i]
        k = torch.Size(shape).numel()
        d = dict(p=(self.master if self.master is not None else self.param).v[off:off + k].float().view(shape))
        if len(shape) == 2:
            d.update(row=self.state.v[so:so + shape[0]], col=self.state.v[so + shape[0]:so + shape[0] + shape[1]])
        else:
            d.update(v=self.state.v[so:so + k])
        return d

    def check_untouched(self, what):
        assert all(s.untouched() for s in self._slabs().values()) and self.ws.untouched(), f"{what}: a guard changed"
        assert torch.equal(self.grad.buf, self.before["grad"]) and torch.equal(self.tab.buf, self.before["tab"]), f"{what}: the gradient or the table changed"
        for name, live in (("param", self.live), ("master", self.live), ("state", self.live_state)):
            slab = self._slabs().get(name)
            if slab is not None:
                assert same(slab.v[~live], torch.full_like(slab.v[~live], CANARY)), f"{what}: the padding between tensors of {name} was written"


def _stock_errors(tensors, refs, dtype, with_master, step, gs, wd):
    """Per tensor dict(name -> largest error against the reference) of transformers' Adafactor on the GPU, one step from the same state."""
    pdt = F32 if with_master else dtype
    params = [torch.nn.Parameter(t["p"].to(pdt)) for t in tensors]
    opt = Adafactor(params, scale_parameter=False, relative_step=False, warmup_init=False, lr=LR, weight_decay=wd)
    for p, t in zip(params, tensors):
        p.grad = (t["g"].float() * gs).to(pdt)
        if step > 1:
            keys = ("exp_avg_sq_row", "exp_avg_sq_col") if p.dim() == 2 else ("exp_avg_sq",)
            opt.state[p] = dict(step=step - 1, RMS=0, **{k: s.clone().view(p.shape if k == "exp_avg_sq" else -1) for k, s in zip(keys, t["state"])})
    opt.step()
    errs = []
    for p, ref in zip(params, refs):
        st = opt.state[p]
        got = dict(p=p.detach(), row=st.get("exp_avg_sq_row"), col=st.get("exp_avg_sq_col"), v=st.get("exp_avg_sq"))
        errs.append({k: ref.err(got[k], k).max().item() for k in ref.want})
    return errs


@pytest.mark.parametrize("scenario", list(SCENARIOS))
@pytest.mark.parametrize("gs, wd", [(1.0, 0.0), (0.5, 0.01)], ids=["gs1-wd0", "gs.5-wd.01"])
@pytest.mark.parametrize("with_master", [False, True], ids=["plain", "master"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_adafactor_step_bounds(dtype, with_master, gs, wd, scenario):
    table, numel = _table()
    steps, scale = SCENARIOS[scenario]
    store = BF16 if dtype == BF16 and not with_master else F32
    tensors = [{k: (tuple(s.cuda() for s in v) if k == "state" else v.cuda() if k != "shape" else v) for k, v in t.items()}
               for t in inputs(dtype, steps[0], seed=0, state_scale=scale)]
    group = f"{NAME[dtype]}{' master' if with_master else ''} {scenario}"
    for step in steps:
        if step != steps[0]:
            for t, fresh in zip(tensors, inputs(dtype, step, seed=step)):
                t["g"] = fresh["g"].cuda()
        if store == BF16:
            for t in tensors:
                t["p"] = t["p"].to(BF16).float()
        what = f"{group} gs{gs} wd{wd} step {step}"
        a, b = Buffers(table, numel, dtype, with_master, tensors), Buffers(table, numel, dtype, with_master, tensors)
        a.call(step, gs, wd)
        b.call(step, gs, wd)
        a.check_untouched(what)
        assert all(torch.equal(x.buf, y.buf) for x, y in zip(a._slabs().values(), b._slabs().values())), f"{what}: two runs differ"
        if with_master and dtype == BF16:
            assert same(a.param.v[a.live], a.master.v[a.live].to(BF16)), f"{what}: the bf16 parameter is not the rounded master"

        refs = [AdafactorRef(t["p"], t["g"], t["state"], LR, step, gs, wd, store=store) for t in tensors]
        outs = [a.out(i) for i in range(len(SHAPES))]
        for name in ("p", "row", "col", "v"):
            err = torch.cat([r.err(o[name], name).reshape(-1) for r, o in zip(refs, outs) if name in r.want])
            bound = torch.cat([r.bound(name).reshape(-1) for r in refs if name in r.want])
            assert all(torch.isfinite(o[name]).all() for o in outs if name in o), f"{what} {name}: non-finite"
            check_bound(err, None, bound, f"adafactor {what} {name}", group, where=lambda bad: f"flat indices over the tensors that hold {name}: {bad[:8, 0].tolist()}")

        clipped = [r.d > 1.0 for r in refs]
        if scenario == "step1000-idle":
            assert sum(clipped) <= len(SHAPES) // 4, "the idle scenario should leave the clip idle on most tensors"
        if scenario == "step1000-active":
            assert sum(clipped) >= len(SHAPES) - len(ZERO_GRAD) - 2, "the active scenario should clip the tensors with a gradient (a one-element tensor may not)"
        for i in ZERO_GRAD:
            assert wd != 0.0 or torch.equal(outs[i]["p"], tensors[i]["p"]), f"{what}: a zero gradient moved tensor {SHAPES[i]}"

        # the yardstick: transformers' Adafactor on this GPU from the same state
        worst = 0.0
        for i, (ref, o, stock) in enumerate(zip(refs, outs, _stock_errors(tensors, refs, dtype, with_master, step, gs, wd))):
            for name in ref.want:
                fused = ref.err(o[name], name).max().item()
                unit = U[store if name == "p" else F32] * ref.want[name].abs().max().item()
                worst = max(worst, fused / max(stock[name], unit / 2))
                assert fused <= max(2 * stock[name], unit), f"{what} {SHAPES[i]} {name}: fused error {fused:.3e}, stock {stock[name]:.3e}, store unit {unit:.3e}"
        print(f"[ratio {group}] adafactor {what}: largest fused / max(stock error, half a store unit) over tensors and outputs {worst:.2f}")

        for t, o in zip(tensors, outs):                                         # the next step starts from what the kernel left
            t["p"], t["state"] = o["p"].clone(), tuple(o[k].clone() for k in _names(t["shape"]))


def test_adafactor_refusals_write_nothing():
    from mmgl_amd import _lib
    table, numel = _table()
    tensors = [{k: (tuple(s.cuda() for s in v) if k == "state" else v.cuda() if k != "shape" else v) for k, v in t.items()} for t in inputs(F32, 2, seed=0)]
    b = Buffers(table, numel, F32, True, tensors)
    args = dict(param=b.param.ptr(), master=b.master.ptr(), grad=b.grad.ptr(), state=b.state.ptr(), tab=b.tab.ptr(), host=table.host, n=table.n,
                ws=b.ws.ptr(), nbytes=table.workspace_bytes, lr=LR, eps1=1e-30, clip=1.0, decay=-0.8, wd=0.0, step=2, gs=1.0, dtype=code(F32))
    zero_host = (ctypes.c_int64 * len(table.host))()
    for kw, msg in ((dict(step=0), "bad arguments"), (dict(param=None), "bad arguments"), (dict(grad=None), "bad arguments"), (dict(state=None), "bad arguments"),
                    (dict(tab=None), "bad arguments"), (dict(ws=None), "bad arguments"), (dict(n=0), "bad arguments"), (dict(dtype=7), "bad dtype"),
                    (dict(clip=0.0), "clip_threshold"), (dict(decay=0.5), "decay_rate"), (dict(nbytes=table.workspace_bytes - 4), "workspace"),
                    (dict(host=zero_host), "not a planned table")):
        with pytest.raises(ValueError, match=msg):
            _lib.call("mmgl_adafactor_step", None, *dict(args, **kw).values(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert all(torch.equal(s.buf, b.before[k]) for k, s in b._slabs().items()) and b.ws.unwritten(), "a refused call wrote"
    from mmgl_amd import ops
    for segs, msg in (([(0, (4, 4)), (8, (4,))], "128-element"), ([(128, (4, 4)), (0, (4,))], "overlap"), ([(0, (2, 3, 4))], "1-D and 2-D")):
        with pytest.raises(ValueError, match=msg):
            ops.AdafactorTable(segs)
