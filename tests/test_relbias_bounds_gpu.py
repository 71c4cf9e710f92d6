"""-m gpu: the T5 attention kernels (csrc/relbias.hip) through the raw entry points against relbias_ref.RelBiasRef -- an fp64 reference
of the storage-rounded operands -- element by element: out, lse, dq, dk, dv and dtable each within the bound of RelBiasRef's docstring
(SelfAttnRef's form and constants, n one more for the bias add, dtable with its chain term L; tests/test_relbias_ref_cpu.py shows on the
CPU that this comparison fails for a dropped, mirrored, shifted, wrongly bucketed or head-swapped bias).  Operands sit between NaN,
every result and the workspace between canaries, and every result holds NaN before the call.  B = 2, H = 3, D = 64.

Shapes: bidirectional (T, S) in (1, 1), (17, 40), (64, 64), (65, 129), (130, 70) -- below, at and past the 64-row tile on either axis,
more than one workgroup and more than one key tile; causal T = S in 1, 63, 65, 129.  Masks: all valid, the last sample right-padded, a
hole in the middle of sample 0.  Every shape with the table and without it, in both dtypes."""
import ctypes

import pytest
import torch

from bounds import BF16, F32, NAME, NAN, ByteSlab, Slab
from relbias_ref import RelBiasRef

pytestmark = pytest.mark.gpu

B, H, D, NB = 2, 3, 64, 32
BIDIR = [(1, 1), (17, 40), (64, 64), (65, 129), (130, 70)]
CAUSAL = [1, 63, 65, 129]


def _table(seed=5):
    return torch.randn(NB, H, generator=torch.Generator().manual_seed(seed))


def _run(dtype, cpu, key_valid, table, bucket_of, causal, p_drop=0.0, seed=0, backward=True):
    """One forward (+ backward) call on operands `cpu` = (q, k, v, dout); returns (results by name, slabs)."""
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr
    q, k, v, dout = (Slab(t.shape, dtype, NAN, src=t) for t in cpu)
    T, S = cpu[0].shape[1], cpu[1].shape[1]
    kv = None if key_valid is None else key_valid.cuda().contiguous()
    tab = None if table is None else Slab(table.shape, F32, NAN, src=table)
    bo = None if bucket_of is None else bucket_of.cuda()
    nb = 0 if table is None else table.shape[0]
    out, lse = Slab((B, T, H * D), dtype, NAN), Slab((B, H, T), F32, NAN)
    code = _lib.dtype_code(q.v)
    tp = None if tab is None else ptr(tab.v)
    _lib.call("mmgl_attn_relbias_fwd", None, ptr(q.v), ptr(k.v), ptr(v.v), ptr(kv), tp, ptr(bo), ptr(out.v), ptr(lse.v), B, H, T, S, D, nb,
              H * D, H * D, int(causal), float(p_drop), int(seed), code, None)
    slabs = [out, lse]
    got = dict(out=out.v, lse=lse.v)
    if backward:
        dq, dk, dv = Slab((B, T, H * D), dtype, NAN), Slab((B, S, H * D), dtype, NAN), Slab((B, S, H * D), dtype, NAN)
        dtab = None if tab is None else Slab(table.shape, F32, NAN)
        nbytes = _lib.lib().mmgl_attn_relbias_bwd_workspace(B, H, T, S)
        ws = ByteSlab(nbytes)
        _lib.call("mmgl_attn_relbias_bwd", None, ptr(dout.v), ptr(q.v), ptr(k.v), ptr(v.v), ptr(out.v), ptr(lse.v), ptr(kv), tp, ptr(bo),
                  ptr(dq.v), ptr(dk.v), ptr(dv.v), None if dtab is None else ptr(dtab.v), ws.ptr(), nbytes, B, H, T, S, D, nb, H * D, H * D,
                  int(causal), float(p_drop), int(seed), code, None)
        slabs += [dq, dk, dv, ws] + ([dtab] if dtab is not None else [])
        got.update(dq=dq.v, dk=dk.v, dv=dv.v)
        if dtab is not None:
            got["dtable"] = dtab.v
    torch.cuda.synchronize()
    for s in slabs:
        assert s.untouched(), "a canary next to a result or the workspace was overwritten"
    return got, slabs


def _bucket(T, S, causal):
    from mmgl_amd import ops
    return ops.t5_bucket_table(T, S, not causal, NB, 128, "cpu")


def _sweep(dtype, T, S, causal):
    cpu = RelBiasRef.inputs(dtype, B, T, S, H, D, seed=T + S)
    worst = {}
    for layout in ("M0", "M1", "M2"):
        key_valid = RelBiasRef.mask(B, S, layout)
        for table in (_table(), None):
            bucket_of = None if table is None else _bucket(T, S, causal)
            ref = RelBiasRef(*cpu[:3], key_valid, cpu[3], H, table=table, bucket_of=bucket_of, causal=causal)
            got, _ = _run(dtype, cpu, None if layout == "M0" else key_valid, table, bucket_of, causal)
            r = ref.check(got, f"{NAME[dtype]} T={T} S={S} causal={causal} {layout} table={table is not None}", dtype)
            for n, x in r.items():
                worst[n] = max(worst.get(n, 0.0), x)
    print(f"[bound relbias worst] {NAME[dtype]} T={T} S={S} causal={causal}: " + ", ".join(f"{n} {x:.3f}" for n, x in worst.items()))


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("T,S", BIDIR)
def test_bidirectional_bounds(dtype, T, S):
    _sweep(dtype, T, S, False)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("T", CAUSAL)
def test_causal_bounds(dtype, T):
    _sweep(dtype, T, T, True)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("T,S,causal", [(65, 129, False), (65, 65, True)])
def test_dropout_follows_the_counter_hash(dtype, T, S, causal):
    """p_drop = 0.3 with a fixed seed: the reference drops the probabilities bounds.hash_keep names; a kernel with another index
    order, threshold or scale leaves the bound everywhere."""
    cpu = RelBiasRef.inputs(dtype, B, T, S, H, D, seed=11)
    key_valid, table, bucket_of = RelBiasRef.mask(B, S, "M1"), _table(), _bucket(T, S, causal)
    seed = 0x1234567 + T
    ref = RelBiasRef(*cpu[:3], key_valid, cpu[3], H, table=table, bucket_of=bucket_of, causal=causal, p_drop=0.3, seed=seed)
    plain = RelBiasRef(*cpu[:3], key_valid, cpu[3], H, table=table, bucket_of=bucket_of, causal=causal)
    assert ref.outside(plain, "out", dtype).double().mean().item() > 0.5          # the undropped result is far outside
    got, _ = _run(dtype, cpu, key_valid, table, bucket_of, causal, p_drop=0.3, seed=seed)
    ref.check(got, f"{NAME[dtype]} dropout T={T} S={S} causal={causal}", dtype)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_dtable_is_reproducible(dtype):
    T, S = 130, 70
    cpu = RelBiasRef.inputs(dtype, B, T, S, H, D, seed=7)
    key_valid, table, bucket_of = RelBiasRef.mask(B, S, "M2"), _table(), _bucket(T, S, False)
    a, _ = _run(dtype, cpu, key_valid, table, bucket_of, False, p_drop=0.3, seed=9)
    b, _ = _run(dtype, cpu, key_valid, table, bucket_of, False, p_drop=0.3, seed=9)
    for n in ("dtable", "dq", "dk", "dv", "out", "lse"):
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("T,S,causal", [(65, 129, False), (65, 65, True)])
def test_sample_without_a_valid_key_gives_finite_zeros(dtype, T, S, causal):
    cpu = RelBiasRef.inputs(dtype, B, T, S, H, D, seed=13)
    key_valid = torch.ones(B, S, dtype=torch.uint8)
    key_valid[0] = 0
    table, bucket_of = _table(), _bucket(T, S, causal)
    got, _ = _run(dtype, cpu, key_valid, table, bucket_of, causal)          # (asserts the canaries)
    for n in ("out", "lse", "dq", "dk", "dv"):
        assert torch.isfinite(got[n].float()).all(), n
        assert (got[n][0] == 0).all(), f"{n} of the sample without a valid key is not zero"
    ref = RelBiasRef(*cpu[:3], key_valid, cpu[3], H, table=table, bucket_of=bucket_of, causal=causal)
    ref.check(got, f"{NAME[dtype]} empty sample T={T} S={S} causal={causal}", dtype)


def test_unsupported_arguments_launch_nothing():
    from mmgl_amd import _lib
    from mmgl_amd._lib import ptr
    L = _lib.lib()
    T, S = 17, 40
    mk = lambda rows, d: Slab((B, rows, H * d), BF16, 1.0)
    for d, causal in ((64, 1), (48, 0)):
        q, k, v, out, lse = mk(T, d), mk(S, d), mk(S, d), Slab((B, T, H * d), BF16, NAN), Slab((B, H, T), F32, NAN)
        rc = L.mmgl_attn_relbias_fwd(ptr(q.v), ptr(k.v), ptr(v.v), None, None, None, ptr(out.v), ptr(lse.v), B, H, T, S, d, 0, H * d, H * d,
                                     causal, 0.0, 0, _lib.BF16, None)
        assert rc == _lib._ERR_UNSUPPORTED
        dq, dk, dv = Slab((B, T, H * d), BF16, NAN), Slab((B, S, H * d), BF16, NAN), Slab((B, S, H * d), BF16, NAN)
        nbytes = L.mmgl_attn_relbias_bwd_workspace(B, H, T, S)
        ws = ByteSlab(nbytes)
        rc = L.mmgl_attn_relbias_bwd(ptr(q.v), ptr(q.v), ptr(k.v), ptr(v.v), ptr(out.v), ptr(lse.v), None, None, None, ptr(dq.v), ptr(dk.v),
                                     ptr(dv.v), None, ws.ptr(), nbytes, B, H, T, S, d, 0, H * d, H * d, causal, 0.0, 0, _lib.BF16, None)
        assert rc == _lib._ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert all(s.unwritten() for s in (out, lse, dq, dk, dv, ws))


def test_op_under_autograd_matches_the_reference():
    """ops.attn_relbias: the table as a bf16 parameter (read as fp32, gradient back in bf16), key_valid None, gradients by autograd."""
    from mmgl_amd import ops
    T, S = 65, 129
    cpu = RelBiasRef.inputs(BF16, B, T, S, H, D, seed=17)
    table = _table().to(BF16)
    bucket_of = _bucket(T, S, False)
    q, k, v = (t.cuda().requires_grad_() for t in cpu[:3])
    tab = table.cuda().requires_grad_()
    out = ops.attn_relbias(q, k, v, None, H, table=tab, bucket_of=bucket_of.cuda())
    out.backward(cpu[3].cuda())
    ref = RelBiasRef(*cpu[:3], None, cpu[3], H, table=table.float(), bucket_of=bucket_of)
    ref.check(dict(out=out, dq=q.grad, dk=k.grad, dv=v.grad), "op bf16", BF16)
    assert tab.grad.dtype == BF16
    err = (tab.grad.double().cpu() - ref.want["dtable"]).abs()
    assert (err <= ref.bound("dtable", BF16) + 2.0 ** -8 * ref.want["dtable"].abs()).all()     # + the bf16 store of the gradient
    with pytest.raises(ValueError):
        ops.attn_relbias(q, k, v, None, H, table=tab, bucket_of=bucket_of.cuda()[:-1])
    with pytest.raises(ValueError):
        ops.attn_relbias(q, k, v, None, H, causal=True)
