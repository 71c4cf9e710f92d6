"""torch.autograd.Function wrappers over the C-ABI kernels (one per fwd/bwd pair).

Each op validates shapes the way the reference does (ValueError), makes inputs contiguous, calls the HIP
entry point on torch's current stream and returns fresh tensors owned by autograd.  GPU only.
"""
import math
import os
import weakref

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import dtype_code, lib, ptr, ptr_off, require_cuda, stream_ptr


def _dropout(p_drop, training, seed):
    """(p, seed) for the kernels: p = 0 outside training; a seed is drawn when something is dropped and the caller gave none."""
    p = float(p_drop) if training else 0.0
    if p > 0.0 and seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    return p, int(seed or 0)


# ------------------------------------------------------------------------------------------ attention core
def _check_mask(key_valid, shape):
    if key_valid.shape != shape:
        raise ValueError(f"Attention mask should be of size {tuple(shape)}, but is {tuple(key_valid.shape)}")


def _key_valid(key_valid):
    """key_valid [B, keys] (True = attend) as the contiguous uint8 the kernels read; after every check, so that a refused call does no
    GPU work."""
    if key_valid.dtype != torch.uint8:
        key_valid = key_valid.to(torch.uint8)
    return key_valid.contiguous()


def _attn_args(op, q, k, v, key_valid, num_heads, extra_keys=None, tail=""):
    """The argument checks of every attention op, raised the way the reference does: q [B,T,d], k and v [B,S,d] (with S = T + extra_keys
    where the op fixes it), d a multiple of num_heads, key_valid [B,S]."""
    if (q.dim() != 3 or k.dim() != 3 or k.shape != v.shape or q.shape[0] != k.shape[0] or q.shape[2] != k.shape[2]
            or (extra_keys is not None and k.shape[1] != q.shape[1] + extra_keys)):
        raise ValueError(f"{op}: incompatible shapes q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)}{tail}")
    if q.shape[2] % num_heads:
        raise ValueError(f"embed_dim must be divisible by num_heads (got `embed_dim`: {q.shape[2]} and `num_heads`: {num_heads}).")
    _check_mask(key_valid, k.shape[:2])


class _XAttnCore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, key_valid, num_heads):
        require_cuda(q, k, v, key_valid)
        B, T, d = q.shape
        S = k.shape[1]
        D = d // num_heads
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        out = torch.empty_like(q)
        lse = torch.empty(B, num_heads, T, dtype=torch.float32, device=q.device)
        _lib.call("mmgl_xattn_fwd", dict(B=B, H=num_heads, T=T, S=S, D=D, esize=q.element_size()), ptr(q), ptr(k), ptr(v), ptr(key_valid), ptr(out), ptr(lse), B, num_heads, T, S, D,
                                   dtype_code(q), stream_ptr())
        ctx.save_for_backward(q, k, v, key_valid, lse)
        ctx.num_heads = num_heads
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, key_valid, lse = ctx.saved_tensors
        H = ctx.num_heads
        B, T, d = q.shape
        S = k.shape[1]
        D = d // H
        dout = dout.contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        nbytes = lib().mmgl_xattn_bwd_workspace(B, H, T, S, D)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
        _lib.call("mmgl_xattn_bwd", dict(B=B, H=H, T=T, S=S, D=D, esize=q.element_size()), ptr(dout), ptr(q), ptr(k), ptr(v), ptr(lse), ptr(key_valid), ptr(dq), ptr(dk), ptr(dv),
                                   ptr(ws), nbytes, B, H, T, S, D, dtype_code(q), stream_ptr())
        return dq, dk, dv, None, None


def xattn_core(q, k, v, key_valid, num_heads):
    """softmax(max(q k^T + M, finfo.min)) v per head.  q [B,T,d] is already scaled; k, v [B,S,d];
    key_valid [B,S] bool/uint8 (True = attend).  Mirrors the core of MPTAttention.forward
    (reference model/modelling_cross_attention.py:206-271)."""
    _attn_args("xattn_core", q, k, v, key_valid, num_heads)
    return _XAttnCore.apply(q, k, v, _key_valid(key_valid), num_heads)


# ------------------------------------------------------------------------------------------ general (unfused) attention core
class _AttnGeneral(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, key_valid, head_mask, num_heads, causal, p_drop, seed, want_probs):
        require_cuda(q, k, v, key_valid)
        B, T, d = q.shape
        S = k.shape[1]
        D = d // num_heads
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        out = torch.empty_like(q)
        lse = torch.empty(B, num_heads, T, dtype=torch.float32, device=q.device)
        probs = torch.empty(B, num_heads, T, S, dtype=q.dtype, device=q.device) if want_probs else None
        hm = None if head_mask is None else head_mask.detach().to(device=q.device, dtype=torch.float32).contiguous()
        _lib.call("mmgl_attn_general_fwd", dict(flops=4.0 * B * T * S * d), ptr(q), ptr(k), ptr(v), ptr(key_valid), ptr(hm),
                  ptr(out), ptr(probs), ptr(lse), B, num_heads, T, S, D, int(causal), float(p_drop), int(seed),
                  dtype_code(q), stream_ptr())
        ctx.save_for_backward(q, k, v, key_valid, lse, hm)
        ctx.cfg = (num_heads, int(causal), float(p_drop), int(seed))
        if probs is not None:
            ctx.mark_non_differentiable(probs)
            return out, probs
        return out, None

    @staticmethod
    def backward(ctx, dout, _dprobs):
        q, k, v, key_valid, lse, hm = ctx.saved_tensors
        H, causal, p_drop, seed = ctx.cfg
        B, T, d = q.shape
        S = k.shape[1]
        D = d // H
        dout = dout.contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        nbytes = lib().mmgl_attn_general_bwd_workspace(B, H, T)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
        _lib.call("mmgl_attn_general_bwd", dict(flops=10.0 * B * T * S * d), ptr(dout), ptr(q), ptr(k), ptr(v), ptr(lse), ptr(key_valid),
                  ptr(hm), ptr(dq), ptr(dk), ptr(dv), ptr(ws), nbytes, B, H, T, S, D, causal, p_drop, seed,
                  dtype_code(q), stream_ptr())
        return dq, dk, dv, None, None, None, None, None, None, None


def attn_general(q, k, v, key_valid, num_heads, causal=False, head_mask=None, p_drop=0.0, training=False, seed=None, output_attentions=False):
    """The attention core with the options the fused kernels leave out (reference model/modelling_cross_attention.py:206-271):
    `head_mask` [H] scales the probabilities of each head (:237-244), `output_attentions` also returns them as [B,H,T,S] -- head-masked,
    before dropout (:246-254); the returned tensor is DETACHED (the reference keeps it in the graph, ":248 make sure that attn_weights
    keeps its gradient": differentiating through the returned probabilities is not supported here and autograd will say so) --, `p_drop` drops probabilities in training (:256; counter hash of (seed, index),
    regenerated in backward).  q [B,T,d] is already scaled; causal = the decoder's self-attention (S == T).  Returns (out, probs | None)."""
    _attn_args("attn_general", q, k, v, key_valid, num_heads)
    if head_mask is not None and tuple(head_mask.shape) != (num_heads,):
        raise ValueError(f"Head mask for a single layer should be of size {(num_heads,)}, but is {tuple(head_mask.shape)}")
    if head_mask is not None and head_mask.requires_grad and torch.is_grad_enabled():
        # the reference's head mask is an ordinary multiplicand (:243): a head-importance / pruning workflow differentiates through it.
        # This kernel treats it as a constant -- refuse rather than hand back a silent zero gradient
        raise NotImplementedError("attn_general: head_mask.requires_grad is not supported (the kernel computes no gradient for the head "
                                  "mask); detach it, or differentiate a per-head scale applied outside the attention core")
    p, seed = _dropout(p_drop, training, seed)
    return _AttnGeneral.apply(q, k, v, _key_valid(key_valid), head_mask, num_heads, bool(causal), p, seed, bool(output_attentions))


def attn_dropout_mask(B, H, T, S, p_drop, seed, device):
    """The keep mask attn_general uses for (p_drop, seed), as uint8 [B,H,T,S]: test / debug aid."""
    m = torch.empty(B, H, T, S, dtype=torch.uint8, device=device)
    _lib.call("mmgl_attn_dropout_mask", None, ptr(m), B, H, T, S, float(p_drop), int(seed), stream_ptr())
    return m


# ------------------------------------------------------------------------------------------ T5 attention (relative-position bias)
class _AttnRelBias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, key_valid, table, bucket_of, num_heads, causal, p_drop, seed):
        require_cuda(q, k, v, key_valid, table, bucket_of)
        B, T, d = q.shape
        S = k.shape[1]
        D = d // num_heads
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        out = torch.empty_like(q)
        lse = torch.empty(B, num_heads, T, dtype=torch.float32, device=q.device)
        tab = None if table is None else table.detach().to(torch.float32).contiguous()
        nb = 0 if tab is None else tab.shape[0]
        _lib.call("mmgl_attn_relbias_fwd", dict(flops=4.0 * B * T * S * d), ptr(q), ptr(k), ptr(v), ptr(key_valid), ptr(tab),
                  ptr(bucket_of), ptr(out), ptr(lse), B, num_heads, T, S, D, nb, d, d, int(causal), float(p_drop), int(seed),
                  dtype_code(q), stream_ptr())
        ctx.save_for_backward(q, k, v, key_valid, tab, bucket_of, out, lse)
        ctx.cfg = (num_heads, int(causal), float(p_drop), int(seed), None if table is None else table.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, key_valid, tab, bucket_of, out, lse = ctx.saved_tensors
        H, causal, p_drop, seed, table_dtype = ctx.cfg
        B, T, d = q.shape
        S = k.shape[1]
        D = d // H
        dout = dout.contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        dtab = None if tab is None else torch.empty_like(tab)
        nb = 0 if tab is None else tab.shape[0]
        nbytes = lib().mmgl_attn_relbias_bwd_workspace(B, H, T, S)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
        _lib.call("mmgl_attn_relbias_bwd", dict(flops=10.0 * B * T * S * d), ptr(dout), ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse),
                  ptr(key_valid), ptr(tab), ptr(bucket_of), ptr(dq), ptr(dk), ptr(dv), ptr(dtab), ptr(ws), nbytes, B, H, T, S, D, nb,
                  d, d, causal, p_drop, seed, dtype_code(q), stream_ptr())
        return dq, dk, dv, None, None if dtab is None else dtab.to(table_dtype), None, None, None, None, None


def attn_relbias(q, k, v, key_valid, num_heads, table=None, bucket_of=None, causal=False, p_drop=0.0, training=False, seed=None):
    """T5's attention core (transformers T5Attention.forward): softmax(q k^T + table[bucket_of[s - t + T - 1], h]) v per head, unscaled,
    over the keys key_valid [B,S] allows (None: all; causal: also s <= t, S == T).  q [B,T,d]; k, v [B,S,d]; `table` [num_buckets, H] is
    the relative_attention_bias weight in its own dtype (read as fp32, its gradient comes back in its dtype) or None for no bias (the
    decoder-to-encoder cross-attention); `bucket_of` int32 [T+S-1] from t5_bucket_table.  `p_drop` drops probabilities in training
    (counter hash of (seed, index), regenerated in backward).  A row without an allowed key gives zeros (HuggingFace: uniform)."""
    if key_valid is None:
        key_valid = torch.ones(k.shape[:2], dtype=torch.uint8, device=k.device)
    _attn_args("attn_relbias", q, k, v, key_valid, num_heads)
    B, T, _ = q.shape
    S = k.shape[1]
    if causal and S != T:
        raise ValueError(f"attn_relbias: causal attention needs S == T (got {S}, {T})")
    if table is not None:
        if table.dim() != 2 or table.shape[1] != num_heads:
            raise ValueError(f"attn_relbias: table should be of size (num_buckets, {num_heads}), but is {tuple(table.shape)}")
        if bucket_of is None or bucket_of.dtype != torch.int32 or tuple(bucket_of.shape) != (T + S - 1,):
            raise ValueError(f"attn_relbias: bucket_of must be int32 of size ({T + S - 1},) (ops.t5_bucket_table)")
        bucket_of = bucket_of.contiguous()
    else:
        bucket_of = None
    p, seed = _dropout(p_drop, training, seed)
    return _AttnRelBias.apply(q, k, v, _key_valid(key_valid), table, bucket_of, num_heads, bool(causal), p, seed)


_BUCKET_TABLES = {}


def t5_bucket_table(T, S, bidirectional, num_buckets, max_distance, device):
    """bucket_of int32 [T+S-1] for attn_relbias: entry s - t + T - 1 is the bucket of the relative position s - t, computed by
    transformers' own T5Attention._relative_position_bucket (so the bucket boundaries are HuggingFace's by construction).  Cached per
    argument tuple."""
    key = (int(T), int(S), bool(bidirectional), int(num_buckets), int(max_distance), str(torch.device(device)))
    t = _BUCKET_TABLES.get(key)
    if t is None:
        from transformers.models.t5.modeling_t5 import T5Attention
        rel = torch.arange(-(int(T) - 1), int(S), dtype=torch.long)
        t = T5Attention._relative_position_bucket(rel, bidirectional=bool(bidirectional), num_buckets=int(num_buckets),
                                                  max_distance=int(max_distance)).to(torch.int32).to(device)
        _BUCKET_TABLES[key] = t
    return t


# ------------------------------------------------------------------------------------------ causal self-attention
# One pair of call helpers for every self-attention op.  q / k / v (and dq / dk / dv) are device pointers.  P is None: the plain entry
# points mmgl_selfattn_fwd / _bwd, rows `ld` (`ldg` for the gradients) elements apart, 0 = packed.  P >= 0: mmgl_selfattn_prefix_fwd /
# _bwd with P always-visible keys in front of the T causal ones, packed.  `like` gives dtype and device.
def _selfattn_fwd(like, qp, kp, vp, key_valid, B, T, d, H, P, ld):
    out = torch.empty(B, T, d, dtype=like.dtype, device=like.device)
    lse = torch.empty(B, H, T, dtype=torch.float32, device=like.device)
    work = dict(flops=2.0 * B * T * (T + 2 * (P or 0)) * d, bytes=4.0 * B * T * d * like.element_size())
    if P is None:
        _lib.call("mmgl_selfattn_fwd", work, qp, kp, vp, ptr(key_valid), ptr(out), ptr(lse), B, H, T, d // H, ld, dtype_code(like), stream_ptr())
    else:
        _lib.call("mmgl_selfattn_prefix_fwd", work, qp, kp, vp, ptr(key_valid), ptr(out), ptr(lse), B, H, T, P, d // H, 0, 0, dtype_code(like),
                  stream_ptr())
    return out, lse


def _selfattn_bwd(like, dout, qp, kp, vp, out, lse, key_valid, dqp, dkp, dvp, B, T, d, H, P, ld, ldg):
    dout = dout.contiguous()
    nbytes = lib().mmgl_selfattn_bwd_workspace(B, H, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=like.device)
    work = dict(flops=5.0 * B * T * (T + 2 * (P or 0)) * d, bytes=8.0 * B * T * d * like.element_size())
    ptrs = (ptr(dout), qp, kp, vp, ptr(out), ptr(lse), ptr(key_valid), dqp, dkp, dvp, ptr(ws), nbytes)
    if P is None:
        _lib.call("mmgl_selfattn_bwd", work, *ptrs, B, H, T, d // H, ld, ldg, dtype_code(like), stream_ptr())
    else:
        _lib.call("mmgl_selfattn_prefix_bwd", work, *ptrs, B, H, T, P, d // H, 0, 0, 0, 0, dtype_code(like), stream_ptr())


class _SelfAttn(torch.autograd.Function):
    """Causal self-attention over separate q [B,T,d], k, v [B,P+T,d]; P is None for selfattn_core (see _selfattn_fwd)."""

    @staticmethod
    def forward(ctx, q, k, v, key_valid, num_heads, P):
        require_cuda(q, k, v, key_valid)
        B, T, d = q.shape
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        out, lse = _selfattn_fwd(q, ptr(q), ptr(k), ptr(v), key_valid, B, T, d, num_heads, P, 0)
        ctx.save_for_backward(q, k, v, key_valid, out, lse)
        ctx.num_heads, ctx.P = num_heads, P
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, key_valid, out, lse = ctx.saved_tensors
        B, T, d = q.shape
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        _selfattn_bwd(q, dout, ptr(q), ptr(k), ptr(v), out, lse, key_valid, ptr(dq), ptr(dk), ptr(dv), B, T, d, ctx.num_heads, ctx.P, 0, 0)
        return dq, dk, dv, None, None, None


class _SelfAttnFusedQKV(torch.autograd.Function):
    """Same kernels, Q/K/V read in place from one fused projection output [B,T,3d] and dQ/dK/dV written into one
    [B,T,3d] buffer (row stride 3d), so the projection's dgrad is ONE GEMM and autograd adds nothing up."""

    @staticmethod
    def forward(ctx, qkv, key_valid, num_heads):
        require_cuda(qkv, key_valid)
        B, T, d3 = qkv.shape
        d = d3 // 3
        qkv = qkv.contiguous()
        es = qkv.element_size()
        out, lse = _selfattn_fwd(qkv, ptr(qkv), ptr_off(qkv, d * es), ptr_off(qkv, 2 * d * es), key_valid, B, T, d, num_heads, None, d3)
        ctx.save_for_backward(qkv, key_valid, out, lse)
        ctx.num_heads = num_heads
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, key_valid, out, lse = ctx.saved_tensors
        B, T, d3 = qkv.shape
        d = d3 // 3
        es = qkv.element_size()
        dqkv = torch.empty_like(qkv)
        _selfattn_bwd(qkv, dout, ptr(qkv), ptr_off(qkv, d * es), ptr_off(qkv, 2 * d * es), out, lse, key_valid,
                      ptr(dqkv), ptr_off(dqkv, d * es), ptr_off(dqkv, 2 * d * es), B, T, d, ctx.num_heads, None, d3, d3)
        return dqkv, None, None


# Grouped-query attention (mmgl_selfattn_gqa_*): k, v [B,T,Hkv*D], query head h reads key / value head h // (H // Hkv).
def _gqa_fwd(like, qp, kp, vp, key_valid, B, T, H, Hkv, D, ldq, ldkv):
    out = torch.empty(B, T, H * D, dtype=like.dtype, device=like.device)
    lse = torch.empty(B, H, T, dtype=torch.float32, device=like.device)
    work = dict(flops=2.0 * B * T * T * H * D, bytes=2.0 * B * T * (H + Hkv) * D * like.element_size())
    _lib.call("mmgl_selfattn_gqa_fwd", work, qp, kp, vp, ptr(key_valid), ptr(out), ptr(lse), B, H, Hkv, T, D, ldq, ldkv, dtype_code(like),
              stream_ptr())
    return out, lse


def _gqa_bwd(like, dout, qp, kp, vp, out, lse, key_valid, dqp, dkp, dvp, B, T, H, Hkv, D, ldq, ldkv, ldgq, ldgkv):
    dout = dout.contiguous()
    nbytes = lib().mmgl_selfattn_gqa_bwd_workspace(B, H, Hkv, T, D, dtype_code(like))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=like.device)
    work = dict(flops=5.0 * B * T * T * H * D, bytes=(4.0 * (H + Hkv) + 4.0 * H) * B * T * D * like.element_size())
    _lib.call("mmgl_selfattn_gqa_bwd", work, ptr(dout), qp, kp, vp, ptr(out), ptr(lse), ptr(key_valid), dqp, dkp, dvp, ptr(ws), nbytes,
              B, H, Hkv, T, D, ldq, ldkv, ldgq, ldgkv, dtype_code(like), stream_ptr())


class _SelfAttnGQA(torch.autograd.Function):
    """Causal grouped-query self-attention over separate q [B,T,H*D], k, v [B,T,Hkv*D]."""

    @staticmethod
    def forward(ctx, q, k, v, key_valid, H, Hkv):
        require_cuda(q, k, v, key_valid)
        B, T, d = q.shape
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        out, lse = _gqa_fwd(q, ptr(q), ptr(k), ptr(v), key_valid, B, T, H, Hkv, d // H, 0, 0)
        ctx.save_for_backward(q, k, v, key_valid, out, lse)
        ctx.heads = (H, Hkv)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, key_valid, out, lse = ctx.saved_tensors
        H, Hkv = ctx.heads
        B, T, d = q.shape
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        _gqa_bwd(q, dout, ptr(q), ptr(k), ptr(v), out, lse, key_valid, ptr(dq), ptr(dk), ptr(dv), B, T, H, Hkv, d // H, 0, 0, 0, 0)
        return dq, dk, dv, None, None, None


class _SelfAttnFusedGQA(torch.autograd.Function):
    """Same kernels, Q/K/V read in place from one fused projection output [B,T,(H+2Hkv)*D] and dQ/dK/dV written into one buffer of
    the same layout, so the projection's dgrad stays ONE GEMM."""

    @staticmethod
    def forward(ctx, qkv, key_valid, H, Hkv):
        require_cuda(qkv, key_valid)
        B, T, ld = qkv.shape
        D = ld // (H + 2 * Hkv)
        qkv = qkv.contiguous()
        es = qkv.element_size()
        out, lse = _gqa_fwd(qkv, ptr(qkv), ptr_off(qkv, H * D * es), ptr_off(qkv, (H + Hkv) * D * es), key_valid, B, T, H, Hkv, D, ld, ld)
        ctx.save_for_backward(qkv, key_valid, out, lse)
        ctx.heads = (H, Hkv)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, key_valid, out, lse = ctx.saved_tensors
        H, Hkv = ctx.heads
        B, T, ld = qkv.shape
        D = ld // (H + 2 * Hkv)
        es = qkv.element_size()
        dqkv = torch.empty_like(qkv)
        _gqa_bwd(qkv, dout, ptr(qkv), ptr_off(qkv, H * D * es), ptr_off(qkv, (H + Hkv) * D * es), out, lse, key_valid,
                 ptr(dqkv), ptr_off(dqkv, H * D * es), ptr_off(dqkv, (H + Hkv) * D * es), B, T, H, Hkv, D, ld, ld, ld, ld)
        return dqkv, None, None, None


def _kv_heads(op, num_heads, num_kv_heads):
    """None for the multi-head path (num_kv_heads is None or == num_heads), else the validated number of key / value heads."""
    if num_kv_heads is None or num_kv_heads == num_heads:
        return None
    if num_kv_heads < 1 or num_heads % num_kv_heads:
        raise ValueError(f"{op}: num_heads = {num_heads} must be a multiple of num_kv_heads = {num_kv_heads}")
    return int(num_kv_heads)


def selfattn_core_fused(qkv, key_valid, num_heads, num_kv_heads=None):
    """selfattn_core over a fused projection output: qkv [B,T,3d] = [q*scale | k | v] along the last dim.  Grouped-query attention
    (num_kv_heads = Hkv < H = num_heads): qkv [B,T,(H+2Hkv)*D], and the gradient comes back in the same layout."""
    Hkv = _kv_heads("selfattn_core_fused", num_heads, num_kv_heads)
    if Hkv is not None:
        if qkv.dim() != 3 or qkv.shape[2] % (num_heads + 2 * Hkv):
            raise ValueError(f"selfattn_core_fused: qkv{tuple(qkv.shape)} is not [B, T, (H+2*Hkv)*D] for H={num_heads}, Hkv={Hkv}")
        _check_mask(key_valid, qkv.shape[:2])
        return _SelfAttnFusedGQA.apply(qkv, _key_valid(key_valid), num_heads, Hkv)
    if qkv.dim() != 3 or qkv.shape[2] % (3 * num_heads):
        raise ValueError(f"selfattn_core_fused: qkv{tuple(qkv.shape)} is not [B, T, 3*H*D] for H={num_heads}")
    _check_mask(key_valid, qkv.shape[:2])
    return _SelfAttnFusedQKV.apply(qkv, _key_valid(key_valid), num_heads)


def selfattn_core(q, k, v, key_valid, num_heads, num_kv_heads=None):
    """Causal self-attention softmax(mask(q k^T)) v with mask = (s <= t) & key_valid[b, s]; q is already scaled.
    The caller guarantees key_valid[:, 0] is all ones (see include/mmgl_hip.h).  (reference :203-271 self branch)
    num_kv_heads = Hkv < num_heads: grouped-query attention, k, v [B,T,Hkv*D], query head h reads key / value head h // (H // Hkv)."""
    Hkv = _kv_heads("selfattn_core", num_heads, num_kv_heads)
    if Hkv is not None:
        if (q.dim() != 3 or k.dim() != 3 or k.shape != v.shape or q.shape[:2] != k.shape[:2] or q.shape[2] % num_heads
                or k.shape[2] != q.shape[2] // num_heads * Hkv):
            raise ValueError(f"selfattn_core: incompatible shapes q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)} for H={num_heads}, Hkv={Hkv}")
        _check_mask(key_valid, k.shape[:2])
        return _SelfAttnGQA.apply(q, k, v, _key_valid(key_valid), num_heads, Hkv)
    _attn_args("selfattn_core", q, k, v, key_valid, num_heads, 0)
    return _SelfAttn.apply(q, k, v, _key_valid(key_valid), num_heads, None)


def selfattn_core_prefix(q, k, v, key_valid, num_heads, prefix_len):
    """softmax(mask(q k^T)) v where k, v [B, P+T, d] carry P = prefix_len always-visible rows in front of the T causal ones:
    mask = (s <= t + P) & key_valid[b, s]; q [B, T, d] is already scaled.  The attention of an OPT layer under peft prefix tuning
    (reference model/modelling_self_attention.py:88-93: HF prepends the learned per-layer key/value prefix as past_key_values)."""
    _attn_args("selfattn_core_prefix", q, k, v, key_valid, num_heads, prefix_len, f" for a prefix of {prefix_len}")
    return _SelfAttn.apply(q, k, v, _key_valid(key_valid), num_heads, int(prefix_len))


# ------------------------------------------------------------------------------------------ live key tiles of the frozen layers
# A padded position is a masked key in every frozen layer: its K and V are never read and its dK, dV are zero.  The flash kernels
# already skip a 64-key tile without a valid key; here such a tile is not projected either.  The LayerNorm in front of the attention
# stores the rows of the live tiles a second time, compact (yc); K | V = yc Wkv^T has 64 x (live tiles) rows, the kernels find a
# tile's rows through a table.  Every element of Q, K and V is the sum the fused [M, 3d] GEMM forms, so the attention output is bitwise
# the dense path's; dQ | dK | dV keep the dense [B, T, 3d] layout and the fused dgrad, whose one rounding of dQ Wq' + dKV Wkv two
# GEMMs cannot reproduce.  Where the whole pre-LN block runs as one node (frozen_attn_block_tiles) the gradient rows are sorted live
# tiles first instead, and that one dgrad launch contracts the row tiles behind them over dQ alone: the same sums minus their zero tails.
KEY_TILE = 64


def key_tile_table(attention_mask):
    """Host side: (table, m_live) of a [B, T] key mask that is still in host memory.  table [B, T // 64] int32: the compact index of
    a key tile that holds a valid key -- tiles are numbered sample by sample, in key order -- and -1 for a tile of padding;
    m_live = 64 x the number of live tiles.  (None, 0) when T is no multiple of 64."""
    am = attention_mask.cpu() != 0
    B, T = am.shape
    if T == 0 or T % KEY_TILE:
        return None, 0
    live = am.view(B, T // KEY_TILE, KEY_TILE).any(dim=-1).reshape(-1)
    index = torch.cumsum(live.to(torch.int32), 0, dtype=torch.int32) - 1
    table = torch.where(live, index, torch.full_like(index, -1)).view(B, T // KEY_TILE).contiguous()
    return table, KEY_TILE * int(live.sum())


def grad_tile_table(table, m_live):
    """(dest, rows) of a key-tile table, on the table's device: the live-first order of the gradient rows.  dest [B, T // 64] int32
    is a permutation of the batch's tiles -- a live tile goes to its compact index, a dead one to m_live // 64 + its rank among the
    dead tiles -- and rows [B * T] int32 the row of every dense row under it, 64 dest + (row % 64).  No synchronisation."""
    t = table.reshape(-1)
    dead = t < 0
    rank = torch.cumsum(dead.to(torch.int32), 0, dtype=torch.int32) - 1
    dest = torch.where(dead, rank + int(m_live) // KEY_TILE, t).to(torch.int32)
    rows = dest.view(-1, 1) * KEY_TILE + torch.arange(KEY_TILE, dtype=torch.int32, device=table.device)
    return dest.view(table.shape).contiguous(), rows.reshape(-1).contiguous()


class KeyTiles:
    """key_tile_table's result on the device, for one forward / backward pass: table [B, T // 64] int32, rowmap [B * T] int32 (the
    compact row of every row of a live tile, -1 elsewhere) and m_live, a host integer -- no synchronisation.  dest / grad_rows: the
    live-first order of the gradient rows (grad_tile_table)."""
    __slots__ = ("table", "rowmap", "m_live", "dest", "grad_rows")

    def __init__(self, table, m_live, device):
        self.table = table.to(device=device, dtype=torch.int32, non_blocking=True).contiguous()
        self.m_live = int(m_live)
        t = self.table.view(-1, 1)
        rows = t * KEY_TILE + torch.arange(KEY_TILE, dtype=torch.int32, device=self.table.device)
        self.rowmap = torch.where(t >= 0, rows, torch.full_like(rows, -1)).reshape(-1).contiguous()
        self.dest, self.grad_rows = grad_tile_table(self.table, self.m_live)

    def fits(self, B, T):
        return self.m_live > 0 and tuple(self.table.shape) == (B, T // KEY_TILE) and T % KEY_TILE == 0


def selfattn_tiles_supported(like, num_heads, tiles):
    """Whether frozen_selfattn_tiles takes activations `like` [B, T, d] with this table: the D = 64 bf16 flash kernels, T a multiple
    of 64 within their 4096 keys."""
    B, T, d = like.shape
    return (tiles is not None and like.is_cuda and like.dtype == torch.bfloat16 and d == 64 * num_heads and T <= 4096
            and tiles.fits(B, T))


def layer_norm_tiles(x, gamma, beta, eps, tiles):
    """(residual, y, yc): layer_norm_fanout plus the compact copy yc [tiles.m_live, d] of the rows of y in live key tiles.  Without
    gradients flowing the plain forward kernel runs (no autograd node, no statistics kept)."""
    if torch.is_grad_enabled() and x.requires_grad:
        return _NormPair.apply(x, None, gamma, beta, float(eps), False, 0.0, 0, tiles)
    yc = x.new_empty(tiles.m_live, x.shape[-1])
    with torch.no_grad():
        _, y, _, _, _ = _norm_fwd(False, x, None, gamma, beta, float(eps), compact=(tiles.rowmap, yc))
    return x, y.view(x.shape), yc


def add_layer_norm_tiles(x, res, gamma, beta, eps, tiles, p_drop=0.0, training=False, seed=None):
    """(s, LayerNorm(s), yc) with s = res + dropout(x): add_layer_norm_pair plus the compact copy (see layer_norm_tiles)."""
    if x.shape != res.shape:
        raise ValueError(f"add_layer_norm_tiles: shapes differ {tuple(x.shape)} vs {tuple(res.shape)}")
    return _NormPair.apply(x, res, gamma, beta, float(eps), False, *_dropout(p_drop, training, seed), tiles)


class _FrozenSelfAttnTiles(torch.autograd.Function):
    """The frozen QKV projection and the causal attention of one layer on live key tiles: Q = y Wq'^T over all rows, K | V = yc Wkv^T
    over the m_live compact rows (both row blocks of the fused frozen weight w [3d, d] = (q * scaling | k | v), without K splits: the
    summation order of the fused GEMM), attention through mmgl_selfattn_tiles_*.  Backward: dQ | dK | dV in the dense [B, T, 3d] layout
    (zeros in the dead tiles) and the fused dgrad of frozen_linear, so the gradient is bitwise the dense path's; yc gets none."""

    @staticmethod
    def forward(ctx, y, yc, w, b, key_valid, tiles, num_heads):
        require_cuda(y, yc, key_valid)
        B, T, d = y.shape
        m = tiles.m_live
        y2 = y.contiguous().view(-1, d)
        q = gemm_nt(y2, w[:d], None if b is None else b[:d], k_splits=False)
        kv = gemm_nt(yc, w[d:], None if b is None else b[d:], k_splits=False)
        out = torch.empty(B, T, d, dtype=y.dtype, device=y.device)
        lse = torch.empty(B, num_heads, T, dtype=torch.float32, device=y.device)
        es = y.element_size()
        work = dict(flops=2.0 * B * T * T * d, bytes=(2.0 * B * T * d + 2.0 * m * d) * es)
        _lib.call("mmgl_selfattn_tiles_fwd", work, ptr(q), ptr(kv), ptr_off(kv, d * es), ptr(key_valid), ptr(tiles.table), ptr(out), ptr(lse),
                  B, num_heads, T, d // num_heads, m, d, 2 * d, dtype_code(y), stream_ptr())
        ctx.save_for_backward(q, kv, key_valid, out, lse, w)
        ctx.tiles, ctx.num_heads = tiles, num_heads
        return out

    @staticmethod
    def backward(ctx, dout):
        q, kv, key_valid, out, lse, w = ctx.saved_tensors
        tiles, H = ctx.tiles, ctx.num_heads
        B, T, d = out.shape
        m, es = tiles.m_live, out.element_size()
        dout = dout.contiguous()
        dqkv = torch.empty(B, T, 3 * d, dtype=out.dtype, device=out.device)
        nbytes = lib().mmgl_selfattn_bwd_workspace(B, H, T)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=out.device)
        work = dict(flops=5.0 * B * T * T * d, bytes=(6.0 * B * T * d + 2.0 * m * d) * es)
        _lib.call("mmgl_selfattn_tiles_bwd", work, ptr(dout), ptr(q), ptr(kv), ptr_off(kv, d * es), ptr(out), ptr(lse), ptr(key_valid),
                  ptr(tiles.table), ptr(dqkv), ptr_off(dqkv, d * es), ptr_off(dqkv, 2 * d * es), ptr(ws), nbytes, B, H, T, d // H, m, d, 2 * d,
                  3 * d, 3 * d, dtype_code(out), stream_ptr())
        return frozen_dgrad(dqkv.view(-1, 3 * d), w).view(B, T, d), None, None, None, None, None, None


def frozen_selfattn_tiles(y, yc, w, b, key_valid, tiles, num_heads):
    """Causal self-attention of a frozen layer from its normed input y [B, T, d] and the compact copy yc [tiles.m_live, d] (see
    layer_norm_tiles): keys and values exist for the live key tiles only.  w [3d, d], b [3d] are the fused frozen projection
    (q * scaling | k | v); pass the same w object from call to call, as frozen_dgrad caches its transpose per object.  Check
    selfattn_tiles_supported first."""
    if not selfattn_tiles_supported(y, num_heads, tiles):
        raise ValueError(f"frozen_selfattn_tiles: y{tuple(y.shape)} {y.dtype} with {num_heads} heads is not a bf16 head_dim-64 batch "
                         f"whose [B, T // 64] table and m_live > 0 are given")
    if w.requires_grad or (b is not None and b.requires_grad) or w.shape != (3 * y.shape[2], y.shape[2]):
        raise ValueError("frozen_selfattn_tiles: w must be the frozen fused [3d, d] projection")
    if yc.shape != (tiles.m_live, y.shape[2]):
        raise ValueError(f"frozen_selfattn_tiles: yc{tuple(yc.shape)} is not [m_live = {tiles.m_live}, d]")
    _check_mask(key_valid, y.shape[:2])
    return _FrozenSelfAttnTiles.apply(y, yc, w, b, _key_valid(key_valid), tiles, num_heads)


def gemm_nt_rowk(x2, w, K_short, m_full, out=None):
    """Raw mmgl_gemm_nt_rowk call: x2 [M, K] @ w [N, K]^T where the 256-row tiles from row ceil(m_full / 256) * 256 on contract over
    the first K_short columns only -- x2 is zero (or uninitialised) behind them there.  One launch without K splits: the sums of
    gemm_nt(k_splits=False), minus a tail of exact zeros.  No autograd."""
    require_cuda(x2, w)
    M, K = x2.shape
    N = w.shape[0]
    if x2.stride(1) != 1 or w.stride(1) != 1 or w.shape[1] != K:
        raise ValueError("gemm_nt_rowk: operands need unit column stride and one K")
    y = torch.empty(M, N, dtype=x2.dtype, device=x2.device) if out is None else out
    mlong = min(M, -(-int(m_full) // 256) * 256)
    _lib.call("mmgl_gemm_nt_rowk", dict(flops=2.0 * N * (mlong * K + (M - mlong) * K_short), bytes=float(M * K + N * K + M * N) * x2.element_size(),
                                        tag=f"{M}x{N}x{K}|{K_short}@{int(m_full)}"),
              ptr(x2), x2.stride(0), ptr(w), w.stride(0), ptr(y), y.stride(0), M, N, K, int(K_short), int(m_full), dtype_code(x2), stream_ptr())
    return y


def frozen_attn_block_supported(like, num_heads, tiles, gamma, beta, w):
    """Whether frozen_attn_block_tiles takes activations `like` [B, T, d]: selfattn_tiles_supported, a frozen LayerNorm affine, and a
    dense fused dgrad [B T, 3d] -> [B T, d] that runs on the persistent GEMM kernel as whole tiles without K splits -- the one sum
    per element that the short-K launch reproduces -- within the 2 GiB of the attention kernels' gradient descriptors."""
    if not selfattn_tiles_supported(like, num_heads, tiles):
        return False
    if any(p is not None and p.requires_grad for p in (gamma, beta)) or w.dtype != like.dtype:
        return False
    B, T, d = like.shape
    M = B * T
    if d % 128 or M * 3 * d * 2 >= 2 ** 31:
        return False
    L = lib()
    return L.mmgl_gemm_nt_fast(M, d, 3 * d, 3 * d, 3 * d, d, _lib.BF16) == 1 and L.mmgl_gemm_nt_workspace(M, d, 3 * d, 3 * d, 3 * d, d, _lib.BF16) == 0


class _FrozenAttnBlockTiles(torch.autograd.Function):
    """The pre-LN attention block of a frozen layer on live key tiles as ONE node: (s, o) with s = x, or res + dropout(x), and
    o = attention(LayerNorm(s)) -- forward: the calls of _NormPair (with the compact copy) and _FrozenSelfAttnTiles, unchanged.
    Backward: the attention backward writes dQ | dK | dV with the rows sorted live key tiles first (KeyTiles.dest), so the rows from
    m_live on have dK = dV = 0 and the fused dgrad contracts their 256-row tiles over dQ alone (gemm_nt_rowk: one launch, one
    rounding, each sum minus its zero tail: the dense dgrad's bits); the LayerNorm backward reads that result through
    KeyTiles.grad_rows.  The permuted gradient lives inside this node only: it never reaches autograd as a tensor."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps, p, seed, tiles, w, b, key_valid, num_heads):
        require_cuda(x, key_valid)
        B, T, d = x.shape
        m = tiles.m_live
        yc = x.new_empty(m, d)
        s, y, g, mean, rstd = _norm_fwd(False, x, res, gamma, beta, eps, p, seed, compact=(tiles.rowmap, yc))
        q = gemm_nt(y, w[:d], None if b is None else b[:d], k_splits=False)
        kv = gemm_nt(yc, w[d:], None if b is None else b[d:], k_splits=False)
        out = torch.empty(B, T, d, dtype=x.dtype, device=x.device)
        lse = torch.empty(B, num_heads, T, dtype=torch.float32, device=x.device)
        es = x.element_size()
        work = dict(flops=2.0 * B * T * T * d, bytes=(2.0 * B * T * d + 2.0 * m * d) * es)
        _lib.call("mmgl_selfattn_tiles_fwd", work, ptr(q), ptr(kv), ptr_off(kv, d * es), ptr(key_valid), ptr(tiles.table), ptr(out), ptr(lse),
                  B, num_heads, T, d // num_heads, m, d, 2 * d, dtype_code(x), stream_ptr())
        ctx.save_for_backward(s, g, mean, rstd, q, kv, key_valid, out, lse, w)
        ctx.set_materialize_grads(False)
        ctx.cfg = (x.shape, p, seed, res is None, tiles, num_heads)
        return (x if res is None else s.view(x.shape)), out       # (autograd wraps the returned input as a view, see _NormPair)

    @staticmethod
    def backward(ctx, ds, dout):
        s, g, mean, rstd, q, kv, key_valid, out, lse, w = ctx.saved_tensors
        shape, p, seed, fanout, tiles, H = ctx.cfg
        nograd = (None,) * 10
        if dout is None:                                      # only the residual stream was used downstream (see _NormPair)
            if ds is None or p == 0.0:
                return (ds, None if fanout else ds) + nograd
            dres, dx, _, _ = _norm_bwd(False, True, torch.zeros_like(ds), ds, s, g, mean, rstd, (False, False), None, p, seed)
            return (dx.view(shape), dres.view(shape)) + nograd
        B, T, d = out.shape
        m, es = tiles.m_live, out.element_size()
        M = B * T
        dkv_rows = min(M, -(-m // 256) * 256)                 # the rows whose dK | dV columns the dgrad reads
        dout = dout.contiguous()
        dqkv = torch.empty(M, 3 * d, dtype=out.dtype, device=out.device)
        nbytes = lib().mmgl_selfattn_bwd_workspace(B, H, T)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=out.device)
        work = dict(flops=5.0 * B * T * T * d, bytes=(4.0 * B * T * d + 2.0 * dkv_rows * d + 2.0 * m * d) * es)
        _lib.call("mmgl_selfattn_tiles_rows_bwd", work, ptr(dout), ptr(q), ptr(kv), ptr_off(kv, d * es), ptr(out), ptr(lse), ptr(key_valid),
                  ptr(tiles.table), ptr(tiles.dest), ptr(dqkv), ptr_off(dqkv, d * es), ptr_off(dqkv, 2 * d * es), ptr(ws), nbytes, B, H, T,
                  d // H, m, dkv_rows, d, 2 * d, 3 * d, 3 * d, dtype_code(out), stream_ptr())
        dy = gemm_nt_rowk(dqkv, _transposed(w), d, m)         # rows in live-first order
        dres, dx, _, _ = _norm_bwd(False, True, dy, ds, s, g, mean, rstd, (False, False), None, p, seed, dy_rows=tiles.grad_rows)
        dres = dres.view(shape)
        if fanout:
            return (dres, None) + nograd
        return ((dres if dx is None else dx.view(shape)), dres) + nograd


def frozen_attn_block_tiles(x, res, gamma, beta, eps, w, b, key_valid, tiles, num_heads, p_drop=0.0, training=False, seed=None):
    """(s, o) of a frozen pre-LN layer's attention block: s = x (res None: the fan-out of layer_norm_tiles) or res + dropout(x)
    (add_layer_norm_tiles), o = frozen_selfattn_tiles(LayerNorm(s), its compact copy, w, b, key_valid, tiles, num_heads) -- the
    same values, one autograd node whose backward skips the zero dK | dV of the dead key tiles.  Check frozen_attn_block_supported
    first."""
    like = x
    if res is not None and x.shape != res.shape:
        raise ValueError(f"frozen_attn_block_tiles: shapes differ {tuple(x.shape)} vs {tuple(res.shape)}")
    if not frozen_attn_block_supported(like, num_heads, tiles, gamma, beta, w):
        raise ValueError(f"frozen_attn_block_tiles: x{tuple(x.shape)} {x.dtype} with {num_heads} heads does not take the one-node route "
                         "(frozen_attn_block_supported)")
    if w.requires_grad or (b is not None and b.requires_grad) or w.shape != (3 * x.shape[2], x.shape[2]):
        raise ValueError("frozen_attn_block_tiles: w must be the frozen fused [3d, d] projection")
    _check_mask(key_valid, x.shape[:2])
    p, seed = (0.0, 0) if res is None else _dropout(p_drop, training, seed)
    return _FrozenAttnBlockTiles.apply(x, res, gamma, beta, float(eps), p, seed, tiles, w, b, _key_valid(key_valid), num_heads)


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------------ LayerNorm / RMSNorm
# One forward and one backward route over the kernel family of csrc/rownorm.hip; between them they make every call to the eight
# mmgl_*norm* entry points.  rms picks RMSNorm (no mean, no beta); tensors are flattened to [rows, cols] here and stay 2-D inside.
def _norm_fwd(rms, x, res, gamma, beta, eps, p=0.0, seed=0, keep_sum=True, keep_stats=True, compact=None):
    """y = norm(s) in one launch, with s = x, or s = res + dropout(x) when `res` is given (the mmgl_add_* entry points, which also
    write s unless keep_sum is off).  Returns (s, y, gamma as the kernel read it, mean, rstd); mean / rstd are what the backward
    needs and are not computed with keep_stats off.  compact = (rowmap, yc): the LayerNorm entry points that also store the rows
    of the live key tiles to yc (see KeyTiles)."""
    require_cuda(x, res)
    cols = x.shape[-1]
    x2 = x.contiguous().view(-1, cols)
    rows = x2.shape[0]
    y = torch.empty_like(x2)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if keep_stats and not rms else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if keep_stats else None
    g = None if gamma is None else gamma.to(x.dtype).contiguous()
    b = None if beta is None else beta.to(x.dtype).contiguous()
    if compact is not None:
        rowmap, yc = compact
        if rms or rowmap.numel() != rows:
            raise ValueError(f"_norm_fwd: the compact copy is LayerNorm's, with one map entry per row ({rowmap.numel()} for {rows} rows)")
        work = dict(bytes=((2.0 if res is None else 3.0 + keep_sum) * rows * cols + yc.numel()) * x.element_size())
        if res is None:
            s = x2
            _lib.call("mmgl_layernorm_tiles_fwd", work, ptr(x2), ptr(g), ptr(b), ptr(y), ptr(yc), ptr(rowmap), ptr(mean), ptr(rstd), rows,
                      cols, yc.shape[0], eps, dtype_code(x), stream_ptr())
        else:
            r2 = res.contiguous().view(-1, cols)
            s = torch.empty_like(x2) if keep_sum else None
            _lib.call("mmgl_add_layernorm_tiles_fwd", work, ptr(x2), ptr(r2), ptr(g), ptr(b), ptr(s), ptr(y), ptr(yc), ptr(rowmap), ptr(mean),
                      ptr(rstd), rows, cols, yc.shape[0], eps, p, seed, dtype_code(x), stream_ptr())
    elif res is None:
        s = x2
        work = dict(bytes=2.0 * rows * cols * x.element_size())
        if rms:
            _lib.call("mmgl_rmsnorm_fwd", work, ptr(x2), ptr(g), ptr(y), ptr(rstd), rows, cols, eps, dtype_code(x), stream_ptr())
        else:
            _lib.call("mmgl_layernorm_fwd", work, ptr(x2), ptr(g), ptr(b), ptr(y), ptr(mean), ptr(rstd), rows, cols, eps, dtype_code(x),
                      stream_ptr())
    else:
        r2 = res.contiguous().view(-1, cols)
        s = torch.empty_like(x2) if keep_sum else None
        work = dict(bytes=(3.0 + keep_sum) * rows * cols * x.element_size())
        if rms:
            _lib.call("mmgl_add_rmsnorm_fwd", work, ptr(x2), ptr(r2), ptr(g), ptr(s), ptr(y), ptr(rstd), rows, cols, eps, dtype_code(x),
                      stream_ptr())
        else:
            _lib.call("mmgl_add_layernorm_fwd", work, ptr(x2), ptr(r2), ptr(g), ptr(b), ptr(s), ptr(y), ptr(mean), ptr(rstd), rows, cols,
                      eps, p, seed, dtype_code(x), stream_ptr())
    return s, y, g, mean, rstd


def _norm_bwd(rms, fused, dy, dsum, s, g, mean, rstd, pgrad, pdtype, p=0.0, seed=0, dy_rows=None):
    """The backward of _norm_fwd in one launch (plus the column reduction when a parameter gradient is wanted).  fused: the
    mmgl_add_* entry points, which add `dsum` (the gradient arriving on s, or None) inside the kernel and with p > 0 also write the
    gradient of the dropped-out x.  pgrad = (gamma, beta) need a gradient: LayerNorm computes both when either does; only the needed
    ones come back, in the parameters' dtype.  dy_rows [rows] int32 (fused LayerNorm only): row r's gradient is row dy_rows[r] of dy.
    Returns (ds, dx | None, dgamma | None, dbeta | None) with ds, dx [rows, cols]."""
    rows, cols = s.shape
    dy = dy.contiguous().view(rows, cols)
    dsum = None if dsum is None else dsum.contiguous().view(rows, cols)
    ds = torch.empty_like(s)
    dx = torch.empty_like(s) if p > 0.0 else None
    want = any(pgrad)
    dgamma = torch.empty(cols, dtype=torch.float32, device=s.device) if want else None
    dbeta = torch.empty(cols, dtype=torch.float32, device=s.device) if want and not rms else None
    nbytes = lib().mmgl_norm_bwd_workspace(rows, cols) if want else 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=s.device) if want else None
    work = dict(bytes=(3.0 + (dsum is not None) + (dx is not None)) * rows * cols * s.element_size())
    if dy_rows is not None:
        if rms or not fused or dy_rows.numel() != rows:
            raise ValueError(f"_norm_bwd: the row map is the fused LayerNorm's, one entry per row ({dy_rows.numel()} for {rows} rows)")
        _lib.call("mmgl_add_layernorm_rows_bwd", work, ptr(dy), ptr(dy_rows), ptr(dsum), ptr(s), ptr(g), ptr(mean), ptr(rstd), ptr(ds), ptr(dx),
                  ptr(dgamma), ptr(dbeta), ptr(ws), nbytes, rows, cols, p, seed, dtype_code(s), stream_ptr())
    elif not fused:
        if rms:
            _lib.call("mmgl_rmsnorm_bwd", work, ptr(dy), ptr(s), ptr(g), ptr(rstd), ptr(ds), ptr(dgamma), ptr(ws), nbytes, rows, cols,
                      dtype_code(s), stream_ptr())
        else:
            _lib.call("mmgl_layernorm_bwd", work, ptr(dy), ptr(s), ptr(g), ptr(mean), ptr(rstd), ptr(ds), ptr(dgamma), ptr(dbeta), ptr(ws),
                      nbytes, rows, cols, dtype_code(s), stream_ptr())
    elif rms:
        _lib.call("mmgl_add_rmsnorm_bwd", work, ptr(dy), ptr(dsum), ptr(s), ptr(g), ptr(rstd), ptr(ds), ptr(dgamma), ptr(ws), nbytes, rows,
                  cols, dtype_code(s), stream_ptr())
    else:
        _lib.call("mmgl_add_layernorm_bwd", work, ptr(dy), ptr(dsum), ptr(s), ptr(g), ptr(mean), ptr(rstd), ptr(ds), ptr(dx), ptr(dgamma),
                  ptr(dbeta), ptr(ws), nbytes, rows, cols, p, seed, dtype_code(s), stream_ptr())
    return ds, dx, (dgamma.to(pdtype) if pgrad[0] else None), (dbeta.to(pdtype) if pgrad[1] else None)


def _norm_ctx(ctx, rms, shape, gamma, beta, p=0.0, seed=0):
    pgrad = (gamma is not None and gamma.requires_grad, beta is not None and beta.requires_grad)
    ctx.cfg = (rms, shape, pgrad, None if gamma is None else gamma.dtype, p, seed)


class _Norm(torch.autograd.Function):
    """y = LayerNorm(x) or RMSNorm(x)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, rms):
        x2, y, g, mean, rstd = _norm_fwd(rms, x, None, gamma, beta, eps)
        ctx.save_for_backward(x2, g, mean, rstd)
        _norm_ctx(ctx, rms, x.shape, gamma, beta)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, g, mean, rstd = ctx.saved_tensors
        rms, shape, pgrad, pdtype, _, _ = ctx.cfg
        dx, _, dg, db = _norm_bwd(rms, False, dy, None, x2, g, mean, rstd, pgrad, pdtype)
        return dx.view(shape), dg, db, None, None


class _NormPair(torch.autograd.Function):
    """(s, y) = (res + dropout(x), norm(s)) in one pass; backward folds the gradient arriving on s into the norm's backward kernel,
    which writes the gradient of res and (when dropout is active) of x -- no separate residual kernels, no autograd accumulation
    add.  res=None is the fan-out of a pre-LN block (reference :316-320 `residual = hidden_states; hidden_states =
    self.self_attn_layer_norm(hidden_states)`, :347-350): s is x itself, returned as an alias of the input, so the gradient of the
    residual stream meets the norm's inside the kernel instead of in autograd's add over [B, T, d] at every fan-out (10 per step at
    config 3).
    tiles (a KeyTiles, else None): a third output yc [tiles.m_live, d], the rows of y that lie in a live key tile -- what a frozen layer
    projects to keys and values (frozen_selfattn_tiles).  It is a copy without a gradient of its own: the fused dgrad of that
    projection returns everything on y."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps, rms, p, seed, tiles):
        yc = None if tiles is None else x.new_empty(tiles.m_live, x.shape[-1])
        s, y, g, mean, rstd = _norm_fwd(rms, x, res, gamma, beta, eps, p, seed, compact=None if tiles is None else (tiles.rowmap, yc))
        ctx.save_for_backward(s, g, mean, rstd)
        ctx.set_materialize_grads(False)                      # an unused output arrives as None, not as a zero tensor to stream
        _norm_ctx(ctx, rms, x.shape, gamma, beta, p, seed)
        ctx.fanout = res is None
        outs = (x if res is None else s.view(x.shape)), y.view(x.shape)      # autograd wraps the returned input as a view
        if tiles is None:
            return outs
        ctx.mark_non_differentiable(yc)
        return outs + (yc,)

    @staticmethod
    def backward(ctx, ds, dy, _dyc=None):
        s, g, mean, rstd = ctx.saved_tensors
        rms, shape, pgrad, pdtype, p, seed = ctx.cfg
        if dy is None:                                        # only the residual stream was used downstream
            if ds is None or p == 0.0:
                return ds, (None if ctx.fanout else ds), None, None, None, None, None, None, None
            dy = torch.zeros_like(ds)                         # dropout: the kernel still has to mask ds into the gradient of x
        dres, dx, dg, db = _norm_bwd(rms, True, dy, ds, s, g, mean, rstd, pgrad, pdtype, p, seed)
        dres = dres.view(shape)
        if ctx.fanout:
            return dres, None, dg, db, None, None, None, None, None
        return (dres if dx is None else dx.view(shape)), dres, dg, db, None, None, None, None, None


def layer_norm(x, gamma, beta, eps=1e-5):
    """nn.LayerNorm over the last dim (reference model/modelling_cross_attention.py:287-294, 319-320, 349-350)."""
    return _Norm.apply(x, gamma, beta, float(eps), False)


def layer_norm_fanout(x, gamma, beta, eps=1e-5):
    """(residual, LayerNorm(x)) with residual == x: use BOTH outputs downstream (the residual add and the normed branch) so that
    the two gradients meet inside the LayerNorm backward kernel."""
    return _NormPair.apply(x, None, gamma, beta, float(eps), False, 0.0, 0, None)


def add_layer_norm_pair(x, res, gamma, beta, eps=1e-5, p_drop=0.0, training=False, seed=None):
    """Differentiable (s, LayerNorm(s)) with s = res + dropout(x): the `hidden = residual + dropout(h)` / next-LayerNorm
    pair of a decoder layer (reference model/modelling_cross_attention.py:332-350) as one forward and one backward
    kernel.  Dropout uses the same counter hash of (seed, element index) as gated_residual."""
    if x.shape != res.shape:
        raise ValueError(f"add_layer_norm_pair: shapes differ {tuple(x.shape)} vs {tuple(res.shape)}")
    return _NormPair.apply(x, res, gamma, beta, float(eps), False, *_dropout(p_drop, training, seed), None)


def rms_norm(x, gamma, eps=1e-6):
    return _Norm.apply(x, gamma, None, float(eps), True)


def add_rms_norm_pair(x, res, gamma, eps=1e-6):
    """Differentiable (s, RMSNorm(s)) with s = res + x: one forward and one backward kernel for the pair."""
    if x.shape != res.shape:
        raise ValueError(f"add_rms_norm_pair: shapes differ {tuple(x.shape)} vs {tuple(res.shape)}")
    return _NormPair.apply(x, res, gamma, None, float(eps), True, 0.0, 0, None)


# ------------------------------------------------------------------------------------------ gated residual
class _GatedResidual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, residual, x, gate, p_drop, seed):
        require_cuda(residual, x)
        residual, x = residual.contiguous(), x.contiguous()
        y = torch.empty_like(x)
        g32 = None if gate is None else gate.detach().to(torch.float32).reshape(1).contiguous()
        _lib.call("mmgl_gated_residual_fwd", dict(bytes=3.0 * x.numel() * x.element_size()), ptr(residual), ptr(x), ptr(g32), ptr(y), x.numel(), p_drop, seed,
                                            dtype_code(x), stream_ptr())
        ctx.save_for_backward(x, g32)
        ctx.p, ctx.seed = p_drop, seed
        ctx.gate_meta = None if gate is None else (gate.dtype, gate.shape, gate.requires_grad)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g32 = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dgate = torch.zeros(1, dtype=torch.float32, device=x.device) if g32 is not None else None
        ws = _ws(lib().mmgl_gated_residual_bwd_workspace(x.numel()), x.device)
        _lib.call("mmgl_gated_residual_bwd", dict(bytes=3.0 * x.numel() * x.element_size()), ptr(dy), ptr(x), ptr(g32), ptr(dx), ptr(dgate), ptr(ws), ws.numel(), x.numel(),
                                            ctx.p, ctx.seed, dtype_code(x), stream_ptr())
        dg = None
        if ctx.gate_meta is not None and ctx.gate_meta[2]:
            dg = dgate.to(ctx.gate_meta[0]).reshape(ctx.gate_meta[1])
        return dy, dx, dg, None, None


def gated_residual(residual, x, gate=None, p_drop=0.0, training=False, seed=None):
    """residual + tanh(gate) * dropout(x)  (reference :332-335, :356-359; gate=None is the ungated :337/:361 form).
    The dropout mask is a counter hash of (seed, index) regenerated in backward."""
    return _GatedResidual.apply(residual, x, gate, *_dropout(p_drop, training, seed))


# ------------------------------------------------------------------------------------------ linear (+bias, scale, ReLU)
_ACTS = {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU}      # the epilogues linear / frozen_linear differentiate


def _act_code(op, act):
    code = _ACTS.get(act)
    if code is None:
        raise ValueError(f"{op}: activation {act!r} is not fused (supported: none, relu)")
    return code


def _mfma_aligned(gemm, x, w, bias=None, residual=None, zmask=None, act=0, out_scale=1.0, out=None):
    """gemm(x, w, bias, residual, zmask, act, out_scale, K, out) -- gemm_nt's signature -- for any feature counts K = w.shape[1],
    N = w.shape[0].  The MFMA kernels move 16-byte chunks along K (8 bf16 / 4 fp32 elements) and 4 outputs per lane along N: an odd
    count (the Laplacian-PE input width k = N_neighbors - 4, a tiny test vocabulary) is zero-padded -- x [..., K] and w along K, w,
    bias, residual and zmask along N -- and the result is sliced back to N columns, into `out` when given.  Under autograd the pads
    and the slice carry the gradients back."""
    N, K = w.shape
    kq = 8 if x.dtype == torch.bfloat16 else 4
    if K % kq == 0 and N % 8 == 0:
        return gemm(x, w, bias, residual, zmask, act, out_scale, K, out)
    pk, pn = (-K) % kq, (-N) % 8
    x = F.pad(x, (0, pk)) if pk else x
    w = F.pad(w, (0, pk, 0, pn))
    bias, residual, zmask = (F.pad(c, (0, pn)) if (pn and c is not None) else c for c in (bias, residual, zmask))
    y = gemm(x, w, bias, residual, zmask, act, out_scale, K + pk, None)
    y = y[..., :N] if pn else y
    return y if out is None else out.copy_(y)


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act, out_scale, mask_dx=False, premasked=False):
        require_cuda(x, weight)
        shape = x.shape
        K = shape[-1]
        N = weight.shape[0]
        x2 = x.contiguous().view(-1, K)
        M = x2.shape[0]
        w = weight.to(x.dtype).contiguous()
        b = None if bias is None else bias.to(x.dtype).contiguous()
        y = torch.empty(M, N, dtype=x.dtype, device=x.device)
        _lib.call("mmgl_linear_fwd", dict(flops=2.0 * M * N * K, bytes=float(M * K + N * K + M * N) * x.element_size()), ptr(x2), ptr(w), ptr(b), ptr(y), M, N, K, act, out_scale, dtype_code(x), stream_ptr())
        # premasked: the consumer of y folds this layer's ReLU backward into its own dgrad (mask_dx there), so the incoming
        # gradient is already dy * (y > 0): differentiate as a plain linear and do not keep y for the mask
        ctx.save_for_backward(x2, w, y if (act and not premasked) else None)
        ctx.meta = (shape, 0 if premasked else act, out_scale, weight.dtype, None if bias is None else bias.dtype)
        ctx.mask_dx = bool(mask_dx)
        ctx.need = (x.requires_grad, weight.requires_grad, bias is not None and bias.requires_grad)
        return y.view(*shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, w, y = ctx.saved_tensors
        shape, act, out_scale, wdt, bdt = ctx.meta
        M, K = x2.shape
        N = w.shape[0]
        dy2 = dy.contiguous().view(M, N)
        code = dtype_code(x2)
        dx = torch.empty_like(x2) if ctx.need[0] else None
        want_w = ctx.need[1] or ctx.need[2]
        dw = torch.empty_like(w) if want_w else None
        db = torch.empty(N, dtype=x2.dtype, device=x2.device) if ctx.need[2] else None
        dx_lin = dx
        if dx is not None and act == _lib.ACT_NONE and not ctx.mask_dx and _dgrad_pad_to(dy2, w) > 1:
            # a contraction length that is no multiple of 128 (a trainable lm_head: N = vocab = 50272) has no large-tile dgrad in
            # mmgl_linear_bwd: frozen_dgrad's padded W^T puts it on the persistent kernel.  Built per call: the weight is being
            # trained, and a cached 2048 x 50304 copy would keep 206 MB alive
            frozen_dgrad(dy2, w, out=dx, out_scale=out_scale, wt=_padded_t(w, 128))
            dx_lin = None
        ws = _ws(lib().mmgl_linear_bwd_workspace(M, N, K, act, code), x2.device)
        _lib.call("mmgl_linear_bwd", dict(flops=2.0 * M * N * K * (int(dx_lin is not None) + int(dw is not None)),
                                         bytes=float(M * K + N * K + M * N) * x2.element_size()),
                  ptr(dy2), ptr(y), ptr(x2), ptr(w), ptr(dx_lin), ptr(dw), ptr(db), ptr(ws), ws.numel(), M, N, K, act, out_scale, 0,
                  int(ctx.mask_dx), code, stream_ptr())
        if dx is not None:
            dx = dx.view(shape)
        dw = dw.to(wdt) if (dw is not None and ctx.need[1]) else None
        db = db.to(bdt) if db is not None else None
        return dx, dw, db, None, None, None, None


def _linear(x, weight, bias, act, out_scale=1.0, mask_dx=False, premasked=False):
    return _mfma_aligned(lambda a, w, b, _r, _z, act_, scale, _K, _out: _Linear.apply(a, w, b, act_, scale, mask_dx, premasked),
                         x, weight, bias, act=act, out_scale=out_scale)


def linear(x, weight, bias=None, act="none", out_scale=1.0):
    """act((x @ weight.T + bias) * out_scale); weight is nn.Linear layout [out, in].
    (reference q/k/v/out_proj :194-199, :273; the fc1+ReLU / fc2 pair :352-355 is relu_ffn's)"""
    if x.shape[-1] != weight.shape[1]:
        raise ValueError(f"linear: x has {x.shape[-1]} features, weight expects {weight.shape[1]}")
    return _linear(x, weight, bias, _act_code("linear", act), float(out_scale))


class _LoraLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, A, Bm, scale):
        require_cuda(x, weight, A, Bm)
        shape = x.shape
        K = shape[-1]
        N, r = weight.shape[0], A.shape[0]
        x2 = x.contiguous().view(-1, K)
        M = x2.shape[0]
        w, a, bm = (t.to(x.dtype).contiguous() for t in (weight, A, Bm))
        b = None if bias is None else bias.to(x.dtype).contiguous()
        y = torch.empty(M, N, dtype=x.dtype, device=x.device)
        xa = torch.empty(M, r, dtype=x.dtype, device=x.device)
        _lib.call("mmgl_lora_linear_fwd", dict(flops=2.0 * M * N * K + 2.0 * M * r * (K + N)), ptr(x2), ptr(w), ptr(b), ptr(a), ptr(bm), ptr(y), ptr(xa), M, N, K, r, scale,
                                         dtype_code(x), stream_ptr())
        ctx.save_for_backward(x2, xa, w, a, bm)
        ctx.meta = (shape, scale, A.dtype, Bm.dtype)
        return y.view(*shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, xa, w, a, bm = ctx.saved_tensors
        shape, scale, adt, bdt = ctx.meta
        M, K = x2.shape
        N, r = w.shape[0], a.shape[0]
        dy2 = dy.contiguous().view(M, N)
        code = dtype_code(x2)
        dx, dA, dB = torch.empty_like(x2), torch.empty_like(a), torch.empty_like(bm)
        dyb = torch.empty(M, r, dtype=x2.dtype, device=x2.device)
        ws = _ws(lib().mmgl_lora_linear_bwd_workspace(M, N, K, r, code), x2.device)
        _lib.call("mmgl_lora_linear_bwd", dict(flops=2.0 * M * N * K + 6.0 * M * r * (K + N)), ptr(dy2), ptr(x2), ptr(xa), ptr(w), ptr(a), ptr(bm), ptr(dx), ptr(dA), ptr(dB), ptr(dyb),
                                         ptr(ws), ws.numel(), M, N, K, r, scale, 0, code, stream_ptr())
        return dx.view(shape), None, None, dA.to(adt), dB.to(bdt), None


def _wgrad_only(dy2, x2, w_like, scale):
    """dW [N, K] = scale * dy2^T x2 through mmgl_linear_bwd (no dx, no bias gradient); w_like: any [N, K] tensor of the dtype."""
    M, K = x2.shape
    N = dy2.shape[1]
    code = dtype_code(x2)
    dw = torch.empty(N, K, dtype=x2.dtype, device=x2.device)
    ws = _ws(lib().mmgl_linear_bwd_workspace(M, N, K, 0, code), x2.device)
    _lib.call("mmgl_linear_bwd", dict(flops=2.0 * M * N * K, bytes=float(M * K + N * K + M * N) * x2.element_size()),
              ptr(dy2), None, ptr(x2), ptr(w_like), None, ptr(dw), None, ptr(ws), ws.numel(), M, N, K, 0, float(scale), 0, 0, code, stream_ptr())
    return dw


def _lora_bwd(g, x2, xa, weight, A_pad, B_pad, dxa_scale, dB_scale, dx_scale, need_dx, need_dA, need_dB):
    """Backward of a frozen base product plus a rank-padded low-rank term, from g = dy [M, N], x2 [M, K], xa = x2 A_pad^T and the
    factors A_pad [256, K], B_pad [N, 256] as the forward used them: dxa = dxa_scale (g B_pad), dA = dxa^T x2, dB = dB_scale g^T xa,
    and dx = dx_scale g W + dxa A_pad as ONE dgrad GEMM with the low-rank term in its epilogue.  Returns (dx, dA, dB), None where
    not needed."""
    dxa = gemm_nt(g, B_pad.t().contiguous(), out_scale=dxa_scale)                   # [M, 256]
    dA = _wgrad_only(dxa, x2, A_pad, 1.0) if need_dA else None                       # [256, K]
    dB = _wgrad_only(g, xa, B_pad, dB_scale) if need_dB else None                    # [N, 256]
    dx = None
    if need_dx:
        low = gemm_nt(dxa, A_pad.t().contiguous())                                  # [M, K]
        dx = frozen_dgrad(g, weight, out_scale=dx_scale, residual=low)
    return dx, dA, dB


class _LoraLinearBig(torch.autograd.Function):
    """lora_linear for large bf16 shapes as ONE autograd node: the same seven GEMMs the composed form ran (rank zero-padded to
    256), but dx = dy W + (dy B) A leaves the second GEMM's residual epilogue instead of an ATen add, the pads / slices of the
    adapter gradients happen once, and nothing but x, x A^T and the padded factors is kept (config 4: 201 adds and 123 copies
    per step came from autograd's bookkeeping around the composed form)."""

    @staticmethod
    def forward(ctx, x, weight, bias, lora_A, lora_B, scale, out_scale=1.0):
        require_cuda(x, weight)
        K, N, r = x.shape[-1], weight.shape[0], lora_A.shape[0]
        rp = (-r) % 256
        A_pad = F.pad(lora_A.detach().to(x.dtype), (0, 0, 0, rp)).contiguous()          # [256, K]
        B_pad = F.pad(lora_B.detach().to(x.dtype), (0, rp)).contiguous()                # [N, 256]
        x2 = x.reshape(-1, K).contiguous()
        xa = gemm_nt(x2, A_pad)                                                         # [M, 256]
        delta = gemm_nt(xa, B_pad, out_scale=scale * out_scale)                         # [M, N]  (out_scale: attention's D^-1/2 on q_proj)
        w = weight if weight.dtype == x.dtype else weight.to(x.dtype)
        b = None if bias is None else (bias if bias.dtype == x.dtype else bias.to(x.dtype))
        out = torch.empty(*x.shape[:-1], N, dtype=x.dtype, device=x.device)
        gemm_nt(x2, w.contiguous(), b, residual=delta, out_scale=out_scale, out=out.view(-1, N))
        ctx.save_for_backward(x2, xa, weight, A_pad, B_pad)
        ctx.meta = (x.shape, float(scale), r, lora_A.dtype, lora_B.dtype, float(out_scale))
        return out

    @staticmethod
    def backward(ctx, dy):
        x2, xa, weight, A_pad, B_pad = ctx.saved_tensors
        xshape, scale, r, adt, bdt, os_ = ctx.meta
        N = weight.shape[0]
        g = dy.reshape(-1, N).contiguous()
        need = ctx.needs_input_grad
        # the scale enters through (dy B) and dB; out_scale (attention's D^-1/2 on q_proj) also scales dy W
        dx, dA, dB = _lora_bwd(g, x2, xa, weight, A_pad, B_pad, scale * os_, scale * os_, os_, need[0], need[3], need[4])
        return (None if dx is None else dx.view(xshape), None, None, None if dA is None else dA[:r].to(adt),
                None if dB is None else dB[:, :r].contiguous().to(bdt), None, None)


class _LoraQKV(torch.autograd.Function):
    """q | k | v of a self-attention layer whose q_proj and v_proj carry LoRA adapters over frozen weights and whose k_proj is
    frozen (peft's default targets for OPT, reference model/modelling_self_attention.py:80-87), as ONE autograd node over the
    layer's fused [3d, K] weight: forward = x [A_q ; A_v]^T (one skinny GEMM, both adapters in one rank-padded factor), the fused
    base GEMM, and the two low-rank updates accumulated IN PLACE into the q and v column blocks (residual = output); backward, from
    the attention kernels' fused dq | dk | dv buffer = (dqkv B_cat) in one GEMM, both adapters' dB / dA in one weight-gradient
    GEMM each, and dx = dqkv W_qkv + (dqkv B_cat) A_cat as ONE dgrad GEMM with the low-rank term in its epilogue.  Against three
    separate projections: 5 GEMMs instead of 11 in backward, 4 instead of 7 forward, and none of autograd's two gradient adds per
    layer (x feeds three nodes there)."""

    @staticmethod
    def forward(ctx, x, w_qkv, b_qkv, Aq, Bq, Av, Bv, scale, q_scale):
        require_cuda(x, w_qkv)
        K, d, r = x.shape[-1], w_qkv.shape[0] // 3, Aq.shape[0]
        dt, dev = x.dtype, x.device
        x2 = x.reshape(-1, K).contiguous()
        M = x2.shape[0]
        A_cat = torch.zeros(256, K, dtype=dt, device=dev)                               # rows 0..r-1: A_q, r..2r-1: A_v
        A_cat[:r], A_cat[r:2 * r] = Aq.detach().to(dt), Av.detach().to(dt)
        B_cat = torch.zeros(3 * d, 256, dtype=dt, device=dev)                           # [q rows | k rows = 0 | v rows] x [q ranks | v ranks]
        B_cat[:d, :r] = Bq.detach().float().mul(scale * q_scale).to(dt)
        B_cat[2 * d:, r:2 * r] = Bv.detach().float().mul(scale).to(dt)
        xa = gemm_nt(x2, A_cat)                                                         # [M, 256]
        qkv = torch.empty(*x.shape[:-1], 3 * d, dtype=dt, device=dev)
        q2 = qkv.view(M, 3 * d)
        gemm_nt(x2, w_qkv, b_qkv, out=q2)
        gemm_nt(xa, B_cat[:d], residual=q2[:, :d], out=q2[:, :d])                       # q += s qs (x A_q^T) B_q^T   (in place)
        gemm_nt(xa, B_cat[2 * d:], residual=q2[:, 2 * d:], out=q2[:, 2 * d:])           # v += s (x A_v^T) B_v^T
        ctx.save_for_backward(x2, xa, w_qkv, A_cat, B_cat)
        ctx.meta = (x.shape, r, float(scale), float(q_scale), Aq.dtype, Bq.dtype)
        return qkv

    @staticmethod
    def backward(ctx, dqkv):
        x2, xa, w_qkv, A_cat, B_cat = ctx.saved_tensors
        xshape, r, scale, q_scale, adt, bdt = ctx.meta
        d = w_qkv.shape[0] // 3
        g = dqkv.reshape(-1, 3 * d).contiguous()
        need = ctx.needs_input_grad
        # the scales sit in B_cat already: dxa = (dq B_q) s qs | (dv B_v) s; dB [3d, 256] = s dqkv^T (x A_cat^T)
        dx, dA, dB = _lora_bwd(g, x2, xa, w_qkv, A_cat, B_cat, 1.0, scale, 1.0, need[0], need[3] or need[5], need[4] or need[6])
        dAq = dAv = dBq = dBv = None
        if dA is not None:
            dAq, dAv = dA[:r].to(adt), dA[r:2 * r].to(adt)
        if dB is not None:
            dBq = (dB[:d, :r].float() * q_scale).to(bdt)
            dBv = dB[2 * d:, r:2 * r].contiguous().to(bdt)
        return None if dx is None else dx.view(xshape), None, None, dAq, dBq, dAv, dBv, None, None


def lora_qkv_supported(x, w_qkv, r):
    """The fused LoRA q | k | v node takes bf16 CUDA activations, both adapters in one 256-wide factor, and a shape whose base GEMM
    runs on the persistent kernel (anything else: the three projections one by one)."""
    M, K = x.numel() // x.shape[-1], x.shape[-1]
    return (x.is_cuda and x.dtype == torch.bfloat16 and w_qkv.dtype == torch.bfloat16 and 2 * r <= 256 and K % 8 == 0 and w_qkv.shape[0] % 24 == 0
            and lib().mmgl_gemm_nt_fast(M, w_qkv.shape[0], K, K, K, w_qkv.shape[0], _lib.BF16) == 1
            and lib().mmgl_gemm_nt_fast(M, w_qkv.shape[0] // 3, 256, 256, 256, w_qkv.shape[0], _lib.BF16) == 1)


def lora_qkv(x, w_qkv, b_qkv, lora_Aq, lora_Bq, lora_Av, lora_Bv, scale, q_scale):
    """[..., 3d] = (q * q_scale | k | v) with q = x W_q^T + b_q + scale (x A_q^T) B_q^T, v likewise, k = x W_k^T + b_k; w_qkv / b_qkv
    are the layer's frozen fused weight and bias with q_scale already folded into the q rows.  Check lora_qkv_supported first."""
    return _LoraQKV.apply(x, w_qkv, b_qkv, lora_Aq, lora_Bq, lora_Av, lora_Bv, float(scale), float(q_scale))


def lora_linear(x, weight, bias, lora_A, lora_B, scale, out_scale=1.0):
    """x W^T + b + scale * (x A^T) B^T with a frozen base weight (peft LoRA semantics, lora_dropout = 0).
    A frozen base product the persistent ping-pong GEMM takes (bf16, enough 256x256 tiles or K-split work items:
    mmgl_gemm_nt_fast == 1): _LoraLinearBig, the base product on that kernel with the low-rank update
    delta = (x A^T)(scale B)^T -- two skinny, HBM-bound GEMMs -- added in its epilogue; backward = the frozen dgrad GEMM plus
    the four skinny products autograd derives from the same pieces.  Everything else: one fused kernel (mmgl_lora_linear_*)
    that carries the rank-r term as a second operand pair in the same accumulators."""
    M = x.numel() // x.shape[-1]
    N, K = weight.shape
    if (not weight.requires_grad and (bias is None or not bias.requires_grad) and x.is_cuda
            and lib().mmgl_gemm_nt_fast(M, N, K, K, K, N, dtype_code(x)) == 1):
        # (fast == 1 implies bf16, K % 128 == 0 and N % 16 == 0: every condition _LoraLinearBig's GEMMs need)
        return _LoraLinearBig.apply(x, weight, bias, lora_A, lora_B, float(scale), float(out_scale))
    y = _LoraLinear.apply(x, weight, bias, lora_A, lora_B, float(scale))
    return y if out_scale == 1.0 else y * out_scale


# ------------------------------------------------------------------------------------------ neighbor interleave
class _Interleave(torch.autograd.Function):
    @staticmethod
    def forward(ctx, text_emb, vis_emb, text_loc, img_loc, text_pos, img_pos):
        require_cuda(text_emb)
        B, Nt, n_tok, d = text_emb.shape
        Ni = 0 if vis_emb is None else vis_emb.shape[1]
        text_emb = text_emb.contiguous()
        vis = None if vis_emb is None else vis_emb.contiguous()
        out = torch.empty(B, (Nt + Ni) * n_tok, d, dtype=text_emb.dtype, device=text_emb.device)
        valid = torch.empty(B, (Nt + Ni) * n_tok, dtype=torch.uint8, device=text_emb.device)
        tl, tp = text_loc.contiguous(), text_pos.contiguous()
        il = None if img_loc is None else img_loc.contiguous()
        ip = None if img_pos is None else img_pos.contiguous()
        _lib.call("mmgl_neighbor_interleave_fwd", None, ptr(text_emb), ptr(vis), ptr(tl), ptr(il), ptr(tp), ptr(ip), ptr(out),
                                                 ptr(valid), B, Nt, Ni, n_tok, d, dtype_code(text_emb), stream_ptr())
        ctx.save_for_backward(tl, il)
        ctx.dims = (B, Nt, Ni, n_tok, d)
        ctx.mark_non_differentiable(valid)
        return out, valid

    @staticmethod
    def backward(ctx, dout, _dvalid):
        tl, il = ctx.saved_tensors
        B, Nt, Ni, n_tok, d = ctx.dims
        dout = dout.contiguous()
        dtext = torch.empty(B, Nt, n_tok, d, dtype=dout.dtype, device=dout.device)
        dvis = torch.empty(B, Ni, n_tok, d, dtype=dout.dtype, device=dout.device) if Ni else None
        _lib.call("mmgl_neighbor_interleave_bwd", None, ptr(dout), ptr(tl), ptr(il), ptr(dtext), ptr(dvis), B, Nt, Ni, n_tok, d,
                                                 dtype_code(dout), stream_ptr())
        return dtext, dvis, None, None, None, None


def neighbor_interleave(text_emb, vis_emb, text_loc, img_loc, text_pos, img_pos):
    """Scatter [B,Nt,n,d] text and [B,Ni,n,d] image neighbor tokens into slot order; returns
    (neighbor_embeds [B,(Nt+Ni)*n,d], key_valid uint8 [B,(Nt+Ni)*n])   (reference :1080-1104)."""
    if vis_emb is not None and vis_emb.shape[2:] != text_emb.shape[2:]:
        raise ValueError("n_text_tokens must equal n_visual_tokens for the interleaved layout (reference :1083-1098)")
    return _Interleave.apply(text_emb, vis_emb, text_loc, img_loc, text_pos, img_pos)


# ------------------------------------------------------------------------------------------ cross entropy
class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        require_cuda(logits, labels)
        rows, V = logits.shape
        logits = logits.contiguous()
        labels = labels.contiguous()
        dev = logits.device
        row_lse = torch.empty(rows, dtype=torch.float32, device=dev)
        row_loss = torch.empty(rows, dtype=torch.float32, device=dev)
        sums = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.call("mmgl_cross_entropy_fwd", dict(bytes=1.0 * rows * V * logits.element_size()), ptr(logits), ptr(labels), ptr(row_lse), ptr(row_loss), ptr(sums[0:1]), ptr(sums[1:2]),
                                           rows, V, ignore_index, dtype_code(logits), stream_ptr())
        ctx.save_for_backward(logits, labels, row_lse, sums)
        ctx.ignore = ignore_index
        return sums[0] / sums[1]

    @staticmethod
    def backward(ctx, dloss):
        logits, labels, row_lse, sums = ctx.saved_tensors
        rows, V = logits.shape
        dl = dloss.detach().to(torch.float32).reshape(1).contiguous()
        dlogits = torch.empty_like(logits)
        _lib.call("mmgl_cross_entropy_bwd", dict(bytes=2.0 * rows * V * logits.element_size()), ptr(logits), ptr(labels), ptr(row_lse), ptr(sums[1:2]), ptr(dl), ptr(dlogits), rows, V,
                                           ctx.ignore, dtype_code(logits), stream_ptr())
        return dlogits, None, None


def cross_entropy(logits, labels, ignore_index=-100):
    """Mean token cross-entropy of [rows, V] logits (fp32 scalar), nn.CrossEntropyLoss semantics (reference :831-836)."""
    return _CrossEntropy.apply(logits, labels, int(ignore_index))


class _LMHeadCrossEntropy(torch.autograd.Function):
    """Token cross-entropy of lm_head(hidden) WITHOUT the [rows, V] logits / dlogits tensors (4.1 GB each at B=64): rows are
    processed in chunks through one scratch buffer -- logits chunk = GEMM, CE statistics, dlogits chunk in place, d hidden
    chunk = GEMM against the cached W^T -- all in the FORWARD pass for a unit upstream gradient; backward scales d hidden by
    the incoming scalar.  Same FLOPs as the unfused path (no recomputation).  The head is frozen (tied to the frozen
    embedding in every peft mode of the reference, :731-737)."""

    @staticmethod
    def forward(ctx, hidden, weight, labels, ignore_index, chunk_rows):
        require_cuda(hidden, weight, labels)
        V, d = weight.shape
        h2 = hidden.reshape(-1, d)
        if not h2.is_contiguous():
            h2 = h2.contiguous()
        M = h2.shape[0]
        lab = labels.reshape(-1).contiguous()
        dev = h2.device
        w = weight if weight.dtype == h2.dtype else weight.to(h2.dtype)
        count = (lab != ignore_index).sum().to(torch.float32).reshape(1)
        one = torch.ones(1, dtype=torch.float32, device=dev)
        loss_sum = torch.zeros(1, dtype=torch.float32, device=dev)
        dh = torch.empty_like(h2)
        chunk = min(M, int(chunk_rows))
        scratch = torch.empty(chunk, V, dtype=h2.dtype, device=dev)
        row_lse = torch.empty(chunk, dtype=torch.float32, device=dev)
        row_loss = torch.empty(chunk, dtype=torch.float32, device=dev)
        part = torch.empty(2, dtype=torch.float32, device=dev)
        code = dtype_code(h2)
        es = h2.element_size()
        for r0 in range(0, M, chunk):
            r1 = min(M, r0 + chunk)
            n = r1 - r0
            lg = scratch[:n]
            gemm_nt(h2[r0:r1], w.contiguous(), out=lg)
            _lib.call("mmgl_cross_entropy_fwd", dict(bytes=1.0 * n * V * es), ptr(lg), ptr(lab[r0:r1]), ptr(row_lse), ptr(row_loss), ptr(part[0:1]),
                      ptr(part[1:2]), n, V, ignore_index, code, stream_ptr())
            loss_sum += part[0:1]
            _lib.call("mmgl_cross_entropy_bwd", dict(bytes=2.0 * n * V * es), ptr(lg), ptr(lab[r0:r1]), ptr(row_lse), ptr(count), ptr(one), ptr(lg), n, V,
                      ignore_index, code, stream_ptr())
            frozen_dgrad(lg, weight, out=dh[r0:r1])
        ctx.save_for_backward(dh)
        ctx.shape = hidden.shape
        return (loss_sum / count.clamp_min(1.0)).reshape(())

    @staticmethod
    def backward(ctx, dloss):
        (dh,) = ctx.saved_tensors
        # scale in fp32 by the device scalar (mmgl_scale: one pass, no host sync): 1 / grad_accumulation_steps rounded to bf16
        # first would bias every hidden gradient by up to 0.4 %
        s = dloss.detach().to(torch.float32).reshape(1).contiguous()
        out = torch.empty_like(dh)
        _lib.call("mmgl_scale", dict(bytes=2.0 * dh.numel() * dh.element_size()), ptr(dh), ptr(s), ptr(out), dh.numel(), dtype_code(dh),
                  stream_ptr())
        return out.view(ctx.shape), None, None, None, None


def lm_head_cross_entropy(hidden, weight, labels, ignore_index=-100, chunk_rows=8192):
    """Mean token cross-entropy of `hidden @ weight.T` against `labels` (nn.CrossEntropyLoss semantics) with a FROZEN head,
    never materialising the logits (reference :826-836 builds [B, T, V] logits, the shifted copy and their gradients).
    hidden [..., d], weight [V, d], labels [...] int64 (already shifted).  fp32 scalar."""
    if weight.requires_grad:
        raise ValueError("lm_head_cross_entropy: the head must be frozen (use lm_head + cross_entropy for a trainable head)")
    if hidden.shape[:-1] != labels.shape or hidden.shape[-1] != weight.shape[1]:
        raise ValueError(f"lm_head_cross_entropy: shapes hidden{tuple(hidden.shape)} weight{tuple(weight.shape)} labels{tuple(labels.shape)}")
    return _LMHeadCrossEntropy.apply(hidden, weight, labels, int(ignore_index), int(chunk_rows))


def position_ids(attention_mask):
    """cumsum(mask) * mask - 1 + 2  (reference MPTLearnedPositionalEmbedding :135-145)."""
    require_cuda(attention_mask)
    m = attention_mask.to(torch.int64).contiguous()
    out = torch.empty_like(m)
    _lib.call("mmgl_position_ids", None, ptr(m), ptr(out), m.shape[0], m.shape[1], stream_ptr())
    return out


def adamw_step_(param, master, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    """In-place fused AdamW over flat buffers (torch.optim.AdamW formula)."""
    require_cuda(param, grad)
    _lib.call("mmgl_adamw_step", None, ptr(param), ptr(master), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), lr, beta1, beta2,
                                eps, weight_decay, step, grad_scale, dtype_code(param), stream_ptr())


class AdafactorTable:
    """The segment table of mmgl_adafactor_step, planned and validated once on the host (mmgl_adafactor_workspace; no GPU needed for
    that): per tensor its offset in the flat buffers, R, C (0 for a 1-D tensor of R elements) and its offset in the flat fp32 state
    (row[R] | col[C], or v[R]).  `segments` gives (flat offset, shape) per tensor, in ascending offsets that are multiples of 128;
    state segments start on 32-float boundaries.  `.state_offsets[i]`, `.state_numel`, `.workspace_bytes` describe the layout; the
    device copy of the table and the workspace are made by `.to(device)` (the engine calls it in its constructor, never in a step)."""

    def __init__(self, segments):
        import ctypes
        self.shapes, self.offsets, self.state_offsets = [], [], []
        rows, st = [], 0
        for off, shape in segments:
            shape = tuple(int(s) for s in shape)
            if not 1 <= len(shape) <= 2:
                raise ValueError(f"fused Adafactor takes 1-D and 2-D tensors, got shape {shape}: transformers factors a tensor of more "
                                 "dimensions over its last two with the leading ones as a batch, which this kernel does not do")
            R, C = (shape[0], 0) if len(shape) == 1 else shape
            if C == 0 and len(shape) == 2 or R == 0:
                raise ValueError(f"fused Adafactor: empty tensor of shape {shape}")
            self.shapes.append(shape), self.offsets.append(int(off)), self.state_offsets.append(st)
            rows += [int(off), R, C, st]
            st += (R + C + 31) // 32 * 32
        self.n, self.state_numel = len(self.shapes), st
        if not self.n:
            raise ValueError("fused Adafactor: no tensors")
        segs = (ctypes.c_int64 * len(rows))(*rows)
        self.host = (ctypes.c_int64 * (8 * (self.n + 1)))()
        self.workspace_bytes = lib().mmgl_adafactor_workspace(segs, self.n, self.host)
        if not self.workspace_bytes:
            raise ValueError(lib().mmgl_last_error().decode("utf-8", "replace"))
        self.n_tiles, self.n_folds = int(self.host[8 * self.n + 4]), int(self.host[8 * self.n + 5])
        self.device = self.workspace = None

    def to(self, device):
        self.device = torch.tensor(list(self.host), dtype=torch.int64).to(device)
        self.workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=device)
        return self


def adafactor_step_(param, master, grad, state, table, lr, step, grad_scale=1.0, weight_decay=0.0, eps1=1e-30, clip_threshold=1.0,
                    decay_rate=-0.8):
    """In-place fused Adafactor over flat buffers (transformers' Adafactor.step with beta1 None, no relative step, no parameter
    scaling): one C-ABI call, four launches, for every tensor of `table` (an AdafactorTable moved to the device)."""
    require_cuda(param, grad, state, table.device, table.workspace)
    if grad.dtype != param.dtype or state.dtype != torch.float32 or (master is not None and master.dtype != torch.float32):
        raise ValueError("adafactor_step_: grad in the parameter's dtype, state and master in float32")
    _lib.call("mmgl_adafactor_step", None, ptr(param), ptr(master), ptr(grad), ptr(state), ptr(table.device), table.host, table.n,
              ptr(table.workspace), table.workspace_bytes, lr, eps1, clip_threshold, decay_rate, weight_decay, step, grad_scale,
              dtype_code(param), stream_ptr())


# ------------------------------------------------------------------------------------------ frozen linears
# The frozen decoder layers, lm_head and the encoders only ever need y = act(x W^T + b) and dx = dy W.  Both run on
# mmgl_gemm_nt (the persistent ping-pong MFMA kernel of csrc/gemm8p.hip for large bf16 shapes): forward with the bias /
# activation epilogue, dgrad as an NT GEMM against a cached W^T copy (the weights never change), and fc1's ReLU backward
# folded into the epilogue of fc2's dgrad (zmask) -- no clamp pass, no pre-activation kept, no library GEMM.
_WT_CACHE = {}
ACT_CODES = {"none": 0, "relu": 1, "gelu": 2, "quick_gelu": 3, "gelu_new": 4, "gelu_pytorch_tanh": 4, "gelu_fast": 4}


def _padded_t(weight, pad_to=1):
    """W^T as a contiguous tensor [in, out_padded] (out zero-padded up to a multiple of `pad_to`)."""
    with torch.no_grad():
        wt = weight.detach().t()
        n = wt.shape[1]
        npad = (n + pad_to - 1) // pad_to * pad_to
        if npad == n:
            return wt.contiguous()
        full = wt.new_zeros(wt.shape[0], npad)
        full[:, :n] = wt
        return full


def _transposed(weight, pad_to=1):
    """_padded_t(weight, pad_to) cached per weight OBJECT (weakref-checked: an id or an address can be reused by a later tensor)
    and rebuilt when its storage / version / dtype changes (load_state_dict, .bfloat16(), flattening)."""
    key = (id(weight), pad_to)
    tag = (weight.data_ptr(), weight._version, weight.dtype, tuple(weight.shape))
    hit = _WT_CACHE.get(key)
    if hit is None or hit[0]() is not weight or hit[1] != tag:
        if len(_WT_CACHE) > 4096:                             # drop entries of dead tensors
            for k in [k for k, h in _WT_CACHE.items() if h[0]() is None]:
                del _WT_CACHE[k]
        hit = (weakref.ref(weight), tag, _padded_t(weight, pad_to))
        _WT_CACHE[key] = hit
    return hit[2]


_tile_counters = {}


def gemm_dynamic_schedule(enable=True, device=None):
    """Switch this process's persistent-GEMM launches between the static tile schedule (default) and the dynamic one
    (mmgl_gemm_set_tile_counter): workgroups take tiles from per-XCD counters as they become free.  The data-parallel engine
    turns it on when it runs with more than one rank: the bucket all-reduces of the backward pass share the CUs with these GEMMs,
    and a statically scheduled GEMM waits for its displaced workgroups (reference DDP overlap: run_generation.py:317-319, 485).
    One counter block per device, process-wide (the backward GEMMs are launched from autograd's device thread); every launch leaves it
    zeroed, GEMMs of one device run on one stream."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(device):                          # the C side keys the setting by hipGetDevice
        if not enable:
            lib().mmgl_gemm_set_tile_counter(None)
            return None
        c = _tile_counters.get(device)
        if c is None:
            c = _tile_counters[device] = torch.zeros(16, dtype=torch.int32, device=device)
        lib().mmgl_gemm_set_tile_counter(ptr(c))
    return c


def gemm_nt(x2, w, bias=None, residual=None, zmask=None, act=0, out_scale=1.0, K=None, out=None, k_splits=True):
    """Raw mmgl_gemm_nt call: act((x2[:, :K] @ w[:, :K]^T + bias) * out_scale) [zeroed where zmask <= 0] [+ residual].
    x2 [M, >=K] and w [N, >=K] are row-major with unit column stride (their row strides are passed as ldx / ldw: K may exceed
    x2's row length when the matching columns of w are zero padding).  k_splits=False brings no K-split scratch: every output element
    is then one sum over K in tile order, whatever M is (a partial round of tiles is not cut along K).  No autograd."""
    require_cuda(x2, w)
    M, N = x2.shape[0], w.shape[0]
    K = x2.shape[1] if K is None else K
    if x2.stride(1) != 1 or w.stride(1) != 1:
        raise ValueError("gemm_nt: operands need unit column stride")
    y = torch.empty(M, N, dtype=x2.dtype, device=x2.device) if out is None else out
    if M == 0:
        return y
    for name, t in (("zmask", zmask), ("residual", residual)):
        if t is not None and (t.stride(1) != 1 or t.stride(0) != y.stride(0)):
            raise ValueError(f"gemm_nt: {name} must share the output's row stride ({t.stride(0)} vs {y.stride(0)})")
    nws = lib().mmgl_gemm_nt_workspace(M, N, K, x2.stride(0), w.stride(0), y.stride(0), dtype_code(x2)) if k_splits else 0
    ws = torch.empty(nws, dtype=torch.uint8, device=x2.device) if nws else None       # K-split partial tiles (few-tile shapes)
    _lib.call("mmgl_gemm_nt", dict(flops=2.0 * M * N * K, bytes=float(M * K + N * K + M * N) * x2.element_size(),
                                   tag=f"{M}x{N}x{K}" + ("+b" if bias is not None else "") + ("+z" if zmask is not None else "")
                                       + ("+r" if residual is not None else "") + (f"+a{act}" if act else "")),
              ptr(x2), x2.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(residual), ptr(zmask), ptr(y), y.stride(0), M, N, K, act,
              float(out_scale), ptr(ws), nws, dtype_code(x2), stream_ptr())
    return y


def relu_bits_bytes(M, N, K, ldx, ldw, ldy, dtype):
    """Bytes of the ReLU mask bits of an [M, N] = relu(x W^T) output (0: that shape does not run as whole tiles of the persistent
    kernel, or the dtype is not bf16 -> keep the activation as the mask)."""
    if dtype != torch.bfloat16:
        return 0
    return lib().mmgl_gemm_nt_relu_bits_bytes(M, N, K, ldx, ldw, ldy, _lib.BF16)


def gemm_nt_relu_bits(x2, w, bias, out, K=None):
    """out = relu(x2[:, :K] @ w^T + bias) plus one bit per element (out > 0), lane-private to the persistent GEMM's tiling:
    (out, bits uint8 [nbytes]).  Callers check relu_bits_bytes() > 0 first.  No autograd."""
    M, N = x2.shape[0], w.shape[0]
    K = x2.shape[1] if K is None else K
    nb = relu_bits_bytes(M, N, K, x2.stride(0), w.stride(0), out.stride(0), x2.dtype)
    if not nb:
        raise ValueError("gemm_nt_relu_bits: shape not eligible (relu_bits_bytes == 0)")
    bits = torch.empty(nb, dtype=torch.uint8, device=x2.device)
    _lib.call("mmgl_gemm_nt_relu_bits", dict(flops=2.0 * M * N * K, bytes=float(M * K + N * K + M * N) * x2.element_size(), tag=f"{M}x{N}x{K}+b+a1+bits"),
              ptr(x2), x2.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(out), out.stride(0), ptr(bits), M, N, K, 1.0, dtype_code(x2), stream_ptr())
    return out, bits


def gemm_nt_masked(x2, w, bits, out, K=None):
    """out = (x2[:, :K] @ w^T) where the element's bit is set, 0 elsewhere (bits from gemm_nt_relu_bits of the same [M, N]).  No autograd."""
    M, N = x2.shape[0], w.shape[0]
    K = x2.shape[1] if K is None else K
    _lib.call("mmgl_gemm_nt_masked", dict(flops=2.0 * M * N * K, bytes=float(M * K + N * K + M * N) * x2.element_size(), tag=f"{M}x{N}x{K}+bits"),
              ptr(x2), x2.stride(0), ptr(w), w.stride(0), ptr(bits), ptr(out), out.stride(0), M, N, K, 1.0, dtype_code(x2), stream_ptr())
    return out


def _dgrad_pad_to(g, weight):
    """pad_to of the W^T operand of dx = g W (see _padded_t): 128 when the contraction N = weight.shape[0] is no multiple of 128
    (lm_head: N = vocab = 50272) and the persistent kernel takes dx against W^T zero-padded to that multiple, g read with its own
    row stride (its row tails meet the zero columns); else 1, dense operands."""
    N, K = weight.shape
    if N % 128 == 0 or not (g.dtype == weight.dtype == torch.bfloat16):
        return 1
    npad = N + (-N) % 128
    return 128 if lib().mmgl_gemm_nt_fast(g.shape[0], K, npad, g.stride(0), npad, K, _lib.BF16) else 1


def frozen_dgrad(g, weight, zmask=None, out=None, bits=None, out_scale=1.0, residual=None, wt=None):
    """dx[M,K] = g[M,N] @ W[N,K] for a frozen W  ==  an NT GEMM against W^T: the cached copy (zero-padded along N where
    _dgrad_pad_to says so) unless the caller brings its own `wt`.  With the ReLU mask as bits (gemm_nt_masked: `out` carries their
    row pitch), else through gemm_nt with its zmask / residual / out_scale epilogue.  No autograd."""
    if wt is None:
        if weight.dtype == g.dtype:
            wt = _transposed(weight, _dgrad_pad_to(g, weight))
        else:
            wt = weight.detach().to(g.dtype).t().contiguous()
    if out is None:
        # zmask (a ReLU output kept with a padded row pitch, see _ffn_pitch) shares the output's row stride in the epilogue
        K = wt.shape[0]
        ld = K if zmask is None else zmask.stride(0)
        out = g.new_empty(g.shape[0], ld)
        out = out[:, :K] if ld != K else out
    if bits is not None:
        return gemm_nt_masked(g, wt, bits, out, K=wt.shape[1])
    return _mfma_aligned(gemm_nt, g, wt, residual=residual, zmask=zmask, out_scale=out_scale, out=out)


def _ffn_pitch(M, N, K, dtype):
    """Row pitch (elements) for the [M, N] hidden buffer between the two linears of a frozen FFN.  A power-of-two row size
    (8192 bf16 = 16 KiB) costs the persistent GEMM ~3 % at that shape (1049 vs 1015 us, tools/probes/gemm_pitch2.py): the buffer
    and its gradient get 128 extra columns of pitch when all four GEMMs that touch them take strided operands (fast path)."""
    if dtype != torch.bfloat16 or (N * 2) % 8192:
        return N
    P, L = N + 128, lib()
    if L.mmgl_gemm_nt_fast(M, N, K, K, K, P, _lib.BF16) == 1 and L.mmgl_gemm_nt_fast(M, K, N, P, N, K, _lib.BF16) == 1:
        return P
    return N


_CU_COUNT = {}


def _round_split_rows(M, N, device):
    """Rows [0, m1) of an [M, N] GEMM output that fill whole rounds of the persistent kernel's 256 x 256 tiles, when the rest is a
    short tail: at the reference's batch (M = 4 * 640 = 2560, reference language_modelling/run_generation.py:124-126) the FFN's
    [2560, 8192] output is 320 tiles on 256 CUs -- a second round at a quarter of the chip (102.6 us); 2048 rows on the persistent
    kernel + 512 rows on the few-tile kernel take 78.3 us (tools/probes/gemm_msplit.py).  0 = do not split."""
    G = _CU_COUNT.get(device.index)
    if G is None:
        G = _CU_COUNT[device.index] = torch.cuda.get_device_properties(device).multi_processor_count
    tm, tn = (M + 255) // 256, (N + 255) // 256
    rounds, rem = divmod(tm * tn, G)
    if not (1 <= rounds <= 3 and 0 < rem <= G // 4) or (rounds * G) % tn:
        return 0
    m1 = rounds * G // tn * 256
    return m1 if 0 < m1 < M else 0


def _row_strided(t2, cols, n_out):
    """t2 [M, cols] as a GEMM operand: itself when it is row-major with unit column stride and a row pitch the fast path
    takes, else a contiguous copy."""
    if t2.is_contiguous():
        return t2
    if (t2.stride(1) == 1 and t2.stride(0) >= cols and t2.stride(0) % 8 == 0 and t2.dtype == torch.bfloat16
            and lib().mmgl_gemm_nt_fast(t2.shape[0], n_out, cols, t2.stride(0), cols, n_out, _lib.BF16)):
        return t2
    return t2.contiguous()


class _FrozenLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act):
        N, K = weight.shape
        x2 = _row_strided(x.reshape(-1, K), K, N)
        # the output is allocated here, in its final shape, and returned as is: consumers such as the in-place rotary embedding may
        # then modify it (a tensor the caller passed in would come back as a view of an input)
        out = torch.empty(*x.shape[:-1], N, dtype=x.dtype, device=x.device)
        _mfma_aligned(gemm_nt, x2, weight.to(x.dtype).contiguous(), None if bias is None else bias.to(x.dtype), act=act, out=out.view(-1, N))
        ctx.save_for_backward(weight, out if act == 1 else None)
        return out

    @staticmethod
    def backward(ctx, dy):
        weight, y = ctx.saved_tensors
        N, K = weight.shape
        g = dy.reshape(-1, N)
        g = _row_strided(g, N, K) if y is None else g.contiguous()
        if y is not None:                                     # a stand-alone act="relu": its own pass over the gradient
            gm = torch.empty_like(g)
            _lib.call("mmgl_relu_bwd", dict(bytes=3.0 * g.numel() * g.element_size()), ptr(g), ptr(y), ptr(gm), g.numel(), dtype_code(g), stream_ptr())
            g = gm
        return frozen_dgrad(g, weight).reshape(*dy.shape[:-1], K), None, None, None


def frozen_linear(x, weight, bias, act="none"):
    """act(x W^T + b) for a FROZEN nn.Linear (reference :194-199, :273 inside the frozen LM layers, lm_head :826), act "none" |
    "relu".  The fc1 + ReLU / fc2 pair of a frozen layer (:352-355) is relu_ffn's."""
    if weight.requires_grad or (bias is not None and bias.requires_grad):
        raise ValueError("frozen_linear: weight and bias must be frozen (requires_grad=False)")
    if x.shape[-1] != weight.shape[1]:
        raise ValueError(f"frozen_linear: x has {x.shape[-1]} features, weight expects {weight.shape[1]}")
    return _FrozenLinear.apply(x, weight, bias, _act_code("frozen_linear", act))


class _FrozenReluFFN(torch.autograd.Function):
    """y = fc2(relu(fc1(x))), w1 [ffn, d_in] and w2 [d_out, ffn] frozen, as one node that owns the hidden buffer h [M, ffn] and the plan
    of its ReLU mask: fc1's ReLU backward rides in the epilogue of fc2's dgrad GEMM -- no pass over [M, ffn] -- and where the shapes
    allow it the mask leaves fc1 as bits (16 bytes per lane and tile), so that h is not kept for backward."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        (F_, K), N = w1.shape, w2.shape[0]
        x2 = x.contiguous().reshape(-1, K)                    # the plan reads x's rows densely
        M = x2.shape[0]
        # h's row pitch and the rows whose mask leaves as bits: whole rounds of the persistent kernel when the rest is a short tail
        # (it runs on the few-tile kernel, its activation rows stay the mask), else all rows where the shape runs as whole tiles
        pitch = _ffn_pitch(M, F_, K, x.dtype)
        rows = nb = 0
        if pitch != F_:
            rows = _round_split_rows(M, F_, x.device)
            nb = relu_bits_bytes(rows, F_, K, K, K, pitch, x.dtype) if rows else 0
            if not nb:
                rows, nb = M, relu_bits_bytes(M, F_, K, K, K, pitch, x.dtype)
        w, b = w1.to(x.dtype).contiguous(), None if b1 is None else b1.to(x.dtype)
        h = x.new_empty(M, pitch)[:, :F_]
        if nb:
            _, bits = gemm_nt_relu_bits(x2[:rows], w, b, h[:rows])
            if rows < M:
                gemm_nt(x2[rows:], w, b, act=1, out=h[rows:])
        else:
            _mfma_aligned(gemm_nt, x2, w, b, act=1, out=h)
        hx = _row_strided(h, F_, N)                           # fc2 reads h with its row pitch
        y = x.new_empty(*x.shape[:-1], N)
        _mfma_aligned(gemm_nt, hx, w2.to(x.dtype).contiguous(), None if b2 is None else b2.to(x.dtype), out=y.view(-1, N))
        # kept for fc2's dgrad: nothing when the bits cover every row and the dgrad's shape takes them, the tail rows when they cover
        # some -- copied (a view would keep the [M, ffn] buffer) with the row pitch the dgrad's output has -- else the activation
        mask, ctx.mask_bits = hx, None
        if nb and hx.stride(0) == pitch and N % 128 == 0 and relu_bits_bytes(rows, F_, N, N, N, pitch, x.dtype) == nb:
            mask, ctx.mask_bits = None, (bits, pitch, rows)
            if rows < M:
                mask = x.new_empty(M - rows, pitch)[:, :F_].copy_(hx[rows:])
        ctx.save_for_backward(w1, w2, mask)
        h = h.view(*x.shape[:-1], F_)
        ctx.mark_non_differentiable(h)
        ctx.set_materialize_grads(False)                      # no zero tensor [M, ffn] for h's gradient
        return y, h

    @staticmethod
    def backward(ctx, dy, _dh=None):
        w1, w2, mask = ctx.saved_tensors
        (F_, K), N = w1.shape, w2.shape[0]
        g = _row_strided(dy.reshape(-1, N), N, F_)
        if ctx.mask_bits is None:
            dh = frozen_dgrad(g, w2, zmask=mask)
        else:
            bits, pitch, rows = ctx.mask_bits
            dh = g.new_empty(g.shape[0], pitch)[:, :F_]
            frozen_dgrad(g[:rows], w2, out=dh[:rows], bits=bits)
            if rows < g.shape[0]:                             # the tail rows with their activation rows as the mask
                frozen_dgrad(g[rows:], w2, zmask=mask, out=dh[rows:])
        return frozen_dgrad(_row_strided(dh, F_, K), w1).reshape(*dy.shape[:-1], K), None, None, None, None


def relu_ffn(x, w1, b1, w2, b2, frozen=None, return_hidden=False):
    """fc2(relu(fc1(x))) (reference :352-355): w1 [ffn, d_in], w2 [d_out, ffn] in nn.Linear layout, biases optional; fc1's ReLU backward
    is folded into fc2's dgrad GEMM.  frozen=None takes the frozen route (_FrozenReluFFN: dgrads only, cached W^T) exactly when none
    of the four parameters requires grad, frozen=False forces the trainable one (two _Linear nodes).  return_hidden: (y, h) with
    h = relu(fc1(x)), which carries a gradient on the trainable route only (the frozen node hands it out non-differentiable)."""
    if x.shape[-1] != w1.shape[1] or w1.shape[0] != w2.shape[1]:
        raise ValueError(f"relu_ffn: x has {x.shape[-1]} features, fc1 maps {w1.shape[1]} to {w1.shape[0]}, fc2 expects {w2.shape[1]}")
    trainable = any(p is not None and p.requires_grad for p in (w1, b1, w2, b2))
    if frozen and trainable:
        raise ValueError("relu_ffn: weight and bias must be frozen (requires_grad=False)")
    if trainable or frozen is False:
        h = _linear(x, w1, b1, _lib.ACT_RELU, premasked=True)
        y = _linear(h, w2, b2, _lib.ACT_NONE, mask_dx=True)
    else:
        y, h = _FrozenReluFFN.apply(x, w1, b1, w2, b2)
    return (y, h) if return_hidden else y


# ------------------------------------------------------------------------------------------ Llama-family elementwise ops
class _RopeQK(torch.autograd.Function):
    """Rotary embedding of the q and k blocks of a fused-QKV buffer [B, T, 3*H*D], in place (the buffer is a fresh GEMM output).
    The kernel sees the row as `nall` column blocks of `unit` heads each and rotates the first `nblk`: (H, 2, 3) for multi-head,
    (Hkv, G + 1, G + 2) for a grouped-query row [q: G blocks | k | v]."""

    @staticmethod
    def forward(ctx, qkv, cos_sin, unit, nblk, nall):
        require_cuda(qkv, cos_sin)
        B, T, ld = qkv.shape
        D = ld // nall // unit
        if not qkv.is_contiguous():
            raise ValueError("rope_qk_: qkv must be contiguous")
        _lib.call("mmgl_rope_inplace", dict(bytes=2.0 * B * T * (nblk * ld // nall) * qkv.element_size()), ptr(qkv), ptr(cos_sin), B * T, T, unit, D, ld, nblk, 0,
                  dtype_code(qkv), stream_ptr())
        ctx.mark_dirty(qkv)
        ctx.save_for_backward(cos_sin)
        ctx.meta = (T, unit, D, nblk, nall)
        return qkv

    @staticmethod
    def backward(ctx, dqkv):
        (cos_sin,) = ctx.saved_tensors
        T, H, D, nblk, nall = ctx.meta
        dqkv = dqkv.contiguous()                                         # autograd owns the incoming buffer: rotate INTO a new one, never in place
        out = torch.empty_like(dqkv)
        rows = dqkv.numel() // dqkv.shape[-1]
        _lib.call("mmgl_rope", dict(bytes=2.0 * rows * dqkv.shape[-1] * dqkv.element_size()), ptr(dqkv), ptr(out), ptr(cos_sin), rows, T, H, D,
                  dqkv.shape[-1], nblk, nall, 1, dtype_code(dqkv), stream_ptr())
        return out, None, None, None, None


def rope_qk_(qkv, cos_sin, num_heads, num_kv_heads=None):
    """In-place rotary position embedding of the q and k thirds of qkv [B, T, 3*H*D] (transformers' rotate_half convention,
    position = index along T).  cos_sin: fp32 [T, D/2, 2].  Grouped-query attention (num_kv_heads = Hkv < H): qkv
    [B, T, (H+2*Hkv)*D]; the H q heads and the Hkv k heads are rotated, the v block is left alone."""
    Hkv = _kv_heads("rope_qk_", num_heads, num_kv_heads)
    if Hkv is not None:
        if qkv.dim() != 3 or qkv.shape[2] % (num_heads + 2 * Hkv):
            raise ValueError(f"rope_qk_: qkv{tuple(qkv.shape)} is not [B, T, (H+2*Hkv)*D] for H={num_heads}, Hkv={Hkv}")
        D, G = qkv.shape[2] // (num_heads + 2 * Hkv), num_heads // Hkv
        unit, nblk, nall = Hkv, G + 1, G + 2
    else:
        if qkv.dim() != 3 or qkv.shape[2] % (3 * num_heads):
            raise ValueError(f"rope_qk_: qkv{tuple(qkv.shape)} is not [B, T, 3*H*D] for H={num_heads}")
        D = qkv.shape[2] // 3 // num_heads
        unit, nblk, nall = num_heads, 2, 3
    if cos_sin.dtype != torch.float32 or tuple(cos_sin.shape) != (qkv.shape[1], D // 2, 2):
        raise ValueError(f"rope_qk_: cos_sin must be fp32 [T={qkv.shape[1]}, D/2={D // 2}, 2], got {cos_sin.dtype} {tuple(cos_sin.shape)}")
    return _RopeQK.apply(qkv, cos_sin.contiguous(), unit, nblk, nall)


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        require_cuda(gu)
        F2 = gu.shape[-1]
        g2 = gu.contiguous().view(-1, F2)
        y = torch.empty(g2.shape[0], F2 // 2, dtype=gu.dtype, device=gu.device)
        _lib.call("mmgl_swiglu_fwd", dict(bytes=1.5 * g2.numel() * g2.element_size()), ptr(g2), ptr(y), g2.shape[0], F2 // 2, dtype_code(g2), stream_ptr())
        ctx.save_for_backward(g2)
        ctx.shape = gu.shape
        return y.view(*gu.shape[:-1], F2 // 2)

    @staticmethod
    def backward(ctx, dy):
        (g2,) = ctx.saved_tensors
        M, F2 = g2.shape
        dy2 = dy.contiguous().view(M, F2 // 2)
        dgu = torch.empty_like(g2)
        _lib.call("mmgl_swiglu_bwd", dict(bytes=2.5 * g2.numel() * g2.element_size()), ptr(dy2), ptr(g2), ptr(dgu), M, F2 // 2, dtype_code(g2), stream_ptr())
        return dgu.view(ctx.shape)


def swiglu(gate_up):
    """silu(gate_up[..., :F]) * gate_up[..., F:] over one fused [gate | up] projection output (LlamaMLP)."""
    if gate_up.shape[-1] % 2:
        raise ValueError("swiglu: last dim must be 2*F")
    return _SwiGLU.apply(gate_up)


# ------------------------------------------------------------------------------------------ frozen encoders (forward only)
def encoder_attention(q, k, v, cu_seqlens, num_heads, max_len, q_rows=None, work=None):
    """Bidirectional attention over packed sequences (no padding rows exist).  q, k, v: [ntok, H*D] views with a common
    row stride (e.g. the three column slices of a fused-QKV output); q pre-scaled by D^-1/2; cu_seqlens int32 [nseq+1].
    Returns [ntok, H*D]; with q_rows < max_len only the first q_rows rows of every sequence are written.
    No autograd: the encoders are frozen (reference modelling_cross_attention.py:922-934)."""
    require_cuda(q, k, v, cu_seqlens)
    ntok, hd = q.shape
    if k.shape != q.shape or v.shape != q.shape or hd % num_heads:
        raise ValueError(f"encoder_attention: incompatible shapes q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)} H={num_heads}")
    ld = q.stride(0)
    if q.stride(1) != 1 or k.stride() != q.stride() or v.stride() != q.stride():
        raise ValueError("encoder_attention: q, k, v need unit column stride and one common row stride")
    if cu_seqlens.dtype != torch.int32:
        raise ValueError("encoder_attention: cu_seqlens must be int32")
    out = torch.empty(ntok, hd, dtype=q.dtype, device=q.device)
    nseq = cu_seqlens.numel() - 1
    if nseq <= 0 or ntok == 0:
        return out
    _lib.call("mmgl_encattn_fwd", work, ptr(q), ptr(k), ptr(v), ptr(cu_seqlens), ptr(out), nseq, num_heads, hd // num_heads, ld, hd,
              int(max_len), int(max_len if q_rows is None else q_rows), dtype_code(q), stream_ptr())
    return out


def add_layer_norm(x, res, gamma, beta, eps, return_sum=False):
    """y = LayerNorm(x + res) in one pass (optionally also returning the sum = the new residual stream).  Forward only."""
    require_cuda(x, res)
    if x.shape != res.shape:
        raise ValueError(f"add_layer_norm: shapes differ {tuple(x.shape)} vs {tuple(res.shape)}")
    if x.shape[-1] and not x.numel():                      # no rows: nothing to launch
        return (torch.empty_like(x), torch.empty_like(x)) if return_sum else torch.empty_like(x)
    s, y, _, _, _ = _norm_fwd(False, x, res, gamma, beta, float(eps), keep_sum=return_sum, keep_stats=False)
    return (s.view(x.shape), y.view(x.shape)) if return_sum else y.view(x.shape)


def activation_(x, name):
    """In-place HF ACT2FN[name] over a contiguous tensor (one pass).  Forward only."""
    require_cuda(x)
    if name not in ACT_CODES:
        raise ValueError(f"activation_: unsupported activation {name!r}")
    if not x.is_contiguous():
        raise ValueError("activation_: tensor must be contiguous")
    _lib.call("mmgl_activation_fwd", dict(bytes=2.0 * x.numel() * x.element_size()), ptr(x), ptr(x), x.numel(), ACT_CODES[name], dtype_code(x), stream_ptr())
    return x


# ------------------------------------------------------------------------------------------ decode step (generate())
def _no_grad_inputs(op, *ts):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise ValueError(f"{op} is forward only (the decode step of generate()): run it under torch.no_grad() or detach its inputs")


def _as_uint8(mask):
    """A bool mask viewed as uint8 (no launch, unlike _key_valid); any other dtype passes through."""
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _decode_gemm_operands(op, x, weight, bias, out):
    """The operands of a decode GEMM x [M, K] x weight [N, K]^T as the skinny kernels take them: x and weight with unit column stride,
    bias in x's dtype, and y -- `out` [M, N] (any row stride) checked, or a new dense tensor."""
    M, N = x.shape[0], weight.shape[0]
    if x.stride(1) != 1:
        x = x.contiguous()
    weight = weight if weight.stride(1) == 1 else weight.contiguous()
    y = torch.empty(M, N, dtype=x.dtype, device=x.device) if out is None else out
    if tuple(y.shape) != (M, N) or y.stride(1) != 1 or y.dtype != x.dtype or weight.dtype != x.dtype:
        raise ValueError(f"{op}: out{tuple(y.shape)} {y.dtype} for x{tuple(x.shape)} {x.dtype} weight{tuple(weight.shape)} {weight.dtype}")
    if bias is not None and bias.dtype != x.dtype:
        bias = bias.to(x.dtype)
    return x, weight, bias, y


def _row_chunks(M):
    """The rows of a decode GEMM as slices of at most 64: what one mmgl_gemm_skinny / mmgl_gemm_skinny_lora call takes."""
    return [slice(m0, min(M, m0 + 64)) for m0 in range(0, M, 64)]


_SKINNY_MAX_N = 32768


def _skinny_route(M, N, K, dtype):
    """Whether mmgl_gemm_skinny takes a dense [M <= 64, K] x [N, K]^T linear of a decode step rather than mmgl_gemm_nt: the table of
    profiles/decode_gemm_skinny.txt (tools/bench_gemm_skinny.py, the two entry points alternating in one process, cold weights).  The
    skinny kernel is 1.4-7x faster on every layer shape (N <= 8192, K = 768 / 2048 / 8192) at M = 2, 16 and 64; on the lm_head shape
    (N = 50272, K = 2048: 3142 workgroups that each re-stage x) mmgl_gemm_nt ties at M = 2 and wins at M = 16 (1.13x) and 64 (1.6x).
    The boundary sits between the two measured widths; fp32 has one route (the plain skinny kernel takes any stride)."""
    return dtype != torch.bfloat16 or N < _SKINNY_MAX_N


def gemm_skinny(x, weight, bias=None, residual=None, act=0, out_scale=1.0, out=None):
    """Raw mmgl_gemm_skinny call: x [M <= 64, K], weight [N, K], out [M, N]; row strides are free, column strides 1.  No autograd."""
    require_cuda(x, weight)
    M, K = x.shape
    N = weight.shape[0]
    y = torch.empty(M, N, dtype=x.dtype, device=x.device) if out is None else out
    _lib.call("mmgl_gemm_skinny", dict(flops=2.0 * M * N * K, bytes=float(M * K + N * K + M * N) * x.element_size(), tag=f"{M}x{N}x{K}"),
              ptr(x), x.stride(0), ptr(weight), weight.stride(0), ptr(bias), ptr(residual), ptr(y), y.stride(0), M, N, K, act,
              float(out_scale), dtype_code(x), stream_ptr())
    return y


def decode_linear(x, weight, bias=None, act="none", out_scale=1.0, residual=None, out=None):
    """act((x @ weight^T + bias) * out_scale) + residual for the few rows of a decode step: x [M, K] (M = batch rows), weight [N, K].
    `out` [M, N] may be a strided view with unit column stride -- a column of the key/value cache -- and `residual` shares its row
    stride.  Rows go to mmgl_gemm_skinny in chunks of 64; a dense bf16 call of a shape where mmgl_gemm_nt measured faster (_skinny_route:
    the lm_head width) goes there.
    Forward only; GPU only."""
    require_cuda(x, weight)
    _no_grad_inputs("decode_linear", x, weight, bias, residual)
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1]:
        raise ValueError(f"decode_linear: shapes x{tuple(x.shape)} weight{tuple(weight.shape)}")
    M, K = x.shape
    N = weight.shape[0]
    code = _act_code("decode_linear", act)
    x, weight, bias, y = _decode_gemm_operands("decode_linear", x, weight, bias, out)
    if residual is not None and (tuple(residual.shape) != (M, N) or residual.stride(1) != 1 or residual.stride(0) != y.stride(0)):
        raise ValueError("decode_linear: residual must have the output's shape and row stride")
    if M == 0:
        return y
    dense = y.stride(0) == N and x.stride(0) == K and weight.stride(0) == K
    if dense and x.dtype == torch.bfloat16 and K % 8 == 0 and N % 8 == 0 and not _skinny_route(M, N, K, x.dtype):
        return gemm_nt(x, weight, bias, residual, None, code, out_scale, K, y)
    for rows in _row_chunks(M):
        gemm_skinny(x[rows], weight, bias, None if residual is None else residual[rows], code, out_scale, y[rows])
    return y


def gemm_skinny_lora(x, weight, lora_A, lora_B, scaling, bias=None, residual=None, act=0, out_scale=1.0, out=None, workspace=None):
    """Raw mmgl_gemm_skinny_lora call: x [M <= 64, K], weight [N, K], lora_A [r, K], lora_B [N, r], out [M, N]; row strides are free,
    column strides 1; workspace: at least M * r fp32 (allocated when None).  No autograd."""
    require_cuda(x, weight, lora_A, lora_B)
    M, K = x.shape
    N, r = lora_B.shape
    y = torch.empty(M, N, dtype=x.dtype, device=x.device) if out is None else out
    ws = torch.empty(M * r, dtype=torch.float32, device=x.device) if workspace is None else workspace
    if ws.dtype != torch.float32 or ws.numel() < M * r or not ws.is_contiguous():
        raise ValueError(f"gemm_skinny_lora: the workspace must hold {M * r} contiguous fp32 values")
    _lib.call("mmgl_gemm_skinny_lora", dict(flops=2.0 * M * (N * K + r * K + N * r), bytes=float(M * (K + N) + N * K + r * K + N * r) * x.element_size(),
                                            tag=f"{M}x{N}x{K}r{r}"),
              ptr(x), x.stride(0), ptr(weight), weight.stride(0), ptr(bias), ptr(residual), ptr(y), y.stride(0), ptr(lora_A), lora_A.stride(0),
              ptr(lora_B), lora_B.stride(0), r, float(scaling), ptr(ws), M, N, K, act, float(out_scale), dtype_code(x), stream_ptr())
    return y


def decode_lora_linear(x, weight, bias, lora_A, lora_B, scaling, out_scale=1.0, out=None):
    """(x @ weight^T + bias + scaling * (x @ lora_A^T) @ lora_B^T) * out_scale for the few rows of a decode step: the forward of a
    LoRA-adapted projection (lora_linear is its training forward) on mmgl_gemm_skinny_lora -- the weight-streaming GEMM with the rank-r
    term added in fp32 in its epilogue; no merged copy of the weight.  x [M, K], weight [N, K], lora_A [r, K], lora_B [N, r], r <= 256.
    `out` [M, N] may be a strided view with unit column stride (the v columns of a key/value cache row).  Rows go in chunks of 64.
    Forward only; GPU only."""
    require_cuda(x, weight, lora_A, lora_B)
    _no_grad_inputs("decode_lora_linear", x, weight, bias, lora_A, lora_B)
    if (x.dim() != 2 or weight.dim() != 2 or lora_A.dim() != 2 or lora_B.dim() != 2 or x.shape[1] != weight.shape[1]
            or lora_A.shape[1] != x.shape[1] or lora_B.shape != (weight.shape[0], lora_A.shape[0])):
        raise ValueError(f"decode_lora_linear: shapes x{tuple(x.shape)} weight{tuple(weight.shape)} lora_A{tuple(lora_A.shape)} "
                         f"lora_B{tuple(lora_B.shape)}")
    M, K = x.shape
    N, r = lora_B.shape
    if not 1 <= r <= 256:
        raise ValueError(f"decode_lora_linear: rank {r} (1..256)")
    x, weight, bias, y = _decode_gemm_operands("decode_lora_linear", x, weight, bias, out)
    A = lora_A.detach().to(x.dtype)
    B = lora_B.detach().to(x.dtype)
    A = A if A.stride(1) == 1 else A.contiguous()
    B = B if B.stride(1) == 1 else B.contiguous()
    if M == 0:
        return y
    ws = torch.empty(min(M, 64) * r, dtype=torch.float32, device=x.device)       # t = x A^T of one chunk
    for rows in _row_chunks(M):
        gemm_skinny_lora(x[rows], weight, A, B, scaling, bias, None, 0, out_scale, y[rows], ws)
    return y


# -- FP8 frozen weights: a weight as e4m3fn codes with one power-of-two scale per row (include/mmgl_hip.h), and the decode GEMM on them
def quantize_weight_fp8(weight, out=None):
    """weight [N, K] (bf16 or fp32, unit column stride, any row stride) -> (codes [N, K] torch.float8_e4m3fn, exps [N] int8) with
    weight ~ codes * 2^exps[:, None]: the FP8 key/value cache's format per weight row (mmgl_weight_quantize, one launch).  Run once per
    frozen weight; non-finite weights are outside the contract.  out: a (codes, exps) pair to fill -- codes [N, K] e4m3fn or uint8 with
    unit column stride and any row stride, exps [N] int8 contiguous.  Forward only; GPU only."""
    require_cuda(weight)
    if weight.dim() != 2 or weight.dtype not in (torch.bfloat16, torch.float32) or weight.shape[0] == 0 or weight.shape[1] == 0:
        raise ValueError(f"quantize_weight_fp8: weight{tuple(weight.shape)} {weight.dtype} must be a non-empty [N, K] bf16 or fp32 matrix")
    w = weight.detach()
    w = w if w.stride(1) == 1 else w.contiguous()
    N, K = w.shape
    if out is None:
        codes = torch.empty(N, K, dtype=KV_FP8, device=w.device)
        exps = torch.empty(N, dtype=torch.int8, device=w.device)
    else:
        codes, exps = out
        require_cuda(codes, exps)
        if (tuple(codes.shape) != (N, K) or codes.dtype not in (KV_FP8, torch.uint8) or codes.stride(1) != 1 or tuple(exps.shape) != (N,)
                or exps.dtype != torch.int8 or not exps.is_contiguous() or codes.device != w.device or exps.device != w.device):
            raise ValueError(f"quantize_weight_fp8: out = (codes{tuple(codes.shape)}/{codes.stride()} {codes.dtype}, exps{tuple(exps.shape)} "
                             f"{exps.dtype}) for weight{tuple(w.shape)}: codes [N, K] {KV_FP8} with unit column stride, exps [N] int8")
    _lib.call("mmgl_weight_quantize", dict(bytes=float(N * K) * (2 * w.element_size() + 1)), ptr(w), w.stride(0), ptr(codes), codes.stride(0),
              ptr(exps), N, K, dtype_code(w), stream_ptr())
    return codes, exps


def _w8_operands(op, x, codes, exps):
    if (x.dim() != 2 or codes.dim() != 2 or x.shape[1] != codes.shape[1] or codes.dtype not in (KV_FP8, torch.uint8) or codes.stride(1) != 1
            or exps.dtype != torch.int8 or tuple(exps.shape) != (codes.shape[0],) or not exps.is_contiguous()
            or codes.device != x.device or exps.device != x.device):
        raise ValueError(f"{op}: shapes x{tuple(x.shape)} codes{tuple(codes.shape)}/{codes.stride()} {codes.dtype} exps{tuple(exps.shape)} "
                         f"{exps.dtype}: codes [N, K] {KV_FP8} with unit column stride and exps [N] int8 on {x.device}")


def gemm_skinny_w8(x, codes, exps, bias=None, residual=None, act=0, out_scale=1.0, out=None):
    """Raw mmgl_gemm_skinny_w8 call: x [M <= 64, K], codes [N, K] e4m3fn (or uint8), exps [N] int8, out [M, N]; row strides are free,
    column strides 1.  No autograd; the operands are the caller's to check (decode_linear_w8 does)."""
    require_cuda(x, codes, exps)
    M, K = x.shape
    N = codes.shape[0]
    y = torch.empty(M, N, dtype=x.dtype, device=x.device) if out is None else out
    _lib.call("mmgl_gemm_skinny_w8", dict(flops=2.0 * M * N * K, bytes=float(M * K + M * N) * x.element_size() + float(N * K + N), tag=f"{M}x{N}x{K}"),
              ptr(x), x.stride(0), ptr(codes), codes.stride(0), ptr(exps), ptr(bias), ptr(residual), ptr(y), y.stride(0), M, N, K, act,
              float(out_scale), dtype_code(x), stream_ptr())
    return y


def decode_linear_w8(x, codes, exps, bias=None, act="none", out_scale=1.0, residual=None, out=None):
    """ops.decode_linear on a quantised weight: act((x @ (codes * 2^exps)^T + bias) * out_scale) + residual for the few rows of a decode
    step, x [M, K], (codes [N, K], exps [N]) as quantize_weight_fp8 returned them.  `out` [M, N] may be a strided view with unit column
    stride -- a column of the key/value cache -- and `residual` shares its row stride.  Rows go to mmgl_gemm_skinny_w8 in chunks of 64;
    there is no other route (mmgl_gemm_nt has no form on codes).  Forward only; GPU only."""
    require_cuda(x, codes, exps)
    _no_grad_inputs("decode_linear_w8", x, bias, residual)
    _w8_operands("decode_linear_w8", x, codes, exps)
    M, N = x.shape[0], codes.shape[0]
    code = _act_code("decode_linear_w8", act)
    if x.stride(1) != 1:
        x = x.contiguous()
    y = torch.empty(M, N, dtype=x.dtype, device=x.device) if out is None else out
    if tuple(y.shape) != (M, N) or y.stride(1) != 1 or y.dtype != x.dtype or x.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"decode_linear_w8: out{tuple(y.shape)} {y.dtype} for x{tuple(x.shape)} {x.dtype} codes{tuple(codes.shape)}")
    if bias is not None and bias.dtype != x.dtype:
        bias = bias.to(x.dtype)
    if residual is not None and (tuple(residual.shape) != (M, N) or residual.stride(1) != 1 or residual.stride(0) != y.stride(0)):
        raise ValueError("decode_linear_w8: residual must have the output's shape and row stride")
    for rows in _row_chunks(M):
        gemm_skinny_w8(x[rows], codes, exps, bias, None if residual is None else residual[rows], code, out_scale, y[rows])
    return y


def _decode_attn_operands(op, q, k, v, key_valid, num_heads, out, q_rows=1, key_cols=None, names=("k", "v", "keys"), tail=""):
    """The operands of single-query attention: q [B * q_rows, d] against the per-sample views k, v [B, S, key_cols] (None: d columns)
    with unit column stride and common strides, and key_valid [B, S].  Returns (B, S, d, the mask as uint8 with unit column stride
    and its own row stride, `out` checked or a new dense [B * q_rows, d]).  names and tail only word the messages."""
    if (q.dim() != 2 or k.dim() != 3 or k.shape != v.shape or q.shape[0] != k.shape[0] * q_rows
            or (q.shape[1] if key_cols is None else key_cols) != k.shape[2] or k.stride() != v.stride() or k.stride(2) != 1 or q.stride(1) != 1
            or k.dtype != q.dtype or v.dtype != q.dtype):
        raise ValueError(f"{op}: incompatible q{tuple(q.shape)} {names[0]}{tuple(k.shape)}/{k.stride()} {names[1]}{tuple(v.shape)}/{v.stride()}{tail}")
    R, d = q.shape
    B, S = k.shape[:2]
    if d % num_heads:
        raise ValueError(f"embed_dim must be divisible by num_heads (got `embed_dim`: {d} and `num_heads`: {num_heads}).")
    _check_mask(key_valid, (B, S))
    if S == 0:
        raise ValueError(f"{op}: no {names[2]}")
    key_valid = _as_uint8(key_valid)
    if key_valid.dtype != torch.uint8:
        key_valid = key_valid.to(torch.uint8)
    if key_valid.stride(1) != 1:
        key_valid = key_valid.contiguous()
    if out is None:
        out = torch.empty(R, d, dtype=q.dtype, device=q.device)
    elif tuple(out.shape) != (R, d) or out.dtype != q.dtype or out.device != q.device or not out.is_contiguous():
        raise ValueError(f"{op}: out{tuple(out.shape)} {out.dtype} must be a dense [{R}, {d}] {q.dtype} tensor on {q.device}")
    return B, S, d, key_valid, out


def attn_decode(q, k, v, key_valid, num_heads, out=None, num_kv_heads=None):
    """One query row per (sample, head) against S keys: q [B, d] already scaled; k, v [B, S, d] views with unit column stride and
    common strides (column slabs of the cache rows [B, capacity, 2d]); key_valid [B, S] bool/uint8 view (True = attend).  Returns [B, d]
    (`out`, a dense [B, d] tensor of q's dtype, when given: a refused call leaves it as it was).
    A sample with no valid key attends uniformly over its S keys.  Forward only; GPU only.
    Grouped-query attention (num_kv_heads = Hkv < num_heads = H, Hkv a divisor of H): k, v [B, S, Hkv*D] with D = d / H -- column
    slabs of cache rows [B, capacity, 2*Hkv*D] -- and query head h reads key / value head h // (H / Hkv) (mmgl_attn_decode_gqa_fwd:
    one read of a cached key serves the H / Hkv query heads of its group; nothing is expanded)."""
    require_cuda(q, k, v, key_valid)
    _no_grad_inputs("attn_decode", q, k, v)
    Hkv = _kv_heads("attn_decode", num_heads, num_kv_heads)
    kd = q.shape[-1] if Hkv is None or q.shape[-1] % num_heads else q.shape[-1] // num_heads * Hkv     # columns of a key row
    B, S, d, key_valid, out = _decode_attn_operands("attn_decode", q, k, v, key_valid, num_heads, out, key_cols=kd,
                                                    tail="" if Hkv is None else f" for H={num_heads}, Hkv={Hkv}")
    if Hkv is None:
        _lib.call("mmgl_attn_decode_fwd", dict(bytes=2.0 * B * S * d * q.element_size()), ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(1), k.stride(0),
                  ptr(key_valid), key_valid.stride(0), ptr(out), B, num_heads, S, d // num_heads, dtype_code(q), stream_ptr())
    else:
        _lib.call("mmgl_attn_decode_gqa_fwd", dict(bytes=2.0 * B * S * kd * q.element_size()), ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(1),
                  k.stride(0), ptr(key_valid), key_valid.stride(0), ptr(out), B, num_heads, Hkv, S, d // num_heads, dtype_code(q), stream_ptr())
    return out


def attn_decode_relbias(q, k, v, bias, num_heads, out=None):
    """The T5 decoder's cached self-attention for one new token: softmax_s(q . k_s + bias[h, S - 1 - s]) v per (sample, head), unscaled
    and unmasked.  q [B, d] is the RAW query projection; k, v [B, S, d] views with unit column stride and common strides (column slabs
    of the cache rows [B, capacity, 2d]) whose last row s = S - 1 is the query's own token; bias fp32 [H, >= S] with unit column
    stride (t5_decode_bias: column = distance to the query).  Returns [B, d] (`out`, a dense [B, d] tensor of q's dtype, when given: a
    refused call leaves it as it was).  Forward only; GPU only."""
    require_cuda(q, k, v, bias)
    _no_grad_inputs("attn_decode_relbias", q, k, v, bias)
    if (q.dim() != 2 or k.dim() != 3 or k.shape != v.shape or q.shape[0] != k.shape[0] or q.shape[1] != k.shape[2] or k.stride() != v.stride()
            or k.stride(2) != 1 or q.stride(1) != 1 or k.dtype != q.dtype or v.dtype != q.dtype):
        raise ValueError(f"attn_decode_relbias: incompatible q{tuple(q.shape)} k{tuple(k.shape)}/{k.stride()} v{tuple(v.shape)}/{v.stride()}")
    B, d = q.shape
    S = k.shape[1]
    if d % num_heads:
        raise ValueError(f"embed_dim must be divisible by num_heads (got `embed_dim`: {d} and `num_heads`: {num_heads}).")
    if S == 0:
        raise ValueError("attn_decode_relbias: no keys")
    if (bias.dim() != 2 or bias.dtype != torch.float32 or bias.shape[0] != num_heads or bias.shape[1] < S
            or (bias.shape[1] > 1 and bias.stride(1) != 1) or bias.device != q.device):
        raise ValueError(f"attn_decode_relbias: bias{tuple(bias.shape)}/{bias.stride()} {bias.dtype} must be fp32 [{num_heads}, >= {S}] with unit "
                         f"column stride on {q.device}")
    if out is None:
        out = torch.empty(B, d, dtype=q.dtype, device=q.device)
    elif tuple(out.shape) != (B, d) or out.dtype != q.dtype or out.device != q.device or not out.is_contiguous():
        raise ValueError(f"attn_decode_relbias: out{tuple(out.shape)} {out.dtype} must be a dense [{B}, {d}] {q.dtype} tensor on {q.device}")
    _lib.call("mmgl_attn_decode_relbias_fwd", dict(bytes=2.0 * B * S * d * q.element_size()), ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(1),
              k.stride(0), ptr(bias), bias.stride(0), ptr(out), B, num_heads, S, d // num_heads, dtype_code(q), stream_ptr())
    return out


def t5_decode_bias(table, capacity, num_buckets, max_distance):
    """The bias rows of attn_decode_relbias for a cache of `capacity` columns: fp32 [H, capacity], entry [h, d] =
    table[bucket(-d), h] -- the word a T5 decoder adds to the score of the key d positions behind the query.  table [num_buckets, H] is
    the decoder's relative_attention_bias weight; the buckets of the relative positions 0, -1, ..., -(capacity - 1) are t5_bucket_table's
    (transformers' own _relative_position_bucket, bidirectional=False).  One small gather, once per generation."""
    if table.dim() != 2 or table.shape[0] != int(num_buckets) or int(capacity) < 1:
        raise ValueError(f"t5_decode_bias: table{tuple(table.shape)} for {num_buckets} buckets, capacity {capacity}")
    bucket_of = t5_bucket_table(int(capacity), 1, False, num_buckets, max_distance, table.device)       # entry i: position i - (capacity - 1)
    rows = torch.empty(table.shape[1], int(capacity), dtype=torch.float32, device=table.device)      # strides (capacity, 1), also at capacity 1
    return rows.copy_(table.detach().float()[bucket_of.flip(0).long()].t())


def rope_kv_append(qkv, cos_sin_row, kv_col, num_heads, num_kv_heads):
    """The new token's row of the fused q | k | v projection, qkv [B, (H + 2*Hkv)*D] (unit column stride), at one position:
    rotates the H query heads in place and writes the rotated Hkv key heads and the unrotated Hkv value heads to kv_col
    [B, 2*Hkv*D] -- the token's column of the cache rows, a strided view with unit column stride; the k and v blocks of qkv stay as
    they were.  cos_sin_row: fp32 [D/2, 2], the position's row of the table rope_qk_ takes (rotate_half convention).  One launch.
    Returns qkv.  A refused call leaves qkv and kv_col untouched.  Forward only; GPU only."""
    require_cuda(qkv, cos_sin_row, kv_col)
    _no_grad_inputs("rope_kv_append", qkv, kv_col)
    H, Hkv = int(num_heads), int(num_kv_heads)
    if H < 1 or Hkv < 1 or H % Hkv:
        raise ValueError(f"rope_kv_append: num_heads = {H} must be a multiple of num_kv_heads = {Hkv}")
    if qkv.dim() != 2 or qkv.shape[1] % (H + 2 * Hkv) or qkv.stride(1) != 1:
        raise ValueError(f"rope_kv_append: qkv{tuple(qkv.shape)}/{qkv.stride()} is not [B, (H+2*Hkv)*D] for H={H}, Hkv={Hkv}")
    B, D = qkv.shape[0], qkv.shape[1] // (H + 2 * Hkv)
    if (tuple(kv_col.shape) != (B, 2 * Hkv * D) or kv_col.stride(1) != 1 or kv_col.dtype != qkv.dtype or kv_col.device != qkv.device):
        raise ValueError(f"rope_kv_append: kv_col{tuple(kv_col.shape)}/{kv_col.stride()} {kv_col.dtype} must be a [{B}, {2 * Hkv * D}] "
                         f"{qkv.dtype} view with unit column stride")
    if cos_sin_row.dtype != torch.float32 or tuple(cos_sin_row.shape) != (D // 2, 2) or not cos_sin_row.is_contiguous():
        raise ValueError(f"rope_kv_append: cos_sin_row must be contiguous fp32 [D/2={D // 2}, 2], got {cos_sin_row.dtype} {tuple(cos_sin_row.shape)}")
    if B == 0:
        return qkv
    _lib.call("mmgl_rope_kv_append", dict(bytes=float(2 * H + 4 * Hkv) * B * D * qkv.element_size()), ptr(qkv), qkv.stride(0), ptr(cos_sin_row),
              ptr(kv_col), kv_col.stride(0), B, H, Hkv, D, dtype_code(qkv), stream_ptr())
    return qkv


# ------------------------------------------------------------------------------------------ FP8 key/value cache (csrc/decode.hip)
KV_FP8 = torch.float8_e4m3fn            # the code dtype of a quantised cache row; its scales are int8 exponents (include/mmgl_hip.h)


def _q8_cache_operands(op, kvq, scale, B, d, num_heads, dtype_like):
    """The two tensors of a quantised cache for rows of B samples, d = H*D channels: kvq [B, capacity, 2d] e4m3fn codes (or uint8)
    and scale [B, capacity, 2H] int8, unit column stride, on one device.  Returns (capacity, D)."""
    if d % num_heads:
        raise ValueError(f"embed_dim must be divisible by num_heads (got `embed_dim`: {d} and `num_heads`: {num_heads}).")
    H = int(num_heads)
    if (kvq.dim() != 3 or scale.dim() != 3 or kvq.dtype not in (KV_FP8, torch.uint8) or scale.dtype != torch.int8
            or tuple(kvq.shape[::2]) != (B, 2 * d) or tuple(scale.shape) != (B, kvq.shape[1], 2 * H) or kvq.stride(2) != 1 or scale.stride(2) != 1
            or kvq.device != dtype_like.device or scale.device != dtype_like.device):
        raise ValueError(f"{op}: incompatible codes{tuple(kvq.shape)}/{kvq.stride()} {kvq.dtype} scale{tuple(scale.shape)}/{scale.stride()} "
                         f"{scale.dtype} for {B} samples of {H} heads, {d} channels: codes [B, capacity, 2d] {KV_FP8} and scale "
                         f"[B, capacity, 2H] int8 on {dtype_like.device}")
    return kvq.shape[1], d // H


def kv_quantize(k, v, kvq, scale, num_heads):
    """Files n key and value rows into columns [0, n) of a quantised cache: k, v [B, n, d] views with unit column stride and common
    strides (the column slabs of a fused qkv output, or two tensors), kvq [B, capacity, 2d] e4m3fn codes, scale [B, capacity, 2H] int8
    exponents (key heads first; the format is include/mmgl_hip.h's).  One launch.  Returns (kvq, scale); a refused call leaves them as
    they were.  Forward only; GPU only."""
    require_cuda(k, v, kvq, scale)
    _no_grad_inputs("kv_quantize", k, v)
    if (k.dim() != 3 or k.shape != v.shape or k.stride() != v.stride() or k.stride(2) != 1 or k.dtype != v.dtype or k.device != v.device):
        raise ValueError(f"kv_quantize: incompatible k{tuple(k.shape)}/{k.stride()} {k.dtype} v{tuple(v.shape)}/{v.stride()} {v.dtype}")
    B, n, d = k.shape
    capacity, D = _q8_cache_operands("kv_quantize", kvq, scale, B, d, num_heads, k)
    if n > capacity:
        raise ValueError(f"kv_quantize: {n} rows for a cache of {capacity} columns")
    code = dtype_code(k)
    if B == 0 or n == 0:
        return kvq, scale
    _lib.call("mmgl_kv_quantize", dict(bytes=2.0 * B * n * d * (k.element_size() + 1)), ptr(k), ptr(v), k.stride(1), k.stride(0), ptr(kvq),
              kvq.stride(1), kvq.stride(0), ptr(scale), scale.stride(1), scale.stride(0), B, n, int(num_heads), D, code, stream_ptr())
    return kvq, scale


def attn_decode_q8(q, k_new, v_new, kvq, scale, key_valid, num_heads, out=None, num_kv_heads=None):
    """ops.attn_decode on a quantised cache, and the filing of the new token into it, one launch (mmgl_attn_decode_q8_fwd).
      q [B, d] already scaled; k_new, v_new [B, d]: views with unit column stride and a common row stride (the halves of the k|v
      projection's dense [B, 2d] output), the new token's key and value: they take part unquantised and always valid;
      kvq [B, capacity, 2d] e4m3fn codes and scale [B, capacity, 2H] int8 exponents (ops.kv_quantize): columns [0, S) are read,
      column S < capacity is WRITTEN with the new token's codes and exponents; key_valid [B, S] bool/uint8 view of the cached
      columns, S >= 1 (a masked cached key weighs nothing).
    The result equals ops.attn_decode on the dequantised columns followed by the new row, up to summation order.  Returns [B, d]
    (`out`, a dense tensor of q's dtype, when given: a refused call leaves it and the cache as they were).  Forward only; GPU only.
    Grouped-query attention (num_kv_heads = Hkv < num_heads = H, Hkv a divisor of H; mmgl_attn_decode_gqa_q8_fwd): the cache holds
    Hkv heads -- kvq [B, capacity, 2*Hkv*D], scale [B, capacity, 2*Hkv], k_new, v_new [B, Hkv*D] with D = d / H (the k and v columns
    of DecodeCache.kv_new after ops.rope_kv_append) -- and query head h reads key / value head h // (H / Hkv): one read and one
    dequantisation of a cached key serves the query heads of its group; nothing is expanded."""
    require_cuda(q, k_new, v_new, kvq, scale, key_valid)
    _no_grad_inputs("attn_decode_q8", q, k_new, v_new)
    Hkv = _kv_heads("attn_decode_q8", num_heads, num_kv_heads)
    H = int(num_heads)
    kd = q.shape[-1] if Hkv is None or q.shape[-1] % H else q.shape[-1] // H * Hkv              # columns of a key row
    if (q.dim() != 2 or q.stride(1) != 1 or k_new.dim() != 2 or tuple(k_new.shape) != (q.shape[0], kd) or k_new.shape != v_new.shape
            or k_new.stride() != v_new.stride() or k_new.stride(1) != 1 or k_new.dtype != q.dtype or v_new.dtype != q.dtype
            or k_new.device != q.device or v_new.device != q.device):
        raise ValueError(f"attn_decode_q8: incompatible q{tuple(q.shape)}/{q.stride()} {q.dtype} k_new{tuple(k_new.shape)}/{k_new.stride()} "
                         f"{k_new.dtype} v_new{tuple(v_new.shape)}/{v_new.stride()} {v_new.dtype}"
                         + ("" if Hkv is None else f" for H={H}, Hkv={Hkv}"))
    B, d = q.shape
    if d % H:
        raise ValueError(f"embed_dim must be divisible by num_heads (got `embed_dim`: {d} and `num_heads`: {num_heads}).")
    capacity, D = _q8_cache_operands("attn_decode_q8", kvq, scale, B, kd, H if Hkv is None else Hkv, q)
    if key_valid.dim() != 2 or key_valid.shape[0] != B or key_valid.device != q.device:
        raise ValueError(f"attn_decode_q8: key_valid{tuple(key_valid.shape)} must be a [{B}, S] mask on {q.device}")
    S = key_valid.shape[1]
    if S == 0:
        raise ValueError("attn_decode_q8: no cached columns")
    if S >= capacity:
        raise ValueError(f"attn_decode_q8: the cache is full ({S} cached columns of capacity {capacity}): no column for the new token")
    code = dtype_code(q)
    if out is None:
        out = torch.empty(B, d, dtype=q.dtype, device=q.device)
    elif tuple(out.shape) != (B, d) or out.dtype != q.dtype or out.device != q.device or not out.is_contiguous():
        raise ValueError(f"attn_decode_q8: out{tuple(out.shape)} {out.dtype} must be a dense [{B}, {d}] {q.dtype} tensor on {q.device}")
    key_valid = _as_uint8(key_valid)
    if key_valid.dtype != torch.uint8:
        key_valid = key_valid.to(torch.uint8)
    if key_valid.stride(1) != 1:
        key_valid = key_valid.contiguous()
    if Hkv is None:
        _lib.call("mmgl_attn_decode_q8_fwd", dict(bytes=2.0 * B * S * (d + H) + 4.0 * B * d * q.element_size()), ptr(q), q.stride(0), ptr(k_new),
                  ptr(v_new), k_new.stride(0), ptr(kvq), ptr_off(kvq, d), kvq.stride(1), kvq.stride(0), ptr(scale), ptr_off(scale, H),
                  scale.stride(1), scale.stride(0), capacity, ptr(key_valid), key_valid.stride(0), ptr(out), B, H, S, D, code, stream_ptr())
    else:
        _lib.call("mmgl_attn_decode_gqa_q8_fwd", dict(bytes=2.0 * B * S * (kd + Hkv) + 2.0 * B * (d + kd) * q.element_size()), ptr(q), q.stride(0),
                  ptr(k_new), ptr(v_new), k_new.stride(0), ptr(kvq), ptr_off(kvq, kd), kvq.stride(1), kvq.stride(0), ptr(scale),
                  ptr_off(scale, Hkv), scale.stride(1), scale.stride(0), capacity, ptr(key_valid), key_valid.stride(0), ptr(out), B, H, Hkv, S,
                  D, code, stream_ptr())
    return out


# ------------------------------------------------------------------------------------------ beam search (csrc/decode.hip, csrc/beam.hip)
MAX_BEAMS = 8


def _beams(op, num_beams):
    W = int(num_beams)
    if W < 1:
        raise ValueError(f"{op}: num_beams = {num_beams} must be positive")
    if W > MAX_BEAMS:
        raise ValueError(f"{op}: {W} beams per sample (1..{MAX_BEAMS})")
    return W


def attn_decode_beam(q, k_pre, v_pre, key_valid, num_heads, num_beams, k_tail=None, v_tail=None, src=None, out=None):
    """Single-query attention for the B*W rows of a beam-search step; row b*W + w is beam slot w of sample b (W = num_beams <= 8).
      q [B*W, d] already scaled; k_pre, v_pre [B, S_pre, d] and key_valid [B, S_pre]: the views ops.attn_decode takes, one row set
      per SAMPLE (the prompt's cache rows or the projected neighbor tokens), read once for the W queries;
      k_tail, v_tail [B*W, n_tail, d]: column slabs of the tail buffer [B*W, n_cap, 2d] (unit column stride, common strides), the keys
      the hypotheses generated themselves; src int32 [B*W, >= n_tail] (unit column stride): tail key j of row (b, w) is row
      b*W + src[b*W + w, j] of the tail.  src values lie in [0, W): the caller's contract (the kernel clamps, nothing is checked on
      the device).  No tail (None, or n_tail = 0) is the cross-attention call.
    A sample whose prefix has no valid key attends uniformly over all its S_pre + n_tail keys.  Returns [B*W, d] (`out`, a dense tensor
    of q's dtype, when given: a refused call leaves it as it was).  Forward only; GPU only."""
    require_cuda(q, k_pre, v_pre, key_valid, k_tail, v_tail, src)
    _no_grad_inputs("attn_decode_beam", q, k_pre, v_pre, k_tail, v_tail)
    W = _beams("attn_decode_beam", num_beams)
    B, S, d, key_valid, out = _decode_attn_operands("attn_decode_beam", q, k_pre, v_pre, key_valid, num_heads, out, q_rows=W,
                                                    names=("k_pre", "v_pre", "prefix keys"), tail=f" for {W} beams")
    R = B * W
    n_tail = 0 if k_tail is None else k_tail.shape[1] if k_tail.dim() == 3 else -1
    if (k_tail is None) != (v_tail is None) or n_tail < 0:
        raise ValueError("attn_decode_beam: k_tail and v_tail come together, as [B*W, n_tail, d] views")
    if n_tail:
        if (tuple(k_tail.shape) != (R, n_tail, d) or k_tail.shape != v_tail.shape or k_tail.stride() != v_tail.stride() or k_tail.stride(2) != 1
                or k_tail.dtype != q.dtype or v_tail.dtype != q.dtype):
            raise ValueError(f"attn_decode_beam: incompatible k_tail{tuple(k_tail.shape)}/{k_tail.stride()} v_tail{tuple(v_tail.shape)}/"
                             f"{v_tail.stride()} for q{tuple(q.shape)}")
        if src is None or src.dtype != torch.int32 or src.dim() != 2 or src.shape[0] != R or src.shape[1] < n_tail or src.stride(1) != 1:
            raise ValueError(f"attn_decode_beam: src must be an int32 [{R}, >= {n_tail}] view with unit column stride")
    tail = (ptr(k_tail), ptr(v_tail), k_tail.stride(1), k_tail.stride(0), ptr(src), src.stride(0)) if n_tail else (None, None, 0, 0, None, 0)
    _lib.call("mmgl_attn_decode_beam_fwd", dict(bytes=2.0 * (B * S + R * n_tail) * d * q.element_size()), ptr(q), q.stride(0), ptr(k_pre),
              ptr(v_pre), k_pre.stride(1), k_pre.stride(0), ptr(key_valid), key_valid.stride(0), *tail, ptr(out), B, W, num_heads, S, n_tail,
              d // num_heads, dtype_code(q), stream_ptr())
    return out


# ------------------------------------------------------------------------------------------ prompt-lookup decoding (csrc/decode.hip, csrc/lookup.hip)
MAX_LOOKUP_TOKENS = 7                   # K: drafted tokens per verify step (K + 1 <= 8 rows per sample)
MAX_LOOKUP_NGRAM = 4                    # N: longest n-gram matched
MAX_LOOKUP_HISTORY = 8192               # T + n_new: the row's history lives in LDS


def _state_vector(op, name, t, rows, dtype, device):
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != (rows,) or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{op}: {name} must be a dense {dtype} [{rows}] tensor on {device}")


def attn_decode_block(q, k_new, v_new, k, v, key_valid, lens, num_heads, m, out=None):
    """Causal attention of m <= 8 new tokens per sample against the cache, and their filing into it, one launch; row b*m + i is new
    token i of sample b.
      q [B*m, d] already scaled; k_new, v_new [B*m, d]: views with unit column stride and a common row stride (the halves of the
      k|v projection's dense [B*m, 2d] output); k, v [B, capacity, d]: the column slabs of the cache rows [B, capacity, 2d], read
      below lens[b] and WRITTEN at columns lens[b] .. lens[b] + m - 1 (a column at or past capacity is dropped); key_valid
      [B, capacity] bool/uint8; lens int32 [B] on the device, 0 <= lens[b] <= capacity: the caller's contract (the kernel clamps,
      nothing is checked on the device).
    Row (b, i) attends the valid cache columns below lens[b] and the new keys j <= i.  Returns [B*m, d] (`out`, a dense tensor of
    q's dtype, when given: a refused call leaves it and the cache as they were).  Forward only; GPU only."""
    require_cuda(q, k_new, v_new, k, v, key_valid, lens)
    _no_grad_inputs("attn_decode_block", q, k_new, v_new, k, v)
    m = int(m)
    if not 1 <= m <= MAX_LOOKUP_TOKENS + 1:
        raise ValueError(f"attn_decode_block: m = {m} new tokens per sample (1..{MAX_LOOKUP_TOKENS + 1})")
    B, S, d, key_valid, out = _decode_attn_operands("attn_decode_block", q, k, v, key_valid, num_heads, out, q_rows=m,
                                                    names=("k", "v", "cache columns"), tail=f" for {m} new tokens per sample")
    if (k_new.dim() != 2 or tuple(k_new.shape) != (B * m, d) or k_new.shape != v_new.shape or k_new.stride() != v_new.stride()
            or k_new.stride(1) != 1 or k_new.dtype != q.dtype or v_new.dtype != q.dtype or k_new.device != q.device or v_new.device != q.device):
        raise ValueError(f"attn_decode_block: incompatible k_new{tuple(k_new.shape)}/{k_new.stride()} v_new{tuple(v_new.shape)}/"
                         f"{v_new.stride()} for q{tuple(q.shape)}")
    _state_vector("attn_decode_block", "lens", lens, B, torch.int32, q.device)
    if k.device != q.device or key_valid.device != q.device:
        raise ValueError("attn_decode_block: the operands are on different devices")
    _lib.call("mmgl_attn_decode_block_fwd", dict(bytes=2.0 * B * (S + m) * d * q.element_size()), ptr(q), q.stride(0), ptr(k_new), ptr(v_new),
              k_new.stride(0), ptr(k), ptr(v), k.stride(1), k.stride(0), S, ptr(key_valid), key_valid.stride(0), ptr(lens), ptr(out), B, m,
              num_heads, d // num_heads, dtype_code(q), stream_ptr())
    return out


def _block_heads(op, num_heads, num_kv_heads, m):
    H, Hkv, m = int(num_heads), int(num_kv_heads), int(m)
    if H < 1 or Hkv < 1 or H % Hkv:
        raise ValueError(f"{op}: num_heads = {H} must be a multiple of num_kv_heads = {Hkv}")
    if not 1 <= m <= MAX_LOOKUP_TOKENS + 1:
        raise ValueError(f"{op}: m = {m} new tokens per sample (1..{MAX_LOOKUP_TOKENS + 1})")
    return H, Hkv, m


def rope_kv_append_block(qkv, cos_sin, kv, lens, num_heads, num_kv_heads, m):
    """rope_kv_append for the B*m rows of a verify step (prompt-lookup decoding on a grouped-query cache); row b*m + i of qkv
    [B*m, (H + 2*Hkv)*D] (unit column stride) is new token i of sample b, at position p = lens[b] + i -- per sample, on the device.
      cos_sin fp32 [n_pos, D/2, 2], contiguous: the table rope_qk_ takes, read at row min(p, n_pos - 1);
      kv [B, capacity, 2*Hkv*D]: the layer's cache rows, a view with unit column stride; lens int32 [B] on the device,
      0 <= lens[b] <= capacity: the caller's contract (the kernel clamps, nothing is checked on the device).
    Rotates the H query heads of every row in place and writes its rotated Hkv key heads and unrotated Hkv value heads to column p of
    kv[b] -- nowhere when p >= capacity; the k and v blocks of qkv stay as they were.  One launch; m = 1 with equal lens is bitwise
    rope_kv_append.  Returns qkv.  A refused call leaves qkv and kv untouched.  Forward only; GPU only."""
    op = "rope_kv_append_block"
    require_cuda(qkv, cos_sin, kv, lens)
    _no_grad_inputs(op, qkv, kv)
    H, Hkv, m = _block_heads(op, num_heads, num_kv_heads, m)
    if qkv.dim() != 2 or qkv.shape[0] % m or qkv.shape[1] % (H + 2 * Hkv) or qkv.stride(1) != 1:
        raise ValueError(f"{op}: qkv{tuple(qkv.shape)}/{qkv.stride()} is not [B*m, (H+2*Hkv)*D] for H={H}, Hkv={Hkv}, m={m}")
    B, D = qkv.shape[0] // m, qkv.shape[1] // (H + 2 * Hkv)
    if (kv.dim() != 3 or kv.shape[0] != B or kv.shape[1] < 1 or kv.shape[2] != 2 * Hkv * D or kv.stride(2) != 1 or kv.dtype != qkv.dtype
            or kv.device != qkv.device):
        raise ValueError(f"{op}: kv{tuple(kv.shape)}/{kv.stride()} {kv.dtype} must be a [{B}, capacity, {2 * Hkv * D}] {qkv.dtype} view with "
                         "unit column stride")
    if (cos_sin.dtype != torch.float32 or cos_sin.dim() != 3 or cos_sin.shape[0] < 1 or tuple(cos_sin.shape[1:]) != (D // 2, 2)
            or not cos_sin.is_contiguous() or cos_sin.device != qkv.device):
        raise ValueError(f"{op}: cos_sin must be contiguous fp32 [n_pos, D/2={D // 2}, 2] on {qkv.device}, got {cos_sin.dtype} "
                         f"{tuple(cos_sin.shape)}")
    _state_vector(op, "lens", lens, B, torch.int32, qkv.device)
    if B == 0:
        return qkv
    _lib.call("mmgl_rope_kv_append_block", dict(bytes=float(2 * H + 4 * Hkv) * B * m * D * qkv.element_size()), ptr(qkv), qkv.stride(0),
              ptr(cos_sin), cos_sin.shape[0], ptr(kv), kv.stride(1), kv.stride(0), kv.shape[1], ptr(lens), B, m, H, Hkv, D, dtype_code(qkv),
              stream_ptr())
    return qkv


def attn_decode_gqa_block(q, k, v, key_valid, lens, num_heads, num_kv_heads, m, out=None):
    """Causal attention of m <= 8 new tokens per sample over a grouped-query cache that holds them already (rope_kv_append_block
    runs first; this call only reads); row b*m + i is new token i of sample b.
      q [B*m, d] already scaled (the rotated query columns of the qkv rows); k, v [B, capacity, Hkv*D] with D = d / H: the column
      slabs of the cache rows [B, capacity, 2*Hkv*D], unit column stride and common strides; key_valid [B, capacity] bool/uint8;
      lens int32 [B] on the device, 0 <= lens[b] <= capacity: the caller's contract (the kernel clamps).
    Row (b, i), query head h, reads key / value head h // (H / Hkv): the valid cache columns below lens[b] and the new columns
    lens[b] .. lens[b] + i below the capacity (always valid).  Nothing is expanded to H heads.  A row whose own column is at or past
    the capacity gets an unspecified value.  Returns [B*m, d] (`out`, a dense tensor of q's dtype, when given: a refused call leaves
    it as it was).  Forward only; GPU only."""
    op = "attn_decode_gqa_block"
    require_cuda(q, k, v, key_valid, lens)
    _no_grad_inputs(op, q, k, v)
    H, Hkv, m = _block_heads(op, num_heads, num_kv_heads, m)
    kd = q.shape[-1] if q.shape[-1] % H else q.shape[-1] // H * Hkv                  # columns of a key row
    B, S, d, key_valid, out = _decode_attn_operands(op, q, k, v, key_valid, H, out, q_rows=m, key_cols=kd,
                                                    names=("k", "v", "cache columns"), tail=f" for H={H}, Hkv={Hkv}, {m} new tokens per sample")
    _state_vector(op, "lens", lens, B, torch.int32, q.device)
    if k.device != q.device or key_valid.device != q.device:
        raise ValueError(f"{op}: the operands are on different devices")
    _lib.call("mmgl_attn_decode_gqa_block_fwd", dict(bytes=2.0 * B * (S + m) * kd * q.element_size()), ptr(q), q.stride(0), ptr(k), ptr(v),
              k.stride(1), k.stride(0), S, ptr(key_valid), key_valid.stride(0), ptr(lens), ptr(out), B, m, H, Hkv, d // H, dtype_code(q),
              stream_ptr())
    return out


def lookup_accept(logits, m_in, block, n_draft, positions, ids, prompt_mask, gen, lens, finished, emitted, n_new, ngram_size,
                  eos_token_id=None, pad_token_id=None, pos_offset=0, pos_max=None):
    """The tail of a prompt-lookup verify step for B samples, one launch, everything in place (mmgl_lookup_accept in
    include/mmgl_hip.h states the accept and the draft rule):
      logits [B*m_in, V] bf16 / fp32 (unit column stride): m_in = 1 -- the prefill's row per sample -- or K + 1, the rows of `block`;
      block int64 [B, K+1], n_draft int32 [B]: the inputs of those rows as the previous call wrote them, replaced by the next
      step's; positions int64 [B, K+1]: the next block's position ids = min(valid prompt tokens + pos_offset + gen - 1 + i, pos_max);
      ids int64 [B, T + n_new] (unit column stride): the prompt, then the new tokens, appended here; prompt_mask uint8 [B, T];
      gen, lens int32 [B], finished uint8 [B]: the rows' state; emitted int32 [B]: the tokens this call appended.
    K = block.shape[1] - 1 in 1..7, ngram_size N in 1..4, T + n_new <= 8192.  eos_token_id None: no end-of-sequence handling.
    A refused call leaves every tensor as it was.  Forward only; GPU only."""
    op = "lookup_accept"
    require_cuda(logits, block, n_draft, positions, ids, prompt_mask, gen, lens, finished, emitted)
    rows, V, code = _logits_operand(op, logits)
    m_in, n_new, N = int(m_in), int(n_new), int(ngram_size)
    if not torch.is_tensor(block) or block.dim() != 2 or block.dtype != torch.int64 or not block.is_contiguous():
        raise ValueError(f"{op}: block must be a dense int64 [B, K + 1] tensor")
    B, K = block.shape[0], block.shape[1] - 1
    if not 1 <= K <= MAX_LOOKUP_TOKENS:
        raise ValueError(f"{op}: K = {K} drafted tokens (1..{MAX_LOOKUP_TOKENS})")
    if not 1 <= N <= MAX_LOOKUP_NGRAM:
        raise ValueError(f"{op}: ngram_size = {N} (1..{MAX_LOOKUP_NGRAM})")
    if m_in not in (1, K + 1) or rows != B * m_in:
        raise ValueError(f"{op}: {rows} logits rows for B = {B}, m_in = {m_in} (1 for the prefill's row, else K + 1 = {K + 1})")
    dev = logits.device
    if block.device != dev or tuple(positions.shape) != (B, K + 1) or positions.dtype != torch.int64 or not positions.is_contiguous() or positions.device != dev:
        raise ValueError(f"{op}: block and positions must be dense int64 [{B}, {K + 1}] tensors on {dev}")
    if n_new < 1 or ids.dim() != 2 or ids.dtype != torch.int64 or ids.shape[0] != B or ids.shape[1] < n_new or ids.stride(1) != 1 or ids.device != dev:
        raise ValueError(f"{op}: ids must be an int64 [{B}, T + n_new] tensor with unit column stride on {dev}, n_new = {n_new} >= 1")
    T = ids.shape[1] - n_new
    if T + n_new > MAX_LOOKUP_HISTORY:
        raise ValueError(f"{op}: a history of T + n_new = {T + n_new} tokens (at most {MAX_LOOKUP_HISTORY})")
    if (prompt_mask.dtype not in (torch.uint8, torch.bool) or tuple(prompt_mask.shape) != (B, T) or (T > 0 and prompt_mask.stride(1) != 1)
            or prompt_mask.device != dev):
        raise ValueError(f"{op}: prompt_mask must be a uint8 [{B}, {T}] tensor with unit column stride on {dev}")
    for name, t, dt in (("n_draft", n_draft, torch.int32), ("gen", gen, torch.int32), ("lens", lens, torch.int32),
                        ("finished", finished, torch.uint8), ("emitted", emitted, torch.int32)):
        _state_vector(op, name, t, B, dt, dev)
    eos = -1 if eos_token_id is None else int(eos_token_id)
    pad = 0 if pad_token_id is None else int(pad_token_id)
    if eos_token_id is not None and (eos < 0 or pad_token_id is None or not 0 <= pad < V):
        raise ValueError(f"{op}: eos_token_id = {eos_token_id} needs a pad_token_id in [0, {V}), got {pad_token_id}")
    pos_max = 2 ** 31 - 1 if pos_max is None else int(pos_max)
    if pos_max < 0 or not 0 <= int(pos_offset) < 2 ** 20:
        raise ValueError(f"{op}: pos_offset = {pos_offset} / pos_max = {pos_max}")
    _lib.call("mmgl_lookup_accept", dict(bytes=float(rows) * V * logits.element_size()), ptr(logits), logits.stride(0), m_in, ptr(block), ptr(n_draft),
              ptr(positions), ptr(ids), ids.stride(0), ptr(_as_uint8(prompt_mask)), prompt_mask.stride(0) if T > 0 else 0, ptr(gen), ptr(lens),
              ptr(finished), ptr(emitted), B, T, n_new, V, K, N, eos, pad, int(pos_offset), pos_max, code, stream_ptr())


def beam_topk(logits, beam_score, num_beams, rows_in=None, out=None):
    """Per sample the 2W best continuations of its rows: logits [B*rows_in, V] (bf16 / fp32, unit column stride, any row stride) with
    rows_in = W = num_beams (the default) or 1 (the first step: the prefill's one row per sample); beam_score fp32 [B*rows_in].
    Returns (cand_score fp32 [B, 2W], cand_index int32 [B, 2W]) -- score = beam_score + log_softmax(logits) in fp32, sorted descending,
    index = r*V + v with r the row's slot in its sample; an exact tie goes to the lower index.  `out`: that pair, preallocated.  Two
    launches, no [rows, V] intermediate, no host synchronisation.  Forward only; GPU only."""
    require_cuda(logits, beam_score)
    W = _beams("beam_topk", num_beams)
    if logits.dim() != 2 or logits.stride(1) != 1 or beam_score.dtype != torch.float32 or beam_score.dim() != 1 or not beam_score.is_contiguous():
        raise ValueError(f"beam_topk: logits{tuple(logits.shape)}/{logits.stride()} [rows, V] with unit column stride, beam_score "
                         f"{beam_score.dtype}{tuple(beam_score.shape)} dense fp32 [rows]")
    rows, V = logits.shape
    if beam_score.shape[0] != rows or rows == 0:
        raise ValueError(f"beam_topk: {beam_score.shape[0]} scores for {rows} rows")
    rows_in = W if rows_in is None else int(rows_in)
    if rows_in not in (1, W) or rows % rows_in:
        raise ValueError(f"beam_topk: rows_in = {rows_in} must be 1 or num_beams = {W} and divide the {rows} rows")
    B = rows // rows_in
    if V < 2 * W:
        raise ValueError(f"beam_topk: V = {V} holds fewer than 2W = {2 * W} candidates")
    code = dtype_code(logits)
    if out is None:
        out = (torch.empty(B, 2 * W, dtype=torch.float32, device=logits.device), torch.empty(B, 2 * W, dtype=torch.int32, device=logits.device))
    cs, ci = out
    if (tuple(cs.shape) != (B, 2 * W) or tuple(ci.shape) != (B, 2 * W) or cs.dtype != torch.float32 or ci.dtype != torch.int32
            or not cs.is_contiguous() or not ci.is_contiguous() or cs.device != logits.device or ci.device != logits.device):
        raise ValueError(f"beam_topk: out must be dense (fp32, int32) [{B}, {2 * W}] tensors on {logits.device}")
    nbytes = _lib.lib().mmgl_beam_topk_workspace(rows, V, W)
    ws = _ws(nbytes, logits.device)
    _lib.call("mmgl_beam_topk", dict(bytes=float(rows) * V * logits.element_size()), ptr(logits), logits.stride(0), ptr(beam_score), ptr(cs), ptr(ci),
              ptr(ws), nbytes, B, rows_in, W, V, code, stream_ptr())
    return cs, ci


# ------------------------------------------------------------------------------------------ contrastive search (csrc/contrastive.hip)
CONTRASTIVE_CTX_CHUNK = 16              # context rows per workgroup of the streaming launch = mmgl_contrastive_chunk()


def contrastive_select(cand_hidden, ctx, ctx_valid, cand_score, cand_index, penalty_alpha, n_ctx, step, src, ids_col, vocab_size,
                       finished=None, eos_token_id=None, pad_token_id=None, hidden_out=None, selected=None, trace=None):
    """The ranking and the bookkeeping of one contrastive-search step for B samples x k candidates, one call, two launches, everything
    in place (mmgl_contrastive_select in include/mmgl_hip.h states the rule):
      cand_hidden [B*k, d] bf16 / fp32 (unit column stride): the candidates' last hidden rows, row b*k + c is candidate c of sample b;
      ctx [B, n_cap, d] in the same dtype (unit column stride), ctx_valid uint8 [B, n_cap]: the context rows [0, n_ctx) with
      ctx_valid set are ranked against; row n_ctx becomes the selected candidate's row and ctx_valid[:, n_ctx] = 1;
      cand_score fp32 / cand_index int32 [B, >= k] with a common row stride: the pair ops.beam_topk(logits, zeros, k, rows_in=1)
      returns -- the first k of each row are the candidates' log-probabilities and tokens;
      src int32 [B*k, >= step + 1] (BeamBook.src): column `step` := the selected candidate for the sample's k rows;
      ids_col int64 [B] (any stride: a column of the result): the selected token, or pad_token_id for a finished row;
      finished uint8 [B] with eos_token_id (None: no end-of-sequence handling).
    k = cand_hidden.shape[0] // B in 2..MAX_BEAMS, d a multiple of the 16-byte vector, 0 <= penalty_alpha <= 1.
    Returns (hidden_out [B, d] dense, selected int32 [B]) -- `hidden_out` / `selected` when given -- and, with trace=True or a
    preallocated triple, also (p, penalty, score) fp32 [B, k].  A refused call leaves every tensor as it was.  Forward only; GPU only."""
    op = "contrastive_select"
    require_cuda(cand_hidden, ctx, ctx_valid, cand_score, cand_index, src, ids_col, finished, hidden_out, selected)
    _no_grad_inputs(op, cand_hidden, ctx)
    if ctx.dim() != 3 or cand_hidden.dim() != 2 or ctx.shape[0] == 0 or cand_hidden.shape[0] % max(ctx.shape[0], 1):
        raise ValueError(f"{op}: cand_hidden{tuple(cand_hidden.shape)} [B*k, d] and ctx{tuple(ctx.shape)} [B, n_cap, d]")
    B, n_cap, d = ctx.shape
    k = cand_hidden.shape[0] // B
    if not 2 <= k <= MAX_BEAMS:
        raise ValueError(f"{op}: k = {k} candidates per sample (2..{MAX_BEAMS})")
    code = dtype_code(cand_hidden)
    dev = cand_hidden.device
    if (cand_hidden.shape[1] != d or ctx.dtype != cand_hidden.dtype or cand_hidden.stride(1) != 1 or ctx.stride(2) != 1 or ctx.device != dev
            or n_cap < 1):
        raise ValueError(f"{op}: incompatible cand_hidden{tuple(cand_hidden.shape)}/{cand_hidden.stride()} {cand_hidden.dtype} and "
                         f"ctx{tuple(ctx.shape)}/{ctx.stride()} {ctx.dtype}")
    if ctx_valid.dtype not in (torch.uint8, torch.bool) or tuple(ctx_valid.shape) != (B, n_cap) or ctx_valid.stride(1) != 1 or ctx_valid.device != dev:
        raise ValueError(f"{op}: ctx_valid must be a uint8 [{B}, {n_cap}] tensor with unit column stride on {dev}")
    if (cand_score.dtype != torch.float32 or cand_index.dtype != torch.int32 or cand_score.dim() != 2 or cand_score.shape != cand_index.shape
            or cand_score.shape[0] != B or cand_score.shape[1] < k or cand_score.stride() != cand_index.stride() or cand_score.stride(1) != 1
            or cand_score.device != dev or cand_index.device != dev):
        raise ValueError(f"{op}: cand_score / cand_index must be (fp32, int32) [{B}, >= {k}] tensors of one layout with unit column stride on {dev}")
    n_ctx, step, V = int(n_ctx), int(step), int(vocab_size)
    if not 0 <= n_ctx <= n_cap - 1:
        raise ValueError(f"{op}: n_ctx = {n_ctx} outside [0, n_cap - 1 = {n_cap - 1}]")
    if (src.dtype != torch.int32 or src.dim() != 2 or src.shape[0] != B * k or src.stride(1) != 1 or not 0 <= step < src.shape[1]
            or src.device != dev):
        raise ValueError(f"{op}: src must be an int32 [{B * k}, > step = {step}] view with unit column stride on {dev}")
    if ids_col.dtype != torch.int64 or tuple(ids_col.shape) != (B,) or ids_col.device != dev:
        raise ValueError(f"{op}: ids_col must be an int64 [{B}] view on {dev}")
    alpha = float(penalty_alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"{op}: penalty_alpha = {penalty_alpha} outside [0, 1]")
    eos = -1 if eos_token_id is None else int(eos_token_id)
    pad = 0 if pad_token_id is None else int(pad_token_id)
    if V < k:
        raise ValueError(f"{op}: vocab_size = {vocab_size} holds fewer than k = {k} candidates")
    if eos_token_id is not None:
        if not 0 <= eos < V or pad_token_id is None or not 0 <= pad < V:
            raise ValueError(f"{op}: eos_token_id = {eos_token_id} needs a pad_token_id, both in [0, {V}), got {pad_token_id}")
        _state_vector(op, "finished", finished, B, torch.uint8, dev)
    if hidden_out is None:
        hidden_out = torch.empty(B, d, dtype=cand_hidden.dtype, device=dev)
    if tuple(hidden_out.shape) != (B, d) or hidden_out.dtype != cand_hidden.dtype or not hidden_out.is_contiguous() or hidden_out.device != dev:
        raise ValueError(f"{op}: hidden_out must be a dense {cand_hidden.dtype} [{B}, {d}] tensor on {dev}")
    if selected is None:
        selected = torch.empty(B, dtype=torch.int32, device=dev)
    _state_vector(op, "selected", selected, B, torch.int32, dev)
    if trace is True:
        trace = tuple(torch.empty(B, k, dtype=torch.float32, device=dev) for _ in range(3))
    if trace:
        if len(trace) != 3 or any(not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (B, k) or not t.is_contiguous()
                                  or t.device != dev for t in trace):
            raise ValueError(f"{op}: trace must be three dense fp32 [{B}, {k}] tensors on {dev}")
    tr = tuple(trace) if trace else (None, None, None)
    nbytes = _lib.lib().mmgl_contrastive_workspace(B, k, n_cap)
    ws = _ws(nbytes, dev)
    _lib.call("mmgl_contrastive_select", dict(bytes=float(B) * (n_ctx + k) * d * ctx.element_size()), ptr(cand_hidden), cand_hidden.stride(0),
              ptr(ctx), ctx.stride(1), ctx.stride(0), ptr(_as_uint8(ctx_valid)), ctx_valid.stride(0), n_cap, ptr(cand_score), ptr(cand_index),
              cand_score.stride(0), alpha, n_ctx, step, ptr(src), src.stride(0), ptr(ids_col), ids_col.stride(0),
              ptr(finished) if eos_token_id is not None else None, eos, pad, ptr(hidden_out), ptr(selected), ptr(tr[0]), ptr(tr[1]), ptr(tr[2]),
              ptr(ws), nbytes, B, k, d, V, code, stream_ptr())
    return (hidden_out, selected, tr) if trace else (hidden_out, selected)


def _logits_operand(op, logits):
    """(rows, V, dtype code) of logits [rows, V]: unit column stride, not empty, V <= 131072 (sample_tokens, process_logits)."""
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[0] == 0 or logits.shape[1] == 0:
        raise ValueError(f"{op}: logits{tuple(logits.shape)}/{logits.stride()} must be [rows, V] with unit column stride")
    rows, V = logits.shape
    code = dtype_code(logits)
    if V > 131072:
        raise ValueError(f"{op}: V = {V} (at most 131072)")
    return rows, V, code


def sample_tokens(logits, u, temperature=1.0, top_k=0, top_p=1.0, finished=None, eos_token_id=None, pad_token_id=None, out=None,
                  return_kept=False):
    """The selection step of generate(do_sample=True) in one launch (mmgl_sample_tokens): transformers' temperature -> top-k -> top-p
    warpers (min_tokens_to_keep = 1) and the draw, per row of logits [rows, V] (bf16 / fp32, unit column stride, any row stride;
    V <= 131072).  u: fp32 [rows, n_draws] (or [rows]: one draw) in [0, 1), n_draws <= 8 draws per row on one kept set.
    With x = logit / temperature in fp32: top_k (0 or >= V: off) keeps v iff fewer than top_k tokens have x > x_v; top_p (1: off)
    keeps a survivor v iff the softmax mass of the survivors with x > x_v is < top_p.  Ties at either boundary are all kept, the
    largest logit always is.  The token is the smallest kept v, in vocabulary index order, whose running mass exceeds u * Z_K.
    finished (uint8 / bool [rows * n_draws], updated in place) with eos_token_id / pad_token_id: a finished draw gets pad_token_id, a
    draw that returns eos_token_id becomes finished.  `out`: an int64 view of rows * n_draws elements with any positive stride (a
    column of the ids tensor).  Returns the tokens (int64 [rows * n_draws], or `out`), with return_kept=True also the size of each
    row's kept set (int32 [rows]).  No [rows, V] intermediate, no host synchronisation, bitwise reproducible.  Forward only; GPU only."""
    require_cuda(logits, u, finished, out)
    rows, V, code = _logits_operand("sample_tokens", logits)
    if u.dtype != torch.float32 or u.dim() not in (1, 2) or u.shape[0] != rows or not u.is_contiguous() or u.device != logits.device:
        raise ValueError(f"sample_tokens: u {u.dtype}{tuple(u.shape)} must be a dense fp32 [{rows}, n_draws] tensor on {logits.device}")
    n_draws = 1 if u.dim() == 1 else u.shape[1]
    if not 1 <= n_draws <= MAX_BEAMS:
        raise ValueError(f"sample_tokens: {n_draws} draws per row (1..{MAX_BEAMS})")
    temperature, top_k, top_p = float(temperature), int(top_k), float(top_p)
    if not (0.0 < temperature < float("inf")):
        raise ValueError(f"sample_tokens: temperature = {temperature} must be positive and finite")
    if top_k < 0:
        raise ValueError(f"sample_tokens: top_k = {top_k} must not be negative (0: off)")
    if not (0.0 < top_p <= 1.0):
        raise ValueError(f"sample_tokens: top_p = {top_p} outside (0, 1]")
    n = rows * n_draws
    if finished is not None:
        finished = _as_uint8(finished)
        if finished.dtype != torch.uint8 or tuple(finished.shape) != (n,) or not finished.is_contiguous() or finished.device != logits.device:
            raise ValueError(f"sample_tokens: finished must be a dense uint8 / bool [{n}] tensor on {logits.device}")
        if eos_token_id is not None and pad_token_id is None:
            raise ValueError("sample_tokens: eos_token_id needs a pad_token_id")
    elif eos_token_id is not None:
        raise ValueError("sample_tokens: eos_token_id needs the finished buffer")
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=logits.device)
    elif out.dtype != torch.int64 or out.dim() != 1 or out.shape[0] != n or (n > 1 and out.stride(0) < 1) or out.device != logits.device:
        raise ValueError(f"sample_tokens: out {out.dtype}{tuple(out.shape)}/{out.stride()} must be an int64 [{n}] view with a positive "
                         f"stride on {logits.device}")
    kept = torch.empty(rows, dtype=torch.int32, device=logits.device) if return_kept else None
    _lib.call("mmgl_sample_tokens", dict(bytes=float(rows) * V * logits.element_size()), ptr(logits), logits.stride(0), ptr(u), ptr(out),
              max(out.stride(0), 1), ptr(finished), ptr(kept), rows, n_draws, V, temperature, top_k, top_p,
              -1 if eos_token_id is None else int(eos_token_id), 0 if pad_token_id is None else int(pad_token_id), code, stream_ptr())
    return (out, kept) if return_kept else out


MAX_HISTORY, MAX_BAN = 8192, 64


def process_logits(logits, history, history_valid=None, n_masked=None, repetition_penalty=1.0, no_repeat_ngram_size=0, ban=None):
    """The logits processors of generate() in one launch (mmgl_logits_process), in place on logits [rows, V] (bf16 / fp32, unit column
    stride, any row stride; V <= 131072): transformers' RepetitionPenalty -> NoRepeatNGram -> (MinNewTokensLength, SuppressTokens as
    `ban`) chain.  history: int64 [rows, L] (unit column stride, ANY row stride -- ids[::R] serves R draws that share a prompt;
    L <= 8192; None: no history), the tokens in front of the column being chosen.  history_valid: bool / uint8 [rows, >= n_masked]
    over the first n_masked columns (default: all of its columns); a column it marks 0 is not part of the history, columns from
    n_masked on always are.  Per row, on its history h[0..L'):
      repetition_penalty p (1: off)     x[t] = x[t] * p if x[t] < 0 else x[t] / p, once per distinct token t, fp32, rounded once
      no_repeat_ngram_size n (0: off)   x[h[i+n-1]] = -inf wherever h[i .. i+n-1) equals the last n-1 tokens
      ban (int32 device tensor [n_ban <= 64], None: none)   x[t] = -inf
    in this order (-inf wins).  A token outside [0, V) is never an address.  Every other element keeps its bits.  Returns `logits`.
    Nothing is launched when everything is off.  No host synchronisation, bitwise reproducible.  Forward only; GPU only."""
    require_cuda(logits, history, history_valid, ban)
    rows, V, code = _logits_operand("process_logits", logits)
    p, n = float(repetition_penalty), int(no_repeat_ngram_size)
    if not (0.0 < p < float("inf")):
        raise ValueError(f"process_logits: repetition_penalty = {repetition_penalty} must be positive and finite")
    if n < 0:
        raise ValueError(f"process_logits: no_repeat_ngram_size = {no_repeat_ngram_size} must not be negative (0: off)")
    L = 0
    if history is not None:
        if (history.dtype != torch.int64 or history.dim() != 2 or history.shape[0] != rows or (history.shape[1] > 1 and history.stride(1) != 1)
                or history.stride(0) < 0 or history.device != logits.device):
            raise ValueError(f"process_logits: history {history.dtype}{tuple(history.shape)}/{history.stride()} must be an int64 "
                             f"[{rows}, L] view with unit column stride on {logits.device}")
        L = history.shape[1]
        if L > MAX_HISTORY:
            raise ValueError(f"process_logits: history of {L} columns (at most {MAX_HISTORY})")
    if history_valid is None:
        if n_masked not in (None, 0):
            raise ValueError(f"process_logits: n_masked = {n_masked} without history_valid")
        n_masked = 0
    else:
        history_valid = _as_uint8(history_valid)
        if (history_valid.dtype != torch.uint8 or history_valid.dim() != 2 or history_valid.shape[0] != rows
                or (history_valid.shape[1] > 1 and history_valid.stride(1) != 1) or history_valid.stride(0) < 0
                or history_valid.device != logits.device):
            raise ValueError(f"process_logits: history_valid {history_valid.dtype}{tuple(history_valid.shape)}/{history_valid.stride()} must "
                             f"be a bool / uint8 [{rows}, n_masked] view with unit column stride on {logits.device}")
        n_masked = history_valid.shape[1] if n_masked is None else int(n_masked)
        if not 0 <= n_masked <= min(L, history_valid.shape[1]):
            raise ValueError(f"process_logits: n_masked = {n_masked} outside [0, min(history columns {L}, mask columns "
                             f"{history_valid.shape[1]})]")
        if n_masked == 0:
            history_valid = None
    n_ban = 0
    if ban is not None:
        if ban.dtype != torch.int32 or ban.dim() != 1 or not ban.is_contiguous() or ban.device != logits.device:
            raise ValueError(f"process_logits: ban {ban.dtype}{tuple(ban.shape)} must be a dense int32 [n_ban] tensor on {logits.device}")
        n_ban = ban.shape[0]
        if n_ban > MAX_BAN:
            raise ValueError(f"process_logits: {n_ban} banned tokens (at most {MAX_BAN})")
    if n_ban == 0 and (L == 0 or (p == 1.0 and n == 0)):
        return logits
    _lib.call("mmgl_logits_process", dict(bytes=float(rows) * (L * 8 + (L + n_ban) * logits.element_size())), ptr(logits), logits.stride(0),
              ptr(history) if L else None, history.stride(0) if L else 0, ptr(history_valid),
              history_valid.stride(0) if history_valid is not None else 0, n_masked, L, ptr(ban) if n_ban else None, n_ban, rows, V, p, n,
              code, stream_ptr())
    return logits


def guidance_logits(logits, batch, guidance_scale):
    """Neighbor guidance of generate(guidance_scale=g) in one launch (mmgl_guidance_logits), in place on logits [2 * batch, V] (bf16 /
    fp32, unit column stride, any row stride; V <= 131072).  Rows b and batch + b are a pair: the logits with neighbors and those of
    the same tokens without the gated layers.  With lc / lu their log_softmax in fp32 (NaN counts as -inf), row b becomes
    lu + g * (lc - lu), rounded once -- transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor.  A conditional -inf stays -inf,
    an unconditional -inf under a finite conditional gives lc; a row without any finite logit is outside the contract.  Rows
    batch .. 2 batch - 1 and every other byte keep their bits.  Returns the guided rows, the view logits[:batch].  No [rows, V]
    intermediate, no host synchronisation, bitwise reproducible.  Forward only; GPU only."""
    require_cuda(logits)
    rows, V, code = _logits_operand("guidance_logits", logits)
    batch, g = int(batch), float(guidance_scale)
    if batch < 1 or rows != 2 * batch:
        raise ValueError(f"guidance_logits: logits of {rows} rows for batch = {batch} (the conditional rows, then the unconditional ones: "
                         f"{2 * batch} rows)")
    if not (0.0 <= g < float("inf")):
        raise ValueError(f"guidance_logits: guidance_scale = {guidance_scale} must be finite and not negative")
    if logits.stride(0) < V:
        raise ValueError(f"guidance_logits: logits{tuple(logits.shape)}/{logits.stride()}: the row stride must be at least V")
    _lib.call("mmgl_guidance_logits", dict(bytes=float(batch) * V * logits.element_size() * 7), ptr(logits), logits.stride(0), batch, V, g,
              code, stream_ptr())
    return logits[:batch]


class BeamBook:
    """The bookkeeping state of a beam search over B samples x W beams, all on the device (ops.beam_advance moves it one step):
      tokens int64 / parents int32 / beam_score fp32 [B*W]   the running beams of the last step (slot order = candidate order)
      src        two int32 [B*W, n_cap] parent tables (ops.attn_decode_beam reads `src`, the current one): src[b*W + w, j] is the slot
                 that held the ancestor of running beam (b, w) at decode step j -- the row of the tail buffer whose column j is its key.
                 Every column starts as the identity (a row reads its own column until a later step has reordered it).
      pool       two sets (score fp32, length int32, ancestry int32 [B*W, n_cap], last token int64) of the W best finished
                 hypotheses per sample, sorted descending; length 0 / score -inf mark an empty slot
      done       int32 [B]: the sample's pool is closed (the early-stop heuristic was met)
      cur        which of the two buffers is current"""

    def __init__(self, batch_size, num_beams, n_cap, device):
        B, W, C = int(batch_size), _beams("BeamBook", num_beams), max(int(n_cap), 1)
        self.B, self.W, self.n_cap, self.cur = B, W, C, 0
        i32 = dict(dtype=torch.int32, device=device)
        self.tokens = torch.zeros(B * W, dtype=torch.int64, device=device)
        self.parents = torch.zeros(B * W, **i32)
        self.beam_score = torch.zeros(B * W, dtype=torch.float32, device=device)
        ident = (torch.arange(B * W, **i32) % W)[:, None].expand(B * W, C)
        self._src = [ident.clone(), ident.clone()]
        self._pool = [(torch.full((B * W,), float("-inf"), dtype=torch.float32, device=device), torch.zeros(B * W, **i32),
                       torch.zeros(B * W, C, **i32), torch.zeros(B * W, dtype=torch.int64, device=device)) for _ in range(2)]
        self.done = torch.zeros(B, **i32)

    @property
    def src(self):
        return self._src[self.cur]

    @property
    def pool(self):
        return self._pool[self.cur]


def beam_advance(cand_score, cand_index, book, n_cols, vocab_size, eos_token_id=None, last_step=False, early_stopping=False,
                 length_divisor=1.0):
    """One step of beam-search bookkeeping in one launch (mmgl_beam_advance): the sorted candidates of ops.beam_topk (fp32 / int32
    [B, 2W]) become book's next state -- the running beams (the first W candidates whose token is not eos_token_id), the parent table
    (new[w, :n_cols-1] = old[parent, :n_cols-1], new[w, n_cols-1] = parent; n_cols = the step index = the tail columns the parents
    own) and the pool: a candidate among the first W that is EOS, or any of them at last_step, enters with score / length_divisor
    (pass float32((step + 1) ** length_penalty)), length n_cols + 1, its ancestry row and its token, unless the sample is frozen
    (book.done, or early_stopping with a pool that was already full).  Flips book.cur; no host synchronisation.  Returns book."""
    require_cuda(cand_score, cand_index, book.tokens)
    B, W = book.B, book.W
    if (tuple(cand_score.shape) != (B, 2 * W) or tuple(cand_index.shape) != (B, 2 * W) or cand_score.dtype != torch.float32
            or cand_index.dtype != torch.int32 or not cand_score.is_contiguous() or not cand_index.is_contiguous()):
        raise ValueError(f"beam_advance: candidates must be dense (fp32, int32) [{B}, {2 * W}] tensors, got {cand_score.dtype}"
                         f"{tuple(cand_score.shape)} / {cand_index.dtype}{tuple(cand_index.shape)}")
    n_cols = int(n_cols)
    if not 0 <= n_cols <= book.n_cap:
        raise ValueError(f"beam_advance: n_cols = {n_cols} outside [0, {book.n_cap}]")
    if int(vocab_size) < 2 * W:
        raise ValueError(f"beam_advance: V = {vocab_size} holds fewer than 2W = {2 * W} candidates")
    if early_stopping not in (True, False):
        raise ValueError(f"beam_advance: early_stopping = {early_stopping!r} (True or False)")
    if not float(length_divisor) > 0.0:
        raise ValueError(f"beam_advance: length_divisor = {length_divisor} must be positive")
    old, new = book.cur, 1 - book.cur
    po, pn = book._pool[old], book._pool[new]
    _lib.call("mmgl_beam_advance", None, ptr(cand_score), ptr(cand_index), ptr(book.tokens), ptr(book.parents), ptr(book.beam_score),
              ptr(book._src[old]), ptr(book._src[new]), book.n_cap, ptr(po[0]), ptr(pn[0]), ptr(po[1]), ptr(pn[1]), ptr(po[2]), ptr(pn[2]),
              ptr(po[3]), ptr(pn[3]), ptr(book.done), B, W, int(vocab_size), n_cols, -1 if eos_token_id is None else int(eos_token_id),
              int(bool(last_step)), int(bool(early_stopping)), float(length_divisor), stream_ptr())
    book.cur = new
    return book
