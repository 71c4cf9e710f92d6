// Internal interface of selfattn32.hip (bf16, head_dim 64 / 128 flash attention on 32x32x16 MFMAs); called by the C ABI entry
// points in selfattn.hip.  Not part of the exported ABI (hidden visibility).
#pragma once
#include "common.h"

#define SA32_HIDDEN __attribute__((visibility("hidden")))

// THE choice between the 32x32 kernels and the 16x16 ones of selfattn.hip: bf16, head_dim 64 / 128, Tk <= 4096 key rows
SA32_HIDDEN bool sa32_supported(int dtype, int D, int Tk);

// causal (+ P prefix keys) forward; same argument meaning as mmgl_selfattn_prefix_fwd.  G > 1: grouped-query attention, k / v hold
// H / G heads and query head h reads head h / G (mmgl_selfattn_gqa_fwd); G = 1 launches the multi-head kernels
SA32_HIDDEN int sa32_fwd(const void* q, const void* k, const void* v, const uint8_t* valid, void* out, float* lse, int B, int H, int T,
                         int P, int D, int ldq, int ldk, hipStream_t st, int G = 1);
// live key tiles only (mmgl_selfattn_tiles_fwd / _bwd): bf16, head_dim 64, T a multiple of 64, no prefix, multi-head.  k, v are
// compact [64 ntc, ldk]: the 64-key tiles with a valid key, `tiles` [B, T / 64] maps a key tile to its compact tile (-1: dead);
// dq, dk, dv are dense [B, T, ldg | ldgk] -- or, with dest [B, T / 64] (a permutation of the batch's tiles), [B * T, ld] buffers that
// take the rows of tile (b, j) at rows 64 dest[b][j] .. + 63 (dk / dv rows from dkv_rows on are not stored)
SA32_HIDDEN int sa32_tiles_fwd(const void* q, const void* k, const void* v, const uint8_t* valid, const int* tiles, void* out, float* lse,
                               int B, int H, int T, int ntc, int ldq, int ldk, hipStream_t st);
SA32_HIDDEN int sa32_tiles_bwd(const void* dout, const void* q, const void* k, const void* v, const void* out, const float* lse,
                               const uint8_t* valid, const int* tiles, void* dq, void* dk, void* dv, float* delta, int B, int H, int T,
                               int ntc, int ldq, int ldk, int ldg, int ldgk, hipStream_t st, const int* dest = nullptr, int dkv_rows = 0);
// packed bidirectional forward; same argument meaning as mmgl_encattn_fwd
SA32_HIDDEN int sa32_enc_fwd(const void* q, const void* k, const void* v, const int* cu, void* out, int nseq, int H, int D, int ld_in,
                             int ld_out, int max_len, int q_rows, hipStream_t st);
// backward: the dQ kernel (also writes delta [B,H,T] = rowsum(dO * O)), then the dK / dV kernel (reads delta).
// Argument meaning as mmgl_selfattn_prefix_bwd: ldg / ldgk are the row strides of dq / dk, dv.  G > 1: k / v hold H / G heads; dk / dv
// are still written per QUERY head ([B, Tk, >= H*D] rows: the caller's scratch, folded over each group afterwards).
SA32_HIDDEN int sa32_bwd(const void* dout, const void* q, const void* k, const void* v, const void* out, const float* lse,
                         const uint8_t* valid, void* dq, void* dk, void* dv, float* delta, int B, int H, int T, int P, int D, int ldq,
                         int ldk, int ldg, int ldgk, hipStream_t st, int G = 1);
