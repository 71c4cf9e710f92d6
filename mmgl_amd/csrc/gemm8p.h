// Internal interface of the persistent 256x256 ping-pong GEMM (gemm8p.hip), used by gemm.hip's dispatchers.
#pragma once
#include "common.h"

// act codes: 0 none, 1 relu, 2 gelu (erf), 3 quick_gelu, 4 gelu (tanh)  (= mmgl_activation_fwd's)
// row strides ldx / ldw / ldy in elements (resid and zmask share ldy)
bool gemm8p_supported(int M, int N, int K, int ldx, int ldw, int ldy);
// 256x256 output tiles from which the kernel runs without K splits (gemm8p_plan) and takes a GEMM whose caller brings no
// K-split scratch (nt_route, gemm.hip)
constexpr int GEMM8P_MIN_TILES = 160;
int gemm8p_splits(int M, int N, int K);      // K splits for few-tile outputs (0 = none)
size_t gemm8p_split_bytes(int M, int N, int K);   // fp32 partial tiles of the K-split path (caller's scratch)
int launch_gemm8p(const bf16* X, int ldx, const bf16* W, int ldw, bf16* Y, int ldy, const bf16* bias, const bf16* resid,
                  const bf16* zmask, int M, int N, int K, int act, float scale, hipStream_t st, float* part = nullptr,
                  size_t part_bytes = 0, unsigned* bits_out = nullptr, const unsigned* bits_in = nullptr);
// Per-row-tile K extent (mmgl_gemm_nt_rowk): row tiles tm < cdiv(m_full, 256) contract over K ("long" tiles), the others over the
// first K_short columns only -- the caller knows that X[m_full.., K_short..K) is zero (or never written).  ONE launch, no K splits,
// every element's K walk starts at 0 and ascends: dropping a zero tail leaves the fp32 accumulator where the full walk leaves it.
// Plain epilogue (no bias / activation / mask / residual), no scratch, the persistent kernel at any tile count.
int launch_gemm8p_rowk(const bf16* X, int ldx, const bf16* W, int ldw, bf16* Y, int ldy, int M, int N, int K, int K_short, int m_full,
                       hipStream_t st);
// Static schedule of that launch: the it-th work item of workgroup wg of G, as a virtual id -- v < L: long tile v, else short tile
// v - L -- or -1 when the workgroup has no it-th item.  q = K / K_short short tiles weigh one long one.  Long tiles go round-robin
// first (round `it`, slot wg); the r = L % G workgroups of the last, partial long round are then one long tile ahead, so the other
// G - r take up to q short tiles each (round-robin among themselves) before the rest of the short tiles goes round-robin over all G:
// no workgroup's K steps exceed the mean by more than one long tile.  (Plain round-robin over "long first" hands the first short
// tiles to the workgroups that already hold the extra long one: 14 against 11 units for 8 workgroups at 776 + 504 tiles on 256.)
__host__ __device__ inline int gemm8p_rowk_item(int G, int L, int S, int q, int wg, int it) {
    const int r = L % G, nl = L / G + (wg < r ? 1 : 0);
    if (it < nl) return it * G + wg;
    const int j = it - nl;
    long long s;
    if (r > 0 && wg >= r) s = j < q ? (long long)j * (G - r) + (wg - r) : (long long)q * (G - r) + (long long)(j - q) * G + wg;
    else s = (r > 0 ? (long long)q * (G - r) : 0) + (long long)j * G + wg;
    return s < S ? L + (int)s : -1;
}

// ReLU mask as bits: 8 KiB per 256x256 output tile ([tile][8 waves][64 lanes][4 dwords], lane-private: the kernel that applies
// them has the same tile -> lane mapping as the one that wrote them); written by the act = 1 epilogue, applied by the plain one
inline size_t gemm8p_bits_bytes(int M, int N) { return (size_t)cdiv(M, 256) * cdiv(N, 256) * 8192; }

// weight gradient on the same structure (gemm8p_tt.hip): Out[RB][RA] = scale * sum_m B[m][rb] A[m][ra], both operands k-major
int gemm8p_tt_splits(int RA, int RB, int M);
int launch_gemm8p_tt(const bf16* A, int lda, const bf16* B, int ldb, bf16* Out, float* part, int RA, int RB, int M, int nsplit, float scale,
                     int accumulate, hipStream_t st);

// 128x128 tiles, two workgroups per CU (gemm_mid.hip): few-tile outputs.  Same epilogue contract as launch_gemm8p.
bool gemm_mid_supported(int M, int N, int K, int ldx, int ldw, int ldy);
int launch_gemm_mid(const bf16* X, int ldx, const bf16* W, int ldw, bf16* Y, int ldy, const bf16* bias, const bf16* resid, const bf16* zmask,
                    int M, int N, int K, int act, float scale, hipStream_t st);
