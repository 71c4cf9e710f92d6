// Decode-step kernels: the weight-streaming GEMM for M = batch rows and single-query attention over a key/value cache.
// Reached only from the generation path (ops.decode_linear / ops.attn_decode / ops.rope_kv_append); no training or prefill caller routes here.
//
// mmgl_gemm_skinny, bf16 (skinny_mfma_kernel).  Y[M,N] = epi(X[M,K] . W[N,K]^T), 1 <= M <= 64.  The step is bound by the weight bytes:
//   * W is the MFMA A operand (as everywhere in this library) and goes HBM -> VGPR as 16-byte lane loads in A-fragment shape, two per lane
//     and 64-wide K unit ("pair"): lane (i, g) reads W[n0 + i][64 p + 16 g .. + 15], so the four lane groups of a row cover one whole
//     128-byte line.  v_mfma_f32_16x16x32_bf16 accepts any k order that A and B share: MFMA t of a pair contracts k = 16 g + 8 t + (0..7).
//     No LDS round trip for W; a ring of DW pairs per lane is in flight (issued DW iterations ahead of their use).
//   * the K range is dealt over the workgroup's 4 waves pair by pair (slot s takes pairs s, s + NS, ...).  Each wave stages only the x
//     columns of its own pairs: whole 128-byte lines (8 rows x 8 lanes x 16 B per instruction) into an XOR-swizzled [rows][8 x 16 B]
//     LDS image, read back as B fragments with ds_read_b128.  x is at most 1 MiB and stays in L2.
//   * a workgroup owns 16 weight rows.  Where N / 16 would leave CUs without work (N = 2048: 128 workgroups on 256 CUs) it owns 8 (HALF):
//     lanes i >= 8 then hold the same 8 rows at the wave's SECOND K slot, and every A fragment feeds two MFMAs -- one against the x
//     of slot 0 (rows 0..7 of that accumulator are the result), one against the x of slot 1 (rows 8..15) -- so no lane loads a byte
//     twice and none idles.
//   * the per-slot fp32 partials are folded through LDS in slot order by the epilogue threads: deterministic, no atomics, no
//     inter-workgroup hand-off.  Epilogue as mmgl_gemm_nt: act((acc + bias) * scale) + residual, ldy free (rows go straight into the cache).
// Any dtype / alignment the MFMA kernel does not take (fp32: a correctness path; K % 64, N % 8, unaligned rows) runs on
// skinny_generic_kernel: one wave per output column, 8 rows of x per wave, fp32 accumulation, same epilogue.
//
// mmgl_gemm_skinny_lora.  The same two kernels with a rank-r term in fp32 in front of the epilogue (a trailing parameter pack E...: empty for
// mmgl_gemm_skinny -- one kernel argument and the same instructions as before -- or one SkLora):
//   * stage 1, lora_t_kernel: t[M, r] = x . A^T in fp32 into the caller's workspace, one wave per (adapter row, 8 rows of x), 16/32-byte
//     lane loads over K where the rows are aligned, a fixed butterfly per sum.  A is r K elements (64 KB at r = 16, K = 2048).
//   * stage 2: the thread that folds output (m, n) adds lora_scale * sum_j t[m, j] B[n, j] to the folded sum -- r FMAs from the
//     L2-resident t and one row of B -- then bias, scale, activation and residual as before.  The adapter never touches W, and the
//     term is never rounded to the storage type on its own (ops.lora_linear keeps it in the fp32 accumulators likewise).
//
// mmgl_attn_decode_fwd (attn_decode_kernel).  One query row per (batch, head) against S keys addressed in place in the [B, S, H*D] cache
// rows.  D / VEC lanes share a key (16-byte K and V loads straight to registers, VEC = 8 bf16 / 4 fp32), so a wave covers 64 VEC / D
// keys per instruction and the 4 waves of the workgroup interleave key blocks; U blocks are loaded before the first is used.  Every lane
// group keeps its own online-softmax state (max, sum, partial O) in fp32; the states are merged by a fixed butterfly inside the wave and
// in wave order through LDS.  A masked key scores -FLT_MAX: with a valid key in the row it weighs exp(-FLT_MAX - max) = 0, and a row of
// masked keys only has every weight exp(0) = 1 -- the uniform distribution of the reference's finfo.min clamp.
//
// mmgl_attn_decode_relbias_fwd (attn_decode_relbias_kernel).  The same kernel for the T5 decoder's cached self-attention: raw scores, no
// mask, plus a learned fp32 word per (head, distance to the query) read from bias rows the caller gathered once.
//
// mmgl_attn_decode_gqa_fwd (attn_decode_gqa_kernel).  The same kernel over a cache of Hkv <= H key/value heads: one workgroup per (sample,
// key/value head, block of at most 8 of the G = H / Hkv query heads that read it).  The decode step is a memory-bound read of the cache,
// so each 16-byte K / V load is issued once and scored against every query head of the block from registers; G > 8 takes further blocks.
// The keys of a sample are not split over workgroups (no flash-decoding: DESIGN.md 4.11).
//
// mmgl_attn_decode_beam_fwd (attn_decode_beam_kernel).  Beam search: the W <= 8 hypotheses of a sample share its prefix keys (one read,
// W queries from registers, as the grouped-query kernel does for its group) and differ only in the few keys generated so far, which a
// per-row int32 parent table addresses in a [B*W, n_cap, 2d] tail buffer.  No cache row is copied when the beams are reordered.
//
// mmgl_attn_decode_block_fwd (attn_decode_block_kernel).  Prompt-lookup decoding: m <= 8 new tokens per sample in one step, causal among
// themselves, against a cache whose length differs per sample (int32 len[b] on the device).  The beam kernel's prefix loop bounded by
// len[b], then the m new keys from the projection's output, which the same launch files at cache columns len[b] .. len[b] + m - 1.
//
// mmgl_kv_quantize / mmgl_attn_decode_q8_fwd (kv_quantize_kernel, attn_decode_q8_kernel).  The FP8 key/value cache: cache rows of OCP
// e4m3fn codes with one power-of-two scale per (sample, column, key-or-value, head).  attn_decode_kernel over 16 codes per lane and
// 16-byte load, the scales folded into the dot product and the softmax weight; the new token's key and value come dense, count
// unquantised, and are filed as codes by the same launch.
//
// mmgl_attn_decode_gqa_q8_fwd (attn_decode_gqa_q8_kernel).  The FP8 cache of the Llama-family LM: code rows of Hkv <= H key/value heads.
// attn_decode_q8_kernel with the workgroups of attn_decode_gqa_kernel -- one per (sample, key/value head, block of at most 4 query heads
// of its group): a 16-byte load of codes is issued and dequantised once and scored against the block's query heads from registers.
// Every block folds the new token unquantised; block 0 of a group alone files it as codes.
//
// mmgl_weight_quantize / mmgl_gemm_skinny_w8 (weight_quantize_kernel, skinny_w8_mfma_kernel, skinny_w8_generic_kernel).  FP8 frozen
// weights: a weight [N, K] as e4m3fn codes with one power-of-two scale per row, quantised once, and the skinny GEMM on the codes --
// skinny_mfma_kernel's structure over a K unit of 128 codes (one 128-byte line per weight row), the codes converted to bf16 fragments
// in registers, the row's scale applied to the folded fp32 sum.
//
// mmgl_rope_kv_append (rope_kv_append_kernel).  The new token's q | k | v row: q rotated in place, k rotated into the token's cache column,
// v copied there -- one launch where separate projections and rotations would take four (the step is launch-bound).
#include "common.h"
#include "attn_common.h"      // make_rsrc / OOB: hardware-bounds-checked buffer loads
#include <float.h>

namespace {

constexpr int SK_WAVES = 4;
constexpr int SK_THREADS = SK_WAVES * WAVE;

template <typename T> struct SkArgs {
    const T* X; const T* W; const T* bias; const T* resid; T* Y;
    int ldx, ldw, ldy, M, N, K, act;
    float scale;
};

template <typename T>
__device__ __forceinline__ void sk_store(const SkArgs<T>& a, int m, int n, float v) {
    if (a.bias) v += Elem<T>::to_f(a.bias[n]);
    v *= a.scale;
    if (a.act == MMGL_ACT_RELU) v = fmaxf(v, 0.f);
    const size_t o = (size_t)m * a.ldy + n;
    if (a.resid) v += Elem<T>::to_f(a.resid[o]);
    a.Y[o] = Elem<T>::from_f(v);
}

// the extra term of the epilogue, lora_scale * t[m, :] . B[n, :]: the trailing kernel argument of mmgl_gemm_skinny_lora.  The kernels take
// it as a parameter pack E...: empty for mmgl_gemm_skinny, whose instantiations keep their one argument and their code.
template <typename T> struct SkLora {
    const T* B; const float* t;
    int ldb, r, vec;                               // vec: r % 8 == 0 and the rows of B and t are aligned for 8-element loads
    float ls;
};

template <typename T> __device__ __forceinline__ float sk_extra(int, int) { return 0.f; }
template <typename T> __device__ __forceinline__ float sk_extra(int m, int n, const SkLora<T>& e) {
    typedef typename Elem<T>::v8 V8;
    const float* tr = e.t + (size_t)m * e.r;
    const T* br = e.B + (size_t)n * e.ldb;
    float s = 0.f;
    if (e.vec) {
        for (int j = 0; j < e.r; j += 8) {
            const V8 bv = *(const V8*)(br + j);
            const f32x4 t0 = *(const f32x4*)(tr + j), t1 = *(const f32x4*)(tr + j + 4);
#pragma unroll
            for (int c = 0; c < 4; ++c) s += t0[c] * Elem<T>::to_f(bv[c]);
#pragma unroll
            for (int c = 0; c < 4; ++c) s += t1[c] * Elem<T>::to_f(bv[4 + c]);
        }
    } else {
        for (int j = 0; j < e.r; ++j) s += tr[j] * Elem<T>::to_f(br[j]);
    }
    return e.ls * s;
}

template <int MT, bool HALF, class... E>
__global__ __launch_bounds__(SK_THREADS) void skinny_mfma_kernel(const SkArgs<bf16> a, const E... e) {
    constexpr int SL = HALF ? 2 : 1;               // K slots per wave
    constexpr int ROWS = HALF ? 8 : 16;            // weight rows per workgroup
    constexpr int NS = SK_WAVES * SL;              // K slots per workgroup
    constexpr int MR = MT * 16;                    // x rows held (rows >= M are zeros)
    constexpr int XL = MR / 8;                     // x loads per lane, slot and pair
    constexpr int DW = 4;                          // W pairs in flight per lane
    constexpr int DX = MT == 1 ? 4 : MT == 2 ? 2 : 1;
    __shared__ __attribute__((aligned(16))) unsigned char smem[NS * MR * 128];      // x staging; the fold reuses it

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * ROWS;
    const int P = a.K >> 6;
    const int iters = (P + NS - 1) / NS;
    const int wslot = HALF ? w * 2 + (i >> 3) : w;
    // branch-free loads (units past K and x rows past M fall outside the descriptors and read as zero): the compiler sees every VMEM
    // op of the loop and waits with exact vmcnt counts, so the W ring stays in flight across iterations
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.W + (size_t)n0 * a.ldw, (uint32_t)(((size_t)(ROWS - 1) * a.ldw + a.K) * 2));
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.X, (uint32_t)(((size_t)(a.M - 1) * a.ldx + a.K) * 2));
    const uint32_t woff = (uint32_t)((HALF ? (i & 7) : i) * a.ldw + 16 * g) * 2u;
    const int xr_row = lane >> 3, xr_c = lane & 7;

    bf16x8 wr[DW][2];
    bf16x8 xr[DX][SL * XL];
    auto load_w = [&](int it, bf16x8 (&dst)[2]) {
        const int p = it * NS + wslot;
        const uint32_t off = p < P ? woff + (uint32_t)p * 128u : OOB;
        dst[0] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rw, off, 0, 2));            // aux 2: non-temporal
        dst[1] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rw, off + 16u, 0, 2));
    };
    auto load_x = [&](int it, bf16x8 (&dst)[SL * XL]) {
#pragma unroll
        for (int sl = 0; sl < SL; ++sl) {
            const int p = it * NS + w * SL + sl;
#pragma unroll
            for (int j = 0; j < XL; ++j) {
                const int r = j * 8 + xr_row;
                const uint32_t off = (p < P && r < a.M) ? ((uint32_t)r * (uint32_t)a.ldx + (uint32_t)p * 64u + (uint32_t)xr_c * 8u) * 2u : OOB;
                dst[sl * XL + j] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
            }
        }
    };
#pragma unroll
    for (int u = 0; u < DW; ++u) load_w(u, wr[u]);
#pragma unroll
    for (int u = 0; u < DX; ++u) load_x(u, xr[u]);

    f32x4 acc0[MT], acc1[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) { acc0[mt] = vzero<f32x4>(); acc1[mt] = vzero<f32x4>(); }

    unsigned char* xs = smem + (size_t)w * SL * MR * 128;          // this wave's staging image
    for (int it0 = 0; it0 < iters; it0 += DW) {
#pragma unroll
        for (int u = 0; u < DW; ++u) {
            const int it = it0 + u;
            if (it < iters) {                                       // uniform over the workgroup
#pragma unroll
                for (int sl = 0; sl < SL; ++sl)
#pragma unroll
                    for (int j = 0; j < XL; ++j) {
                        const int r = j * 8 + xr_row;
                        *(bf16x8*)(xs + ((sl * MR + r) * 128) + ((xr_c ^ (r & 7)) << 4)) = xr[u % DX][sl * XL + j];
                    }
                __syncthreads();
                load_x(it + DX, xr[u % DX]);
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        const int row = mt * 16 + i;
                        const int off = row * 128 + (((2 * g + t) ^ (i & 7)) << 4);
                        const bf16x8 b0 = *(const bf16x8*)(xs + off);
                        mma16(acc0[mt], wr[u][t], b0);
                        if (HALF) {
                            const bf16x8 b1 = *(const bf16x8*)(xs + MR * 128 + off);
                            mma16(acc1[mt], wr[u][t], b1);
                        }
                    }
                load_w(it + DW, wr[u]);
                __syncthreads();
            }
        }
    }

    // fold: part[slot][m][ROWS] fp32, summed in slot order
    float* part = (float*)smem;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if (HALF) {
            const int slot = 2 * w + (g >> 1);
            *(f32x4*)&part[((size_t)slot * MR + mt * 16 + i) * 8 + 4 * (g & 1)] = g < 2 ? acc0[mt] : acc1[mt];
        } else {
            *(f32x4*)&part[((size_t)w * MR + mt * 16 + i) * 16 + 4 * g] = acc0[mt];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < ROWS * a.M; idx += SK_THREADS) {
        const int n = idx % ROWS, m = idx / ROWS;
        float s = 0.f;
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) s += part[((size_t)sl * MR + m) * ROWS + n];
        if (sizeof...(E)) s += sk_extra<bf16>(m, n0 + n, e...);
        sk_store(a, m, n0 + n, s);
    }
}

template <typename T, class... E>
__global__ __launch_bounds__(256) void skinny_generic_kernel(const SkArgs<T> a, const E... e) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = blockIdx.x * 4 + w, m0 = blockIdx.y * 8;
    if (n >= a.N) return;                           // whole waves leave; the kernel has no barrier
    float acc[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = 0.f;
    const T* wrow = a.W + (size_t)n * a.ldw;
    for (int k = lane; k < a.K; k += WAVE) {
        const float wv = Elem<T>::to_f(wrow[k]);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int m = min(m0 + r, a.M - 1);
            acc[r] += wv * Elem<T>::to_f(a.X[(size_t)m * a.ldx + k]);
        }
    }
    float mine = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const float s = wave_sum(acc[r]);
        if (lane == r) mine = s;
    }
    if (lane < 8 && m0 + lane < a.M) {
        if (sizeof...(E)) mine += sk_extra<T>(m0 + lane, n, e...);
        sk_store(a, m0 + lane, n, mine);
    }
}

// stage 1 of mmgl_gemm_skinny_lora: t[M, r] = X[M, K] . A[r, K]^T, fp32.  One wave per adapter row j and 8 rows of x.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void lora_t_kernel(const T* __restrict__ X, int ldx, const T* __restrict__ A, int lda,
                                                     float* __restrict__ t, int M, int r, int K) {
    typedef typename Elem<T>::v8 V8;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = blockIdx.x * 4 + w, m0 = blockIdx.y * 8;
    if (j >= r) return;                             // whole waves leave; the kernel has no barrier
    float acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.f;
    const T* arow = A + (size_t)j * lda;
    if (VEC) {
        for (int k = lane * 8; k < K; k += WAVE * 8) {
            const V8 av = *(const V8*)(arow + k);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int m = min(m0 + q, M - 1);
                const V8 xv = *(const V8*)(X + (size_t)m * ldx + k);
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[q] += Elem<T>::to_f(av[c]) * Elem<T>::to_f(xv[c]);
            }
        }
    } else {
        for (int k = lane; k < K; k += WAVE) {
            const float av = Elem<T>::to_f(arow[k]);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int m = min(m0 + q, M - 1);
                acc[q] += av * Elem<T>::to_f(X[(size_t)m * ldx + k]);
            }
        }
    }
    float mine = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float s = wave_sum(acc[q]);
        if (lane == q) mine = s;
    }
    if (lane < 8 && m0 + lane < M) t[(size_t)(m0 + lane) * r + j] = mine;
}

template <int MT, bool HALF, class... E> int launch_skinny_mfma(const SkArgs<bf16>& a, hipStream_t st, const E&... e) {
    hipLaunchKernelGGL((skinny_mfma_kernel<MT, HALF, E...>), dim3(a.N / (HALF ? 8 : 16)), dim3(SK_THREADS), 0, st, a, e...);
    MMGL_CHECK_LAUNCH(sizeof...(E) ? "mmgl_gemm_skinny_lora" : "mmgl_gemm_skinny");
    return MMGL_OK;
}

template <bool HALF, class... E> int launch_skinny_mt(const SkArgs<bf16>& a, hipStream_t st, const E&... e) {
    if (a.M <= 16) return launch_skinny_mfma<1, HALF>(a, st, e...);
    if (a.M <= 32) return launch_skinny_mfma<2, HALF>(a, st, e...);
    return launch_skinny_mfma<4, HALF>(a, st, e...);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename T, class... E> int launch_skinny_generic(const SkArgs<T>& a, hipStream_t st, const E&... e) {
    hipLaunchKernelGGL((skinny_generic_kernel<T, E...>), dim3(cdiv(a.N, 4), cdiv(a.M, 8)), dim3(256), 0, st, a, e...);
    MMGL_CHECK_LAUNCH(sizeof...(E) ? "mmgl_gemm_skinny_lora" : "mmgl_gemm_skinny");
    return MMGL_OK;
}

// the route of a bf16 call, with or without the extra term: the MFMA kernel where it takes the shape, else the generic one
template <class... E> int skinny_bf16(const SkArgs<bf16>& a, hipStream_t st, const E&... e) {
    // the MFMA kernel addresses W rows of a workgroup and the whole x through 32-bit buffer offsets
    const bool mfma = a.K % 64 == 0 && a.N % 8 == 0 && a.ldx % 8 == 0 && a.ldw % 8 == 0 && aligned16(a.X) && aligned16(a.W) &&
                      ((size_t)(a.M - 1) * a.ldx + a.K) * 2 < (1ull << 31) && (size_t)16 * a.ldw * 2 < (1ull << 31);
    if (!mfma) return launch_skinny_generic<bf16>(a, st, e...);
    // 16 weight rows per workgroup where that still gives every CU one, else 8
    if (a.N % 16 == 0 && a.N / 16 >= mmgl_num_cu()) return launch_skinny_mt<false>(a, st, e...);
    return launch_skinny_mt<true>(a, st, e...);
}

template <typename T>
int launch_lora_t(const T* x, int ldx, const T* A, int lda, float* t, int M, int r, int K, hipStream_t st) {
    const size_t al = 8 * sizeof(T);
    const bool vec = K % 8 == 0 && ldx % 8 == 0 && lda % 8 == 0 && (uintptr_t)x % al == 0 && (uintptr_t)A % al == 0;
    const dim3 grid(cdiv(r, 4), cdiv(M, 8));
    if (vec) hipLaunchKernelGGL((lora_t_kernel<T, true>), grid, dim3(256), 0, st, x, ldx, A, lda, t, M, r, K);
    else hipLaunchKernelGGL((lora_t_kernel<T, false>), grid, dim3(256), 0, st, x, ldx, A, lda, t, M, r, K);
    MMGL_CHECK_LAUNCH("mmgl_gemm_skinny_lora (x A^T)");
    return MMGL_OK;
}

// ------------------------------------------------------------------------------------------------ single-query attention
template <typename T> struct Vec16;
template <> struct Vec16<bf16> { typedef bf16x8 type; };
template <> struct Vec16<float> { typedef f32x4 type; };

constexpr int AD_WAVES = 4;
constexpr int AD_UNROLL = 4;

// The operands every single-query attention entry point shares: q [rows, ldq] and out [rows, H*D] (rows = B, or B*W beam rows), the
// per-sample keys / values k, v [B, S, ldkv] of Hkv heads (batch stride bs_kv) and their mask valid [B, ld_valid].
struct AttnPrefix {
    const void *q, *k, *v;
    const uint8_t* valid;
    void* out;
    int ldq, ldkv, ld_valid, B, H, Hkv, S, D, dtype;
    size_t bs_kv;
};

// returns FN<T, D>(...) at the head_dim that check_attn_prefix let through: nothing after it runs
#define RETURN_BY_HEAD_DIM(FN, T, D, ...)               \
    do {                                                \
        switch (D) {                                    \
            case 16: return FN<T, 16>(__VA_ARGS__);     \
            case 32: return FN<T, 32>(__VA_ARGS__);     \
            case 64: return FN<T, 64>(__VA_ARGS__);     \
            default: return FN<T, 128>(__VA_ARGS__);    \
        }                                               \
    } while (0)

template <typename T, int D>
__global__ __launch_bounds__(AD_WAVES * WAVE) void attn_decode_kernel(const T* __restrict__ q, int ldq, const T* __restrict__ k,
                                                                      const T* __restrict__ v, int ldkv, size_t bs_kv,
                                                                      const uint8_t* __restrict__ valid, int ld_valid,
                                                                      T* __restrict__ out, int H, int S) {
    typedef typename Vec16<T>::type V;
    constexpr int VEC = 16 / sizeof(T);
    constexpr int LPK = D / VEC;                    // lanes per key
    constexpr int KPI = WAVE / LPK;                 // keys per wave and load instruction
    constexpr float NEG = -FLT_MAX;
    __shared__ float sm_m[AD_WAVES], sm_l[AD_WAVES], sm_o[AD_WAVES][D];

    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane % LPK, kk = lane / LPK;

    float qf[VEC];
    {
        const V qv = *(const V*)(q + (size_t)b * ldq + h * D + c * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) qf[e] = Elem<T>::to_f(qv[e]);
    }
    // branch-free loads: keys past S fall outside the descriptors
    const uint32_t slab = (uint32_t)(((size_t)(S - 1) * ldkv + D) * sizeof(T)), row_bytes = (uint32_t)(ldkv * sizeof(T));
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(k + b * bs_kv + h * D, slab);
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(v + b * bs_kv + h * D, slab);
    const uint8_t* mb = valid + (size_t)b * ld_valid;

    float m = NEG, l = 0.f, acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;

    for (int base = w * KPI; base < S; base += AD_WAVES * KPI * AD_UNROLL) {          // wave-uniform trip count
        V kr[AD_UNROLL], vr[AD_UNROLL];
        uint8_t ok[AD_UNROLL];
#pragma unroll
        for (int u = 0; u < AD_UNROLL; ++u) {
            const int s = base + u * AD_WAVES * KPI + kk;
            const uint32_t off = s < S ? (uint32_t)s * row_bytes + (uint32_t)(c * 16) : OOB;
            kr[u] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rk, off, 0, 0));
            vr[u] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rv, off, 0, 0));
            ok[u] = mb[min(s, S - 1)];
        }
#pragma unroll
        for (int u = 0; u < AD_UNROLL; ++u) {
            const int s = base + u * AD_WAVES * KPI + kk;
            float dot = 0.f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) dot += qf[e] * Elem<T>::to_f(kr[u][e]);
#pragma unroll
            for (int o = 1; o < LPK; o <<= 1) dot += __shfl_xor(dot, o);
            if (s < S) {
                const float sc = ok[u] ? dot : NEG;
                const float mn = fmaxf(m, sc);
                const float corr = __expf(m - mn), p = __expf(sc - mn);
                l = l * corr + p;
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] = acc[e] * corr + p * Elem<T>::to_f(vr[u][e]);
                m = mn;
            }
        }
    }
    // merge the lane groups of the wave (fixed butterfly), then the waves in order
#pragma unroll
    for (int o = LPK; o < WAVE; o <<= 1) {
        const float m2 = __shfl_xor(m, o), l2 = __shfl_xor(l, o);
        const float mn = fmaxf(m, m2);
        const float c1 = __expf(m - mn), c2 = __expf(m2 - mn);
        l = l * c1 + l2 * c2;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = acc[e] * c1 + __shfl_xor(acc[e], o) * c2;
        m = mn;
    }
    if (lane < LPK) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) sm_o[w][c * VEC + e] = acc[e];
        if (lane == 0) { sm_m[w] = m; sm_l[w] = l; }
    }
    __syncthreads();
    if (tid < D) {
        float mm = sm_m[0];
#pragma unroll
        for (int i = 1; i < AD_WAVES; ++i) mm = fmaxf(mm, sm_m[i]);
        float ll = 0.f, o = 0.f;
#pragma unroll
        for (int i = 0; i < AD_WAVES; ++i) {
            const float ci = __expf(sm_m[i] - mm);
            ll += sm_l[i] * ci;
            o += sm_o[i][tid] * ci;
        }
        out[((size_t)b * H + h) * D + tid] = Elem<T>::from_f(o / ll);
    }
}

template <typename T, int D>
int launch_attn_decode(const AttnPrefix& a, hipStream_t st) {
    hipLaunchKernelGGL((attn_decode_kernel<T, D>), dim3(a.B * a.H), dim3(AD_WAVES * WAVE), 0, st, (const T*)a.q, a.ldq, (const T*)a.k,
                       (const T*)a.v, a.ldkv, a.bs_kv, a.valid, a.ld_valid, (T*)a.out, a.H, a.S);
    MMGL_CHECK_LAUNCH("mmgl_attn_decode_fwd");
    return MMGL_OK;
}

// ------------------------------------------------------------------------------------------------ single-query attention, T5 bias
// attn_decode_kernel for the T5 decoder's self-attention: the same lanes, trips, loads and merges, with no key mask (a decoder row
// has no padding) and no scale, and bias[h][S - 1 - s] -- a learned fp32 word per (head, distance to the query, which is the newest
// key s = S - 1) -- added to the raw score of key s.  The LPK lanes of a key read the same bias word; past S the index is clamped to
// distance 0 and the word is not used.
template <typename T, int D>
__global__ __launch_bounds__(AD_WAVES * WAVE) void attn_decode_relbias_kernel(const T* __restrict__ q, int ldq, const T* __restrict__ k,
                                                                              const T* __restrict__ v, int ldkv, size_t bs_kv,
                                                                              const float* __restrict__ bias, int ld_bias,
                                                                              T* __restrict__ out, int H, int S) {
    typedef typename Vec16<T>::type V;
    constexpr int VEC = 16 / sizeof(T);
    constexpr int LPK = D / VEC;                    // lanes per key
    constexpr int KPI = WAVE / LPK;                 // keys per wave and load instruction
    constexpr float NEG = -FLT_MAX;
    __shared__ float sm_m[AD_WAVES], sm_l[AD_WAVES], sm_o[AD_WAVES][D];

    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane % LPK, kk = lane / LPK;

    float qf[VEC];
    {
        const V qv = *(const V*)(q + (size_t)b * ldq + h * D + c * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) qf[e] = Elem<T>::to_f(qv[e]);
    }
    // branch-free loads: keys past S fall outside the descriptors
    const uint32_t slab = (uint32_t)(((size_t)(S - 1) * ldkv + D) * sizeof(T)), row_bytes = (uint32_t)(ldkv * sizeof(T));
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(k + b * bs_kv + h * D, slab);
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(v + b * bs_kv + h * D, slab);
    const float* bh = bias + (size_t)h * ld_bias;

    float m = NEG, l = 0.f, acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;

    for (int base = w * KPI; base < S; base += AD_WAVES * KPI * AD_UNROLL) {          // wave-uniform trip count
        V kr[AD_UNROLL], vr[AD_UNROLL];
        float bs[AD_UNROLL];
#pragma unroll
        for (int u = 0; u < AD_UNROLL; ++u) {
            const int s = base + u * AD_WAVES * KPI + kk;
            const uint32_t off = s < S ? (uint32_t)s * row_bytes + (uint32_t)(c * 16) : OOB;
            kr[u] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rk, off, 0, 0));
            vr[u] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rv, off, 0, 0));
            bs[u] = bh[S - 1 - min(s, S - 1)];
        }
#pragma unroll
        for (int u = 0; u < AD_UNROLL; ++u) {
            const int s = base + u * AD_WAVES * KPI + kk;
            float dot = 0.f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) dot += qf[e] * Elem<T>::to_f(kr[u][e]);
#pragma unroll
            for (int o = 1; o < LPK; o <<= 1) dot += __shfl_xor(dot, o);
            if (s < S) {
                const float sc = dot + bs[u];
                const float mn = fmaxf(m, sc);
                const float corr = __expf(m - mn), p = __expf(sc - mn);
                l = l * corr + p;
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] = acc[e] * corr + p * Elem<T>::to_f(vr[u][e]);
                m = mn;
            }
        }
    }
    // merge the lane groups of the wave (fixed butterfly), then the waves in order
#pragma unroll
    for (int o = LPK; o < WAVE; o <<= 1) {
        const float m2 = __shfl_xor(m, o), l2 = __shfl_xor(l, o);
        const float mn = fmaxf(m, m2);
        const float c1 = __expf(m - mn), c2 = __expf(m2 - mn);
        l = l * c1 + l2 * c2;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = acc[e] * c1 + __shfl_xor(acc[e], o) * c2;
        m = mn;
    }
    if (lane < LPK) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) sm_o[w][c * VEC + e] = acc[e];
        if (lane == 0) { sm_m[w] = m; sm_l[w] = l; }
    }
    __syncthreads();
    if (tid < D) {
        float mm = sm_m[0];
#pragma unroll
        for (int i = 1; i < AD_WAVES; ++i) mm = fmaxf(mm, sm_m[i]);
        float ll = 0.f, o = 0.f;
#pragma unroll
        for (int i = 0; i < AD_WAVES; ++i) {
            const float ci = __expf(sm_m[i] - mm);
            ll += sm_l[i] * ci;
            o += sm_o[i][tid] * ci;
        }
        out[((size_t)b * H + h) * D + tid] = Elem<T>::from_f(o / ll);
    }
}

template <typename T, int D>
int launch_attn_decode_relbias(const AttnPrefix& a, const float* bias, int ld_bias, hipStream_t st) {
    hipLaunchKernelGGL((attn_decode_relbias_kernel<T, D>), dim3(a.B * a.H), dim3(AD_WAVES * WAVE), 0, st, (const T*)a.q, a.ldq, (const T*)a.k,
                       (const T*)a.v, a.ldkv, a.bs_kv, bias, ld_bias, (T*)a.out, a.H, a.S);
    MMGL_CHECK_LAUNCH("mmgl_attn_decode_relbias_fwd");
    return MMGL_OK;
}

// ------------------------------------------------------------------------------------------------ grouped-query single-query attention
// One workgroup per (sample, key/value head, block of NQ <= 8 query heads of that head's group): the key and value registers of
// attn_decode_kernel (same lane layout, same trip constants) feed NQ online-softmax states per lane group, so every 16-byte K / V load
// is issued once for the whole block and nothing is expanded in memory.  A block with fewer than NQ heads (nq < NQ) computes its last
// head NQ - nq times more and stores nq rows: no divergent branch in the loop.
template <typename T, int D, int NQ>
__global__ __launch_bounds__(AD_WAVES * WAVE) void attn_decode_gqa_kernel(const T* __restrict__ q, int ldq, const T* __restrict__ k,
                                                                          const T* __restrict__ v, int ldkv, size_t bs_kv,
                                                                          const uint8_t* __restrict__ valid, int ld_valid,
                                                                          T* __restrict__ out, int H, int Hkv, int S, int qpb, int nblk) {
    typedef typename Vec16<T>::type V;
    constexpr int VEC = 16 / sizeof(T);
    constexpr int LPK = D / VEC;                    // lanes per key
    constexpr int KPI = WAVE / LPK;                 // keys per wave and load instruction
    constexpr float NEG = -FLT_MAX;
    __shared__ float sm_m[AD_WAVES][NQ], sm_l[AD_WAVES][NQ], sm_o[AD_WAVES][NQ][D];

    const int G = H / Hkv;
    const int qb = blockIdx.x % nblk, kvh = (blockIdx.x / nblk) % Hkv, b = blockIdx.x / (nblk * Hkv);
    const int h0 = kvh * G + qb * qpb, nq = min(qpb, G - qb * qpb);        // query heads h0 .. h0 + nq - 1
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane % LPK, kk = lane / LPK;

    float qf[NQ][VEC];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const V qv = *(const V*)(q + (size_t)b * ldq + (h0 + min(j, nq - 1)) * D + c * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) qf[j][e] = Elem<T>::to_f(qv[e]);
    }
    // branch-free loads: keys past S fall outside the descriptors
    const uint32_t slab = (uint32_t)(((size_t)(S - 1) * ldkv + D) * sizeof(T)), row_bytes = (uint32_t)(ldkv * sizeof(T));
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(k + b * bs_kv + kvh * D, slab);
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(v + b * bs_kv + kvh * D, slab);
    const uint8_t* mb = valid + (size_t)b * ld_valid;

    float m[NQ], l[NQ], acc[NQ][VEC];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        m[j] = NEG;
        l[j] = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[j][e] = 0.f;
    }

    for (int base = w * KPI; base < S; base += AD_WAVES * KPI * AD_UNROLL) {          // wave-uniform trip count
        V kr[AD_UNROLL], vr[AD_UNROLL];
        uint8_t ok[AD_UNROLL];
        bool in[AD_UNROLL];
#pragma unroll
        for (int u = 0; u < AD_UNROLL; ++u) {
            const int s = base + u * AD_WAVES * KPI + kk;
            in[u] = s < S;
            const uint32_t off = in[u] ? (uint32_t)s * row_bytes + (uint32_t)(c * 16) : OOB;
            kr[u] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rk, off, 0, 0));
            vr[u] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rv, off, 0, 0));
            ok[u] = mb[min(s, S - 1)];
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            // the trip's AD_UNROLL keys enter the online softmax together: one rescale of the state per trip instead of one per key
            float sc[AD_UNROLL], mn = m[j];
#pragma unroll
            for (int u = 0; u < AD_UNROLL; ++u) {
                float dot = 0.f;
#pragma unroll
                for (int e = 0; e < VEC; ++e) dot += qf[j][e] * Elem<T>::to_f(kr[u][e]);
                dot = group_sum<LPK>(dot);
                sc[u] = ok[u] ? dot : NEG;
                if (in[u]) mn = fmaxf(mn, sc[u]);
            }
            const float corr = __expf(m[j] - mn);
            float pu[AD_UNROLL], ps = 0.f;
#pragma unroll
            for (int u = 0; u < AD_UNROLL; ++u) {
                pu[u] = in[u] ? __expf(sc[u] - mn) : 0.f;             // a key past S weighs nothing, also in a row of masked keys
                ps += pu[u];
            }
            l[j] = l[j] * corr + ps;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                float a = acc[j][e] * corr;
#pragma unroll
                for (int u = 0; u < AD_UNROLL; ++u) a += pu[u] * Elem<T>::to_f(vr[u][e]);
                acc[j][e] = a;
            }
            m[j] = mn;
        }
    }
    // per query head: merge the lane groups of the wave (fixed butterfly), then the waves in order
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
#pragma unroll
        for (int o = LPK; o < WAVE; o <<= 1) {
            const float m2 = __shfl_xor(m[j], o), l2 = __shfl_xor(l[j], o);
            const float mn = fmaxf(m[j], m2);
            const float c1 = __expf(m[j] - mn), c2 = __expf(m2 - mn);
            l[j] = l[j] * c1 + l2 * c2;
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[j][e] = acc[j][e] * c1 + __shfl_xor(acc[j][e], o) * c2;
            m[j] = mn;
        }
        if (lane < LPK) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) sm_o[w][j][c * VEC + e] = acc[j][e];
            if (lane == 0) { sm_m[w][j] = m[j]; sm_l[w][j] = l[j]; }
        }
    }
    __syncthreads();
    for (int idx = tid; idx < nq * D; idx += AD_WAVES * WAVE) {
        const int j = idx / D, x = idx % D;
        float mm = sm_m[0][j];
#pragma unroll
        for (int i = 1; i < AD_WAVES; ++i) mm = fmaxf(mm, sm_m[i][j]);
        float ll = 0.f, o = 0.f;
#pragma unroll
        for (int i = 0; i < AD_WAVES; ++i) {
            const float ci = __expf(sm_m[i][j] - mm);
            ll += sm_l[i][j] * ci;
            o += sm_o[i][j][x] * ci;
        }
        out[((size_t)b * H + h0 + j) * D + x] = Elem<T>::from_f(o / ll);
    }
}

template <typename T, int D>
int attn_decode_gqa_nq(const AttnPrefix& a, hipStream_t st) {
    const int G = a.H / a.Hkv, nblk = cdiv(G, 8), qpb = cdiv(G, nblk);    // G > 8: further blocks, of equal size up to one head
    const dim3 grid(a.B * a.Hkv * nblk), block(AD_WAVES * WAVE);
#define MMGL_GQA_DECODE(NQ)                                                                                                          \
    hipLaunchKernelGGL((attn_decode_gqa_kernel<T, D, NQ>), grid, block, 0, st, (const T*)a.q, a.ldq, (const T*)a.k, (const T*)a.v, a.ldkv, \
                       a.bs_kv, a.valid, a.ld_valid, (T*)a.out, a.H, a.Hkv, a.S, qpb, nblk)
    if (qpb == 1) MMGL_GQA_DECODE(1);
    else if (qpb == 2) MMGL_GQA_DECODE(2);
    else if (qpb <= 4) MMGL_GQA_DECODE(4);
    else MMGL_GQA_DECODE(8);
#undef MMGL_GQA_DECODE
    MMGL_CHECK_LAUNCH("mmgl_attn_decode_gqa_fwd");
    return MMGL_OK;
}

// ------------------------------------------------------------------------------------------------ beam-shared single-query attention
// One workgroup per (sample, head) serves the W <= NQ beam rows b*W + w of the sample.  Phase 1 is the loop of attn_decode_gqa_kernel
// over the sample's S_pre shared prefix keys (the prompt's cache rows or the projected neighbor tokens): every 16-byte K / V load is
// issued once and scored against the NQ queries from registers.  Phase 2 walks the n_tail keys the hypotheses generated themselves:
// tail key t of row (b, w) is row b*W + src[b*W + w][t], column t, of the [B*W, n_cap, 2d] tail buffer, so reordering the beams rewrites
// the small int32 table and never a cache row.  The same lane layout and online-softmax state run through both phases (one rescale per
// trip: AD_UNROLL prefix keys, TAIL_UNROLL tail keys of a row), then the merge of attn_decode_kernel.  Surplus rows (w >= W) repeat row W - 1 and are not stored.  A src
// value is clamped into [0, W): a table the caller filled wrongly reads a wrong beam's key, never memory outside the sample's rows.
// A sample whose prefix has no valid key weighs ALL its S_pre + n_tail keys equally (the tail scores take -FLT_MAX too).
template <typename T, int D, int NQ>
__global__ __launch_bounds__(AD_WAVES * WAVE) void attn_decode_beam_kernel(const T* __restrict__ q, int ldq, const T* __restrict__ kp,
                                                                           const T* __restrict__ vp, int ld_pre, size_t bs_pre,
                                                                           const uint8_t* __restrict__ valid, int ld_valid,
                                                                           const T* __restrict__ kt, const T* __restrict__ vt, int ld_tail,
                                                                           size_t rs_tail, const int* __restrict__ src, int ld_src,
                                                                           T* __restrict__ out, int W, int H, int S, int n_tail) {
    typedef typename Vec16<T>::type V;
    constexpr int VEC = 16 / sizeof(T);
    constexpr int LPK = D / VEC;                    // lanes per key
    constexpr int KPI = WAVE / LPK;                 // keys per wave and load instruction
    constexpr float NEG = -FLT_MAX;
    constexpr int TAIL_UNROLL = 2;                  // keys per trip of the tail: W rows of loads are in flight at once, and a tail is short
    __shared__ float sm_m[AD_WAVES][NQ], sm_l[AD_WAVES][NQ], sm_o[AD_WAVES][NQ][D];

    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane % LPK, kk = lane / LPK;
    const size_t row0 = (size_t)b * W;

    float qf[NQ][VEC];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const V qv = *(const V*)(q + (row0 + min(j, W - 1)) * ldq + h * D + c * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) qf[j][e] = Elem<T>::to_f(qv[e]);
    }
    float m[NQ], l[NQ], acc[NQ][VEC];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        m[j] = NEG;
        l[j] = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[j][e] = 0.f;
    }
    // the AD_UNROLL keys of a trip enter row j's online softmax together: one rescale of the state per trip
    auto fold = [&](int j, const auto& kr, const auto& vr, const auto& ok, const auto& in) {
        constexpr int U = sizeof(ok) / sizeof(bool);
        float sc[U], mn = m[j];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float dot = 0.f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) dot += qf[j][e] * Elem<T>::to_f(kr[u][e]);
            dot = group_sum<LPK>(dot);
            sc[u] = ok[u] ? dot : NEG;
            if (in[u]) mn = fmaxf(mn, sc[u]);
        }
        const float corr = __expf(m[j] - mn);
        float pu[U], ps = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            pu[u] = in[u] ? __expf(sc[u] - mn) : 0.f;                 // a key past the end weighs nothing, also in a row of masked keys
            ps += pu[u];
        }
        l[j] = l[j] * corr + ps;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float a = acc[j][e] * corr;
#pragma unroll
            for (int u = 0; u < U; ++u) a += pu[u] * Elem<T>::to_f(vr[u][e]);
            acc[j][e] = a;
        }
        m[j] = mn;
    };

    // ---- phase 1: the shared prefix (branch-free loads: keys past S fall outside the descriptors)
    bool any_ok = false;
    {
        const uint32_t slab = (uint32_t)(((size_t)(S - 1) * ld_pre + D) * sizeof(T)), row_bytes = (uint32_t)(ld_pre * sizeof(T));
        const __amdgpu_buffer_rsrc_t rk = make_rsrc(kp + b * bs_pre + h * D, slab);
        const __amdgpu_buffer_rsrc_t rv = make_rsrc(vp + b * bs_pre + h * D, slab);
        const uint8_t* mb = valid + (size_t)b * ld_valid;
        for (int base = w * KPI; base < S; base += AD_WAVES * KPI * AD_UNROLL) {          // wave-uniform trip count
            V kr[AD_UNROLL], vr[AD_UNROLL];
            bool ok[AD_UNROLL], in[AD_UNROLL];
#pragma unroll
            for (int u = 0; u < AD_UNROLL; ++u) {
                const int s = base + u * AD_WAVES * KPI + kk;
                in[u] = s < S;
                const uint32_t off = in[u] ? (uint32_t)s * row_bytes + (uint32_t)(c * 16) : OOB;
                kr[u] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rk, off, 0, 0));
                vr[u] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rv, off, 0, 0));
                ok[u] = mb[min(s, S - 1)] != 0;
                any_ok |= in[u] && ok[u];
            }
#pragma unroll
            for (int j = 0; j < NQ; ++j) fold(j, kr, vr, ok, in);
        }
    }
    // ---- phase 2: the per-beam tail, addressed through src
    if (n_tail > 0) {
        const bool live = __syncthreads_or(any_ok) != 0;           // some prefix key of the sample is valid (uniform over the workgroup)
        const uint32_t span = (uint32_t)(((size_t)(W - 1) * rs_tail + (size_t)(n_tail - 1) * ld_tail + D) * sizeof(T));
        const uint32_t col_bytes = (uint32_t)(ld_tail * sizeof(T)), beam_bytes = (uint32_t)(rs_tail * sizeof(T));
        const __amdgpu_buffer_rsrc_t rk = make_rsrc(kt + row0 * rs_tail + h * D, span);
        const __amdgpu_buffer_rsrc_t rv = make_rsrc(vt + row0 * rs_tail + h * D, span);
        for (int base = w * KPI; base < n_tail; base += AD_WAVES * KPI * TAIL_UNROLL) {     // wave-uniform trip count
            int from[NQ][TAIL_UNROLL];
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                const int* sr = src + (row0 + min(j, W - 1)) * ld_src;
#pragma unroll
                for (int u = 0; u < TAIL_UNROLL; ++u) from[j][u] = sr[min(base + u * AD_WAVES * KPI + kk, n_tail - 1)];
            }
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                V kr[TAIL_UNROLL], vr[TAIL_UNROLL];
                bool ok[TAIL_UNROLL], in[TAIL_UNROLL];
#pragma unroll
                for (int u = 0; u < TAIL_UNROLL; ++u) {
                    const int t = base + u * AD_WAVES * KPI + kk;
                    in[u] = t < n_tail;
                    ok[u] = live;
                    const uint32_t beam = (uint32_t)min(max(from[j][u], 0), W - 1);
                    const uint32_t off = in[u] ? beam * beam_bytes + (uint32_t)t * col_bytes + (uint32_t)(c * 16) : OOB;
                    kr[u] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rk, off, 0, 0));
                    vr[u] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rv, off, 0, 0));
                }
                fold(j, kr, vr, ok, in);
            }
        }
    }
    // per beam row: merge the lane groups of the wave (fixed butterfly), then the waves in order
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
#pragma unroll
        for (int o = LPK; o < WAVE; o <<= 1) {
            const float m2 = __shfl_xor(m[j], o), l2 = __shfl_xor(l[j], o);
            const float mn = fmaxf(m[j], m2);
            const float c1 = __expf(m[j] - mn), c2 = __expf(m2 - mn);
            l[j] = l[j] * c1 + l2 * c2;
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[j][e] = acc[j][e] * c1 + __shfl_xor(acc[j][e], o) * c2;
            m[j] = mn;
        }
        if (lane < LPK) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) sm_o[w][j][c * VEC + e] = acc[j][e];
            if (lane == 0) { sm_m[w][j] = m[j]; sm_l[w][j] = l[j]; }
        }
    }
    __syncthreads();
    for (int idx = tid; idx < W * D; idx += AD_WAVES * WAVE) {
        const int j = idx / D, x = idx % D;
        float mm = sm_m[0][j];
#pragma unroll
        for (int i = 1; i < AD_WAVES; ++i) mm = fmaxf(mm, sm_m[i][j]);
        float ll = 0.f, o = 0.f;
#pragma unroll
        for (int i = 0; i < AD_WAVES; ++i) {
            const float ci = __expf(sm_m[i][j] - mm);
            ll += sm_l[i][j] * ci;
            o += sm_o[i][j][x] * ci;
        }
        out[((row0 + j) * H + h) * D + x] = Elem<T>::from_f(o / ll);
    }
}

struct BeamAttnArgs {
    AttnPrefix p;                                  // the sample's shared prefix; q and out have B*W rows
    const void *kt, *vt;
    const int* src;
    int ld_tail, ld_src, W, n_tail;
    size_t rs_tail;
};

template <typename T, int D>
int attn_decode_beam_nq(const BeamAttnArgs& a, hipStream_t st) {
    const AttnPrefix& p = a.p;
    const dim3 grid(p.B * p.H), block(AD_WAVES * WAVE);
#define MMGL_BEAM_DECODE(NQ)                                                                                                            \
    hipLaunchKernelGGL((attn_decode_beam_kernel<T, D, NQ>), grid, block, 0, st, (const T*)p.q, p.ldq, (const T*)p.k, (const T*)p.v,    \
                       p.ldkv, p.bs_kv, p.valid, p.ld_valid, (const T*)a.kt, (const T*)a.vt, a.ld_tail, a.rs_tail, a.src, a.ld_src,    \
                       (T*)p.out, a.W, p.H, p.S, a.n_tail)
    if (a.W == 1) MMGL_BEAM_DECODE(1);
    else if (a.W == 2) MMGL_BEAM_DECODE(2);
    else if (a.W <= 4) MMGL_BEAM_DECODE(4);
    else MMGL_BEAM_DECODE(8);
#undef MMGL_BEAM_DECODE
    MMGL_CHECK_LAUNCH("mmgl_attn_decode_beam_fwd");
    return MMGL_OK;
}

// ------------------------------------------------------------------------------------------------ causal block of m new tokens per sample
// One workgroup per (sample, head) serves the W <= NQ new tokens b*W + i of the sample (a verify step of prompt-lookup decoding).  Phase 1
// is phase 1 of attn_decode_beam_kernel over the L = len[b] cache columns the sample has filed so far -- L is clamped into [0, capacity]
// and is uniform over the workgroup, so every wave makes the same trips.  Phase 2 scores the W new keys, read from the dense projection
// output [B*W, ld_new]: 4 waves x KPI >= 2 lane groups hold one new key each, so one trip covers them; row i folds key t only for t <= i
// (new keys are always valid).  The lane group that holds new key t then files it, and its value, at cache column L + t of head h, unless
// that column is at or past `capacity`: such a key belongs to an input whose output the caller discards.  Phase 1 reads only columns below
// L and every (sample, head, column) has one writer, so nothing races.  Same state, rescale per trip and merge as the beam kernel; surplus
// rows (i >= W) repeat row W - 1 and are not stored.
template <typename T, int D, int NQ>
__global__ __launch_bounds__(AD_WAVES * WAVE) void attn_decode_block_kernel(const T* __restrict__ q, int ldq, const T* __restrict__ kn,
                                                                            const T* __restrict__ vn, int ld_new, T* kc, T* vc, int ldkv,
                                                                            size_t bs_kv, int capacity, const uint8_t* __restrict__ valid,
                                                                            int ld_valid, const int* __restrict__ len, T* __restrict__ out,
                                                                            int W, int H) {
    typedef typename Vec16<T>::type V;
    constexpr int VEC = 16 / sizeof(T);
    constexpr int LPK = D / VEC;                    // lanes per key
    constexpr int KPI = WAVE / LPK;                 // keys per wave and load instruction
    constexpr float NEG = -FLT_MAX;
    __shared__ float sm_m[AD_WAVES][NQ], sm_l[AD_WAVES][NQ], sm_o[AD_WAVES][NQ][D];

    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane % LPK, kk = lane / LPK;
    const size_t row0 = (size_t)b * W;
    const int S = min(max(len[b], 0), capacity);    // the caller's contract; clamped, never trusted as an address

    float qf[NQ][VEC];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const V qv = *(const V*)(q + (row0 + min(j, W - 1)) * ldq + h * D + c * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) qf[j][e] = Elem<T>::to_f(qv[e]);
    }
    float m[NQ], l[NQ], acc[NQ][VEC];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        m[j] = NEG;
        l[j] = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[j][e] = 0.f;
    }
    // the keys of a trip enter row j's online softmax together: one rescale of the state per trip
    auto fold = [&](int j, const auto& kr, const auto& vr, const auto& ok, const auto& in) {
        constexpr int U = sizeof(ok) / sizeof(bool);
        float sc[U], mn = m[j];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float dot = 0.f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) dot += qf[j][e] * Elem<T>::to_f(kr[u][e]);
            dot = group_sum<LPK>(dot);
            sc[u] = ok[u] ? dot : NEG;
            if (in[u]) mn = fmaxf(mn, sc[u]);
        }
        const float corr = __expf(m[j] - mn);
        float pu[U], ps = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            pu[u] = in[u] ? __expf(sc[u] - mn) : 0.f;                 // a key the row does not see weighs nothing
            ps += pu[u];
        }
        l[j] = l[j] * corr + ps;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float a = acc[j][e] * corr;
#pragma unroll
            for (int u = 0; u < U; ++u) a += pu[u] * Elem<T>::to_f(vr[u][e]);
            acc[j][e] = a;
        }
        m[j] = mn;
    };

    T* kb = kc + b * bs_kv + h * D;
    T* vb = vc + b * bs_kv + h * D;
    // ---- phase 1: the cache columns below L (branch-free loads: keys past L fall outside the descriptors)
    if (S > 0) {
        const uint32_t slab = (uint32_t)(((size_t)(S - 1) * ldkv + D) * sizeof(T)), row_bytes = (uint32_t)(ldkv * sizeof(T));
        const __amdgpu_buffer_rsrc_t rk = make_rsrc(kb, slab);
        const __amdgpu_buffer_rsrc_t rv = make_rsrc(vb, slab);
        const uint8_t* mb = valid + (size_t)b * ld_valid;
        for (int base = w * KPI; base < S; base += AD_WAVES * KPI * AD_UNROLL) {          // wave-uniform trip count
            V kr[AD_UNROLL], vr[AD_UNROLL];
            bool ok[AD_UNROLL], in[AD_UNROLL];
#pragma unroll
            for (int u = 0; u < AD_UNROLL; ++u) {
                const int s = base + u * AD_WAVES * KPI + kk;
                in[u] = s < S;
                const uint32_t off = in[u] ? (uint32_t)s * row_bytes + (uint32_t)(c * 16) : OOB;
                kr[u] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rk, off, 0, 0));
                vr[u] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rv, off, 0, 0));
                ok[u] = mb[min(s, S - 1)] != 0;
            }
#pragma unroll
            for (int j = 0; j < NQ; ++j) fold(j, kr, vr, ok, in);
        }
    }
    // ---- phase 2: the W new keys, causal among themselves, then their way into the cache
    if (w * KPI < W) {                                                                     // wave-uniform
        const uint32_t span = (uint32_t)(((size_t)(W - 1) * ld_new + D) * sizeof(T)), new_bytes = (uint32_t)(ld_new * sizeof(T));
        const __amdgpu_buffer_rsrc_t rk = make_rsrc(kn + row0 * ld_new + h * D, span);
        const __amdgpu_buffer_rsrc_t rv = make_rsrc(vn + row0 * ld_new + h * D, span);
        const int t = w * KPI + kk;
        const bool mine = t < W;
        const uint32_t off = mine ? (uint32_t)t * new_bytes + (uint32_t)(c * 16) : OOB;
        V kr[1], vr[1];
        kr[0] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rk, off, 0, 0));
        vr[0] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rv, off, 0, 0));
        const bool ok[1] = {true};
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const bool in[1] = {mine && t <= j};
            fold(j, kr, vr, ok, in);
        }
        if (mine && S + t < capacity) {
            const size_t at = (size_t)(S + t) * ldkv + c * VEC;
            *(V*)(kb + at) = kr[0];
            *(V*)(vb + at) = vr[0];
        }
    }
    // per row: merge the lane groups of the wave (fixed butterfly), then the waves in order
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
#pragma unroll
        for (int o = LPK; o < WAVE; o <<= 1) {
            const float m2 = __shfl_xor(m[j], o), l2 = __shfl_xor(l[j], o);
            const float mn = fmaxf(m[j], m2);
            const float c1 = __expf(m[j] - mn), c2 = __expf(m2 - mn);
            l[j] = l[j] * c1 + l2 * c2;
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[j][e] = acc[j][e] * c1 + __shfl_xor(acc[j][e], o) * c2;
            m[j] = mn;
        }
        if (lane < LPK) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) sm_o[w][j][c * VEC + e] = acc[j][e];
            if (lane == 0) { sm_m[w][j] = m[j]; sm_l[w][j] = l[j]; }
        }
    }
    __syncthreads();
    for (int idx = tid; idx < W * D; idx += AD_WAVES * WAVE) {
        const int j = idx / D, x = idx % D;
        float mm = sm_m[0][j];
#pragma unroll
        for (int i = 1; i < AD_WAVES; ++i) mm = fmaxf(mm, sm_m[i][j]);
        float ll = 0.f, o = 0.f;
#pragma unroll
        for (int i = 0; i < AD_WAVES; ++i) {
            const float ci = __expf(sm_m[i][j] - mm);
            ll += sm_l[i][j] * ci;
            o += sm_o[i][j][x] * ci;
        }
        out[((row0 + j) * H + h) * D + x] = Elem<T>::from_f(o / ll);
    }
}

struct BlockAttnArgs {
    AttnPrefix p;                                  // the sample's cache slabs (S = capacity); q and out have B*W rows
    const void *kn, *vn;
    const int* len;
    int ld_new, W;
};

template <typename T, int D>
int attn_decode_block_nq(const BlockAttnArgs& a, hipStream_t st) {
    const AttnPrefix& p = a.p;
    const dim3 grid(p.B * p.H), block(AD_WAVES * WAVE);
#define MMGL_BLOCK_DECODE(NQ)                                                                                                          \
    hipLaunchKernelGGL((attn_decode_block_kernel<T, D, NQ>), grid, block, 0, st, (const T*)p.q, p.ldq, (const T*)a.kn, (const T*)a.vn, \
                       a.ld_new, (T*)p.k, (T*)p.v, p.ldkv, p.bs_kv, p.S, p.valid, p.ld_valid, a.len, (T*)p.out, a.W, p.H)
    if (a.W == 1) MMGL_BLOCK_DECODE(1);
    else if (a.W == 2) MMGL_BLOCK_DECODE(2);
    else if (a.W <= 4) MMGL_BLOCK_DECODE(4);
    else MMGL_BLOCK_DECODE(8);
#undef MMGL_BLOCK_DECODE
    MMGL_CHECK_LAUNCH("mmgl_attn_decode_block_fwd");
    return MMGL_OK;
}

// ------------------------------------------------------------------------------------------------ causal block over a grouped-query cache
// attn_decode_block_kernel for a cache of Hkv <= H heads whose new columns are filed already (rope_kv_append_block_kernel runs first:
// this kernel only reads).  The m new tokens of a sample times the G = H / Hkv query heads of a key/value head are m*G (token, head)
// pairs, p = i*G + g; one workgroup serves one (sample, key/value head) and a block of at most NQ <= 8 consecutive pairs, held in
// registers as the NQ query heads of attn_decode_gqa_kernel are, so every 16-byte K / V load is issued once for the whole block and
// nothing is expanded in memory.  Phase 1 walks the L = len[b] columns filed before this step (L clamped into [0, capacity], uniform
// over the workgroup); phase 2 the new columns L + t, t < m, below the capacity: one per lane group, pair (i, g) folds column t only
// for t <= i (new columns are always valid).  A pair whose own column L + i is at or past the capacity sees the columns below it: its
// output is the caller's to discard.  Same state, rescale per trip and merge as the block kernel; surplus pairs (j >= np) repeat pair
// np - 1 and are not stored.
template <typename T, int D, int NQ>
__global__ __launch_bounds__(AD_WAVES * WAVE) void attn_decode_gqa_block_kernel(const T* __restrict__ q, int ldq, const T* __restrict__ kc,
                                                                                const T* __restrict__ vc, int ldkv, size_t bs_kv, int capacity,
                                                                                const uint8_t* __restrict__ valid, int ld_valid,
                                                                                const int* __restrict__ len, T* __restrict__ out, int W, int H,
                                                                                int Hkv, int ppb, int nblk) {
    typedef typename Vec16<T>::type V;
    constexpr int VEC = 16 / sizeof(T);
    constexpr int LPK = D / VEC;                    // lanes per key
    constexpr int KPI = WAVE / LPK;                 // keys per wave and load instruction
    constexpr float NEG = -FLT_MAX;
    __shared__ float sm_m[AD_WAVES][NQ], sm_l[AD_WAVES][NQ], sm_o[AD_WAVES][NQ][D];

    const int G = H / Hkv;
    const int pb = blockIdx.x % nblk, kvh = (blockIdx.x / nblk) % Hkv, b = blockIdx.x / (nblk * Hkv);
    const int p0 = pb * ppb, np = min(ppb, W * G - p0);                    // pairs p0 .. p0 + np - 1
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane % LPK, kk = lane / LPK;
    const size_t row0 = (size_t)b * W;
    const int S = min(max(len[b], 0), capacity);    // the caller's contract; clamped, never trusted as an address

    float qf[NQ][VEC];
    int tok[NQ];                                    // the pair's token i: wave-uniform
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int p = p0 + min(j, np - 1);
        tok[j] = p / G;
        const V qv = *(const V*)(q + (row0 + tok[j]) * ldq + (kvh * G + p % G) * D + c * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) qf[j][e] = Elem<T>::to_f(qv[e]);
    }
    float m[NQ], l[NQ], acc[NQ][VEC];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        m[j] = NEG;
        l[j] = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[j][e] = 0.f;
    }
    // the keys of a trip enter pair j's online softmax together: one rescale of the state per trip
    auto fold = [&](int j, const auto& kr, const auto& vr, const auto& ok, const auto& in) {
        constexpr int U = sizeof(ok) / sizeof(bool);
        float sc[U], mn = m[j];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float dot = 0.f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) dot += qf[j][e] * Elem<T>::to_f(kr[u][e]);
            dot = group_sum<LPK>(dot);
            sc[u] = ok[u] ? dot : NEG;
            if (in[u]) mn = fmaxf(mn, sc[u]);
        }
        const float corr = __expf(m[j] - mn);
        float pu[U], ps = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            pu[u] = in[u] ? __expf(sc[u] - mn) : 0.f;                 // a key the pair does not see weighs nothing
            ps += pu[u];
        }
        l[j] = l[j] * corr + ps;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float a = acc[j][e] * corr;
#pragma unroll
            for (int u = 0; u < U; ++u) a += pu[u] * Elem<T>::to_f(vr[u][e]);
            acc[j][e] = a;
        }
        m[j] = mn;
    };

    const T* kb = kc + b * bs_kv + kvh * D;
    const T* vb = vc + b * bs_kv + kvh * D;
    const uint32_t row_bytes = (uint32_t)(ldkv * sizeof(T));
    // ---- phase 1: the cache columns below L (branch-free loads: keys past L fall outside the descriptors)
    if (S > 0) {
        const uint32_t slab = (uint32_t)(((size_t)(S - 1) * ldkv + D) * sizeof(T));
        const __amdgpu_buffer_rsrc_t rk = make_rsrc(kb, slab);
        const __amdgpu_buffer_rsrc_t rv = make_rsrc(vb, slab);
        const uint8_t* mb = valid + (size_t)b * ld_valid;
        for (int base = w * KPI; base < S; base += AD_WAVES * KPI * AD_UNROLL) {          // wave-uniform trip count
            V kr[AD_UNROLL], vr[AD_UNROLL];
            bool ok[AD_UNROLL], in[AD_UNROLL];
#pragma unroll
            for (int u = 0; u < AD_UNROLL; ++u) {
                const int s = base + u * AD_WAVES * KPI + kk;
                in[u] = s < S;
                const uint32_t off = in[u] ? (uint32_t)s * row_bytes + (uint32_t)(c * 16) : OOB;
                kr[u] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rk, off, 0, 0));
                vr[u] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rv, off, 0, 0));
                ok[u] = mb[min(s, S - 1)] != 0;
            }
#pragma unroll
            for (int j = 0; j < NQ; ++j) fold(j, kr, vr, ok, in);
        }
    }
    // ---- phase 2: the new columns L .. L + n_new - 1 (n_new = the tokens filed below the capacity), causal among themselves
    const int n_new = min(W, capacity - S);
    if (w * KPI < n_new) {                                                                 // wave-uniform
        const uint32_t span = (uint32_t)(((size_t)(n_new - 1) * ldkv + D) * sizeof(T));
        const __amdgpu_buffer_rsrc_t rk = make_rsrc(kb + (size_t)S * ldkv, span);
        const __amdgpu_buffer_rsrc_t rv = make_rsrc(vb + (size_t)S * ldkv, span);
        const int t = w * KPI + kk;
        const bool mine = t < n_new;
        const uint32_t off = mine ? (uint32_t)t * row_bytes + (uint32_t)(c * 16) : OOB;
        V kr[1], vr[1];
        kr[0] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rk, off, 0, 0));
        vr[0] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rv, off, 0, 0));
        const bool ok[1] = {true};
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const bool in[1] = {mine && t <= tok[j]};
            fold(j, kr, vr, ok, in);
        }
    }
    // per pair: merge the lane groups of the wave (fixed butterfly), then the waves in order
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
#pragma unroll
        for (int o = LPK; o < WAVE; o <<= 1) {
            const float m2 = __shfl_xor(m[j], o), l2 = __shfl_xor(l[j], o);
            const float mn = fmaxf(m[j], m2);
            const float c1 = __expf(m[j] - mn), c2 = __expf(m2 - mn);
            l[j] = l[j] * c1 + l2 * c2;
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[j][e] = acc[j][e] * c1 + __shfl_xor(acc[j][e], o) * c2;
            m[j] = mn;
        }
        if (lane < LPK) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) sm_o[w][j][c * VEC + e] = acc[j][e];
            if (lane == 0) { sm_m[w][j] = m[j]; sm_l[w][j] = l[j]; }
        }
    }
    __syncthreads();
    for (int idx = tid; idx < np * D; idx += AD_WAVES * WAVE) {
        const int j = idx / D, x = idx % D, p = p0 + j;
        float mm = sm_m[0][j];
#pragma unroll
        for (int i = 1; i < AD_WAVES; ++i) mm = fmaxf(mm, sm_m[i][j]);
        float ll = 0.f, o = 0.f;
#pragma unroll
        for (int i = 0; i < AD_WAVES; ++i) {
            const float ci = __expf(sm_m[i][j] - mm);
            ll += sm_l[i][j] * ci;
            o += sm_o[i][j][x] * ci;
        }
        out[((row0 + p / G) * H + kvh * G + p % G) * D + x] = Elem<T>::from_f(o / ll);
    }
}

struct GqaBlockAttnArgs {
    AttnPrefix p;                                  // the sample's cache slabs of Hkv heads (S = capacity); q and out have B*W rows
    const int* len;
    int W;
};

template <typename T, int D>
int attn_decode_gqa_block_nq(const GqaBlockAttnArgs& a, hipStream_t st) {
    const AttnPrefix& p = a.p;
    // pairs per block: 8 shares a K / V load among the most pairs, but with 8 states per lane group the loop is ALU-bound and a small
    // batch leaves most CUs idle.  So the blocks shrink (8 -> 4 -> 2 -> 1) while the grid stays within two workgroups per CU: at
    // B = 2, Hkv = 8, m = 2 that is 128 workgroups of one pair (17 us) instead of 16 of eight (34 us); at 512 workgroups and more the
    // blocks of 8 win.  The re-read K / V of a (sample, head) comes from L2.
    const int P = a.W * (p.H / p.Hkv), room = 2 * mmgl_num_cu();
    int most = 8;
    while (most > 1 && (long long)p.B * p.Hkv * cdiv(P, most / 2) <= room) most /= 2;
    const int nblk = cdiv(P, most), ppb = cdiv(P, nblk);                   // blocks of equal size up to one pair
    const dim3 grid(p.B * p.Hkv * nblk), block(AD_WAVES * WAVE);
#define MMGL_GQA_BLOCK_DECODE(NQ)                                                                                                          \
    hipLaunchKernelGGL((attn_decode_gqa_block_kernel<T, D, NQ>), grid, block, 0, st, (const T*)p.q, p.ldq, (const T*)p.k, (const T*)p.v,   \
                       p.ldkv, p.bs_kv, p.S, p.valid, p.ld_valid, a.len, (T*)p.out, a.W, p.H, p.Hkv, ppb, nblk)
    if (ppb == 1) MMGL_GQA_BLOCK_DECODE(1);
    else if (ppb == 2) MMGL_GQA_BLOCK_DECODE(2);
    else if (ppb <= 4) MMGL_GQA_BLOCK_DECODE(4);
    else MMGL_GQA_BLOCK_DECODE(8);
#undef MMGL_GQA_BLOCK_DECODE
    MMGL_CHECK_LAUNCH("mmgl_attn_decode_gqa_block_fwd");
    return MMGL_OK;
}

// ------------------------------------------------------------------------------------------------ rotary embedding of one new token
// qkv [B, ldqkv] = [q: H heads | k: Hkv | v: Hkv] x D of the new token; cs [D/2] float2 (cos, sin) of its position.  One thread = VN
// consecutive i of one (sample, head): the pair (i, i + D/2) of a q head is rotated in place, that of a k head is rotated into the
// cache column, that of a v head is copied there; the k and v blocks of qkv are only read.  The arithmetic of rope_kernel (llama_ops.hip).
template <typename T>
__global__ __launch_bounds__(256) void rope_kv_append_kernel(T* __restrict__ qkv, int ldqkv, const f32x2* __restrict__ cs, T* __restrict__ kv_col,
                                                             size_t bs_kv, int B, int H, int Hkv, int D) {
    constexpr int VN = 16 / sizeof(T);
    typedef typename Vec16<T>::type V;
    const int half = D / 2, per_head = half / VN, heads = H + 2 * Hkv;
    const int total = B * heads * per_head;
    for (int id = blockIdx.x * 256 + threadIdx.x; id < total; id += gridDim.x * 256) {
        const int b = id / (heads * per_head), rem = id - b * heads * per_head;
        const int hd = rem / per_head, c = rem - hd * per_head;
        T* src = qkv + (size_t)b * ldqkv + (size_t)hd * D + c * VN;
        V lo = *(const V*)src, hi = *(const V*)(src + half);
        if (hd < H + Hkv) {
            const f32x2* a = cs + c * VN;
            V olo, ohi;
#pragma unroll
            for (int e = 0; e < VN; ++e) {
                const float co = a[e][0], si = a[e][1];
                const float x0 = (float)lo[e], x1 = (float)hi[e];
                olo[e] = (T)(x0 * co - x1 * si);
                ohi[e] = (T)(x1 * co + x0 * si);
            }
            lo = olo;
            hi = ohi;
        }
        T* dst = hd < H ? src : kv_col + (size_t)b * bs_kv + (size_t)(hd - H) * D + c * VN;     // k | v in qkv = k | v in the cache row
        *(V*)dst = lo;
        *(V*)(dst + half) = hi;
    }
}

// rope_kv_append_kernel for the rows of a verify step: row b*m + i of qkv is new token i of sample b, at position p = len[b] + i (len
// clamped into [0, capacity]: never trusted as an address).  Its angles are row min(p, n_pos - 1) of the table cs [n_pos, D/2]; its q
// heads are rotated in place; its k and v heads go to column p of the sample's cache rows kv [capacity, ldkv] -- or nowhere when p is at
// or past the capacity.  Same thread layout and arithmetic: m = 1 with equal len is bitwise rope_kv_append_kernel.
template <typename T>
__global__ __launch_bounds__(256) void rope_kv_append_block_kernel(T* __restrict__ qkv, int ldqkv, const f32x2* __restrict__ cs, int n_pos,
                                                                   T* __restrict__ kv, int ldkv, size_t bs_kv, int capacity,
                                                                   const int* __restrict__ len, int rows, int m, int H, int Hkv, int D) {
    constexpr int VN = 16 / sizeof(T);
    typedef typename Vec16<T>::type V;
    const int half = D / 2, per_head = half / VN, heads = H + 2 * Hkv;
    const int total = rows * heads * per_head;
    for (int id = blockIdx.x * 256 + threadIdx.x; id < total; id += gridDim.x * 256) {
        const int r = id / (heads * per_head), rem = id - r * heads * per_head;
        const int hd = rem / per_head, c = rem - hd * per_head;
        const int b = r / m;
        const int p = min(max(len[b], 0), capacity) + (r - b * m);
        if (hd >= H && p >= capacity) continue;                            // a key / value past the cache: dropped
        T* src = qkv + (size_t)r * ldqkv + (size_t)hd * D + c * VN;
        V lo = *(const V*)src, hi = *(const V*)(src + half);
        if (hd < H + Hkv) {
            const f32x2* a = cs + (size_t)min(p, n_pos - 1) * half + c * VN;
            V olo, ohi;
#pragma unroll
            for (int e = 0; e < VN; ++e) {
                const float co = a[e][0], si = a[e][1];
                const float x0 = (float)lo[e], x1 = (float)hi[e];
                olo[e] = (T)(x0 * co - x1 * si);
                ohi[e] = (T)(x1 * co + x0 * si);
            }
            lo = olo;
            hi = ohi;
        }
        T* dst = hd < H ? src : kv + b * bs_kv + (size_t)p * ldkv + (size_t)(hd - H) * D + c * VN;
        *(V*)dst = lo;
        *(V*)(dst + half) = hi;
    }
}

// ------------------------------------------------------------------------------------------------ FP8 key/value cache
// A cached key or value row is stored as OCP e4m3fn codes, 16 per lane and 16-byte access, with one power-of-two scale per (sample,
// column, key-or-value, head): an int8 exponent e, value = code * 2^e.  A cache row is [k codes: H*D | v codes: H*D] bytes and its
// scale row [k exponents: H | v exponents: H].  gfx950 converts both ways in hardware (v_cvt_pk_fp8_f32, round to nearest even;
// v_cvt_pk_f32_fp8), and code * 2^e is exact in fp32, so a dequantised column is the same number in every kernel that reads it.
constexpr int Q8_VEC = 16;                          // codes per lane

template <typename T> __device__ __forceinline__ void load16(const T* p, float (&f)[Q8_VEC]) {
    typedef typename Vec16<T>::type V;
    constexpr int VEC = 16 / sizeof(T);
#pragma unroll
    for (int i = 0; i < Q8_VEC / VEC; ++i) {
        const V x = *(const V*)(p + i * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) f[i * VEC + e] = Elem<T>::to_f(x[e]);
    }
}

// the exponent of a head whose largest magnitude is a: the smallest e with a * 2^-e <= 448 = 0.875 * 2^9, clamped to [-120, 120];
// 0 for a = 0.  With a = m * 2^x, m in [0.5, 1): e = x - 9 if m <= 0.875 else x - 8.  (A subnormal a lands on the clamp.)
__device__ __forceinline__ int q8_exponent(float a) {
    const uint32_t bits = __builtin_bit_cast(uint32_t, a);
    if (bits == 0) return 0;
    const int x = (int)(bits >> 23) - 126;
    const int e = (bits & 0x7fffffu) <= 0x600000u ? x - 9 : x - 8;
    return min(max(e, -120), 120);
}

__device__ __forceinline__ float q8_pow2(int e) { return __builtin_bit_cast(float, (uint32_t)(e + 127) << 23); }

__device__ __forceinline__ u32x4 q8_encode(const float (&f)[Q8_VEC], float inv) {
    u32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int w = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * i] * inv, f[4 * i + 1] * inv, 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * i + 2] * inv, f[4 * i + 3] * inv, w, true);
        r[i] = (uint32_t)w;
    }
    return r;
}

__device__ __forceinline__ void q8_decode(const u32x4& c, float (&f)[Q8_VEC]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[i], true);
        f[4 * i] = lo[0];
        f[4 * i + 1] = lo[1];
        f[4 * i + 2] = hi[0];
        f[4 * i + 3] = hi[1];
    }
}

// max over the N = 2^n <= 8 lanes of an aligned lane group, in every lane of the group
template <int N> __device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int o = 1; o < N; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// the 16 elements a lane holds of one head (D / 16 lanes share the head): their codes, and the head's exponent
template <int LPH> __device__ __forceinline__ u32x4 q8_quantize(const float (&f)[Q8_VEC], int& e) {
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < Q8_VEC; ++i) a = fmaxf(a, fabsf(f[i]));
    e = q8_exponent(group_max<LPH>(a));
    return q8_encode(f, q8_pow2(-e));
}

// mmgl_kv_quantize: one lane per 16 elements of a (sample, row, key-or-value, head); whole lane groups are in or out of `total`.
template <typename T, int D>
__global__ __launch_bounds__(256) void kv_quantize_kernel(const T* __restrict__ k, const T* __restrict__ v, int ld_src, size_t bs_src,
                                                          uint8_t* __restrict__ code, int ld_code, size_t bs_code, int8_t* __restrict__ scale,
                                                          int ld_scale, size_t bs_scale, int n, int H, long long total) {
    constexpr int LPH = D / Q8_VEC;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;                        // total is a multiple of LPH: a lane group leaves together
    const int c = (int)(id % LPH);
    long long r = id / LPH;
    const int hh = (int)(r % (2 * H));              // key heads first, then value heads
    r /= 2 * H;
    const int row = (int)(r % n), b = (int)(r / n);
    const T* src = (hh < H ? k : v) + b * bs_src + (size_t)row * ld_src + (size_t)(hh % H) * D + c * Q8_VEC;
    float f[Q8_VEC];
    load16<T>(src, f);
    int e;
    const u32x4 q = q8_quantize<LPH>(f, e);
    *(u32x4*)(code + b * bs_code + (size_t)row * ld_code + (size_t)hh * D + c * Q8_VEC) = q;
    if (c == 0) scale[b * bs_scale + (size_t)row * ld_scale + hh] = (int8_t)e;
}

// ------------------------------------------------------------------------------------------------ FP8 frozen weights
// A frozen weight [N, K] in the cache's format, per weight row: e4m3fn codes [N, K] (row stride ldc bytes) and one int8 exponent per
// row, value = code * 2^exps[n], exps[n] = q8_exponent(max |w[n, :]|).  Every e4m3 value is exact in bf16, so the decode GEMM keeps
// its bf16 MFMA and its fp32 accumulation and reads half the bytes; the power of two multiplies the folded sum (exact).
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// mmgl_weight_quantize: one wave per weight row, two passes over it (the second re-reads the row from L2): the row's largest magnitude
// by a butterfly (a maximum does not depend on the order), then the codes.  VEC: 16 elements per lane and trip, 16-byte code stores
// (K % 16 == 0 and aligned rows); else element by element.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void weight_quantize_kernel(const T* __restrict__ w, long long ldw, uint8_t* __restrict__ codes, long long ldc,
                                                             int8_t* __restrict__ exps, int N, int K) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;                             // whole waves leave; the kernel has no barrier
    const T* src = w + (size_t)n * ldw;
    uint8_t* dst = codes + (size_t)n * ldc;
    float a = 0.f;
    if (VEC) {
        for (int k = lane * Q8_VEC; k < K; k += WAVE * Q8_VEC) {
            float f[Q8_VEC];
            load16<T>(src + k, f);
#pragma unroll
            for (int i = 0; i < Q8_VEC; ++i) a = fmaxf(a, fabsf(f[i]));
        }
    } else {
        for (int k = lane; k < K; k += WAVE) a = fmaxf(a, fabsf(Elem<T>::to_f(src[k])));
    }
    const int e = q8_exponent(wave_max(a));
    const float inv = q8_pow2(-e);
    if (VEC) {
        for (int k = lane * Q8_VEC; k < K; k += WAVE * Q8_VEC) {
            float f[Q8_VEC];
            load16<T>(src + k, f);
            *(u32x4*)(dst + k) = q8_encode(f, inv);
        }
    } else {
        for (int k = lane; k < K; k += WAVE)
            dst[k] = (uint8_t)__builtin_amdgcn_cvt_pk_fp8_f32(Elem<T>::to_f(src[k]) * inv, 0.f, 0, false);
    }
    if (lane == 0) exps[n] = (int8_t)e;
}

template <typename T> struct SkW8Args {
    SkArgs<T> a;                                    // x, bias, residual, y and the sizes; a.W and a.ldw are unused
    const uint8_t* C; const int8_t* E;
    int ldc;
};

// 8 codes (two 32-bit words, k ascending from the low byte) as a bf16 A fragment: v_cvt_scalef32_pk_bf16_fp8, scale 1
__device__ __forceinline__ bf16x8 w8_frag(uint32_t lo, uint32_t hi) {
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
    const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
    const bf16x4 ab = __builtin_shufflevector(a, b, 0, 1, 2, 3), cd = __builtin_shufflevector(c, d, 0, 1, 2, 3);
    return __builtin_shufflevector(ab, cd, 0, 1, 2, 3, 4, 5, 6, 7);
}

// mmgl_gemm_skinny_w8, bf16: skinny_mfma_kernel on code loads.  The K unit is 128 codes = one 128-byte line of a weight row: lane
// (i, g) reads codes[n0 + i][128 p + 64 h + 16 g .. + 15] for h = 0, 1, so each of the two 16-byte loads of a unit covers a 64-byte
// half line over the four lane groups and the pair the whole line.  Half h of unit p is "pair" 2 p + h of skinny_mfma_kernel: the
// same 64 x columns, staged and read the same way, and MFMA t of it contracts k = 128 p + 64 h + 16 g + 8 t + (0..7).  The K slots
// are dealt unit by unit (slot s takes units s, s + NS, ...); a ring of DW units = DW x 32 bytes per lane is in flight, the bytes
// skinny_mfma_kernel keeps in flight over twice the K.  Codes become bf16 fragments in registers (w8_frag); the row's power of two
// multiplies the folded fp32 sum in front of the epilogue.
template <int MT, bool HALF>
__global__ __launch_bounds__(SK_THREADS) void skinny_w8_mfma_kernel(const SkW8Args<bf16> q) {
    constexpr int SL = HALF ? 2 : 1;               // K slots per wave
    constexpr int ROWS = HALF ? 8 : 16;            // weight rows per workgroup
    constexpr int NS = SK_WAVES * SL;              // K slots per workgroup
    constexpr int MR = MT * 16;                    // x rows held (rows >= M are zeros)
    constexpr int XL = MR / 8;                     // x loads per lane, slot and half unit
    constexpr int DW = 4;                          // W units in flight per lane
    constexpr int DX = MT == 1 ? 4 : MT == 2 ? 2 : 1;      // x half units in flight per lane
    __shared__ __attribute__((aligned(16))) unsigned char smem[NS * MR * 128];      // x staging of one half unit; the fold reuses it

    const SkArgs<bf16>& a = q.a;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * ROWS;
    const int P = a.K >> 7;
    const int iters = (P + NS - 1) / NS;
    const int wslot = HALF ? w * 2 + (i >> 3) : w;
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(q.C + (size_t)n0 * q.ldc, (uint32_t)((size_t)(ROWS - 1) * q.ldc + a.K));
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.X, (uint32_t)(((size_t)(a.M - 1) * a.ldx + a.K) * 2));
    const uint32_t woff = (uint32_t)((HALF ? (i & 7) : i) * q.ldc + 16 * g);
    const int xr_row = lane >> 3, xr_c = lane & 7;

    u32x4 wr[DW][2];
    bf16x8 xr[DX][SL * XL];
    auto load_w = [&](int it, u32x4 (&dst)[2]) {
        const int p = it * NS + wslot;
        const uint32_t off = p < P ? woff + (uint32_t)p * 128u : OOB;
        dst[0] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, off, 0, 2));              // aux 2: non-temporal
        dst[1] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, off + 64u, 0, 2));
    };
    auto load_x = [&](int j, bf16x8 (&dst)[SL * XL]) {          // j: half unit 2 it + h of the slots' sequence
#pragma unroll
        for (int sl = 0; sl < SL; ++sl) {
            const int p = (j >> 1) * NS + w * SL + sl;
#pragma unroll
            for (int r8 = 0; r8 < XL; ++r8) {
                const int r = r8 * 8 + xr_row;
                const uint32_t off = (p < P && r < a.M)
                                         ? ((uint32_t)r * (uint32_t)a.ldx + (uint32_t)p * 128u + (uint32_t)(j & 1) * 64u + (uint32_t)xr_c * 8u) * 2u
                                         : OOB;
                dst[sl * XL + r8] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
            }
        }
    };
#pragma unroll
    for (int u = 0; u < DW; ++u) load_w(u, wr[u]);
#pragma unroll
    for (int u = 0; u < DX; ++u) load_x(u, xr[u]);

    f32x4 acc0[MT], acc1[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) { acc0[mt] = vzero<f32x4>(); acc1[mt] = vzero<f32x4>(); }

    unsigned char* xs = smem + (size_t)w * SL * MR * 128;          // this wave's staging image
    for (int it0 = 0; it0 < iters; it0 += DW) {
#pragma unroll
        for (int u = 0; u < DW; ++u) {
            const int it = it0 + u;
            if (it < iters) {                                       // uniform over the workgroup
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int xi = (2 * u + h) % DX;                // = (2 it + h) % DX: DX divides 2 DW
#pragma unroll
                    for (int sl = 0; sl < SL; ++sl)
#pragma unroll
                        for (int r8 = 0; r8 < XL; ++r8) {
                            const int r = r8 * 8 + xr_row;
                            *(bf16x8*)(xs + ((sl * MR + r) * 128) + ((xr_c ^ (r & 7)) << 4)) = xr[xi][sl * XL + r8];
                        }
                    __syncthreads();
                    load_x(2 * it + h + DX, xr[xi]);
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const bf16x8 af = w8_frag(wr[u][h][2 * t], wr[u][h][2 * t + 1]);
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
                            const int row = mt * 16 + i;
                            const int off = row * 128 + (((2 * g + t) ^ (i & 7)) << 4);
                            const bf16x8 b0 = *(const bf16x8*)(xs + off);
                            mma16(acc0[mt], af, b0);
                            if (HALF) {
                                const bf16x8 b1 = *(const bf16x8*)(xs + MR * 128 + off);
                                mma16(acc1[mt], af, b1);
                            }
                        }
                    }
                    if (h == 1) load_w(it + DW, wr[u]);
                    __syncthreads();
                }
            }
        }
    }

    // fold: part[slot][m][ROWS] fp32, summed in slot order, then the row's power of two
    float* part = (float*)smem;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if (HALF) {
            const int slot = 2 * w + (g >> 1);
            *(f32x4*)&part[((size_t)slot * MR + mt * 16 + i) * 8 + 4 * (g & 1)] = g < 2 ? acc0[mt] : acc1[mt];
        } else {
            *(f32x4*)&part[((size_t)w * MR + mt * 16 + i) * 16 + 4 * g] = acc0[mt];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < ROWS * a.M; idx += SK_THREADS) {
        const int n = idx % ROWS, m = idx / ROWS;
        float s = 0.f;
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) s += part[((size_t)sl * MR + m) * ROWS + n];
        sk_store(a, m, n0 + n, s * q8_pow2(q.E[n0 + n]));
    }
}

// skinny_generic_kernel on codes: one wave per output column, 8 rows of x per wave, fp32 accumulation, any K, N, stride and alignment
template <typename T>
__global__ __launch_bounds__(256) void skinny_w8_generic_kernel(const SkW8Args<T> q) {
    const SkArgs<T>& a = q.a;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = blockIdx.x * 4 + w, m0 = blockIdx.y * 8;
    if (n >= a.N) return;                           // whole waves leave; the kernel has no barrier
    float acc[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = 0.f;
    const uint8_t* crow = q.C + (size_t)n * q.ldc;
    for (int k = lane; k < a.K; k += WAVE) {
        const float wv = __builtin_amdgcn_cvt_f32_fp8((int)crow[k], 0);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int m = min(m0 + r, a.M - 1);
            acc[r] += wv * Elem<T>::to_f(a.X[(size_t)m * a.ldx + k]);
        }
    }
    float mine = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const float s = wave_sum(acc[r]);
        if (lane == r) mine = s;
    }
    if (lane < 8 && m0 + lane < a.M) sk_store(a, m0 + lane, n, mine * q8_pow2(q.E[n]));
}

template <int MT, bool HALF> int launch_skinny_w8_mfma(const SkW8Args<bf16>& q, hipStream_t st) {
    hipLaunchKernelGGL((skinny_w8_mfma_kernel<MT, HALF>), dim3(q.a.N / (HALF ? 8 : 16)), dim3(SK_THREADS), 0, st, q);
    MMGL_CHECK_LAUNCH("mmgl_gemm_skinny_w8");
    return MMGL_OK;
}

template <bool HALF> int launch_skinny_w8_mt(const SkW8Args<bf16>& q, hipStream_t st) {
    if (q.a.M <= 16) return launch_skinny_w8_mfma<1, HALF>(q, st);
    if (q.a.M <= 32) return launch_skinny_w8_mfma<2, HALF>(q, st);
    return launch_skinny_w8_mfma<4, HALF>(q, st);
}

template <typename T> int launch_skinny_w8_generic(const SkW8Args<T>& q, hipStream_t st) {
    hipLaunchKernelGGL((skinny_w8_generic_kernel<T>), dim3(cdiv(q.a.N, 4), cdiv(q.a.M, 8)), dim3(256), 0, st, q);
    MMGL_CHECK_LAUNCH("mmgl_gemm_skinny_w8");
    return MMGL_OK;
}

// the route of a bf16 call on codes: skinny_bf16's rule with the 128-code unit and 16-byte code rows
int skinny_w8_bf16(const SkW8Args<bf16>& q, hipStream_t st) {
    const SkArgs<bf16>& a = q.a;
    const bool mfma = a.K % 128 == 0 && a.N % 8 == 0 && a.ldx % 8 == 0 && q.ldc % 16 == 0 && aligned16(a.X) && aligned16(q.C) &&
                      ((size_t)(a.M - 1) * a.ldx + a.K) * 2 < (1ull << 31) && (size_t)16 * q.ldc < (1ull << 31);
    if (!mfma) return launch_skinny_w8_generic<bf16>(q, st);
    if (a.N % 16 == 0 && a.N / 16 >= mmgl_num_cu()) return launch_skinny_w8_mt<false>(q, st);
    return launch_skinny_w8_mt<true>(q, st);
}

template <typename T> int launch_weight_quantize(const void* w, int ldw, void* codes, int ldc, void* exps, int N, int K, hipStream_t st) {
    const bool vec = K % Q8_VEC == 0 && ((size_t)ldw * sizeof(T)) % 16 == 0 && ldc % 16 == 0 && aligned16(w) && aligned16(codes);
    const dim3 grid(cdiv(N, 4)), block(256);
    if (vec) hipLaunchKernelGGL((weight_quantize_kernel<T, true>), grid, block, 0, st, (const T*)w, (long long)ldw, (uint8_t*)codes, (long long)ldc, (int8_t*)exps, N, K);
    else hipLaunchKernelGGL((weight_quantize_kernel<T, false>), grid, block, 0, st, (const T*)w, (long long)ldw, (uint8_t*)codes, (long long)ldc, (int8_t*)exps, N, K);
    MMGL_CHECK_LAUNCH("mmgl_weight_quantize");
    return MMGL_OK;
}

// mmgl_attn_decode_q8_fwd: attn_decode_kernel over a cache of codes.  D / 16 lanes share a key (one 16-byte load of K codes and one
// of V codes per lane: 16 codes), a wave covers 1024 / D keys per instruction, the 4 waves interleave key blocks and AD_UNROLL blocks
// are in flight; keys past S fall outside the descriptors.  The key's scale multiplies the dot product, the value's scale multiplies
// p; the AD_UNROLL keys of a trip enter the fp32 online softmax together.  The new token's key and value come dense, in T, from the
// projection's output: lane group 0 of the last wave scores the key unquantised (it is always valid, so a row of masked cached keys
// weighs only it), then quantises both and files codes and exponents at column S -- one writer per (sample, head, column), and no
// workgroup reads column S.  Merge as attn_decode_kernel: fixed butterfly, then the waves in order through LDS; no atomics.
template <typename T, int D>
__global__ __launch_bounds__(AD_WAVES * WAVE) void attn_decode_q8_kernel(const T* __restrict__ q, int ldq, const T* __restrict__ kn,
                                                                         const T* __restrict__ vn, int ld_new, uint8_t* kc, uint8_t* vc,
                                                                         int ld_code, size_t bs_code, int8_t* ks, int8_t* vs, int ld_scale,
                                                                         size_t bs_scale, const uint8_t* __restrict__ valid, int ld_valid,
                                                                         T* __restrict__ out, int H, int S) {
    constexpr int LPK = D / Q8_VEC;                 // lanes per key
    constexpr int KPI = WAVE / LPK;                 // keys per wave and load instruction
    constexpr float NEG = -FLT_MAX;
    __shared__ float sm_m[AD_WAVES], sm_l[AD_WAVES], sm_o[AD_WAVES][D];

    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane % LPK, kk = lane / LPK;

    float qf[Q8_VEC];
    load16<T>(q + (size_t)b * ldq + h * D + c * Q8_VEC, qf);
    uint8_t* kb = kc + b * bs_code + h * D;
    uint8_t* vb = vc + b * bs_code + h * D;
    int8_t* ksb = ks + b * bs_scale + h;
    int8_t* vsb = vs + b * bs_scale + h;
    // branch-free loads: keys past S fall outside the descriptors
    const uint32_t slab = (uint32_t)((size_t)(S - 1) * ld_code + D), row_bytes = (uint32_t)ld_code;
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(kb, slab);
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(vb, slab);
    const uint8_t* mb = valid + (size_t)b * ld_valid;

    float m = NEG, l = 0.f, acc[Q8_VEC];
#pragma unroll
    for (int e = 0; e < Q8_VEC; ++e) acc[e] = 0.f;

    for (int base = w * KPI; base < S; base += AD_WAVES * KPI * AD_UNROLL) {          // wave-uniform trip count
        u32x4 kr[AD_UNROLL], vr[AD_UNROLL];
        int ke[AD_UNROLL], ve[AD_UNROLL];
        bool ok[AD_UNROLL], in[AD_UNROLL];
#pragma unroll
        for (int u = 0; u < AD_UNROLL; ++u) {
            const int s = base + u * AD_WAVES * KPI + kk;
            in[u] = s < S;
            const uint32_t off = in[u] ? (uint32_t)s * row_bytes + (uint32_t)(c * Q8_VEC) : OOB;
            kr[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rk, off, 0, 0));
            vr[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rv, off, 0, 0));
            const int sc = min(s, S - 1);
            ok[u] = mb[sc] != 0;
            ke[u] = ksb[(size_t)sc * ld_scale];
            ve[u] = vsb[(size_t)sc * ld_scale];
        }
        float sc[AD_UNROLL], mn = m;
#pragma unroll
        for (int u = 0; u < AD_UNROLL; ++u) {
            float kf[Q8_VEC], dot = 0.f;
            q8_decode(kr[u], kf);
#pragma unroll
            for (int e = 0; e < Q8_VEC; ++e) dot += qf[e] * kf[e];
            dot = group_sum<LPK>(dot) * q8_pow2(ke[u]);
            sc[u] = ok[u] ? dot : NEG;
            if (in[u]) mn = fmaxf(mn, sc[u]);
        }
        const float corr = __expf(m - mn);
        float pu[AD_UNROLL], ps = 0.f;
#pragma unroll
        for (int u = 0; u < AD_UNROLL; ++u) {
            pu[u] = in[u] ? __expf(sc[u] - mn) : 0.f;                 // a key past S weighs nothing, also in a group of masked keys
            ps += pu[u];
        }
        l = l * corr + ps;
#pragma unroll
        for (int e = 0; e < Q8_VEC; ++e) acc[e] *= corr;
#pragma unroll
        for (int u = 0; u < AD_UNROLL; ++u) {
            float vf[Q8_VEC];
            q8_decode(vr[u], vf);
            const float pv = in[u] ? pu[u] * q8_pow2(ve[u]) : 0.f;    // the exponent of a key past S is another column's
#pragma unroll
            for (int e = 0; e < Q8_VEC; ++e) acc[e] += pv * vf[e];
        }
        m = mn;
    }
    // the new token: scored and weighed as it came, filed as codes
    if (w == AD_WAVES - 1 && kk == 0) {
        float kf[Q8_VEC], vf[Q8_VEC], dot = 0.f;
        load16<T>(kn + (size_t)b * ld_new + h * D + c * Q8_VEC, kf);
        load16<T>(vn + (size_t)b * ld_new + h * D + c * Q8_VEC, vf);
#pragma unroll
        for (int e = 0; e < Q8_VEC; ++e) dot += qf[e] * kf[e];
        dot = group_sum<LPK>(dot);
        const float mn = fmaxf(m, dot);
        const float corr = __expf(m - mn), p = __expf(dot - mn);
        l = l * corr + p;
#pragma unroll
        for (int e = 0; e < Q8_VEC; ++e) acc[e] = acc[e] * corr + p * vf[e];
        m = mn;
        int ek, ev;
        const u32x4 kq = q8_quantize<LPK>(kf, ek), vq = q8_quantize<LPK>(vf, ev);
        const size_t at = (size_t)S * ld_code + c * Q8_VEC;
        *(u32x4*)(kb + at) = kq;
        *(u32x4*)(vb + at) = vq;
        if (c == 0) {
            ksb[(size_t)S * ld_scale] = (int8_t)ek;
            vsb[(size_t)S * ld_scale] = (int8_t)ev;
        }
    }
    // merge the lane groups of the wave (fixed butterfly), then the waves in order
#pragma unroll
    for (int o = LPK; o < WAVE; o <<= 1) {
        const float m2 = __shfl_xor(m, o), l2 = __shfl_xor(l, o);
        const float mn = fmaxf(m, m2);
        const float c1 = __expf(m - mn), c2 = __expf(m2 - mn);
        l = l * c1 + l2 * c2;
#pragma unroll
        for (int e = 0; e < Q8_VEC; ++e) acc[e] = acc[e] * c1 + __shfl_xor(acc[e], o) * c2;
        m = mn;
    }
    if (lane < LPK) {
#pragma unroll
        for (int e = 0; e < Q8_VEC; ++e) sm_o[w][c * Q8_VEC + e] = acc[e];
        if (lane == 0) { sm_m[w] = m; sm_l[w] = l; }
    }
    __syncthreads();
    if (tid < D) {
        float mm = sm_m[0];
#pragma unroll
        for (int i = 1; i < AD_WAVES; ++i) mm = fmaxf(mm, sm_m[i]);
        float ll = 0.f, o = 0.f;
#pragma unroll
        for (int i = 0; i < AD_WAVES; ++i) {
            const float ci = __expf(sm_m[i] - mm);
            ll += sm_l[i] * ci;
            o += sm_o[i][tid] * ci;
        }
        out[((size_t)b * H + h) * D + tid] = Elem<T>::from_f(o / ll);
    }
}

struct KvQuantArgs {
    const void *k, *v;
    uint8_t* code;
    int8_t* scale;
    int ld_src, ld_code, ld_scale, B, n, H;
    size_t bs_src, bs_code, bs_scale;
};

template <typename T, int D>
int launch_kv_quantize(const KvQuantArgs& a, hipStream_t st) {
    const long long total = (long long)a.B * a.n * 2 * a.H * (D / Q8_VEC);
    hipLaunchKernelGGL((kv_quantize_kernel<T, D>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const T*)a.k, (const T*)a.v, a.ld_src,
                       a.bs_src, a.code, a.ld_code, a.bs_code, a.scale, a.ld_scale, a.bs_scale, a.n, a.H, total);
    MMGL_CHECK_LAUNCH("mmgl_kv_quantize");
    return MMGL_OK;
}

struct Q8AttnArgs {
    const void *q, *kn, *vn;
    uint8_t *kc, *vc;
    int8_t *ks, *vs;
    const uint8_t* valid;
    void* out;
    int ldq, ld_new, ld_code, ld_scale, ld_valid, B, H, S;
    size_t bs_code, bs_scale;
};

template <typename T, int D>
int launch_attn_decode_q8(const Q8AttnArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((attn_decode_q8_kernel<T, D>), dim3(a.B * a.H), dim3(AD_WAVES * WAVE), 0, st, (const T*)a.q, a.ldq, (const T*)a.kn,
                       (const T*)a.vn, a.ld_new, a.kc, a.vc, a.ld_code, a.bs_code, a.ks, a.vs, a.ld_scale, a.bs_scale, a.valid, a.ld_valid,
                       (T*)a.out, a.H, a.S);
    MMGL_CHECK_LAUNCH("mmgl_attn_decode_q8_fwd");
    return MMGL_OK;
}

// mmgl_attn_decode_gqa_q8_fwd: attn_decode_q8_kernel over a cache of Hkv <= H key/value heads, with the workgroups of
// attn_decode_gqa_kernel: one per (sample, key/value head, block of NQ <= Q8_GQA_HEADS of the G = H / Hkv query heads that read it).
// Lane layout, trip constants and descriptors are attn_decode_q8_kernel's (16 codes per lane and 16-byte load).  A trip decodes each of
// its AD_UNROLL keys ONCE into 16 fp32 registers and scores it against the NQ queries from registers, then does the same with the
// values: the 16 conversions per load are paid once per NQ dot products.  The block is capped at 4 heads, not the bf16 kernel's 8:
// qf and acc cost 32 registers per head at 16 codes per lane (DESIGN.md 4.19 has the table).  A block with nq < NQ heads repeats its
// last head and stores nq rows.  The new token: lane group 0 of the last wave of EVERY block folds the unquantised key and value of the
// kv head into its NQ states; block 0 of the group alone quantises them and files column S -- one writer per (sample, kv head).
constexpr int Q8_GQA_HEADS = 4;

// The second launch bound (waves per SIMD) holds the allocation to 168 registers for NQ = 1 and to 256 for NQ = 2, where the compiler
// left alone spends 257 (fp32, D = 64) and halves the waves that keep loads in flight.  NQ = 4 is left alone: it fits 2 waves
// everywhere but bf16 D = 16 (260 registers, 1 wave), and a bound there costs scratch.
template <typename T, int D, int NQ>
__global__ __launch_bounds__(AD_WAVES * WAVE, NQ == 1 ? 3 : NQ == 2 ? 2 : 1) void attn_decode_gqa_q8_kernel(const T* __restrict__ q, int ldq, const T* __restrict__ kn,
                                                                             const T* __restrict__ vn, int ld_new, uint8_t* kc, uint8_t* vc,
                                                                             int ld_code, size_t bs_code, int8_t* ks, int8_t* vs, int ld_scale,
                                                                             size_t bs_scale, const uint8_t* __restrict__ valid, int ld_valid,
                                                                             T* __restrict__ out, int H, int Hkv, int S, int qpb, int nblk) {
    constexpr int LPK = D / Q8_VEC;                 // lanes per key
    constexpr int KPI = WAVE / LPK;                 // keys per wave and load instruction
    constexpr float NEG = -FLT_MAX;
    __shared__ float sm_m[AD_WAVES][NQ], sm_l[AD_WAVES][NQ], sm_o[AD_WAVES][NQ][D];

    const int G = H / Hkv;
    const int qb = blockIdx.x % nblk, kvh = (blockIdx.x / nblk) % Hkv, b = blockIdx.x / (nblk * Hkv);
    const int h0 = kvh * G + qb * qpb, nq = min(qpb, G - qb * qpb);        // query heads h0 .. h0 + nq - 1
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane % LPK, kk = lane / LPK;

    float qf[NQ][Q8_VEC];
#pragma unroll
    for (int j = 0; j < NQ; ++j) load16<T>(q + (size_t)b * ldq + (h0 + min(j, nq - 1)) * D + c * Q8_VEC, qf[j]);
    uint8_t* kb = kc + b * bs_code + kvh * D;
    uint8_t* vb = vc + b * bs_code + kvh * D;
    int8_t* ksb = ks + b * bs_scale + kvh;
    int8_t* vsb = vs + b * bs_scale + kvh;
    // branch-free loads: keys past S fall outside the descriptors
    const uint32_t slab = (uint32_t)((size_t)(S - 1) * ld_code + D), row_bytes = (uint32_t)ld_code;
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(kb, slab);
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(vb, slab);
    const uint8_t* mb = valid + (size_t)b * ld_valid;

    float m[NQ], l[NQ], acc[NQ][Q8_VEC];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        m[j] = NEG;
        l[j] = 0.f;
#pragma unroll
        for (int e = 0; e < Q8_VEC; ++e) acc[j][e] = 0.f;
    }

    for (int base = w * KPI; base < S; base += AD_WAVES * KPI * AD_UNROLL) {          // wave-uniform trip count
        u32x4 kr[AD_UNROLL], vr[AD_UNROLL];
        int ke[AD_UNROLL], ve[AD_UNROLL];
        bool ok[AD_UNROLL], in[AD_UNROLL];
#pragma unroll
        for (int u = 0; u < AD_UNROLL; ++u) {
            const int s = base + u * AD_WAVES * KPI + kk;
            in[u] = s < S;
            const uint32_t off = in[u] ? (uint32_t)s * row_bytes + (uint32_t)(c * Q8_VEC) : OOB;
            kr[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rk, off, 0, 0));
            vr[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rv, off, 0, 0));
            const int sc = min(s, S - 1);
            ok[u] = mb[sc] != 0;
            ke[u] = ksb[(size_t)sc * ld_scale];
            ve[u] = vsb[(size_t)sc * ld_scale];
        }
        // each key is dequantised once and scored against the NQ queries
        float sc[NQ][AD_UNROLL];
#pragma unroll
        for (int u = 0; u < AD_UNROLL; ++u) {
            float kf[Q8_VEC];
            q8_decode(kr[u], kf);
            const float kscale = q8_pow2(ke[u]);
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                float dot = 0.f;
#pragma unroll
                for (int e = 0; e < Q8_VEC; ++e) dot += qf[j][e] * kf[e];
                dot = group_sum<LPK>(dot) * kscale;
                sc[j][u] = ok[u] ? dot : NEG;
            }
        }
        // the trip's AD_UNROLL keys enter each online softmax together: one rescale of a state per trip
        float pv[NQ][AD_UNROLL];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            float mn = m[j];
#pragma unroll
            for (int u = 0; u < AD_UNROLL; ++u)
                if (in[u]) mn = fmaxf(mn, sc[j][u]);
            const float corr = __expf(m[j] - mn);
            float ps = 0.f;
#pragma unroll
            for (int u = 0; u < AD_UNROLL; ++u) {
                const float p = in[u] ? __expf(sc[j][u] - mn) : 0.f;  // a key past S weighs nothing, also in a group of masked keys
                ps += p;
                pv[j][u] = in[u] ? p * q8_pow2(ve[u]) : 0.f;          // the exponent of a key past S is another column's
            }
            l[j] = l[j] * corr + ps;
#pragma unroll
            for (int e = 0; e < Q8_VEC; ++e) acc[j][e] *= corr;
            m[j] = mn;
        }
#pragma unroll
        for (int u = 0; u < AD_UNROLL; ++u) {
            float vf[Q8_VEC];
            q8_decode(vr[u], vf);
#pragma unroll
            for (int j = 0; j < NQ; ++j)
#pragma unroll
                for (int e = 0; e < Q8_VEC; ++e) acc[j][e] += pv[j][u] * vf[e];
        }
    }
    // the new token: scored and weighed as it came by every block, filed as codes by block 0 of the group
    if (w == AD_WAVES - 1 && kk == 0) {
        float kf[Q8_VEC], vf[Q8_VEC];
        load16<T>(kn + (size_t)b * ld_new + kvh * D + c * Q8_VEC, kf);
        load16<T>(vn + (size_t)b * ld_new + kvh * D + c * Q8_VEC, vf);
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            float dot = 0.f;
#pragma unroll
            for (int e = 0; e < Q8_VEC; ++e) dot += qf[j][e] * kf[e];
            dot = group_sum<LPK>(dot);
            const float mn = fmaxf(m[j], dot);
            const float corr = __expf(m[j] - mn), p = __expf(dot - mn);
            l[j] = l[j] * corr + p;
#pragma unroll
            for (int e = 0; e < Q8_VEC; ++e) acc[j][e] = acc[j][e] * corr + p * vf[e];
            m[j] = mn;
        }
        if (qb == 0) {
            int ek, ev;
            const u32x4 kq = q8_quantize<LPK>(kf, ek), vq = q8_quantize<LPK>(vf, ev);
            const size_t at = (size_t)S * ld_code + c * Q8_VEC;
            *(u32x4*)(kb + at) = kq;
            *(u32x4*)(vb + at) = vq;
            if (c == 0) {
                ksb[(size_t)S * ld_scale] = (int8_t)ek;
                vsb[(size_t)S * ld_scale] = (int8_t)ev;
            }
        }
    }
    // per query head: merge the lane groups of the wave (fixed butterfly), then the waves in order
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
#pragma unroll
        for (int o = LPK; o < WAVE; o <<= 1) {
            const float m2 = __shfl_xor(m[j], o), l2 = __shfl_xor(l[j], o);
            const float mn = fmaxf(m[j], m2);
            const float c1 = __expf(m[j] - mn), c2 = __expf(m2 - mn);
            l[j] = l[j] * c1 + l2 * c2;
#pragma unroll
            for (int e = 0; e < Q8_VEC; ++e) acc[j][e] = acc[j][e] * c1 + __shfl_xor(acc[j][e], o) * c2;
            m[j] = mn;
        }
        if (lane < LPK) {
#pragma unroll
            for (int e = 0; e < Q8_VEC; ++e) sm_o[w][j][c * Q8_VEC + e] = acc[j][e];
            if (lane == 0) { sm_m[w][j] = m[j]; sm_l[w][j] = l[j]; }
        }
    }
    __syncthreads();
    for (int idx = tid; idx < nq * D; idx += AD_WAVES * WAVE) {
        const int j = idx / D, x = idx % D;
        float mm = sm_m[0][j];
#pragma unroll
        for (int i = 1; i < AD_WAVES; ++i) mm = fmaxf(mm, sm_m[i][j]);
        float ll = 0.f, o = 0.f;
#pragma unroll
        for (int i = 0; i < AD_WAVES; ++i) {
            const float ci = __expf(sm_m[i][j] - mm);
            ll += sm_l[i][j] * ci;
            o += sm_o[i][j][x] * ci;
        }
        out[((size_t)b * H + h0 + j) * D + x] = Elem<T>::from_f(o / ll);
    }
}

template <typename T, int D>
int attn_decode_gqa_q8_nq(const Q8AttnArgs& a, int Hkv, hipStream_t st) {
    const int G = a.H / Hkv, nblk = cdiv(G, Q8_GQA_HEADS), qpb = cdiv(G, nblk);     // G > 4: further blocks, of equal size up to one head
    const dim3 grid(a.B * Hkv * nblk), block(AD_WAVES * WAVE);
#define MMGL_GQA_Q8_DECODE(NQ)                                                                                                            \
    hipLaunchKernelGGL((attn_decode_gqa_q8_kernel<T, D, NQ>), grid, block, 0, st, (const T*)a.q, a.ldq, (const T*)a.kn, (const T*)a.vn,   \
                       a.ld_new, a.kc, a.vc, a.ld_code, a.bs_code, a.ks, a.vs, a.ld_scale, a.bs_scale, a.valid, a.ld_valid, (T*)a.out, a.H, \
                       Hkv, a.S, qpb, nblk)
    if (qpb == 1) MMGL_GQA_Q8_DECODE(1);
    else if (qpb == 2) MMGL_GQA_Q8_DECODE(2);
    else MMGL_GQA_Q8_DECODE(4);
#undef MMGL_GQA_Q8_DECODE
    MMGL_CHECK_LAUNCH("mmgl_attn_decode_gqa_q8_fwd");
    return MMGL_OK;
}

// what every single-query attention entry point over a cache of codes refuses (Hkv key/value heads in the cache rows, H query heads),
// after its own test of the sizes
int check_attn_q8(const char* who, const Q8AttnArgs& a, int Hkv, int capacity, int D, int dtype) {
    MMGL_CHECK_ARG(dtype == MMGL_BF16 || dtype == MMGL_F32, "%s: bad dtype %d", who, dtype);
    if (D != 16 && D != 32 && D != 64 && D != 128) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: head_dim %d (16, 32, 64, 128)", who, D);
    const int vec = dtype == MMGL_BF16 ? 8 : 4;
    if (a.ldq % vec || a.ld_new % vec || a.ld_code % 16 || a.bs_code % 16)
        MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: strides (%d, %d, %d, %zu) must be multiples of 16 bytes", who, a.ldq, a.ld_new, a.ld_code, a.bs_code);
    MMGL_CHECK_ARG(a.q && a.kn && a.vn && a.kc && a.vc && a.ks && a.vs && a.valid && a.out, "%s: null pointer", who);
    const long long hd = (long long)a.H * D, kd = (long long)Hkv * D;
    MMGL_CHECK_ARG(a.ldq >= hd && a.ld_new >= kd && a.ld_code >= kd && a.ld_scale >= Hkv && a.ld_valid >= a.S &&
                       (a.B == 1 || (a.bs_code >= (size_t)(capacity - 1) * a.ld_code + (size_t)kd &&
                                     a.bs_scale >= (size_t)(capacity - 1) * a.ld_scale + (size_t)Hkv)),
                   "%s: strides (%d, %d, %d, %zu, %d, %zu, %d) smaller than the rows", who, a.ldq, a.ld_new, a.ld_code, a.bs_code, a.ld_scale,
                   a.bs_scale, a.ld_valid);
    if (!aligned16(a.q) || !aligned16(a.kn) || !aligned16(a.vn) || !aligned16(a.kc) || !aligned16(a.vc))
        MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: q, k_new, v_new, k_codes and v_codes must be 16-byte aligned", who);
    if ((size_t)(capacity - 1) * a.ld_code + D >= (1ull << 31))
        MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: a sample's cache rows span 2 GiB or more (capacity=%d, ld_code=%d)", who, capacity, a.ld_code);
    return MMGL_OK;
}

// what the two skinny GEMM entry points refuse alike (their sizes and leading dimensions differ by the adapter's).  ptrs: every
// required pointer is set; hint: the way out of M > 64 that `who` offers
int check_skinny(const char* who, const char* hint, bool ptrs, int M, int act, int dtype) {
    if (M > 64) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: M=%d > 64 rows (%s)", who, M, hint);
    MMGL_CHECK_ARG(dtype == MMGL_BF16 || dtype == MMGL_F32, "%s: bad dtype %d", who, dtype);
    MMGL_CHECK_ARG(ptrs, "%s: null pointer", who);
    MMGL_CHECK_ARG(act == MMGL_ACT_NONE || act == MMGL_ACT_RELU, "%s: unknown activation %d", who, act);
    return MMGL_OK;
}

// what every single-query attention entry point refuses about its prefix operands, after its own test of the sizes.  kv, rows, s_name
// and ld_name are the entry point's words for its keys in the messages.
int check_attn_prefix(const AttnPrefix& a, const char* who, const char* kv = "k and v", const char* rows = "key", const char* s_name = "S",
                      const char* ld_name = "ldkv") {
    MMGL_CHECK_ARG(a.dtype == MMGL_BF16 || a.dtype == MMGL_F32, "%s: bad dtype %d", who, a.dtype);
    if (a.D != 16 && a.D != 32 && a.D != 64 && a.D != 128) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: head_dim %d (16, 32, 64, 128)", who, a.D);
    const int vec = a.dtype == MMGL_BF16 ? 8 : 4;
    if (a.ldq % vec || a.ldkv % vec || a.bs_kv % vec)
        MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: strides (%d, %d, %zu) must be multiples of 16 bytes", who, a.ldq, a.ldkv, a.bs_kv);
    MMGL_CHECK_ARG(a.q && a.k && a.v && a.valid && a.out, "%s: null pointer", who);
    MMGL_CHECK_ARG(a.ldq >= a.H * a.D && a.ldkv >= a.Hkv * a.D && a.ld_valid >= a.S, "%s: strides (%d, %d, %d) smaller than the rows", who, a.ldq,
                   a.ldkv, a.ld_valid);
    if (!aligned16(a.q) || !aligned16(a.k) || !aligned16(a.v)) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: q, %s must be 16-byte aligned", who, kv);
    if (((size_t)(a.S - 1) * a.ldkv + a.D) * (a.dtype == MMGL_BF16 ? 2 : 4) >= (1ull << 31))
        MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: a sample's %s rows span 2 GiB or more (%s=%d, %s=%d)", who, rows, s_name, a.S, ld_name, a.ldkv);
    return MMGL_OK;
}

// what the two rotary append entry points refuse alike about the `rows` rows of qkv and the cache they file into, after their own test
// of the sizes.  kv_name and cs_name are the entry point's words for its cache pointer and its angles in the messages.
int check_rope_append(const char* who, const char* kv_name, const char* cs_name, const void* qkv, int ldqkv, const void* cs, const void* kv,
                      size_t bs_kv, int B, int rows, int H, int Hkv, int D, int dtype) {
    MMGL_CHECK_ARG(H % Hkv == 0, "%s: %d query heads are no multiple of %d key/value heads", who, H, Hkv);
    MMGL_CHECK_ARG(dtype == MMGL_BF16 || dtype == MMGL_F32, "%s: bad dtype %d", who, dtype);
    if (D != 16 && D != 32 && D != 64 && D != 128) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: head_dim %d (16, 32, 64, 128)", who, D);
    const int vec = dtype == MMGL_BF16 ? 8 : 4;
    if (ldqkv % vec || bs_kv % vec) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: strides (%d, %zu) must be multiples of 16 bytes", who, ldqkv, bs_kv);
    MMGL_CHECK_ARG(qkv && cs && kv, "%s: null pointer", who);
    MMGL_CHECK_ARG((long long)ldqkv >= (long long)(H + 2 * Hkv) * D && (B == 1 || bs_kv >= (size_t)2 * Hkv * D),
                   "%s: strides (%d, %zu) smaller than the rows", who, ldqkv, bs_kv);
    if (!aligned16(qkv) || !aligned16(kv) || ((uintptr_t)cs & 7))
        MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: qkv and %s must be 16-byte aligned, %s 8-byte", who, kv_name, cs_name);
    MMGL_CHECK_ARG((long long)rows * (H + 2 * Hkv) * (D / 2 / vec) < (1ll << 31), "%s: %d rows of %d heads are too many", who, rows, H + 2 * Hkv);
    return MMGL_OK;
}

}  // namespace

extern "C" int mmgl_gemm_skinny(const void* x, int ldx, const void* W, int ldw, const void* bias, const void* residual, void* y, int ldy,
                                int M, int N, int K, int act, float scale, int dtype, void* stream) {
    MMGL_CHECK_ARG(M >= 1 && N >= 1 && K >= 1, "mmgl_gemm_skinny: bad sizes M=%d N=%d K=%d", M, N, K);
    const int bad = check_skinny(__func__, "chunk the rows or use mmgl_gemm_nt", x && W && y, M, act, dtype);
    if (bad) return bad;
    MMGL_CHECK_ARG(ldx >= K && ldw >= K && ldy >= N, "mmgl_gemm_skinny: leading dimensions (%d, %d, %d) smaller than the rows (K=%d, N=%d)",
                   ldx, ldw, ldy, K, N);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MMGL_F32) {
        SkArgs<float> a{(const float*)x, (const float*)W, (const float*)bias, (const float*)residual, (float*)y, ldx, ldw, ldy, M, N, K, act, scale};
        return launch_skinny_generic<float>(a, st);
    }
    SkArgs<bf16> a{(const bf16*)x, (const bf16*)W, (const bf16*)bias, (const bf16*)residual, (bf16*)y, ldx, ldw, ldy, M, N, K, act, scale};
    return skinny_bf16(a, st);
}

extern "C" int mmgl_gemm_skinny_lora(const void* x, int ldx, const void* W, int ldw, const void* bias, const void* residual, void* y, int ldy,
                                     const void* lora_A, int lda, const void* lora_B, int ldb, int r, float lora_scale, void* workspace,
                                     int M, int N, int K, int act, float scale, int dtype, void* stream) {
    MMGL_CHECK_ARG(M >= 1 && N >= 1 && K >= 1 && r >= 1, "mmgl_gemm_skinny_lora: bad sizes M=%d N=%d K=%d r=%d", M, N, K, r);
    if (r > 256) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_gemm_skinny_lora: rank %d > 256", r);
    const int bad = check_skinny(__func__, "chunk the rows", x && W && y && lora_A && lora_B && workspace, M, act, dtype);
    if (bad) return bad;
    MMGL_CHECK_ARG(ldx >= K && ldw >= K && ldy >= N && lda >= K && ldb >= r,
                   "mmgl_gemm_skinny_lora: leading dimensions (%d, %d, %d, %d, %d) smaller than the rows (K=%d, N=%d, r=%d)", ldx, ldw, ldy, lda,
                   ldb, K, N, r);
    MMGL_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "mmgl_gemm_skinny_lora: the fp32 workspace is not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float* t = (float*)workspace;
    if (dtype == MMGL_F32) {
        const int rc = launch_lora_t<float>((const float*)x, ldx, (const float*)lora_A, lda, t, M, r, K, st);
        if (rc != MMGL_OK) return rc;
        SkArgs<float> a{(const float*)x, (const float*)W, (const float*)bias, (const float*)residual, (float*)y, ldx, ldw, ldy, M, N, K, act, scale};
        const int vec = r % 8 == 0 && ldb % 8 == 0 && ((uintptr_t)lora_B & 31) == 0 && aligned16(t);
        return launch_skinny_generic<float>(a, st, SkLora<float>{(const float*)lora_B, t, ldb, r, vec, lora_scale});
    }
    const int rc = launch_lora_t<bf16>((const bf16*)x, ldx, (const bf16*)lora_A, lda, t, M, r, K, st);
    if (rc != MMGL_OK) return rc;
    SkArgs<bf16> a{(const bf16*)x, (const bf16*)W, (const bf16*)bias, (const bf16*)residual, (bf16*)y, ldx, ldw, ldy, M, N, K, act, scale};
    const int vec = r % 8 == 0 && ldb % 8 == 0 && aligned16(lora_B) && aligned16(t);
    return skinny_bf16(a, st, SkLora<bf16>{(const bf16*)lora_B, t, ldb, r, vec, lora_scale});
}

extern "C" int mmgl_attn_decode_fwd(const void* q, int ldq, const void* k, const void* v, int ldkv, size_t batch_stride_kv,
                                    const uint8_t* key_valid, int ld_valid, void* out, int B, int H, int S, int D, int dtype, void* stream) {
    MMGL_CHECK_ARG(B >= 1 && H >= 1 && S >= 1, "mmgl_attn_decode_fwd: bad sizes B=%d H=%d S=%d", B, H, S);
    const AttnPrefix a{q, k, v, key_valid, out, ldq, ldkv, ld_valid, B, H, H, S, D, dtype, batch_stride_kv};
    const int bad = check_attn_prefix(a, __func__);
    if (bad) return bad;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MMGL_BF16) RETURN_BY_HEAD_DIM(launch_attn_decode, bf16, D, a, st);
    RETURN_BY_HEAD_DIM(launch_attn_decode, float, D, a, st);
}

extern "C" int mmgl_attn_decode_relbias_fwd(const void* q, int ldq, const void* k, const void* v, int ldkv, size_t batch_stride_kv,
                                            const float* bias, int ld_bias, void* out, int B, int H, int S, int D, int dtype, void* stream) {
    MMGL_CHECK_ARG(B >= 1 && H >= 1 && S >= 1, "mmgl_attn_decode_relbias_fwd: bad sizes B=%d H=%d S=%d", B, H, S);
    // the bias rows stand where the other entry points have their mask: one word per key, non-null, a pitch of at least S
    const AttnPrefix a{q, k, v, (const uint8_t*)bias, out, ldq, ldkv, ld_bias, B, H, H, S, D, dtype, batch_stride_kv};
    const int bad = check_attn_prefix(a, __func__);
    if (bad) return bad;
    if ((uintptr_t)bias & 3) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_attn_decode_relbias_fwd: bias must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MMGL_BF16) RETURN_BY_HEAD_DIM(launch_attn_decode_relbias, bf16, D, a, bias, ld_bias, st);
    RETURN_BY_HEAD_DIM(launch_attn_decode_relbias, float, D, a, bias, ld_bias, st);
}

extern "C" int mmgl_attn_decode_gqa_fwd(const void* q, int ldq, const void* k, const void* v, int ldkv, size_t batch_stride_kv,
                                        const uint8_t* key_valid, int ld_valid, void* out, int B, int H, int Hkv, int S, int D, int dtype,
                                        void* stream) {
    MMGL_CHECK_ARG(B >= 1 && H >= 1 && Hkv >= 1 && S >= 1, "mmgl_attn_decode_gqa_fwd: bad sizes B=%d H=%d Hkv=%d S=%d", B, H, Hkv, S);
    MMGL_CHECK_ARG(H % Hkv == 0, "mmgl_attn_decode_gqa_fwd: %d query heads are no multiple of %d key/value heads", H, Hkv);
    const AttnPrefix a{q, k, v, key_valid, out, ldq, ldkv, ld_valid, B, H, Hkv, S, D, dtype, batch_stride_kv};
    const int bad = check_attn_prefix(a, __func__);
    if (bad) return bad;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MMGL_BF16) RETURN_BY_HEAD_DIM(attn_decode_gqa_nq, bf16, D, a, st);
    RETURN_BY_HEAD_DIM(attn_decode_gqa_nq, float, D, a, st);
}

extern "C" int mmgl_attn_decode_beam_fwd(const void* q, int ldq, const void* k_pre, const void* v_pre, int ld_pre, size_t batch_stride_pre,
                                         const uint8_t* key_valid, int ld_valid, const void* k_tail, const void* v_tail, int ld_tail,
                                         size_t row_stride_tail, const int* src, int ld_src, void* out, int B, int W, int H, int S_pre,
                                         int n_tail, int D, int dtype, void* stream) {
    MMGL_CHECK_ARG(B >= 1 && W >= 1 && H >= 1 && S_pre >= 1 && n_tail >= 0, "mmgl_attn_decode_beam_fwd: bad sizes B=%d W=%d H=%d S_pre=%d n_tail=%d",
                   B, W, H, S_pre, n_tail);
    if (W > 8) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_attn_decode_beam_fwd: %d beams per sample (1..8)", W);
    const BeamAttnArgs a{{q, k_pre, v_pre, key_valid, out, ldq, ld_pre, ld_valid, B, H, H, S_pre, D, dtype, batch_stride_pre},
                         k_tail, v_tail, src, ld_tail, ld_src, W, n_tail, row_stride_tail};
    const int bad = check_attn_prefix(a.p, __func__, "k_pre and v_pre", "prefix", "S_pre", "ld_pre");
    if (bad) return bad;
    if (n_tail > 0) {
        const int vec = dtype == MMGL_BF16 ? 8 : 4, esz = dtype == MMGL_BF16 ? 2 : 4;
        MMGL_CHECK_ARG(k_tail && v_tail && src, "mmgl_attn_decode_beam_fwd: null tail pointer with n_tail=%d", n_tail);
        if (ld_tail % vec || row_stride_tail % vec || !aligned16(k_tail) || !aligned16(v_tail) || ((uintptr_t)src & 3))
            MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_attn_decode_beam_fwd: tail strides (%d, %zu) must be multiples of 16 bytes, k_tail and v_tail 16-byte "
                                            "aligned, src 4-byte", ld_tail, row_stride_tail);
        MMGL_CHECK_ARG(ld_tail >= H * D && ld_src >= n_tail && (B * W == 1 || row_stride_tail >= (size_t)(n_tail - 1) * ld_tail + (size_t)H * D),
                       "mmgl_attn_decode_beam_fwd: tail strides (%d, %zu, %d) smaller than the rows", ld_tail, row_stride_tail, ld_src);
        if (((size_t)(W - 1) * row_stride_tail + (size_t)(n_tail - 1) * ld_tail + D) * esz >= (1ull << 31))
            MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_attn_decode_beam_fwd: a sample's tail rows span 2 GiB or more (W=%d, row stride %zu)", W, row_stride_tail);
        // a table the host can read is checked here; a device table is the caller's contract (the kernel clamps, it never asserts)
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, src) != hipSuccess) (void)hipGetLastError();
        else if (attr.type == hipMemoryTypeHost && attr.hostPointer) {
            const int* hs = (const int*)attr.hostPointer;
            for (int r = 0; r < B * W; ++r)
                for (int t = 0; t < n_tail; ++t) {
                    const int sv = hs[(size_t)r * ld_src + t];
                    MMGL_CHECK_ARG(sv >= 0 && sv < W, "mmgl_attn_decode_beam_fwd: src[%d][%d] = %d outside [0, %d)", r, t, sv, W);
                }
        }
    }
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MMGL_BF16) RETURN_BY_HEAD_DIM(attn_decode_beam_nq, bf16, D, a, st);
    RETURN_BY_HEAD_DIM(attn_decode_beam_nq, float, D, a, st);
}

extern "C" int mmgl_attn_decode_block_fwd(const void* q, int ldq, const void* k_new, const void* v_new, int ld_new, void* k, void* v, int ldkv,
                                          size_t batch_stride_kv, int capacity, const uint8_t* key_valid, int ld_valid, const int* len,
                                          void* out, int B, int m, int H, int D, int dtype, void* stream) {
    MMGL_CHECK_ARG(B >= 1 && m >= 1 && H >= 1 && capacity >= 1, "mmgl_attn_decode_block_fwd: bad sizes B=%d m=%d H=%d capacity=%d", B, m, H, capacity);
    if (m > 8) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_attn_decode_block_fwd: %d new tokens per sample (1..8)", m);
    const BlockAttnArgs a{{q, k, v, key_valid, out, ldq, ldkv, ld_valid, B, H, H, capacity, D, dtype, batch_stride_kv}, k_new, v_new, len, ld_new, m};
    const int bad = check_attn_prefix(a.p, __func__, "k and v", "cache", "capacity");
    if (bad) return bad;
    MMGL_CHECK_ARG(k_new && v_new && len, "mmgl_attn_decode_block_fwd: null pointer");
    if (ld_new % (dtype == MMGL_BF16 ? 8 : 4) || !aligned16(k_new) || !aligned16(v_new) || ((uintptr_t)len & 3))
        MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_attn_decode_block_fwd: ld_new %d must be a multiple of 16 bytes, k_new and v_new 16-byte aligned, len 4-byte",
                  ld_new);
    MMGL_CHECK_ARG(ld_new >= H * D && (B == 1 || batch_stride_kv >= (size_t)(capacity - 1) * ldkv + (size_t)H * D),
                   "mmgl_attn_decode_block_fwd: strides (%d, %zu) smaller than the rows", ld_new, batch_stride_kv);
    if (((size_t)(m - 1) * ld_new + D) * (dtype == MMGL_BF16 ? 2 : 4) >= (1ull << 31))
        MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_attn_decode_block_fwd: a sample's new rows span 2 GiB or more (m=%d, ld_new=%d)", m, ld_new);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MMGL_BF16) RETURN_BY_HEAD_DIM(attn_decode_block_nq, bf16, D, a, st);
    RETURN_BY_HEAD_DIM(attn_decode_block_nq, float, D, a, st);
}

extern "C" int mmgl_attn_decode_gqa_block_fwd(const void* q, int ldq, const void* k, const void* v, int ldkv, size_t batch_stride_kv, int capacity,
                                              const uint8_t* key_valid, int ld_valid, const int* len, void* out, int B, int m, int H, int Hkv,
                                              int D, int dtype, void* stream) {
    MMGL_CHECK_ARG(B >= 1 && m >= 1 && H >= 1 && Hkv >= 1 && capacity >= 1, "mmgl_attn_decode_gqa_block_fwd: bad sizes B=%d m=%d H=%d Hkv=%d capacity=%d",
                   B, m, H, Hkv, capacity);
    if (m > 8) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_attn_decode_gqa_block_fwd: %d new tokens per sample (1..8)", m);
    MMGL_CHECK_ARG(H % Hkv == 0, "mmgl_attn_decode_gqa_block_fwd: %d query heads are no multiple of %d key/value heads", H, Hkv);
    const GqaBlockAttnArgs a{{q, k, v, key_valid, out, ldq, ldkv, ld_valid, B, H, Hkv, capacity, D, dtype, batch_stride_kv}, len, m};
    const int bad = check_attn_prefix(a.p, __func__, "k and v", "cache", "capacity");
    if (bad) return bad;
    MMGL_CHECK_ARG(len, "mmgl_attn_decode_gqa_block_fwd: null pointer");
    if ((uintptr_t)len & 3) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_attn_decode_gqa_block_fwd: len must be 4-byte aligned");
    MMGL_CHECK_ARG(B == 1 || batch_stride_kv >= (size_t)(capacity - 1) * ldkv + (size_t)Hkv * D,
                   "mmgl_attn_decode_gqa_block_fwd: batch stride %zu smaller than the rows", batch_stride_kv);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MMGL_BF16) RETURN_BY_HEAD_DIM(attn_decode_gqa_block_nq, bf16, D, a, st);
    RETURN_BY_HEAD_DIM(attn_decode_gqa_block_nq, float, D, a, st);
}

extern "C" int mmgl_rope_kv_append_block(void* qkv, int ldqkv, const float* cos_sin, int n_pos, void* kv, int ldkv, size_t batch_stride_kv,
                                         int capacity, const int* len, int B, int m, int H, int Hkv, int D, int dtype, void* stream) {
    MMGL_CHECK_ARG(B >= 1 && m >= 1 && H >= 1 && Hkv >= 1 && capacity >= 1 && n_pos >= 1,
                   "mmgl_rope_kv_append_block: bad sizes B=%d m=%d H=%d Hkv=%d capacity=%d n_pos=%d", B, m, H, Hkv, capacity, n_pos);
    if (m > 8) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_rope_kv_append_block: %d new tokens per sample (1..8)", m);
    const int bad = check_rope_append(__func__, "kv", "cos_sin", qkv, ldqkv, cos_sin, kv, batch_stride_kv, B, B * m, H, Hkv, D, dtype);
    if (bad) return bad;
    MMGL_CHECK_ARG(len, "mmgl_rope_kv_append_block: null pointer");
    const int vec = dtype == MMGL_BF16 ? 8 : 4;
    if (ldkv % vec || ((uintptr_t)len & 3))
        MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_rope_kv_append_block: ldkv %d must be a multiple of 16 bytes, len 4-byte aligned", ldkv);
    MMGL_CHECK_ARG(ldkv >= 2 * Hkv * D && (B == 1 || batch_stride_kv >= (size_t)(capacity - 1) * ldkv + (size_t)2 * Hkv * D),
                   "mmgl_rope_kv_append_block: strides (%d, %zu) smaller than the rows", ldkv, batch_stride_kv);
    hipStream_t st = (hipStream_t)stream;
    const int rows = B * m, total = rows * (H + 2 * Hkv) * (D / 2 / vec);
    const dim3 grid(min(cdiv(total, 256), 4096)), block(256);
    if (dtype == MMGL_BF16)
        hipLaunchKernelGGL(rope_kv_append_block_kernel<bf16>, grid, block, 0, st, (bf16*)qkv, ldqkv, (const f32x2*)cos_sin, n_pos, (bf16*)kv, ldkv,
                           batch_stride_kv, capacity, len, rows, m, H, Hkv, D);
    else
        hipLaunchKernelGGL(rope_kv_append_block_kernel<float>, grid, block, 0, st, (float*)qkv, ldqkv, (const f32x2*)cos_sin, n_pos, (float*)kv, ldkv,
                           batch_stride_kv, capacity, len, rows, m, H, Hkv, D);
    MMGL_CHECK_LAUNCH("mmgl_rope_kv_append_block");
    return MMGL_OK;
}

extern "C" int mmgl_rope_kv_append(void* qkv, int ldqkv, const float* cos_sin_row, void* kv_col, size_t batch_stride_kv, int B, int H, int Hkv,
                                   int D, int dtype, void* stream) {
    MMGL_CHECK_ARG(B >= 1 && H >= 1 && Hkv >= 1, "mmgl_rope_kv_append: bad sizes B=%d H=%d Hkv=%d", B, H, Hkv);
    const int bad = check_rope_append(__func__, "kv_col", "cos_sin_row", qkv, ldqkv, cos_sin_row, kv_col, batch_stride_kv, B, B, H, Hkv, D, dtype);
    if (bad) return bad;
    hipStream_t st = (hipStream_t)stream;
    const int total = B * (H + 2 * Hkv) * (D / 2 / (dtype == MMGL_BF16 ? 8 : 4));
    const dim3 grid(min(cdiv(total, 256), 4096)), block(256);
    if (dtype == MMGL_BF16)
        hipLaunchKernelGGL(rope_kv_append_kernel<bf16>, grid, block, 0, st, (bf16*)qkv, ldqkv, (const f32x2*)cos_sin_row, (bf16*)kv_col, batch_stride_kv, B, H, Hkv, D);
    else
        hipLaunchKernelGGL(rope_kv_append_kernel<float>, grid, block, 0, st, (float*)qkv, ldqkv, (const f32x2*)cos_sin_row, (float*)kv_col, batch_stride_kv, B, H, Hkv, D);
    MMGL_CHECK_LAUNCH("mmgl_rope_kv_append");
    return MMGL_OK;
}

extern "C" int mmgl_kv_quantize(const void* k, const void* v, int ld_src, size_t batch_stride_src, void* codes, int ld_code,
                                size_t batch_stride_code, void* scale, int ld_scale, size_t batch_stride_scale, int B, int n, int H, int D,
                                int dtype, void* stream) {
    MMGL_CHECK_ARG(B >= 1 && n >= 1 && H >= 1, "mmgl_kv_quantize: bad sizes B=%d n=%d H=%d", B, n, H);
    MMGL_CHECK_ARG(dtype == MMGL_BF16 || dtype == MMGL_F32, "mmgl_kv_quantize: bad dtype %d", dtype);
    if (D != 16 && D != 32 && D != 64 && D != 128) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_kv_quantize: head_dim %d (16, 32, 64, 128)", D);
    const int vec = dtype == MMGL_BF16 ? 8 : 4;
    if (ld_src % vec || batch_stride_src % vec || ld_code % 16 || batch_stride_code % 16)
        MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_kv_quantize: strides (%d, %zu, %d, %zu) must be multiples of 16 bytes", ld_src, batch_stride_src,
                  ld_code, batch_stride_code);
    MMGL_CHECK_ARG(k && v && codes && scale, "mmgl_kv_quantize: null pointer");
    const long long hd = (long long)H * D;
    MMGL_CHECK_ARG(ld_src >= hd && ld_code >= 2 * hd && ld_scale >= 2 * H &&
                       (B == 1 || (batch_stride_src >= (size_t)(n - 1) * ld_src + (size_t)hd &&
                                   batch_stride_code >= (size_t)(n - 1) * ld_code + (size_t)(2 * hd) &&
                                   batch_stride_scale >= (size_t)(n - 1) * ld_scale + (size_t)(2 * H))),
                   "mmgl_kv_quantize: strides (%d, %zu, %d, %zu, %d, %zu) smaller than the rows", ld_src, batch_stride_src, ld_code,
                   batch_stride_code, ld_scale, batch_stride_scale);
    if (!aligned16(k) || !aligned16(v) || !aligned16(codes)) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_kv_quantize: k, v and codes must be 16-byte aligned");
    if ((long long)B * n * 2 * H * (D / 16) >= (1ll << 31)) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_kv_quantize: %d rows of %d heads are too many", B * n, 2 * H);
    const KvQuantArgs a{k, v, (uint8_t*)codes, (int8_t*)scale, ld_src, ld_code, ld_scale, B, n, H, batch_stride_src, batch_stride_code, batch_stride_scale};
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MMGL_BF16) RETURN_BY_HEAD_DIM(launch_kv_quantize, bf16, D, a, st);
    RETURN_BY_HEAD_DIM(launch_kv_quantize, float, D, a, st);
}

extern "C" int mmgl_attn_decode_q8_fwd(const void* q, int ldq, const void* k_new, const void* v_new, int ld_new, void* k_codes, void* v_codes,
                                       int ld_code, size_t batch_stride_code, void* k_scale, void* v_scale, int ld_scale,
                                       size_t batch_stride_scale, int capacity, const uint8_t* key_valid, int ld_valid, void* out, int B, int H,
                                       int S, int D, int dtype, void* stream) {
    MMGL_CHECK_ARG(B >= 1 && H >= 1 && S >= 1 && capacity > S, "mmgl_attn_decode_q8_fwd: bad sizes B=%d H=%d S=%d capacity=%d", B, H, S, capacity);
    const Q8AttnArgs a{q, k_new, v_new, (uint8_t*)k_codes, (uint8_t*)v_codes, (int8_t*)k_scale, (int8_t*)v_scale, key_valid, out,
                       ldq, ld_new, ld_code, ld_scale, ld_valid, B, H, S, batch_stride_code, batch_stride_scale};
    const int bad = check_attn_q8(__func__, a, H, capacity, D, dtype);
    if (bad) return bad;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MMGL_BF16) RETURN_BY_HEAD_DIM(launch_attn_decode_q8, bf16, D, a, st);
    RETURN_BY_HEAD_DIM(launch_attn_decode_q8, float, D, a, st);
}

extern "C" int mmgl_attn_decode_gqa_q8_fwd(const void* q, int ldq, const void* k_new, const void* v_new, int ld_new, void* k_codes, void* v_codes,
                                           int ld_code, size_t batch_stride_code, void* k_scale, void* v_scale, int ld_scale,
                                           size_t batch_stride_scale, int capacity, const uint8_t* key_valid, int ld_valid, void* out, int B,
                                           int H, int Hkv, int S, int D, int dtype, void* stream) {
    MMGL_CHECK_ARG(B >= 1 && H >= 1 && Hkv >= 1 && S >= 1 && capacity > S, "mmgl_attn_decode_gqa_q8_fwd: bad sizes B=%d H=%d Hkv=%d S=%d capacity=%d",
                   B, H, Hkv, S, capacity);
    MMGL_CHECK_ARG(H % Hkv == 0, "mmgl_attn_decode_gqa_q8_fwd: %d query heads are no multiple of %d key/value heads", H, Hkv);
    const Q8AttnArgs a{q, k_new, v_new, (uint8_t*)k_codes, (uint8_t*)v_codes, (int8_t*)k_scale, (int8_t*)v_scale, key_valid, out,
                       ldq, ld_new, ld_code, ld_scale, ld_valid, B, H, S, batch_stride_code, batch_stride_scale};
    const int bad = check_attn_q8(__func__, a, Hkv, capacity, D, dtype);
    if (bad) return bad;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MMGL_BF16) RETURN_BY_HEAD_DIM(attn_decode_gqa_q8_nq, bf16, D, a, Hkv, st);
    RETURN_BY_HEAD_DIM(attn_decode_gqa_q8_nq, float, D, a, Hkv, st);
}

extern "C" int mmgl_weight_quantize(const void* w, int ldw, void* codes, int ld_codes, void* exps, int N, int K, int dtype, void* stream) {
    MMGL_CHECK_ARG(N >= 1 && K >= 1, "mmgl_weight_quantize: bad sizes N=%d K=%d", N, K);
    MMGL_CHECK_ARG(dtype == MMGL_BF16 || dtype == MMGL_F32, "mmgl_weight_quantize: bad dtype %d", dtype);
    MMGL_CHECK_ARG(w && codes && exps, "mmgl_weight_quantize: null pointer");
    MMGL_CHECK_ARG(ldw >= K && ld_codes >= K, "mmgl_weight_quantize: leading dimensions (%d, %d) smaller than the rows (K=%d)", ldw, ld_codes, K);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MMGL_BF16) return launch_weight_quantize<bf16>(w, ldw, codes, ld_codes, exps, N, K, st);
    return launch_weight_quantize<float>(w, ldw, codes, ld_codes, exps, N, K, st);
}

extern "C" int mmgl_gemm_skinny_w8(const void* x, int ldx, const void* codes, int ld_codes, const void* exps, const void* bias,
                                   const void* residual, void* y, int ldy, int M, int N, int K, int act, float scale, int dtype, void* stream) {
    MMGL_CHECK_ARG(M >= 1 && N >= 1 && K >= 1, "mmgl_gemm_skinny_w8: bad sizes M=%d N=%d K=%d", M, N, K);
    const int bad = check_skinny(__func__, "chunk the rows", x && codes && exps && y, M, act, dtype);
    if (bad) return bad;
    MMGL_CHECK_ARG(ldx >= K && ld_codes >= K && ldy >= N, "mmgl_gemm_skinny_w8: leading dimensions (%d, %d, %d) smaller than the rows (K=%d, N=%d)",
                   ldx, ld_codes, ldy, K, N);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MMGL_F32) {
        const SkW8Args<float> q{{(const float*)x, nullptr, (const float*)bias, (const float*)residual, (float*)y, ldx, 0, ldy, M, N, K, act, scale},
                                (const uint8_t*)codes, (const int8_t*)exps, ld_codes};
        return launch_skinny_w8_generic<float>(q, st);
    }
    const SkW8Args<bf16> q{{(const bf16*)x, nullptr, (const bf16*)bias, (const bf16*)residual, (bf16*)y, ldx, 0, ldy, M, N, K, act, scale},
                           (const uint8_t*)codes, (const int8_t*)exps, ld_codes};
    return skinny_w8_bf16(q, st);
}
