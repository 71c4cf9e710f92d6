// Prompt-lookup decoding of generate(): the selection tail of a verify step, one launch.  Reached only from ops.lookup_accept.
//
// mmgl_lookup_accept (lookup_accept_kernel), one workgroup of 1024 threads per sample:
//   1. argmax of the sample's m_in logits rows in one pass over V, 16-byte loads where the rows allow them (every thread keeps m_in
//      running bests; a tie goes to the lower index, a NaN is never chosen; butterfly inside the wave, the 16 waves in order through LDS).
//   2. thread 0 applies the accept rule to the block the previous call wrote and publishes the k emitted tokens
//      in LDS; the id columns, the pads behind an EOS, emitted[b] and the row's gen / len / finished follow.
//   3. the row's history -- prompt columns under the mask, the tokens generated before this call (ids), the k new ones (LDS) -- is
//      compacted into an LDS image of int32 tokens by the ballot / wave-count scheme of logits_process_kernel.  A token outside
//      [0, V) is kept as -1: it equals nothing and ends a draft list.
//   4. draft rule: every thread walks its end positions e <= L - 2 and finds how many tokens (at most N) ending at e equal the last
//      ones of the history; per n the LATEST such e wins (max over the workgroup, fixed order).  The largest n with a match gives
//      the drafts h[e + 1 .. e + 1 + K), cut at the history's end.
//   5. thread 0 writes the next block [t_last, drafts, filler], its draft count and its position ids (clamped to pos_max).
// No atomics, no workspace, no [rows, V] intermediate; two runs are bitwise equal.  Plain vector stores only.
#include "common.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int LK_THREADS = 1024;
constexpr int LK_WAVES = LK_THREADS / 64;
constexpr int LK_MAX_HIST = 8192;            // tokens of a row's history (T + n_new) the LDS image holds: 32 KiB
constexpr int LK_MAX_M = 8;                  // logits rows per sample = K + 1
constexpr int LK_MAX_N = 4;                  // longest n-gram matched

template <typename T> struct LkVec;
template <> struct LkVec<bf16> { typedef bf16x8 type; };
template <> struct LkVec<float> { typedef f32x4 type; };

template <typename T>
__global__ __launch_bounds__(LK_THREADS) void lookup_accept_kernel(const T* __restrict__ logits, size_t ld, int vec, int m_in, long long* __restrict__ block,
                                                                   int* __restrict__ n_draft, long long* __restrict__ pos,
                                                                   long long* __restrict__ ids, size_t ld_ids,
                                                                   const unsigned char* __restrict__ mask, size_t ld_mask, int* __restrict__ gen,
                                                                   int* __restrict__ len, unsigned char* __restrict__ finished,
                                                                   int* __restrict__ emitted, int Tp, int n_new, int V, int K, int N,
                                                                   long long eos, long long pad, int pos_offset, int pos_max) {
    __shared__ int tok[LK_MAX_HIST];
    __shared__ int wcnt[LK_WAVES];
    __shared__ float red_v[LK_WAVES][LK_MAX_M];
    __shared__ int red_i[LK_WAVES][LK_MAX_M];
    __shared__ int red_e[LK_WAVES][LK_MAX_N];
    __shared__ int sh_e[LK_MAX_M];              // the tokens this call emits
    __shared__ int sh_state[5];                 // k, gen before, gen after, finished after, t_last
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t b = blockIdx.x;
    const int M1 = K + 1;

    // ---- 1. argmax of the m_in rows
    float bv[LK_MAX_M];
    int bi[LK_MAX_M];
#pragma unroll
    for (int i = 0; i < LK_MAX_M; ++i) { bv[i] = -INFINITY; bi[i] = INT_MAX; }
    // rows whose start and stride are multiples of 16 bytes are read as 16-byte vectors (8 bf16 / 4 fp32 per load), the columns behind
    // the last whole vector and any other layout element by element; either way (value, index) decides, so the result is the same
    constexpr int VEC = 16 / sizeof(T);
    const int v_vec = vec ? V / VEC * VEC : 0;
    for (int v0 = tid * VEC; v0 < v_vec; v0 += LK_THREADS * VEC) {
#pragma unroll
        for (int i = 0; i < LK_MAX_M; ++i)
            if (i < m_in) {
                const typename LkVec<T>::type xs = *(const typename LkVec<T>::type*)(logits + (b * m_in + i) * ld + v0);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float x = Elem<T>::to_f(xs[e]);
                    if (x > bv[i] || (x == bv[i] && v0 + e < bi[i])) { bv[i] = x; bi[i] = v0 + e; }
                }
            }
    }
    for (int v = v_vec + tid; v < V; v += LK_THREADS) {
#pragma unroll
        for (int i = 0; i < LK_MAX_M; ++i)
            if (i < m_in) {
                const float x = Elem<T>::to_f(logits[(b * m_in + i) * ld + v]);
                if (x > bv[i] || (x == bv[i] && v < bi[i])) { bv[i] = x; bi[i] = v; }
            }
    }
#pragma unroll
    for (int i = 0; i < LK_MAX_M; ++i) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float xv = __shfl_xor(bv[i], o);
            const int xi = __shfl_xor(bi[i], o);
            if (xv > bv[i] || (xv == bv[i] && xi < bi[i])) { bv[i] = xv; bi[i] = xi; }
        }
        if (lane == 0) { red_v[w][i] = bv[i]; red_i[w][i] = bi[i]; }
    }
    __syncthreads();

    // ---- 2. the accept rule
    if (tid == 0) {
        const int g = min(max(gen[b], 0), n_new);                  // the caller's state; clamped, never trusted as an address
        int fin = finished[b] != 0 || g >= n_new;
        const int nd = m_in > 1 ? min(max(n_draft[b], 0), m_in - 1) : 0;
        int k = 0, prev = -1;
        if (!fin) {
            for (int i = 0; i < m_in; ++i) {
                if (i > 0 && !(i <= nd && block[b * M1 + i] == (long long)prev)) break;
                float xv = red_v[0][i];
                int xi = red_i[0][i];
                for (int ww = 1; ww < LK_WAVES; ++ww)
                    if (red_v[ww][i] > xv || (red_v[ww][i] == xv && red_i[ww][i] < xi)) { xv = red_v[ww][i]; xi = red_i[ww][i]; }
                prev = xi < V ? xi : 0;                            // a row of NaN only: token 0
                sh_e[k] = prev;
                ids[b * ld_ids + Tp + g + k] = prev;
                ++k;
                if (eos >= 0 && (long long)prev == eos) { fin = 1; break; }
                if (g + k >= n_new) { fin = 1; break; }
            }
        }
        const bool hit_eos = k > 0 && eos >= 0 && (long long)prev == eos;
        sh_state[0] = k;
        sh_state[1] = g;
        sh_state[2] = hit_eos ? n_new : g + k;                     // the pads behind an EOS complete the row
        sh_state[3] = fin;
        sh_state[4] = min(max(k > 0 ? prev : (int)block[b * M1], 0), V - 1);      // a frozen row keeps feeding the token it fed before
        emitted[b] = k;
        gen[b] = sh_state[2];
        if (m_in > 1) len[b] += k;                                  // block inputs 0 .. k-1 are the row's new cache keys
        finished[b] = (unsigned char)fin;
    }
    __syncthreads();
    const int k = sh_state[0], g0 = sh_state[1], fin = sh_state[3], t_last = sh_state[4];
    const int G = g0 + k;                                           // tokens generated so far, this call's included
    if (sh_state[2] > G)                                            // EOS: pad the rest of the row at once
        for (int c = G + tid; c < n_new; c += LK_THREADS) ids[b * ld_ids + Tp + c] = pad;

    // ---- 3. the history, in order, as int32
    const int hist_len = Tp + G;
    int L = 0;
    for (int c0 = 0; c0 < hist_len; c0 += LK_THREADS) {
        const int c = c0 + tid;
        int t = -1;
        bool keep = false;
        if (c < hist_len) {
            keep = c >= Tp || mask[b * ld_mask + c] != 0;
            if (keep) {
                const long long hh = c < Tp + g0 ? ids[b * ld_ids + c] : (long long)sh_e[c - Tp - g0];
                t = (hh >= 0 && hh < (long long)V) ? (int)hh : -1;
            }
        }
        const unsigned long long mm = __ballot(keep);
        if (lane == 0) wcnt[w] = __popcll(mm);
        __syncthreads();
        int base = L, total = 0;
#pragma unroll
        for (int i = 0; i < LK_WAVES; ++i) {
            const int n = wcnt[i];
            base += i < w ? n : 0;
            total += n;
        }
        if (keep) tok[base + __popcll(mm & ((1ull << lane) - 1ull))] = t;      // base + rank < L + total <= c0 + 1024 <= 8192
        L += total;
        __syncthreads();
    }

    // ---- 4. the draft rule: per n the latest end position e <= L - 2 whose n last tokens equal the history's n last
    int be[LK_MAX_N];
#pragma unroll
    for (int n = 0; n < LK_MAX_N; ++n) be[n] = -1;
    if (!fin) {
        for (int e = tid; e <= L - 2; e += LK_THREADS) {
#pragma unroll
            for (int n = 0; n < LK_MAX_N; ++n) {
                if (n >= N || e - n < 0) break;
                const int a = tok[e - n];
                if (a < 0 || a != tok[L - 1 - n]) break;
                be[n] = e;                                          // e ascends per thread: the last one kept is its latest
            }
        }
    }
#pragma unroll
    for (int n = 0; n < LK_MAX_N; ++n) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) be[n] = max(be[n], __shfl_xor(be[n], o));
        if (lane == 0) red_e[w][n] = be[n];
    }
    __syncthreads();

    // ---- 5. the next block, its draft count and positions
    if (tid == 0) {
        int e = -1;
        for (int n = min(N, LK_MAX_N) - 1; n >= 0 && e < 0; --n)
            for (int ww = 0; ww < LK_WAVES; ++ww) e = max(e, red_e[ww][n]);
        int nd = 0;
        long long* blk = block + b * M1;
        blk[0] = t_last;
        if (e >= 0)
            for (; nd < K && e + 1 + nd < L && tok[e + 1 + nd] >= 0; ++nd) blk[1 + nd] = tok[e + 1 + nd];
        for (int i = 1 + nd; i < M1; ++i) blk[i] = t_last;          // filler: i > nd is never accepted
        n_draft[b] = nd;
        const int p0 = (L - G) + pos_offset + sh_state[2] - 1;      // the row's last token: valid prompt tokens + gen - 1 (frozen with gen)
        for (int i = 0; i < M1; ++i) pos[b * M1 + i] = min(max(p0 + i, 0), pos_max);
    }
}

}  // namespace

extern "C" int mmgl_lookup_accept(const void* logits, size_t ld_logits, int m_in, int64_t* block, int* n_draft, int64_t* positions, int64_t* ids,
                                  size_t ld_ids, const uint8_t* prompt_mask, size_t ld_mask, int* gen, int* len, uint8_t* finished, int* emitted,
                                  int B, int T, int n_new, int V, int K, int N, int64_t eos_token_id, int64_t pad_token_id, int pos_offset,
                                  int pos_max, int dtype, void* stream) {
    MMGL_CHECK_ARG(B >= 1 && T >= 0 && n_new >= 1 && V >= 1, "mmgl_lookup_accept: bad sizes B=%d T=%d n_new=%d V=%d", B, T, n_new, V);
    if (K < 1 || K > LK_MAX_M - 1) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_lookup_accept: K=%d drafted tokens (1..%d)", K, LK_MAX_M - 1);
    if (N < 1 || N > LK_MAX_N) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_lookup_accept: n-grams of N=%d tokens (1..%d)", N, LK_MAX_N);
    MMGL_CHECK_ARG(m_in == 1 || m_in == K + 1, "mmgl_lookup_accept: m_in=%d logits rows per sample (1 for the prefill, else K + 1 = %d)", m_in, K + 1);
    if ((long long)T + n_new > LK_MAX_HIST)
        MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_lookup_accept: a history of T + n_new = %lld tokens (at most %d)", (long long)T + n_new, LK_MAX_HIST);
    MMGL_CHECK_ARG(dtype == MMGL_BF16 || dtype == MMGL_F32, "mmgl_lookup_accept: bad dtype %d", dtype);
    MMGL_CHECK_ARG(logits && block && n_draft && positions && ids && (prompt_mask || T == 0) && gen && len && finished && emitted,
                   "mmgl_lookup_accept: null pointer");
    MMGL_CHECK_ARG(ld_logits >= (size_t)V && ld_ids >= (size_t)T + n_new && ld_mask >= (size_t)T,
                   "mmgl_lookup_accept: row strides (%zu, %zu, %zu) smaller than the rows", ld_logits, ld_ids, ld_mask);
    MMGL_CHECK_ARG(eos_token_id < 0 || (pad_token_id >= 0 && pad_token_id < V), "mmgl_lookup_accept: pad_token_id %lld outside [0, %d)",
                   (long long)pad_token_id, V);
    MMGL_CHECK_ARG(pos_max >= 0, "mmgl_lookup_accept: pos_max=%d", pos_max);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(B), threads(LK_THREADS);
    const size_t per16 = dtype == MMGL_BF16 ? 8 : 4;
    const int vec = ld_logits % per16 == 0 && ((uintptr_t)logits & 15) == 0;
    if (dtype == MMGL_BF16)
        hipLaunchKernelGGL(lookup_accept_kernel<bf16>, grid, threads, 0, st, (const bf16*)logits, ld_logits, vec, m_in, (long long*)block, n_draft,
                           (long long*)positions, (long long*)ids, ld_ids, prompt_mask, ld_mask, gen, len, finished, emitted, T, n_new, V, K, N,
                           (long long)eos_token_id, (long long)pad_token_id, pos_offset, pos_max);
    else
        hipLaunchKernelGGL(lookup_accept_kernel<float>, grid, threads, 0, st, (const float*)logits, ld_logits, vec, m_in, (long long*)block, n_draft,
                           (long long*)positions, (long long*)ids, ld_ids, prompt_mask, ld_mask, gen, len, finished, emitted, T, n_new, V, K, N,
                           (long long)eos_token_id, (long long)pad_token_id, pos_offset, pos_max);
    MMGL_CHECK_LAUNCH("mmgl_lookup_accept");
    return MMGL_OK;
}
