// Logits processors of generate(): repetition penalty, n-gram ban and token bans, in place, one launch.  Reached only from
// ops.process_logits, in front of the selection tails (argmax / mmgl_sample_tokens).
//
// mmgl_logits_process (logits_process_kernel), one workgroup of 1024 threads per logits row.  The row's history (int64, any row
// stride, columns [0, n_masked) under an optional validity mask) is compacted once into an LDS image of int32 tokens: per chunk of
// 1024 columns a ballot gives every valid column its rank inside the wave, the 16 wave counts give the wave's base.  A token outside
// [0, V) keeps its place in the image as -1: it is never an address and equals nothing, itself included.  Then, on the L tokens:
//   1. penalty: every thread READS the logits of its (at most 8) tokens, barrier, then writes x * p (x < 0) or x / p, computed in
//      fp32 and rounded once.  Every occurrence of a token read the untouched logit, so all of them store the same bits: a token is
//      penalised once whatever the thread order.
//   2. barrier; n-gram: thread i compares h[i .. i+n-1) with the last n-1 tokens and stores -inf at h[i+n-1]; the bans store -inf.
//      They come after the barrier, so -inf wins over a penalised value.
// At most L + n_ban elements of the row are written; no [rows, V] pass, no workspace, no atomics.  Plain vector stores only.
#include "common.h"
#include <math.h>

namespace {

constexpr int LP_THREADS = 1024;
constexpr int LP_WAVES = LP_THREADS / 64;
constexpr int LP_MAX_HIST = 8192;
constexpr int LP_PER_THREAD = LP_MAX_HIST / LP_THREADS;
constexpr int LP_MAX_BAN = 64;
constexpr int LP_MAX_V = 131072;

template <typename T>
__global__ __launch_bounds__(LP_THREADS) void logits_process_kernel(T* __restrict__ logits, size_t ld, const long long* __restrict__ history,
                                                                    size_t ld_hist, const unsigned char* __restrict__ valid, size_t ld_valid,
                                                                    int n_masked, int hist_len, const int* __restrict__ ban, int n_ban, int V,
                                                                    float penalty, int ngram) {
    __shared__ int tok[LP_MAX_HIST];
    __shared__ int wcnt[LP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t rowi = blockIdx.x;
    T* row = logits + rowi * ld;
    const T ninf = Elem<T>::from_f(-INFINITY);

    // ---- the valid tokens, in order, as int32
    int L = 0;
    for (int c0 = 0; c0 < hist_len; c0 += LP_THREADS) {
        const int c = c0 + tid;
        int t = -1;
        bool keep = false;
        if (c < hist_len) {
            keep = c >= n_masked || valid[rowi * ld_valid + c] != 0;
            if (keep) {
                const long long h = history[rowi * ld_hist + c];
                t = (h >= 0 && h < (long long)V) ? (int)h : -1;
            }
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wcnt[w] = __popcll(m);
        __syncthreads();
        int base = L, total = 0;
#pragma unroll
        for (int i = 0; i < LP_WAVES; ++i) {
            const int n = wcnt[i];
            base += i < w ? n : 0;
            total += n;
        }
        if (keep) tok[base + __popcll(m & ((1ull << lane) - 1ull))] = t;      // base + rank < L + total <= c0 + 1024 <= 8192
        L += total;
        __syncthreads();                                                    // wcnt is rewritten by the next chunk; tok is read below
    }

    // ---- 1. repetition penalty: read every candidate, barrier, write
    if (penalty != 1.f) {
        float x[LP_PER_THREAD];
#pragma unroll
        for (int k = 0; k < LP_PER_THREAD; ++k) {
            const int i = tid + k * LP_THREADS;
            const int t = i < L ? tok[i] : -1;
            x[k] = t >= 0 ? Elem<T>::to_f(row[t]) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < LP_PER_THREAD; ++k) {
            const int i = tid + k * LP_THREADS;
            const int t = i < L ? tok[i] : -1;
            if (t >= 0) row[t] = Elem<T>::from_f(x[k] < 0.f ? x[k] * penalty : x[k] / penalty);
        }
        __syncthreads();
    }

    // ---- 2. n-gram ban: the token that followed an earlier occurrence of the last n-1 tokens
    if (ngram > 0 && L >= ngram) {
        const int pre = L - ngram + 1;                                      // tok[pre .. L): the last n-1 tokens
        for (int i = tid; i <= L - ngram; i += LP_THREADS) {
            bool eq = true;
            for (int j = 0; j < ngram - 1 && eq; ++j) {
                const int a = tok[i + j];
                eq = a >= 0 && a == tok[pre + j];
            }
            const int t = tok[i + ngram - 1];
            if (eq && t >= 0) row[t] = ninf;
        }
    }

    // ---- 3. bans
    if (tid < n_ban) {
        const int t = ban[tid];
        if (t >= 0 && t < V) row[t] = ninf;
    }
}

}  // namespace

extern "C" int mmgl_logits_process(void* logits, size_t ld_logits, const int64_t* history, size_t ld_history, const uint8_t* hist_valid,
                                   size_t ld_valid, int n_masked, int hist_len, const int* ban, int n_ban, int rows, int V,
                                   float repetition_penalty, int no_repeat_ngram_size, int dtype, void* stream) {
    MMGL_CHECK_ARG(rows >= 1 && V >= 1, "mmgl_logits_process: bad sizes rows=%d V=%d", rows, V);
    MMGL_CHECK_ARG(hist_len >= 0 && n_masked >= 0 && n_masked <= hist_len, "mmgl_logits_process: hist_len=%d n_masked=%d (0 <= n_masked <= hist_len)",
                   hist_len, n_masked);
    MMGL_CHECK_ARG(n_ban >= 0 && no_repeat_ngram_size >= 0, "mmgl_logits_process: n_ban=%d / no_repeat_ngram_size=%d must not be negative", n_ban,
                   no_repeat_ngram_size);
    if (V > LP_MAX_V) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_logits_process: V=%d (at most %d)", V, LP_MAX_V);
    if (hist_len > LP_MAX_HIST) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_logits_process: hist_len=%d (at most %d)", hist_len, LP_MAX_HIST);
    if (n_ban > LP_MAX_BAN) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_logits_process: n_ban=%d (at most %d)", n_ban, LP_MAX_BAN);
    MMGL_CHECK_ARG(repetition_penalty > 0.f && isfinite(repetition_penalty), "mmgl_logits_process: repetition_penalty %g must be positive and finite",
                   (double)repetition_penalty);
    MMGL_CHECK_ARG(dtype == MMGL_BF16 || dtype == MMGL_F32, "mmgl_logits_process: bad dtype %d", dtype);
    MMGL_CHECK_ARG(logits && (history || hist_len == 0) && (hist_valid || n_masked == 0) && (ban || n_ban == 0), "mmgl_logits_process: null pointer");
    MMGL_CHECK_ARG(ld_logits >= (size_t)V, "mmgl_logits_process: row stride %zu smaller than V=%d", ld_logits, V);
    const bool history_used = hist_len > 0 && (repetition_penalty != 1.f || no_repeat_ngram_size > 0);
    if (!history_used && n_ban == 0) return MMGL_OK;                        // everything off: nothing to write
    if (!history_used) hist_len = n_masked = 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(rows), block(LP_THREADS);
    if (dtype == MMGL_BF16)
        hipLaunchKernelGGL(logits_process_kernel<bf16>, grid, block, 0, st, (bf16*)logits, ld_logits, (const long long*)history, ld_history, hist_valid,
                           ld_valid, n_masked, hist_len, ban, n_ban, V, repetition_penalty, no_repeat_ngram_size);
    else
        hipLaunchKernelGGL(logits_process_kernel<float>, grid, block, 0, st, (float*)logits, ld_logits, (const long long*)history, ld_history,
                           hist_valid, ld_valid, n_masked, hist_len, ban, n_ban, V, repetition_penalty, no_repeat_ngram_size);
    MMGL_CHECK_LAUNCH("mmgl_logits_process");
    return MMGL_OK;
}
