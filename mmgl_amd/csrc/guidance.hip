// Neighbor guidance of generate(guidance_scale=g): the contrast of the next-token distribution with neighbors against the one without,
// in place, one launch.  Reached only from ops.guidance_logits, in front of the logits processors and the selection tails.
//
// mmgl_guidance_logits (guidance_kernel), one workgroup of 1024 threads per PAIR of rows of logits [2B, V]: row b holds the logits
// with neighbors (conditional), row B + b the logits of the same tokens without the gated layers (unconditional).  With
//   lc = xc - lse(xc),  lu = xu - lse(xu)        (log-probabilities, fp32; a NaN logit counts as -inf)
// row b becomes  lu + g (lc - lu), evaluated in fp32 and rounded once to the storage type; row B + b is only read.  Three passes
// over the two rows (200 KB of bf16 at V = 50272: re-read from L2), element loads at stride 1024, any row stride, any alignment, each
// loop unrolled by four so that eight loads are in flight per thread (the additions keep their order):
//   1. the two maxima;  2. the two sums of expf(x - max);  3. the guided scores.
// Both reductions have a fixed order: a thread's elements in ascending index order, the wave's butterfly, the 16 waves in order
// through LDS -- two runs are bitwise equal.  All reads of row b by passes 1 and 2 lie in front of the barrier of pass 2's LDS
// exchange; in pass 3 a thread reads an element of row b only to write that same element.
// -inf: a conditional -inf stays -inf (the token is banned with neighbors); an unconditional -inf under a finite conditional gives lc
// (there is nothing to subtract).  A row without any finite logit is outside the contract (lm_head cannot produce one): the call does
// not fault on it, what it stores there is unspecified.
// No atomics, no workspace, no [rows, V] intermediate, no host synchronisation.  Plain vector stores only.
#include "common.h"
#include <math.h>

namespace {

constexpr int GL_THREADS = 1024;
constexpr int GL_WAVES = GL_THREADS / 64;
constexpr int GL_MAX_V = 131072;

template <typename T> __device__ __forceinline__ float gl_load(const T* row, int v) {
    const float x = Elem<T>::to_f(row[v]);
    return x == x ? x : -INFINITY;
}

template <typename T>
__global__ __launch_bounds__(GL_THREADS) void guidance_kernel(T* logits, size_t ld, int B, int V, float g) {
    __shared__ float red[2][GL_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    T* rc = logits + (size_t)blockIdx.x * ld;
    const T* ru = logits + ((size_t)B + blockIdx.x) * ld;

    // ---- 1. the maxima
    float mc = -INFINITY, mu = -INFINITY;
#pragma unroll 4
    for (int v = tid; v < V; v += GL_THREADS) {
        mc = fmaxf(mc, gl_load(rc, v));
        mu = fmaxf(mu, gl_load(ru, v));
    }
    mc = wave_max(mc);
    mu = wave_max(mu);
    if (lane == 0) { red[0][w] = mc; red[1][w] = mu; }
    __syncthreads();
    mc = red[0][0];
    mu = red[1][0];
#pragma unroll
    for (int i = 1; i < GL_WAVES; ++i) { mc = fmaxf(mc, red[0][i]); mu = fmaxf(mu, red[1][i]); }
    __syncthreads();                                                        // red is rewritten below

    // ---- 2. the sums of expf(x - max): thread-sequential, the wave's butterfly, the waves in order
    float sc = 0.f, su = 0.f;
#pragma unroll 4
    for (int v = tid; v < V; v += GL_THREADS) {
        sc += expf(gl_load(rc, v) - mc);
        su += expf(gl_load(ru, v) - mu);
    }
    sc = wave_sum(sc);
    su = wave_sum(su);
    if (lane == 0) { red[0][w] = sc; red[1][w] = su; }
    __syncthreads();                                                        // every read of row b by passes 1 and 2 is done
    sc = red[0][0];
    su = red[1][0];
#pragma unroll
    for (int i = 1; i < GL_WAVES; ++i) { sc += red[0][i]; su += red[1][i]; }
    const float lse_c = mc + logf(sc), lse_u = mu + logf(su);

    // ---- 3. the guided scores
#pragma unroll 4
    for (int v = tid; v < V; v += GL_THREADS) {
        const float xc = gl_load(rc, v), xu = gl_load(ru, v);
        const float lc = xc - lse_c, lu = xu - lse_u;
        float s;
        if (xc == -INFINITY) s = -INFINITY;
        else if (xu == -INFINITY) s = lc;
        else s = lu + g * (lc - lu);
        rc[v] = Elem<T>::from_f(s);
    }
}

}  // namespace

extern "C" int mmgl_guidance_logits(void* logits, size_t ld_logits, int batch, int V, float guidance_scale, int dtype, void* stream) {
    MMGL_CHECK_ARG(batch >= 1 && V >= 1, "mmgl_guidance_logits: bad sizes batch=%d V=%d", batch, V);
    if (V > GL_MAX_V) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_guidance_logits: V=%d (at most %d)", V, GL_MAX_V);
    MMGL_CHECK_ARG(guidance_scale >= 0.f && isfinite(guidance_scale), "mmgl_guidance_logits: guidance_scale %g must be finite and not negative",
                   (double)guidance_scale);
    MMGL_CHECK_ARG(dtype == MMGL_BF16 || dtype == MMGL_F32, "mmgl_guidance_logits: bad dtype %d", dtype);
    MMGL_CHECK_ARG(logits, "mmgl_guidance_logits: null pointer");
    MMGL_CHECK_ARG(ld_logits >= (size_t)V, "mmgl_guidance_logits: row stride %zu smaller than V=%d", ld_logits, V);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(batch), block(GL_THREADS);
    if (dtype == MMGL_BF16)
        hipLaunchKernelGGL(guidance_kernel<bf16>, grid, block, 0, st, (bf16*)logits, ld_logits, batch, V, guidance_scale);
    else
        hipLaunchKernelGGL(guidance_kernel<float>, grid, block, 0, st, (float*)logits, ld_logits, batch, V, guidance_scale);
    MMGL_CHECK_LAUNCH("mmgl_guidance_logits");
    return MMGL_OK;
}
