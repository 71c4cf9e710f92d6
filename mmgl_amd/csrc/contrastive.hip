// Contrastive search of generate(penalty_alpha > 0, top_k = k): the ranking of a sample's k candidate tokens against the hidden-state
// history of its context, and the bookkeeping of the step.  Reached only from ops.contrastive_select.  No atomics, fixed reduction
// orders: two runs are bitwise equal.  Plain vector stores only.
//
// mmgl_contrastive_select.  score(c) = (1 - alpha) p_c - alpha pen_c with p_c = exp(cand_score[c]) and pen_c = max over the live
// context rows j of cos(h_c, h_j), everything in fp32.  Two launches:
//   * contrastive_part_kernel, one workgroup per (sample, chunk of CS_CHUNK = 16 context rows): the memory-bound pass.  The sample's k
//     candidate rows are staged in LDS once per workgroup (k d elements against CS_CHUNK d of context); each of the 4 waves then owns 4
//     context rows, which it streams with 16-byte loads -- four loads in flight per lane -- while every 16-byte LDS read of a candidate
//     feeds the four rows.  dot(h_j, h_j) is accumulated beside the k dots, so no norm is stored anywhere.  A masked row and a row at
//     or past n_ctx is never loaded.  Lane sums run on DPP up to 16 lanes (group_sum, common.h).  One partial max per (sample, chunk,
//     candidate) goes to the workspace; the running max starts at -inf, which a chunk without a live row keeps.
//   * contrastive_pick_kernel, one workgroup per sample: folds the chunks in chunk order (-inf, an empty context, becomes 0), scores,
//     picks the lowest c among the maxima (NaN never wins), does the token / EOS bookkeeping of GreedyTail, writes column `step` of the
//     sample's k rows of the parent table, and copies the selected hidden row into context row n_ctx and into hidden_out.
#include "common.h"
#include <math.h>

namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_WAVES = CS_THREADS / WAVE;
constexpr int CS_ROWS = 4;                                  // context rows a wave streams at once
constexpr int CS_CHUNK = CS_WAVES * CS_ROWS;                // context rows per workgroup
constexpr int CS_MAX_K = 8;
constexpr size_t CS_MAX_LDS = 64 * 1024;                    // the k candidate rows of a sample

template <typename T> struct CsVec;
template <> struct CsVec<bf16> { typedef bf16x8 type; static constexpr int N = 8; };
template <> struct CsVec<float> { typedef f32x4 type; static constexpr int N = 4; };

template <typename T, int K>
__global__ __launch_bounds__(CS_THREADS) void contrastive_part_kernel(const T* __restrict__ cand, size_t ld_cand, const T* __restrict__ ctx,
                                                                      size_t ld_ctx, size_t bs_ctx, const uint8_t* __restrict__ valid,
                                                                      size_t ld_valid, int n_ctx, int d, int nchunk, float* __restrict__ ws) {
    typedef typename CsVec<T>::type V;
    constexpr int N = CsVec<T>::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char cs_smem[];
    V* sc = (V*)cs_smem;                                    // [K][d / N]
    __shared__ float cn[CS_MAX_K];                          // |h_c|^2
    __shared__ float wmax[CS_WAVES][CS_MAX_K];
    const int b = blockIdx.x / nchunk, ch = blockIdx.x - b * nchunk;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nv = d / N;

    for (int i = tid; i < K * nv; i += CS_THREADS) {
        const int c = i / nv, j = i - c * nv;
        sc[i] = *(const V*)(cand + ((size_t)b * K + c) * ld_cand + (size_t)j * N);
    }
    __syncthreads();
    for (int c = w; c < K; c += CS_WAVES) {
        float s = 0.f;
        for (int j = lane; j < nv; j += WAVE) {
            const V x = sc[c * nv + j];
#pragma unroll
            for (int e = 0; e < N; ++e) s = fmaf(Elem<T>::to_f(x[e]), Elem<T>::to_f(x[e]), s);
        }
        s = group_sum<WAVE>(s);
        if (lane == 0) cn[c] = s;
    }

    // this wave's rows: liveness is wave-uniform
    const int r0 = ch * CS_CHUNK + w * CS_ROWS;
    bool live[CS_ROWS];
    const T* rowp[CS_ROWS];
    bool any = false;
#pragma unroll
    for (int r = 0; r < CS_ROWS; ++r) {
        const int row = r0 + r;
        live[r] = row < n_ctx && valid[(size_t)b * ld_valid + (row < n_ctx ? row : 0)] != 0;
        rowp[r] = ctx + (size_t)b * bs_ctx + (size_t)(live[r] ? row : 0) * ld_ctx;
        any |= live[r];
    }
    float dot[K][CS_ROWS], nn[CS_ROWS];
#pragma unroll
    for (int r = 0; r < CS_ROWS; ++r) {
        nn[r] = 0.f;
#pragma unroll
        for (int c = 0; c < K; ++c) dot[c][r] = 0.f;
    }
    if (any) {
        for (int j = lane; j < nv; j += WAVE) {
            float xf[CS_ROWS][N];
#pragma unroll
            for (int r = 0; r < CS_ROWS; ++r) {
                V x = vzero<V>();
                if (live[r]) x = *(const V*)(rowp[r] + (size_t)j * N);
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    xf[r][e] = Elem<T>::to_f(x[e]);
                    nn[r] = fmaf(xf[r][e], xf[r][e], nn[r]);
                }
            }
#pragma unroll
            for (int c = 0; c < K; ++c) {
                const V cv = sc[c * nv + j];
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    const float cf = Elem<T>::to_f(cv[e]);
#pragma unroll
                    for (int r = 0; r < CS_ROWS; ++r) dot[c][r] = fmaf(cf, xf[r][e], dot[c][r]);
                }
            }
        }
    }
    __syncthreads();                                        // cn is complete
    float best[K];
#pragma unroll
    for (int c = 0; c < K; ++c) best[c] = -INFINITY;
    if (any) {
#pragma unroll
        for (int r = 0; r < CS_ROWS; ++r) {
            const float n2 = group_sum<WAVE>(nn[r]);
#pragma unroll
            for (int c = 0; c < K; ++c) {
                const float dt = group_sum<WAVE>(dot[c][r]);
                const float cs = (n2 == 0.f || cn[c] == 0.f) ? 0.f : dt / (sqrtf(n2) * sqrtf(cn[c]));
                if (live[r]) best[c] = fmaxf(best[c], cs);  // fmaxf drops a NaN cosine
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) wmax[w][c] = best[c];
    }
    __syncthreads();
    if (tid < K) {
        float m = wmax[0][tid];
#pragma unroll
        for (int k = 1; k < CS_WAVES; ++k) m = fmaxf(m, wmax[k][tid]);
        ws[((size_t)b * nchunk + ch) * K + tid] = m;
    }
}

struct PickArgs {
    const float* ws;
    const float* cand_score;
    const int* cand_index;
    size_t ld_pair;
    uint8_t* ctx_valid;
    size_t ld_valid;
    int* src;
    size_t ld_src;
    long long* ids;
    size_t ld_ids;
    uint8_t* finished;
    int* selected;
    float* trace_p;
    float* trace_pen;
    float* trace_score;
    long long eos, pad;
    float alpha;
    int K, nchunk, n_ctx, step, d;
};

template <typename T>
__global__ __launch_bounds__(CS_THREADS) void contrastive_pick_kernel(const PickArgs a, const T* __restrict__ cand, size_t ld_cand,
                                                                      T* __restrict__ ctx, size_t ld_ctx, size_t bs_ctx,
                                                                      T* __restrict__ hidden_out) {
    typedef typename CsVec<T>::type V;
    constexpr int N = CsVec<T>::N;
    __shared__ float sc[CS_MAX_K];
    __shared__ int sel_sh;
    const int b = blockIdx.x, tid = threadIdx.x, K = a.K;
    if (tid < K) {
        float pen = -INFINITY;
        for (int ch = 0; ch < a.nchunk; ++ch) pen = fmaxf(pen, a.ws[((size_t)b * a.nchunk + ch) * K + tid]);
        if (pen == -INFINITY) pen = 0.f;                    // no live context row
        const float p = expf(a.cand_score[(size_t)b * a.ld_pair + tid]);
        const float s = (1.f - a.alpha) * p - a.alpha * pen;
        sc[tid] = s;
        if (a.trace_p) {
            a.trace_p[(size_t)b * K + tid] = p;
            a.trace_pen[(size_t)b * K + tid] = pen;
            a.trace_score[(size_t)b * K + tid] = s;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int sel = -1;
        float bv = 0.f;
        for (int c = 0; c < K; ++c) {
            const float s = sc[c];
            if (s == s && (sel < 0 || s > bv)) { sel = c; bv = s; }
        }
        if (sel < 0) sel = 0;                               // every score NaN
        sel_sh = sel;
        a.selected[b] = sel;
        long long tok = a.cand_index[(size_t)b * a.ld_pair + sel];
        if (a.eos >= 0) {
            if (a.finished[b]) tok = a.pad;
            else if (tok == a.eos) a.finished[b] = 1;
        }
        a.ids[(size_t)b * a.ld_ids] = tok;
        a.ctx_valid[(size_t)b * a.ld_valid + a.n_ctx] = 1;
    }
    __syncthreads();
    const int sel = sel_sh;
    if (tid < K) a.src[((size_t)b * K + tid) * a.ld_src + a.step] = sel;
    const T* from = cand + ((size_t)b * K + sel) * ld_cand;
    T* to_ctx = ctx + (size_t)b * bs_ctx + (size_t)a.n_ctx * ld_ctx;
    T* to_out = hidden_out + (size_t)b * a.d;
    for (int j = tid; j < a.d / N; j += CS_THREADS) {
        const V x = *(const V*)(from + (size_t)j * N);
        *(V*)(to_ctx + (size_t)j * N) = x;
        *(V*)(to_out + (size_t)j * N) = x;
    }
}

template <typename T, int K> int launch_part(size_t lds, dim3 grid, hipStream_t st, const void* cand, size_t ld_cand, const void* ctx, size_t ld_ctx,
                                             size_t bs_ctx, const uint8_t* valid, size_t ld_valid, int n_ctx, int d, int nchunk, float* ws) {
    auto kern = contrastive_part_kernel<T, K>;
    const int rc = mmgl_set_lds(kern, lds, "mmgl_contrastive_select");
    if (rc) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(CS_THREADS), lds, st, (const T*)cand, ld_cand, (const T*)ctx, ld_ctx, bs_ctx, valid, ld_valid, n_ctx, d,
                       nchunk, ws);
    return MMGL_OK;
}

template <typename T, typename... A> int launch_part_k(int K, A... args) {
    switch (K) {
        case 2: return launch_part<T, 2>(args...);
        case 3: return launch_part<T, 3>(args...);
        case 4: return launch_part<T, 4>(args...);
        case 5: return launch_part<T, 5>(args...);
        case 6: return launch_part<T, 6>(args...);
        case 7: return launch_part<T, 7>(args...);
        default: return launch_part<T, 8>(args...);
    }
}

}  // namespace

extern "C" int mmgl_contrastive_chunk(void) { return CS_CHUNK; }

extern "C" size_t mmgl_contrastive_workspace(int B, int k, int n_cap) {
    if (B < 1 || k < 1 || n_cap < 1) return 0;
    return (size_t)B * cdiv(n_cap, CS_CHUNK) * k * sizeof(float);
}

extern "C" int mmgl_contrastive_select(const void* cand_hidden, size_t ld_cand, void* ctx, size_t ld_ctx, size_t batch_stride_ctx, uint8_t* ctx_valid,
                                       size_t ld_valid, int n_cap, const float* cand_score, const int* cand_index, size_t ld_pair, float alpha,
                                       int n_ctx, int step, int* src, size_t ld_src, int64_t* ids, size_t ld_ids, uint8_t* finished,
                                       int64_t eos_token_id, int64_t pad_token_id, void* hidden_out, int* selected, float* trace_p,
                                       float* trace_pen, float* trace_score, void* workspace, size_t workspace_bytes, int B, int k, int d, int V,
                                       int dtype, void* stream) {
    const char* who = "mmgl_contrastive_select";
    MMGL_CHECK_ARG(B >= 1 && d >= 1 && V >= 1 && n_cap >= 1, "%s: bad sizes B=%d d=%d V=%d n_cap=%d", who, B, d, V, n_cap);
    if (k < 2 || k > CS_MAX_K) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: k=%d candidates per sample (2..%d)", who, k, CS_MAX_K);
    MMGL_CHECK_ARG(V >= k, "%s: V=%d holds fewer than k=%d candidates", who, V, k);
    MMGL_CHECK_ARG(dtype == MMGL_BF16 || dtype == MMGL_F32, "%s: bad dtype %d", who, dtype);
    MMGL_CHECK_ARG(cand_hidden && ctx && ctx_valid && cand_score && cand_index && src && ids && hidden_out && selected && workspace &&
                       (finished || eos_token_id < 0),
                   "%s: null pointer", who);
    MMGL_CHECK_ARG((trace_p != nullptr) == (trace_pen != nullptr) && (trace_p != nullptr) == (trace_score != nullptr),
                   "%s: trace_p, trace_pen and trace_score come together", who);
    MMGL_CHECK_ARG(n_ctx >= 0 && n_ctx <= n_cap - 1, "%s: n_ctx=%d outside [0, n_cap - 1 = %d]", who, n_ctx, n_cap - 1);
    MMGL_CHECK_ARG(alpha >= 0.f && alpha <= 1.f, "%s: alpha=%g outside [0, 1]", who, (double)alpha);
    const size_t per16 = dtype == MMGL_BF16 ? 8 : 4;
    if ((size_t)d % per16) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: d=%d is no multiple of the 16-byte vector (%zu elements)", who, d, per16);
    MMGL_CHECK_ARG(ld_cand >= (size_t)d && ld_ctx >= (size_t)d && batch_stride_ctx >= (size_t)(n_cap - 1) * ld_ctx + d && ld_valid >= (size_t)n_cap &&
                       ld_pair >= (size_t)k && ld_src > (size_t)step && step >= 0 && ld_ids >= 1,
                   "%s: strides (%zu, %zu, %zu, %zu, %zu, %zu, %zu) smaller than the rows (step=%d)", who, ld_cand, ld_ctx, batch_stride_ctx, ld_valid,
                   ld_pair, ld_src, ld_ids, step);
    if (ld_cand % per16 || ld_ctx % per16 || batch_stride_ctx % per16)
        MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: strides (%zu, %zu, %zu) must be multiples of 16 bytes", who, ld_cand, ld_ctx, batch_stride_ctx);
    if (((uintptr_t)cand_hidden | (uintptr_t)ctx | (uintptr_t)hidden_out) & 15)
        MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: cand_hidden, ctx and hidden_out must be 16-byte aligned", who);
    MMGL_CHECK_ARG((((uintptr_t)cand_score | (uintptr_t)cand_index | (uintptr_t)src | (uintptr_t)selected | (uintptr_t)workspace | (uintptr_t)trace_p |
                     (uintptr_t)trace_pen | (uintptr_t)trace_score) & 3) == 0 && ((uintptr_t)ids & 7) == 0,
                   "%s: the fp32 / int32 operands must be 4-byte aligned, ids 8-byte", who);
    MMGL_CHECK_ARG(eos_token_id < 0 || (eos_token_id < V && pad_token_id >= 0 && pad_token_id < V),
                   "%s: eos_token_id %lld / pad_token_id %lld outside [0, %d)", who, (long long)eos_token_id, (long long)pad_token_id, V);
    const size_t esize = dtype == MMGL_BF16 ? 2 : 4, lds = (size_t)k * d * esize;
    if (lds > CS_MAX_LDS) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: k=%d candidate rows of d=%d take %zu B of LDS (at most %zu)", who, k, d, lds, CS_MAX_LDS);
    MMGL_CHECK_ARG((long long)B * cdiv(n_cap, CS_CHUNK) < (1ll << 31), "%s: too many chunks", who);
    MMGL_CHECK_ARG(workspace_bytes >= mmgl_contrastive_workspace(B, k, n_cap), "%s: the workspace holds %zu bytes, %zu needed", who, workspace_bytes,
                   mmgl_contrastive_workspace(B, k, n_cap));
    hipStream_t st = (hipStream_t)stream;
    const int nchunk = cdiv(n_ctx, CS_CHUNK);               // 0: an empty context, nothing to stream
    if (nchunk > 0) {
        const dim3 grid(B * nchunk);
        const int rc = dtype == MMGL_BF16
                           ? launch_part_k<bf16>(k, lds, grid, st, cand_hidden, ld_cand, (const void*)ctx, ld_ctx, batch_stride_ctx,
                                                 (const uint8_t*)ctx_valid, ld_valid, n_ctx, d, nchunk, (float*)workspace)
                           : launch_part_k<float>(k, lds, grid, st, cand_hidden, ld_cand, (const void*)ctx, ld_ctx, batch_stride_ctx,
                                                  (const uint8_t*)ctx_valid, ld_valid, n_ctx, d, nchunk, (float*)workspace);
        if (rc) return rc;
        MMGL_CHECK_LAUNCH("mmgl_contrastive_select (chunks)");
    }
    const PickArgs a{(const float*)workspace, cand_score, cand_index, ld_pair, ctx_valid, ld_valid, src, ld_src, (long long*)ids, ld_ids, finished,
                     selected, trace_p, trace_pen, trace_score, (long long)eos_token_id, (long long)pad_token_id, alpha, k, nchunk, n_ctx, step, d};
    if (dtype == MMGL_BF16)
        hipLaunchKernelGGL(contrastive_pick_kernel<bf16>, dim3(B), dim3(CS_THREADS), 0, st, a, (const bf16*)cand_hidden, ld_cand, (bf16*)ctx, ld_ctx,
                           batch_stride_ctx, (bf16*)hidden_out);
    else
        hipLaunchKernelGGL(contrastive_pick_kernel<float>, dim3(B), dim3(CS_THREADS), 0, st, a, (const float*)cand_hidden, ld_cand, (float*)ctx,
                           ld_ctx, batch_stride_ctx, (float*)hidden_out);
    MMGL_CHECK_LAUNCH("mmgl_contrastive_select (pick)");
    return MMGL_OK;
}
