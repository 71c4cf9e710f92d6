// Beam search bookkeeping of generate(num_beams = W): candidate selection over the vocabulary and the per-step state update.
// Reached only from ops.beam_topk / ops.beam_advance.  No atomics, fixed reduction orders: two runs are bitwise equal.
//
// mmgl_beam_topk.  score(row, v) = beam_score[row] + (logit[row][v] - lse(row)) in fp32; per sample the K = 2W best of its rows_in * V
// candidates, sorted descending, an exact tie going to the lower flat index r*V + v (r = the row's slot in the sample).  Two launches:
//   * beam_topk_part_kernel, one workgroup per (row, chunk of BT_CHUNK = 4096 logits): 16 logits per thread in registers (stride-256
//     element loads: any row stride, any alignment, a ragged last chunk), the chunk's (max, sum exp) for the log-sum-exp and its K best
//     logits by K rounds of a workgroup arg-max.  A round needs no removal pass: a candidate is eligible when it orders after the
//     previous round's winner.  The record [max, sum, K values, K indices] goes to the workspace -- 4 (2 + 2K) bytes per (row, chunk),
//     never a [rows, V] intermediate.  Within a row the score is a monotone function of the logit, so the chunk's K best logits hold
//     its K best scores (fp32 rounding can map two different logits of a row to one score; such a pair is ordered by logit here).
//   * beam_topk_merge_kernel, one workgroup per sample: folds each row's chunk states into its lse in chunk order, scores the
//     rows_in * chunks * K surviving candidates into LDS (at most BT_MAX_CAND = 4096, which bounds V: see the entry point) and runs
//     the same K rounds on (score, flat index).
//
// mmgl_beam_advance (beam_advance_kernel), one wave per sample: the sorted candidates become the next step's running beams (the first
// W whose token is not EOS), the parent table of mmgl_attn_decode_beam_fwd (new[w][0..j) = old[parent][0..j), new[w][j] = parent; the
// table is double-buffered) and the pool of finished hypotheses (score / length^penalty, length, ancestry row, last token; the W best,
// sorted; double-buffered likewise).  Plain vector stores only; every float written is a copy or one IEEE division.
#include "common.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int BT_THREADS = 256;
constexpr int BT_PER_THREAD = 16;
constexpr int BT_CHUNK = BT_THREADS * BT_PER_THREAD;
constexpr int BT_MAX_CAND = 4096;
constexpr int BT_MAX_K = 16;

// (value, index) ordering of the selection: higher value first, lower index on a tie; idx < 0 marks "none" and orders last
__device__ __forceinline__ bool bt_before(float va, int ia, float vb, int ib) {
    if (ib < 0) return ia >= 0;
    if (ia < 0) return false;
    return va > vb || (va == vb && ia < ib);
}

// workgroup arg-best of (v, i) in the order of bt_before: butterfly inside the wave, the waves in order through LDS
__device__ __forceinline__ void bt_block_best(float& v, int& i, float* sm_v, int* sm_i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(v, o);
        const int i2 = __shfl_xor(i, o);
        if (bt_before(v2, i2, v, i)) { v = v2; i = i2; }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();                                       // the previous round's readers are done with sm_*
    if (lane == 0) { sm_v[w] = v; sm_i[w] = i; }
    __syncthreads();
    v = sm_v[0];
    i = sm_i[0];
#pragma unroll
    for (int k = 1; k < BT_THREADS / 64; ++k)
        if (bt_before(sm_v[k], sm_i[k], v, i)) { v = sm_v[k]; i = sm_i[k]; }
}

template <typename T>
__global__ __launch_bounds__(BT_THREADS) void beam_topk_part_kernel(const T* __restrict__ logits, size_t ld, int V, int K, int nchunk,
                                                                    float* __restrict__ ws) {
    __shared__ float sm_v[BT_THREADS / 64];
    __shared__ int sm_i[BT_THREADS / 64];
    const int row = blockIdx.x / nchunk, ch = blockIdx.x % nchunk;
    const int tid = threadIdx.x, v0 = ch * BT_CHUNK;
    const T* x = logits + (size_t)row * ld;
    float val[BT_PER_THREAD];
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < BT_PER_THREAD; ++e) {
        const int v = v0 + e * BT_THREADS + tid;
        val[e] = v < V ? Elem<T>::to_f(x[v]) : -INFINITY;
        mx = fmaxf(mx, val[e]);
    }
    // chunk max, then sum exp(x - max): fixed order (thread-sequential, wave butterfly, waves in order)
    mx = wave_max(mx);
    __syncthreads();
    if ((tid & 63) == 0) sm_v[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sm_v[0], sm_v[1]), fmaxf(sm_v[2], sm_v[3]));
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < BT_PER_THREAD; ++e) sum += v0 + e * BT_THREADS + tid < V ? expf(val[e] - mx) : 0.f;
    sum = wave_sum(sum);
    __syncthreads();
    if ((tid & 63) == 0) sm_v[tid >> 6] = sum;
    __syncthreads();
    sum = ((sm_v[0] + sm_v[1]) + sm_v[2]) + sm_v[3];

    float* rec = ws + ((size_t)row * nchunk + ch) * (2 + 2 * K);
    if (tid == 0) { rec[0] = mx; rec[1] = sum; }
    float last_v = 0.f;
    int last_i = -1;                                        // no winner yet: everything is eligible
    for (int r = 0; r < K; ++r) {
        float bv = 0.f;
        int bi = -1;
#pragma unroll
        for (int e = 0; e < BT_PER_THREAD; ++e) {
            const int v = v0 + e * BT_THREADS + tid;
            const bool eligible = v < V && (r == 0 || bt_before(last_v, last_i, val[e], v));
            if (eligible && bt_before(val[e], v, bv, bi)) { bv = val[e]; bi = v; }
        }
        bt_block_best(bv, bi, sm_v, sm_i);
        if (tid == 0) {
            rec[2 + r] = bv;
            ((int*)rec)[2 + K + r] = bi;                    // -1: the chunk has fewer than K logits
        }
        if (bi < 0) {                                       // uniform: nothing left in this chunk
            for (int r2 = r + 1 + tid; r2 < K; r2 += BT_THREADS) { rec[2 + r2] = 0.f; ((int*)rec)[2 + K + r2] = -1; }
            break;
        }
        last_v = bv;
        last_i = bi;
    }
}

__global__ __launch_bounds__(BT_THREADS) void beam_topk_merge_kernel(const float* __restrict__ ws, const float* __restrict__ beam_score,
                                                                     int rows_in, int V, int K, int nchunk,
                                                                     float* __restrict__ cand_score, int* __restrict__ cand_index) {
    __shared__ float sc[BT_MAX_CAND];
    __shared__ int fl[BT_MAX_CAND];
    __shared__ float lse[8];
    __shared__ float sm_v[BT_THREADS / 64];
    __shared__ int sm_i[BT_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int rec_words = 2 + 2 * K;
    if (tid < rows_in) {
        const float* rec = ws + (size_t)(b * rows_in + tid) * nchunk * rec_words;
        float mx = rec[0];
        for (int c = 1; c < nchunk; ++c) mx = fmaxf(mx, rec[(size_t)c * rec_words]);
        float s = 0.f;
        for (int c = 0; c < nchunk; ++c) s += rec[(size_t)c * rec_words + 1] * expf(rec[(size_t)c * rec_words] - mx);
        lse[tid] = mx + logf(s);
    }
    __syncthreads();
    const int per_row = nchunk * K, ncand = rows_in * per_row;
    for (int i = tid; i < ncand; i += BT_THREADS) {
        const int r = i / per_row, rem = i - r * per_row, c = rem / K, k = rem - c * K;
        const float* rec = ws + ((size_t)(b * rows_in + r) * nchunk + c) * rec_words;
        const int v = ((const int*)rec)[2 + K + k];
        sc[i] = beam_score[b * rows_in + r] + (rec[2 + k] - lse[r]);
        fl[i] = v < 0 ? -1 : r * V + v;
    }
    __syncthreads();
    float last_v = 0.f;
    int last_i = -1;
    for (int r = 0; r < K; ++r) {
        float bv = 0.f;
        int bi = -1;
        for (int i = tid; i < ncand; i += BT_THREADS) {
            const float v = sc[i];
            const int f = fl[i];
            const bool eligible = f >= 0 && (r == 0 || bt_before(last_v, last_i, v, f));
            if (eligible && bt_before(v, f, bv, bi)) { bv = v; bi = f; }
        }
        bt_block_best(bv, bi, sm_v, sm_i);
        if (tid == 0) {
            cand_score[(size_t)b * K + r] = bv;
            cand_index[(size_t)b * K + r] = bi;
        }
        last_v = bv;
        last_i = bi;
    }
}

struct AdvanceArgs {
    const float* cand_score;
    const int* cand_index;
    long long* tokens;
    int* parents;
    float* beam_score;
    const int* src_old;
    int* src_new;
    const float* pool_score_old;
    float* pool_score_new;
    const int* pool_len_old;
    int* pool_len_new;
    const int* pool_anc_old;
    int* pool_anc_new;
    const long long* pool_tok_old;
    long long* pool_tok_new;
    int* done;
    int ld_src, W, V, n_cols, eos, last, early_stopping;
    float len_div;
};

// lane r < 2W holds candidate r; lane W + i (i < W) doubles as the holder of old pool entry i in the merge
__global__ __launch_bounds__(64) void beam_advance_kernel(const AdvanceArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x, W = a.W, K = 2 * W;
    const size_t row0 = (size_t)b * W;
    const bool is_cand = lane < K;
    const float cs = is_cand ? a.cand_score[(size_t)b * K + lane] : 0.f;
    const int flat = is_cand ? a.cand_index[(size_t)b * K + lane] : 0;
    const int parent = flat / a.V, tok = flat - parent * a.V;
    const bool eos = is_cand && tok == a.eos;

    // ---- running beams: the first W candidates that do not end their hypothesis
    const unsigned long long open = __ballot(is_cand && !eos);
    const int slot = __popcll(open & ((1ull << lane) - 1ull));
    const bool runs = is_cand && !eos && slot < W;
    if (runs) {
        a.tokens[row0 + slot] = tok;
        a.parents[row0 + slot] = parent;
        a.beam_score[row0 + slot] = cs;
    }
    const int nc = a.n_cols;                                // columns of the parent table the running beams carry after this step
    for (int s = 0; s < W; ++s) {                           // slot s: which lane feeds it (wave-uniform), then a lane-parallel row copy
        const unsigned long long who = __ballot(runs && slot == s);
        if (!who) continue;
        const int p = __shfl(parent, __ffsll((long long)who) - 1);
        for (int c = lane; c < nc; c += 64)
            a.src_new[(row0 + s) * a.ld_src + c] = c == nc - 1 ? p : a.src_old[(row0 + p) * a.ld_src + c];
    }

    // ---- pool of finished hypotheses: W old entries and the finishing candidates among the first W, the W best sorted descending
    int full_old = 1;
    for (int i = 0; i < W; ++i) full_old &= a.pool_len_old[row0 + i] > 0;
    const bool frozen = a.done[b] != 0 || (a.early_stopping && full_old);
    const bool enters = is_cand && lane < W && (eos || a.last) && !frozen;
    // merged order: old pool entry i at position i, candidate r at position W + r; entry = (valid, score)
    const bool old_holder = lane >= W && lane < K;          // lane W + i reads old entry i
    const int oi = lane - W;
    const bool old_valid = old_holder && a.pool_len_old[row0 + (old_holder ? oi : 0)] > 0;
    const float old_score = old_valid ? a.pool_score_old[row0 + oi] : 0.f;
    const float new_score = cs / a.len_div;
    // rank of an entry = number of entries ordered before it (higher score, or equal score and earlier merged position)
    int rank_new = 0, rank_old = 0;
    for (int x = 0; x < K; ++x) {
        const bool xv_old = __shfl((int)old_valid, x) != 0;         // lane x as old holder (position x - W)
        const float xs_old = __shfl(old_score, x);
        const bool xv_new = __shfl((int)enters, x) != 0;            // lane x as candidate (position W + x)
        const float xs_new = __shfl(new_score, x);
        const int xp_old = x - W, xp_new = W + x;
        if (xv_old) {
            if (xs_old > new_score || (xs_old == new_score && xp_old < W + lane)) ++rank_new;
            if (xs_old > old_score || (xs_old == old_score && xp_old < oi)) ++rank_old;
        }
        if (xv_new) {
            if (xs_new > new_score || (xs_new == new_score && xp_new < W + lane)) ++rank_new;
            if (xs_new > old_score || (xs_new == old_score && xp_new < oi)) ++rank_old;
        }
    }
    const int ac = nc;                                      // an ancestry row has as many columns as the parents' table after this step
    int n_valid = 0;
    for (int s = 0; s < W; ++s) {                           // pool slot s: filled by one old entry, one candidate, or left empty
        const unsigned long long from_old = __ballot(old_valid && rank_old == s);
        const unsigned long long from_new = __ballot(enters && rank_new == s);
        if (from_old) {
            const int i = __ffsll((long long)from_old) - 1 - W;
            if (lane == 0) {
                a.pool_score_new[row0 + s] = a.pool_score_old[row0 + i];
                a.pool_len_new[row0 + s] = a.pool_len_old[row0 + i];
                a.pool_tok_new[row0 + s] = a.pool_tok_old[row0 + i];
            }
            for (int c = lane; c < a.ld_src; c += 64) a.pool_anc_new[(row0 + s) * a.ld_src + c] = a.pool_anc_old[(row0 + i) * a.ld_src + c];
            ++n_valid;
        } else if (from_new) {
            const int r = __ffsll((long long)from_new) - 1;
            const int p = __shfl(parent, r);
            const int t = __shfl(tok, r);
            const float sco = __shfl(new_score, r);
            if (lane == 0) {
                a.pool_score_new[row0 + s] = sco;
                a.pool_len_new[row0 + s] = nc + 1;
                a.pool_tok_new[row0 + s] = t;
            }
            for (int c = lane; c < a.ld_src; c += 64)
                a.pool_anc_new[(row0 + s) * a.ld_src + c] = c < ac - 1 ? a.src_old[(row0 + p) * a.ld_src + c] : (c == ac - 1 ? p : 0);
            ++n_valid;
        } else {
            if (lane == 0) {
                a.pool_score_new[row0 + s] = -INFINITY;
                a.pool_len_new[row0 + s] = 0;
                a.pool_tok_new[row0 + s] = 0;
            }
            for (int c = lane; c < a.ld_src; c += 64) a.pool_anc_new[(row0 + s) * a.ld_src + c] = 0;
        }
    }
    // ---- the early-stop heuristic: once the best running beam cannot beat the worst pooled hypothesis, the pool is closed for good
    if (n_valid == W) {
        const unsigned long long lastq = __ballot((old_valid && rank_old == W - 1) || (enters && rank_new == W - 1));
        const int x = __ffsll((long long)lastq) - 1;
        const bool is_old = __shfl((int)(old_valid && rank_old == W - 1), x) != 0;
        const float worst = is_old ? __shfl(old_score, x) : __shfl(new_score, x);
        const unsigned long long first = __ballot(runs && slot == 0);
        const float best = __shfl(cs, __ffsll((long long)first) - 1) / a.len_div;
        if (lane == 0 && !(best > worst)) a.done[b] = 1;
    }
}

}  // namespace

extern "C" size_t mmgl_beam_topk_workspace(int rows, int V, int W) {
    if (rows < 1 || V < 1 || W < 1) return 0;
    return (size_t)rows * cdiv(V, BT_CHUNK) * (2 + 4 * W) * sizeof(float);
}

extern "C" int mmgl_beam_topk(const void* logits, size_t ld_logits, const float* beam_score, float* cand_score, int* cand_index, void* workspace,
                              size_t workspace_bytes, int B, int rows_in, int W, int V, int dtype, void* stream) {
    MMGL_CHECK_ARG(B >= 1 && rows_in >= 1 && W >= 1 && V >= 1, "mmgl_beam_topk: bad sizes B=%d rows_in=%d W=%d V=%d", B, rows_in, W, V);
    if (W > 8) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_beam_topk: %d beams per sample (1..8)", W);
    MMGL_CHECK_ARG(rows_in == 1 || rows_in == W, "mmgl_beam_topk: rows_in=%d is neither 1 (the prefill's row) nor W=%d", rows_in, W);
    MMGL_CHECK_ARG(V >= 2 * W, "mmgl_beam_topk: V=%d holds fewer than 2W=%d candidates", V, 2 * W);
    MMGL_CHECK_ARG(dtype == MMGL_BF16 || dtype == MMGL_F32, "mmgl_beam_topk: bad dtype %d", dtype);
    MMGL_CHECK_ARG(logits && beam_score && cand_score && cand_index && workspace, "mmgl_beam_topk: null pointer");
    MMGL_CHECK_ARG(ld_logits >= (size_t)V, "mmgl_beam_topk: row stride %zu smaller than V=%d", ld_logits, V);
    const int K = 2 * W, nchunk = cdiv(V, BT_CHUNK);
    if ((long long)rows_in * nchunk * K > BT_MAX_CAND)
        MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_beam_topk: rows_in=%d x %d chunks x 2W=%d candidates exceed %d (V <= %d at this W)", rows_in, nchunk, K,
                  BT_MAX_CAND, BT_MAX_CAND / (rows_in * K) * BT_CHUNK);
    MMGL_CHECK_ARG((long long)B * rows_in * nchunk < (1ll << 31), "mmgl_beam_topk: too many rows");
    MMGL_CHECK_ARG((long long)rows_in * V < (1ll << 31), "mmgl_beam_topk: the flat index rows_in * V overflows int32");
    MMGL_CHECK_ARG(workspace_bytes >= mmgl_beam_topk_workspace(B * rows_in, V, W) && ((uintptr_t)workspace & 3) == 0,
                   "mmgl_beam_topk: the workspace holds %zu bytes, %zu needed (4-byte aligned)", workspace_bytes,
                   mmgl_beam_topk_workspace(B * rows_in, V, W));
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(B * rows_in * nchunk), block(BT_THREADS);
    if (dtype == MMGL_BF16)
        hipLaunchKernelGGL(beam_topk_part_kernel<bf16>, grid, block, 0, st, (const bf16*)logits, ld_logits, V, K, nchunk, (float*)workspace);
    else
        hipLaunchKernelGGL(beam_topk_part_kernel<float>, grid, block, 0, st, (const float*)logits, ld_logits, V, K, nchunk, (float*)workspace);
    MMGL_CHECK_LAUNCH("mmgl_beam_topk (chunks)");
    hipLaunchKernelGGL(beam_topk_merge_kernel, dim3(B), block, 0, st, (const float*)workspace, beam_score, rows_in, V, K, nchunk, cand_score, cand_index);
    MMGL_CHECK_LAUNCH("mmgl_beam_topk (merge)");
    return MMGL_OK;
}

extern "C" int mmgl_beam_advance(const float* cand_score, const int* cand_index, int64_t* tokens, int* parents, float* beam_score,
                                 const int* src_old, int* src_new, int ld_src, const float* pool_score_old, float* pool_score_new,
                                 const int* pool_len_old, int* pool_len_new, const int* pool_anc_old, int* pool_anc_new,
                                 const int64_t* pool_tok_old, int64_t* pool_tok_new, int* done, int B, int W, int V, int n_cols, int eos_token_id,
                                 int last_step, int early_stopping, float length_divisor, void* stream) {
    MMGL_CHECK_ARG(B >= 1 && W >= 1 && V >= 2 * W && n_cols >= 0, "mmgl_beam_advance: bad sizes B=%d W=%d V=%d n_cols=%d", B, W, V, n_cols);
    if (W > 8) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_beam_advance: %d beams per sample (1..8)", W);
    MMGL_CHECK_ARG(cand_score && cand_index && tokens && parents && beam_score && src_old && src_new && pool_score_old && pool_score_new &&
                       pool_len_old && pool_len_new && pool_anc_old && pool_anc_new && pool_tok_old && pool_tok_new && done,
                   "mmgl_beam_advance: null pointer");
    MMGL_CHECK_ARG(src_old != src_new && pool_score_old != pool_score_new && pool_len_old != pool_len_new && pool_anc_old != pool_anc_new &&
                       pool_tok_old != pool_tok_new,
                   "mmgl_beam_advance: the old and the new buffers must differ (rows are read while others are written)");
    MMGL_CHECK_ARG(ld_src >= n_cols && ld_src >= 1, "mmgl_beam_advance: row stride %d smaller than n_cols=%d", ld_src, n_cols);
    MMGL_CHECK_ARG(length_divisor > 0.f, "mmgl_beam_advance: length divisor %g", (double)length_divisor);
    const AdvanceArgs a{cand_score, cand_index, (long long*)tokens, parents, beam_score, src_old, src_new, pool_score_old, pool_score_new, pool_len_old,
                        pool_len_new, pool_anc_old, pool_anc_new, (const long long*)pool_tok_old, (long long*)pool_tok_new, done, ld_src, W, V, n_cols,
                        eos_token_id, last_step, early_stopping, length_divisor};
    hipLaunchKernelGGL(beam_advance_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    MMGL_CHECK_LAUNCH("mmgl_beam_advance");
    return MMGL_OK;
}
