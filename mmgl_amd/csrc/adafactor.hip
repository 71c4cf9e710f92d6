// Fused Adafactor over the flat buffers of DataParallelEngine: transformers.optimization.Adafactor.step as the reference configures it
// (beta1 None, no relative step, no parameter scaling), every trainable tensor of the engine in FOUR launches whatever their number.
//
//   tiles      a 2-D tensor [R, C] is cut into TR x TC = 64 x 256 tiles, a 1-D tensor into runs of TR * TC elements; a workgroup of 256
//              threads finds its (tensor, tile) by a binary search over the table's tile-count prefix.  Thread t owns column tc * 256 + t
//              of the tile and walks its rows: every access is one element per lane, consecutive lanes on consecutive addresses, so a row
//              of odd C that starts on no vector boundary needs no special case and no lane reaches past its tensor.
//   launch 1   2-D: per tile the row sums (over the tile's columns) and column sums (over its rows) of g^2 + eps1 -> workspace.
//              1-D: v = beta2t v + (1 - beta2t)(g^2 + eps1) in place, and the tile's sum of u^2, u = g rsqrt(v).
//   launch 2   fold: row_i = beta2t row_i + (1 - beta2t) (sum_tc rowpart) / C, 256 rows per workgroup, and the workgroup's sum of the new
//              rows; col_j = beta2t col_j + (1 - beta2t) (sum_tr colpart) / R, 64 columns per workgroup, the tile rows in four runs.
//   launch 3   2-D: per tile the sum of u^2, u = (rsqrt(row_i / mean(row)) rsqrt(col_j)) g.  sum u^2 is no function of the row and
//              column sums, so the gradient is read a second time here and a third time by the apply pass.
//   launch 4   apply: d = max(1, sqrt(sum u^2 / numel) / clip); p = p + (-lr wd) p - lr (u / d); master and parameter stored.
//
// Every reduction has a fixed order -- a thread's own run in index order, the 64 lanes by the xor butterfly, the four waves and the
// workgroups' partials in index order -- and nothing is accumulated by atomics: two runs give the same bits.  The sums themselves are
// accumulated in double, their partials kept as doubles in the workspace, and the new row, col and v are formed in double and rounded to
// fp32 once: a gradient of 1e4 beside
// gradients of 1 puts 1e8 into a row and a column, and an fp32 run of 64 adds behind it drops every one of the small terms (measured:
// 3.5 fp32 units on that column where torch's own reduction is within a tenth of one).  The elementwise arithmetic stays fp32.
// The padding between tensors is never read or written.  The table is validated on the host when it is planned (mmgl_adafactor_workspace); the kernels trust it.
#include "common.h"
#include <math.h>

namespace {

constexpr int TR = 64, TC = 256, NT = 256;      // tile rows, tile columns, threads
constexpr int FR = 256, FC = 64;                // rows / columns one fold workgroup owns
constexpr int TW = 8;                           // int64 words of a table row
// table row i (i < n): 0 flat offset, 1 R (1-D: numel), 2 C (1-D: 0), 3 state offset (row | col, or v), 4 first tile, 5 first fold
// workgroup, 6 workspace offset (doubles), 7 tile columns.  Row n: the totals in words 4, 5, 6.
// workspace of a 2-D tensor: rowpart [R, ntc] | colpart [ntr, C] | rowsum [ceil(R / FR)] | u2part [ntr * ntc]; of a 1-D tensor: u2part.

struct Seg {
    long long off, R, C, st, tile0, fold0, ws;
    int ntc, ntr, nfr, ntiles;
    __device__ __forceinline__ long long rowpart() const { return ws; }
    __device__ __forceinline__ long long colpart() const { return ws + R * ntc; }
    __device__ __forceinline__ long long rowsum() const { return colpart() + (long long)ntr * C; }
    __device__ __forceinline__ long long u2part() const { return C ? rowsum() + nfr : ws; }
};

__device__ __forceinline__ Seg find_seg(const long long* __restrict__ table, int n, long long id, int field) {
    int lo = 0, hi = n;                          // the last tensor whose first tile / fold workgroup is <= id
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (table[(size_t)mid * TW + field] <= id) lo = mid; else hi = mid;
    }
    const long long* r = table + (size_t)lo * TW;
    Seg s;
    s.off = r[0], s.R = r[1], s.C = r[2], s.st = r[3], s.tile0 = r[4], s.fold0 = r[5], s.ws = r[6], s.ntc = (int)r[7];
    s.ntiles = (int)(r[TW + 4] - r[4]);
    s.ntr = s.C ? (int)((s.R + TR - 1) / TR) : s.ntiles;
    s.nfr = (int)((s.R + FR - 1) / FR);
    return s;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the sum over the workgroup, in every thread: butterfly inside a wave, the four waves in index order.  `red` holds 4 doubles.
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    __syncthreads();                             // the previous use of red is over
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// the sum of n workspace partials, in every thread: thread t adds partials t, t + 256, ... in that order, then block_sum
__device__ __forceinline__ double fold_partials(const double* __restrict__ p, int n, double* red) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += NT) s += p[i];
    return block_sum(s, red);
}

template <typename T> __device__ __forceinline__ float ldg(const T* __restrict__ grad, long long i, float gs) {
    return Elem<T>::to_f(grad[i]) * gs;
}

// ------------------------------------------------------------------------------------------ launch 1
template <typename T>
__global__ __launch_bounds__(NT) void adafactor_partials_kernel(const T* __restrict__ grad, float* __restrict__ state,
                                                                const long long* __restrict__ table, int n, double* __restrict__ wsp,
                                                                float b2, float omb2, float eps1, float gs) {
    __shared__ double red[4];
    __shared__ double rows[TR][4];
    const Seg s = find_seg(table, n, blockIdx.x, 4);
    const int t = (int)(blockIdx.x - s.tile0), tid = threadIdx.x;
    if (s.C == 0) {                              // 1-D: the second moment is per element, updated here
        const long long e0 = (long long)t * (TR * TC);
        double acc = 0.0;
#pragma unroll 8
        for (int k = 0; k < TR; ++k) {
            const long long e = e0 + k * TC + tid;
            if (e < s.R) {
                const float g = ldg(grad, s.off + e, gs);
                const float v = (float)((double)b2 * (double)state[s.st + e] + (double)omb2 * ((double)g * (double)g + (double)eps1));
                state[s.st + e] = v;
                const float u = g * rsqrtf(v);
                acc += (double)(u * u);
            }
        }
        acc = block_sum(acc, red);
        if (tid == 0) wsp[s.u2part() + t] = acc;
        return;
    }
    const int tr = t / s.ntc, tc = t - tr * s.ntc;
    const long long r0 = (long long)tr * TR, c = (long long)tc * TC + tid;
    const int nr = (int)min((long long)TR, s.R - r0);
    const bool live = c < s.C;
    double col = 0.0;
    for (int k0 = 0; k0 < nr; k0 += 8) {
        float x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            x[k] = 0.f;
            if (live && k0 + k < nr) {
                const float g = ldg(grad, s.off + (r0 + k0 + k) * s.C + c, gs);
                x[k] = g * g + eps1;
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            col += (double)x[k];
            const double rs = wave_sum((double)x[k]);
            if ((tid & 63) == 0 && k0 + k < nr) rows[k0 + k][tid >> 6] = rs;
        }
    }
    if (live) wsp[s.colpart() + (long long)tr * s.C + c] = col;
    __syncthreads();
    if (tid < nr) wsp[s.rowpart() + (r0 + tid) * s.ntc + tc] = ((rows[tid][0] + rows[tid][1]) + rows[tid][2]) + rows[tid][3];
}

// ------------------------------------------------------------------------------------------ launch 2
__global__ __launch_bounds__(NT) void adafactor_fold_kernel(float* __restrict__ state, const long long* __restrict__ table, int n,
                                                            double* __restrict__ wsp, float b2, float omb2) {
    __shared__ double red[4];
    __shared__ double quarter[4][FC];
    const Seg s = find_seg(table, n, blockIdx.x, 5);
    const int f = (int)(blockIdx.x - s.fold0), tid = threadIdx.x;
    if (f < s.nfr) {                             // 256 rows
        const long long r = (long long)f * FR + tid;
        float nv = 0.f;
        if (r < s.R) {
            const double* p = wsp + s.rowpart() + r * s.ntc;
            double sum = 0.0;
            for (int k = 0; k < s.ntc; ++k) sum += p[k];
            nv = (float)((double)b2 * (double)state[s.st + r] + (double)omb2 * (sum / (double)s.C));
            state[s.st + r] = nv;
        }
        const double tot = block_sum((double)nv, red);
        if (tid == 0) wsp[s.rowsum() + f] = tot;
        return;
    }
    // 64 columns; the ntr tile rows in four runs of `run`, one per thread quarter, summed in run order
    const int q = tid >> 6;
    const long long c = (long long)(f - s.nfr) * FC + (tid & 63);
    const int run = (s.ntr + 3) / 4, k0 = q * run, k1 = min(s.ntr, k0 + run);
    double sum = 0.0;
    if (c < s.C) {
        const double* p = wsp + s.colpart() + c;
#pragma unroll 8
        for (int k = k0; k < k1; ++k) sum += p[(long long)k * s.C];
    }
    quarter[q][tid & 63] = sum;
    __syncthreads();
    if (q == 0 && c < s.C) {
        sum = ((quarter[0][tid] + quarter[1][tid]) + quarter[2][tid]) + quarter[3][tid];
        state[s.st + s.R + c] = (float)((double)b2 * (double)state[s.st + s.R + c] + (double)omb2 * (sum / (double)s.R));
    }
}

// ------------------------------------------------------------------------------------------ launches 3 and 4
// APPLY false: the tile's sum of u^2 (2-D tensors; a 1-D tile has its sum from launch 1).  APPLY true: the parameter update.
template <typename T, bool APPLY>
__global__ __launch_bounds__(NT) void adafactor_update_kernel(T* __restrict__ param, float* __restrict__ master, const T* __restrict__ grad,
                                                              const float* __restrict__ state, const long long* __restrict__ table, int n,
                                                              double* __restrict__ wsp, float lr, float wdlr, float clip, float gs) {
    __shared__ double red[4];
    __shared__ float rf[TR];
    const Seg s = find_seg(table, n, blockIdx.x, 4);
    const int t = (int)(blockIdx.x - s.tile0), tid = threadIdx.x;
    if (!APPLY && s.C == 0) return;
    float d = 1.f;
    if (APPLY) {
        const double u2 = fold_partials(wsp + s.u2part(), s.ntiles, red);
        d = fmaxf(1.f, sqrtf((float)(u2 / (double)(s.C ? s.R * s.C : s.R))) / clip);
    }
    auto step = [&](long long i, float u) {      // i: flat index
        float p = master ? master[i] : Elem<T>::to_f(param[i]);
        u = (u / d) * lr;
        if (wdlr != 0.f) p = p + wdlr * p;
        p = p - u;
        if (master) master[i] = p;
        param[i] = Elem<T>::from_f(p);
    };
    if (s.C == 0) {
        const long long e0 = (long long)t * (TR * TC);
#pragma unroll 8
        for (int k = 0; k < TR; ++k) {
            const long long e = e0 + k * TC + tid;
            if (e < s.R) step(s.off + e, ldg(grad, s.off + e, gs) * rsqrtf(state[s.st + e]));
        }
        return;
    }
    const float mean = (float)(fold_partials(wsp + s.rowsum(), s.nfr, red) / (double)s.R);
    const int tr = t / s.ntc, tc = t - tr * s.ntc;
    const long long r0 = (long long)tr * TR, c = (long long)tc * TC + tid;
    const int nr = (int)min((long long)TR, s.R - r0);
    if (tid < nr) rf[tid] = rsqrtf(state[s.st + r0 + tid] / mean);
    __syncthreads();
    const bool live = c < s.C;
    const float cf = live ? rsqrtf(state[s.st + s.R + c]) : 0.f;
    double acc = 0.0;
    if (live) {
#pragma unroll 8
        for (int k = 0; k < nr; ++k) {
            const long long i = s.off + (r0 + k) * s.C + c;
            const float u = (rf[k] * cf) * ldg(grad, i, gs);
            if (APPLY) step(i, u); else acc += (double)(u * u);
        }
    }
    if (!APPLY) {
        acc = block_sum(acc, red);
        if (tid == 0) wsp[s.u2part() + t] = acc;
    }
}

}  // namespace

// Host-side plan: validates the segments and lays out tiles, fold workgroups and workspace.  segs [n, 4] int64: flat offset, R, C
// (0: a 1-D tensor of R elements), state offset.  table_out (NULL, or [n + 1, 8] int64) receives the table the kernels read.
extern "C" size_t mmgl_adafactor_workspace(const int64_t* segs, int n, int64_t* table_out) {
    if (!segs || n < 1) { mmgl_set_error("mmgl_adafactor_workspace: no segments"); return 0; }
    int64_t tiles = 0, folds = 0, ws = 0, end = 0, st_end = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t off = segs[4 * i], R = segs[4 * i + 1], C = segs[4 * i + 2], st = segs[4 * i + 3];
        const int64_t numel = C ? R * C : R, nstate = C ? R + C : R;
        if (R < 1 || C < 0 || R > (1ll << 31) || C > (1ll << 31) || numel > (1ll << 40) || off < end || off % 128 || st < st_end) {
            mmgl_set_error("mmgl_adafactor_workspace: segment %d (offset %lld, R %lld, C %lld, state offset %lld): sizes out of range, a start "
                           "off a 128-element boundary, or an overlap with its predecessor", i, (long long)off, (long long)R, (long long)C,
                           (long long)st);
            return 0;
        }
        end = off + numel, st_end = st + nstate;
        const int64_t ntc = C ? (C + TC - 1) / TC : 0, ntr = (R + TR - 1) / TR;
        const int64_t nt = C ? ntr * ntc : (R + TR * TC - 1) / (TR * TC);
        const int64_t nf = C ? (R + FR - 1) / FR + (C + FC - 1) / FC : 0;
        if (table_out) {
            int64_t* r = table_out + (size_t)i * TW;
            r[0] = off, r[1] = R, r[2] = C, r[3] = st, r[4] = tiles, r[5] = folds, r[6] = ws, r[7] = ntc;
        }
        tiles += nt, folds += nf;
        ws += C ? R * ntc + ntr * C + (R + FR - 1) / FR + nt : nt;
        if (tiles > 0x7fffffff || folds > 0x7fffffff) { mmgl_set_error("mmgl_adafactor_workspace: more than 2^31 tiles"); return 0; }
    }
    if (table_out) {
        int64_t* r = table_out + (size_t)n * TW;
        r[0] = end, r[1] = 0, r[2] = 0, r[3] = st_end, r[4] = tiles, r[5] = folds, r[6] = ws, r[7] = 0;
    }
    return (size_t)ws * sizeof(double);
}

extern "C" int mmgl_adafactor_step(void* param, float* master, const void* grad, float* state, const int64_t* table,
                                   const int64_t* table_host, int n, void* workspace, size_t workspace_bytes, float lr, float eps1,
                                   float clip_threshold, double decay_rate, float weight_decay, int step, float grad_scale, int dtype,
                                   void* stream) {
    MMGL_CHECK_ARG(param && grad && state && table && table_host && workspace && n >= 1 && step >= 1, "mmgl_adafactor_step: bad arguments");
    MMGL_CHECK_ARG(dtype == MMGL_BF16 || dtype == MMGL_F32, "mmgl_adafactor_step: bad dtype %d", dtype);
    MMGL_CHECK_ARG(clip_threshold > 0.f && eps1 >= 0.f && decay_rate < 0.0, "mmgl_adafactor_step: clip_threshold <= 0, eps1 < 0 or decay_rate >= 0");
    const int64_t* tot = table_host + (size_t)n * TW;
    const int64_t tiles = tot[4], folds = tot[5];
    MMGL_CHECK_ARG(tiles >= 1 && tiles <= 0x7fffffff && folds >= 0 && folds <= 0x7fffffff && tot[6] >= 1, "mmgl_adafactor_step: not a planned table");
    MMGL_CHECK_ARG(workspace_bytes >= (size_t)tot[6] * sizeof(double) && ((uintptr_t)workspace & 7) == 0,
                   "mmgl_adafactor_step: workspace of %zu bytes, the table needs %zu (8-byte aligned)", workspace_bytes, (size_t)tot[6] * sizeof(double));
    // in double, rounded once: beta2t = 1 - step^decay_rate and its complement (step 1: 0 and 1 exactly)
    const double pw = pow((double)step, decay_rate);
    const float b2 = (float)(1.0 - pw), omb2 = (float)pw;
    const float wdlr = (float)(-(double)weight_decay * (double)lr);
    hipStream_t st = (hipStream_t)stream;
    double* wsp = (double*)workspace;
    const long long* tb = (const long long*)table;
#define ADAFACTOR_LAUNCHES(T)                                                                                                          \
    do {                                                                                                                               \
        hipLaunchKernelGGL(adafactor_partials_kernel<T>, dim3((unsigned)tiles), dim3(NT), 0, st, (const T*)grad, state, tb, n, wsp, b2, \
                           omb2, eps1, grad_scale);                                                                                    \
        if (folds) {                                                                                                                   \
            hipLaunchKernelGGL(adafactor_fold_kernel, dim3((unsigned)folds), dim3(NT), 0, st, state, tb, n, wsp, b2, omb2);            \
            hipLaunchKernelGGL((adafactor_update_kernel<T, false>), dim3((unsigned)tiles), dim3(NT), 0, st, (T*)param, master,         \
                               (const T*)grad, (const float*)state, tb, n, wsp, lr, wdlr, clip_threshold, grad_scale);                 \
        }                                                                                                                              \
        hipLaunchKernelGGL((adafactor_update_kernel<T, true>), dim3((unsigned)tiles), dim3(NT), 0, st, (T*)param, master,              \
                           (const T*)grad, (const float*)state, tb, n, wsp, lr, wdlr, clip_threshold, grad_scale);                     \
    } while (0)
    if (dtype == MMGL_BF16) ADAFACTOR_LAUNCHES(bf16); else ADAFACTOR_LAUNCHES(float);
#undef ADAFACTOR_LAUNCHES
    MMGL_CHECK_LAUNCH("mmgl_adafactor_step");
    return MMGL_OK;
}
