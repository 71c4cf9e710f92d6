// Sampling step of generate(do_sample=True): temperature, top-k, top-p and the draw in one launch.  Reached only from ops.sample_tokens.
//
// mmgl_sample_tokens (sample_tokens_kernel), one workgroup of 1024 threads per logits row; the row (100 KB of bf16 at V = 50272) is
// re-read from L2 by every pass, element loads at stride 1024 (any row stride, any alignment).  With x = logit / temperature in fp32
// (NaN counts as -inf):
//   * both filters are thresholds on a monotone integer key (the order-preserving bits of x for fp32 rows; of the logit for bf16 rows,
//     16 bits): token v is kept iff measure{w : x_w > x_v} < bound, the measure being a count (top-k, bound k) or a probability mass
//     (top-p, bound top_p * Z over the top-k survivors).  A radix descent, 8 key bits per pass, finds the lowest kept key: a 256-bin
//     histogram of (count, mass) of the elements that match the prefix found so far, then the lowest digit whose measure-above is
//     below the bound.  Every token tied with the boundary shares its key, so ties are all in.
//   * a mass is the INTEGER m_v = trunc(2^40 * expf(x_v - max x)) (the row's max has m = 2^40; V <= 2^17 keeps every sum below 2^57).
//     Integer sums do not depend on their order: the histograms are LDS integer atomics, two runs are bitwise equal, and the sums of
//     the draw's two phases agree exactly.  No floating-point atomics anywhere.
//   * draw: target = floor(Z_K * floor(u * 2^32) / 2^32) < Z_K; the token is the smallest kept v, in vocabulary index order, whose
//     running sum of m exceeds it.  Phase 1: wave w sums segment [w S, (w+1) S) (S = 64 ceil(V / 1024), coalesced tiles of 64), the 16
//     totals give the segment; phase 2: the workgroup scans that one segment, ceil(S / 1024) <= 8 contiguous elements per thread.
//     n_draws > 1 (the first step of num_return_sequences) repeats phase 2 per draw on the same kept set.
//   * EOS bookkeeping of the greedy loops: a finished draw gets pad_token_id, a draw that returns eos_token_id becomes finished.
// The token is an index the scan visited, so it lies in [0, V) whatever the logits hold.  Plain vector stores only.
#include "common.h"
#include <math.h>

namespace {

constexpr int ST_THREADS = 1024;
constexpr int ST_WAVES = ST_THREADS / 64;
constexpr int ST_BINS = 256;
constexpr int ST_REP = 8;                                   // histogram replicas, indexed by lane & 7: logits crowd into few exponent bins
constexpr float ST_ONE = 1099511627776.f;                   // 2^40
constexpr int ST_MAX_V = 131072;
constexpr int ST_MAX_DRAWS = 8;

typedef unsigned long long u64;

template <typename T> struct StKey;
template <> struct StKey<float> {
    static constexpr int BITS = 32;
    static __device__ __forceinline__ void load(const float* row, int v, float temp, float& x, uint32_t& key) {
        x = row[v] / temp + 0.f;                            // + 0: -0 and +0 are one value, so one key
        if (!(x == x)) { x = -INFINITY; key = 0u; return; }
        const uint32_t b = __float_as_uint(x);
        key = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    }
};
template <> struct StKey<bf16> {
    static constexpr int BITS = 16;
    static __device__ __forceinline__ void load(const bf16* row, int v, float temp, float& x, uint32_t& key) {
        uint32_t b = ((const unsigned short*)row)[v];
        x = __uint_as_float(b << 16) / temp + 0.f;
        if (!(x == x)) { x = -INFINITY; key = 0u; return; }
        if (b == 0x8000u) b = 0u;
        key = b ^ ((b >> 15) ? 0xFFFFu : 0x8000u);
    }
};

__device__ __forceinline__ u64 st_mass(float x, float mx) { return x == mx ? (u64)ST_ONE : (u64)(expf(x - mx) * ST_ONE); }

__device__ __forceinline__ u64 st_wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct StShared {
    u64 h_mass[ST_BINS * ST_REP];
    u64 b_mass[ST_BINS];
    u64 g_mass[16];
    u64 wave[ST_WAVES];                                     // phase 1 segment totals
    u64 scan[ST_WAVES];                                     // phase 2 wave totals
    u64 sel_above_m, sel_bin_m;
    unsigned int h_cnt[ST_BINS * ST_REP];
    unsigned int b_cnt[ST_BINS];
    unsigned int g_cnt[16];
    unsigned int sel_digit, sel_above_c, sel_bin_c;
    float mx[ST_WAVES];
};

// Lowest kept key among the elements with key >= floor_key: by count (bound_c > 0: fewer than bound_c elements above) or by mass
// (bound_c = 0: less than top_p of their total mass above).  Returns the key; cnt = the elements kept.
template <typename T>
__device__ __forceinline__ uint32_t st_descend(StShared& sm, const T* row, int V, float temp, float mx, uint32_t floor_key, unsigned int bound_c,
                                               float top_p, unsigned int& cnt) {
    const int tid = threadIdx.x;
    uint32_t prefix = 0u;
    unsigned int base_c = 0u;
    u64 base_m = 0ull, bound_m = 0ull;
    for (int shift = StKey<T>::BITS - 8; shift >= 0; shift -= 8) {
        for (int i = tid; i < ST_BINS * ST_REP; i += ST_THREADS) { sm.h_cnt[i] = 0u; sm.h_mass[i] = 0ull; }
        __syncthreads();
        const bool first = shift == StKey<T>::BITS - 8;
        for (int v = tid; v < V; v += ST_THREADS) {
            float x;
            uint32_t key;
            StKey<T>::load(row, v, temp, x, key);
            const bool match = key >= floor_key && (first || ((key ^ prefix) >> ((shift + 8) & 31)) == 0u);
            if (match) {
                const int slot = (int)((key >> shift) & 255u) * ST_REP + (tid & (ST_REP - 1));
                atomicAdd(&sm.h_cnt[slot], 1u);
                atomicAdd(&sm.h_mass[slot], st_mass(x, mx));
            }
        }
        __syncthreads();
        if (tid < ST_BINS) {
            unsigned int c = 0u;
            u64 m = 0ull;
#pragma unroll
            for (int r = 0; r < ST_REP; ++r) { c += sm.h_cnt[tid * ST_REP + r]; m += sm.h_mass[tid * ST_REP + r]; }
            sm.b_cnt[tid] = c;
            sm.b_mass[tid] = m;
        }
        __syncthreads();
        if (tid < 16) {
            unsigned int c = 0u;
            u64 m = 0ull;
            for (int i = 0; i < 16; ++i) { c += sm.b_cnt[tid * 16 + i]; m += sm.b_mass[tid * 16 + i]; }
            sm.g_cnt[tid] = c;
            sm.g_mass[tid] = m;
        }
        __syncthreads();
        if (first && bound_c == 0u) {                       // the bins of the first pass hold every survivor: their total is Z
            u64 z = 0ull;
            for (int g = 0; g < 16; ++g) z += sm.g_mass[g];
            bound_m = (u64)((double)top_p * (double)z);
            if (bound_m < 1ull) bound_m = 1ull;             // the largest logit is always kept
        }
        if (tid < ST_BINS) {
            const int d = tid, g = d >> 4;
            unsigned int ac = base_c;
            u64 am = base_m;
            for (int gg = g + 1; gg < 16; ++gg) { ac += sm.g_cnt[gg]; am += sm.g_mass[gg]; }
            for (int dd = d + 1; dd < g * 16 + 16; ++dd) { ac += sm.b_cnt[dd]; am += sm.b_mass[dd]; }
            const unsigned int bc = sm.b_cnt[d];
            const u64 bm = sm.b_mass[d];
            const bool here = bound_c ? ac < bound_c : am < bound_m;
            const bool lower = d > 0 && (bound_c ? ac + bc < bound_c : am + bm < bound_m);
            if (here && !lower) {                           // exactly one digit: `here` is monotone in d and holds at d = 255
                sm.sel_digit = (unsigned int)d;
                sm.sel_above_c = ac;
                sm.sel_above_m = am;
                sm.sel_bin_c = bc;
                sm.sel_bin_m = bm;
            }
        }
        __syncthreads();
        prefix |= sm.sel_digit << shift;
        base_c = sm.sel_above_c;
        base_m = sm.sel_above_m;
    }
    cnt = base_c + sm.sel_bin_c;
    return prefix;
}

template <typename T>
__global__ __launch_bounds__(ST_THREADS) void sample_tokens_kernel(const T* __restrict__ logits, size_t ld, const float* __restrict__ u,
                                                                   long long* __restrict__ tokens, long long tok_stride,
                                                                   unsigned char* __restrict__ finished, int* __restrict__ kept_out, int V,
                                                                   int n_draws, float temp, int top_k, float top_p, int eos, long long pad) {
    __shared__ StShared sm;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int rowi = blockIdx.x;
    const T* row = logits + (size_t)rowi * ld;

    // ---- max of x
    float mx = -INFINITY;
    for (int v = tid; v < V; v += ST_THREADS) {
        float x;
        uint32_t key;
        StKey<T>::load(row, v, temp, x, key);
        mx = fmaxf(mx, x);
    }
    mx = wave_max(mx);
    if (lane == 0) sm.mx[w] = mx;
    __syncthreads();
    mx = sm.mx[0];
#pragma unroll
    for (int i = 1; i < ST_WAVES; ++i) mx = fmaxf(mx, sm.mx[i]);

    // ---- the kept set: key >= floor_key
    uint32_t floor_key = 0u;
    unsigned int kept = (unsigned int)V;
    if (top_k > 0 && top_k < V) floor_key = st_descend<T>(sm, row, V, temp, mx, 0u, (unsigned int)top_k, 1.f, kept);
    if (top_p < 1.f) {
        const uint32_t t = st_descend<T>(sm, row, V, temp, mx, floor_key, 0u, top_p, kept);
        floor_key = t > floor_key ? t : floor_key;
    }
    if (tid == 0 && kept_out) kept_out[rowi] = (int)kept;

    // ---- draw, phase 1: the kept mass of each wave's segment
    const int S = 64 * ((V + ST_THREADS - 1) / ST_THREADS);
    {
        const int lo = w * S, hi = min(lo + S, V);
        u64 col = 0ull;
        for (int v = lo + lane; v < hi; v += 64) {
            float x;
            uint32_t key;
            StKey<T>::load(row, v, temp, x, key);
            col += key >= floor_key ? st_mass(x, mx) : 0ull;
        }
        col = st_wave_sum(col);
        if (lane == 0) sm.wave[w] = col;
    }
    __syncthreads();
    u64 Z = 0ull;
#pragma unroll
    for (int i = 0; i < ST_WAVES; ++i) Z += sm.wave[i];

    // ---- phase 2, per draw
    const int e = (S + ST_THREADS - 1) / ST_THREADS;
    for (int j = 0; j < n_draws; ++j) {
        const float uu = u[(size_t)rowi * n_draws + j];
        const uint32_t U = uu >= 0.f ? (uu >= 1.f ? 0xFFFFFFFFu : (uint32_t)(uu * 4294967296.f)) : 0u;      // NaN: 0
        const u64 target = __umul64hi(Z, (u64)U << 32);      // floor(Z U / 2^32) < Z
        int ws = ST_WAVES - 1;
        u64 acc = 0ull;
        for (int i = 0; i < ST_WAVES; ++i) {
            const u64 t = sm.wave[i];
            if (target < acc + t) { ws = i; break; }
            acc += t;
        }
        const u64 r = target - acc;
        const int seg_hi = min(ws * S + S, V);
        const int lo = min(ws * S + tid * e, seg_hi), hi = min(lo + e, seg_hi);
        u64 own = 0ull;
        for (int v = lo; v < hi; ++v) {
            float x;
            uint32_t key;
            StKey<T>::load(row, v, temp, x, key);
            own += key >= floor_key ? st_mass(x, mx) : 0ull;
        }
        u64 incl = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u64 t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63) sm.scan[w] = incl;
        __syncthreads();
        u64 excl = incl - own;
        for (int i = 0; i < w; ++i) excl += sm.scan[i];
        if (excl <= r && r < excl + own) {                   // one thread: the segment's masses sum to sm.wave[ws] > r exactly
            u64 c = excl;
            int tok = hi - 1;
            for (int v = lo; v < hi; ++v) {
                float x;
                uint32_t key;
                StKey<T>::load(row, v, temp, x, key);
                c += key >= floor_key ? st_mass(x, mx) : 0ull;
                if (c > r) { tok = v; break; }
            }
            const size_t i = (size_t)rowi * n_draws + j;
            long long out = tok;
            if (finished) {
                if (finished[i]) out = pad;
                else if (tok == eos) finished[i] = 1;
            }
            tokens[i * tok_stride] = out;
        }
        __syncthreads();                                     // sm.scan is rewritten by the next draw
    }
}

}  // namespace

extern "C" int mmgl_sample_tokens(const void* logits, size_t ld_logits, const float* u, int64_t* tokens, int64_t token_stride, uint8_t* finished,
                                  int* kept, int rows, int n_draws, int V, float temperature, int top_k, float top_p, int eos_token_id,
                                  int64_t pad_token_id, int dtype, void* stream) {
    MMGL_CHECK_ARG(rows >= 1 && V >= 1 && n_draws >= 1, "mmgl_sample_tokens: bad sizes rows=%d V=%d n_draws=%d", rows, V, n_draws);
    if (V > ST_MAX_V) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_sample_tokens: V=%d (at most %d)", V, ST_MAX_V);
    if (n_draws > ST_MAX_DRAWS) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "mmgl_sample_tokens: %d draws per row (1..%d)", n_draws, ST_MAX_DRAWS);
    MMGL_CHECK_ARG(temperature > 0.f && temperature <= 3.0e38f, "mmgl_sample_tokens: temperature %g must be positive and finite", (double)temperature);
    MMGL_CHECK_ARG(top_k >= 0, "mmgl_sample_tokens: top_k=%d must not be negative (0: off)", top_k);
    MMGL_CHECK_ARG(top_p > 0.f && top_p <= 1.f, "mmgl_sample_tokens: top_p %g outside (0, 1]", (double)top_p);
    MMGL_CHECK_ARG(dtype == MMGL_BF16 || dtype == MMGL_F32, "mmgl_sample_tokens: bad dtype %d", dtype);
    MMGL_CHECK_ARG(logits && u && tokens, "mmgl_sample_tokens: null pointer");
    MMGL_CHECK_ARG(ld_logits >= (size_t)V, "mmgl_sample_tokens: row stride %zu smaller than V=%d", ld_logits, V);
    MMGL_CHECK_ARG(token_stride >= 1, "mmgl_sample_tokens: token stride %lld must be positive", (long long)token_stride);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(rows), block(ST_THREADS);
    if (dtype == MMGL_BF16)
        hipLaunchKernelGGL(sample_tokens_kernel<bf16>, grid, block, 0, st, (const bf16*)logits, ld_logits, u, (long long*)tokens, (long long)token_stride,
                           finished, kept, V, n_draws, temperature, top_k, top_p, eos_token_id, (long long)pad_token_id);
    else
        hipLaunchKernelGGL(sample_tokens_kernel<float>, grid, block, 0, st, (const float*)logits, ld_logits, u, (long long*)tokens,
                           (long long)token_stride, finished, kept, V, n_draws, temperature, top_k, top_p, eos_token_id, (long long)pad_token_id);
    MMGL_CHECK_LAUNCH("mmgl_sample_tokens");
    return MMGL_OK;
}
