// T5 attention for gfx950: unscaled scores plus a learned per-head relative-position bias, bidirectional over a rectangular T x S
// problem or causal (T == S), dropout on the probabilities.
//   score[t, s] = q_t . k_s + table[bucket_of[s - t + T - 1], h]          (no D^-0.5: T5 has none; table NULL: no bias)
//   P = softmax over the allowed keys (key_valid[b, s], and s <= t when causal), fp32
//   out = (P * keep(b, h, t, s) / (1 - p_drop)) V                          keep = counter hash of (seed, ((b H + h) T + t) S + s), as
//                                                                          attn_general.hip; regenerated in the backward
// replaces: transformers T5Attention.forward (scores, position_bias = compute_bias(T, S) + mask, softmax, dropout, matmul with V)
// for the three uses of a T5 stack: encoder self-attention, decoder self-attention (causal), decoder-to-encoder cross-attention
// (table NULL).
//
// The lane geometry is selfattn.hip's 16x16 family: swapped products, lane = one query row (forward, dQ) or one key column (dK/dV),
// the additive term of a score tile as the MFMA C-input -- here the key mask AND the bias, read from an LDS-staged row that holds
// table[bucket_of[.], h] along the 127 diagonals of a 64 x 64 tile --, P and dS fed back as the B operand without leaving the lane.
// Kept plain otherwise: one LDS tile buffer, two barriers per tile, D = 64 only.
//
// Backward: delta = rowsum(dO * O); a dQ kernel (workgroup = 64 queries, loop over key tiles) that also sums every row's
// exp(s - lse) and hands 1 / sum to the next kernel (the rounding of lse, the same relative error on a whole row of p, drops out);
// a dK/dV kernel (workgroup = 64 keys, wave = 16 keys, loop over query tiles; every element written once) that also sums dS along the
// diagonals of every tile.
// dtable without floating-point atomics, in a fixed order:
//   1. per 64 x 64 tile each wave of the dK/dV kernel adds its dS into four wave-private LDS rows (one per 16-lane group g: the 16 lanes of a group hold
//      16 different diagonals, so no two lanes of one store meet), one accumulator element after the other;
//   2. thread i of the workgroup folds diagonal i of the tile over g = 0..3 inside wave 0..3, in that order, and writes it to the
//      tile's own 128-float row of the workspace (written once, never accumulated);
//   3. rb_diag_kernel: one thread per (head, diagonal) adds the tile rows that hold it over b, query block, key tile in index order;
//   4. rb_bucket_kernel: one thread per (bucket, head) adds its diagonals in index order.  A bucket no pair reaches gets 0.
// A query row without an allowed key (outside T5's contract) writes zeros to out, 0 to lse and contributes to no gradient.
#include "attn_common.h"

namespace {

constexpr int RB_TILE = 64;        // keys per LDS tile (forward, dQ), queries per LDS tile (dK/dV); rows per workgroup = 4 waves x 16
constexpr int RB_BINS = 80;        // 79 diagonals of a wave's 16 x 64 tile, padded

struct RBArgs {
    const void *q, *k, *v, *dout;
    const uint8_t* key_valid;      // [B, S] or NULL
    const float* table;            // [NB, H] or NULL
    const int32_t* bucket_of;      // [T + S - 1]
    void* out;
    float* lse;                    // [B, H, T]
    float* delta;                  // [B, H, T]
    float* corr;                   // [B, H, T] 1 / sum_s exp(s - lse) of a row: the dQ kernel writes it, the dK/dV kernel reads it
    void *dq, *dk, *dv;
    float* part;                   // [B H nqb nkt][128] diagonal sums per tile
    int B, H, T, S, ldq, ldkv, NB, causal, nqb, nkt;
    float p_drop;
    unsigned long long seed;
};

// one [64, D] operand tile in LDS that serves both the row fragments (A operand of X Y^T) and the transposed fragments (A operand
// of X^T Z): row-major with the LDS transpose read (bf16), fragment-linear row image with gathers (fp32)
template <typename T, typename C> struct Img {
    typedef typename Elem<T>::v8 v8;
    static constexpr int SIZE = C::TIMG ? C::RMIMG : C::ROWIMG;            // elements
    static __device__ __forceinline__ void stage(T* img, const T* base, int row_stride, int rows) {
        if constexpr (C::TIMG) stage_rowmajor_image<T, C>(img, base, row_stride, rows);
        else stage_row_image<T, C>(img, base, row_stride, rows);
    }
    static __device__ __forceinline__ v8 row(const T* img, int sb, int dc, int lane) {
        if constexpr (C::TIMG) return rm_rowfrag<T, C>(img, sb, dc, lane);
        else return *(const v8*)(img + rf_idx<C>(sb, dc, lane));
    }
    static __device__ __forceinline__ v8 tr(const T* img, int db, int ks, int lane) {
        if constexpr (C::TIMG) return rm_tfrag_tr16<C>(img, db, ks, lane);
        else return load_tfrag<T, C>(img, img, db, ks, lane);
    }
};

__device__ __forceinline__ uint32_t rb_thr(float p) { return (uint32_t)fminf(p * 4294967296.f, 4294967295.f); }

// brow[i] = table[bucket_of[s - t + T - 1], h] for the pairs of the tile (queries q0.., keys s0..) with (s - s0) - (t - q0) + 63 == i
__device__ __forceinline__ void rb_stage_brow(float* brow, const RBArgs& a, int h, int q0, int s0) {
    if (threadIdx.x < 128) {
        const int i = threadIdx.x;
        const long long d = (long long)s0 - q0 + (i - 63) + (a.T - 1);
        float val = 0.f;
        if (a.table && i < 127 && d >= 0 && d < (long long)a.T + a.S - 1) {
            const int n = min(max(a.bucket_of[d], 0), a.NB - 1);
            val = a.table[(size_t)n * a.H + h];
        }
        brow[i] = val;
    }
}

__device__ __forceinline__ int rb_key_tiles(int causal, int q0, int T, int S) {
    return causal ? (min(q0 + RB_TILE, T) + RB_TILE - 1) / RB_TILE : (S + RB_TILE - 1) / RB_TILE;
}

// p = exp(s - lse) in the backward, with the integer part c of lse log2(e) applied as an exact power of two:
//   p = exp2(fma(s, log2(e), -r)) 2^-c,   r = fma(lse, log2(e), -c)  (|r| <= 1/2, one rounding).
// The exp2 argument stays as small as the score is.  Formed directly, (s - lse) log2(e) is a number of the size of lse -- about
// -log2(S) on every key of a flat row -- and each p would carry the two roundings of a number of that size (fp32, 70 keys: 3 times
// the error of softmax's own exp(s - max) / sum).  |c| > 64 (scores near +-44: their own rounding dominates): the direct fma form.
struct RBRowExp { float r, sc; };
__device__ __forceinline__ RBRowExp rb_row_exp(float lse) {
    float c = rintf(lse * LOG2E);
    c = fabsf(c) <= 64.f ? c : 0.f;
    RBRowExp e;
    e.r = fmaf(lse, LOG2E, -c);
    e.sc = __builtin_bit_cast(float, (uint32_t)(127 - (int)c) << 23);
    return e;
}
__device__ __forceinline__ float rb_exp(float s, float r, float sc) { return __builtin_amdgcn_exp2f(fmaf(s, LOG2E, -r)) * sc; }

__device__ __forceinline__ void rb_wave_order() {
    // wave-private LDS rows: the LDS operations of one wave execute in order; this only stops the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <typename T, int D> __global__ __launch_bounds__(256) void rb_fwd_kernel(RBArgs a) {
    typedef XC<T, D, 4> C;
    typedef Img<T, C> IM;
    typedef typename Elem<T>::v8 v8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* Kimg = (T*)smem;
    T* Vimg = Kimg + IM::SIZE;
    float* brow = (float*)(Vimg + IM::SIZE);          // [128]
    uint8_t* vld = (uint8_t*)(brow + 128);            // [64]

    const int qblk = blockIdx.x % a.nqb, bh = blockIdx.x / a.nqb, h = bh % a.H, b = bh / a.H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, x = lane & 15, g = lane >> 4;
    const int q0 = qblk * RB_TILE, t = q0 + wave * 16 + x;
    const size_t HD = (size_t)a.H * D;
    const T* qb = (const T*)a.q + (size_t)b * a.T * a.ldq + (size_t)h * D;
    const T* kb = (const T*)a.k + (size_t)b * a.S * a.ldkv + (size_t)h * D;
    const T* vb = (const T*)a.v + (size_t)b * a.S * a.ldkv + (size_t)h * D;
    const uint8_t* kv = a.key_valid ? a.key_valid + (size_t)b * a.S : nullptr;
    const uint32_t thr = rb_thr(a.p_drop);
    const float inv_keep = 1.f / (1.f - a.p_drop);
    const uint64_t rowbase = (((uint64_t)b * a.H + h) * a.T + (uint64_t)min(t, a.T - 1)) * (uint64_t)a.S;

    v8 qf[C::NDC];
#pragma unroll
    for (int dc = 0; dc < C::NDC; ++dc) qf[dc] = load_qfrag<T, C>(qb, t, a.T, (size_t)a.ldq, dc * 32 + g * 8);
    float m = -INFINITY, l = 0.f;
    f32x4 oacc[C::NDB];
#pragma unroll
    for (int db = 0; db < C::NDB; ++db) oacc[db] = vzero<f32x4>();

    const int nkt = rb_key_tiles(a.causal, q0, a.T, a.S);
    for (int j = 0; j < nkt; ++j) {
        const int s0 = j * RB_TILE;
        __syncthreads();
        IM::stage(Kimg, kb + (size_t)s0 * a.ldkv, a.ldkv, a.S - s0);
        IM::stage(Vimg, vb + (size_t)s0 * a.ldkv, a.ldkv, a.S - s0);
        if (threadIdx.x < RB_TILE) {
            const int s = s0 + (int)threadIdx.x;
            vld[threadIdx.x] = (s < a.S && (!kv || kv[s])) ? 1 : 0;
        }
        rb_stage_brow(brow, a, h, q0, s0);
        __syncthreads();

        f32x4 sc[4];
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kk = sb * 16 + g * 4 + r;
                const bool ok = vld[kk] && (!a.causal || s0 + kk <= t);
                sc[sb][r] = ok ? brow[kk - (wave * 16 + x) + 63] : -INFINITY;
            }
#pragma unroll
            for (int dc = 0; dc < C::NDC; ++dc) mma16(sc[sb], IM::row(Kimg, sb, dc, lane), qf[dc]);
        }
        float tm = -INFINITY;
#pragma unroll
        for (int sb = 0; sb < 4; ++sb)
#pragma unroll
            for (int r = 0; r < 4; ++r) tm = fmaxf(tm, sc[sb][r]);
        tm = xg_max(tm);
        const float mn = fmaxf(m, tm);
        const float mu = (mn == -INFINITY) ? 0.f : mn;                    // no allowed key so far: every p stays 0
        const float alpha = __builtin_amdgcn_exp2f((m - mu) * LOG2E);      // m = -inf -> 0; maximum unchanged -> exactly 1
        m = mn;
        float ps = 0.f;
#pragma unroll
        for (int sb = 0; sb < 4; ++sb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f((sc[sb][r] - mu) * LOG2E);
                ps += p;
                sc[sb][r] = p;
            }
        l = l * alpha + ps;
        if (a.p_drop > 0.f) {
#pragma unroll
            for (int sb = 0; sb < 4; ++sb)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    sc[sb][r] *= mmgl_hash32(a.seed, rowbase + (uint64_t)(s0 + sb * 16 + g * 4 + r)) < thr ? 0.f : inv_keep;
        }
        v8 pf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) pf[ks] = pack8<T>(sc[2 * ks], sc[2 * ks + 1]);
#pragma unroll
        for (int db = 0; db < C::NDB; ++db) {
            oacc[db] *= alpha;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) mma16(oacc[db], IM::tr(Vimg, db, ks, lane), pf[ks]);
        }
    }
    const float lt = xg_sum(l);
    const float inv = lt > 0.f ? 1.f / lt : 0.f;                           // a row without an allowed key: zeros
    if (t < a.T) {
        T* o = (T*)a.out + ((size_t)b * a.T + t) * HD + (size_t)h * D + g * 4;
#pragma unroll
        for (int db = 0; db < C::NDB; ++db) store4<T>(o + db * 16, oacc[db] * inv);
        if (g == 0) a.lse[(size_t)bh * a.T + t] = lt > 0.f ? m + __logf(lt) : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- delta = rowsum(dO * O)
template <typename T, int D>
__global__ __launch_bounds__(256) void rb_rowdot_kernel(const T* __restrict__ dout, const T* __restrict__ out, float* __restrict__ delta,
                                                        int B, int H, int T_) {
    const size_t total = (size_t)B * T_ * H;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        typedef typename Elem<T>::v8 v8;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < D / 8; ++c) {
            const v8 x = *(const v8*)(dout + i * D + c * 8), y = *(const v8*)(out + i * D + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += (float)x[e] * (float)y[e];
        }
        const int h = (int)(i % H);
        const size_t bt = i / H;
        const int t = (int)(bt % T_), b = (int)(bt / T_);
        delta[((size_t)b * H + h) * T_ + t] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------- backward: dQ, row sums
template <typename T, int D> __global__ __launch_bounds__(256) void rb_bwd_dq_kernel(RBArgs a) {
    typedef XC<T, D, 4> C;
    typedef Img<T, C> IM;
    typedef typename Elem<T>::v8 v8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* Kimg = (T*)smem;
    T* Vimg = Kimg + IM::SIZE;
    float* brow = (float*)(Vimg + IM::SIZE);          // [128]
    uint8_t* vld = (uint8_t*)(brow + 128);            // [64]

    const int qblk = blockIdx.x % a.nqb, bh = blockIdx.x / a.nqb, h = bh % a.H, b = bh / a.H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, x = lane & 15, g = lane >> 4;
    const int q0 = qblk * RB_TILE, t = q0 + wave * 16 + x;
    const size_t HD = (size_t)a.H * D;
    const T* qb = (const T*)a.q + (size_t)b * a.T * a.ldq + (size_t)h * D;
    const T* gb = (const T*)a.dout + (size_t)b * a.T * HD + (size_t)h * D;
    const T* kb = (const T*)a.k + (size_t)b * a.S * a.ldkv + (size_t)h * D;
    const T* vb = (const T*)a.v + (size_t)b * a.S * a.ldkv + (size_t)h * D;
    const uint8_t* kv = a.key_valid ? a.key_valid + (size_t)b * a.S : nullptr;
    const uint32_t thr = rb_thr(a.p_drop);
    const float inv_keep = 1.f / (1.f - a.p_drop);
    const bool tin = t < a.T;
    const uint64_t rowbase = (((uint64_t)b * a.H + h) * a.T + (uint64_t)min(t, a.T - 1)) * (uint64_t)a.S;

    v8 qf[C::NDC], gf[C::NDC];
#pragma unroll
    for (int dc = 0; dc < C::NDC; ++dc) {
        qf[dc] = load_qfrag<T, C>(qb, t, a.T, (size_t)a.ldq, dc * 32 + g * 8);
        gf[dc] = load_qfrag<T, C>(gb, t, a.T, HD, dc * 32 + g * 8);
    }
    const RBRowExp rex = rb_row_exp(tin ? a.lse[(size_t)bh * a.T + t] : 0.f);
    const float dlt = tin ? a.delta[(size_t)bh * a.T + t] : 0.f;
    f32x4 acc[C::NDB];
#pragma unroll
    for (int db = 0; db < C::NDB; ++db) acc[db] = vzero<f32x4>();
    float lsum = 0.f;

    const int nkt = rb_key_tiles(a.causal, q0, a.T, a.S);
    for (int j = 0; j < nkt; ++j) {
        const int s0 = j * RB_TILE;
        __syncthreads();
        IM::stage(Kimg, kb + (size_t)s0 * a.ldkv, a.ldkv, a.S - s0);
        IM::stage(Vimg, vb + (size_t)s0 * a.ldkv, a.ldkv, a.S - s0);
        if (threadIdx.x < RB_TILE) {
            const int s = s0 + (int)threadIdx.x;
            vld[threadIdx.x] = (s < a.S && (!kv || kv[s])) ? 1 : 0;
        }
        rb_stage_brow(brow, a, h, q0, s0);
        __syncthreads();

        f32x4 ds[4];
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
            f32x4 sa, pa = vzero<f32x4>();
            bool ok[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kk = sb * 16 + g * 4 + r;
                ok[r] = tin && vld[kk] && (!a.causal || s0 + kk <= t);
                sa[r] = brow[kk - (wave * 16 + x) + 63];
            }
#pragma unroll
            for (int dc = 0; dc < C::NDC; ++dc) {
                mma16(sa, IM::row(Kimg, sb, dc, lane), qf[dc]);
                mma16(pa, IM::row(Vimg, sb, dc, lane), gf[dc]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = ok[r] ? rb_exp(sa[r], rex.r, rex.sc) : 0.f;
                lsum += p;
                float ks = 1.f;
                if (a.p_drop > 0.f) ks = mmgl_hash32(a.seed, rowbase + (uint64_t)(s0 + sb * 16 + g * 4 + r)) < thr ? 0.f : inv_keep;
                ds[sb][r] = p * (ks * pa[r] - dlt);
            }
        }
        v8 dsf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) dsf[ks] = pack8<T>(ds[2 * ks], ds[2 * ks + 1]);
#pragma unroll
        for (int db = 0; db < C::NDB; ++db)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) mma16(acc[db], IM::tr(Kimg, db, ks, lane), dsf[ks]);
    }
    // exp(s - lse) sums to 1 only up to the rounding of the one fp32 number lse is (half an ulp of a number of the size of log S,
    // plus the logarithm's own error: the same relative error on every p of the row).  The row's own sum takes it out again: dQ is
    // linear in p, so it is scaled once here, and the dK/dV kernel reads the factor per row.
    const float L = xg_sum(lsum);
    const float inv = L > 0.f ? 1.f / L : 0.f;
    if (tin) {
        T* o = (T*)a.dq + ((size_t)b * a.T + t) * HD + (size_t)h * D + g * 4;
#pragma unroll
        for (int db = 0; db < C::NDB; ++db) store4<T>(o + db * 16, acc[db] * inv);
        if (g == 0) a.corr[(size_t)bh * a.T + t] = inv;
    }
}

// ---------------------------------------------------------------------------------------------------------------- backward: dK, dV
// Non-swapped products: lane = key column, acc[r] = S[query 4g + r][key x]; P and dS are the B operands of the contractions over t,
// dO^T and Q^T the transposed fragments of the staged query tile.
template <typename T, int D> __global__ __launch_bounds__(256) void rb_bwd_dkv_kernel(RBArgs a) {
    typedef XC<T, D, 4> C;
    typedef Img<T, C> IM;
    typedef typename Elem<T>::v8 v8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* Qimg = (T*)smem;
    T* Gimg = Qimg + IM::SIZE;
    float* brow = (float*)(Gimg + IM::SIZE);          // [128]
    float* rex_r = brow + 128;                        // [64] rb_row_exp of the tile's query rows
    float* rex_sc = rex_r + 64;                       // [64]
    float* dlt_s = rex_sc + 64;                       // [64]
    float* bins = dlt_s + 64;                         // [4 waves][4 groups][RB_BINS] diagonal sums of the tile

    const int nkb = (a.S + RB_TILE - 1) / RB_TILE;
    const int kblk = blockIdx.x % nkb, bh = blockIdx.x / nkb, h = bh % a.H, b = bh / a.H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, x = lane & 15, g = lane >> 4;
    const int k0 = kblk * RB_TILE, s = k0 + wave * 16 + x;
    const size_t HD = (size_t)a.H * D;
    const T* qb = (const T*)a.q + (size_t)b * a.T * a.ldq + (size_t)h * D;
    const T* gb = (const T*)a.dout + (size_t)b * a.T * HD + (size_t)h * D;
    const T* kb = (const T*)a.k + (size_t)b * a.S * a.ldkv + (size_t)h * D;
    const T* vb = (const T*)a.v + (size_t)b * a.S * a.ldkv + (size_t)h * D;
    const uint32_t thr = rb_thr(a.p_drop);
    const float inv_keep = 1.f / (1.f - a.p_drop);
    const bool kok = s < a.S && (!a.key_valid || a.key_valid[(size_t)b * a.S + s]);
    const uint64_t headbase = ((uint64_t)b * a.H + h) * (uint64_t)a.T;
    const bool has_bias = a.table != nullptr;
    float* mybin = bins + (wave * 4 + g) * RB_BINS;

    v8 kf[C::NDC], vf[C::NDC];
#pragma unroll
    for (int dc = 0; dc < C::NDC; ++dc) {
        kf[dc] = load_qfrag<T, C>(kb, s, a.S, (size_t)a.ldkv, dc * 32 + g * 8);
        vf[dc] = load_qfrag<T, C>(vb, s, a.S, (size_t)a.ldkv, dc * 32 + g * 8);
    }
    f32x4 dka[C::NDB], dva[C::NDB];
#pragma unroll
    for (int db = 0; db < C::NDB; ++db) { dka[db] = vzero<f32x4>(); dva[db] = vzero<f32x4>(); }

    for (int t0 = a.causal ? k0 : 0; t0 < a.T; t0 += RB_TILE) {            // causal: T == S, the rows before k0 see none of these keys
        __syncthreads();
        IM::stage(Qimg, qb + (size_t)t0 * a.ldq, a.ldq, a.T - t0);
        IM::stage(Gimg, gb + (size_t)t0 * HD, (int)HD, a.T - t0);
        if (threadIdx.x < RB_TILE) {
            const int tt = t0 + (int)threadIdx.x;
            const RBRowExp e = rb_row_exp(tt < a.T ? a.lse[(size_t)bh * a.T + tt] : 0.f);
            rex_r[threadIdx.x] = e.r;
            rex_sc[threadIdx.x] = tt < a.T ? e.sc * a.corr[(size_t)bh * a.T + tt] : 0.f;
            dlt_s[threadIdx.x] = tt < a.T ? a.delta[(size_t)bh * a.T + tt] : 0.f;
        }
        rb_stage_brow(brow, a, h, t0, k0);
        for (int i = lane; i < 4 * RB_BINS; i += 64) bins[wave * 4 * RB_BINS + i] = 0.f;
        __syncthreads();

        f32x4 pr[4], dsr[4];
#pragma unroll
        for (int qs = 0; qs < 4; ++qs) {
            f32x4 sa, pa = vzero<f32x4>();
#pragma unroll
            for (int r = 0; r < 4; ++r) sa[r] = brow[(wave * 16 + x) - (qs * 16 + g * 4 + r) + 63];
#pragma unroll
            for (int dc = 0; dc < C::NDC; ++dc) {
                mma16(sa, IM::row(Qimg, qs, dc, lane), kf[dc]);
                mma16(pa, IM::row(Gimg, qs, dc, lane), vf[dc]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ql = qs * 16 + g * 4 + r, tq = t0 + ql;
                const bool ok = kok && tq < a.T && (!a.causal || s <= tq);
                const float p = ok ? rb_exp(sa[r], rex_r[ql], rex_sc[ql]) : 0.f;
                float ks = 1.f;
                if (a.p_drop > 0.f)
                    ks = mmgl_hash32(a.seed, (headbase + (uint64_t)min(tq, a.T - 1)) * (uint64_t)a.S + (uint64_t)min(s, a.S - 1)) < thr ? 0.f : inv_keep;
                pr[qs][r] = p * ks;
                dsr[qs][r] = p * (ks * pa[r] - dlt_s[ql]);
            }
        }
        v8 pB[2], dsB[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            pB[ks] = pack8<T>(pr[2 * ks], pr[2 * ks + 1]);
            dsB[ks] = pack8<T>(dsr[2 * ks], dsr[2 * ks + 1]);
        }
#pragma unroll
        for (int db = 0; db < C::NDB; ++db)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                mma16(dva[db], IM::tr(Gimg, db, ks, lane), pB[ks]);
                mma16(dka[db], IM::tr(Qimg, db, ks, lane), dsB[ks]);
            }

        if (has_bias) {                                // (workgroup-uniform) dtable: the tile's dS summed along its diagonals
#pragma unroll
            for (int qs = 0; qs < 4; ++qs)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    mybin[x - (qs * 16 + g * 4 + r) + 63] += dsr[qs][r];
                    rb_wave_order();
                }
            __syncthreads();
            if (threadIdx.x < 128) {
                const int i = threadIdx.x;             // diagonal of the tile: key - query + 63 (both local)
                float sum = 0.f;
                if (i < 127) {
                    for (int w = 0; w < 4; ++w) {
                        const int d = i - 16 * w;      // the wave's own diagonal index: x - query + 63
                        if (d >= 0 && d < 79)
                            for (int gg = 0; gg < 4; ++gg) sum += bins[(w * 4 + gg) * RB_BINS + d];
                    }
                }
                a.part[(((size_t)bh * a.nqb + t0 / RB_TILE) * a.nkt + kblk) * 128 + i] = sum;
            }
        }
    }
    if (s < a.S) {
        const size_t off = ((size_t)b * a.S + s) * HD + (size_t)h * D + g * 4;
#pragma unroll
        for (int db = 0; db < C::NDB; ++db) {
            store4<T>((T*)a.dk + off + db * 16, dka[db]);
            store4<T>((T*)a.dv + off + db * 16, dva[db]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- dtable folds
// diag[h, d] = sum over b, query block, key tile (index order) of the tile rows' entry for diagonal d = s - t + T - 1
__global__ __launch_bounds__(256) void rb_diag_kernel(const float* __restrict__ part, float* __restrict__ diag, int B, int H, int T, int S,
                                                      int nqb, int nktmax, int causal) {
    const int nd = T + S - 1;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * nd) return;
    const int h = i / nd, rel = i % nd - (T - 1);
    float acc = 0.f;
    for (int b = 0; b < B; ++b)
        for (int qblk = 0; qblk < nqb; ++qblk) {
            const int nkt = rb_key_tiles(causal, qblk * RB_TILE, T, S);
            const int u = rel + 63 + RB_TILE * qblk;                       // = 64 j + i_local
            const int j = u >= 0 ? u / RB_TILE : -((-u + RB_TILE - 1) / RB_TILE);
            const int il = u - RB_TILE * j;                                // 0..63; tile j - 1 holds the diagonal at il + 64 (<= 126)
            const size_t row = ((size_t)(b * H + h) * nqb + qblk) * nktmax;
            if (il <= 62 && j - 1 >= 0 && j - 1 < nkt) acc += part[(row + j - 1) * 128 + il + 64];
            if (j >= 0 && j < nkt) acc += part[(row + j) * 128 + il];
        }
    diag[i] = acc;
}

// dtable[n, h] = sum over the diagonals d with bucket_of[d] == n, in index order
__global__ __launch_bounds__(64) void rb_bucket_kernel(const float* __restrict__ diag, const int32_t* __restrict__ bucket_of,
                                                       float* __restrict__ dtable, int NB, int H, int nd) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= NB * H) return;
    const int n = i / H, h = i % H;
    float acc = 0.f;
    for (int d = 0; d < nd; ++d)
        if (min(max(bucket_of[d], 0), NB - 1) == n) acc += diag[(size_t)h * nd + d];
    dtable[i] = acc;
}

int rb_check(const char* who, int B, int H, int T, int S, int D, int NB, int ldq, int ldkv, int causal, float p, int dtype, bool has_table) {
    MMGL_CHECK_ARG(B > 0 && H > 0 && T > 0 && S > 0 && D > 0, "%s: bad sizes B=%d H=%d T=%d S=%d D=%d", who, B, H, T, S, D);
    MMGL_CHECK_ARG(dtype == MMGL_F32 || dtype == MMGL_BF16, "%s: dtype must be MMGL_F32 or MMGL_BF16", who);
    if (D != 64) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: head_dim %d not supported (T5's d_kv = 64 only)", who, D);
    if (causal && T != S) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: causal attention needs S == T (got %d, %d)", who, S, T);
    MMGL_CHECK_ARG(p >= 0.f && p < 1.f, "%s: dropout probability %g outside [0, 1)", who, (double)p);
    MMGL_CHECK_ARG(ldq >= H * D && ldkv >= H * D && ldq % 8 == 0 && ldkv % 8 == 0,
                   "%s: row pitches (%d, %d) must be >= H*D = %d and multiples of 8 elements", who, ldq, ldkv, H * D);
    MMGL_CHECK_ARG(!has_table || NB > 0, "%s: num_buckets must be positive (got %d)", who, NB);
    MMGL_CHECK_ARG((long long)B * H * (cdiv(T, RB_TILE) > cdiv(S, RB_TILE) ? cdiv(T, RB_TILE) : cdiv(S, RB_TILE)) < (1ll << 31),
                   "%s: too many workgroups", who);
    return MMGL_OK;
}

template <typename T> constexpr size_t rb_lds(int extra_floats, int extra_bytes) {
    return 2 * sizeof(T) * Img<T, XC<T, 64, 4>>::SIZE + sizeof(float) * (128 + extra_floats) + extra_bytes;
}

struct RBWorkspace {
    size_t delta, part, diag, total;
    RBWorkspace(int B, int H, int T, int S) {
        delta = align_up((size_t)B * H * T * sizeof(float), 256);
        part = align_up((size_t)B * H * cdiv(T, RB_TILE) * cdiv(S, RB_TILE) * 128 * sizeof(float), 256);
        diag = align_up((size_t)H * ((size_t)T + S - 1) * sizeof(float), 256);
        total = 2 * delta + part + diag;
    }
};

template <typename T> int rb_fwd_launch(const RBArgs& a, hipStream_t st) {
    const size_t lds = rb_lds<T>(0, RB_TILE);
    if (int rc = mmgl_set_lds(rb_fwd_kernel<T, 64>, lds, "attn_relbias_fwd")) return rc;
    hipLaunchKernelGGL((rb_fwd_kernel<T, 64>), dim3(a.B * a.H * a.nqb), dim3(256), lds, st, a);
    MMGL_CHECK_LAUNCH("attn_relbias_fwd");
    return MMGL_OK;
}

template <typename T> int rb_bwd_launch(const RBArgs& a, float* diag, float* dtable, hipStream_t st) {
    const size_t rows = (size_t)a.B * a.T * a.H;
    hipLaunchKernelGGL((rb_rowdot_kernel<T, 64>), dim3((unsigned)((rows + 255) / 256 > 4096 ? 4096 : (rows + 255) / 256)), dim3(256), 0, st,
                       (const T*)a.dout, (const T*)a.out, a.delta, a.B, a.H, a.T);
    const size_t lds1 = rb_lds<T>(0, RB_TILE), lds2 = rb_lds<T>(192 + 16 * RB_BINS, 0);
    if (int rc = mmgl_set_lds(rb_bwd_dq_kernel<T, 64>, lds1, "attn_relbias_bwd")) return rc;
    if (int rc = mmgl_set_lds(rb_bwd_dkv_kernel<T, 64>, lds2, "attn_relbias_bwd")) return rc;
    hipLaunchKernelGGL((rb_bwd_dq_kernel<T, 64>), dim3(a.B * a.H * a.nqb), dim3(256), lds1, st, a);
    hipLaunchKernelGGL((rb_bwd_dkv_kernel<T, 64>), dim3(a.B * a.H * a.nkt), dim3(256), lds2, st, a);
    if (a.table) {
        const int nd = a.T + a.S - 1;
        hipLaunchKernelGGL(rb_diag_kernel, dim3(cdiv(a.H * nd, 256)), dim3(256), 0, st, (const float*)a.part, diag, a.B, a.H, a.T, a.S, a.nqb,
                           a.nkt, a.causal);
        hipLaunchKernelGGL(rb_bucket_kernel, dim3(cdiv(a.NB * a.H, 64)), dim3(64), 0, st, (const float*)diag, a.bucket_of, dtable, a.NB, a.H, nd);
    }
    MMGL_CHECK_LAUNCH("attn_relbias_bwd");
    return MMGL_OK;
}

}  // namespace

extern "C" int mmgl_attn_relbias_fwd(const void* q, const void* k, const void* v, const uint8_t* key_valid, const float* table,
                                     const int32_t* bucket_of, void* out, float* lse, int B, int H, int T, int S, int D, int num_buckets,
                                     int ldq, int ldkv, int causal, float p_drop, uint64_t seed, int dtype, void* stream) {
    if (int rc = rb_check("mmgl_attn_relbias_fwd", B, H, T, S, D, num_buckets, ldq, ldkv, causal, p_drop, dtype, table != nullptr)) return rc;
    MMGL_CHECK_ARG(q && k && v && out && lse && (!table || bucket_of), "mmgl_attn_relbias_fwd: null pointer");
    RBArgs a{};
    a.q = q; a.k = k; a.v = v; a.key_valid = key_valid; a.table = table; a.bucket_of = bucket_of; a.out = out; a.lse = lse;
    a.B = B; a.H = H; a.T = T; a.S = S; a.ldq = ldq; a.ldkv = ldkv; a.NB = num_buckets; a.causal = causal;
    a.nqb = cdiv(T, RB_TILE); a.nkt = cdiv(S, RB_TILE); a.p_drop = p_drop; a.seed = seed;
    return dtype == MMGL_BF16 ? rb_fwd_launch<bf16>(a, (hipStream_t)stream) : rb_fwd_launch<float>(a, (hipStream_t)stream);
}

extern "C" size_t mmgl_attn_relbias_bwd_workspace(int B, int H, int T, int S) {
    if (B <= 0 || H <= 0 || T <= 0 || S <= 0) return 0;
    return RBWorkspace(B, H, T, S).total;
}

extern "C" int mmgl_attn_relbias_bwd(const void* dout, const void* q, const void* k, const void* v, const void* out, const float* lse,
                                     const uint8_t* key_valid, const float* table, const int32_t* bucket_of, void* dq, void* dk, void* dv,
                                     float* dtable, void* workspace, size_t workspace_bytes, int B, int H, int T, int S, int D,
                                     int num_buckets, int ldq, int ldkv, int causal, float p_drop, uint64_t seed, int dtype, void* stream) {
    if (int rc = rb_check("mmgl_attn_relbias_bwd", B, H, T, S, D, num_buckets, ldq, ldkv, causal, p_drop, dtype, table != nullptr)) return rc;
    MMGL_CHECK_ARG(dout && q && k && v && out && lse && dq && dk && dv && workspace && (!table || (bucket_of && dtable)),
                   "mmgl_attn_relbias_bwd: null pointer");
    const RBWorkspace ws(B, H, T, S);
    MMGL_CHECK_ARG(workspace_bytes >= ws.total, "mmgl_attn_relbias_bwd: workspace too small");
    MMGL_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "mmgl_attn_relbias_bwd: workspace must be 16-byte aligned");
    RBArgs a{};
    a.q = q; a.k = k; a.v = v; a.dout = dout; a.key_valid = key_valid; a.table = table; a.bucket_of = bucket_of; a.out = (void*)out;
    a.lse = (float*)lse; a.delta = (float*)workspace; a.corr = (float*)((char*)workspace + ws.delta); a.part = (float*)((char*)workspace + 2 * ws.delta);
    a.dq = dq; a.dk = dk; a.dv = dv;
    a.B = B; a.H = H; a.T = T; a.S = S; a.ldq = ldq; a.ldkv = ldkv; a.NB = num_buckets; a.causal = causal;
    a.nqb = cdiv(T, RB_TILE); a.nkt = cdiv(S, RB_TILE); a.p_drop = p_drop; a.seed = seed;
    float* diag = (float*)((char*)workspace + 2 * ws.delta + ws.part);
    return dtype == MMGL_BF16 ? rb_bwd_launch<bf16>(a, diag, dtable, (hipStream_t)stream) : rb_bwd_launch<float>(a, diag, dtable, (hipStream_t)stream);
}
