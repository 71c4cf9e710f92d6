// Flash attention for gfx950 on v_mfma_f32_32x32x16_bf16: the bf16, head_dim 64 / 128 kernels behind mmgl_selfattn_fwd /
// mmgl_selfattn_prefix_fwd (causal self-attention of the frozen decoder layers, reference model/modelling_cross_attention.py:
// 203-271 with the masks of :51-79, 455-476) and mmgl_encattn_fwd (packed bidirectional attention of the frozen neighbor
// encoders, :978-1027).  selfattn.hip keeps the fp32 / small-head_dim kernels and the C ABI entry points.
//
// Why this kernel exists.  At the OPT-1.3B shape (B = 64, H = 32, T = 640, D = 64) Q, K, V and O are 671 MB per call: 112 us at
// 6 TB/s, against 43 us of MFMA time -- the forward pass is HBM-bound once its inner loop stops being VALU-bound.  The 16x16 kernel
// it replaces issued ~560 instructions per 64-key tile and wave (32 MFMAs among them) and ran at 300 us.  Here:
//   * workgroup = 4 waves = 128 query rows of one (batch, head); wave = 32 rows; 2-3 workgroups per CU (12 / 8 waves), so a SIMD
//     always has one wave in its MFMAs while another does softmax arithmetic, without a hand-built ping-pong.
//   * swapped products on 32x32x16 MFMAs: S^T = K Q^T (A = K rows from LDS, B = Q^T from registers), O^T += V^T P^T.  A lane owns
//     ONE query row (two lanes per row: hi = lane >> 5 splits the keys 4-by-4), so row max / sum are in-lane chains plus one
//     v_permlane32_swap, and the S^T accumulator layout IS the B-operand layout of the second product: P never leaves its lane.
//   * K / V tiles (64 keys) travel global -> LDS by LDS-DMA (buffer_load ... lds, 1 KiB pieces, whole rows per 8 / 16 lanes: fully
//     coalesced) into a ring of NS slots, one s_barrier per tile, counted vmcnt (the next tile stays in flight across the barrier).
//     No register staging, no ds_write.  The 16-byte slot of a row is XOR-swizzled on the SOURCE side (the DMA destination is
//     lane-linear): K rows so that the ds_read_b128 A-fragment reads are bank-conflict free, V rows so that the four key rows a
//     ds_read_b64_tr_b16 touches per 32 lanes fall into four different 64-byte bank quarters.
//   * masks cost nothing on ordinary tiles: a 64-bit key-valid word per tile (built once per workgroup in LDS) classifies a tile as
//     all-valid (no masking code runs), all-masked (the tile is SKIPPED: exp(-inf) = 0 exactly, so the result is unchanged -- the
//     padded middle of a WikiWeb2M sequence, wikiweb2m/data.py:321-333, is 30 % of the keys) or mixed (per-element select, rare);
//     the causal select runs only on the 32-key blocks the diagonal touches.
//   * online softmax in the log2 domain with a deferred rescale: O and l are rescaled only when some row's maximum grew by more
//     than 2^8 since the last rescale (P <= 256 then: bf16 keeps its 8 relative bits, l and O accumulate in fp32), a wave-uniform
//     branch that is almost never taken after the first tiles.
#include "attn_common.h"
#include "selfattn32.h"
#include <type_traits>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void lds_void;

#define SA32_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define SA32_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#ifndef SA32_THR
#define SA32_THR 8.0f             // deferred rescale threshold (log2 units)
#endif
#ifndef SA32_NS64
#define SA32_NS64 2               // ring slots at head_dim 64 (3: two tiles in flight, 3 workgroups per CU; 2: one tile, 4 workgroups)
#endif
#ifndef SA32_NS_DQ
#define SA32_NS_DQ 2              // ring slots of the dQ kernel (K / V tiles)
#endif
#ifndef SA32_NS_DKV
#define SA32_NS_DKV 2             // ring slots of the dK / dV kernel (Q / dO tiles + row statistics)
#endif
#ifndef SA32_NS_DKV128
#define SA32_NS_DKV128 2          // ... at head_dim 128 (one workgroup per CU: up to 4 slots of 33 KiB fit)
#endif
#ifndef SA32_DKV_OCC64
#define SA32_DKV_OCC64 2          // workgroups per CU the dK / dV kernel at head_dim 64 is compiled for (176 registers: two per CU).  3 = a
                                  // 168-register budget (9 spilled): backward 603 -> 668 us at B = 64, T = 640 (round 5): more waves, slower
#endif
#ifndef SA32_DQ_OCC
#define SA32_DQ_OCC 2             // ... and the dQ kernel
#endif
#ifndef SA32_TRACE
#define SA32_TRACE 0              // timing experiments only: wall-clock stamps of every workgroup of the forward kernel (MMGL_SA32_TRACE = device pointer)
#endif

template <int D> struct G32 {
    static constexpr int KT = 64;                     // keys per tile
    static constexpr int ROWB = D * 2;                // bytes per K / V row in LDS
    static constexpr int TILEB = KT * ROWB;           // one operand tile
    static constexpr int PIECES = TILEB / 1024;       // 1 KiB LDS-DMA pieces per operand tile
    static constexpr int RPP = 1024 / ROWB;           // rows per piece
    static constexpr int LPR = 64 / RPP;              // lanes per row of a piece (= 16-byte slots per row)
    static constexpr int NKS = D / 16;                // contraction steps of S^T = K Q^T
    static constexpr int NDB = D / 32;                // 32-channel blocks of O^T
    static constexpr int NS = (D == 64) ? SA32_NS64 : 2;      // ring slots (K tile + V tile each)
    static constexpr int SLOTB = 2 * TILEB;
    static constexpr int NP = 2 * PIECES / 4;         // LDS-DMA instructions per wave and tile
    static constexpr int MAXT = 64;                   // key tiles per sequence the valid-word table holds (4096 keys)
    static constexpr int LDS = NS * SLOTB + MAXT * 8;
    static constexpr int OCC = (D == 64) ? (SA32_NS64 == 3 ? 3 : 4) : 2;     // workgroups per CU the kernel is sized for
};
template <int D> __device__ __forceinline__ int swz_k(int row) { return D == 64 ? ((row >> 1) & 7) : (row & 15); }
template <int D> __device__ __forceinline__ int swz_v(int row) { return D == 64 ? (((row >> 1) & 1) << 2) : ((row & 3) << 2); }

struct SA32Args {
    const bf16 *q, *k, *v;
    const uint8_t* valid;      // [B, P + T] (batch mode) or null
    bf16* out;
    float* lse;                // [B, H, T] or null
    const int* cu;             // packed mode: sequence i owns rows cu[i] .. cu[i+1]-1; null = batch mode
    int B, H, T, P, nqb, ldq, ldk, ldo, q_rows;
    long long* trace;          // SA32_TRACE builds (timing experiments): 8 x int64 per workgroup
    int G;                     // grouped-query attention (GQA instantiations only): query head h reads key / value head h / G
    const int* tiles;          // TILES instantiations only: [B, T / 64] compact tile of key tile j, -1 = dead (no such rows in k / v)
    int ntc;                   // ... and the compact tiles in k / v ([64 ntc, ldk] rows for the whole batch)
};

__device__ __forceinline__ f32x16 mma32(const bf16x8& a, const bf16x8& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// key (within its 32-key block) of accumulator register r on a lane of half `hi`: (r & 3) + 8 (r >> 2) + 4 hi
__device__ __forceinline__ constexpr int kreg(int r) { return (r & 3) + 8 * (r >> 2); }

__device__ __forceinline__ void swap32_u32(uint32_t& a, uint32_t& b) {
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}

// TILES = true (live key tiles only): k / v hold the 64-key tiles that have a valid key and nothing else, [64 ntc, ldk] for the whole
// batch.  A lane keeps its sample's row of the tile table (lane j: compact tile of key tile j, at most 64 tiles per sequence), so a
// tile's base row is one v_readlane.  Masks, causal tests and valid words keep using j.  A dead tile that is requested all the same
// (the prologue's, before the mask is known) reads the sample's first live tile; every index is clamped to the buffer's tiles, as
// the scalar offset of a buffer access is outside the descriptor's range check.
struct TileRow {
    int tv, first, last;
    __device__ __forceinline__ void load(const int* tiles, int b, int ntl, int ntc, int lane) {
        const __amdgpu_buffer_rsrc_t rt = make_rsrc(tiles + (size_t)b * ntl, (uint32_t)ntl * 4u);
        const int t = (int)__builtin_amdgcn_raw_buffer_load_b32(rt, (uint32_t)lane * 4u, 0, 0);
        tv = lane < ntl ? t : -1;
        last = ntc - 1;
        const uint64_t lv = __builtin_amdgcn_ballot_w64(tv >= 0);
        first = lv != 0ull ? __builtin_amdgcn_readlane(tv, __builtin_ctzll(lv)) : 0;
        first = max(min(first, last), 0);
    }
    __device__ __forceinline__ int row(int j) const {                   // j wave-uniform, < 64
        const int t = __builtin_amdgcn_readlane(tv, j);
        return (t < 0 ? first : min(t, last)) * 64;
    }
};

// GQA = true: k, v [B, Tk, (H / G) * D], query head h reads key / value head h / a.G (HF's repeat_kv); nothing else differs, and the
// GQA = false instantiations are the multi-head kernels as they were
template <int D, bool CAUSAL, bool GQA = false, bool TILES = false>
__global__ __launch_bounds__(256, G32<D>::OCC) void sa32_fwd_kernel(SA32Args a) {
    typedef G32<D> G;
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int key = lane & 31, hi = lane >> 5;

#if SA32_TRACE
    const long long tr0 = wall_clock64();
#endif
    const int vid = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = vid / a.nqb;
    const int qblk = CAUSAL ? a.nqb - 1 - vid % a.nqb : vid % a.nqb;      // causal: longest (most key tiles) first
    const int b = bh / a.H, h = bh % a.H;
    TileRow tr{};
    if constexpr (TILES) tr.load(a.tiles, b, a.T / G::KT, a.ntc, lane);   // the oldest load of the prologue: the first K / V request waits for it alone
    int Tq, Tk;
    const bf16 *qb, *kb, *vb;
    bf16* ob;
    const uint8_t* valid_row = nullptr;
    if (a.cu) {
        const int start = a.cu[b], len = a.cu[b + 1] - start;
        Tq = min(len, a.q_rows);
        Tk = len;
        qb = a.q + (size_t)start * a.ldq + h * D;
        kb = a.k + (size_t)start * a.ldk + h * D;
        vb = a.v + (size_t)start * a.ldk + h * D;
        ob = a.out + (size_t)start * a.ldo + h * D;
    } else {
        Tq = a.T;
        Tk = a.T + a.P;
        const int hk = GQA ? h / a.G : h;
        qb = a.q + (size_t)b * a.T * a.ldq + h * D;
        kb = a.k + (TILES ? (size_t)0 : (size_t)b * Tk * a.ldk) + hk * D;
        vb = a.v + (TILES ? (size_t)0 : (size_t)b * Tk * a.ldk) + hk * D;
        ob = a.out + (size_t)b * a.T * a.ldo + h * D;
        if (a.valid) valid_row = a.valid + (size_t)b * Tk;
    }
    if (qblk * 128 >= Tq) return;                                       // workgroup-uniform, before any barrier
    const int t0 = qblk * 128 + wave * 32;
    const int nkt = CAUSAL ? (min(Tq, (qblk + 1) * 128) + a.P + G::KT - 1) / G::KT : (Tk + G::KT - 1) / G::KT;

    const uint32_t ldqB = (uint32_t)a.ldq * 2u, ldkB = (uint32_t)a.ldk * 2u, ldoB = (uint32_t)a.ldo * 2u;
    const __amdgpu_buffer_rsrc_t rq = make_rsrc(qb, (uint32_t)(Tq - 1) * ldqB + D * 2);
    const int kvrows = TILES ? a.ntc * G::KT : Tk;                      // rows behind the K / V descriptors
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(kb, (uint32_t)(kvrows - 1) * ldkB + D * 2);
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(vb, (uint32_t)(kvrows - 1) * ldkB + D * 2);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(ob, (uint32_t)(Tq - 1) * ldoB + D * 2);

    // ---- per-tile key-valid words (bit s of word j: key 64 j + s exists and is attendable).  The bytes of this wave's first four
    // tiles are only REQUESTED here (oldest loads of the prologue); they are turned into words after Q and the first K / V tiles
    // have been requested too, so that the three round trips overlap
    uint64_t* vbits = (uint64_t*)(smem + G::NS * G::SLOTB);
    const bool nomask = valid_row == nullptr;                           // branch-free: without a mask the descriptor is empty and reads as 0
    const __amdgpu_buffer_rsrc_t rvalid = make_rsrc(valid_row, nomask ? 0u : (uint32_t)Tk);
    uint8_t vraw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) vraw[i] = __builtin_amdgcn_raw_buffer_load_b8(rvalid, (uint32_t)((wave + 4 * i) * G::KT + lane), 0, 0);

    // ---- Q^T fragments (B operand of S^T = K Q^T): lane (row = lane & 31, hi) holds channels 16 ks + 8 hi .. + 7
    const int trow = t0 + key;
    bf16x8 qf[G::NKS];
#pragma unroll
    for (int ks = 0; ks < G::NKS; ++ks) qf[ks] = buf_load8<bf16>(rq, (uint32_t)trow * ldqB + (uint32_t)(16 * ks + 8 * hi) * 2u);

    // ---- LDS-DMA of K / V tile j into ring slot `slot`: wave w moves pieces w, w + 4, .. (RPP rows each) of both operands
    uint32_t kvoff, vvoff;
    {
        const int row = G::RPP * wave + lane / G::LPR, sl = lane % G::LPR;
        kvoff = (uint32_t)row * ldkB + (uint32_t)((sl ^ swz_k<D>(row)) << 4);
        vvoff = (uint32_t)row * ldkB + (uint32_t)((sl ^ swz_v<D>(row)) << 4);
    }
    auto issue = [&](int j, int slot) __attribute__((always_inline)) {
        char* base = smem + slot * G::SLOTB + wave * 1024;
        const int jrow = TILES ? tr.row(j) : j * G::KT;
#pragma unroll
        for (int i = 0; i < G::PIECES / 4; ++i) {
            const int soff = (int)((uint32_t)(jrow + i * 4 * G::RPP) * ldkB);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (lds_void*)(base + i * 4096), 16, kvoff, soff, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (lds_void*)(base + G::TILEB + i * 4096), 16, vvoff, soff, 0, 0);
        }
    };
    constexpr int PD = G::NS - 1;                                       // tiles in flight
#pragma unroll
    for (int j = 0; j < PD; ++j) issue(j, j);                           // unconditional (a tile past the last key reads as zeros): hipcc's vmcnt for Q stays exact
    constexpr bool EARLY = G::NS == 2;      // two-slot ring: tile 1 is requested in the prologue together with tile 0 (both slots are free then), not behind tile 0's barrier (+1 %)
    if (EARLY) issue(1, 1);

    // ---- fragment addresses (byte offsets inside a slot)
    // K row `key`, logical 16-byte slot 2 ks + hi, physical slot ^ swz_k(key): one lane base, the step as an XOR at the point of use
    const int lds0 = (int)(unsigned)(size_t)(lds_void*)smem;
    const int kbase = key * G::ROWB + (((hi ^ swz_k<D>(key)) & 1) << 4) + ((swz_k<D>(key) & ~1) << 4);
    // V^T via ds_read_b64_tr_b16: in its 16-lane group lane i points at key row (i >> 2), channels 4 (i & 3) .. + 3 of the group's
    // 16-channel block and receives channel i of the four rows.  Group gg = lane >> 4: channel block (gg & 1), key half hi = gg >> 1.
    int vbase;
    {
        const int i = lane & 15, gg = lane >> 4;
        const int row = 4 * (gg >> 1) + (i >> 2);
        vbase = lds0 + G::TILEB + row * G::ROWB + (((2 * (gg & 1) + ((i & 3) >> 1)) ^ swz_v<D>(row)) << 4) + 8 * (i & 1);
    }

    f32x16 o[G::NDB];
#pragma unroll
    for (int db = 0; db < G::NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
    float m2 = -INFINITY, lsum = 0.f;                                  // running row maximum (log2 units), this lane's share of the row sum

    // this wave's causal bounds: tiles above its diagonal are not computed (it still takes part in barriers and DMA)
    const bool wave_active = t0 < Tq;
    const int tl = t0 + 31 + a.P;                                       // last key any row of this wave may see
    const int jlast = !wave_active ? -1 : (CAUSAL ? min(nkt - 1, tl >> 6) : nkt - 1);

    auto body = [&](auto nb_tag, int j, uint32_t vlo, uint32_t vhi, bool mixed, int slot) __attribute__((always_inline)) {
        constexpr int NB = decltype(nb_tag)::value;
        const char* Ks = smem + slot * G::SLOTB;
        f32x16 s[NB];
#pragma unroll
        for (int blk = 0; blk < NB; ++blk)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[blk][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < G::NKS; ++ks)
#pragma unroll
            for (int blk = 0; blk < NB; ++blk) {
                const bf16x8 kf = *(const bf16x8*)(Ks + blk * 32 * G::ROWB + (kbase ^ (ks << 5)));
                s[blk] = mma32(kf, qf[ks], s[blk]);
            }
        // V^T fragments of ONE 32-channel block db: [blk][jj] = keys 32 blk + 16 jj + {4 hi + 0..3, 8 + 4 hi + 0..3}.  Two register sets:
        // block db + 1 is requested before block db's MFMAs (its LDS latency hides under them), block 0 before the softmax arithmetic.
        // The transpose reads are inline asm (behind the builtin hipcc drains the LDS-DMA prefetch with vmcnt(0) in front of each), so
        // the waits are ours too: counted lgkmcnt, naming every destination so that no consumer is scheduled above the wait.
        bf16x4 va[2][NB][2][2];
        const int vslot = vbase + slot * G::SLOTB;
        auto vreads = [&](int db, bf16x4 (&f)[NB][2][2]) __attribute__((always_inline)) {
            const int ad = vslot ^ (db << 6);
#pragma unroll
            for (int blk = 0; blk < NB; ++blk)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f[blk][jj][0]) : "v"(ad), "i"((32 * blk + 16 * jj) * G::ROWB));
                    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f[blk][jj][1]) : "v"(ad), "i"((32 * blk + 16 * jj + 8) * G::ROWB));
                }
        };
        vreads(0, va[0]);                                     // V^T fragments requested before the softmax arithmetic: their latency hides under it (+4 % otherwise)

        // ---- masks (wave-uniform branches: ordinary tiles run none of this)
        if (mixed) {
#pragma unroll
            for (int blk = 0; blk < NB; ++blk) {
                const uint32_t w = (blk ? vhi : vlo) >> (4 * hi);
#pragma unroll
                for (int r = 0; r < 16; ++r) s[blk][r] = ((w >> kreg(r)) & 1u) ? s[blk][r] : -INFINITY;
            }
        }
        if (CAUSAL) {
#pragma unroll
            for (int blk = 0; blk < NB; ++blk) {
                const int k0 = j * G::KT + 32 * blk;
                if (k0 + 31 > t0 + a.P) {                               // the diagonal crosses this block (wave-uniform)
                    const int c = trow + a.P - k0 - 4 * hi;             // key kreg(r) + 4 hi of the block is visible iff kreg(r) <= c
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[blk][r] = (kreg(r) <= c) ? s[blk][r] : -INFINITY;
                }
            }
        }
        // ---- online softmax (log2 domain), one query row per lane pair
        float tm = s[0][0];
#pragma unroll
        for (int blk = 0; blk < NB; ++blk)
#pragma unroll
            for (int r = 0; r < 16; ++r) tm = fmaxf(tm, s[blk][r]);
        {
            float lo, up;
            swap32(tm, lo, up);
            tm = fmaxf(lo, up);
        }
        const float tm2 = tm * LOG2E;
        if (__builtin_amdgcn_ballot_w64(tm2 > m2 + SA32_THR) != 0ull) {
            const float mn = fmaxf(m2, tm2);
            const float alpha = (mn == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f(m2 - mn);
            m2 = mn;
            lsum *= alpha;
#pragma unroll
            for (int db = 0; db < G::NDB; ++db) o[db] *= alpha;
        }
        const float nms = (m2 == -INFINITY) ? 0.f : -m2;
        float ps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int blk = 0; blk < NB; ++blk)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(fmaf(s[blk][r], LOG2E, nms));
                s[blk][r] = p;
                ps[r & 3] += p;
            }
        lsum += (ps[0] + ps[1]) + (ps[2] + ps[3]);
        bf16x8 pf[NB][2];
#pragma unroll
        for (int blk = 0; blk < NB; ++blk)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                f32x8 t;
#pragma unroll
                for (int e = 0; e < 8; ++e) t[e] = s[blk][8 * jj + e];
                pf[blk][jj] = __builtin_convertvector(t, bf16x8);
            }
#pragma unroll
        for (int db = 0; db < G::NDB; ++db) {
            bf16x4 (&f)[NB][2][2] = va[db & 1];
            if (db + 1 < G::NDB) {
                vreads(db + 1, va[(db + 1) & 1]);
                if (NB == 2) asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(f[0][0][0]), "+v"(f[0][0][1]), "+v"(f[0][1][0]), "+v"(f[0][1][1]), "+v"(f[1][0][0]), "+v"(f[1][0][1]), "+v"(f[1][1][0]), "+v"(f[1][1][1]));
                else asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(f[0][0][0]), "+v"(f[0][0][1]), "+v"(f[0][1][0]), "+v"(f[0][1][1]));
            } else {
                if (NB == 2) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0][0][0]), "+v"(f[0][0][1]), "+v"(f[0][1][0]), "+v"(f[0][1][1]), "+v"(f[1][0][0]), "+v"(f[1][0][1]), "+v"(f[1][1][0]), "+v"(f[1][1][1]));
                else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0][0][0]), "+v"(f[0][0][1]), "+v"(f[0][1][0]), "+v"(f[0][1][1]));
            }
#pragma unroll
            for (int blk = 0; blk < NB; ++blk)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const bf16x4 x = f[blk][jj][0], y = f[blk][jj][1];
                    const bf16x8 vf = {x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]};
                    o[db] = mma32(vf, pf[blk][jj], o[db]);
                }
        }
    };

#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int jt = wave + 4 * i, s = jt * G::KT + lane;
        const uint64_t m = __builtin_amdgcn_ballot_w64(s < Tk && (nomask || vraw[i] != 0));
        if (lane == 0 && jt < nkt) vbits[jt] = m;
    }
    for (int jt = wave + 16; jt < nkt; jt += 4) {                       // sequences beyond 1024 keys: the remaining tiles, one by one
        const int s = jt * G::KT + lane;
        const uint8_t vbyte = valid_row ? valid_row[min(s, Tk - 1)] : (uint8_t)1;
        const uint64_t m = __builtin_amdgcn_ballot_w64(s < Tk && vbyte != 0);
        if (lane == 0) vbits[jt] = m;
    }
    // "Q is complete": a load issued before a loop and first used inside it stays pending in hipcc's waitcnt scoreboard at the loop
    // header -- every iteration would wait (vmcnt) for the LDS-DMA prefetch just issued as well
#pragma unroll
    for (int ks = 0; ks < G::NKS; ++ks) asm volatile("" ::"v"(qf[ks]));
    SA32_BARRIER();                                                     // the valid words are visible
#if SA32_TRACE
    const long long tr1 = wall_clock64();
    long long tr2 = tr1;
#endif
    // ---- the LIVE key tiles of this workgroup (round 6).  A tile whose 64 keys are all padding contributes nothing; until round 5 it
    // was still fetched (LDS-DMA), waited for and barriered, only its arithmetic was skipped -- and the kernel is bound by exactly
    // that traffic and latency, not by the arithmetic.  WikiWeb2M prompts are padded to max_input_length (data.py:320-321): on the
    // synthetic batches ~45 % of the key tiles a late query block walks are dead.  bit j of `live` <=> tile j has an attendable key;
    // the NPRO tiles requested by the prologue (before the mask bytes were known) stay in the walk whatever their words say.
    constexpr int NPRO = EARLY ? 2 : PD;
    uint64_t live = __builtin_amdgcn_ballot_w64(lane < nkt && vbits[min(lane, nkt - 1)] != 0ull);
    live |= (1ull << NPRO) - 1ull;
    if (nkt < 64) live &= (1ull << nkt) - 1ull;
    const int nlive = __builtin_popcountll(live);
    uint64_t rem = live & (live - 1ull);                                // tiles still to walk after tile j (= 0, forced live)
    uint64_t irem = live & ~((1ull << NPRO) - 1ull);                    // live tiles not yet requested
    int j = 0;
    uint64_t vm = vbits[0];
    int slot = 0, islot = PD % G::NS;
    for (int c = 0; c < nlive; ++c) {
#if SA32_TRACE
        if (c == 1) tr2 = wall_clock64();
#endif
        // walk step c has landed (this wave's pieces: all but the NP * (tiles still in flight behind it) youngest loads), then everybody's
        if (EARLY ? c == 0 : (PD >= 2 && c + 1 < nlive)) {
            if (G::NP == 4) SA32_VMCNT(4); else SA32_VMCNT(8);
        } else {
            SA32_VMCNT(0);
        }
        SA32_BARRIER();
        if (irem != 0ull && !(EARLY && c == 0)) {
            issue(__builtin_ctzll(irem), islot);
            irem &= irem - 1ull;
        }
        const int jn = rem != 0ull ? __builtin_ctzll(rem) : j;
        rem &= rem - 1ull;
        const uint64_t vnext = vbits[jn];
        const uint32_t vlo = __builtin_amdgcn_readfirstlane((uint32_t)vm), vhi = __builtin_amdgcn_readfirstlane((uint32_t)(vm >> 32));
        if (j <= jlast && (vlo | vhi) != 0u) {
            const bool mixed = (vlo & vhi) != 0xffffffffu;
            // (a one-block variant of the body for a diagonal tile whose second 32 keys lie above the whole wave would save 5 % of
            // the block steps at T = 640; as a second inlined body it costs 42 VGPRs and 48 accumulator copies per tile)
            body(std::integral_constant<int, 2>(), j, vlo, vhi, mixed, slot);
        }
        j = jn;
        vm = vnext;
        slot = (slot + 1 == G::NS) ? 0 : slot + 1;
        islot = (islot + 1 == G::NS) ? 0 : islot + 1;
    }

    if (EARLY) SA32_VMCNT(0);                                           // (one key tile: the early request of "tile 1" must not outlive the workgroup's LDS)
    // ---- epilogue: fold the lane pair's row sums, normalise, store O (16-byte stores after a v_permlane32_swap) and the LSE
#if SA32_TRACE
    const long long tr3 = wall_clock64();
#endif
    {
        float lo, up;
        swap32(lsum, lo, up);
        lsum = lo + up;
    }
    const float inv = __builtin_amdgcn_rcpf(lsum);
    const uint32_t orow = wave_active ? (uint32_t)trow * ldoB : OOB;
#pragma unroll
    for (int db = 0; db < G::NDB; ++db)
#pragma unroll
        for (int c = 0; c < 4; c += 2) {
            f32x4 ga, gb;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ga[r] = o[db][4 * c + r] * inv;
                gb[r] = o[db][4 * c + 4 + r] * inv;
            }
            u32x2 ua = __builtin_bit_cast(u32x2, __builtin_convertvector(ga, bf16x4)), ub = __builtin_bit_cast(u32x2, __builtin_convertvector(gb, bf16x4));
            uint32_t a0 = ua[0], a1 = ua[1], b0 = ub[0], b1 = ub[1];
            swap32_u32(a0, b0);
            swap32_u32(a1, b1);
            const u32x4 val = {a0, a1, b0, b1};
            __builtin_amdgcn_raw_buffer_store_b128(val, ro, orow + (uint32_t)(32 * db + 8 * (c + hi)) * 2u, 0, ATTN_STORE_AUX);
        }
    if (a.lse && hi == 0 && trow < Tq) a.lse[(size_t)bh * a.T + trow] = (m2 + __builtin_amdgcn_logf(lsum)) * LN2;
#if SA32_TRACE
    if (a.trace && threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // the output stores have been acknowledged
        long long* t = a.trace + (size_t)blockIdx.x * 8;
        t[0] = tr0; t[1] = tr1; t[2] = tr2; t[3] = tr3; t[4] = wall_clock64();
        t[5] = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));           // HW_REG_HW_ID
        t[6] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11));          // HW_REG_XCC_ID
        t[7] = nkt;
    }
#endif
}


// ================================================================================================================== backward
// Two kernels with the forward's skeleton (32x32x16 MFMAs, swapped products, LDS-DMA rings, tile classes from the valid words):
//   sa32_bwd_dq_kernel   workgroup = 128 query rows, loop over key tiles: dQ, and delta = rowsum(dO * O) for the second kernel
//   sa32_bwd_dkv_kernel  workgroup = 128 keys, loop over query tiles: dK, dV
// Every tile of the backward pass is read row-wise (ds_read_b128 A-operand fragments) AND transposed (ds_read_b64_tr_b16), so the
// ring tiles use one swizzle that is conflict-free for both: the 3 (4) row bits that the row-fragment read needs spread over
// distinct slots, bit-reversed so that rows r and r + 2 (which share a bank half) land in different 64-byte quarters.
template <int D> __device__ __forceinline__ int swz_u(int row) {
    if (D == 64) { const int x = (row >> 1) & 7; return ((x & 1) << 2) | (x & 2) | (x >> 2); }
    return ((row & 3) << 2) | ((row >> 2) & 3);
}
// lane base of the A-operand row fragment (row = lane & 31, 16-byte slot 2 ks + hi): address = base ^ (ks << 5)
template <int D> __device__ __forceinline__ int rowfrag_base(int lane) {
    const int row = lane & 31, hi = lane >> 5;
    return row * G32<D>::ROWB + ((hi ^ swz_u<D>(row)) << 4);
}
// lane base of the transposed fragment read (see the forward kernel): second read of a fragment (rows + 8) = (base ^ TRX) + 8 rows
template <int D> __device__ __forceinline__ int trfrag_base(int lane) {
    const int i = lane & 15, gg = lane >> 4;
    const int row = 4 * (gg >> 1) + (i >> 2);
    return row * G32<D>::ROWB + (((2 * (gg & 1) + ((i & 3) >> 1)) ^ swz_u<D>(row)) << 4) + 8 * (i & 1);
}
template <int D> struct TRX { static constexpr int value = (D == 64) ? 16 : 32; };      // what swz_u(row + 8) flips

struct SA32BwdArgs {
    const bf16 *dout, *q, *k, *v, *out;
    const float* lse;
    const uint8_t* valid;
    bf16 *dq, *dk, *dv;
    float* delta;              // [B, H, T]: written by the dQ kernel, read by the dK / dV kernel
    int B, H, T, P, nqb, nkb, ldq, ldk, ldg, ldgk;
    int G;                     // GQA instantiations only: query head h reads key / value head h / G (dk, dv stay per QUERY head)
    const int* tiles;          // TILES instantiations only (see SA32Args): k, v are compact [64 ntc, ldk]; dq, dk, dv stay dense
    int ntc;
    // TILES instantiations, optional (null: the dense layout above).  Live-first gradient rows: dest [B, T / 64] is a permutation of
    // the batch's 64-row tiles, and the rows of tile j of sample b are stored at rows 64 dest[b][j] .. + 63 of dq, dk, dv taken as
    // [B * T, ld] buffers.  Only the store addresses change.  dk / dv rows from dkv_rows on are not stored (nobody reads them).
    const int* dest;
    int dkv_rows;
};

// 16 transposed fragments' worth of reads for ONE 32-channel block: f[blk][jj][half]; rows 32 blk + 16 jj (+ 8) of the tile at `ad`
#define SA32_TR_READ(dst, ad, off) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(ad), "i"(off))

template <int D, bool GQA = false, bool TILES = false>
__global__ __launch_bounds__(256, SA32_DQ_OCC) void sa32_bwd_dq_kernel(SA32BwdArgs a) {
    typedef G32<D> G;
    constexpr int NS = SA32_NS_DQ, PD = NS - 1;
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int key = lane & 31, hi = lane >> 5;

    const int vid = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = vid / a.nqb, qblk = a.nqb - 1 - vid % a.nqb;
    const int b = bh / a.H, h = bh % a.H, hk = GQA ? h / a.G : h;
    const int Tq = a.T, Tk = a.T + a.P, HD = a.H * D;
    const int t0 = qblk * 128 + wave * 32, trow = t0 + key;
    const int nkt = (min(Tq, (qblk + 1) * 128) + a.P + G::KT - 1) / G::KT;
    TileRow tr{};
    if constexpr (TILES) tr.load(a.tiles, b, a.T / G::KT, a.ntc, lane);   // (see the forward kernel)

    const uint32_t ldqB = (uint32_t)a.ldq * 2u, ldkB = (uint32_t)a.ldk * 2u, ldoB = (uint32_t)HD * 2u, ldgB = (uint32_t)a.ldg * 2u;
    const int kvrows = TILES ? a.ntc * G::KT : Tk;
    const size_t kvbase = (TILES ? (size_t)0 : (size_t)b * Tk * a.ldk) + hk * D;
    const __amdgpu_buffer_rsrc_t rq = make_rsrc(a.q + (size_t)b * Tq * a.ldq + h * D, (uint32_t)(Tq - 1) * ldqB + D * 2);
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(a.k + kvbase, (uint32_t)(kvrows - 1) * ldkB + D * 2);
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(a.v + kvbase, (uint32_t)(kvrows - 1) * ldkB + D * 2);
    const __amdgpu_buffer_rsrc_t rg = make_rsrc(a.dout + (size_t)b * Tq * HD + h * D, (uint32_t)(Tq - 1) * ldoB + D * 2);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(a.out + (size_t)b * Tq * HD + h * D, (uint32_t)(Tq - 1) * ldoB + D * 2);
    const __amdgpu_buffer_rsrc_t rd = make_rsrc(a.dq + (size_t)b * Tq * a.ldg + h * D, (uint32_t)(Tq - 1) * ldgB + D * 2);
    const __amdgpu_buffer_rsrc_t rl = make_rsrc(a.lse + (size_t)bh * Tq, (uint32_t)Tq * 4u);

    uint64_t* vbits = (uint64_t*)(smem + NS * G::SLOTB);
    const __amdgpu_buffer_rsrc_t rvalid = make_rsrc(a.valid + (size_t)b * Tk, (uint32_t)Tk);
    uint8_t vraw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) vraw[i] = __builtin_amdgcn_raw_buffer_load_b8(rvalid, (uint32_t)((wave + 4 * i) * G::KT + lane), 0, 0);
    const float lraw = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rl, (uint32_t)trow * 4u, 0, 0));    // 0 past T

    // Q^T, dO^T (B operands) and O (for delta): lane (row, hi) holds channels 16 ks + 8 hi .. + 7
    bf16x8 qf[G::NKS], gf[G::NKS], of[G::NKS];
#pragma unroll
    for (int ks = 0; ks < G::NKS; ++ks) {
        const uint32_t c = (uint32_t)(16 * ks + 8 * hi) * 2u;
        qf[ks] = buf_load8<bf16>(rq, (uint32_t)trow * ldqB + c);
        gf[ks] = buf_load8<bf16>(rg, (uint32_t)trow * ldoB + c);
        of[ks] = buf_load8<bf16>(ro, (uint32_t)trow * ldoB + c);
    }
    uint32_t tvoff;
    {
        const int row = G::RPP * wave + lane / G::LPR, sl = lane % G::LPR;
        tvoff = (uint32_t)row * ldkB + (uint32_t)((sl ^ swz_u<D>(row)) << 4);
    }
    auto issue = [&](int j, int slot) __attribute__((always_inline)) {
        char* base = smem + slot * G::SLOTB + wave * 1024;
        const int jrow = TILES ? tr.row(j) : j * G::KT;
#pragma unroll
        for (int i = 0; i < G::PIECES / 4; ++i) {
            const int soff = (int)((uint32_t)(jrow + i * 4 * G::RPP) * ldkB);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (lds_void*)(base + i * 4096), 16, tvoff, soff, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (lds_void*)(base + G::TILEB + i * 4096), 16, tvoff, soff, 0, 0);
        }
    };
#pragma unroll
    for (int j = 0; j < PD; ++j) issue(j, j);
    constexpr bool EARLY = NS == 2;
    if (EARLY) issue(1, 1);

    const int lds0 = (int)(unsigned)(size_t)(lds_void*)smem;
    const int rbase = rowfrag_base<D>(lane);
    const int tbase = lds0 + trfrag_base<D>(lane);

    // delta = rowsum(dO * O) of this lane pair's row; the dK / dV kernel reads it from the workspace
    float delta = 0.f;
#pragma unroll
    for (int ks = 0; ks < G::NKS; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) delta = fmaf((float)gf[ks][e], (float)of[ks][e], delta);
    {
        float lo, up;
        swap32(delta, lo, up);
        delta = lo + up;
    }
    if (hi == 0 && trow < Tq) a.delta[(size_t)bh * Tq + trow] = delta;
    const float nlse2 = -lraw * LOG2E;

#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int jt = wave + 4 * i, s = jt * G::KT + lane;
        const uint64_t m = __builtin_amdgcn_ballot_w64(s < Tk && vraw[i] != 0);
        if (lane == 0 && jt < nkt) vbits[jt] = m;
    }
    for (int jt = wave + 16; jt < nkt; jt += 4) {
        const int s = jt * G::KT + lane;
        const uint8_t vbyte = a.valid[(size_t)b * Tk + min(s, Tk - 1)];
        const uint64_t m = __builtin_amdgcn_ballot_w64(s < Tk && vbyte != 0);
        if (lane == 0) vbits[jt] = m;
    }
#pragma unroll
    for (int ks = 0; ks < G::NKS; ++ks) asm volatile("" ::"v"(qf[ks]), "v"(gf[ks]));

    f32x16 acc[G::NDB];
#pragma unroll
    for (int db = 0; db < G::NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[db][r] = 0.f;
    const bool wave_active = t0 < Tq;
    const int tl = t0 + 31 + a.P;
    const int jlast = !wave_active ? -1 : min(nkt - 1, tl >> 6);

    auto body = [&](int j, uint32_t vlo, uint32_t vhi, bool mixed, int slot) __attribute__((always_inline)) {
        const char* Ks = smem + slot * G::SLOTB;
        const char* Vs = Ks + G::TILEB;
        bf16x8 dsf[2][2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int ks = 0; ks < G::NKS; ++ks) {
                const bf16x8 kf = *(const bf16x8*)(Ks + blk * 32 * G::ROWB + (rbase ^ (ks << 5)));
                const bf16x8 vf = *(const bf16x8*)(Vs + blk * 32 * G::ROWB + (rbase ^ (ks << 5)));
                s = mma32(kf, qf[ks], s);
                dp = mma32(vf, gf[ks], dp);
            }
            if (mixed) {
                const uint32_t w = (blk ? vhi : vlo) >> (4 * hi);
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = ((w >> kreg(r)) & 1u) ? s[r] : -INFINITY;
            }
            const int k0 = j * G::KT + 32 * blk;
            if (k0 + 31 > t0 + a.P) {
                const int c = trow + a.P - k0 - 4 * hi;
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = (kreg(r) <= c) ? s[r] : -INFINITY;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(fmaf(s[r], LOG2E, nlse2));
                s[r] = p * (dp[r] - delta);
            }
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                f32x8 t;
#pragma unroll
                for (int e = 0; e < 8; ++e) t[e] = s[8 * jj + e];
                dsf[blk][jj] = __builtin_convertvector(t, bf16x8);
            }
        }
        // dQ^T += K^T dS^T: K^T fragments by transposed reads of the same K tile, one 32-channel block at a time, two register sets
        bf16x4 ka[2][2][2][2];
        const int kslot = tbase + slot * G::SLOTB;
        auto treads = [&](int db, bf16x4 (&f)[2][2][2]) __attribute__((always_inline)) {
            const int ad0 = kslot ^ (db << 6), ad1 = ad0 ^ TRX<D>::value;
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    SA32_TR_READ(f[blk][jj][0], ad0, (32 * blk + 16 * jj) * G::ROWB);
                    SA32_TR_READ(f[blk][jj][1], ad1, (32 * blk + 16 * jj + 8) * G::ROWB);
                }
        };
        treads(0, ka[0]);
#pragma unroll
        for (int db = 0; db < G::NDB; ++db) {
            bf16x4 (&f)[2][2][2] = ka[db & 1];
            if (db + 1 < G::NDB) {
                treads(db + 1, ka[(db + 1) & 1]);
                asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(f[0][0][0]), "+v"(f[0][0][1]), "+v"(f[0][1][0]), "+v"(f[0][1][1]), "+v"(f[1][0][0]), "+v"(f[1][0][1]), "+v"(f[1][1][0]), "+v"(f[1][1][1]));
            } else {
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0][0][0]), "+v"(f[0][0][1]), "+v"(f[0][1][0]), "+v"(f[0][1][1]), "+v"(f[1][0][0]), "+v"(f[1][0][1]), "+v"(f[1][1][0]), "+v"(f[1][1][1]));
            }
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const bf16x4 x = f[blk][jj][0], y = f[blk][jj][1];
                    const bf16x8 kt = {x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]};
                    acc[db] = mma32(kt, dsf[blk][jj], acc[db]);
                }
        }
    };

    SA32_BARRIER();
    // the live key tiles only (see the forward kernel): dead tiles are neither fetched nor waited for
    constexpr int NPRO = EARLY ? 2 : PD;
    uint64_t live = __builtin_amdgcn_ballot_w64(lane < nkt && vbits[min(lane, nkt - 1)] != 0ull);
    live |= (1ull << NPRO) - 1ull;
    if (nkt < 64) live &= (1ull << nkt) - 1ull;
    const int nlive = __builtin_popcountll(live);
    uint64_t rem = live & (live - 1ull);
    uint64_t irem = live & ~((1ull << NPRO) - 1ull);
    int j = 0;
    uint64_t vm = vbits[0];
    int slot = 0, islot = PD % NS;
    for (int c = 0; c < nlive; ++c) {
        if (EARLY ? c == 0 : (PD >= 2 && c + 1 < nlive)) { if (G::NP == 4) SA32_VMCNT(4); else SA32_VMCNT(8); }       // step c landed, step c + 1 may be in flight
        else SA32_VMCNT(0);
        SA32_BARRIER();
        if (irem != 0ull && !(EARLY && c == 0)) {
            issue(__builtin_ctzll(irem), islot);
            irem &= irem - 1ull;
        }
        const int jn = rem != 0ull ? __builtin_ctzll(rem) : j;
        rem &= rem - 1ull;
        const uint64_t vnext = vbits[jn];
        const uint32_t vlo = __builtin_amdgcn_readfirstlane((uint32_t)vm), vhi = __builtin_amdgcn_readfirstlane((uint32_t)(vm >> 32));
        if (j <= jlast && (vlo | vhi) != 0u) body(j, vlo, vhi, (vlo & vhi) != 0xffffffffu, slot);
        j = jn;
        vm = vnext;
        slot = (slot + 1 == NS) ? 0 : slot + 1;
        islot = (islot + 1 == NS) ? 0 : islot + 1;
    }

    if (EARLY) SA32_VMCNT(0);
    uint32_t orow = wave_active ? (uint32_t)trow * ldgB : OOB;
    __amdgpu_buffer_rsrc_t rdst = rd;
    if constexpr (TILES) {
        if (a.dest) {                        // live-first rows: the wave's 32 rows lie in one 64-row tile (T is a multiple of 64)
            const int dt = wave_active ? a.dest[(size_t)b * (Tq / G::KT) + (t0 >> 6)] : -1;
            rdst = make_rsrc(a.dq + h * D, (uint32_t)(a.B * Tq - 1) * ldgB + D * 2);
            orow = (dt >= 0 && dt < a.B * (Tq / G::KT)) ? (uint32_t)(dt * G::KT + (trow & 63)) * ldgB : OOB;
        }
    }
#pragma unroll
    for (int db = 0; db < G::NDB; ++db)
#pragma unroll
        for (int c = 0; c < 4; c += 2) {
            f32x4 ga, gb;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ga[r] = acc[db][4 * c + r];
                gb[r] = acc[db][4 * c + 4 + r];
            }
            u32x2 ua = __builtin_bit_cast(u32x2, __builtin_convertvector(ga, bf16x4)), ub = __builtin_bit_cast(u32x2, __builtin_convertvector(gb, bf16x4));
            uint32_t a0 = ua[0], a1 = ua[1], b0 = ub[0], b1 = ub[1];
            swap32_u32(a0, b0);
            swap32_u32(a1, b1);
            const u32x4 val = {a0, a1, b0, b1};
            __builtin_amdgcn_raw_buffer_store_b128(val, TILES ? rdst : rd, orow + (uint32_t)(32 * db + 8 * (c + hi)) * 2u, 0, ATTN_STORE_AUX);
        }
}


// dK, dV: workgroup = 128 keys of one (batch, head), wave = 32 keys; loop over 64-row query tiles from the first row that sees the
// workgroup's keys to the last.  Per tile the ring slot holds Q and dO (row-major, swz_u) and the tile's lse / delta vectors.
// Non-swapped products put the KEY on the lane: S = Q K^T (A = Q rows from LDS, B = K^T in registers) leaves P / dS in the
// accumulators as [query (r, hi)][key = lane & 31] -- the B-operand layout of the contraction over queries -- and dV^T += dO^T P,
// dK^T += Q^T dS take their A operands by transposed reads of the same dO / Q tiles.  The row statistics enter as the MFMA
// C-input: with K and V NEGATED in registers the accumulators start at lse / delta (16-byte broadcast reads straight into the
// accumulator registers) and end at lse - q.k and delta - dO.v, so p = exp2(-log2e * acc + key bias) and dS = -p * acc': the sign
// of dS is folded into the final store of dK.  No row reductions, no per-element subtraction.
template <int D> struct GB32 {
    typedef G32<D> G;
    static constexpr int SLOTB = 2 * G::TILEB + 1024;                    // Q tile, dO tile, lse[64], delta[64], padding
    static constexpr int NS = (D == 64) ? SA32_NS_DKV : SA32_NS_DKV128;
    static constexpr int LDS = NS * SLOTB;
    static constexpr int NPB = 2 * G::PIECES / 4 + 2;                    // LDS-DMA instructions per wave and tile
};

// GQA = true: K / V of head h / a.G, dK / dV still of QUERY head h (the host points dk / dv at the expanded scratch and folds the group)
// TILES = true: k, v are compact (see the forward kernel).  A wave's 32 keys lie in one key tile: its compact row replaces the key's
// row in the K / V loads (by the per-lane offset: inside the descriptors' range check), and a wave in a dead tile -- no valid key, so
// no arithmetic either -- loads zeros.  dK / dV keep the dense layout, zeros in the dead tiles, as the fused dgrad reads them.
template <int D, bool GQA = false, bool TILES = false>
__global__ __launch_bounds__(256, D == 64 ? SA32_DKV_OCC64 : 1) void sa32_bwd_dkv_kernel(SA32BwdArgs a) {
    typedef G32<D> G;
    typedef GB32<D> GB;
    constexpr int NS = GB::NS, PD = NS - 1;
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int kl = lane & 31, hi = lane >> 5;

    const int vid = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = vid / a.nkb, kblk = vid % a.nkb;                      // low key blocks (most query tiles) first
    const int b = bh / a.H, h = bh % a.H, hk = GQA ? h / a.G : h;
    const int Tq = a.T, Tk = a.T + a.P, HD = a.H * D;
    const int k0 = kblk * 128 + wave * 32, krow = k0 + kl;               // this lane's key
    const int nqt = (Tq + 63) / 64;
    const int i0 = max(kblk * 128 - a.P, 0) / 64;                        // first query tile with a row that sees key kblk * 128
    int crow = krow;                                                     // this lane's row in k / v
    bool tile_ok = true;
    if constexpr (TILES) {
        const int ntl = Tk / G::KT, jt = k0 >> 6;                        // wave-uniform
        const int t = jt < ntl ? a.tiles[(size_t)b * ntl + jt] : -1;
        tile_ok = t >= 0 && t < a.ntc;
        crow = t * G::KT + (krow & 63);
    }

    const uint32_t ldqB = (uint32_t)a.ldq * 2u, ldkB = (uint32_t)a.ldk * 2u, ldoB = (uint32_t)HD * 2u, ldgB = (uint32_t)a.ldgk * 2u;
    const int kvrows = TILES ? a.ntc * G::KT : Tk;
    const size_t kvbase = (TILES ? (size_t)0 : (size_t)b * Tk * a.ldk) + hk * D;
    const __amdgpu_buffer_rsrc_t rq = make_rsrc(a.q + (size_t)b * Tq * a.ldq + h * D, (uint32_t)(Tq - 1) * ldqB + D * 2);
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(a.k + kvbase, (uint32_t)(kvrows - 1) * ldkB + D * 2);
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(a.v + kvbase, (uint32_t)(kvrows - 1) * ldkB + D * 2);
    const __amdgpu_buffer_rsrc_t rg = make_rsrc(a.dout + (size_t)b * Tq * HD + h * D, (uint32_t)(Tq - 1) * ldoB + D * 2);
    const __amdgpu_buffer_rsrc_t rdk = make_rsrc(a.dk + (size_t)b * Tk * a.ldgk + h * D, (uint32_t)(Tk - 1) * ldgB + D * 2);
    const __amdgpu_buffer_rsrc_t rdv = make_rsrc(a.dv + (size_t)b * Tk * a.ldgk + h * D, (uint32_t)(Tk - 1) * ldgB + D * 2);
    const __amdgpu_buffer_rsrc_t rl = make_rsrc(a.lse + (size_t)bh * Tq, (uint32_t)Tq * 4u);
    const __amdgpu_buffer_rsrc_t rdl = make_rsrc(a.delta + (size_t)bh * Tq, (uint32_t)Tq * 4u);
    const __amdgpu_buffer_rsrc_t rvalid = make_rsrc(a.valid + (size_t)b * Tk, (uint32_t)Tk);

    // K^T, V^T (B operands; lane = key): channels 16 ks + 8 hi .. + 7 of this lane's key row, sign flipped (see above)
    const uint8_t kvraw = __builtin_amdgcn_raw_buffer_load_b8(rvalid, (uint32_t)krow, 0, 0);       // 0 past the last key
    bf16x8 kf[G::NKS], vf[G::NKS];
#pragma unroll
    for (int ks = 0; ks < G::NKS; ++ks) {
        const uint32_t c = (tile_ok ? (uint32_t)crow * ldkB : OOB) + (uint32_t)(16 * ks + 8 * hi) * 2u;
        kf[ks] = buf_load8<bf16>(rk, c);
        vf[ks] = buf_load8<bf16>(rv, c);
    }
    uint32_t qvoff, gvoff;
    {
        const int row = G::RPP * wave + lane / G::LPR, sl = lane % G::LPR;
        const uint32_t sw = (uint32_t)((sl ^ swz_u<D>(row)) << 4);
        qvoff = (uint32_t)row * ldqB + sw;
        gvoff = (uint32_t)row * ldoB + sw;
    }
    auto issue = [&](int i, int slot) __attribute__((always_inline)) {
        char* base = smem + slot * GB::SLOTB;
#pragma unroll
        for (int c = 0; c < G::PIECES / 4; ++c) {
            const int r0 = i * 64 + c * 4 * G::RPP;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rq, (lds_void*)(base + wave * 1024 + c * 4096), 16, qvoff, (int)((uint32_t)r0 * ldqB), 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rg, (lds_void*)(base + G::TILEB + wave * 1024 + c * 4096), 16, gvoff, (int)((uint32_t)r0 * ldoB), 0, 0);
        }
        // the tile's 64 lse / delta values: every wave requests them (same bytes to the same place; keeps the vmcnt bookkeeping uniform)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rl, (lds_void*)(base + 2 * G::TILEB), 4, (uint32_t)lane * 4u, i * 256, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rdl, (lds_void*)(base + 2 * G::TILEB + 256), 4, (uint32_t)lane * 4u, i * 256, 0, 0);
    };
#pragma unroll
    for (int t = 0; t < PD; ++t) issue(i0 + t, t);                      // (a tile past the last query row reads as zeros)
    constexpr bool EARLY = NS == 2;
    if (EARLY) issue(i0 + 1, 1);

    const int lds0 = (int)(unsigned)(size_t)(lds_void*)smem;
    const int rbase = rowfrag_base<D>(lane);
    const int tbase = lds0 + trfrag_base<D>(lane);

    f32x16 dka[G::NDB], dva[G::NDB];
#pragma unroll
    for (int db = 0; db < G::NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dka[db][r] = 0.f; dva[db][r] = 0.f; }

    // sign flip + "these registers are complete" (see the forward kernel: loads first used inside the loop)
#pragma unroll
    for (int ks = 0; ks < G::NKS; ++ks) {
        u32x4 x = __builtin_bit_cast(u32x4, kf[ks]), y = __builtin_bit_cast(u32x4, vf[ks]);
#pragma unroll
        for (int e = 0; e < 4; ++e) { x[e] ^= 0x80008000u; y[e] ^= 0x80008000u; }
        kf[ks] = __builtin_bit_cast(bf16x8, x);
        vf[ks] = __builtin_bit_cast(bf16x8, y);
        asm volatile("" ::"v"(kf[ks]), "v"(vf[ks]));
    }
    const float kbias = (krow < Tk && kvraw != 0) ? 0.f : -INFINITY;
    const bool wave_has_keys = __builtin_amdgcn_ballot_w64(kbias == 0.f) != 0ull;     // a wave of masked / absent keys has dK = dV = 0

    auto body = [&](int i, int slot) __attribute__((always_inline)) {
        const char* Qs = smem + slot * GB::SLOTB;
        const char* Gs = Qs + G::TILEB;
        const char* St = Qs + 2 * G::TILEB;
        // per 32-query block: S^T / dP^T (lse, delta ride in as C), P and -dS, then dV^T += dO^T P and (-dK^T) += Q^T (-dS) through
        // transposed reads of that block's dO / Q rows, one 32-channel block of one operand at a time (reads of step + 1 under the MFMAs of step)
        const int qslot = tbase + slot * GB::SLOTB, gslot = qslot + G::TILEB;
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            f32x16 s, dp;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const f32x4 l4 = *(const f32x4*)(St + (32 * qb + 8 * c + 4 * hi) * 4);
                const f32x4 d4 = *(const f32x4*)(St + 256 + (32 * qb + 8 * c + 4 * hi) * 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) { s[4 * c + r] = l4[r]; dp[4 * c + r] = d4[r]; }
            }
#pragma unroll
            for (int ks = 0; ks < G::NKS; ++ks) {
                const bf16x8 qr = *(const bf16x8*)(Qs + qb * 32 * G::ROWB + (rbase ^ (ks << 5)));
                s = mma32(qr, kf[ks], s);
            }
#pragma unroll
            for (int ks = 0; ks < G::NKS; ++ks) {
                const bf16x8 gr = *(const bf16x8*)(Gs + qb * 32 * G::ROWB + (rbase ^ (ks << 5)));
                dp = mma32(gr, vf[ks], dp);
            }
            bf16x4 fa[2][2][2];
            auto treads = [&](int step, bf16x4 (&f)[2][2]) __attribute__((always_inline)) {     // step = 2 db + (0: dO, 1: Q)
                const int ad0 = ((step & 1) ? qslot : gslot) ^ ((step >> 1) << 6), ad1 = ad0 ^ TRX<D>::value;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    SA32_TR_READ(f[jj][0], ad0, (32 * qb + 16 * jj) * G::ROWB);
                    SA32_TR_READ(f[jj][1], ad1, (32 * qb + 16 * jj + 8) * G::ROWB);
                }
            };
            treads(0, fa[0]);
            // s = lse - q.k, dp = delta - dO.v;  query of register r: 64 i + 32 qb + kreg(r) + 4 hi
            const int q0 = i * 64 + 32 * qb;
            const bool diag = q0 + a.P < k0 + 31;                        // some (query, key) pair of this block with key > query + P
            const int c2 = krow - a.P - q0 - 4 * hi;                     // visible iff kreg(r) >= c2
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = fmaf(s[r], -LOG2E, kbias);
            if (diag) {                                                  // wave-uniform branch: off-diagonal blocks run none of this
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = (kreg(r) >= c2) ? s[r] : -INFINITY;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(s[r]);
                s[r] = p;
                dp[r] = p * dp[r];                                       // = -dS
            }
            bf16x8 pf[2], dsf[2];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                f32x8 t, u;
#pragma unroll
                for (int e = 0; e < 8; ++e) { t[e] = s[8 * jj + e]; u[e] = dp[8 * jj + e]; }
                pf[jj] = __builtin_convertvector(t, bf16x8);
                dsf[jj] = __builtin_convertvector(u, bf16x8);
            }
#pragma unroll
            for (int step = 0; step < 2 * G::NDB; ++step) {
                bf16x4 (&f)[2][2] = fa[step & 1];
                if (step + 1 < 2 * G::NDB) {
                    treads(step + 1, fa[(step + 1) & 1]);
                    asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(f[0][0]), "+v"(f[0][1]), "+v"(f[1][0]), "+v"(f[1][1]));
                } else {
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0][0]), "+v"(f[0][1]), "+v"(f[1][0]), "+v"(f[1][1]));
                }
                const int db = step >> 1;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const bf16x4 x = f[jj][0], y = f[jj][1];
                    const bf16x8 tf = {x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]};
                    if (step & 1) dka[db] = mma32(tf, dsf[jj], dka[db]);
                    else dva[db] = mma32(tf, pf[jj], dva[db]);
                }
            }
        }
    };

    // A workgroup whose 128 keys are ALL padding (round 6): its dK / dV are zero.  Until round 5 it still walked every query tile
    // (LDS-DMA, waits, barriers; only the arithmetic was skipped per wave).  The four waves exchange their ballots through the unused
    // tail of ring slot 0 behind one extra barrier; a dead workgroup's loop has no trips (a `break` out of the loop instead moved the
    // D = 128 accumulators into AGPRs: 304 -> 408 registers, +27 % time) and the epilogue stores the zero accumulators.
    int* wflag = (int*)(smem + 2 * G::TILEB + 512);
    if (lane == 0) wflag[wave] = wave_has_keys ? 1 : 0;
    SA32_BARRIER();
    const bool wg_dead = __builtin_amdgcn_readfirstlane(wflag[0] | wflag[1] | wflag[2] | wflag[3]) == 0;
    const int nqe = wg_dead ? i0 : nqt;                                 // workgroup-uniform
    int slot = 0, islot = PD % NS;
    for (int i = i0; i < nqe; ++i) {
        if (EARLY ? i == i0 : (PD >= 2 && i + 1 < nqe)) { if (GB::NPB == 6) SA32_VMCNT(6); else SA32_VMCNT(10); }     // tile i landed, tile i + 1 may be in flight
        else SA32_VMCNT(0);
        SA32_BARRIER();
        if (i + PD < nqe && !(EARLY && i == i0)) issue(i + PD, islot);
        // this wave's keys are seen by some row of the tile iff its first key k0 <= last row + P
        if (wave_has_keys && k0 <= i * 64 + 63 + a.P) body(i, slot);
        slot = (slot + 1 == NS) ? 0 : slot + 1;
        islot = (islot + 1 == NS) ? 0 : islot + 1;
    }

    if (EARLY || wg_dead) SA32_VMCNT(0);                                 // (the prologue's requests must not outlive the workgroup's LDS)
    // ---- epilogue: dK = -acc, dV rows (lane = key row: the forward kernel's output store)
    uint32_t orow = (krow < Tk) ? (uint32_t)krow * ldgB : OOB;
    __amdgpu_buffer_rsrc_t rdkd = rdk, rdvd = rdv;
    if constexpr (TILES) {
        if (a.dest) {                        // live-first rows (see SA32BwdArgs): the wave's 32 keys lie in one tile
            const int ntl = Tk / G::KT, jt = k0 >> 6;
            const int dt = jt < ntl ? a.dest[(size_t)b * ntl + jt] : -1;
            const uint32_t span = (uint32_t)(a.B * Tk - 1) * ldgB + D * 2;
            rdkd = make_rsrc(a.dk + h * D, span);
            rdvd = make_rsrc(a.dv + h * D, span);
            const int drow0 = dt * G::KT;
            orow = (dt >= 0 && dt < a.B * ntl && drow0 < a.dkv_rows) ? (uint32_t)(drow0 + (krow & 63)) * ldgB : OOB;
        }
    }
#pragma unroll
    for (int which = 0; which < 2; ++which)
#pragma unroll
        for (int db = 0; db < G::NDB; ++db)
#pragma unroll
            for (int c = 0; c < 4; c += 2) {
                f32x4 ga, gb;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    ga[r] = which ? dva[db][4 * c + r] : -dka[db][4 * c + r];
                    gb[r] = which ? dva[db][4 * c + 4 + r] : -dka[db][4 * c + 4 + r];
                }
                u32x2 ua = __builtin_bit_cast(u32x2, __builtin_convertvector(ga, bf16x4)), ub = __builtin_bit_cast(u32x2, __builtin_convertvector(gb, bf16x4));
                uint32_t a0 = ua[0], a1 = ua[1], b0 = ub[0], b1 = ub[1];
                swap32_u32(a0, b0);
                swap32_u32(a1, b1);
                const u32x4 val = {a0, a1, b0, b1};
                __builtin_amdgcn_raw_buffer_store_b128(val, TILES ? (which ? rdvd : rdkd) : (which ? rdv : rdk), orow + (uint32_t)(32 * db + 8 * (c + hi)) * 2u, 0,
                                                       ATTN_STORE_AUX);
            }
}

template <int D, bool CAUSAL, bool GQA = false, bool TILES = false> int launch_fwd(const SA32Args& a, int nblocks, hipStream_t st) {
    typedef G32<D> G;
    auto kern = sa32_fwd_kernel<D, CAUSAL, GQA, TILES>;
    if (int rc = mmgl_set_lds(kern, G::LDS, "sa32_fwd")) return rc;
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(256), G::LDS, st, a);
    MMGL_CHECK_LAUNCH("sa32_fwd");
    return MMGL_OK;
}

template <int D, bool GQA = false, bool TILES = false> int launch_bwd_dq(const SA32BwdArgs& a, hipStream_t st) {
    typedef G32<D> G;
    constexpr int LDS = SA32_NS_DQ * G::SLOTB + G::MAXT * 8;
    auto kern = sa32_bwd_dq_kernel<D, GQA, TILES>;
    if (int rc = mmgl_set_lds(kern, LDS, "sa32_bwd_dq")) return rc;
    hipLaunchKernelGGL(kern, dim3(a.B * a.H * a.nqb), dim3(256), LDS, st, a);
    MMGL_CHECK_LAUNCH("sa32_bwd_dq");
    return MMGL_OK;
}

template <int D, bool GQA = false, bool TILES = false> int launch_bwd_dkv(const SA32BwdArgs& a, hipStream_t st) {
    typedef GB32<D> GB;
    auto kern = sa32_bwd_dkv_kernel<D, GQA, TILES>;
    if (int rc = mmgl_set_lds(kern, GB::LDS, "sa32_bwd_dkv")) return rc;
    hipLaunchKernelGGL(kern, dim3(a.B * a.H * a.nkb), dim3(256), GB::LDS, st, a);
    MMGL_CHECK_LAUNCH("sa32_bwd_dkv");
    return MMGL_OK;
}

}  // namespace

bool sa32_supported(int dtype, int D, int Tk) { return dtype == MMGL_BF16 && (D == 64 || D == 128) && Tk <= 64 * 64; }

int sa32_fwd(const void* q, const void* k, const void* v, const uint8_t* valid, void* out, float* lse, int B, int H, int T, int P,
             int D, int ldq, int ldk, hipStream_t st, int G) {
    SA32Args a{};
    a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.valid = valid; a.out = (bf16*)out; a.lse = lse; a.cu = nullptr;
    a.B = B; a.H = H; a.T = T; a.P = P; a.nqb = cdiv(T, 128); a.ldq = ldq; a.ldk = ldk; a.ldo = H * D; a.q_rows = T;
#if SA32_TRACE
    if (const char* e = getenv("MMGL_SA32_TRACE")) a.trace = (long long*)strtoull(e, nullptr, 0);
#endif
    const int nblocks = B * H * a.nqb;
    a.G = G;
    if (G > 1) return D == 64 ? launch_fwd<64, true, true>(a, nblocks, st) : launch_fwd<128, true, true>(a, nblocks, st);
    return D == 64 ? launch_fwd<64, true>(a, nblocks, st) : launch_fwd<128, true>(a, nblocks, st);
}

int sa32_tiles_fwd(const void* q, const void* k, const void* v, const uint8_t* valid, const int* tiles, void* out, float* lse, int B,
                   int H, int T, int ntc, int ldq, int ldk, hipStream_t st) {
    SA32Args a{};
    a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.valid = valid; a.out = (bf16*)out; a.lse = lse; a.cu = nullptr;
    a.B = B; a.H = H; a.T = T; a.P = 0; a.nqb = cdiv(T, 128); a.ldq = ldq; a.ldk = ldk; a.ldo = H * 64; a.q_rows = T;
    a.G = 1; a.tiles = tiles; a.ntc = ntc;
    return launch_fwd<64, true, false, true>(a, B * H * a.nqb, st);
}

int sa32_enc_fwd(const void* q, const void* k, const void* v, const int* cu, void* out, int nseq, int H, int D, int ld_in, int ld_out,
                 int max_len, int q_rows, hipStream_t st) {
    SA32Args a{};
    a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.valid = nullptr; a.out = (bf16*)out; a.lse = nullptr; a.cu = cu;
    a.B = nseq; a.H = H; a.T = max_len; a.P = 0; a.nqb = cdiv(max_len < q_rows ? max_len : q_rows, 128); a.ldq = ld_in; a.ldk = ld_in;
    a.ldo = ld_out; a.q_rows = q_rows; a.G = 1;
    const int nblocks = nseq * H * a.nqb;
    return D == 64 ? launch_fwd<64, false>(a, nblocks, st) : launch_fwd<128, false>(a, nblocks, st);
}

int sa32_bwd(const void* dout, const void* q, const void* k, const void* v, const void* out, const float* lse, const uint8_t* valid,
             void* dq, void* dk, void* dv, float* delta, int B, int H, int T, int P, int D, int ldq, int ldk, int ldg, int ldgk,
             hipStream_t st, int G) {
    SA32BwdArgs a{};
    a.dout = (const bf16*)dout; a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.out = (const bf16*)out; a.lse = lse;
    a.valid = valid; a.dq = (bf16*)dq; a.dk = (bf16*)dk; a.dv = (bf16*)dv; a.delta = delta;
    a.B = B; a.H = H; a.T = T; a.P = P; a.nqb = cdiv(T, 128); a.nkb = cdiv(T + P, 128); a.ldq = ldq; a.ldk = ldk; a.ldg = ldg; a.ldgk = ldgk;
    a.G = G;
    if (G > 1) {
        if (int rc = D == 64 ? launch_bwd_dq<64, true>(a, st) : launch_bwd_dq<128, true>(a, st)) return rc;
        return D == 64 ? launch_bwd_dkv<64, true>(a, st) : launch_bwd_dkv<128, true>(a, st);
    }
    if (int rc = D == 64 ? launch_bwd_dq<64>(a, st) : launch_bwd_dq<128>(a, st)) return rc;
    return D == 64 ? launch_bwd_dkv<64>(a, st) : launch_bwd_dkv<128>(a, st);
}

int sa32_tiles_bwd(const void* dout, const void* q, const void* k, const void* v, const void* out, const float* lse, const uint8_t* valid,
                   const int* tiles, void* dq, void* dk, void* dv, float* delta, int B, int H, int T, int ntc, int ldq, int ldk, int ldg,
                   int ldgk, hipStream_t st, const int* dest, int dkv_rows) {
    SA32BwdArgs a{};
    a.dest = dest; a.dkv_rows = dkv_rows;
    a.dout = (const bf16*)dout; a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.out = (const bf16*)out; a.lse = lse;
    a.valid = valid; a.dq = (bf16*)dq; a.dk = (bf16*)dk; a.dv = (bf16*)dv; a.delta = delta;
    a.B = B; a.H = H; a.T = T; a.P = 0; a.nqb = cdiv(T, 128); a.nkb = cdiv(T, 128); a.ldq = ldq; a.ldk = ldk; a.ldg = ldg; a.ldgk = ldgk;
    a.G = 1; a.tiles = tiles; a.ntc = ntc;
    if (int rc = launch_bwd_dq<64, false, true>(a, st)) return rc;
    return launch_bwd_dkv<64, false, true>(a, st);
}
