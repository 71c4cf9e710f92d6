/*
 * mmgl_hip.h -- C ABI of libmmgl_hip.so: the MI355X (gfx950) kernels behind MMGL's
 * neighbor-fusion hot path.
 *
 * The reference (minjiyoon/MMGL) has no FFI: the path sits behind a Python module API
 * (SURVEY.md 8b).  Each entry point below replaces a run of stock ATen ops inside one reference
 * function; the citation after "replaces:" is reference file:line.  The Python binding that a
 * maintainer of the reference would add is in INTEGRATION.md (ctypes, one torch.autograd.Function
 * per fwd/bwd pair).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is allocated inside; scratch
 *     is passed explicitly (query the size with the matching *_workspace function).
 *   - tensors are dense row-major in the layout given in the comment.
 *   - dtype: element type of the activations (MMGL_F32 / MMGL_BF16); reductions, softmax and
 *     accumulation are always fp32.
 *   - last argument: the hipStream_t to launch on, passed as void* (0 = default stream).
 *   - returns 0 on success, otherwise an MMGL_ERR_* code; mmgl_last_error() gives the message.
 *     The Python shim maps INVALID/UNSUPPORTED to ValueError (the reference raises ValueError for
 *     shape / mode mismatches, modelling_cross_attention.py:160-164,214-224,260-264) and HIP to
 *     RuntimeError.
 *   - re-entrant.  Global state: the last-error string (thread-local), and ONE opt-in per-device setting, the dynamic tile
 *     schedule of the persistent GEMM (mmgl_gemm_set_tile_counter below): while it is set, that device's persistent-GEMM launches
 *     COUNTERS are bound to one stream (the first one that launches after the call); a launch on another stream runs on the static
 *     schedule (MMGL_GEMM_STRICT_STREAM=1: returns MMGL_ERR_INVALID instead).  With the default static schedule nothing is shared
 *     between calls.
 */
#ifndef MMGL_HIP_H
#define MMGL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MMGL_F32 = 0, MMGL_BF16 = 1 };
enum { MMGL_OK = 0, MMGL_ERR_INVALID = 1, MMGL_ERR_UNSUPPORTED = 2, MMGL_ERR_HIP = 3 };
enum { MMGL_ACT_NONE = 0, MMGL_ACT_RELU = 1 };

const char* mmgl_last_error(void);
int mmgl_version(void);

/* ---------------------------------------------------------------------------------------------
 * Masked cross-attention core:  O = softmax(max(Q K^T + M, finfo.min)) V   per (batch, head)
 * replaces: MPTAttention.forward, model/modelling_cross_attention.py:206-271 (head split, bmm,
 *           additive mask + clamp, softmax, bmm, head merge) and _expand_mask :68-79 (the
 *           [B,1,T,S] additive mask is never materialised: the [B,S] byte mask is consumed).
 *   q         [B,T,H*D]  already projected AND scaled by D^-0.5 (:194)
 *   k, v      [B,S,H*D]  projected neighbor tokens (:198-199)
 *   key_valid [B,S] uint8, 1 = attend (neighbor pos_id > 0, :1077/:1084-1104)
 *   out       [B,T,H*D]
 *   lse       [B,H,T] fp32 log-sum-exp of the masked scores (saved for backward)
 * A sample with no valid key yields the uniform distribution over its S keys (the reference's
 * finfo.min clamp, :226-228), never NaN; its lse is m + log l with m = 0, i.e. log S (the backward
 * never reads it for such a sample).  D in {16,32,64,128}; S <= 256; fp32 with D = 128 serves
 * S <= 128 (K and V of 256 keys would be 256 KiB of LDS): beyond, both entry points return
 * MMGL_ERR_UNSUPPORTED before any launch.
 * No attention dropout here (:256): OPT's attention_dropout is 0.0, where it is the identity; a config that asks for it (or for a
 * head mask / output_attentions) is routed to mmgl_attn_general_* below by the host mirror.
 */
int mmgl_xattn_fwd(const void* q, const void* k, const void* v, const uint8_t* key_valid,
                   void* out, float* lse, int B, int H, int T, int S, int D, int dtype, void* stream);

/* Backward of the above.  dq [B,T,H*D], dk/dv [B,S,H*D].  `workspace` must hold
 * mmgl_xattn_bwd_workspace(...) bytes (fp32 row-dots + per-chunk dK/dV partials, reduced in a
 * fixed order => bitwise deterministic).  On a sample with no valid key dQ/dK are halved exactly
 * as autograd does for the reference's torch.max tie (see oracle/lm_ref.py attention_core). */
size_t mmgl_xattn_bwd_workspace(int B, int H, int T, int S, int D);
int mmgl_xattn_bwd(const void* dout, const void* q, const void* k, const void* v, const float* lse,
                   const uint8_t* key_valid, void* dq, void* dk, void* dv,
                   void* workspace, size_t workspace_bytes,
                   int B, int H, int T, int S, int D, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Causal self-attention of the (frozen) decoder layers, flash style:  O = softmax(mask(Q K^T)) V,
 * mask = (s <= t) AND key_valid[b,s].
 * replaces: MPTAttention.forward self branch, model/modelling_cross_attention.py:203-271 with the additive masks of
 *           _make_causal_mask / _expand_mask (:51-79, :455-476): neither the [B,1,T,T] mask nor the [B,H,T,T] scores exist.
 *   q [B,T,H*D] already scaled by D^-0.5 ; k, v [B,T,H*D] ; key_valid [B,T] uint8 (the LM attention_mask)
 *   out [B,T,H*D] ; lse [B,H,T] fp32.
 * Precondition: key_valid[b,0] == 1 for every b (right-padded sequences, wikiweb2m/data.py:321-333), so every query row
 * keeps at least one key and the result equals the reference's finfo.min-clamped softmax; the host wrapper checks it.
 * SURVEY.md 8(f) row 2.  Backward returns dq, dk, dv (the layers are frozen, activations still need gradients);
 * `out` is the forward output (delta = rowsum(dO*O)); workspace >= mmgl_selfattn_bwd_workspace bytes.
 * ld_qkv / ld_dqkv: row stride in elements of q,k,v / dq,dk,dv; 0 = packed (H*D).  With 3*H*D the three pointers are
 * column slices of ONE fused projection output / gradient buffer (one fused-QKV GEMM forward, one dgrad GEMM backward).
 * out, dout are always packed.
 */
int mmgl_selfattn_fwd(const void* q, const void* k, const void* v, const uint8_t* key_valid, void* out, float* lse,
                      int B, int H, int T, int D, int ld_qkv, int dtype, void* stream);
size_t mmgl_selfattn_bwd_workspace(int B, int H, int T);
int mmgl_selfattn_bwd(const void* dout, const void* q, const void* k, const void* v, const void* out, const float* lse,
                      const uint8_t* key_valid, void* dq, void* dk, void* dv, void* workspace, size_t workspace_bytes,
                      int B, int H, int T, int D, int ld_qkv, int ld_dqkv, int dtype, void* stream);
/* The same attention with P always-visible PREFIX keys in front of the T causal ones: key s is visible to query t iff
 * s <= t + P (and key_valid[b][s]).
 * replaces: the self-attention of an OPT layer under peft prefix tuning (reference model/modelling_self_attention.py:88-93,
 *   PrefixTuningConfig(num_virtual_tokens=20): a learned per-layer key/value prefix that HF concatenates in front of the layer's
 *   keys and values as past_key_values).
 *   q, dq [B,T,·] (row strides ld_q / ld_dq), k, v, dk, dv [B,P+T,·] (ld_kv / ld_dkv), key_valid [B,P+T], out, dout [B,T,H*D]
 *   packed, lse [B,H,T].  P = 0 is mmgl_selfattn_fwd / _bwd.  Workspace: mmgl_selfattn_bwd_workspace(B, H, T). */
int mmgl_selfattn_prefix_fwd(const void* q, const void* k, const void* v, const uint8_t* key_valid, void* out, float* lse,
                             int B, int H, int T, int P, int D, int ld_q, int ld_kv, int dtype, void* stream);
int mmgl_selfattn_prefix_bwd(const void* dout, const void* q, const void* k, const void* v, const void* out, const float* lse,
                             const uint8_t* key_valid, void* dq, void* dk, void* dv, void* workspace, size_t workspace_bytes,
                             int B, int H, int T, int P, int D, int ld_q, int ld_kv, int ld_dq, int ld_dkv, int dtype, void* stream);
/* The same attention (no prefix) with GROUPED-QUERY heads: k, v, dk, dv hold Hkv heads, H = G * Hkv, and query head h reads key /
 * value head h / G -- transformers' repeat_kv, the self-attention of Llama-2-70B, Llama-3.x, TinyLlama (Hkv = 1: multi-query).
 *   q, dq [B,T,·] (row strides ld_q / ld_dq >= H*D), k, v, dk, dv [B,T,·] (ld_kv / ld_dkv >= Hkv*D), 0 = packed; three column
 *   slices of one [B,T,(H + 2 Hkv)*D] buffer are the intended use.  out, dout [B,T,H*D] packed, lse [B,H,T], key_valid [B,T].
 * H % Hkv != 0 or Hkv < 1: MMGL_ERR_INVALID before any launch.  head_dim / dtype rules and the kernel family chosen are those of
 * mmgl_selfattn_*; Hkv == H IS mmgl_selfattn_fwd / _bwd (same kernels, same numbers, workspace = mmgl_selfattn_bwd_workspace).
 * Backward, Hkv < H: out, lse, dq are computed per query head exactly as in the multi-head kernels; the dK / dV kernel writes one
 * gradient per QUERY head into the workspace ([B,T,2,H*D] behind delta) and a fold kernel sums each group in fp32, g = 0 .. G-1,
 * into dk / dv with one rounding (no atomics, deterministic).  dk, dv and workspace must be 16-byte aligned. */
int mmgl_selfattn_gqa_fwd(const void* q, const void* k, const void* v, const uint8_t* key_valid, void* out, float* lse,
                          int B, int H, int Hkv, int T, int D, int ld_q, int ld_kv, int dtype, void* stream);
size_t mmgl_selfattn_gqa_bwd_workspace(int B, int H, int Hkv, int T, int D, int dtype);
int mmgl_selfattn_gqa_bwd(const void* dout, const void* q, const void* k, const void* v, const void* out, const float* lse,
                          const uint8_t* key_valid, void* dq, void* dk, void* dv, void* workspace, size_t workspace_bytes,
                          int B, int H, int Hkv, int T, int D, int ld_q, int ld_kv, int ld_dq, int ld_dkv, int dtype, void* stream);

/* Live key tiles only: mmgl_selfattn_fwd / _bwd for a batch whose padded keys fill whole 64-key tiles (bf16, D = 64, T a multiple of
 * 64 up to 4096, multi-head; anything else returns MMGL_ERR_UNSUPPORTED).  A key tile (keys 64 j .. 64 j + 63 of a sample) is live
 * when any of its keys is valid.  k, v hold the live tiles and nothing else: [m_live, ld_kv] rows for the whole batch, m_live = 64 x
 * live tiles, tiles numbered sample by sample in key order.  key_tiles [B, T / 64] int32 gives the compact tile of every key tile,
 * -1 for a dead one.  q, out, lse and dq, dk, dv keep their dense [B, T, ld] layout (dk, dv of a dead tile are zero).  The arithmetic
 * is that of the dense entry points (a dead tile contributes nothing there either), so out, lse, dq, dk and dv are bitwise theirs.
 * Every index read from key_tiles is clamped to the m_live rows.  Workspace: mmgl_selfattn_bwd_workspace(B, H, T). */
int mmgl_selfattn_tiles_fwd(const void* q, const void* k, const void* v, const uint8_t* key_valid, const int32_t* key_tiles,
                            void* out, float* lse, int B, int H, int T, int D, int m_live, int ld_q, int ld_kv, int dtype,
                            void* stream);
int mmgl_selfattn_tiles_bwd(const void* dout, const void* q, const void* k, const void* v, const void* out, const float* lse,
                            const uint8_t* key_valid, const int32_t* key_tiles, void* dq, void* dk, void* dv, void* workspace,
                            size_t workspace_bytes, int B, int H, int T, int D, int m_live, int ld_q, int ld_kv, int ld_dq,
                            int ld_dkv, int dtype, void* stream);
/* mmgl_selfattn_tiles_rows_bwd: mmgl_selfattn_tiles_bwd with live-first gradient rows.  dq, dk, dv are [B * T, ld] buffers and
 * dest_tiles [B, T / 64] int32 is a permutation of the batch's 64-row tiles: the rows of tile j of sample b go to rows
 * 64 dest_tiles[b][j] .. + 63.  The caller sends a live tile to its compact index (key_tiles) and the dead ones behind them, so
 * that the rows from m_live on have dk = dv = 0 and a GEMM over [dq | dk | dv] may skip those columns there (mmgl_gemm_nt_rowk).
 * Every value is bitwise that of mmgl_selfattn_tiles_bwd; only the store addresses differ.  dk / dv rows from dkv_rows on (a
 * multiple of 64, >= m_live) are not stored at all; the zeros of the dead tiles below it are.  An entry of dest_tiles outside
 * [0, B * T / 64) drops that tile's stores.  The gradient buffers must stay below 2 GiB. */
int mmgl_selfattn_tiles_rows_bwd(const void* dout, const void* q, const void* k, const void* v, const void* out, const float* lse,
                                 const uint8_t* key_valid, const int32_t* key_tiles, const int32_t* dest_tiles, void* dq, void* dk,
                                 void* dv, void* workspace, size_t workspace_bytes, int B, int H, int T, int D, int m_live,
                                 int dkv_rows, int ld_q, int ld_kv, int ld_dq, int ld_dkv, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * General attention core: the options of MPTAttention.forward the fused kernels above leave out -- attention-probability dropout,
 * layer_head_mask, output_attentions -- for both call sites of the class (causal = 0: the gated cross-attention layers, key mask only;
 * causal = 1: the decoder's self-attention, (s <= t) AND key_valid, S == T).
 * replaces: model/modelling_cross_attention.py:206-271 incl. :237-244 (layer_head_mask scales the probabilities of a head),
 *           :246-254 (attn_weights_reshaped: the head-masked probabilities, returned BEFORE dropout), :256 (nn.functional.dropout on
 *           the probabilities); model/modelling_self_attention.py reaches the same class through the OPT decoder.
 *   q [B,T,H*D] already scaled; k, v [B,S,H*D]; key_valid [B,S] uint8; head_mask [H] fp32 or NULL
 *   out [B,T,H*D]; probs [B,H,T,S] (dtype of q) or NULL; lse [B,H,T] fp32: log-sum-exp of the allowed scores, and exactly +inf on
 *   a query ROW without any allowed key (per row, not per sample: left padding under the causal mask).  Such a row is uniform
 *   over all S keys, future and padded ones included -- probs holds dtype(fp32(1 / S) * head_mask[h]) there --, as the reference's
 *   finfo.min clamp gives; the backward keys off the +inf (dS halved at the tie, zero on keys both future and padded).
 *   A masked key's probs are exact zeros, and so are its dk, dv unless such a row reaches it.
 *   p_drop in [0, 1): probability of dropping a probability; the keep mask is the counter hash of (seed, element index) every
 *   dropout of this library uses, at element index ((b H + h) T + t) S + s (64-bit), kept iff hash >= uint32(min(p 2^32, 2^32 - 1)),
 *   scaled by fp32(1 / (1 - p)); regenerated by the backward from the same (p_drop, seed) -- nothing is stored.
 *   workspace: mmgl_attn_general_bwd_workspace(B, H, T) bytes (delta, B H T fp32); a shorter one is refused.
 * Written for exactness, not speed (fp32 VALU arithmetic, two passes over the keys): these options are inert on every BASELINE config
 * (attention_dropout = 0, no head masks); every other call stays on mmgl_xattn_* / mmgl_selfattn_*.  D <= 128, any S.
 * mmgl_attn_dropout_mask writes the keep mask as bytes [B,H,T,S] (1 = kept): a test / debug entry point (the parity tests hand it to
 * the oracle so both sides drop the same probabilities).
 */
int mmgl_attn_general_fwd(const void* q, const void* k, const void* v, const uint8_t* key_valid, const float* head_mask, void* out,
                          void* probs, float* lse, int B, int H, int T, int S, int D, int causal, float p_drop,
                          uint64_t seed, int dtype, void* stream);
size_t mmgl_attn_general_bwd_workspace(int B, int H, int T);
int mmgl_attn_general_bwd(const void* dout, const void* q, const void* k, const void* v, const float* lse, const uint8_t* key_valid,
                          const float* head_mask, void* dq, void* dk, void* dv, void* workspace, size_t workspace_bytes, int B, int H,
                          int T, int S, int D, int causal, float p_drop, uint64_t seed, int dtype, void* stream);
int mmgl_attn_dropout_mask(uint8_t* mask, int B, int H, int T, int S, float p_drop, uint64_t seed, void* stream);

/* ---------------------------------------------------------------------------------------------
 * T5 attention (csrc/relbias.hip): unscaled scores plus a learned per-head relative-position bias, on the MFMAs.
 * replaces: transformers T5Attention.forward (scores + compute_bias(T, S) + mask, softmax in fp32, dropout, matmul with V).
 *   q [B,T,H*D] rows ldq elements apart; k, v [B,S,H*D] rows ldkv elements apart (pitches: multiples of 8, >= H*D)
 *   key_valid [B,S] uint8, or NULL for all valid
 *   table [num_buckets,H] fp32, or NULL for no bias (the decoder-to-encoder cross-attention); bucket_of int32 [T+S-1], the entry of
 *   the pair (t, s) at s - t + T - 1, values in [0, num_buckets) (clamped into it)
 *   score = q . k + table[bucket_of[s - t + T - 1], h]  -- no D^-0.5 scale; causal: s <= t only, needs T == S
 *   p_drop, seed: dropout on the probabilities, the counter hash of (seed, ((b H + h) T + t) S + s) of mmgl_attn_general_*
 *   out [B,T,H*D] packed; lse [B,H,T] fp32
 * D = 64 only (every T5 up to t5-large has d_kv = 64), any T, S >= 1; everything else returns MMGL_ERR_UNSUPPORTED before any launch.
 * A query row without an allowed key is outside the contract (T5's prompts always hold tokens): it writes zeros to out, 0 to lse and
 * contributes nothing to any gradient (HuggingFace gives such a row the uniform distribution).
 * Backward: dout, out, dq [B,T,H*D] and dk, dv [B,S,H*D] packed; dtable fp32 [num_buckets,H] (NULL when table is NULL) is written
 * completely -- a bucket no pair reaches gets 0 -- and reproducibly: no floating-point atomics, per-tile diagonal sums in the workspace
 * are folded in a fixed order.  `workspace`: mmgl_attn_relbias_bwd_workspace(B, H, T, S) bytes, 16-byte aligned.
 */
int mmgl_attn_relbias_fwd(const void* q, const void* k, const void* v, const uint8_t* key_valid, const float* table,
                          const int32_t* bucket_of, void* out, float* lse, int B, int H, int T, int S, int D, int num_buckets,
                          int ldq, int ldkv, int causal, float p_drop, uint64_t seed, int dtype, void* stream);
size_t mmgl_attn_relbias_bwd_workspace(int B, int H, int T, int S);
int mmgl_attn_relbias_bwd(const void* dout, const void* q, const void* k, const void* v, const void* out, const float* lse,
                          const uint8_t* key_valid, const float* table, const int32_t* bucket_of, void* dq, void* dk, void* dv,
                          float* dtable, void* workspace, size_t workspace_bytes, int B, int H, int T, int S, int D,
                          int num_buckets, int ldq, int ldkv, int causal, float p_drop, uint64_t seed, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LayerNorm (affine, eps inside the sqrt) over the last dim.
 * replaces: nn.LayerNorm at modelling_cross_attention.py:319-320, 340-341, 349-350, 364-365, 635-636
 *   x,y [rows,cols]; gamma,beta [cols] (same dtype as x; may be NULL = no affine); mean,rstd [rows] fp32
 */
int mmgl_layernorm_fwd(const void* x, const void* gamma, const void* beta, void* y, float* mean, float* rstd,
                       int rows, int cols, float eps, int dtype, void* stream);
/* dgamma/dbeta are fp32 [cols] (may be NULL for a frozen norm); workspace >= mmgl_norm_bwd_workspace bytes. */
size_t mmgl_norm_bwd_workspace(int rows, int cols);
int mmgl_layernorm_bwd(const void* dy, const void* x, const void* gamma, const float* mean, const float* rstd,
                       void* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                       int rows, int cols, int dtype, void* stream);

/* RMSNorm  y = x * rsqrt(mean(x^2)+eps) * gamma   (Llama variant of the same block; no reference
 * counterpart in MMGL -- SURVEY.md 7.3 "config 5") */
int mmgl_rmsnorm_fwd(const void* x, const void* gamma, void* y, float* rstd,
                     int rows, int cols, float eps, int dtype, void* stream);
int mmgl_rmsnorm_bwd(const void* dy, const void* x, const void* gamma, const float* rstd,
                     void* dx, float* dgamma, void* workspace, size_t workspace_bytes,
                     int rows, int cols, int dtype, void* stream);

/* The residual add of a Llama layer fused with the RMSNorm that follows it (transformers' LlamaDecoderLayer: "hidden = residual +
 * hidden" then the next layer's input_layernorm / this layer's post_attention_layernorm; the OPT counterpart is
 * mmgl_add_layernorm_fwd/bwd):  sum_out = res + x,  y = RMSNorm(sum_out).  Backward: dres = RMSNorm'(dy) + dsum (dsum = the gradient
 * arriving on the residual stream, may be NULL) -- also the gradient of x.  dgamma fp32 optional (workspace as mmgl_rmsnorm_bwd). */
int mmgl_add_rmsnorm_fwd(const void* x, const void* res, const void* gamma, void* sum_out, void* y, float* rstd,
                         int rows, int cols, float eps, int dtype, void* stream);
int mmgl_add_rmsnorm_bwd(const void* dy, const void* dsum, const void* sum, const void* gamma, const float* rstd,
                         void* dres, float* dgamma, void* workspace, size_t workspace_bytes,
                         int rows, int cols, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gated residual:  y = residual + tanh(gate) * dropout(x, p)
 * replaces: nn.functional.dropout + "residual + tanh(gating) * h", modelling_cross_attention.py:332-335, 356-359
 *   residual,x,y [n] ; gate: device fp32 scalar (NULL => ungated, tanh(gate) := 1, :337/:361)
 *   dropout mask is a counter-based hash of (seed, element index): regenerated in backward.
 */
int mmgl_gated_residual_fwd(const void* residual, const void* x, const float* gate, void* y,
                            size_t n, float p_drop, uint64_t seed, int dtype, void* stream);
/* dres = dy (caller aliases it); dx = tanh(g)*mask*dy ; dgate (fp32 scalar, OVERWRITTEN) =
 * (1-tanh^2 g) * sum(dy * dropout(x)).  workspace >= mmgl_gated_residual_bwd_workspace(n). */
size_t mmgl_gated_residual_bwd_workspace(size_t n);
int mmgl_gated_residual_bwd(const void* dy, const void* x, const float* gate, void* dx, float* dgate,
                            void* workspace, size_t workspace_bytes,
                            size_t n, float p_drop, uint64_t seed, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Linear with fused epilogue:  y[M,N] = act( (x[M,K] @ W[N,K]^T + bias[N]) * out_scale )
 * replaces: nn.Linear q/k/v/out_proj (:194,198-199,273; out_scale = D^-0.5 for q_proj), fc1+ReLU, fc2 (:352-355)
 *   W is torch's nn.Linear layout [out_features, in_features]; bias may be NULL.
 * MFMA: bf16 -> v_mfma_f32_16x16x32_bf16 ; f32 -> v_mfma_f32_16x16x4_f32 (exact fp32 fma chain).
 */
int mmgl_linear_fwd(const void* x, const void* W, const void* bias, void* y,
                    int M, int N, int K, int act, float out_scale, int dtype, void* stream);
/* Whole backward of one linear in a single call: dyp = dy * out_scale * act'(y) is formed once (y = forward OUTPUT; NULL if act
 * none), then dx[M,K] = dyp @ W, dW[N,K] (+)= dyp^T @ x, dbias[N] (+)= colsum(dyp), each in the activation dtype and each
 * optional (NULL); accumulate != 0 adds dW / dbias to the existing contents (gradient accumulation across micro-batches).
 * N must be a multiple of 8; the fp32 path needs dW whenever dbias is requested.
 * mask_dx != 0: x is itself the output of a ReLU (fc2 after fc1+ReLU: the trainable route of ops.relu_ffn) and that ReLU's
 * backward is folded into this call: dx is zeroed where x <= 0 (in the dgrad GEMM's epilogue for the large-shape kernel), so
 * the producing linear can be differentiated with act = none on the already-masked gradient. */
size_t mmgl_linear_bwd_workspace(int M, int N, int K, int act, int dtype);
int mmgl_linear_bwd(const void* dy, const void* y, const void* x, const void* W, void* dx, void* dW, void* dbias,
                    void* workspace, size_t workspace_bytes, int M, int N, int K, int act, float out_scale,
                    int accumulate, int mask_dx, int dtype, void* stream);

/* LoRA-fused linear:  y = x W^T + bias + scale * (x A^T) B^T        A [r,K], Bm [N,r]
 * (peft semantics, lora_dropout = 0; replaces peft's LoRA Linear injected at
 *  model/modelling_self_attention.py:80-87 -- third-party, parity unpinned)
 *   xa [M,r] scratch/output in the activation dtype (saved for backward). */
int mmgl_lora_linear_fwd(const void* x, const void* W, const void* bias, const void* A, const void* Bm,
                         void* y, void* xa, int M, int N, int K, int r, float scale, int dtype, void* stream);
/* dx = dy W + scale * (dy Bm) A ; dA = scale * (dy Bm)^T x ; dB = scale * dy^T xa.  dyb [M,r] scratch/output. */
size_t mmgl_lora_linear_bwd_workspace(int M, int N, int K, int r, int dtype);
int mmgl_lora_linear_bwd(const void* dy, const void* x, const void* xa, const void* W, const void* A,
                         const void* Bm, void* dx, void* dA, void* dB, void* dyb, void* workspace,
                         size_t workspace_bytes, int M, int N, int K, int r, float scale, int accumulate,
                         int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Neighbor interleave: scatter text / image neighbor tokens into slot order + build the key mask.
 * replaces: CrossAttentionModel.forward, modelling_cross_attention.py:1084-1104 (zeros + index_put x4)
 *   text_emb [B,Nt,n_tok*d], vis_emb [B,Ni,n_tok*d] (vis_emb may be NULL with Ni = 0: text_only :1075-1078)
 *   text_loc/img_loc, text_pos/img_pos: int64 [B,Nt] / [B,Ni]
 *   out_emb [B,(Nt+Ni)*n_tok,d] ; out_valid [B,(Nt+Ni)*n_tok] uint8.  Slots nobody writes stay zero/invalid.
 *   Both directions copy whole 16-byte vectors and refuse, before anything is written, an n_tok*d that is no whole number of
 *   16-byte chunks (MMGL_ERR_UNSUPPORTED), n_tok > 256 and an unknown dtype (MMGL_ERR_INVALID).  The backward writes every element of
 *   d_text_emb / d_vis_emb: the gathered slot, or zeros for a neighbor whose location is outside [0, Nt+Ni).
 */
int mmgl_neighbor_interleave_fwd(const void* text_emb, const void* vis_emb, const int64_t* text_loc,
                                 const int64_t* img_loc, const int64_t* text_pos, const int64_t* img_pos,
                                 void* out_emb, uint8_t* out_valid, int B, int Nt, int Ni, int n_tok, int d,
                                 int dtype, void* stream);
int mmgl_neighbor_interleave_bwd(const void* d_out_emb, const int64_t* text_loc, const int64_t* img_loc,
                                 void* d_text_emb, void* d_vis_emb, int B, int Nt, int Ni, int n_tok, int d,
                                 int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Shifted token cross-entropy over [rows, V] logits (mean over rows whose label != ignore_index).
 * replaces: CrossEntropyLoss at modelling_cross_attention.py:831-836 (the shift is done by the caller's
 * pointer arithmetic: row r of `logits` is scored against labels[r]).
 *   loss_sum, count: fp32 device scalars (OVERWRITTEN); row_lse, row_loss [rows] fp32 (row_lse saved for backward).
 *   bwd writes dlogits = (softmax - onehot) * (*dloss_scale) / count, zero on ignored rows.
 *   A label < 0 or >= V counts as ignored.  V may be any positive size (a row that is no whole number of 16-byte chunks takes the
 *   element-wise path).
 *   -inf logits (a logits processor's banned tokens) are allowed where the row keeps at least one finite logit and the label's
 *   logit is finite: they carry no mass, row_lse is that of the finite logits, dlogits is exactly 0 at them.  +inf and NaN are not.
 *   In place: dlogits == logits (the same pointer, the same layout) is allowed -- every element is read and then written by the
 *   same thread and by no other, so no thread sees a gradient where it expects a logit (the LM head scores each chunk of logits
 *   this way).  A partial overlap of the two buffers is not allowed.
 */
int mmgl_cross_entropy_fwd(const void* logits, const int64_t* labels, float* row_lse, float* row_loss,
                           float* loss_sum, float* count, int rows, int V, int64_t ignore_index, int dtype,
                           void* stream);
int mmgl_cross_entropy_bwd(const void* logits, const int64_t* labels, const float* row_lse,
                           const float* count, const float* dloss, void* dlogits,
                           int rows, int V, int64_t ignore_index, int dtype, void* stream);

/* Learned-position ids: pos[b,t] = cumsum(mask)[b,t]*mask[b,t] - 1 + 2
 * replaces: MPTLearnedPositionalEmbedding.forward, modelling_cross_attention.py:135-145 */
int mmgl_position_ids(const int64_t* attention_mask, int64_t* pos, int B, int T, void* stream);

/* Fused AdamW step over a flat parameter bucket (torch.optim.AdamW semantics, run_generation.py:327-330).
 * param/grad in `dtype`; exp_avg/exp_avg_sq fp32; master (fp32 copy of param) may be NULL. grad is read * grad_scale.
 * The bias corrections 1 - beta^step are formed in double from the float betas and rounded once (step >= 1). */
int mmgl_adamw_step(void* param, float* master, const void* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                    float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                    float grad_scale, int dtype, void* stream);

/* Fused Adafactor step over the flat buffers of a data-parallel engine: transformers.optimization.Adafactor.step with beta1 = None,
 * relative_step = scale_parameter = warmup_init = False (run_generation.py:321-324), every tensor of the table in four launches.
 * With g = grad * grad_scale in fp32 and beta2t = 1 - step^decay_rate (formed in double, rounded once, as is its complement):
 *   2-D [R, C]: row_i = beta2t row_i + (1 - beta2t) mean_j(g^2 + eps1); col_j likewise over i;
 *               u = (rsqrt(row_i / mean(row)) * rsqrt(col_j)) * g
 *   1-D:        v = beta2t v + (1 - beta2t)(g^2 + eps1); u = g * rsqrt(v)
 *   both:       u /= max(1, sqrt(mean(u^2)) / clip_threshold); p = p + (-lr weight_decay) p - lr u
 *
 * mmgl_adafactor_workspace: the host-side plan.  segs [n, 4] int64 (host): per tensor its offset in the flat buffers (a multiple of 128,
 *   ascending, no overlap), R, C (C = 0: a 1-D tensor of R elements) and its offset in `state` (row[R] | col[C], or v[R]; ascending, no
 *   overlap).  Returns the workspace bytes of a step and, with table_out != NULL ([n + 1, 8] int64, host), writes the table the kernels
 *   read: the caller copies it to the device once and keeps the host copy.  0 with mmgl_last_error() set: an invalid segment.
 * mmgl_adafactor_step:
 *   param, grad   the flat buffers in `dtype`; master: fp32 copy of param or NULL (param is then stored as its rounding)
 *   state         fp32; table: the planned table on the device, table_host: the same words on the host (the totals are read from it)
 *   workspace     mmgl_adafactor_workspace bytes, 8-byte aligned (the partial sums are doubles); every word a step reads it has written before
 *   No host synchronisation, no allocation, no atomics: reductions in a fixed order, two runs give the same bits.  Elements of the
 *   flat buffers outside the table's tensors are neither read nor written.  The device table is the caller's contract.
 *   step < 1, n < 1, a null pointer, a bad dtype, clip_threshold <= 0, eps1 < 0, decay_rate >= 0, a table that was not planned or a
 *   workspace too small: MMGL_ERR_INVALID, nothing launched. */
size_t mmgl_adafactor_workspace(const int64_t* segs, int n, int64_t* table_out);
int mmgl_adafactor_step(void* param, float* master, const void* grad, float* state, const int64_t* table, const int64_t* table_host,
                        int n, void* workspace, size_t workspace_bytes, float lr, float eps1, float clip_threshold, double decay_rate,
                        float weight_decay, int step, float grad_scale, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Frozen neighbor encoders, forward only (padding-free RoBERTa / CLIP-ViT passes).
 * replaces: the HF encoder calls in get_text_embs / get_visual_embs, modelling_cross_attention.py:978-1027
 * (self.text_model(...), self.visual_model(...)): their attention, residual-add + LayerNorm and activation steps.
 *
 * mmgl_encattn_fwd: bidirectional softmax(QK^T)V over PACKED sequences.  Sequence i owns rows
 *   cu_seqlens[i] .. cu_seqlens[i+1]-1 (int32 device array, nseq+1 entries) of q/k/v [ntok, ld_in] (three column slices
 *   of a fused-QKV GEMM output are fine: ld_in = 3*H*D) and of out [ntok, ld_out]; head h uses columns h*D..h*D+D-1.
 *   q must be pre-scaled by D^-1/2.  max_len = an UPPER BOUND of the longest sequence (host knows it from the packing): it selects
 *   the kernel (bf16, D 64 / 128: the 32x32 kernel up to 4096, the 16x16 one above) and sizes the grid, nothing else -- a larger
 *   value gives the same bits inside one kernel; a sequence longer than max_len gets only its first max_len rows written.
 *   q_rows > 0 = number of leading query rows per sequence to compute (pass max_len for all, 1 for the CLS row only): rows
 *   cu_seqlens[i] + q_rows and later of a sequence are NOT written (the caller's bytes stay), nor are columns H*D .. ld_out-1.
 *   ld_in, ld_out >= H*D, multiples of 8 elements.  No padding token is read.  A sequence of no tokens
 *   (cu_seqlens[i] == cu_seqlens[i+1]) is allowed: both kernels return before any load, nothing is written for it.
 * mmgl_add_layernorm_fwd: s = x + res (rounded to dtype), y = LayerNorm(s); sum_out (may be NULL) receives s; mean, rstd
 *   [rows] fp32 may be NULL (inference).  Also the residual-add + LayerNorm pair of the decoder layers
 *   (modelling_cross_attention.py:334-350: `hidden = residual + h` followed by the next LayerNorm) when they are saved.
 *   p_drop > 0: s = res + dropout(x) (inverted dropout, the counter hash of mmgl_gated_residual_fwd under `seed`).
 * mmgl_add_layernorm_bwd: given dy (grad of y) and dsum (grad arriving on s itself, may be NULL),
 *   dres = LayerNorm'(dy) + dsum; with p_drop == 0 that is also the gradient of x (dx ignored, may be NULL), otherwise
 *   dx = dres * keep / (1 - p).  dgamma/dbeta fp32 optional (workspace as for mmgl_layernorm_bwd).
 * mmgl_activation_fwd: y = act(x) elementwise, in place allowed; act 1 relu, 2 gelu (erf), 3 quick_gelu, 4 gelu (tanh).
 */
/* General NT GEMM with fused epilogue (the frozen path's linears, their dgrads, lm_head, the encoder linears):
 *   y[M,N] = act( (x[M,K] @ W[N,K]^T + bias[N]) * out_scale )   then   y = (zmask > 0 ? y : 0)   then   y += residual
 * replaces: nn.Linear inside the frozen MPTDecoderLayer / MPTAttention (model/modelling_cross_attention.py:194-199, :273,
 *           :352-355), lm_head (:826), the RobertaModel / CLIPVisionModel linears behind :992 / :1018, and autograd's
 *           dgrad of each of them (dx = dy @ W  ==  an NT GEMM against the cached W^T; zmask = the ReLU output whose
 *           backward is folded into the epilogue).
 *   bias [N], residual [M,N], zmask [M,N] may be NULL; act: 0 none, 1 relu, 2 gelu (erf), 3 quick_gelu, 4 gelu (tanh).
 * bf16 shapes with K % 128 == 0, K >= 256, N % 16 == 0 and enough 256x256 tiles run on the persistent ping-pong kernel
 * (gemm8p.hip; mmgl_gemm_nt_fast returns 1), other bf16 shapes with K % 64 == 0, N % 8 == 0 on the 128x128 kernel (gemm_mid.hip;
 * returns 2): both take strided operands and apply the whole epilogue in the kernel.  Anything else (returns 0) runs on gemm.hip's
 * dense 128x128 kernel followed by the elementwise kernels.  mmgl_linear_fwd and the LoRA linears (no K-split scratch: the
 * persistent kernel from a full chip of tiles on) and mmgl_linear_bwd's dgrad follow the same plan (gemm.hip: nt_route).
 * ldx / ldw / ldy: row strides in elements (residual and zmask share ldy); the composed path needs dense operands.
 * K may exceed ldx by less than 128 when columns ldx.. of W are zero (a contraction length padded to the kernels' K step: the
 * lm_head dgrad over a 50272-entry vocabulary): the tail of row r of x then reads the head of row r + 1 (nothing is read past
 * the last row: the buffer descriptor zero-fills).  PRECONDITION of that form: x finite -- 0 * Inf = NaN, so a non-finite element
 * at the head of row r + 1 would also poison row r of the output.
 * mmgl_relu_bwd: out = dy * (y > 0), the backward of a stand-alone ReLU epilogue (in place allowed). */
int mmgl_gemm_nt_fast(int M, int N, int K, int ldx, int ldw, int ldy, int dtype);
/* workspace: shapes with fewer 256x256 output tiles than the chip has CUs and a long contraction (the reference's batch of 4:
 * M = 2560, K >= 3072), and the last partial round of tiles of a one-to-three-round output (2560 x 8192: 320 tiles on 256 CUs),
 * are cut into K-split work items whose fp32 partial tiles live in caller memory, like every other
 * scratch of this library (no allocation inside).  mmgl_gemm_nt_workspace returns the bytes that takes (0 for every other
 * shape); with workspace == NULL or fewer bytes the same kernel runs unsplit (same result up to fp32 summation order). */
size_t mmgl_gemm_nt_workspace(int M, int N, int K, int ldx, int ldw, int ldy, int dtype);
int mmgl_gemm_nt(const void* x, int ldx, const void* W, int ldw, const void* bias, const void* residual, const void* zmask,
                 void* y, int ldy, int M, int N, int K, int act, float out_scale, void* workspace, size_t workspace_bytes,
                 int dtype, void* stream);
int mmgl_relu_bwd(const void* dy, const void* y, void* out, size_t n, int dtype, void* stream);
/* mmgl_gemm_nt_rowk: y[M,N] = x[M,K] W[N,K]^T (bf16, no epilogue) on the persistent 256x256 kernel, where only the 256-row tiles
 * that hold a row below m_full contract over all of K; the tiles behind them contract over the first K_short columns and never
 * read x[.., K_short..K) -- which the caller knows to be zero there (it may be uninitialised from row ceil(m_full / 256) * 256 on).
 * One launch, no K splits, no scratch, at any tile count; every output element is the sum mmgl_gemm_nt without K-split workspace
 * forms, minus a tail of exact zeros.  K, K_short multiples of 128, 256 <= K_short <= K, N a multiple of 16, 0 <= m_full <= M;
 * anything else returns MMGL_ERR_UNSUPPORTED / MMGL_ERR_INVALID.  Tiles are handed out so that no workgroup's K steps exceed the
 * mean by more than one long tile; under the dynamic tile schedule (below) long tiles first.
 * mmgl_gemm_nt_rowk_item: that static schedule for tests -- the it-th work item of workgroup wg of G for n_long + n_short tiles,
 * q = K / K_short: a long tile's index, n_long + a short tile's index, or -1. */
int mmgl_gemm_nt_rowk(const void* x, int ldx, const void* W, int ldw, void* y, int ldy, int M, int N, int K, int K_short,
                      int m_full, int dtype, void* stream);
int mmgl_gemm_nt_rowk_item(int G, int n_long, int n_short, int q, int wg, int it);
/* Dynamic tile schedule of the persistent bf16 GEMM kernel behind mmgl_gemm_nt / _relu_bits / _masked / mmgl_linear_*.
 * replaces: nothing in the reference -- it is what lets those GEMMs share the GPU with the gradient all-reduce that
 *   DistributedDataParallel overlaps with the backward pass (language_modelling/run_generation.py:317-319, 485): with the default
 *   static schedule (tile i * grid + workgroup) a workgroup whose CU is shared with the collective's kernel finishes its tiles
 *   late and the whole GEMM waits for it (+38 % measured); with a counter, workgroups take tiles as they become free.
 *   counter: DEVICE pointer to 16 uint32, all zero, owned by the caller and left all zero by every launch; NULL (the default)
 *   = static schedule.  The setting belongs to the CURRENT DEVICE (hipGetDevice of the caller), process-wide: it also applies to
 *   launches from other host threads -- autograd runs the backward GEMMs, the ones that overlap the collective, on its own device
 *   thread.  The counters serve ONE stream per device: the first persistent-GEMM launch after this call binds them to its stream,
 *   and a launch of that device on any other stream while they are set returns MMGL_ERR_INVALID (two launches in flight would hand
 *   out each other's tiles); setting the counter again (or NULL) releases the binding.
 *   mmgl_gemm_get_tile_counter: the current device's counter (NULL: static schedule). */
int mmgl_gemm_set_tile_counter(void* counter);
void* mmgl_gemm_get_tile_counter(void);
/* The ReLU mask of a frozen FFN as bits (replaces: keeping relu(fc1(x)) [M, ffn] for autograd's threshold_backward of
 * model/modelling_cross_attention.py:352-355, and re-reading it in fc2's dgrad).
 *   mmgl_gemm_nt_relu_bits: y = relu((x W^T + bias) * out_scale) as mmgl_gemm_nt with act = 1, plus bits_out: one bit per
 *     output element (y > 0), mmgl_gemm_nt_relu_bits_bytes() bytes of caller memory (8 KiB per 256 x 256 output tile).
 *   mmgl_gemm_nt_masked: y = (x W^T) * out_scale where the bit of that element is set, 0 elsewhere -- fc2's dgrad with fc1's
 *     ReLU backward folded in, reading 16 bytes of mask per lane and tile instead of the [M, ffn] activation.
 * The bits are private to the persistent kernel's tile -> lane mapping: write and apply them with the same M and N.
 * mmgl_gemm_nt_relu_bits_bytes returns 0 for shapes / dtypes that do not run as whole tiles of that kernel (then use
 * mmgl_gemm_nt with act = 1 and its zmask argument instead). */
size_t mmgl_gemm_nt_relu_bits_bytes(int M, int N, int K, int ldx, int ldw, int ldy, int dtype);
int mmgl_gemm_nt_relu_bits(const void* x, int ldx, const void* W, int ldw, const void* bias, void* y, int ldy, void* bits_out,
                           int M, int N, int K, float out_scale, int dtype, void* stream);
int mmgl_gemm_nt_masked(const void* x, int ldx, const void* W, int ldw, const void* bits_in, void* y, int ldy, int M, int N, int K,
                        float out_scale, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Elementwise pieces of frozen Llama-family decoder layers (BASELINE.json config 5; the reference's fork is OPT-only,
 * model/modelling_cross_attention.py:278-375, so these follow transformers' LlamaDecoderLayer loaded through the same HF API).
 * mmgl_rope_inplace: rotary embedding of the first `nblk` column blocks (H heads x D each: q, then k) of buf [rows, ld], row r
 *   at position r % T; cos_sin [T, D/2, 2] fp32 (cos, sin); rotate_half convention; backward != 0 applies the transpose
 *   rotation (the gradient of the forward one).  In place.
 * mmgl_rope: the same from src into dst (src != dst, same [rows, ld] layout); column blocks nblk .. nall-1 (v of a fused
 *   q | k | v buffer) are copied unrotated -- the backward of the rotation without touching the gradient buffer autograd owns.
 * mmgl_swiglu_fwd: y[M,F] = silu(gate_up[:, :F]) * gate_up[:, F:]   (gate_up = one fused [gate | up] GEMM output [M, 2F]).
 * mmgl_swiglu_bwd: dgate_up[M,2F] from dy[M,F] and the saved gate_up. */
int mmgl_rope_inplace(void* buf, const float* cos_sin, size_t rows, int T, int H, int D, int ld, int nblk, int backward,
                      int dtype, void* stream);
int mmgl_rope(const void* src, void* dst, const float* cos_sin, size_t rows, int T, int H, int D, int ld, int nblk, int nall,
              int backward, int dtype, void* stream);
int mmgl_swiglu_fwd(const void* gate_up, void* y, size_t M, int F, int dtype, void* stream);
int mmgl_swiglu_bwd(const void* dy, const void* gate_up, void* dgate_up, size_t M, int F, int dtype, void* stream);

int mmgl_encattn_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens, void* out, int nseq,
                     int H, int D, int ld_in, int ld_out, int max_len, int q_rows, int dtype, void* stream);
int mmgl_add_layernorm_fwd(const void* x, const void* res, const void* gamma, const void* beta, void* sum_out,
                           void* y, float* mean, float* rstd, int rows, int cols, float eps, float p_drop, uint64_t seed,
                           int dtype, void* stream);
int mmgl_add_layernorm_bwd(const void* dy, const void* dsum, const void* sum, const void* gamma, const float* mean,
                           const float* rstd, void* dres, void* dx, float* dgamma, float* dbeta, void* workspace,
                           size_t workspace_bytes, int rows, int cols, float p_drop, uint64_t seed, int dtype,
                           void* stream);
/* The LayerNorm in front of a frozen layer's self-attention when only the live key tiles are projected to keys and values
 * (mmgl_selfattn_tiles_*).  mmgl_layernorm_tiles_fwd / mmgl_add_layernorm_tiles_fwd are mmgl_layernorm_fwd / mmgl_add_layernorm_fwd
 * (same y, sum_out, mean, rstd, same dropout hash, keyed by the full row index) plus a compact copy: row r of y is also stored to
 * row rowmap[r] of yc [crows, cols] when 0 <= rowmap[r] < crows.  rowmap [rows] int32 maps every row of a live 64-key tile,
 * its padding rows included, to its compact row and every other row to -1.  yc is a copy for the frozen K | V projection, whose
 * gradient reaches y through the dense fused dgrad: the backward is mmgl_layernorm_bwd / mmgl_add_layernorm_bwd as it is. */
int mmgl_layernorm_tiles_fwd(const void* x, const void* gamma, const void* beta, void* y, void* yc, const int32_t* rowmap,
                             float* mean, float* rstd, int rows, int cols, int crows, float eps, int dtype, void* stream);
int mmgl_add_layernorm_tiles_fwd(const void* x, const void* res, const void* gamma, const void* beta, void* sum_out, void* y,
                                 void* yc, const int32_t* rowmap, float* mean, float* rstd, int rows, int cols, int crows,
                                 float eps, float p_drop, uint64_t seed, int dtype, void* stream);
/* mmgl_add_layernorm_rows_bwd: mmgl_add_layernorm_bwd with dy read through a row map: the gradient of row r of y is row dy_rows[r]
 * of dy (dy_rows [rows] int32, every entry in [0, rows)) -- the live-first row order in which mmgl_selfattn_tiles_rows_bwd and
 * mmgl_gemm_nt_rowk leave the gradient of a frozen layer's normed input.  Everything else -- sum, mean, rstd, dsum, dres, dx, the
 * dropout counters -- keeps the dense row, and every output is bitwise that of mmgl_add_layernorm_bwd on the un-permuted dy. */
int mmgl_add_layernorm_rows_bwd(const void* dy, const int32_t* dy_rows, const void* dsum, const void* sum, const void* gamma,
                                const float* mean, const float* rstd, void* dres, void* dx, float* dgamma, float* dbeta,
                                void* workspace, size_t workspace_bytes, int rows, int cols, float p_drop, uint64_t seed,
                                int dtype, void* stream);
int mmgl_activation_fwd(const void* x, void* y, size_t n, int act, int dtype, void* stream);
/* y[i] = x[i] * (*scale), product in fp32, scale read from device memory (x == y allowed).  The upstream gradient of a scalar
 * loss -- `loss / args.grad_accumulation_steps` at reference language_modelling/run_generation.py:483 -- applied to a saved
 * gradient without a host sync. */
int mmgl_scale(const void* x, const float* scale, void* y, size_t n, int dtype, void* stream);

/* ---- gradient exchange over RCCL (xGMI) --------------------------------------------------------------------------------
 * replaces: the NCCL process group behind the reference's data-parallel wiring -- language_modelling/run_generation.py:283
 *   (dist.init_process_group("nccl")), :317-319 (DistributedDataParallel: the constructor's parameter broadcast and the bucketed
 *   gradient all-reduce of every backward pass, :485), language_modelling/utils.py:113-118 (AverageMeter.all_reduce),
 *   run_generation.py:608-616 (all_gather of the evaluation predictions).  One process per GPU; single node, like the reference.
 *   mmgl_comm_unique_id: rank 0 fills 128 bytes (ncclUniqueId) and hands them to the other ranks out of band (file, socket, env).
 *   mmgl_comm_init: every rank, with its HIP device current, joins the communicator of that id; *comm is the handle.
 *   mmgl_allreduce_sum: buf[count] <- sum over ranks, in place, on `stream` (averaging: fold 1/world into mmgl_adamw_step's
 *     grad_scale).  mmgl_allgather: out[world * count_per_rank] <- every rank's in[count_per_rank], rank order.
 *   mmgl_broadcast: buf[count] of `root` to every rank (DDP's constructor broadcast).  mmgl_comm_destroy: frees the handle.
 *   dtype: MMGL_F32, MMGL_BF16 or MMGL_COMM_I64 (token ids of the eval gather).  Collectives of one communicator must be issued
 *   in the same order on every rank (mmgl_amd.distributed.DataParallelEngine issues its buckets in index order).
 *   RCCL is resolved at run time (the librccl.so the process already holds, else the system's); without it these six return
 *   MMGL_ERR_UNSUPPORTED and every other entry point is unaffected.  mmgl_amd's own trainer reaches the same RCCL through
 *   torch.distributed's "nccl" backend; these are the calls for a host program that has no torch.distributed. */
enum { MMGL_COMM_I64 = 2 };
int mmgl_comm_unique_id(void* out128);
int mmgl_comm_init(int rank, int world, const void* unique_id, void** comm);
int mmgl_allreduce_sum(void* comm, void* buf, size_t count, int dtype, void* stream);
int mmgl_allgather(void* comm, const void* in, void* out, size_t count_per_rank, int dtype, void* stream);
int mmgl_broadcast(void* comm, void* buf, size_t count, int dtype, int root, void* stream);
int mmgl_comm_destroy(void* comm);

/* ---------------------------------------------------------------------------------------------
 * Greedy generation with a key/value cache: the kernels of a decode step (csrc/decode.hip).
 * replaces: the sequential generation of the test protocol, language_modelling/run_generation.py:597-603
 *   (model.module.generate(..., max_new_tokens=32)), which the reference's wrappers cannot serve: its self-attention
 *   returns no cache (model/modelling_cross_attention.py:372), the decoder collects none (:629) and the causal LM hands
 *   past_key_values = None on (:851-870).  Forward only.
 *
 * mmgl_gemm_skinny: y[M,N] = act((x[M,K] . W[N,K]^T + bias) * scale) + residual for 1 <= M <= 64 rows -- every linear of a decode
 *   step (q, k|v, out_proj, fc1 + ReLU, fc2, lm_head on the last row).  x, W, y row-major with unit column stride and row strides
 *   ldx, ldw, ldy; ldy may be a whole cache row (the k|v projection writes column `t` of the cache in place).  bias [N] and
 *   residual [M, ldy] may be NULL.  act: MMGL_ACT_NONE / MMGL_ACT_RELU.  bf16 with K % 64 == 0, N % 8 == 0 and 16-byte aligned
 *   rows streams W from HBM once into MFMA fragments; every other shape, and fp32, runs a plain one-wave-per-column kernel.
 *   Deterministic (fixed-order fold of the K partials, no atomics).  M > 64: MMGL_ERR_UNSUPPORTED -- chunk the rows or call mmgl_gemm_nt.
 *
 * mmgl_attn_decode_fwd: out[b, h*D..] = softmax(q[b, h] . K[b, :, h]^T masked) V[b, :, h], one query row per (batch, head).
 *   q         [B, H*D] row stride ldq, already scaled by D^-0.5
 *   k, v      S rows of H*D per sample, row stride ldkv, sample stride batch_stride_kv (elements): column slabs of the cache rows
 *             [B, capacity, 2 H D], or the projected neighbor tokens [B, S, H*D]
 *   key_valid [B, S] uint8 with row stride ld_valid, 1 = attend.  Causality is the caller's: a cache holds only keys at or before
 *             the query.  A sample with no valid key gets the uniform distribution over its S keys (as mmgl_xattn_fwd).
 *   out       [B, H*D] dense
 *   D in {16,32,64,128} (those of mmgl_xattn_fwd); any S >= 1; strides multiples of 16 bytes.  fp32 softmax.
 *
 * mmgl_gemm_skinny_lora: y[M,N] = act((x . W^T + bias + lora_scale * (x . A^T) . B^T) * scale) + residual -- mmgl_gemm_skinny for a
 *   projection that carries a LoRA adapter (q_proj / v_proj of model/modelling_self_attention.py's LoRALinear; the training forward
 *   is mmgl_lora_linear_fwd).  lora_A [r, K] row stride lda, lora_B [N, r] row stride ldb, 1 <= r <= 256 (> 256: MMGL_ERR_UNSUPPORTED);
 *   x, W, bias, residual, y, act, scale, the dtypes and the M <= 64 limit as mmgl_gemm_skinny (ldy free: v goes into its cache
 *   column in place).  workspace: M * r floats owned by the caller, 4-byte aligned; on return it holds t = x . A^T in fp32.
 *   Two launches: t (fp32, never rounded to the storage type), then the kernels of mmgl_gemm_skinny with sum_j t[m,j] B[n,j] added in
 *   fp32 to the folded K sum, in front of bias, scale, activation and residual.  W is not modified and no merged copy of it is
 *   built.  Any r works on either kernel; deterministic (no atomics). */
int mmgl_gemm_skinny_lora(const void* x, int ldx, const void* W, int ldw, const void* bias, const void* residual, void* y, int ldy,
                          const void* lora_A, int lda, const void* lora_B, int ldb, int r, float lora_scale, void* workspace,
                          int M, int N, int K, int act, float scale, int dtype, void* stream);
int mmgl_gemm_skinny(const void* x, int ldx, const void* W, int ldw, const void* bias, const void* residual, void* y, int ldy,
                     int M, int N, int K, int act, float scale, int dtype, void* stream);
int mmgl_attn_decode_fwd(const void* q, int ldq, const void* k, const void* v, int ldkv, size_t batch_stride_kv,
                         const uint8_t* key_valid, int ld_valid, void* out, int B, int H, int S, int D, int dtype, void* stream);

/* The decode step of the Llama-family LM (model/modelling_llama_cross_attention.py: LlamaNeighborLM.generate): a key/value cache of
 * Hkv <= H heads and a rotary embedding at one position.  No reference counterpart (its fork is OPT-only).  Forward only.
 *
 * mmgl_attn_decode_gqa_fwd: mmgl_attn_decode_fwd over Hkv key/value heads: query head h reads key / value head h / (H / Hkv)
 *   (transformers' repeat_kv, the mapping of mmgl_selfattn_gqa_*).
 *   q, out    [B, H*D] (q: row stride ldq, already scaled by D^-0.5; out dense)
 *   k, v      S rows of Hkv*D per sample, row stride ldkv, sample stride batch_stride_kv (elements): column slabs of the cache rows
 *             [B, capacity, 2 Hkv D].  Nothing is expanded to H heads in memory.
 *   key_valid [B, S] uint8, row stride ld_valid; a sample with no valid key attends uniformly over its S keys.
 *   One workgroup per (sample, key/value head, block of at most 8 query heads of its group): each 16-byte K / V load is issued once
 *   and used for every query head of the block; a group of more than 8 heads takes further blocks (12 = 6 + 6).  Softmax and
 *   accumulation in fp32, partial states merged in a fixed order (no atomics: deterministic).  The S keys of a sample are not split
 *   over workgroups.  D in {16,32,64,128} (else MMGL_ERR_UNSUPPORTED); Hkv any divisor of H (else MMGL_ERR_INVALID); any S >= 1;
 *   strides multiples of 16 bytes, q / k / v 16-byte aligned.
 *
 * mmgl_rope_kv_append: the new token's row of the fused q | k | v projection, rotated and filed in one launch.
 *   qkv         [B, (H + 2 Hkv) * D], row stride ldqkv: the H query heads are rotated IN PLACE; the k and v blocks are only read
 *   cos_sin_row fp32 [D/2, 2] (cos, sin): the row of the position's angles of the table mmgl_rope_inplace takes; rotate_half
 *               convention and the arithmetic of mmgl_rope_inplace
 *   kv_col      the cache column of the new token: sample b's rotated Hkv key heads and unrotated Hkv value heads go to
 *               kv_col[b * batch_stride_kv + 0 .. 2 Hkv D)
 *   D in {16,32,64,128}; strides multiples of 16 bytes; qkv and kv_col 16-byte aligned. */
int mmgl_attn_decode_gqa_fwd(const void* q, int ldq, const void* k, const void* v, int ldkv, size_t batch_stride_kv,
                             const uint8_t* key_valid, int ld_valid, void* out, int B, int H, int Hkv, int S, int D, int dtype,
                             void* stream);
int mmgl_rope_kv_append(void* qkv, int ldqkv, const float* cos_sin_row, void* kv_col, size_t batch_stride_kv, int B, int H, int Hkv,
                        int D, int dtype, void* stream);

/* Beam search on a beam-shared key/value cache (generate(num_beams = W), 1 <= W <= 8; csrc/decode.hip, csrc/beam.hip).
 * replaces: HuggingFace generate(num_beams=W) behind the reference's test protocol (language_modelling/run_generation.py:597-603),
 *   which repeats the prompt W times and reorders whole cache rows at every step.  Forward only; deterministic (no atomics).
 *
 * mmgl_attn_decode_beam_fwd: single-query attention for the R = B*W rows of a beam step; row b*W + w is beam slot w of sample b.
 *   q, out      [B*W, H*D] (q: row stride ldq, already scaled by D^-0.5; out dense)
 *   k_pre,v_pre S_pre >= 1 rows of H*D per SAMPLE, row stride ld_pre, sample stride batch_stride_pre (elements), and
 *   key_valid   [B, S_pre] uint8, row stride ld_valid: exactly the k / v / key_valid of mmgl_attn_decode_fwd -- the prompt's cache
 *               rows [B, T, 2 H D] or the projected neighbor tokens.  Read once per (sample, head) and scored against the W queries.
 *   k_tail,v_tail column slabs of the tail buffer [B*W, n_cap, 2 H D]: column stride ld_tail, row stride row_stride_tail (elements);
 *               n_tail >= 0 columns are in use.  The keys the hypotheses generated themselves; always valid.
 *   src         int32 [B*W, n_cap], row stride ld_src: tail key j of row (b, w) is row b*W + src[b*W + w][j], column j, of the
 *               tail buffer.  Values lie in [0, W).  A table in host-visible memory is checked here (MMGL_ERR_INVALID); a device table
 *               is the caller's contract: the kernel clamps a value into [0, W) (a wrong beam's key, never an access outside the
 *               sample's W rows) and asserts nothing.
 *   n_tail = 0 is the cross-attention call: k_tail, v_tail and src may be NULL.
 *   A masked prefix key scores -FLT_MAX.  A sample whose prefix has NO valid key is uniform over all its S_pre + n_tail keys
 *   (the tail keys then weigh as the masked ones do), so n_tail = 0 gives mmgl_attn_decode_fwd's uniform distribution.
 *   One workgroup per (sample, head); W in {1, 2, 4, 8} instantiations, W = 3, 5, 6, 7 run the next size up with the surplus rows
 *   computed and not stored; W > 8: MMGL_ERR_UNSUPPORTED.  D in {16,32,64,128}; strides multiples of 16 bytes; q, k_*, v_* 16-byte
 *   aligned; a sample's prefix rows and its W tail rows each span less than 2 GiB.  fp32 softmax, partial states merged in a fixed order.
 *
 * mmgl_beam_topk: per sample the 2W best of its rows_in * V candidates score = beam_score[row] + (logit[row][v] - logsumexp(row)),
 *   fp32, sorted descending; an exact tie goes to the lower flat index r*V + v (r: the row's slot in its sample).
 *   logits      [B*rows_in, V] bf16 / fp32, row stride ld_logits (elements); rows_in = 1 (the prefill's row per sample) or W
 *   beam_score  fp32 [B*rows_in];  cand_score fp32 [B, 2W];  cand_index int32 [B, 2W] (flat indices)
 *   workspace   mmgl_beam_topk_workspace(B*rows_in, V, W) bytes, 4-byte aligned: per (row, chunk of 4096 logits) the chunk's
 *               (max, sum exp) and its 2W best logits -- no [rows, V] intermediate.  Two launches.
 *   Any V >= 2W with rows_in * ceil(V / 4096) * 2W <= 4096 candidates after the first launch (V <= 131072 at W = 8, rows_in = 8;
 *   else MMGL_ERR_UNSUPPORTED).  Within a row candidates are ordered by logit (two logits that round to one score keep that order).
 *
 * mmgl_beam_advance: one launch, one wave per sample: the sorted candidates of step s become the state of step s + 1.
 *   tokens int64 / parents int32 / beam_score fp32 [B*W]: the next running beams = the first W candidates whose token is not
 *               eos_token_id (< 0: none), in candidate order; score copied.
 *   src_old -> src_new (int32 [B*W, ld_src], different buffers): new[w][0..n_cols-1) = old[parent][0..n_cols-1),
 *               new[w][n_cols-1] = parent; columns >= n_cols are not written.  n_cols = s: the tail columns the parents own.
 *   pool_*_old -> pool_*_new ([B*W] score fp32 / len int32 / tok int64, anc int32 [B*W, ld_src]; different buffers): the finished
 *               hypotheses of a sample, the W best sorted descending (ties: older entry first, then candidate order); len = 0 and
 *               score = -inf mark an empty slot.  A candidate among the first W that is EOS, or any of the first W when last_step
 *               is set, enters with score = cand_score / length_divisor (the caller passes (s + 1)^length_penalty as fp32: one IEEE
 *               division), len = n_cols + 1, its ancestry row (old[parent][0..n_cols-1), parent) and its token -- unless the sample
 *               is frozen: done[b] is set, or early_stopping and its pool was full before this step.
 *   done        int32 [B]: set once the pool is full and NOT best_running_score / length_divisor > worst pooled score (the
 *               early-stop heuristic of transformers' beam search, early_stopping in {False, True}); never cleared.
 *   Plain vector stores only. */
size_t mmgl_beam_topk_workspace(int rows, int V, int W);
int mmgl_attn_decode_beam_fwd(const void* q, int ldq, const void* k_pre, const void* v_pre, int ld_pre, size_t batch_stride_pre,
                              const uint8_t* key_valid, int ld_valid, const void* k_tail, const void* v_tail, int ld_tail,
                              size_t row_stride_tail, const int* src, int ld_src, void* out, int B, int W, int H, int S_pre, int n_tail,
                              int D, int dtype, void* stream);
int mmgl_beam_topk(const void* logits, size_t ld_logits, const float* beam_score, float* cand_score, int* cand_index, void* workspace,
                   size_t workspace_bytes, int B, int rows_in, int W, int V, int dtype, void* stream);
int mmgl_beam_advance(const float* cand_score, const int* cand_index, int64_t* tokens, int* parents, float* beam_score,
                      const int* src_old, int* src_new, int ld_src, const float* pool_score_old, float* pool_score_new,
                      const int* pool_len_old, int* pool_len_new, const int* pool_anc_old, int* pool_anc_new,
                      const int64_t* pool_tok_old, int64_t* pool_tok_new, int* done, int B, int W, int V, int n_cols, int eos_token_id,
                      int last_step, int early_stopping, float length_divisor, void* stream);

/* ---- sampling (generate(do_sample=True)): temperature, top-k, top-p and the draw, one launch --------------------------------------
 * replaces: transformers' TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper (min_tokens_to_keep = 1) -> softmax ->
 *           multinomial, and the where / full_like / == / | / setitem tail of the greedy loops
 *
 * mmgl_sample_tokens: per row of logits [rows, V] (bf16 / fp32, row stride ld_logits elements) n_draws tokens.
 *   x = logit / temperature in fp32 (a NaN logit counts as -inf).
 *   top-k  (top_k = 0 or >= V: off): v survives iff fewer than top_k tokens have x > x_v -- every token tied with the k-th is kept.
 *   top-p  (top_p = 1: off): with p = softmax(x) over the survivors, v is kept iff the mass of the survivors with x > x_v is < top_p;
 *          every token tied with the boundary is kept; the largest logit is always kept.
 *   draw   u fp32 [rows, n_draws] in [0, 1): the smallest kept v, in vocabulary index order, whose running mass over the kept set
 *          exceeds u * Z_K.  Always in [0, V).
 *   Masses are the integers trunc(2^40 * expf(x - max x)), summed as integers: no sum depends on an order, two runs are bitwise equal.
 *   tokens   int64, draw i = row * n_draws + j is written to tokens[i * token_stride] (a column of an ids tensor)
 *   finished optional uint8 [rows * n_draws], read and written: a finished draw gets pad_token_id; a draw that returns eos_token_id
 *            (< 0: none) becomes finished
 *   kept     optional int32 [rows]: the size of the kept set
 *   V <= 131072 and n_draws <= 8, else MMGL_ERR_UNSUPPORTED; temperature > 0, top_k >= 0, 0 < top_p <= 1.  A refused call writes nothing.
 *   One workgroup per row, no workspace, no host synchronisation.  Plain vector stores only. */
int mmgl_sample_tokens(const void* logits, size_t ld_logits, const float* u, int64_t* tokens, int64_t token_stride, uint8_t* finished,
                       int* kept, int rows, int n_draws, int V, float temperature, int top_k, float top_p, int eos_token_id,
                       int64_t pad_token_id, int dtype, void* stream);

/* ---- logits processors (generate(repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens)), one launch ----------
 * replaces: transformers' RepetitionPenaltyLogitsProcessor -> NoRepeatNGramLogitsProcessor -> MinNewTokensLengthLogitsProcessor ->
 *           SuppressTokensLogitsProcessor (three to five aten launches each, on [rows, V] or [rows, L] intermediates)
 *
 * mmgl_logits_process: rewrites, in place, at most hist_len + n_ban elements per row of logits [rows, V] (bf16 / fp32, row stride
 * ld_logits >= V elements).  The row's history h[0..L) is the row of `history` (int64 [rows, hist_len], ANY row stride ld_history
 * in elements, 0 and strided views included) with the columns c < n_masked whose hist_valid[row * ld_valid + c] is 0 removed;
 * columns from n_masked on are always valid.  hist_valid may be NULL with n_masked = 0, history may be NULL with hist_len = 0.
 * On x = the row, in this order:
 *   1. repetition_penalty p (1: off): for every DISTINCT token t of the history, x[t] = x[t] * p if x[t] < 0 else x[t] / p, in fp32
 *      (one IEEE division), rounded once to the logits' dtype.  A token that occurs several times is penalised once.
 *   2. no_repeat_ngram_size n (0: off): with pre = h[L-n+1 .. L) (empty for n = 1), x[h[i+n-1]] = -inf for every i in [0, L-n]
 *      with h[i .. i+n-1) == pre.  Nothing while L < n.
 *   3. x[t] = -inf for the n_ban tokens of `ban` (int32, device memory; NULL with n_ban = 0).  -inf wins over a penalised value.
 * A history or ban token outside [0, V) is never an address; such a history token keeps its place in the sequence and equals
 * nothing, so an n-gram that contains it neither matches nor bans.  Every other logit, and the columns between V and ld_logits, keep
 * their bits.  Two runs are bitwise equal.
 *   hist_len <= 8192, n_ban <= 64, V <= 131072, else MMGL_ERR_UNSUPPORTED.  MMGL_ERR_INVALID: a null pointer, rows <= 0, ld_logits < V,
 *   a non-positive or non-finite penalty, negative n / n_ban / n_masked / hist_len, n_masked > hist_len, a bad dtype.  A refused call
 *   writes nothing; a call with everything off (p = 1 and n = 0, or hist_len = 0, and n_ban = 0) launches nothing.
 *   One workgroup per row, no workspace, no atomics on global memory, no host synchronisation.  Plain vector stores only. */
int mmgl_logits_process(void* logits, size_t ld_logits, const int64_t* history, size_t ld_history, const uint8_t* hist_valid,
                        size_t ld_valid, int n_masked, int hist_len, const int* ban, int n_ban, int rows, int V,
                        float repetition_penalty, int no_repeat_ngram_size, int dtype, void* stream);

/* ---- neighbor guidance (generate(guidance_scale = g); csrc/guidance.hip), one launch -----------------------------------------------
 * replaces: transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor arithmetic -- log_softmax of the conditional and of the
 *           unconditional logits and their combination, three aten launches and two [rows, V] fp32 intermediates.
 *
 * mmgl_guidance_logits: logits [2 * batch, V] (bf16 / fp32, row stride ld_logits >= V elements, any alignment).  Rows b and batch + b
 * are a pair: row b the logits with neighbors, row batch + b those of the same tokens without the gated layers.  With
 * lc = log_softmax(row b), lu = log_softmax(row batch + b) in fp32 (a NaN logit counts as -inf), row b is rewritten in place with
 *   lu + guidance_scale * (lc - lu)
 * evaluated in fp32 and rounded once to the logits' dtype.  Where the conditional logit is -inf the result is -inf; where only the
 * unconditional one is, the result is lc.  A row without any finite logit is outside the contract: nothing faults, what is stored is
 * unspecified.  Rows batch .. 2 batch - 1, the columns between V and ld_logits and everything else keep their bits.
 * Both log-sum-exps are reduced in a fixed order (a thread's elements in index order, a wave butterfly, the waves in order): two
 * runs are bitwise equal.
 *   V <= 131072, else MMGL_ERR_UNSUPPORTED.  MMGL_ERR_INVALID: a null pointer, batch <= 0, V <= 0, ld_logits < V, a bad dtype, a
 *   guidance_scale that is negative or not finite.  A refused call writes nothing.
 *   One workgroup per pair, no workspace, no atomics, no host synchronisation.  Plain vector stores only. */
int mmgl_guidance_logits(void* logits, size_t ld_logits, int batch, int V, float guidance_scale, int dtype, void* stream);

/* ---- prompt-lookup decoding (generate(prompt_lookup_num_tokens = K), 1 <= K <= 7; csrc/decode.hip, csrc/lookup.hip) ---------------
 * replaces: transformers' PromptLookupCandidateGenerator + the assisted-decoding verification behind generate(
 *           prompt_lookup_num_tokens=K), which re-runs a [B = 1, K + 1] forward through the dynamic cache and crops it afterwards.
 *           Forward only; deterministic (no atomics).
 *
 * mmgl_attn_decode_block_fwd: causal attention of m = K + 1 <= 8 new tokens per sample against a cache whose length differs per
 * sample, and the filing of the new keys / values into that cache, one launch; row b*m + i is new token i of sample b.
 *   q, out      [B*m, H*D] (q: row stride ldq, already scaled by D^-0.5; out dense)
 *   k_new,v_new [B*m, H*D], row stride ld_new: the keys / values of the new tokens (the halves of a dense [B*m, 2 H D] projection)
 *   k, v        the cache slabs: `capacity` rows of H*D per sample, row stride ldkv, sample stride batch_stride_kv (elements)
 *   key_valid   [B, capacity] uint8, row stride ld_valid
 *   len         int32 [B], device memory: the columns sample b has filed.  Clamped into [0, capacity] by the kernel; keeping it
 *               there is the caller's contract (as src of mmgl_attn_decode_beam_fwd).
 *   Row (b, i) attends the cache columns s < len[b] with key_valid set and the new keys j <= i (always valid).  New key / value j
 *   is written to cache column len[b] + j when that column is below `capacity`, else dropped (it belongs to an input whose output
 *   the caller discards); no other cache byte is written, and only columns below len[b] are read.
 *   One workgroup per (sample, head), the m queries in registers; softmax and accumulation in fp32, one rescale per loop trip, partial
 *   states merged in a fixed order.  D in {16,32,64,128} and m <= 8 (else MMGL_ERR_UNSUPPORTED); strides multiples of 16 bytes,
 *   q / k_new / v_new / k / v 16-byte aligned.  Plain vector stores only.
 *
 * mmgl_lookup_accept: the tail of a verify step, one launch, one workgroup per sample.
 *   logits      [B*m_in, V] bf16 / fp32, row stride ld_logits: m_in = 1 (the prefill's row per sample) or K + 1 (the rows of `block`)
 *   block       int64 [B, K+1], n_draft int32 [B]: read (m_in > 1) as the inputs of those rows -- [t_last, d_1 .. d_nd, filler] --
 *               then overwritten with the next step's; positions int64 [B, K+1]: the next block's position ids, written
 *   ids         int64 [B, >= T + n_new], row stride ld_ids: columns [0, T) hold the prompt, the new tokens are appended behind
 *   prompt_mask uint8 [B, T], row stride ld_mask: the prompt columns that count as history
 *   gen, len    int32 [B]: tokens the row has (pads behind an EOS included) / its cache columns;  finished uint8 [B];  all read and written
 *   emitted     int32 [B], written: the tokens this call appended to the row
 *   Accept rule, with a_i the argmax of row i (ties to the lowest index, NaN never chosen): e_0 = a_0; e_i = a_i while i <= nd and
 *   d_i == e_{i-1}; stop behind eos_token_id (< 0: none; the rest of the row gets pad_token_id at once and gen = n_new) and at n_new
 *   tokens; either finishes the row.  gen grows by the k tokens emitted, and so does len unless m_in = 1.  A finished row emits
 *   nothing and keeps its state.
 *   Draft rule, on the history h = the valid prompt tokens followed by the row's new tokens, L of them: for n = min(N, L - 1) down to
 *   1, the largest p <= L - n - 1 with h[p .. p+n) == h[L-n .. L) gives the drafts h[p+n .. min(p+n+K, L)); no match: no drafts.
 *   A history token outside [0, V) equals nothing and ends a draft list.  Next block = [e_{k-1}, drafts, e_{k-1} ...]; a finished
 *   row has no drafts and repeats the first token of its block.  positions[b][i] = min(valid prompt tokens + pos_offset + gen - 1 + i,
 *   pos_max).
 *   T + n_new <= 8192 (the history lives in LDS), 1 <= K <= 7, 1 <= N <= 4, else MMGL_ERR_UNSUPPORTED.  A refused call writes nothing.
 *   No workspace, no atomics, no host synchronisation; two runs are bitwise equal.  Plain vector stores only. */
int mmgl_attn_decode_block_fwd(const void* q, int ldq, const void* k_new, const void* v_new, int ld_new, void* k, void* v, int ldkv,
                               size_t batch_stride_kv, int capacity, const uint8_t* key_valid, int ld_valid, const int* len, void* out,
                               int B, int m, int H, int D, int dtype, void* stream);
int mmgl_lookup_accept(const void* logits, size_t ld_logits, int m_in, int64_t* block, int* n_draft, int64_t* positions, int64_t* ids,
                       size_t ld_ids, const uint8_t* prompt_mask, size_t ld_mask, int* gen, int* len, uint8_t* finished, int* emitted,
                       int B, int T, int n_new, int V, int K, int N, int64_t eos_token_id, int64_t pad_token_id, int pos_offset,
                       int pos_max, int dtype, void* stream);

/* The verify step of prompt-lookup decoding on the Llama-family LM (LlamaNeighborLM.generate(prompt_lookup_num_tokens = K)): the cache
 * holds Hkv <= H heads, and a token's rotary position is its cache column len[b] + i -- per sample, on the device.  Two launches per
 * layer, in this order; row b*m + i is new token i of sample b, 1 <= m = K + 1 <= 8.  No reference counterpart.  Forward only.
 *   len         int32 [B], device memory: the columns sample b has filed.  Both kernels clamp it into [0, capacity] and never use it as
 *               an address unclamped; keeping it there is the caller's contract.
 *
 * mmgl_rope_kv_append_block: mmgl_rope_kv_append for the B*m rows of the fused q | k | v projection.
 *   qkv         [B*m, (H + 2 Hkv) * D], row stride ldqkv: the H query heads of a row are rotated IN PLACE by the angles of position
 *               p = len[b] + i; the k and v blocks are only read
 *   cos_sin     fp32 [n_pos, D/2, 2] (cos, sin), dense: the table mmgl_rope_inplace takes, read at row min(p, n_pos - 1)
 *   kv          the cache rows [B, capacity, 2 Hkv D], row stride ldkv, sample stride batch_stride_kv (elements): the row's rotated Hkv
 *               key heads and unrotated Hkv value heads go to column p of sample b when p < capacity, else they are dropped (they
 *               belong to an input whose output the caller discards).  No other byte is written.
 *   The arithmetic of mmgl_rope_kv_append: m = 1 with every len[b] = col is bitwise that call on column col.
 *
 * mmgl_attn_decode_gqa_block_fwd: causal attention of the m new tokens per sample over the cache of Hkv heads, AFTER the append; the
 *   cache is only read.
 *   q, out      [B*m, H*D] (q: row stride ldq, the rotated rows of qkv, already scaled by D^-0.5; out dense)
 *   k, v        the cache slabs: `capacity` rows of Hkv*D per sample, row stride ldkv, sample stride batch_stride_kv (elements)
 *   key_valid   [B, capacity] uint8, row stride ld_valid
 *   Row (b, i), query head h, reads key / value head h / (H / Hkv).  With L = len[b] clamped it attends the columns s < L with
 *   key_valid set, and the new columns L .. min(L + i, capacity - 1), always valid.  A row whose own column L + i is at or past
 *   `capacity` stays in bounds; its value is unspecified (the caller discards it).
 *   One workgroup per (sample, key/value head, block of at most 8 (token, query head) pairs of its m * H / Hkv): each 16-byte K / V
 *   load is issued once for the pairs of the block and nothing is expanded to H heads in memory.  Softmax and accumulation in fp32, one
 *   rescale per loop trip, partial states merged in a fixed order.
 * Both: D in {16,32,64,128} and m <= 8 (else MMGL_ERR_UNSUPPORTED); Hkv any divisor of H (else MMGL_ERR_INVALID); strides multiples of
 * 16 bytes, qkv / q / k / v / kv 16-byte aligned, len 4-byte.  A refused call writes nothing.  No workspace, no atomics, no host
 * synchronisation; two runs are bitwise equal.  Plain vector stores only. */
int mmgl_rope_kv_append_block(void* qkv, int ldqkv, const float* cos_sin, int n_pos, void* kv, int ldkv, size_t batch_stride_kv, int capacity,
                              const int* len, int B, int m, int H, int Hkv, int D, int dtype, void* stream);
int mmgl_attn_decode_gqa_block_fwd(const void* q, int ldq, const void* k, const void* v, int ldkv, size_t batch_stride_kv, int capacity,
                                   const uint8_t* key_valid, int ld_valid, const int* len, void* out, int B, int m, int H, int Hkv, int D,
                                   int dtype, void* stream);

/* ---- contrastive search (generate(penalty_alpha = alpha > 0, top_k = k), 2 <= k <= 8; csrc/contrastive.hip) -------------------------
 * replaces: transformers' _contrastive_search (penalty_alpha + top_k), which repeats the key/value cache k times and ranks with a
 *           [B*k, n, d] similarity through aten.  Here the k candidates of a sample run one decode step on the beam-shared cache
 *           (mmgl_attn_decode_beam_fwd) and this call ranks them.  Forward only; deterministic (no atomics).
 *
 * mmgl_contrastive_select: per sample b the candidate c in [0, k) with the largest
 *     score_c = (1 - alpha) p_c - alpha pen_c,   p_c = exp(cand_score[b][c]),   pen_c = max_j cos(h_c, h_j)
 * in fp32, and the bookkeeping of the step.  Row b*k + c of cand_hidden is h_c; j runs over the context rows [0, n_ctx) of sample b
 * with ctx_valid set.  Dot products and squared norms are accumulated in fp32; the cosine is 0 when either vector has norm 0;
 * pen_c = 0 when no context row is live.  The lowest c among the maxima is selected; a NaN score is never selected (all NaN: c = 0).
 *   cand_hidden [B*k, d], row stride ld_cand                      read
 *   ctx         [B, n_cap, d], row stride ld_ctx, sample stride batch_stride_ctx (elements): rows [0, n_ctx) are read where
 *               ctx_valid is set -- no other row is loaded -- and row n_ctx is written: a copy of the selected candidate row
 *   ctx_valid   uint8 [B, n_cap], row stride ld_valid: entries [0, n_ctx) read, entry n_ctx set to 1
 *   cand_score, cand_index   fp32 / int32 rows of stride ld_pair, the pair mmgl_beam_topk writes (rows_in = 1, beam_score = 0): the
 *               first k entries of a row are the candidates' log-probabilities and token ids
 *   src         int32 [B*k, ld_src]: column `step` of the sample's k rows := the selected c (the parent table of
 *               mmgl_attn_decode_beam_fwd: tail column `step` of every row of the sample now names the chosen key)
 *   ids         int64, row stride ld_ids: ids[b * ld_ids] := the selected token, or pad_token_id if finished[b] was set
 *   finished    uint8 [B]: set when the row's token is eos_token_id; eos_token_id < 0: no end-of-sequence handling, may be null
 *   hidden_out  dense [B, d]: the selected candidate row;  selected  int32 [B]: the selected c
 *   trace_p, trace_pen, trace_score   fp32 [B, k], dense, all three or none: p, pen and score as computed
 *   workspace   mmgl_contrastive_workspace(B, k, n_cap) bytes, 4-byte aligned: one partial max per (sample, chunk, candidate)
 * Two launches: one workgroup per (sample, chunk of mmgl_contrastive_chunk() context rows) streams the context once with 16-byte
 * loads against the k candidate rows held in LDS and writes the chunk's partial maxima (starting at -inf); one workgroup per sample
 * folds them in chunk order and does the rest.  n_ctx = 0 skips the first launch.
 * Refused: null pointers, k outside 2..8 (MMGL_ERR_UNSUPPORTED above 8 and below 2), d no multiple of the 16-byte vector, strides
 * smaller than the rows or no multiples of 16 bytes, misaligned pointers, n_ctx outside [0, n_cap - 1], alpha outside [0, 1], k d
 * elements beyond 64 KiB of LDS, a bad dtype.  A refused call writes nothing.  No atomics, no host synchronisation; two runs are
 * bitwise equal.  Plain vector stores only. */
int mmgl_contrastive_chunk(void);
size_t mmgl_contrastive_workspace(int B, int k, int n_cap);
int mmgl_contrastive_select(const void* cand_hidden, size_t ld_cand, void* ctx, size_t ld_ctx, size_t batch_stride_ctx, uint8_t* ctx_valid,
                            size_t ld_valid, int n_cap, const float* cand_score, const int* cand_index, size_t ld_pair, float alpha, int n_ctx,
                            int step, int* src, size_t ld_src, int64_t* ids, size_t ld_ids, uint8_t* finished, int64_t eos_token_id,
                            int64_t pad_token_id, void* hidden_out, int* selected, float* trace_p, float* trace_pen, float* trace_score,
                            void* workspace, size_t workspace_bytes, int B, int k, int d, int V, int dtype, void* stream);

/* ---- FP8 key/value cache (generate(kv_cache_dtype="fp8"); csrc/decode.hip) -----------------------------------------------------------
 * replaces: nothing in the reference (its cache holds keys and values in the model's dtype).  Forward only; deterministic (no atomics).
 *
 * Format.  A cached key or value row is stored as OCP e4m3fn codes with one power-of-two scale per (sample, column, key-or-value,
 * head).  For the D elements x of one head (as stored in T), a = max |x|:  e = 0 if a = 0, else with a = m * 2^X, m in [0.5, 1):
 * e = X - 9 if m <= 0.875 else X - 8 -- the smallest integer with a * 2^-e <= 448 -- clamped to [-120, 120];
 * code = e4m3fn(x * 2^-e), round to nearest even; value = code * 2^e.  The scaled magnitude lies in (224, 448] unless a = 0 or e is
 * clamped, and every value is exactly representable in bf16 and fp32.  Inputs are finite; magnitudes outside [2^-100, 2^100] meet the
 * clamp and -0.0 keeps no promise about its sign.
 *   codes   [B, capacity, 2 H D] bytes: a row is [key head 0 .. H-1 | value head 0 .. H-1], row stride ld_code, sample stride
 *           batch_stride_code (bytes)
 *   scale   [B, capacity, 2 H] int8: a row is [key exponents | value exponents], row stride ld_scale, sample stride batch_stride_scale
 *
 * mmgl_kv_quantize: the prefill's filing.  k, v [B, n, H*D] of T with common row stride ld_src and sample stride batch_stride_src
 * (elements) -- the column views of a fused qkv output, or two tensors -- into rows 0 .. n-1 of `codes` and `scale` (pointers to the
 * first row written).  One launch; one lane per 16 elements.
 *
 * mmgl_attn_decode_q8_fwd: mmgl_attn_decode_fwd over S >= 1 cached columns of codes plus the new token, one launch.
 *   q, out        [B, H*D] (q: row stride ldq, already scaled by D^-0.5; out dense)
 *   k_new, v_new  [B, H*D] of T, row stride ld_new: the new token's key and value as projected.  They take part in the attention
 *                 unquantised and always valid; the launch quantises them and files codes and exponents at column S
 *   k_codes, v_codes / k_scale, v_scale   the key and the value slab of `codes` / `scale` (v_codes = k_codes + H*D, v_scale =
 *                 k_scale + H in a cache row); columns [0, S) are read, column S < capacity is written -- one writer per
 *                 (sample, head, column), no reader of column S in the launch
 *   key_valid     [B, S] uint8, row stride ld_valid: a masked cached key weighs nothing (the new key is valid: no all-masked case)
 *   One workgroup per (sample, head); D / 16 lanes share a key, 16-byte loads of 16 codes, keys past S outside the buffer descriptor;
 *   the key's scale multiplies the dot product, the value's scale the weight; fp32 online softmax, states merged in a fixed order:
 *   two runs are bitwise equal.  The result equals mmgl_attn_decode_fwd on the dequantised columns followed by the new row, up to
 *   summation order.
 * Both: D in {16,32,64,128} (else MMGL_ERR_UNSUPPORTED); strides multiples of 16 bytes and q / k / v / k_new / v_new / codes 16-byte
 * aligned, a sample's code rows below 2 GiB (else MMGL_ERR_UNSUPPORTED); null pointers, sizes < 1, capacity <= S, strides smaller than
 * the rows, a bad dtype: MMGL_ERR_INVALID.  A refused call writes nothing.  Plain vector stores only. */
int mmgl_kv_quantize(const void* k, const void* v, int ld_src, size_t batch_stride_src, void* codes, int ld_code, size_t batch_stride_code,
                     void* scale, int ld_scale, size_t batch_stride_scale, int B, int n, int H, int D, int dtype, void* stream);
int mmgl_attn_decode_q8_fwd(const void* q, int ldq, const void* k_new, const void* v_new, int ld_new, void* k_codes, void* v_codes,
                            int ld_code, size_t batch_stride_code, void* k_scale, void* v_scale, int ld_scale, size_t batch_stride_scale,
                            int capacity, const uint8_t* key_valid, int ld_valid, void* out, int B, int H, int S, int D, int dtype,
                            void* stream);

/* mmgl_attn_decode_gqa_q8_fwd: mmgl_attn_decode_q8_fwd over a cache of Hkv <= H key/value heads (the Llama-family LM; H % Hkv == 0,
 * query head h reads key/value head h / (H / Hkv)).  The code and scale rows are the format above with H replaced by Hkv:
 * codes [B, capacity, 2 Hkv D] bytes, scale [B, capacity, 2 Hkv] int8 (v_codes = k_codes + Hkv*D, v_scale = k_scale + Hkv in a row).
 *   q, out        [B, H*D] as above;  k_new, v_new  [B, Hkv*D] of T, row stride ld_new: unquantised and always valid in the
 *                 attention, filed as codes and exponents at column S by the same launch
 *   One workgroup per (sample, key/value head, block of at most 4 query heads of that head's group): every 16-byte load of 16 codes
 *   is issued once per block, dequantised once and scored against the block's query heads from registers; nothing is expanded to H
 *   heads in memory.  G = H / Hkv > 4 takes ceil(G / 4) blocks: every block folds the new key and value unquantised, block 0 alone
 *   files column S -- exactly one writer per (sample, key/value head), and no workgroup reads column S.  A sample whose cached keys
 *   are all masked returns the new value row of its key/value head for every query head of the group, bitwise.  Scales, softmax,
 *   merge order, determinism and every refusal as mmgl_attn_decode_q8_fwd (the strides are measured against Hkv-head rows), plus
 *   Hkv < 1 and H % Hkv != 0: MMGL_ERR_INVALID.  A refused call writes nothing.  Plain vector stores only. */
int mmgl_attn_decode_gqa_q8_fwd(const void* q, int ldq, const void* k_new, const void* v_new, int ld_new, void* k_codes, void* v_codes,
                                int ld_code, size_t batch_stride_code, void* k_scale, void* v_scale, int ld_scale,
                                size_t batch_stride_scale, int capacity, const uint8_t* key_valid, int ld_valid, void* out, int B, int H,
                                int Hkv, int S, int D, int dtype, void* stream);

/* ---- FP8 frozen weights (generate(weight_dtype="fp8"); csrc/decode.hip) ---------------------------------------------------------------
 * replaces: nothing in the reference (its decode step multiplies weights in the model's dtype).  Forward only; deterministic (no atomics).
 *
 * Format.  The FP8 key/value cache's, per weight row: a weight W [N, K] is `codes` [N, K] OCP e4m3fn bytes (unit column stride, row
 * stride ld_codes bytes) and `exps` [N] int8; W[n, k] = codes[n, k] * 2^exps[n].  exps[n] is the exponent rule above applied to
 * a = max_k |W[n, k]| (one function in the library, q8_exponent), the codes are e4m3fn(W[n, k] * 2^-exps[n]), round to nearest even:
 * nothing saturates, and every value is exact in bf16.  Weights are finite: a NaN or an infinity is outside the contract (the row's
 * exponent and codes are then unspecified); magnitudes outside [2^-100, 2^100] meet the exponent clamp.
 *
 * mmgl_weight_quantize: W [N, K] of T (bf16 or fp32, row stride ldw elements) -> codes, exps.  One launch, run once per weight: one
 * wave per row, a first pass for the row's maximum, a second that encodes; 16 elements per lane and 16-byte stores where K % 16 == 0
 * and the rows are 16-byte aligned, element by element otherwise.  Bitwise reproducible.  N, K < 1, a bad dtype, a null pointer,
 * ldw < K or ld_codes < K: MMGL_ERR_INVALID, nothing written.
 *
 * mmgl_gemm_skinny_w8: y[M,N] = act((x[M,K] . (codes * 2^exps)^T + bias) * scale) + residual for 1 <= M <= 64 rows: mmgl_gemm_skinny
 * on a quantised weight.  dtype is the type of x, bias, residual and y; ldx, ldy (elements) and ld_codes (bytes) are free.
 *   bf16, K % 128 == 0, N % 8 == 0, ldx % 8 == 0, ld_codes % 16 == 0, x and codes 16-byte aligned: the MFMA kernel of
 *   mmgl_gemm_skinny on code loads -- a K unit of 128 codes (one 128-byte line per weight row, two 16-byte loads per lane, non-temporal,
 *   no LDS round trip, a ring of 4 units per lane in flight), codes -> bf16 A fragments in registers (v_cvt_scalef32_pk_bf16_fp8),
 *   bf16 MFMA, fp32 accumulation, 16 or 8 weight rows per workgroup by mmgl_gemm_skinny's rule, the K slots folded in slot order; 2^exps[n]
 *   multiplies the folded fp32 sum (exact) in front of bias, scale, activation and residual.
 *   Anything else (fp32, other K / N, unaligned rows): one wave per output column, fp32 accumulation, the same epilogue.
 * Two runs are bitwise equal.  Refusals as mmgl_gemm_skinny, under this name: sizes < 1, a bad dtype, a null x / codes / exps / y, an
 * unknown activation, ldx < K, ld_codes < K or ldy < N: MMGL_ERR_INVALID; M > 64: MMGL_ERR_UNSUPPORTED.  A refused call writes
 * nothing.  Plain vector stores only. */
int mmgl_weight_quantize(const void* w, int ldw, void* codes, int ld_codes, void* exps, int N, int K, int dtype, void* stream);
int mmgl_gemm_skinny_w8(const void* x, int ldx, const void* codes, int ld_codes, const void* exps, const void* bias, const void* residual,
                        void* y, int ldy, int M, int N, int K, int act, float scale, int dtype, void* stream);

/* ---- cached decoding of a T5 (model/t5_hip.py: T5HipRunner.generate; csrc/decode.hip) -------------------------------------------------
 * replaces: HuggingFace generate() behind the reference's test protocol for a T5 (language_modelling/run_generation.py:600), whose
 *   cached decoder self-attention is T5Attention.forward with past_key_value: scores + position_bias[:, :, -1:, :].  Forward only.
 *
 * mmgl_attn_decode_relbias_fwd: out[b, h*D..] = softmax_s(q[b, h] . K[b, s, h] + bias[h, S - 1 - s]) V[b, :, h], one query row per
 *   (batch, head) over the S cached keys; the query is the newest key s = S - 1, at distance 0.
 *   q, k, v, out, ldq, ldkv, batch_stride_kv, D, dtype as mmgl_attn_decode_fwd, except that q is the RAW projection: T5 is unscaled
 *             and no D^-0.5 appears anywhere
 *   bias      fp32 [H, ld_bias], ld_bias >= S: bias[h, d] = relative_attention_bias[bucket(-d), h], the learned word of distance d
 *             (ops.t5_decode_bias builds the rows once per generation from transformers' own bucket function)
 *   There is no key mask: a T5 decoder row starts with the start token and has no padding.
 *   The kernel is mmgl_attn_decode_fwd's (lane geometry, trip constants, 16-byte buffer loads, fixed-order merges: deterministic, no
 *   atomics) with the bias word added to the raw score in fp32.  Refusals as mmgl_attn_decode_fwd under this name, the bias rows in
 *   the mask's place: sizes < 1, a bad dtype, a null pointer, ldq or ldkv < H*D, ld_bias < S: MMGL_ERR_INVALID; D outside
 *   {16,32,64,128}, strides no multiples of 16 bytes, q / k / v not 16-byte or bias not 4-byte aligned, a sample's key rows spanning
 *   2 GiB: MMGL_ERR_UNSUPPORTED.  A refused call launches nothing and leaves `out` as it was. */
int mmgl_attn_decode_relbias_fwd(const void* q, int ldq, const void* k, const void* v, int ldkv, size_t batch_stride_kv,
                                 const float* bias, int ld_bias, void* out, int B, int H, int S, int D, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMGL_HIP_H */
