// libmmgl_hip.so: error channel, launch configuration shared by every kernel family, version.
#include "common.h"
#include <string.h>
#include <atomic>
#include <mutex>

static thread_local char g_err[512] = "";

void mmgl_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* mmgl_last_error(void) { return g_err; }

// The dynamic-LDS limit is raised ONCE per (kernel, device), to the hardware maximum (the attribute is a launch limit, not an allocation: the
// launch's own dynamic size decides occupancy): at the reference's batch the step is launch-bound and this call sat in front of every
// launch above 48 KiB.  Lookup is lock-free; the first use of a (kernel, device) pair takes a mutex, so two threads
// with different LDS sizes cannot leave the attribute below what the table says (it is never lowered: there is one value).
// The value set is the 160 KiB of a CU minus the kernel's static LDS: two attn_general kernels carry 256 B that the compiler put there,
// every other kernel with dynamic LDS has none and gets the whole maximum.
int mmgl_set_lds(const void* kernel, size_t bytes, const char* who) {
    constexpr size_t kMaxLds = 160 * 1024;
    if (bytes > kMaxLds) MMGL_FAIL(MMGL_ERR_UNSUPPORTED, "%s: needs %zu B of LDS (> 160 KiB)", who, bytes);
    if (bytes <= 48 * 1024) return MMGL_OK;
    constexpr int kSlots = 1024;                        // (kernel, device) pairs; under 200 kernels take dynamic LDS, few of them above 48 KiB
    struct Slot { std::atomic<const void*> fn{nullptr}; int dev = -1; };
    static Slot slots[kSlots];
    static std::atomic<int> used{0};
    static std::mutex mu;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const int n = used.load(std::memory_order_acquire);
    for (int i = 0; i < n; ++i)
        if (slots[i].fn.load(std::memory_order_relaxed) == kernel && slots[i].dev == dev) return MMGL_OK;
    std::lock_guard<std::mutex> lock(mu);
    const int n2 = used.load(std::memory_order_acquire);
    for (int i = n; i < n2; ++i)
        if (slots[i].fn.load(std::memory_order_relaxed) == kernel && slots[i].dev == dev) return MMGL_OK;
    hipFuncAttributes fa;
    hipError_t e = hipFuncGetAttributes(&fa, kernel);
    if (e == hipSuccess) e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kMaxLds - fa.sharedSizeBytes));
    if (e != hipSuccess) MMGL_FAIL(MMGL_ERR_HIP, "%s: raising the dynamic LDS limit: %s", who, hipGetErrorString(e));
    if (n2 < kSlots) {                                  // a full table only costs the call again next time
        slots[n2].dev = dev;
        slots[n2].fn.store(kernel, std::memory_order_relaxed);
        used.store(n2 + 1, std::memory_order_release);
    }
    return MMGL_OK;
}

// CUs of the current device (= workgroups of a full persistent launch), looked up once per device; 256 where there is no device to ask
// (the planners that size K splits by it also run on a machine without one).
int mmgl_num_cu() {
    static std::atomic<int> cus[64];
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    std::atomic<int>& slot = cus[dev & 63];
    if ((n = slot.load(std::memory_order_relaxed))) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    slot.store(n, std::memory_order_relaxed);
    return n;
}

// ABI version: bumped whenever an exported signature changes (mmgl_amd/_lib.py refuses a library that reports another one -- a
// stale build would otherwise load and run with misaligned arguments).  101: mmgl_xattn_fwd lost p_drop / seed / offset.
// 102: round 4 (tile counters bound to one stream; entry points added / removed with the kernel families).
// 103: mmgl_comm_* / mmgl_allreduce_sum / mmgl_allgather / mmgl_broadcast.
// 105: the stand-alone dgrad, weight-gradient and transpose entry points removed (mmgl_linear_bwd covers them).
// 106: mmgl_gemm_skinny / mmgl_attn_decode_fwd (the decode step of generate()).
// 107: mmgl_gemm_skinny_lora (the decode step of a LoRA-adapted projection).
// 108: mmgl_selfattn_gqa_fwd / _bwd_workspace / _bwd (grouped-query self-attention of the Llama family).
// 109: mmgl_attn_decode_gqa_fwd / mmgl_rope_kv_append (the decode step of the Llama-family LM: grouped-query cache, rotary at one position).
// 110: mmgl_attn_decode_beam_fwd / mmgl_beam_topk(_workspace) / mmgl_beam_advance (beam search on a beam-shared cache).
// mmgl_sample_tokens (sampling for generate()) was added at 110 without a bump: no existing signature changed, and the binding
// resolves every declared symbol at load, so a library built without it is refused all the same.
// mmgl_logits_process (repetition penalty, n-gram and token bans for generate()) was added at 110 the same way.
// mmgl_attn_decode_block_fwd / mmgl_lookup_accept (prompt-lookup decoding for generate()) were added at 110 the same way.
// mmgl_selfattn_tiles_fwd / _bwd and mmgl_layernorm_tiles_fwd / mmgl_add_layernorm_tiles_fwd (keys and values of the live key
// tiles only in the frozen layers) were added at 110 the same way.
// mmgl_rope_kv_append_block / mmgl_attn_decode_gqa_block_fwd (prompt-lookup decoding on the Llama-family LM) were added at 110 the same way.
// mmgl_contrastive_chunk / mmgl_contrastive_workspace / mmgl_contrastive_select (contrastive search for generate()) were added at 110 the same way.
// mmgl_kv_quantize / mmgl_attn_decode_q8_fwd (FP8 key/value cache for generate()) were added at 110 the same way.
// mmgl_attn_decode_gqa_q8_fwd (FP8 key/value cache on the Llama-family LM) was added at 110 the same way.
// mmgl_weight_quantize / mmgl_gemm_skinny_w8 (FP8 frozen weights for generate()) were added at 110 the same way.
// mmgl_selfattn_tiles_rows_bwd / mmgl_gemm_nt_rowk(_item) / mmgl_add_layernorm_rows_bwd (live-first gradient rows of the frozen layers:
// the fused QKV dgrad skips the zero dK | dV of dead key tiles) were added at 110 the same way.
// mmgl_attn_relbias_fwd / mmgl_attn_relbias_bwd(_workspace) (T5 attention: relative-position bias, native T5 forward) were added at
// 110 the same way.
// mmgl_adafactor_workspace / mmgl_adafactor_step (fused Adafactor for T5 training) were added at 110 the same way.
extern "C" int mmgl_version(void) { return 110; }
