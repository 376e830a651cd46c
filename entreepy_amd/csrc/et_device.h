// et_device.h -- what every kernel file (et_kernels.hip, et_kernels_fallback.hip, et_treewalk.hip, et_rowsync.hip, et_batch.hip)
// needs, defined once: the wavefront / workgroup scans, the 16-byte chunk of a text that loads only the text's own bytes, the stream word that is zero beyond the stream's end, the hand-over of
// pinned memory to the host that polls (the device half of wait_for_word, et_ctx.h), and on the host side the CU count, the
// residency query and the launch that carries its own events.  No LDS is declared here.  Included by .hip files only.
#pragma once

#include "et_kernels.h"

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

namespace et {

// --------------------------------------------------------------------------------
// wavefront / workgroup scans (DPP, no LDS traffic inside a wavefront)
// --------------------------------------------------------------------------------
// The six DPP moves of an inclusive scan over a wavefront, as (control, row mask) handed to STEP_ in order; lanes nothing
// moves into keep `old`.  A prefix sum adds what moves in (below); k_row_sync composes maps with the same moves.
#define ET_WAVE_SCAN_STEPS(STEP_)                                \
    STEP_(0x111, 0xf) /* row_shr:1 */                            \
    STEP_(0x112, 0xf) /* row_shr:2 */                            \
    STEP_(0x114, 0xf) /* row_shr:4 */                            \
    STEP_(0x118, 0xf) /* row_shr:8  -> each row of 16 scanned */ \
    STEP_(0x142, 0xa) /* row_bcast:15 into rows 1 and 3 */       \
    STEP_(0x143, 0xc) /* row_bcast:31 into rows 2 and 3 */

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_add(uint32_t x) {
    return x + static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), CTRL, ROW_MASK, 0xf, false));
}

// Inclusive prefix sum over the 64 lanes of a wavefront: lane 63 holds the wavefront's total.
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x) {
#define ET_DPP_ADD_STEP(ctrl_, row_mask_) x = dpp_add<ctrl_, row_mask_>(x);
    ET_WAVE_SCAN_STEPS(ET_DPP_ADD_STEP)
#undef ET_DPP_ADD_STEP
    return x;
}

__device__ __forceinline__ uint64_t wave_inclusive_scan64(uint64_t x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// Exclusive prefix sum over the 256 threads of a workgroup; *total = sum of all.
// `scratch` is 4 LDS words.  Contains ONE barrier; the caller must separate two
// calls that reuse `scratch` by another barrier.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t x, uint32_t *scratch, uint32_t *total) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (scalar: what lies before a wavefront is added up on the scalar unit)
    const uint32_t inc = wave_inclusive_scan(x);
    if (lane == 63) scratch[wave] = inc;
    __syncthreads();
    const uint32_t w0 = __builtin_amdgcn_readfirstlane(scratch[0]), w1 = __builtin_amdgcn_readfirstlane(scratch[1]),
                   w2 = __builtin_amdgcn_readfirstlane(scratch[2]), w3 = __builtin_amdgcn_readfirstlane(scratch[3]);
    uint32_t before = 0;
    if (wave > 0) before += w0;
    if (wave > 1) before += w1;
    if (wave > 2) before += w2;
    *total = w0 + w1 + w2 + w3;
    return before + (inc - x);
}

// --------------------------------------------------------------------------------
// input addressing
// --------------------------------------------------------------------------------
// The text is addressed relative to a 16-byte aligned base: the stream occupies
// bytes [lo, hi) of it (lo < 16).  A lane's 16-byte chunk is loaded with one
// dwordx4 when it lies fully inside [lo, hi); the (at most two) partial chunks of a
// stream are assembled from guarded byte loads so nothing outside it is touched.
struct Chunk {
    uint32_t w[4];
    uint32_t valid;  // bit k set <=> byte k belongs to the stream
};

__device__ __forceinline__ Chunk load_chunk(const uint8_t *__restrict__ base, uint64_t off, uint64_t lo, uint64_t hi) {
    Chunk c;
    if (off >= lo && off + 16 <= hi) {
        const uint4 v = *reinterpret_cast<const uint4 *>(base + off);
        c.w[0] = v.x; c.w[1] = v.y; c.w[2] = v.z; c.w[3] = v.w;
        c.valid = 0xffffu;
    } else {
        c.w[0] = c.w[1] = c.w[2] = c.w[3] = 0;
        c.valid = 0;
        if (off < hi && off + 16 > lo) {
            for (int k = 0; k < 16; ++k) {
                const uint64_t p = off + k;
                if (p >= lo && p < hi) {
                    c.w[k >> 2] |= static_cast<uint32_t>(base[p]) << (8 * (k & 3));
                    c.valid |= 1u << k;
                }
            }
        }
    }
    return c;
}

// --------------------------------------------------------------------------------
// the stream's words at its end
// --------------------------------------------------------------------------------
// Word `idx` of the stream AS IT LIES IN MEMORY (stream byte k of the word is its byte k), zero beyond n_bytes: the one
// byte-wise tail.  Inlined (the window kernels); the walks, which are at their register limits, call it (below).
__device__ __forceinline__ uint32_t stream_word_guarded(const uint32_t *__restrict__ words, uint64_t idx, uint64_t n_bytes) {
    const uint64_t b0 = idx * 4;
    if (b0 + 4 <= n_bytes) return words[idx];
    uint32_t v = 0;
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(words);
    for (int k = 0; k < 4; ++k)
        if (b0 + k < n_bytes) v |= static_cast<uint32_t>(bytes[b0 + k]) << (8 * k);
    return v;
}
// ... as a call (the row walk, the fixed-length write)
inline __device__ __attribute__((noinline)) uint32_t stream_word_guarded_call(const uint32_t *__restrict__ words, uint64_t idx, uint64_t n_bytes) {
    return stream_word_guarded(words, idx, n_bytes);
}
// ... as a call, for an index that may be negative (before `words`: zero -- or, front_ok, the four words in front of `words`
// are stream bytes too: a range of a stream that began earlier).  The tree walk's.
inline __device__ __attribute__((noinline)) uint32_t stream_word_guarded_front(const uint32_t *__restrict__ words, long long idx, uint64_t n_bytes, bool front_ok) {
    if (idx < 0) return front_ok && idx >= -4 ? words[idx] : 0u;
    return stream_word_guarded(words, static_cast<uint64_t>(idx), n_bytes);
}

// --------------------------------------------------------------------------------
// hand-over to the host: an answer in pinned memory, then the epoch word the host polls (wait_for_word, et_ctx.h)
// --------------------------------------------------------------------------------
// "What this thread stored to pinned memory is visible to the host": called by every thread that stored, in front of the
// barrier behind which one thread stores the epoch.
__device__ __forceinline__ void pinned_stores_visible() { __threadfence_system(); }
// The epoch itself, by ONE thread, behind that barrier.
template <typename T>
__device__ __forceinline__ void store_epoch(T *word, T epoch) {
    __hip_atomic_store(word, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// Both at once, for the thread that stored the answer itself (or has just learnt that everybody else's is visible).
template <typename T>
__device__ __forceinline__ void hand_over(T *word, T epoch) {
    pinned_stores_visible();
    store_epoch(word, epoch);
}

// ---- launch helpers (host) -------------------------------------------------------------------------------
// A launch that carries its own timing events (hipExtLaunchKernelGGL: the dispatch's completion
// signal records begin and end, no marker packets in the stream -- ten hipEventRecord markers per
// encode+decode cost ~70 us at 1 GiB), or a plain launch when no events are asked for.
#define ET_LAUNCH_TIMED(kernel_, grid_, block_, smem_, stream_, evs_, ...)                                                        \
    do {                                                                                                                          \
        if ((evs_).start || (evs_).stop) hipExtLaunchKernelGGL(kernel_, grid_, block_, smem_, stream_, (evs_).start, (evs_).stop, 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel_, grid_, block_, smem_, stream_, __VA_ARGS__);                                             \
    } while (0)

// CUs of the current device (asked once per thread and device: this sits on the launch path); 256 if the device does not say.
[[maybe_unused]] static int device_cus() {
    static thread_local int cus_dev = -1, cus = 256;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev != cus_dev) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
        cus_dev = dev;
    }
    return cus;
}

// Workgroups of `kernel` a CU holds at once (occupancy query; 0 when the query fails: every caller has its own answer to
// that), remembered per (kernel, device, LDS size): the query sits on the launch path, and kernels that share a signature
// (the k_encode_tiles<RING> variants, k_dec_sync<first/later>, the k_dec_sync_reg variants) are different entries.
[[maybe_unused]] static int resident_per_cu(const void *kernel, size_t smem, int *cus_out, int threads = BLOCK) {
    struct Entry {
        const void *kernel;
        size_t smem;
        int dev, cus, per_cu;
    };
    static thread_local Entry cache[24];
    static thread_local int n_cached = 0;
    int dev = 0;
    (void)hipGetDevice(&dev);
    for (int i = 0; i < n_cached; ++i)
        if (cache[i].kernel == kernel && cache[i].smem == smem && cache[i].dev == dev) {
            *cus_out = cache[i].cus;
            return cache[i].per_cu;
        }
    const int cus = device_cus();
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, smem) != hipSuccess) per_cu = 0;
    if (n_cached < 24) cache[n_cached++] = Entry{kernel, smem, dev, cus, per_cu};
    *cus_out = cus;
    return per_cu;
}

// Grid of a chunked decode kernel: one workgroup per chunk, or -- ticketed -- as many
// workgroups as the occupancy API reports resident (an over-estimate is harmless).
template <typename K>
static uint32_t decode_grid(K kernel, size_t smem, uint32_t n_chunks, bool ticketed, int threads = BLOCK) {
    if (!ticketed) return n_chunks;
    int cus = 256;
    int per_cu = resident_per_cu(reinterpret_cast<const void *>(kernel), smem, &cus, threads);
    if (per_cu < 1) per_cu = 1;
    const uint32_t g = static_cast<uint32_t>(cus) * static_cast<uint32_t>(per_cu);
    return n_chunks < g ? (n_chunks ? n_chunks : 1) : g;
}

}  // namespace et
