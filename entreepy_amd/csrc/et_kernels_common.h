// et_kernels_common.h -- what et_kernels.hip (the kernels on the common path) and et_kernels_fallback.hip (the round-1
// kernels that remain as the decoder of what lies outside the tree walk's and the row walk's domains) ALONE share: the
// decode kernels' dynamic LDS block, which blocks are "special", the write walks' word window, the fallback write's
// launcher.  The scans, the guarded stream word, the hand-over to the host and the launch helpers are every kernel
// file's: et_device.h.  Device code; included by .hip files only.
#pragma once

#include "et_device.h"

namespace et {

extern __shared__ __attribute__((aligned(16))) uint8_t dec_smem_raw[];  // ALL dynamic LDS of a decode kernel

// Big-endian numeric value of stream bytes [4*idx, 4*idx+4), zero beyond n_bytes.  NOT a wrapper over stream_word_guarded
// (et_device.h): a tail assembled in memory order and swapped afterwards changes the instructions of k_dec_write_wave's and
// k_dec_sync's edge loads (byte shifts 8k and a v_perm instead of shifts 24 - 8k; other registers) -- so this tail stays.
__device__ __forceinline__ uint32_t load_be32_guarded(const uint32_t *__restrict__ words, uint64_t idx, uint64_t n_bytes) {
    const uint64_t b0 = idx * 4;
    if (b0 + 4 <= n_bytes) return __builtin_bswap32(words[idx]);
    uint32_t v = 0;
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(words);
    for (int k = 0; k < 4; ++k)
        if (b0 + k < n_bytes) v |= static_cast<uint32_t>(bytes[b0 + k]) << (24 - 8 * k);
    return v;
}
__device__ __forceinline__ uint32_t block_limit(uint64_t n_bytes, uint64_t block) {
    const uint64_t rel = n_bytes * 8 - block * DEC_BLOCK_WORDS * 32 + DEC_WARMUP_BITS;  // same origin as walk_subsequence
    // UINT32_MAX unless the stream ends inside (or just after) the staged words of this block
    return rel < DEC_STAGED_WORDS * 32 + 64 ? static_cast<uint32_t>(rel) : 0xffffffffu;
}

// Special blocks keep the LDS-window kernels: the stream's first block and the one or two
// whose staged words reach the stream's end; everything else is "interior".
__device__ __forceinline__ bool special_block(uint64_t b, uint64_t n_bytes) { return b == 0 || block_limit(n_bytes, b) != 0xffffffffu; }
// workgroup i of a special-only launch (grid 3) looks at block 0, n-2, n-1
__device__ __forceinline__ uint64_t special_candidate(uint32_t i, uint32_t n_blocks) {
    if (i == 0) return 0;
    const uint64_t c = static_cast<uint64_t>(n_blocks) + i;
    return c >= 4 ? c - 3 : ~0ull;  // i = 1 -> n-2, i = 2 -> n-1; never block 0 again
}

// k_dec_sync_reg2 works on superblocks of two blocks (512-bit lanes) and takes those whose
// two blocks are both interior; the LDS-window kernel then gets the rest: blocks 0, 1 and
// up to six at the end (workgroup i of a grid of 8).
__device__ __forceinline__ bool super_interior(uint64_t s, uint64_t n_bytes, uint32_t n_blocks) {
    return 2 * s + 1 < n_blocks && !special_block(2 * s, n_bytes) && !special_block(2 * s + 1, n_bytes);
}
__device__ __forceinline__ uint64_t special_candidate2(uint32_t i, uint32_t n_blocks) {
    if (i < 2) return i;
    const uint64_t c = static_cast<uint64_t>(n_blocks) + i;
    return c >= 10 ? c - 8 : ~0ull;  // i = 2..7 -> n-6..n-1, never 0 or 1 again
}

constexpr int RW_WORDS = 13;  // W[j] = stream word 8 * sub - 4 + j (host order): 4 run-in words, 8 own, 1 beyond

typedef __attribute__((address_space(3))) uint8_t lds_u8;

// k_dec_write_wave's fallback pair (et_kernels_fallback.hip): k_dec_write_reg for the interior blocks, k_dec_write for the first / last ones
void launch_dec_write_fallback(hipStream_t stream, const DecSpan &s, const DecodeTables &tb, uint64_t n_symbols, uint8_t *out, DecFlag ticket_word,
                               const SideLane *side, bool ticket_is_zero, bool speculative, KernelEvents ev);

}  // namespace et
