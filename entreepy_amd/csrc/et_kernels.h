// et_kernels.h -- geometry constants and launch wrappers of et_kernels.hip and et_kernels_fallback.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "et_tables.h"

// A value made "new" to the compiler at this point of the program (an empty asm statement with the value as an in/out
// operand).  Three of round 3's gains hang on such pins: K4's and D3's prefetches (where the wait for a load that was asked
// for a round / a unit ahead is placed) and D1's edge-block step limits (kept from being hoisted in front of every block).
// None changes a result, so no parity test sees one go missing -- tests/test_isa_guard.py compiles the kernels to ISA and
// checks what the pins hold in place, and builds them once more with -DET_GUARD_DROP_PINS to show that it would notice.
#ifdef ET_GUARD_DROP_PINS
#define ET_PIN(x_) ((void)0)
#else
#define ET_PIN(x_) asm volatile("" : "+v"(x_))
#endif

namespace et {

constexpr int BLOCK = 256;                    // threads per workgroup: 4 wavefronts of 64
constexpr uint32_t ROUND_BYTES = BLOCK * 16;  // one 16-byte load per lane
constexpr uint32_t MAX_ROUNDS_PER_TILE = 128;  // tile <= 512 KiB (u32 tile counters; u32 bit cursors: 2^19 symbols of <= 255 bits)
constexpr uint32_t HIST_REDUCE_GROUPS = 128;   // k_hist_reduce: two histogram columns each
constexpr uint32_t MAX_GRID = 2048;           // 256 CUs x 8 workgroups, grid-stride beyond

constexpr uint32_t SUB_BITS = 256;                             // decode: bits per lane subsequence
constexpr uint32_t DEC_BLOCK_WORDS = BLOCK * SUB_BITS / 32;    // 8 KiB of bitstream per workgroup
constexpr uint32_t DEC_GUARD_WORDS = 4;                        // words a lane may read past its workgroup's 8 KiB
// How the round-1 decode kernels take their 8 KiB blocks: the LDS-window kernels (k_dec_sync, k_dec_maps, k_dec_resolve,
// k_dec_write) one block per workgroup -- they run over three blocks at the most, or over a call's special blocks; the
// register-window kernels by ticket, k_dec_write_reg in chunks of
constexpr uint32_t WRITE_CHUNK = 4;  // consecutive blocks (k_dec_sync_reg / _reg2: the chunk sizes in launch_dec_sync)
constexpr uint32_t DEC_FIRST_SWEEP_TRIPS = 6;                   // local fixed-point trips before a block is declared non-synchronising
constexpr uint32_t DEC_REPAIR_SWEEP_TRIPS = 8;                  // same cap for the two speculatively enqueued repair sweeps
// ONE rule for "the sweeps left a final synchronisation state", applied by the host to its copy of
// the flags and by a speculatively launched D3 to the flags themselves -- the two must agree, or the
// host keeps output that the kernel declined to write: the verification passed, and no more blocks
// gave up in the first sweep than the repair sweeps are meant for (beyond that the host goes the
// exhaustive way).  Blocks that gave up AND were repaired by the second sweep are fine.
__host__ __device__ inline bool dec_state_final(uint32_t gave_up, uint32_t verify_failed, uint32_t n_blocks) {
    return verify_failed == 0 && static_cast<uint64_t>(gave_up) * 64 <= n_blocks;
}
constexpr uint32_t DEC_HAVE_START = 1, DEC_FRONT_OK = 2;       // k_dec_sync flags (ranges of a stream split over GPUs)
constexpr uint32_t DEC_SPECIAL_SUPER = 8;                      // with DEC_SPECIAL_ONLY: the blocks of 16 KiB superblocks k_dec_sync_reg2 leaves out
constexpr uint32_t DEC_SPECIAL_ONLY = 4;                       // k_dec_sync flag, k_dec_maps / _resolve / _write mode: first/last blocks only (the _reg kernel has the rest)
constexpr uint32_t DEC_FRONT_WORDS = 4;                        // words staged BEFORE the workgroup's 8 KiB (warm-up run-in)
constexpr uint32_t DEC_WARMUP_BITS = DEC_FRONT_WORDS * 32;     // run-in before each subsequence in the first sync sweep
constexpr uint32_t DEC_STAGED_WORDS = DEC_FRONT_WORDS + DEC_BLOCK_WORDS + DEC_GUARD_WORDS;
constexpr uint32_t DEC_SDATA_WORDS = (DEC_STAGED_WORDS + (DEC_STAGED_WORDS >> 5) + 4) & ~3u;  // 1 pad word per 32
constexpr uint32_t DEC_STAGE_BYTES = 16384;                    // LDS staging of decoded symbols

// The 16 device words the decode's kernels and the host share (et_ctx::flag; DecWs::flag below), and the host's copy of them
// (k_scan_fused's report: words 0 .. 11 as they are, then the total and the epoch).
enum DecFlag : uint32_t {
    FLAG_CHANGED = 0,        // a sweep changed something (every repair sweep clears it first)
    FLAG_GAVE_UP = 1,        // blocks that gave up in the first sweep
    FLAG_VERIFY_FAILED = 2,  // the scan's verification failed
    FLAG_ROW_BLIND = 3,      // the row walk: a chunk never saw the chunks before it
    FLAG_SYNC_TICKET = 4,    // ticket of k_dec_sync_reg / _reg2 (D1's first sweep), and of k_dec_write_reg in a range's write
    FLAG_WRITE_TICKET = 5,   // ticket of k_dec_write_reg in the whole-stream write (D3); no LDS-window kernel draws a ticket
    FLAG_WORK_COUNT = 8,     // worklist count
    FLAG_RANGE_EXIT = 9,     // a tree-walked range's exit bit (k_tw_sync's exit_bits)
    FLAG_TOTAL_LO = 12,      // symbol total ...
    FLAG_TOTAL_HI = 13,
    FLAG_REPORT_EPOCH = 14,  // the host's copy only: the epoch of the report that filled it
    DEC_FLAG_WORDS = 16
};
constexpr uint32_t DEC_SWEEP_FLAGS = 4;  // the words in front of the tickets: all a first window sweep needs cleared
static_assert(FLAG_CHANGED < DEC_SWEEP_FLAGS && FLAG_GAVE_UP < DEC_SWEEP_FLAGS && FLAG_VERIFY_FAILED < DEC_SWEEP_FLAGS && FLAG_ROW_BLIND < DEC_SWEEP_FLAGS &&
                  FLAG_SYNC_TICKET >= DEC_SWEEP_FLAGS && FLAG_WRITE_TICKET >= DEC_SWEEP_FLAGS,
              "the sweeps' flags lie in front of the tickets, which the launches that draw on them clear (unless told they are zero)");

// The workspaces every synchronisation writes, as the kernels take them.
struct DecWs {
    uint32_t *sub_state, *blk_exit, *blk_count, *flag, *worklist;
    unsigned long long *blk_off, *group_sum;
};

// What a decode launch runs over: a whole stream, or a range of one split over GPUs.
struct DecSpan : DecWs {
    const uint32_t *words;     // from a 4-byte aligned base
    uint64_t n_bytes, n_subs;  // a range's: the bytes after it included, the subsequences after it not
    uint32_t n_blocks, first_bit;  // n_blocks = n_subs in workgroups of BLOCK, rounded up
};

// The three-workgroup launches for the stream's first/last blocks take ~25 us each (one
// block's latency); given a side lane they run beside the big launch instead of after it.
struct SideLane {
    hipStream_t stream;
    hipEvent_t fork, join;
};

// Timing events carried by a launch itself (no marker packets): begin / end of that kernel.
struct KernelEvents {
    hipEvent_t start = nullptr, stop = nullptr;
};

void launch_hist(hipStream_t stream, const uint8_t *base, uint64_t lo, uint64_t hi, uint32_t rounds_per_tile, uint32_t n_tiles,
                 uint32_t *tile_hist, unsigned long long *block_hist, unsigned long long *hist, unsigned long long *host_hist = nullptr, unsigned long long epoch = 0,  // host_hist: 256 + HIST_REDUCE_GROUPS words of pinned host memory: the totals, and per reducing workgroup `epoch` once its two are stored
                 KernelEvents ev = {}, unsigned long long *hist_also = nullptr);  // hist_also: a second device copy of the totals
// Bytes that hold the header and the dictionary of a stream whose first byte is d (decode.zig:34: d + 1 entries of at
// most 8 + 8 + 32 bits behind 5 header bytes), rounded up.
__host__ __device__ inline uint32_t header_bound(uint8_t d) { return 8u + 6u * (static_cast<uint32_t>(d) + 1u); }
// the first min(n, header_bound(d_src[0])) bytes of d_src -> host_dst (pinned host memory, 4-byte aligned, room for that
// rounded up to 4), then *host_done = epoch (pinned as well)
// d_src[0 .. n_words) dwords (4-byte aligned) -> host_dst (pinned), then *host_done = epoch (pinned)
void launch_words_to_host(hipStream_t stream, const void *d_src, uint32_t n_words, void *host_dst, unsigned long long *host_done, unsigned long long epoch);
void launch_header_to_host(hipStream_t stream, const void *d_src, uint32_t n, void *host_dst, unsigned long long *host_done, unsigned long long epoch);
// lengths: the 256 code lengths (host memory; they travel as a kernel argument).  host_src / dev_dst / copy_words: a
// pinned host block the first kernel copies into device memory for the kernels behind it (K4's code table, the header);
// once it has, it stores taken_epoch into *host_taken (pinned): the block may be filled again.
void launch_tile_scan(hipStream_t stream, const uint32_t *tile_hist, uint32_t n_tiles, const uint8_t *lengths, const uint32_t *host_src, uint32_t *dev_dst,
                      uint32_t copy_words, unsigned long long *host_taken, unsigned long long taken_epoch, unsigned long long *tile_bits, unsigned long long *group_sum, uint32_t epoch, unsigned long long base_bit,  // group_sum, epoch: k_scan_fused's pub words (zeroed once) and a value in 1 .. 65535 not used on them since
                      unsigned long long *tile_off, uint32_t *out32, const uint32_t *header_src = nullptr, uint32_t header_words = 0);  // header_src (device): the file header, copied to out32[0 .. header_words) behind the seam word's zeroing
void launch_encode(hipStream_t stream, const uint8_t *base, uint64_t lo, uint64_t hi, uint32_t rounds_per_tile, uint32_t n_tiles,
                   const unsigned long long *tile_off, const uint2 *enc_table, uint32_t max_len, uint32_t *out32, KernelEvents ev = {});
// D1 by window sweeps over s, number iter of it; raises FLAG_CHANGED; a first sweep over more than three blocks counts on FLAG_SYNC_TICKET
// (ticket_is_zero: the caller has just cleared it).  listed (iter >= 1): the blocks that
// disagree with the one before them go on s.worklist (FLAG_WORK_COUNT, zeroed by the caller, counts them) and the sweep is over
// those; else over every block.
void launch_dec_sync(hipStream_t stream, const DecSpan &s, const DecodeTables &tb, uint32_t iter, uint32_t max_trips, uint32_t flags = DEC_HAVE_START,
                     bool listed = false, const SideLane *side = nullptr, bool ticket_is_zero = false, KernelEvents ev = {});  // ev: the first sweep's main kernel
void launch_dec_maps(hipStream_t stream, const DecSpan &s, bool have_start, const DecodeTables &tb, uint32_t n_starts, uint32_t map_stride,
                     uint8_t *lane_maps, uint8_t *blk_maps, uint8_t *grp_maps);
void launch_dec_resolve(hipStream_t stream, const DecSpan &s, bool const_first, const DecodeTables &tb, uint32_t map_stride, const uint8_t *lane_maps,
                        const uint8_t *blk_maps, const uint8_t *grp_maps, uint8_t *blk_in, uint8_t *grp_in);
// Fill the decode tables in a device block (et_tables.h DecTableLayout) from the host's plan, which lies at plan_at of that block; the
// write-step table goes to wsteps_at.  The tables as the host builders': lut[1 << lut_bits], longc[2 * n_long], sub[n_sub << sub_bits],
// sym_len[256], steps[(1 << step_bits) + second level], wsteps[(1 << wstep_bits) + second level].
// zero16 (optional): 16 words the kernel also clears (the decode's flags).
void launch_build_dec_tables(hipStream_t stream, uint8_t *d_block, size_t wsteps_at, size_t plan_at, uint32_t *zero16 = nullptr);
// D2, the scan of s.blk_count into s.blk_off, and what it may do on its way.  ScanVerify: every block started where the one before it
// ends (s.blk_exit), block 0 at `first`, or FLAG_VERIFY_FAILED is raised -- state: s.sub_state, or (rows) the tree walk's blk_start, one
// row per block; nullptr: nothing is verified.  ScanReport: the total to FLAG_TOTAL_LO / _HI, and FLAG_CHANGED .. 11, the total and then
// epoch (FLAG_REPORT_EPOCH) to host, 15 words of pinned host memory.
struct ScanVerify { const uint32_t *state; bool rows; uint32_t first; };
struct ScanReport { uint32_t *host; uint32_t epoch; };
void launch_dec_scan(hipStream_t stream, const DecSpan &s, uint32_t epoch, const ScanVerify *verify = nullptr, const ScanReport *report = nullptr);
// D3 over the chained lookup tables (et_treewalk.h; chain_max_len: the dictionary's longest code), every block by k_dec_write_wave --
// strips: by its instantiation for streams with many symbols per subsequence (quarters that overflow the stage walk once, into
// strips) -- or, chain == nullptr, over tb, a span of more than three blocks counting on flag word `ticket` (FLAG_SYNC_TICKET or
// FLAG_WRITE_TICKET; a smaller one leaves the word alone).  speculative: the
// kernel itself looks at the sweeps' flags and does nothing if the state is not final (dec_state_final).
void launch_dec_write(hipStream_t stream, const DecSpan &s, const DecodeTables &tb, uint64_t n_symbols, uint8_t *out, DecFlag ticket = FLAG_SYNC_TICKET,
                      const SideLane *side = nullptr, bool ticket_is_zero = false, bool speculative = false, KernelEvents ev = {},  // ev: the main write kernel
                      const uint64_t *chain = nullptr, uint32_t n_chain = 0, uint32_t chain_max_len = 32, bool strips = false);

}  // namespace et
