// et_ctx.h -- internal to libentreepy_hip.so: the context behind the extern "C" boundary, and the few helpers its two host
// translation units share (et_api.cpp: context, timings, encode, I/O; et_decode.cpp: decode).
#pragma once

#include "entreepy_hip.h"

#include "et_io.h"
#include "et_kernels.h"
#include "et_rowsync.h"
#include "et_tables.h"
#include "et_treewalk.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>

// What a workspace holds BETWEEN calls (include/entreepy_hip.h, "STATE A CTX KEEPS BETWEEN CALLS"): a buffer that ensure() has to
// replace takes what it held with it, and the link that named it is dropped there.
enum Holds : uint32_t { HOLDS_NOTHING = 0, HOLDS_HISTOGRAM = 1, HOLDS_RANGE = 2 };

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    uint32_t holds = HOLDS_NOTHING;
};

constexpr size_t HEADER_STAGE = 8192;  // >= 4631-byte worst-case header, padded
constexpr size_t DEC_TABLES_BYTES = et::DecTableLayout::BYTES;  // the decode tables' block (et_tables.h)

// The decode families.  The first two are sweeps that may give up on a stream (it then goes to the plan's fallback); the
// others synchronise whatever the stream, or (FIXED_WRITE) need not.
enum class Family { TREE_WALK, WINDOWS, ROWS, FIXED_SYNC, FIXED_WRITE, EXIT_MAPS };

using et::DecWs;

// What is being synchronised -- a whole stream (et_decode_body_device) or a range of one split over GPUs (et_decode_range_*) --
// as the decode's stages (et_decode.cpp) take it: the geometry and workspaces the kernels' launches take (et_kernels.h), and
// what the families add to them.
struct Span : et::DecSpan {
    uint32_t tw_mode, dec_flags, row_mode;  // the kernels' mode bits: TW_FRONT_OK, TW_START_UNKNOWN / DEC_HAVE_START, DEC_FRONT_OK / ROW_MAP_ONLY, ROW_START_UNKNOWN
    const et_codebook *cb;
    et::RowCode row_code;           // ROWS
    et::DecodeTables tb, tb_write;  // WINDOWS, EXIT_MAPS (prepare_decode_tables)
    const uint16_t *tw_table;       // TREE_WALK (tw_setup) ...
    uint32_t tw_n_int;
    uint32_t *blk_start, *blk_pub;
    uint32_t *exit_bits;    // ... where a tree-walked range's exit bit goes (nullptr: a whole stream has none)
    const uint64_t *chain;  // the chained write tables, n_chain entries (nullptr: the write goes over the window tables')
    uint32_t n_chain;
};

// The slots of et_ctx::h_scalar, 8 bytes each: what the device hands to the host in pinned memory.
enum HostScalar {
    HS_TOTAL = 1,         // a range's symbol total; the row walk's map of a range
    HS_RANGE_FLAGS = 2,   // the range calls' words, as uint32_t: RF_* below
    HS_BODY_FLAGS = 4,    // 4 .. 11, as uint32_t: the body decode's copy of the flag words (et::DecFlag)
    HS_ENC_TAKEN = 12,    // == enc_block_epoch: the device has taken its copy of h_enc
    HS_HEADER_DONE = 14,  // == header_epoch: the header bytes of the current decode are in h_header
    HS_SLOTS = 16
};
enum RangeFlag { RF_START = 0, RF_EXIT = 1, RF_ROW_BLIND = 2 };  // (before a range is finished RF_START takes the one word its sweeps wait for: the worklist count, FLAG_CHANGED)

struct et_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    et::SideLane side = {};  // second lane for the first/last-block launches of a decode
    hipStream_t stream = nullptr;
    hipEvent_t switch_ev = nullptr;  // a stream switch orders the new stream after this one, recorded on the old (switch_stream)
    bool timing = false;       // every phase carries events (et_ctx_enable_timing(ctx, 1))
    bool timing_body = false;  // only the decode's write kernel does (et_ctx_enable_timing(ctx, ET_TIMING_DECODE_BODY))
    uint32_t force_rpt = 0;
    std::string err;

    // encode workspaces
    DevBuf tile_hist{nullptr, 0, HOLDS_HISTOGRAM}, hist{nullptr, 0, HOLDS_HISTOGRAM};  // the link between et_histogram_device and the shard encode
    DevBuf block_hist, tile_bits, tile_off, enc_table, group_sum;
    // decode workspaces
    // flag: the et::DEC_FLAG_WORDS words the decode's kernels and the host share (et_kernels.h DecFlag); lut: all decode tables, DEC_TABLES_BYTES
    // (HOLDS_RANGE: what a held range -- `range` below -- reads again in et_decode_range_resolve and et_decode_range_write)
    DevBuf sub_state{nullptr, 0, HOLDS_RANGE}, blk_exit{nullptr, 0, HOLDS_RANGE}, blk_count{nullptr, 0, HOLDS_RANGE}, blk_off{nullptr, 0, HOLDS_RANGE};
    DevBuf lut{nullptr, 0, HOLDS_RANGE}, flag{nullptr, 0, HOLDS_RANGE}, worklist;
    DevBuf lane_maps{nullptr, 0, HOLDS_RANGE}, blk_maps{nullptr, 0, HOLDS_RANGE}, grp_maps{nullptr, 0, HOLDS_RANGE}, blk_in, grp_in;  // exhaustive synchronisation only
    DevBuf row_scratch;                                    // the row walk's published words and ticket (et_rowsync.h)
    // tree-walk synchronisation, chained write tables (et_treewalk.h)
    DevBuf tw_table{nullptr, 0, HOLDS_RANGE}, tw_tree{nullptr, 0, HOLDS_RANGE}, blk_start{nullptr, 0, HOLDS_RANGE}, blk_pub, chain_table{nullptr, 0, HOLDS_RANGE};
    et::TwUpload *h_tw_tree[2] = {};                       // pinned, used in turn like h_lut_buf
    int tw_turn = 0;
    // staging for the host-pointer / file-descriptor entry points
    DevBuf io_in, io_out;
    et_io::Pipe *io = nullptr;  // pinned double buffer + copy threads, made on first use

    // the batched calls (et_batch.cpp): job records and the uploaded block of the current chunk, the kernels' completion counter
    DevBuf batch_jobs, batch_blob, batch_counter;
    DevBuf packed_ws;               // the packed calls: table, counters, a size word per record (the match call: counters, pattern, tile counts, masks)
    uint8_t *h_batch = nullptr;     // pinned: epoch words, job records, what the kernels report, the block to upload (made on first use)
    uint64_t batch_epoch = 0;       // the h_batch epoch word of a launch == batch_epoch: its report is there

    // pinned host staging
    uint64_t *h_hist = nullptr;     // 256
    uint32_t *h_enc = nullptr;      // 768 words: {code,len} x 256, then len x 256; HEADER_STAGE bytes: the file header on its way to the image
    uint8_t *h_header = nullptr;    // HEADER_STAGE
    uint8_t *h_lut_buf[2] = {};     // DEC_TABLES_BYTES each, used in turn: the host fills one while the other's upload may still be queued
    int lut_turn = 0;
    uint64_t *h_scalar = nullptr;   // HS_SLOTS words (HostScalar above)

    // link between et_histogram_device and et_encode_body_device
    const void *hist_text = nullptr;
    size_t hist_n = 0;
    uint32_t hist_rpt = 0, hist_tiles = 0;
    bool hist_on_host = false;  // h_hist holds the counts of hist_text
    bool hist_empty = false;    // the last et_histogram_device was of an empty text (zeros everywhere, no tiles)
    const void *scan_buf = nullptr;  // the group_sum buffer scan_epoch_n counts on
    size_t scan_cap = 0;
    uint32_t scan_epoch_n = 0;
    uint32_t report_epoch = 0;     // word FLAG_REPORT_EPOCH of the HS_BODY_FLAGS words == report_epoch: the current decode's flags and total are there
    uint64_t enc_block_epoch = 0;  // h_scalar[HS_ENC_TAKEN] == enc_block_epoch: the device has taken its copy of h_enc
    uint64_t header_epoch = 0;  // h_scalar[HS_HEADER_DONE] == header_epoch: the header bytes of the current decode are in h_header
    uint64_t hist_epoch = 0;    // h_hist[256 + w] == hist_epoch: reducing workgroup w of the current histogram has stored its totals

    hipEvent_t ev[12] = {};  // 0..5: encode calls, EV_DEC + 0..5: decode calls
    et_timings tm_enc = {}, tm_dec = {};
    // A full encode / body decode with timing on leaves its event arithmetic for the first
    // et_last_timings[_of] call (which waits for the call's last event): the call itself
    // then returns as asynchronously as it does with timing off.
    bool pend_enc = false, pend_dec = false, pend_enc_bits = false, pend_enc_shard = false, pend_dec_first = false;
    int last_kind = 0;  // 0 encode, 1 decode
    et_codebook last_cb = {};
    bool have_cb = false;


    // et_decode_range_sync / _maps + _resolve -> et_decode_range_write
    struct {
        bool valid = false;  // synchronised: the write may run
        Family family = Family::WINDOWS;  // what synchronised it
        Span s = {};
        et_codebook cb = {};  // s.cb
        uint64_t total = 0;
        // et_decode_range_maps -> et_decode_range_resolve
        bool maps_valid = false, maps_const = false;
    } range;
};

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

inline int fail(et_ctx *ctx, int status, const char *what, hipError_t e = hipSuccess) {
    if (ctx) {
        ctx->err = what;
        if (e != hipSuccess) {
            ctx->err += ": ";
            ctx->err += hipGetErrorString(e);
        }
    }
    return status;
}

#define ET_HIP(call)                                                     \
    do {                                                                 \
        hipError_t e_ = (call);                                          \
        if (e_ != hipSuccess) return fail(ctx, ET_ERR_HIP, #call, e_);   \
    } while (0)

inline int ensure(et_ctx *ctx, DevBuf &b, size_t bytes) {
    if (b.cap >= bytes) return ET_OK;
    if (b.p) {
        // Synchronising the current stream covers every stream the ctx ran on before it: each switch (switch_stream)
        // made the new stream wait for all the work the ctx had enqueued on the old one.
        ET_HIP(hipStreamSynchronize(ctx->stream));
        ET_HIP(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
        // What the buffer held is gone: the calls that would read it again find no first call (hist_empty stays: an empty
        // text's histogram is zeros, which et_histogram_host hands out without the device).
        if (b.holds & HOLDS_HISTOGRAM) ctx->hist_text = nullptr;
        if (b.holds & HOLDS_RANGE) ctx->range.valid = ctx->range.maps_valid = false;
    }
    const size_t want = (bytes + 4095) & ~static_cast<size_t>(4095);
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(ctx, e == hipErrorOutOfMemory ? ET_ERR_NOMEM : ET_ERR_HIP, "hipMalloc", e);
    }
    b.cap = want;
    return ET_OK;
}

#define ET_TRY(expr)                 \
    do {                             \
        int rc_ = (expr);            \
        if (rc_ != ET_OK) return rc_; \
    } while (0)

// A fresh epoch for k_scan_fused's published words in ctx->group_sum (call after the buffer is ensured): 1 .. 65535
// within one lifetime of the zeroed buffer; a new buffer, or the counter running out, zeroes it.
inline uint32_t scan_epoch(et_ctx *ctx) {
    if (ctx->group_sum.p != ctx->scan_buf || ctx->group_sum.cap != ctx->scan_cap || ctx->scan_epoch_n >= 0xffffu) {
        (void)hipMemsetAsync(ctx->group_sum.p, 0, ctx->group_sum.cap, ctx->stream);
        ctx->scan_buf = ctx->group_sum.p;
        ctx->scan_cap = ctx->group_sum.cap;
        ctx->scan_epoch_n = 0;
    }
    return ++ctx->scan_epoch_n;
}

inline void record(et_ctx *ctx, int i) {
    if (ctx->timing) (void)hipEventRecord(ctx->ev[i], ctx->stream);
}

constexpr int EV_DEC = 6;

// Events a timed kernel launch carries itself (begin = ev[a], end = ev[b]); none when timing is off.
inline et::KernelEvents timed(et_ctx *ctx, int a, int b) { return ctx->timing ? et::KernelEvents{ctx->ev[a], ctx->ev[b]} : et::KernelEvents{}; }

// The decode's write kernel: also when it alone is timed.
inline et::KernelEvents timed_body(et_ctx *ctx, int a, int b) {
    return ctx->timing || ctx->timing_body ? et::KernelEvents{ctx->ev[a], ctx->ev[b]} : et::KernelEvents{};
}

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Where a call needs an answer from the GPU before it can go on, a kernel stores the answer into pinned host memory and
// then `want` into *word, and the calling thread polls that word: no copy command, no completion signal, no wake-up
// (a stream wait returns ~10 us after the kernel).  After patience_ms without the word -- a stream blocked by somebody
// else's work, or a fault -- the stream wait takes over and reports.
template <typename T>
int wait_for_word(et_ctx *ctx, volatile const T *word, T want, double patience_ms, const char *what) {
    const double t0 = now_ms();
    for (uint32_t spin = 0; *word != want; ++spin)
        if ((spin & 1023u) == 1023u && now_ms() - t0 > patience_ms) {
            ET_HIP(hipStreamSynchronize(ctx->stream));
            if (*word != want) return fail(ctx, ET_ERR_HIP, what);
        }
    std::atomic_thread_fence(std::memory_order_acquire);
    return ET_OK;
}
