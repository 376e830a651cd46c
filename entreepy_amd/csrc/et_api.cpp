// et_api.cpp -- the extern "C" boundary of libentreepy_hip.so (include/entreepy_hip.h): context, workspaces, timings, the encode's
// orchestration of the kernels in et_kernels.hip, and the host-pointer / file-descriptor entry points.  The decode: et_decode.cpp.
//
// Encode (replaces encode.zig:25-337):
//   K1 histogram (totals stored into pinned host memory, polled) -> host code construction (et_codebook.cpp) -> K2 tile bit totals
//   (its first workgroup takes the code table and the header out of the pinned block) + scan -> K4 code scatter.
// There is no CPU fallback anywhere in this file: without a usable HIP device every
// entry point returns ET_ERR_HIP.
#include <sys/stat.h>

#include "et_ctx.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace {

// Tile geometry for a stream of `span` bytes measured from the aligned base.
struct Geometry {
    const uint8_t *base;
    uint64_t lo, hi;
    uint32_t rpt, n_tiles;
};

Geometry make_geometry(const et_ctx *ctx, const void *d_text, size_t n) {
    Geometry g;
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_text);
    g.base = reinterpret_cast<const uint8_t *>(a & ~static_cast<uintptr_t>(15));
    g.lo = a & 15;
    g.hi = g.lo + n;
    // Aim for >= 2048 tiles (one per resident K4 workgroup) before growing the tile towards 512 KiB: 1 GiB is 2048 tiles of
    // 512 KiB.  A tile costs K1 a flush of its 32 counter replicas between two barriers and K4 a shared seam word and a
    // restart of its ring; with 64 KiB tiles (round 2: 16384 of them for 1 GiB) that was ~2 % of a step (775-780 -> 792-797 GB/s),
    // and the tile scan reads 2 MiB of tile histograms instead of 16.
    uint32_t rpt = 1;
    while (rpt < et::MAX_ROUNDS_PER_TILE && g.hi / (static_cast<uint64_t>(rpt) * et::ROUND_BYTES) > 2048) rpt <<= 1;
    if (ctx && ctx->force_rpt) rpt = ctx->force_rpt;
    g.rpt = rpt;
    const uint64_t tile_bytes = static_cast<uint64_t>(rpt) * et::ROUND_BYTES;
    g.n_tiles = static_cast<uint32_t>((g.hi + tile_bytes - 1) / tile_bytes);
    return g;
}

int ensure_encode_ws(et_ctx *ctx, uint32_t n_tiles) {
    ET_TRY(ensure(ctx, ctx->tile_hist, static_cast<size_t>(n_tiles) * 256 * sizeof(uint32_t)));
    ET_TRY(ensure(ctx, ctx->block_hist, static_cast<size_t>(et::MAX_GRID) * 256 * sizeof(uint64_t)));
    ET_TRY(ensure(ctx, ctx->hist, 256 * sizeof(uint64_t)));
    ET_TRY(ensure(ctx, ctx->tile_bits, (static_cast<size_t>(n_tiles) + 1) * sizeof(uint64_t)));
    ET_TRY(ensure(ctx, ctx->tile_off, (static_cast<size_t>(n_tiles) + 1) * sizeof(uint64_t)));
    ET_TRY(ensure(ctx, ctx->enc_table, 768 * sizeof(uint32_t) + HEADER_STAGE));  // {code,len} x 256, then len x 256, then the file header: one upload
    ET_TRY(ensure(ctx, ctx->group_sum, (static_cast<size_t>(n_tiles) / 1024 + 2) * sizeof(uint64_t)));
    return ET_OK;
}

float elapsed(et_ctx *ctx, int a, int b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev[a], ctx->ev[b]) != hipSuccess) ms = 0.f;
    return ms;
}

int run_histogram(et_ctx *ctx, const void *d_text, size_t n, const Geometry &g, void *d_hist_also = nullptr) {
    ET_TRY(ensure_encode_ws(ctx, g.n_tiles));
    et::launch_hist(ctx->stream, g.base, g.lo, g.hi, g.rpt, g.n_tiles, static_cast<uint32_t *>(ctx->tile_hist.p),
                    static_cast<unsigned long long *>(ctx->block_hist.p), static_cast<unsigned long long *>(ctx->hist.p),
                    reinterpret_cast<unsigned long long *>(ctx->h_hist), ++ctx->hist_epoch, timed(ctx, 0, 1),  // (the totals land in h_hist too: fetch_histogram only waits)
                    static_cast<unsigned long long *>(d_hist_also));
    ET_HIP(hipGetLastError());
    ctx->hist_text = d_text;
    ctx->hist_empty = false;
    ctx->hist_n = n;
    ctx->hist_rpt = g.rpt;
    ctx->hist_tiles = g.n_tiles;
    ctx->hist_on_host = false;
    return ET_OK;
}

// Upload the code table and run K2 + K4 for the text whose tile histograms are in ctx.
int run_body(et_ctx *ctx, const et_codebook *cb, const Geometry &g, uint32_t *out32, uint64_t base_bit,
             const uint8_t *header, size_t header_len, int ev_scan, int ev_body) {
    const bool long_codes = cb->max_length > 32;
    // (the pinned block is read by the device itself, K2's first workgroup: not before that has happened for the call
    // before may it be filled again -- it says so in h_scalar[HS_ENC_TAKEN]; normally long ago)
    ET_TRY(wait_for_word<uint64_t>(ctx, ctx->h_scalar + HS_ENC_TAKEN, ctx->enc_block_epoch, 100.0, "the code table block was never taken"));
    for (int s = 0; s < 256; ++s) {
        const uint32_t len = cb->length[s];
        uint32_t code = cb->data[s];
        if (!long_codes) code = len ? (len == 32 ? code : (code & ((1u << len) - 1u)) << (32 - len)) : 0u;  // left-aligned
        ctx->h_enc[2 * s] = code;
        ctx->h_enc[2 * s + 1] = len;
        ctx->h_enc[512 + s] = len;
    }
    // The header rides behind the code table in ONE upload; the scan kernel copies it into the image
    // once the word holding the header/body seam is zeroed (no copy command between K2 and K4).
    const size_t padded = (header_len + 3) & ~static_cast<size_t>(3);
    if (header_len) {
        if (padded > HEADER_STAGE) return fail(ctx, ET_ERR_ARG, "header too long");
        uint8_t *stage = reinterpret_cast<uint8_t *>(ctx->h_enc + 768);
        std::memcpy(stage, header, header_len);
        std::memset(stage + header_len, 0, padded - header_len);
    }
    // (no upload: the code lengths ride in K2's kernel arguments, and its first workgroup copies the pinned block --
    // code table, lengths, header -- into enc_table for the kernels behind it)
    et::launch_tile_scan(ctx->stream, static_cast<const uint32_t *>(ctx->tile_hist.p), g.n_tiles, cb->length, ctx->h_enc, static_cast<uint32_t *>(ctx->enc_table.p),
                         static_cast<uint32_t>(768 + padded / 4), reinterpret_cast<unsigned long long *>(ctx->h_scalar + HS_ENC_TAKEN), ++ctx->enc_block_epoch,
                         static_cast<unsigned long long *>(ctx->tile_bits.p),
                         static_cast<unsigned long long *>(ctx->group_sum.p), scan_epoch(ctx), base_bit,
                         static_cast<unsigned long long *>(ctx->tile_off.p), out32, static_cast<const uint32_t *>(ctx->enc_table.p) + 768,
                         static_cast<uint32_t>(padded / 4));
    ET_HIP(hipGetLastError());
    et::launch_encode(ctx->stream, g.base, g.lo, g.hi, g.rpt, g.n_tiles, static_cast<const unsigned long long *>(ctx->tile_off.p),
                      static_cast<const uint2 *>(ctx->enc_table.p), cb->max_length, out32, timed(ctx, ev_scan, ev_body));  // K4 carries its two events
    ET_HIP(hipGetLastError());
    return ET_OK;
}

int fetch_histogram(et_ctx *ctx) {
    if (ctx->hist_on_host) return ET_OK;
    // k_hist_reduce stores the totals into h_hist and, behind them, one "done" word per workgroup (this sits between
    // the two halves of every encode)
    for (uint32_t w = 0; w < et::HIST_REDUCE_GROUPS; ++w)
        ET_TRY(wait_for_word<uint64_t>(ctx, ctx->h_hist + 256 + w, ctx->hist_epoch, 100.0, "the histogram never reached the host"));
    ctx->hist_on_host = true;
    return ET_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------
extern "C" const char *et_version(void) { return "entreepy-hip 0.1.0 (gfx950; .et format 0x01, reference v1.1.0)"; }

extern "C" const char *et_last_error(const et_ctx *ctx) { return ctx ? ctx->err.c_str() : ""; }


extern "C" int et_ctx_create(int device, et_ctx **out) {
    if (!out) return ET_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return ET_ERR_HIP;
    et_ctx *ctx = new (std::nothrow) et_ctx();
    if (!ctx) return ET_ERR_NOMEM;
    ctx->device = device;
    DeviceGuard guard(device);
    bool ok = guard.ok;
    ok = ok && hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) == hipSuccess;
    ctx->stream = ctx->own_stream;
    ok = ok && hipStreamCreateWithFlags(&ctx->side.stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&ctx->side.fork, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&ctx->side.join, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&ctx->switch_ev, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void **>(&ctx->h_hist), (256 + et::HIST_REDUCE_GROUPS) * sizeof(uint64_t)) == hipSuccess;
    if (ok) std::memset(ctx->h_hist, 0, (256 + et::HIST_REDUCE_GROUPS) * sizeof(uint64_t));  // (no workgroup's word reads as the first epoch)
    ok = ok && hipHostMalloc(reinterpret_cast<void **>(&ctx->h_enc), 768 * sizeof(uint32_t) + HEADER_STAGE) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void **>(&ctx->h_header), HEADER_STAGE) == hipSuccess;
    for (int i = 0; i < 2; ++i) ok = ok && hipHostMalloc(reinterpret_cast<void **>(&ctx->h_lut_buf[i]), DEC_TABLES_BYTES) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void **>(&ctx->h_scalar), HS_SLOTS * sizeof(uint64_t)) == hipSuccess;
    if (ok) std::memset(ctx->h_scalar, 0, HS_SLOTS * sizeof(uint64_t));
    for (int i = 0; i < 2; ++i) ok = ok && hipHostMalloc(reinterpret_cast<void **>(&ctx->h_tw_tree[i]), sizeof(et::TwUpload)) == hipSuccess;
    // timing-only events: no system-scope fence when they complete (hip_runtime_api.h: "for events that
    // are only being used to measure timing"); with the default flags the ten records of an
    // encode+decode cost ~65 us of cache write-backs and waits at 1 GiB
    for (auto &e : ctx->ev) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableSystemFence) == hipSuccess;
    if (!ok) {
        et_ctx_destroy(ctx);
        return ET_ERR_HIP;
    }
    *out = ctx;
    return ET_OK;
}

extern "C" void et_ctx_destroy(et_ctx *ctx) {
    if (!ctx) return;
    DeviceGuard guard(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);  // (and so every earlier stream of the ctx: switch_stream)
    DevBuf *bufs[] = {&ctx->tile_hist, &ctx->block_hist, &ctx->hist, &ctx->tile_bits, &ctx->tile_off, &ctx->enc_table, &ctx->group_sum,
                      &ctx->sub_state, &ctx->blk_exit, &ctx->blk_count, &ctx->blk_off, &ctx->lut, &ctx->flag,
                      &ctx->worklist, &ctx->lane_maps, &ctx->blk_maps, &ctx->grp_maps, &ctx->blk_in, &ctx->grp_in, &ctx->row_scratch,
                      &ctx->tw_table, &ctx->tw_tree, &ctx->blk_start, &ctx->blk_pub, &ctx->chain_table, &ctx->io_in, &ctx->io_out,
                      &ctx->batch_jobs, &ctx->batch_blob, &ctx->batch_counter, &ctx->packed_ws};
    for (DevBuf *b : bufs)
        if (b->p) (void)hipFree(b->p);
    delete ctx->io;
    void *pinned[] = {ctx->h_hist, ctx->h_enc, ctx->h_header, ctx->h_lut_buf[0], ctx->h_lut_buf[1], ctx->h_scalar, ctx->h_tw_tree[0], ctx->h_tw_tree[1], ctx->h_batch};
    for (void *p : pinned)
        if (p) (void)hipHostFree(p);
    for (auto &e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    if (ctx->side.stream) (void)hipStreamDestroy(ctx->side.stream);
    if (ctx->side.fork) (void)hipEventDestroy(ctx->side.fork);
    if (ctx->side.join) (void)hipEventDestroy(ctx->side.join);
    if (ctx->switch_ev) (void)hipEventDestroy(ctx->switch_ev);
    delete ctx;
}

namespace {

// The ctx onto stream s: s first waits for everything the ctx enqueued on its old stream.  Calls return before their last
// kernels finish (a decode's write pass, an encode's K4, a whole histogram), and the next call rewrites the workspaces
// those kernels still read; one event pair per switch keeps the next call behind them wherever it runs.
int switch_stream(et_ctx *ctx, hipStream_t s) {
    if (s == ctx->stream) return ET_OK;
    DeviceGuard guard(ctx->device);
    ET_HIP(hipEventRecord(ctx->switch_ev, ctx->stream));
    ET_HIP(hipStreamWaitEvent(s, ctx->switch_ev, 0));
    ctx->stream = s;
    return ET_OK;
}

}  // namespace

extern "C" int et_ctx_set_stream(et_ctx *ctx, void *hip_stream) {
    if (!ctx) return ET_ERR_ARG;
    return switch_stream(ctx, static_cast<hipStream_t>(hip_stream));
}

extern "C" int et_ctx_use_own_stream(et_ctx *ctx) {
    if (!ctx) return ET_ERR_ARG;
    return switch_stream(ctx, ctx->own_stream);
}

extern "C" void *et_ctx_stream(const et_ctx *ctx) { return ctx ? static_cast<void *>(ctx->stream) : nullptr; }

extern "C" int et_ctx_device(const et_ctx *ctx) { return ctx ? ctx->device : -1; }

extern "C" int et_ctx_set_tile_rounds(et_ctx *ctx, uint32_t rounds) {
    if (!ctx) return ET_ERR_ARG;
    if (rounds > et::MAX_ROUNDS_PER_TILE || (rounds & (rounds - 1))) return ET_ERR_ARG;
    ctx->force_rpt = rounds;
    ctx->hist_text = nullptr;  // tile histograms of another geometry are stale
    return ET_OK;
}

extern "C" int et_ctx_enable_timing(et_ctx *ctx, int on) {
    if (!ctx) return ET_ERR_ARG;
    ctx->timing = on != 0 && on != ET_TIMING_DECODE_BODY;
    ctx->timing_body = on == ET_TIMING_DECODE_BODY;
    ctx->pend_enc = ctx->pend_dec = false;  // (what an earlier mode left to be worked out is gone with its events)
    return ET_OK;
}

extern "C" int et_last_timings_of(et_ctx *ctx, int which, et_timings *out) {
    if (!ctx || !out || which < 0 || which > 1) return ET_ERR_ARG;
    DeviceGuard guard(ctx->device);
    if (which == 0 && ctx->pend_enc) {
        ET_HIP(hipEventSynchronize(ctx->ev[3]));
        if (!ctx->pend_enc_shard) {  // (a shard encode's histogram was a call of its own, hist_ms is its)
            ctx->tm_enc.hist_ms = elapsed(ctx, 0, 1);
            ctx->tm_enc.total_ms = elapsed(ctx, 0, 3);
        }
        ctx->tm_enc.scan_ms = ctx->pend_enc_bits ? elapsed(ctx, 1, 2) : 0.f;  // everything between K1 and K4: histogram reduce, host code construction, tile scan, uploads
        ctx->tm_enc.body_ms = elapsed(ctx, 2, 3);
        ctx->pend_enc = ctx->pend_enc_shard = false;
    }
    if (which == 1 && ctx->pend_dec && ctx->timing_body) {  // the write kernel's own pair is all there is
        ET_HIP(hipEventSynchronize(ctx->ev[EV_DEC + 3]));
        ctx->tm_dec.body_ms = elapsed(ctx, EV_DEC + 2, EV_DEC + 3);
        ctx->pend_dec = false;
    }
    if (which == 1 && ctx->pend_dec) {
        ET_HIP(hipEventSynchronize(ctx->ev[EV_DEC + 3]));
        // events 0/5 = begin/end of the first sweep's main kernel, 2/3 = of the write kernel
        ctx->tm_dec.sync_ms = elapsed(ctx, EV_DEC + 0, EV_DEC + 2);  // everything before the write: sweeps, check, scan
        ctx->tm_dec.scan_ms = elapsed(ctx, EV_DEC + 5, EV_DEC + 2);  // ... of which after the first sweep (repair sweep, verification, scan)
        ctx->tm_dec.body_ms = elapsed(ctx, EV_DEC + 2, EV_DEC + 3);
        ctx->tm_dec.total_ms = elapsed(ctx, EV_DEC + 0, EV_DEC + 3);
        ctx->tm_dec.sync_first_ms = ctx->pend_dec_first ? elapsed(ctx, EV_DEC + 0, EV_DEC + 5) : 0.f;
        ctx->pend_dec = false;
    }
    *out = which == 0 ? ctx->tm_enc : ctx->tm_dec;
    return ET_OK;
}

extern "C" int et_last_timings(et_ctx *ctx, et_timings *out) {
    if (!ctx) return ET_ERR_ARG;
    return et_last_timings_of(ctx, ctx->last_kind, out);
}

extern "C" int et_last_codebook(const et_ctx *ctx, et_codebook *out) {
    if (!ctx || !out) return ET_ERR_ARG;
    if (!ctx->have_cb) return ET_ERR_ARG;
    *out = ctx->last_cb;
    return ET_OK;
}

extern "C" int et_ctx_reserve(et_ctx *ctx, size_t max_text_bytes) {
    if (!ctx) return ET_ERR_ARG;
    DeviceGuard guard(ctx->device);
    const Geometry g = make_geometry(nullptr, reinterpret_cast<const void *>(static_cast<uintptr_t>(15)), max_text_bytes);
    ET_TRY(ensure_encode_ws(ctx, g.n_tiles + 1));  // size-based geometry; a forced smaller tile grows on demand
    // decode: the body is at most ~max_text_bytes (+ header) bytes
    const uint64_t n_subs = (static_cast<uint64_t>(max_text_bytes) + 8192) * 8 / et::SUB_BITS + 2;
    const uint64_t n_blocks = n_subs / et::BLOCK + 2;
    ET_TRY(ensure(ctx, ctx->sub_state, n_subs * sizeof(uint32_t)));
    ET_TRY(ensure(ctx, ctx->blk_exit, n_blocks * sizeof(uint32_t)));
    ET_TRY(ensure(ctx, ctx->blk_count, n_blocks * sizeof(uint32_t)));
    ET_TRY(ensure(ctx, ctx->blk_off, (n_blocks + 1) * sizeof(uint64_t)));
    ET_TRY(ensure(ctx, ctx->worklist, (n_blocks + 1) * sizeof(uint32_t)));
    ET_TRY(ensure(ctx, ctx->group_sum, (n_blocks / 1024 + 2) * sizeof(uint64_t)));
    ET_TRY(ensure(ctx, ctx->lut, DEC_TABLES_BYTES));
    ET_TRY(ensure(ctx, ctx->flag, et::DEC_FLAG_WORDS * sizeof(uint32_t)));
    ET_TRY(ensure(ctx, ctx->tw_table, static_cast<size_t>(et::tw_table_entries(et::TW_MAX_NODES)) * sizeof(uint16_t) + 64));
    ET_TRY(ensure(ctx, ctx->tw_tree, sizeof(et::TwUpload)));
    ET_TRY(ensure(ctx, ctx->chain_table, static_cast<size_t>(et::CH_MAX_ENTRIES) * sizeof(uint64_t)));
    ET_TRY(ensure(ctx, ctx->blk_start, n_blocks * sizeof(uint32_t)));
    return ET_OK;
}

// ---------------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------------
extern "C" int et_histogram_device(et_ctx *ctx, const void *d_text, size_t n, void *d_hist) {
    if (!ctx || (n && !d_text)) return ET_ERR_ARG;
    DeviceGuard guard(ctx->device);
    if (n == 0) {
        ET_TRY(ensure(ctx, ctx->hist, 256 * sizeof(uint64_t)));
        ET_HIP(hipMemsetAsync(ctx->hist.p, 0, 256 * sizeof(uint64_t), ctx->stream));
        if (d_hist) ET_HIP(hipMemsetAsync(d_hist, 0, 256 * sizeof(uint64_t), ctx->stream));
        std::memset(ctx->h_hist, 0, 256 * sizeof(uint64_t));
        ctx->hist_text = nullptr;
        ctx->hist_empty = true;
        return ET_OK;
    }
    ctx->hist_empty = false;
    const Geometry g = make_geometry(ctx, d_text, n);
    ET_TRY(run_histogram(ctx, d_text, n, g, d_hist));  // (K1 carries events 0 and 1; the reduction stores the totals into d_hist as well: no copy behind it)
    if (ctx->timing) {
        ET_HIP(hipStreamSynchronize(ctx->stream));
        ctx->tm_enc = et_timings{};
        ctx->tm_enc.hist_ms = elapsed(ctx, 0, 1);
        ctx->pend_enc = false;
        ctx->last_kind = 0;
    }
    return ET_OK;
}

namespace {

int encode_shard(et_ctx *ctx, const et_codebook *cb, const void *d_text, size_t n, void *d_out, size_t cap_bytes, uint64_t start_bit,
                 const uint8_t *header, size_t header_len, uint64_t *end_bit) {
    if (!ctx || !cb || !d_out || !end_bit || (n && !d_text)) return ET_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(d_out) & 3) return fail(ctx, ET_ERR_ARG, "d_out must be 4-byte aligned");
    if (header_len > HEADER_STAGE - 4) return fail(ctx, ET_ERR_ARG, "header too long");
    DeviceGuard guard(ctx->device);
    // A shard without text, or with nothing but zero-length symbols, still owns the word its start bit lies
    // in: that word (after the header, padded to a word, for the head shard) is written as zeros, so that a
    // concatenation which ORs pieces together never reads what an earlier call left in d_out.
    auto empty_shard = [&]() -> int {
        const size_t head_words = (header_len + 3) / 4;
        const size_t own_word = header_len ? 0 : static_cast<size_t>(start_bit / 32);  // (a body shard's start bit may lie behind d_out's first word)
        const size_t need = (header_len ? head_words : own_word + 1) * 4;
        if (need > cap_bytes) return fail(ctx, ET_ERR_CAP, "body does not fit d_out");
        if (header_len) {
            std::memset(ctx->h_header, 0, head_words * 4);
            std::memcpy(ctx->h_header, header, header_len);
            ET_HIP(hipMemcpyAsync(d_out, ctx->h_header, head_words * 4, hipMemcpyHostToDevice, ctx->stream));
        } else {
            ET_HIP(hipMemsetAsync(static_cast<uint8_t *>(d_out) + own_word * 4, 0, 4, ctx->stream));
        }
        *end_bit = start_bit;
        return ET_OK;
    };
    if (n == 0) {
        ET_HIP(hipStreamSynchronize(ctx->stream));  // pinned staging may still feed an earlier call
        return empty_shard();
    }
    if (ctx->hist_text != d_text || ctx->hist_n != n)
        return fail(ctx, ET_ERR_ARG, "shard encode needs et_histogram_device on the same (d_text, n) first");
    ET_TRY(fetch_histogram(ctx));
    ET_HIP(hipStreamSynchronize(ctx->stream));  // pinned staging may still feed an earlier call
    uint64_t bits = 0;
    et_codebook_bits(cb, ctx->h_hist, &bits);
    const uint64_t end = start_bit + bits;
    if (((end + 31) / 32) * 4 > cap_bytes) return fail(ctx, ET_ERR_CAP, "body does not fit d_out");
    if (header_len) {
        std::memset(ctx->h_header, 0, HEADER_STAGE);
        std::memcpy(ctx->h_header, header, header_len);
    }
    Geometry g = make_geometry(ctx, d_text, n);
    g.rpt = ctx->hist_rpt;
    g.n_tiles = ctx->hist_tiles;
    if (bits == 0) return empty_shard();  // nothing but zero-length symbols
    ET_TRY(run_body(ctx, cb, g, static_cast<uint32_t *>(d_out), start_bit, header_len ? ctx->h_header : nullptr, header_len, 2, 3));
    *end_bit = end;
    if (ctx->timing) {  // hist_ms is already there (et_histogram_device); the rest when asked for
        ctx->pend_enc = true;
        ctx->pend_enc_bits = true;
        ctx->pend_enc_shard = true;
        ctx->last_kind = 0;
    }
    return ET_OK;
}

}  // namespace

extern "C" int et_histogram_host(et_ctx *ctx, uint64_t counts[256]) {
    if (!ctx || !counts) return ET_ERR_ARG;
    if (ctx->hist_empty) {  // an empty shard's: zeros
        std::memset(counts, 0, 256 * sizeof(uint64_t));
        return ET_OK;
    }
    if (!ctx->hist_text) return fail(ctx, ET_ERR_ARG, "no current histogram (et_histogram_device first)");
    DeviceGuard guard(ctx->device);
    ET_TRY(fetch_histogram(ctx));
    std::memcpy(counts, ctx->h_hist, 256 * sizeof(uint64_t));
    return ET_OK;
}

extern "C" int et_histogram_device_ptr(et_ctx *ctx, const void **d_hist) {
    if (!ctx || !d_hist) return ET_ERR_ARG;
    if (!ctx->hist_text && !ctx->hist_empty) return fail(ctx, ET_ERR_ARG, "no current histogram (et_histogram_device first)");
    *d_hist = ctx->hist.p;
    return ET_OK;
}

extern "C" int et_histogram_on_host(et_ctx *ctx, const uint64_t counts[256]) {
    if (!ctx || !counts) return ET_ERR_ARG;
    if (!ctx->hist_text) return fail(ctx, ET_ERR_ARG, "no current histogram (et_histogram_device first)");
    std::memcpy(ctx->h_hist, counts, 256 * sizeof(uint64_t));
    ctx->hist_on_host = true;
    return ET_OK;
}

extern "C" int et_encode_body_device(et_ctx *ctx, const et_codebook *cb, const void *d_text, size_t n, void *d_out, size_t cap_bytes,
                                     uint64_t start_bit, uint64_t *end_bit) {
    return encode_shard(ctx, cb, d_text, n, d_out, cap_bytes, start_bit, nullptr, 0, end_bit);
}

extern "C" int et_encode_head_shard_device(et_ctx *ctx, const et_codebook *cb, const void *d_text, size_t n, void *d_out, size_t cap_bytes,
                                           const uint8_t *header, size_t header_len, uint64_t *end_bit) {
    if (!header || !header_len) return ET_ERR_ARG;
    return encode_shard(ctx, cb, d_text, n, d_out, cap_bytes, static_cast<uint64_t>(header_len) * 8, header, header_len, end_bit);
}

extern "C" int et_encode_device(et_ctx *ctx, const void *d_text, size_t n, void *d_out, size_t cap, size_t *out_len) {
    if (!ctx || !d_out || !out_len || (n && !d_text)) return ET_ERR_ARG;
    *out_len = 0;
    if (n == 0) return fail(ctx, ET_ERR_EMPTY, "empty input");
    if (reinterpret_cast<uintptr_t>(d_out) & 15) return fail(ctx, ET_ERR_ARG, "d_out must be 16-byte aligned");
    if (cap < et_encode_bound(n)) return fail(ctx, ET_ERR_CAP, "cap < et_encode_bound(n)");
    DeviceGuard guard(ctx->device);
    const Geometry g = make_geometry(ctx, d_text, n);
    ET_TRY(run_histogram(ctx, d_text, n, g));  // (K1 carries events 0 and 1)
    ET_TRY(fetch_histogram(ctx));
    const double t1 = now_ms();

    et_codebook cb;
    int rc = et_build_codebook(ctx->h_hist, &cb);
    if (rc != ET_OK) return fail(ctx, rc, "et_build_codebook");
    ctx->last_cb = cb;
    ctx->have_cb = true;
    size_t header_len = 0;
    std::memset(ctx->h_header, 0, HEADER_STAGE);
    rc = et_write_header(&cb, n, ctx->h_header, HEADER_STAGE - 4, &header_len);
    if (rc != ET_OK) return fail(ctx, rc, "et_write_header");
    uint64_t bits = 0;
    et_codebook_bits(&cb, ctx->h_hist, &bits);
    const double t2 = now_ms();

    if (bits == 0) {
        // Single distinct symbol: the whole file is the 9-byte header (encode.zig:137-138, :270-275).
        const size_t padded = (header_len + 3) & ~static_cast<size_t>(3);
        ET_HIP(hipMemcpyAsync(d_out, ctx->h_header, padded, hipMemcpyHostToDevice, ctx->stream));
        record(ctx, 2);
        record(ctx, 3);
    } else {
        ET_TRY(run_body(ctx, &cb, g, static_cast<uint32_t *>(d_out), static_cast<uint64_t>(header_len) * 8, ctx->h_header, header_len, 2, 3));
    }
    *out_len = header_len + static_cast<size_t>((bits + 7) / 8);  // encode.zig:318,336
    if (ctx->timing) {
        ctx->tm_enc = et_timings{};
        ctx->tm_enc.host_ms = static_cast<float>(t2 - t1);
        ctx->pend_enc = true;
        ctx->pend_enc_bits = bits != 0;
        ctx->pend_enc_shard = false;
        ctx->last_kind = 0;
    }
    return ET_OK;
}

namespace {

// The staging pipeline of the host-pointer / fd entry points (et_io.h).
int ensure_io(et_ctx *ctx) {
    if (ctx->io) return ET_OK;
    size_t chunk = 32u << 20;
    int threads = static_cast<int>(std::thread::hardware_concurrency() / 2);
    if (threads > 8) threads = 8;
    if (const char *e = std::getenv("ET_IO_CHUNK_MB")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 1 && v <= 1024) chunk = static_cast<size_t>(v) << 20;
    }
    if (const char *e = std::getenv("ET_IO_THREADS")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 1 && v <= 64) threads = static_cast<int>(v);
    }
    ctx->io = new (std::nothrow) et_io::Pipe();
    if (!ctx->io || !ctx->io->init(chunk, threads)) {
        delete ctx->io;
        ctx->io = nullptr;
        return fail(ctx, ET_ERR_NOMEM, "pinned staging buffers");
    }
    return ET_OK;
}

int io_status(et_ctx *ctx, int rc, const char *what) {
    if (rc == 0) return ET_OK;
    if (rc == -1) return fail(ctx, ET_ERR_IO, what);
    return fail(ctx, ET_ERR_HIP, what, ctx->io->last_hip);
}

int file_size(int fd, uint64_t *size) {
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) return -1;
    *size = static_cast<uint64_t>(st.st_size);
    return 0;
}

// encode: source -> io_in -> kernels -> io_out -> sink
int encode_through_pipe(et_ctx *ctx, const et_io::HostEnd &src, size_t n, const et_io::HostEnd *dst, size_t cap, size_t *out_len) {
    *out_len = 0;
    if (n == 0) return fail(ctx, ET_ERR_EMPTY, "empty input");
    const size_t bound = et_encode_bound(n);
    ET_TRY(ensure_io(ctx));
    ET_TRY(ensure(ctx, ctx->io_in, n + 16));
    ET_TRY(ensure(ctx, ctx->io_out, bound + 16));
    ET_TRY(io_status(ctx, ctx->io->upload(ctx->stream, ctx->io_in.p, src, n), "reading the input"));
    size_t len = 0;
    ET_TRY(et_encode_device(ctx, ctx->io_in.p, n, ctx->io_out.p, bound, &len));
    if (len > cap) return fail(ctx, ET_ERR_CAP, "output buffer too small");
    if (dst) ET_TRY(io_status(ctx, ctx->io->download(ctx->stream, *dst, ctx->io_out.p, len), "writing the output"));
    else ET_HIP(hipStreamSynchronize(ctx->stream));
    *out_len = len;
    return ET_OK;
}

}  // namespace

extern "C" int et_encode(et_ctx *ctx, const uint8_t *text, size_t n, uint8_t *out, size_t cap, size_t *out_len) {
    if (!ctx || !out || !out_len || (n && !text)) return ET_ERR_ARG;
    DeviceGuard guard(ctx->device);
    et_io::HostEnd src, dst;
    src.ptr = const_cast<uint8_t *>(text);
    dst.ptr = out;
    return encode_through_pipe(ctx, src, n, &dst, cap, out_len);
}

extern "C" int et_encode_fd(et_ctx *ctx, int in_fd, int out_fd, size_t *in_len, size_t *out_len) {
    if (!ctx || !in_len || !out_len || in_fd < 0) return ET_ERR_ARG;
    *in_len = *out_len = 0;
    uint64_t n = 0;
    if (file_size(in_fd, &n) != 0) return fail(ctx, ET_ERR_IO, "input is not a regular file");
    DeviceGuard guard(ctx->device);
    et_io::HostEnd src, dst;
    src.fd = in_fd;
    dst.fd = out_fd;
    *in_len = static_cast<size_t>(n);
    return encode_through_pipe(ctx, src, static_cast<size_t>(n), out_fd >= 0 ? &dst : nullptr, ~static_cast<size_t>(0), out_len);
}

extern "C" int et_fd_to_device(et_ctx *ctx, int fd, uint64_t file_offset, size_t len, void *d_dst) {
    if (!ctx || fd < 0 || (len && !d_dst)) return ET_ERR_ARG;
    if (len == 0) return ET_OK;
    DeviceGuard guard(ctx->device);
    ET_TRY(ensure_io(ctx));
    et_io::HostEnd src;
    src.fd = fd;
    src.offset = file_offset;
    return io_status(ctx, ctx->io->upload(ctx->stream, d_dst, src, len), "reading the input");
}

extern "C" int et_device_to_fd(et_ctx *ctx, const void *d_src, size_t len, int fd, uint64_t file_offset) {
    if (!ctx || fd < 0 || (len && !d_src)) return ET_ERR_ARG;
    if (len == 0) return ET_OK;
    DeviceGuard guard(ctx->device);
    ET_TRY(ensure_io(ctx));
    et_io::HostEnd dst;
    dst.fd = fd;
    dst.offset = file_offset;
    return io_status(ctx, ctx->io->download(ctx->stream, dst, d_src, len), "writing the output");
}

namespace {

// decode: source -> io_in (header parsed from the bytes as they pass) -> kernels -> io_out -> sink
int decode_through_pipe(et_ctx *ctx, const et_io::HostEnd &src, size_t len, const et_io::HostEnd *dst, size_t cap, size_t *out_len) {
    *out_len = 0;
    if (len < 5) return fail(ctx, ET_ERR_FORMAT, "stream shorter than its header");
    ET_TRY(ensure_io(ctx));
    ET_TRY(ensure(ctx, ctx->io_in, len + 16));
    std::vector<uint8_t> head(len < HEADER_STAGE ? len : HEADER_STAGE);
    ET_TRY(io_status(ctx, ctx->io->upload(ctx->stream, ctx->io_in.p, src, len, head.data(), head.size()), "reading the input"));
    et_codebook cb;
    uint64_t n_symbols = 0;
    size_t body_offset = 0;
    const int rc = et_parse_header(head.data(), head.size(), &cb, &n_symbols, &body_offset);
    if (rc != ET_OK) return fail(ctx, rc, "et_parse_header");
    if (body_offset > len) return fail(ctx, ET_ERR_FORMAT, "dictionary runs past the end of the stream");
    ET_TRY(ensure(ctx, ctx->io_out, n_symbols + 64));
    size_t n_out = 0;
    ET_TRY(et_decode_body_device(ctx, &cb, static_cast<const uint8_t *>(ctx->io_in.p) + body_offset, len - body_offset, 0, n_symbols, ctx->io_out.p,
                                 n_symbols + 64, &n_out));
    if (n_out > cap) return fail(ctx, ET_ERR_CAP, "output buffer too small");
    if (dst && n_out) ET_TRY(io_status(ctx, ctx->io->download(ctx->stream, *dst, ctx->io_out.p, n_out), "writing the output"));
    else ET_HIP(hipStreamSynchronize(ctx->stream));
    *out_len = n_out;
    return ET_OK;
}

}  // namespace

extern "C" int et_decode(et_ctx *ctx, const uint8_t *compressed, size_t len, uint8_t *out, size_t cap, size_t *out_len) {
    if (!ctx || !compressed || !out_len) return ET_ERR_ARG;
    DeviceGuard guard(ctx->device);
    et_io::HostEnd src, dst;
    src.ptr = const_cast<uint8_t *>(compressed);
    dst.ptr = out;
    return decode_through_pipe(ctx, src, len, out ? &dst : nullptr, out ? cap : 0, out_len);
}

extern "C" int et_decode_fd(et_ctx *ctx, int in_fd, size_t in_skip, int out_fd, size_t *in_len, size_t *out_len) {
    if (!ctx || !in_len || !out_len || in_fd < 0) return ET_ERR_ARG;
    *in_len = *out_len = 0;
    uint64_t size = 0;
    if (file_size(in_fd, &size) != 0) return fail(ctx, ET_ERR_IO, "input is not a regular file");
    if (size < in_skip) return fail(ctx, ET_ERR_FORMAT, "file shorter than the bytes to skip");
    DeviceGuard guard(ctx->device);
    et_io::HostEnd src, dst;
    src.fd = in_fd;
    src.offset = in_skip;
    dst.fd = out_fd;
    *in_len = static_cast<size_t>(size - in_skip);
    return decode_through_pipe(ctx, src, *in_len, out_fd >= 0 ? &dst : nullptr, ~static_cast<size_t>(0), out_len);
}
