// et_decode.cpp -- the decode behind the extern "C" boundary of libentreepy_hip.so (include/entreepy_hip.h): the decode tables, the path
// planners, and the orchestration of the kernels in et_kernels.hip, et_treewalk.hip, et_rowsync.hip and et_kernels_fallback.hip.
//
// Decode (replaces decode.zig:13-220):
//   header to pinned host memory (polled) -> host parse, the code as a tree + the chained tables' plan -> k_tw_build -> D1
//   synchronisation by tree walk (one launch; repair sweeps only if the verification fails) -> D2 scan of the blocks' symbol counts
//   (+ verification, report to the host) -> D3 write over chained tables.  Complete codes of 7- and 8-bit codewords (uniform-like
//   bytes): k_row_sync -> D2 -> k_row_write (et_rowsync.h); fixed-length codes (2^L codewords of L bits): k_fixed_write alone.
//   Anything outside those domains: et_kernels_fallback.hip.
// A whole stream (et_decode_body_device) and a range of one split over GPUs (et_decode_range_*) are both a Span (et_ctx.h) and run
// the same stages over it.  The host-pointer / file-descriptor entry points (et_decode, et_decode_fd) are et_api.cpp's, with the I/O.
// There is no CPU fallback anywhere in this file: without a usable HIP device every entry point returns ET_ERR_HIP.
#include "et_ctx.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

// ---------------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------------
namespace {

// The switches that overrule the decode's choices, each ET_<NAME>=1 (A/B runs, and the tests that pin the paths
// behind them, in child processes), read once per process.  Value-initialised: the choices as they are.
struct DecodeSwitches {
    bool no_quick_sync, quick_sync_always, no_fixed_sync, no_fixed_write, no_row_sync, no_row_write, no_strips, dec_tables_host;
};

const DecodeSwitches &decode_switches() {
    static const DecodeSwitches sw = [] {
        auto on = [](const char *name) { const char *e = std::getenv(name); return e && e[0] == '1'; };
        return DecodeSwitches{on("ET_NO_QUICK_SYNC"), on("ET_QUICK_SYNC_ALWAYS"), on("ET_NO_FIXED_SYNC"), on("ET_NO_FIXED_WRITE"),
                              on("ET_NO_ROW_SYNC"),   on("ET_NO_ROW_WRITE"),      on("ET_NO_STRIPS"),     on("ET_DEC_TABLES_HOST")};
    }();
    return sw;
}

using et::HostDecodeTables;
using et::table_at;
using Layout = et::DecTableLayout;

// The decode tables of cb into the ctx's device block (et_tables.h DecTableLayout), and the two views of them the kernels
// take: ONE set of first/second-level tables + long list in the older format (index DEC_LUT_BITS_WRITE, two symbols per
// entry) for the LDS-window kernels -- first/last blocks, ranges, the exhaustive path -- and the slow path of the step walks,
// with the step table of the register-window sweeps (k_dec_sync_reg: index DEC_STEP_BITS_DEFAULT, symbol-free) in *tb_out and
// the write's (k_dec_write_reg: index DEC_LUT_BITS_WRITE, two symbols) in *tb_write_out.  The host only decides -- widths,
// second-level tables, long-list order: a TablePlan -- and uploads the plan and the two structs; k_build_dec_tables fills the
// tables.  ET_DEC_TABLES_HOST=1: the host builders fill a pinned block instead, and one copy uploads it as far as it is in use.
// (A three-symbol set for the counting kernels used to be built as well: 12 us of host time per call for kernels that now see
// three blocks of a stream; near-fixed-length codes, the exhaustive path's domain, rarely fit two codes in an index anyway.)
// zero16 / zeroed (optional): 16 device words the table-building kernel clears on its way, and
// whether it did (the host-built variant has no kernel: the caller clears them itself).
int prepare_decode_tables(et_ctx *ctx, const et_codebook *cb, et::DecodeTables *tb_out, et::DecodeTables *tb_write_out, uint32_t *zero16 = nullptr,
                          bool *zeroed = nullptr) {
    if (zeroed) *zeroed = false;
    ET_TRY(ensure(ctx, ctx->lut, DEC_TABLES_BYTES));
    ET_TRY(ensure(ctx, ctx->flag, et::DEC_FLAG_WORDS * sizeof(uint32_t)));
    // Two pinned blocks used in turn, and no wait here: every caller waits for something enqueued
    // behind this upload before it returns (the decode for its flags, the range calls and the
    // self-test for the stream), so the upload from the block filled two calls ago is long done and
    // the host can fill this one while the stream is still busy with whatever precedes this decode.
    uint8_t *h_lut = ctx->h_lut_buf[ctx->lut_turn ^= 1], *d_lut = static_cast<uint8_t *>(ctx->lut.p);
    const bool on_host = decode_switches().dec_tables_host;  // (the host builders are what the device's tables are tested against)
    HostDecodeTables hw;
    uint32_t step_bits = 0, step_sub_bits = 0, n_step_sub = 0, wstep_bits = 0, wstep_sub_bits = 0, n_wstep_sub = 0;
    et::TablePlan plan;
    if (on_host) {
        et::build_decode_tables(cb, et::DEC_LUT_BITS_WRITE, et::DEC_WRITE_SYMS, table_at<uint32_t>(h_lut, Layout::LUT), table_at<uint32_t>(h_lut, Layout::LONG),
                            table_at<uint16_t>(h_lut, Layout::SUB), &hw);
        std::memcpy(h_lut + Layout::SYM_LEN, cb->length, Layout::SYM_LEN_BYTES);
        step_bits = et::build_step_table(cb, et::DEC_STEP_BITS_DEFAULT, table_at<uint32_t>(h_lut, Layout::STEPS), &step_sub_bits, &n_step_sub);
    } else {
        et::plan_tables(cb, et::DEC_LUT_BITS_WRITE, et::DEC_WRITE_SYMS, et::DEC_STEP_BITS_DEFAULT, et::DEC_LUT_BITS_WRITE, &plan);
        hw = HostDecodeTables{plan.lut_bits, plan.n_long, plan.sub_bits, plan.n_sub};
        step_bits = plan.step_bits;
        step_sub_bits = plan.step_sub_bits;
        n_step_sub = plan.n_step_sub;
        wstep_bits = plan.wstep_bits;
        wstep_sub_bits = plan.wstep_sub_bits;
        n_wstep_sub = plan.n_wstep_sub;
    }
    const size_t wsteps_at = Layout::STEPS + et::step_table_bytes(step_bits, step_sub_bits, n_step_sub);  // right behind, one upload
    if (on_host) wstep_bits = et::build_write_step_table(cb, et::DEC_LUT_BITS_WRITE, table_at<uint32_t>(h_lut, wsteps_at), &wstep_sub_bits, &n_wstep_sub);
    // device copies of the two structs ride behind the tables (slow path of the step walks), the plan behind them
    const size_t structs_at = wsteps_at + et::step_table_bytes(wstep_bits, wstep_sub_bits, n_wstep_sub), plan_at = structs_at + 2 * sizeof(et::DecodeTables);
    const et::DecodeTables *d_structs = table_at<const et::DecodeTables>(d_lut, structs_at);
    et::DecodeTables &tb = *tb_out, &tbw = *tb_write_out;
    tb = et::DecodeTables{table_at<uint32_t>(d_lut, Layout::LUT), table_at<uint32_t>(d_lut, Layout::LONG), table_at<uint16_t>(d_lut, Layout::SUB), d_lut + Layout::SYM_LEN, hw.lut_bits, hw.n_long,
                          hw.sub_bits, hw.n_sub, table_at<uint32_t>(d_lut, Layout::STEPS), step_bits, step_sub_bits, n_step_sub, d_structs};
    tbw = tb;  // the same tables, another step table
    tbw.steps = table_at<uint32_t>(d_lut, wsteps_at);
    tbw.step_bits = wstep_bits;
    tbw.step_sub_bits = wstep_sub_bits;
    tbw.n_step_sub = n_wstep_sub;
    tbw.dev_copy = d_structs + 1;
    et::DecodeTables *h_structs = table_at<et::DecodeTables>(h_lut, structs_at);
    h_structs[0] = tb;
    h_structs[1] = tbw;
    if (on_host) {
        ET_HIP(hipMemcpyAsync(d_lut, h_lut, plan_at, hipMemcpyHostToDevice, ctx->stream));
    } else {
        std::memcpy(h_lut + plan_at, &plan, sizeof plan);
        ET_HIP(hipMemcpyAsync(d_lut + structs_at, h_structs, 2 * sizeof(et::DecodeTables) + sizeof plan, hipMemcpyHostToDevice, ctx->stream));
        et::launch_build_dec_tables(ctx->stream, d_lut, wsteps_at, plan_at, zero16);
        ET_HIP(hipGetLastError());
        if (zeroed) *zeroed = zero16 != nullptr;
    }
    return ET_OK;
}

}  // namespace

extern "C" int et_selftest_decode_tables(et_ctx *ctx, const et_codebook *cb, int *where) {
    if (!ctx || !cb || !where) return ET_ERR_ARG;
    *where = 0;
    if (cb->max_length > 32 || cb->n_coded == 0) return fail(ctx, ET_ERR_UNSUPPORTED, "no decode tables for this code table");
    DeviceGuard guard(ctx->device);
    ctx->range.valid = ctx->range.maps_valid = false;  // shares the tables (ctx->lut)
    et::DecodeTables tb, tbw;
    ET_TRY(prepare_decode_tables(ctx, cb, &tb, &tbw));  // the device's (unless ET_DEC_TABLES_HOST=1: then this compares the host's with themselves)
    std::vector<uint8_t> dev(DEC_TABLES_BYTES);
    ET_HIP(hipMemcpyAsync(dev.data(), ctx->lut.p, DEC_TABLES_BYTES, hipMemcpyDeviceToHost, ctx->stream));
    ET_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<uint32_t> lut(Layout::LUT_BYTES / sizeof(uint32_t)), longc(Layout::LONG_BYTES / sizeof(uint32_t)), steps(Layout::STEPS_BYTES / sizeof(uint32_t)),
        wsteps(Layout::WSTEPS_BYTES / sizeof(uint32_t));
    std::vector<uint16_t> sub(Layout::SUB_BYTES / sizeof(uint16_t));
    HostDecodeTables hw;
    et::build_decode_tables(cb, et::DEC_LUT_BITS_WRITE, et::DEC_WRITE_SYMS, lut.data(), longc.data(), sub.data(), &hw);
    uint32_t ssb = 0, nss = 0, wsb = 0, nws = 0;
    const uint32_t sbits = et::build_step_table(cb, et::DEC_STEP_BITS_DEFAULT, steps.data(), &ssb, &nss);
    const uint32_t wbits = et::build_write_step_table(cb, et::DEC_LUT_BITS_WRITE, wsteps.data(), &wsb, &nws);
    auto at = [&](const void *dptr) { return dev.data() + (static_cast<const uint8_t *>(dptr) - static_cast<const uint8_t *>(ctx->lut.p)); };
    const bool meta_ok = hw.lut_bits == tbw.lut_bits && hw.n_long == tbw.n_long && hw.sub_bits == tbw.sub_bits && hw.n_sub == tbw.n_sub &&
                         sbits == tb.step_bits && ssb == tb.step_sub_bits && nss == tb.n_step_sub && wbits == tbw.step_bits &&
                         wsb == tbw.step_sub_bits && nws == tbw.n_step_sub;
    if (!meta_ok) *where = 7;
    else if (std::memcmp(at(tbw.lut), lut.data(), sizeof(uint32_t) << hw.lut_bits)) *where = 1;
    else if (std::memcmp(at(tbw.longc), longc.data(), 2 * sizeof(uint32_t) * hw.n_long)) *where = 2;
    else if (std::memcmp(at(tbw.sub), sub.data(), (sizeof(uint16_t) * hw.n_sub) << hw.sub_bits)) *where = 3;
    else if (std::memcmp(at(tbw.sym_len), cb->length, Layout::SYM_LEN_BYTES)) *where = 4;
    else if (std::memcmp(at(tb.steps), steps.data(), sizeof(uint32_t) * ((1u << sbits) + (nss << ssb)))) *where = 5;
    else if (std::memcmp(at(tbw.steps), wsteps.data(), sizeof(uint32_t) * ((1u << wbits) + (nws << wsb)))) *where = 6;
    return *where ? fail(ctx, ET_ERR_FORMAT, "device-built decode tables differ from the host builders'") : ET_OK;
}

extern "C" int et_selftest_treewalk_table(et_ctx *ctx, const et_codebook *cb, uint32_t *first_diff) {
    if (!ctx || !cb || !first_diff) return ET_ERR_ARG;
    *first_diff = 0;
    DeviceGuard guard(ctx->device);
    ctx->range.valid = ctx->range.maps_valid = false;  // shares the tables (ctx->tw_table, ctx->chain_table)
    et::TwUpload *up = ctx->h_tw_tree[0];
    et::TwTree *tree = &up->tree;
    ET_HIP(hipStreamSynchronize(ctx->stream));
    if (et::tw_build_tree(cb, tree) != ET_OK) return fail(ctx, ET_ERR_UNSUPPORTED, "not a full code tree: the tree walk does not apply");
    et::tw_chain_plan(tree, &up->plan);
    const uint32_t entries = et::tw_table_entries(tree->n_int), n_chain = up->plan.n_entries;
    ET_TRY(ensure(ctx, ctx->tw_table, static_cast<size_t>(et::tw_table_entries(et::TW_MAX_NODES)) * sizeof(uint16_t) + 64));
    ET_TRY(ensure(ctx, ctx->tw_tree, sizeof(et::TwUpload)));
    ET_TRY(ensure(ctx, ctx->chain_table, static_cast<size_t>(et::CH_MAX_ENTRIES) * sizeof(uint64_t)));
    ET_HIP(hipMemcpyAsync(ctx->tw_tree.p, up, et::tw_upload_bytes(up), hipMemcpyHostToDevice, ctx->stream));
    et::launch_tw_build(ctx->stream, static_cast<const et::TwUpload *>(ctx->tw_tree.p), static_cast<uint32_t>(et::tw_upload_bytes(up)), tree->n_int, static_cast<uint16_t *>(ctx->tw_table.p), n_chain,
                        static_cast<uint64_t *>(ctx->chain_table.p));
    ET_HIP(hipGetLastError());
    std::vector<uint16_t> dev(entries), host(entries);
    std::vector<uint64_t> dev_chain(n_chain), host_chain(n_chain);
    ET_HIP(hipMemcpyAsync(dev.data(), ctx->tw_table.p, entries * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
    ET_HIP(hipMemcpyAsync(dev_chain.data(), ctx->chain_table.p, n_chain * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    ET_HIP(hipStreamSynchronize(ctx->stream));
    et::tw_fill_table(tree, host.data());
    et::tw_chain_fill(tree, &up->plan, host_chain.data());
    for (uint32_t i = 0; i < entries; ++i)
        if (dev[i] != host[i]) {
            *first_diff = i + 1;
            return fail(ctx, ET_ERR_FORMAT, "device-built tree-walk table differs from the host fill");
        }
    for (uint32_t i = 0; i < n_chain; ++i)
        if (dev_chain[i] != host_chain[i]) {
            *first_diff = entries + i + 1;
            return fail(ctx, ET_ERR_FORMAT, "device-built chained write tables differ from the host fill");
        }
    return ET_OK;
}

extern "C" int et_treewalk_table(const et_codebook *cb, uint16_t *table, size_t cap_entries, uint32_t *n_int) {
    if (!cb || !n_int) return ET_ERR_ARG;
    static thread_local et::TwTree tree;
    const int rc = et::tw_build_tree(cb, &tree);
    if (rc != ET_OK) return rc;
    *n_int = tree.n_int;
    if (table) {
        if (cap_entries < et::tw_table_entries(tree.n_int)) return ET_ERR_CAP;
        et::tw_fill_table(&tree, table);
    }
    return ET_OK;
}

extern "C" int et_chain_tables(const et_codebook *cb, uint64_t *table, size_t cap_entries, uint32_t *n_entries, uint32_t *table_first, uint8_t *table_bits,
                               size_t cap_tables, uint32_t *n_tables) {
    if (!cb || !n_entries || !n_tables) return ET_ERR_ARG;
    static thread_local et::TwUpload up;
    const int rc = et::tw_build_tree(cb, &up.tree);
    if (rc != ET_OK) return rc;
    et::tw_chain_plan(&up.tree, &up.plan);
    *n_entries = up.plan.n_entries;
    *n_tables = up.plan.n_tables;
    if (table) {
        if (cap_entries < up.plan.n_entries) return ET_ERR_CAP;
        et::tw_chain_fill(&up.tree, &up.plan, table);
    }
    if (table_first && table_bits) {
        if (cap_tables < up.plan.n_tables) return ET_ERR_CAP;
        for (uint32_t t = 0; t < up.plan.n_tables; ++t) {
            table_first[t] = up.plan.tab[t].first;
            table_bits[t] = up.plan.tab[t].bits;
        }
    }
    return ET_OK;
}

extern "C" int et_row_code(const et_codebook *cb, uint32_t *t) {
    if (!cb || !t) return ET_ERR_ARG;
    et::RowCode rc{};
    if (!et::row_code_of(cb, &rc)) return ET_ERR_UNSUPPORTED;
    *t = rc.t;
    return ET_OK;
}

namespace {

bool is_sweep(Family f) { return f == Family::TREE_WALK || f == Family::WINDOWS; }

struct DecodePlan {
    Family first;          // what starts the decode
    Family fallback;       // where a first sweep whose blocks give up goes: ROWS or EXIT_MAPS
    bool full_tree;        // the code as a tree with a leaf for every codeword and none more (an encoder's)
    et::RowCode row_code;  // for ROWS
    bool row_write;        // ROWS written by rows (else over the chained tables)
    bool strips;           // the chained-table write may take its strips instantiation
};

// Which way a one-GPU decode of a whole stream goes for this code table and its tree (nullptr: none), before it has seen the stream.
DecodePlan plan_decode(const et_codebook *cb, const et::TwTree *tree, const DecodeSwitches &sw) {
    DecodePlan p{};
    p.full_tree = tree && tree->n_int + 1 == cb->n_coded;
    // Fixed-length codes (2^L codewords of L bits, so L <= 8: two, four, 16, 64 symbols of about equal weight): where the codewords
    // begin is arithmetic, and so is where symbol i lies -- the write alone (k_fixed_write), no synchronisation, no scan, no tables.
    const bool fixed = p.full_tree && !sw.no_fixed_sync && cb->n_coded >= 2 && cb->min_length == cb->max_length;
    // Uniform-like bytes (complete codes of 7 and 8 bits, BASELINE's worst case): one pass by rows and columns (et_rowsync.h)
    // instead of the exit maps for every start offset.
    const bool rows = tree && !fixed && !sw.no_row_sync && et::row_code_of(cb, &p.row_code);
    // A (nearly) fixed-length code has little to re-synchronise on: unless its mix of L- and (L + 1)-bit codewords says otherwise
    // (et::quick_to_synchronise), do not even try.
    const bool near_fixed = et::nearly_fixed_length(cb) && !sw.quick_sync_always && (sw.no_quick_sync || !et::quick_to_synchronise(cb));
    p.fallback = rows ? Family::ROWS : Family::EXIT_MAPS;
    if (fixed) p.first = sw.no_fixed_write ? Family::FIXED_SYNC : Family::FIXED_WRITE;
    else if (near_fixed) p.first = p.fallback;
    else p.first = tree ? Family::TREE_WALK : Family::WINDOWS;
    p.row_write = !sw.no_row_write;
    p.strips = !sw.no_strips;
    return p;
}

// Which way the range calls go (a stream split over GPUs): et_decode_range_sync by tree walk if the code is a tree (nullptr: it is
// not), else by window sweeps; et_decode_range_maps + _resolve by rows for a row code, else by exit maps.  Which of the two pairs
// a rank calls is the group sequence's choice (et_shard_seq.cpp cold_plan: the maps for every et::nearly_fixed_length code).
struct RangePlan {
    Family sync, maps;
    et::RowCode row_code;  // for ROWS
};

RangePlan plan_range(const et_codebook *cb, const et::TwTree *tree, const DecodeSwitches &sw) {
    RangePlan p{};
    p.sync = tree ? Family::TREE_WALK : Family::WINDOWS;
    p.maps = !sw.no_row_sync && et::row_code_of(cb, &p.row_code) ? Family::ROWS : Family::EXIT_MAPS;
    return p;
}

// The workspaces every synchronisation writes: each lane's state, each block's exit and count, the scan's offsets and group
// sums, the flags; the sweeps' worklist.
int ensure_dec_ws(et_ctx *ctx, uint64_t n_subs, uint32_t n_blocks) {
    ET_TRY(ensure(ctx, ctx->sub_state, n_subs * sizeof(uint32_t)));
    ET_TRY(ensure(ctx, ctx->blk_exit, static_cast<size_t>(n_blocks) * sizeof(uint32_t)));
    ET_TRY(ensure(ctx, ctx->blk_count, static_cast<size_t>(n_blocks) * sizeof(uint32_t)));
    ET_TRY(ensure(ctx, ctx->blk_off, (static_cast<size_t>(n_blocks) + 1) * sizeof(uint64_t)));
    ET_TRY(ensure(ctx, ctx->group_sum, (static_cast<size_t>(n_blocks) / 1024 + 2) * sizeof(uint64_t)));
    ET_TRY(ensure(ctx, ctx->flag, et::DEC_FLAG_WORDS * sizeof(uint32_t)));
    ET_TRY(ensure(ctx, ctx->worklist, (static_cast<size_t>(n_blocks) + 1) * sizeof(uint32_t)));
    return ET_OK;
}

// ... as the kernels take them
DecWs dec_ws(const et_ctx *ctx) {
    return DecWs{static_cast<uint32_t *>(ctx->sub_state.p), static_cast<uint32_t *>(ctx->blk_exit.p), static_cast<uint32_t *>(ctx->blk_count.p),
                 static_cast<uint32_t *>(ctx->flag.p), static_cast<uint32_t *>(ctx->worklist.p), static_cast<unsigned long long *>(ctx->blk_off.p),
                 static_cast<unsigned long long *>(ctx->group_sum.p)};
}

// The geometry of a span whose subsequences cover n_bits bits, and the workspaces for it.
int span_ws(et_ctx *ctx, et::DecSpan *s, uint64_t n_bits, const char *too_large) {
    s->n_subs = (n_bits + et::SUB_BITS - 1) / et::SUB_BITS;
    const uint64_t n_blocks64 = (s->n_subs + et::BLOCK - 1) / et::BLOCK;
    if (n_blocks64 > 0x7fffffffull) return fail(ctx, ET_ERR_ARG, too_large);
    s->n_blocks = static_cast<uint32_t>(n_blocks64);
    ET_TRY(ensure_dec_ws(ctx, s->n_subs, s->n_blocks));
    static_cast<DecWs &>(*s) = dec_ws(ctx);
    return ET_OK;
}

int not_converged(et_ctx *ctx) { return fail(ctx, ET_ERR_HIP, "decode synchronisation did not converge"); }

// blind: the row walk's word (FLAG_ROW_BLIND) as the host has it
int check_row_walk(et_ctx *ctx, uint32_t blind) { return blind ? fail(ctx, ET_ERR_HIP, "the row walk's chunks never saw the chunks before them") : ET_OK; }

int launched(et_ctx *ctx) {  // behind every launch of a stage
    ET_HIP(hipGetLastError());
    return ET_OK;
}

// ---- the stages, each over a Span: what et_decode_body_device and the range calls are put together from ----

// Tree-walk set-up, from the code as a tree in a pinned block: the chained tables' plan, then the tree walk's table (sweeps: if it is
// to synchronise) and the chained write tables, both filled by ONE small launch that reads tree and plan from the pinned block
// itself and on its way clears the flags (zero_flags) and, for the sweeps, blk_pub.
int tw_setup(et_ctx *ctx, Span &s, et::TwUpload *h_up, bool sweeps, bool zero_flags) {
    et::tw_chain_plan(&h_up->tree, &h_up->plan);
    ET_TRY(ensure(ctx, ctx->chain_table, static_cast<size_t>(et::CH_MAX_ENTRIES) * sizeof(uint64_t)));
    if (sweeps) {
        ET_TRY(ensure(ctx, ctx->tw_table, static_cast<size_t>(et::tw_table_entries(et::TW_MAX_NODES)) * sizeof(uint16_t) + 64));
        ET_TRY(ensure(ctx, ctx->blk_start, static_cast<size_t>(s.n_blocks) * sizeof(uint32_t)));
        ET_TRY(ensure(ctx, ctx->blk_pub, static_cast<size_t>(s.n_blocks) * sizeof(uint32_t)));
        s.tw_table = static_cast<const uint16_t *>(ctx->tw_table.p);
        s.blk_start = static_cast<uint32_t *>(ctx->blk_start.p);
        s.blk_pub = static_cast<uint32_t *>(ctx->blk_pub.p);
    }
    s.tw_n_int = h_up->tree.n_int;
    s.n_chain = h_up->plan.n_entries;
    s.chain = static_cast<const uint64_t *>(ctx->chain_table.p);
    et::launch_tw_build(ctx->stream, h_up, static_cast<uint32_t>(et::tw_upload_bytes(h_up)), s.tw_n_int, sweeps ? static_cast<uint16_t *>(ctx->tw_table.p) : nullptr, s.n_chain,
                        static_cast<uint64_t *>(ctx->chain_table.p), zero_flags ? s.flag : nullptr, s.blk_pub, s.n_blocks);
    return ET_OK;
}

// A tree-walk sweep.  The first: every block runs in, settles inside and then with the block before it (k_tw_sync's blk_pub); what
// that leaves open -- a block that did not re-synchronise within its 8 KiB -- a verification finds.  listed: a repair sweep over the
// blocks tw_list has put on the worklist.
int tw_sweep(et_ctx *ctx, const Span &s, bool listed, et::KernelEvents ev = {}) {
    et::launch_tw_sync(ctx->stream, s, s.tw_table, s.tw_n_int, s.blk_start, listed ? 0xffffffffu : et::DEC_FIRST_SWEEP_TRIPS, listed, ev, listed ? nullptr : s.blk_pub, s.tw_mode,
                       s.exit_bits);
    return launched(ctx);
}

// The blocks whose first lane did not start where the block before ends -> the worklist (FLAG_WORK_COUNT, zeroed by the caller, counts them).
void tw_list(et_ctx *ctx, const Span &s) { et::launch_tw_check(ctx->stream, s, s.blk_start, !(s.tw_mode & et::TW_START_UNKNOWN)); }

// A window sweep, number iter of its stream or range.  listed: the first sweeps fill the worklist, the later ones go over it.
int window_sweep(et_ctx *ctx, const Span &s, uint32_t iter, uint32_t max_trips, bool listed, const et::SideLane *side = nullptr, bool ticket_is_zero = false,
                 et::KernelEvents ev = {}) {
    et::launch_dec_sync(ctx->stream, s, s.tb, iter, max_trips, s.dec_flags, listed, side, ticket_is_zero, ev);
    return launched(ctx);
}

// Repair sweeps until one changes nothing (FLAG_CHANGED, fetched into *h_changed): tree-walk sweeps over the blocks whose start their
// predecessor's exit contradicts, or window sweeps -- listed: over the worklist their predecessors left, else over every block --
// numbered from iter.  *sweeps counts them on.
int repair_sweeps(et_ctx *ctx, const Span &s, Family family, bool listed, uint32_t iter, uint32_t *sweeps, uint32_t *h_changed) {
    for (;;) {
        ET_HIP(hipMemsetAsync(s.flag + et::FLAG_CHANGED, 0, sizeof(uint32_t), ctx->stream));
        if (listed) ET_HIP(hipMemsetAsync(s.flag + et::FLAG_WORK_COUNT, 0, sizeof(uint32_t), ctx->stream));
        if (family == Family::TREE_WALK) {
            tw_list(ctx, s);
            ET_TRY(tw_sweep(ctx, s, true));
        } else {
            ET_TRY(window_sweep(ctx, s, iter++, 0xffffffffu, listed));
        }
        ++*sweeps;
        ET_HIP(hipMemcpyAsync(h_changed, s.flag + et::FLAG_CHANGED, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        ET_HIP(hipStreamSynchronize(ctx->stream));
        if (*h_changed == 0) return ET_OK;
        if (*sweeps > s.n_blocks + 4) return not_converged(ctx);
    }
}

// The row walk (et_rowsync.h) from s.first_bit, under s.row_mode.  d_map: where a ROW_MAP_ONLY walk leaves its map.
int row_walk(et_ctx *ctx, const Span &s, const unsigned long long **d_map = nullptr) {
    ET_TRY(ensure(ctx, ctx->row_scratch, et::row_sync_scratch_bytes(s.n_blocks)));
    et::launch_row_sync(ctx->stream, s, s.row_code, ctx->row_scratch.p, s.row_mode, d_map);
    return launched(ctx);
}

// The exit maps (et_kernels_fallback.hip): a map of the L = max_length start offsets per lane, block and group of 256 blocks.
// const_start: the span's first bit is s.first_bit whatever the map is entered with.
uint32_t map_stride(uint32_t n_starts) { return n_starts <= 8 ? 8 : (n_starts <= 16 ? 16 : 32); }

int exit_maps(et_ctx *ctx, const Span &s, bool const_start) {
    const uint32_t n_starts = s.cb->max_length, stride = map_stride(n_starts);
    const size_t n_groups = (static_cast<size_t>(s.n_blocks) + 255) / 256;
    ET_TRY(ensure(ctx, ctx->lane_maps, s.n_subs * stride + 64));
    ET_TRY(ensure(ctx, ctx->blk_maps, static_cast<size_t>(s.n_blocks) * 32 + 64));
    ET_TRY(ensure(ctx, ctx->grp_maps, n_groups * 32 + 64));
    ET_TRY(ensure(ctx, ctx->blk_in, static_cast<size_t>(s.n_blocks) + 64));
    ET_TRY(ensure(ctx, ctx->grp_in, n_groups + 64));
    et::launch_dec_maps(ctx->stream, s, const_start, s.tb, n_starts, stride, static_cast<uint8_t *>(ctx->lane_maps.p), static_cast<uint8_t *>(ctx->blk_maps.p),
                        static_cast<uint8_t *>(ctx->grp_maps.p));
    return launched(ctx);
}

// ... and every lane's start, exit and count from them, the span entered at s.first_bit.
int exit_resolve(et_ctx *ctx, const Span &s, bool const_start) {
    et::launch_dec_resolve(ctx->stream, s, const_start, s.tb, map_stride(s.cb->max_length), static_cast<const uint8_t *>(ctx->lane_maps.p), static_cast<const uint8_t *>(ctx->blk_maps.p),
                           static_cast<const uint8_t *>(ctx->grp_maps.p), static_cast<uint8_t *>(ctx->blk_in.p), static_cast<uint8_t *>(ctx->grp_in.p));
    return launched(ctx);
}

// D3: at most clamp symbols to out, the way the family that synchronised the span left them.  What only the whole-stream decode has:
struct WriteExtras {
    bool by_rows = true;                   // ROWS by rows (else over the chained tables: ET_NO_ROW_WRITE)
    et::DecFlag ticket = et::FLAG_SYNC_TICKET;  // the flag word the window tables' write counts on
    const et::SideLane *side = nullptr;    // beside which its first/last blocks run
    bool ticket_is_zero = false;
    bool speculative = false;              // the kernel itself looks at the sweeps' flags and does nothing if the state is not final
    et::KernelEvents ev = {};
    bool strips = false;                   // the chained tables' strips instantiation
};

int write_span(et_ctx *ctx, const Span &s, Family family, uint64_t clamp, uint8_t *out, const WriteExtras &x = {}) {
    switch (family == Family::ROWS && !x.by_rows ? Family::EXIT_MAPS : family) {
    case Family::ROWS:  // by rows (et_rowsync.h): no table chain, no bank conflicts between the lanes' regions
        et::launch_row_write(ctx->stream, s, s.row_code, s.cb, clamp, out, x.ev);
        break;
    case Family::FIXED_WRITE:  // symbol i is the L bits at first_bit + i L (et_rowsync.h): no walk, no state
        et::launch_fixed_write(ctx->stream, s, s.cb, clamp, out, x.ev);
        break;
    default:  // over the chained tables (s.chain) or the window tables'
        et::launch_dec_write(ctx->stream, s, s.tb_write, clamp, out, x.ticket, x.side, x.ticket_is_zero, x.speculative, x.ev, s.chain, s.n_chain, s.cb->max_length, x.strips);
    }
    return launched(ctx);
}

// ---- one whole-stream decode (et_decode_body_device), as its steps share it ----
struct BodyDecode : Span {
    et_ctx *ctx;
    uint8_t *out;  // cap bytes
    size_t cap;
    uint64_t n_symbols;
    uint32_t *h_flags;  // the host copy of the flag words (et::DecFlag)
    float host_ms;
    et::TwUpload *h_up;  // the code as a tree (one of the pinned blocks; nullptr: none)
    DecodePlan plan;
    Family family;  // what runs now: plan.first, then plan.fallback if a first sweep gives up
    uint32_t iters;
    bool flags_zeroed, more_sweeps, wrote, write_ticket_zero;
    bool strips;  // the write whose output is kept took the strips instantiation
};

// The tree (if the code is one: an encoder's always is) and the plan; the window kernels' tables up front for the families that start
// on them (their building kernel clears the flags on its way).  The host time a decode reports is this.  Then tw_setup.
int body_setup(BodyDecode &d) {
    et_ctx *ctx = d.ctx;
    const double t0 = now_ms();
    d.h_up = ctx->h_tw_tree[ctx->tw_turn ^= 1];  // two pinned blocks in turn, as prepare_decode_tables' (this call waits for its flags before it returns)
    if (et::tw_build_tree(d.cb, &d.h_up->tree, true) != ET_OK) d.h_up = nullptr;  // (bit patterns without a symbol become leaves that decode as byte 0)
    d.plan = plan_decode(d.cb, d.h_up ? &d.h_up->tree : nullptr, decode_switches());
    d.row_code = d.plan.row_code;
    d.family = d.plan.first;
    if (d.family == Family::WINDOWS || d.family == Family::EXIT_MAPS) ET_TRY(prepare_decode_tables(ctx, d.cb, &d.tb, &d.tb_write, d.flag, &d.flags_zeroed));
    d.host_ms = static_cast<float>(now_ms() - t0);
    if (!d.h_up || d.family == Family::FIXED_WRITE) return ET_OK;
    const bool zero_here = !d.flags_zeroed && d.family != Family::EXIT_MAPS;
    ET_TRY(tw_setup(ctx, d, d.h_up, d.family == Family::TREE_WALK, zero_here));
    d.flags_zeroed = d.flags_zeroed || zero_here;
    return ET_OK;
}

// D2, the scan of the blocks' symbol counts; its last thread stores the flags and the total into the pinned h_flags and then the
// launch's epoch into FLAG_REPORT_EPOCH, which the host waits for (wait_report).  first: behind the first sweep, whose block starts (tree walk)
// or lane states (windows) it verifies.
int wait_report(BodyDecode &d) { return wait_for_word<uint32_t>(d.ctx, d.h_flags + et::FLAG_REPORT_EPOCH, d.ctx->report_epoch, 200.0, "the decode's report never reached the host"); }

int body_scan(BodyDecode &d, bool first) {
    et_ctx *ctx = d.ctx;
    const bool tw = first && d.tw_table;
    const et::ScanVerify verify{tw ? d.blk_start : (first ? d.sub_state : nullptr), tw, tw ? 0u : d.first_bit};
    const et::ScanReport report{d.h_flags, ++ctx->report_epoch};
    et::launch_dec_scan(ctx->stream, d, scan_epoch(ctx), &verify, &report);
    return launched(ctx);
}

// D3 with what belongs to this caller: the events, the side lane, FLAG_WRITE_TICKET, the strips.  speculative: see WriteExtras.
int write_symbols(BodyDecode &d, uint64_t clamp, bool speculative) {
    WriteExtras x{d.plan.row_write, et::FLAG_WRITE_TICKET, &d.ctx->side, d.write_ticket_zero, speculative, timed_body(d.ctx, EV_DEC + 2, EV_DEC + 3), false};
    const bool tables = d.family != Family::FIXED_WRITE && !(d.family == Family::ROWS && d.plan.row_write);
    // More than 128 symbols per 256-bit subsequence: a quarter's output is three or more
    // windows of the write's 4 KiB stage, i.e. it would be walked three or more times -- the instantiation that walks it once, into strips
    // (measured: +45 % at 140 symbols per subsequence, +75 % at 200; at 90-110, two windows, the strips' scattered stores cost what they save).
    // The symbols are the ones this write stores: the header's count when it is speculative, the counted ones behind the report -- a body cut
    // short of its header's count holds no more per subsequence than the whole stream did, and takes the whole stream's instantiation.
    // (A preference, not a repair: by the header's count such a body took the strips, and its bytes and extent were right all the same.)
    d.strips = x.strips = tables && d.plan.strips && d.chain && clamp / 128 > d.n_subs;
    ET_TRY(write_span(d.ctx, d, d.family, clamp, d.out, x));
    if (tables) d.write_ticket_zero = false;
    return ET_OK;
}

// D1 and D2 for the sweep families.  Sweep 0 runs in and repairs inside each block; (the windows') sweep 1 repairs across blocks
// (on text ~0.4 % of the block boundaries); the scan that follows also verifies that every block starts where its predecessor ends
// (the "sweep that changes nothing").  Everything up to the write kernel is enqueued without waiting, the speculative write
// included; the flags and the total reach the host with ONE wait, and only if they say so -- blocks that gave up: the plan's
// fallback; verification failed: more sweeps -- is the tail redone.  (The flag words: et_kernels.h DecFlag.)
int body_first_sweep(BodyDecode &d) {
    if (!is_sweep(d.family)) return ET_OK;
    et_ctx *ctx = d.ctx;
    const et::SideLane *side = &ctx->side;  // the first/last blocks' small launches run beside the large kernels (2.3 % at 1 GiB)
    if (!d.flags_zeroed) ET_HIP(hipMemsetAsync(d.flag, 0, et::DEC_FLAG_WORDS * sizeof(uint32_t), ctx->stream));
    d.write_ticket_zero = true;
    if (d.tw_table) {
        ET_TRY(tw_sweep(ctx, d, false, timed(ctx, EV_DEC + 0, EV_DEC + 5)));
    } else {
        ET_TRY(window_sweep(ctx, d, 0, et::DEC_FIRST_SWEEP_TRIPS, false, side, true, timed(ctx, EV_DEC + 0, EV_DEC + 5)));
        ET_TRY(window_sweep(ctx, d, 1, et::DEC_REPAIR_SWEEP_TRIPS, true, side));
    }
    d.iters = d.tw_table ? 2 : 3;  // run-in sweep, (repair sweep,) verification
    ET_TRY(body_scan(d, true));
    if (d.cap >= d.n_symbols) {
        ET_TRY(write_symbols(d, d.n_symbols, true));
        d.wrote = true;
    }
    ET_TRY(wait_report(d));  // not the stream: the write kernel keeps running while the caller moves on
    const uint32_t n_gave_up = d.h_flags[et::FLAG_GAVE_UP], verify_failed = d.h_flags[et::FLAG_VERIFY_FAILED];
    const bool gave_up = static_cast<uint64_t>(n_gave_up) * 64 > d.n_blocks;
    if (gave_up) d.family = d.plan.fallback;
    d.more_sweeps = !gave_up && verify_failed != 0;
    if (!et::dec_state_final(n_gave_up, verify_failed, d.n_blocks)) d.wrote = d.strips = false;  // the speculative launch declined by the same rule
    return ET_OK;
}

// The families that synchronise whatever the stream: the row walk, k_fixed_sync (k_fixed_write needs nothing), the exit maps.
// Where no first sweep carried the decode's first events, two plain markers stand in front of them.
int body_exhaustive(BodyDecode &d) {
    if (is_sweep(d.family)) return ET_OK;
    et_ctx *ctx = d.ctx;
    if (d.iters == 0) {
        record(ctx, EV_DEC + 0);
        record(ctx, EV_DEC + 5);
    }
    if (d.family == Family::ROWS) {
        ET_TRY(row_walk(ctx, d));
        d.iters += 1;
    } else if (d.family == Family::FIXED_SYNC) {
        et::launch_fixed_sync(ctx->stream, d, d.cb->max_length);
        d.iters += 1;
    } else if (d.family == Family::EXIT_MAPS) {
        if (d.plan.first == Family::TREE_WALK) ET_TRY(prepare_decode_tables(ctx, d.cb, &d.tb, &d.tb_write));  // (the others built them up front)
        // The exhaustive kernels count with the older lookup tables, for which a bit pattern without a symbol is passed
        // over bit by bit; in the chained tables it is a leaf that decodes as byte 0.  The two agree on every stream of a
        // FULL tree (an encoder's) -- for a completed one the write has to count like the synchronisation did.
        if (!d.plan.full_tree) d.chain = nullptr;
        ET_TRY(exit_maps(ctx, d, true));
        ET_TRY(exit_resolve(ctx, d, true));
        d.iters += 5;
    }
    return launched(ctx);
}

// The scan behind the exhaustive families and the repair sweeps (k_fixed_write has nothing to scan).
int body_final_scan(BodyDecode &d) {
    if ((is_sweep(d.family) && !d.more_sweeps) || d.family == Family::FIXED_WRITE) return ET_OK;
    ET_TRY(body_scan(d, false));
    ET_TRY(wait_report(d));
    return d.family == Family::ROWS ? check_row_walk(d.ctx, d.h_flags[et::FLAG_ROW_BLIND]) : ET_OK;
}

// What et_last_timings reports; the events' arithmetic waits for the first call that asks.  The bits of et_timings.reserved, as
// include/entreepy_hip.h documents them (and entreepy_amd/codec.py reads them):
enum : uint32_t { TM_EXHAUSTIVE = 1, TM_TREE_WALK = 2, TM_CHAINED_WRITE = 4, TM_ROWS = 8, TM_FIXED = 16, TM_STRIPS = 32 };

void body_timings(const BodyDecode &d) {
    et_ctx *ctx = d.ctx;
    if (!ctx->timing && !ctx->timing_body) return;
    const bool fixed = d.plan.first == Family::FIXED_SYNC || d.plan.first == Family::FIXED_WRITE;
    ctx->tm_dec = et_timings{};
    ctx->tm_dec.host_ms = d.host_ms;
    ctx->tm_dec.sync_iters = d.iters;
    ctx->tm_dec.reserved = (is_sweep(d.family) ? 0u : TM_EXHAUSTIVE) | (d.tw_table ? TM_TREE_WALK : 0u) | (d.chain ? TM_CHAINED_WRITE : 0u) |
                           (d.family == Family::ROWS ? TM_ROWS : 0u) | (fixed ? TM_FIXED : 0u) | (d.strips ? TM_STRIPS : 0u);
    ctx->pend_dec = true;
    ctx->pend_dec_first = is_sweep(d.plan.first);
    ctx->last_kind = 1;
}

}  // namespace

// Which way a one-GPU decode of a whole stream goes for this code table (the ET_NO_* switches aside).
extern "C" int et_decode_path(const et_codebook *cb, uint32_t *path) {
    if (!cb || !path) return ET_ERR_ARG;
    if (cb->n_coded == 0) return ET_ERR_ARG;
    if (cb->max_length > 32) return ET_ERR_UNSUPPORTED;
    et::TwTree tree;
    const bool have_tree = et::tw_build_tree(cb, &tree, true) == ET_OK;
    switch (plan_decode(cb, have_tree ? &tree : nullptr, DecodeSwitches{}).first) {
    case Family::TREE_WALK: *path = ET_PATH_TREE_WALK; break;
    case Family::WINDOWS: *path = ET_PATH_WINDOWS; break;
    case Family::ROWS: *path = ET_PATH_ROWS; break;
    case Family::FIXED_SYNC: case Family::FIXED_WRITE: *path = ET_PATH_FIXED; break;
    case Family::EXIT_MAPS: *path = ET_PATH_EXIT_MAPS; break;
    }
    return ET_OK;
}

extern "C" int et_decode_body_device(et_ctx *ctx, const et_codebook *cb, const void *d_body, size_t body_bytes, uint32_t start_bit,
                                     uint64_t n_symbols, void *d_out, size_t cap, size_t *out_len) {
    if (!ctx || !cb || !out_len) return ET_ERR_ARG;
    *out_len = 0;
    if (cb->max_length > 32) return fail(ctx, ET_ERR_UNSUPPORTED, "code length > 32");
    if (start_bit >= 8) return fail(ctx, ET_ERR_ARG, "start_bit must be < 8");
    if (n_symbols == 0 || body_bytes == 0 || cb->n_coded == 0 || static_cast<uint64_t>(body_bytes) * 8 <= start_bit) return ET_OK;
    if (!d_body || !d_out) return ET_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(d_out) & 15) return fail(ctx, ET_ERR_ARG, "d_out must be 16-byte aligned");
    DeviceGuard guard(ctx->device);

    BodyDecode d{};
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_body);
    d.words = reinterpret_cast<const uint32_t *>(a & ~static_cast<uintptr_t>(3));
    d.first_bit = static_cast<uint32_t>(a & 3) * 8 + start_bit;
    d.n_bytes = (a & 3) + body_bytes;  // stream bytes measured from the aligned base
    ET_TRY(span_ws(ctx, &d, d.n_bytes * 8, "body too large"));
    d.dec_flags = et::DEC_HAVE_START;
    ctx->range.valid = ctx->range.maps_valid = false;  // shares the workspaces
    d.ctx = ctx;
    d.cb = cb;
    d.out = static_cast<uint8_t *>(d_out);
    d.cap = cap;
    d.n_symbols = n_symbols;
    d.h_flags = reinterpret_cast<uint32_t *>(ctx->h_scalar + HS_BODY_FLAGS);

    ET_TRY(body_setup(d));
    ET_TRY(body_first_sweep(d));
    ET_TRY(body_exhaustive(d));
    if (d.more_sweeps) ET_TRY(repair_sweeps(ctx, d, d.family, true, d.iters, &d.iters, d.h_flags));
    ET_TRY(body_final_scan(d));
    const uint64_t decodable = d.family == Family::FIXED_WRITE
                                   ? (d.n_bytes * 8 >= d.first_bit ? (d.n_bytes * 8 - d.first_bit) / cb->max_length : 0)  // the whole codewords from first_bit on
                                   : static_cast<uint64_t>(d.h_flags[et::FLAG_TOTAL_LO]) | (static_cast<uint64_t>(d.h_flags[et::FLAG_TOTAL_HI]) << 32);
    const uint64_t n_out = decodable < n_symbols ? decodable : n_symbols;
    if (n_out > cap) return fail(ctx, ET_ERR_CAP, "output buffer too small");
    if (n_out && !d.wrote) ET_TRY(write_symbols(d, n_out, false));
    *out_len = static_cast<size_t>(n_out);
    body_timings(d);
    return ET_OK;
}

namespace {

// The argument checks et_decode_range_sync and _maps both make, and the range as a Span: geometry, first bit, workspaces.
int range_span(et_ctx *ctx, const et_codebook *cb, const void *d_range, size_t range_bytes, size_t tail_bytes, int32_t in_start_bit, bool unknown_start_ok, Span *s) {
    if (reinterpret_cast<uintptr_t>(d_range) & 3) return fail(ctx, ET_ERR_ARG, "d_range must be 4-byte aligned");
    if (tail_bytes && (range_bytes % (et::DEC_BLOCK_WORDS * 4) || tail_bytes < 16)) return fail(ctx, ET_ERR_ARG, "an inner range is a multiple of 8192 bytes with >= 16 bytes after it");
    if (in_start_bit >= 32) return fail(ctx, ET_ERR_ARG, "in_start_bit must be < 32");
    if (in_start_bit < 0 && !unknown_start_ok) return fail(ctx, ET_ERR_ARG, "an unknown start needs the 16 bytes in front of the range");
    if (cb->max_length > 32) return fail(ctx, ET_ERR_UNSUPPORTED, "code length > 32");
    if (cb->n_coded == 0) return fail(ctx, ET_ERR_ARG, "empty code table");
    *s = Span{};
    s->words = static_cast<const uint32_t *>(d_range);
    s->n_bytes = static_cast<uint64_t>(range_bytes) + tail_bytes;
    s->first_bit = in_start_bit >= 0 ? static_cast<uint32_t>(in_start_bit) : 0u;
    return span_ws(ctx, s, static_cast<uint64_t>(range_bytes) * 8, "range too large");
}

// The range the ctx holds becomes s, to be synchronised by family; nothing of it is valid yet.
Span &begin_range(et_ctx *ctx, const Span &s, const et_codebook *cb, Family family) {
    auto &rs = ctx->range;
    rs.valid = rs.maps_valid = false;
    rs.family = family;
    rs.cb = *cb;
    rs.s = s;
    rs.s.cb = &rs.cb;
    return rs.s;
}

// A second et_decode_range_sync by window sweeps for the range the ctx holds, now with the predecessor's exit: its states and
// tables stand, only the repair sweeps run.
bool same_range_again(const et_ctx *ctx, const Span &s, bool known) {
    const auto &rs = ctx->range;
    return rs.valid && rs.family == Family::WINDOWS && rs.s.words == s.words && rs.s.n_subs == s.n_subs && known;
}

// The range calls' words in pinned host memory (RangeFlag).
uint32_t *range_flags(et_ctx *ctx) { return reinterpret_cast<uint32_t *>(ctx->h_scalar + HS_RANGE_FLAGS); }

// The tail of every range synchronisation: the scan of its blocks' counts, then its start, exit (the tree walk's exit bit, else the last
// block's exit) and total to the host; the range is ready for et_decode_range_write.
int finish_range(et_ctx *ctx, uint32_t sweeps, et_range_info *info) {
    auto &rs = ctx->range;
    const Span &s = rs.s;
    const uint32_t *row_word = rs.family == Family::ROWS ? s.flag + et::FLAG_ROW_BLIND : nullptr;
    uint32_t *h_flags = range_flags(ctx);
    et::launch_dec_scan(ctx->stream, s, scan_epoch(ctx));
    ET_HIP(hipGetLastError());
    ET_HIP(hipMemcpyAsync(ctx->h_scalar + HS_TOTAL, s.blk_off + s.n_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    ET_HIP(hipMemcpyAsync(h_flags + RF_START, s.sub_state, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    ET_HIP(hipMemcpyAsync(h_flags + RF_EXIT, s.exit_bits ? s.exit_bits : s.blk_exit + (s.n_blocks - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (row_word) ET_HIP(hipMemcpyAsync(h_flags + RF_ROW_BLIND, row_word, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    ET_HIP(hipStreamSynchronize(ctx->stream));
    if (row_word) ET_TRY(check_row_walk(ctx, h_flags[RF_ROW_BLIND]));
    rs.total = ctx->h_scalar[HS_TOTAL];
    rs.valid = true;
    info->start_bit = h_flags[RF_START] & 0xffu;
    info->exit_bit = h_flags[RF_EXIT];
    info->n_symbols = rs.total;
    info->sweeps = sweeps;
    switch (rs.family) {  // as include/entreepy_hip.h documents et_range_info.reserved
    case Family::TREE_WALK: info->reserved = 2; break;
    case Family::ROWS: info->reserved = 3; break;
    case Family::EXIT_MAPS: info->reserved = 1; break;
    default: info->reserved = 0;  // WINDOWS (the fixed-length families never synchronise a range)
    }
    return ET_OK;
}

}  // namespace

extern "C" int et_decode_range_sync(et_ctx *ctx, const et_codebook *cb, const void *d_range, size_t range_bytes, size_t tail_bytes,
                                    int has_front, int32_t in_start_bit, et_range_info *info) {
    if (!ctx || !cb || !d_range || !info || range_bytes == 0) return ET_ERR_ARG;
    DeviceGuard guard(ctx->device);
    Span g;
    ET_TRY(range_span(ctx, cb, d_range, range_bytes, tail_bytes, in_start_bit, has_front != 0, &g));
    const bool known = in_start_bit >= 0;
    uint32_t *h_flags = range_flags(ctx);
    et::TwUpload *h_up = ctx->h_tw_tree[ctx->tw_turn ^= 1];
    const bool have_tree = et::tw_build_tree(cb, &h_up->tree, true) == ET_OK;
    uint32_t sweeps = 0;
    if (plan_range(cb, have_tree ? &h_up->tree : nullptr, decode_switches()).sync == Family::TREE_WALK) {
        // A full code tree (an encoder's always is): the sweeps of et_decode_body_device -- k_tw_sync with its seam step,
        // told that the words in front of the range are stream bytes and that the first lane runs in like any other unless
        // the caller knows its first bit -- then list + repair launches until no block disagrees with the one before it.
        // A second call for the same range with the predecessor's exit simply sweeps again from that bit.
        Span &s = begin_range(ctx, g, cb, Family::TREE_WALK);
        s.tw_mode = (has_front ? et::TW_FRONT_OK : 0u) | (known ? 0u : et::TW_START_UNKNOWN);
        s.exit_bits = s.flag + et::FLAG_RANGE_EXIT;
        ET_TRY(tw_setup(ctx, s, h_up, true, true));
        ET_TRY(tw_sweep(ctx, s, false));
        ++sweeps;
        // Not repair_sweeps: the whole-stream decode comes here knowing from its scan that a block disagrees and asks each sweep
        // whether it changed anything; a range has no scan yet and asks the list itself, before the first repair sweep.
        for (;;) {  // (normally one look: nothing on the list)
            ET_HIP(hipMemsetAsync(s.flag + et::FLAG_WORK_COUNT, 0, sizeof(uint32_t), ctx->stream));
            tw_list(ctx, s);
            ET_HIP(hipMemcpyAsync(h_flags + RF_START, s.flag + et::FLAG_WORK_COUNT, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            ET_HIP(hipStreamSynchronize(ctx->stream));
            if (h_flags[RF_START] == 0) break;
            if (sweeps > s.n_blocks + 4) return not_converged(ctx);
            ET_TRY(tw_sweep(ctx, s, true));
            ++sweeps;
        }
        return finish_range(ctx, sweeps, info);
    }
    const uint32_t dec_flags = (known ? et::DEC_HAVE_START : 0u) | (has_front ? et::DEC_FRONT_OK : 0u);
    if (same_range_again(ctx, g, known)) {
        static_cast<DecWs &>(ctx->range.s) = g;
        ctx->range.s.first_bit = g.first_bit;
        ctx->range.s.dec_flags = dec_flags;
    } else {
        Span &s = begin_range(ctx, g, cb, Family::WINDOWS);
        s.dec_flags = dec_flags;
        ET_TRY(prepare_decode_tables(ctx, cb, &s.tb, &s.tb_write));
        // Sweep 0 (run-in, local repair with a trip cap); codes that do not synchronise take
        // many capped sweeps here -- the exhaustive path is single-GPU only for now.
        ET_HIP(hipMemsetAsync(s.flag, 0, et::DEC_SWEEP_FLAGS * sizeof(uint32_t), ctx->stream));
        ET_TRY(window_sweep(ctx, s, 0, et::DEC_FIRST_SWEEP_TRIPS, false));
        ++sweeps;
    }
    ET_TRY(repair_sweeps(ctx, ctx->range.s, Family::WINDOWS, false, 1 + sweeps, &sweeps, h_flags + RF_START));
    return finish_range(ctx, sweeps, info);
}

extern "C" int et_decode_range_maps(et_ctx *ctx, const et_codebook *cb, const void *d_range, size_t range_bytes, size_t tail_bytes,
                                    int32_t in_start_bit, uint8_t map[32], uint32_t *n_starts_out) {
    if (!ctx || !cb || !d_range || !map || !n_starts_out || range_bytes == 0) return ET_ERR_ARG;
    DeviceGuard guard(ctx->device);
    Span g;
    ET_TRY(range_span(ctx, cb, d_range, range_bytes, tail_bytes, in_start_bit, true, &g));
    const bool known = in_start_bit >= 0;
    const RangePlan plan = plan_range(cb, nullptr, decode_switches());
    Span &s = begin_range(ctx, g, cb, plan.maps);
    ctx->range.maps_const = known;
    if (plan.maps == Family::ROWS) {
        // Uniform-like bytes (a complete code of 7- and 8-bit codewords): the range's map by rows and columns -- every chunk publishes
        // its map, the last one composes them (k_row_sync, ROW_MAP_ONLY); the resolve is a second run with the start known.
        s.row_code = plan.row_code;
        s.row_mode = et::ROW_MAP_ONLY | (known ? 0u : et::ROW_START_UNKNOWN);
        ET_HIP(hipMemsetAsync(s.flag, 0, et::DEC_FLAG_WORDS * sizeof(uint32_t), ctx->stream));
        const unsigned long long *d_map = nullptr;
        ET_TRY(row_walk(ctx, s, &d_map));
        ET_HIP(hipMemcpyAsync(ctx->h_scalar + HS_TOTAL, d_map, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        ET_HIP(hipMemcpyAsync(range_flags(ctx) + RF_ROW_BLIND, s.flag + et::FLAG_ROW_BLIND, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        ET_HIP(hipStreamSynchronize(ctx->stream));
        ET_TRY(check_row_walk(ctx, range_flags(ctx)[RF_ROW_BLIND]));
        const uint64_t m = ctx->h_scalar[HS_TOTAL];
        for (uint32_t p = 0; p < 32; ++p) map[p] = static_cast<uint8_t>(p < 8 ? (m >> (8 * p)) & 0xffu : (known ? m & 0xffu : p));
        *n_starts_out = 8;
    } else {
        const uint32_t n_starts = cb->max_length;
        const size_t n_groups = (static_cast<size_t>(s.n_blocks) + 255) / 256;
        ET_TRY(prepare_decode_tables(ctx, cb, &s.tb, &s.tb_write));
        ET_TRY(exit_maps(ctx, s, known));
        // last level on the host: compose the group maps (32 bytes per 2 MiB of stream)
        std::vector<uint8_t> grp(n_groups * 32);
        ET_HIP(hipMemcpyAsync(grp.data(), ctx->grp_maps.p, grp.size(), hipMemcpyDeviceToHost, ctx->stream));
        ET_HIP(hipStreamSynchronize(ctx->stream));
        for (uint32_t p = 0; p < 32; ++p) {
            uint32_t sidx = p;
            if (p < n_starts || known)
                for (size_t i = 0; i < n_groups; ++i) sidx = grp[i * 32 + sidx];
            map[p] = static_cast<uint8_t>(sidx);
        }
        *n_starts_out = n_starts;
    }
    ctx->range.maps_valid = true;
    return ET_OK;
}

extern "C" int et_decode_range_resolve(et_ctx *ctx, uint32_t in_start_bit, et_range_info *info) {
    if (!ctx || !info) return ET_ERR_ARG;
    auto &rs = ctx->range;
    if (!rs.maps_valid) return fail(ctx, ET_ERR_ARG, "et_decode_range_resolve needs et_decode_range_maps first");
    if (in_start_bit >= 32) return fail(ctx, ET_ERR_ARG, "in_start_bit must be < 32");
    DeviceGuard guard(ctx->device);
    Span &s = rs.s;
    static_cast<DecWs &>(s) = dec_ws(ctx);
    s.first_bit = in_start_bit;  // (kept in the span for both families; after this call only the row walk's write looks at it)
    if (rs.family == Family::ROWS) {  // the same walk again, the start known: every lane's start, exit and count
        s.row_mode = 0;
        ET_HIP(hipMemsetAsync(s.flag, 0, et::DEC_FLAG_WORDS * sizeof(uint32_t), ctx->stream));
        ET_TRY(row_walk(ctx, s));
    } else {
        ET_TRY(exit_resolve(ctx, s, rs.maps_const));
    }
    return finish_range(ctx, 0, info);
}

extern "C" int et_decode_range_write(et_ctx *ctx, uint64_t max_symbols, void *d_out, size_t cap, size_t *out_len) {
    if (!ctx || !out_len) return ET_ERR_ARG;
    *out_len = 0;
    auto &rs = ctx->range;
    if (!rs.valid) return fail(ctx, ET_ERR_ARG, "et_decode_range_write needs et_decode_range_sync first");
    const uint64_t n_out = rs.total < max_symbols ? rs.total : max_symbols;
    if (n_out == 0) return ET_OK;
    if (!d_out || (reinterpret_cast<uintptr_t>(d_out) & 15)) return fail(ctx, ET_ERR_ARG, "d_out must be 16-byte aligned");
    if (n_out > cap) return fail(ctx, ET_ERR_CAP, "output buffer too small");
    DeviceGuard guard(ctx->device);
    static_cast<DecWs &>(rs.s) = dec_ws(ctx);
    ET_TRY(write_span(ctx, rs.s, rs.family, n_out, static_cast<uint8_t *>(d_out)));
    *out_len = static_cast<size_t>(n_out);
    return ET_OK;
}

extern "C" int et_decode_device(et_ctx *ctx, const void *d_compressed, size_t len, void *d_out, size_t cap, size_t *out_len) {
    if (!ctx || !d_compressed || !out_len) return ET_ERR_ARG;
    *out_len = 0;
    if (len < 5) return fail(ctx, ET_ERR_FORMAT, "stream shorter than its header");
    DeviceGuard guard(ctx->device);
    // The header and dictionary (<= 4627 bytes after the 4 stripped ones) are parsed on the host.
    const size_t head = len < HEADER_STAGE ? len : HEADER_STAGE;
    // (no wait before the copy: an earlier encode's upload FROM the pinned header stage is
    // ahead of this copy INTO it on the same stream)
    // A one-workgroup kernel stores the bytes into the pinned stage and then a "done" word, which the host polls (a
    // copy command and a stream wait cost ~10 us more, between the two halves of an encode + decode pipeline).
    uint8_t *hdr_data = ctx->h_header;
    volatile uint64_t *done = ctx->h_scalar + HS_HEADER_DONE;
    const uint64_t epoch = ++ctx->header_epoch;
    et::launch_header_to_host(ctx->stream, d_compressed, static_cast<uint32_t>(head), hdr_data, const_cast<unsigned long long *>(reinterpret_cast<volatile unsigned long long *>(done)), epoch);
    ET_HIP(hipGetLastError());
    ET_TRY(wait_for_word<uint64_t>(ctx, done, epoch, 100.0, "the header never reached the host"));
    et_codebook cb;
    uint64_t n_symbols = 0;
    size_t body_offset = 0;
    // Parsing only needs the dictionary (the kernel has sent as many bytes as one with that many entries can
    // have); give the parser the true length when the stream is short so that truncation is detected.
    const size_t sent = std::min<size_t>(head, et::header_bound(hdr_data[0]));
    int rc = et_parse_header(hdr_data, sent, &cb, &n_symbols, &body_offset);
    if (rc != ET_OK) return fail(ctx, rc, "et_parse_header");
    if (body_offset > len) return fail(ctx, ET_ERR_FORMAT, "dictionary runs past the end of the stream");
    return et_decode_body_device(ctx, &cb, static_cast<const uint8_t *>(d_compressed) + body_offset, len - body_offset, 0, n_symbols, d_out, cap, out_len);
}
