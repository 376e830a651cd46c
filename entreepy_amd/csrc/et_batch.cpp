// et_batch.cpp -- host side of the calls of include/entreepy_hip.h that take many small streams or records at once.  A call's
// fixed price -- its launches and its hand-over to the host -- is paid once per chunk or per call, not once per stream.
//
// ONE pinned block (ctx->h_batch) serves every call, in three regions, and each may be refilled WITHOUT ASKING.  The invariant:
// every call that uploads from a region ends with a poll for the report of a kernel that runs behind that upload on the stream
// (stream order; a switch of streams keeps it, et_ctx_set_stream), or with a terminal ET_ERR_HIP.  When that epoch word has
// arrived, the kernel is over, and so is every upload in front of it: whoever fills the region next finds it free.  On the device
// the workspaces are rewritten in stream order behind the kernels that read them.
//   batch    its chunks BEGIN with the polled kernel, whose records lie where no later upload of a chunk reads; the region is
//            kept apart because et_encode_batch_device ends with uploads and a kernel nobody polls for.  What the batch kernels are
//            not made for -- texts above et_batch_small_max(), codes beyond 32 bits on encode, dictionaries that are not a full tree
//            on decode -- runs through et_encode_device / et_decode_device for that stream alone, behind the batch launches (path = 1)
//   shared   the table goes up once per call, the job records once per chunk of SHARED_CHUNK streams; every chunk ends with its poll
//   packed   [table 2 KiB][the counters' first values][the match's pattern][the order modes' boundaries]: one upload per call of the part it needs, then the
//            launches, then one poll.  The records are u64 offset arrays ON THE DEVICE: no job records, no chunks, no host loop.  A
//            report that leaves in front of the call's last kernel carries the figures that kernel decides by (do the bodies, or the
//            rows, fit?), so the host returns ET_ERR_CAP or ET_OK from the same figures without waiting for it.
// The launches, (poll) where the host waits:
//   batch encode  per chunk: k_batch_hist (poll) -> code table + header per stream, one upload -> k_batch_encode
//   batch decode  per chunk: k_batch_heads (poll) -> et_parse_header per stream, one upload -> k_batch_decode (poll)
//   shared        per chunk: k_shared_encode / k_shared_decode (poll)
//   encode        table + counters -> k_packed_count -> k_packed_scan (poll) -> unless sizes only: k_packed_pack
//   decode        table + counters -> k_packed_decode (poll)
//   gather        table + counters -> k_gather_plan -> k_packed_scan -> k_packed_gather (poll: it alone knows the short rows); sizes only: the scan's (poll)
//   match         counters + pattern (et_encode_pattern, on the host) -> k_match_flag -> k_packed_scan (poll) -> unless count only: k_rows_emit
//   order         (the match's LESS modes) sorted codes + counters + pattern + boundaries -> k_order_flag -> k_packed_scan (poll) -> unless count only: k_rows_emit
//   search        sorted codes + counters + pattern -> k_search_flag -> k_search_long -> k_packed_scan (poll) -> unless count only: k_rows_emit
//   join          counters -> clear the table -> k_join_build -> k_join_flag (the keys' counters into the report) -> k_packed_scan (poll) -> unless count only: k_rows_emit
//   group         counters -> clear the table -> k_group_build (the store as its own key set) -> k_group_flag -> k_packed_scan (poll) -> unless count only: k_group_emit, k_group_number
//   take          counters -> k_take_plan -> k_take_scan (poll) -> unless sizes only: k_take_copy
//   slice         sorted codes + counters -> k_slice_plan -> k_slice_long -> k_take_scan (poll) -> unless sizes only: k_take_copy (reading bits)
//   field         sorted codes + counters -> k_field_plan -> k_field_long -> k_take_scan (poll) -> unless sizes only: k_take_copy (reading bits)
//   concat        sorted codes + counters + the encoded literal -> k_concat_plan -> k_concat_long -> k_take_scan (poll) -> unless sizes only: k_concat_copy
//   recode        sorted codes of table IN + counters + the output table -> k_recode_plan -> k_recode_long -> k_take_scan (poll) -> unless sizes only: k_recode_write, k_recode_write_long
//   number        sorted codes + counters -> the aggregates' first values (hipMemsetAsync, k_number_fill) -> k_number_plan -> k_number_long -> k_number_fold (poll)
#include "et_ctx.h"

#include "et_batch.h"
#include "et_join.h"

#include <algorithm>
#include <vector>

namespace {

constexpr size_t CH = et::BATCH_CHUNK;
// the pinned block
constexpr size_t PIN_WORDS = 0;                                   // u64[8]: [0] k_batch_hist, [1] k_batch_heads, [2] k_batch_decode, [3] k_shared_*, [4] k_packed_*
constexpr size_t PIN_SPANS = 64;                                  // BatchSpan[CH]
constexpr size_t PIN_JOBS = PIN_SPANS + CH * sizeof(et::BatchSpan);  // BatchEncJob / BatchDecJob [CH]
constexpr size_t PIN_TOTALS = PIN_JOBS + CH * sizeof(et::BatchDecJob);
constexpr size_t PIN_REPORT = PIN_TOTALS + CH * sizeof(uint32_t);   // histograms (1 KiB per stream) or heads (BATCH_HEAD_STRIDE)
constexpr size_t PIN_BLOB = PIN_REPORT + CH * et::BATCH_HEAD_STRIDE;
// ... and the shared-table calls' region
constexpr size_t SCH = et::SHARED_CHUNK;
constexpr size_t PIN_SH_TABLE = PIN_BLOB + CH * et::BATCH_ENC_SLOT;  // 2 KiB: {left-aligned code, length} x 256, or the sorted codes
constexpr size_t PIN_SH_JOBS = PIN_SH_TABLE + 2048;                  // SharedJob[SCH]
constexpr size_t PIN_SH_RESULTS = PIN_SH_JOBS + SCH * sizeof(et::SharedJob);  // uint2[SCH]
// ... and the packed calls': what goes up -- the table, the counters' first values, the match's encoded needle (zero-padded to a
// multiple of 4 bytes), each call one copy of the part it needs -- and the report
constexpr size_t PK_COUNTER_BYTES = et::PACKED_WORDS * 8;
constexpr size_t PIN_PK_TABLE = PIN_SH_RESULTS + SCH * 8;  // 2 KiB, as PIN_SH_TABLE
constexpr size_t PIN_PK_STATS = PIN_PK_TABLE + 2048;       // u64[PACKED_WORDS]
constexpr size_t PIN_PK_PATTERN = PIN_PK_STATS + PK_COUNTER_BYTES;  // MATCH_PATTERN_BYTES
constexpr size_t PK_STARTS_BYTES = ((et::MATCH_NEEDLE_MAX + 1) * 4 + 15) & ~static_cast<size_t>(15);  // the order modes' boundary table, behind the pattern
constexpr size_t PIN_PK_REPORT = PIN_PK_PATTERN + et::MATCH_PATTERN_BYTES + PK_STARTS_BYTES;  // u64[PACKED_WORDS]
constexpr size_t PIN_BYTES = PIN_PK_REPORT + PK_COUNTER_BYTES;
static_assert(PIN_PK_TABLE % 16 == 0 && PIN_PK_REPORT % 8 == 0, "layout of the pinned block");
// The packed calls' device workspace (ctx->packed_ws) begins as the pinned region does, so an upload lands where it came from: the
// table, the counters at PK_STATS for EVERY call, the match's pattern.  Behind the counters each call has its own layout:
//   encode, gather   from PK_SIZES: a size word per record, or per row        take   from PK_SIZES: a TakeRow per row
//   slice, field   from PK_SIZES: a TakeRow per row, then a list entry per row
//   number  from PK_SIZES: a NumberRow per row, then a list entry per row
//   concat  the encoded literal at PK_PATTERN (it ends in front of PK_SIZES); from PK_SIZES: a TakeRow per row, a list entry per row, a ConcatPiece per row
//   recode  the output table (256 x {code of map[s] under table OUT, length}, 2 KiB) at PK_PATTERN; behind it a TakeRow per row, then a list entry per row
//   search  as the match, then a position and a list entry per record
//   match   behind the pattern: the tile workspace (tile_ws)                   join   behind the counters: the tile workspace, the table's slots, a key number per record
//   group   as the join, the table sized for the records themselves, then a hash, a representative and a group number per record
//   order   (the match's LESS modes) the sorted codes, the counters, the pattern, the boundary table behind the pattern's last word, the tile workspace
constexpr size_t PK_STATS = 2048, PK_PATTERN = PK_STATS + PK_COUNTER_BYTES, PK_SIZES = 4096, PK_MATCH_TILES = PK_PATTERN + et::MATCH_PATTERN_BYTES;
static_assert(PK_PATTERN % 16 == 0 && PK_MATCH_TILES % 16 == 0 && PK_SIZES % 16 == 0 && sizeof(et::TakeRow) == 16,
              "k_match_flag loads pattern words, k_packed_scan 16 bytes of counts or sizes, k_take_plan stores a TakeRow as 16 bytes");
static_assert(int(et::PACKED_OK) == int(ET_OK) && int(et::PACKED_ARG) == int(ET_ERR_ARG) && int(et::PACKED_UNSUPPORTED) == int(ET_ERR_UNSUPPORTED), "a record's status byte is its et_status");
static_assert(sizeof(et::SharedJob) == 24 && PIN_SH_TABLE % 16 == 0, "layout of the pinned block");
static_assert(sizeof(et::BatchSpan) == 16 && sizeof(et::BatchEncJob) == 32 && sizeof(et::BatchDecJob) == 40, "job records are plain, packed data");
static_assert(et::BATCH_HEAD_STRIDE >= 1024 && PIN_BLOB % 16 == 0 && PIN_JOBS % 8 == 0, "layout of the pinned block");
// the device block of records: spans, then jobs
constexpr size_t DEV_JOBS = CH * sizeof(et::BatchSpan);

int ensure_batch(et_ctx *ctx, size_t n_items, size_t slot_bytes) {
    if (!ctx->h_batch) {
        ET_HIP(hipHostMalloc(reinterpret_cast<void **>(&ctx->h_batch), PIN_BYTES));
        std::memset(ctx->h_batch, 0, 64);
    }
    const size_t n = std::min(n_items, CH);
    ET_TRY(ensure(ctx, ctx->batch_jobs, DEV_JOBS + n * sizeof(et::BatchDecJob)));
    ET_TRY(ensure(ctx, ctx->batch_blob, n * slot_bytes));
    if (!ctx->batch_counter.p) {
        ET_TRY(ensure(ctx, ctx->batch_counter, 64));
        ET_HIP(hipMemsetAsync(ctx->batch_counter.p, 0, 64, ctx->stream));
    }
    return ET_OK;
}

// The low `len` bits of `code` (1 <= len <= 32) at the top of a word.
uint32_t et_left_aligned(uint32_t code, uint32_t len) { return len == 32 ? code : (code & ((1u << len) - 1u)) << (32 - len); }

template <typename T>
T *pin(et_ctx *ctx, size_t off) { return reinterpret_cast<T *>(ctx->h_batch + off); }

volatile uint64_t *epoch_word(et_ctx *ctx, int which) { return pin<uint64_t>(ctx, PIN_WORDS) + which; }

unsigned long long *epoch_word_dev(et_ctx *ctx, int which) { return reinterpret_cast<unsigned long long *>(pin<uint64_t>(ctx, PIN_WORDS) + which); }

// Has one of the addresses a bit of low_bits set?
template <typename... P>
bool misaligned(uintptr_t low_bits, P... ptrs) { return ((reinterpret_cast<uintptr_t>(ptrs) | ...) & low_bits) != 0; }

// The shared-table and the packed kernels decode, and compare, under a full tree alone.
int require_complete(et_ctx *ctx, const et_codebook *cb) {
    if (et_codebook_is_complete(cb) != ET_OK) return fail(ctx, ET_ERR_UNSUPPORTED, "the code table is not a full prefix-free tree of codes up to 32 bits");
    return ET_OK;
}

// Outputs of different items may not overlap (items that ask for no room take none).
bool outputs_overlap(const et_batch_item *items, size_t n) {
    std::vector<uint32_t> order;
    order.reserve(n);
    for (size_t i = 0; i < n; ++i)
        if (items[i].out_cap) order.push_back(static_cast<uint32_t>(i));
    auto by_off = [&](uint32_t a, uint32_t b) { return items[a].out_off < items[b].out_off; };
    if (!std::is_sorted(order.begin(), order.end(), by_off)) std::sort(order.begin(), order.end(), by_off);
    for (size_t k = 0; k + 1 < order.size(); ++k) {
        const et_batch_item &a = items[order[k]], &b = items[order[k + 1]];
        if (a.out_cap > b.out_off - a.out_off) return true;
    }
    return false;
}

int check_call(et_ctx *ctx, const void *d_in, void *d_out, et_batch_item *items, size_t n_items) {
    if (!ctx) return ET_ERR_ARG;
    if (n_items == 0) return ET_OK;
    if (!items || !d_in || !d_out) return fail(ctx, ET_ERR_ARG, "null pointer");
    if (n_items > 0x7fffffffu) return fail(ctx, ET_ERR_ARG, "too many items");
    for (size_t i = 0; i < n_items; ++i) {
        items[i].out_len = 0;
        items[i].status = ET_OK;
        items[i].path = 0;
    }
    if (outputs_overlap(items, n_items)) return fail(ctx, ET_ERR_ARG, "outputs of different items overlap");
    return ET_OK;
}

// The 2 KiB a shared-table or packed kernel keeps in LDS: 256 x {left-aligned code, length} for an encode; the codes sorted by
// left-aligned value, {code, length << 8 | symbol}, for a decode.  Returns how many codes there are.
uint32_t fill_shared_table(const et_codebook *cb, uint32_t *tab, bool encode) {
    uint32_t n_codes = 0;
    if (encode) {
        for (int s = 0; s < 256; ++s) {
            const uint32_t len = cb->length[s];
            tab[2 * s] = len ? et_left_aligned(cb->data[s], len) : 0u;
            tab[2 * s + 1] = len;
            n_codes += len != 0;
        }
    } else {
        struct Code { uint32_t lo, meta; };
        Code *codes = reinterpret_cast<Code *>(tab);
        for (int s = 0; s < 256; ++s)
            if (cb->length[s]) codes[n_codes++] = Code{et_left_aligned(cb->data[s], cb->length[s]), static_cast<uint32_t>(cb->length[s]) << 8 | static_cast<uint32_t>(s)};
        std::sort(codes, codes + n_codes, [](const Code &a, const Code &b) { return a.lo < b.lo; });
    }
    return n_codes;
}

// Both shared-table calls.  encode: d_out may be null (sizes only).
int shared_call(et_ctx *ctx, const et_codebook *cb, const void *d_in, void *d_out, et_batch_item *items, size_t n_items, bool encode) {
    if (!ctx) return ET_ERR_ARG;
    if (n_items == 0) return ET_OK;
    if (!cb || !items || !d_in || (!d_out && !encode)) return fail(ctx, ET_ERR_ARG, "null pointer");
    if (n_items > 0x7fffffffu) return fail(ctx, ET_ERR_ARG, "too many items");
    for (size_t i = 0; i < n_items; ++i) {
        items[i].out_len = 0;
        items[i].status = ET_OK;
        items[i].path = 0;
    }
    ET_TRY(require_complete(ctx, cb));
    if (d_out && outputs_overlap(items, n_items)) return fail(ctx, ET_ERR_ARG, "outputs of different items overlap");
    DeviceGuard guard(ctx->device);

    std::vector<uint32_t> todo;
    for (size_t i = 0; i < n_items; ++i) {
        et_batch_item &it = items[i];
        if (it.in_len == 0 || (!encode && it.out_cap == 0)) continue;  // an empty record is a record: ET_OK, nothing to do
        if ((encode ? it.in_len : it.out_cap) > et::BATCH_SMALL_MAX) it.status = ET_ERR_UNSUPPORTED;
        else todo.push_back(static_cast<uint32_t>(i));
    }
    if (todo.empty()) return ET_OK;
    ET_TRY(ensure_batch(ctx, 1, 2048));
    ET_TRY(ensure(ctx, ctx->batch_jobs, std::min(todo.size(), SCH) * sizeof(et::SharedJob)));

    // the table: free to fill (this file's header), up in front of the first chunk
    uint32_t *tab = pin<uint32_t>(ctx, PIN_SH_TABLE);
    const uint32_t n_codes = fill_shared_table(cb, tab, encode);
    ET_HIP(hipMemcpyAsync(ctx->batch_blob.p, tab, 2048, hipMemcpyHostToDevice, ctx->stream));

    for (size_t c0 = 0; c0 < todo.size(); c0 += SCH) {
        const uint32_t n = static_cast<uint32_t>(std::min(SCH, todo.size() - c0));
        et::SharedJob *jobs = pin<et::SharedJob>(ctx, PIN_SH_JOBS);
        for (uint32_t j = 0; j < n; ++j) {
            const et_batch_item &it = items[todo[c0 + j]];
            if (encode) {
                const uint64_t cap = d_out ? it.out_cap : ~0ull;
                jobs[j] = et::SharedJob{it.in_off, it.out_off, static_cast<uint32_t>(it.in_len), static_cast<uint32_t>(std::min<uint64_t>(cap, 0xffffffffu))};
            } else {
                jobs[j] = et::SharedJob{it.in_off, it.out_off, static_cast<uint32_t>(et::clip_body(it.in_len, it.out_cap)), static_cast<uint32_t>(it.out_cap)};
            }
        }
        ET_HIP(hipMemcpyAsync(ctx->batch_jobs.p, jobs, n * sizeof(et::SharedJob), hipMemcpyHostToDevice, ctx->stream));
        const uint64_t epoch = ++ctx->batch_epoch;
        uint2 *results = pin<uint2>(ctx, PIN_SH_RESULTS);
        if (encode)
            et::launch_shared_encode(ctx->stream, d_in, d_out, static_cast<const et::SharedJob *>(ctx->batch_jobs.p), n, static_cast<const uint2 *>(ctx->batch_blob.p),
                                     results, static_cast<uint32_t *>(ctx->batch_counter.p), epoch_word_dev(ctx, 3), epoch);
        else
            et::launch_shared_decode(ctx->stream, d_in, d_out, static_cast<const et::SharedJob *>(ctx->batch_jobs.p), n, static_cast<const uint2 *>(ctx->batch_blob.p),
                                     n_codes, results, static_cast<uint32_t *>(ctx->batch_counter.p), epoch_word_dev(ctx, 3), epoch);
        ET_HIP(hipGetLastError());
        ET_TRY(wait_for_word<uint64_t>(ctx, epoch_word(ctx, 3), epoch, 2000.0, "the shared-table batch's results never reached the host"));
        for (uint32_t j = 0; j < n; ++j) {
            et_batch_item &it = items[todo[c0 + j]];
            it.status = results[j].y == et::SHARED_OK ? ET_OK : results[j].y == et::SHARED_CAP ? ET_ERR_CAP : ET_ERR_UNSUPPORTED;
            it.out_len = results[j].x;
        }
    }
    return ET_OK;
}

// ---- what the packed calls are made of -------------------------------------------------------------------------------------
// Offsets into ctx->packed_ws, handed out from `end` on: a call lays its workspace out ONCE, sizes ensure() by `end` and forms its
// pointers from the offsets it got.
struct Bump {
    size_t end;
    size_t take(size_t bytes, size_t align) {
        const size_t at = (end + align - 1) & ~(align - 1);
        end = at + bytes;
        return at;
    }
};

template <typename T>
T *ws(et_ctx *ctx, size_t off) { return reinterpret_cast<T *>(static_cast<uint8_t *>(ctx->packed_ws.p) + off); }

// The tile workspace of the match and the join: a count per tile (padded to 16 bytes), the tiles' first places (tiles + 1), four masks per tile.
struct TileOffsets { size_t counts, base, masks; };

TileOffsets tile_ws(Bump &b, size_t n_records) {
    const size_t n_tiles = (n_records + et::MATCH_TILE - 1) / et::MATCH_TILE;
    TileOffsets t;
    t.counts = b.take((n_tiles * 4 + 15) & ~static_cast<size_t>(15), 16);
    t.base = b.take((n_tiles + 1) * 8, 16);
    t.masks = b.take(n_tiles * (et::MATCH_TILE / 64) * 8, 8);
    return t;
}

et::TileWs tile_ptrs(et_ctx *ctx, const TileOffsets &t) { return et::TileWs{ws<unsigned long long>(ctx, t.masks), ws<uint32_t>(ctx, t.counts), ws<uint64_t>(ctx, t.base)}; }

// The pinned block and a workspace of ws_bytes.
int packed_ensure(et_ctx *ctx, size_t ws_bytes) {
    ET_TRY(ensure_batch(ctx, 1, 2048));
    return ensure(ctx, ctx->packed_ws, ws_bytes);
}

// The counters' first values in the pinned region (free to fill: this file's header): zero, and no failed record yet.
uint64_t *first_counters(et_ctx *ctx) {
    uint64_t *first = pin<uint64_t>(ctx, PIN_PK_STATS);
    std::memset(first, 0, PK_COUNTER_BYTES);
    first[et::PACKED_FIRST] = ~0ull;
    return first;
}

// The next epoch, and where the kernels of this call count and report.
et::PackedReport next_report(et_ctx *ctx) {
    return et::PackedReport{ws<unsigned long long>(ctx, PK_STATS), reinterpret_cast<unsigned long long *>(pin<uint64_t>(ctx, PIN_PK_REPORT)), epoch_word_dev(ctx, 4), ++ctx->batch_epoch};
}

// Behind the launches: the poll; the report's words are there when it returns ET_OK.
int packed_poll(et_ctx *ctx, uint64_t epoch, const char *what) {
    ET_HIP(hipGetLastError());
    return wait_for_word<uint64_t>(ctx, epoch_word(ctx, 4), epoch, 2000.0, what);
}

const uint64_t *report_words(et_ctx *ctx) { return pin<uint64_t>(ctx, PIN_PK_REPORT); }

// The pair of failure counters at rep[word]: how many failed and, when any did, the lowest of them and its status.
void read_failures(const uint64_t *rep, int word, uint64_t *n, uint64_t *first, int32_t *status) {
    *n = rep[word];
    if (!*n) return;
    *first = rep[word + 1] >> 8;
    *status = static_cast<int32_t>(rep[word + 1] & 0xffu);
}
static_assert(et::PACKED_FIRST == et::PACKED_N_FAILED + 1 && et::JOIN_KEYS_FIRST == et::JOIN_KEYS_FAILED + 1, "read_failures");

// The calls with a table on the device (encode, decode, gather), behind their argument check: the table is judged, the workspace
// made (ws_words size words behind the table and the counters), then the table and the counters' first values go up in one copy.
int packed_upload(et_ctx *ctx, const et_codebook *cb, bool encode, size_t ws_words, uint32_t *n_codes) {
    ET_TRY(require_complete(ctx, cb));
    ET_TRY(packed_ensure(ctx, PK_SIZES + ws_words * sizeof(uint32_t)));
    *n_codes = fill_shared_table(cb, pin<uint32_t>(ctx, PIN_PK_TABLE), encode);
    first_counters(ctx);
    ET_HIP(hipMemcpyAsync(ctx->packed_ws.p, pin<uint8_t>(ctx, PIN_PK_TABLE), PK_STATS + PK_COUNTER_BYTES, hipMemcpyHostToDevice, ctx->stream));
    return ET_OK;
}

// ... their arguments (the encode's and the range decode's), and *res cleared ...
int packed_args(et_ctx *ctx, const et_codebook *cb, const void *d_in, const void *d_out, const uint64_t *idx_a, const uint64_t *idx_b, size_t n, et_packed_result *res,
                bool encode) {
    if (!cb || !res || !d_in || !idx_a || !idx_b || (!d_out && !encode)) return fail(ctx, ET_ERR_ARG, "null pointer");
    if (misaligned(7, idx_a, idx_b)) return fail(ctx, ET_ERR_ARG, "an offset array is not 8-byte aligned");
    if (n > 0x7fffffffu) return fail(ctx, ET_ERR_ARG, "too many records");
    *res = et_packed_result{};
    return ET_OK;
}

// ... and their end: the poll, the report into *res; ET_ERR_CAP (`too_much`) when a capacity was given and the report exceeds it.
int packed_end(et_ctx *ctx, uint64_t epoch, et_packed_result *res, bool capped, uint64_t cap, const char *too_much) {
    ET_TRY(packed_poll(ctx, epoch, "the packed batch's report never reached the host"));
    const uint64_t *rep = report_words(ctx);
    res->out_bytes = rep[et::PACKED_BYTES];
    res->n_short = rep[et::PACKED_N_SHORT];
    read_failures(rep, et::PACKED_N_FAILED, &res->n_failed, &res->first_failed, &res->first_status);
    if (capped && res->out_bytes > cap) return fail(ctx, ET_ERR_CAP, too_much);  // (the call's last kernel saw the same two figures)
    return ET_OK;
}

// ---- the calls that select records of a packed store (match with its order modes, search, join, group) ------------------------
// A store as a selecting or a deriving call is given it, and what the kernels take it for.
struct Source {
    const void *bodies;
    size_t body_bytes;
    const uint64_t *body_index, *text_index;
    size_t n;
    const uint32_t *rows;  // null: row k is record k
};

et::PackedStore packed_store(const Source &s) { return et::PackedStore{s.bodies, s.body_bytes, s.body_index, s.text_index, static_cast<uint32_t>(s.n), 0}; }

// The head of a selecting call, the checks in THIS order: the store (and the join's key set, unless empty) is there and `missing`, one of
// the call's own pointers, is not true; the offset arrays are 8-byte, the 32-bit outputs `out32` 4-byte aligned; `most` records at most.
struct SelectTexts { const char *unaligned4, *too_many; };  // the two texts that differ between the calls

int select_args(et_ctx *ctx, const et_codebook *cb, const void *res, const Source &s, const Source *keys, bool missing, std::initializer_list<const void *> out32, size_t most,
                const SelectTexts &t) {
    const bool no_keys = keys && keys->n && (!keys->bodies || !keys->body_index || !keys->text_index);
    if (!cb || !res || !s.bodies || !s.body_index || !s.text_index || missing || no_keys) return fail(ctx, ET_ERR_ARG, "null pointer");
    if (misaligned(7, s.body_index, s.text_index) || (keys && misaligned(7, keys->body_index, keys->text_index))) return fail(ctx, ET_ERR_ARG, "an offset array is not 8-byte aligned");
    for (const void *out : out32)
        if (misaligned(3, out)) return fail(ctx, ET_ERR_ARG, t.unaligned4);
    if (s.n > most) return fail(ctx, ET_ERR_ARG, t.too_many);
    return ET_OK;
}

// ... and its tail, behind the launches: the poll (`never`), the fault bit of a call with a hash table (`fault`: ET_ERR_HIP), how many
// were selected (res->*count), the records' failures; ET_ERR_CAP (`too_much`) when rows were asked for and more are selected than `cap`.
template <typename Res>
int selected_end(et_ctx *ctx, uint64_t epoch, Res *res, uint64_t Res::*count, const void *d_rows, uint64_t cap, const char *never, const char *too_much, const char *fault = nullptr) {
    ET_TRY(packed_poll(ctx, epoch, never));
    const uint64_t *rep = report_words(ctx);
    if (fault && (rep[et::PACKED_N_FAILED] & et::JOIN_FAULT_BIT)) return fail(ctx, ET_ERR_HIP, fault);
    res->*count = rep[et::PACKED_BYTES];
    read_failures(rep, et::PACKED_N_FAILED, &res->n_failed, &res->first_failed, &res->first_status);
    if (d_rows && res->*count > cap) return fail(ctx, ET_ERR_CAP, too_much);
    return ET_OK;
}

// The needle of the match, its order modes and the search: the pattern of its first n_coded bytes (et_encode_pattern) in the pinned
// block (behind packed_ensure), zero-padded to a word and `spare` bytes on; the bits, the length and the flags the three jobs share (a byte
// without a code: MATCH_F_NEVER; the order modes' codable prefix has none); pattern_bits.  The head words are each family's own.
struct Needle { const uint8_t *pattern; size_t pat_bytes, padded; };

template <typename Job>
int needle_job(et_ctx *ctx, const et_codebook *cb, const uint8_t *needle, size_t n_coded, size_t needle_len, size_t pattern_cap, int mode, size_t spare, Job *job,
               et_match_result *res, Needle *nd) {
    uint8_t *pattern = pin<uint8_t>(ctx, PIN_PK_PATTERN);
    uint64_t bits = 0;
    const int rc = et_encode_pattern(cb, needle, n_coded, pattern, pattern_cap, &bits);
    if (rc != ET_OK && rc != ET_ERR_UNSUPPORTED) return fail(ctx, rc, "et_encode_pattern");
    const size_t pat_bytes = static_cast<size_t>((bits + 7) / 8), padded = (pat_bytes + 3) & ~static_cast<size_t>(3);
    std::memset(pattern + pat_bytes, 0, padded + spare - pat_bytes);
    job->pat_bits = static_cast<uint32_t>(bits);
    job->needle_len = static_cast<uint32_t>(needle_len);
    job->flags = ((mode & ET_MATCH_NOT) ? et::MATCH_F_NOT : 0u) | (rc == ET_ERR_UNSUPPORTED ? et::MATCH_F_NEVER : 0u);
    res->pattern_bits = job->pat_bits;
    *nd = Needle{pattern, pat_bytes, padded};
    return ET_OK;
}

// The order modes of et_match_packed_device, behind its argument check.  A needle byte without a code ends the codable prefix
// needle[:K]: no record holds that byte, so the prefix's bits and the byte itself (the table's last entry) decide.
int order_call(et_ctx *ctx, const et_codebook *cb, const et::PackedStore &store, const uint8_t *needle, size_t needle_len, int mode, uint32_t *d_rows, size_t cap_rows,
               uint8_t *d_status, et_match_result *res) {
    size_t K = 0, bits = 0;
    while (K < needle_len && cb->length[needle[K]] >= 1 && cb->length[needle[K]] <= 32) bits += cb->length[needle[K++]];
    const size_t pat_bytes = static_cast<size_t>((bits + 7) / 8), padded = (pat_bytes + 3) & ~static_cast<size_t>(3);
    Bump layout{PK_PATTERN + padded};
    const size_t at_starts = layout.take((K + 1) * 4, 4);
    const TileOffsets tiles = tile_ws(layout, store.n);
    ET_TRY(packed_ensure(ctx, layout.end));

    // the sorted codes, the counters' first values, the prefix's bits and the boundaries lie one behind the other: up in one copy
    // (2 KiB + 64 bytes + at most 16 KiB of pattern + at most 4 097 words: 35 KiB at the most, where EQUAL and PREFIX send 16 KiB)
    const uint32_t n_codes = fill_shared_table(cb, pin<uint32_t>(ctx, PIN_PK_TABLE), false);
    first_counters(ctx);
    et::OrderJob job{};
    Needle nd;
    ET_TRY(needle_job(ctx, cb, needle, K, needle_len, et::MATCH_PATTERN_BYTES, mode, 0, &job, res, &nd));
    uint32_t *starts = pin<uint32_t>(ctx, PIN_PK_TABLE + at_starts);
    uint32_t bit = 0;
    for (size_t i = 0; i < K; ++i) {
        starts[i] = bit << 8 | needle[i];
        bit += cb->length[needle[i]];
    }
    starts[K] = bit << 8 | (K < needle_len ? needle[K] : 0u);
    job.n_coded = static_cast<uint32_t>(K);
    job.flags |= ((mode & ~ET_MATCH_NOT) == ET_MATCH_LESS_EQUAL ? et::ORDER_F_EQUAL_TOO : 0u) | (K < needle_len ? et::ORDER_F_TAIL : 0u);
    for (uint32_t k = 0; k < std::min<size_t>(nd.pat_bytes, 8); ++k) job.head |= static_cast<uint64_t>(nd.pattern[k]) << (56 - 8 * k);  // (big-endian: bit 0 of the body is bit 63)
    ET_HIP(hipMemcpyAsync(ctx->packed_ws.p, pin<uint8_t>(ctx, PIN_PK_TABLE), at_starts + (K + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    const et::PackedReport report = next_report(ctx);
    et::launch_order(ctx->stream, store, ws<const uint2>(ctx, 0), n_codes, ws<const uint32_t>(ctx, PK_PATTERN), ws<const uint32_t>(ctx, at_starts), job, d_rows, cap_rows, d_status,
                     tile_ptrs(ctx, tiles), report);
    return selected_end(ctx, report.epoch, res, &et_match_result::n_match, d_rows, cap_rows, "the match's report never reached the host", "more records are selected than cap_rows");
}

// An item's own failure is the item's; a failure of the runtime under a delegated stream is the call's.
bool call_level(int rc) { return rc == ET_ERR_HIP || rc == ET_ERR_NOMEM; }

}  // namespace

extern "C" size_t et_batch_small_max(void) { return et::BATCH_SMALL_MAX; }

extern "C" size_t et_batch_item_size(void) { return sizeof(et_batch_item); }

extern "C" int et_encode_shared_device(et_ctx *ctx, const et_codebook *cb, const void *d_in, void *d_out, et_batch_item *items, size_t n_items) {
    return shared_call(ctx, cb, d_in, d_out, items, n_items, true);
}

extern "C" int et_decode_shared_device(et_ctx *ctx, const et_codebook *cb, const void *d_in, void *d_out, et_batch_item *items, size_t n_items) {
    return shared_call(ctx, cb, d_in, d_out, items, n_items, false);
}

extern "C" size_t et_packed_result_size(void) { return sizeof(et_packed_result); }

extern "C" int et_encode_packed_device(et_ctx *ctx, const et_codebook *cb, const void *d_text, size_t text_bytes, const uint64_t *d_text_index, size_t n, void *d_out,
                                       size_t cap, uint64_t *d_out_index, uint8_t *d_status, et_packed_result *res) {
    if (!ctx) return ET_ERR_ARG;
    DeviceGuard guard(ctx->device);
    ET_TRY(packed_args(ctx, cb, d_text, d_out, d_text_index, d_out_index, n, res, true));
    if (n == 0) return ET_OK;
    uint32_t n_codes = 0;
    ET_TRY(packed_upload(ctx, cb, true, n, &n_codes));
    const et::PackedReport report = next_report(ctx);
    et::launch_packed_encode(ctx->stream, d_text, text_bytes, d_text_index, static_cast<uint32_t>(n), d_out, cap, d_out_index, d_status, ws<const uint2>(ctx, 0),
                             ws<uint32_t>(ctx, PK_SIZES), report);
    return packed_end(ctx, report.epoch, res, d_out != nullptr, cap, "the bodies take more than cap bytes");
}

extern "C" int et_decode_packed_device(et_ctx *ctx, const et_codebook *cb, const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                                       const uint64_t *d_text_index, size_t n, void *d_out, size_t cap, uint32_t *d_written, uint8_t *d_status, et_packed_result *res) {
    if (!ctx) return ET_ERR_ARG;
    DeviceGuard guard(ctx->device);
    ET_TRY(packed_args(ctx, cb, d_bodies, d_out, d_body_index, d_text_index, n, res, false));
    if (n == 0) return ET_OK;
    uint32_t n_codes = 0;
    ET_TRY(packed_upload(ctx, cb, false, 0, &n_codes));
    const et::PackedReport report = next_report(ctx);
    et::launch_packed_decode(ctx->stream, et::PackedStore{d_bodies, body_bytes, d_body_index, d_text_index, static_cast<uint32_t>(n), 0}, d_out, cap, ws<const uint2>(ctx, 0),
                             n_codes, d_written, d_status, report, static_cast<uint32_t *>(ctx->batch_counter.p));
    return packed_end(ctx, report.epoch, res, true, cap, "text_index[n] lies beyond cap");
}

extern "C" int et_decode_packed_gather_device(et_ctx *ctx, const et_codebook *cb, const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                                              const uint64_t *d_text_index, size_t n_records, const uint32_t *d_rows, size_t n_rows, void *d_out, size_t cap,
                                              uint64_t *d_out_index, uint32_t *d_written, uint8_t *d_status, et_packed_result *res) {
    if (!ctx) return ET_ERR_ARG;
    if (!cb || !res || !d_bodies || !d_body_index || !d_text_index || !d_rows || !d_out_index) return fail(ctx, ET_ERR_ARG, "null pointer");
    if (misaligned(7, d_body_index, d_text_index, d_out_index)) return fail(ctx, ET_ERR_ARG, "an offset array is not 8-byte aligned");
    if (misaligned(3, d_rows)) return fail(ctx, ET_ERR_ARG, "the rows are not 4-byte aligned");
    if (n_records > 0x7fffffffu || n_rows > 0x7fffffffu) return fail(ctx, ET_ERR_ARG, "too many records or rows");
    *res = et_packed_result{};
    if (n_rows == 0) return ET_OK;
    DeviceGuard guard(ctx->device);
    uint32_t n_codes = 0;
    ET_TRY(packed_upload(ctx, cb, false, n_rows, &n_codes));
    const et::PackedReport report = next_report(ctx);
    et::launch_packed_gather(ctx->stream, et::PackedStore{d_bodies, body_bytes, d_body_index, d_text_index, static_cast<uint32_t>(n_records), 0}, d_rows,
                             static_cast<uint32_t>(n_rows), d_out, cap, d_out_index, ws<const uint2>(ctx, 0), n_codes, d_written, d_status, ws<uint32_t>(ctx, PK_SIZES), report,
                             static_cast<uint32_t *>(ctx->batch_counter.p));
    return packed_end(ctx, report.epoch, res, d_out != nullptr, cap, "the rows take more than cap bytes");
}

extern "C" size_t et_match_pattern_max(void) { return et::MATCH_NEEDLE_MAX; }

extern "C" size_t et_match_result_size(void) { return sizeof(et_match_result); }

extern "C" int et_match_packed_device(et_ctx *ctx, const et_codebook *cb, const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                                      const uint64_t *d_text_index, size_t n_records, const uint8_t *needle, size_t needle_len, int mode, uint32_t *d_rows,
                                      size_t cap_rows, uint8_t *d_status, et_match_result *res) {
    if (!ctx) return ET_ERR_ARG;
    const Source src{d_bodies, body_bytes, d_body_index, d_text_index, n_records, nullptr};
    ET_TRY(select_args(ctx, cb, res, src, nullptr, !needle && needle_len, {d_rows}, 0x7fffffffu, {"the rows are not 4-byte aligned", "too many records"}));
    if (needle_len > et::MATCH_NEEDLE_MAX) return fail(ctx, ET_ERR_ARG, "the needle is longer than et_match_pattern_max()");
    const int what = mode & ~ET_MATCH_NOT;
    const bool order = what == ET_MATCH_LESS || what == ET_MATCH_LESS_EQUAL;
    if (what != ET_MATCH_EQUAL && what != ET_MATCH_PREFIX && !order) return fail(ctx, ET_ERR_ARG, "unknown mode");
    *res = et_match_result{};
    if (n_records == 0) return ET_OK;
    ET_TRY(require_complete(ctx, cb));
    DeviceGuard guard(ctx->device);
    const et::PackedStore store = packed_store(src);
    if (order) return order_call(ctx, cb, store, needle, needle_len, mode, d_rows, cap_rows, d_status, res);
    Bump layout{PK_MATCH_TILES};
    const TileOffsets tiles = tile_ws(layout, store.n);
    ET_TRY(packed_ensure(ctx, layout.end));

    // the counters' first values and the needle's bits, up in one copy
    const uint64_t *first = first_counters(ctx);
    et::MatchJob job{};
    Needle nd;
    ET_TRY(needle_job(ctx, cb, needle, needle_len, needle_len, et::MATCH_PATTERN_BYTES, mode, 0, &job, res, &nd));
    job.flags |= what == ET_MATCH_EQUAL ? et::MATCH_F_EQUAL : 0u;
    const uint64_t head_bits = std::min<uint64_t>(job.pat_bits, et::MATCH_HEAD_BITS);
    for (uint32_t k = 0; k < (head_bits + 7) / 8; ++k) {  // (memory order: byte k of the body is bits 8k .. 8k + 7 of the word)
        const uint64_t left = head_bits - 8 * k;
        job.head |= static_cast<uint64_t>(nd.pattern[k]) << (8 * k);
        job.head_mask |= static_cast<uint64_t>(left >= 8 ? 0xffu : (0xffu << (8 - left)) & 0xffu) << (8 * k);
    }
    ET_HIP(hipMemcpyAsync(ws<uint8_t>(ctx, PK_STATS), first, PK_COUNTER_BYTES + nd.padded, hipMemcpyHostToDevice, ctx->stream));
    const et::PackedReport report = next_report(ctx);
    et::launch_match(ctx->stream, store, ws<const uint32_t>(ctx, PK_PATTERN), job, d_rows, cap_rows, d_status, tile_ptrs(ctx, tiles), report);
    return selected_end(ctx, report.epoch, res, &et_match_result::n_match, d_rows, cap_rows, "the match's report never reached the host", "more records match than cap_rows");
}

extern "C" size_t et_search_needle_max(void) { return et::SEARCH_NEEDLE_MAX; }

extern "C" size_t et_search_lane_bytes(void) { return et::SEARCH_LANE_BYTES; }

extern "C" int et_search_packed_device(et_ctx *ctx, const et_codebook *cb, const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                                       const uint64_t *d_text_index, size_t n_records, const uint8_t *needle, size_t needle_len, int mode, uint32_t *d_rows,
                                       size_t cap_rows, uint32_t *d_pos, uint8_t *d_status, et_match_result *res) {
    if (!ctx) return ET_ERR_ARG;
    const Source src{d_bodies, body_bytes, d_body_index, d_text_index, n_records, nullptr};
    ET_TRY(select_args(ctx, cb, res, src, nullptr, !needle && needle_len, {d_rows, d_pos}, 0x7fffffffu, {"the rows or the positions are not 4-byte aligned", "too many records"}));
    if (needle_len > et::SEARCH_NEEDLE_MAX) return fail(ctx, ET_ERR_ARG, "the needle is longer than et_search_needle_max()");
    const int what = mode & ~ET_MATCH_NOT;
    if (what != ET_SEARCH_CONTAINS && what != ET_SEARCH_SUFFIX) return fail(ctx, ET_ERR_ARG, "unknown mode");
    if (d_pos && (mode & ET_MATCH_NOT)) return fail(ctx, ET_ERR_ARG, "a record without an occurrence has no position");
    if (d_pos && !d_rows) return fail(ctx, ET_ERR_ARG, "positions without rows");
    *res = et_match_result{};
    if (n_records == 0) return ET_OK;
    ET_TRY(require_complete(ctx, cb));
    DeviceGuard guard(ctx->device);
    const et::PackedStore store = packed_store(src);
    Bump layout{PK_MATCH_TILES};
    const TileOffsets tiles = tile_ws(layout, store.n);
    const size_t at_pos = layout.take(static_cast<size_t>(store.n) * 4, 4), at_list = layout.take(static_cast<size_t>(store.n) * 4, 4);
    ET_TRY(packed_ensure(ctx, layout.end));

    // the sorted codes, the counters' first values and the needle's bits lie one behind the other: up in one copy
    const uint32_t n_codes = fill_shared_table(cb, pin<uint32_t>(ctx, PIN_PK_TABLE), false);
    first_counters(ctx);
    et::SearchJob job{};
    Needle nd;  // (4 spare bytes: the word the head is read from, for a pattern of no bytes)
    ET_TRY(needle_job(ctx, cb, needle, needle_len, needle_len, et::SEARCH_PATTERN_BYTES, mode, 4, &job, res, &nd));
    job.flags |= what == ET_SEARCH_SUFFIX ? et::SEARCH_F_SUFFIX : 0u;
    job.head_mask = job.pat_bits >= 32 ? 0xffffffffu : job.pat_bits ? ~(0xffffffffu >> job.pat_bits) : 0u;
    job.head = (static_cast<uint32_t>(nd.pattern[0]) << 24 | static_cast<uint32_t>(nd.pattern[1]) << 16 | static_cast<uint32_t>(nd.pattern[2]) << 8 | nd.pattern[3]) & job.head_mask;
    ET_HIP(hipMemcpyAsync(ctx->packed_ws.p, pin<uint8_t>(ctx, PIN_PK_TABLE), PK_PATTERN + nd.padded, hipMemcpyHostToDevice, ctx->stream));
    const et::PackedReport report = next_report(ctx);
    et::launch_search(ctx->stream, store, ws<const uint2>(ctx, 0), n_codes, ws<const uint32_t>(ctx, PK_PATTERN), job, d_rows, cap_rows, d_pos, d_status, tile_ptrs(ctx, tiles),
                      ws<uint32_t>(ctx, at_pos), ws<uint32_t>(ctx, at_list), report);
    return selected_end(ctx, report.epoch, res, &et_match_result::n_match, d_rows, cap_rows, "the search's report never reached the host", "more records are selected than cap_rows");
}

extern "C" size_t et_join_keys_max(void) { return et::ET_JOIN_KEYS_MAX; }

extern "C" size_t et_join_result_size(void) { return sizeof(et_join_result); }

extern "C" size_t et_join_table_slots(size_t n_keys) { return et::et_join_slots_for(std::min(n_keys, et::ET_JOIN_KEYS_MAX)); }

extern "C" uint64_t et_join_hash(const uint8_t *body, size_t n_bytes, uint64_t length) {
    uint64_t sum = 0;
    for (size_t i = 0; 8 * i < n_bytes; ++i) {
        uint64_t word = 0;
        for (size_t k = 0; k < std::min<size_t>(8, n_bytes - 8 * i); ++k) word |= static_cast<uint64_t>(body[8 * i + k]) << (8 * k);
        sum += et::et_join_term(i, word);
    }
    return et::et_join_finish(sum, n_bytes, length);
}

extern "C" int et_join_packed_device(et_ctx *ctx, const et_codebook *cb, const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                                     const uint64_t *d_text_index, size_t n_records, const void *d_key_bodies, size_t key_body_bytes, const uint64_t *d_key_body_index,
                                     const uint64_t *d_key_text_index, size_t n_keys, int mode, uint32_t *d_rows, size_t cap_rows, uint32_t *d_key_of_row, uint8_t *d_status,
                                     uint8_t *d_key_status, et_join_result *res) {
    if (!ctx) return ET_ERR_ARG;
    const Source src{d_bodies, body_bytes, d_body_index, d_text_index, n_records, nullptr}, key_src{d_key_bodies, key_body_bytes, d_key_body_index, d_key_text_index, n_keys, nullptr};
    ET_TRY(select_args(ctx, cb, res, src, &key_src, false, {d_rows, d_key_of_row}, 0x7fffffffu, {"the rows are not 4-byte aligned", "too many records"}));
    if (n_keys > et::ET_JOIN_KEYS_MAX) return fail(ctx, ET_ERR_ARG, "more keys than et_join_keys_max()");
    if (mode != 0 && mode != ET_MATCH_NOT) return fail(ctx, ET_ERR_ARG, "unknown mode");
    if (d_key_of_row && (mode & ET_MATCH_NOT)) return fail(ctx, ET_ERR_ARG, "a record no key equals has no key number");
    if (d_key_of_row && !d_rows) return fail(ctx, ET_ERR_ARG, "key numbers without rows");
    *res = et_join_result{};
    if (n_records == 0) return ET_OK;
    ET_TRY(require_complete(ctx, cb));
    DeviceGuard guard(ctx->device);
    const et::PackedStore records = packed_store(src), keys = packed_store(key_src);
    const size_t slots = et::et_join_slots_for(n_keys);
    Bump layout{PK_STATS + PK_COUNTER_BYTES};
    const TileOffsets tiles = tile_ws(layout, records.n);
    const size_t at_table = layout.take(slots * 8, 8), at_key_of = layout.take(static_cast<size_t>(records.n) * 4, 4);
    ET_TRY(packed_ensure(ctx, layout.end));

    // the counters' first values: the keys' lowest failure and the smallest body of a key beside the records'
    uint64_t *first = first_counters(ctx);
    first[et::JOIN_KEYS_FIRST] = first[et::JOIN_MIN] = ~0ull;
    ET_HIP(hipMemcpyAsync(ws<uint8_t>(ctx, PK_STATS), first, PK_COUNTER_BYTES, hipMemcpyHostToDevice, ctx->stream));
    if (n_keys) ET_HIP(hipMemsetAsync(ws<uint8_t>(ctx, at_table), 0xff, slots * 8, ctx->stream));
    const et::PackedReport report = next_report(ctx);
    et::launch_join(ctx->stream, records, keys, (mode & ET_MATCH_NOT) ? et::MATCH_F_NOT : 0u, ws<unsigned long long>(ctx, at_table), slots, d_rows, cap_rows, d_key_of_row,
                    d_status, d_key_status, tile_ptrs(ctx, tiles), ws<uint32_t>(ctx, at_key_of), report);
    const int rc = selected_end(ctx, report.epoch, res, &et_join_result::n_match, d_rows, cap_rows, "the join's report never reached the host",
                                "more records are selected than cap_rows", "a probe sequence of the join's table met no empty slot");
    if (rc == ET_OK || rc == ET_ERR_CAP) read_failures(report_words(ctx), et::JOIN_KEYS_FAILED, &res->n_keys_failed, &res->first_key_failed, &res->first_key_status);
    return rc;  // (the keys' failures are reported with ET_ERR_CAP too, as the records' are)
}

extern "C" size_t et_group_result_size(void) { return sizeof(et_group_result); }

extern "C" size_t et_group_records_max(void) { return et::ET_JOIN_KEYS_MAX; }

static_assert(ET_GROUP_NONE == et::GROUP_NONE, "d_group_of of a failed record");

extern "C" int et_group_packed_device(et_ctx *ctx, const et_codebook *cb, const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                                      const uint64_t *d_text_index, size_t n_records, uint32_t *d_first_rows, size_t cap_groups, uint32_t *d_count, uint32_t *d_group_of,
                                      uint8_t *d_status, et_group_result *res) {
    if (!ctx) return ET_ERR_ARG;
    const Source src{d_bodies, body_bytes, d_body_index, d_text_index, n_records, nullptr};
    ET_TRY(select_args(ctx, cb, res, src, nullptr, false, {d_first_rows, d_count, d_group_of}, et::ET_JOIN_KEYS_MAX,
                       {"the first rows, the counts or the group numbers are not 4-byte aligned", "more records than et_group_records_max()"}));
    if ((d_count || d_group_of) && !d_first_rows) return fail(ctx, ET_ERR_ARG, "counts or group numbers without first rows");
    *res = et_group_result{};
    if (n_records == 0) return ET_OK;
    ET_TRY(require_complete(ctx, cb));
    DeviceGuard guard(ctx->device);
    const et::PackedStore records = packed_store(src);
    // the join's layout, the store as its own key set, plus three words per record: its hash, its representative, and a representative's group
    const size_t slots = et::et_join_slots_for(n_records);
    Bump layout{PK_STATS + PK_COUNTER_BYTES};
    const TileOffsets tiles = tile_ws(layout, records.n);
    const size_t at_table = layout.take(slots * 8, 8), at_hash_of = layout.take(n_records * 8, 8), at_rep_of = layout.take(n_records * 4, 4), at_dense = layout.take(n_records * 4, 4);
    ET_TRY(packed_ensure(ctx, layout.end));

    const uint64_t *first = first_counters(ctx);
    ET_HIP(hipMemcpyAsync(ws<uint8_t>(ctx, PK_STATS), first, PK_COUNTER_BYTES, hipMemcpyHostToDevice, ctx->stream));
    ET_HIP(hipMemsetAsync(ws<uint8_t>(ctx, at_table), 0xff, slots * 8, ctx->stream));
    const et::PackedReport report = next_report(ctx);
    et::launch_group(ctx->stream, records, ws<unsigned long long>(ctx, at_table), slots, d_first_rows, cap_groups, d_count, d_group_of, d_status, tile_ptrs(ctx, tiles),
                     ws<uint64_t>(ctx, at_hash_of), ws<uint32_t>(ctx, at_rep_of), ws<uint32_t>(ctx, at_dense), report);
    return selected_end(ctx, report.epoch, res, &et_group_result::n_groups, d_first_rows, cap_groups, "the group call's report never reached the host",
                        "more groups than cap_groups", "a probe sequence of the group call's table met no slot of its text");
}

// ---- the calls that derive a new packed store from an old one (take, slice, field, concat, recode) ---------------------------
// The head of such a call, behind the null check of what is the call's own: one source against the rows and the output, the checks
// in THIS order.  unaligned4: one of the call's own per-row arrays is not 4-byte aligned.  The texts that differ between the calls:
struct SourceTexts {
    const char *unaligned4, *too_many, *without_rows, *overlap;
};
constexpr const char *ROWS_ARE_RECORDS = "without d_rows, row k is record k: n_rows must be n_records";

int source_args(et_ctx *ctx, const Source &s, size_t n_rows, bool unaligned4, const void *d_out, size_t cap, const uint64_t *d_out_body_index, const uint64_t *d_out_text_index,
                const SourceTexts &t) {
    if (!s.bodies || !s.body_index || !s.text_index) return fail(ctx, ET_ERR_ARG, "null pointer");
    if (misaligned(7, s.body_index, s.text_index, d_out_body_index, d_out_text_index)) return fail(ctx, ET_ERR_ARG, "an offset array is not 8-byte aligned");
    if (unaligned4 || misaligned(3, s.rows)) return fail(ctx, ET_ERR_ARG, t.unaligned4);
    if (s.n > 0x7fffffffu || n_rows > 0x7fffffffu) return fail(ctx, ET_ERR_ARG, t.too_many);
    if (!s.rows && n_rows != s.n) return fail(ctx, ET_ERR_ARG, t.without_rows);
    if (d_out && cap && s.body_bytes) {  // (deriving in place is not these calls')
        const uintptr_t o = reinterpret_cast<uintptr_t>(d_out), b = reinterpret_cast<uintptr_t>(s.bodies);
        if (o < b + s.body_bytes && b < o + cap) return fail(ctx, ET_ERR_ARG, t.overlap);
    }
    return ET_OK;
}

// ... and its tail, behind the launches: the poll (`never`: the call's message), the report into *res; ET_ERR_CAP (`too_much`)
// when d_out was given and the report exceeds cap -- the call's last kernels saw the same two figures.
int derived_end(et_ctx *ctx, uint64_t epoch, et_take_result *res, const void *d_out, uint64_t cap, const char *never, const char *too_much) {
    ET_TRY(packed_poll(ctx, epoch, never));
    const uint64_t *rep = report_words(ctx);
    res->out_bytes = rep[et::PACKED_BYTES];
    res->text_bytes = rep[et::TAKE_TEXT_BYTES];
    read_failures(rep, et::PACKED_N_FAILED, &res->n_failed, &res->first_failed, &res->first_status);
    if (d_out && res->out_bytes > cap) return fail(ctx, ET_ERR_CAP, too_much);
    return ET_OK;
}

extern "C" size_t et_take_result_size(void) { return sizeof(et_take_result); }

extern "C" int et_take_packed_device(et_ctx *ctx, const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index, const uint64_t *d_text_index, size_t n_records,
                                     const uint32_t *d_rows, size_t n_rows, void *d_out, size_t cap, uint64_t *d_out_body_index, uint64_t *d_out_text_index, uint8_t *d_status,
                                     et_take_result *res) {
    if (!ctx) return ET_ERR_ARG;
    if (!res || !d_rows || !d_out_body_index || !d_out_text_index) return fail(ctx, ET_ERR_ARG, "null pointer");
    const Source src{d_bodies, body_bytes, d_body_index, d_text_index, n_records, d_rows};
    ET_TRY(source_args(ctx, src, n_rows, false, d_out, cap, d_out_body_index, d_out_text_index,
                       {"the rows are not 4-byte aligned", "too many records or rows", ROWS_ARE_RECORDS, "d_out overlaps d_bodies"}));
    *res = et_take_result{};
    if (n_rows == 0) return ET_OK;
    DeviceGuard guard(ctx->device);
    ET_TRY(packed_ensure(ctx, PK_SIZES + n_rows * sizeof(et::TakeRow)));
    ET_HIP(hipMemcpyAsync(ws<uint8_t>(ctx, PK_STATS), first_counters(ctx), PK_COUNTER_BYTES, hipMemcpyHostToDevice, ctx->stream));
    const et::PackedReport report = next_report(ctx);
    et::launch_take(ctx->stream, packed_store(src), d_rows, static_cast<uint32_t>(n_rows), d_out, cap, d_out_body_index, d_out_text_index, d_status,
                    ws<et::TakeRow>(ctx, PK_SIZES), report);
    return derived_end(ctx, report.epoch, res, d_out, cap, "the take's report never reached the host", "the taken bodies need more than cap bytes");
}

extern "C" size_t et_slice_lane_bytes(void) { return et::SLICE_LANE_BYTES; }

extern "C" int et_slice_packed_device(et_ctx *ctx, const et_codebook *cb, const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                                      const uint64_t *d_text_index, size_t n_records, const uint32_t *d_rows, size_t n_rows, const uint32_t *d_first, uint32_t first,
                                      const uint32_t *d_count, uint32_t count, int stop, void *d_out, size_t cap, uint64_t *d_out_body_index, uint64_t *d_out_text_index,
                                      uint8_t *d_status, et_take_result *res) {
    if (!ctx) return ET_ERR_ARG;
    if (!cb || !res || !d_out_body_index || !d_out_text_index) return fail(ctx, ET_ERR_ARG, "null pointer");
    const Source src{d_bodies, body_bytes, d_body_index, d_text_index, n_records, d_rows};
    ET_TRY(source_args(ctx, src, n_rows, misaligned(3, d_first, d_count), d_out, cap, d_out_body_index, d_out_text_index,
                       {"the rows, the firsts or the counts are not 4-byte aligned", "too many records or rows", ROWS_ARE_RECORDS, "d_out overlaps d_bodies"}));
    if (stop < ET_SLICE_NO_STOP || stop > 255) return fail(ctx, ET_ERR_ARG, "stop is a byte, or ET_SLICE_NO_STOP");
    *res = et_take_result{};
    if (n_rows == 0) return ET_OK;
    DeviceGuard guard(ctx->device);
    // the sorted codes and the counters' first values, up in one copy; behind them a TakeRow and a list entry per row
    uint32_t n_codes = 0;
    ET_TRY(packed_upload(ctx, cb, false, n_rows * (sizeof(et::TakeRow) / 4 + 1), &n_codes));
    et::SliceJob job{};
    job.rows = d_rows;
    job.d_first = d_first;
    job.d_count = d_count;
    job.n_rows = static_cast<uint32_t>(n_rows);
    job.first = first;
    job.count = count;
    job.stop = stop < 0 ? et::SLICE_NO_STOP : static_cast<uint32_t>(stop);  // (a byte without a code is no symbol of the table: it cuts nothing)
    const et::PackedReport report = next_report(ctx);
    et::launch_slice(ctx->stream, packed_store(src), ws<const uint2>(ctx, 0), n_codes, job, d_out, cap, d_out_body_index, d_out_text_index, d_status,
                     ws<et::TakeRow>(ctx, PK_SIZES), ws<uint32_t>(ctx, PK_SIZES + n_rows * sizeof(et::TakeRow)), report);
    return derived_end(ctx, report.epoch, res, d_out, cap, "the slice's report never reached the host", "the slices need more than cap bytes");
}

extern "C" size_t et_field_lane_bytes(void) { return et::FIELD_LANE_BYTES; }

extern "C" int et_field_packed_device(et_ctx *ctx, const et_codebook *cb, const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                                      const uint64_t *d_text_index, size_t n_records, const uint32_t *d_rows, size_t n_rows, const uint32_t *d_field, uint32_t field,
                                      const uint32_t *d_n_fields, uint32_t n_fields, int delim, void *d_out, size_t cap, uint64_t *d_out_body_index,
                                      uint64_t *d_out_text_index, uint32_t *d_pos, uint8_t *d_status, et_take_result *res) {
    if (!ctx) return ET_ERR_ARG;
    if (!cb || !res || !d_out_body_index || !d_out_text_index) return fail(ctx, ET_ERR_ARG, "null pointer");
    const Source src{d_bodies, body_bytes, d_body_index, d_text_index, n_records, d_rows};
    ET_TRY(source_args(ctx, src, n_rows, misaligned(3, d_field, d_n_fields, d_pos), d_out, cap, d_out_body_index, d_out_text_index,
                       {"the rows, the fields, the field counts or the positions are not 4-byte aligned", "too many records or rows", ROWS_ARE_RECORDS, "d_out overlaps d_bodies"}));
    if (delim < 0 || delim > 255) return fail(ctx, ET_ERR_ARG, "delim is a byte");
    *res = et_take_result{};
    if (n_rows == 0) return ET_OK;
    DeviceGuard guard(ctx->device);
    // the slice's upload and layout: the sorted codes and the counters' first values; behind them a TakeRow and a list entry per row
    uint32_t n_codes = 0;
    ET_TRY(packed_upload(ctx, cb, false, n_rows * (sizeof(et::TakeRow) / 4 + 1), &n_codes));
    et::FieldJob job{};
    job.rows = d_rows;
    job.d_field = d_field;
    job.d_n_fields = d_n_fields;
    job.d_pos = d_pos;
    job.n_rows = static_cast<uint32_t>(n_rows);
    job.field = field;
    job.n_fields = n_fields;
    job.delim = static_cast<uint32_t>(delim);  // (a byte without a code is no symbol of the table: it occurs nowhere)
    const et::PackedReport report = next_report(ctx);
    et::launch_field(ctx->stream, packed_store(src), ws<const uint2>(ctx, 0), n_codes, job, d_out, cap, d_out_body_index, d_out_text_index, d_status,
                     ws<et::TakeRow>(ctx, PK_SIZES), ws<uint32_t>(ctx, PK_SIZES + n_rows * sizeof(et::TakeRow)), report);
    return derived_end(ctx, report.epoch, res, d_out, cap, "the field call's report never reached the host", "the fields need more than cap bytes");
}

extern "C" size_t et_concat_sep_max(void) { return et::CONCAT_SEP_MAX; }

extern "C" size_t et_concat_lane_bytes(void) { return et::CONCAT_LANE_BYTES; }

static_assert(sizeof(et::ConcatPiece) == 32 && et::CONCAT_SEP_MAX * 4 <= et::SEARCH_PATTERN_BYTES && PK_PATTERN + et::SEARCH_PATTERN_BYTES <= PK_SIZES,
              "k_concat_plan stores a ConcatPiece as 2 x 16 bytes; the encoded literal lies between the counters and the plan");

extern "C" int et_concat_packed_device(et_ctx *ctx, const et_codebook *cb, const void *d_a_bodies, size_t a_body_bytes, const uint64_t *d_a_body_index,
                                       const uint64_t *d_a_text_index, size_t n_a, const uint32_t *d_rows_a, const uint8_t *sep, size_t sep_len, const void *d_b_bodies,
                                       size_t b_body_bytes, const uint64_t *d_b_body_index, const uint64_t *d_b_text_index, size_t n_b, const uint32_t *d_rows_b, size_t n_rows,
                                       void *d_out, size_t cap, uint64_t *d_out_body_index, uint64_t *d_out_text_index, uint8_t *d_status, et_take_result *res) {
    if (!ctx) return ET_ERR_ARG;
    if (!cb || !res || !d_out_body_index || !d_out_text_index || (!sep && sep_len)) return fail(ctx, ET_ERR_ARG, "null pointer");
    if (!d_a_bodies && !d_b_bodies) return fail(ctx, ET_ERR_ARG, "both sides are absent");
    const Source sides[2] = {{d_a_bodies, a_body_bytes, d_a_body_index, d_a_text_index, n_a, d_rows_a}, {d_b_bodies, b_body_bytes, d_b_body_index, d_b_text_index, n_b, d_rows_b}};
    if (misaligned(7, d_out_body_index, d_out_text_index)) return fail(ctx, ET_ERR_ARG, "an offset array is not 8-byte aligned");
    if (n_rows > 0x7fffffffu) return fail(ctx, ET_ERR_ARG, "too many rows");
    for (const Source &s : sides) {
        if (!s.bodies) {  // an absent side: no records, no offsets (its rows are not looked at)
            if (s.n || s.body_bytes || s.body_index || s.text_index) return fail(ctx, ET_ERR_ARG, "an absent side has no records, no bytes and no offset arrays");
            continue;
        }
        ET_TRY(source_args(ctx, s, n_rows, false, d_out, cap, d_out_body_index, d_out_text_index,
                           {"the rows are not 4-byte aligned", "too many records", "without d_rows, row k is record k: n_rows must be that side's n", "d_out overlaps a side's bodies"}));
    }
    if (sep_len > et::CONCAT_SEP_MAX) return fail(ctx, ET_ERR_ARG, "the literal is longer than et_concat_sep_max()");
    *res = et_take_result{};
    if (n_rows == 0) return ET_OK;
    ET_TRY(require_complete(ctx, cb));
    uint8_t encoded[et::SEARCH_PATTERN_BYTES];
    uint64_t bits = 0;
    const int rc = et_encode_pattern(cb, sep, sep_len, encoded, sizeof(encoded), &bits);
    if (rc != ET_OK) return fail(ctx, rc, "a byte of the literal has no code");
    DeviceGuard guard(ctx->device);
    // the slice's layout with the side array behind the list; the sorted codes, the counters' first values and the literal's bits lie
    // one behind the other: up in one copy
    Bump layout{PK_SIZES};
    const size_t at_plan = layout.take(n_rows * sizeof(et::TakeRow), 16), at_list = layout.take(n_rows * 4, 4), at_pieces = layout.take(n_rows * sizeof(et::ConcatPiece), 16);
    ET_TRY(packed_ensure(ctx, layout.end));
    const uint32_t n_codes = fill_shared_table(cb, pin<uint32_t>(ctx, PIN_PK_TABLE), false);
    first_counters(ctx);
    const size_t pat_bytes = static_cast<size_t>((bits + 7) / 8), padded = (pat_bytes + 3) & ~static_cast<size_t>(3);
    uint8_t *pattern = pin<uint8_t>(ctx, PIN_PK_PATTERN);
    std::memcpy(pattern, encoded, pat_bytes);
    std::memset(pattern + pat_bytes, 0, padded - pat_bytes);
    ET_HIP(hipMemcpyAsync(ctx->packed_ws.p, pin<uint8_t>(ctx, PIN_PK_TABLE), PK_PATTERN + padded, hipMemcpyHostToDevice, ctx->stream));
    et::ConcatJob job{};
    job.rows_a = d_rows_a;
    job.rows_b = d_rows_b;
    job.sep = ws<const uint8_t>(ctx, PK_PATTERN);
    job.n_rows = static_cast<uint32_t>(n_rows);
    job.sep_bits = static_cast<uint32_t>(bits);
    job.sep_len = static_cast<uint32_t>(sep_len);
    const et::PackedReport report = next_report(ctx);
    et::launch_concat(ctx->stream, packed_store(sides[0]), packed_store(sides[1]), ws<const uint2>(ctx, 0), n_codes, job, d_out, cap, d_out_body_index, d_out_text_index, d_status,
                      ws<et::TakeRow>(ctx, at_plan), ws<uint32_t>(ctx, at_list), ws<et::ConcatPiece>(ctx, at_pieces), report);
    return derived_end(ctx, report.epoch, res, d_out, cap, "the concat's report never reached the host", "the rows need more than cap bytes");
}

extern "C" size_t et_recode_lane_bytes(void) { return et::RECODE_LANE_BYTES; }

static_assert(PK_PATTERN % 16 == 0 && 2048 <= et::MATCH_PATTERN_BYTES, "the recode's output table lies where the match's pattern does, in both blocks");

extern "C" int et_recode_packed_device(et_ctx *ctx, const et_codebook *cb_in, const et_codebook *cb_out, const int16_t *map, const void *d_bodies, size_t body_bytes,
                                       const uint64_t *d_body_index, const uint64_t *d_text_index, size_t n_records, const uint32_t *d_rows, size_t n_rows, void *d_out,
                                       size_t cap, uint64_t *d_out_body_index, uint64_t *d_out_text_index, uint8_t *d_status, et_take_result *res) {
    if (!ctx) return ET_ERR_ARG;
    if (!cb_in || !cb_out || !res || !d_out_body_index || !d_out_text_index) return fail(ctx, ET_ERR_ARG, "null pointer");
    const Source src{d_bodies, body_bytes, d_body_index, d_text_index, n_records, d_rows};
    ET_TRY(source_args(ctx, src, n_rows, false, d_out, cap, d_out_body_index, d_out_text_index,
                       {"the rows are not 4-byte aligned", "too many records or rows", ROWS_ARE_RECORDS, "d_out overlaps d_bodies"}));
    if (map)
        for (int s = 0; s < 256; ++s)
            if (map[s] < ET_RECODE_DROP || map[s] > 255) return fail(ctx, ET_ERR_ARG, "a map entry is a byte, or ET_RECODE_DROP");
    *res = et_take_result{};
    if (n_rows == 0) return ET_OK;
    ET_TRY(require_complete(ctx, cb_in));
    ET_TRY(require_complete(ctx, cb_out));
    DeviceGuard guard(ctx->device);
    // the slice's layout behind the output table; the sorted codes of cb_in, the counters' first values and the output table lie one
    // behind the other: up in one copy
    Bump layout{PK_PATTERN + 2048};
    const size_t at_plan = layout.take(n_rows * sizeof(et::TakeRow), 16), at_list = layout.take(n_rows * 4, 4);
    ET_TRY(packed_ensure(ctx, layout.end));
    const uint32_t n_codes = fill_shared_table(cb_in, pin<uint32_t>(ctx, PIN_PK_TABLE), false);
    first_counters(ctx);
    // the map composed with cb_out, by the INPUT symbol: the device looks one entry up per symbol and knows neither
    uint32_t *out_tab = pin<uint32_t>(ctx, PIN_PK_PATTERN);
    for (int s = 0; s < 256; ++s) {
        const int to = map ? map[s] : s;
        const uint32_t len = to < 0 ? 0u : cb_out->length[to];
        out_tab[2 * s] = len ? et_left_aligned(cb_out->data[to], len) : 0u;
        out_tab[2 * s + 1] = to < 0 ? 0u : len ? len : et::RECODE_UNCODED;
    }
    ET_HIP(hipMemcpyAsync(ctx->packed_ws.p, pin<uint8_t>(ctx, PIN_PK_TABLE), PK_PATTERN + 2048, hipMemcpyHostToDevice, ctx->stream));
    et::RecodeJob job{};
    job.rows = d_rows;
    job.out_tab = ws<const uint2>(ctx, PK_PATTERN);
    job.n_rows = static_cast<uint32_t>(n_rows);
    const et::PackedReport report = next_report(ctx);
    et::launch_recode(ctx->stream, packed_store(src), ws<const uint2>(ctx, 0), n_codes, job, d_out, cap, d_out_body_index, d_out_text_index, d_status,
                      ws<et::TakeRow>(ctx, at_plan), ws<uint32_t>(ctx, at_list), report);
    return derived_end(ctx, report.epoch, res, d_out, cap, "the recode's report never reached the host", "the recoded rows need more than cap bytes");
}

extern "C" size_t et_number_result_size(void) { return sizeof(et_number_result); }

extern "C" size_t et_number_symbols_max(void) { return et::NUMBER_SYMBOLS_MAX; }

extern "C" size_t et_number_lane_bytes(void) { return et::NUMBER_LANE_BYTES; }

static_assert(int(et::NUMBER_OK) == ET_NUMBER_OK && int(et::NUMBER_EMPTY) == ET_NUMBER_EMPTY && int(et::NUMBER_BAD) == ET_NUMBER_BAD && int(et::NUMBER_RANGE) == ET_NUMBER_RANGE,
              "a row's kind byte is its ET_NUMBER_*");
static_assert(sizeof(et::NumberRow) == 16 && sizeof(et_number_result) == 56 && int(et::NUMBER_N_RANGE) < int(et::PACKED_WORDS) && int(et::NUMBER_N_EMPTY) > int(et::SLICE_N_LONG),
              "k_number_plan stores a NumberRow as 16 bytes; the kinds' counters lie in the free words behind the list's");

extern "C" int et_number_packed_device(et_ctx *ctx, const et_codebook *cb, const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                                       const uint64_t *d_text_index, size_t n_records, const uint32_t *d_rows, size_t n_rows, const uint32_t *d_first, uint32_t first,
                                       const uint32_t *d_count, uint32_t count, int stop, int64_t *d_values, uint8_t *d_kind, const uint32_t *d_group_of, size_t n_groups,
                                       int64_t *d_sum, uint64_t *d_n, int64_t *d_min, int64_t *d_max, uint8_t *d_status, et_number_result *res) {
    if (!ctx) return ET_ERR_ARG;
    if (!cb || !res) return fail(ctx, ET_ERR_ARG, "null pointer");
    const Source src{d_bodies, body_bytes, d_body_index, d_text_index, n_records, d_rows};
    ET_TRY(source_args(ctx, src, n_rows, misaligned(3, d_first, d_count), nullptr, 0, nullptr, nullptr,
                       {"the rows, the firsts or the counts are not 4-byte aligned", "too many records or rows", ROWS_ARE_RECORDS, ""}));
    if (stop < ET_SLICE_NO_STOP || stop > 255) return fail(ctx, ET_ERR_ARG, "stop is a byte, or ET_SLICE_NO_STOP");
    const bool aggregates = d_sum || d_n || d_min || d_max;
    if (misaligned(7, d_values, d_sum, d_n, d_min, d_max)) return fail(ctx, ET_ERR_ARG, "the values or an aggregate array are not 8-byte aligned");
    if (misaligned(3, d_group_of)) return fail(ctx, ET_ERR_ARG, "the group numbers are not 4-byte aligned");
    if (d_group_of && !aggregates) return fail(ctx, ET_ERR_ARG, "group numbers without an aggregate output");
    if (aggregates && n_groups == 0) return fail(ctx, ET_ERR_ARG, "an aggregate output without a group");
    if (n_groups > 0x7fffffffu) return fail(ctx, ET_ERR_ARG, "too many groups");
    if (aggregates && !d_group_of && n_groups != 1) return fail(ctx, ET_ERR_ARG, "without d_group_of every row is in group 0: n_groups must be 1");
    *res = et_number_result{};
    if (n_rows == 0) return ET_OK;
    DeviceGuard guard(ctx->device);
    // the slice's upload -- the sorted codes and the counters' first values in one copy -- and its layout: behind them a NumberRow
    // and a list entry per row
    uint32_t n_codes = 0;
    ET_TRY(packed_upload(ctx, cb, false, n_rows * (sizeof(et::NumberRow) / 4 + 1), &n_codes));
    // the aggregates' first values where a byte pattern gives them; launch_number fills min and max
    if (d_sum) ET_HIP(hipMemsetAsync(d_sum, 0, n_groups * 8, ctx->stream));
    if (d_n) ET_HIP(hipMemsetAsync(d_n, 0, n_groups * 8, ctx->stream));
    et::NumberJob job{};
    job.ask.rows = d_rows;
    job.ask.d_first = d_first;
    job.ask.d_count = d_count;
    job.ask.n_rows = static_cast<uint32_t>(n_rows);
    job.ask.first = first;
    job.ask.count = count;
    job.ask.stop = stop < 0 ? et::SLICE_NO_STOP : static_cast<uint32_t>(stop);  // (a byte without a code is no symbol of the table: it cuts nothing)
    job.d_values = d_values;
    job.d_kind = d_kind;
    job.group_of = d_group_of;
    job.n_groups = aggregates ? static_cast<uint32_t>(n_groups) : 0u;
    job.d_sum = d_sum;
    job.d_n = reinterpret_cast<unsigned long long *>(d_n);
    job.d_min = d_min;
    job.d_max = d_max;
    const et::PackedReport report = next_report(ctx);
    et::launch_number(ctx->stream, packed_store(src), ws<const uint2>(ctx, 0), n_codes, job, d_status, ws<et::NumberRow>(ctx, PK_SIZES),
                      ws<uint32_t>(ctx, PK_SIZES + n_rows * sizeof(et::NumberRow)), report);
    ET_TRY(packed_poll(ctx, report.epoch, "the number call's report never reached the host"));
    const uint64_t *rep = report_words(ctx);
    res->n_empty = rep[et::NUMBER_N_EMPTY];
    res->n_bad = rep[et::NUMBER_N_BAD];
    res->n_range = rep[et::NUMBER_N_RANGE];
    read_failures(rep, et::PACKED_N_FAILED, &res->n_failed, &res->first_failed, &res->first_status);
    res->n_ok = n_rows - res->n_empty - res->n_bad - res->n_range - res->n_failed;
    return ET_OK;
}


extern "C" int et_selftest_join_hash(et_ctx *ctx, const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index, const uint64_t *d_text_index, size_t n,
                                     uint64_t *d_hash) {
    if (!ctx) return ET_ERR_ARG;
    if (!d_bodies || !d_body_index || !d_text_index || !d_hash) return fail(ctx, ET_ERR_ARG, "null pointer");
    if (misaligned(7, d_body_index, d_text_index, d_hash)) return fail(ctx, ET_ERR_ARG, "an array is not 8-byte aligned");
    if (n > 0x7fffffffu) return fail(ctx, ET_ERR_ARG, "too many records");
    if (n == 0) return ET_OK;
    DeviceGuard guard(ctx->device);
    et::launch_join_hash(ctx->stream, et::PackedStore{d_bodies, body_bytes, d_body_index, d_text_index, static_cast<uint32_t>(n), 0}, d_hash);
    ET_HIP(hipGetLastError());
    ET_HIP(hipStreamSynchronize(ctx->stream));
    return ET_OK;
}

extern "C" int et_encode_batch_device(et_ctx *ctx, const void *d_in, void *d_out, et_batch_item *items, size_t n_items) {
    ET_TRY(check_call(ctx, d_in, d_out, items, n_items));
    if (n_items == 0) return ET_OK;
    DeviceGuard guard(ctx->device);
    const uint8_t *in = static_cast<const uint8_t *>(d_in);
    uint8_t *out = static_cast<uint8_t *>(d_out);

    std::vector<uint32_t> small, large;  // by the batch kernels; by et_encode_device
    for (size_t i = 0; i < n_items; ++i) {
        et_batch_item &it = items[i];
        if (it.in_len == 0) it.status = ET_ERR_EMPTY;
        else if (reinterpret_cast<uintptr_t>(out + it.out_off) & 15) it.status = ET_ERR_ARG;
        else if (it.out_cap < et_encode_bound(it.in_len)) it.status = ET_ERR_CAP;
        else (it.in_len > et::BATCH_SMALL_MAX ? large : small).push_back(static_cast<uint32_t>(i));
    }
    if (!small.empty()) ET_TRY(ensure_batch(ctx, small.size(), et::BATCH_ENC_SLOT));

    for (size_t c0 = 0; c0 < small.size(); c0 += CH) {
        const uint32_t n = static_cast<uint32_t>(std::min(CH, small.size() - c0));
        et::BatchSpan *spans = pin<et::BatchSpan>(ctx, PIN_SPANS);
        for (uint32_t j = 0; j < n; ++j) {
            const et_batch_item &it = items[small[c0 + j]];
            spans[j] = et::BatchSpan{it.in_off, static_cast<uint32_t>(it.in_len), 0};
        }
        uint8_t *d_rec = static_cast<uint8_t *>(ctx->batch_jobs.p);
        ET_HIP(hipMemcpyAsync(d_rec, spans, n * sizeof(et::BatchSpan), hipMemcpyHostToDevice, ctx->stream));
        const uint64_t epoch = ++ctx->batch_epoch;
        et::launch_batch_hist(ctx->stream, in, reinterpret_cast<const et::BatchSpan *>(d_rec), n, pin<uint32_t>(ctx, PIN_REPORT),
                              static_cast<uint32_t *>(ctx->batch_counter.p), epoch_word_dev(ctx, 0), epoch);
        ET_HIP(hipGetLastError());
        ET_TRY(wait_for_word<uint64_t>(ctx, epoch_word(ctx, 0), epoch, 200.0, "the batch's histograms never reached the host"));

        // per stream: encode.zig:54-299 on the host, as et_encode_device does it
        et::BatchEncJob *jobs = pin<et::BatchEncJob>(ctx, PIN_JOBS);
        uint8_t *blob = pin<uint8_t>(ctx, PIN_BLOB);
        const uint32_t *counts = pin<uint32_t>(ctx, PIN_REPORT);
        uint32_t n_jobs = 0, blob_len = 0;
        for (uint32_t j = 0; j < n; ++j) {
            et_batch_item &it = items[small[c0 + j]];
            uint64_t hist[256];
            for (int s = 0; s < 256; ++s) hist[s] = counts[static_cast<size_t>(j) * 256 + s];
            et_codebook cb;
            int rc = et_build_codebook(hist, &cb);
            if (rc != ET_OK) {
                it.status = rc;
                continue;
            }
            if (cb.max_length > 32) {  // (the reference's u32 truncation, quirk Q3: k_encode_tiles_long implements it)
                large.push_back(small[c0 + j]);
                continue;
            }
            uint8_t *slot = blob + blob_len;
            fill_shared_table(&cb, reinterpret_cast<uint32_t *>(slot), true);
            size_t header_len = 0;
            rc = et_write_header(&cb, it.in_len, slot + 2048, et::BATCH_HEADER_PAD - 8, &header_len);
            if (rc != ET_OK) {
                it.status = rc;
                continue;
            }
            const uint32_t padded = static_cast<uint32_t>((header_len + 15) & ~static_cast<size_t>(15));
            std::memset(slot + 2048 + header_len, 0, padded - header_len);
            uint64_t bits = 0;
            et_codebook_bits(&cb, hist, &bits);
            it.out_len = header_len + (bits + 7) / 8;  // encode.zig:318,336
            jobs[n_jobs++] = et::BatchEncJob{it.in_off, it.out_off, static_cast<uint32_t>(it.in_len), static_cast<uint32_t>(header_len), blob_len, 0};
            blob_len += 2048 + padded;
        }
        if (!n_jobs) continue;
        ET_HIP(hipMemcpyAsync(d_rec + DEV_JOBS, jobs, n_jobs * sizeof(et::BatchEncJob), hipMemcpyHostToDevice, ctx->stream));
        ET_HIP(hipMemcpyAsync(ctx->batch_blob.p, blob, blob_len, hipMemcpyHostToDevice, ctx->stream));
        et::launch_batch_encode(ctx->stream, in, out, reinterpret_cast<const et::BatchEncJob *>(d_rec + DEV_JOBS), n_jobs,
                                static_cast<const uint8_t *>(ctx->batch_blob.p));
        ET_HIP(hipGetLastError());
    }

    std::sort(large.begin(), large.end());
    for (uint32_t i : large) {
        et_batch_item &it = items[i];
        size_t len = 0;
        const int rc = et_encode_device(ctx, in + it.in_off, it.in_len, out + it.out_off, it.out_cap, &len);
        it.path = 1;
        it.status = rc;
        it.out_len = rc == ET_OK ? len : 0;
        if (call_level(rc)) return rc;
    }
    return ET_OK;
}

extern "C" int et_decode_batch_device(et_ctx *ctx, const void *d_in, void *d_out, et_batch_item *items, size_t n_items) {
    ET_TRY(check_call(ctx, d_in, d_out, items, n_items));
    if (n_items == 0) return ET_OK;
    DeviceGuard guard(ctx->device);
    const uint8_t *in = static_cast<const uint8_t *>(d_in);
    uint8_t *out = static_cast<uint8_t *>(d_out);

    std::vector<uint32_t> cand, large;
    for (size_t i = 0; i < n_items; ++i) {
        et_batch_item &it = items[i];
        if (it.in_len < 5) it.status = ET_ERR_FORMAT;  // (as et_decode_device: shorter than its header)
        else cand.push_back(static_cast<uint32_t>(i));
    }
    if (!cand.empty()) ET_TRY(ensure_batch(ctx, cand.size(), et::BATCH_DEC_SLOT));

    std::vector<uint32_t> of_job(CH);
    for (size_t c0 = 0; c0 < cand.size(); c0 += CH) {
        const uint32_t n = static_cast<uint32_t>(std::min(CH, cand.size() - c0));
        et::BatchSpan *spans = pin<et::BatchSpan>(ctx, PIN_SPANS);
        for (uint32_t j = 0; j < n; ++j) {
            const et_batch_item &it = items[cand[c0 + j]];
            spans[j] = et::BatchSpan{it.in_off, static_cast<uint32_t>(std::min<uint64_t>(it.in_len, et::BATCH_HEAD_STRIDE)), 0};
        }
        uint8_t *d_rec = static_cast<uint8_t *>(ctx->batch_jobs.p);
        ET_HIP(hipMemcpyAsync(d_rec, spans, n * sizeof(et::BatchSpan), hipMemcpyHostToDevice, ctx->stream));
        uint64_t epoch = ++ctx->batch_epoch;
        et::launch_batch_heads(ctx->stream, in, reinterpret_cast<const et::BatchSpan *>(d_rec), n, pin<uint32_t>(ctx, PIN_REPORT),
                               static_cast<uint32_t *>(ctx->batch_counter.p), epoch_word_dev(ctx, 1), epoch);
        ET_HIP(hipGetLastError());
        ET_TRY(wait_for_word<uint64_t>(ctx, epoch_word(ctx, 1), epoch, 200.0, "the batch's headers never reached the host"));

        // per stream: decode.zig:34-141 on the host (et_parse_header validates), the codes sorted for k_batch_decode
        et::BatchDecJob *jobs = pin<et::BatchDecJob>(ctx, PIN_JOBS);
        uint8_t *blob = pin<uint8_t>(ctx, PIN_BLOB);
        uint32_t n_jobs = 0, blob_len = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t i = cand[c0 + j];
            et_batch_item &it = items[i];
            const uint8_t *head = pin<uint8_t>(ctx, PIN_REPORT) + static_cast<size_t>(j) * et::BATCH_HEAD_STRIDE;
            const size_t sent = static_cast<size_t>(std::min<uint64_t>(it.in_len, et::header_bound(head[0])));
            et_codebook cb;
            uint64_t n_symbols = 0;
            size_t body_offset = 0;
            const int rc = et_parse_header(head, sent, &cb, &n_symbols, &body_offset);
            if (rc != ET_OK) {
                it.status = rc;
                continue;
            }
            if (body_offset > it.in_len) {
                it.status = ET_ERR_FORMAT;
                continue;
            }
            const uint64_t body_bytes = it.in_len - body_offset;
            if (n_symbols == 0 || body_bytes == 0 || cb.n_coded == 0) continue;  // decodes to nothing (a lone symbol's bare header: Q2)
            // a full tree: the prefix-free codes (et_parse_header) cover every 32-bit window
            uint64_t covered = 0;
            for (int s = 0; s < 256; ++s)
                if (cb.length[s]) covered += 1ull << (32 - cb.length[s]);
            if (n_symbols > et::BATCH_SMALL_MAX || covered != (1ull << 32)) {
                large.push_back(i);
                continue;
            }
            struct Code { uint32_t lo, meta; };
            Code *codes = reinterpret_cast<Code *>(blob + blob_len);
            uint32_t k = 0;
            for (int s = 0; s < 256; ++s)
                if (cb.length[s]) codes[k++] = Code{cb.length[s] == 32 ? cb.data[s] : cb.data[s] << (32 - cb.length[s]), static_cast<uint32_t>(cb.length[s]) << 8 | static_cast<uint32_t>(s)};
            std::sort(codes, codes + k, [](const Code &a, const Code &b) { return a.lo < b.lo; });
            // (n_symbols codewords of at most 32 bits end within 4 n_symbols bytes: the kernel's bit positions stay small)
            const uint32_t clipped = static_cast<uint32_t>(std::min<uint64_t>(body_bytes, n_symbols * 4 + 8));
            jobs[n_jobs] = et::BatchDecJob{it.in_off + body_offset, it.out_off, clipped, static_cast<uint32_t>(n_symbols),
                                           static_cast<uint32_t>(std::min<uint64_t>(it.out_cap, n_symbols)), k, blob_len, 0};
            of_job[n_jobs++] = i;
            blob_len += (k * 8 + 15) & ~15u;
        }
        if (!n_jobs) continue;
        ET_HIP(hipMemcpyAsync(d_rec + DEV_JOBS, jobs, n_jobs * sizeof(et::BatchDecJob), hipMemcpyHostToDevice, ctx->stream));
        ET_HIP(hipMemcpyAsync(ctx->batch_blob.p, blob, blob_len, hipMemcpyHostToDevice, ctx->stream));
        epoch = ++ctx->batch_epoch;
        et::launch_batch_decode(ctx->stream, in, out, reinterpret_cast<const et::BatchDecJob *>(d_rec + DEV_JOBS), n_jobs,
                                static_cast<const uint8_t *>(ctx->batch_blob.p), pin<uint32_t>(ctx, PIN_TOTALS), static_cast<uint32_t *>(ctx->batch_counter.p),
                                epoch_word_dev(ctx, 2), epoch);
        ET_HIP(hipGetLastError());
        // a truncated body's length is only known to the kernel: the totals come back the way the scan report of a single decode does
        ET_TRY(wait_for_word<uint64_t>(ctx, epoch_word(ctx, 2), epoch, 2000.0, "the batch's symbol totals never reached the host"));
        const uint32_t *totals = pin<uint32_t>(ctx, PIN_TOTALS);
        for (uint32_t j = 0; j < n_jobs; ++j) {
            et_batch_item &it = items[of_job[j]];
            if (totals[j] > it.out_cap) it.status = ET_ERR_CAP;
            else it.out_len = totals[j];
        }
    }

    std::sort(large.begin(), large.end());
    for (uint32_t i : large) {
        et_batch_item &it = items[i];
        size_t len = 0;
        const int rc = et_decode_device(ctx, in + it.in_off, it.in_len, out + it.out_off, it.out_cap, &len);
        it.path = 1;
        it.status = rc;
        it.out_len = rc == ET_OK ? len : 0;
        if (call_level(rc)) return rc;
    }
    return ET_OK;
}
