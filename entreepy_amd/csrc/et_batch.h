// et_batch.h -- geometry, job records and launch wrappers of et_batch.hip: many small streams in one call, ONE workgroup
// per stream from its first byte to its last (et_encode_batch_device / et_decode_batch_device, host side et_batch.cpp).
// Nothing here is shared with the single-stream kernels; streams these kernels are not made for go to those, whole.
// The shared-table calls (et_encode_shared_device / et_decode_shared_device) have the same shape -- one workgroup per
// stream -- but ONE code table for the whole batch, set up once per workgroup: SharedJob and its two launches below.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace et {

// The longest text the batch kernels take themselves.  A workgroup packs ~4 KiB per round and decodes 8 KiB of bitstream per
// block, one after the other: a stream of this size keeps its workgroup for a few hundred rounds, which is about what the
// five-launch single-stream call costs for the same bytes; beyond it the large path is the faster one.
constexpr size_t BATCH_SMALL_MAX = 256u << 10;
constexpr uint32_t BATCH_CHUNK = 1024;          // streams per pair of launches (bounds the pinned blocks)
constexpr uint32_t BATCH_HEAD_STRIDE = 1544;    // header_bound(255): bytes of pinned memory per stream for k_batch_heads
constexpr uint32_t BATCH_HEADER_PAD = 4640;     // the longest file header (4631 bytes), padded to 16
constexpr uint32_t BATCH_ENC_SLOT = 2048 + BATCH_HEADER_PAD;  // most a stream takes of the encode block: code table + header
constexpr uint32_t BATCH_DEC_SLOT = 2048;       // ... of the decode block: 256 x {left-aligned code, length << 8 | symbol}
constexpr uint32_t BATCH_LUT_BITS = 11;         // k_batch_decode's first-level table
constexpr uint32_t BATCH_STAGE_BYTES = 16384;   // k_batch_decode: symbols staged in LDS per flush

struct BatchSpan {  // k_batch_hist / k_batch_heads: stream j reads d_in[in_off, in_off + in_len)
    uint64_t in_off;
    uint32_t in_len, pad;
};

struct BatchEncJob {
    uint64_t in_off, out_off;  // text at d_in + in_off, image at d_out + out_off (16-byte aligned address)
    uint32_t in_len;
    uint32_t header_len;       // bytes of file header in front of the body
    uint32_t blob_off;         // where in the uploaded block: 256 x {left-aligned code, length}, then the header padded to 16
    uint32_t pad;
};

struct BatchDecJob {
    uint64_t body_off, out_off;  // body at d_in + body_off (any alignment), symbols to d_out + out_off (any alignment)
    uint32_t body_bytes;         // (clipped by the host to what n_symbols codewords can span)
    uint32_t n_symbols;          // stop after this many
    uint32_t write_cap;          // ... but store only the first write_cap of them
    uint32_t n_codes;            // entries of the sorted code list at blob_off
    uint32_t blob_off;
    uint32_t pad;
};

// et_encode_shared_device / et_decode_shared_device: a body alone, under the call's one table.
struct SharedJob {
    uint64_t in_off, out_off;  // any alignment, both
    uint32_t in_len;           // encode: text bytes; decode: body bytes (clipped like BatchDecJob's)
    uint32_t cap;              // encode: bytes the body may take (0xffffffff: no limit); decode: symbols to decode
};
// Streams per launch and hand-over of the shared-table calls (a stream costs 24 + 8 bytes of pinned memory here, not a
// table), and the grids: what is resident at once on 256 CUs (8 and 4 workgroups per CU by LDS), so that a workgroup's
// tables serve several streams of a full chunk.
constexpr uint32_t SHARED_CHUNK = 4096;
constexpr uint32_t SHARED_ENC_GRID = 2048, SHARED_DEC_GRID = 1024;
// What k_shared_encode reports per stream beside its length (the host turns it into an et_status).
enum SharedStatus : uint32_t { SHARED_OK = 0, SHARED_UNCODED = 1, SHARED_CAP = 2 };

// counter: one device word, zero between launches (the last workgroup to finish resets it and stores `epoch` into the
// pinned *host_done, which the host polls).
void launch_batch_hist(hipStream_t stream, const void *d_in, const BatchSpan *spans, uint32_t n, uint32_t *host_hist, uint32_t *counter,
                       unsigned long long *host_done, unsigned long long epoch);
void launch_batch_encode(hipStream_t stream, const void *d_in, void *d_out, const BatchEncJob *jobs, uint32_t n, const uint8_t *blob);
void launch_batch_heads(hipStream_t stream, const void *d_in, const BatchSpan *spans, uint32_t n, uint32_t *host_heads, uint32_t *counter,
                        unsigned long long *host_done, unsigned long long epoch);
void launch_batch_decode(hipStream_t stream, const void *d_in, void *d_out, const BatchDecJob *jobs, uint32_t n, const uint8_t *blob,
                         uint32_t *host_totals, uint32_t *counter, unsigned long long *host_done, unsigned long long epoch);

// table: 256 x {left-aligned code, length} on the device.  d_out == nullptr: sizes only.  host_results (pinned): per stream
// {body bytes (0 unless SHARED_OK), SharedStatus}.
void launch_shared_encode(hipStream_t stream, const void *d_in, void *d_out, const SharedJob *jobs, uint32_t n, const uint2 *table,
                          uint2 *host_results, uint32_t *counter, unsigned long long *host_done, unsigned long long epoch);
// codes: the n_codes codes of a full prefix-free tree sorted by left-aligned value, {code, length << 8 | symbol}, on the device.
// host_results (pinned): per stream {symbols written, 0}.
void launch_shared_decode(hipStream_t stream, const void *d_in, void *d_out, const SharedJob *jobs, uint32_t n, const uint2 *codes,
                          uint32_t n_codes, uint2 *host_results, uint32_t *counter, unsigned long long *host_done, unsigned long long epoch);

// The packed calls: the shared-table kernels with their jobs read from u64 offset arrays on the device.  What a record's status
// byte holds is its et_status itself (et_batch.cpp asserts the values).
enum PackedStatus : uint32_t { PACKED_OK = 0, PACKED_ARG = 6, PACKED_UNSUPPORTED = 7 };
// The words of the counters in device memory (`stats`; the host uploads {0, ~0, 0} in front of a call) and of the report in
// pinned memory (`host_result`): PACKED_FIRST = the lowest failed record << 8 | its status.
enum PackedWord { PACKED_BYTES = 0, PACKED_N_FAILED = 1, PACKED_FIRST = 2, PACKED_N_SHORT = 3, PACKED_WORDS = 8 };
constexpr uint32_t PACKED_SCAN_TILE = 4096;  // records per trip of k_packed_scan's one workgroup

struct PackedStore {  // a packed store on the device: record j is bodies[body_index[j], body_index[j + 1]), text_index[j + 1] - text_index[j] symbols
    const void *bodies;
    uint64_t body_bytes;
    const uint64_t *body_index, *text_index;
    uint32_t n, pad;
};
// Where a call's counters lie and where its report goes: `stats` on the device (PackedWord), host_result and host_done pinned; the
// kernel that reports stores host_result, then `epoch` into *host_done.
struct PackedReport {
    unsigned long long *stats, *host_result, *host_done;
    unsigned long long epoch;
};
// count codewords of at most 32 bits end within 4 count bytes: what of a body of `bytes` the decode kernels look at, so that
// decode_stream's bit positions stay small.
constexpr uint64_t clip_body(uint64_t bytes, uint64_t count) { return bytes < count * 4 + 8 ? bytes : count * 4 + 8; }

// The encode (et_encode_packed_device): k_packed_count, k_packed_scan and -- unless d_out is null: sizes only -- k_packed_pack, in
// stream order.  table: 256 x {left-aligned code, length} on the device; sizes: n words of workspace.  The report leaves with the
// scan, in front of the pack.
void launch_packed_encode(hipStream_t stream, const void *d_text, uint64_t text_bytes, const uint64_t *text_index, uint32_t n, void *d_out, uint64_t cap,
                          uint64_t *out_index, uint8_t *d_status, const uint2 *table, uint32_t *sizes, const PackedReport &report);
// The decode (et_decode_packed_device): k_packed_decode.  codes as launch_shared_decode's; counter as above.
void launch_packed_decode(hipStream_t stream, const PackedStore &store, void *d_out, uint64_t cap, const uint2 *codes, uint32_t n_codes, uint32_t *d_written,
                          uint8_t *d_status, const PackedReport &report, uint32_t *counter);
// The gather (et_decode_packed_gather_device): k_gather_plan (one lane per row: the room of record rows[k], or none and why, into
// `sizes`, n_rows words of workspace, and d_status), k_packed_scan (sizes -> out_index) and -- unless d_out is null: sizes only --
// k_packed_gather (k_packed_decode's loop over the rows), in stream order.  The report leaves with the last of them: with the
// decode, which alone knows the short rows, or with the scan of a sizes-only call.
constexpr uint32_t GATHER_PLAN_GRID = 1024;  // workgroups of k_gather_plan at most: a row per lane and trip
void launch_packed_gather(hipStream_t stream, const PackedStore &store, const uint32_t *rows, uint32_t n_rows, void *d_out, uint64_t cap, uint64_t *out_index,
                          const uint2 *codes, uint32_t n_codes, uint32_t *d_written, uint8_t *d_status, uint32_t *sizes, const PackedReport &report, uint32_t *counter);

// The match (et_match_packed_device): which records of a packed store begin with, or equal, a needle -- judged on the compressed
// bytes, against the needle's own bits under the table (et_encode_pattern, on the host); no table on the device.
//   k_match_flag   one record per lane, tiles of MATCH_TILE records: the record judged, its status byte, the first MATCH_HEAD_BITS
//                  bits of the pattern compared per lane, the rest by the whole wavefront for one surviving lane at a time; a u64
//                  ballot mask per 64 records and a u32 count per tile into the workspace
//   k_packed_scan  the tile counts -> the tiles' first places in d_rows, n_match; its report is the call's
//   k_rows_emit    (unless d_rows is null: count only) per tile, a record's rank is a popcount prefix over the tile's masks
constexpr uint32_t MATCH_HEAD_BITS = 64;                      // what a lane compares alone: one aligned 8-byte load, or two
constexpr uint32_t MATCH_TILE = 256;                          // records per tile: one trip of a workgroup
constexpr uint32_t MATCH_GRID = 2048;                         // workgroups of k_match_flag and k_rows_emit at most
constexpr uint32_t MATCH_NEEDLE_MAX = 4096;                   // bytes of text in a needle
constexpr uint32_t MATCH_PATTERN_BYTES = MATCH_NEEDLE_MAX * 4;  // ... which take at most 32 bits each
enum MatchFlag : uint32_t { MATCH_F_EQUAL = 1, MATCH_F_NOT = 2, MATCH_F_NEVER = 4 };  // NEVER: a needle byte without a code
struct MatchJob {
    uint64_t head, head_mask;  // the pattern's first min(8, bytes) bytes as they lie in memory, and which of their bits count
    uint32_t pat_bits;         // bits of the encoded needle
    uint32_t needle_len;       // its bytes of text
    uint32_t flags;            // MatchFlag
    uint32_t pad;
};
struct TileWs {  // the tile workspace of the match and the join
    unsigned long long *masks;  // 4 u64 per tile: a ballot per 64 records
    uint32_t *counts;           // a u32 per tile (16-byte aligned)
    uint64_t *base;             // tiles + 1 u64: k_packed_scan's out_index
};
// pattern: the encoded needle on the device, zero-padded to a multiple of 4 bytes (4-byte aligned).  The report ({n_match, failed,
// first << 8 | status}, then `epoch`) leaves with the scan, in front of k_rows_emit.
void launch_match(hipStream_t stream, const PackedStore &store, const uint32_t *pattern, const MatchJob &job, uint32_t *d_rows, uint64_t cap_rows, uint8_t *d_status,
                  const TileWs &tiles, const PackedReport &report);

// The order modes of the match (ET_MATCH_LESS, ET_MATCH_LESS_EQUAL): which records' stored text lies below the needle, or at it, as
// unsigned bytes -- judged on the compressed bytes.  A Huffman code does not keep the order of its symbols, but record and needle are
// parsed by the same prefix-free code: the first BIT at which body and encoded needle differ lies inside the codeword of the first
// SYMBOL at which the texts differ, and the host knows where the needle's codewords begin.  So a record costs its first differing
// bit, one binary search among the needle's boundaries, ONE codeword decoded from the body there, and one byte comparison.
//   k_order_flag   k_match_flag's frame (tiles, judgement, status bytes, tally, masks, counts) with the sorted codes in LDS: the
//                  first MATCH_HEAD_BITS compared per lane, a longer common stretch by the whole wavefront for one lane at a time,
//                  leaving at the first step with a difference; then per lane the boundary (`starts`, global memory), the codeword
//                  (search_codes) and the comparison
//   k_packed_scan, k_rows_emit   the match's, unchanged
// `starts` (u32[n_coded + 1], strictly increasing): entry i = (the bit at which the needle's codeword i begins) << 8 | needle[i];
// entry n_coded = pat_bits << 8 | the needle's first byte without a code (0 when every byte has one).  n_coded is the number of
// leading needle bytes with a code; pattern and pat_bits are those bytes' alone.
enum OrderFlag : uint32_t { ORDER_F_EQUAL_TOO = 1, ORDER_F_TAIL = 4 };  // LESS_EQUAL; a needle byte without a code follows (beside MATCH_F_NOT)
struct OrderJob {
    uint64_t head;        // the pattern's first 64 bits, the first at the top, zero behind pat_bits
    uint32_t pat_bits;    // bits of the encoded codable prefix
    uint32_t n_coded;     // its bytes of text (K)
    uint32_t needle_len;  // the whole needle's (for the record: the kernel decides by n_coded and ORDER_F_TAIL and does not read it)
    uint32_t flags;       // OrderFlag | MATCH_F_NOT
};
// codes: the sorted codes on the device (launch_shared_decode's); pattern: as launch_match's; starts: 4-byte aligned.
void launch_order(hipStream_t stream, const PackedStore &store, const uint2 *codes, uint32_t n_codes, const uint32_t *pattern, const uint32_t *starts, const OrderJob &job,
                  uint32_t *d_rows, uint64_t cap_rows, uint8_t *d_status, const TileWs &tiles, const PackedReport &report);

// The search (et_search_packed_device): which records of a packed store CONTAIN, or END WITH, a needle, and where -- judged on the
// compressed bytes by a walk over the codeword boundaries with nothing written: the needle occurs at symbol i exactly when its bits
// (et_encode_pattern) lie at the bit where codeword i begins, end inside the body, and i + needle_len <= length.
//   k_search_flag  one record per lane, tiles of MATCH_TILE records, the sorted codes, the first-level table and the pattern in LDS:
//                  judged, its status byte; a body of up to SEARCH_LANE_BYTES is walked by its lane alone, from global memory; a
//                  longer one that can hold the needle goes onto a list in the workspace and counts as "no occurrence" for now; a
//                  u32 position per record (SEARCH_NONE: none), ballot masks and tile counts as k_match_flag's
//   k_search_long  one workgroup per listed record (k_packed_decode's shape, decode_stream's blocks without the write half): the
//                  pattern's head compared at every boundary while the lanes' walks settle -- what a lane's last walk found is the
//                  settled walk's --, the rest confirmed from global memory, the lowest hit reduced over the workgroup; a record with
//                  an occurrence gets its position, and thread 0 corrects its bit of the tile's mask and the tile's count by one
//                  atomic each
//   k_packed_scan  the tile counts -> the tiles' first places in d_rows, n_match; its report is the call's
//   k_rows_emit    (unless d_rows is null: count only) the match's, with the positions as the join's key numbers
// SEARCH_LANE_BYTES is taken from the search_sweep leg of tools/batch_bench.py (profiles/search_bench.json): with
// records of one size the lane path is the faster one up to bodies of 600 bytes and the slower one at 2 400; 512 leaves room for
// stores of mixed sizes, where a wavefront waits for its longest body.
constexpr uint32_t SEARCH_NEEDLE_MAX = 256;                        // bytes of text in a needle
constexpr uint32_t SEARCH_PATTERN_BYTES = SEARCH_NEEDLE_MAX * 4;   // ... which take at most 32 bits each: 1 KiB, in LDS
#ifndef ET_SEARCH_LANE_BYTES  // (a build for the sweep sets it: 0 sends every body to a workgroup, 8192 every body of the sweep to a lane)
#define ET_SEARCH_LANE_BYTES 512
#endif
constexpr uint32_t SEARCH_LANE_BYTES = ET_SEARCH_LANE_BYTES;       // bodies up to this many bytes are walked by one lane
constexpr uint32_t SEARCH_GRID = 2048;                             // workgroups of k_search_flag and k_rows_emit at most
constexpr uint32_t SEARCH_NONE = 0xffffffffu;                      // the position of a record without an occurrence
enum SearchFlag : uint32_t { SEARCH_F_SUFFIX = 1 };                // beside MATCH_F_NOT and MATCH_F_NEVER
enum SearchWord { SEARCH_N_LONG = 4 };                             // the counters' word beside the records' two: records on the list
struct SearchJob {
    uint32_t head, head_mask;  // the pattern's first min(32, bits) bits at the top of a word, and which of its bits count
    uint32_t pat_bits;         // bits of the encoded needle
    uint32_t needle_len;       // its bytes of text
    uint32_t flags;            // SearchFlag | MatchFlag
    uint32_t pad;
};
// codes: the sorted codes on the device (launch_shared_decode's); pattern: the encoded needle on the device, zero-padded to a multiple
// of 4 bytes; pos_of, long_list: a u32 per record each -- workspace.  The report leaves with the scan, in front of k_rows_emit.
void launch_search(hipStream_t stream, const PackedStore &store, const uint2 *codes, uint32_t n_codes, const uint32_t *pattern, const SearchJob &job, uint32_t *d_rows,
                   uint64_t cap_rows, uint32_t *d_pos, uint8_t *d_status, const TileWs &tiles, uint32_t *pos_of, uint32_t *long_list, const PackedReport &report);

// The join (et_join_packed_device): which records of a packed store equal SOME key of a key set -- a packed store itself -- decided
// on the compressed bytes through a hash table in the workspace (et_join.h: the hash, the slot format, the table's size).
//   (clear)        the table's slots to ET_JOIN_EMPTY: one hipMemsetAsync
//   k_join_build   one key per lane: judged, its status byte, hashed, inserted by compare-and-swap and linear probing; equal keys
//                  meet in one slot and atomicMin leaves the lowest number there; the smallest and largest body of the valid keys
//   k_join_flag    one record per lane, tiles of MATCH_TILE records: judged, its status byte; a record whose body is no longer or
//                  shorter than some key's is hashed, probed and confirmed by bytes; a u64 ballot mask per 64 records, a u32 count
//                  per tile and a u32 key number per record into the workspace; its first workgroup reports the keys' counters
//   k_packed_scan  the tile counts -> the tiles' first places in d_rows, n_match; its report is the call's
//   k_rows_emit    (unless d_rows is null: count only) the match's; the record's number and, when asked for, its key's
// A lane hashes and compares a body of up to JOIN_LANE_BYTES alone; a longer one is taken from the ballot and handled by its
// whole wavefront, 8 bytes per lane and step, as k_match_flag handles its survivors.
constexpr uint32_t JOIN_LANE_BYTES = 128;  // 16 words of the hash
constexpr uint32_t JOIN_GRID = 2048;       // workgroups of k_join_build, k_join_flag and k_rows_emit at most
// The join's words of the counters and of the report, beside PACKED_N_FAILED and PACKED_FIRST (the records'): the keys' two, and in
// the counters the smallest and largest body of a valid key (first values ~0 and 0).  A probe or insert loop that ran through the
// whole table -- a bug -- sets JOIN_FAULT_BIT in PACKED_N_FAILED (a count is below 2^31), which k_packed_scan reports as it finds it.
enum JoinWord { JOIN_KEYS_FAILED = 4, JOIN_KEYS_FIRST = 5, JOIN_MIN = 6, JOIN_MAX = 7 };
constexpr unsigned long long JOIN_FAULT_BIT = 1ull << 63;
// table: `slots` u64 (a power of two, at least 2 * keys.n); key_of: a u32 per record -- workspace.  flags: MATCH_F_NOT or 0.  The
// report ({n_match, failed, first << 8 | status} by the scan, the keys' two by k_join_flag in front of it, then `epoch`) leaves with
// the scan.
void launch_join(hipStream_t stream, const PackedStore &records, const PackedStore &keys, uint32_t flags, unsigned long long *table, uint64_t slots, uint32_t *d_rows,
                 uint64_t cap_rows, uint32_t *d_key_of_row, uint8_t *d_status, uint8_t *d_key_status, const TileWs &tiles, uint32_t *key_of, const PackedReport &report);
// et_selftest_join_hash: d_hash[b] = the hash of record b as k_join_build and k_join_flag compute it (a failed record's entry is left).
void launch_join_hash(hipStream_t stream, const PackedStore &records, uint64_t *d_hash);

// The group (et_group_packed_device): which records of a packed store hold the same text -- the distinct texts in order of first
// appearance, how many records hold each, and every record's group -- decided on the compressed bytes as a join of the store with
// itself.  With the store as its own key set, the slot a record ends in names the lowest-numbered record of its text: the group's
// representative, whose rank among the representatives is the group's number.
//   (clear)         the table's slots to ET_JOIN_EMPTY: one hipMemsetAsync
//   k_group_build   k_join_build's tiles over the store itself: judged, hashed (the hash kept: a u64 per record), inserted -- the slot LOADED before
//                   any atomic, so that a record behind the first of its text, which finds a lower number there, issues none; the
//                   table is final behind it
//   k_group_flag    one record per lane, tiles of MATCH_TILE records: judged, its status byte, probed with the kept hash for the slot of its
//                   text; a slot that holds the record's own number ends the probe with no look at bytes, any other is confirmed by length,
//                   byte count and bytes; a u32 representative per record, ballot masks and tile counts of "is its own representative"
//   k_packed_scan   the tile counts -> the tiles' first group numbers, n_groups; its report is the call's
//   k_group_emit    (unless count only) per representative: d_first_rows[g], d_count[g] = 0, and g into a second word per record
//   k_group_number  (unless neither is asked for) per record: d_group_of[b] = its representative's g, and d_count[g] += 1 -- combined in
//                   the wavefront by rounds of "the lowest lane left takes its group, one atomic adds the popcount of the lanes that
//                   share it" until GROUP_COMBINE_MISSES rounds served their leader alone, the remainder adding singly
// Bodies above JOIN_LANE_BYTES are handled by the whole wavefront in the build and in the flag kernel, as in the join.
constexpr uint32_t GROUP_NONE = 0xffffffffu;      // d_group_of[b], and the representative, of a failed record
constexpr uint32_t GROUP_COMBINE_MISSES = 4;      // k_group_number stops combining after this many rounds that found their leader alone
// table: `slots` u64 (et_join_slots_for(records.n)), cleared; hash_of: a u64 per record, rep_of, dense: a u32 per record each --
// workspace.  The report ({n_groups, failed, first << 8 | status}, then `epoch`) leaves with the scan, in front of k_group_emit.
void launch_group(hipStream_t stream, const PackedStore &records, unsigned long long *table, uint64_t slots, uint32_t *d_first_rows, uint64_t cap_groups, uint32_t *d_count,
                  uint32_t *d_group_of, uint8_t *d_status, const TileWs &tiles, uint64_t *hash_of, uint32_t *rep_of, uint32_t *dense, const PackedReport &report);

// The take (et_take_packed_device): a selection of a packed store's records as a NEW packed store -- the bodies of rows[] copied
// back to back as they are, both offset arrays made by a scan -- without a table: no bit is interpreted.
//   k_take_plan   one row per lane (k_gather_plan's shape, plus: a body above TAKE_BODY_MAX is unsupported): a TakeRow per row into
//                 the workspace, its status byte
//   k_take_scan   ONE workgroup, tiles of TAKE_SCAN_TILE rows: the rows' body sizes -> out_body_index, their lengths ->
//                 out_text_index; the report ({body bytes, failed, first << 8 | status, text bytes}, then `epoch`) leaves with it
//   k_take_copy   (unless d_out is null: sizes only) destination-driven: the dense output is cut into tiles of TAKE_TILE_BYTES at
//                 multiples of that size of d_out's ADDRESS; a lane owns aligned 16-byte words of a tile, finds the rows that own the
//                 word's bytes in out_body_index and assembles it from the aligned 8-byte source words that hold them
struct TakeRow {  // what k_take_plan leaves per row: 16 bytes, one load of k_take_copy
    uint32_t body_bytes;  // 0 for a failed row
    uint32_t length;      // the record's text_index difference; 0 for a failed row
    uint64_t src;         // body_index[rows[k]]: where in d_bodies the body begins (0 for a failed row)
};
constexpr uint64_t TAKE_BODY_MAX = 4 * BATCH_SMALL_MAX;  // no body of symbols with codes of at most 32 bits is longer
constexpr uint32_t TAKE_SCAN_TILE = 4096;    // rows per trip of k_take_scan's one workgroup
constexpr uint32_t TAKE_TILE_BYTES = 8192;   // k_take_copy: bytes of output per trip of a workgroup, two 16-byte words per lane
constexpr uint32_t TAKE_STAGE_ROWS = 1024;   // ... entries of out_body_index a workgroup keeps in LDS for a tile (more: read in place)
constexpr uint32_t TAKE_GRID = 2048;         // workgroups of k_take_copy at most: what is resident at once on 256 CUs
enum TakeWord { TAKE_TEXT_BYTES = 3 };       // the report's word beside PACKED_BYTES, PACKED_N_FAILED and PACKED_FIRST
// plan: n_rows TakeRow of workspace (16-byte aligned).
void launch_take(hipStream_t stream, const PackedStore &store, const uint32_t *rows, uint32_t n_rows, void *d_out, uint64_t cap, uint64_t *out_body_index,
                 uint64_t *out_text_index, uint8_t *d_status, TakeRow *plan, const PackedReport &report);

// The derived stores -- the slice, the field, the concat and the recode below -- share one frame, stated once in et_batch.hip: a plan
// kernel is plan_rows (a row per lane: judge_row, reach_body, lane_walks; the lane's walk is lane_walk; the status byte, the tally, the
// wavefront's rows onto long_list with one atomic), a long kernel is long_rows (a listed row per workgroup, the list strided, nothing set
// up beyond the list; settle_block per 8 KiB block, reduce_min_min_max, cut_at_length, fail_row_late).  What is said of a kernel below
// is its family's middle.  The counters' word for the list is SLICE_N_LONG for all four, and for the number call, the frame's fifth member.
//
// The slice (et_slice_packed_device): symbols [first, first + count) of rows[]' stored texts, cut in front of a stop byte, as a NEW
// packed store -- under one complete prefix-free table a substring is the run of bits between two codeword boundaries, so the body the
// encoder would write for it is that run shifted to bit 7 of a byte, its last byte padded with zeros.  The search's walk finds the two
// boundaries, the take's scan lays the rows out and the take's copy, reading bits for bytes, writes them.
//   k_slice_plan  plan_rows, the sorted codes and the first-level table in LDS: judged as k_take_plan judges (judge_row);
//                 a body of which the slice's end can reach up to SLICE_LANE_BYTES (clip_body: 4 bytes per symbol in front of the end)
//                 is walked by its lane alone, from global memory, the walk ending where the slice does; a longer one goes onto a list
//                 and is an empty row for now; a TakeRow per row: {bytes of the new body, symbols, where its first BIT lies}
//   k_slice_long  long_rows: the blocks in front of the slice's end settled by a counting
//                 walk, the lanes whose codewords meet [first, end) walk again; begin, end and the lowest stop reduced over the
//                 workgroup; thread 0 stores the row's TakeRow
//   k_take_scan   the take's, unchanged: its report is the call's
//   k_take_copy   (unless d_out is null: sizes only) the take's tiles, rows and stores; a row's piece is a funnel shift of the source
//                 bytes that hold its bits -- none behind the slice's last bit is loaded -- and a row's last byte is masked to its bits
// A slice's TakeRow::src is the ADDRESS of its first bit (the byte's address * 8 + the bit, from the top) with the pad bits of its last
// byte (0 .. 7) above it: bits = body_bytes * 8 - pad.
// SLICE_LANE_BYTES is the search's threshold, kept: the lane's walk is search_lane's less the comparison and the workgroup's is
// search_stream's with a counting visitor, so the search's sweep is about these two loops as well; no sweep of
// the slice's own has been run.
#ifndef ET_SLICE_LANE_BYTES  // (a build for the sweep sets it, as ET_SEARCH_LANE_BYTES)
#define ET_SLICE_LANE_BYTES ET_SEARCH_LANE_BYTES
#endif
constexpr uint32_t SLICE_LANE_BYTES = ET_SLICE_LANE_BYTES;
constexpr uint32_t SLICE_NO_STOP = 0x100;   // SliceJob::stop when nothing cuts: no symbol
constexpr uint32_t SLICE_PAD_SHIFT = 61;    // TakeRow::src of a slice: the pad bits' place (an address of bits stays below 2^61)
enum SliceWord { SLICE_N_LONG = 4 };        // the counters' word beside the rows' two: rows on the list
struct SliceJob {
    const uint32_t *rows;              // null: row k is record k
    const uint32_t *d_first, *d_count; // null: the scalar beside it
    uint32_t n_rows, first, count;
    uint32_t stop;                     // the byte in front of which a slice ends, or SLICE_NO_STOP
};
// codes: the sorted codes on the device (launch_shared_decode's); plan: n_rows TakeRow of workspace (16-byte aligned); long_list: a
// u32 per row.  The report leaves with the scan, in front of the copy.
void launch_slice(hipStream_t stream, const PackedStore &store, const uint2 *codes, uint32_t n_codes, const SliceJob &job, void *d_out, uint64_t cap,
                  uint64_t *out_body_index, uint64_t *out_text_index, uint8_t *d_status, TakeRow *plan, uint32_t *long_list, const PackedReport &report);

// The field (et_field_packed_device): fields [field, field + n_fields) of rows[]' stored texts, cut at a delimiter byte, as a NEW
// packed store -- under one complete prefix-free table a delimiter is a codeword boundary whose codeword decodes to `delim`, so a run
// of fields is the run of bits between two such boundaries and is written exactly as a slice is.  The walk counts the delimiters it
// steps over; a codeword at or behind the record's length is no symbol of the stored text and is never counted.
//   k_field_plan  plan_rows: a body (clip_body of the whole length: nothing bounds where field k lies) up to
//                 FIELD_LANE_BYTES is walked by its lane alone with a running delimiter count, the walk ending at the closing
//                 delimiter; a longer one goes onto a list; a TakeRow per row in the slice's form, and d_pos
//   k_field_long  long_rows: per block the settling walk counts each lane's delimiters, a
//                 second scan numbers them across the lanes, the count carried across the blocks beside the codewords'; the lanes
//                 that hold one of the two target delimiters walk again; begin, closing delimiter and the text's end reduced over the
//                 workgroup; thread 0 stores the row's TakeRow and d_pos
//   k_take_scan, k_take_copy<BITS>   the slice's, unchanged
// FIELD_LANE_BYTES is the search's threshold, kept: the lane's walk is the slice's (lane_walk) with a counter.
#ifndef ET_FIELD_LANE_BYTES  // (a build for the sweep sets it, as ET_SEARCH_LANE_BYTES)
#define ET_FIELD_LANE_BYTES ET_SEARCH_LANE_BYTES
#endif
constexpr uint32_t FIELD_LANE_BYTES = ET_FIELD_LANE_BYTES;
constexpr uint32_t FIELD_ABSENT = 0xffffffffu;  // d_pos of a row whose record has no such field, and of a failed row
struct FieldJob {
    const uint32_t *rows;                   // null: row k is record k
    const uint32_t *d_field, *d_n_fields;   // null: the scalar beside it
    uint32_t *d_pos;                        // null: not asked for
    uint32_t n_rows, field, n_fields;
    uint32_t delim;                         // the delimiter byte
};
// codes, plan, long_list: as launch_slice's.
void launch_field(hipStream_t stream, const PackedStore &store, const uint2 *codes, uint32_t n_codes, const FieldJob &job, void *d_out, uint64_t cap,
                  uint64_t *out_body_index, uint64_t *out_text_index, uint8_t *d_status, TakeRow *plan, uint32_t *long_list, const PackedReport &report);

// The concat (et_concat_packed_device): row k = text(A[rows_a[k]]) + a literal + text(B[rows_b[k]]) as a NEW packed store -- under one
// complete prefix-free table the body the encoder writes for x + y is the bits of x followed by the bits of y, so a row is three runs
// of bits laid end to end: the left record's stored text (its pad dropped), the literal (et_encode_pattern, in the workspace), the
// right record's stored text.  Both sides are walked to the end of their stored text, as the slice walks; the row's length is the
// symbols of the three.  Either store may be absent (no bodies).
//   k_concat_plan  plan_rows over pairs of records: both judged as k_take_plan judges (judge_row), the row's status byte (the left's
//                  unless OK, else the right's, else PACKED_UNSUPPORTED for a new length above BATCH_SMALL_MAX); each side's body
//                  (clip_body of its length) up to CONCAT_LANE_BYTES is walked by the row's lane to the end of its stored text; a row
//                  with a longer one goes onto a list, that run absent for now; a TakeRow {new bytes, new length} and a ConcatPiece per row
//   k_concat_long  long_rows: the slice's counting walk (slice_stream) to the end of each stored text the lane left, one after
//                  the other; thread 0 completes the row's two records -- and fails the row where the length it found is above the limit
//   k_take_scan    the take's, unchanged: its report is the call's
//   k_concat_copy  (unless d_out is null: sizes only) k_take_copy's tiles, rows and stores; a row's bytes are the OR of its runs, each
//                  a funnel shift of the source bytes that hold its bits to the destination BIT the run begins at
// CONCAT_LANE_BYTES is the search's threshold, kept: the lane's walk is the slice's own (slice_lane); no sweep of its own.
#ifndef ET_CONCAT_LANE_BYTES  // (a build for the sweep sets it, as ET_SEARCH_LANE_BYTES)
#define ET_CONCAT_LANE_BYTES ET_SEARCH_LANE_BYTES
#endif
constexpr uint32_t CONCAT_LANE_BYTES = ET_CONCAT_LANE_BYTES;
constexpr uint32_t CONCAT_SEP_MAX = SEARCH_NEEDLE_MAX;  // bytes of text in the literal: its bits take SEARCH_PATTERN_BYTES at most
// Where a row's runs lie: 32 bytes, a 16-byte and an 8-byte load of k_concat_copy, four rows to a 128-byte line -- with the literal's
// place known to the kernel, the row's bits are [0, a_bits) from a_bit, [a_bits, a_bits + sep_bits) the literal, then b_bits from b_bit.
// Sources are ADDRESSES of bits (the byte's address * 8 + the bit, from the top): the two sides may be different stores.  The symbols
// are what k_concat_long needs of a walk the lane has done.  A side not walked yet, or without a stored text, is all zeros.
struct ConcatPiece {
    uint64_t a_bit;          // the address of the left run's first bit
    uint32_t a_bits, b_bits; // the two runs' bits
    uint64_t b_bit;          // the address of the right run's first bit
    uint32_t a_syms, b_syms; // the two stored texts' symbols
};
struct ConcatJob {
    const uint32_t *rows_a, *rows_b;  // null: row k is record k of that side
    const uint8_t *sep;               // the encoded literal on the device, zero-padded to a multiple of 4 bytes
    uint32_t n_rows;
    uint32_t sep_bits, sep_len;       // its bits; its bytes of text
    uint32_t pad;
};
// codes, plan, long_list: as launch_slice's; pieces: n_rows ConcatPiece of workspace
// (16-byte aligned).  a.bodies or b.bodies null: that side is absent.  The report leaves with the scan, in front of the copy.
void launch_concat(hipStream_t stream, const PackedStore &a, const PackedStore &b, const uint2 *codes, uint32_t n_codes, const ConcatJob &job, void *d_out, uint64_t cap,
                   uint64_t *out_body_index, uint64_t *out_text_index, uint8_t *d_status, TakeRow *plan, uint32_t *long_list, ConcatPiece *pieces, const PackedReport &report);


// The recode (et_recode_packed_device): rows[]' stored texts under table IN, each byte sent through a 256-entry map (or dropped), as
// a NEW packed store under table OUT -- the walk of the decodes feeding the pack loop of the encodes with nothing in between: for
// every symbol s of the stored text the codeword of map[s] under OUT is laid behind the one before.  The first packed call whose
// output bits are no copy of input bits, and the first with two tables; the map costs the device nothing: the host composes it with
// OUT into ONE table indexed by the INPUT symbol (RecodeEntry below).  Five launches, three for a sizes-only call:
//   k_recode_plan   plan_rows: judged as k_take_plan judges (judge_row); a body (clip_body of the whole length) up to
//                   RECODE_LANE_BYTES is walked by its lane to the end of its stored text, summing output bits, kept symbols and the
//                   "uncoded" flag; a longer one goes onto a list; a TakeRow per row: {new bytes, new length, new BITS}
//   k_recode_long   long_rows: the blocks settled by a walk whose visitor sums the same three per lane, the lane in which symbol
//                   `length` falls walks again, cut there (cut_at_length); the totals carried across the blocks; thread 0 stores the
//                   row's TakeRow, or fails the row where a kept symbol has no code
//   k_take_scan     the take's, unchanged: its report is the call's
//   k_recode_write  (unless d_out is null: sizes only) one lane per row the lane has planned: the walk again, the codes into a 64-bit
//                   accumulator that begins at the destination's aligned word; whole words leave as dword stores, the row's first and
//                   last word clipped to its bytes
//   k_recode_write_long   (likewise) long_rows, block by block: settled and cut, the lanes' output bits scanned to each
//                   lane's destination bit, the lanes walk again and OR their codes into an LDS bit image (pack_round's inner loop),
//                   flushed in rounds of RECODE_ROUND_BITS destination bits -- a block of 1-bit codes becomes 256 KiB of 32-bit ones
//                   --, the partial word carried as `pending` (pack_rounds' hand-over)
// A row owns whole bytes, so no two rows share an output byte and no workgroup waits for another.  The short and the long write are
// two kernels: one lane's registers and 8 KiB of LDS against a workgroup's 35 KiB; neither pays for the other's occupancy.
// RECODE_LANE_BYTES is the search's threshold, kept: the recode_sweep leg of tools/batch_bench.py (profiles/recode_sweep.json)
// has the lane path the faster one up to source bodies of 600 bytes and the slower one at 1 200 with records of one size; 512 leaves room for
// stores of mixed sizes, where a wavefront waits for its longest body.
#ifndef ET_RECODE_LANE_BYTES  // (a build for the sweep sets it, as ET_SEARCH_LANE_BYTES)
#define ET_RECODE_LANE_BYTES ET_SEARCH_LANE_BYTES
#endif
constexpr uint32_t RECODE_LANE_BYTES = ET_RECODE_LANE_BYTES;
constexpr uint32_t RECODE_ROUND_BITS = BATCH_STAGE_BYTES * 8;  // destination bits per flush of the long write: BatchDecLds::out is the image
// The output table's entry for INPUT symbol s: {the left-aligned code of map[s] under OUT, its length}; length 0: s is dropped;
// RECODE_UNCODED: s is kept but map[s] has no code under OUT -- a row whose stored text holds such a symbol fails.
constexpr uint32_t RECODE_UNCODED = 0x80000000u;
constexpr uint32_t RECODE_LEN_MASK = 0x3fu;
struct RecodeJob {
    const uint32_t *rows;  // null: row k is record k
    const uint2 *out_tab;  // 256 RecodeEntry-shaped pairs on the device (16-byte aligned)
    uint32_t n_rows, pad;
};
// codes: the sorted codes of table IN on the device (launch_shared_decode's); plan, long_list: as launch_slice's.
// The report leaves with the scan, in front of the two writes.
void launch_recode(hipStream_t stream, const PackedStore &store, const uint2 *codes, uint32_t n_codes, const RecodeJob &job, void *d_out, uint64_t cap,
                   uint64_t *out_body_index, uint64_t *out_text_index, uint8_t *d_status, TakeRow *plan, uint32_t *long_list, const PackedReport &report);

// The number (et_number_packed_device): rows[]' slices READ as integers -- CAST(SUBSTR(..) AS BIGINT), SUM / COUNT / MIN / MAX per group
// -- on the compressed bytes.  The fifth member of the derived-store frame, and the first that makes no store: the ask, the judgement,
// the reach and both walks are the slice's, but what a walk notes is not two bit positions: it is the digits, accumulated by ONE state
// machine (NumberParse, et_batch.hip) that both paths use -- sign seen, digits seen, the magnitude in a u64 that saturates, symbols
// seen, bad.  A row's output is a word, so there is no scan and no copy.
//   (fill)          the aggregates' first values: hipMemsetAsync for sum and n (0), k_number_fill for min and max (INT64_MAX, INT64_MIN)
//   k_number_plan   plan_rows: judged (judge_row), and a row whose group number is neither ET_GROUP_NONE nor below n_groups fails with
//                   PACKED_ARG; the ask is slice_ask, the reach reach_body(.., ask.end); a reach up to NUMBER_LANE_BYTES is walked by
//                   its lane (lane_walk), the visitor parsing from ask.first on, ending the walk at `stop` or at the first symbol that
//                   makes the row BAD; a longer one goes onto long_list and is EMPTY for now; the lane stores d_values[k], d_kind[k] and
//                   the row's NumberRow in the workspace
//   k_number_long   long_rows with slice_stream unchanged: its Sliced{begin, end, n} is the number's run of bits; n above
//                   NUMBER_SYMBOLS_MAX is BAD without another look, otherwise thread 0 walks the n codewords from `begin` (lane_walk over
//                   that run alone: nothing behind the slice's end is visited) and stores the row's three outputs
//   k_number_fold   always launched, a row per lane over the NumberRows: the three kinds tallied into the counters' words 5 .. 7, the
//                   aggregates that were asked for folded in -- combined in the wavefront as k_group_number combines its counts:
//                   the lowest lane left broadcasts its group, the ballot of the lanes with that group is its share, sum, min and max
//                   are reduced over them (the others hold the identity), the leader issues one atomic per aggregate, and after
//                   GROUP_COMBINE_MISSES rounds that served their leader alone the rest adds singly --; the last workgroup to arrive
//                   at the counters' word 0 sends the report {failed, first << 8 | status, empty, bad, range}, then `epoch`
// NUMBER_LANE_BYTES is the search's threshold, kept, as the slice and the field keep it: the lane's walk is the slice's with four more
// registers, the workgroup's IS the slice's; no sweep of its own has been run.
// Every loop is bounded as the frame states; the parse lane of k_number_long takes at most NUMBER_SYMBOLS_MAX trips.
#ifndef ET_NUMBER_LANE_BYTES  // (a build for the sweep sets it, as ET_SEARCH_LANE_BYTES)
#define ET_NUMBER_LANE_BYTES ET_SEARCH_LANE_BYTES
#endif
constexpr uint32_t NUMBER_LANE_BYTES = ET_NUMBER_LANE_BYTES;
constexpr uint32_t NUMBER_SYMBOLS_MAX = 32;  // 19 digits and a sign are what int64 needs; the rest is room for leading zeros
// A row's kind: et_number_packed_device's four (et_batch.cpp asserts the values), and in the workspace one more: the row failed.
enum NumberKind : uint32_t { NUMBER_OK = 0, NUMBER_EMPTY = 1, NUMBER_BAD = 2, NUMBER_RANGE = 3, NUMBER_FAILED = 4 };
// The counters' words beside PACKED_N_FAILED, PACKED_FIRST and SLICE_N_LONG: workgroups of k_number_fold that have arrived; rows of
// each kind but OK, which is the remainder.  The report's words are the same.
enum NumberWord { NUMBER_ARRIVED = 0, NUMBER_N_EMPTY = 5, NUMBER_N_BAD = 6, NUMBER_N_RANGE = 7 };
struct NumberRow {  // what the plan and the long kernel leave per row for the fold: 16 bytes, one load
    int64_t value;  // 0 unless NUMBER_OK
    uint32_t kind;  // NumberKind
    uint32_t pad;
};
struct NumberJob {
    SliceJob ask;               // the rows and the ask: the slice's, word for word
    int64_t *d_values;          // null: not asked for
    uint8_t *d_kind;            // likewise
    const uint32_t *group_of;   // the group of ROW k; null: every row in group 0
    uint32_t n_groups, pad;
    int64_t *d_sum;             // the aggregates, n_groups entries each; null: not asked for
    unsigned long long *d_n;
    int64_t *d_min, *d_max;
};
// codes, long_list: as launch_slice's; rows: n_rows NumberRow of workspace (16-byte aligned).  The report leaves with the fold.
void launch_number(hipStream_t stream, const PackedStore &store, const uint2 *codes, uint32_t n_codes, const NumberJob &job, uint8_t *d_status, NumberRow *rows,
                   uint32_t *long_list, const PackedReport &report);

}  // namespace et
