/*
 * entreepy_hip.h -- C ABI of libentreepy_hip.so: the MI355X (gfx950) Huffman
 * encode/decode path that drops in for typio/entreepy's src/encode.zig and
 * src/decode.zig.
 *
 * The reference has no FFI of its own; the seam is the pair of Zig functions
 *     pub fn encode(allocator, text, out_writer, std_out, flags) !usize   (src/encode.zig:25)
 *     pub fn decode(allocator, compressed_text, out_writer, std_out, flags) !usize (src/decode.zig:13)
 * called from src/main.zig:202,204 and src/test.zig:15,26.  Each entry point below
 * names the reference lines it replaces; INTEGRATION.md shows the Zig `extern fn`
 * declarations a maintainer adds to bind them.
 *
 * Conventions: plain pointers and sizes, no C++ or torch types.  Every function
 * returns an et_status (0 == ET_OK); nothing aborts or prints.  An et_ctx owns one
 * GPU's stream, workspaces and pinned staging and is NOT thread-safe; use one per
 * thread/GPU.  Pointers named d_* are device (HBM) pointers on the ctx's GPU,
 * everything else is host memory.
 */
#ifndef ENTREEPY_HIP_H
#define ENTREEPY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum et_status {
    ET_OK = 0,
    ET_ERR_EMPTY = 1,       /* error.QueueEmpty: empty input (queue.zig:28-30 via encode.zig:137-138) */
    ET_ERR_NOMEM = 2,       /* error.OutOfMemory (encode.zig:254) */
    ET_ERR_CAP = 3,         /* output buffer too small (writer error / error.NoSpaceLeft) */
    ET_ERR_FORMAT = 4,      /* malformed .et stream (the reference performs no validation, main.zig:199) */
    ET_ERR_HIP = 5,         /* HIP runtime failure; et_last_error() has the text */
    ET_ERR_ARG = 6,         /* null/misaligned/out-of-range argument */
    ET_ERR_UNSUPPORTED = 7, /* stream needs a feature outside the decoder's domain (code length > 32) */
    ET_ERR_IO = 8,          /* read/write on a file descriptor failed (et_encode_fd / et_decode_fd) */
    ET_ERR_RCCL = 9         /* the exchange between the GPUs of a group failed (RCCL error, or the callback's) */
} et_status;

/* The reference's `dictionary: [256]Code` (encode.zig:141-146) plus what its -d dump
 * and header need.  Plain data; filled by et_build_codebook / et_parse_header. */
typedef struct et_codebook {
    uint32_t data[256];      /* Code.data: path bits, u32-truncated (encode.zig:142,181,195) */
    uint8_t length[256];     /* Code.length: 0 == symbol absent (or dropped, 256-symbol quirk) */
    uint8_t dfs_order[256];  /* leaf symbols in the order encode.zig:204-212 prints them */
    uint32_t n_coded;        /* symbols with length > 0 */
    uint32_t min_length;     /* shortest non-zero length (0 when n_coded == 0) */
    uint32_t max_length;     /* longest length */
} et_codebook;

/* Wall-clock split of the last whole call, in milliseconds.  Device phases come from HIP events on
 * the ctx stream that the four large kernels carry themselves (begin and end of the histogram, pack,
 * first synchronisation sweep and write kernels; no marker packets between the kernels).
 * Replaces the -d "time taken" line (encode.zig:26-28). */
typedef struct et_timings {
    float hist_ms;      /* encode: the byte histogram kernel */
    float host_ms;      /* encode: tree/code build on the host; decode: header parse + table plan */
    float scan_ms;      /* encode: between the histogram and the pack kernel (reduce, host code construction, tile
                           scan, uploads); decode: between the first sweep and the write kernel (repair sweep,
                           verification, block count scan) */
    float body_ms;      /* encode: code scatter (pack) kernel; decode: symbol write kernel */
    float sync_ms;      /* decode: everything in front of the write kernel (sweeps, verification, scan) */
    float total_ms;     /* begin of the first large kernel to the end of the last */
    uint32_t sync_iters;/* decode: synchronisation launches */
    uint32_t reserved;  /* decode: bit 0 = the exhaustive synchronisation path ran, bit 1 = the sweeps ran as a tree walk, bit 2 = the write pass used the chained tables, bit 3 = synchronised (and, unless switched off, written) by rows: a complete code of 7- and 8-bit codewords, et_row_code, bit 4 = a fixed-length code (2^L codewords of L bits): decoded by arithmetic, no synchronisation (csrc/et_rowsync.h, k_fixed_write), bit 5 = the write pass whose output was kept ran as its instantiation for streams with more than 128 symbols per 256-bit subsequence (quarters that overflow the stage walk once, into strips) */
    float sync_first_ms;/* decode: the first synchronisation sweep alone (k_dec_sync<first>) */
    uint32_t pad_;
} et_timings;

typedef struct et_ctx et_ctx;

/* ---- lifetime ---------------------------------------------------------------- */
/* The reference call is stateless; a ctx amortises hipMalloc, pinned staging and
 * stream creation across calls.  `device` is a HIP device ordinal. */
int et_ctx_create(int device, et_ctx **ctx);
void et_ctx_destroy(et_ctx *ctx);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream) instead of the
 * ctx's own.  NULL is HIP's default (null) stream, as everywhere in HIP.
 * STREAM SWITCHES.  Calls return before their kernels finish.  A switch (this call or
 * et_ctx_use_own_stream, with a stream other than the current one) orders the new stream
 * after all the work the ctx enqueued before it, so the ctx may move between streams
 * with its calls in flight.  The old stream must still be valid at the moment of the
 * switch.  A buffer the ctx wrote on stream A and a later ctx call reads on stream B is
 * therefore safe; ordering against work that is not the ctx's stays the caller's job.
 * STATE A CTX KEEPS BETWEEN CALLS.  Two pairs of calls belong together through the ctx's workspaces:
 *   et_histogram_device(d_text, n)  ->  et_encode_body_device / et_encode_head_shard_device of the same (d_text, n), and
 *       et_histogram_host, et_histogram_device_ptr, et_histogram_on_host (the histogram link);
 *   et_decode_range_sync, or et_decode_range_maps -> et_decode_range_resolve  ->  et_decode_range_write (the held range).
 * Any other call of the ctx may come between the two halves, and then exactly one of two things holds: the second half gives what
 * it gives without that call, or it returns ET_ERR_ARG, enqueues nothing and writes nothing, and et_last_error names the first
 * half that is missing.  What drops the histogram link: a histogram of another text -- et_histogram_device, or a whole encode
 * (et_encode_device, et_encode, et_encode_fd, a stream that et_encode_batch_device hands to et_encode_device), after which the link
 * names THAT text --, et_ctx_set_tile_rounds, and any call that has to replace a workspace the histograms lie in (et_ctx_reserve
 * for a larger text).  What drops the held range: a whole-stream decode (et_decode_device, et_decode, et_decode_fd,
 * et_decode_body_device, a stream that et_decode_batch_device hands to et_decode_device), et_selftest_decode_tables and
 * et_selftest_treewalk_table (they rebuild the tables), and any call that has to replace a workspace the range lies in
 * (et_ctx_reserve again); another et_decode_range_sync / _maps puts its own range in place.  Everything else -- stream switches,
 * timing, the batched, shared-table and packed calls, the other pair's calls -- leaves both alone (tests/retained.py is the table). */
int et_ctx_set_stream(et_ctx *ctx, void *hip_stream);
/* Back to the non-blocking stream the ctx created for itself (a switch, as above). */
int et_ctx_use_own_stream(et_ctx *ctx);
/* The hipStream_t the ctx's calls are enqueued on, and its HIP device ordinal. */
void *et_ctx_stream(const et_ctx *ctx);
int et_ctx_device(const et_ctx *ctx);
/* Pre-size workspaces for inputs of up to max_text_bytes so that no allocation
 * happens inside a timed call. */
int et_ctx_reserve(et_ctx *ctx, size_t max_text_bytes);
/* Tuning/test knob: force the encode tile to `rounds` x 4 KiB (a power of two, 1 .. 128);
 * 0 restores the size-based choice.  Results never depend on it. */
int et_ctx_set_tile_rounds(et_ctx *ctx, uint32_t rounds);
/* Record per-phase HIP events (small overhead); off by default.  The calls stay as
 * asynchronous as they are without: the event arithmetic happens in et_last_timings[_of],
 * which waits for the call's last event.  et_last_timings = the last call's; _of: which =
 * 0 the last encode-side call, 1 the last decode (separate event sets, so the encode
 * figures can be fetched after the decode that followed has been enqueued).
 * on = ET_TIMING_DECODE_BODY: only the decode's write kernel carries its pair of events (a
 * dispatch that carries events costs ~5 us of queue time on either side of it: ~35 us of a
 * 1.4 ms step with all four large kernels timed); et_timings then holds body_ms, host_ms,
 * sync_iters and the flags, everything else 0. */
#define ET_TIMING_DECODE_BODY 2
int et_ctx_enable_timing(et_ctx *ctx, int on);
int et_last_timings(et_ctx *ctx, et_timings *out);
int et_last_timings_of(et_ctx *ctx, int which, et_timings *out);
const char *et_last_error(const et_ctx *ctx);
const char *et_strerror(int status);
const char *et_version(void);

/* ---- whole-call entry points (what the Zig shims bind) -------------------------- */
/* encode.zig:253-254: the reference sizes its scratch as 7200 + text.len; same bound
 * here (rounded up to a multiple of 16). */
size_t et_encode_bound(size_t text_len);

/* Replaces encode() (encode.zig:25-337) for write_output=true: histogram (:43-47),
 * code construction (:54-214), header+dictionary (:253-299), body pack (:303-318).
 * Writes the complete .et file image to out[0..*out_len).  ET_ERR_EMPTY for n == 0
 * (the reference raises error.QueueEmpty). */
int et_encode(et_ctx *ctx, const uint8_t *text, size_t n,
              uint8_t *out, size_t cap, size_t *out_len);

/* Replaces decode() (decode.zig:13-220).  `compressed` is the .et file MINUS its
 * first 4 bytes, exactly what main.zig:204 / test.zig:26 pass.  Emits body_len
 * symbols (header field, decode.zig:36-42), or fewer when the bitstream ends first. */
int et_decode(et_ctx *ctx, const uint8_t *compressed, size_t len,
              uint8_t *out, size_t cap, size_t *out_len);

/* The same two calls on open files: the reference reads the whole input
 * (main.zig:34-40,186) and writes the result with one writeAll (encode.zig:319,
 * main.zig:192-197); these move the file through two pinned staging buffers in chunks
 * (pread by a small thread pool while the previous chunk crosses PCIe; the result leaves
 * the same way with pwrite), so host memory stays bounded whatever the file size.
 * Regular files only (sized with fstat, positioned I/O).  out_fd < 0: code, write nothing
 * (main.zig's -t).  et_decode_fd skips `in_skip` bytes first: 4 = main.zig:204's
 * `text_in[4..]`.  *in_len = bytes consumed after the skip, *out_len = bytes produced.
 * et_encode / et_decode use the same pipeline on host memory. */
int et_encode_fd(et_ctx *ctx, int in_fd, int out_fd, size_t *in_len, size_t *out_len);
int et_decode_fd(et_ctx *ctx, int in_fd, size_t in_skip, int out_fd, size_t *in_len, size_t *out_len);

/* Code table of the ctx's most recent et_encode / et_encode_device (for the -d dump,
 * encode.zig:204-212, which the reference prints from inside encode()). */
int et_last_codebook(const et_ctx *ctx, et_codebook *out);

/* The -d self-check of encode.zig:221-247: every ordered pair (i, j) of coded symbols for which the
 * reference's loop finds one code a prefix of the other (pairs[2k] = i, pairs[2k+1] = j, in the reference's
 * i-then-j order; *n_pairs = how many there are, also beyond cap_pairs).  The reference prints "Found
 * colliding prefix codes for {i} {c} and {j} {c}" for each; a Huffman table never has any. */
int et_prefix_collisions(const et_codebook *cb, uint8_t *pairs, size_t cap_pairs, size_t *n_pairs);

/* The four bytes decode() never sees (main.zig:204 passes text_in[4..] unchecked, TODO at
 * main.zig:199): magic e7 c0 de and format version 01 (encode.zig:262-266).  ET_OK, or
 * ET_ERR_FORMAT with the reason in *why (static string; may be NULL).  The CLI refuses
 * files that fail this check instead of decoding whatever follows. */
int et_check_magic(const uint8_t first4[4], const char **why);

/* Diagnostics: build the decode lookup tables of `cb` both ways -- on the device (what every
 * decode call does, from the host's plan) and with the host-side reference builders -- and compare
 * them entry for entry.  ET_OK when identical; ET_ERR_FORMAT with *where = 1 first-level table,
 * 2 long list, 3 second-level tables, 4 code lengths, 5 step table, 6 write-step table. */
int et_selftest_decode_tables(et_ctx *ctx, const et_codebook *cb, int *where);

/* The synchronisation sweeps of a decode run as a fixed-rate walk over the code TREE when the dictionary is a
 * full binary tree (an encoder's always is): one table row per internal node, one byte of the stream per step
 * (csrc/et_treewalk.h).  et_treewalk_table: that table as the host fills it -- (*n_int + 7) x 256 entries of
 * next row | codewords completed in the byte << 8 | bit at which the first of them ends << 12 -- or
 * ET_ERR_UNSUPPORTED when the walk does not apply (table may be NULL to ask just that).
 * et_selftest_treewalk_table: build it on the device (what a decode does) and compare it with the host fill;
 * *first_diff = 1 + the first differing entry. */
int et_treewalk_table(const et_codebook *cb, uint16_t *table, size_t cap_entries, uint32_t *n_int);
int et_selftest_treewalk_table(et_ctx *ctx, const et_codebook *cb, uint32_t *first_diff);
/* Under the same condition the write pass (decode.zig:143-203 again, now emitting symbols) looks codewords up in
 * CHAINED tables: a root table indexed by the next 11 bits, and for every tree node such an index can end on
 * without completing a codeword a table of its own; each entry names the table of the NEXT lookup, so a long code
 * is one more step of its lane, not an exception (csrc/et_treewalk.h).  et_chain_tables: the tables as the host
 * fills them (u64 entries: lo = i16 (symbols << 10) - bits | first symbol << 16 | bits to the end of the first
 * symbol << 24; hi = byte offset of the next table | second symbol << 16 | (32 - its index bits) << 24), and where
 * each table begins / how many index bits it has.  et_selftest_treewalk_table compares the device fill of these
 * as well (*first_diff counts on behind the tree-walk table's entries). */
int et_chain_tables(const et_codebook *cb, uint64_t *table, size_t cap_entries, uint32_t *n_entries, uint32_t *table_first, uint8_t *table_bits,
                    size_t cap_tables, uint32_t *n_tables);

/* (Nearly) uniform bytes -- BASELINE.json's worst case -- give a complete code of 7- and 8-bit codewords that never
 * re-synchronises (decode.zig:143-203 has no trouble with it; a parallel decoder has).  When the 7-bit codewords are
 * the values 0 .. t-1, which is how encode.zig:82-138 hands them out, a decode synchronises such a stream in one pass by
 * rows (bytes) and columns (bit offsets): csrc/et_rowsync.h.  et_row_code: ET_OK and *t when `cb` is such a code,
 * ET_ERR_UNSUPPORTED otherwise (the exit maps for every start offset then, csrc/et_kernels_fallback.hip).  (A code of
 * 2^L codewords of L bits each -- t = 0 and t = 128 among them -- is decoded by arithmetic before either: symbol i is
 * the L bits at first_bit + i L.) */
int et_row_code(const et_codebook *cb, uint32_t *t);

/* Which synchronisation a one-GPU decode of a whole stream starts with for this code table (diagnostics; decode.zig:143-203
 * needs no such choice -- one thread walks the stream).  The stream itself can still overrule the two sweeps, TREE_WALK and
 * WINDOWS: blocks that do not settle under them go to the exit maps, or by rows if the code is a row code.
 *   ET_PATH_TREE_WALK  the tree walk (text, and codes of L and L + 1 bits whose mix of lengths settles quickly: csrc/et_rowsync_host.cpp)
 *   ET_PATH_EXIT_MAPS  exit maps for every start offset (codes of one or two neighbouring lengths that do not settle and are neither
 *                      fixed-length nor row codes, with or without a tree; csrc/et_kernels_fallback.hip)
 *   ET_PATH_ROWS       by byte rows and bit columns (complete codes of 7 and 8 bits that do not settle: uniform bytes; et_row_code)
 *   ET_PATH_FIXED      2^L codewords of L bits: no synchronisation, symbol i is the L bits at first_bit + i L
 *   ET_PATH_WINDOWS    the round-1 window kernels (a dictionary whose completed tree has more than 255 internal nodes or is not
 *                      prefix-free, unless its lengths send it to the exit maps) */
enum { ET_PATH_TREE_WALK = 0, ET_PATH_EXIT_MAPS = 1, ET_PATH_ROWS = 2, ET_PATH_FIXED = 3, ET_PATH_WINDOWS = 4 };
int et_decode_path(const et_codebook *cb, uint32_t *path);

/* Header field "length of body" (decode.zig:36-42) so callers can size `out`. */
int et_decoded_size(const uint8_t *compressed, size_t len, size_t *n_symbols);

/* Same two calls with input and output resident in HBM (benchmarks, pipelines).
 * d_out must hold et_encode_bound(n) bytes / n_symbols bytes.  Both are
 * stream-ordered: *out_len is final on return, the bytes in d_out are complete once the
 * ctx's stream has drained (enqueue consumers on it, or synchronise it).
 * WHAT A CALL WRITES (tests/test_gpu_extent.py, guard bytes around d_out): nothing in front of d_out, nothing at or past
 * d_out + cap; a call that returns ET_ERR_CAP has written nothing and stored *out_len = 0, and the ctx is as good as before
 * it.  et_decode_device and et_decode_body_device: cap >= n_symbols suffices, and nothing outside [d_out, d_out + *out_len)
 * is written -- measured on an MI355X for every decode write kernel at ragged, clamped and truncated lengths; none uses the 16 bytes
 * of slack this comment used to ask for. */
int et_encode_device(et_ctx *ctx, const void *d_text, size_t n,
                     void *d_out, size_t cap, size_t *out_len);
int et_decode_device(et_ctx *ctx, const void *d_compressed, size_t len,
                     void *d_out, size_t cap, size_t *out_len);

/* ---- batches of small streams ------------------------------------------------------------------- */
/* The calls above cost about 0.05 ms each before the first byte moves (their launches, and a hand-over to the host
 * for the code table / the dictionary); a caller with ten thousand pages or records pays that ten thousand times.
 * These two take B independent streams in ONE call: one workgroup per stream, two launches and one hand-over per
 * 1024 streams (csrc/et_batch.h).  The reference has no counterpart (one file per run, main.zig:186-204); every
 * stream's result is exactly what et_encode_device / et_decode_device give for it alone.
 * Stream b reads d_in[in_off, in_off + in_len) and may write d_out[out_off, out_off + out_cap), nothing else.
 *   encode: input = text (any alignment); output = the complete .et image; out_cap >= et_encode_bound(in_len),
 *           d_out + out_off 16-byte aligned.
 *   decode: input = the .et file minus its first 4 bytes (any alignment); out_cap >= the symbols it holds.
 * The return value is about the call: ET_ERR_ARG (a null pointer; outputs of two items that overlap -- checked
 * on the host before anything is enqueued), ET_ERR_HIP, ET_ERR_NOMEM.  What became of stream b is in
 * items[b].status -- ET_ERR_EMPTY (no text), ET_ERR_CAP, ET_ERR_FORMAT, ET_ERR_UNSUPPORTED (a code beyond 32 bits in
 * a dictionary) -- and a stream that fails fails alone.  n_items == 0 is ET_OK and enqueues nothing.
 * Stream-ordered like et_encode_device: out_len and status are final on return, the bytes once the ctx's stream
 * has drained.  Streams the batch kernels are not made for -- texts above et_batch_small_max(), codes beyond 32 bits
 * on encode, dictionaries that are not a full tree on decode -- run through et_encode_device / et_decode_device
 * inside the same call (path = 1; then d_out + out_off must be 16-byte aligned for a decode, too). */
typedef struct et_batch_item {
    uint64_t in_off, in_len;
    uint64_t out_off, out_cap;
    uint64_t out_len;   /* result: bytes produced (0 unless status == ET_OK) */
    int32_t status;     /* result: this stream's et_status */
    uint32_t path;      /* result: 0 = the batch kernels, 1 = the single-stream path */
} et_batch_item;
int et_encode_batch_device(et_ctx *ctx, const void *d_in, void *d_out, et_batch_item *items, size_t n_items);
int et_decode_batch_device(et_ctx *ctx, const void *d_in, void *d_out, et_batch_item *items, size_t n_items);
/* The longest text the batch kernels take themselves, and sizeof(et_batch_item) as the library was built (bindings
 * check their mirror of the struct against it). */
size_t et_batch_small_max(void);
size_t et_batch_item_size(void);

/* Batched BODIES under ONE code table given by the caller (what a record store calls a dictionary): no magic, no
 * header and no dictionary per record, and no per-record table work on either side -- the kernels set their tables up
 * once per workgroup, and the only hand-over to the host is each chunk's lengths and statuses (4096 records per chunk,
 * csrc/et_batch.h).  The calls do NOT store the table: the caller writes it once with et_write_header and reads it
 * back with et_parse_header.  A table from et_build_codebook covers at most 255 byte values (and only those its
 * histogram saw); a record with a byte outside it comes back ET_ERR_UNSUPPORTED and the caller stores it raw.
 * et_batch_item as above, path always 0; stream-ordered as above (out_len and status final on return, the bytes once the
 * ctx's stream has drained); a record that fails fails alone.
 *   et_codebook_is_complete (host only): ET_OK when the coded symbols form a full prefix-free tree -- at least two of
 *     them, every length <= 32, no code a prefix of another, sum of 2^(32 - length) == 2^32; ET_ERR_UNSUPPORTED otherwise
 *     (a lone symbol, a hand-made table with holes, a code beyond 32 bits).  Both calls ask it first: for a table that
 *     fails they return ET_ERR_UNSUPPORTED with nothing enqueued and every out_len = 0.
 *   et_body_bound (host only): (n * max_length + 7) / 8, an out_cap that always suffices for n bytes of text.
 *   encode: d_in[in_off, in_off + in_len) (any alignment) -> its codewords MSB-first from bit 7 of d_out[out_off] (ANY
 *     alignment), the last byte padded with zero bits; out_len = ceil(bits / 8).  Exactly [out_off, out_off + out_len) is
 *     written -- not the rest of a word, unlike et_encode_batch_device -- so bodies may lie back to back.  in_len == 0:
 *     ET_OK, out_len 0.  in_len > et_batch_small_max(): ET_ERR_UNSUPPORTED.  A byte without a code: ET_ERR_UNSUPPORTED.
 *     ceil(bits / 8) > out_cap: ET_ERR_CAP.  A failed record has written nothing and has out_len 0.
 *     SIZES ONLY: with d_out == NULL nothing is written and no overlap is checked; out_len and status are what the
 *     writing call gives with out_cap unlimited.  A caller sizes first, prefix-sums, then packs densely.
 *   decode: the body d_in[in_off, in_off + in_len) (any alignment); out_cap is THE NUMBER OF SYMBOLS TO DECODE -- the
 *     caller keeps a record's length; the pad bits may decode as symbols otherwise.  out_len = min(out_cap, codewords
 *     that end inside the body) symbols go to d_out[out_off, ...) (any alignment), and nothing outside
 *     [out_off, out_off + out_len) is written.  A body that ends early: ET_OK with the shorter out_len.  in_len == 0 or
 *     out_cap == 0: ET_OK, out_len 0.  out_cap > et_batch_small_max(): ET_ERR_UNSUPPORTED.
 * The call's own status: ET_ERR_ARG (null ctx, cb, items or d_in; null d_out on decode; overlapping outputs, checked
 * before anything is enqueued), ET_ERR_UNSUPPORTED (the table), ET_ERR_HIP, ET_ERR_NOMEM.  n_items == 0: ET_OK. */
int et_encode_shared_device(et_ctx *ctx, const et_codebook *cb, const void *d_in, void *d_out, et_batch_item *items, size_t n_items);
int et_decode_shared_device(et_ctx *ctx, const et_codebook *cb, const void *d_in, void *d_out, et_batch_item *items, size_t n_items);
int et_codebook_is_complete(const et_codebook *cb);
size_t et_body_bound(const et_codebook *cb, size_t n);

/* PACKED record batches: the same bodies under the same one table, but input and output are both what a record store keeps --
 * dense bytes plus n + 1 offsets of 64 bits, all in device memory -- and the offsets of the bodies are computed on the GPU.
 * One call where the shared-table calls need a sizes-only call, a prefix sum on the host and a writing call; no per-record
 * structs on the host at all.  Passing a sub-range of the offsets decodes that sub-range of the records (random access to one
 * run of records; a selection of records in any order goes through et_decode_packed_gather_device, below).
 * All d_* pointers are device pointers on the ctx's GPU.  The offset arrays hold n + 1 entries and must be 8-byte aligned; the
 * data pointers may have any alignment.  Each record is judged from its own pair of entries: a pair that decreases or
 * leaves its buffer fails that record alone (ET_ERR_ARG), and no kernel reads or writes where such a pair points.
 *   encode: record b = d_text[text_index[b], text_index[b+1]) -> exactly the bytes the shared-table encode gives for it, at
 *     d_out[out_index[b], out_index[b+1]); out_index[0] = 0, the bodies lie back to back, nothing at or beyond
 *     d_out + out_index[n] is written.  A failed record takes no bytes (out_index[b+1] == out_index[b]); d_status[b] (one
 *     et_status byte per record; d_status may be NULL) says why: ET_ERR_UNSUPPORTED for a byte without a code or a record above
 *     the small-stream limit, ET_ERR_ARG unless text_index[b] <= text_index[b+1] <= text_bytes.  An empty record: ET_OK, no bytes.
 *     d_out == NULL: sizes only -- d_out_index, d_status and *res are the writing call's, cap is ignored.
 *     out_index[n] > cap: the call returns ET_ERR_CAP, not a byte of d_out is written, d_out_index is still complete and
 *     res->out_bytes is the room needed.
 *   decode: record b = text_index[b+1] - text_index[b] symbols from d_bodies[body_index[b], body_index[b+1]) to
 *     d_out + text_index[b]: the text offsets are the store's record lengths and lay the output out.  d_written[b] (may be
 *     NULL) = symbols stored; nothing outside [text_index[b], text_index[b] + written[b]) is written for any record.  A body
 *     that ends early: ET_OK with fewer symbols, counted in n_short, the rest of its room untouched.  An empty body or a
 *     count of zero: ET_OK, nothing written -- so a record the encoder failed (kept raw elsewhere) leaves its room alone
 *     (an empty body under a count above zero ended early like any other: n_short counts it).
 *     ET_ERR_ARG unless body_index[b] <= body_index[b+1] <= body_bytes and text_index[b] <= text_index[b+1] <= cap;
 *     ET_ERR_UNSUPPORTED for a count above the small-stream limit.  text_index[n] > cap: the call returns ET_ERR_CAP and
 *     nothing is written (d_written and d_status neither).
 * The call's own status: ET_ERR_ARG (a null ctx, cb, res, input pointer or offset array; a null d_out_index on encode; a null
 * d_out on decode; a misaligned offset array; n > 0x7fffffff), ET_ERR_UNSUPPORTED (the table is not complete: nothing is
 * enqueued), ET_ERR_CAP, ET_ERR_HIP, ET_ERR_NOMEM.  n == 0: ET_OK, nothing enqueued, *res zeroed.  Stream-ordered like the other
 * device calls: *res is final on return, the device arrays once the ctx's stream has drained.  Packed and shared-table calls
 * may follow each other on one ctx, with different tables, with nothing in between. */
typedef struct et_packed_result {
    uint64_t out_bytes;     /* encode: out_index[n] = bytes the bodies take, also when the call returns ET_ERR_CAP or d_out is NULL;
                               decode: text_index[n] */
    uint64_t n_failed;      /* records whose status is not ET_OK */
    uint64_t first_failed;  /* the lowest such record (valid when n_failed > 0) */
    uint64_t n_short;       /* decode: ET_OK records whose body ended before their symbol count; encode: 0 */
    int32_t first_status;   /* et_status of record first_failed */
    uint32_t pad;
} et_packed_result;
size_t et_packed_result_size(void);
int et_encode_packed_device(et_ctx *ctx, const et_codebook *cb,
                            const void *d_text, size_t text_bytes, const uint64_t *d_text_index, size_t n,
                            void *d_out, size_t cap, uint64_t *d_out_index, uint8_t *d_status,
                            et_packed_result *res);
int et_decode_packed_device(et_ctx *ctx, const et_codebook *cb,
                            const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                            const uint64_t *d_text_index, size_t n,
                            void *d_out, size_t cap, uint32_t *d_written, uint8_t *d_status,
                            et_packed_result *res);
/* GATHER: a SELECTION of a packed store's records -- what a filter, a join or an index lookup leaves -- decoded into a dense
 * output with offsets, on the device, in one call.  The store is et_decode_packed_device's: d_bodies, and d_body_index and
 * d_text_index of n_records + 1 entries each; the text offsets serve as record lengths only.  d_rows[k] (n_rows of them, 32 bits,
 * 4-byte aligned, on the device) is the record that row k of the result is; rows may come in any order and may repeat.  The output
 * is laid out by the call, on the GPU: out_index[0] = 0, row k owns d_out[out_index[k], out_index[k+1]), and its room is its
 * record's length text_index[r+1] - text_index[r] when its status is ET_OK, 0 when it failed.  d_written[k] (may be NULL) = symbols
 * stored at d_out + out_index[k]; nothing outside [out_index[k], out_index[k] + written[k]) is written for any row, and nothing at
 * or beyond d_out + out_index[n_rows].
 *   A body that ends early: ET_OK with fewer symbols, counted in n_short, the rest of its room untouched -- an empty body under a
 *     length above zero among them, whose room is kept so that a record the encoder failed (kept raw elsewhere) can be patched into
 *     place; as in et_decode_packed_device.
 *   d_status[k] (one et_status byte per ROW; may be NULL): ET_ERR_ARG when d_rows[k] >= n_records, and unless
 *     body_index[r] <= body_index[r+1] <= body_bytes and text_index[r] <= text_index[r+1]; ET_ERR_UNSUPPORTED for a length above
 *     the small-stream limit.  A row fails alone, no kernel reads or writes where a bad pair points, and a bad record that no row
 *     selects does not matter.  In *res, n_failed, first_failed and first_status are about ROWS (positions k), and out_bytes is
 *     out_index[n_rows].
 *   d_out == NULL: sizes only -- d_out_index, d_status and *res are the writing call's except that n_short is 0; cap is ignored
 *     and d_written is not touched.
 *   out_index[n_rows] > cap: the call returns ET_ERR_CAP, not a byte of d_out is written and d_written is not touched;
 *     d_out_index and d_status are complete and res->out_bytes is the room needed.  d_written is complete whenever the call
 *     returns ET_OK with d_out given.
 * The call's own status: ET_ERR_ARG (a null ctx, cb, res, d_bodies, d_body_index, d_text_index, d_rows or d_out_index; an offset
 * array that is not 8-byte aligned, d_rows not 4-byte aligned; n_records or n_rows above 0x7fffffff -- all checked before
 * anything touches a device), ET_ERR_UNSUPPORTED (the table is not complete: nothing is enqueued), ET_ERR_CAP, ET_ERR_HIP,
 * ET_ERR_NOMEM.  n_rows == 0: ET_OK, nothing enqueued, *res zeroed.  One upload (the table and zeroed counters), three launches
 * and one hand-over per call; stream-ordered like the other packed calls, and it may follow or precede packed, shared-table and
 * single-stream calls on one ctx with nothing in between. */
int et_decode_packed_gather_device(et_ctx *ctx, const et_codebook *cb,
                                   const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                                   const uint64_t *d_text_index, size_t n_records,
                                   const uint32_t *d_rows, size_t n_rows,
                                   void *d_out, size_t cap, uint64_t *d_out_index,
                                   uint32_t *d_written, uint8_t *d_status, et_packed_result *res);

/* MATCH: which records of a packed store equal a key, or begin with it -- the list of record numbers the gather call consumes,
 * produced on the device WITHOUT decoding.  Under one complete prefix-free table a record's body begins at bit 7 of its first
 * byte, so its text begins with the needle exactly when its body begins with the needle's codewords and its length is at least
 * the needle's; the filter reads two pairs of offsets and usually one cache line of body per record.
 *   et_encode_pattern (host only, HIP-free): the bits of `text` under cb exactly as the shared-table encode lays a body out --
 *     MSB-first from bit 7 of out[0], the last byte zero-padded; *n_bits = their number.  n == 0: ET_OK, 0 bits.
 *     ET_ERR_UNSUPPORTED: a byte without a code, or a code beyond 32 bits (*n_bits = 0).  ET_ERR_CAP: (n_bits + 7) / 8 > cap
 *     (*n_bits is still the need).  ET_ERR_ARG: null cb or n_bits, null text with n > 0, null out with bytes to store.
 *   The store is the gather call's: d_bodies, and d_body_index and d_text_index of n_records + 1 entries each, 8-byte aligned; the
 *     text offsets serve as record lengths only.  A record is judged from its own two pairs: ET_ERR_ARG unless
 *     body_index[b] <= body_index[b+1] <= body_bytes and text_index[b] <= text_index[b+1]; ET_ERR_UNSUPPORTED for a length above
 *     the small-stream limit.  A failed record is never selected -- not under ET_MATCH_NOT either -- it fails alone, and no kernel
 *     reads where its pair points.  d_status[b] (one et_status byte per record; may be NULL) holds its status.
 *   A match: let text_b be what et_decode_packed_device would store for record b, the first min(length_b, codewords that end
 *     inside its body) symbols.  ET_MATCH_PREFIX: text_b starts with the needle.  ET_MATCH_EQUAL: length_b == needle_len and
 *     text_b == needle -- so a record whose body ends before its length (kept raw elsewhere, or cut) can match a prefix of what is
 *     there and never matches EQUAL.  ET_MATCH_NOT, or-ed in, selects the valid records that do NOT match.  The empty needle
 *     matches every valid record under PREFIX, every valid record of length 0 under EQUAL.  A needle byte without a code matches
 *     nothing: the call is ET_OK, pattern_bits is 0, and under NOT every valid record is selected.  needle is HOST memory.
 *   Order: ET_MATCH_LESS selects the valid records with text_b < needle, ET_MATCH_LESS_EQUAL those with text_b <= needle; with
 *     ET_MATCH_NOT or-ed in they are >= and > (a failed record is never selected).  The comparison is memcmp's, and Python's on
 *     bytes: byte by byte as unsigned values, a proper prefix is less.  It is decided on the compressed bytes too: the first bit
 *     at which body and encoded needle differ lies inside the codeword of the first symbol at which the texts differ, so a record
 *     costs one codeword decoded at a boundary of the needle's -- `key < x`, `key >= x`, and the bucket counts of a range
 *     partition from count-only calls.  text_b is the stored text above, hence: a record kept raw elsewhere (no body bytes, a
 *     length above zero) reads as the empty text and lies below every needle that is not empty.  A body cut exactly behind the
 *     needle's last codeword compares EQUAL here -- its stored text IS the needle: LESS_EQUAL selects it, LESS does not -- while
 *     ET_MATCH_EQUAL, which asks for length_b == needle_len, rejects it: `<=` is not `<` or `==` on such a record.  Nothing is
 *     less than the empty needle; LESS_EQUAL selects the records whose stored text is empty.  A needle byte without a code is
 *     handled exactly here (EQUAL and PREFIX keep their rule): with j its first position, no record holds that byte, so the order
 *     is decided against needle[:j], and for a record that starts with needle[:j] and goes on, by its symbol j against the byte
 *     needle[j]; pattern_bits is the bit count of needle[:j] -- of the whole needle when every byte has a code.  The values 2
 *     and 3 are no modes.
 *   d_rows[0 .. n_match) (32 bits each, 4-byte aligned, on the device) = the selected record numbers, ascending: the gather
 *     call's d_rows.  Nothing at or beyond d_rows + n_match is written.  d_rows == NULL: count only -- cap_rows is ignored,
 *     d_status and *res are the writing call's.  n_match > cap_rows: the call returns ET_ERR_CAP, no entry of d_rows is written,
 *     d_status is complete and res->n_match is the room needed.
 * The call's own status: ET_ERR_ARG (a null ctx, cb, res, d_bodies, d_body_index or d_text_index; a null needle with
 * needle_len > 0; an offset array that is not 8-byte aligned, d_rows not 4-byte aligned; n_records above 0x7fffffff; needle_len
 * above et_match_pattern_max(); an unknown mode -- all checked before anything touches a device, *res untouched),
 * ET_ERR_UNSUPPORTED (the table is not complete: nothing is enqueued), ET_ERR_CAP, ET_ERR_HIP, ET_ERR_NOMEM.  n_records == 0:
 * ET_OK, nothing enqueued, *res zeroed.  One upload (zeroed counters and the encoded needle, 16 KiB at most), three launches and
 * one hand-over per call; stream-ordered like the other packed calls -- *res is final on return, the device arrays once the ctx's
 * stream has drained -- and it may follow or precede packed, gather, shared-table and single-stream calls on one ctx with nothing
 * in between and with different tables: d_rows may go straight into et_decode_packed_gather_device on the same ctx. */
int et_encode_pattern(const et_codebook *cb, const uint8_t *text, size_t n, uint8_t *out, size_t cap, uint64_t *n_bits);
enum { ET_MATCH_EQUAL = 0, ET_MATCH_PREFIX = 1, ET_MATCH_LESS = 4, ET_MATCH_LESS_EQUAL = 5,
       ET_MATCH_NOT = 0x100 /* or-ed in: select the valid records that do NOT match */ };
size_t et_match_pattern_max(void);          /* longest needle in bytes of text: 4096 */
typedef struct et_match_result {
    uint64_t n_match;       /* rows selected -- also when the call returns ET_ERR_CAP or d_rows is NULL */
    uint64_t n_failed, first_failed;   /* records whose status is not ET_OK, the lowest of them (valid when n_failed > 0) */
    int32_t first_status;   /* et_status of record first_failed */
    uint32_t pattern_bits;  /* bits of the encoded needle (0 when a needle byte has no code; LESS modes: of the bytes in front of it) */
} et_match_result;
size_t et_match_result_size(void);
int et_match_packed_device(et_ctx *ctx, const et_codebook *cb,
                           const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                           const uint64_t *d_text_index, size_t n_records,
                           const uint8_t *needle, size_t needle_len, int mode,   /* needle: HOST memory */
                           uint32_t *d_rows, size_t cap_rows, uint8_t *d_status, et_match_result *res);

/* SEARCH: which records of a packed store CONTAIN a needle, or END with it, and at which symbol -- key LIKE '%x%' and key LIKE '%x' --
 * found on the device WITHOUT decoding: the decode's walk over the codeword boundaries with a bit comparison at each and nothing
 * written.  Under one complete prefix-free table the needle occurs at symbol i of a record's text exactly when its bits
 * (et_encode_pattern) lie at the bit where codeword i begins, end inside the body, and i + needle_len <= length_b: the parse from a
 * boundary is unique, the same bits at a bit that is no boundary are no occurrence, and the length bound rejects what the pad bits
 * behind the last codeword read as.
 *   The store, the judgement of a record from its own two pairs, d_status, d_rows, cap_rows, ET_MATCH_NOT and *res are the match
 *     call's: a failed record is never read and never selected -- not under ET_MATCH_NOT either -- and fails alone.
 *   text_b is what et_decode_packed_device would store for record b: the first n_b = min(length_b, codewords that end inside its
 *     body) symbols.  ET_SEARCH_CONTAINS: the needle occurs in text_b; its position is the lowest symbol index, text_b.find(needle).
 *     ET_SEARCH_SUFFIX: n_b == length_b and text_b ends with the needle; its position is length_b - needle_len -- so a record whose
 *     body ends before its length never matches SUFFIX, as it never matches ET_MATCH_EQUAL, and can match CONTAINS on what is
 *     there.  The empty needle: CONTAINS selects every valid record at position 0, SUFFIX every valid record with n_b == length_b
 *     at position length_b.  A needle byte without a code matches nothing: the call is ET_OK, pattern_bits is 0, and under NOT
 *     every valid record is selected.  needle is HOST memory.
 *   d_rows[0 .. n_match): the selected record numbers, ascending -- the gather and take calls' d_rows; nothing at or beyond
 *     d_rows + n_match is written.  d_rows == NULL: count only.  n_match > cap_rows: ET_ERR_CAP, no entry of d_rows or d_pos is
 *     written, d_status is complete and res->n_match is the room needed.
 *   d_pos (may be NULL; 32 bits each, 4-byte aligned, as large as d_rows and written only where d_rows is): d_pos[i] = the position
 *     in record d_rows[i].
 *   et_search_lane_bytes(): a body of up to this many bytes is walked by one lane, a longer one by a workgroup -- for tests that
 *     want records on both sides; the answer does not depend on it.
 * The call's own status: ET_ERR_ARG (a null ctx, cb, res, d_bodies, d_body_index or d_text_index; a null needle with
 * needle_len > 0; an offset array that is not 8-byte aligned, d_rows or d_pos not 4-byte aligned; n_records above 0x7fffffff;
 * needle_len above et_search_needle_max(); an unknown mode; d_pos with ET_MATCH_NOT, or with d_rows == NULL -- all checked before
 * anything touches a device, *res untouched), ET_ERR_UNSUPPORTED (the table is not complete: nothing is enqueued), ET_ERR_CAP,
 * ET_ERR_HIP, ET_ERR_NOMEM.  n_records == 0: ET_OK, nothing enqueued, *res zeroed.  One upload (the sorted codes, zeroed counters
 * and the encoded needle, 3.2 KiB at most), four launches and one hand-over per call; stream-ordered like the other packed calls --
 * *res is final on return, the device arrays once the ctx's stream has drained -- and it may follow or precede any of them on one
 * ctx with nothing in between: d_rows may go straight into et_decode_packed_gather_device or et_take_packed_device.
 * Out of scope: case folding and wildcards inside the needle, several needles per call, counting every occurrence, needles above
 * et_search_needle_max() and records above et_batch_small_max(). */
enum { ET_SEARCH_CONTAINS = 0, ET_SEARCH_SUFFIX = 1 };   /* ET_MATCH_NOT may be or-ed in */
size_t et_search_needle_max(void);          /* longest needle in bytes of text: 256 */
size_t et_search_lane_bytes(void);          /* bodies up to this many bytes are walked by one lane */
int et_search_packed_device(et_ctx *ctx, const et_codebook *cb,
                            const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                            const uint64_t *d_text_index, size_t n_records,
                            const uint8_t *needle, size_t needle_len, int mode,   /* needle: HOST memory */
                            uint32_t *d_rows, size_t cap_rows, uint32_t *d_pos,
                            uint8_t *d_status, et_match_result *res);

/* JOIN: which records of a packed store equal SOME key of a key set -- itself a packed store under the same table, in device
 * memory (e.g. what et_encode_packed_device made of a key column, or a run of another store) -- decided on the compressed bytes:
 * key IN (...), a semi-join against another table's key column, with ET_MATCH_NOT an anti-join.  One build pass over the keys (a
 * hash table in the ctx's workspace) and one probe pass over the records replace one et_match_packed_device call per key.
 *   Both sides are judged by the match call's rule, each from its own arrays: ET_ERR_ARG unless
 *     body_index[i] <= body_index[i+1] <= its buffer's bytes (body_bytes, key_body_bytes) and text_index[i] <= text_index[i+1];
 *     ET_ERR_UNSUPPORTED for a length above the small-stream limit.  A failed record is never selected -- not under ET_MATCH_NOT
 *     either --, a failed key equals nothing, either fails alone, and no kernel reads where a bad pair points.  d_status[b] (one
 *     et_status byte per record) and d_key_status[k] (one per key) hold the statuses; either may be NULL.
 *   Record b EQUALS key k when both are valid, their lengths (text_index differences) are equal, their body byte counts are equal
 *     and those bytes are identical -- except that a body of no bytes under a length above zero, which is how a record looks whose
 *     encode failed and which is kept raw elsewhere, equals nothing on either side (not even its like).  A length of 0 with an empty
 *     body equals a key of the same kind.  Under one table the encoder is deterministic, so for bodies exactly as this library's
 *     encoders write them (ceil(bits / 8) bytes, the pad bits zero) the join selects b exactly when
 *     et_match_packed_device(ET_MATCH_EQUAL, needle = key k's text) selects it for some k.  A hand-made body with bytes behind its
 *     last codeword, or with pad bits that are not zero, can equal a needle under ET_MATCH_EQUAL and does not equal that needle's
 *     encoder-made key here; the join never selects a record whose stored text differs from every key's.
 *   mode: 0, or ET_MATCH_NOT: the valid records that equal NO key.  n_keys == 0: nothing equals -- under ET_MATCH_NOT every valid
 *     record is selected -- and the records are still judged; the key pointers may then be NULL.
 *   d_rows[0 .. n_match) (32 bits each, 4-byte aligned, on the device) = the selected record numbers, ascending: the gather call's
 *     d_rows.  Nothing at or beyond d_rows + n_match is written.  d_rows == NULL: count only -- cap_rows is ignored, the status
 *     bytes and *res are the writing call's.  n_match > cap_rows: the call returns ET_ERR_CAP, no entry of d_rows or d_key_of_row
 *     is written, d_status and d_key_status are complete and res->n_match is the room needed.
 *   d_key_of_row (may be NULL; as large as d_rows and written only where d_rows is): d_key_of_row[i] = the LOWEST key number whose
 *     content equals record d_rows[i] -- key sets may hold duplicates, and the answer does not depend on the order in which the
 *     device inserted them.
 *   et_join_hash, et_join_table_slots (host only): the 64-bit hash of (length, n_bytes, body bytes) the table is built on -- a
 *     key's first slot is hash & (slots - 1), the next ones follow with wrap-around -- and the slots of a table for n_keys keys: a
 *     power of two, at least 2 * n_keys.  For tests that craft collisions; the hash never decides alone, every hit is confirmed by
 *     length, byte count and bytes.
 * The call's own status: ET_ERR_ARG (a null ctx, cb, res, d_bodies, d_body_index or d_text_index; with n_keys > 0 a null
 * d_key_bodies, d_key_body_index or d_key_text_index; an offset array that is not 8-byte aligned, d_rows or d_key_of_row not 4-byte
 * aligned; n_records above 0x7fffffff; n_keys above et_join_keys_max(); a mode other than 0 or ET_MATCH_NOT; d_key_of_row with
 * ET_MATCH_NOT, or with d_rows == NULL -- all checked before anything touches a device, *res untouched), ET_ERR_UNSUPPORTED (the
 * table is not complete: nothing is enqueued), ET_ERR_CAP, ET_ERR_HIP, ET_ERR_NOMEM.  n_records == 0: ET_OK, nothing enqueued,
 * *res zeroed.  One upload (64 bytes of counters), a clear of the table, four launches and one hand-over per call;
 * stream-ordered like the other packed calls -- *res is final on return, the device arrays once the ctx's stream has drained -- and
 * it may follow or precede packed, gather, match, shared-table and single-stream calls on one ctx with nothing in between and with
 * different tables: the keys may come straight from et_encode_packed_device, and d_rows may go straight into
 * et_decode_packed_gather_device, on the same ctx. */
typedef struct et_join_result {
    uint64_t n_match;                       /* rows selected -- also when the call returns ET_ERR_CAP or d_rows is NULL */
    uint64_t n_failed, first_failed;        /* records whose status is not ET_OK, the lowest of them (valid when n_failed > 0) */
    uint64_t n_keys_failed, first_key_failed;   /* the same for keys */
    int32_t first_status, first_key_status; /* et_status of record first_failed, of key first_key_failed */
} et_join_result;
size_t et_join_result_size(void);
size_t et_join_keys_max(void);              /* most keys per call: 1 << 24 */
uint64_t et_join_hash(const uint8_t *body, size_t n_bytes, uint64_t length);
size_t et_join_table_slots(size_t n_keys);
int et_join_packed_device(et_ctx *ctx, const et_codebook *cb,
                          const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                          const uint64_t *d_text_index, size_t n_records,
                          const void *d_key_bodies, size_t key_body_bytes, const uint64_t *d_key_body_index,
                          const uint64_t *d_key_text_index, size_t n_keys,
                          int mode,             /* 0, or ET_MATCH_NOT: the valid records that equal NO key (anti-join) */
                          uint32_t *d_rows, size_t cap_rows, uint32_t *d_key_of_row,
                          uint8_t *d_status, uint8_t *d_key_status, et_join_result *res);
/* Diagnostics: d_hash[b] (8-byte aligned, on the device) = et_join_hash of every valid record of a packed store as the join's
 * kernels compute it -- a lane alone, or a wavefront together for a long body; a failed record's entry is left alone.  Returns with
 * the stream drained. */
int et_selftest_join_hash(et_ctx *ctx, const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                          const uint64_t *d_text_index, size_t n, uint64_t *d_hash);

/* GROUP: which records of a packed store hold the SAME text -- SELECT DISTINCT key, GROUP BY key and COUNT(*) -- decided on the
 * compressed bytes, nothing decoded: the distinct texts in order of first appearance, how many records hold each, and the group of
 * every record.  A join of the store with itself: one build pass puts the store's own records into the join's hash table, where equal
 * records meet in one slot that keeps the lowest record number; one probe pass finds every record's slot.  (Unrelated to et_group,
 * the multi-GPU membership further down.)
 *   The store is the join call's, and a record is judged as the join judges it, from its own two pairs of offsets: ET_ERR_ARG
 *     unless body_index[b] <= body_index[b+1] <= body_bytes and text_index[b] <= text_index[b+1]; ET_ERR_UNSUPPORTED for a length
 *     above the small-stream limit.  d_status[b] (one et_status byte per record; may be NULL) holds the status.  A failed record
 *     belongs to no group, is never a first row and is counted nowhere; its d_group_of entry is ET_GROUP_NONE.  It fails alone, and
 *     no kernel reads where its pair points.
 *   Records a and b are EQUAL by the join's rule, word for word: both valid, their lengths (text_index differences) equal, their body
 *     byte counts equal and those bytes identical -- except that a body of no bytes under a length above zero, which is how a record
 *     looks whose encode failed and which is kept raw elsewhere, equals nothing, not even its like: each such record is a group of its
 *     own, with count 1.  A length of 0 with an empty body equals its like.  Under one table the encoder is deterministic, so for
 *     bodies exactly as this library's encoders write them (ceil(bits / 8) bytes, the pad bits zero) two records are in one group
 *     exactly when their stored texts are the same.  A hand-made body with bytes behind its last codeword, or with pad bits that are
 *     not zero, can equal a needle under ET_MATCH_EQUAL and is put in a group apart from the encoder-made body of the same text here;
 *     records whose stored texts differ are never in one group.
 *   The group of a valid record is the set of valid records equal to it; its REPRESENTATIVE is the lowest record number in it.
 *     Groups are numbered 0 .. n_groups - 1 by ascending representative: the order of first appearance, the same on every call.
 *   d_first_rows[0 .. n_groups) (32 bits each, 4-byte aligned, on the device) = the representatives, ascending: the d_rows that the
 *     take and gather calls consume -- take(d_first_rows) is the store of the distinct texts.  d_count[g] (may be NULL) = the members
 *     of group g; their sum is the number of valid records, and the counts are exact and the same on every call.  d_group_of[b]
 *     (may be NULL; n_records entries) = the group of record b, or ET_GROUP_NONE.  Nothing at or beyond d_first_rows + n_groups or
 *     d_count + n_groups is written.
 *   d_first_rows == NULL: count only -- cap_groups is ignored, d_status and *res are the writing call's; d_count or d_group_of given
 *     without d_first_rows is ET_ERR_ARG.  n_groups > cap_groups: the call returns ET_ERR_CAP, no entry of d_first_rows, d_count or
 *     d_group_of is written, d_status is complete and res->n_groups is the room needed.
 * The call's own status: ET_ERR_ARG (a null ctx, cb, res, d_bodies, d_body_index or d_text_index; an offset array that is not
 * 8-byte aligned; d_first_rows, d_count or d_group_of not 4-byte aligned; n_records above et_group_records_max(); d_count or
 * d_group_of with d_first_rows == NULL -- all checked before anything touches a device, *res untouched), ET_ERR_UNSUPPORTED (the table
 * is not complete: nothing is enqueued), ET_ERR_CAP, ET_ERR_HIP, ET_ERR_NOMEM.  n_records == 0: ET_OK, nothing enqueued, *res zeroed.
 * One upload (64 bytes of counters), a clear of the table (et_join_table_slots(n_records) slots), three launches and one hand-over
 * for a count-only call, behind the scan; up to two more launches behind the hand-over for a writing one.  Stream-ordered like the
 * other packed calls -- *res is final on return, the device arrays once the ctx's stream has drained -- and it may follow or precede
 * any other packed, gather, match, search, join, take, slice, field, concat, recode, number, shared-table or single-stream call on one ctx
 * with nothing in between: the store may come straight from et_field_packed_device, d_first_rows may go straight into
 * et_take_packed_device, d_group_of straight into et_number_packed_device.  It keeps the state a ctx holds between calls (the histogram
 * link, the held range) as it is.
 * Out of scope: groups in SORTED order (ORDER BY: groups come in order of first appearance); grouping a selection given by d_rows
 * (take first); grouping over several columns in one call (concat first); more than et_group_records_max() records per call; sums
 * or other aggregates over a value column (et_number_packed_device takes d_group_of for that); case-insensitive grouping (recode
 * first). */
#define ET_GROUP_NONE 0xffffffffu
typedef struct et_group_result {
    uint64_t n_groups;                      /* groups found -- also when the call returns ET_ERR_CAP or d_first_rows is NULL */
    uint64_t n_failed, first_failed;        /* records whose status is not ET_OK, the lowest of them (valid when n_failed > 0) */
    int32_t first_status;                   /* et_status of record first_failed */
    uint32_t pad;
} et_group_result;
size_t et_group_result_size(void);
size_t et_group_records_max(void);          /* most records per call: et_join_keys_max(), 1 << 24 */
int et_group_packed_device(et_ctx *ctx, const et_codebook *cb,
                           const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                           const uint64_t *d_text_index, size_t n_records,
                           uint32_t *d_first_rows, size_t cap_groups,
                           uint32_t *d_count, uint32_t *d_group_of,
                           uint8_t *d_status, et_group_result *res);

/* TAKE: a SELECTION of a packed store's records as a NEW packed store, on the device, nothing decoded and nothing encoded again: what
 * keeps the result of a match or a join compressed -- as the key set of the next join, as the store that is left when rows are
 * deleted or reordered, or as the bytes that go to another rank or a file.  Under one table a record's body is a self-contained byte
 * string, so row k of the result is the body of record r = d_rows[k] as it is, and its length is r's.  There is NO et_codebook
 * argument: the call never interprets a bit, so it works under any table, complete or not, and the new store is read under the table
 * the old one was written with.
 *   The store and d_rows are the gather call's: d_bodies, and d_body_index and d_text_index of n_records + 1 entries each, 8-byte
 *     aligned, the text offsets serving as record lengths only; d_rows[k] (n_rows of them, 32 bits, 4-byte aligned, on the device) in
 *     any order, repeats allowed.
 *   A row whose status is ET_OK: d_out[out_body_index[k], out_body_index[k+1]) holds exactly the bytes
 *     d_bodies[body_index[r], body_index[r+1]), and out_text_index[k+1] - out_text_index[k] == text_index[r+1] - text_index[r].  Both
 *     output arrays have n_rows + 1 entries (8-byte aligned, on the device) and begin with 0; the bodies lie back to back.  A body of
 *     no bytes under a length above zero (a record kept raw elsewhere) is valid and is taken as such -- no bytes, the length kept --
 *     so the new store behaves under decode, match and join as the old record did.
 *   d_status[k] (one et_status byte per ROW; may be NULL): the gather call's rule -- ET_ERR_ARG when d_rows[k] >= n_records, and unless
 *     body_index[r] <= body_index[r+1] <= body_bytes and text_index[r] <= text_index[r+1]; ET_ERR_UNSUPPORTED for a length above the
 *     small-stream limit -- and one more: ET_ERR_UNSUPPORTED for a body of more than 4 * et_batch_small_max() bytes, which no record
 *     of codes up to 32 bits has.  A failed row becomes an EMPTY record of the new store: no bytes, length 0.  A row fails alone, no
 *     kernel reads where a bad pair points, and a bad record that no row selects does not matter.  In *res, n_failed, first_failed and
 *     first_status are about ROWS (positions k).
 *   Nothing outside [d_out, d_out + out_body_index[n_rows]) is written, at any alignment of d_out and of d_bodies.
 *   d_out == NULL: sizes only -- both output arrays, d_status and *res are the writing call's; cap is ignored.
 *   out_body_index[n_rows] > cap: the call returns ET_ERR_CAP, not a byte of d_out is written; both output arrays and d_status are
 *     complete and res->out_bytes is the room needed.
 * Out of scope: compaction in place -- [d_out, d_out + cap) may not overlap [d_bodies, d_bodies + body_bytes) --, taking from several
 * stores in one call, and records above the limits named above.
 * The call's own status: ET_ERR_ARG (a null ctx, res, d_bodies, d_body_index, d_text_index, d_rows, d_out_body_index or
 * d_out_text_index; an offset array that is not 8-byte aligned, d_rows not 4-byte aligned; n_records or n_rows above 0x7fffffff; d_out
 * overlapping d_bodies -- all checked before anything touches a device, *res untouched), ET_ERR_CAP, ET_ERR_HIP, ET_ERR_NOMEM.
 * n_rows == 0: ET_OK, nothing enqueued, *res zeroed.  One upload (64 bytes of counters), three launches and one hand-over per call;
 * stream-ordered like the other packed calls -- *res is final on return, the device arrays once the ctx's stream has drained -- and it
 * may follow or precede packed, gather, match, join, shared-table and single-stream calls on one ctx with nothing in between: d_rows
 * may come straight from et_match_packed_device or et_join_packed_device, and the outputs may go straight into et_join_packed_device
 * (as the key set), et_decode_packed_device or et_decode_packed_gather_device. */
typedef struct et_take_result {
    uint64_t out_bytes;      /* out_body_index[n_rows]: bytes the taken bodies need -- also when the call returns ET_ERR_CAP or d_out is NULL */
    uint64_t text_bytes;     /* out_text_index[n_rows]: the sum of the taken records' lengths */
    uint64_t n_failed, first_failed;   /* rows whose status is not ET_OK, the lowest of them (valid when n_failed > 0) */
    int32_t first_status;    /* et_status of row first_failed */
    uint32_t pad;
} et_take_result;
size_t et_take_result_size(void);
int et_take_packed_device(et_ctx *ctx,
                          const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                          const uint64_t *d_text_index, size_t n_records,
                          const uint32_t *d_rows, size_t n_rows,
                          void *d_out, size_t cap, uint64_t *d_out_body_index, uint64_t *d_out_text_index,
                          uint8_t *d_status, et_take_result *res);

/* SLICE: a PART of each selected record as a NEW packed store, on the device, nothing decoded and nothing encoded again --
 * SUBSTR(key, a, n), LEFT(key, n), "the value behind user= up to the next ;" -- and what consumes the search call's d_pos: search ->
 * slice -> join -> gather runs on one ctx with nothing in between.  Under one complete prefix-free table symbols [i, j) of a record
 * are the bits from the boundary of codeword i to the boundary of codeword j, so the body the encoder would write for the substring
 * is that run of bits shifted to bit 7 of a byte, the last byte padded with zeros: the search's walk finds the two boundaries, a
 * bit-shifting version of the take's copy writes the result.
 *   The store, d_rows (any order, repeats allowed), d_status (one et_status byte per ROW; may be NULL) and the judgement of a row are
 *     the take call's: ET_ERR_ARG when d_rows[k] >= n_records and unless body_index[r] <= body_index[r+1] <= body_bytes and
 *     text_index[r] <= text_index[r+1]; ET_ERR_UNSUPPORTED for a length above the small-stream limit and for a body above
 *     4 * et_batch_small_max() bytes.  A failed row becomes an EMPTY record of the new store (no bytes, length 0), fails alone, and no
 *     kernel reads where a bad pair points.  d_rows == NULL: row k is record k, and n_rows must equal n_records.
 *   d_first[k], d_count[k] (32 bits each, 4-byte aligned, on the device; either may be NULL: then the scalar `first` or `count` holds
 *     for every row; with the pointer the scalar is ignored): where row k's slice begins and how many symbols it has at most.
 *     ET_SLICE_TO_END as a count: to the end.  d_first may be the search call's d_pos, or that plus the needle's length.  (et_number_packed_device
 *     takes the same ask and reads the slice as an integer instead of storing it.)
 *   text_b is the stored text of record r = d_rows[k] as every packed call defines it: the first min(length_r, codewords that end
 *     inside its body) symbols.  Row k of the result is s = text_b[first : first + count], clamped as Python clamps a slice
 *     (first >= len(text_b): the empty record; first + count does not wrap).  0 <= stop <= 255: s is cut in front of the first
 *     occurrence of byte `stop` in it (s[: s.find(stop)] when there is one); a stop byte without a code occurs in no record and cuts
 *     nothing; ET_SLICE_NO_STOP: nothing cuts.
 *   d_out[out_body_index[k], out_body_index[k+1]) holds exactly the bytes et_encode_packed_device writes for s under cb --
 *     ceil(bits / 8) bytes, MSB-first from bit 7, the pad bits zero, also from a hand-made source body whose own pad bits are set: the
 *     copied bits are codewords, the pad is masked and not copied -- and out_text_index[k+1] - out_text_index[k] == len(s).  Both
 *     output arrays have n_rows + 1 entries (8-byte aligned, on the device) and begin with 0; the bodies lie back to back.  A body of
 *     no bytes under a length above zero (a record kept raw elsewhere) has the empty stored text and slices to the empty record with
 *     length 0 -- UNLIKE the take call, which keeps such a record's length: a slice's length is the symbols its body holds.
 *   Nothing outside [d_out, d_out + out_body_index[n_rows]) is written, at any alignment of d_out and of d_bodies.
 *   d_out == NULL: sizes only -- both output arrays, d_status and *res are the writing call's; cap is ignored.
 *   out_body_index[n_rows] > cap: the call returns ET_ERR_CAP, not a byte of d_out is written; both output arrays and d_status are
 *     complete and res->out_bytes is the room needed.  res->text_bytes is the sum of the slices' lengths.
 *   et_slice_lane_bytes(): a body of which the slice's end can reach up to this many bytes (4 bytes per symbol in front of the end, and
 *     8: a LEFT of a few symbols reaches little of a long body) is walked by one lane, a longer one by a workgroup -- for tests that
 *     want rows on both sides; the answer does not depend on it.
 * Out of scope: negative or from-the-end indices (the caller has text_index on the device for that); slicing in place -- [d_out,
 * d_out + cap) may not overlap [d_bodies, d_bodies + body_bytes) --; several stores per call; records above the limits named above.
 * The call's own status: ET_ERR_ARG (a null ctx, cb, res, d_bodies, d_body_index, d_text_index, d_out_body_index or
 * d_out_text_index; an offset array that is not 8-byte aligned; d_rows, d_first or d_count not 4-byte aligned; n_records or n_rows
 * above 0x7fffffff; d_rows == NULL with n_rows != n_records; d_out overlapping d_bodies; a stop outside [-1, 255] -- all checked
 * before anything touches a device, *res untouched), ET_ERR_UNSUPPORTED (the table is not complete: nothing is enqueued), ET_ERR_CAP,
 * ET_ERR_HIP, ET_ERR_NOMEM.  n_rows == 0: ET_OK, nothing enqueued, *res zeroed.  One upload (the sorted codes and zeroed counters,
 * 2.1 KiB), four launches and one hand-over per call; stream-ordered like the other packed calls -- *res is final on return, the
 * device arrays once the ctx's stream has drained -- and it may follow or precede any of them on one ctx with nothing in between. */
#define ET_SLICE_TO_END 0xffffffffu
#define ET_SLICE_NO_STOP (-1)
size_t et_slice_lane_bytes(void);           /* a reach (min(body bytes, 4 * slice end + 8)) up to this is walked by one lane */
int et_slice_packed_device(et_ctx *ctx, const et_codebook *cb,
                           const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                           const uint64_t *d_text_index, size_t n_records,
                           const uint32_t *d_rows, size_t n_rows,
                           const uint32_t *d_first, uint32_t first,
                           const uint32_t *d_count, uint32_t count,
                           int stop,
                           void *d_out, size_t cap, uint64_t *d_out_body_index, uint64_t *d_out_text_index,
                           uint8_t *d_status, et_take_result *res);

/* FIELD: the k-th DELIMITED FIELD of each selected record as a NEW packed store, on the device, nothing decoded and nothing encoded
 * again -- SPLIT_PART(line, ',', k), column k of a CSV row, the third token of a log line.  Under one complete prefix-free table a
 * delimiter is a codeword boundary whose codeword decodes to `delim`, so a run of fields is the run of bits between two such
 * boundaries: the slice's walk counts the delimiters it steps over, the slice's scan and bit-shifting copy write the result.
 *   The store, d_rows, d_status, the judgement of a row and what a failed row becomes are the slice call's.
 *   d_field[k], d_n_fields[k] (32 bits each, 4-byte aligned, on the device; either may be NULL: then the scalar `field` or `n_fields`
 *     holds for every row; with the pointer the scalar is ignored): row k's first field, counted from 0, and how many consecutive
 *     fields it takes, the delimiters between them kept.  ET_FIELD_TO_END as n_fields: every field from `field` on.
 *   text_b is the stored text of record r = d_rows[k] as every packed call defines it: the first min(length_r, codewords that end
 *     inside its body) symbols -- a codeword at or behind length_r is no symbol and never a delimiter, nor is what the pad bits read
 *     as.  With parts = text_b.split(delim) as Python splits: field >= len(parts): the field is ABSENT -- row k is the empty record,
 *     d_pos[k] = ET_FIELD_ABSENT, the row's status stays ET_OK (SQL's SPLIT_PART).  Otherwise row k is
 *     delim.join(parts[field : field + n_fields]), field + n_fields taken in 64 bits and clamped as Python clamps a slice;
 *     n_fields == 0 is the empty record, present; d_pos[k] = the symbol of text_b at which parts[field] begins.  The empty stored
 *     text -- also that of a body of no bytes under a length above zero -- has one empty field 0 at position 0.  A delim without a
 *     code occurs in no record: every record is one field.
 *   d_pos (n_rows entries of 32 bits, 4-byte aligned, on the device; may be NULL): as above; ET_FIELD_ABSENT for a failed row too.
 *     It may be the slice call's d_first, or the number call's.
 *   d_out, both output arrays (n_rows + 1 entries, the first 0), the bytes -- exactly what et_encode_packed_device writes for the
 *     result, pad bits zero whatever the source's are --, d_out == NULL (sizes only; d_pos is written) and ET_ERR_CAP (no byte of d_out
 *     written; both arrays, d_status and d_pos complete, res->out_bytes the room needed) are the slice call's.
 *   et_field_lane_bytes(): a body (min(body bytes, 4 * length + 8)) up to this many bytes is walked by one lane, a longer one by a
 *     workgroup -- for tests that want rows on both sides; the answer does not depend on it.
 * Out of scope: several fields of a row into several output rows in one walk; multi-byte or regex delimiters; quoting and escapes;
 * fields counted from the end; a count of absent rows in *res; cutting in place; several stores per call; records above the slice
 * call's limits.
 * The call's own status: ET_ERR_ARG (the slice call's argument errors; delim outside [0, 255]; d_field, d_n_fields or d_pos not
 * 4-byte aligned -- all checked before anything touches a device, *res untouched), ET_ERR_UNSUPPORTED (the table is not complete:
 * nothing is enqueued), ET_ERR_CAP, ET_ERR_HIP, ET_ERR_NOMEM.  n_rows == 0: ET_OK, nothing enqueued, *res zeroed.  One upload (the
 * sorted codes and zeroed counters, 2.1 KiB), four launches and one hand-over per call; stream-ordered like the other packed calls --
 * *res is final on return, the device arrays once the ctx's stream has drained -- and it may follow or precede any of them on one
 * ctx with nothing in between. */
#define ET_FIELD_TO_END 0xffffffffu
#define ET_FIELD_ABSENT 0xffffffffu
size_t et_field_lane_bytes(void);           /* a body (min(body bytes, 4 * length + 8)) up to this is walked by one lane */
int et_field_packed_device(et_ctx *ctx, const et_codebook *cb,
                           const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                           const uint64_t *d_text_index, size_t n_records,
                           const uint32_t *d_rows, size_t n_rows,
                           const uint32_t *d_field, uint32_t field,
                           const uint32_t *d_n_fields, uint32_t n_fields,
                           int delim,
                           void *d_out, size_t cap, uint64_t *d_out_body_index, uint64_t *d_out_text_index,
                           uint32_t *d_pos,
                           uint8_t *d_status, et_take_result *res);

/* CONCAT: ROW-WISE STRING CONCATENATION as a NEW packed store, on the device, nothing decoded and nothing encoded again --
 * last || ',' || first as a join key, id re-keyed as user=<id>, columns 0 and 3 of a CSV line put back together: the one call that
 * builds a record from parts.  Under one complete prefix-free table the body the encoder writes for x + y is the bits of x followed
 * by the bits of y, so a row is three runs of bits -- a stored text's, a literal's, a stored text's -- laid end to end: field -> concat -> join runs on
 * one ctx with no text in between.  (Appending stores, UNION ALL, is a different thing and not this call's.)
 *   Row k of the new store is text(A[rows_a[k]]) + sep + text(B[rows_b[k]]), text() the stored text as every packed call defines it:
 *     the first min(length, codewords that end inside the body) symbols.  Both stores are the take call's, under the one table cb; A
 *     and B may be the same store.  Either side may be ABSENT: d_x_bodies == NULL, with n_x == 0, x_body_bytes == 0 and null offset
 *     arrays (its d_rows is not looked at); it contributes nothing to any row.  An absent left side with a literal prefixes every
 *     record, an absent right side suffixes it.  At least one side is present.
 *   d_rows_a[k], d_rows_b[k] (32 bits each, 4-byte aligned, on the device; any order, repeats allowed): the record of that side in
 *     row k.  d_rows_x == NULL: row k is record k of that side, and n_rows must equal n_x.
 *   sep (HOST memory, sep_len <= et_concat_sep_max() bytes; may be empty): the literal between the two, encoded once on the host by
 *     et_encode_pattern.
 *   How the pieces are laid: three runs of bits, end to end.  LEFT: its stored text's bits, found by the slice's walk from symbol 0
 *     to the end, nothing cutting; the pad behind its last codeword is dropped, set or not.  LITERAL: et_encode_pattern's bits.
 *     RIGHT: its stored text's bits, found the same way -- NOT its body as the take would take it: 8 * bytes bits behind a run that
 *     ends inside a byte would push its pad into a byte the encoder does not write, and a length that does not end its text (a body
 *     cut short, a record kept raw) would let the row's own pad read as symbols.  A record kept raw (no bytes, a length above 0) has
 *     the empty stored text on either side, as in the slice.  Hence, for EVERY input: d_out[out_body_index[k], out_body_index[k+1])
 *     holds exactly the bytes et_encode_packed_device writes for the concatenation of the three stored texts under cb --
 *     ceil(bits / 8) bytes, MSB-first from bit 7, the pad bits zero whatever the sources' are -- and the new record's stored text is
 *     that concatenation.
 *   Sizes: out_text_index advances by symbols(A) + sep_len + symbols(B) per row, out_body_index by
 *     ceil((bits(A) + sep_bits + bits(B)) / 8), symbols() and bits() the stored text's.  Both arrays have n_rows + 1 entries (8-byte
 *     aligned, on the device) and begin with 0; the bodies lie back to back.
 *   d_status[k] (one et_status byte per ROW; may be NULL): each side's record is judged as the take call judges a row (ET_ERR_ARG
 *     for a number beyond that store or a bad pair of offsets, ET_ERR_UNSUPPORTED for a length above the small-stream limit or a body
 *     above 4 * et_batch_small_max() bytes); the row's status is the left record's if that is not ET_OK, else the right's, else
 *     ET_ERR_UNSUPPORTED when the new length exceeds et_batch_small_max() -- the output stays a store every packed call accepts.  A
 *     failed row is the EMPTY record, fails alone and is tallied once; no byte is read where its pairs point.
 *   *res is the take call's, as the slice reports it: out_bytes, text_bytes (the sum of the new lengths), n_failed, first_failed,
 *     first_status.  Nothing outside [d_out, d_out + out_body_index[n_rows]) is written, at any alignment of d_out and of the bodies.
 *     d_out == NULL: sizes only -- both output arrays, d_status and *res are the writing call's; cap is ignored.
 *     out_body_index[n_rows] > cap: ET_ERR_CAP, not a byte of d_out is written; both output arrays and d_status are complete and
 *     res->out_bytes is the room needed.
 *   et_concat_lane_bytes(): a body of either side (min(body bytes, 4 * length + 8)) up to this many bytes is walked by one lane, a
 *     longer one by a workgroup (the slice's threshold, kept) -- for tests that want rows on both sides; the answer does not depend on it.
 * Out of scope: more than two store sides per call (chain the call); per-row literals; appending stores (UNION ALL); concatenating in
 * place -- [d_out, d_out + cap) may overlap neither side's bodies --; records above the limits named above.
 * The call's own status: ET_ERR_ARG (a null ctx, cb, res, d_out_body_index or d_out_text_index; both sides absent; an absent side with
 * records, bytes or offset arrays; a present side with a null offset array, an offset array that is not 8-byte aligned, d_rows not
 * 4-byte aligned, n above 0x7fffffff, or d_rows == NULL with n_rows != n; n_rows above 0x7fffffff; d_out overlapping either side's
 * bodies; sep_len > et_concat_sep_max(); sep == NULL with sep_len > 0 -- all checked before anything touches a device, *res
 * untouched), ET_ERR_UNSUPPORTED (the table is not complete, or a byte of the literal has no code: nothing is enqueued), ET_ERR_CAP,
 * ET_ERR_HIP, ET_ERR_NOMEM.  n_rows == 0: ET_OK, nothing enqueued, *res zeroed.  One upload (the sorted codes, zeroed counters and the
 * encoded literal, 3.1 KiB at most), four launches -- three without d_out -- and one hand-over per call; stream-ordered like the other packed calls -- *res is final on return, the device arrays once the ctx's stream
 * has drained -- and it may follow or precede any of them on one ctx with nothing in between. */
size_t et_concat_sep_max(void);             /* 256, the search's needle limit: the encoded literal is at most 1 KiB */
size_t et_concat_lane_bytes(void);          /* a body (min(body bytes, 4 * length + 8)) up to this is walked by one lane */
int et_concat_packed_device(et_ctx *ctx, const et_codebook *cb,
                            const void *d_a_bodies, size_t a_body_bytes, const uint64_t *d_a_body_index,
                            const uint64_t *d_a_text_index, size_t n_a, const uint32_t *d_rows_a,
                            const uint8_t *sep, size_t sep_len,
                            const void *d_b_bodies, size_t b_body_bytes, const uint64_t *d_b_body_index,
                            const uint64_t *d_b_text_index, size_t n_b, const uint32_t *d_rows_b,
                            size_t n_rows,
                            void *d_out, size_t cap, uint64_t *d_out_body_index, uint64_t *d_out_text_index,
                            uint8_t *d_status, et_take_result *res);

/* RECODE: A STORE UNDER A SECOND TABLE, THROUGH A BYTE MAP (re-tabling, UPPER, LOWER, TRANSLATE, stripping characters) as a NEW packed
 * store, on the device, no text in between: the codewords of a record are walked under cb_in and for each symbol s the codeword of
 * map[s] under cb_out is emitted, or nothing where the byte is dropped.  The call that lifts "one table" from the others: a key set
 * written under yesterday's table is recoded and joined against today's store, two stores are brought under one table and
 * concatenated, and case-insensitive =, LIKE and IN are match / search / join on the store recoded through an ASCII upper-casing map
 * against the upper-cased needle -- all on one ctx with nothing in between.
 *   The store, d_rows (any order, repeats allowed; NULL: row k is record k, and n_rows must equal n_records) and d_status are the
 *     slice call's, and a row is judged as the slice call judges it: ET_ERR_ARG for a number beyond the store or a bad pair of
 *     offsets, ET_ERR_UNSUPPORTED for a length above the small-stream limit or a body above 4 * et_batch_small_max() bytes.  A failed
 *     row is the EMPTY record of the new store (no bytes, length 0), fails alone and is tallied once; nothing is read where its
 *     offsets point.
 *   text_r is the stored text of record r under cb_in as every packed call defines it: the first min(length_r, codewords that end
 *     inside its body) symbols.  A codeword at or behind length_r is no symbol, and neither is whatever the pad bits read as.
 *   map (HOST memory, 256 entries; NULL: the identity): map[c] is a byte value in [0, 255], or ET_RECODE_DROP to delete that byte.
 *   Row k is t = bytes(map[c] for c in text_r if map[c] != DROP), r = rows[k], and d_out[out_body_index[k], out_body_index[k+1])
 *     holds exactly the bytes et_encode_packed_device writes for t under cb_out -- ceil(bits / 8) bytes, MSB-first from bit 7, the pad
 *     bits zero whatever the source's are -- with out_text_index[k+1] - out_text_index[k] == len(t).  A body of no bytes under a
 *     length above zero (a record kept raw elsewhere) has the empty stored text and recodes to the empty record, length 0: the
 *     slice's rule, not the take's.
 *   A kept byte map[c] without a code in cb_out fails the row with ET_ERR_UNSUPPORTED (the encoder's status for a byte without a
 *     code); the row is the empty record.  Only symbols of the stored text can fail a row: the same byte behind the length, or in the
 *     pad bits, or dropped by the map, does not.
 *   Both tables must be complete (et_codebook_is_complete).  cb_out may be cb_in: a pure TRANSLATE.  The identity map with cb_out ==
 *     cb_in is NOT short-cut to the take: it runs, and NORMALISES the store -- pad bits cleared, lengths cut to what the bodies hold.
 *     A new record has at most as many symbols as the old and at most 4 bytes per symbol: the output is a store every packed call
 *     accepts.
 *   Both output arrays have n_rows + 1 entries (8-byte aligned, on the device) and begin with 0; the bodies lie back to back.
 *   *res is the take call's: out_bytes, text_bytes (the sum of the new lengths), n_failed, first_failed, first_status.  Nothing
 *     outside [d_out, d_out + out_body_index[n_rows]) is written, at any alignment of d_out and of the bodies.
 *     d_out == NULL: sizes only -- both output arrays, d_status and *res are the writing call's; cap is ignored.
 *     out_body_index[n_rows] > cap: ET_ERR_CAP, not a byte of d_out is written; both output arrays and d_status are complete and
 *     res->out_bytes is the room needed.
 *   et_recode_lane_bytes(): a body (min(body bytes, 4 * length + 8)) up to this many bytes is walked by one lane, a longer one by a
 *     workgroup (the search's threshold, kept) -- for tests that want rows on both sides; the answer does not depend on it.
 * Out of scope: per-row maps; one byte to several, or several to one (REPLACE of substrings); UTF-8 case folding; recoding in place
 * -- [d_out, d_out + cap) may not overlap the bodies --; several stores per call; the symbol histogram of a store taken on its
 * compressed bytes, which a caller would want in order to build the best cb_out: until then the caller decodes and uses
 * et_histogram_device.
 * The call's own status: ET_ERR_ARG (a null ctx, cb_in, cb_out, res, d_bodies or offset array; an offset array that is not 8-byte
 * aligned; d_rows not 4-byte aligned; n_records or n_rows above 0x7fffffff; d_rows == NULL with n_rows != n_records; d_out
 * overlapping the bodies; a map entry that is neither a byte nor ET_RECODE_DROP -- all checked before anything touches a device,
 * *res untouched), ET_ERR_UNSUPPORTED (a table is not complete: nothing is enqueued), ET_ERR_CAP, ET_ERR_HIP, ET_ERR_NOMEM.
 * n_rows == 0: ET_OK, nothing enqueued, *res zeroed.  One upload (the sorted codes of cb_in, zeroed counters and the output table --
 * map composed with cb_out on the host, indexed by the input symbol: 4.1 KiB), five launches -- plan, long rows, scan, the lanes'
 * write, the workgroups' write; three without d_out -- and one hand-over per call; stream-ordered like the other packed calls --
 * *res is final on return, the device arrays once the ctx's stream has drained -- and it may follow or precede any of them on one
 * ctx with nothing in between. */
#define ET_RECODE_DROP (-1)
size_t et_recode_lane_bytes(void);          /* a body (min(body bytes, 4 * length + 8)) up to this is walked by one lane */
int et_recode_packed_device(et_ctx *ctx, const et_codebook *cb_in, const et_codebook *cb_out,
                            const int16_t *map,                     /* HOST, 256 entries, or NULL = identity */
                            const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                            const uint64_t *d_text_index, size_t n_records,
                            const uint32_t *d_rows, size_t n_rows,
                            void *d_out, size_t cap, uint64_t *d_out_body_index, uint64_t *d_out_text_index,
                            uint8_t *d_status, et_take_result *res);

/* NUMBER: a part of each selected record READ AS AN INTEGER, on the device, nothing decoded -- CAST(SPLIT_PART(line, ',', 3) AS
 * BIGINT), "the number behind user= up to the next ;" -- and SUM, COUNT, MIN and MAX of those values per group: SELECT key,
 * SUM(amount) ... GROUP BY key runs as field -> group -> number on one ctx with nothing in between, and what consumes the field
 * call's and the search call's d_pos as a number.  The slice's walk finds the value; what it notes is not two bit positions but the
 * digits themselves, and the output is one word per row, not a new store.
 *   The store, d_rows (NULL: row k is record k, and n_rows must equal n_records), d_first / first, d_count / count, stop, d_status
 *     (one et_status byte per ROW; may be NULL) and the judgement of a row are the slice call's, word for word.  Row k's text is
 *     s = text_b[first : first + count], clamped as Python clamps a slice, first + count not wrapping, cut in front of the first
 *     `stop` byte in it; text_b is the stored text of record r = d_rows[k] as every packed call defines it: a codeword at or behind
 *     the record's length is no symbol, what the pad bits read as is no symbol, and a body of no bytes under a length above zero (a
 *     record kept raw elsewhere) has the empty stored text.
 *   The grammar is [+-]?[0-9]+ over the WHOLE of s, ASCII, nothing else.  d_kind[k] (one byte per row; may be NULL):
 *     ET_NUMBER_OK     s is of the grammar and lies in [-2^63, 2^63 - 1]
 *     ET_NUMBER_EMPTY  s is empty: SQL's NULL -- and the kind of a failed row
 *     ET_NUMBER_BAD    s is not of the grammar, or has more than et_number_symbols_max() = 32 symbols: 19 digits and a sign are what
 *                      int64 needs, the rest is room for leading zeros
 *     ET_NUMBER_RANGE  s is of the grammar, within 32 symbols, and lies outside [-2^63, 2^63 - 1]; the magnitude saturates and never
 *                      wraps: "1" followed by 31 zeros is RANGE, "-9223372036854775808" is OK
 *     d_values[k] (int64, 8-byte aligned, n_rows entries; may be NULL) = the value for ET_NUMBER_OK, 0 otherwise.
 *   The aggregates are asked for by passing any of d_sum (int64), d_n (uint64), d_min, d_max (int64): n_groups entries each, 8-byte
 *     aligned, on the device, each may be NULL.  d_group_of[k] (32 bits, 4-byte aligned, n_rows entries) is the group of ROW k -- with
 *     d_rows == NULL the group call's d_group_of as it is; NULL: every row is in group 0, and n_groups must be 1.  ET_GROUP_NONE
 *     skips the row; any other value >= n_groups fails the row alone with ET_ERR_ARG.  The call initialises the entries itself -- sum
 *     0, n 0, min INT64_MAX, max INT64_MIN: what a group without an OK row keeps -- and folds in every ET_NUMBER_OK row.  d_sum wraps
 *     modulo 2^64.  Integer adds, min and max commute: every output is exact and the same on every call.
 *   A failed row is ET_NUMBER_EMPTY with value 0, is folded nowhere and is counted in res->n_failed ONLY; it fails alone, and no
 *     kernel reads where a bad pair points.  res->n_ok + n_empty + n_bad + n_range + n_failed == n_rows.
 *   Every output pointer NULL: the call only counts -- d_status and *res are the writing call's.
 *   There is no ET_ERR_CAP: every output has a size the caller knows.  Nothing outside the n_rows entries of d_values, d_kind and
 *     d_status and the n_groups entries of the aggregates is written.
 *   et_number_lane_bytes(): a reach (min(body bytes, 4 * slice end + 8)) up to this many bytes is walked by one lane, a longer one by
 *     a workgroup -- the slice's threshold, kept -- for tests that want rows on both sides; the answer does not depend on it.
 * Out of scope: whitespace, hex, floats, exponents and thousands separators; several numbers per row; values wider than 64 bits; AVG
 * (it is sum / n); per-row stop bytes.
 * The call's own status: ET_ERR_ARG (the slice call's argument errors, in its order: a null ctx, cb, res, d_bodies, d_body_index or
 * d_text_index; an offset array that is not 8-byte aligned; d_rows, d_first or d_count not 4-byte aligned; n_records or n_rows above
 * 0x7fffffff; d_rows == NULL with n_rows != n_records; a stop outside [-1, 255]; then d_values or an aggregate array not 8-byte
 * aligned; d_group_of not 4-byte aligned; d_group_of without an aggregate output; an aggregate output with n_groups == 0; n_groups
 * above 0x7fffffff; an aggregate output without d_group_of and n_groups != 1 -- all checked before anything touches a device, *res
 * untouched), ET_ERR_UNSUPPORTED (the table is not complete: nothing is enqueued), ET_ERR_HIP, ET_ERR_NOMEM.  n_rows == 0: ET_OK,
 * nothing enqueued, *res zeroed -- and the aggregates are NOT initialised either.  One upload (the slice's: the sorted codes and
 * zeroed counters, 2.1 KiB), the fill of the aggregates that were asked for, three launches -- plan, long rows, fold -- and one
 * hand-over per call, behind the fold; stream-ordered like the other packed calls -- *res is final on return, the device arrays once
 * the ctx's stream has drained -- and it may follow or precede any of them on one ctx with nothing in between: d_first may come
 * straight from et_field_packed_device or et_search_packed_device, d_group_of from et_group_packed_device.  It keeps the state a ctx
 * holds between calls (the histogram link, the held range) as it is. */
#define ET_NUMBER_OK 0
#define ET_NUMBER_EMPTY 1
#define ET_NUMBER_BAD 2
#define ET_NUMBER_RANGE 3
typedef struct et_number_result {
    uint64_t n_ok, n_empty, n_bad, n_range; /* rows of each kind; a failed row is in none of them */
    uint64_t n_failed, first_failed;        /* rows whose status is not ET_OK, the lowest of them (valid when n_failed > 0) */
    int32_t first_status;                   /* et_status of row first_failed */
    uint32_t pad;
} et_number_result;
size_t et_number_result_size(void);
size_t et_number_symbols_max(void);         /* most symbols of a number: 32 */
size_t et_number_lane_bytes(void);          /* a reach (min(body bytes, 4 * slice end + 8)) up to this is walked by one lane */
int et_number_packed_device(et_ctx *ctx, const et_codebook *cb,
                            const void *d_bodies, size_t body_bytes, const uint64_t *d_body_index,
                            const uint64_t *d_text_index, size_t n_records,
                            const uint32_t *d_rows, size_t n_rows,
                            const uint32_t *d_first, uint32_t first,
                            const uint32_t *d_count, uint32_t count,
                            int stop,
                            int64_t *d_values, uint8_t *d_kind,
                            const uint32_t *d_group_of, size_t n_groups,
                            int64_t *d_sum, uint64_t *d_n, int64_t *d_min, int64_t *d_max,
                            uint8_t *d_status, et_number_result *res);

/* ---- staged entry points (sharded multi-GPU encode, tests) ------------------------ */
/* encode.zig:43-47 on the GPU: 256 x u64 counts of d_text[0..n) into d_hist (device).
 * Also leaves per-tile histograms in the ctx for a following et_encode_body_device
 * on the SAME (d_text, n). */
int et_histogram_device(et_ctx *ctx, const void *d_text, size_t n, void *d_hist256_u64);
/* The same counts on the HOST: the reduction stores them into pinned host memory as it stores them on the device, so
 * this only waits for that histogram (a poll, no copy command) and copies 2 KiB.  After it the shard encode that
 * follows needs no et_histogram_on_host.  et_histogram_device may be given d_hist = NULL when only the host wants
 * the counts; et_histogram_device_ptr: where the ctx itself keeps them on the device (valid until its next
 * histogram), e.g. as the send buffer of a collective.  ET_ERR_ARG unless a histogram of this ctx is current. */
int et_histogram_host(et_ctx *ctx, uint64_t counts[256]);
int et_histogram_device_ptr(et_ctx *ctx, const void **d_hist256_u64);
/* A caller that already holds the counts et_histogram_device produced for (d_text, n) on the host
 * (a sharded encode reads them back for the exchange anyway) hands them over, and the shard encode
 * that follows does not copy them from the device again.  ET_ERR_ARG unless a histogram of this ctx
 * is current.  The counts must be the ones the device holds. */
int et_histogram_on_host(et_ctx *ctx, const uint64_t counts[256]);

/* encode.zig:54-214 + queue.zig:9-43 on the host: sort, two-queue tree, codes.
 * Bit-exact including the u8 book_index saturation (256 distinct symbols), the u32
 * path truncation and single-symbol inputs.  ET_ERR_EMPTY when every count is 0. */
int et_build_codebook(const uint64_t hist[256], et_codebook *cb);

/* encode.zig:259-299: magic, version, D, low 32 bits of text_len, bit-packed
 * dictionary, zero pad to a byte.  At most 4631 bytes. */
int et_write_header(const et_codebook *cb, uint64_t text_len,
                    uint8_t *out, size_t cap, size_t *header_len);

/* Sum over s of hist[s] * length[s]: the body bit count of a shard, from its local
 * histogram alone (no data pass). */
int et_codebook_bits(const et_codebook *cb, const uint64_t hist[256], uint64_t *bits);

/* The host step of a sharded encode in one call: hists = world rows of 256 local counts (the
 * all-gathered histograms, row r = shard r).  Their sum is the stream's histogram (encode.zig:43-47)
 * -> code table, header (text_len = the sum of all counts), and start_bits[0..world]: shard r's body
 * occupies file bits [start_bits[r], start_bits[r+1]), start_bits[0] = 8 * header_len.  Every rank
 * computes the same plan from the same rows.  ET_ERR_EMPTY when every count is 0. */
int et_plan_shards(const uint64_t *hists, uint32_t world, et_codebook *cb, uint8_t *header, size_t header_cap,
                   size_t *header_len, uint64_t *start_bits);

/* encode.zig:303-315 on the GPU for one shard: pack the codes of d_text[0..n) into
 * d_out as a MSB-first bitstream whose first bit lands at bit `start_bit` of d_out
 * (d_out 4-byte aligned).  Every 32-bit word the shard touches is fully overwritten
 * (bits outside [start_bit, *end_bit) in the first/last word become 0), so adjacent
 * shards are concatenated by OR-ing their boundary bytes.  Requires the preceding
 * et_histogram_device on the same (d_text, n).
 * d_out is the word that holds bit 0, whatever start_bit is: the words touched are start_bit / 32 .. (*end_bit + 31) / 32 - 1,
 * cap_bytes is measured from d_out and must reach the end of the last one (else ET_ERR_CAP, nothing written), and the
 * words in front of start_bit / 32 are left alone.  An EMPTY shard (n = 0, or only symbols without a codeword) still owns the
 * word its start bit lies in: it zeroes word start_bit / 32, needs cap_bytes >= (start_bit / 32 + 1) * 4, and *end_bit == start_bit. */
int et_encode_body_device(et_ctx *ctx, const et_codebook *cb, const void *d_text, size_t n,
                          void *d_out, size_t cap_bytes, uint64_t start_bit, uint64_t *end_bit);

/* Same, for the shard that also carries the file header (rank 0): header[0..header_len)
 * is written to d_out[0..header_len) and the body starts right after it
 * (start bit = 8 * header_len, encode.zig:299-303). */
int et_encode_head_shard_device(et_ctx *ctx, const et_codebook *cb, const void *d_text, size_t n,
                                void *d_out, size_t cap_bytes, const uint8_t *header, size_t header_len,
                                uint64_t *end_bit);

/* decode.zig:34-141 on the host: D, body length, dictionary.  *body_offset is the
 * byte offset of the body inside `compressed` (decode.zig:156: 5 + global_pos). */
int et_parse_header(const uint8_t *compressed, size_t len, et_codebook *cb,
                    uint64_t *n_symbols, size_t *body_offset);

/* decode.zig:143-203 on the GPU: decode up to n_symbols symbols from the bitstream
 * d_body[0..body_bytes) beginning at bit `start_bit` (< 8) of d_body.  `cb` is any prefix-free table with codes of
 * up to 32 bits.  A bit pattern that is no symbol's code cannot occur in a stream of the table's own encoder; in a
 * corrupted one it decodes as byte 0 -- or, for tables too sparse for the tree walk (more than 255 internal nodes),
 * is passed over one bit at a time; the reference spins there (quirk Q6).  A table the tree walk can hold is decoded
 * bit by bit, too, whenever the tree walk is not what decodes it: after its sweep has given up on the stream (blocks
 * that do not synchronise), and from the start for a nearly fixed-length code -- the whole stream then follows that
 * one rule, the synchronisation and the write alike.  Only hand-made tables leave such patterns at all: an encoder's
 * tree is full. */
int et_decode_body_device(et_ctx *ctx, const et_codebook *cb, const void *d_body,
                          size_t body_bytes, uint32_t start_bit, uint64_t n_symbols,
                          void *d_out, size_t cap, size_t *out_len);

/* ---- one stream decoded on several GPUs (cold .et file, no side information) ---------- */
/* The body is split at multiples of 8192 bytes counted from its 4-byte aligned base; every
 * rank synchronises its own range, the ranks exchange (start, exit, symbols), a rank whose
 * start differs from its predecessor's exit calls et_decode_range_sync again with that
 * exit, and when all agree each rank writes its symbols (entreepy_amd/sharded.py
 * decode_cold is the reference sequence).  decode.zig:143-203 has no counterpart: the
 * reference walks the stream serially. */
typedef struct et_range_info {
    uint32_t start_bit;   /* where the first codeword of the range begins, bits from d_range */
    uint32_t exit_bit;    /* first codeword boundary at or after the range end, bits past it */
    uint64_t n_symbols;   /* codewords that begin inside the range */
    uint32_t sweeps;      /* synchronisation launches of this call */
    uint32_t reserved;    /* diagnostics: what synchronised the range -- 0 window sweeps, 1 exit maps, 2 tree walk, 3 row walk */
} et_range_info;

/* d_range: 4-byte aligned pointer to the range's first byte (range_bytes long; a multiple
 * of 8192 unless the stream ends with it); tail_bytes more stream bytes are readable after
 * it (0 only when the stream ends there, else >= 16); has_front: the 16 bytes before
 * d_range are stream bytes too.  in_start_bit >= 0: the range's first codeword begins at
 * that bit (rank 0: the body's start; later calls: the predecessor's exit_bit); -1: unknown,
 * run in from the bytes in front (requires has_front).  Calling again for the same d_range
 * with a corrected in_start_bit repairs the previous result instead of starting over. */
int et_decode_range_sync(et_ctx *ctx, const et_codebook *cb, const void *d_range, size_t range_bytes, size_t tail_bytes,
                         int has_front, int32_t in_start_bit, et_range_info *info);
/* Write the first max_symbols symbols of the range synchronised last into d_out. */
int et_decode_range_write(et_ctx *ctx, uint64_t max_symbols, void *d_out, size_t cap, size_t *out_len);

/* The same split for codes that do NOT self-synchronise (near-fixed-length ones; SURVEY
 * §8e's "fall back" case), where run-ins find nothing: et_decode_range_maps computes, for
 * every bit offset p < *n_starts (= the longest code length, <= 32) at which the range's
 * first codeword might begin, the offset map[p] at which decoding leaves the range
 * (exhaustive synchronisation: one walk per offset, maps composed per block and per 256
 * blocks on the GPU, the last level on the host).  in_start_bit >= 0: the start is known
 * (the stream's first range), every entry is that start's exit.  The ranks exchange their
 * 32-byte maps, chain them from the stream's start, and call et_decode_range_resolve with
 * the start that reaches them; et_decode_range_write then works as above. */
int et_decode_range_maps(et_ctx *ctx, const et_codebook *cb, const void *d_range, size_t range_bytes, size_t tail_bytes,
                         int32_t in_start_bit, uint8_t map[32], uint32_t *n_starts);
int et_decode_range_resolve(et_ctx *ctx, uint32_t in_start_bit, et_range_info *info);

/* ---- groups: one stream over the GPUs of a node ------------------------------------------------ */
/* The reference has one thread and one buffer (encode.zig:25-337); north_star shards the text by
 * contiguous chunk over the GPUs.  An et_group is one rank's membership: its ctx (one GPU), its rank,
 * and how the ranks exchange small host buffers -- a callback (MPI, gloo, threads: anything that can
 * all-gather `bytes_per_rank` bytes) or RCCL over xGMI (loaded with dlopen on first use; a process that
 * already holds an RCCL, e.g. PyTorch's, shares it).  All ranks make the same calls in the same order. */
typedef struct et_group et_group;
/* send: bytes_per_rank bytes of this rank; recv: world x bytes_per_rank, rank order.  0 = success. */
typedef int (*et_allgather_fn)(void *user, const void *send, void *recv, size_t bytes_per_rank);
#define ET_RCCL_ID_BYTES 128
int et_group_create(et_ctx *ctx, int rank, int world, et_allgather_fn allgather, void *user, et_group **group);
/* RCCL: rank 0 obtains an id (ncclGetUniqueId) and hands it to the others out of band (the launcher's
 * store, a file, MPI); every rank then calls et_group_create_rccl with it (ncclCommInitRank).
 * ET_ERR_RCCL when librccl.so cannot be loaded or the communicator cannot be made. */
int et_rccl_unique_id(uint8_t id[ET_RCCL_ID_BYTES]);
int et_group_create_rccl(et_ctx *ctx, int rank, int world, const uint8_t id[ET_RCCL_ID_BYTES], et_group **group);
void et_group_destroy(et_group *group);  /* (does not touch the group's ctx: either may be destroyed first) */
const char *et_group_last_error(const et_group *group);
/* Which RCCL the library bound (the object's name), or why it could not. */
const char *et_rccl_library(void);
/* FAILURES.  Every row a rank contributes to an exchange carries its status.  A rank whose local step failed (a
 * null or too small buffer, a HIP error, a corrupted range) still makes every exchange of the call, and once the
 * rows are in ALL ranks return the status of the first rank that failed: no rank leaves a collective sequence
 * early, nobody waits for a rank that has gone.  The reference's error union (encode.zig:25 `!usize`) reaches
 * every caller.  A failure BEHIND a call's last exchange (an enqueue that failed) is returned by that rank alone
 * and poisons its group: later calls of that rank only take part in their exchanges, carrying the status, so its
 * peers hear of it at their next call.  A transport failure (ET_ERR_RCCL: a peer never arrived within the
 * timeout, the callback failed) ends the call where it is; destroy the group.
 * Options: ET_GROUP_FORCE_COLLECTIVES (value != 0): a group of ONE takes the transport's path all the same --
 * the all-gather from device memory, the kernel that hands the rows to the polling host, send/receive to itself in
 * et_shard_gather -- where it otherwise just copies (one-GPU tests of the N > 1 path).  ET_GROUP_TIMEOUT_MS: how
 * long an RCCL exchange waits for the other ranks (default 600 000). */
enum { ET_GROUP_FORCE_COLLECTIVES = 1, ET_GROUP_TIMEOUT_MS = 2 };
int et_group_set_option(et_group *group, int option, int64_t value);

/* Where this rank's shard sits in the .et image.  Bits and words are counted from the image's first
 * byte; a "word" is 4 bytes.  The rank's buffer holds words [piece_word_lo, piece_word_hi) (word
 * piece_word_lo at d_out[0]); it CONTRIBUTES words [owned_word_lo, owned_word_hi): a word two shards
 * share belongs to the first of them. */
typedef struct et_shard_info {
    uint64_t start_bit, end_bit;      /* the shard's body: image bits [start_bit, end_bit) */
    uint64_t local_start_bit;         /* bit of d_out at which that body begins (rank 0: 8 x header_len; else start_bit % 32) */
    uint64_t header_len;              /* rank 0: bytes of header + dictionary in front of its body; else 0 */
    uint64_t file_bytes;              /* length of the whole image (encode.zig:318,336) */
    uint64_t text_len;                /* bytes of text over all ranks */
    uint64_t piece_word_lo, piece_word_hi, owned_word_lo, owned_word_hi;
    float exchange_ms, plan_ms;       /* host clock: the histogram all-gather (incl. the wait for K1); code table + header + offsets */
    float seam_ms, concat_ms;         /* host clock: et_shard_merge_seams; the last et_shard_write_fd / et_shard_gather */
} et_shard_info;

/* encode() (encode.zig:25-337) for one rank's chunk d_text[0..n) of the group's text: local histogram
 * (K1), ONE exchange (all-gather of the 256 x u64 local histograms: their sum is encode.zig:43-47's
 * histogram, each row gives a shard's bit count; the row also carries the rank's status and cap), the same
 * code table, header and offsets on every rank (et_plan_shards), then the shard's body at its bit offset
 * (K2 + K4).  d_out: 4-byte aligned, cap >= et_encode_bound(n) -- which holds any shard whose symbols are as
 * frequent in it as in the whole text; a shard of symbols that are rare elsewhere packs to more, and then ALL
 * ranks return ET_ERR_CAP (every rank knows every shard's size and cap from the rows).  A rank may hold no text
 * (n = 0).  ET_ERR_EMPTY when all ranks are empty. */
int et_encode_sharded(et_group *group, const void *d_text, size_t n, void *d_out, size_t cap, et_shard_info *info);
/* The bit-offset-adjusted concatenation (encode.zig:319 writes ONE image).  After et_encode_sharded:
 * et_shard_merge_seams -- the owner of a word that several shards share receives their bits (one exchange
 * of 8 bytes per rank; d_out's last word is patched on the device).  From then on the ranks' owned words
 * are disjoint ranges of the image and travel independently:
 * et_shard_write_fd   pwrite this rank's owned bytes at their offset of `fd` (any rank order; rank-local),
 * et_shard_place      copy them into an image in device memory this rank can address (same GPU, or a
 *                     peer-mapped pointer), on the ctx stream,
 * et_shard_gather     RCCL groups: every rank's owned words to `root`'s d_image over xGMI (send/recv;
 *                     d_image and cap are read on root only; cap >= file_bytes rounded up to 4). */
int et_shard_merge_seams(et_group *group, void *d_out);
int et_shard_write_fd(et_group *group, const void *d_out, int fd);
int et_shard_place(et_group *group, const void *d_out, void *d_image, size_t cap);
int et_shard_gather(et_group *group, const void *d_out, void *d_image, size_t cap, int root);
/* The plan of the group's last et_encode_sharded: code table, the world + 1 shard offsets, this rank's info
 * (with the timings of the calls made since). */
int et_group_codebook(const et_group *group, et_codebook *cb);
int et_group_start_bits(const et_group *group, uint64_t *start_bits);
int et_group_last_info(const et_group *group, et_shard_info *info);
/* The host arithmetic of the concatenation, on its own (tests, other hosts): words[4] = {piece_lo, piece_hi,
 * owned_lo, owned_hi} of `rank`; et_seam_word: the word that closes `rank`'s owned range with the bits of
 * every later shard that begins in it (first_last = per rank {first word, last word} of its buffer, own bits
 * only); *has_seam = 0 when the rank shares no word it owns. */
int et_shard_words(const uint64_t *start_bits, uint32_t world, uint32_t rank, uint64_t words[4]);
int et_seam_word(const uint64_t *start_bits, uint32_t world, uint32_t rank, const uint32_t *first_last, uint32_t *merged, int *has_seam);
/* d_src[0..len) -> fd at file_offset, and back, through the ctx's pinned staging (pwrite / pread in chunks,
 * overlapped with the copies; main.zig:34-40 and encode.zig:319 for one rank's part of a file). */
int et_device_to_fd(et_ctx *ctx, const void *d_src, size_t len, int fd, uint64_t file_offset);
int et_fd_to_device(et_ctx *ctx, int fd, uint64_t file_offset, size_t len, void *d_dst);

/* decode() (decode.zig:13-220) of ONE cold stream by the ranks of a group: d_compressed = the .et file
 * minus its first 4 bytes, resident on every rank (at least its own 8 KiB-block range with 16 bytes on
 * either side, and the first 8 KiB for the dictionary).  Rank r decodes blocks [r, r+1) x n_blocks / world:
 * *written symbols into d_out, the first of which is symbol *first_index of the text (the output stays
 * sharded).  One exchange of (start, exit, symbols) per round (expected: one round); codes that do not
 * self-synchronise exchange their 32-byte exit maps instead. */
int et_decode_sharded(et_group *group, const void *d_compressed, size_t len, void *d_out, size_t cap, size_t *written,
                      uint64_t *first_index);
/* The same in two steps, for a rank that holds only what it needs of the stream and sizes its output once it knows
 * its share.  Offsets count from compressed[0] (the .et file minus its first 4 bytes), which is taken to sit on a
 * 4-byte boundary; d_compressed above must be 4-byte aligned for the same reason.
 * et_decode_shard_window: which bytes of `compressed` rank `rank` of `world` needs besides the dictionary -- its
 *   8 KiB-block range with 16 bytes on either side (window_len 0: the rank holds no blocks); head = the first
 *   min(len, 8192) bytes of `compressed` in HOST memory (header + dictionary, decode.zig:34-141), len = all of it.
 * et_decode_sharded_begin (collective): d_window = bytes [window_off, window_off + window_len) of `compressed` in
 *   device memory (window_off a multiple of 4, d_window 4-byte aligned; at least the window above); cap = symbols
 *   the rank's output will hold, ~0 when it is sized afterwards.  *n_mine = the symbols this rank writes, the
 *   first of which is symbol *first_index of the text.
 * et_decode_sharded_write (rank-local): those symbols into d_out. */
int et_decode_shard_window(const uint8_t *head, size_t head_len, uint64_t len, int rank, int world, uint64_t *window_off, uint64_t *window_len);
int et_decode_sharded_begin(et_group *group, const uint8_t *head, size_t head_len, uint64_t len, const void *d_window, uint64_t window_off,
                            size_t window_len, uint64_t cap, uint64_t *n_mine, uint64_t *first_index);
int et_decode_sharded_write(et_group *group, void *d_out, size_t cap, size_t *written);

#ifdef __cplusplus
}
#endif
#endif /* ENTREEPY_HIP_H */
