// et_batch.hip -- gfx950 kernels of the batched calls (et_batch.h): B independent small streams, one workgroup of 256
// per stream from first byte to last, a grid-stride loop over the streams.  No workgroup ever waits for another: there is
// no look-back, no ticket and no flag, and every loop's trip count is bounded by the stream's own length.
//
//   encode   k_batch_hist    256 counts per stream into pinned host memory            (encode.zig:43-47)
//            (host: code table and header per stream, one upload)
//            k_batch_encode  header, then the codes MSB-first, rounds of 4 KiB          (encode.zig:259-318)
//   decode   k_batch_heads   header + dictionary bytes per stream into pinned memory   (decode.zig:34-141 runs on the host)
//            k_batch_decode  LDS lookup table, then the body 8 KiB at a time, in order  (decode.zig:143-203)
// and of the shared-table calls, where ONE table serves the whole batch and is set up once per workgroup, in front of the loop:
//   encode   k_shared_encode count pass (length, uncoded bytes, capacity), then k_batch_encode's rounds: the body alone, at any
//            output alignment, not a byte beyond it
//   decode   k_shared_decode k_batch_decode's stream loop under that one table
// and of the packed calls: the shared-table kernels with their jobs read from u64 offset arrays on the device, each record judged
// from its own pair of entries, and the bodies laid back to back by a scan on the device:
//   encode   k_packed_count  k_shared_encode's count pass alone: body bytes per record into a workspace, its status
//            k_packed_scan   ONE workgroup, a loop over tiles of 4096 records: sizes -> u64 offsets, the total, the report to the host
//            k_packed_pack   k_shared_encode's pack pass alone, destination and length from the offsets the scan stored
//   decode   k_packed_decode k_shared_decode's loop; counters in device memory, the last workgroup reports them
//   gather   k_gather_plan   one lane per row of a selection: its record's offsets judged, its room into the workspace, its status
//            k_packed_scan   the rooms -> out_index (its report optional: a writing call's leaves with the decode)
//            k_packed_gather k_packed_decode's loop over the rows, each to its place in a dense output
//   match    k_match_flag    one lane per record: judged, compared with the encoded needle on the compressed bytes; ballot masks, tile counts
//            k_packed_scan   the tile counts -> each tile's first place among the rows, the report
//            k_rows_emit     the selected record numbers, ascending, by popcount ranks
//   search   k_search_flag   one lane per record: judged; a short body walked codeword by codeword with the needle's bits compared at every boundary;
//                            a long one listed; positions, ballot masks, tile counts
//            k_search_long   one workgroup per listed record: k_packed_decode's walk without its write half, compared on the settled boundaries
//            k_packed_scan   as in the match
//            k_rows_emit     as in the match, with the needle's position beside the record's number where asked for
//   join     k_join_build    one lane per key of a key set: judged, hashed on the compressed bytes, inserted into a table in the workspace
//            k_join_flag     one lane per record: judged, hashed, probed, every hit confirmed by bytes; ballot masks, tile counts, key numbers
//            k_packed_scan   as in the match
//            k_rows_emit     as in the match, with the lowest equal key's number beside the record's where asked for
//   group    k_group_build   the join's build with the store as its own key set: equal records meet in one slot, which keeps the lowest number; the slot is loaded before any atomic
//            k_group_flag    one lane per record: judged, probed with the build's hash for its representative; ballot masks and tile counts of the representatives
//            k_packed_scan   as in the match
//            k_group_emit    the representatives, ascending, by popcount ranks: first rows, counts zeroed, each one's dense number
//            k_group_number  one lane per record: its group's number; the counts by adds combined in the wavefront
//   take     k_take_plan     one lane per row of a selection: its record judged, {body bytes, length, where the body begins} into the workspace
//            k_take_scan     ONE workgroup: the two sizes -> out_body_index and out_text_index, the report
//            k_take_copy     the selected bodies back to back as they are: one lane per aligned 16-byte word of the OUTPUT
//   slice    k_slice_plan    one lane per row: judged; a short body walked to the slice's two boundaries, cut in front of a stop byte; a long one listed
//            k_slice_long    one workgroup per listed row: k_search_long's settled blocks, the boundaries reduced over the workgroup
//            k_take_scan     as in the take
//            k_take_copy     as in the take, a row's source a run of BITS: each byte a funnel shift of two, the last one masked to its bits
//   field    k_field_plan    one lane per row: judged; a short body walked with a running delimiter count to the field's two boundaries; a long one listed
//            k_field_long    one workgroup per listed row: settled blocks whose walks count delimiters, a second scan numbers them, the boundaries reduced
//            k_take_scan     as in the take
//            k_take_copy     as in the slice
//   concat   k_concat_plan   one lane per row of two stores: both judged; short bodies walked to the end of their stored text; a long one listed
//            k_concat_long   one workgroup per listed row: the slice's counting walk for each long side
//            k_take_scan     as in the take
//            k_concat_copy   k_take_copy's frame: a row's bytes are the OR of its three runs of bits
//   recode   k_recode_plan   one lane per row: judged; a short body walked under table IN, the output table's bits, symbols and flag summed; a long one listed
//            k_recode_long   one workgroup per listed row: settled blocks whose walks sum the same three, cut at the length
//            k_take_scan     as in the take
//            k_recode_write  one lane per short row: the walk again, the codes under table OUT into a 64-bit accumulator, dword stores
//            k_recode_write_long   one workgroup per listed row: settled blocks, the walk again into an LDS bit image, flushed in rounds
//   number   k_number_plan   one lane per row: judged; a short reach walked to the slice's end, its symbols from `first` on parsed as an integer; a long one listed
//            k_number_long   one workgroup per listed row: the slice's settled blocks, then ONE lane parses the at most 32 codewords of the run they found
//            k_number_fold   one lane per row: the kinds counted, the aggregates folded in by adds combined in the wavefront, the report
//
// The kernels the host waits for end the same way: the last workgroup to finish (a device counter tells which)
// stores the launch's epoch into a pinned word the host polls.
//
// What the kernels share is defined once: the text span and the pack rounds of the encodes (text_span, pack_rounds); the code tables,
// the codeword step, the walk and the settling of a block of the decodes and the long search (CodeTables, code_at, walk, settle_block).
// The workgroup scans, the 16-byte chunk load and the hand-over itself are et_device.h's.
#include "et_batch.h"

#include "et_device.h"

#define ET_JOIN_FN __host__ __device__ __forceinline__
#include "et_join.h"

namespace et {

namespace {

constexpr int BB = 256;  // threads per workgroup

// After the workgroup's last store to pinned memory: count it; the last one resets the counter and tells the host.
__device__ __forceinline__ void batch_done(uint32_t *counter, unsigned long long *host_done, unsigned long long epoch) {
    pinned_stores_visible();
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t before = atomicAdd(counter, 1u);
        if (before == gridDim.x - 1) {
            atomicExch(counter, 0u);
            hand_over(host_done, epoch);
        }
    }
}

// A text of `len` bytes at ptr + off as load_chunk (et_device.h) takes it: bytes [lo, hi) from a 16-byte aligned base.  Its
// neighbours in the buffer are other streams, or nothing: only its own bytes are loaded.
struct TextSpan {
    const uint8_t *base;
    uint64_t lo, hi;
};

__device__ __forceinline__ TextSpan text_span(const uint8_t *ptr, uint64_t off, uint64_t len) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(ptr) + off;
    return TextSpan{reinterpret_cast<const uint8_t *>(a & ~static_cast<uintptr_t>(15)), a & 15, (a & 15) + len};
}

// block_exclusive_scan in u64 (k_packed_scan: a tile of body sizes can reach 2^32).  `scratch` is 4 LDS words of 8 bytes; ONE
// barrier, and the caller separates two calls by another.
__device__ __forceinline__ uint64_t block_exclusive_scan64(uint64_t x, uint64_t *scratch, uint64_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t inc = wave_inclusive_scan64(x);
    if (lane == 63) scratch[wave] = inc;
    __syncthreads();
    uint64_t before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint64_t v = scratch[w];
        if (w < wave) before += v;
        sum += v;
    }
    *total = sum;
    return before + (inc - x);
}

}  // namespace

// --------------------------------------------------------------------------------
// k_batch_hist: LDS counters [bin][32] as k_hist_tiles keeps them -- lane l adds to replica l & 31, its own bank
// whatever the symbol -- 32 KiB, five workgroups per CU.  Thread = bin sums (and clears) the replicas and stores the
// stream's 256 counts into pinned host memory.
// --------------------------------------------------------------------------------
__global__ __launch_bounds__(BB) void k_batch_hist(const uint8_t *__restrict__ d_in, const BatchSpan *__restrict__ spans, uint32_t n,
                                                   uint32_t *__restrict__ host_hist, uint32_t *__restrict__ counter,
                                                   unsigned long long *__restrict__ host_done, unsigned long long epoch) {
    __shared__ __attribute__((aligned(16))) uint32_t sh[256 * 32];
    const int tid = threadIdx.x;
    for (int i = tid; i < 256 * 32; i += BB) sh[i] = 0;
    __syncthreads();
    uint32_t *mine = sh + (tid & 31);
    for (uint32_t j = blockIdx.x; j < n; j += gridDim.x) {
        const BatchSpan sp = spans[j];
        const TextSpan t = text_span(d_in, sp.in_off, sp.in_len);
        for (uint64_t off = static_cast<uint64_t>(tid) * 16; off < t.hi; off += ROUND_BYTES) {
            const Chunk c = load_chunk(t.base, off, t.lo, t.hi);
            if (c.valid == 0xffffu) {
#pragma unroll
                for (int k = 0; k < 16; ++k) atomicAdd(mine + ((c.w[k >> 2] >> (8 * (k & 3))) & 0xffu) * 32, 1u);
            } else if (c.valid) {
                for (int k = 0; k < 16; ++k)
                    if (c.valid & (1u << k)) atomicAdd(mine + ((c.w[k >> 2] >> (8 * (k & 3))) & 0xffu) * 32, 1u);
            }
        }
        __syncthreads();
        uint32_t total = 0;
        uint4 *row = reinterpret_cast<uint4 *>(sh + tid * 32);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = (q + tid) & 7;  // (rotated: the 16-lane groups of a ds_read_b128 on different bank quads)
            const uint4 v = row[r];
            total += v.x + v.y + v.z + v.w;
            row[r] = make_uint4(0, 0, 0, 0);
        }
        host_hist[static_cast<uint64_t>(j) * 256 + tid] = total;
        __syncthreads();
    }
    batch_done(counter, host_done, epoch);
}

// --------------------------------------------------------------------------------
// k_batch_encode: the stream's code table in LDS (2 KiB), its header copied to the image, then rounds of 4 KiB: 16 bytes
// per lane, the lane's bit total, a workgroup scan whose sum is carried to the next round, and each lane ORs its codes
// into an LDS image of the round's bits (big-endian words: bit b of the image is bit 31 - b % 32 of word b / 32).  Whole
// words leave as byte-swapped dword stores; the word the round ends in is carried into the next as `pending` (the
// header's last, partial word seeds it).  The stream's last word is stored whole, zero bits behind the body: the pad to
// the byte of encode.zig:316, and at most 3 bytes more inside the caller's et_encode_bound.
// LDS: 2 KiB + 16.4 KiB stage -> 8 workgroups per CU.
// --------------------------------------------------------------------------------
constexpr uint32_t ENC_STAGE_WORDS = ROUND_BYTES * 32 / 32 + 8;  // 4096 symbols of at most 32 bits, + the shared first word

// One round of the pack: the lane's bit total over its 16 bytes, the workgroup
// scan, and the lane's codes ORed into the LDS image from stage bit (carry & 31) + what lies before the lane; `pending` (the
// partial word the round before ended in) goes into stage word 0.  Returns the round's bits.  The caller's barrier follows.
__device__ __forceinline__ uint32_t pack_round(const Chunk &c,const uint2 *s_tab, uint32_t *s_stage, uint32_t *s_wsum, uint32_t carry, uint32_t pending) {
    const int tid = threadIdx.x;
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (c.valid & (1u << k)) bits += s_tab[(c.w[k >> 2] >> (8 * (k & 3))) & 0xffu].y;
    uint32_t round_bits;
    const uint32_t before = block_exclusive_scan(bits, s_wsum, &round_bits);  // (s_wsum: the caller's barriers lie between two rounds' scans)
    if (tid == 0 && pending) atomicOr(&s_stage[0], pending);
    // the lane's codes, from stage bit p on
    uint32_t p = (carry & 31) + before;
    uint32_t wi = p >> 5, fill = p & 31;
    uint64_t acc = 0;
    if (bits) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (!(c.valid & (1u << k))) continue;
            const uint2 e = s_tab[(c.w[k >> 2] >> (8 * (k & 3))) & 0xffu];
            if (!e.y) continue;  // (a symbol without a code: the 256-symbol quirk)
            acc |= (static_cast<uint64_t>(e.x) << 32) >> fill;
            fill += e.y;
            if (fill >= 32) {
                atomicOr(&s_stage[wi], static_cast<uint32_t>(acc >> 32));
                acc <<= 32;
                ++wi;
                fill -= 32;
            }
        }
        if (fill) atomicOr(&s_stage[wi], static_cast<uint32_t>(acc >> 32));
    }
    return round_bits;
}

// Word g of the image at `line` (4-byte aligned): whole when it lies inside the image bytes [lo, hi), else its bytes that do.
__device__ __forceinline__ void store_image_word(uint8_t *line, uint32_t g, uint32_t v, uint32_t lo, uint32_t hi) {
    const uint32_t b0 = g * 4;
    if (b0 >= lo && b0 + 4 <= hi) {
        reinterpret_cast<uint32_t *>(line)[g] = v;
    } else {
        for (uint32_t k = 0; k < 4; ++k)
            if (b0 + k >= lo && b0 + k < hi) line[b0 + k] = static_cast<uint8_t>(v >> (8 * k));
    }
}

// The rounds of a text's pack, every encode's: its codes into the bit image at `line` (4-byte aligned) from image bit `carry` on,
// `pending` = the bits of word carry / 32 in front of that (the header's last, partial word; 0 where the image begins with the body).
// CLIP: image bytes [lo, hi) are the body, and all that is stored; else every word leaves whole, the last one with zero bits behind
// the body.  s_stage is zero on entry and on return.
template <bool CLIP>
__device__ __forceinline__ void pack_rounds(const TextSpan &t, uint8_t *__restrict__ line, uint32_t carry, uint32_t pending, uint32_t lo, uint32_t hi, const uint2 *s_tab,
                                            uint32_t *s_stage, uint32_t *s_wsum) {
    const uint32_t tid = threadIdx.x;
    auto store = [&](uint32_t g, uint32_t big_endian) {
        if (CLIP) store_image_word(line, g, __builtin_bswap32(big_endian), lo, hi);
        else reinterpret_cast<uint32_t *>(line)[g] = __builtin_bswap32(big_endian);
    };
    for (uint64_t r0 = 0; r0 < t.hi; r0 += ROUND_BYTES) {
        const Chunk c = load_chunk(t.base, r0 + static_cast<uint64_t>(tid) * 16, t.lo, t.hi);
        const uint32_t round_bits = pack_round(c, s_tab, s_stage, s_wsum, carry, pending);
        __syncthreads();
        const uint32_t t_bits = (carry & 31) + round_bits, full = t_bits >> 5, w0 = carry >> 5;
        pending = (t_bits & 31) ? s_stage[full] : 0u;
        __syncthreads();
        for (uint32_t i = tid; i <= full; i += BB) {
            if (i < full) store(w0 + i, s_stage[i]);
            s_stage[i] = 0;
        }
        carry += round_bits;
        __syncthreads();
    }
    if (tid == 0 && (carry & 31)) store(carry >> 5, pending);
}

__global__ __launch_bounds__(BB) void k_batch_encode(const uint8_t *__restrict__ d_in, uint8_t *__restrict__ d_out, const BatchEncJob *__restrict__ jobs,
                                                     uint32_t n, const uint8_t *__restrict__ blob) {
    __shared__ uint2 s_tab[256];
    __shared__ uint32_t s_stage[ENC_STAGE_WORDS];
    __shared__ uint32_t s_wsum[4];
    const int tid = threadIdx.x;
    for (uint32_t i = tid; i < ENC_STAGE_WORDS; i += BB) s_stage[i] = 0;
    for (uint32_t j = blockIdx.x; j < n; j += gridDim.x) {
        const BatchEncJob job = jobs[j];
        const uint2 *tab = reinterpret_cast<const uint2 *>(blob + job.blob_off);
        const uint32_t *hdr = reinterpret_cast<const uint32_t *>(blob + job.blob_off + 2048);
        uint32_t *out32 = reinterpret_cast<uint32_t *>(d_out + job.out_off);
        __syncthreads();  // (the stream before: its table and stage are done with)
        s_tab[tid] = tab[tid];
        const uint32_t hw = job.header_len >> 2;
        for (uint32_t i = tid; i < hw; i += BB) out32[i] = hdr[i];
        const uint32_t pending = (job.header_len & 3) ? __builtin_bswap32(hdr[hw]) : 0u;  // (the pad behind the header is zero)
        __syncthreads();
        pack_rounds<false>(text_span(d_in, job.in_off, job.in_len), d_out + job.out_off, job.header_len * 8, pending, 0, 0, s_tab, s_stage, s_wsum);
    }
}

// --------------------------------------------------------------------------------
// k_batch_heads: the first min(in_len, header_bound(d)) bytes of every stream (d = its first byte: the dictionary has
// d + 1 entries, decode.zig:34) into its BATCH_HEAD_STRIDE bytes of pinned host memory, any source alignment.
// --------------------------------------------------------------------------------
__global__ __launch_bounds__(BB) void k_batch_heads(const uint8_t *__restrict__ d_in, const BatchSpan *__restrict__ spans, uint32_t n,
                                                    uint32_t *__restrict__ host_heads, uint32_t *__restrict__ counter,
                                                    unsigned long long *__restrict__ host_done, unsigned long long epoch) {
    for (uint32_t j = blockIdx.x; j < n; j += gridDim.x) {
        const BatchSpan sp = spans[j];
        if (!sp.in_len) continue;
        const uint8_t *src = d_in + sp.in_off;
        uint32_t len = header_bound(src[0]);
        if (sp.in_len < len) len = sp.in_len;
        uint32_t *dst = host_heads + static_cast<uint64_t>(j) * (BATCH_HEAD_STRIDE / 4);
        for (uint32_t w = threadIdx.x; w * 4 < len; w += BB) {
            uint32_t v = 0;
            for (uint32_t k = 0; k < 4 && w * 4 + k < len; ++k) v |= static_cast<uint32_t>(src[w * 4 + k]) << (8 * k);
            dst[w] = v;
        }
    }
    batch_done(counter, host_done, epoch);
}

// --------------------------------------------------------------------------------
// k_batch_decode.  The dictionary arrives as its codes sorted by left-aligned value; it is a full prefix-free tree (the
// host sends nothing else here), so the code a 32-bit window begins with is the largest one not above the window: a
// binary search of at most 8 steps.  That search fills the first-level table (2048 x u16: length << 8 | symbol, 0 = longer
// than 11 bits) and serves the longer codes directly.
// The body is taken 8 KiB (2048 words from its 4-byte aligned base) at a time, in order, so the bit at which a block's
// first codeword begins is always known: the body's start, then the exit of the block before.  Lane i owns bits
// [256 i, 256 i + 256) of the block and walks from its entry until it leaves them; its exit is lane i + 1's entry.  Lane 0's
// entry is right from the start, so lane i's is after i trips at most: the fixed point is capped at 256 trips and exact for
// every code, self-synchronising or not.  A codeword counts when it ends inside the body (decode.zig:143-203 stops when
// the bits run out).  Counts are scanned, the symbols go to an LDS stage laid out at the output's own alignment, and leave
// as aligned dword stores (bytes at the two ends).
// LDS: 2 + 4 + 9 + 1 + 16 KiB = 33 KiB -> 4 workgroups per CU.
// --------------------------------------------------------------------------------
constexpr uint32_t DEC_WORDS = 2048;                                 // words per block
constexpr uint32_t DEC_STAGED = DEC_WORDS + 2;                       // + what a window at the block's last bits reads
__device__ __forceinline__ uint32_t padded(uint32_t k) { return k + (k >> 3); }  // lanes 8 words apart on different banks

// The two tables every walk looks a codeword up in; the first member of the LDS of every kernel that walks.
struct CodeTables {
    uint2 codes[256];                    // the sorted codes: {left-aligned value, length << 8 | symbol}
    uint16_t lut[1u << BATCH_LUT_BITS];  // by a window's first 11 bits: length << 8 | symbol, 0 = longer than 11 bits
};

struct BatchDecLds {
    CodeTables t;
    uint32_t bits[DEC_STAGED + (DEC_STAGED >> 3) + 2];
    uint32_t entry[BB + 1];
    uint32_t wsum[4];
    uint32_t out[BATCH_STAGE_BYTES / 4 + 2];
};

// The code the window begins with, by the binary search alone.
__device__ __forceinline__ uint32_t search_codes(const uint2 *codes, uint32_t n_codes, uint32_t win) {
    uint32_t lo = 0, hi = n_codes;  // codes[0] is the all-zero code of a full tree: codes[lo].x <= win throughout
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (codes[mid].x <= win) lo = mid; else hi = mid;
    }
    return codes[lo].y;
}

__device__ __forceinline__ uint32_t search_codes(const CodeTables &t, uint32_t n_codes, uint32_t win) { return search_codes(t.codes, n_codes, win); }

// THE codeword step: length << 8 | symbol of the code the window begins with -- the first-level table, then the search.
__device__ __forceinline__ uint32_t code_at(const CodeTables &t, uint32_t n_codes, uint32_t win) {
    uint32_t meta = t.lut[win >> (32 - BATCH_LUT_BITS)];
    if (!meta) meta = search_codes(t, n_codes, win);
    return meta;
}

// The prologue of every kernel that walks: the sorted codes into LDS, a barrier, the first-level table from them.  A barrier lies
// between this and the first code_at: a block's first (settle_block), or the caller's own.
__device__ __forceinline__ void load_tables(CodeTables &t, const uint2 *__restrict__ codes, uint32_t n_codes) {
    if (threadIdx.x < n_codes) t.codes[threadIdx.x] = codes[threadIdx.x];
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < (1u << BATCH_LUT_BITS); e += BB) {
        const uint32_t meta = search_codes(t, n_codes, e << (32 - BATCH_LUT_BITS));
        t.lut[e] = (meta >> 8) <= BATCH_LUT_BITS ? static_cast<uint16_t>(meta) : static_cast<uint16_t>(0);
    }
}

// A body as the walks see it: counted in bits from the 4-byte aligned word it begins in.
struct BodyBits {
    const uint32_t *words;
    uint32_t first_bit, end_bit, n_words;  // the body's first bit, its last + 1, the aligned words that hold a byte of it
};

__device__ __forceinline__ BodyBits body_bits_of(const uint8_t *d_bodies, uint64_t body_off, uint32_t body_bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_bodies) + body_off;
    BodyBits g;
    g.words = reinterpret_cast<const uint32_t *>(a & ~static_cast<uintptr_t>(3));
    g.first_bit = static_cast<uint32_t>(a & 3) * 8;
    g.end_bit = g.first_bit + body_bytes * 8;
    g.n_words = (g.end_bit + 31) >> 5;
    return g;
}

// Word k of the body, big-endian; zero behind the last word that holds a byte of it (which is never loaded).
__device__ __forceinline__ uint64_t body_word_be(const BodyBits &g, uint32_t k) { return k < g.n_words ? __builtin_bswap32(g.words[k]) : 0u; }

// The 32 bits from bit `bit` on, from global memory.
__device__ __forceinline__ uint32_t body_window(const BodyBits &g, uint32_t bit) {
    const uint32_t k = bit >> 5;
    return static_cast<uint32_t>((((body_word_be(g, k) << 32) | body_word_be(g, k + 1)) << (bit & 31)) >> 32);
}

// The 32 bits from bit `bit` of the staged block on.
__device__ __forceinline__ uint32_t lane_window(const BatchDecLds &s, uint32_t bit) {
    const uint32_t k = bit >> 5;
    const uint64_t two = (static_cast<uint64_t>(s.bits[padded(k)]) << 32) | s.bits[padded(k + 1)];
    return static_cast<uint32_t>((two << (bit & 31)) >> 32);
}

// THE walk: the lane's codewords from `entry` (bits into its 256) until it leaves them.  Returns its exit; *count = the codewords
// it stepped over, each of which ends at or before the body's last bit (`room` = bits from the lane's first bit to there; 0 when
// the lane lies behind the body).  visit(cnt, pos, win, meta) sees every such codeword -- its number in this walk, its bit, the
// window there, its length << 8 | symbol -- in front of the step over it, and ends the walk there by returning false (the exit of
// a walk that was ended is nobody's entry: 512 like that of one whose bits ran out).
template <class Visit>
__device__ __forceinline__ uint32_t walk(const BatchDecLds &s, uint32_t n_codes, uint32_t entry, uint32_t room, uint32_t *count, Visit &&visit) {
    const uint32_t lane_bit = threadIdx.x * 256;
    uint32_t pos = entry, cnt = 0;
    while (pos < 256) {
        const uint32_t win = lane_window(s, lane_bit + pos);
        const uint32_t meta = code_at(s.t, n_codes, win), len = meta >> 8;
        if (pos + len > room || !visit(cnt, pos, win, meta)) {  // THE rule: the bits ran out inside this codeword: nothing behind it
            pos = 512;                                           // is one, so the next lane's entry (256) lies behind ITS bits as well
            break;
        }
        ++cnt;
        pos += len;
    }
    *count = cnt;
    return pos;
}

// The visitor of a walk that only counts.
struct JustCount {
    __device__ __forceinline__ bool operator()(uint32_t, uint32_t, uint32_t, uint32_t) const { return true; }
};

// One block of a body by the whole workgroup, up to where every lane knows its codewords: the block's DEC_STAGED big-endian words
// into the stage, the fixed point over the lanes' entries (a lane walks again, with a fresh copy of `visit`, whenever its entry
// changes: what `visit` holds on return is the settled walk's), the scan of the counts.  Begins with a barrier: the one between
// load_tables, or the block before (its stages, entry[BB], what the caller keeps in LDS), and this block's first walk.
struct Settled {
    uint32_t used, count, first;  // the lane's settled entry, its codewords, how many of the block's lie in front of them
    uint32_t room;                // bits from the lane's first to the body's last + 1; 0 when the lane lies behind the body
    uint32_t total, start;        // the block's codewords; the bit of the next block at which its first codeword begins
};

template <class Visit>
__device__ __forceinline__ Settled settle_block(BatchDecLds &s, uint32_t n_codes, const BodyBits &g, uint32_t blk, uint32_t start, Visit &visit) {
    const uint32_t tid = threadIdx.x;
    const Visit fresh = visit;
    __syncthreads();
    for (uint32_t k = tid; k < DEC_STAGED; k += BB) s.bits[padded(k)] = static_cast<uint32_t>(body_word_be(g, blk * DEC_WORDS + k));
    s.entry[tid] = tid == 0 ? start : 0u;
    __syncthreads();
    Settled b;
    const uint32_t at = blk * DEC_WORDS * 32 + tid * 256;  // the lane's first bit, from the body's aligned base
    b.room = g.end_bit > at ? g.end_bit - at : 0u;
    b.used = 0xffffffffu;
    b.count = 0;
    uint32_t exit = 256;
    for (uint32_t trip = 0; trip < BB; ++trip) {
        const uint32_t mine = s.entry[tid];
        int changed = 0;
        if (mine != b.used) {
            const uint32_t was = exit;
            visit = fresh;
            exit = b.room ? walk(s, n_codes, mine, b.room, &b.count, visit) : 256u;
            b.used = mine;
            changed = exit != was || trip == 0;
        }
        __syncthreads();
        if (changed) s.entry[tid + 1] = exit - 256;
        if (!__syncthreads_or(changed)) break;
    }
    b.first = block_exclusive_scan(b.count, s.wsum, &b.total);  // (s.wsum: the next block's first barrier lies between two scans)
    b.start = s.entry[BB];
    return b;
}

// One stream under the tables in `s`, its symbols to `out`: its blocks in order, each settled, then written.  Returns the symbols
// it holds, at most n_symbols; the first write_cap of them are stored.
__device__ __forceinline__ uint32_t decode_stream(BatchDecLds &s, uint32_t n_codes, const BodyBits &g, uint8_t *__restrict__ out, uint32_t n_symbols, uint32_t write_cap) {
    const uint32_t tid = threadIdx.x;
    const uint32_t n_blocks = (g.n_words + DEC_WORDS - 1) / DEC_WORDS;
    uint32_t start = g.first_bit, done = 0;  // the block's first codeword; symbols so far
    for (uint32_t blk = 0; blk < n_blocks && done < n_symbols; ++blk) {
        JustCount counting;
        const Settled b = settle_block(s, n_codes, g, blk, start, counting);
        // counts -> where the lane's symbols go
        const uint32_t left = n_symbols - done, take = b.total < left ? b.total : left;
        const uint32_t cap_left = write_cap > done ? write_cap - done : 0u, n_write = take < cap_left ? take : cap_left;
        for (uint32_t s0 = 0; s0 < n_write; s0 += BATCH_STAGE_BYTES) {
            const uint32_t s1 = s0 + BATCH_STAGE_BYTES < n_write ? s0 + BATCH_STAGE_BYTES : n_write;
            uint8_t *dst = out + done + s0;
            const uint32_t align = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(dst) & 3);
            uint8_t *stage = reinterpret_cast<uint8_t *>(s.out);
            if (b.count && b.first < s1 && b.first + b.count > s0) {
                // the settled walk once more: symbol number first + cnt goes to stage byte first + cnt - s0 + align for numbers in [s0, s1),
                // which are the walk's codewords [from, stop) (base: modulo 2^32 where s0 > first)
                const uint32_t stop = s1 - b.first, from = s0 > b.first ? s0 - b.first : 0u, base = b.first - s0 + align;
                uint32_t again;
                (void)walk(s, n_codes, b.used, b.room, &again, [&](uint32_t cnt, uint32_t, uint32_t, uint32_t meta) {
                    if (cnt >= stop) return false;
                    if (cnt >= from) stage[cnt + base] = static_cast<uint8_t>(meta);
                    return true;
                });
            }
            __syncthreads();
            const uint32_t lo = align, hi = align + (s1 - s0);  // stage bytes [lo, hi) -> dst - align + [lo, hi)
            uint8_t *line = dst - align;
            for (uint32_t w = tid; w * 4 < hi; w += BB) {
                if (w * 4 >= lo && w * 4 + 4 <= hi) {
                    reinterpret_cast<uint32_t *>(line)[w] = s.out[w];
                } else {
                    for (uint32_t k = w * 4; k < w * 4 + 4; ++k)
                        if (k >= lo && k < hi) line[k] = stage[k];
                }
            }
            __syncthreads();
        }
        start = b.start;
        done += take;
    }
    return done;
}

__global__ __launch_bounds__(BB) void k_batch_decode(const uint8_t *__restrict__ d_in, uint8_t *__restrict__ d_out, const BatchDecJob *__restrict__ jobs,
                                                     uint32_t n, const uint8_t *__restrict__ blob, uint32_t *__restrict__ host_totals,
                                                     uint32_t *__restrict__ counter, unsigned long long *__restrict__ host_done, unsigned long long epoch) {
    __shared__ BatchDecLds s;
    const uint32_t tid = threadIdx.x;
    for (uint32_t j = blockIdx.x; j < n; j += gridDim.x) {
        const BatchDecJob job = jobs[j];
        __syncthreads();  // (the stream before is done with the tables)
        load_tables(s.t, reinterpret_cast<const uint2 *>(blob + job.blob_off), job.n_codes);
        const uint32_t done = decode_stream(s, job.n_codes, body_bits_of(d_in, job.body_off, job.body_bytes), d_out + job.out_off, job.n_symbols, job.write_cap);
        if (tid == 0) host_totals[j] = done;
    }
    batch_done(counter, host_done, epoch);
}

// --------------------------------------------------------------------------------
// k_shared_encode: ONE code table for every stream, in LDS before the loop.  Per stream a count pass over the text -- the
// body's bits, and whether a byte has no code -- decides its status and length before a byte is stored (and is all there
// is when d_out is null: sizes only).  Then k_batch_encode's rounds, with the LDS bit image beginning at bit 8 * (address & 3)
// of the output's aligned word: whole words inside the body leave as dword stores, the bytes of the first and the last
// word that belong to it as byte stores, so that [out_off, out_off + bytes) is all the stream writes and bodies may lie
// back to back.  LDS as k_batch_encode.
// --------------------------------------------------------------------------------
// The count pass of a text (k_shared_encode, k_packed_count): the bytes
// its body takes, and *uncoded = whether a byte of it has no code (the same for every lane).  Ends with a barrier: s_wsum is
// free for the next scan.
__device__ __forceinline__ uint32_t count_body(const TextSpan &t, const uint2 *s_tab, uint32_t *s_wsum, int *uncoded) {
    uint32_t bits = 0;
    int none = 0;
    for (uint64_t off = static_cast<uint64_t>(threadIdx.x) * 16; off < t.hi; off += ROUND_BYTES) {
        const Chunk c = load_chunk(t.base, off, t.lo, t.hi);
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (c.valid & (1u << k)) {
                const uint32_t len = s_tab[(c.w[k >> 2] >> (8 * (k & 3))) & 0xffu].y;
                bits += len;
                none |= !len;
            }
    }
    uint32_t total;
    (void)block_exclusive_scan(bits, s_wsum, &total);
    *uncoded = __syncthreads_or(none);  // (and the barrier between this scan and the next one's s_wsum)
    return (total + 7) >> 3;
}

// The pack pass of that text (k_shared_encode, k_packed_pack): its body, `bytes` long, to dst at any alignment -- image bytes
// [lead, lead + bytes) of the aligned line are the body, and all that is stored.  s_stage is zero on entry and on return.
__device__ __forceinline__ void pack_body(const TextSpan &t, uint8_t *__restrict__ dst, uint32_t bytes, const uint2 *s_tab, uint32_t *s_stage, uint32_t *s_wsum) {
    const uint32_t lead = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(dst) & 3);
    pack_rounds<true>(t, dst - lead, lead * 8, 0u, lead, lead + bytes, s_tab, s_stage, s_wsum);
}

__global__ __launch_bounds__(BB) void k_shared_encode(const uint8_t *__restrict__ d_in, uint8_t *__restrict__ d_out, const SharedJob *__restrict__ jobs,
                                                      uint32_t n, const uint2 *__restrict__ table, uint2 *__restrict__ host_results,
                                                      uint32_t *__restrict__ counter, unsigned long long *__restrict__ host_done, unsigned long long epoch) {
    __shared__ uint2 s_tab[256];
    __shared__ uint32_t s_stage[ENC_STAGE_WORDS];
    __shared__ uint32_t s_wsum[4];
    const int tid = threadIdx.x;
    s_tab[tid] = table[tid];
    for (uint32_t i = tid; i < ENC_STAGE_WORDS; i += BB) s_stage[i] = 0;
    __syncthreads();
    for (uint32_t j = blockIdx.x; j < n; j += gridDim.x) {
        const SharedJob job = jobs[j];
        const TextSpan text = text_span(d_in, job.in_off, job.in_len);
        // the count pass
        int uncoded;
        const uint32_t bytes = count_body(text, s_tab, s_wsum, &uncoded);
        const uint32_t status = uncoded ? SHARED_UNCODED : bytes > job.cap ? SHARED_CAP : SHARED_OK;
        if (tid == 0) host_results[j] = make_uint2(status == SHARED_OK ? bytes : 0u, status);
        if (status != SHARED_OK || !d_out || !bytes) continue;  // (the same for every lane)
        pack_body(text, d_out + job.out_off, bytes, s_tab, s_stage, s_wsum);
    }
    batch_done(counter, host_done, epoch);
}

// --------------------------------------------------------------------------------
// k_shared_decode: the sorted codes and the first-level table ONCE per workgroup, then k_batch_decode's loop for every
// stream the workgroup takes.  A stream decodes job.cap symbols (the caller keeps a record's length: the pad bits behind
// the last codeword would decode as symbols otherwise) or as many codewords as end inside its body.  LDS as k_batch_decode.
// --------------------------------------------------------------------------------
__global__ __launch_bounds__(BB) void k_shared_decode(const uint8_t *__restrict__ d_in, uint8_t *__restrict__ d_out, const SharedJob *__restrict__ jobs,
                                                      uint32_t n, const uint2 *__restrict__ codes, uint32_t n_codes, uint2 *__restrict__ host_results,
                                                      uint32_t *__restrict__ counter, unsigned long long *__restrict__ host_done, unsigned long long epoch) {
    __shared__ BatchDecLds s;
    const uint32_t tid = threadIdx.x;
    load_tables(s.t, codes, n_codes);
    for (uint32_t j = blockIdx.x; j < n; j += gridDim.x) {
        const SharedJob job = jobs[j];
        const uint32_t done = decode_stream(s, n_codes, body_bits_of(d_in, job.in_off, job.in_len), d_out + job.out_off, job.cap, job.cap);
        if (tid == 0) host_results[j] = make_uint2(done, 0u);
    }
    batch_done(counter, host_done, epoch);
}

// --------------------------------------------------------------------------------
// The packed calls.  Record j is bytes [index[j], index[j + 1]) of a dense buffer, and that pair of entries is all that is
// believed about it: a pair that decreases or leaves the buffer fails its record (PACKED_ARG) before a byte is read.
// What failed is counted in registers -- thread 0's in the kernels that give a record to a workgroup, every lane's in those that give
// it to a lane (tally_lanes) -- and added to the counters in device memory once per workgroup, at the end.
// --------------------------------------------------------------------------------
// THE rule for believing a record's two pairs of offsets, for every kernel that takes a record by its number (k_packed_decode, which
// also asks where the text goes, has its own): PACKED_ARG for a number beyond the store or a pair that decreases or leaves the
// bodies, PACKED_UNSUPPORTED for a text above BATCH_SMALL_MAX.  b0, nb and len mean something under PACKED_OK alone, and only such a
// record's body is read.
struct Judged {
    uint32_t status;
    uint64_t b0, nb, len;  // where in the bodies it begins, its bytes, its symbols
};

__device__ __forceinline__ Judged judge_record(const PackedStore &store, uint32_t r) {
    if (r >= store.n) return Judged{PACKED_ARG, 0, 0, 0};
    const uint64_t b0 = store.body_index[r], b1 = store.body_index[r + 1], t0 = store.text_index[r], t1 = store.text_index[r + 1];
    const bool sound = b0 <= b1 && b1 <= store.body_bytes && t0 <= t1;
    return Judged{!sound ? PACKED_ARG : t1 - t0 > BATCH_SMALL_MAX ? PACKED_UNSUPPORTED : PACKED_OK, b0, b1 - b0, t1 - t0};
}

struct PackedTally {
    unsigned long long failed = 0, first = ~0ull, n_short = 0;
    __device__ __forceinline__ void note(uint32_t j, uint32_t status) {
        if (!status) return;
        ++failed;
        const unsigned long long key = static_cast<unsigned long long>(j) << 8 | status;  // (j ascends: the first is the lowest)
        if (key < first) first = key;
    }
    __device__ __forceinline__ void add_to(unsigned long long *stats) const {
        if (failed) {
            atomicAdd(stats + PACKED_N_FAILED, failed);
            atomicMin(stats + PACKED_FIRST, first);
        }
        if (n_short) atomicAdd(stats + PACKED_N_SHORT, n_short);
    }
};

// The end of a kernel that judges an item per lane: what each lane noted -- how many failed, the lowest of them << 8 | its status (a
// lane's items ascend) -- reduced over the wavefront by shuffles and over the workgroup through 4 + 4 words of LDS: one pair of
// atomics per workgroup that saw a failure.
__device__ __forceinline__ void tally_lanes(const PackedTally &mine, unsigned long long *s_failed, unsigned long long *s_first, unsigned long long *stats) {
    unsigned long long failed = mine.failed, first = mine.first;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        failed += __shfl_xor(failed, d, 64);
        const unsigned long long other = __shfl_xor(first, d, 64);
        if (other < first) first = other;
    }
    if ((threadIdx.x & 63) == 0) {
        s_failed[threadIdx.x >> 6] = failed;
        s_first[threadIdx.x >> 6] = first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        PackedTally tally;
        for (int w = 0; w < BB / 64; ++w) {
            tally.failed += s_failed[w];
            if (s_first[w] < tally.first) tally.first = s_first[w];
        }
        tally.add_to(stats);
    }
}

// The report of a decode kernel (k_packed_decode, k_packed_gather), by thread 0 of every workgroup at its end: the workgroup's
// counts are in `stats` before its tick of the counter; the last one to tick reads them all back, stores {out_bytes, failed,
// first << 8 | status, short} and hands over.
__device__ __forceinline__ void packed_report(const PackedTally &tally, uint64_t out_bytes, const PackedReport &report, uint32_t *counter) {
    unsigned long long *stats = report.stats, *host_result = report.host_result;
    tally.add_to(stats);  // (device-scope atomics, like the tick and the read-back below: no cache in between)
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the counts have landed before the tick leaves
    const uint32_t before = atomicAdd(counter, 1u);
    if (before == gridDim.x - 1) {
        __threadfence();
        atomicExch(counter, 0u);
        host_result[PACKED_BYTES] = out_bytes;
        host_result[PACKED_N_FAILED] = atomicAdd(stats + PACKED_N_FAILED, 0ull);
        host_result[PACKED_FIRST] = atomicMin(stats + PACKED_FIRST, ~0ull);
        host_result[PACKED_N_SHORT] = atomicAdd(stats + PACKED_N_SHORT, 0ull);
        hand_over(report.host_done, report.epoch);
    }
}

// k_packed_count: the table in LDS once, then per record k_shared_encode's count pass.  sizes[j] = bytes of body (0 for a
// record that failed, or is empty), d_status[j] (may be null) = its et_status.  LDS 2 KiB.
__global__ __launch_bounds__(BB) void k_packed_count(const uint8_t *__restrict__ d_text, uint64_t text_bytes, const uint64_t *__restrict__ text_index, uint32_t n,
                                                     const uint2 *__restrict__ table, uint32_t *__restrict__ sizes, uint8_t *__restrict__ d_status,
                                                     unsigned long long *__restrict__ stats) {
    __shared__ uint2 s_tab[256];
    __shared__ uint32_t s_wsum[4];
    const int tid = threadIdx.x;
    s_tab[tid] = table[tid];
    __syncthreads();
    PackedTally tally;
    for (uint32_t j = blockIdx.x; j < n; j += gridDim.x) {
        const uint64_t t0 = text_index[j], t1 = text_index[j + 1];
        uint32_t status = PACKED_OK, bytes = 0;
        if (!(t0 <= t1 && t1 <= text_bytes)) {
            status = PACKED_ARG;
        } else if (t1 - t0 > BATCH_SMALL_MAX) {
            status = PACKED_UNSUPPORTED;
        } else if (t1 > t0) {  // (the same for every lane, like every branch above)
            int uncoded;
            bytes = count_body(text_span(d_text, t0, t1 - t0), s_tab, s_wsum, &uncoded);
            if (uncoded) {
                status = PACKED_UNSUPPORTED;
                bytes = 0;
            }
        }
        if (tid == 0) {
            sizes[j] = bytes;
            if (d_status) d_status[j] = static_cast<uint8_t>(status);
            tally.note(j, status);
        }
    }
    if (tid == 0) tally.add_to(stats);
}

// k_packed_scan: ONE workgroup; per trip a tile of 4096 sizes, 16 consecutive ones per lane, becomes 4096 u64 offsets (an
// exclusive scan, the tiles before carried in a register); the total goes to out_index[n].  The trip count is n / 4096, fixed
// by the host.  REPORT: thread 0 then reports to the host: {total, records that failed, the first of them << 8 | its status} and
// the epoch.  k_packed_pack, enqueued behind, takes everything it needs from out_index: the host does not wait in between.
// Without REPORT (a writing gather call: k_packed_gather reports, behind its decode) the offsets are all it leaves.
template <bool REPORT>
__global__ __launch_bounds__(BB) void k_packed_scan(const uint32_t *__restrict__ sizes, uint32_t n, uint64_t *__restrict__ out_index,
                                                    const unsigned long long *__restrict__ stats, unsigned long long *__restrict__ host_result,
                                                    unsigned long long *__restrict__ host_done, unsigned long long epoch) {
    __shared__ uint64_t s_sum[4];
    const uint32_t tid = threadIdx.x;
    uint64_t carry = 0;
    for (uint32_t tile = 0; tile < n; tile += PACKED_SCAN_TILE) {
        const uint32_t i0 = tile + tid * 16;
        uint32_t v[16];
        if (i0 + 16 <= n) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 x = reinterpret_cast<const uint4 *>(sizes + i0)[q];
                v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = i0 + k < n ? sizes[i0 + k] : 0u;
        }
        uint64_t mine = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) mine += v[k];
        uint64_t total;
        uint64_t at = carry + block_exclusive_scan64(mine, s_sum, &total);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (i0 + k < n) out_index[i0 + k] = at;
            at += v[k];
        }
        carry += total;
        __syncthreads();  // (s_sum: between two scans)
    }
    if (tid == 0) {
        out_index[n] = carry;
        if (!REPORT) return;
        host_result[PACKED_BYTES] = carry;
        host_result[PACKED_N_FAILED] = stats[PACKED_N_FAILED];
        host_result[PACKED_FIRST] = stats[PACKED_FIRST];
        host_result[PACKED_N_SHORT] = 0;
        hand_over(host_done, epoch);
    }
}

// k_packed_pack: k_shared_encode's pack pass; record j's body goes to d_out[out_index[j], out_index[j + 1]), and a record
// that takes no bytes (empty, or failed in k_packed_count) is passed over without a look at its text.  No count pass: the
// length comes from the scan.  Every workgroup returns at once when the bodies do not fit: ET_ERR_CAP writes nothing.
// LDS as k_batch_encode.
__global__ __launch_bounds__(BB) void k_packed_pack(const uint8_t *__restrict__ d_text, uint64_t text_bytes, const uint64_t *__restrict__ text_index, uint32_t n,
                                                    uint8_t *__restrict__ d_out, uint64_t cap, const uint64_t *__restrict__ out_index, const uint2 *__restrict__ table) {
    __shared__ uint2 s_tab[256];
    __shared__ uint32_t s_stage[ENC_STAGE_WORDS];
    __shared__ uint32_t s_wsum[4];
    const int tid = threadIdx.x;
    if (out_index[n] > cap) return;
    s_tab[tid] = table[tid];
    for (uint32_t i = tid; i < ENC_STAGE_WORDS; i += BB) s_stage[i] = 0;
    __syncthreads();
    for (uint32_t j = blockIdx.x; j < n; j += gridDim.x) {
        const uint64_t o0 = out_index[j], o1 = out_index[j + 1];
        if (o1 <= o0) continue;
        const uint64_t t0 = text_index[j], t1 = text_index[j + 1];
        if (!(t0 < t1 && t1 <= text_bytes && t1 - t0 <= BATCH_SMALL_MAX)) continue;  // (k_packed_count gave such a record no bytes; asked again, for what is read below)
        pack_body(text_span(d_text, t0, t1 - t0), d_out + o0, static_cast<uint32_t>(o1 - o0), s_tab, s_stage, s_wsum);
    }
}

// k_packed_decode: k_shared_decode with record j's job made here: text_index[j + 1] - text_index[j] symbols from the body
// d_bodies[body_index[j], body_index[j + 1]) to d_out + text_index[j].  d_written[j] (may be null) = symbols stored, d_status[j]
// (may be null) = its et_status.  Nothing is decoded when text_index[n] > cap (the host returns ET_ERR_CAP from the report).
// The last workgroup to finish reports {text_index[n], failed, first << 8 | status, short} and the epoch.  LDS as k_batch_decode.
__global__ __launch_bounds__(BB) void k_packed_decode(PackedStore store, uint8_t *__restrict__ d_out, uint64_t cap, const uint2 *__restrict__ codes, uint32_t n_codes,
                                                      uint32_t *__restrict__ d_written, uint8_t *__restrict__ d_status, PackedReport report, uint32_t *__restrict__ counter) {
    __shared__ BatchDecLds s;
    const uint32_t tid = threadIdx.x;
    const uint8_t *d_bodies = static_cast<const uint8_t *>(store.bodies);
    const uint64_t out_bytes = store.text_index[store.n];
    PackedTally tally;
    if (out_bytes <= cap) {
        load_tables(s.t, codes, n_codes);
        for (uint32_t j = blockIdx.x; j < store.n; j += gridDim.x) {
            const uint64_t b0 = store.body_index[j], b1 = store.body_index[j + 1], t0 = store.text_index[j], t1 = store.text_index[j + 1];
            uint32_t status = PACKED_OK, done = 0;
            // (not judge_record's rule: the text pair says where the symbols GO, so it must end within cap as well, and a record that
            // decodes to nothing is judged empty before it is judged oversize)
            if (!(b0 <= b1 && b1 <= store.body_bytes && t0 <= t1 && t1 <= cap)) {
                status = PACKED_ARG;
            } else if (t1 == t0 || b1 == b0) {  // decodes to nothing, as in the shared-table call; an empty body is a short one
                if (tid == 0 && t1 > t0) ++tally.n_short;
            } else if (t1 - t0 > BATCH_SMALL_MAX) {
                status = PACKED_UNSUPPORTED;
            } else {
                const uint32_t count = static_cast<uint32_t>(t1 - t0);
                done = decode_stream(s, n_codes, body_bits_of(d_bodies, b0, static_cast<uint32_t>(clip_body(b1 - b0, count))), d_out + t0, count, count);
                if (tid == 0 && done < count) ++tally.n_short;
            }
            if (tid == 0) {
                if (d_written) d_written[j] = done;
                if (d_status) d_status[j] = static_cast<uint8_t>(status);
                tally.note(j, status);
            }
        }
    }
    if (tid == 0) packed_report(tally, out_bytes, report, counter);
}

// --------------------------------------------------------------------------------
// The gather call: row k of the result is record rows[k] of a packed store, in any order, with repeats; the rows lie back to
// back in d_out, laid out here.  Three launches in stream order (et_batch.h), the host waiting for the last alone.
// --------------------------------------------------------------------------------
// k_gather_plan: one lane per row, a grid-stride loop; rows[] is loaded coalesced, the four offsets are gathered.  The record judged,
// its room (its length; 0 when it failed) into the workspace, its status byte.  No LDS beyond tally_lanes' 4 + 4 words.
__global__ __launch_bounds__(BB) void k_gather_plan(PackedStore store, const uint32_t *__restrict__ rows, uint32_t n_rows, uint32_t *__restrict__ sizes,
                                                    uint8_t *__restrict__ d_status, unsigned long long *__restrict__ stats) {
    __shared__ unsigned long long s_failed[BB / 64], s_first[BB / 64];
    PackedTally tally;
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * BB + threadIdx.x; k < n_rows; k += static_cast<uint64_t>(gridDim.x) * BB) {
        const Judged rec = judge_record(store, rows[k]);
        sizes[k] = rec.status ? 0u : static_cast<uint32_t>(rec.len);
        if (d_status) d_status[k] = static_cast<uint8_t>(rec.status);
        tally.note(static_cast<uint32_t>(k), rec.status);
    }
    tally_lanes(tally, s_failed, s_first, stats);
}

// k_packed_gather: k_packed_decode with row k's job made from rows[k]: out_index[k + 1] - out_index[k] symbols (the room
// k_gather_plan gave it) from the body d_bodies[body_index[r], body_index[r + 1]) to d_out + out_index[k].  A row without room
// (failed, or of length zero) is passed over without a look at its record; a row with room was judged by k_gather_plan, so its
// pairs are believed.  d_written[k] (may be null) = symbols stored.  Nothing is decoded when out_index[n_rows] > cap.  The failure
// counters in `stats` are k_gather_plan's; this kernel adds the short rows, and its last workgroup reports.  LDS as k_batch_decode.
__global__ __launch_bounds__(BB) void k_packed_gather(PackedStore store, const uint32_t *__restrict__ rows, uint32_t n_rows, uint8_t *__restrict__ d_out, uint64_t cap,
                                                      const uint64_t *__restrict__ out_index, const uint2 *__restrict__ codes, uint32_t n_codes,
                                                      uint32_t *__restrict__ d_written, PackedReport report, uint32_t *__restrict__ counter) {
    __shared__ BatchDecLds s;
    const uint32_t tid = threadIdx.x;
    const uint8_t *d_bodies = static_cast<const uint8_t *>(store.bodies);
    const uint64_t out_bytes = out_index[n_rows];
    PackedTally tally;
    if (out_bytes <= cap) {
        load_tables(s.t, codes, n_codes);
        for (uint32_t k = blockIdx.x; k < n_rows; k += gridDim.x) {
            const uint64_t o0 = out_index[k], o1 = out_index[k + 1];
            uint32_t done = 0;
            if (o1 > o0) {  // (the same for every lane)
                const uint32_t r = rows[k], count = static_cast<uint32_t>(o1 - o0);
                const uint64_t b0 = store.body_index[r], b1 = store.body_index[r + 1];
                if (b1 > b0) done = decode_stream(s, n_codes, body_bits_of(d_bodies, b0, static_cast<uint32_t>(clip_body(b1 - b0, count))), d_out + o0, count, count);
                if (tid == 0 && done < count) ++tally.n_short;  // (an empty body under a length above zero is a short one)
            }
            if (tid == 0 && d_written) d_written[k] = done;
        }
    }
    if (tid == 0) packed_report(tally, out_bytes, report, counter);
}

// --------------------------------------------------------------------------------
// The match call: which records of a packed store begin with (or equal) a needle, decided on the compressed bytes.  Under one
// complete prefix-free table a record's text begins with the needle exactly when its body begins with the needle's codewords, its
// length is at least the needle's and its body holds those bits; equality asks for the same length.  The host encodes the needle;
// no table comes to the device.  Three launches in stream order (et_batch.h), the host waiting for the second alone.
// --------------------------------------------------------------------------------
// The end of a tile of a flag kernel (k_match_flag, k_join_flag): the ballot of the lanes whose record is selected is the wavefront's
// mask, the four popcounts meet in s_count[set] -- two sets: a tile's counts are read while the next tile's are stored -- and thread 0
// stores their sum as the tile's count.  One barrier.
__device__ __forceinline__ void end_tile(bool selected, uint32_t tile, uint32_t set, const TileWs &tiles, uint32_t (*s_count)[BB / 64]) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(selected);
    if (lane == 0) {
        tiles.masks[static_cast<uint64_t>(tile) * (MATCH_TILE / 64) + wave] = mask;
        s_count[set][wave] = __popcll(mask);
    }
    __syncthreads();
    if (threadIdx.x == 0) tiles.counts[tile] = s_count[set][0] + s_count[set][1] + s_count[set][2] + s_count[set][3];
}

// k_match_flag: a workgroup takes tiles of 256 consecutive records, one per lane, so both offset arrays are read coalesced.  A lane
// whose record can match (valid, the length fits, the body holds the pattern's bytes) compares the pattern's first 8 bytes alone:
// the aligned 8-byte words that hold them -- one, or two; each holds a byte of the body -- shifted into place, against job.head
// under job.head_mask.  Where the pattern is longer, the lanes that passed are taken one at a time from the ballot and all 64
// lanes compare 4 bytes each per step (aligned words that hold a byte of THAT body, shifted), the wavefront leaving at the first
// step with a mismatch: keys share long prefixes, and one lane walking 16 KiB alone would hold its wavefront.  The pattern's last
// byte counts with its top pat_bits % 8 bits only: the body's next codeword begins behind them.
// A failed record is never read and never selected.  LDS: 8 + 8 + 8 words.
__global__ __launch_bounds__(BB) void k_match_flag(PackedStore store, const uint32_t *__restrict__ pattern, MatchJob job, TileWs tiles, uint8_t *__restrict__ d_status,
                                                   unsigned long long *__restrict__ stats) {
    __shared__ unsigned long long s_failed[BB / 64], s_first[BB / 64];
    __shared__ uint32_t s_count[2][BB / 64];
    constexpr uint32_t HEAD_BYTES = MATCH_HEAD_BITS / 8;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint8_t *d_bodies = static_cast<const uint8_t *>(store.bodies);
    const uint32_t pat_bytes = (job.pat_bits + 7) >> 3, head_bytes = pat_bytes < HEAD_BYTES ? pat_bytes : HEAD_BYTES;
    const uint32_t last_bits = job.pat_bits & 7;
    const uint32_t n_tiles = (store.n + MATCH_TILE - 1) / MATCH_TILE;
    const bool equal = job.flags & MATCH_F_EQUAL, negate = job.flags & MATCH_F_NOT, never = job.flags & MATCH_F_NEVER;
    PackedTally tally;
    uint32_t set = 0;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, set ^= 1) {
        const uint32_t b = tile * MATCH_TILE + tid;  // (n <= 0x7fffffff: no wrap)
        bool valid = false, hit = false;
        uint64_t b0 = 0;
        if (b < store.n) {
            const Judged rec = judge_record(store, b);
            if (d_status) d_status[b] = static_cast<uint8_t>(rec.status);
            tally.note(b, rec.status);
            if (!rec.status) {
                valid = true;
                b0 = rec.b0;
                hit = !never && (equal ? rec.len == job.needle_len : rec.len >= job.needle_len) && rec.nb >= pat_bytes;
                if (hit && head_bytes) {
                    const uintptr_t a = reinterpret_cast<uintptr_t>(d_bodies) + b0;
                    const uint64_t *q = reinterpret_cast<const uint64_t *>(a & ~static_cast<uintptr_t>(7));
                    const uint32_t lead = static_cast<uint32_t>(a & 7);
                    uint64_t v = q[0] >> (8 * lead);
                    if (lead + head_bytes > 8) v |= q[1] << (64 - 8 * lead);  // (lead > 0 here; q[1] holds a byte of the head)
                    hit = ((v ^ job.head) & job.head_mask) == 0;
                }
            }
        }
        if (pat_bytes > HEAD_BYTES) {  // (the same for every lane)
            unsigned long long survivors = __ballot(hit);
            while (survivors) {
                const int src = __ffsll(survivors) - 1;
                survivors &= survivors - 1;
                const uintptr_t body = reinterpret_cast<uintptr_t>(d_bodies) + __shfl(b0, src, 64);
                bool same = true;
                for (uint32_t step = HEAD_BYTES; step < pat_bytes; step += 64 * 4) {
                    const uint32_t off = step + lane * 4;
                    bool differs = false;
                    if (off < pat_bytes) {
                        const uint32_t nb = pat_bytes - off < 4 ? pat_bytes - off : 4;
                        const uintptr_t a = body + off;
                        const uint32_t *w = reinterpret_cast<const uint32_t *>(a & ~static_cast<uintptr_t>(3));
                        const uint32_t lead = static_cast<uint32_t>(a & 3);
                        uint32_t v = w[0] >> (8 * lead);
                        if (lead + nb > 4) v |= w[1] << (32 - 8 * lead);  // (lead > 0 here; w[1] holds one of the nb bytes)
                        uint32_t m = nb == 4 ? 0xffffffffu : (1u << (8 * nb)) - 1u;
                        if (off + nb == pat_bytes && last_bits) m &= ~(((1u << (8 - last_bits)) - 1u) << (8 * (nb - 1)));
                        differs = ((v ^ pattern[off >> 2]) & m) != 0;
                    }
                    if (__any(differs)) {
                        same = false;
                        break;
                    }
                }
                if (static_cast<int>(lane) == src) hit = same;
            }
        }
        end_tile(valid && hit != negate, tile, set, tiles, s_count);
    }
    tally_lanes(tally, s_failed, s_first, stats);
}

// k_order_flag: k_match_flag's tiles for the order modes (et_batch.h): is the record's stored text -- its first min(length,
// codewords that end inside the body) symbols -- below the needle, equal to it, or above?  With B = the body's bits, P = pat_bits,
// K = n_coded and d = the first bit below min(B, P) at which body and pattern differ (MSB-first: the lowest differing byte, its
// highest differing bit):
//   d found      i = the needle's codeword d lies in (starts[i] <= d < starts[i + 1], i < K).  i >= length: the text is needle[:length],
//                a proper prefix: LESS.  Else the body's codeword at bit starts[i] -- it begins where the needle's does, the bits
//                in front agree -- ends beyond B: the text is needle[:i], LESS; or inside: its symbol differs from needle[i] (a
//                prefix-free code: different bits inside the needle's codeword are another codeword) and the bytes decide.
//   none, B < P  the body is a prefix of the pattern, the text a proper prefix of the needle: LESS.
//   none, P <= B length < K: LESS.  length == K: EQUAL, or LESS where a byte without a code follows in the needle (the tail byte t).
//                length > K: the codeword at bit P ends beyond B: as length == K; inside: GREATER, or with a tail byte its symbol
//                against t (no record holds t: they differ).
// The pad bits behind a body's last codeword decide nothing: a difference there has i >= length or a codeword that ends beyond B.
// The head: the aligned 8-byte words that hold the body's first min(8, bytes) bytes -- one, or two -- shifted into place; what lies
// behind the body's bytes in them is garbage that d < min(B, P) keeps out.  Where the first MATCH_HEAD_BITS agree and more can be
// compared, the lanes are taken one at a time from the ballot and all 64 compare 4 bytes each per step (k_match_flag's loads), the
// wavefront leaving at the first step with a difference, whose lowest lane's bit goes back to the owner.  A lane then makes at
// most one binary search in `starts` and decodes at most one codeword.  A failed record is never read and never selected.
// LDS: the sorted codes (2 KiB) + 8 + 8 + 8 words.
__global__ __launch_bounds__(BB) void k_order_flag(PackedStore store, const uint2 *__restrict__ codes, uint32_t n_codes, const uint32_t *__restrict__ pattern,
                                                   const uint32_t *__restrict__ starts, OrderJob job, TileWs tiles, uint8_t *__restrict__ d_status,
                                                   unsigned long long *__restrict__ stats) {
    __shared__ uint2 s_codes[256];
    __shared__ unsigned long long s_failed[BB / 64], s_first[BB / 64];
    __shared__ uint32_t s_count[2][BB / 64];
    constexpr uint32_t HEAD_BYTES = MATCH_HEAD_BITS / 8, NONE = 0xffffffffu;
    enum : uint32_t { LESS = 0, EQUAL = 1, GREATER = 2 };
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint8_t *d_bodies = static_cast<const uint8_t *>(store.bodies);
    const uint32_t P = job.pat_bits, K = job.n_coded;
    const uint32_t n_tiles = (store.n + MATCH_TILE - 1) / MATCH_TILE;
    const bool equal_too = job.flags & ORDER_F_EQUAL_TOO, negate = job.flags & MATCH_F_NOT, tail = job.flags & ORDER_F_TAIL;
    if (tid < n_codes) s_codes[tid] = codes[tid];
    __syncthreads();
    PackedTally tally;
    uint32_t set = 0;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, set ^= 1) {
        const uint32_t b = tile * MATCH_TILE + tid;  // (n <= 0x7fffffff: no wrap)
        bool valid = false, walk_on = false;
        uint64_t b0 = 0, len = 0;
        uint32_t B = 0, m = 0, d = NONE;  // the body's bits (clipped: below), min(B, P), the first differing bit below m
        if (b < store.n) {
            const Judged rec = judge_record(store, b);
            if (d_status) d_status[b] = static_cast<uint8_t>(rec.status);
            tally.note(b, rec.status);
            if (!rec.status) {
                valid = true;
                b0 = rec.b0;
                len = rec.len;
                // (no bit beyond P + 32 is asked for: a longer body counts as one that holds them all)
                B = static_cast<uint32_t>(rec.nb < MATCH_PATTERN_BYTES + 8 ? rec.nb : MATCH_PATTERN_BYTES + 8) * 8;
                m = B < P ? B : P;
                if (m) {
                    const uint32_t head_bytes = (m + 7) >> 3 < HEAD_BYTES ? (m + 7) >> 3 : HEAD_BYTES;  // (of the body: m <= B)
                    const uintptr_t a = reinterpret_cast<uintptr_t>(d_bodies) + b0;
                    const uint64_t *q = reinterpret_cast<const uint64_t *>(a & ~static_cast<uintptr_t>(7));
                    const uint32_t lead = static_cast<uint32_t>(a & 7);
                    uint64_t v = q[0] >> (8 * lead);
                    if (lead + head_bytes > 8) v |= q[1] << (64 - 8 * lead);  // (lead > 0 here; q[1] holds a byte of the head)
                    const uint64_t x = __builtin_bswap64(v) ^ job.head;
                    const uint32_t at = x ? static_cast<uint32_t>(__clzll(x)) : 64u;
                    if (at < (m < MATCH_HEAD_BITS ? m : MATCH_HEAD_BITS)) d = at;
                    else walk_on = m > MATCH_HEAD_BITS;
                }
            }
        }
        if (P > MATCH_HEAD_BITS) {  // (the same for every lane)
            unsigned long long pending = __ballot(walk_on);
            while (pending) {
                const int src = __ffsll(pending) - 1;
                pending &= pending - 1;
                const uintptr_t body = reinterpret_cast<uintptr_t>(d_bodies) + __shfl(b0, src, 64);
                const uint32_t m_src = __shfl(m, src, 64), cmp_bytes = (m_src + 7) >> 3;  // (of that body, and of the pattern)
                uint32_t found = NONE;
                for (uint32_t step = HEAD_BYTES; step < cmp_bytes; step += 64 * 4) {
                    const uint32_t off = step + lane * 4;
                    uint32_t x = 0;
                    if (off < cmp_bytes) {
                        const uint32_t nb = cmp_bytes - off < 4 ? cmp_bytes - off : 4;
                        const uintptr_t a = body + off;
                        const uint32_t *w = reinterpret_cast<const uint32_t *>(a & ~static_cast<uintptr_t>(3));
                        const uint32_t lead = static_cast<uint32_t>(a & 3);
                        uint32_t v = w[0] >> (8 * lead);
                        if (lead + nb > 4) v |= w[1] << (32 - 8 * lead);  // (lead > 0 here; w[1] holds one of the nb bytes)
                        x = (v ^ pattern[off >> 2]) & (nb == 4 ? 0xffffffffu : (1u << (8 * nb)) - 1u);
                    }
                    const unsigned long long differ = __ballot(x != 0);
                    if (differ) {  // the lowest lane holds the lowest bytes; its first differing bit in stream order
                        const uint32_t at = off * 8 + static_cast<uint32_t>(__clz(static_cast<int>(__builtin_bswap32(x))));
                        found = __shfl(at, __ffsll(differ) - 1, 64);
                        break;
                    }
                }
                if (static_cast<int>(lane) == src && found < m_src) d = found;  // (behind m: the pattern's last byte, beyond its bits)
            }
        }
        bool selected = false;
        if (valid) {
            uint32_t cmp = LESS, at = NONE, against = 0, cut = LESS;  // decode at bit `at`: `cut` if the codeword ends beyond B, else its symbol against `against`
            if (d != NONE) {
                uint32_t lo = 0, hi = K;  // starts[lo] >> 8 <= d < starts[hi] >> 8 = P throughout
                while (hi - lo > 1) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if ((starts[mid] >> 8) <= d) lo = mid; else hi = mid;
                }
                if (lo < len) {
                    const uint32_t e = starts[lo];
                    at = e >> 8;
                    against = e & 0xffu;
                }
            } else if (B >= P && len >= K) {
                cut = tail ? LESS : EQUAL;
                if (len == K) cmp = cut;
                else {
                    at = P;
                    against = starts[K] & 0xffu;  // the tail byte; 0 without one: no symbol is below it, GREATER
                }
            }
            if (at != NONE) {
                const uint32_t left = B - at;  // (at <= P <= B, or at <= d < B); the window is zero beyond B
                cmp = cut;                     // no bit left: no byte of the body is there to read
                if (left) {
                    const BodyBits g = body_bits_of(d_bodies, b0, B >> 3);
                    uint32_t win = body_window(g, g.first_bit + at);
                    if (left < 32) win &= ~(0xffffffffu >> left);
                    const uint32_t meta = search_codes(s_codes, n_codes, win);
                    if ((meta >> 8) <= left) cmp = (meta & 0xffu) < against ? LESS : GREATER;
                }
            }
            selected = (cmp == LESS || (equal_too && cmp == EQUAL)) != negate;
        }
        end_tile(selected, tile, set, tiles, s_count);
    }
    tally_lanes(tally, s_failed, s_first, stats);
}

// k_rows_emit (the match's and the join's last launch): a tile per trip, a record per lane: the tile's four masks (the same 32 bytes
// for every lane), the record's rank among the tile's selected ones by popcounts, its number to rows[base[tile] + rank] -- ascending,
// as tiles and ranks are -- and, KEYS, its key's (key_of[record]) to key_rows at the same place.  Every workgroup returns at once when
// the rows do not fit: ET_ERR_CAP writes nothing.  No LDS.
template <bool KEYS>
__global__ __launch_bounds__(BB) void k_rows_emit(const unsigned long long *__restrict__ masks, const uint64_t *__restrict__ base, uint32_t n_tiles,
                                                  uint32_t *__restrict__ rows, uint64_t cap_rows, const uint32_t *__restrict__ key_of, uint32_t *__restrict__ key_rows) {
    if (base[n_tiles] > cap_rows) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const unsigned long long *m = masks + static_cast<uint64_t>(tile) * (MATCH_TILE / 64);
        const unsigned long long mine = m[wave];
        if (!((mine >> lane) & 1)) continue;
        uint32_t rank = __popcll(mine & ((1ull << lane) - 1ull));
        for (uint32_t w = 0; w < wave; ++w) rank += __popcll(m[w]);
        const uint32_t record = tile * MATCH_TILE + tid;
        rows[base[tile] + rank] = record;
        if (KEYS) key_rows[base[tile] + rank] = key_of[record];
    }
}

// --------------------------------------------------------------------------------
// The search call: which records of a packed store contain (or end with) a needle, and at which symbol, decided on the compressed
// bytes.  Under one complete prefix-free table the needle occurs at symbol i of a record's stored text exactly when the pattern's
// bits (et_encode_pattern) lie at the bit where codeword i begins, they end inside the body, and i + needle_len <= length: the
// parse from a boundary is unique, the same bits at a bit that is no boundary are no occurrence, and the length rejects what the
// pad bits behind the last codeword read as.  So a search is the decode's walk over the boundaries with a bit comparison at each
// and nothing written.  Four launches in stream order (et_batch.h), the host waiting for the scan alone.
// Every loop is bounded: a lane's walk by the record's length (a trip per symbol), the workgroup's by the body's blocks, its fixed
// point by 256 trips and a lane's walk inside it by its 256 bits -- a complete table (the host's require_complete) makes every step
// advance.  No workgroup waits for another: k_search_long corrects a mask and a count by atomics nobody waits for.
// --------------------------------------------------------------------------------
struct SearchLds {  // k_search_flag's tables: 7 KiB
    CodeTables t;
    uint32_t pat[SEARCH_PATTERN_BYTES / 4];  // the pattern, big-endian words: bit q of it is bit 31 - q % 32 of word q / 32
};

// Do the pattern's bits behind its first 32 lie behind bit `at` + 32 of the body?  The caller has compared the first 32 and knows
// that at + pat_bits <= end_bit: every word compared under the mask holds a byte of the body.
__device__ __forceinline__ bool confirm_rest(const uint32_t *pat, uint32_t pat_bits, const BodyBits &g, uint32_t at) {
    for (uint32_t q = 32; q < pat_bits; q += 32) {
        const uint32_t left = pat_bits - q, mask = left >= 32 ? 0xffffffffu : ~(0xffffffffu >> left);
        if ((body_window(g, at + q) ^ pat[q >> 5]) & mask) return false;
    }
    return true;
}

// One lane, one body of a few words, from global memory: a trip per symbol.  At boundary idx (CONTAINS: every one up to `target` =
// length - needle_len, the last at which an occurrence fits the length; SUFFIX: `target` alone) the pattern is compared -- its head
// against the window the step needs anyway, the rest by confirm_rest --, then the codeword there is stepped over.  Returns the
// lowest boundary with an occurrence, or SEARCH_NONE.  64 bits of body are kept in registers and move on a word at a time.
__device__ __forceinline__ uint32_t search_lane(const SearchLds &s, uint32_t n_codes, const SearchJob &job, const BodyBits &g, uint32_t target) {
    const bool suffix = job.flags & SEARCH_F_SUFFIX;
    uint32_t pos = g.first_bit, k = 0;
    uint64_t two = (body_word_be(g, 0) << 32) | body_word_be(g, 1);
    for (uint32_t idx = 0; idx <= target; ++idx) {
        if ((pos >> 5) != k) {  // (a codeword has at most 32 bits: one word on)
            k = pos >> 5;
            two = (two << 32) | body_word_be(g, k + 1);
        }
        const uint32_t win = static_cast<uint32_t>((two << (pos & 31)) >> 32);
        if (!suffix || idx == target) {
            if (pos + job.pat_bits > g.end_bit) return SEARCH_NONE;  // (nor does it fit at a later boundary)
            if (((win ^ job.head) & job.head_mask) == 0 && confirm_rest(s.pat, job.pat_bits, g, pos)) return idx;
        }
        pos += code_at(s.t, n_codes, win) >> 8;
        if (pos > g.end_bit) return SEARCH_NONE;  // the bits ran out inside this codeword: no boundary behind it
    }
    return SEARCH_NONE;
}

// k_search_flag: k_match_flag's tiles, judgement, status bytes, tally, masks and counts, with the sorted codes, the first-level table
// and the pattern in LDS once per workgroup.  A valid record whose length or body cannot hold the needle has no occurrence and is not
// read; the empty needle is decided without a walk where the answer needs none; a body of up to SEARCH_LANE_BYTES is walked by its
// lane (search_lane); a longer one goes onto long_list -- one atomic per wavefront that has any -- and counts as "no occurrence"
// here: k_search_long corrects the records that have one.  pos_of[b] = the position, or SEARCH_NONE.  LDS 7 KiB + 24 words.
__global__ __launch_bounds__(BB) void k_search_flag(PackedStore store, const uint2 *__restrict__ codes, uint32_t n_codes, const uint32_t *__restrict__ pattern, SearchJob job,
                                                    TileWs tiles, uint32_t *__restrict__ pos_of, uint32_t *__restrict__ long_list, uint8_t *__restrict__ d_status,
                                                    unsigned long long *__restrict__ stats) {
    __shared__ SearchLds s;
    __shared__ unsigned long long s_failed[BB / 64], s_first[BB / 64];
    __shared__ uint32_t s_count[2][BB / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint8_t *d_bodies = static_cast<const uint8_t *>(store.bodies);
    const uint32_t n_tiles = (store.n + MATCH_TILE - 1) / MATCH_TILE;
    const bool suffix = job.flags & SEARCH_F_SUFFIX, negate = job.flags & MATCH_F_NOT, never = job.flags & MATCH_F_NEVER;
    const uint32_t pat_bytes = (job.pat_bits + 7) >> 3;
    if (tid < (job.pat_bits + 31) >> 5) s.pat[tid] = __builtin_bswap32(pattern[tid]);  // (at most 256 words)
    load_tables(s.t, codes, n_codes);
    __syncthreads();
    PackedTally tally;
    uint32_t set = 0;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, set ^= 1) {
        const uint32_t b = tile * MATCH_TILE + tid;  // (n <= 0x7fffffff: no wrap)
        bool valid = false, is_long = false;
        uint32_t pos = SEARCH_NONE;
        if (b < store.n) {
            const Judged rec = judge_record(store, b);
            if (d_status) d_status[b] = static_cast<uint8_t>(rec.status);
            tally.note(b, rec.status);
            if (!rec.status) {
                valid = true;
                if (!never && rec.len >= job.needle_len && rec.nb >= pat_bytes) {
                    const uint32_t len = static_cast<uint32_t>(rec.len);
                    if (!job.pat_bits && (!suffix || len == 0)) pos = 0;  // the empty needle: everywhere; at the end of an empty record
                    else if (rec.nb == 0) pos = SEARCH_NONE;              // ... and not at the end of a text that is not there
                    else if (rec.nb <= SEARCH_LANE_BYTES) pos = search_lane(s, n_codes, job, body_bits_of(d_bodies, rec.b0, static_cast<uint32_t>(clip_body(rec.nb, len))), len - job.needle_len);
                    else is_long = true;
                }
                pos_of[b] = pos;
            }
        }
        const unsigned long long longs = __ballot(is_long);
        if (longs) {  // (the same for the whole wavefront)
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(stats + SEARCH_N_LONG, static_cast<unsigned long long>(__popcll(longs)));
            base = __shfl(base, 0, 64);
            if (is_long) long_list[base + __popcll(longs & ((1ull << lane) - 1ull))] = b;
        }
        end_tile(valid && (pos != SEARCH_NONE) != negate, tile, set, tiles, s_count);
    }
    tally_lanes(tally, s_failed, s_first, stats);
}

// Do the pattern's bits lie at bit `at` of the body, where the 32-bit window is `win`?  The head against the window, a pass confirmed on
// the rest from global memory (an occurrence may run past the lane's bits and past the staged block).
__device__ __forceinline__ bool pattern_at(const SearchJob &job, const uint32_t *pat, const BodyBits &g, uint32_t at, uint32_t win) {
    return ((win ^ job.head) & job.head_mask) == 0 && at + job.pat_bits <= g.end_bit && confirm_rest(pat, job.pat_bits, g, at);
}

// CONTAINS, the visitor of the fixed point's walks: the pattern compared at every codeword on the way, with the window the step holds
// anyway.  hit = how many codewords of THIS walk lie in front of the first occurrence (SEARCH_NONE: none); `at` = the bit of the body's
// aligned base at which the lane's bits begin.
struct SeekPattern {
    const SearchJob *job;
    const uint32_t *pat;
    const BodyBits *g;
    uint32_t at, hit;
    __device__ __forceinline__ bool operator()(uint32_t cnt, uint32_t pos, uint32_t win, uint32_t) {
        if (hit == SEARCH_NONE && pattern_at(*job, pat, *g, at + pos, win)) hit = cnt;
        return true;
    }
};

// One record by the whole workgroup under the tables in `s`: decode_stream's blocks without its write half.  CONTAINS compares inside
// the fixed point's walks (SeekPattern) and believes what each lane's LAST walk found, which is the settled walk's: a third pass over
// the bits, after the scan, cost as much as the write pass it replaced.  A lane's hit becomes a symbol number once the scan has given
// its first codeword's, and counts when the length allows it (a lane's later hits lie further on).  SUFFIX settles by a counting walk
// and compares at one boundary: the lane whose codewords hold number `target` walks to it again -- the settled walk counted it, so the
// walk gets there -- and compares; of the empty needle it asks only whether boundary `target` = length exists.  The lowest hit is
// reduced over the workgroup through s_min (4 words, free again at the next block's first barrier); the blocks end with the first that
// has one, or once `target` boundaries lie behind.
__device__ __forceinline__ uint32_t search_stream(BatchDecLds &s, uint32_t n_codes, const BodyBits &g, uint32_t target, const SearchJob &job, const uint32_t *pat,
                                                  uint32_t *s_min) {
    const uint32_t tid = threadIdx.x;
    const bool suffix = job.flags & SEARCH_F_SUFFIX;
    const uint32_t n_blocks = (g.n_words + DEC_WORDS - 1) / DEC_WORDS;
    uint32_t start = g.first_bit, done = 0;  // the block's first codeword; boundaries so far
    for (uint32_t blk = 0; blk < n_blocks && done <= target; ++blk) {
        const uint32_t at = blk * DEC_WORDS * 32 + tid * 256;
        JustCount counting;
        SeekPattern seek{&job, pat, &g, at, SEARCH_NONE};
        const Settled b = suffix ? settle_block(s, n_codes, g, blk, start, counting) : settle_block(s, n_codes, g, blk, start, seek);
        const uint32_t first = done + b.first;
        uint32_t found = SEARCH_NONE;
        if (!suffix) {
            if (seek.hit != SEARCH_NONE && first + seek.hit <= target) found = first + seek.hit;
        } else if (!job.pat_bits) {
            if (done + b.total >= target) found = target;  // (the same for every lane)
        } else if (first <= target && target < first + b.count) {
            uint32_t again;
            (void)walk(s, n_codes, b.used, b.room, &again, [&](uint32_t cnt, uint32_t pos, uint32_t win, uint32_t) {
                if (first + cnt != target) return true;
                if (pattern_at(job, pat, g, at + pos, win)) found = target;
                return false;
            });
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const uint32_t other = __shfl_xor(found, d, 64);
            if (other < found) found = other;
        }
        if ((tid & 63) == 0) s_min[tid >> 6] = found;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < BB / 64; ++w)
            if (s_min[w] < found) found = s_min[w];
        if (found != SEARCH_NONE) return found;  // (the same for every lane; boundaries ascend with the blocks: the lowest)
        start = b.start;
        done += b.total;
    }
    return SEARCH_NONE;
}


// k_search_long: k_packed_decode's shape over long_list -- the sorted codes and the first-level table once per workgroup, the listed
// records strided; the pattern (big-endian words) and the reduction's 4 words lie in the stage the decode keeps its symbols in.  A
// workgroup beyond the list returns before it sets anything up: a store of short records pays a launch of empty workgroups.  A record
// with an occurrence: pos_of[b] = its position, and thread 0 turns the record's bit of its tile's mask and moves the tile's count by
// one (k_search_flag left "no occurrence" there; the scan runs behind this kernel).  LDS as k_batch_decode.
__global__ __launch_bounds__(BB) void k_search_long(PackedStore store, const uint2 *__restrict__ codes, uint32_t n_codes, const uint32_t *__restrict__ pattern, SearchJob job,
                                                    TileWs tiles, uint32_t *__restrict__ pos_of, const uint32_t *__restrict__ long_list,
                                                    const unsigned long long *__restrict__ stats) {
    __shared__ BatchDecLds s;
    static_assert(SEARCH_PATTERN_BYTES / 4 + BB / 64 <= sizeof(s.out) / 4, "the pattern and s_min in the symbol stage");
    const uint32_t tid = threadIdx.x;
    const uint32_t n_long = static_cast<uint32_t>(stats[SEARCH_N_LONG]);
    if (blockIdx.x >= n_long) return;
    uint32_t *pat = s.out, *s_min = s.out + SEARCH_PATTERN_BYTES / 4;
    if (tid < (job.pat_bits + 31) >> 5) pat[tid] = __builtin_bswap32(pattern[tid]);
    load_tables(s.t, codes, n_codes);
    const uint8_t *d_bodies = static_cast<const uint8_t *>(store.bodies);
    for (uint32_t i = blockIdx.x; i < n_long; i += gridDim.x) {
        const uint32_t b = long_list[i];
        const Judged rec = judge_record(store, b);
        if (rec.status || rec.len < job.needle_len || rec.nb == 0) continue;  // (k_search_flag lists no such record; the same for every lane)
        const uint32_t len = static_cast<uint32_t>(rec.len);
        const uint32_t found = search_stream(s, n_codes, body_bits_of(d_bodies, rec.b0, static_cast<uint32_t>(clip_body(rec.nb, len))), len - job.needle_len, job, pat, s_min);
        if (tid == 0 && found != SEARCH_NONE) {
            pos_of[b] = found;
            const unsigned long long bit = 1ull << (b & 63);
            if (job.flags & MATCH_F_NOT) {
                atomicAnd(tiles.masks + (b >> 6), ~bit);
                atomicSub(tiles.counts + b / MATCH_TILE, 1u);
            } else {
                atomicOr(tiles.masks + (b >> 6), bit);
                atomicAdd(tiles.counts + b / MATCH_TILE, 1u);
            }
        }
    }
}

// --------------------------------------------------------------------------------
// The join call: which records of a packed store equal SOME key of a key set, itself a packed store under the same table, decided on
// the compressed bytes.  Under one table the encoder is deterministic, so two records have the same text exactly when they have the
// same length (symbols), the same body byte count and the same body bytes -- for bodies as the encoders write them; a body of no
// bytes under a length above zero (a record kept raw elsewhere) equals nothing, on either side.  The keys go into a hash table in the
// workspace (et_join.h: the hash, a slot = tag << 32 | key number, ET_JOIN_EMPTY), the records probe it, and every hit is confirmed by
// length, byte count and bytes.  The launches (et_batch.h) run in stream order, the host waiting for the scan alone.
// No workgroup waits for another: an insert is a compare-and-swap per slot visited, and every probe and insert loop ends after
// `slots` trips at the latest -- with a table at most half full it ends at an empty slot long before; a loop that runs out sets the
// fault bit (JOIN_FAULT_BIT of the records' failure count, which the scan reports as it is), and the host returns ET_ERR_HIP.
// --------------------------------------------------------------------------------
constexpr uint32_t JOIN_NONE = 0xffffffffu;  // key_of[b] of a record that equals no key

// Word i (8 i < nb) of the body of nb bytes at `body`, any alignment, zero-extended: from the aligned 8-byte words that hold a byte of
// it -- one, or two -- shifted into place, as k_match_flag reads its head.
__device__ __forceinline__ uint64_t body_word(uintptr_t body, uint64_t nb, uint64_t i) {
    const uint64_t left = nb - 8 * i;
    const uint32_t cnt = left < 8 ? static_cast<uint32_t>(left) : 8u;
    const uintptr_t a = body + 8 * i;
    const uint64_t *q = reinterpret_cast<const uint64_t *>(a & ~static_cast<uintptr_t>(7));
    const uint32_t lead = static_cast<uint32_t>(a & 7);
    uint64_t v = q[0] >> (8 * lead);
    if (lead + cnt > 8) v |= q[1] << (64 - 8 * lead);  // (lead > 0 here; q[1] holds one of the cnt bytes)
    if (cnt < 8) v &= (1ull << (8 * cnt)) - 1ull;
    return v;
}

// The sum of the hash's terms over a whole body by one lane, and over a body shared by the 64 lanes of a wavefront (every lane gets it).
__device__ __forceinline__ uint64_t lane_terms(uintptr_t body, uint64_t nb) {
    uint64_t sum = 0;
    for (uint64_t i = 0; 8 * i < nb; ++i) sum += et_join_term(i, body_word(body, nb, i));
    return sum;
}

__device__ __forceinline__ uint64_t wave_terms(uintptr_t body, uint64_t nb, uint32_t lane) {
    uint64_t sum = 0;
    for (uint64_t i = lane; 8 * i < nb; i += 64) sum += et_join_term(i, body_word(body, nb, i));
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    return sum;
}

// Are the nb bytes at a and at b the same?  By one lane; by a wavefront (the same answer in every lane), which leaves at the first
// step of 512 bytes with a difference.
__device__ __forceinline__ bool lane_same(uintptr_t a, uintptr_t b, uint64_t nb) {
    for (uint64_t i = 0; 8 * i < nb; ++i)
        if (body_word(a, nb, i) != body_word(b, nb, i)) return false;
    return true;
}

__device__ __forceinline__ bool wave_same(uintptr_t a, uintptr_t b, uint64_t nb, uint32_t lane) {
    for (uint64_t i0 = 0; 8 * i0 < nb; i0 += 64) {
        const uint64_t i = i0 + lane;
        const bool differs = 8 * i < nb && body_word(a, nb, i) != body_word(b, nb, i);
        if (__any(differs)) return false;
    }
    return true;
}

// The hash of one item per lane, called by whole wavefronts: a lane that wants one and whose body is at most JOIN_LANE_BYTES long walks
// it alone; the lanes with longer ones are taken one at a time from the ballot and the wavefront walks that body together.
__device__ __forceinline__ uint64_t join_hash_lanes(bool want, uintptr_t body, uint64_t nb, uint64_t len, uint32_t lane) {
    uint64_t h = 0;
    if (want && nb <= JOIN_LANE_BYTES) h = et_join_finish(lane_terms(body, nb), nb, len);
    unsigned long long longs = __ballot(want && nb > JOIN_LANE_BYTES);
    while (longs) {
        const int src = __ffsll(longs) - 1;
        longs &= longs - 1;
        const uint64_t sum = wave_terms(__shfl(static_cast<uint64_t>(body), src, 64), __shfl(nb, src, 64), lane);
        if (static_cast<int>(lane) == src) h = et_join_finish(sum, nb, len);
    }
    return h;
}

// An item as its kernel judged it: where its body lies, its byte count and its length.  Of a key in a slot: read again from the keys'
// offsets -- only a valid key is ever inserted.
struct JoinItem {
    uintptr_t body;
    uint64_t nb, len;
};

__device__ __forceinline__ JoinItem key_item(const PackedStore &keys, uint32_t k) {
    const uint64_t b0 = keys.body_index[k], b1 = keys.body_index[k + 1];
    return JoinItem{reinterpret_cast<uintptr_t>(keys.bodies) + b0, b1 - b0, keys.text_index[k + 1] - keys.text_index[k]};
}

// Key k into the table: linear probing from hash & slot_mask.  An empty slot is taken by compare-and-swap.  A slot with this tag
// holds a key that may be equal: if it is, the slot keeps the lower of the two numbers (atomicMin; the tags are the same) and the
// insert is over -- a slot never becomes empty again and keeps its content's text, so equal keys all end in the first slot of their
// common probe sequence that no other text holds, whatever the order.  false: `slots` trips without an end.
// WAVE: the whole wavefront inserts one key (the arguments are the same in every lane); lane 0 issues the atomics.
template <bool WAVE>
__device__ __forceinline__ bool join_insert(const PackedStore &keys, unsigned long long *table, uint64_t slot_mask, uint32_t k, uint64_t h, const JoinItem &me, uint32_t lane) {
    const unsigned long long word = (h & 0xffffffff00000000ull) | k;
    uint64_t pos = h & slot_mask;
    for (uint64_t trip = 0; trip <= slot_mask; ++trip, pos = (pos + 1) & slot_mask) {
        unsigned long long old = 0;
        if (!WAVE || lane == 0) old = atomicCAS(table + pos, ET_JOIN_EMPTY, word);
        if (WAVE) old = __shfl(old, 0, 64);
        if (old == ET_JOIN_EMPTY) return true;
        if ((old ^ word) >> 32) continue;
        const JoinItem other = key_item(keys, static_cast<uint32_t>(old));
        if (other.len != me.len || other.nb != me.nb) continue;
        if (!(WAVE ? wave_same(me.body, other.body, me.nb, lane) : lane_same(me.body, other.body, me.nb))) continue;
        if (!WAVE || lane == 0) atomicMin(table + pos, word);
        return true;
    }
    return false;
}

// The key that equals `me`, or JOIN_NONE: the probe sequence up to its first empty slot; a slot with the hash's tag is confirmed by
// length, byte count and bytes, and passed when they differ.  The table is final (k_join_build is over): plain loads.
template <bool WAVE>
__device__ __forceinline__ uint32_t join_probe(const PackedStore &keys, const unsigned long long *table, uint64_t slot_mask, uint64_t h, const JoinItem &me, uint32_t lane, bool *fault) {
    uint64_t pos = h & slot_mask;
    for (uint64_t trip = 0; trip <= slot_mask; ++trip, pos = (pos + 1) & slot_mask) {
        const unsigned long long slot = table[pos];
        if (slot == ET_JOIN_EMPTY) return JOIN_NONE;
        if ((slot ^ h) >> 32) continue;
        const JoinItem other = key_item(keys, static_cast<uint32_t>(slot));
        if (other.len != me.len || other.nb != me.nb) continue;
        if (WAVE ? wave_same(me.body, other.body, me.nb, lane) : lane_same(me.body, other.body, me.nb)) return static_cast<uint32_t>(slot);
    }
    *fault = true;
    return JOIN_NONE;
}

// k_join_build: tiles of 256 keys, one per lane.  A key is judged as k_match_flag judges a record, its status byte stored, its failure
// tallied into the keys' two counters; a valid key -- unless it is a body of no bytes under a length above zero, which equals
// nothing -- is hashed and inserted, alone up to JOIN_LANE_BYTES of body, by its wavefront above.  The smallest and largest body of
// the inserted keys go to JOIN_MIN and JOIN_MAX: one pair of atomics per workgroup.  LDS: 8 + 8 + 8 + 8 words.
__global__ __launch_bounds__(BB) void k_join_build(PackedStore keys, unsigned long long *__restrict__ table, uint64_t slot_mask, uint8_t *__restrict__ d_key_status,
                                                   unsigned long long *__restrict__ stats) {
    __shared__ unsigned long long s_failed[BB / 64], s_first[BB / 64], s_min[BB / 64], s_max[BB / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n_tiles = (keys.n + MATCH_TILE - 1) / MATCH_TILE;
    unsigned long long lo = ~0ull, hi = 0;
    PackedTally tally;
    bool fault = false;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t k = tile * MATCH_TILE + tid;  // (n <= 2^24: no wrap)
        bool enter = false;
        JoinItem me{0, 0, 0};
        if (k < keys.n) {
            const Judged rec = judge_record(keys, k);
            if (d_key_status) d_key_status[k] = static_cast<uint8_t>(rec.status);
            tally.note(k, rec.status);
            if (!rec.status) {
                me = JoinItem{reinterpret_cast<uintptr_t>(keys.bodies) + rec.b0, rec.nb, rec.len};
                enter = me.nb > 0 || me.len == 0;
                if (enter) {
                    if (me.nb < lo) lo = me.nb;
                    if (me.nb > hi) hi = me.nb;
                }
            }
        }
        const uint64_t h = join_hash_lanes(enter, me.body, me.nb, me.len, lane);
        if (enter && me.nb <= JOIN_LANE_BYTES && !join_insert<false>(keys, table, slot_mask, k, h, me, lane)) fault = true;
        unsigned long long longs = __ballot(enter && me.nb > JOIN_LANE_BYTES);
        while (longs) {
            const int src = __ffsll(longs) - 1;
            longs &= longs - 1;
            const JoinItem it{static_cast<uintptr_t>(__shfl(static_cast<uint64_t>(me.body), src, 64)), __shfl(me.nb, src, 64), __shfl(me.len, src, 64)};
            if (!join_insert<true>(keys, table, slot_mask, __shfl(k, src, 64), __shfl(h, src, 64), it, lane)) fault = true;
        }
    }
    if (fault) atomicOr(stats + PACKED_N_FAILED, JOIN_FAULT_BIT);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long other_lo = __shfl_xor(lo, d, 64), other_hi = __shfl_xor(hi, d, 64);
        if (other_lo < lo) lo = other_lo;
        if (other_hi > hi) hi = other_hi;
    }
    if (lane == 0) {
        s_min[wave] = lo;
        s_max[wave] = hi;
    }
    tally_lanes(tally, s_failed, s_first, stats + (JOIN_KEYS_FAILED - PACKED_N_FAILED));  // (the keys' pair of counters lies like the records')
    if (tid == 0) {
        for (int w = 0; w < BB / 64; ++w) {
            if (s_min[w] < lo) lo = s_min[w];
            if (s_max[w] > hi) hi = s_max[w];
        }
        if (lo <= hi) {  // (a key went in)
            atomicMin(stats + JOIN_MIN, lo);
            atomicMax(stats + JOIN_MAX, hi);
        }
    }
}

// k_join_flag: k_match_flag's tiles, judgement, status bytes, tally, masks and counts.  A valid record whose body is shorter than
// every inserted key's or longer (JOIN_MIN, JOIN_MAX: final, k_join_build is over) is decided without a look at its body -- a store
// of pages joined against short keys hashes no page -- as is the body of no bytes under a length above zero.  The others are hashed
// and probed: alone up to JOIN_LANE_BYTES of body, by their wavefront above.  key_of[b] = the key record b equals, or JOIN_NONE.
// Its first workgroup puts the keys' two counters -- final as well -- into the report, in front of the scan that hands it over; a
// tick per workgroup to find the last one costs more than the whole kernel (a device-scope fence each).  LDS: 8 + 8 + 8 words.
__global__ __launch_bounds__(BB) void k_join_flag(PackedStore recs, PackedStore keys, const unsigned long long *__restrict__ table, uint64_t slot_mask, uint32_t flags,
                                                  TileWs tiles, uint32_t *__restrict__ key_of, uint8_t *__restrict__ d_status, unsigned long long *stats,
                                                  unsigned long long *__restrict__ host_result) {
    __shared__ unsigned long long s_failed[BB / 64], s_first[BB / 64];
    __shared__ uint32_t s_count[2][BB / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t n_tiles = (recs.n + MATCH_TILE - 1) / MATCH_TILE;
    const bool negate = flags & MATCH_F_NOT;
    const unsigned long long lo = stats[JOIN_MIN], hi = stats[JOIN_MAX];
    if (blockIdx.x == 0 && tid == 0) {
        host_result[JOIN_KEYS_FAILED] = stats[JOIN_KEYS_FAILED];
        host_result[JOIN_KEYS_FIRST] = stats[JOIN_KEYS_FIRST];
        pinned_stores_visible();
    }
    PackedTally tally;
    bool fault = false;
    uint32_t set = 0;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, set ^= 1) {
        const uint32_t b = tile * MATCH_TILE + tid;  // (n <= 0x7fffffff: no wrap)
        bool valid = false, probe = false;
        JoinItem me{0, 0, 0};
        if (b < recs.n) {
            const Judged rec = judge_record(recs, b);
            if (d_status) d_status[b] = static_cast<uint8_t>(rec.status);
            tally.note(b, rec.status);
            if (!rec.status) {
                valid = true;
                me = JoinItem{reinterpret_cast<uintptr_t>(recs.bodies) + rec.b0, rec.nb, rec.len};
                probe = (me.nb > 0 || me.len == 0) && me.nb >= lo && me.nb <= hi;
            }
        }
        const uint64_t h = join_hash_lanes(probe, me.body, me.nb, me.len, lane);
        uint32_t key = JOIN_NONE;
        if (probe && me.nb <= JOIN_LANE_BYTES) key = join_probe<false>(keys, table, slot_mask, h, me, lane, &fault);
        unsigned long long longs = __ballot(probe && me.nb > JOIN_LANE_BYTES);
        while (longs) {
            const int src = __ffsll(longs) - 1;
            longs &= longs - 1;
            const JoinItem it{static_cast<uintptr_t>(__shfl(static_cast<uint64_t>(me.body), src, 64)), __shfl(me.nb, src, 64), __shfl(me.len, src, 64)};
            const uint32_t found = join_probe<true>(keys, table, slot_mask, __shfl(h, src, 64), it, lane, &fault);
            if (static_cast<int>(lane) == src) key = found;
        }
        if (b < recs.n) key_of[b] = key;
        end_tile(valid && (key != JOIN_NONE) != negate, tile, set, tiles, s_count);
    }
    if (fault) atomicOr(stats + PACKED_N_FAILED, JOIN_FAULT_BIT);
    tally_lanes(tally, s_failed, s_first, stats);
}

// k_join_hash: et_selftest_join_hash -- the hash of every valid record as k_join_build and k_join_flag compute it (join_hash_lanes).
__global__ __launch_bounds__(BB) void k_join_hash(PackedStore recs, uint64_t *__restrict__ d_hash) {
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t n_tiles = (recs.n + MATCH_TILE - 1) / MATCH_TILE;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t b = tile * MATCH_TILE + tid;
        bool valid = false;
        JoinItem me{0, 0, 0};
        if (b < recs.n) {
            const Judged rec = judge_record(recs, b);
            valid = !rec.status;
            if (valid) me = JoinItem{reinterpret_cast<uintptr_t>(recs.bodies) + rec.b0, rec.nb, rec.len};
        }
        const uint64_t h = join_hash_lanes(valid, me.body, me.nb, me.len, lane);
        if (valid) d_hash[b] = h;
    }
}

// --------------------------------------------------------------------------------
// The group call: which records of a packed store hold the same text, decided on the compressed bytes -- a join of the store with
// itself.  k_group_build is k_join_build with the store as its own key set; when it is over, the slot a valid record's probe sequence ends
// in holds the LOWEST number among the records of its text (the insert's atomicMin), whatever the order of the workgroups: that record
// is the group's representative, and its rank among the representatives -- the flag kernels' masks, counts and scan -- is the group's
// number.  A body of no bytes under a length above zero equals nothing: it was never inserted and is its own representative.
// Every probe loop ends after `slots` trips at the latest and sets the join's fault bit when it runs out; a valid record that was
// inserted always finds its text in front of the first empty slot, so an empty slot met here is the same fault.  No workgroup waits
// for another: the counts are added by atomics nobody waits for, behind the launch that zeroed them.
// --------------------------------------------------------------------------------
// The representative of `me`, record b of the store the table was built over: the probe sequence to the slot with the hash's tag that
// holds b itself -- no byte is looked at: b is the lowest of its text -- or a record that is confirmed by length, byte count and bytes.
template <bool WAVE>
__device__ __forceinline__ uint32_t group_probe(const PackedStore &recs, const unsigned long long *table, uint64_t slot_mask, uint64_t h, const JoinItem &me, uint32_t b,
                                                uint32_t lane, bool *fault) {
    uint64_t pos = h & slot_mask;
    for (uint64_t trip = 0; trip <= slot_mask; ++trip, pos = (pos + 1) & slot_mask) {
        const unsigned long long slot = table[pos];
        if (slot == ET_JOIN_EMPTY) break;
        if ((slot ^ h) >> 32) continue;
        if (static_cast<uint32_t>(slot) == b) return b;
        const JoinItem other = key_item(recs, static_cast<uint32_t>(slot));
        if (other.len != me.len || other.nb != me.nb) continue;
        if (WAVE ? wave_same(me.body, other.body, me.nb, lane) : lane_same(me.body, other.body, me.nb)) return static_cast<uint32_t>(slot);
    }
    *fault = true;
    return b;
}

// Record k into the table: join_insert for a store in which MOST records may hold one text.  There join_insert sends a failed
// compare-and-swap and an atomicMin per record to one slot (262 144 records, 90 % of them one text: 5.4 ms of a 5.4 ms call, DESIGN
// section 6).  Here the slot is LOADED first.  What a load returns may be old, but a slot only ever goes from empty to a text's word and
// from there to lower numbers of the same text, so an old value is never wrong, only late: "empty" is settled by the compare-and-swap;
// a word of another tag or text is passed; a word of this text BELOW k's means the slot holds a number no higher now and k has
// nothing to add -- no atomic at all, which is the case for nearly every record behind the first of its text --; a higher one gets
// the atomicMin.  false: `slots` trips without an end.  WAVE: as join_insert's.
template <bool WAVE>
__device__ __forceinline__ bool group_insert(const PackedStore &recs, unsigned long long *table, uint64_t slot_mask, uint32_t k, uint64_t h, const JoinItem &me, uint32_t lane) {
    const unsigned long long word = (h & 0xffffffff00000000ull) | k;
    uint64_t pos = h & slot_mask;
    for (uint64_t trip = 0; trip <= slot_mask; ++trip, pos = (pos + 1) & slot_mask) {
        unsigned long long old = 0;
        if (!WAVE || lane == 0) {
            old = __atomic_load_n(table + pos, __ATOMIC_RELAXED);
            if (old == ET_JOIN_EMPTY) old = atomicCAS(table + pos, ET_JOIN_EMPTY, word);
        }
        if (WAVE) old = __shfl(old, 0, 64);
        if (old == ET_JOIN_EMPTY) return true;
        if ((old ^ word) >> 32) continue;
        const JoinItem other = key_item(recs, static_cast<uint32_t>(old));
        if (other.len != me.len || other.nb != me.nb) continue;
        if (!(WAVE ? wave_same(me.body, other.body, me.nb, lane) : lane_same(me.body, other.body, me.nb))) continue;
        if (old > word && (!WAVE || lane == 0)) atomicMin(table + pos, word);
        return true;
    }
    return false;
}

// k_group_build: k_join_build's tiles over the store itself, less what the group call has no use for (status bytes and tally are
// k_group_flag's; no [min, max]): a valid record -- unless it is a body of no bytes under a length above zero -- is hashed, its hash
// kept for k_group_flag (hash_of[k]: the body is hashed once per call), and inserted by group_insert, alone up to JOIN_LANE_BYTES of
// body, by its wavefront above.  No LDS.
__global__ __launch_bounds__(BB) void k_group_build(PackedStore recs, unsigned long long *__restrict__ table, uint64_t slot_mask, uint64_t *__restrict__ hash_of,
                                                    unsigned long long *__restrict__ stats) {
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t n_tiles = (recs.n + MATCH_TILE - 1) / MATCH_TILE;
    bool fault = false;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t k = tile * MATCH_TILE + tid;  // (n <= 2^24: no wrap)
        bool enter = false;
        JoinItem me{0, 0, 0};
        if (k < recs.n) {
            const Judged rec = judge_record(recs, k);
            if (!rec.status) {
                me = JoinItem{reinterpret_cast<uintptr_t>(recs.bodies) + rec.b0, rec.nb, rec.len};
                enter = me.nb > 0 || me.len == 0;
            }
        }
        const uint64_t h = join_hash_lanes(enter, me.body, me.nb, me.len, lane);
        if (enter) hash_of[k] = h;
        if (enter && me.nb <= JOIN_LANE_BYTES && !group_insert<false>(recs, table, slot_mask, k, h, me, lane)) fault = true;
        unsigned long long longs = __ballot(enter && me.nb > JOIN_LANE_BYTES);
        while (longs) {
            const int src = __ffsll(longs) - 1;
            longs &= longs - 1;
            const JoinItem it{static_cast<uintptr_t>(__shfl(static_cast<uint64_t>(me.body), src, 64)), __shfl(me.nb, src, 64), __shfl(me.len, src, 64)};
            if (!group_insert<true>(recs, table, slot_mask, __shfl(k, src, 64), __shfl(h, src, 64), it, lane)) fault = true;
        }
    }
    if (fault) atomicOr(stats + PACKED_N_FAILED, JOIN_FAULT_BIT);
}

// k_group_flag: k_join_flag's tiles, judgement, status bytes, tally, masks and counts over the store the table was built from (final:
// k_group_build is over).  A valid record is probed with the hash the build kept -- alone up to JOIN_LANE_BYTES of body, by its
// wavefront above -- for its representative; the body of no bytes under a length above zero is its own without a probe.  rep_of[b] =
// the representative, or GROUP_NONE for a failed record; the flag of the tile's masks is "valid and its own representative".
// LDS: 8 + 8 + 8 words.
__global__ __launch_bounds__(BB) void k_group_flag(PackedStore recs, const unsigned long long *__restrict__ table, uint64_t slot_mask, const uint64_t *__restrict__ hash_of,
                                                   TileWs tiles, uint32_t *__restrict__ rep_of, uint8_t *__restrict__ d_status, unsigned long long *__restrict__ stats) {
    __shared__ unsigned long long s_failed[BB / 64], s_first[BB / 64];
    __shared__ uint32_t s_count[2][BB / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t n_tiles = (recs.n + MATCH_TILE - 1) / MATCH_TILE;
    PackedTally tally;
    bool fault = false;
    uint32_t set = 0;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, set ^= 1) {
        const uint32_t b = tile * MATCH_TILE + tid;  // (n <= 2^24: no wrap)
        bool valid = false, probe = false;
        JoinItem me{0, 0, 0};
        if (b < recs.n) {
            const Judged rec = judge_record(recs, b);
            if (d_status) d_status[b] = static_cast<uint8_t>(rec.status);
            tally.note(b, rec.status);
            if (!rec.status) {
                valid = true;
                me = JoinItem{reinterpret_cast<uintptr_t>(recs.bodies) + rec.b0, rec.nb, rec.len};
                probe = me.nb > 0 || me.len == 0;
            }
        }
        const uint64_t h = probe ? hash_of[b] : 0;  // (the build judged b as this kernel does: a record that is probed was hashed)
        uint32_t rep = valid ? b : GROUP_NONE;
        if (probe && me.nb <= JOIN_LANE_BYTES) rep = group_probe<false>(recs, table, slot_mask, h, me, b, lane, &fault);
        unsigned long long longs = __ballot(probe && me.nb > JOIN_LANE_BYTES);
        while (longs) {
            const int src = __ffsll(longs) - 1;
            longs &= longs - 1;
            const JoinItem it{static_cast<uintptr_t>(__shfl(static_cast<uint64_t>(me.body), src, 64)), __shfl(me.nb, src, 64), __shfl(me.len, src, 64)};
            const uint32_t found = group_probe<true>(recs, table, slot_mask, __shfl(h, src, 64), it, __shfl(b, src, 64), lane, &fault);
            if (static_cast<int>(lane) == src) rep = found;
        }
        if (b < recs.n) rep_of[b] = rep;
        end_tile(valid && rep == b, tile, set, tiles, s_count);
    }
    if (fault) atomicOr(stats + PACKED_N_FAILED, JOIN_FAULT_BIT);
    tally_lanes(tally, s_failed, s_first, stats);
}

// k_group_emit: k_rows_emit's tiles and ranks over the representatives: group g = base[tile] + rank of a representative gets its
// first row, its count zeroed (COUNT) and its number stored where k_group_number finds it: dense[representative] = g.  Every
// workgroup returns at once when the groups do not fit: ET_ERR_CAP writes nothing.  No LDS.
template <bool COUNT>
__global__ __launch_bounds__(BB) void k_group_emit(const unsigned long long *__restrict__ masks, const uint64_t *__restrict__ base, uint32_t n_tiles,
                                                   uint32_t *__restrict__ first_rows, uint64_t cap_groups, uint32_t *__restrict__ count, uint32_t *__restrict__ dense) {
    if (base[n_tiles] > cap_groups) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const unsigned long long *m = masks + static_cast<uint64_t>(tile) * (MATCH_TILE / 64);
        const unsigned long long mine = m[wave];
        if (!((mine >> lane) & 1)) continue;
        uint32_t rank = __popcll(mine & ((1ull << lane) - 1ull));
        for (uint32_t w = 0; w < wave; ++w) rank += __popcll(m[w]);
        const uint32_t record = tile * MATCH_TILE + tid;
        const uint64_t g = base[tile] + rank;
        first_rows[g] = record;
        if (COUNT) count[g] = 0u;
        dense[record] = static_cast<uint32_t>(g);
    }
}

// k_group_number: a record per lane.  g = dense[rep_of[b]] is the record's group; a failed record's is GROUP_NONE.  group_of[b] = g
// (may be null), and -- COUNT -- the record is added into count[g], which k_group_emit zeroed.  The adds are combined in the
// wavefront first: per round the lowest lane still holding a record takes its group, the ballot of the lanes with the same group is
// that group's share of the wavefront, and the leader adds its popcount with ONE atomic.  The rounds go on while they pay: after
// GROUP_COMBINE_MISSES rounds that served their leader alone the rest adds singly, so a round that shares removes two lanes at least
// and there are 32 + GROUP_COMBINE_MISSES at the most.  A column in which one value holds most records sends one add per wavefront to
// that value's count, not 64; 64 records in 16 groups cost 16; a column of all different values pays GROUP_COMBINE_MISSES rounds -- a
// readlane, a compare and a ballot each, and the leader's add is one it owed anyway -- and adds as it would have.
// Integer adds commute: the counts are exact, whatever the order.  Returns at once when the groups do not fit.  No LDS.
template <bool COUNT>
__global__ __launch_bounds__(BB) void k_group_number(const uint32_t *__restrict__ rep_of, const uint32_t *__restrict__ dense, const uint64_t *__restrict__ base,
                                                     uint32_t n_tiles, uint32_t n, uint64_t cap_groups, uint32_t *__restrict__ group_of, uint32_t *__restrict__ count) {
    const uint64_t n_groups = base[n_tiles];
    if (n_groups > cap_groups) return;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t b = tile * MATCH_TILE + threadIdx.x;
        uint32_t g = GROUP_NONE;
        if (b < n) {
            const uint32_t rep = rep_of[b];
            if (rep < n) g = dense[rep];
            if (g >= n_groups) g = GROUP_NONE;  // (only behind a fault, which the host reports: a word k_group_emit never stored indexes nothing)
            if (group_of) group_of[b] = g;
        }
        if (COUNT) {
            unsigned long long left = __ballot(g != GROUP_NONE);
            for (uint32_t alone = 0; left && alone < GROUP_COMBINE_MISSES;) {
                const int leader = __ffsll(left) - 1;
                const uint32_t lead_g = __shfl(g, leader, 64);
                const unsigned long long same = __ballot(g == lead_g);  // (lead_g is a group: no failed lane is in it; a lane served before has another group)
                if (static_cast<int>(threadIdx.x & 63) == leader) atomicAdd(count + lead_g, static_cast<uint32_t>(__popcll(same)));
                left &= ~same;
                alone += (same & (same - 1)) == 0;  // (a round that served its leader alone cost what a single add costs, and bought nothing)
            }
            if ((left >> (threadIdx.x & 63)) & 1) atomicAdd(count + g, 1u);
        }
    }
}

// --------------------------------------------------------------------------------
// The take call: rows[] of a packed store as a new packed store.  Under one table a body is a self-contained byte string, so row k of
// the result is the bytes d_bodies[body_index[r], body_index[r + 1]) of its record r = rows[k] as they are, and its length is r's; no
// bit is interpreted and no table comes to the device.  Three launches in stream order (et_batch.h), the host waiting for the second
// alone; the copy is driven by the DESTINATION: every aligned 16-byte word of the output is assembled and stored by one lane, whatever
// the rows' sizes -- a 20-byte body does not scatter byte stores, a 40 KiB body is spread over ten wavefronts.
// --------------------------------------------------------------------------------
// k_take_plan: k_gather_plan with a TakeRow per row in place of a size word, and one more test behind the record's judgement: a body
// above TAKE_BODY_MAX is unsupported too.  A failed row is an empty record: {0, 0, 0}.
__global__ __launch_bounds__(BB) void k_take_plan(PackedStore store, const uint32_t *__restrict__ rows, uint32_t n_rows, TakeRow *__restrict__ plan,
                                                  uint8_t *__restrict__ d_status, unsigned long long *__restrict__ stats) {
    __shared__ unsigned long long s_failed[BB / 64], s_first[BB / 64];
    PackedTally tally;
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * BB + threadIdx.x; k < n_rows; k += static_cast<uint64_t>(gridDim.x) * BB) {
        const Judged rec = judge_record(store, rows[k]);
        const uint32_t status = !rec.status && rec.nb > TAKE_BODY_MAX ? PACKED_UNSUPPORTED : rec.status;
        uint4 row = make_uint4(0u, 0u, 0u, 0u);
        if (!status) row = make_uint4(static_cast<uint32_t>(rec.nb), static_cast<uint32_t>(rec.len), static_cast<uint32_t>(rec.b0), static_cast<uint32_t>(rec.b0 >> 32));
        reinterpret_cast<uint4 *>(plan)[k] = row;  // (TakeRow as it lies in memory)
        if (d_status) d_status[k] = static_cast<uint8_t>(status);
        tally.note(static_cast<uint32_t>(k), status);
    }
    tally_lanes(tally, s_failed, s_first, stats);
}

// k_take_scan: k_packed_scan over pairs -- ONE workgroup; per trip a tile of TAKE_SCAN_TILE rows; two exclusive scans in u64, the tiles
// before carried in two registers; both totals go to entry n.  The trip count is n / 4096, fixed by the host.  A lane scans 16
// consecutive rows, but global memory is read and written with consecutive lanes at consecutive rows (a lane at its own 16 rows reads
// 256 bytes and writes 2 x 128 bytes apart from its neighbour: one workgroup then spends its time on cache lines, 7 - 10 us per trip):
// the sizes pass through LDS, where a lane's 16 words lie 17 apart from its neighbour's (take_pad: different banks), are replaced
// there by their exclusive prefixes within the lane -- 16 bodies of at most TAKE_BODY_MAX fit 32 bits --, and a row's offset is its
// lane's base plus that prefix.  Thread 0 then reports {body bytes, rows that failed, the first of them << 8 | its status, text bytes}
// and the epoch; k_take_copy, enqueued behind, takes everything it needs from out_body_index and the plan: the host does not wait in
// between.  LDS 38 KiB.
__device__ __forceinline__ uint32_t take_pad(uint32_t k) { return k + (k >> 4); }

__global__ __launch_bounds__(BB) void k_take_scan(const TakeRow *__restrict__ plan, uint32_t n, uint64_t *__restrict__ out_body_index, uint64_t *__restrict__ out_text_index,
                                                  const unsigned long long *__restrict__ stats, unsigned long long *__restrict__ host_result,
                                                  unsigned long long *__restrict__ host_done, unsigned long long epoch) {
    constexpr uint32_t PER = TAKE_SCAN_TILE / BB;
    static_assert(PER == 16 && PER * TAKE_BODY_MAX <= 0xffffffffull, "take_pad; a lane's prefixes fit 32 bits");
    __shared__ uint32_t s_b[TAKE_SCAN_TILE + BB], s_t[TAKE_SCAN_TILE + BB];  // sizes, then prefixes within a lane, at take_pad(row)
    __shared__ uint64_t s_base_b[BB], s_base_t[BB];                          // where a lane's 16 rows begin
    __shared__ uint64_t s_body[4], s_text[4];
    const uint32_t tid = threadIdx.x;
    uint64_t carry_body = 0, carry_text = 0;
    for (uint32_t tile = 0; tile < n; tile += TAKE_SCAN_TILE) {
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) {
            const uint32_t k = j * BB + tid;
            uint2 x = make_uint2(0u, 0u);
            if (tile + k < n) x = *reinterpret_cast<const uint2 *>(plan + tile + k);  // {body_bytes, length}
            s_b[take_pad(k)] = x.x;
            s_t[take_pad(k)] = x.y;
        }
        __syncthreads();
        uint32_t my_body = 0, my_text = 0;
#pragma unroll
        for (uint32_t i = 0; i < PER; ++i) {
            const uint32_t p = take_pad(tid * PER + i);
            const uint32_t vb = s_b[p], vt = s_t[p];
            s_b[p] = my_body;
            s_t[p] = my_text;
            my_body += vb;
            my_text += vt;
        }
        uint64_t total_body, total_text;
        s_base_b[tid] = carry_body + block_exclusive_scan64(my_body, s_body, &total_body);
        s_base_t[tid] = carry_text + block_exclusive_scan64(my_text, s_text, &total_text);
        carry_body += total_body;
        carry_text += total_text;
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) {
            const uint32_t k = j * BB + tid;
            if (tile + k < n) {
                out_body_index[tile + k] = s_base_b[k >> 4] + s_b[take_pad(k)];
                out_text_index[tile + k] = s_base_t[k >> 4] + s_t[take_pad(k)];
            }
        }
        __syncthreads();  // (every LDS array: between two trips)
    }
    if (tid == 0) {
        out_body_index[n] = carry_body;
        out_text_index[n] = carry_text;
        host_result[PACKED_BYTES] = carry_body;
        host_result[PACKED_N_FAILED] = stats[PACKED_N_FAILED];
        host_result[PACKED_FIRST] = stats[PACKED_FIRST];
        host_result[TAKE_TEXT_BYTES] = carry_text;
        hand_over(host_done, epoch);
    }
}

// How many threads of the workgroup hold `p`.  Two barriers: s_cnt (4 words) is free again on return.
__device__ __forceinline__ uint32_t block_count(bool p, uint32_t *s_cnt) {
    const unsigned long long m = __ballot(p);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = static_cast<uint32_t>(__popcll(m));
    __syncthreads();
    const uint32_t c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    __syncthreads();
    return c;
}

// The first i in [lo, hi] with i == hi or index[i] > target, by the whole workgroup; index ascends (not strictly) and every entry in
// front of `lo` is at most `target`.  The first trip probes the 256 entries from lo on -- the answer of a tile that follows its
// neighbour lies there unless a long run of empty rows does --, every later trip 256 evenly spaced ones, which leaves at most a 256th of
// the range: 2^32 entries are done in six trips.  Every thread returns the same value.
__device__ __forceinline__ uint32_t wg_upper_bound(const uint64_t *__restrict__ index, uint32_t lo, uint32_t hi, uint64_t target, uint32_t *s_cnt) {
    uint64_t step = 1;
    for (int trip = 0; trip < 8 && lo < hi; ++trip) {
        const uint64_t p = lo + threadIdx.x * step;
        const uint32_t c = block_count(p < hi && index[p] <= target, s_cnt);  // (the probes ascend: the first c of them)
        if (c == 0) return lo;
        const uint64_t above = lo + c * step;  // probe c, when there was one, lies above the target
        lo = static_cast<uint32_t>(lo + (c - 1) * step + 1);
        if (c < BB && above < hi) hi = static_cast<uint32_t>(above);
        step = (static_cast<uint64_t>(hi - lo) + BB - 1) / BB;
    }
    return lo;
}

// `cnt` bytes (1 .. 8) at address a, all of them bytes of one body, zero-extended: from the aligned 8-byte words that hold them --
// one, or two -- shifted into place (body_word's rule: a word that holds no byte of the body is never loaded).
__device__ __forceinline__ uint64_t span_word(uintptr_t a, uint32_t cnt) {
    const uint64_t *q = reinterpret_cast<const uint64_t *>(a & ~static_cast<uintptr_t>(7));
    const uint32_t lead = static_cast<uint32_t>(a & 7);
    uint64_t v = q[0] >> (8 * lead);
    if (lead + cnt > 8) v |= q[1] << (64 - 8 * lead);  // (lead > 0 here; q[1] holds the last of the cnt bytes)
    if (cnt < 8) v &= (1ull << (8 * cnt)) - 1ull;
    return v;
}

// x's bytes to bytes d, d + 1, ... (d < 16) of the 16-byte word {v0, v1}.
__device__ __forceinline__ void put_bytes(uint64_t &v0, uint64_t &v1, uint64_t x, uint32_t d) {
    if (d < 8) {
        v0 |= x << (8 * d);
        if (d) v1 |= x >> (64 - 8 * d);
    } else {
        v1 |= x << (8 * (d - 8));
    }
}

// The slice's piece: `c` bytes (1 .. 8) of a new body whose bits are the source's from bit address bit0 on (a byte's address * 8 + the
// bit, from the top), of which `left` >= 1 belong to the slice.  Each byte is a funnel shift of two source bytes; only the source
// bytes that hold one of the min(left, 8 c) bits are loaded (span_word: at most 9, all of them the record's), and where the slice
// ends inside the piece's last byte the bits behind it are zero: the encoder's pad, whatever the source holds there.
__device__ __forceinline__ uint64_t bit_span(uint64_t bit0, uint32_t c, uint32_t left) {
    constexpr uint64_t ONES = 0x0101010101010101ull;
    const uint32_t sh = static_cast<uint32_t>(bit0 & 7), v = left < 8 * c ? left : 8 * c, n = (sh + v + 7) >> 3;
    const uintptr_t a = static_cast<uintptr_t>(bit0 >> 3);
    const uint64_t lo = span_word(a, n < 8 ? n : 8u), hi = n > 8 ? span_word(a + 8, 1) : 0ull;
    const uint64_t next = lo >> 8 | hi << 56;  // byte j: source byte j + 1
    uint64_t x = ((lo & (ONES * (0xffu >> sh))) << sh) | ((next >> (8 - sh)) & (ONES * (0xffu >> (8 - sh))));
    if (c < 8) x &= (1ull << (8 * c)) - 1ull;
    if (v < 8 * c) x &= ~(((1ull << (8 * c - v)) - 1ull) << (8 * (c - 1)));  // (the row ends in this piece: 8 c - v pad bits, 1 .. 7)
    return x;
}

// k_take_copy: the output's bytes [0, total) lie at d_out, any alignment; tile t is what of them lies in the t-th TAKE_TILE_BYTES
// block counted from d_out's address rounded down, so every word below is an aligned 16 bytes of MEMORY.  A workgroup takes a run of
// consecutive tiles.  Per tile it finds, together, the rows that own the tile's first and last byte (wg_upper_bound: a run of empty rows
// shares its offset with the row behind it, and the LAST row at an offset is the one that owns the byte) and keeps that stretch of
// out_body_index in LDS when it fits (TAKE_STAGE_ROWS entries: 8 KiB), else reads it in place.  A lane then owns words tid and
// tid + 256 of the tile.  For a word it finds the row that owns its first byte (binary search over the tile's stretch: at most 31
// steps), and walks the rows that own the rest -- a step to the next row, or where empty rows follow a search again --, at most 16
// trips: each takes a byte of the word at least.  A row's piece comes from its TakeRow (one 16-byte load) and one to three aligned
// 8-byte source words.  A full word leaves as ONE 16-byte store; the first and the last word of the whole output, where d_out or its
// end is not aligned, leave as byte stores of their own bytes.  Nothing is written when total > cap, no workgroup waits for another,
// and a row that owns a byte was judged by k_take_plan, so its TakeRow is believed.  LDS 8 KiB + 16 bytes.
// BITS (the slice call): a row's source is a run of BITS -- TakeRow::src as k_slice_plan leaves it -- and a piece is bit_span's; the
// tiles, the rows and the stores are the same, and d_bodies is not looked at.
// (k_concat_copy below is a second copy of this frame with another piece: a fix to the frame belongs in both.)
template <bool BITS>
__global__ __launch_bounds__(BB) void k_take_copy(const uint8_t *__restrict__ d_bodies, const TakeRow *__restrict__ plan, const uint64_t *__restrict__ out_index,
                                                  uint32_t n_rows, uint8_t *__restrict__ d_out, uint64_t cap) {
    __shared__ uint64_t s_idx[TAKE_STAGE_ROWS];
    __shared__ uint32_t s_cnt[4];
    const uint32_t tid = threadIdx.x;
    const uint64_t total = out_index[n_rows];
    if (total > cap || total == 0) return;
    const uintptr_t out = reinterpret_cast<uintptr_t>(d_out), bodies = reinterpret_cast<uintptr_t>(d_bodies);
    const uint64_t skew = out & (TAKE_TILE_BYTES - 1);  // bytes of tile 0 in front of d_out
    const uint64_t n_tiles = (skew + total + TAKE_TILE_BYTES - 1) / TAKE_TILE_BYTES;
    const uint64_t per = (n_tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t t_begin = blockIdx.x * per, t_end = t_begin + per < n_tiles ? t_begin + per : n_tiles;
    uint32_t hint = 0;  // every entry of out_index in front of it is at most the tile's first offset
    for (uint64_t t = t_begin; t < t_end; ++t) {
        // the tile's bytes as offsets into the output: [o0, o1), o0 < o1 <= total
        const uint64_t o0 = t ? t * TAKE_TILE_BYTES - skew : 0, o1_full = (t + 1) * TAKE_TILE_BYTES - skew, o1 = o1_full < total ? o1_full : total;
        // out_index[row_lo] <= o0 < out_index[row_lo + 1], out_index[row_end - 1] < o1 <= out_index[row_end]: rows [row_lo, row_end) own the tile
        const uint32_t row_lo = wg_upper_bound(out_index, hint, n_rows + 1, o0, s_cnt) - 1;  // (out_index[0] = 0 <= o0: at least 1)
        const uint32_t row_end = wg_upper_bound(out_index, row_lo + 1, n_rows + 1, o1 - 1, s_cnt);  // (out_index[n_rows] = total > o1 - 1: at most n_rows)
        hint = row_end;
        const uint32_t entries = row_end - row_lo + 1;
        const bool staged = entries <= TAKE_STAGE_ROWS;  // (the same for every thread)
        if (staged)
            for (uint32_t i = tid; i < entries; i += BB) s_idx[i] = out_index[row_lo + i];
        __syncthreads();
        auto idx = [&](uint32_t r) -> uint64_t { return staged ? s_idx[r - row_lo] : out_index[r]; };  // r in [row_lo, row_end]
        const uintptr_t tile_addr = (out - skew) + t * TAKE_TILE_BYTES;
#pragma unroll
        for (uint32_t j = 0; j < TAKE_TILE_BYTES / (16 * BB); ++j) {
            const uintptr_t aw = tile_addr + (j * BB + tid) * 16;
            const int64_t rel = static_cast<int64_t>(aw) - static_cast<int64_t>(out);  // the word's first byte as an offset: negative in front of d_out
            if (rel + 16 <= 0 || rel >= static_cast<int64_t>(total)) continue;
            const uint64_t w0 = rel < 0 ? 0 : static_cast<uint64_t>(rel), w1 = static_cast<uint64_t>(rel + 16) < total ? static_cast<uint64_t>(rel + 16) : total;
            // the row that owns byte w0: the last r in [row_lo, row_end) with out_index[r] <= w0
            uint32_t k = row_lo, hi = row_end;
            while (hi - k > 1) {
                const uint32_t mid = k + (hi - k) / 2;
                if (idx(mid) <= w0) k = mid;
                else hi = mid;
            }
            uint64_t v0 = 0, v1 = 0, pos = w0;
            for (int trip = 0; trip < 16; ++trip) {  // row k owns byte pos: out_index[k] <= pos < out_index[k + 1]
                const uint64_t s = idx(k), e = idx(k + 1), piece_end = e < w1 ? e : w1;
                const uint32_t c = static_cast<uint32_t>(piece_end - pos);  // 1 .. 16
                const uint32_t d = static_cast<uint32_t>(static_cast<int64_t>(pos) - rel);
                if constexpr (BITS) {
                    const uint64_t src = plan[k].src, bit0 = (src & ((1ull << SLICE_PAD_SHIFT) - 1ull)) + 8 * (pos - s);
                    const uint32_t left = static_cast<uint32_t>(e - pos) * 8 - static_cast<uint32_t>(src >> SLICE_PAD_SHIFT);  // the slice's bits from bit0 on
                    put_bytes(v0, v1, bit_span(bit0, c < 8 ? c : 8u, left), d);
                    if (c > 8) put_bytes(v0, v1, bit_span(bit0 + 64, c - 8, left - 64), d + 8);  // (9 bytes are left at least: left >= 65)
                } else {
                    const uintptr_t a = bodies + plan[k].src + (pos - s);
                    put_bytes(v0, v1, span_word(a, c < 8 ? c : 8u), d);
                    if (c > 8) put_bytes(v0, v1, span_word(a + 8, c - 8), d + 8);
                }
                pos = piece_end;
                if (pos >= w1) break;
                ++k;  // (a row behind owns byte pos < o1: k < row_end)
                if (idx(k + 1) <= pos) {  // empty rows follow: the last r in [k, row_end) with out_index[r] <= pos
                    hi = row_end;
                    while (hi - k > 1) {
                        const uint32_t mid = k + (hi - k) / 2;
                        if (idx(mid) <= pos) k = mid;
                        else hi = mid;
                    }
                }
            }
            if (w1 - w0 == 16) {
                *reinterpret_cast<uint4 *>(aw) = make_uint4(static_cast<uint32_t>(v0), static_cast<uint32_t>(v0 >> 32), static_cast<uint32_t>(v1), static_cast<uint32_t>(v1 >> 32));
            } else {  // the output's first or last word: its own bytes alone
                for (uint32_t i = static_cast<uint32_t>(static_cast<int64_t>(w0) - rel); i < static_cast<uint32_t>(static_cast<int64_t>(w1) - rel); ++i)
                    reinterpret_cast<uint8_t *>(aw)[i] = static_cast<uint8_t>((i < 8 ? v0 >> (8 * i) : v1 >> (8 * (i - 8))) & 0xffu);
            }
        }
        __syncthreads();  // (s_idx: between two tiles)
    }
}

// --------------------------------------------------------------------------------
// The derived stores: the slice, the field, the concat and the recode each make a NEW packed store out of rows[] of an old one on the
// compressed bytes, and share the frame that is stated here once.  The number call, behind them, reads a word per row where they make a store, in the same frame.
//   plan_rows   a row per lane: the row is judged (judge_row), what the ask can reach of its body is taken (reach_body), and a body
//               up to the family's threshold (lane_walks) is walked by that lane from global memory (lane_walk); a longer one goes
//               onto long_list -- one atomic per wavefront that has any -- and is the empty record for now
//   long_rows   a listed row per workgroup, the list strided: the body settled block by block (settle_block), what the lanes found
//               reduced (reduce_min_min_max) or scanned, a lane that reaches the record's length cut there (cut_at_length); thread 0
//               stores the row's TakeRow, or fails the row (fail_row_late): the plan kernel left the empty record there and held the
//               row for OK, and k_take_scan runs behind both kernels
// A family below is its middle: what it asks of a row, and what its walks note.
// Every loop is bounded as the search's are: a lane's walk by the symbols its caller allows (a trip per symbol, at most the record's
// length), the workgroup's by the blocks of what the reach leaves of the body, its fixed point by 256 trips and a lane's walk inside
// it by its 256 bits.  No workgroup waits for another: a long kernel stores what belongs to its own row and nothing else.
// --------------------------------------------------------------------------------
// Row k's record as the take judges it: judge_record, and a body above TAKE_BODY_MAX is unsupported too.  rows null: row k is record
// k.  A store without bodies (the concat's absent side) contributes an OK record of nothing and is not looked at.
__device__ __forceinline__ Judged judge_row(const PackedStore &store, const uint32_t *rows, uint32_t k) {
    if (!store.bodies) return Judged{PACKED_OK, 0, 0, 0};
    Judged rec = judge_record(store, rows ? rows[k] : k);
    if (!rec.status && rec.nb > TAKE_BODY_MAX) rec.status = PACKED_UNSUPPORTED;
    return rec;
}

// A judged record whose body is read: one kept raw, or empty, has the empty stored text.
__device__ __forceinline__ bool stored_text(const Judged &rec) { return !rec.status && rec.nb && rec.len; }

// What the walks look at of such a record when nothing behind symbol `reach` is asked for (clip_body: 4 bytes per symbol in front
// of it), and whether its lane walks that alone.
__device__ __forceinline__ BodyBits reach_body(const PackedStore &store, const Judged &rec, uint64_t reach) {
    return body_bits_of(static_cast<const uint8_t *>(store.bodies), rec.b0, static_cast<uint32_t>(clip_body(rec.nb, reach)));
}

__device__ __forceinline__ bool lane_walks(const BodyBits &g, uint32_t lane_bytes) { return g.end_bit - g.first_bit <= lane_bytes * 8; }

__device__ __forceinline__ void store_row(TakeRow *__restrict__ plan, uint32_t k, uint4 row) { reinterpret_cast<uint4 *>(plan)[k] = row; }  // (TakeRow as it lies in memory)

// The plan frame: row(k) does a row's work -- its TakeRow included -- and returns its status and whether it goes onto long_list; the
// frame stores the status byte, tallies, and appends the wavefront's long rows with one atomic.  The caller has its tables in LDS
// and a barrier behind them.  LDS: 8 words.
struct RowPlan {
    uint32_t status;
    bool is_long;
};

template <class Row>
__device__ __forceinline__ void plan_rows(uint32_t n_rows, uint32_t *__restrict__ long_list, uint8_t *__restrict__ d_status, unsigned long long *__restrict__ stats, Row &&row) {
    __shared__ unsigned long long s_failed[BB / 64], s_first[BB / 64];
    const uint32_t lane = threadIdx.x & 63;
    PackedTally tally;
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * BB; base < n_rows; base += static_cast<uint64_t>(gridDim.x) * BB) {
        const uint32_t k = static_cast<uint32_t>(base) + threadIdx.x;  // (n_rows <= 0x7fffffff: no wrap)
        bool is_long = false;
        if (k < n_rows) {
            const RowPlan p = row(k);
            is_long = p.is_long;
            if (d_status) d_status[k] = static_cast<uint8_t>(p.status);
            tally.note(k, p.status);
        }
        const unsigned long long longs = __ballot(is_long);
        if (longs) {  // (the same for the whole wavefront)
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(stats + SLICE_N_LONG, static_cast<unsigned long long>(__popcll(longs)));
            at = __shfl(at, 0, 64);
            if (is_long) long_list[at + __popcll(longs & ((1ull << lane) - 1ull))] = k;
        }
    }
    tally_lanes(tally, s_failed, s_first, stats);
}

// The long-row frame (k_search_long's shape): a workgroup beyond the list returns before it sets anything up; set_up() then loads
// the tables once per workgroup -- false: nothing to do in this call, the same for every thread --; row(k) sees the listed rows,
// strided.  row re-judges its record and skips what the plan kernel never lists; everything in it is the same for every lane.
template <class SetUp, class Row>
__device__ __forceinline__ void long_rows(uint32_t n_rows, const uint32_t *__restrict__ long_list, const unsigned long long *__restrict__ stats, SetUp &&set_up, Row &&row) {
    const uint32_t n_long = static_cast<uint32_t>(stats[SLICE_N_LONG]);
    if (blockIdx.x >= n_long || !set_up()) return;
    for (uint32_t i = blockIdx.x; i < n_long; i += gridDim.x) {
        const uint32_t k = long_list[i];
        if (k < n_rows) row(k);  // (the plan kernel lists rows)
    }
}

// A row that fails behind its plan kernel, which held it for OK: its status byte and two atomics, by thread 0.
__device__ __forceinline__ void fail_row_late(uint32_t k, uint32_t status, uint8_t *__restrict__ d_status, unsigned long long *__restrict__ stats) {
    if (d_status) d_status[k] = static_cast<uint8_t>(status);
    PackedTally tally;
    tally.note(k, status);
    tally.add_to(stats);
}

// One lane, one body of a few words, from global memory (search_lane's shape): a trip per symbol of the stored text, `most` at most.
// 64 bits of body are kept in registers and move on a word at a time.  visit(idx, pos, meta) sees symbol idx -- its bit, its length
// << 8 | symbol -- in front of the step over it and ends the walk there by returning false; the stored text ends where the bits run
// out inside a codeword.  Returns the symbol and the bit at which the walk ended: those of the codeword it did not step over.
struct LaneEnd {
    uint32_t idx, pos;
};

template <class Visit>
__device__ __forceinline__ LaneEnd lane_walk(const CodeTables &t, uint32_t n_codes, const BodyBits &g, uint32_t most, Visit &&visit) {
    uint32_t pos = g.first_bit, k = 0, idx = 0;
    uint64_t two = (body_word_be(g, 0) << 32) | body_word_be(g, 1);
    for (; idx < most; ++idx) {
        if ((pos >> 5) != k) {  // (a codeword has at most 32 bits: one word on)
            k = pos >> 5;
            two = (two << 32) | body_word_be(g, k + 1);
        }
        const uint32_t meta = code_at(t, n_codes, static_cast<uint32_t>((two << (pos & 31)) >> 32));
        if (pos + (meta >> 8) > g.end_bit) break;  // the bits ran out inside this codeword: the stored text ends here
        if (!visit(idx, pos, meta)) break;
        pos += meta >> 8;
    }
    return LaneEnd{idx, pos};
}

// Three words of symbol << 32 | bit, one per lane, reduced over the workgroup -- the lowest `a`, the lowest `b`, the highest `c` --
// by shuffles and through s_red (12 words, free again at the next block's first barrier).  Every lane has the three on return.
__device__ __forceinline__ void reduce_min_min_max(unsigned long long &a, unsigned long long &b, unsigned long long &c, unsigned long long *s_red) {
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long oa = __shfl_xor(a, d, 64), ob = __shfl_xor(b, d, 64), oc = __shfl_xor(c, d, 64);
        if (oa < a) a = oa;
        if (ob < b) b = ob;
        if (oc > c) c = oc;
    }
    if ((tid & 63) == 0) {
        s_red[tid >> 6] = a;
        s_red[4 + (tid >> 6)] = b;
        s_red[8 + (tid >> 6)] = c;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < BB / 64; ++w) {
        if (s_red[w] < a) a = s_red[w];
        if (s_red[4 + w] < b) b = s_red[4 + w];
        if (s_red[8 + w] > c) c = s_red[8 + w];
    }
}

// The cut at the length, behind settle_block: what this lane holds of the STORED TEXT.  THE rule of what counts: codeword number i
// of a body is a symbol of the stored text when it ends inside the body AND i < length.  The settling visitor does not know its
// lane's symbol numbers; once the scan has given them (`lo`: the number of the lane's first codeword), the lanes behind `len` hold
// nothing and `visit` is `fresh` again; the one lane whose codewords reach `len` -- a lane of the text's last block -- walks again
// with a fresh visitor up to it, so nothing at or behind `len` is ever seen.  Returns the lane's symbols; `visit` holds what they give.
template <class Visit>
__device__ __forceinline__ uint32_t cut_at_length(const BatchDecLds &s, uint32_t n_codes, const Settled &b, uint32_t lo, uint32_t len, Visit &visit, const Visit &fresh) {
    if (lo + b.count <= len) return b.count;  // (lo + count <= 4 * len + 16: no wrap)
    visit = fresh;
    if (lo >= len) return 0u;
    const uint32_t held = len - lo;
    uint32_t again;
    (void)walk(s, n_codes, b.used, b.room, &again, [&](uint32_t cnt, uint32_t pos, uint32_t win, uint32_t meta) { return cnt < held && visit(cnt, pos, win, meta); });
    return held;
}

// --------------------------------------------------------------------------------
// The slice call: symbols [first, first + count) of rows[]' stored texts, cut in front of the first `stop` byte among them, as a new
// packed store.  Under one complete prefix-free table symbols [i, j) of a record are the bits from the boundary of codeword i to the
// boundary of codeword j, so a slice is found by a walk over the boundaries -- nothing compared but the symbol the step yields
// anyway, nothing written -- and written by the take's scan and copy, the copy reading a run of bits where the take reads a run of
// bytes.  Four launches in stream order (et_batch.h), the host waiting for the scan alone.  The reach of a slice is its end: no
// block behind it is visited.
// --------------------------------------------------------------------------------
// What row k asks of a stored text of at most `len` symbols: [first, end), end <= len; nothing when end <= first.  (first + count does
// not wrap: 64 bits; ET_SLICE_TO_END lies beyond every length.)
struct SliceAsk {
    uint32_t first, end;
};

__device__ __forceinline__ SliceAsk slice_ask(const SliceJob &job, uint32_t k, uint32_t len) {
    const uint32_t first = job.d_first ? job.d_first[k] : job.first, count = job.d_count ? job.d_count[k] : job.count;
    const uint64_t end = static_cast<uint64_t>(first) + count;
    return SliceAsk{first, end < len ? static_cast<uint32_t>(end) : len};
}

// What a walk found: the bit (from the body's aligned base) at which the slice's first codeword begins, the bit behind its last, its symbols.
struct Sliced {
    uint32_t begin, end, n;
};

// The TakeRow of a slice as it lies in memory: the new body's bytes, its symbols, the address of its first bit with the pad above it.
__device__ __forceinline__ uint4 slice_row(const BodyBits &g, const Sliced &sl) {
    if (!sl.n) return make_uint4(0u, 0u, 0u, 0u);  // (a codeword has a bit at least: symbols mean bits)
    const uint32_t bits = sl.end - sl.begin, bytes = (bits + 7) >> 3;
    const uint64_t src = (static_cast<uint64_t>(reinterpret_cast<uintptr_t>(g.words)) * 8 + sl.begin) | static_cast<uint64_t>(bytes * 8 - bits) << SLICE_PAD_SHIFT;
    return make_uint4(bytes, sl.n, static_cast<uint32_t>(src), static_cast<uint32_t>(src >> 32));
}

// lane_walk in front of the slice's end: the slice ends where the stored text does, at ask.end, or in front of the first `stop` at
// or behind ask.first.
__device__ __forceinline__ Sliced slice_lane(const CodeTables &t, uint32_t n_codes, const BodyBits &g, const SliceAsk &ask, uint32_t stop) {
    uint32_t begin = 0;
    const LaneEnd e = lane_walk(t, n_codes, g, ask.end, [&](uint32_t idx, uint32_t pos, uint32_t meta) {
        if (idx == ask.first) begin = pos;
        return idx < ask.first || (meta & 0xffu) != stop;
    });
    return Sliced{begin, e.pos, e.idx > ask.first ? e.idx - ask.first : 0u};
}

// k_slice_plan: plan_rows with the sorted codes and the first-level table in LDS once per workgroup.  A row that asks for nothing,
// or of a record without bytes or symbols, is the empty record and is not read; a body of which the slice's end can reach up to
// SLICE_LANE_BYTES is walked by its lane (slice_lane).  LDS 6 KiB + 8 words.
__global__ __launch_bounds__(BB) void k_slice_plan(PackedStore store, const uint2 *__restrict__ codes, uint32_t n_codes, SliceJob job, TakeRow *__restrict__ plan,
                                                   uint32_t *__restrict__ long_list, uint8_t *__restrict__ d_status, unsigned long long *__restrict__ stats) {
    __shared__ CodeTables t;
    load_tables(t, codes, n_codes);
    __syncthreads();
    plan_rows(job.n_rows, long_list, d_status, stats, [&](uint32_t k) {
        const Judged rec = judge_row(store, job.rows, k);
        RowPlan p{rec.status, false};
        uint4 row = make_uint4(0u, 0u, 0u, 0u);
        if (stored_text(rec)) {
            const SliceAsk ask = slice_ask(job, k, static_cast<uint32_t>(rec.len));
            if (ask.end > ask.first) {
                const BodyBits g = reach_body(store, rec, ask.end);
                if (lane_walks(g, SLICE_LANE_BYTES)) row = slice_row(g, slice_lane(t, n_codes, g, ask, job.stop));
                else p.is_long = true;
            }
        }
        store_row(plan, k, row);
        return p;
    });
}

// One row's body by the whole workgroup under the tables in `s`: search_stream's blocks with a counting walk to settle them.  Once the
// scan has numbered a block's codewords, the lanes whose codewords meet [ask.first, ask.end) walk again and note, as symbol << 32 |
// bit: where symbol ask.first begins, where the first `stop` among their symbols begins (the walk ends there), and where the last of
// their symbols in the range ends.  The three are reduced over the workgroup (reduce_min_min_max): the slice begins at the one
// begin, and ends at the lowest stop or else behind the highest symbol of the range that the stored text holds.  The blocks end with
// the first that has a stop, or once ask.end codewords lie behind: none behind the slice's end is visited.
__device__ __forceinline__ Sliced slice_stream(BatchDecLds &s, uint32_t n_codes, const BodyBits &g, const SliceAsk &ask, uint32_t stop, unsigned long long *s_red) {
    constexpr unsigned long long NONE = ~0ull;
    const uint32_t tid = threadIdx.x;
    const uint32_t n_blocks = (g.n_words + DEC_WORDS - 1) / DEC_WORDS;
    uint32_t start = g.first_bit, done = 0;  // the block's first codeword; codewords so far
    unsigned long long begin = NONE, end = 0;
    for (uint32_t blk = 0; blk < n_blocks && done < ask.end; ++blk) {
        const uint32_t at = blk * DEC_WORDS * 32 + tid * 256;
        JustCount counting;
        const Settled b = settle_block(s, n_codes, g, blk, start, counting);
        const uint32_t lo = done + b.first;  // the number of the lane's first codeword
        unsigned long long my_begin = NONE, my_stop = NONE, my_last = 0;
        if (b.count && lo < ask.end && lo + b.count > ask.first) {
            uint32_t again;
            (void)walk(s, n_codes, b.used, b.room, &again, [&](uint32_t cnt, uint32_t pos, uint32_t, uint32_t meta) {
                const uint32_t sym = lo + cnt;
                if (sym >= ask.end) return false;
                if (sym < ask.first) return true;
                const unsigned long long here = static_cast<unsigned long long>(sym) << 32 | (at + pos);
                if (sym == ask.first) my_begin = here;
                if ((meta & 0xffu) == stop) {
                    my_stop = here;
                    return false;
                }
                my_last = static_cast<unsigned long long>(sym + 1) << 32 | (at + pos + (meta >> 8));
                return true;
            });
        }
        reduce_min_min_max(my_begin, my_stop, my_last, s_red);
        if (my_begin != NONE) begin = my_begin;  // (the same for every lane, like all below)
        if (my_last > end) end = my_last;
        if (my_stop != NONE) {  // the lowest stop: nothing at or behind it belongs to the slice
            end = my_stop;
            break;
        }
        start = b.start;
        done += b.total;
    }
    if (begin == NONE) return Sliced{0u, 0u, 0u};  // the stored text ends in front of ask.first
    return Sliced{static_cast<uint32_t>(begin), static_cast<uint32_t>(end), static_cast<uint32_t>(end >> 32) - ask.first};
}

// k_slice_long: long_rows with slice_stream.  LDS as k_batch_decode, and the reduction's 12 words.
__global__ __launch_bounds__(BB) void k_slice_long(PackedStore store, const uint2 *__restrict__ codes, uint32_t n_codes, SliceJob job, TakeRow *__restrict__ plan,
                                                   const uint32_t *__restrict__ long_list, const unsigned long long *__restrict__ stats) {
    __shared__ BatchDecLds s;
    __shared__ unsigned long long s_red[3 * (BB / 64)];
    long_rows(job.n_rows, long_list, stats, [&] { return load_tables(s.t, codes, n_codes), true; }, [&](uint32_t k) {
        const Judged rec = judge_row(store, job.rows, k);
        if (!stored_text(rec)) return;
        const SliceAsk ask = slice_ask(job, k, static_cast<uint32_t>(rec.len));
        if (ask.end <= ask.first) return;
        const BodyBits g = reach_body(store, rec, ask.end);
        const Sliced sl = slice_stream(s, n_codes, g, ask, job.stop, s_red);
        if (threadIdx.x == 0) store_row(plan, k, slice_row(g, sl));
    });
}

// --------------------------------------------------------------------------------
// The field call: fields [field, field + n_fields) of rows[]' stored texts -- text_b.split(delim) --, the delimiters between them
// kept, as a new packed store.  A delimiter is a codeword of the stored text that decodes to `delim`; the walks count them.  Numbered
// from 1, the field begins behind delimiter `a` = field (a = 0: at the text's first symbol) and ends in front of delimiter `b` =
// field + n_fields, or where the stored text ends when it has fewer; a text with fewer than `a` has no such field.  What lies between
// is a run of bits between two codeword boundaries: a slice, written by the take's scan and the bit-reading copy.  The reach of a
// field is the record's whole length: nothing bounds where field k lies.
// --------------------------------------------------------------------------------
struct FieldAsk {
    uint32_t a, b;  // a <= b
};

__device__ __forceinline__ FieldAsk field_ask(const FieldJob &job, uint32_t k) {
    const uint32_t field = job.d_field ? job.d_field[k] : job.field, n = job.d_n_fields ? job.d_n_fields[k] : job.n_fields;
    const uint64_t b = static_cast<uint64_t>(field) + n;  // (64 bits: no wrap; a text has fewer than 2^32 - 1 delimiters)
    return FieldAsk{field, b < 0xffffffffull ? static_cast<uint32_t>(b) : 0xffffffffu};
}

// What a walk found: the slice's three, and the symbol at which the field begins -- FIELD_ABSENT: no such field (n is 0 then).
struct Fielded {
    uint32_t begin, end, n, pos;
};

__device__ __forceinline__ uint4 field_row(const BodyBits &g, const Fielded &f) { return slice_row(g, Sliced{f.begin, f.end, f.n}); }

// lane_walk with a running delimiter count, ended at the closing delimiter -- or behind the opening one when no field was asked for
// (a == b).  (a == b == 0 asks for nothing of the body: the caller does not come here.)
__device__ __forceinline__ Fielded field_lane(const CodeTables &t, uint32_t n_codes, const BodyBits &g, uint32_t len, const FieldAsk &ask, uint32_t delim) {
    uint32_t seen = 0;
    bool closed = false;
    Fielded f{g.first_bit, g.first_bit, 0u, ask.a ? FIELD_ABSENT : 0u};
    const LaneEnd e = lane_walk(t, n_codes, g, len, [&](uint32_t idx, uint32_t pos, uint32_t meta) {
        if ((meta & 0xffu) != delim) return true;
        ++seen;
        if (seen == ask.a) {  // the field begins behind this one
            f.begin = f.end = pos + (meta >> 8);
            f.pos = idx + 1;
            closed = ask.b == ask.a;  // ... and no field was asked for: the empty record, present
        } else if (seen == ask.b) {  // the closing one
            f.end = pos;
            f.n = idx - f.pos;
            closed = true;
        }
        return !closed;
    });
    if (closed || f.pos == FIELD_ABSENT) return f;
    f.end = e.pos;  // the stored text's end
    f.n = e.idx - f.pos;
    return f;
}

// k_field_plan: plan_rows.  A record without bytes or symbols has the empty stored text: one empty field 0.  A row that asks for no
// field of field 0 on is the empty record and is not read.  A body that the length can reach up to FIELD_LANE_BYTES is walked by its
// lane (field_lane).  d_pos[k] = the symbol at which the field begins, FIELD_ABSENT without one and for a failed row; k_field_long
// stores a listed row's.  LDS 6 KiB + 8 words.
__global__ __launch_bounds__(BB) void k_field_plan(PackedStore store, const uint2 *__restrict__ codes, uint32_t n_codes, FieldJob job, TakeRow *__restrict__ plan,
                                                   uint32_t *__restrict__ long_list, uint8_t *__restrict__ d_status, unsigned long long *__restrict__ stats) {
    __shared__ CodeTables t;
    load_tables(t, codes, n_codes);
    __syncthreads();
    plan_rows(job.n_rows, long_list, d_status, stats, [&](uint32_t k) {
        const Judged rec = judge_row(store, job.rows, k);
        RowPlan p{rec.status, false};
        uint4 row = make_uint4(0u, 0u, 0u, 0u);
        uint32_t pos = FIELD_ABSENT;
        if (!rec.status) {
            const FieldAsk ask = field_ask(job, k);
            if (!stored_text(rec) || !ask.b) {
                if (!ask.a) pos = 0;
            } else {
                const uint32_t len = static_cast<uint32_t>(rec.len);
                const BodyBits g = reach_body(store, rec, len);
                if (lane_walks(g, FIELD_LANE_BYTES)) {
                    const Fielded f = field_lane(t, n_codes, g, len, ask, job.delim);
                    row = field_row(g, f);
                    pos = f.pos;
                } else {
                    p.is_long = true;
                }
            }
        }
        store_row(plan, k, row);
        if (job.d_pos) job.d_pos[k] = pos;
        return p;
    });
}

// The visitor of the settling walks of the field call: the walk's delimiters, and the bit of the lane's 256 behind its last codeword.
struct CountDelims {
    uint32_t delim, n, last;
    __device__ __forceinline__ bool operator()(uint32_t, uint32_t pos, uint32_t, uint32_t meta) {
        n += (meta & 0xffu) == delim;
        last = pos + (meta >> 8);
        return true;
    }
};

// One row's body by the whole workgroup under the tables in `s`: slice_stream's blocks, settled by a walk that counts its delimiters
// and cut at the length (cut_at_length), so no codeword at or behind `len` is ever a delimiter.  A second scan (s_scan, 4 words, free
// again at the next block's first barrier) numbers the delimiters across the lanes, `seen` carries them across the blocks beside
// `done`.  The lanes that hold delimiter a or b walk again and note, as symbol << 32 | bit, where the field begins and where the
// closing delimiter does; every lane notes where its last symbol ends.  The three are reduced over the workgroup
// (reduce_min_min_max).  The begin found in one block is kept in a register until the end is found, blocks later.  The blocks end
// with the one that holds the closing delimiter, or once `len` codewords lie behind: nothing behind is visited.
__device__ __forceinline__ Fielded field_stream(BatchDecLds &s, uint32_t n_codes, const BodyBits &g, uint32_t len, const FieldAsk &ask, uint32_t delim,
                                                unsigned long long *s_red, uint32_t *s_scan) {
    constexpr unsigned long long NONE = ~0ull;
    const uint32_t tid = threadIdx.x;
    const uint32_t n_blocks = (g.n_words + DEC_WORDS - 1) / DEC_WORDS;
    uint32_t start = g.first_bit, done = 0, seen = 0;  // the block's first codeword; codewords and delimiters so far
    unsigned long long begin = ask.a ? NONE : g.first_bit, end = 0;
    const CountDelims fresh{delim, 0u, 0u};
    for (uint32_t blk = 0; blk < n_blocks && done < len; ++blk) {
        const uint32_t at = blk * DEC_WORDS * 32 + tid * 256;
        CountDelims counting = fresh;
        const Settled b = settle_block(s, n_codes, g, blk, start, counting);
        const uint32_t lo = done + b.first;  // the number of the lane's first codeword
        const uint32_t held = cut_at_length(s, n_codes, b, lo, len, counting, fresh), mine = counting.n;  // the lane's symbols of the stored text, the delimiters among them
        uint32_t block_delims;
        const uint32_t before = seen + block_exclusive_scan(mine, s_scan, &block_delims);  // delimiters in front of the lane's first symbol
        unsigned long long my_begin = NONE, my_close = NONE, my_last = held ? static_cast<unsigned long long>(lo + held) << 32 | (at + counting.last) : 0ull;
        const bool has_a = ask.a > before && ask.a - before <= mine, has_b = ask.b > before && ask.b - before <= mine;
        if (has_a || has_b) {
            uint32_t again, d = before;
            (void)walk(s, n_codes, b.used, b.room, &again, [&](uint32_t cnt, uint32_t pos, uint32_t, uint32_t meta) {
                if (cnt >= held) return false;
                if ((meta & 0xffu) != delim) return true;
                ++d;
                if (d == ask.a) my_begin = static_cast<unsigned long long>(lo + cnt + 1) << 32 | (at + pos + (meta >> 8));
                if (d == ask.b) {
                    my_close = static_cast<unsigned long long>(lo + cnt) << 32 | (at + pos);
                    return false;
                }
                return true;
            });
        }
        reduce_min_min_max(my_begin, my_close, my_last, s_red);
        if (my_begin != NONE) begin = my_begin;  // (the same for every lane, like all below)
        if (my_last > end) end = my_last;
        if (my_close != NONE) {  // nothing at or behind the closing delimiter belongs to the field
            end = my_close;
            break;
        }
        start = b.start;
        done += b.total;
        seen += block_delims;
    }
    if (begin == NONE) return Fielded{0u, 0u, 0u, FIELD_ABSENT};  // the stored text has fewer than `a` delimiters
    const uint32_t pos = static_cast<uint32_t>(begin >> 32);
    if (ask.a == ask.b || end < begin) return Fielded{static_cast<uint32_t>(begin), static_cast<uint32_t>(begin), 0u, pos};  // (no field asked for; a text without a symbol)
    return Fielded{static_cast<uint32_t>(begin), static_cast<uint32_t>(end), static_cast<uint32_t>(end >> 32) - pos, pos};
}

// k_field_long: long_rows with field_stream; thread 0 stores the row's position beside its TakeRow.
// LDS as k_batch_decode, the reduction's 12 words and the second scan's 4.
__global__ __launch_bounds__(BB) void k_field_long(PackedStore store, const uint2 *__restrict__ codes, uint32_t n_codes, FieldJob job, TakeRow *__restrict__ plan,
                                                   const uint32_t *__restrict__ long_list, const unsigned long long *__restrict__ stats) {
    __shared__ BatchDecLds s;
    __shared__ unsigned long long s_red[3 * (BB / 64)];
    __shared__ uint32_t s_scan[BB / 64];
    long_rows(job.n_rows, long_list, stats, [&] { return load_tables(s.t, codes, n_codes), true; }, [&](uint32_t k) {
        const Judged rec = judge_row(store, job.rows, k);
        if (!stored_text(rec)) return;
        const FieldAsk ask = field_ask(job, k);
        if (!ask.b) return;
        const uint32_t len = static_cast<uint32_t>(rec.len);
        const BodyBits g = reach_body(store, rec, len);
        const Fielded f = field_stream(s, n_codes, g, len, ask, job.delim, s_red, s_scan);
        if (threadIdx.x == 0) {
            store_row(plan, k, field_row(g, f));
            if (job.d_pos) job.d_pos[k] = f.pos;
        }
    });
}

// --------------------------------------------------------------------------------
// The concat call: row k of the new store is text(A[rows_a[k]]) + the literal + text(B[rows_b[k]]), text() the stored text.  Under one
// complete prefix-free table the body the encoder writes for x + y is the bits of x followed by the bits of y, so a row is three runs
// of BITS laid end to end: the left record's stored text (the slice's walk from symbol 0 to the end finds where its last codeword
// ends; the pad is dropped), the literal (et_encode_pattern, in the workspace) and the right record's stored text, found the same
// way.  The right run cannot be taken as the take takes a body, 8 * bytes bits and the length whole: behind a left run that ends
// inside a byte its pad would spill into a byte the encoder does not write, and where its length does not end its text the row's own
// pad would read as symbols.  k_take_scan lays the rows out; k_concat_copy writes them, each run shifted to the destination BIT it
// begins at.  The reach of a side is its record's whole length; k_concat_copy's loops are bounded as k_take_copy's.  k_concat_long
// stores the two records of its own row (and, where the walked length fails the row, its status byte and two atomics) and nothing else.
// --------------------------------------------------------------------------------
// A side's run: the ADDRESS of its stored text's first bit, its bits and its symbols; nothing until it is walked.
struct ConcatRun {
    uint64_t bit;
    uint32_t bits, syms;
};

__device__ __forceinline__ ConcatRun concat_run(const BodyBits &g, const Sliced &sl) {
    if (!sl.n) return ConcatRun{0, 0, 0};  // (no codeword ends inside the body: the empty stored text)
    return ConcatRun{static_cast<uint64_t>(reinterpret_cast<uintptr_t>(g.words)) * 8 + sl.begin, sl.end - sl.begin, sl.n};
}

// The row's two records, from its status so far and its runs, and its status: a failed row, and one whose new length lies above the
// limit (PACKED_UNSUPPORTED), is the empty record.
__device__ __forceinline__ uint32_t concat_store(const ConcatJob &job, uint32_t k, uint32_t status, const ConcatRun &a, const ConcatRun &b, TakeRow *__restrict__ plan,
                                                 ConcatPiece *__restrict__ pieces) {
    const uint64_t len = static_cast<uint64_t>(a.syms) + job.sep_len + b.syms;
    if (!status && len > BATCH_SMALL_MAX) status = PACKED_UNSUPPORTED;
    uint4 row = make_uint4(0u, 0u, 0u, 0u), p0 = row, p1 = row;
    if (!status) {
        const uint64_t bits = static_cast<uint64_t>(a.bits) + job.sep_bits + b.bits;  // (three runs of at most 2^23 bits and a little)
        row = make_uint4(static_cast<uint32_t>((bits + 7) >> 3), static_cast<uint32_t>(len), 0u, 0u);
        p0 = make_uint4(static_cast<uint32_t>(a.bit), static_cast<uint32_t>(a.bit >> 32), a.bits, b.bits);
        p1 = make_uint4(static_cast<uint32_t>(b.bit), static_cast<uint32_t>(b.bit >> 32), a.syms, b.syms);
    }
    store_row(plan, k, row);
    reinterpret_cast<uint4 *>(pieces)[2 * k] = p0;  // (ConcatPiece as it lies in memory)
    reinterpret_cast<uint4 *>(pieces)[2 * k + 1] = p1;
    return status;
}

// k_concat_plan: plan_rows over pairs of records.  The row's status is the left record's if that is not OK, else the right's, else
// the new length's; a failed row is the empty record and neither of its bodies is read.  Each side's body up to CONCAT_LANE_BYTES is
// walked by the row's lane (slice_lane, from symbol 0 to the end, nothing cuts); a row with a longer one goes onto long_list and that
// run counts as absent here: k_concat_long completes the row.  LDS 6 KiB + 8 words.
__global__ __launch_bounds__(BB) void k_concat_plan(PackedStore a, PackedStore b, const uint2 *__restrict__ codes, uint32_t n_codes, ConcatJob job, TakeRow *__restrict__ plan,
                                                    ConcatPiece *__restrict__ pieces, uint32_t *__restrict__ long_list, uint8_t *__restrict__ d_status,
                                                    unsigned long long *__restrict__ stats) {
    __shared__ CodeTables t;
    load_tables(t, codes, n_codes);
    __syncthreads();
    plan_rows(job.n_rows, long_list, d_status, stats, [&](uint32_t k) {
        const Judged ra = judge_row(a, job.rows_a, k), rb = judge_row(b, job.rows_b, k);
        RowPlan p{ra.status ? ra.status : rb.status, false};
        ConcatRun run_a{0, 0, 0}, run_b{0, 0, 0};
#pragma unroll 1
        for (int right = 0; right < 2 && !p.status; ++right) {
            const Judged &rec = right ? rb : ra;
            if (!stored_text(rec)) continue;
            const BodyBits g = reach_body(right ? b : a, rec, rec.len);
            if (!lane_walks(g, CONCAT_LANE_BYTES)) {
                p.is_long = true;
                continue;
            }
            const ConcatRun run = concat_run(g, slice_lane(t, n_codes, g, SliceAsk{0u, static_cast<uint32_t>(rec.len)}, SLICE_NO_STOP));
            if (right) run_b = run;
            else run_a = run;
        }
        p.status = concat_store(job, k, p.status, run_a, run_b, plan, pieces);
        if (p.status) p.is_long = false;  // (too long without its long runs already)
        return p;
    });
}

// k_concat_long: long_rows with slice_stream from symbol 0 to the record's end, nothing cuts, for each side of the row that
// k_concat_plan left to it -- one after the other, so a row has one writer.  Thread 0 completes the row's two records from what
// k_concat_plan left of the other side; a row whose length the walks bring above the limit fails here (fail_row_late), the empty
// record.  LDS as k_batch_decode, and the reduction's 12 words.
__global__ __launch_bounds__(BB) void k_concat_long(PackedStore a, PackedStore b, const uint2 *__restrict__ codes, uint32_t n_codes, ConcatJob job, TakeRow *__restrict__ plan,
                                                    ConcatPiece *__restrict__ pieces, const uint32_t *__restrict__ long_list, uint8_t *__restrict__ d_status,
                                                    unsigned long long *__restrict__ stats) {
    __shared__ BatchDecLds s;
    __shared__ unsigned long long s_red[3 * (BB / 64)];
    long_rows(job.n_rows, long_list, stats, [&] { return load_tables(s.t, codes, n_codes), true; }, [&](uint32_t k) {
        const Judged ra = judge_row(a, job.rows_a, k), rb = judge_row(b, job.rows_b, k);
        if (ra.status || rb.status) return;
        const uint4 p0 = reinterpret_cast<const uint4 *>(pieces)[2 * k], p1 = reinterpret_cast<const uint4 *>(pieces)[2 * k + 1];  // what the lane has walked
        ConcatRun run_a{static_cast<uint64_t>(p0.y) << 32 | p0.x, p0.z, p1.z}, run_b{static_cast<uint64_t>(p1.y) << 32 | p1.x, p0.w, p1.w};
#pragma unroll 1
        for (int right = 0; right < 2; ++right) {
            const Judged &rec = right ? rb : ra;
            if (!stored_text(rec)) continue;
            const BodyBits g = reach_body(right ? b : a, rec, rec.len);
            if (lane_walks(g, CONCAT_LANE_BYTES)) continue;
            const ConcatRun run = concat_run(g, slice_stream(s, n_codes, g, SliceAsk{0u, static_cast<uint32_t>(rec.len)}, SLICE_NO_STOP, s_red));
            if (right) run_b = run;
            else run_a = run;
        }
        if (threadIdx.x == 0) {
            const uint32_t status = concat_store(job, k, PACKED_OK, run_a, run_b, plan, pieces);
            if (status) fail_row_late(k, status, d_status, stats);
        }
    });
}

// `n` bits (1 .. 64) from bit address `bit` on (a byte's address * 8 + the bit, from the top), the first at the top of the word and
// zeros behind the last: from the 1 .. 9 bytes that hold one of them (span_word: no aligned word without such a byte is loaded).
__device__ __forceinline__ uint64_t bits_at(uint64_t bit, uint32_t n) {
    const uint32_t sh = static_cast<uint32_t>(bit & 7), nb = (sh + n + 7) >> 3;
    const uintptr_t a = static_cast<uintptr_t>(bit >> 3);
    uint64_t v = __builtin_bswap64(span_word(a, nb < 8 ? nb : 8u)) << sh;
    if (nb > 8) v |= span_word(a + 8, 1) >> (8 - sh);  // (sh > 0 here: the ninth byte's first sh bits)
    if (n < 64) v &= ~0ull << (64 - n);
    return v;
}

// What a run -- the row's bits [r0, r1), which lie at bit address `src` on -- gives to the row's bits [q, qe), qe - q <= 64: its bits
// among them at their places counted from the top, zeros elsewhere.  Nothing is loaded in front of the run's first bit or behind its last.
__device__ __forceinline__ uint64_t run_bits(uint64_t src, uint32_t r0, uint32_t r1, uint32_t q, uint32_t qe) {
    const uint32_t lo = q > r0 ? q : r0, hi = qe < r1 ? qe : r1;
    if (lo >= hi) return 0ull;
    return bits_at(src + (lo - r0), hi - lo) >> (lo - q);
}

// k_concat_copy: k_take_copy's frame -- its tiles, its rows (wg_upper_bound, the TAKE_STAGE_ROWS stretch in LDS), its words and its
// stores, kept apart from it so that the take's two instantiations keep their code (a fix to the frame belongs in both).  What differs is the piece: `c` bytes (1 .. 8) of a
// row from its bit q on are the OR of up to three runs -- the left bits, the literal's, the right bits -- each shifted to the bit it
// begins at and masked to its own bits (run_bits); behind the last run the row's last byte keeps zeros, the encoder's pad.  A row's
// runs come from its ConcatPiece (a 16-byte and an 8-byte load).  LDS 8 KiB + 16 bytes.
__global__ __launch_bounds__(BB) void k_concat_copy(const ConcatPiece *__restrict__ pieces, const uint8_t *__restrict__ sep, uint32_t sep_bits,
                                                    const uint64_t *__restrict__ out_index, uint32_t n_rows, uint8_t *__restrict__ d_out, uint64_t cap) {
    __shared__ uint64_t s_idx[TAKE_STAGE_ROWS];
    __shared__ uint32_t s_cnt[4];
    const uint32_t tid = threadIdx.x;
    const uint64_t total = out_index[n_rows];
    if (total > cap || total == 0) return;
    const uintptr_t out = reinterpret_cast<uintptr_t>(d_out);
    const uint64_t sep_bit = static_cast<uint64_t>(reinterpret_cast<uintptr_t>(sep)) * 8;
    const uint64_t skew = out & (TAKE_TILE_BYTES - 1);  // bytes of tile 0 in front of d_out
    const uint64_t n_tiles = (skew + total + TAKE_TILE_BYTES - 1) / TAKE_TILE_BYTES;
    const uint64_t per = (n_tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t t_begin = blockIdx.x * per, t_end = t_begin + per < n_tiles ? t_begin + per : n_tiles;
    uint32_t hint = 0;  // every entry of out_index in front of it is at most the tile's first offset
    for (uint64_t t = t_begin; t < t_end; ++t) {
        const uint64_t o0 = t ? t * TAKE_TILE_BYTES - skew : 0, o1_full = (t + 1) * TAKE_TILE_BYTES - skew, o1 = o1_full < total ? o1_full : total;
        const uint32_t row_lo = wg_upper_bound(out_index, hint, n_rows + 1, o0, s_cnt) - 1;
        const uint32_t row_end = wg_upper_bound(out_index, row_lo + 1, n_rows + 1, o1 - 1, s_cnt);
        hint = row_end;
        const uint32_t entries = row_end - row_lo + 1;
        const bool staged = entries <= TAKE_STAGE_ROWS;  // (the same for every thread)
        if (staged)
            for (uint32_t i = tid; i < entries; i += BB) s_idx[i] = out_index[row_lo + i];
        __syncthreads();
        auto idx = [&](uint32_t r) -> uint64_t { return staged ? s_idx[r - row_lo] : out_index[r]; };  // r in [row_lo, row_end]
        const uintptr_t tile_addr = (out - skew) + t * TAKE_TILE_BYTES;
#pragma unroll
        for (uint32_t j = 0; j < TAKE_TILE_BYTES / (16 * BB); ++j) {
            const uintptr_t aw = tile_addr + (j * BB + tid) * 16;
            const int64_t rel = static_cast<int64_t>(aw) - static_cast<int64_t>(out);  // the word's first byte as an offset: negative in front of d_out
            if (rel + 16 <= 0 || rel >= static_cast<int64_t>(total)) continue;
            const uint64_t w0 = rel < 0 ? 0 : static_cast<uint64_t>(rel), w1 = static_cast<uint64_t>(rel + 16) < total ? static_cast<uint64_t>(rel + 16) : total;
            uint32_t k = row_lo, hi = row_end;
            while (hi - k > 1) {
                const uint32_t mid = k + (hi - k) / 2;
                if (idx(mid) <= w0) k = mid;
                else hi = mid;
            }
            uint64_t v0 = 0, v1 = 0, pos = w0;
            for (int trip = 0; trip < 16; ++trip) {  // row k owns byte pos: out_index[k] <= pos < out_index[k + 1]
                const uint64_t s = idx(k), e = idx(k + 1), piece_end = e < w1 ? e : w1;
                const uint32_t c = static_cast<uint32_t>(piece_end - pos);  // 1 .. 16
                const uint32_t d = static_cast<uint32_t>(static_cast<int64_t>(pos) - rel);
                const uint4 p0 = reinterpret_cast<const uint4 *>(pieces)[2 * k];
                const uint2 p1 = reinterpret_cast<const uint2 *>(pieces)[4 * k + 2];
                const uint64_t a_bit = static_cast<uint64_t>(p0.y) << 32 | p0.x, b_bit = static_cast<uint64_t>(p1.y) << 32 | p1.x;
                const uint32_t r1 = p0.z, r2 = r1 + sep_bits, r3 = r2 + p0.w;  // where the runs end, in bits of the row
                const uint32_t q = static_cast<uint32_t>(pos - s) * 8, qm = q + 8 * (c < 8 ? c : 8u), qe = q + 8 * c;
                put_bytes(v0, v1, __builtin_bswap64(run_bits(a_bit, 0u, r1, q, qm) | run_bits(sep_bit, r1, r2, q, qm) | run_bits(b_bit, r2, r3, q, qm)), d);
                if (c > 8) put_bytes(v0, v1, __builtin_bswap64(run_bits(a_bit, 0u, r1, qm, qe) | run_bits(sep_bit, r1, r2, qm, qe) | run_bits(b_bit, r2, r3, qm, qe)), d + 8);
                pos = piece_end;
                if (pos >= w1) break;
                ++k;  // (a row behind owns byte pos < o1: k < row_end)
                if (idx(k + 1) <= pos) {  // empty rows follow: the last r in [k, row_end) with out_index[r] <= pos
                    hi = row_end;
                    while (hi - k > 1) {
                        const uint32_t mid = k + (hi - k) / 2;
                        if (idx(mid) <= pos) k = mid;
                        else hi = mid;
                    }
                }
            }
            if (w1 - w0 == 16) {
                *reinterpret_cast<uint4 *>(aw) = make_uint4(static_cast<uint32_t>(v0), static_cast<uint32_t>(v0 >> 32), static_cast<uint32_t>(v1), static_cast<uint32_t>(v1 >> 32));
            } else {  // the output's first or last word: its own bytes alone
                for (uint32_t i = static_cast<uint32_t>(static_cast<int64_t>(w0) - rel); i < static_cast<uint32_t>(static_cast<int64_t>(w1) - rel); ++i)
                    reinterpret_cast<uint8_t *>(aw)[i] = static_cast<uint8_t>((i < 8 ? v0 >> (8 * i) : v1 >> (8 * (i - 8))) & 0xffu);
            }
        }
        __syncthreads();  // (s_idx: between two tiles)
    }
}

// --------------------------------------------------------------------------------
// The recode call: row k of the new store is bytes(map[c] for c in text(rows[k]) if map[c] is kept), text() the stored text under
// table IN, written as the encoder writes it under table OUT.  The walk of the decodes feeds the pack loop of the encodes with
// nothing in between: for every symbol s of the stored text the entry s of ONE table -- map composed with OUT by the host, 256 x
// {left-aligned code, length} indexed by the INPUT symbol -- is laid behind the one before.  Length 0: the byte is dropped;
// RECODE_UNCODED: it is kept but has no code under OUT, and the row fails (PACKED_UNSUPPORTED, the empty record).
// Nothing but a symbol of the stored text (cut_at_length's rule) is looked up in the output table, so a codeword behind the length
// or in the pad fails no row.  The reach of a row is its record's whole length.
// The body is read twice (sizes, then bits) and the new body written once.  A row owns whole bytes: no two rows share an output
// byte, pad bits are zero because the accumulators begin as zeros, and every store is clipped to the row's own bytes.
// Beside the derived stores' bounds: the flush rounds of a block are bounded by the block's output bits (at most 65 536 codewords of
// 32 bits: 16 rounds).
// --------------------------------------------------------------------------------
// What a walk over a stored text sums: the new body's bits, its symbols, and whether a kept symbol has no code under OUT.
struct Recoded {
    uint32_t bits, kept, uncoded;
    __device__ __forceinline__ void add(const uint2 e) {
        bits += e.y & RECODE_LEN_MASK;
        kept += e.y != 0;
        uncoded |= e.y >> 31;
    }
};

// The TakeRow of a recoded row as it lies in memory: the new body's bytes, its symbols, its BITS (the long write bounds its rounds by them).
__device__ __forceinline__ uint4 recode_row(const Recoded &r) {
    if (r.uncoded || !r.bits) return make_uint4(0u, 0u, 0u, 0u);
    return make_uint4((r.bits + 7) >> 3, r.kept, r.bits, 0u);
}

// k_recode_plan: plan_rows with the output table beside the code tables in LDS.  A record without bytes or symbols has the empty
// stored text and is not read; a body up to RECODE_LANE_BYTES is walked by its lane (lane_walk to the end of the stored text), and
// a kept symbol without a code fails the row here.  LDS 8 KiB + 8 words.
__global__ __launch_bounds__(BB) void k_recode_plan(PackedStore store, const uint2 *__restrict__ codes, uint32_t n_codes, RecodeJob job, TakeRow *__restrict__ plan,
                                                    uint32_t *__restrict__ long_list, uint8_t *__restrict__ d_status, unsigned long long *__restrict__ stats) {
    __shared__ CodeTables t;
    __shared__ uint2 s_otab[256];
    s_otab[threadIdx.x] = job.out_tab[threadIdx.x];
    load_tables(t, codes, n_codes);
    __syncthreads();
    plan_rows(job.n_rows, long_list, d_status, stats, [&](uint32_t k) {
        const Judged rec = judge_row(store, job.rows, k);
        RowPlan p{rec.status, false};
        uint4 row = make_uint4(0u, 0u, 0u, 0u);
        if (stored_text(rec)) {
            const BodyBits g = reach_body(store, rec, rec.len);
            if (lane_walks(g, RECODE_LANE_BYTES)) {
                Recoded sum{0u, 0u, 0u};
                (void)lane_walk(t, n_codes, g, static_cast<uint32_t>(rec.len), [&](uint32_t, uint32_t, uint32_t meta) {
                    sum.add(s_otab[meta & 0xffu]);
                    return true;
                });
                if (sum.uncoded) p.status = PACKED_UNSUPPORTED;
                row = recode_row(sum);
            } else {
                p.is_long = true;
            }
        }
        store_row(plan, k, row);
        return p;
    });
}

// The visitor of the settling walks of the recode: what the walk's codewords give under the output table.
struct SumRecoded {
    const uint2 *otab;
    Recoded r;
    __device__ __forceinline__ bool operator()(uint32_t, uint32_t, uint32_t, uint32_t meta) {
        r.add(otab[meta & 0xffu]);
        return true;
    }
};

// One block of a long row, settled and cut at the length (cut_at_length): what each lane's symbols OF THE STORED TEXT give.  `done`:
// the codewords of the blocks before.
struct RecodedBlock {
    Settled b;
    uint32_t held;  // the lane's symbols of the stored text
    Recoded mine;   // ... and what they give
};

__device__ __forceinline__ RecodedBlock recode_block(BatchDecLds &s, const uint2 *otab, uint32_t n_codes, const BodyBits &g, uint32_t blk, uint32_t start, uint32_t done,
                                                     uint32_t len) {
    const SumRecoded fresh{otab, Recoded{0u, 0u, 0u}};
    SumRecoded summing = fresh;
    RecodedBlock rb;
    rb.b = settle_block(s, n_codes, g, blk, start, summing);
    rb.held = cut_at_length(s, n_codes, rb.b, done + rb.b.first, len, summing, fresh);
    rb.mine = summing.r;
    return rb;
}

// k_recode_long: long_rows.  Per block the lanes' three sums are added up over the workgroup (two scans: the bits; the symbols with
// the flag's count above them) and carried in registers across the blocks.  Thread 0 stores the row's TakeRow, or fails the row
// (fail_row_late) where a kept symbol has no code.
// LDS as k_batch_decode, the output table's 2 KiB and the scans' 4 words: 35.2 KiB.
__global__ __launch_bounds__(BB) void k_recode_long(PackedStore store, const uint2 *__restrict__ codes, uint32_t n_codes, RecodeJob job, TakeRow *__restrict__ plan,
                                                    const uint32_t *__restrict__ long_list, uint8_t *__restrict__ d_status, unsigned long long *__restrict__ stats) {
    __shared__ BatchDecLds s;
    __shared__ uint2 s_otab[256];
    __shared__ uint32_t s_scan[BB / 64];
    const auto set_up = [&] {
        s_otab[threadIdx.x] = job.out_tab[threadIdx.x];
        load_tables(s.t, codes, n_codes);
        return true;
    };
    long_rows(job.n_rows, long_list, stats, set_up, [&](uint32_t k) {
        const Judged rec = judge_row(store, job.rows, k);
        if (!stored_text(rec)) return;
        const uint32_t len = static_cast<uint32_t>(rec.len);
        const BodyBits g = reach_body(store, rec, len);
        const uint32_t n_blocks = (g.n_words + DEC_WORDS - 1) / DEC_WORDS;
        uint32_t start = g.first_bit, done = 0;  // the block's first codeword; codewords so far
        Recoded sum{0u, 0u, 0u};
        for (uint32_t blk = 0; blk < n_blocks && done < len; ++blk) {
            const RecodedBlock rb = recode_block(s, s_otab, n_codes, g, blk, start, done, len);
            uint32_t bits, rest;  // (a block's codewords: at most 65 536 + 8, its flags at most 256: the two share a word)
            (void)block_exclusive_scan(rb.mine.bits, s_scan, &bits);
            __syncthreads();
            (void)block_exclusive_scan(rb.mine.kept | rb.mine.uncoded << 20, s_scan, &rest);
            sum.bits += bits;
            sum.kept += rest & 0xfffffu;
            sum.uncoded |= rest >> 20;
            start = rb.b.start;
            done += rb.b.total;
        }
        if (threadIdx.x == 0) {
            store_row(plan, k, recode_row(sum));
            if (sum.uncoded) fail_row_late(k, PACKED_UNSUPPORTED, d_status, stats);
        }
    });
}

// store_image_word for the recode's writes (a copy: shared, it changed the comparison sequence of k_shared_encode's and k_packed_pack's clipped stores).
__device__ __forceinline__ void recode_store_word(uint8_t *line, uint32_t g, uint32_t v, uint32_t lo, uint32_t hi) {
    const uint32_t b0 = g * 4;
    if (b0 >= lo && b0 + 4 <= hi) {
        reinterpret_cast<uint32_t *>(line)[g] = v;
    } else {
        for (uint32_t k = 0; k < 4; ++k)
            if (b0 + k >= lo && b0 + k < hi) line[b0 + k] = static_cast<uint8_t>(v >> (8 * k));
    }
}

// Where a row's bits go: the image begins at the aligned word that holds the row's first byte; the row's bytes are image bytes [lo, hi).
struct RecodeDst {
    uint8_t *line;
    uint32_t lo, hi;
};

__device__ __forceinline__ RecodeDst recode_dst(uint8_t *d_out, uint64_t at, uint32_t bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_out) + at;
    const uint32_t lo = static_cast<uint32_t>(a & 3);
    return RecodeDst{reinterpret_cast<uint8_t *>(a & ~static_cast<uintptr_t>(3)), lo, lo + bytes};
}

// k_recode_write: the rows a lane has planned, a row per lane, k_recode_plan's walk once more: every kept symbol's code goes into a
// 64-bit accumulator that begins at the destination's aligned word (the bytes in front of the row are zeros in it and are clipped
// from the store); a word that has filled leaves as one dword store, the row's first and last word as their own bytes
// (recode_store_word), the last one with zero bits behind the body.  Failed and empty rows have no bytes; a listed row is
// k_recode_write_long's.  Nothing is written when the rows need more than cap.  LDS 8 KiB.
__global__ __launch_bounds__(BB) void k_recode_write(PackedStore store, const uint2 *__restrict__ codes, uint32_t n_codes, RecodeJob job, const TakeRow *__restrict__ plan,
                                                     const uint64_t *__restrict__ out_index, uint8_t *__restrict__ d_out, uint64_t cap) {
    __shared__ CodeTables t;
    __shared__ uint2 s_otab[256];
    if (out_index[job.n_rows] > cap) return;  // (the same for every thread)
    s_otab[threadIdx.x] = job.out_tab[threadIdx.x];
    load_tables(t, codes, n_codes);
    __syncthreads();
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * BB + threadIdx.x; k < job.n_rows; k += static_cast<uint64_t>(gridDim.x) * BB) {
        const uint32_t bytes = plan[k].body_bytes;
        if (!bytes) continue;
        const Judged rec = judge_row(store, job.rows, static_cast<uint32_t>(k));
        if (!stored_text(rec)) continue;  // (such a row has no bytes)
        const BodyBits g = reach_body(store, rec, rec.len);
        if (!lane_walks(g, RECODE_LANE_BYTES)) continue;
        const RecodeDst dst = recode_dst(d_out, out_index[k], bytes);
        uint32_t word = 0, fill = dst.lo * 8;
        uint64_t acc = 0;
        (void)lane_walk(t, n_codes, g, static_cast<uint32_t>(rec.len), [&](uint32_t, uint32_t, uint32_t meta) {
            const uint2 e = s_otab[meta & 0xffu];
            const uint32_t n = e.y & RECODE_LEN_MASK;
            if (!n) return true;
            acc |= (static_cast<uint64_t>(e.x) << 32) >> fill;  // (fill < 32 here: the code's 32 bits stay inside the 64)
            fill += n;
            if (fill >= 32) {
                recode_store_word(dst.line, word, __builtin_bswap32(static_cast<uint32_t>(acc >> 32)), dst.lo, dst.hi);
                acc <<= 32;
                ++word;
                fill -= 32;
            }
            return true;
        });
        if (fill) recode_store_word(dst.line, word, __builtin_bswap32(static_cast<uint32_t>(acc >> 32)), dst.lo, dst.hi);
    }
}

// k_recode_write_long: long_rows over the listed rows that have bytes, block by block: the block settled and cut as k_recode_long
// does it (recode_block), the lanes' output bits scanned to each lane's destination bit within the block, then rounds of
// RECODE_ROUND_BITS destination bits -- one 8 KiB block of 1-bit codes becomes 256 KiB of 32-bit ones, sixteen rounds; a block of
// 32-bit codes that become 1-bit ones is one round of 256 bytes: a round never spans two input blocks, the partial word is what
// crosses.  In a round the lanes whose bits meet it walk again and OR their codes into the LDS image (BatchDecLds::out: pack_round's
// inner loop -- an accumulator, atomicOr where a word fills); a code that straddles a round's edge leaves its bits on either side in
// their own rounds.  Whole words leave as byte-swapped dword stores, the row's first and last word clipped to its bytes, the word a
// round ends in is carried as `pending` (pack_rounds' hand-over).  The image is zero between rounds: the set-up zeroes it, behind the
// two returns.  Nothing is written when the rows need more than cap.
// LDS as k_recode_long: 35.2 KiB, three workgroups per CU.
__global__ __launch_bounds__(BB) void k_recode_write_long(PackedStore store, const uint2 *__restrict__ codes, uint32_t n_codes, RecodeJob job,
                                                          const TakeRow *__restrict__ plan, const uint32_t *__restrict__ long_list,
                                                          const unsigned long long *__restrict__ stats, const uint64_t *__restrict__ out_index,
                                                          uint8_t *__restrict__ d_out, uint64_t cap) {
    static_assert(RECODE_ROUND_BITS / 32 + 2 <= sizeof(BatchDecLds::out) / 4, "a round's words, the word it begins in and the one it ends in");
    __shared__ BatchDecLds s;
    __shared__ uint2 s_otab[256];
    __shared__ uint32_t s_scan[BB / 64];
    const uint32_t tid = threadIdx.x;
    const auto set_up = [&] {
        if (out_index[job.n_rows] > cap) return false;  // (the same for every thread)
        s_otab[tid] = job.out_tab[tid];
        load_tables(s.t, codes, n_codes);
        for (uint32_t i = tid; i < sizeof(s.out) / 4; i += BB) s.out[i] = 0u;
        return true;
    };
    long_rows(job.n_rows, long_list, stats, set_up, [&](uint32_t k) {
        const uint32_t bytes = plan[k].body_bytes;
        if (!bytes) return;  // a failed row, or one whose every symbol is dropped
        const Judged rec = judge_row(store, job.rows, k);
        if (!stored_text(rec)) return;
        const uint32_t len = static_cast<uint32_t>(rec.len);
        const BodyBits g = reach_body(store, rec, len);
        const RecodeDst dst = recode_dst(d_out, out_index[k], bytes);
        const uint32_t n_blocks = (g.n_words + DEC_WORDS - 1) / DEC_WORDS;
        uint32_t start = g.first_bit, done = 0;     // the block's first codeword; codewords so far
        uint32_t carry = dst.lo * 8, pending = 0;   // the image bit the next round begins at; the bits of word carry / 32 in front of it
        for (uint32_t blk = 0; blk < n_blocks && done < len; ++blk) {
            const RecodedBlock rb = recode_block(s, s_otab, n_codes, g, blk, start, done, len);
            uint32_t block_bits;
            const uint32_t before = block_exclusive_scan(rb.mine.bits, s_scan, &block_bits);  // the lane's first output bit within the block
            for (uint32_t w0 = 0; w0 < block_bits; w0 += RECODE_ROUND_BITS) {
                const uint32_t round_bits = block_bits - w0 < RECODE_ROUND_BITS ? block_bits - w0 : RECODE_ROUND_BITS, w1 = w0 + round_bits;
                const uint32_t base = carry & 31;  // the round's first bit in the image
                if (tid == 0 && pending) atomicOr(&s.out[0], pending);
                if (rb.mine.bits && before < w1 && before + rb.mine.bits > w0) {
                    uint32_t p = before, wi = 0, fill = 0, again;
                    uint64_t acc = 0;
                    bool open = false;
                    (void)walk(s, n_codes, rb.b.used, rb.b.room, &again, [&](uint32_t cnt, uint32_t, uint32_t, uint32_t meta) {
                        if (cnt >= rb.held) return false;
                        const uint2 e = s_otab[meta & 0xffu];
                        uint32_t n = e.y & RECODE_LEN_MASK, v = e.x, at = p;
                        if (!n) return true;
                        if (at >= w1) return false;
                        p += n;
                        if (p <= w0) return true;
                        if (at < w0) {  // the code's first bits went out with the round before
                            v <<= w0 - at;
                            n -= w0 - at;
                            at = w0;
                        }
                        if (at + n > w1) {  // ... and its last ones go out with the next
                            n = w1 - at;
                            v &= ~0u << (32 - n);
                        }
                        if (!open) {
                            const uint32_t q = base + (at - w0);
                            wi = q >> 5;
                            fill = q & 31;
                            open = true;
                        }
                        acc |= (static_cast<uint64_t>(v) << 32) >> fill;
                        fill += n;
                        if (fill >= 32) {
                            atomicOr(&s.out[wi], static_cast<uint32_t>(acc >> 32));
                            acc <<= 32;
                            ++wi;
                            fill -= 32;
                        }
                        return true;
                    });
                    if (fill) atomicOr(&s.out[wi], static_cast<uint32_t>(acc >> 32));
                }
                __syncthreads();
                const uint32_t t_bits = base + round_bits, full = t_bits >> 5, first_word = carry >> 5;
                pending = (t_bits & 31) ? s.out[full] : 0u;
                __syncthreads();
                for (uint32_t w = tid; w <= full; w += BB) {
                    if (w < full) recode_store_word(dst.line, first_word + w, __builtin_bswap32(s.out[w]), dst.lo, dst.hi);
                    s.out[w] = 0u;
                }
                carry += round_bits;
                __syncthreads();
            }
            start = rb.b.start;
            done += rb.b.total;
        }
        if (tid == 0 && (carry & 31)) recode_store_word(dst.line, carry >> 5, __builtin_bswap32(pending), dst.lo, dst.hi);
    });
}

// --------------------------------------------------------------------------------
// The number call: rows[]' slices s = text_b[first : first + count], cut in front of the first `stop`, READ as integers of the
// grammar [+-]?[0-9]+ -- a word per row, and sums, counts, minima and maxima per group -- with nothing decoded and no store made.  The
// ask, the judgement, the reach and both walks are the slice's; the family's middle is what a walk notes: not two bit positions
// but the digits themselves, accumulated by NumberParse, which the lane's walk and the workgroup's parse lane both use.  Three
// launches in stream order behind the fill of the aggregates (et_batch.h), the host waiting for the last: the fold.
// --------------------------------------------------------------------------------
// THE state machine: take(sym) per symbol of s, in order; false: the row is BAD and nothing behind changes that.  The magnitude
// SATURATES at 2^64 - 1 (`over`), so a run of digits of any length is judged right: never wrapped into range.
struct NumberParse {
    enum : uint32_t { NEG = 1, DIGITS = 2, OVER = 4, BAD = 8 };
    uint64_t mag = 0;
    uint32_t n = 0, flags = 0;  // symbols seen; what they were (one word of bits: the state is a lane's own, in registers)

    __device__ __forceinline__ bool take(uint32_t sym) {
        constexpr uint64_t TENTH = ~0ull / 10;  // (2^64 - 1 = 10 * TENTH + 5)
        const uint32_t d = sym - '0';
        const bool digit = d <= 9u, sign = n == 0 && (sym == '+' || sym == '-');
        uint32_t f = flags;
        f |= ++n > NUMBER_SYMBOLS_MAX || !(digit || sign) ? BAD : 0u;
        f |= digit ? DIGITS : 0u;
        f |= sign && sym == '-' ? NEG : 0u;
        if (digit) {
            const bool over = (f & OVER) || mag > TENTH || (mag == TENTH && d > 5u);
            mag = over ? ~0ull : mag * 10 + d;
            f |= over ? OVER : 0u;
        }
        flags = f;
        return !(f & BAD);
    }

    __device__ __forceinline__ NumberRow row() const {
        const uint64_t most = flags & NEG ? 1ull << 63 : (1ull << 63) - 1;
        const uint32_t kind = !n ? NUMBER_EMPTY : (flags & BAD) || !(flags & DIGITS) ? NUMBER_BAD : (flags & OVER) || mag > most ? NUMBER_RANGE : NUMBER_OK;
        return NumberRow{kind ? 0 : static_cast<int64_t>(flags & NEG ? 0 - mag : mag), kind, 0u};  // (-2^63 is 0 - 2^63 in 64 bits)
    }
};

// A row's outputs: the two the caller may have asked for, and the NumberRow the fold reads.  A failed row is EMPTY with value 0 to
// the caller and NUMBER_FAILED to the fold, which counts it nowhere.
__device__ __forceinline__ void store_number(const NumberJob &job, NumberRow *__restrict__ rows, uint32_t k, const NumberRow &r) {
    reinterpret_cast<uint4 *>(rows)[k] = make_uint4(static_cast<uint32_t>(r.value), static_cast<uint32_t>(static_cast<uint64_t>(r.value) >> 32), r.kind, 0u);  // (NumberRow as it lies in memory)
    if (job.d_values) job.d_values[k] = r.value;
    if (job.d_kind) job.d_kind[k] = static_cast<uint8_t>(r.kind == NUMBER_FAILED ? NUMBER_EMPTY : r.kind);
}

// k_number_fill: min and max have first values that no byte pattern gives.  A group per lane; either may be null.
__global__ __launch_bounds__(BB) void k_number_fill(int64_t *__restrict__ d_min, int64_t *__restrict__ d_max, uint32_t n_groups) {
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * BB + threadIdx.x; g < n_groups; g += static_cast<uint64_t>(gridDim.x) * BB) {
        if (d_min) d_min[g] = INT64_MAX;
        if (d_max) d_max[g] = INT64_MIN;
    }
}

// k_number_plan: plan_rows, k_slice_plan's tables and ask.  A row whose group number names no group fails here, alone, like a row
// whose record does.  A row that asks for nothing, or of a record without bytes or symbols, is EMPTY and is not read.  The lane's
// visitor steps over the symbols in front of ask.first, ends the walk at `stop`, and hands every other symbol to the state machine,
// which ends it at the first that makes the row BAD -- the 33rd at the latest.  LDS 6 KiB + 8 words.
__global__ __launch_bounds__(BB) void k_number_plan(PackedStore store, const uint2 *__restrict__ codes, uint32_t n_codes, NumberJob job, NumberRow *__restrict__ rows,
                                                    uint32_t *__restrict__ long_list, uint8_t *__restrict__ d_status, unsigned long long *__restrict__ stats) {
    __shared__ CodeTables t;
    load_tables(t, codes, n_codes);
    __syncthreads();
    plan_rows(job.ask.n_rows, long_list, d_status, stats, [&](uint32_t k) {
        const Judged rec = judge_row(store, job.ask.rows, k);
        RowPlan p{rec.status, false};
        if (!p.status && job.group_of) {
            const uint32_t group = job.group_of[k];
            if (group != GROUP_NONE && group >= job.n_groups) p.status = PACKED_ARG;
        }
        NumberRow r{0, p.status ? NUMBER_FAILED : NUMBER_EMPTY, 0u};
        if (!p.status && stored_text(rec)) {
            const SliceAsk ask = slice_ask(job.ask, k, static_cast<uint32_t>(rec.len));
            if (ask.end > ask.first) {
                const BodyBits g = reach_body(store, rec, ask.end);
                if (lane_walks(g, NUMBER_LANE_BYTES)) {
                    NumberParse parse;
                    (void)lane_walk(t, n_codes, g, ask.end, [&](uint32_t idx, uint32_t, uint32_t meta) {
                        if (idx < ask.first) return true;
                        return (meta & 0xffu) != job.ask.stop && parse.take(meta & 0xffu);
                    });
                    r = parse.row();
                } else {
                    p.is_long = true;
                }
            }
        }
        store_number(job, rows, k, r);
        return p;
    });
}

// The run of bits [begin, end) of a body as a body of its own: counted from the aligned word `begin` lies in, as lane_walk takes it.
__device__ __forceinline__ BodyBits bits_between(const BodyBits &g, uint32_t begin, uint32_t end) {
    BodyBits h;
    h.words = g.words + (begin >> 5);
    h.first_bit = begin & 31;
    h.end_bit = end - (begin & ~31u);
    h.n_words = (h.end_bit + 31) >> 5;  // (end <= g.end_bit: no word behind the body's last)
    return h;
}

// k_number_long: long_rows with slice_stream, unchanged: what it returns is the number's run of bits and its symbols.  More than
// NUMBER_SYMBOLS_MAX symbols are BAD without another look; otherwise thread 0 alone walks the run -- at most 32 trips, nothing behind
// the slice's end visited, no stop among its symbols -- with the lane's state machine, and stores the row's outputs.  The plan kernel
// lists OK rows only: nothing fails here.  LDS as k_slice_long.
__global__ __launch_bounds__(BB) void k_number_long(PackedStore store, const uint2 *__restrict__ codes, uint32_t n_codes, NumberJob job, NumberRow *__restrict__ rows,
                                                    const uint32_t *__restrict__ long_list, const unsigned long long *__restrict__ stats) {
    __shared__ BatchDecLds s;
    __shared__ unsigned long long s_red[3 * (BB / 64)];
    long_rows(job.ask.n_rows, long_list, stats, [&] { return load_tables(s.t, codes, n_codes), true; }, [&](uint32_t k) {
        const Judged rec = judge_row(store, job.ask.rows, k);
        if (!stored_text(rec)) return;
        const SliceAsk ask = slice_ask(job.ask, k, static_cast<uint32_t>(rec.len));
        if (ask.end <= ask.first) return;
        const BodyBits g = reach_body(store, rec, ask.end);
        const Sliced sl = slice_stream(s, n_codes, g, ask, job.ask.stop, s_red);
        if (threadIdx.x != 0 || !sl.n) return;  // (no symbols: the plan kernel's EMPTY stands)
        NumberRow r{0, NUMBER_BAD, 0u};
        if (sl.n <= NUMBER_SYMBOLS_MAX && sl.end > sl.begin && sl.end <= g.end_bit) {
            NumberParse parse;
            (void)lane_walk(s.t, n_codes, bits_between(g, sl.begin, sl.end), sl.n, [&](uint32_t, uint32_t, uint32_t meta) { return parse.take(meta & 0xffu); });
            r = parse.row();
        }
        store_number(job, rows, k, r);
    });
}

// Sum, minimum and maximum of the lanes of a wavefront; a lane outside holds the identity.  Every lane has the three on return.
__device__ __forceinline__ void reduce_sum_min_max(uint64_t &sum, int64_t &lo, int64_t &hi) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sum += __shfl_xor(sum, d, 64);
        const int64_t ol = __shfl_xor(lo, d, 64), oh = __shfl_xor(hi, d, 64);
        if (ol < lo) lo = ol;
        if (oh > hi) hi = oh;
    }
}

// One atomic per aggregate that was asked for.  The sum wraps modulo 2^64: an unsigned add.
__device__ __forceinline__ void fold_into(const NumberJob &job, uint32_t group, uint64_t sum, unsigned long long n, int64_t lo, int64_t hi) {
    if (job.d_sum) atomicAdd(reinterpret_cast<unsigned long long *>(job.d_sum) + group, static_cast<unsigned long long>(sum));
    if (job.d_n) atomicAdd(job.d_n + group, n);
    if (job.d_min) atomicMin(reinterpret_cast<long long *>(job.d_min) + group, static_cast<long long>(lo));
    if (job.d_max) atomicMax(reinterpret_cast<long long *>(job.d_max) + group, static_cast<long long>(hi));
}

// k_number_fold: a row per lane over the NumberRows that the two kernels in front left, whatever the caller asked to see.  The
// kinds but OK are counted per lane, reduced over the wavefront and the workgroup (4 x 3 words of LDS) and added to the counters by
// thread 0.  AGG: every OK row whose group is one (a row of ET_GROUP_NONE is skipped; a number beyond n_groups failed its row in the
// plan kernel, and is asked again for what is written below) is folded into its group's aggregates, the adds combined in the
// wavefront first, by k_group_number's rounds: the lowest lane left takes its group, the ballot of the lanes with that group is its
// share, the three values are reduced over the share -- a round that found its leader alone skips that --, the leader issues the
// atomics; after GROUP_COMBINE_MISSES rounds without company the rest adds singly.  A whole-column SUM sends one add per wavefront to
// its one address, not 64.  Integer adds, min and max commute: every aggregate is exact and the same on every call.
// The report: thread 0's counts are in `stats` before its tick of NUMBER_ARRIVED (packed_report's fences); the last workgroup to tick
// reads the counters back, stores them and hands over.  No workgroup waits for another.
template <bool AGG>
__global__ __launch_bounds__(BB) void k_number_fold(const NumberRow *__restrict__ rows, NumberJob job, PackedReport report) {
    __shared__ unsigned long long s_kinds[3][BB / 64];
    const uint32_t n_rows = job.ask.n_rows, lane = threadIdx.x & 63;
    unsigned long long kinds[3] = {0, 0, 0};
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * BB; base < n_rows; base += static_cast<uint64_t>(gridDim.x) * BB) {
        const uint32_t k = static_cast<uint32_t>(base) + threadIdx.x;
        uint32_t group = GROUP_NONE;
        int64_t value = 0;
        if (k < n_rows) {
            const uint4 r = reinterpret_cast<const uint4 *>(rows)[k];  // (NumberRow as it lies in memory)
            kinds[0] += r.z == NUMBER_EMPTY;
            kinds[1] += r.z == NUMBER_BAD;
            kinds[2] += r.z == NUMBER_RANGE;
            if (AGG && r.z == NUMBER_OK) {
                group = job.group_of ? job.group_of[k] : 0u;
                if (group >= job.n_groups) group = GROUP_NONE;
                value = static_cast<int64_t>(static_cast<uint64_t>(r.y) << 32 | r.x);
            }
        }
        if (AGG) {
            unsigned long long left = __ballot(group != GROUP_NONE);
            for (uint32_t alone = 0; left && alone < GROUP_COMBINE_MISSES;) {
                const int leader = __ffsll(left) - 1;
                const uint32_t lead_group = __shfl(group, leader, 64);
                const bool in = group == lead_group;  // (lead_group is a group: no lane without one is in it; a lane served before has another)
                const unsigned long long same = __ballot(in);
                const bool single = (same & (same - 1)) == 0;
                uint64_t sum = in ? static_cast<uint64_t>(value) : 0ull;
                int64_t lo = in ? value : INT64_MAX, hi = in ? value : INT64_MIN;
                if (!single) reduce_sum_min_max(sum, lo, hi);  // (the same for the whole wavefront)
                if (static_cast<int>(lane) == leader) fold_into(job, lead_group, sum, static_cast<unsigned long long>(__popcll(same)), lo, hi);
                left &= ~same;
                alone += single;
            }
            if ((left >> lane) & 1) fold_into(job, group, static_cast<uint64_t>(value), 1ull, value, value);
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) kinds[i] += __shfl_xor(kinds[i], d, 64);
        if (lane == 0) s_kinds[i][threadIdx.x >> 6] = kinds[i];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long *stats = report.stats, *host_result = report.host_result;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        unsigned long long total = 0;
        for (int w = 0; w < BB / 64; ++w) total += s_kinds[i][w];
        if (total) atomicAdd(stats + NUMBER_N_EMPTY + i, total);
    }
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the counts have landed before the tick leaves
    const unsigned long long before = atomicAdd(stats + NUMBER_ARRIVED, 1ull);
    if (before != gridDim.x - 1) return;
    __threadfence();
    host_result[NUMBER_ARRIVED] = 0;
    host_result[PACKED_N_FAILED] = atomicAdd(stats + PACKED_N_FAILED, 0ull);
    host_result[PACKED_FIRST] = atomicMin(stats + PACKED_FIRST, ~0ull);
    host_result[NUMBER_N_EMPTY] = atomicAdd(stats + NUMBER_N_EMPTY, 0ull);
    host_result[NUMBER_N_BAD] = atomicAdd(stats + NUMBER_N_BAD, 0ull);
    host_result[NUMBER_N_RANGE] = atomicAdd(stats + NUMBER_N_RANGE, 0ull);
    hand_over(report.host_done, report.epoch);
}

// --------------------------------------------------------------------------------
static uint32_t batch_grid(uint32_t n) { return n < MAX_GRID ? n : MAX_GRID; }

static uint32_t capped(uint64_t n, uint32_t most) { return n < most ? static_cast<uint32_t>(n) : most; }

static uint32_t tiles_of(uint32_t n) { return (n + MATCH_TILE - 1) / MATCH_TILE; }

// k_packed_scan over n sizes; REPORT: the call's report leaves with it.
template <bool REPORT>
static void launch_scan(hipStream_t stream, const uint32_t *sizes, uint32_t n, uint64_t *out_index, const PackedReport &r) {
    hipLaunchKernelGGL(k_packed_scan<REPORT>, dim3(1), dim3(BB), 0, stream, sizes, n, out_index, static_cast<const unsigned long long *>(r.stats), r.host_result, r.host_done, r.epoch);
}

// The match's and the join's last two launches: the scan of the tile counts, which reports, and -- unless d_rows is null -- the emit.
static void launch_scan_emit(hipStream_t stream, uint32_t n_tiles, uint32_t grid, const TileWs &tiles, uint32_t *d_rows, uint64_t cap_rows, const uint32_t *key_of,
                             uint32_t *d_key_of_row, const PackedReport &r) {
    launch_scan<true>(stream, tiles.counts, n_tiles, tiles.base, r);
    if (!d_rows) return;
    const unsigned long long *masks = tiles.masks;
    const uint64_t *base = tiles.base;
    if (d_key_of_row) hipLaunchKernelGGL(k_rows_emit<true>, dim3(grid), dim3(BB), 0, stream, masks, base, n_tiles, d_rows, cap_rows, key_of, d_key_of_row);
    else hipLaunchKernelGGL(k_rows_emit<false>, dim3(grid), dim3(BB), 0, stream, masks, base, n_tiles, d_rows, cap_rows, key_of, d_key_of_row);
}

// The grids of the take and the derived stores: a plan kernel's (a row per lane), a long kernel's (a listed row per workgroup).
static uint32_t plan_grid(uint32_t n_rows) { return capped((n_rows + BB - 1) / BB, GATHER_PLAN_GRID); }

static uint32_t long_grid(uint32_t n_rows) { return capped(n_rows, SHARED_DEC_GRID); }

// k_take_scan behind the plan: the call's report leaves with it.
static void launch_take_scan(hipStream_t stream, const TakeRow *plan, uint32_t n_rows, uint64_t *out_body_index, uint64_t *out_text_index, const PackedReport &r) {
    hipLaunchKernelGGL(k_take_scan, dim3(1), dim3(BB), 0, stream, plan, n_rows, out_body_index, out_text_index, static_cast<const unsigned long long *>(r.stats), r.host_result,
                       r.host_done, r.epoch);
}

// k_take_copy behind the scan; BITS: the rows' sources are addresses of bits, and d_bodies is not looked at.
template <bool BITS>
static void launch_take_copy(hipStream_t stream, const void *d_bodies, const TakeRow *plan, const uint64_t *out_body_index, uint32_t n_rows, void *d_out, uint64_t cap) {
    // (what fits into cap spans no more than cap / TAKE_TILE_BYTES + 2 tiles, at any alignment)
    hipLaunchKernelGGL(k_take_copy<BITS>, dim3(capped(cap / TAKE_TILE_BYTES + 2, TAKE_GRID)), dim3(BB), 0, stream, static_cast<const uint8_t *>(d_bodies), plan, out_body_index,
                       n_rows, static_cast<uint8_t *>(d_out), cap);
}

void launch_take(hipStream_t stream, const PackedStore &store, const uint32_t *rows, uint32_t n_rows, void *d_out, uint64_t cap, uint64_t *out_body_index,
                 uint64_t *out_text_index, uint8_t *d_status, TakeRow *plan, const PackedReport &r) {
    hipLaunchKernelGGL(k_take_plan, dim3(plan_grid(n_rows)), dim3(BB), 0, stream, store, rows, n_rows, plan, d_status, r.stats);
    launch_take_scan(stream, plan, n_rows, out_body_index, out_text_index, r);
    if (d_out) launch_take_copy<false>(stream, store.bodies, plan, out_body_index, n_rows, d_out, cap);
}

// The slice's and the field's four launches: the two differ in their kernels and their job alone.
template <class Job, class PlanKernel, class LongKernel>
static void launch_cut(hipStream_t stream, PlanKernel plan_kernel, LongKernel long_kernel, const PackedStore &store, const uint2 *codes, uint32_t n_codes, const Job &job,
                       void *d_out, uint64_t cap, uint64_t *out_body_index, uint64_t *out_text_index, uint8_t *d_status, TakeRow *plan, uint32_t *long_list,
                       const PackedReport &r) {
    hipLaunchKernelGGL(plan_kernel, dim3(plan_grid(job.n_rows)), dim3(BB), 0, stream, store, codes, n_codes, job, plan, long_list, d_status, r.stats);
    hipLaunchKernelGGL(long_kernel, dim3(long_grid(job.n_rows)), dim3(BB), 0, stream, store, codes, n_codes, job, plan, static_cast<const uint32_t *>(long_list),
                       static_cast<const unsigned long long *>(r.stats));
    launch_take_scan(stream, plan, job.n_rows, out_body_index, out_text_index, r);
    if (d_out) launch_take_copy<true>(stream, nullptr, plan, out_body_index, job.n_rows, d_out, cap);
}

void launch_slice(hipStream_t stream, const PackedStore &store, const uint2 *codes, uint32_t n_codes, const SliceJob &job, void *d_out, uint64_t cap,
                  uint64_t *out_body_index, uint64_t *out_text_index, uint8_t *d_status, TakeRow *plan, uint32_t *long_list, const PackedReport &r) {
    launch_cut(stream, k_slice_plan, k_slice_long, store, codes, n_codes, job, d_out, cap, out_body_index, out_text_index, d_status, plan, long_list, r);
}

void launch_field(hipStream_t stream, const PackedStore &store, const uint2 *codes, uint32_t n_codes, const FieldJob &job, void *d_out, uint64_t cap,
                  uint64_t *out_body_index, uint64_t *out_text_index, uint8_t *d_status, TakeRow *plan, uint32_t *long_list, const PackedReport &r) {
    launch_cut(stream, k_field_plan, k_field_long, store, codes, n_codes, job, d_out, cap, out_body_index, out_text_index, d_status, plan, long_list, r);
}

void launch_concat(hipStream_t stream, const PackedStore &a, const PackedStore &b, const uint2 *codes, uint32_t n_codes, const ConcatJob &job, void *d_out, uint64_t cap,
                   uint64_t *out_body_index, uint64_t *out_text_index, uint8_t *d_status, TakeRow *plan, uint32_t *long_list, ConcatPiece *pieces, const PackedReport &r) {
    const uint32_t n_rows = job.n_rows;
    hipLaunchKernelGGL(k_concat_plan, dim3(plan_grid(n_rows)), dim3(BB), 0, stream, a, b, codes, n_codes, job, plan, pieces, long_list, d_status, r.stats);
    hipLaunchKernelGGL(k_concat_long, dim3(long_grid(n_rows)), dim3(BB), 0, stream, a, b, codes, n_codes, job, plan, pieces, static_cast<const uint32_t *>(long_list), d_status,
                       r.stats);
    launch_take_scan(stream, plan, n_rows, out_body_index, out_text_index, r);
    if (!d_out) return;
    hipLaunchKernelGGL(k_concat_copy, dim3(capped(cap / TAKE_TILE_BYTES + 2, TAKE_GRID)), dim3(BB), 0, stream, static_cast<const ConcatPiece *>(pieces), job.sep, job.sep_bits,
                       static_cast<const uint64_t *>(out_body_index), n_rows, static_cast<uint8_t *>(d_out), cap);
}

void launch_recode(hipStream_t stream, const PackedStore &store, const uint2 *codes, uint32_t n_codes, const RecodeJob &job, void *d_out, uint64_t cap,
                   uint64_t *out_body_index, uint64_t *out_text_index, uint8_t *d_status, TakeRow *plan, uint32_t *long_list, const PackedReport &r) {
    const uint32_t n_rows = job.n_rows, lanes = plan_grid(n_rows), groups = long_grid(n_rows);
    hipLaunchKernelGGL(k_recode_plan, dim3(lanes), dim3(BB), 0, stream, store, codes, n_codes, job, plan, long_list, d_status, r.stats);
    hipLaunchKernelGGL(k_recode_long, dim3(groups), dim3(BB), 0, stream, store, codes, n_codes, job, plan, static_cast<const uint32_t *>(long_list), d_status, r.stats);
    launch_take_scan(stream, plan, n_rows, out_body_index, out_text_index, r);
    if (!d_out) return;
    hipLaunchKernelGGL(k_recode_write, dim3(lanes), dim3(BB), 0, stream, store, codes, n_codes, job, static_cast<const TakeRow *>(plan),
                       static_cast<const uint64_t *>(out_body_index), static_cast<uint8_t *>(d_out), cap);
    hipLaunchKernelGGL(k_recode_write_long, dim3(groups), dim3(BB), 0, stream, store, codes, n_codes, job, static_cast<const TakeRow *>(plan),
                       static_cast<const uint32_t *>(long_list), static_cast<const unsigned long long *>(r.stats), static_cast<const uint64_t *>(out_body_index),
                       static_cast<uint8_t *>(d_out), cap);
}

void launch_number(hipStream_t stream, const PackedStore &store, const uint2 *codes, uint32_t n_codes, const NumberJob &job, uint8_t *d_status, NumberRow *rows,
                   uint32_t *long_list, const PackedReport &r) {
    const uint32_t n_rows = job.ask.n_rows, lanes = plan_grid(n_rows);
    if (job.d_min || job.d_max) hipLaunchKernelGGL(k_number_fill, dim3(plan_grid(job.n_groups)), dim3(BB), 0, stream, job.d_min, job.d_max, job.n_groups);
    hipLaunchKernelGGL(k_number_plan, dim3(lanes), dim3(BB), 0, stream, store, codes, n_codes, job, rows, long_list, d_status, r.stats);
    hipLaunchKernelGGL(k_number_long, dim3(long_grid(n_rows)), dim3(BB), 0, stream, store, codes, n_codes, job, rows, static_cast<const uint32_t *>(long_list),
                       static_cast<const unsigned long long *>(r.stats));
    const NumberRow *left = rows;
    if (job.d_sum || job.d_n || job.d_min || job.d_max) hipLaunchKernelGGL(k_number_fold<true>, dim3(lanes), dim3(BB), 0, stream, left, job, r);
    else hipLaunchKernelGGL(k_number_fold<false>, dim3(lanes), dim3(BB), 0, stream, left, job, r);
}

void launch_join(hipStream_t stream, const PackedStore &records, const PackedStore &keys, uint32_t flags, unsigned long long *table, uint64_t slots, uint32_t *d_rows,
                 uint64_t cap_rows, uint32_t *d_key_of_row, uint8_t *d_status, uint8_t *d_key_status, const TileWs &tiles, uint32_t *key_of, const PackedReport &r) {
    const uint32_t n_tiles = tiles_of(records.n), grid = capped(n_tiles, JOIN_GRID);
    if (keys.n) hipLaunchKernelGGL(k_join_build, dim3(capped(tiles_of(keys.n), JOIN_GRID)), dim3(BB), 0, stream, keys, table, slots - 1, d_key_status, r.stats);
    hipLaunchKernelGGL(k_join_flag, dim3(grid), dim3(BB), 0, stream, records, keys, static_cast<const unsigned long long *>(table), slots - 1, flags, tiles, key_of, d_status,
                       r.stats, r.host_result);
    launch_scan_emit(stream, n_tiles, grid, tiles, d_rows, cap_rows, key_of, d_key_of_row, r);
}

void launch_group(hipStream_t stream, const PackedStore &records, unsigned long long *table, uint64_t slots, uint32_t *d_first_rows, uint64_t cap_groups, uint32_t *d_count,
                  uint32_t *d_group_of, uint8_t *d_status, const TileWs &tiles, uint64_t *hash_of, uint32_t *rep_of, uint32_t *dense, const PackedReport &r) {
    const uint32_t n_tiles = tiles_of(records.n), grid = capped(n_tiles, JOIN_GRID);
    hipLaunchKernelGGL(k_group_build, dim3(grid), dim3(BB), 0, stream, records, table, slots - 1, hash_of, r.stats);
    hipLaunchKernelGGL(k_group_flag, dim3(grid), dim3(BB), 0, stream, records, static_cast<const unsigned long long *>(table), slots - 1, static_cast<const uint64_t *>(hash_of), tiles,
                       rep_of, d_status, r.stats);
    launch_scan<true>(stream, tiles.counts, n_tiles, tiles.base, r);
    if (!d_first_rows) return;
    const unsigned long long *masks = tiles.masks;
    const uint64_t *base = tiles.base;
    if (d_count) hipLaunchKernelGGL(k_group_emit<true>, dim3(grid), dim3(BB), 0, stream, masks, base, n_tiles, d_first_rows, cap_groups, d_count, dense);
    else hipLaunchKernelGGL(k_group_emit<false>, dim3(grid), dim3(BB), 0, stream, masks, base, n_tiles, d_first_rows, cap_groups, d_count, dense);
    if (!d_count && !d_group_of) return;
    const uint32_t *reps = rep_of, *numbers = dense;
    if (d_count) hipLaunchKernelGGL(k_group_number<true>, dim3(grid), dim3(BB), 0, stream, reps, numbers, base, n_tiles, records.n, cap_groups, d_group_of, d_count);
    else hipLaunchKernelGGL(k_group_number<false>, dim3(grid), dim3(BB), 0, stream, reps, numbers, base, n_tiles, records.n, cap_groups, d_group_of, d_count);
}

void launch_join_hash(hipStream_t stream, const PackedStore &records, uint64_t *d_hash) {
    hipLaunchKernelGGL(k_join_hash, dim3(capped(tiles_of(records.n), JOIN_GRID)), dim3(BB), 0, stream, records, d_hash);
}

void launch_match(hipStream_t stream, const PackedStore &store, const uint32_t *pattern, const MatchJob &job, uint32_t *d_rows, uint64_t cap_rows, uint8_t *d_status,
                  const TileWs &tiles, const PackedReport &r) {
    const uint32_t n_tiles = tiles_of(store.n), grid = capped(n_tiles, MATCH_GRID);
    hipLaunchKernelGGL(k_match_flag, dim3(grid), dim3(BB), 0, stream, store, pattern, job, tiles, d_status, r.stats);
    launch_scan_emit(stream, n_tiles, grid, tiles, d_rows, cap_rows, nullptr, nullptr, r);
}

void launch_order(hipStream_t stream, const PackedStore &store, const uint2 *codes, uint32_t n_codes, const uint32_t *pattern, const uint32_t *starts, const OrderJob &job,
                  uint32_t *d_rows, uint64_t cap_rows, uint8_t *d_status, const TileWs &tiles, const PackedReport &r) {
    const uint32_t n_tiles = tiles_of(store.n), grid = capped(n_tiles, MATCH_GRID);
    hipLaunchKernelGGL(k_order_flag, dim3(grid), dim3(BB), 0, stream, store, codes, n_codes, pattern, starts, job, tiles, d_status, r.stats);
    launch_scan_emit(stream, n_tiles, grid, tiles, d_rows, cap_rows, nullptr, nullptr, r);
}

void launch_search(hipStream_t stream, const PackedStore &store, const uint2 *codes, uint32_t n_codes, const uint32_t *pattern, const SearchJob &job, uint32_t *d_rows,
                   uint64_t cap_rows, uint32_t *d_pos, uint8_t *d_status, const TileWs &tiles, uint32_t *pos_of, uint32_t *long_list, const PackedReport &r) {
    const uint32_t n_tiles = tiles_of(store.n), grid = capped(n_tiles, SEARCH_GRID);
    hipLaunchKernelGGL(k_search_flag, dim3(grid), dim3(BB), 0, stream, store, codes, n_codes, pattern, job, tiles, pos_of, long_list, d_status, r.stats);
    if (!(job.flags & MATCH_F_NEVER))  // (nothing was listed)
        hipLaunchKernelGGL(k_search_long, dim3(capped(store.n, SHARED_DEC_GRID)), dim3(BB), 0, stream, store, codes, n_codes, pattern, job, tiles, pos_of,
                           static_cast<const uint32_t *>(long_list), static_cast<const unsigned long long *>(r.stats));
    launch_scan_emit(stream, n_tiles, grid, tiles, d_rows, cap_rows, pos_of, d_pos, r);
}

void launch_packed_encode(hipStream_t stream, const void *d_text, uint64_t text_bytes, const uint64_t *text_index, uint32_t n, void *d_out, uint64_t cap,
                          uint64_t *out_index, uint8_t *d_status, const uint2 *table, uint32_t *sizes, const PackedReport &r) {
    const uint8_t *text = static_cast<const uint8_t *>(d_text);
    hipLaunchKernelGGL(k_packed_count, dim3(batch_grid(n)), dim3(BB), 0, stream, text, text_bytes, text_index, n, table, sizes, d_status, r.stats);
    launch_scan<true>(stream, sizes, n, out_index, r);
    if (d_out)
        hipLaunchKernelGGL(k_packed_pack, dim3(capped(n, SHARED_ENC_GRID)), dim3(BB), 0, stream, text, text_bytes, text_index, n, static_cast<uint8_t *>(d_out), cap,
                           static_cast<const uint64_t *>(out_index), table);
}

void launch_packed_decode(hipStream_t stream, const PackedStore &store, void *d_out, uint64_t cap, const uint2 *codes, uint32_t n_codes, uint32_t *d_written,
                          uint8_t *d_status, const PackedReport &r, uint32_t *counter) {
    hipLaunchKernelGGL(k_packed_decode, dim3(capped(store.n, SHARED_DEC_GRID)), dim3(BB), 0, stream, store, static_cast<uint8_t *>(d_out), cap, codes, n_codes, d_written, d_status,
                       r, counter);
}

void launch_packed_gather(hipStream_t stream, const PackedStore &store, const uint32_t *rows, uint32_t n_rows, void *d_out, uint64_t cap, uint64_t *out_index,
                          const uint2 *codes, uint32_t n_codes, uint32_t *d_written, uint8_t *d_status, uint32_t *sizes, const PackedReport &r, uint32_t *counter) {
    hipLaunchKernelGGL(k_gather_plan, dim3(capped((n_rows + BB - 1) / BB, GATHER_PLAN_GRID)), dim3(BB), 0, stream, store, rows, n_rows, sizes, d_status, r.stats);
    if (!d_out) return launch_scan<true>(stream, sizes, n_rows, out_index, r);
    launch_scan<false>(stream, sizes, n_rows, out_index, r);
    hipLaunchKernelGGL(k_packed_gather, dim3(capped(n_rows, SHARED_DEC_GRID)), dim3(BB), 0, stream, store, rows, n_rows, static_cast<uint8_t *>(d_out), cap,
                       static_cast<const uint64_t *>(out_index), codes, n_codes, d_written, r, counter);
}

void launch_shared_encode(hipStream_t stream, const void *d_in, void *d_out, const SharedJob *jobs, uint32_t n, const uint2 *table,
                          uint2 *host_results, uint32_t *counter, unsigned long long *host_done, unsigned long long epoch) {
    hipLaunchKernelGGL(k_shared_encode, dim3(n < SHARED_ENC_GRID ? n : SHARED_ENC_GRID), dim3(BB), 0, stream, static_cast<const uint8_t *>(d_in), static_cast<uint8_t *>(d_out), jobs, n, table,
                       host_results, counter, host_done, epoch);
}

void launch_shared_decode(hipStream_t stream, const void *d_in, void *d_out, const SharedJob *jobs, uint32_t n, const uint2 *codes,
                          uint32_t n_codes, uint2 *host_results, uint32_t *counter, unsigned long long *host_done, unsigned long long epoch) {
    hipLaunchKernelGGL(k_shared_decode, dim3(n < SHARED_DEC_GRID ? n : SHARED_DEC_GRID), dim3(BB), 0, stream, static_cast<const uint8_t *>(d_in), static_cast<uint8_t *>(d_out), jobs, n, codes,
                       n_codes, host_results, counter, host_done, epoch);
}

void launch_batch_hist(hipStream_t stream, const void *d_in, const BatchSpan *spans, uint32_t n, uint32_t *host_hist, uint32_t *counter,
                       unsigned long long *host_done, unsigned long long epoch) {
    hipLaunchKernelGGL(k_batch_hist, dim3(batch_grid(n)), dim3(BB), 0, stream, static_cast<const uint8_t *>(d_in), spans, n, host_hist, counter, host_done, epoch);
}

void launch_batch_encode(hipStream_t stream, const void *d_in, void *d_out, const BatchEncJob *jobs, uint32_t n, const uint8_t *blob) {
    hipLaunchKernelGGL(k_batch_encode, dim3(batch_grid(n)), dim3(BB), 0, stream, static_cast<const uint8_t *>(d_in), static_cast<uint8_t *>(d_out), jobs, n, blob);
}

void launch_batch_heads(hipStream_t stream, const void *d_in, const BatchSpan *spans, uint32_t n, uint32_t *host_heads, uint32_t *counter,
                        unsigned long long *host_done, unsigned long long epoch) {
    hipLaunchKernelGGL(k_batch_heads, dim3(batch_grid(n)), dim3(BB), 0, stream, static_cast<const uint8_t *>(d_in), spans, n, host_heads, counter, host_done, epoch);
}

void launch_batch_decode(hipStream_t stream, const void *d_in, void *d_out, const BatchDecJob *jobs, uint32_t n, const uint8_t *blob,
                         uint32_t *host_totals, uint32_t *counter, unsigned long long *host_done, unsigned long long epoch) {
    hipLaunchKernelGGL(k_batch_decode, dim3(batch_grid(n)), dim3(BB), 0, stream, static_cast<const uint8_t *>(d_in), static_cast<uint8_t *>(d_out), jobs, n, blob,
                       host_totals, counter, host_done, epoch);
}

}  // namespace et
