// et_tables.h -- formats of the decode lookup tables and their host-side builders.
// No HIP in here: et_tables.cpp also compiles with plain g++ (tests/test_sanitizers.py
// runs the builders under AddressSanitizer/UBSan against a brute-force decoder).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "entreepy_hip.h"

namespace et {

constexpr uint32_t DEC_LUT_BITS_MAX = 12;    // older-format first-level table: at most 4096 x u32
constexpr uint32_t DEC_LUT_BITS_WRITE = 11;  // index width of the write kernels' tables: measured 10 / 11 / 12 -> 0.65 / 0.60 / 0.68 ms at 1 GiB
// Older format (LDS-window kernels k_dec_sync / k_dec_write / k_dec_maps / k_dec_resolve, and
// the slow path of the step walks).  First-level entry (u32), indexed by the next lut_bits
// bits: bytes 0..2 = up to three symbols whose codes all fit in the index, bits 24..27 = total
// length of those codes, bits 28..29 = how many (0: the first code is longer than the table,
// or no code starts here).  Escape entries (count 0): bit 30 set -> byte 0 is the index of a
// second-level table of 1 << sub_bits u16 entries ((len << 8) | sym, 0 = not here) indexed
// by the sub_bits bits that follow the first lut_bits.  longc: {left-aligned code, (len << 8)
// | sym} of every code longer than lut_bits.
constexpr uint32_t LUT_LEN_SHIFT = 24, LUT_N_SHIFT = 28, LUT_SUB_SHIFT = 30;
constexpr uint32_t DEC_WRITE_SYMS = 2;  // symbols per entry: k_dec_write stores at most two per step
constexpr uint32_t DEC_SUB_BITS_MAX = 8, DEC_SUB_TABLES_MAX = 16;

// Step table of k_dec_sync_reg / k_dec_sync_reg2 (no symbols, only how far a lookup moves the
// walk).  The walk state X is one u32: bits 0..15 = G, the position relative to the current
// register pair (et_kernels_fallback.hip walk_steps), bits 16..27 = symbols begun, bits 28..31 junk;
// entry = (len_first << 28) + (n << 16) - len_total is simply ADDED to X (n = all the whole
// codes inside the index, len_first = length of the first one for single steps).  No code
// inside the index: STEP_ESCAPE = one "symbol" of STEP_ESCAPE_BITS bits, which throws the
// lane out of the word loop it is in; the loop's exit test sees how far it flew and resolves
// the long code: bits 28..31 of the escape entry = 1 + the second-level table (entries
// (1 << 16) - len, 0 = not here) indexed by the step_sub_bits bits after the index, 0 = no
// table (older-format tables in global memory, slow).
constexpr uint32_t DEC_STEP_BITS_MAX = 13, DEC_STEP_BITS_DEFAULT = 12;
constexpr uint32_t STEP_ESCAPE_BITS = 64, STEP_ESCAPE = (1u << 16) - STEP_ESCAPE_BITS;
// k_dec_write_reg's table has the same shape with symbols: state X = (stage address << 10) |
// G; entry = sym2 << 24 | sym1 << 16 | u16((n << 10) - len_total), n <= 2, whose low half
// is added to X; escape = WSTEP_ESCAPE in the low half, 1 + second-level table in bits
// 24..31; second-level entries sym << 16 | ((1 << 10) - len), 0 = not here.
constexpr uint32_t WSTEP_ESCAPE = (1u << 10) - STEP_ESCAPE_BITS;
constexpr uint32_t DEC_STEP_SUB_WORDS = 1024;  // second-level entries, all tables of one step table together

// A nearly fixed-length code -- codewords of L and L + 1 bits only, more than two of them -- has little to re-synchronise on: the one
// rule behind "go the exhaustive way at once" on one GPU (et_decode.cpp plan_decode, which then looks closer) and across ranks
// (et_shard_seq.cpp cold_plan).
inline bool nearly_fixed_length(const et_codebook *cb) { return cb->n_coded > 2 && cb->max_length <= cb->min_length + 1; }

struct HostDecodeTables {
    uint32_t lut_bits, n_long, sub_bits, n_sub;
};

// What the HOST decides about a code table's decode tables -- index widths, which long codes get
// which second-level table, the order of the long list -- handed to the device, which fills the
// tables themselves (et_kernels_fallback.hip k_build_dec_tables: same entries as the builders below, which
// stay as the reference the device's output is tested against, and as ET_DEC_TABLES_HOST=1).
struct TablePlan {
    uint32_t data[256];
    uint8_t length[256];
    uint8_t lut_sub[256];    // symbol longer than lut_bits: 1 + its second-level table in the older format (0: none)
    uint8_t step_sub[256];   // ... in the step table
    uint8_t wstep_sub[256];  // ... in the write-step table
    uint8_t long_idx[256];   // ... its position in the long list
    uint32_t lut_bits, n_long, sub_bits, n_sub, max_syms;
    uint32_t step_bits, step_sub_bits, n_step_sub;
    uint32_t wstep_bits, wstep_sub_bits, n_wstep_sub;
    uint32_t pad_;
};
void plan_tables(const et_codebook *cb, uint32_t lut_bits_max, uint32_t max_syms, uint32_t step_bits_max, uint32_t wstep_bits_max, TablePlan *plan);

// The decode tables as the kernels take them: pointers into the device's table block (DecTableLayout below).
struct DecodeTables {
    const uint32_t *lut;     // [1 << lut_bits] first-level entries (LUT_* above)
    const uint32_t *longc;   // [n_long * 2]: {left-aligned code, (len << 8) | sym} of every code longer than lut_bits
    const uint16_t *sub;     // [n_sub << sub_bits] second-level tables
    const uint8_t *sym_len;  // [256] code length per symbol (single-symbol steps)
    uint32_t lut_bits;
    uint32_t n_long;
    uint32_t sub_bits;
    uint32_t n_sub;
    const uint32_t *steps;   // [1 << step_bits] packed walk increments for k_dec_sync_reg (STEP_* above), or null;
                             // followed by n_step_sub second-level tables of 1 << step_sub_bits entries
    uint32_t step_bits;
    uint32_t step_sub_bits;
    uint32_t n_step_sub;
    const DecodeTables *dev_copy;  // this struct in device memory (slow path of the step walks), or null
};

// Bytes a step table of this shape takes in the block: index and second level, rounded up to 16.
inline size_t step_table_bytes(uint32_t bits, uint32_t sub_bits, uint32_t n_sub) {
    return (((static_cast<size_t>(1) << bits) + (static_cast<size_t>(n_sub) << sub_bits) + 3) & ~static_cast<size_t>(3)) * sizeof(uint32_t);
}

// The block all decode tables of a code lie in -- one in device memory, two in pinned host memory filled in turn -- described
// once: offsets and capacities in bytes.  ONE set of older-format tables (index DEC_LUT_BITS_WRITE, DEC_WRITE_SYMS symbols per
// entry), the code lengths right behind its second level, then the step table (k_dec_sync_reg: index DEC_STEP_BITS_DEFAULT).
// From there on the block is packed, so that one upload covers what is in use and no more: the write-step table
// (k_dec_write_reg) step_table_bytes behind STEPS, the two DecodeTables structs (the sweeps' and the write's: dev_copy) behind
// its step_table_bytes, and the TablePlan of device-built tables behind them.
struct DecTableLayout {
    static constexpr size_t LUT = 0, LUT_BYTES = sizeof(uint32_t) << DEC_LUT_BITS_MAX;
    static constexpr size_t LONG = LUT + LUT_BYTES, LONG_BYTES = 256 * 2 * sizeof(uint32_t);  // every symbol a long code
    static constexpr size_t SUB = LONG + LONG_BYTES, SUB_BYTES = (static_cast<size_t>(DEC_SUB_TABLES_MAX) << DEC_SUB_BITS_MAX) * sizeof(uint16_t) + 64;
    static constexpr size_t SYM_LEN = SUB + SUB_BYTES, SYM_LEN_BYTES = 256;
    static constexpr size_t STEPS = SYM_LEN + SYM_LEN_BYTES;
    static constexpr size_t STEPS_BYTES = (sizeof(uint32_t) << DEC_STEP_BITS_MAX) + (DEC_STEP_SUB_WORDS + 4) * sizeof(uint32_t);
    static constexpr size_t WSTEPS_BYTES = (sizeof(uint32_t) << DEC_LUT_BITS_MAX) + (DEC_STEP_SUB_WORDS + 4) * sizeof(uint32_t);
    static constexpr size_t TAIL_BYTES = 2 * sizeof(DecodeTables) + sizeof(TablePlan);
    static constexpr size_t BYTES = STEPS + STEPS_BYTES + WSTEPS_BYTES + TAIL_BYTES + 64;  // + slack for 16-byte rounded copies
};
// The kernels stage these tables with wide loads.
static_assert(DecTableLayout::LUT % 64 == 0 && DecTableLayout::LONG % 64 == 0 && DecTableLayout::SUB % 64 == 0 && DecTableLayout::SYM_LEN % 64 == 0 &&
                  DecTableLayout::STEPS % 64 == 0,
              "every decode table begins at a multiple of 64 bytes");
static_assert(DEC_LUT_BITS_WRITE <= DEC_LUT_BITS_MAX && DEC_STEP_BITS_DEFAULT <= DEC_STEP_BITS_MAX, "the index widths in use fit their tables");

// The table (or struct) at `offset` of a block, in host or in device memory.
template <typename T>
T *table_at(uint8_t *block, size_t offset) { return reinterpret_cast<T *>(block + offset); }

// Older-format tables: lut[1 << k], longc[2 * n_long], sub[n_sub << sub_bits]; k =
// min(longest code, lut_bits_max).
void build_decode_tables(const et_codebook *cb, uint32_t lut_bits_max, uint32_t max_syms, uint32_t *lut, uint32_t *longc, uint16_t *sub,
                         HostDecodeTables *out);
// Step tables: steps[1 << k] followed by *n_sub second-level tables of 1 << *sub_bits
// entries (at most DEC_STEP_SUB_WORDS in all).  Return k = min(longest code, bits_max).
uint32_t build_step_table(const et_codebook *cb, uint32_t bits_max, uint32_t *steps, uint32_t *sub_bits, uint32_t *n_sub);
uint32_t build_write_step_table(const et_codebook *cb, uint32_t bits_max, uint32_t *steps, uint32_t *sub_bits, uint32_t *n_sub);

}  // namespace et
