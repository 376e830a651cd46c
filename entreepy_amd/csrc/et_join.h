// et_join.h -- what the host and the device must agree on about the join call's hash table (et_join_packed_device): the 64-bit hash
// of a packed record (length, body byte count, body bytes) and the size of the table.  HIP-free: et_batch.hip includes it with
// ET_JOIN_FN set to its device attributes, et_batch.cpp as it stands (et_join_hash, et_join_table_slots).
//
// The hash is defined over the body's 8-byte little-endian words, the last one zero-extended:
//   word i   = bytes [8 i, 8 i + 8) of the body, byte k of them at bits 8 k .. 8 k + 7
//   term i   = mix(word i + (i + 1) * ET_JOIN_STEP)                 -- the word's position enters its term
//   sum      = term 0 + term 1 + ... (mod 2^64)                     -- commutative: any division of the words among lanes gives it
//   hash     = mix(sum + mix(length * ET_JOIN_STEP + n_bytes))
// with mix the finaliser of splitmix64.  A body of no bytes has no words: its hash is that of (length, 0) alone.  The hash picks a
// slot and its upper half is the slot's tag; it never decides alone -- every hit is confirmed by length, byte count and bytes.
// That sentence is held by the collide_* fixtures of tests/test_gpu_join.py and tests/test_gpu_group.py: mix is a bijection and the
// sum is plain, so tests/hashcraft.py solves a body's last word for any wanted hash, and the fixtures hold DIFFERENT texts with one
// tag and one home slot, with one whole 64-bit hash, with one hash under other lengths and byte counts, and with one hash and equal
// first 512 bytes -- a confirmation that looks at less merges them (tests/test_join_host.py shows which fixture catches what).
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifndef ET_JOIN_FN
#define ET_JOIN_FN inline
#endif

namespace et {

constexpr uint64_t ET_JOIN_STEP = 0x9E3779B97F4A7C15ull;
constexpr uint64_t ET_JOIN_EMPTY = ~0ull;                 // a slot nobody took; a taken one is tag << 32 | key number, key number < 2^24
constexpr size_t ET_JOIN_KEYS_MAX = size_t(1) << 24;      // most keys per call
constexpr size_t ET_JOIN_SLOTS_MIN = 256;                 // the smallest table

ET_JOIN_FN uint64_t et_join_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

ET_JOIN_FN uint64_t et_join_term(uint64_t i, uint64_t word) { return et_join_mix(word + (i + 1) * ET_JOIN_STEP); }

ET_JOIN_FN uint64_t et_join_finish(uint64_t sum, uint64_t n_bytes, uint64_t length) { return et_join_mix(sum + et_join_mix(length * ET_JOIN_STEP + n_bytes)); }

// Slots of the table for n_keys keys: a power of two, at least 2 * n_keys and at least ET_JOIN_SLOTS_MIN.  The load of at most 1/2
// is what the probe loops rest on: with a free slot for every taken one, every probe sequence meets an empty slot.
ET_JOIN_FN size_t et_join_slots_for(size_t n_keys) {
    size_t slots = ET_JOIN_SLOTS_MIN;
    while (slots < 2 * n_keys) slots <<= 1;
    return slots;
}

}  // namespace et
