// mask.hpp -- hashcat -a 3 mask language (host only, no HIP): parser, keyspace, candidate i, and the device table
// image k_prep_mask reads (internal to libdwpa22000.so; the C entry points dwpa_mask_keyspace / dwpa_mask_candidate
// are in mask.cpp).
//
// Language: ?l a-z, ?u A-Z, ?d 0-9, ?h 0-9a-f, ?H 0-9A-F, ?s the 33 ASCII specials in byte order, ?a = ?l?u?d?s,
// ?b 0x00-0xff, ?? a literal '?', ?1..?4 the caller's custom sets, any other byte a literal (a position of radix 1).
// A custom set is raw bytes in the same language: built-in references, references to lower-numbered custom sets, ??
// and literal bytes; duplicate bytes are dropped (first occurrence kept), as hashcat does.
//
// Order (the project's own; hashcat's Markov order differs, the candidate set is the same): candidate i is the
// mixed-radix numeral of i over the positions' radices with the LAST position fastest -- itertools.product order,
// and ?d x N at index v is the zero-padded decimal v.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dwpa22000.h"

namespace dwpa {

constexpr uint32_t MASK_MAX_POS = 63;  // m22000's longest PSK

struct MaskPos {
    uint32_t radix;      // 1..256
    uint8_t bytes[256];  // the set in order; bytes[radix..] are 0
};

// No heap: a Mask lives on the caller's stack or inside a scan (16 KiB).
struct Mask {
    uint32_t npos = 0;
    uint64_t keyspace = 0;  // product of the radices, <= 2^64 - 1
    MaskPos pos[MASK_MAX_POS];
};

// Parses mask[0..len) with custom[0..4) (ptr == NULL: undefined; nullable array = none defined).  Returns 0 or
// DWPA_E_ARG: ?x with an unknown letter, a trailing lone '?', a reference to an undefined or (inside a custom set)
// not lower-numbered custom set, an empty set, no position or more than 63, a keyspace above 2^64 - 1.  Every defined
// custom set is expanded, referenced or not (hashcat parses -1..-4 at start-up).
int mask_parse(const char* mask, size_t len, const dwpa_bytes* custom, Mask* out);
// The same without the keyspace test: the positions' sets alone, keyspace left 0 (markov.hpp cuts the sets down by a
// threshold before it multiplies them).
int mask_parse_sets(const char* mask, size_t len, const dwpa_bytes* custom, Mask* out);
// The first n positions of m as a mask of their own (1 <= n <= m.npos; the product of fewer radices cannot overflow).
void mask_prefix(const Mask& m, uint32_t n, Mask* out);
// Candidate `index` (< keyspace) into out[0..npos).
void mask_candidate(const Mask& m, uint64_t index, uint8_t* out);
// digits[p] = digit of `index` at position p (last position fastest), for p < npos; 0 beyond.
void mask_digits(const Mask& m, uint64_t index, uint8_t digits[64]);

// Device table (one upload per set_mask), MASK_TABLE_BYTES = 16 KiB:
//   u32 radix[64]        radix of position p (1..256); 0 for p >= npos
//   u8  sets[63][256]    set bytes of position p at sets[p * 256 ..]
constexpr size_t MASK_TABLE_SETS = 64 * sizeof(uint32_t);
constexpr size_t MASK_TABLE_BYTES = MASK_TABLE_SETS + (size_t)MASK_MAX_POS * 256;
void mask_table(const Mask& m, uint8_t* table /* MASK_TABLE_BYTES */);

}  // namespace dwpa
