// markov.hpp -- Markov-ordered mask attack, host side (no HIP): the model, its file, the trainer, the thresholded
// keyspace, candidate i, and the device table image k_prep_markov reads (internal to libdwpa22000.so; the C entry
// points dwpa_markov_train / dwpa_markov_load / dwpa_mask_keyspace_markov / dwpa_mask_candidate_markov are in
// markov.cpp).
//
// Model: position-dependent, first order, over bytes, positions 0..62.  n[p][a][b] = training words whose byte at
// position p is b and whose byte at p - 1 is a; the predecessor of position 0 is byte 0.  order[p][a] = the 256 byte
// values by n[p][a][b] descending, ties by byte value ascending.  The file holds the ranking, not the counts:
//   "DWPAMKV1", u32 LE positions (63), u32 LE 0, then order as 63 x 256 rows of 256 bytes: 4,128,784 bytes.
//
// Order (the project's own; hashcat's statistics file is not read, so index parity with hashcat stays unpinned): for
// the mask's sets S_p (sizes n_p) and a threshold t (0: none), r_p = n_p (t = 0) or min(n_p, t), K = the product of
// the r_p.  Candidate i: the digits d_p of i over the radices r_p, last position fastest; c_0 = row(0, 0)[d_0], c_p =
// row(p, c_{p-1})[d_p], where row(p, a) = order[p][a] filtered to the members of S_p, its first r_p entries.  A literal
// is a position of radix 1: its own byte, and the predecessor of the next position.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "dwpa22000.h"
#include "mask.hpp"

namespace dwpa {

constexpr uint32_t MARKOV_POS = MASK_MAX_POS;
constexpr size_t MARKOV_HEADER = 16;
constexpr size_t MARKOV_FILE_BYTES = MARKOV_HEADER + (size_t)MARKOV_POS * 256 * 256;

// 0, or DWPA_E_ARG: another size, another header, a row that is not a permutation of 0..255.
int markov_validate(const uint8_t* model, size_t len);
// order[p][a] of a validated image
inline const uint8_t* markov_row(const uint8_t* model, uint32_t p, uint32_t a) {
    return model + MARKOV_HEADER + ((size_t)p * 256 + a) * 256;
}
// The file at `path`, validated: 0, DWPA_E_IO (unreadable) or DWPA_E_ARG.
int markov_read_file(const char* path, std::vector<uint8_t>* out);

// A mask under a threshold.  About 16 KiB, as a Mask: kept on the heap.
struct MarkovMask {
    uint32_t npos = 0;
    uint64_t keyspace = 0;           // product of the radices, <= 2^64 - 1
    uint32_t radix[MARKOV_POS];      // r_p
    uint8_t member[MARKOV_POS][256];  // 1: the byte is in S_p
};
// sets: mask_parse_sets' result.  DWPA_E_ARG: threshold > 256, K above 2^64 - 1.
int markov_mask(const Mask& sets, uint32_t threshold, MarkovMask* out);
// The first n positions (1 <= n <= npos).
void markov_prefix(const MarkovMask& mm, uint32_t n, MarkovMask* out);
// digits[p] = digit of `index` at position p (last position fastest); 0 beyond npos.
void markov_digits(const MarkovMask& mm, uint64_t index, uint8_t digits[64]);
// Candidate `index` (< keyspace) into out[0..npos); model: a validated image.
void markov_candidate(const MarkovMask& mm, const uint8_t* model, uint64_t index, uint8_t* out);

// Device table (one upload per set call), markov_table_bytes(npos) <= 4 MiB + 256 B:
//   u32 radix[64]               r_p; 0 for p >= npos
//   u8  next[npos][256][256]    next[p][a][d] = row(p, a)[d] for d < r_p and every predecessor a that can occur at p
//                               (position 0: a = 0 only); 0 elsewhere
constexpr size_t MARKOV_TABLE_NEXT = 64 * sizeof(uint32_t);
inline size_t markov_table_bytes(uint32_t npos) { return MARKOV_TABLE_NEXT + (size_t)npos * 256 * 256; }
void markov_table(const MarkovMask& mm, const uint8_t* model, uint8_t* table /* zeroed, markov_table_bytes(npos) */);

}  // namespace dwpa
