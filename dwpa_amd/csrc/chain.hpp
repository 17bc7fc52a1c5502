// chain.hpp -- the chain attack's host arithmetic (no HIP): a chain is 1..4 parts, each a word list or a mask,
// concatenated left to right.  Candidate i is the mixed-radix numeral of i over the parts' radices (a list's word
// count, a mask's keyspace) with the LAST part fastest -- itertools.product order; a mask part's own index is in
// mask.hpp's order.  The C entry points dwpa_chain_keyspace / dwpa_chain_split are in chain.cpp.
#pragma once
#include <stdint.h>

#include "dwpa22000.h"

namespace dwpa {

constexpr uint32_t CHAIN_MAX_PARTS = DWPA_CHAIN_MAX_PARTS;

// K = the product of radix[0..nparts).  DWPA_E_ARG: nparts outside 1..4, or K above 2^64 - 1.  A radix of 0 gives
// K = 0 whatever the others are.
int chain_keyspace(const uint64_t* radix, uint32_t nparts, uint64_t* keyspace);
// digits[p] = digit of `index` at part p (last part fastest).  DWPA_E_ARG: as chain_keyspace, or index >= K.
int chain_split(const uint64_t* radix, uint32_t nparts, uint64_t index, uint64_t* digits);

}  // namespace dwpa
