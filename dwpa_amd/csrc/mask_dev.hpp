// mask_dev.hpp -- the mask numeral in registers, shared by k_prep_mask (mask_dev.hip) and k_prep_hybrid
// (hybrid_dev.hip); mask.hpp has the language, the order and the table layout.
//
// Candidate first + add is the mixed-radix numeral of that index, last position fastest.  The host decomposes `first`
// once per load into one digit per position and passes the 64 digits by value in the kernel arguments (no upload, no
// synchronisation); a lane adds its offset to that numeral: one 32-bit divide per position, carry upwards.  The sum
// never leaves 32 bits: the carry is split as q * r + rem before the digit is added, and digit + rem < 2r <= 512.
// Exact for every 64-bit index, since first + count <= keyspace is checked on the host and the carry out of position
// 0 is 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mask.hpp"

namespace dwpa {

struct MaskDigits {
    uint32_t w[16];  // digit of `first` at position p: byte p & 3 (little-endian) of w[p >> 2]
};

inline MaskDigits mask_digits_pack(const uint8_t digits[64]) {
    MaskDigits base;
    for (int j = 0; j < 16; j++)
        base.w[j] = (uint32_t)digits[4 * j] | (uint32_t)digits[4 * j + 1] << 8 | (uint32_t)digits[4 * j + 2] << 16 |
                    (uint32_t)digits[4 * j + 3] << 24;
    return base;
}

// kb = the bytes of candidate (base + add) at byte positions 0..npos-1 of a big-endian 16-word block, zero beyond.
// The position loop is fully unrolled, so every word index and byte shift is a compile-time constant (positions
// >= npos are skipped by a wave-uniform branch) and kb stays in registers.  The radices are wave-uniform loads; the
// set byte of each position is one byte load from the 16 KiB table, which stays in L2 / the vector cache for the
// whole launch.
__device__ __forceinline__ void mask_key_block(const MaskDigits& base, uint32_t add, uint32_t npos,
                                               const uint8_t* __restrict__ table, uint32_t kb[16]) {
    const uint32_t* __restrict__ radix = (const uint32_t*)table;
    const uint8_t* __restrict__ sets = table + MASK_TABLE_SETS;
#pragma unroll
    for (int j = 0; j < 16; j++) kb[j] = 0;
    uint32_t carry = add;
#pragma unroll
    for (int p = (int)MASK_MAX_POS - 1; p >= 0; p--) {
        if ((uint32_t)p < npos) {
            const uint32_t r = radix[p];
            const uint32_t digit = (base.w[p >> 2] >> (8 * (p & 3))) & 0xffu;
            uint32_t q = carry / r;
            uint32_t t = digit + (carry - q * r);
            if (t >= r) {
                t -= r;
                q++;
            }
            carry = q;
            kb[p >> 2] |= (uint32_t)sets[p * 256 + (t & 255u)] << (24 - 8 * (p & 3));
        }
    }
}

}  // namespace dwpa
