// mask_dev.hip -- k_prep_mask: hashcat -a 3 mask keyspace generated in-kernel -> HMAC key midstates (mask.hpp has the
// language, the order and the table layout).
//
// Candidate first + i is the mixed-radix numeral of that index, last position fastest.  The host decomposes `first`
// once per load into one digit per position and passes the 64 digits by value in the kernel arguments (no upload, no
// synchronisation); lane i adds i to that numeral: one 32-bit divide per position, carry upwards.  The sum never
// leaves 32 bits: the carry is split as q * r + rem before the digit is added, and digit + rem < 2r <= 512.  Exact for
// every 64-bit index, since first + count <= keyspace is checked on the host and the carry out of position 0 is 0.
//
// The 16-word key block is built in registers: the position loop is fully unrolled, so every word index and byte
// shift is a compile-time constant (positions >= npos are skipped by a wave-uniform branch).  The radices are
// wave-uniform loads; the set byte of each position is one byte load from the 16 KiB table, which stays in L2 / the
// vector cache for the whole launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crypto_dev.hpp"
#include "prep_dev.hpp"
#include "kernels.hpp"
#include "mask.hpp"

namespace dwpa {

struct MaskDigits {
    uint32_t w[16];  // digit of `first` at position p: byte p & 3 (little-endian) of w[p >> 2]
};

__global__ __launch_bounds__(256) void k_prep_mask(MaskDigits base, uint64_t first, uint32_t count, uint32_t npos,
                                                   const uint8_t* __restrict__ table, uint32_t* __restrict__ mid,
                                                   uint64_t* __restrict__ ids, uint32_t* __restrict__ counter,
                                                   uint32_t cap) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) counter[0] = count;  // the loaded-slot count the PBKDF2 and verify kernels read: no host copy
    if (i >= count || i >= cap) return;
    const uint32_t* __restrict__ radix = (const uint32_t*)table;
    const uint8_t* __restrict__ sets = table + MASK_TABLE_SETS;
    uint32_t kb[16];
#pragma unroll
    for (int j = 0; j < 16; j++) kb[j] = 0;
    uint32_t carry = i;
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
    store_mid(mid, cap, i, kb);
    ids[i] = first + i;
}

hipError_t launch_prep_mask(const uint8_t digits[64], uint64_t first, uint32_t count, uint32_t npos,
                            const uint8_t* table, uint32_t* mid, uint64_t* ids, uint32_t* counter, uint32_t cap,
                            hipStream_t s) {
    MaskDigits base;
    for (int j = 0; j < 16; j++)
        base.w[j] = (uint32_t)digits[4 * j] | (uint32_t)digits[4 * j + 1] << 8 | (uint32_t)digits[4 * j + 2] << 16 |
                    (uint32_t)digits[4 * j + 3] << 24;
    const uint32_t blocks = count ? (count + 255u) / 256u : 1u;  // count 0: one block, for the counter
    hipLaunchKernelGGL(k_prep_mask, dim3(blocks), dim3(256), 0, s, base, first, count, npos, table, mid, ids, counter,
                       cap);
    return hipGetLastError();
}

}  // namespace dwpa
