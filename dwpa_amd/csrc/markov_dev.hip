// markov_dev.hip -- k_prep_markov: the Markov-ordered mask keyspace generated in-kernel -> HMAC key midstates
// (markov.hpp has the model, the order and the table layout).
//
// A position's byte depends on the byte before it, so a lane makes two passes over the positions, both fully unrolled
// with the wave-uniform p < npos guard (every register index and shift is a compile-time constant):
//   1. last position first: the digits of first + lane, with mask_key_block's 32-bit carry arithmetic (mask_dev.hpp:
//      one 32-bit divide per position, digit + remainder < 2r <= 512), kept packed four to a register;
//   2. first position first: one byte load next[p][prev][digit] per position, or'ed into the big-endian key block;
//      the loaded byte is the next position's predecessor.
// The table (at most 4 MiB + 256 B) stays in global memory: the rows a launch touches are few, and the loads of one
// lane depend on each other, so only occupancy hides them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crypto_dev.hpp"
#include "prep_dev.hpp"
#include "kernels.hpp"
#include "markov.hpp"
#include "mask_dev.hpp"

namespace dwpa {

// 80 SGPRs: left alone the compiler loads all 63 radices ahead (106 SGPRs) and a SIMD then admits 7 waves, not 8.
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80))) void k_prep_markov(
    MaskDigits base, uint64_t first, uint32_t count, uint32_t npos, const uint8_t* __restrict__ table,
    uint32_t* __restrict__ mid, uint64_t* __restrict__ ids, uint32_t* __restrict__ counter, uint32_t cap) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) counter[0] = count;  // the loaded-slot count the PBKDF2 and verify kernels read: no host copy
    if (i >= count || i >= cap) return;
    const uint32_t* __restrict__ radix = (const uint32_t*)table;
    const uint8_t* __restrict__ next = table + MARKOV_TABLE_NEXT;
    uint32_t dg[16], kb[16];
#pragma unroll
    for (int j = 0; j < 16; j++) dg[j] = kb[j] = 0;
    uint32_t carry = i;
#pragma unroll
    for (int p = (int)MARKOV_POS - 1; p >= 0; p--) {
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
            dg[p >> 2] |= (t & 255u) << (8 * (p & 3));
        }
    }
    uint32_t prev = 0;  // unsigned: a predecessor >= 0x80 must not sign-extend into the address
#pragma unroll
    for (int p = 0; p < (int)MARKOV_POS; p++) {
        if ((uint32_t)p < npos) {
            const uint32_t d = (dg[p >> 2] >> (8 * (p & 3))) & 0xffu;
            prev = next[((uint32_t)p * 256u + prev) * 256u + d];
            kb[p >> 2] |= prev << (24 - 8 * (p & 3));
        }
    }
    store_mid(mid, cap, i, kb);
    ids[i] = first + i;
}

hipError_t launch_prep_markov(const uint8_t digits[64], uint64_t first, uint32_t count, uint32_t npos,
                              const uint8_t* table, uint32_t* mid, uint64_t* ids, uint32_t* counter, uint32_t cap,
                              hipStream_t s) {
    const MaskDigits base = mask_digits_pack(digits);
    const uint32_t blocks = count ? (count + 255u) / 256u : 1u;  // count 0: one block, for the counter
    hipLaunchKernelGGL(k_prep_markov, dim3(blocks), dim3(256), 0, s, base, first, count, npos, table, mid, ids,
                       counter, cap);
    return hipGetLastError();
}

}  // namespace dwpa
