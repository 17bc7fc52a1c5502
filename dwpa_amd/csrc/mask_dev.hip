// mask_dev.hip -- k_prep_mask: hashcat -a 3 mask keyspace generated in-kernel -> HMAC key midstates (mask.hpp has the
// language, the order and the table layout).
//
// The mask numeral and the key block it leaves in registers are mask_key_block (mask_dev.hpp, shared with
// k_prep_hybrid): lane i adds i to the digits of `first` that travel in the kernel arguments.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crypto_dev.hpp"
#include "prep_dev.hpp"
#include "kernels.hpp"
#include "mask.hpp"
#include "mask_dev.hpp"

namespace dwpa {

__global__ __launch_bounds__(256) void k_prep_mask(MaskDigits base, uint64_t first, uint32_t count, uint32_t npos,
                                                   const uint8_t* __restrict__ table, uint32_t* __restrict__ mid,
                                                   uint64_t* __restrict__ ids, uint32_t* __restrict__ counter,
                                                   uint32_t cap) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) counter[0] = count;  // the loaded-slot count the PBKDF2 and verify kernels read: no host copy
    if (i >= count || i >= cap) return;
    uint32_t kb[16];
    mask_key_block(base, i, npos, table, kb);
    store_mid(mid, cap, i, kb);
    ids[i] = first + i;
}

hipError_t launch_prep_mask(const uint8_t digits[64], uint64_t first, uint32_t count, uint32_t npos,
                            const uint8_t* table, uint32_t* mid, uint64_t* ids, uint32_t* counter, uint32_t cap,
                            hipStream_t s) {
    const MaskDigits base = mask_digits_pack(digits);
    const uint32_t blocks = count ? (count + 255u) / 256u : 1u;  // count 0: one block, for the counter
    hipLaunchKernelGGL(k_prep_mask, dim3(blocks), dim3(256), 0, s, base, first, count, npos, table, mid, ids, counter,
                       cap);
    return hipGetLastError();
}

}  // namespace dwpa
