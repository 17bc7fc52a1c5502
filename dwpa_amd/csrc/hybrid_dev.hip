// hybrid_dev.hip -- k_prep_hybrid: hashcat -a 6 (word || mask) and -a 7 (mask || word) -> HMAC key midstates.
//
// One lane per (word w, mask offset j) of a load of nwords x mask_count raw candidates, word-major: w = t / mask_count,
// j = t % mask_count (one 32-bit divide: the launch has fewer than 2^32 lanes).  The word comes from the dictionary
// in HBM (offsets[] / bytes[], as k_prep_dict reads it) through load_key_block; the mask candidate mask_first + j is
// built in registers by mask_key_block (mask_dev.hpp), the carry-add k_prep_mask uses.  Both halves are 16-word
// big-endian blocks that start at byte 0; the second half is moved behind the first by shift_right_bytes and the two
// are ORed:
//   mode 6: kb = word_block | shift_right_bytes(mask_block, L)    L per lane
//   mode 7: kb = mask_block | shift_right_bytes(word_block, P)    P wave-uniform
// A word is kept iff L <= 63 and minlen <= L + P <= maxlen (maxlen <= 64 here: the launcher clamps it, one key
// block holds 64 bytes); all mask_count lanes of a word share that decision.  Kept lanes take compacted slots
// (one atomic per wave, lane order inside the wave), so dropped words leave no holes and ids[slot] carries
// (first_word + w) * K + mask_first + j.  The counter ends as the raw kept count, which may exceed cap in a fill-mode
// load (lanes beyond cap store nothing), exactly as k_prep_dict's compact mode leaves it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crypto_dev.hpp"
#include "prep_dev.hpp"
#include "kernels.hpp"
#include "mask.hpp"
#include "mask_dev.hpp"

namespace dwpa {

__global__ __launch_bounds__(256) void k_prep_hybrid(MaskDigits base, const uint64_t* __restrict__ off,
                                                     const uint8_t* __restrict__ bytes, uint64_t first_word,
                                                     uint32_t total, uint64_t mask_first, uint32_t mask_count,
                                                     uint64_t keyspace, uint32_t npos, uint32_t mask_then_word,
                                                     uint32_t minlen, uint32_t maxlen,
                                                     const uint8_t* __restrict__ table, uint32_t* __restrict__ mid,
                                                     uint64_t* __restrict__ ids, uint32_t* __restrict__ counter,
                                                     uint32_t cap) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    uint64_t b0 = 0;
    uint32_t len = 0, w = 0, j = 0;
    if (t < total) {
        w = t / mask_count;
        j = t - w * mask_count;
        b0 = off[first_word + w];
        const uint64_t l64 = off[first_word + w + 1] - b0;
        len = (uint32_t)(l64 < 64 ? l64 : 64);
        keep = l64 <= 63 && len + npos >= minlen && len + npos <= maxlen;
    }
    const uint32_t slot = compact_slot(keep, counter);  // every lane of the wave takes part
    if (!keep || slot >= cap) return;
    uint32_t head[16], tail[16];
    uint32_t n;
    // an empty word reads nothing: it may stand at the very end of the byte buffer
    const uint8_t* wp = len ? bytes + b0 : (const uint8_t*)nullptr;
    if (mask_then_word) {  // wave-uniform
        mask_key_block(base, j, npos, table, head);
        load_key_block(wp, len, tail);
        n = npos;
    } else {
        load_key_block(wp, len, head);
        mask_key_block(base, j, npos, table, tail);
        n = len;
    }
    shift_right_bytes(tail, n);
#pragma unroll
    for (int k = 0; k < 16; k++) head[k] |= tail[k];
    store_mid(mid, cap, slot, head);
    ids[slot] = (first_word + w) * keyspace + mask_first + j;
}

hipError_t launch_prep_hybrid(const uint8_t digits[64], const uint64_t* off, const uint8_t* bytes, uint64_t first_word,
                              uint32_t nwords, uint64_t mask_first, uint32_t mask_count, uint64_t keyspace,
                              uint32_t npos, bool mask_then_word, uint32_t minlen, uint32_t maxlen,
                              const uint8_t* table, uint32_t* mid, uint64_t* ids, uint32_t* counter, uint32_t cap,
                              hipStream_t s) {
    const uint64_t total = (uint64_t)nwords * mask_count;
    if (total == 0) return hipSuccess;  // the caller zeroed the counter
    if (total > 0xffffffffull) return hipErrorInvalidValue;
    const MaskDigits base = mask_digits_pack(digits);
    hipLaunchKernelGGL(k_prep_hybrid, dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0, s, base, off, bytes,
                       first_word, (uint32_t)total, mask_first, mask_count, keyspace, npos, mask_then_word ? 1u : 0u,
                       minlen, maxlen < 64u ? maxlen : 64u, table, mid, ids, counter, cap);
    return hipGetLastError();
}

}  // namespace dwpa
