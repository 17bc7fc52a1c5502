// table_dev.hip -- the table attack on the device (table.hpp has the table, the filter and the order).
//
// k_table_count: one lane per list word.  Its u32 count -- the product of nalt over its bytes -- or 0 for a word the
// filter drops (length outside minlen..maxlen, product above word_max).  The product is kept in 64 bits and tested
// after every factor: it is at most (2^32 - 1) * 16 before the test, so it saturates and never wraps.
//
// k_prep_table: one lane per index first + t, t < count.  The keyspace is the prefix sum start[0..nkept] over the kept
// words, so a lane has to find its word before it can decode its digits:
//   1. one wave-uniform binary search over start[] for the wave's FIRST id.  Every operand is uniform -- the wave's
//      base comes through readfirstlane of a value all lanes agree on, the bounds are kernel arguments -- so the loop's
//      condition is uniform, its loads are scalar and no lane can fall behind and restart it;
//   2. every kept word has at least one candidate, so the wave's 64 ids lie in at most 64 consecutive index entries:
//      a 6-step search per lane inside [j0, j0 + 64), clipped at nkept;
//   3. the word's bytes through load_key_block (any byte offset), then positions last to first: one 32-bit divide of
//      the remaining sub-index by nalt[c], alt[c][digit] into the big-endian key block.  The position loop is unrolled
//      over 63 with the per-lane guard p < len, so every word index and shift is a compile-time constant.
// Then store_mid, ids[slot] = first + slot, and lane 0 of the grid writes the loaded count, as k_prep_mask does: every
// index is a candidate, there is no compaction.  The table image and both index arrays are __restrict__ kernel
// parameters of their own; the table (4,352 bytes) stays in global memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crypto_dev.hpp"
#include "prep_dev.hpp"
#include "kernels.hpp"
#include "table.hpp"

namespace dwpa {

__global__ __launch_bounds__(256) void k_table_count(const uint64_t* __restrict__ off, const uint8_t* __restrict__ bytes,
                                                     uint32_t nwords, const uint8_t* __restrict__ table,
                                                     uint32_t minlen, uint32_t maxlen, uint32_t word_max,
                                                     uint32_t* __restrict__ counts) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nwords) return;
    const uint64_t b0 = off[i];
    const uint64_t len = off[(uint64_t)i + 1] - b0;
    uint32_t k = 0;
    if (len >= minlen && len <= maxlen) {  // maxlen <= 63: the launcher clamps it
        uint64_t prod = 1;
        for (uint32_t p = 0; p < (uint32_t)len && prod <= word_max; p++) prod *= table[bytes[b0 + p]];
        k = prod <= word_max ? (uint32_t)prod : 0u;
    }
    counts[i] = k;
}

__global__ __launch_bounds__(256) void k_prep_table(uint64_t first, uint32_t count, uint32_t nkept,
                                                    const uint64_t* __restrict__ start,
                                                    const uint32_t* __restrict__ kword,
                                                    const uint64_t* __restrict__ off, const uint8_t* __restrict__ bytes,
                                                    const uint8_t* __restrict__ table, uint32_t* __restrict__ mid,
                                                    uint64_t* __restrict__ ids, uint32_t* __restrict__ counter,
                                                    uint32_t cap) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) counter[0] = count;  // the loaded-slot count the PBKDF2 and verify kernels read: no host copy
    if (i >= count || i >= cap) return;
    // all lanes of a wave hold the same i & ~63: whichever lane is read, the value is the wave's
    const uint32_t wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)(i & ~63u));
    const uint64_t id0 = first + wbase;
    uint32_t lo = 0, hi = nkept;  // start[lo] <= id0 < start[hi]: start[0] = 0 and id0 < K = start[nkept]
    while (hi - lo > 1) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (start[m] <= id0) lo = m;
        else hi = m;
    }
    const uint64_t id = first + i;
    uint32_t j = 0;
#pragma unroll
    for (uint32_t step = 32; step >= 1; step >>= 1) {
        const uint32_t c = j + step;
        if (lo + c < nkept && start[lo + c] <= id) j = c;
    }
    j += lo;
    uint32_t sub = (uint32_t)(id - start[j]);  // below the word's count, which is below 2^32
    const uint32_t wi = kword[j];
    const uint64_t b0 = off[wi];
    const uint32_t len = (uint32_t)(off[(uint64_t)wi + 1] - b0);  // minlen..63: the word is kept
    uint32_t w[16], kb[16];
    load_key_block(bytes + b0, len, w);
    const uint8_t* __restrict__ alt = table + 256;
#pragma unroll
    for (int k = 0; k < 16; k++) kb[k] = 0;
#pragma unroll
    for (int p = (int)TABLE_MAX_LEN - 1; p >= 0; p--) {
        if ((uint32_t)p < len) {
            const uint32_t c = (w[p >> 2] >> (24 - 8 * (p & 3))) & 0xffu;
            const uint32_t n = table[c];
            const uint32_t q = sub / n;
            const uint32_t d = sub - q * n;
            sub = q;
            kb[p >> 2] |= (uint32_t)alt[c * TABLE_MAX_ALT + d] << (24 - 8 * (p & 3));
        }
    }
    store_mid(mid, cap, i, kb);
    ids[i] = id;
}

hipError_t launch_table_count(const uint64_t* off, const uint8_t* bytes, uint32_t nwords, const uint8_t* table,
                              uint32_t minlen, uint32_t maxlen, uint32_t word_max, uint32_t* counts, hipStream_t s) {
    if (nwords == 0) return hipSuccess;
    if (!off || !bytes || !table || !counts || word_max == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_table_count, dim3((nwords + 255u) / 256u), dim3(256), 0, s, off, bytes, nwords, table, minlen,
                       maxlen < TABLE_MAX_LEN ? maxlen : TABLE_MAX_LEN, word_max, counts);
    return hipGetLastError();
}

hipError_t launch_prep_table(uint64_t first, uint32_t count, uint32_t nkept, const uint64_t* start,
                             const uint32_t* kword, const uint64_t* off, const uint8_t* bytes, const uint8_t* table,
                             uint32_t* mid, uint64_t* ids, uint32_t* counter, uint32_t cap, hipStream_t s) {
    if (count && (nkept == 0 || !start || !kword || !off || !bytes || !table || count > cap))
        return hipErrorInvalidValue;
    const uint32_t blocks = count ? (count + 255u) / 256u : 1u;  // count 0: one block, for the counter
    hipLaunchKernelGGL(k_prep_table, dim3(blocks), dim3(256), 0, s, first, count, nkept, start, kword, off, bytes,
                       table, mid, ids, counter, cap);
    return hipGetLastError();
}

}  // namespace dwpa
