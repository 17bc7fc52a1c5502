// chain_dev.hip -- k_prep_chain: a chain of 1..4 parts, each a word list in HBM or a mask, joined left to right ->
// HMAC key midstates.  It generalises k_prep_mask (one mask part), k_prep_hybrid (list + mask, mask + list) and
// k_prep_combinator (list + list); chain.hpp has the order.
//
// One lane per raw index first + t, t < count.  The host has decomposed `first` into one digit per part (a list's
// word index; a mask part's own index as its 64 position digits) and passes everything by value in the kernel
// arguments.  A lane adds t at the last part and carries upwards, in two passes:
//
// Pass 1, every lane, lengths only.  Part p takes the carry c of the parts behind it (c = t at the last part).  With
// radix N (a list's word count, a mask part's keyspace) and d the digit of `first`:
//   q = c / N, rem = c - q * N          one 32-bit divide; N >= 2^32 (a wide mask part): q = 0, rem = c
//   wrap = rem >= N - d                 `room` = N - d >= 1 comes from the host; compared in 64 bits, so the sum
//                                       d + rem, which can reach 2^33, is never formed
//   digit = wrap ? rem - room : d + rem
//   carry out = q + wrap                <= c: nothing overflows for any 64-bit `first`
// A list part keeps its word index and reads its two offsets for the word's length.  A mask part keeps c itself:
// mask_key_block adds any 32-bit offset to the part's digits and drops the carry out of its position 0, which is the
// index modulo the part's keyspace -- so its position loop is the one k_prep_mask and k_prep_hybrid run, unchanged,
// and the carry that has to leave the part is computed here instead.  The carry out of part 0 is 0, because the host
// checks first + count <= K.  A candidate is kept iff every list word is <= 63 bytes and minlen <= total length <=
// maxlen (maxlen <= 64: the launcher clamps it, one key block holds 64 bytes): the decision needs lengths alone, so
// dropped lanes read no text and build no mask block.
//
// Kept lanes take compacted slots (compact_slot, every lane of the wave taking part) and only they run pass 2, the
// join, last part first:
//   acc = part_block | shift_right_bytes(acc, len_p)
// acc is the suffix's block starting at byte 0; part_block comes from load_key_block (only dwords that hold a byte of
// the word; an empty word reads nothing) or mask_key_block.  Two 16-word blocks are live.  Every shift is a kept
// part's length, 0..63, which shift_right_bytes defines; a word above 63 bytes is never read or shifted by.
//
// Part kinds and nparts are wave-uniform; the part loops are unrolled over 4 with uniform guards, so no register
// array is indexed dynamically.  No LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crypto_dev.hpp"
#include "prep_dev.hpp"
#include "kernels.hpp"
#include "mask.hpp"
#include "mask_dev.hpp"

namespace dwpa {

struct ChainPartArg {
    const uint64_t* off;   // list: radix + 1 byte offsets
    const uint8_t* bytes;  // list: the words' bytes
    const uint8_t* table;  // mask: the 16 KiB table (mask.hpp)
    uint64_t radix;        // N
    uint64_t room;         // N - digit of `first`, >= 1
    uint32_t digit;        // list: the word index of `first`
    uint32_t npos;         // mask: positions, 1..63; 0: a list
};

struct ChainArgs {
    ChainPartArg part[DWPA_CHAIN_MAX_PARTS];
    MaskDigits digits[DWPA_CHAIN_MAX_PARTS];  // mask parts: the position digits of `first`
    uint32_t nparts;
};

__global__ __launch_bounds__(256) void k_prep_chain(ChainArgs a, uint64_t first, uint32_t count, uint32_t minlen,
                                                    uint32_t maxlen, uint32_t* __restrict__ mid,
                                                    uint64_t* __restrict__ ids, uint32_t* __restrict__ counter,
                                                    uint32_t cap) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = t < count;
    uint32_t sel[DWPA_CHAIN_MAX_PARTS] = {0, 0, 0, 0};  // list: word index; mask: offset added to the part's digits
    uint32_t carry = live ? t : 0u;
    uint32_t total = 0;
    bool fits = true;
#pragma unroll
    for (int p = DWPA_CHAIN_MAX_PARTS - 1; p >= 0; p--) {
        if ((uint32_t)p < a.nparts) {  // wave-uniform
            const ChainPartArg& pa = a.part[p];
            uint32_t q = 0, rem = carry;
            if ((pa.radix >> 32) == 0) {  // wave-uniform
                q = carry / (uint32_t)pa.radix;
                rem = carry - q * (uint32_t)pa.radix;
            }
            const bool wrap = (uint64_t)rem >= pa.room;
            if (pa.npos) {  // a mask part
                sel[p] = carry;
                total += pa.npos;
            } else {
                const uint32_t w = wrap ? rem - (uint32_t)pa.room : pa.digit + rem;
                sel[p] = w;
                if (live) {
                    const uint64_t l64 = pa.off[(uint64_t)w + 1] - pa.off[w];
                    fits = fits && l64 <= 63;
                    total += (uint32_t)(l64 < 64 ? l64 : 64);
                }
            }
            carry = q + (wrap ? 1u : 0u);
        }
    }
    const bool keep = live && fits && total >= minlen && total <= maxlen;
    const uint32_t slot = compact_slot(keep, counter);  // every lane of the wave takes part
    if (!keep || slot >= cap) return;
    uint32_t acc[16], blk[16];
#pragma unroll
    for (int p = DWPA_CHAIN_MAX_PARTS - 1; p >= 0; p--) {
        if ((uint32_t)p < a.nparts) {  // wave-uniform
            const ChainPartArg& pa = a.part[p];
            uint32_t len;
            if (pa.npos) {  // wave-uniform
                len = pa.npos;
                mask_key_block(a.digits[p], sel[p], len, pa.table, blk);
            } else {
                const uint64_t b0 = pa.off[sel[p]];
                len = (uint32_t)(pa.off[(uint64_t)sel[p] + 1] - b0);  // <= 63: the lane is kept
                // an empty word reads nothing: it may stand at the very end of its byte buffer
                load_key_block(len ? pa.bytes + b0 : (const uint8_t*)nullptr, len, blk);
            }
            if ((uint32_t)p + 1 == a.nparts) {  // the last part starts the suffix
#pragma unroll
                for (int k = 0; k < 16; k++) acc[k] = blk[k];
            } else {
                shift_right_bytes(acc, len);
#pragma unroll
                for (int k = 0; k < 16; k++) acc[k] |= blk[k];
            }
        }
    }
    store_mid(mid, cap, slot, acc);
    ids[slot] = first + t;
}

hipError_t launch_prep_chain(const ChainPartLaunch* parts, uint32_t nparts, uint64_t first, uint32_t count,
                             uint32_t minlen, uint32_t maxlen, uint32_t* mid, uint64_t* ids, uint32_t* counter,
                             uint32_t cap, hipStream_t s) {
    if (count == 0) return hipSuccess;  // the caller zeroed the counter
    if (!parts || nparts == 0 || nparts > DWPA_CHAIN_MAX_PARTS || count > cap) return hipErrorInvalidValue;
    ChainArgs a = {};
    a.nparts = nparts;
    for (uint32_t p = 0; p < nparts; p++) {
        const ChainPartLaunch& in = parts[p];
        if (in.digit >= in.radix) return hipErrorInvalidValue;
        ChainPartArg& pa = a.part[p];
        pa.radix = in.radix;
        pa.room = in.radix - in.digit;
        if (in.is_mask) {
            if (!in.table || in.npos == 0 || in.npos > MASK_MAX_POS) return hipErrorInvalidValue;
            pa.table = in.table;
            pa.npos = in.npos;
            a.digits[p] = mask_digits_pack(in.digits);
        } else {
            if (!in.off || in.radix > 0xffffffffull) return hipErrorInvalidValue;
            pa.off = in.off;
            pa.bytes = in.bytes;
            pa.digit = (uint32_t)in.digit;
        }
    }
    hipLaunchKernelGGL(k_prep_chain, dim3((count + 255u) / 256u), dim3(256), 0, s, a, first, count, minlen,
                       maxlen < 64u ? maxlen : 64u, mid, ids, counter, cap);
    return hipGetLastError();
}

}  // namespace dwpa
