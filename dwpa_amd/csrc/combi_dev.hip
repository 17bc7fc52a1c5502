// combi_dev.hip -- k_prep_combinator: hashcat -a 1 (left word || right word) -> HMAC key midstates.
//
// Terms.  A candidate is left || right, left from the first list and right from the second, as `hashcat -a 1 left
// right` joins them.  One of the two lists is the *amplifier*: it lies whole in HBM and its index runs fastest.  The
// other is the *base*: the caller streams it through in pieces.  amp_is_left (wave-uniform) says which of the two
// stands left in the join; it changes the order of the candidates and nothing about the join itself.
//
// One lane per (base word s, amplifier offset j) of a load of nbase x amp_count raw pairs, base-major: s = t /
// amp_count, j = t % amp_count (one 32-bit divide: the launch has fewer than 2^32 lanes).  Both words come from
// offsets[] / bytes[] arrays in HBM (as k_prep_dict reads its dictionary) through load_key_block, which reads only the
// dwords that hold a byte of the word; an empty word reads nothing.  Both halves are 16-word big-endian blocks that
// start at byte 0; the right one is moved behind the left by shift_right_bytes (prep_dev.hpp) and the two are ORed:
//   kb = left_block | shift_right_bytes(right_block, L_left)
// A pair is kept iff both words are <= 63 bytes and minlen <= L + R <= maxlen (maxlen <= 64 here: the launcher
// clamps it, one key block holds 64 bytes).  The decision depends on both halves, so it is per lane.  Kept lanes take
// compacted slots (one atomic per wave, lane order inside the wave), so dropped pairs leave no holes and ids[slot]
// carries (first_base + s) * A + amp_first + j, A the amplifier's word count.  The counter ends as the raw kept count,
// which may exceed cap in a fill-mode load (lanes beyond cap store nothing), exactly as k_prep_hybrid leaves it.
//
// With amp_count >= 64 a wave usually holds one base word, but nothing here relies on that: each lane reads its own
// base word (the lanes of a wave then read the same dwords, which the memory pipeline serves as one request).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crypto_dev.hpp"
#include "prep_dev.hpp"
#include "kernels.hpp"

namespace dwpa {

__global__ __launch_bounds__(256) void k_prep_combinator(const uint64_t* __restrict__ base_off,
                                                         const uint8_t* __restrict__ base_bytes, uint64_t first_base,
                                                         const uint64_t* __restrict__ amp_off,
                                                         const uint8_t* __restrict__ amp_bytes, uint64_t amp_words,
                                                         uint64_t amp_first, uint32_t amp_count, uint32_t total,
                                                         uint32_t amp_is_left, uint32_t minlen, uint32_t maxlen,
                                                         uint32_t* __restrict__ mid, uint64_t* __restrict__ ids,
                                                         uint32_t* __restrict__ counter, uint32_t cap) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    uint64_t bb = 0, ab = 0;
    uint32_t blen = 0, alen = 0, s = 0, j = 0;
    if (t < total) {
        s = t / amp_count;
        j = t - s * amp_count;
        bb = base_off[first_base + s];
        const uint64_t bl = base_off[first_base + s + 1] - bb;
        ab = amp_off[amp_first + j];
        const uint64_t al = amp_off[amp_first + j + 1] - ab;
        blen = (uint32_t)(bl < 64 ? bl : 64);
        alen = (uint32_t)(al < 64 ? al : 64);
        keep = bl <= 63 && al <= 63 && blen + alen >= minlen && blen + alen <= maxlen;
    }
    const uint32_t slot = compact_slot(keep, counter);  // every lane of the wave takes part
    if (!keep || slot >= cap) return;
    // an empty word reads nothing: it may stand at the very end of its byte buffer
    const uint8_t* bp = blen ? base_bytes + bb : (const uint8_t*)nullptr;
    const uint8_t* ap = alen ? amp_bytes + ab : (const uint8_t*)nullptr;
    const uint8_t* lp = amp_is_left ? ap : bp;  // wave-uniform choice
    const uint8_t* rp = amp_is_left ? bp : ap;
    const uint32_t llen = amp_is_left ? alen : blen, rlen = amp_is_left ? blen : alen;
    uint32_t head[16], tail[16];
    load_key_block(lp, llen, head);
    load_key_block(rp, rlen, tail);
    shift_right_bytes(tail, llen);
#pragma unroll
    for (int k = 0; k < 16; k++) head[k] |= tail[k];
    store_mid(mid, cap, slot, head);
    ids[slot] = (first_base + s) * amp_words + amp_first + j;
}

hipError_t launch_prep_combinator(const uint64_t* base_off, const uint8_t* base_bytes, uint64_t first_base,
                                  uint32_t nbase, const uint64_t* amp_off, const uint8_t* amp_bytes, uint64_t amp_words,
                                  uint64_t amp_first, uint32_t amp_count, bool amp_is_left, uint32_t minlen,
                                  uint32_t maxlen, uint32_t* mid, uint64_t* ids, uint32_t* counter, uint32_t cap,
                                  hipStream_t s) {
    const uint64_t total = (uint64_t)nbase * amp_count;
    if (total == 0) return hipSuccess;  // the caller zeroed the counter
    if (total > 0xffffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_prep_combinator, dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0, s, base_off,
                       base_bytes, first_base, amp_off, amp_bytes, amp_words, amp_first, amp_count, (uint32_t)total,
                       amp_is_left ? 1u : 0u, minlen, maxlen < 64u ? maxlen : 64u, mid, ids, counter, cap);
    return hipGetLastError();
}

}  // namespace dwpa
