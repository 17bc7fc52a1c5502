// chain_rules_dev.hip -- k_prep_chain_rules: k_prep_chain (chain_dev.hip) for a chain in which at least one list part
// carries a rule set.  A chain with no ruled part never comes here: it launches k_prep_chain.
//
// A ruled list of nwords words under R rules has nwords * R choices (< 2^32, checked on the host), RULE-MAJOR with
// the word fastest: choice c = rule * nwords + word.  The piece is rule_apply(word) by the shared interpreter
// (rules_apply.hpp); the input word is rejected at 0 bytes or above 256 as k_rules_prep's load_word rejects it, and a
// rejected choice drops the candidate.  The "list word <= 63 bytes" test applies to the RESULT of a ruled part (a
// 100-byte word under '8 is legal, a 40-byte word under d drops); a result of 0 bytes is an ordinary empty piece.
// Un-ruled parts keep k_prep_chain's semantics: an empty word is ordinary and reads nothing, a raw length above 63
// drops.
//
// One lane per raw index first + t, t < count.  Pass 1 is k_prep_chain's carry arithmetic with radix = nwords * R for
// a ruled part; its digit is the choice, which one more 32-bit divide by nwords splits into (rule, word).  No 64-bit
// divide.
//
// Rule dispatch is wave-uniform by construction.  The word is fastest, so the 64 raw indices of a wave hold few
// distinct rules at a ruled part: at the last part at most ceil(64 / nwords) + 1, at an earlier part 1 or 2 (its
// digit moves only with a carry).  Per ruled part the wave loops over those distinct rules: while __ballot(pending)
// is non-zero it takes the rule r of the first pending lane into a scalar, the lanes with rule == r run rule_apply
// with roffs[r] and the code pointer formed from that scalar (scalar loads of the rule code, a uniform branch at the
// interpreter's switch), and clear `pending`.  Every iteration clears at least the lane it took r from, so the loop
// ends after as many iterations as the wave holds distinct rules; lanes with t >= count, dropped lanes and lanes whose
// input word is rejected start with pending = false, so a partial last wave ends too.  r is read from the first
// PENDING lane (readlane at the ballot's lowest bit), not from the first active one: the loop's condition is uniform,
// so lanes that are done stay active in it, and their rule must not be taken again.
//
// One private w[] / mem[] pair (RULE_RP + 4 bytes each, in scratch as in k_rules_prep) is reused part after part.  A
// ruled piece is packed into a 16-word big-endian block as k_rules_prep packs kb[], never from more than 63 bytes (a
// longer result marks the lane dropped and packs nothing), and joined as in k_prep_chain, last part first:
//   acc = part_block | shift_right_bytes(acc, len_p)
// with every len_p in 0..63 (a dropped lane joins with 0).  The lengths are known only after the rules have run, so
// `keep` is decided after all parts; then compact_slot with every lane of the wave taking part, then store_mid.
//
// Part kinds, rule sets and nparts are wave-uniform; the part loops are unrolled over 4 with uniform guards.  No LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crypto_dev.hpp"
#include "prep_dev.hpp"
#include "kernels.hpp"
#include "mask.hpp"
#include "mask_dev.hpp"
#include "rules_apply.hpp"

namespace dwpa {

struct ChainRulesPartArg {
    const uint64_t* off;    // list: nwords + 1 byte offsets
    const uint8_t* bytes;   // list: the words' bytes
    const uint8_t* table;   // mask: the 16 KiB table (mask.hpp)
    uint64_t radix;         // N: a list's word count, a ruled list's nwords * R, a mask's keyspace
    uint64_t room;          // N - digit of `first`, >= 1
    uint32_t digit;         // list: the word index (ruled: the choice) of `first`
    uint32_t npos;          // mask: positions, 1..63; 0: a list
    uint32_t nwords;        // ruled list: its word count, >= 1; 0: not ruled
};

// The rule image of part p (RuleSet::flatten: R + 1 offsets into the op words; null for a part without rules).  These
// travel as __restrict__ kernel parameters of their own and not inside ChainRulesArgs: only then does the compiler
// know that nothing the kernel stores can change them, and fetch the offsets and the op words by scalar loads.
#define CHAIN_RULES_PARAMS                                                                                     \
    const uint32_t *__restrict__ roffs0, const uint32_t *__restrict__ rcode0, const uint32_t *__restrict__ roffs1, \
        const uint32_t *__restrict__ rcode1, const uint32_t *__restrict__ roffs2,                              \
        const uint32_t *__restrict__ rcode2, const uint32_t *__restrict__ roffs3, const uint32_t *__restrict__ rcode3

struct ChainRulesArgs {
    ChainRulesPartArg part[DWPA_CHAIN_MAX_PARTS];
    MaskDigits digits[DWPA_CHAIN_MAX_PARTS];  // mask parts: the position digits of `first`
    uint32_t nparts;
};

// Word wi into w: its length, or -1 where the rule engine rejects the input (0 bytes, above RULE_RP), as load_word in
// rules_dev.hip.  *src = where the word lies in HBM (the memory functions' initial memory).
__device__ __forceinline__ int chain_load_word(const uint64_t* __restrict__ off, const uint8_t* __restrict__ bytes,
                                               uint32_t wi, uint8_t* w, const uint8_t** src) {
    const uint64_t b0 = off[wi], b1 = off[(uint64_t)wi + 1];
    const uint64_t n = b1 - b0;
    *src = bytes + b0;
    if (n < 1 || n > (uint64_t)RULE_RP) return -1;
    for (uint32_t i = 0; i < (uint32_t)n; i++) w[i] = bytes[b0 + i];
    return (int)n;
}

__global__ __launch_bounds__(256) void k_prep_chain_rules(ChainRulesArgs a, CHAIN_RULES_PARAMS, uint64_t first,
                                                          uint32_t count, uint32_t minlen, uint32_t maxlen,
                                                          uint32_t* __restrict__ mid, uint64_t* __restrict__ ids,
                                                          uint32_t* __restrict__ counter, uint32_t cap) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = t < count;
    // list: word index; ruled list: choice; mask: offset added to the part's digits
    uint32_t sel[DWPA_CHAIN_MAX_PARTS] = {0, 0, 0, 0};
    uint32_t ulen[DWPA_CHAIN_MAX_PARTS] = {0, 0, 0, 0};  // un-ruled list: the word's length, where it is <= 63
    uint32_t carry = live ? t : 0u;
    bool ok = live;  // no part has dropped the candidate so far
#pragma unroll
    for (int p = DWPA_CHAIN_MAX_PARTS - 1; p >= 0; p--) {
        if ((uint32_t)p < a.nparts) {  // wave-uniform
            const ChainRulesPartArg& pa = a.part[p];
            uint32_t q = 0, rem = carry;
            if ((pa.radix >> 32) == 0) {  // wave-uniform
                q = carry / (uint32_t)pa.radix;
                rem = carry - q * (uint32_t)pa.radix;
            }
            const bool wrap = (uint64_t)rem >= pa.room;
            if (pa.npos) {  // a mask part
                sel[p] = carry;
            } else {
                const uint32_t d = wrap ? rem - (uint32_t)pa.room : pa.digit + rem;
                sel[p] = d;
                if (pa.nwords == 0 && live) {  // an un-ruled list: its length decides now
                    const uint64_t l64 = pa.off[(uint64_t)d + 1] - pa.off[d];
                    ok = ok && l64 <= 63;
                    ulen[p] = l64 <= 63 ? (uint32_t)l64 : 0u;
                }
            }
            carry = q + (wrap ? 1u : 0u);
        }
    }
    uint8_t w[RULE_RP + 4], mem[RULE_RP + 4];
    uint32_t acc[16], blk[16];
    uint32_t total = 0;
#pragma unroll
    for (int p = DWPA_CHAIN_MAX_PARTS - 1; p >= 0; p--) {
        if ((uint32_t)p < a.nparts) {  // wave-uniform
            const ChainRulesPartArg& pa = a.part[p];
            uint32_t len = 0;  // 0..63 on every lane: the shift below is defined
#pragma unroll
            for (int k = 0; k < 16; k++) blk[k] = 0;
            if (pa.npos) {  // wave-uniform
                len = pa.npos;
                if (ok) mask_key_block(a.digits[p], sel[p], len, pa.table, blk);
            } else if (pa.nwords == 0) {  // wave-uniform: an un-ruled list
                if (ok) {
                    len = ulen[p];
                    // an empty word reads nothing: it may stand at the very end of its byte buffer
                    load_key_block(len ? pa.bytes + pa.off[sel[p]] : (const uint8_t*)nullptr, len, blk);
                }
            } else {  // a ruled list
                // p is a constant of the unrolled loop: these fold to one parameter each
                const uint32_t* __restrict__ roffs = p == 0 ? roffs0 : p == 1 ? roffs1 : p == 2 ? roffs2 : roffs3;
                const uint32_t* __restrict__ rcode = p == 0 ? rcode0 : p == 1 ? rcode1 : p == 2 ? rcode2 : rcode3;
                const uint32_t rule = sel[p] / pa.nwords;
                const uint32_t word = sel[p] - rule * pa.nwords;
                int rl = -1;
                const uint8_t* src = nullptr;
                if (ok) rl = chain_load_word(pa.off, pa.bytes, word, w, &src);
                bool pending = rl > 0;
                uint64_t m;
                while ((m = __ballot(pending)) != 0) {
                    const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)rule, (int)__builtin_ctzll(m));
                    // formed here, from the scalar and ahead of the branch: below `rule == r` the compiler may put
                    // the lane's own `rule` in r's place, and the fetches would turn into vector loads
                    const uint32_t c0 = roffs[r], c1 = roffs[r + 1];
                    const uint32_t* code = rcode + c0;
                    if (pending && rule == r) {
                        rl = rule_apply(w, rl, mem, src, rl, code, c1 - c0);
                        pending = false;
                    }
                }
                ok = ok && rl >= 0 && rl <= 63;
                len = ok ? (uint32_t)rl : 0u;
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    uint32_t v = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        const uint32_t k = 4 * j + b;
                        v = (v << 8) | (k < len ? (uint32_t)w[k] : 0u);
                    }
                    blk[j] = v;
                }
            }
            if ((uint32_t)p + 1 == a.nparts) {  // the last part starts the suffix
#pragma unroll
                for (int k = 0; k < 16; k++) acc[k] = blk[k];
            } else {
                shift_right_bytes(acc, len);
#pragma unroll
                for (int k = 0; k < 16; k++) acc[k] |= blk[k];
            }
            total += len;
        }
    }
    const bool keep = ok && total >= minlen && total <= maxlen;
    const uint32_t slot = compact_slot(keep, counter);  // every lane of the wave takes part
    if (!keep || slot >= cap) return;
    store_mid(mid, cap, slot, acc);
    ids[slot] = first + t;
}

hipError_t launch_prep_chain_rules(const ChainPartLaunch* parts, uint32_t nparts, uint64_t first, uint32_t count,
                                   uint32_t minlen, uint32_t maxlen, uint32_t* mid, uint64_t* ids, uint32_t* counter,
                                   uint32_t cap, hipStream_t s) {
    if (count == 0) return hipSuccess;  // the caller zeroed the counter
    if (!parts || nparts == 0 || nparts > DWPA_CHAIN_MAX_PARTS || count > cap) return hipErrorInvalidValue;
    ChainRulesArgs a = {};
    a.nparts = nparts;
    const uint32_t *roffs[DWPA_CHAIN_MAX_PARTS] = {}, *rcode[DWPA_CHAIN_MAX_PARTS] = {};
    for (uint32_t p = 0; p < nparts; p++) {
        const ChainPartLaunch& in = parts[p];
        if (in.digit >= in.radix) return hipErrorInvalidValue;
        ChainRulesPartArg& pa = a.part[p];
        pa.radix = in.radix;
        pa.room = in.radix - in.digit;
        if (in.is_mask) {
            if (!in.table || in.npos == 0 || in.npos > MASK_MAX_POS || in.nrules) return hipErrorInvalidValue;
            pa.table = in.table;
            pa.npos = in.npos;
            a.digits[p] = mask_digits_pack(in.digits);
        } else {
            if (!in.off || in.radix > 0xffffffffull) return hipErrorInvalidValue;
            pa.off = in.off;
            pa.bytes = in.bytes;
            pa.digit = (uint32_t)in.digit;
            if (in.nrules) {  // radix = nwords * nrules, exactly
                if (!in.roffs || !in.rcode || in.radix % in.nrules) return hipErrorInvalidValue;
                roffs[p] = in.roffs;
                rcode[p] = in.rcode;
                pa.nwords = (uint32_t)(in.radix / in.nrules);
            }
        }
    }
    hipLaunchKernelGGL(k_prep_chain_rules, dim3((count + 255u) / 256u), dim3(256), 0, s, a, roffs[0], rcode[0],
                       roffs[1], rcode[1], roffs[2], rcode[2], roffs[3], rcode[3], first, count, minlen,
                       maxlen < 64u ? maxlen : 64u, mid, ids, counter, cap);
    return hipGetLastError();
}

}  // namespace dwpa
