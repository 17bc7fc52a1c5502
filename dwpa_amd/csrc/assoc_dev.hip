// assoc_dev.hip -- the association attack on the device (assoc.hpp has the nets, the entries and the order).
//
// k_prep_assoc: one lane per raw index first + t, t < count.  The keyspace is the prefix sum start[0..nidx] over the
// nets that own indices (W_n x R > 0), so a lane finds its net as k_prep_table finds its word:
//   1. one wave-uniform binary search over start[] for the wave's FIRST id: the wave's base comes through
//      readfirstlane of a value all lanes agree on, the bounds are kernel arguments, so the loop's condition is uniform
//      and its loads are scalar;
//   2. a net in the index owns at least one index, so the wave's 64 ids lie in at most 64 consecutive entries: a
//      6-step search per lane inside [j0, j0 + 64), clipped at nidx;
//   3. sub = id - start[j] < W x R < 2^32 splits into (rule, word) with one 32-bit divide, rule-major with the word
//      fastest, as a ruled chain part.
// The candidate is rule(word) by the shared interpreter under k_prep_chain_rules' distinct-rules ballot loop: while
// __ballot(pending) is non-zero the wave takes the rule of the first PENDING lane into a scalar, forms the code pointer
// from that scalar (scalar loads of the rule code, a uniform branch at the interpreter's switch) and the lanes with that
// rule run it.  The rule image travels as __restrict__ parameters of its own.  Without rules (R = 1, the identity) the
// RULES = false instantiation skips the interpreter and packs the word with load_key_block.
//
// keep = not rejected, minlen <= length <= min(maxlen, 63), and the net has a live line.  compact_slot (every lane of
// the wave takes part) gives the slot; store_mid, ids[slot] = first + t, sref[slot] = the word offset of the net's ESSID
// salt entry {nsalt, [2][nsalt][16]} (what launch_pbkdf2_ms reads).
//
// Segments.  compact_slot keeps lane order inside a wave and the nets are ascending in the index, so the kept lanes of
// one net in one wave hold consecutive slots.  The first kept lane of each such run walks the net's live lines
// (net_line_off[] / net_line[], rebuilt by the host when the retired set changes; an entry is line | class << 30) and
// appends SegDev{line, the run's first slot, the run's kept lanes} to the list of the line's verify class (PMKID,
// keyver 1, 2, 3: one device counter each).  A counter counts past its list's capacity, but the record is then not
// written: the host grows the list and repeats the load.  No LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crypto_dev.hpp"
#include "prep_dev.hpp"
#include "kernels.hpp"
#include "rules_apply.hpp"

namespace dwpa {

struct AssocSegs {
    SegDev* list[4];
    uint32_t cap[4];
};

template <bool RULES>
__global__ __launch_bounds__(256) void k_prep_assoc(uint64_t first, uint32_t count, uint32_t nidx,
                                                    const uint64_t* __restrict__ start,
                                                    const AssocEntry* __restrict__ ent,
                                                    const uint64_t* __restrict__ woff, const uint8_t* __restrict__ wbytes,
                                                    const uint32_t* __restrict__ roffs, const uint32_t* __restrict__ rcode,
                                                    const uint32_t* __restrict__ net_line_off,
                                                    const uint32_t* __restrict__ net_line, uint32_t minlen,
                                                    uint32_t maxlen, uint32_t* __restrict__ mid,
                                                    uint64_t* __restrict__ ids, uint32_t* __restrict__ sref,
                                                    uint32_t* __restrict__ counter, uint32_t cap, AssocSegs segs,
                                                    uint32_t* __restrict__ segcnt) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    // all lanes of a wave hold the same t & ~63: whichever lane is read, the value is the wave's
    const uint32_t wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t & ~63u));
    if (wbase >= count) return;  // the whole wave: uniform
    const bool live = t < count;
    const uint64_t id0 = first + wbase;
    uint32_t lo = 0, hi = nidx;  // start[lo] <= id0 < start[hi]: start[0] = 0 and id0 < K = start[nidx]
    while (hi - lo > 1) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (start[m] <= id0) lo = m;
        else hi = m;
    }
    const uint64_t id = live ? first + t : id0;  // a lane past the load stands on the wave's first id and keeps nothing
    uint32_t j = 0;
#pragma unroll
    for (uint32_t step = 32; step >= 1; step >>= 1) {
        const uint32_t c = j + step;
        if (lo + c < nidx && start[lo + c] <= id) j = c;
    }
    j += lo;
    const uint32_t sub = (uint32_t)(id - start[j]);  // below W x R, which is below 2^32
    const AssocEntry e = ent[j];
    const uint32_t rule = sub / e.nwords;
    const uint64_t wi = (uint64_t)e.wfirst + (sub - rule * e.nwords);
    const bool want = live && net_line_off[e.net + 1] > net_line_off[e.net];  // a net without a live line costs nothing

    uint32_t kb[16];
    uint32_t len = 0;
    bool ok = false;
    if constexpr (RULES) {
        uint8_t w[RULE_RP + 4], mem[RULE_RP + 4];
        int rl = -1;
        const uint8_t* src = wbytes;
        if (want) {  // as load_word in rules_dev.hip: 0 bytes or above RULE_RP is rejected
            const uint64_t b0 = woff[wi], n = woff[wi + 1] - b0;
            src = wbytes + b0;
            if (n >= 1 && n <= (uint64_t)RULE_RP) {
                for (uint32_t i = 0; i < (uint32_t)n; i++) w[i] = src[i];
                rl = (int)n;
            }
        }
        bool pending = rl > 0;
        uint64_t m;
        while ((m = __ballot(pending)) != 0) {
            const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)rule, (int)__builtin_ctzll(m));
            // formed here, from the scalar and ahead of the branch: below `rule == r` the compiler may put the lane's
            // own `rule` in r's place, and the fetches would turn into vector loads
            const uint32_t c0 = roffs[r], c1 = roffs[r + 1];
            const uint32_t* code = rcode + c0;
            if (pending && rule == r) {
                rl = rule_apply(w, rl, mem, src, rl, code, c1 - c0);
                pending = false;
            }
        }
        ok = rl >= 0 && rl <= 63;
        len = ok ? (uint32_t)rl : 0u;
#pragma unroll
        for (int q = 0; q < 16; q++) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const uint32_t k = 4 * q + b;
                v = (v << 8) | (k < len ? (uint32_t)w[k] : 0u);
            }
            kb[q] = v;
        }
    } else {
        if (want) {
            const uint64_t b0 = woff[wi], n = woff[wi + 1] - b0;
            ok = n >= 1 && n <= 63;
            len = ok ? (uint32_t)n : 0u;
            if (ok) load_key_block(wbytes + b0, len, kb);
        }
    }
    const bool keep = ok && len >= minlen && len <= maxlen;
    const uint32_t slot = compact_slot(keep, counter);  // every lane of the wave takes part
    const uint64_t kept = __ballot(keep);
    const bool fits = keep && slot < cap;  // count <= cap, so every kept lane fits: the test only guards the stores
    if (fits) {
        store_mid(mid, cap, slot, kb);
        ids[slot] = first + t;
        sref[slot] = e.sref;
    }
    // the runs: a kept lane whose nearest kept lane below stands in another net starts one
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t below = kept & ((1ull << lane) - 1ull);
    const int prev = below ? 63 - (int)__builtin_clzll(below) : 0;
    const uint32_t jprev = (uint32_t)__shfl((int)j, prev);
    const bool head = keep && (!below || jprev != j);
    const uint64_t heads = __ballot(head);
    if (!head || !fits) return;
    const uint64_t from = ~((1ull << lane) - 1ull);                         // this lane and above
    const uint64_t above = lane < 63 ? heads & ~((2ull << lane) - 1ull) : 0ull;  // the heads after this one
    const uint64_t upto = above ? (1ull << __builtin_ctzll(above)) - 1ull : ~0ull;
    const uint32_t n = (uint32_t)__popcll(kept & from & upto);
    for (uint32_t l = net_line_off[e.net]; l < net_line_off[e.net + 1]; l++) {
        const uint32_t v = net_line[l];
        const uint32_t c = v >> 30;
        const uint32_t pos = atomicAdd(segcnt + c, 1u);
        if (pos < segs.cap[c]) {
            SegDev sg;
            sg.line = v & 0x3fffffffu;
            sg.slot = slot;
            sg.count = n;
            sg.pad = 0;
            segs.list[c][pos] = sg;
        }
    }
}

hipError_t launch_prep_assoc(const AssocLaunch& a, uint64_t first, uint32_t count, uint32_t minlen, uint32_t maxlen,
                             uint32_t* mid, uint64_t* ids, uint32_t* sref, uint32_t* counter, uint32_t cap,
                             SegDev* const seg[4], const uint32_t segcap[4], uint32_t* segcnt, hipStream_t s) {
    if (count == 0) return hipSuccess;  // the caller zeroed the counters
    if (a.nidx == 0 || !a.start || !a.ent || !a.woff || !a.wbytes || !a.net_line_off || !a.net_line || !mid || !ids ||
        !sref || !counter || !segcnt || count > cap || (a.nrules && (!a.roffs || !a.rcode)))
        return hipErrorInvalidValue;
    AssocSegs sg;
    for (int c = 0; c < 4; c++) {
        if (segcap[c] && !seg[c]) return hipErrorInvalidValue;
        sg.list[c] = seg[c];
        sg.cap[c] = segcap[c];
    }
    const dim3 grid((count + 255u) / 256u), block(256);
    const uint32_t mx = maxlen < 63u ? maxlen : 63u;
    if (a.nrules)
        hipLaunchKernelGGL(k_prep_assoc<true>, grid, block, 0, s, first, count, a.nidx, a.start, a.ent, a.woff, a.wbytes,
                           a.roffs, a.rcode, a.net_line_off, a.net_line, minlen, mx, mid, ids, sref, counter, cap, sg,
                           segcnt);
    else
        hipLaunchKernelGGL(k_prep_assoc<false>, grid, block, 0, s, first, count, a.nidx, a.start, a.ent, a.woff, a.wbytes,
                           a.roffs, a.rcode, a.net_line_off, a.net_line, minlen, mx, mid, ids, sref, counter, cap, sg,
                           segcnt);
    return hipGetLastError();
}

}  // namespace dwpa
