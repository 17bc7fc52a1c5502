// kernels.hpp -- host-side launchers for kernels.hip (internal to libdwpa22000.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "tables.hpp"

namespace dwpa {

hipError_t launch_prep_dict(const uint64_t* off, const uint8_t* bytes, uint64_t first, uint32_t count, uint32_t minlen,
                            uint32_t maxlen, uint32_t* mid, uint64_t* ids, uint32_t* counter, uint32_t cap,
                            bool compact, hipStream_t s);
// check path: unique key u = slot uslot[u] of the call's key bytes (koff/klen per slot) -> mid row u
hipError_t launch_prep_keys(const uint64_t* koff, const uint32_t* klen, const uint8_t* kbytes, const uint32_t* uslot,
                            uint32_t count, uint32_t* mid, uint32_t cap, hipStream_t s);
hipError_t launch_prep_numeric(uint64_t first, uint32_t count, uint32_t digits, uint32_t* mid, uint64_t* ids,
                               uint32_t cap, hipStream_t s);
// mask_dev.hip: mask candidates [first, first + count) -> midstates, ids[slot] = first + slot, *counter = count
// (written by the kernel).  digits: the mixed-radix digits of `first` (mask_digits), table: the device copy of
// mask_table (mask.hpp).  count <= cap.
hipError_t launch_prep_mask(const uint8_t digits[64], uint64_t first, uint32_t count, uint32_t npos,
                            const uint8_t* table, uint32_t* mid, uint64_t* ids, uint32_t* counter, uint32_t cap,
                            hipStream_t s);
// markov_dev.hip: the same for the Markov-ordered mask (markov.hpp): digits over the thresholded radices
// (markov_digits), table: the device copy of markov_table.
hipError_t launch_prep_markov(const uint8_t digits[64], uint64_t first, uint32_t count, uint32_t npos,
                              const uint8_t* table, uint32_t* mid, uint64_t* ids, uint32_t* counter, uint32_t cap,
                              hipStream_t s);
// table_dev.hip: counts[i] = word i's candidate count under the table image (table.hpp Table), 0 for a word the filter
// drops (length outside minlen..min(maxlen, 63), count above word_max >= 1).  off: nwords + 1 byte offsets.
hipError_t launch_table_count(const uint64_t* off, const uint8_t* bytes, uint32_t nwords, const uint8_t* table,
                              uint32_t minlen, uint32_t maxlen, uint32_t word_max, uint32_t* counts, hipStream_t s);
// table candidates [first, first + count) -> midstates, ids[slot] = first + slot, *counter = count (written by the
// kernel).  start: nkept + 1 prefix sums of the kept words' counts, kword: their nkept list indices (table.hpp
// TableIndex), both on the device.  The caller has checked first + count <= start[nkept] and count <= cap.
hipError_t launch_prep_table(uint64_t first, uint32_t count, uint32_t nkept, const uint64_t* start,
                             const uint32_t* kword, const uint64_t* off, const uint8_t* bytes, const uint8_t* table,
                             uint32_t* mid, uint64_t* ids, uint32_t* counter, uint32_t cap, hipStream_t s);
// assoc_dev.hip: association candidates [first, first + count) (assoc.hpp) -> midstates in compacted slots, ids[slot] =
// the raw index, sref[slot] = the word offset of the net's salt entry for launch_pbkdf2_ms, and per verify class c
// (PMKID, keyver 1, 2, 3) the segments {line, slot, count} of the kept candidates against their own net's live lines:
// segcnt[c] counts them all, seg[c] holds the first segcap[c].  The counter and segcnt[0..4) are zeroed by the caller;
// it has checked first + count <= start[nidx] and count <= cap.
struct AssocEntry {
    uint32_t wfirst;  // the net's first entry in woff
    uint32_t nwords;  // W_n >= 1
    uint32_t net;     // index into net_line_off
    uint32_t sref;    // word offset of its ESSID's salt entry {nsalt, [2][nsalt][16]}
};
struct AssocLaunch {
    uint32_t nidx = 0;                 // nets that own indices
    const uint64_t* start = nullptr;   // nidx + 1 prefix sums of W_n x R
    const AssocEntry* ent = nullptr;   // nidx
    const uint64_t* woff = nullptr;    // entries + 1 byte offsets into wbytes
    const uint8_t* wbytes = nullptr;
    const uint32_t* roffs = nullptr;   // the rule image (RuleSet::flatten); nrules 0: the identity
    const uint32_t* rcode = nullptr;
    uint32_t nrules = 0;
    const uint32_t* net_line_off = nullptr;  // nets + 1 offsets into net_line
    const uint32_t* net_line = nullptr;      // live lines per net: table line | class index << 30
};
hipError_t launch_prep_assoc(const AssocLaunch& a, uint64_t first, uint32_t count, uint32_t minlen, uint32_t maxlen,
                             uint32_t* mid, uint64_t* ids, uint32_t* sref, uint32_t* counter, uint32_t cap,
                             SegDev* const seg[4], const uint32_t segcap[4], uint32_t* segcnt, hipStream_t s);
// hybrid_dev.hip: words [first_word, first_word + nwords) of off/bytes x mask candidates [mask_first, mask_first +
// mask_count), word-major, joined as word || mask or (mask_then_word) mask || word -> midstates in compacted slots;
// kept iff len <= 63 and minlen <= len + npos <= min(maxlen, 64); ids[slot] = word * keyspace + mask index.  The
// counter (zeroed by the caller) ends as the raw kept count, which may exceed cap.  nwords * mask_count < 2^32.
hipError_t launch_prep_hybrid(const uint8_t digits[64], const uint64_t* off, const uint8_t* bytes, uint64_t first_word,
                              uint32_t nwords, uint64_t mask_first, uint32_t mask_count, uint64_t keyspace,
                              uint32_t npos, bool mask_then_word, uint32_t minlen, uint32_t maxlen,
                              const uint8_t* table, uint32_t* mid, uint64_t* ids, uint32_t* counter, uint32_t cap,
                              hipStream_t s);
// combi_dev.hip: base words [first_base, first_base + nbase) of base_off/base_bytes x amplifier words [amp_first,
// amp_first + amp_count) of amp_off/amp_bytes, base-major, joined as base || amplifier or (amp_is_left) amplifier ||
// base -> midstates in compacted slots; kept iff both words <= 63 bytes and minlen <= L + R <= min(maxlen, 64);
// ids[slot] = base index * amp_words + amplifier index.  The counter (zeroed by the caller) ends as the raw kept
// count, which may exceed cap.  nbase * amp_count < 2^32.
hipError_t launch_prep_combinator(const uint64_t* base_off, const uint8_t* base_bytes, uint64_t first_base,
                                  uint32_t nbase, const uint64_t* amp_off, const uint8_t* amp_bytes, uint64_t amp_words,
                                  uint64_t amp_first, uint32_t amp_count, bool amp_is_left, uint32_t minlen,
                                  uint32_t maxlen, uint32_t* mid, uint64_t* ids, uint32_t* counter, uint32_t cap,
                                  hipStream_t s);
// chain_dev.hip: raw candidates [first, first + count) of a chain of 1..4 parts (lists in HBM and masks, chain.hpp),
// joined left to right -> midstates in compacted slots; kept iff every list word <= 63 bytes and minlen <= total
// length <= min(maxlen, 64); ids[slot] = the raw index.  The counter (zeroed by the caller) ends as the kept count.
// The caller has checked first + count <= K and count <= cap, and decomposed `first`: part p's digit (a list's word
// index, or a mask part's own index as its 64 position digits).
struct ChainPartLaunch {
    bool is_mask = false;
    const uint64_t* off = nullptr;   // list: radix + 1 byte offsets into bytes
    const uint8_t* bytes = nullptr;
    const uint8_t* table = nullptr;  // mask: the device copy of mask_table (mask.hpp)
    uint32_t npos = 0;               // mask: positions
    uint64_t radix = 0;              // a list's word count (< 2^32), a mask's keyspace; a ruled list's nwords * nrules
    uint64_t digit = 0;              // digit of `first` at this part, < radix
    uint8_t digits[64] = {};         // mask: mask_digits of `digit`
    // a ruled list (launch_prep_chain_rules only): the device image of its rule set (RuleSet::flatten); 0: no rules
    const uint32_t* roffs = nullptr;
    const uint32_t* rcode = nullptr;
    uint32_t nrules = 0;
};
hipError_t launch_prep_chain(const ChainPartLaunch* parts, uint32_t nparts, uint64_t first, uint32_t count,
                             uint32_t minlen, uint32_t maxlen, uint32_t* mid, uint64_t* ids, uint32_t* counter,
                             uint32_t cap, hipStream_t s);
// chain_rules_dev.hip: the same for a chain in which at least one list part carries rules: such a part's choices are
// the (rule, word) pairs, rule-major (choice = rule * nwords + word, radix = nwords * nrules < 2^32), its piece is
// rule_apply(word), and the <= 63 bytes test applies to that result; a choice the rule engine rejects drops the
// candidate.  Un-ruled parts, the filter, the ids and the counter are launch_prep_chain's.
hipError_t launch_prep_chain_rules(const ChainPartLaunch* parts, uint32_t nparts, uint64_t first, uint32_t count,
                                   uint32_t minlen, uint32_t maxlen, uint32_t* mid, uint64_t* ids, uint32_t* counter,
                                   uint32_t cap, hipStream_t s);
// product launch: issue-pass code object (pbkdf2_module.cpp); DWPA_PBKDF2_PLAIN=1 -> launch_pbkdf2_plain
// work (nullable): a 4-byte device counter the work-queue kernel may use (zeroed here before the launch)
hipError_t launch_pbkdf2(const uint32_t* mid, uint32_t cap, uint32_t base, uint32_t count, const uint32_t* counter,
                         const uint32_t* salt, uint32_t nsalt, uint32_t* pmk, hipStream_t s, uint32_t* work = nullptr);
hipError_t launch_pbkdf2_plain(const uint32_t* mid, uint32_t cap, uint32_t base, uint32_t count,
                               const uint32_t* counter, const uint32_t* salt, uint32_t nsalt, uint32_t* pmk,
                               hipStream_t s);
const char* pbkdf2_variant();
// Which PBKDF2 entry kernels this process has launched: one bit each, set by the launchers (a relaxed fetch_or per
// launch), read and optionally cleared through dwpa_debug_pbkdf2_kernels (engine.cpp; not part of the public ABI).
// A mask and not "the last kernel": crack_files launches from one worker thread per device.  The bit order is
// PBKDF2_KERNEL_NAMES in dwpa_amd/_lib.py.
enum Pbkdf2Kernel : uint32_t {
    PK_PLAIN = 1u << 0,          // k_pbkdf2
    PK_PLAIN_MS = 1u << 1,       // k_pbkdf2_ms
    PK_PLAIN_MG = 1u << 2,       // k_pbkdf2_mg
    PK_PLAIN_MS_TAIL = 1u << 3,  // k_pbkdf2_ms_tail
    PK_ONE = 1u << 4,            // k_pbkdf2_gfx950
    PK_MS = 1u << 5,             // k_pbkdf2_gfx950_ms
    PK_MG = 1u << 6,             // k_pbkdf2_gfx950_mg
    PK_ONE_P = 1u << 7,          // k_pbkdf2_gfx950_p
    PK_MS_P = 1u << 8,           // k_pbkdf2_gfx950_ms_p
    PK_MG_P = 1u << 9,           // k_pbkdf2_gfx950_mg_p
    PK_ONE_Q = 1u << 10,         // k_pbkdf2_gfx950_q
    PK_MG_Q = 1u << 11,          // k_pbkdf2_gfx950_mg_q
};
extern std::atomic<uint32_t> g_pbkdf2_kernels;
inline void note_pbkdf2_kernel(uint32_t bit) { g_pbkdf2_kernels.fetch_or(bit, std::memory_order_relaxed); }
// Which verify kernels this process has launched, the same way (dwpa_debug_verify_kernels): one bit per mode
// (key-parallel k_verify, attempt-parallel k_eapol_keys + k_verify_att) and instantiated class, so a test sees which
// verifier a line took.  The bit order is VERIFY_KERNEL_NAMES in dwpa_amd/_lib.py: the classes of DWPA_VC_DISPATCH
// (PMKID, keyver 1, 2, 3, 1|2, all) key-parallel, then the same attempt-parallel.
constexpr uint32_t VK_ATT_SHIFT = 6;
inline uint32_t verify_kernel_bit(uint32_t vc, bool att) {
    const uint32_t c = vc == VC_PMKID ? 0u : vc == VC_KV1 ? 1u : vc == VC_KV2 ? 2u : vc == VC_KV3 ? 3u
                       : vc == (VC_KV1 | VC_KV2) ? 4u : 5u;
    return 1u << (c + (att ? VK_ATT_SHIFT : 0u));
}
extern std::atomic<uint32_t> g_verify_kernels;
inline void note_verify_kernel(uint32_t vc, bool att) {
    g_verify_kernels.fetch_or(verify_kernel_bit(vc, att), std::memory_order_relaxed);
}
// PMKs that give every SIMD of the current device one PBKDF2 wave (two output-block lanes per PMK); 0 on error
uint32_t pbkdf2_wave_unit();
// many ESSIDs per launch: slot s uses the salt entry pool + sref[s] = {nsalt, [2][nsalt][16] words}
hipError_t launch_pbkdf2_ms(const uint32_t* mid, uint32_t cap, uint32_t count, const uint32_t* pool,
                            const uint32_t* sref, uint32_t* pmk, hipStream_t s);
hipError_t launch_pbkdf2_ms_plain(const uint32_t* mid, uint32_t cap, uint32_t count, const uint32_t* pool,
                                  const uint32_t* sref, uint32_t* pmk, hipStream_t s);
// attempt-parallel verification of EAPOL lists with >= ATT_PARALLEL_MIN attempts: lane = (key, attempt) item,
// segs[i].pad = first wave of segment i (ceil(count * natt / 64) waves each, nwaves in all), segs[i].count <= segk
// (1..64); keys = scratch of eapol_key_words(vc) x kstride words, kstride >= segk * nsegs
uint32_t eapol_key_words(uint32_t vc);
// first_hit (nullable): per line, the smallest key ordinal (ids[slot]: a job's keys numbered in input order, across
// all chunks of the call) with a hit so far (~0u: none); waves whose keys all come after it exit at once, and hits
// lower it (the check wants only the first key in input order).  Reset it once per call, not per chunk.
hipError_t launch_verify_att(const uint32_t* pmk, uint32_t cap, const uint64_t* ids, const SegDev* segs,
                             uint32_t nsegs, uint32_t nwaves, uint32_t* keys, uint32_t kstride, uint32_t segk,
                             const LineDev* lines, const uint32_t* pool, const AttDev* atts, HitDev* hits,
                             uint32_t* hitcnt, uint32_t hitcap, uint32_t* first_hit, uint32_t vc, hipStream_t s);
// many ESSID groups x one batch per launch (cap % 64 == 0): gsalt[c] = {salt word offset, nsalt} of chunk group c,
// PMK word k of (c, slot) at pmk[k * pstride + c * cap + slot]
hipError_t launch_pbkdf2_mg(const uint32_t* mid, uint32_t cap, const uint32_t* counter, uint32_t ngroups,
                            const uint32_t* salt, const uint32_t* gsalt, uint32_t* pmk, uint32_t pstride,
                            hipStream_t s, uint32_t* work = nullptr);
hipError_t launch_pbkdf2_mg_plain(const uint32_t* mid, uint32_t cap, const uint32_t* counter, uint32_t ngroups,
                                  const uint32_t* salt, const uint32_t* gsalt, uint32_t* pmk, uint32_t pstride,
                                  hipStream_t s);
// Check-path tail: PBKDF2 of slots [0, count) like launch_pbkdf2_ms_plain, at wave priority 0 until *flag != 0,
// then at `prio` (0 = never raised); every wave that raises itself adds 1 to *raised.  launch_set_flag sets the
// flag (queue it after the head).
hipError_t launch_pbkdf2_ms_tail(const uint32_t* mid, uint32_t cap, uint32_t count, const uint32_t* pool,
                                 const uint32_t* sref, uint32_t* pmk, uint32_t* flag, uint32_t prio,
                                 uint32_t* raised, hipStream_t s);
hipError_t launch_set_flag(uint32_t* flag, hipStream_t s);
constexpr uint32_t GATHER_CALLER = 0x80000000u;
hipError_t launch_gather_pmk(const uint32_t* upmk, uint32_t ucap, const uint32_t* cpmk, const uint32_t* src,
                             uint32_t n, uint32_t* pmk, uint32_t cap, hipStream_t s);
// out: host-mapped, >= 16 + hitcap * sizeof(HitDev) bytes (word 0 = hit count, word 1 = *raised or 0, HitDev
// records from byte 16)
hipError_t launch_hits_out(const uint32_t* hitcnt, const HitDev* hits, uint32_t hitcap, uint32_t* out,
                           const uint32_t* raised, hipStream_t s);
hipError_t launch_set_pmk(uint32_t* pmk, uint32_t cap, uint32_t slot, const uint32_t w[8], hipStream_t s);
hipError_t launch_verify(const uint32_t* pmk, uint32_t cap, const uint64_t* ids, const uint32_t* counter,
                         const SegDev* segs, uint32_t nsegs, uint32_t line_base, uint32_t nlines, const LineDev* lines,
                         const uint32_t* pool, const AttDev* atts, HitDev* hits, uint32_t* hitcnt, uint32_t hitcap,
                         uint32_t vc, hipStream_t s, const uint32_t* line_list = nullptr,
                         const uint32_t* line_poff = nullptr, uint32_t pstride = 0);

}  // namespace dwpa
