// crack.cpp -- dwpa_crack_files(): the in-process replacement of help_crack.py's hashcat subprocess
// (run_cracker, help_crack/help_crack.py:765-802; command line :773; rc handling :776-786; outfile parsed by
// get_key :804-879).
//
// Work distribution: the dictionary stream is cut into chunks; each chunk is split into contiguous, equal
// shards, one per active device, and every device thread scans its shard in batches (load -> per-ESSID PBKDF2 ->
// verify).  There is no device-to-device traffic: hits (a few bytes) are gathered on the host, where the first
// hit of each hashline is written to the outfile and the line is retired on every device (hashcat reports each
// hash once).  Rules (hashcat -r, help_crack.py:445-447,931-933) are applied on the GPU (rules.cpp).
// dwpa_crack_hybrid() (hashcat -a 6 / -a 7) is the same call with a mask amplifying every word where the rule set
// would: each word is joined with the mask's candidates on the GPU (hybrid_dev.hip).
// dwpa_crack_combinator() (hashcat -a 1) is the same call again with a second word list as the amplifier: it lies
// whole in device memory and every streamed word is joined with its words on the GPU (combi_dev.hip).
// The call frame -- checks, hash file, outfile, scan workers, retirement, hit reporting, statistics -- is the one all
// crack calls share (crack_common.hpp); what is here is the dictionary feed and the sizing of the loads.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "dwpa22000.h"
#include "crack_common.hpp"
#include "engine.hpp"
#include "m22000_host.hpp"
#include "dict_reader.hpp"
#include "rules.hpp"
#include "mask.hpp"

namespace dwpa {

// dwpa_crack_hybrid: the mask is the amplifier of every word, where the rule set is in a rules run.  valid = false:
// the mask or the mode was refused (the call fails after it has marked unreadable dictionaries).
struct HybridSpec {
    const Mask* mask = nullptr;
    int mode = 0;
    bool valid = false;
};

// dwpa_crack_combinator: one of the two lists is the amplifier of every word of the other (the base, which is
// streamed as a dictionary run streams its words).  The amplifier is read whole into host memory once: it is uploaded
// once per worker and kept here to rebuild a hit's PSK.  valid = false: the side was refused.
struct CombiSpec : HostList {      // the amplifier list, A words
    int side = DWPA_COMBI_AMP_RIGHT;
    bool valid = false;
    uint64_t below[65] = {};       // below[k]: amplifier words shorter than k bytes, k <= 64
    // A > batch: range_below[r * 65 + k] = amplifier words before index r * range that are shorter than k bytes
    std::vector<uint32_t> range_below;
    uint64_t range = 0;

    size_t base_index() const { return side == DWPA_COMBI_AMP_RIGHT ? 0 : 1; }  // of {left, right}
    // The amplifier words that a base word of L bytes keeps have lo..hi bytes (8 <= L + R <= 63); false: none can.
    static bool window(uint64_t L, uint32_t* lo, uint32_t* hi) {
        if (L > 63) return false;
        *lo = L < 8 ? 8 - (uint32_t)L : 0;
        *hi = 63 - (uint32_t)L;
        return true;
    }
    // kept pairs of a base word of L bytes x the whole amplifier: exact, from the amplifier's length histogram
    uint64_t kept(uint64_t L) const {
        uint32_t lo, hi;
        return window(L, &lo, &hi) ? below[hi + 1] - below[lo] : 0;
    }
    // ... x amplifier range r, [r * range, (r + 1) * range)
    uint64_t kept_in_range(uint64_t L, size_t r) const {
        uint32_t lo, hi;
        if (!window(L, &lo, &hi)) return 0;
        const uint32_t* p = &range_below[r * 65];
        return (uint64_t)(p[65 + hi + 1] - p[65 + lo]) - (p[hi + 1] - p[lo]);
    }
    void count_lengths() {
        uint64_t hist[65] = {};
        for (size_t i = 0; i + 1 < off.size(); i++) hist[std::min<uint64_t>(off[i + 1] - off[i], 64)]++;
        below[0] = 0;
        for (int k = 1; k <= 64; k++) below[k] = below[k - 1] + hist[k - 1];
    }
    void count_ranges(uint64_t cap) {
        range = cap;
        const uint64_t A = words();
        const size_t R = (size_t)((A + cap - 1) / cap);
        range_below.assign((R + 1) * 65, 0);
        uint32_t hist[65] = {};  // words so far, by length
        auto mark = [&](size_t r) {
            uint32_t* p = &range_below[r * 65];
            for (int k = 1; k <= 64; k++) p[k] = p[k - 1] + hist[k - 1];
        };
        for (uint64_t i = 0; i < A; i++) {
            if (i % cap == 0) mark((size_t)(i / cap));
            hist[std::min<uint64_t>(off[i + 1] - off[i], 64)]++;
        }
        mark(R);
    }
};

// What the sizing loops of scan_shard and scan_shard_combi have issued in this process (dwpa_debug_crack_loads, a test
// hook): device loads, loads that overflowed the batch and were repeated, loads that kept nothing, loads scanned.
static std::atomic<uint64_t> g_loads_issued{0}, g_loads_overflowed{0}, g_loads_empty{0}, g_loads_scanned{0};
static void count_load(std::atomic<uint64_t>& c) { c.fetch_add(1, std::memory_order_relaxed); }

// One shard worker (one per device, or DWPA_CRACK_SHARDS_PER_DEVICE per device).  Its stager thread uploads the
// next item into the free one of two buffer slots on the `up` stream while its scanner thread scans the other.
struct DevWork : ScanWorker {
    DevRules rules;
    DevBuf off[2], bytes[2];
    DevBuf amp_off, amp_bytes;      // dwpa_crack_combinator: the amplifier list, uploaded once
    std::vector<uint64_t> hoff[2];  // host staging of the rebased offsets (alive until the upload completes)
    hipStream_t up = nullptr;
    hipEvent_t staged[2] = {nullptr, nullptr};
    double keep = 1.0;              // surviving candidates per (word x rule), carried from item to item
    size_t words = 0;               // of the items scanned (DWPA_TRACE, dwpa_crack_last_stats)
    double wait_s = 0;              // scanner time spent waiting for a staged item
    // stager -> scanner hand-over
    std::mutex mu;
    std::condition_variable cv;
    WorkItem slot_item[2];
    bool slot_full[2] = {false, false};
    std::deque<int> ready;
    bool staging_done = false;
};

// Upload words [b, e) of chunk c (offsets rebased to the item) into slot `slot` of worker w.
static int stage_shard(DevWork& w, const Chunk& c, size_t b, size_t e, int slot) {
    if (hipSetDevice(w.device) != hipSuccess) return DWPA_E_HIP;
    std::vector<uint64_t>& off = w.hoff[slot];
    off.resize(e - b + 1);
    for (size_t i = b; i <= e; i++) off[i - b] = c.off[i] - c.off[b];
    const size_t nbytes = c.off[e] - c.off[b];
    DevBuf& ob = w.off[slot];
    DevBuf& bb = w.bytes[slot];
    if ((ob.n < off.size() * 8 && ob.ensure(off.size() * 8 * 3 / 2)) || (bb.n < nbytes + 64 && bb.ensure((nbytes + 64) * 3 / 2)))
        return DWPA_E_NOMEM;
    if (hipMemcpyAsync(ob.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, w.up) != hipSuccess ||
        (nbytes && hipMemcpyAsync(bb.p, c.bytes.data() + c.off[b], nbytes, hipMemcpyHostToDevice, w.up) != hipSuccess) ||
        hipEventRecord(w.staged[slot], w.up) != hipSuccess || hipStreamSynchronize(w.up) != hipSuccess)
        return DWPA_E_HIP;
    return 0;
}

// A mask wider than the batch: one word x consecutive mask ranges of a batch each.  Whether a word survives the
// 8..63 filter follows from its length alone, so a dropped word costs no launch.  Each word is loaded as word 0 of
// the offsets from its own entry on: the ids are then the mask indices, whatever words * K would come to.
static int scan_shard_wide(DevWork& w, CrackShared& sh, const Chunk& c, size_t b, size_t e, const HybridSpec& hy,
                           int slot) {
    const uint32_t cap = scan_batch_cap(w.scan);
    const uint64_t K = hy.mask->keyspace;
    const uint32_t P = hy.mask->npos;
    std::vector<HitDev> hits;
    for (size_t wi = b; wi < e; wi++) {
        const uint64_t L = c.off[wi + 1] - c.off[wi];
        if (L > 63 || L + P < 8 || L + P > 63) continue;
        for (uint64_t mf = 0; mf < K && !sh.stop.load(std::memory_order_relaxed); mf += cap) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(cap, K - mf);
            int r;
            if ((r = scan_load_hybrid(w.scan, (const uint64_t*)w.off[slot].p + (wi - b), (const uint8_t*)w.bytes[slot].p,
                                      0, 1, mf, n, hy.mode, 8, 63, w.stream)) < 0)
                return r;
            r = scan_step(w, sh, hits, [&](uint64_t cand, std::string* plain) {
                if (cand >= K) return false;
                uint8_t m[64];
                mask_candidate(*hy.mask, cand, m);
                const std::string word(c.bytes.data() + c.off[wi], (size_t)L), ms((const char*)m, P);
                *plain = hy.mode == DWPA_HYBRID_WORD_MASK ? word + ms : ms + word;
                return true;
            });
            if (r < 0) return r;
            w.cands += n;
        }
        if (sh.stop.load(std::memory_order_relaxed)) break;
    }
    return 0;
}

// More rules than the batch: one word's results no longer fit a load, so the sizing loop has nothing to size (it
// gave up with DWPA_E_OVERFLOW, and past 16 batches of rules rules_load refused the load).  As scan_shard_wide does
// for a mask: one word x consecutive rule ranges of a batch each.  A word the rule engine refuses (empty, or longer
// than its 256 bytes) costs no launch, a range that keeps nothing no scan.  The ids stay word * nrules + rule.
static int scan_shard_rules_wide(DevWork& w, CrackShared& sh, const Chunk& c, size_t b, size_t e, const RuleSet& rules,
                                 int slot) {
    const uint32_t cap = scan_batch_cap(w.scan);
    const uint64_t nrules = rules.size();
    std::vector<HitDev> hits;
    for (size_t wi = b; wi < e; wi++) {
        const uint64_t L = c.off[wi + 1] - c.off[wi];
        if (L < 1 || L > (uint64_t)RP_PASSWORD_SIZE) continue;
        for (uint64_t rf = 0; rf < nrules && !sh.stop.load(std::memory_order_relaxed); rf += cap) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(cap, nrules - rf);
            int r;
            if ((r = rules_load(w.scan, &w.rules, (const uint64_t*)w.off[slot].p, (const uint8_t*)w.bytes[slot].p,
                                wi - b, 1, w.stream, false, (uint32_t)rf, n)) < 0)
                return r;
            uint32_t raw = 0;
            if ((r = scan_counter_raw(w.scan, w.stream, &raw)) < 0) return r;
            if (raw > n) return DWPA_E_OVERFLOW;  // cannot happen: one word x n <= batch rules
            if (raw == 0) continue;
            r = scan_step(w, sh, hits, [&](uint64_t cand, std::string* plain) {
                if (cand / nrules != wi - b) return false;
                plain->assign(c.bytes.data() + c.off[wi], (size_t)L);
                return rules.apply_host((size_t)(cand % nrules), *plain, plain);
            });
            if (r < 0) return r;
            w.cands += raw;
        }
        if (sh.stop.load(std::memory_order_relaxed)) break;
    }
    return 0;
}

// A combinator run's item: base words [b, e) of chunk c x the worker's amplifier list.  Nothing is sized by trial:
// the host knows every length, so the kept pairs of a load follow from the amplifier's length counts (CombiSpec).
//   A <= batch: nw whole base words x the whole amplifier, nw the most whose kept pairs fit the batch (and whose raw
//               pairs fit a fill-mode load).  The kernel's own count is read back and must agree.
//   A >  batch: one base word x consecutive amplifier ranges of a batch, as scan_shard_wide does; a word or a range
//               that keeps no pair costs no launch.  The word is loaded as word 0 from its own offset, so the ids
//               are the amplifier indices.
static int scan_shard_combi(DevWork& w, CrackShared& sh, const Chunk& c, size_t b, size_t e, const CombiSpec& cb,
                            int slot) {
    const uint32_t cap = scan_batch_cap(w.scan);
    const uint64_t A = cb.words();
    if (A == 0) return 0;
    const uint64_t* boff = (const uint64_t*)w.off[slot].p;
    const uint8_t* bbytes = (const uint8_t*)w.bytes[slot].p;
    const uint64_t* aoff = (const uint64_t*)w.amp_off.p;
    const uint8_t* abytes = (const uint8_t*)w.amp_bytes.p;
    auto len_of = [&](size_t wi) { return c.off[wi + 1] - c.off[wi]; };
    auto join = [&](size_t wi, uint64_t ai, std::string* plain) {
        const std::string base(c.bytes.data() + c.off[wi], (size_t)len_of(wi));
        const std::string amp(cb.bytes.data() + cb.off[ai], (size_t)(cb.off[ai + 1] - cb.off[ai]));
        *plain = cb.side == DWPA_COMBI_AMP_LEFT ? amp + base : base + amp;
    };
    std::vector<HitDev> hits;
    int r;
    if (A > cap) {
        const size_t R = (size_t)((A + cap - 1) / cap);
        for (size_t wi = b; wi < e && !sh.stop.load(std::memory_order_relaxed); wi++) {
            if (cb.kept(len_of(wi)) == 0) continue;
            for (size_t ri = 0; ri < R && !sh.stop.load(std::memory_order_relaxed); ri++) {
                const uint64_t kept = cb.kept_in_range(len_of(wi), ri);
                if (kept == 0) continue;
                const uint64_t af = (uint64_t)ri * cap;
                const uint32_t n = (uint32_t)std::min<uint64_t>(cap, A - af);
                if ((r = scan_load_combinator(w.scan, boff + (wi - b), bbytes, 0, 1, aoff, abytes, A, af, n, cb.side, 8,
                                              63, w.stream)) < 0)
                    return r;
                r = scan_step(w, sh, hits, [&](uint64_t cand, std::string* plain) {
                    if (cand >= A) return false;
                    join(wi, cand, plain);
                    return true;
                });
                if (r < 0) return r;
                w.cands += kept;
            }
        }
        return 0;
    }
    const uint64_t most = std::min<uint64_t>(16ull * cap, UINT32_MAX) / A;  // raw pairs of a fill-mode load; >= 16
    const size_t words = e - b;
    for (size_t wb = 0; wb < words && !sh.stop.load(std::memory_order_relaxed);) {
        uint32_t nw = 0;
        uint64_t kept = 0;
        for (; wb + nw < words && nw < most; nw++) {  // one word keeps at most A <= cap pairs: nw >= 1
            const uint64_t k = cb.kept(len_of(b + wb + nw));
            if (kept + k > cap) break;
            kept += k;
        }
        count_load(g_loads_issued);
        if (kept == 0) {
            count_load(g_loads_empty);
            wb += nw;
            continue;
        }
        if ((r = scan_load_combinator(w.scan, boff, bbytes, wb, nw, aoff, abytes, A, 0, (uint32_t)A, cb.side, 8, 63,
                                      w.stream, true)) < 0)
            return r;
        uint32_t raw = 0;
        if ((r = scan_counter_raw(w.scan, w.stream, &raw)) < 0) return r;
        if (raw != kept) {  // a guard, not the mechanism: the two counts follow from the same lengths
            fprintf(stderr, "[dwpa] combinator load kept %u pairs where the lengths give %llu\n", raw,
                    (unsigned long long)kept);
            return DWPA_E_OVERFLOW;
        }
        r = scan_step(w, sh, hits, [&](uint64_t cand, std::string* plain) {
            const uint64_t word = cand / A - wb, ai = cand % A;
            if (word >= nw) return false;
            join(b + wb + word, ai, plain);
            return true;
        });
        if (r < 0) return r;
        count_load(g_loads_scanned);
        wb += nw;
        w.cands += kept;
    }
    return 0;
}

static int scan_shard(DevWork& w, CrackShared& sh, const Chunk& c, size_t b, size_t e, const RuleSet* rules,
                      const HybridSpec* hy, const CombiSpec* cb, int slot) {
    if (e <= b) return 0;
    if (hipSetDevice(w.device) != hipSuccess) return DWPA_E_HIP;
    if (hipStreamWaitEvent(w.stream, w.staged[slot], 0) != hipSuccess) return DWPA_E_HIP;
    if (cb) return scan_shard_combi(w, sh, c, b, e, *cb, slot);
    const DevBuf& woff = w.off[slot];
    const DevBuf& wbytes = w.bytes[slot];
    const uint32_t cap = scan_batch_cap(w.scan);
    const size_t words = e - b;
    if (hy && hy->mask->keyspace > cap) return scan_shard_wide(w, sh, c, b, e, *hy, slot);
    if (!hy && rules && rules->size() > cap) return scan_shard_rules_wide(w, sh, c, b, e, *rules, slot);
    // a hybrid run's amplifier is its mask: K candidates per word where a rules run has nrules
    const uint64_t nrules = hy ? hy->mask->keyspace : rules ? rules->size() : 1;
    // candidate id = word * nrules + rule; batches walk the candidate space in order.  Every PBKDF2 lane runs the
    // same 4096 iterations, so a batch costs ceil(candidates / 256K) wave rounds whatever its fill: the words per
    // batch follow the observed fraction of candidates that survive the 8..63 filter (and the rules), aiming at
    // 99.5 % of the batch.  A load that overflows the batch (the compaction drops and counts the excess) is
    // repeated with fewer words before anything is derived.
    double& keep = w.keep;
    std::vector<HitDev> hits;
    for (size_t wb = 0; wb < words && !sh.stop.load(std::memory_order_relaxed);) {
        // keep == 1 (nothing filtered so far): exactly one batch of candidates, which cannot overflow
        const double want = (keep >= 1.0 ? 1.0 : 0.995) * cap / ((double)nrules * keep);
        // kernel-side bound on a fill-mode load (a hybrid load also stays below 2^32 lanes)
        const uint64_t most = (hy ? std::min<uint64_t>(16ull * cap, UINT32_MAX) : 16ull * cap) / nrules;
        const uint32_t nw = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)want, most, words - wb}));
        int r;
        if (hy)
            r = scan_load_hybrid(w.scan, (const uint64_t*)woff.p, (const uint8_t*)wbytes.p, wb, nw, 0,
                                 (uint32_t)nrules, hy->mode, 8, 63, w.stream, true);
        else if (rules)
            r = rules_load(w.scan, &w.rules, (const uint64_t*)woff.p, (const uint8_t*)wbytes.p, wb, nw, w.stream, true);
        else
            r = scan_load_dict(w.scan, (const uint64_t*)woff.p, (const uint8_t*)wbytes.p, wb, nw, 8, 63, w.stream,
                               true);
        if (r < 0) return r;
        count_load(g_loads_issued);
        uint32_t raw = 0;
        if ((r = scan_counter_raw(w.scan, w.stream, &raw)) < 0) return r;
        const double seen = (double)raw / ((double)nw * nrules);
        if (raw > cap) {  // overflow: nothing derived yet, retry these words in a smaller batch
            if (nw == 1) return DWPA_E_OVERFLOW;
            count_load(g_loads_overflowed);
            keep = std::max(seen, keep * 1.05);
            continue;
        }
        if (raw > 0) keep = std::min(1.0, std::max(0.01, seen));
        if (raw == 0) {
            count_load(g_loads_empty);
            wb += nw;
            continue;
        }
        r = scan_step(w, sh, hits, [&](uint64_t cand, std::string* plain) {
            const uint64_t word = cand / nrules, rule = cand % nrules;
            plain->assign(c.bytes.data() + c.off[b + word], c.off[b + word + 1] - c.off[b + word]);
            if (hy) {
                uint8_t m[64];
                mask_candidate(*hy->mask, rule, m);
                const std::string ms((const char*)m, hy->mask->npos);
                *plain = hy->mode == DWPA_HYBRID_WORD_MASK ? *plain + ms : ms + *plain;
                return true;
            }
            return !rules || rules->apply_host((size_t)rule, *plain, plain);  // false cannot happen: the GPU kept it
        });
        if (r < 0) return r;
        count_load(g_loads_scanned);
        wb += nw;
        w.cands += raw;
    }
    return 0;
}

static bool trace_on() {
    const char* e = getenv("DWPA_TRACE");
    return e && *e == '1';
}

static int crack_impl(const char* hash_file, const char* const* dicts, size_t ndicts, const char* rules_file, int nec,
                      const char* out_file, const dwpa_config* cfg, int32_t* dict_status,
                      const HybridSpec* hy = nullptr, CombiSpec* cb = nullptr) {
    CrackCall call;
    if (dict_status)
        for (size_t i = 0; i < ndicts; i++) dict_status[i] = DWPA_DICT_OK;
    if (!hash_file || !out_file || (!dicts && ndicts)) return DWPA_RC_ERROR;
    if (!crack_check_args(cfg, nec)) return DWPA_RC_ERROR;
    // hashcat refuses to start when a wordlist cannot be opened; so does this call, before touching a device, and it
    // names the file (DWPA_E_IO in dict_status): a deterministic input error, which help_crack's drop-in does not retry
    bool unreadable = false;
    for (size_t i = 0; i < ndicts; i++) {
        FILE* f = dicts[i] ? fopen(dicts[i], "rb") : nullptr;
        if (!f) {
            unreadable = true;
            if (dict_status) dict_status[i] = DWPA_E_IO;
            fprintf(stderr, "[dwpa] dictionary %s: cannot be opened\n", dicts[i] ? dicts[i] : "(null)");
        } else {
            fclose(f);
        }
    }
    if (unreadable || (hy && !hy->valid) || (cb && !cb->valid)) return DWPA_RC_ERROR;
    if (cb) {  // dicts = {left, right}: the amplifier is read whole, before any device is touched
        FILE* f = fopen(hash_file, "rb");
        if (!f) return DWPA_RC_ERROR;
        fclose(f);
        const size_t ai = 1 - cb->base_index();
        const int r = read_list(dicts[ai], cb);
        if (r == DWPA_E_OVERFLOW) {
            fprintf(stderr, "[dwpa] list %s: too large to be the amplifier (at most %llu bytes of text and offsets, "
                            "fewer than 2^32 words); take the other list with amp_side %d (--amplifier %s)\n",
                    dicts[ai], (unsigned long long)DWPA_COMBI_AMP_MAX_BYTES,
                    cb->side == DWPA_COMBI_AMP_RIGHT ? DWPA_COMBI_AMP_LEFT : DWPA_COMBI_AMP_RIGHT,
                    cb->side == DWPA_COMBI_AMP_RIGHT ? "left" : "right");
            return DWPA_RC_ERROR;
        }
        if (r < 0) {
            if (dict_status) dict_status[ai] = DWPA_E_IO;
            fprintf(stderr, "[dwpa] dictionary %s: read error\n", dicts[ai]);
            return DWPA_RC_ERROR;
        }
        cb->count_lengths();
    }
    CrackPlan plan;
    if (!crack_plan(cfg, nec, &plan)) return DWPA_RC_ERROR;
    CrackShared sh;
    HashLines hl;
    if (!sh.load_hashes(hash_file, &hl)) return DWPA_RC_ERROR;

    // hashcat -r: lines that do not parse -- and, in the default DWPA_RULES_HASHCAT mode, lines using reject or
    // memory functions, which hashcat's -r loader skips too -- are skipped with a message each (RuleSet::add_line)
    // and counted in dwpa_crack_last_stats; a file with no rule left fails the call, as hashcat refuses to start
    RuleSet rules;
    const int want = DWPA_CFG_HAS(cfg, rule_mode) ? cfg->rule_mode : DWPA_RULES_DEFAULT;
    if (want != DWPA_RULES_DEFAULT && want != DWPA_RULES_HASHCAT && want != DWPA_RULES_FULL) return DWPA_RC_ERROR;
    rules.mode = want == DWPA_RULES_DEFAULT ? engine_rule_mode() : want;
    const RuleSet* rp = nullptr;
    if (rules_file) {
        const int lr = rules.load_file(rules_file);
        call.st.rules = (uint32_t)rules.size();
        call.st.rules_skipped = (uint32_t)rules.skipped.size();
        call.st.rules_rejmem = rules.rejmem;
        crack_publish_stats(call.st, {});  // whatever becomes of the call
        if (lr < 0) return DWPA_RC_ERROR;
        if (!rules.all_noop()) rp = &rules;
    }

    if (!sh.open_out(out_file)) return DWPA_RC_ERROR;

    const uint32_t batch = plan.batch;
    std::vector<std::unique_ptr<DevWork>> work;
    int rc = 0;
    for (int dev : plan.devs)
        for (size_t k = 0; k < plan.shards && rc >= 0; k++) {
            work.push_back(std::make_unique<DevWork>());
            DevWork& w = *work.back();
            rc = scan_worker_open(w, dev, hl, plan);
            if (rc >= 0 && (hipStreamCreateWithFlags(&w.up, hipStreamNonBlocking) != hipSuccess ||
                            hipEventCreateWithFlags(&w.staged[0], hipEventDisableTiming) != hipSuccess ||
                            hipEventCreateWithFlags(&w.staged[1], hipEventDisableTiming) != hipSuccess))
                rc = DWPA_E_HIP;
            if (rc >= 0 && rp) rc = rules_upload(dev, rules, &w.rules);
            if (rc >= 0 && hy) rc = scan_set_mask(w.scan, *hy->mask);
            if (rc >= 0 && cb) rc = upload_list(*cb, &w.amp_off, &w.amp_bytes);
        }
    const size_t G = work.size();
    if (rc >= 0 && cb && cb->words() > scan_batch_cap(work[0]->scan)) cb->count_ranges(scan_batch_cap(work[0]->scan));

    // the streamed dictionaries: all of them, or a combinator run's base list (dmap: their places in dicts)
    std::vector<std::string> dpaths;
    std::vector<size_t> dmap;
    for (size_t i = 0; i < ndicts; i++)
        if (!cb || i == cb->base_index()) {
            dpaths.push_back(dicts[i]);
            dmap.push_back(i);
        }
    // Items: the first is 1/16 of a batch of candidates (a device starts after ~1M words have been read, not a
    // whole 16M-word batch: on a dictionary's first pass that read took ~0.5 s of a 21 s C2 pass), doubling to
    // 16 batches (a partial last batch per item then costs ~1 % of its wave rounds).  The reader's chunks start at
    // one item per worker and grow to two full items per worker, so reading stays ahead of the scans without
    // holding much more than that in memory.
    // A hybrid run divides by its mask's keyspace K: K = 1 sizes items as a plain dictionary run does; K above the
    // batch makes every item one word (first_item = most_item = 1), which is K / batch launches.
    // A combinator run divides by its amplifier's word count A in the same way.
    const size_t nr = cb ? std::max<size_t>(1, (size_t)cb->words()) : hy ? (size_t)hy->mask->keyspace : rp ? rp->size() : 1;
    const size_t first_item = std::max<size_t>(1, batch / nr / 16), most_item = std::max<size_t>(1, 16 * (size_t)batch / nr);
    ChunkSource source(dpaths, first_item * G, 2 * most_item * G);
    // several workers: items of at most 2 batches, so an item handed out just before the readers reach the end
    // cannot outlast the balanced tail by more than that
    ItemQueue items(source, first_item, G > 1 ? std::min(most_item, std::max<size_t>(first_item, 2 * (size_t)batch / nr))
                                              : most_item, G);
    const auto t0 = std::chrono::steady_clock::now();

    auto stop_all = [&]() {
        sh.stop = true;
        source.cancel();  // a stager blocked on the reader returns at once
        for (auto& wp : work) {
            std::lock_guard<std::mutex> lk(wp->mu);
            wp->cv.notify_all();
        }
    };
    auto fail = [&](int r) {
        sh.fail(r);
        stop_all();
    };
    std::vector<std::thread> th;
    // A worker thread that cannot start (std::system_error, e.g. under RLIMIT_NPROC) stops the ones that did and
    // fails the call; the vector never unwinds with joinable threads in it.
    if (rc >= 0) try {
        for (size_t k = 0; k < G; k++) {
            th.emplace_back([&, k] {  // stager
                DevWork& w = *work[k];
                for (int slot = 0;; slot ^= 1) {
                    {
                        std::unique_lock<std::mutex> lk(w.mu);
                        w.cv.wait(lk, [&] { return !w.slot_full[slot] || sh.stop; });
                    }
                    WorkItem it;
                    if (sh.stop || !items.next(it)) break;
                    const int r = guarded([&] { return stage_shard(w, *it.chunk, it.b, it.e, slot); });
                    if (r < 0) {
                        fail(r);
                        break;
                    }
                    std::lock_guard<std::mutex> lk(w.mu);
                    w.slot_item[slot] = std::move(it);
                    w.slot_full[slot] = true;
                    w.ready.push_back(slot);
                    w.cv.notify_all();
                }
                std::lock_guard<std::mutex> lk(w.mu);
                w.staging_done = true;
                w.cv.notify_all();
            });
            th.emplace_back([&, k] {  // scanner
                DevWork& w = *work[k];
                for (;;) {
                    int slot;
                    WorkItem it;
                    {
                        const auto tw = std::chrono::steady_clock::now();
                        std::unique_lock<std::mutex> lk(w.mu);
                        w.cv.wait(lk, [&] { return !w.ready.empty() || w.staging_done || sh.stop; });
                        w.wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count();
                        if (w.ready.empty() || sh.stop) break;
                        slot = w.ready.front();
                        w.ready.pop_front();
                        it = w.slot_item[slot];
                    }
                    const auto ts = std::chrono::steady_clock::now();
                    const int r = guarded([&] { return scan_shard(w, sh, *it.chunk, it.b, it.e, rp, hy, cb, slot); });
                    w.scan_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - ts).count();
                    w.items++;
                    w.words += it.e - it.b;
                    {
                        std::lock_guard<std::mutex> lk(w.mu);
                        w.slot_item[slot] = WorkItem();
                        w.slot_full[slot] = false;
                        w.cv.notify_all();
                    }
                    if (r < 0) {
                        fail(r);
                        break;
                    }
                    if (sh.stop) {
                        stop_all();
                        break;
                    }
                }
            });
        }
    } catch (...) {
        fail(DWPA_E_NOMEM);
    }
    for (auto& t : th) t.join();
    source.finish();
    const bool ioerr = items.io_error();
    const std::vector<int> fst = source.file_status();
    for (size_t k = 0; k < dmap.size(); k++) {
        const size_t i = dmap[k];
        if (fst[k] == ChunkSource::FILE_DAMAGED)
            fprintf(stderr, "[dwpa] dictionary %s: damaged gzip stream (truncated or corrupt); scanned up to the damage, "
                            "as hashcat's gzread does\n", dicts[i]);
        else if (fst[k] == ChunkSource::FILE_UNREADABLE)
            fprintf(stderr, "[dwpa] dictionary %s: read error\n", dicts[i]);
        if (dict_status)
            dict_status[i] = fst[k] == ChunkSource::FILE_DAMAGED ? DWPA_DICT_DAMAGED
                             : fst[k] == ChunkSource::FILE_UNREADABLE ? DWPA_E_IO : DWPA_DICT_OK;
    }
    if (cb && cb->damaged) {
        const size_t ai = 1 - cb->base_index();
        fprintf(stderr, "[dwpa] dictionary %s: damaged gzip stream (truncated or corrupt); joined up to the damage\n",
                dicts[ai]);
        if (dict_status) dict_status[ai] = DWPA_DICT_DAMAGED;
    }
    if (trace_on()) {
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[dwpa] crack dictionary cache: %zu files replayed from memory so far\n", DictCache::get().hits());
        for (size_t k = 0; k < G; k++)
            fprintf(stderr, "[dwpa] crack worker %zu (device %d): %zu items, %zu words, %.3f s waiting for input of %.3f s\n",
                    k, work[k]->device, work[k]->items, work[k]->words, work[k]->wait_s, el);
    }
    std::vector<dwpa_crack_worker> wst;
    for (auto& wp : work) {
        DevWork& w = *wp;
        scan_worker_close(w);  // waits for the device: the worker's buffers are free after it
        for (int q = 0; q < 2; q++) {
            w.off[q].release();
            w.bytes[q].release();
            if (w.staged[q]) (void)hipEventDestroy(w.staged[q]);
        }
        w.amp_off.release();
        w.amp_bytes.release();
        rules_release(&w.rules);
        if (w.up) (void)hipStreamDestroy(w.up);
        wst.push_back(dwpa_crack_worker{w.device, (uint32_t)w.items, (uint64_t)w.words, w.cands, w.wait_s, w.scan_s});
    }
    return call.finish(sh, wst, rc < 0 || ioerr);
}

// `hashcat --stdout -r rules_file sources... -o out_path` (help_crack.py:508 expandcracked, :575 prdict): the words
// of the sources (plain or gzip, one per line, $HEX[] decoded, as hashcat reads wordlists) x every rule, expanded on
// the GPU in sub-batches of ~1M candidates (k_rules_expand into 256-byte slots), and packed on the GPU too
// (k_text_*: a scan of every candidate's text length, then each candidate copied to its offset): word-major order,
// rejected candidates skipped, raw bytes and '\n' as hashcat's --stdout writes them, $HEX[..] for a candidate holding
// '\n' or '\r'.  Only the packed text (~14 bytes per candidate) crosses PCIe -- round 4 copied the 256-byte slots
// back (189 GB for 740M candidates) and packed them on one host thread.  Two sets on two streams: the GPU expands and
// packs sub-batch i+1 while the host writes sub-batch i.
static int rules_expand_file_impl(int device, const char* rules_file, const char* const* sources, size_t nsources,
                                  const char* out_path, int gzip_level, uint64_t* words_out, uint64_t* cands_out) {
    if (!rules_file || !out_path || (!sources && nsources)) return DWPA_E_ARG;
    for (size_t i = 0; i < nsources; i++) {
        FILE* f = sources[i] ? fopen(sources[i], "rb") : nullptr;
        if (!f) return DWPA_E_IO;
        fclose(f);
    }
    RuleSet rs;
    rs.mode = engine_rule_mode();
    int rc = rs.load_file(rules_file);
    if (rc < 0) return rc;
    if ((rc = engine_init()) < 0) return rc;
    if (hipSetDevice(device) != hipSuccess) return DWPA_E_NODEV;
    FILE* fo = nullptr;
    gzFile gz = nullptr;
    if (gzip_level > 0) {
        char mode[8];
        snprintf(mode, sizeof mode, "wb%d", std::min(9, gzip_level));
        gz = gzopen(out_path, mode);
        if (!gz) return DWPA_E_IO;
        gzbuffer(gz, 1 << 20);
    } else if (!(fo = fopen(out_path, "wb"))) {
        return DWPA_E_IO;
    }
    // The text packer's offsets and totals are 32-bit: one word's candidates (nr of them, at most TEXT_MAX bytes each
    // as $HEX[..]) must fit 4 GiB, which bounds a rules file here to ~8.27M rules (bestWPA.rule has 145).
    constexpr size_t TEXT_MAX = 5 + 2 * (size_t)RP_PASSWORD_SIZE + 2;
    if (rs.size() > (size_t)UINT32_MAX / TEXT_MAX) {
        fprintf(stderr, "[dwpa] %zu rules: more than the %zu one expansion packs\n", rs.size(), (size_t)UINT32_MAX / TEXT_MAX);
        return DWPA_E_RULE;
    }
    DevRules dr;
    rc = rules_upload(device, rs, &dr);
    const size_t nr = rs.size();
    const size_t wpb = std::max<size_t>(1, (1u << 20) / nr);  // words per sub-batch: ~1M candidate slots
    const size_t ncap = wpb * nr;
    const size_t nblk = text_pack_blocks((uint32_t)ncap);
    struct Set {
        DevBuf off, bytes, out, len, tlen, bsum, bcnt, tot, text;
        uint32_t* h_tot = nullptr;  // pinned: text bytes, kept candidates
        uint8_t* h_text = nullptr;  // pinned, h_cap bytes (== text.n)
        size_t h_cap = 0;
        hipStream_t s = nullptr;
        hipEvent_t done = nullptr, up = nullptr;  // expansion + pack done and totals copied back / inputs uploaded
        std::vector<uint64_t> hoff;
        size_t words = 0;  // words of the sub-batch
        bool busy = false;
        int grow(size_t want) {  // device text buffer and its pinned host mirror, both `want` bytes
            pinned_free(h_text, h_cap);
            h_text = nullptr;
            h_cap = 0;
            if (text.ensure(want) || pinned_alloc((void**)&h_text, want) < 0) return DWPA_E_NOMEM;
            h_cap = want;
            return 0;
        }
    } set[2];
    for (Set& S : set) {
        if (rc < 0) break;
        if (S.out.ensure(ncap * 256) || S.len.ensure(ncap * 4) || S.tlen.ensure(ncap * 4) ||
            S.off.ensure((wpb + 1) * 8) || S.bsum.ensure(nblk * 4) || S.bcnt.ensure(nblk * 4) || S.tot.ensure(8) ||
            S.grow(ncap * 24) || pinned_alloc((void**)&S.h_tot, 8) < 0)
            rc = DWPA_E_NOMEM;
        else if (hipStreamCreateWithFlags(&S.s, hipStreamNonBlocking) != hipSuccess ||
                 hipEventCreateWithFlags(&S.done, hipEventDisableTiming) != hipSuccess ||
                 hipEventCreateWithFlags(&S.up, hipEventDisableTiming) != hipSuccess)
            rc = DWPA_E_HIP;
    }
    uint64_t words = 0, cands = 0;
    auto pack = [&](Set& S) -> int {  // pack S's expansion into its text buffer, copy the totals back
        const uint32_t n = (uint32_t)(S.words * nr);
        if (launch_text_pack((const uint8_t*)S.out.p, (const uint32_t*)S.len.p, (const uint32_t*)S.tlen.p, n,
                             (uint32_t*)S.bsum.p, (uint32_t*)S.bcnt.p, (uint32_t*)S.tot.p, (uint8_t*)S.text.p, S.h_cap,
                             S.s) != hipSuccess ||
            hipMemcpyAsync(S.h_tot, S.tot.p, 8, hipMemcpyDeviceToHost, S.s) != hipSuccess ||
            hipEventRecord(S.done, S.s) != hipSuccess)
            return DWPA_E_HIP;
        return 0;
    };
    auto drain = [&](Set& S) -> int {  // wait for S's text, copy it back and write it
        if (!S.busy) return 0;
        S.busy = false;
        if (hipEventSynchronize(S.done) != hipSuccess) return DWPA_E_HIP;
        size_t bytes = S.h_tot[0];
        if (bytes > S.h_cap) {  // longer candidates than budgeted: a bigger buffer, and the same slots packed again
            if (S.grow(bytes + bytes / 4) < 0) return DWPA_E_NOMEM;
            int r = pack(S);
            if (r < 0) return r;
            if (hipEventSynchronize(S.done) != hipSuccess) return DWPA_E_HIP;
            bytes = S.h_tot[0];
        }
        if (bytes && (hipMemcpyAsync(S.h_text, S.text.p, bytes, hipMemcpyDeviceToHost, S.s) != hipSuccess ||
                      hipStreamSynchronize(S.s) != hipSuccess))
            return DWPA_E_HIP;
        cands += S.h_tot[1];
        const size_t put = gz ? (size_t)gzwrite(gz, S.h_text, (unsigned)bytes) : fwrite(S.h_text, 1, bytes, fo);
        return put == bytes ? 0 : DWPA_E_IO;
    };
    if (rc >= 0) {
        std::vector<std::string> paths(sources, sources + nsources);
        DictReader reader(paths);
        Chunk c;
        bool err = false;
        int cur = 0;
        auto uploads_done = [&]() {  // the chunk's bytes may change only when no upload still reads them
            for (Set& S : set)
                if (S.busy && hipEventSynchronize(S.up) != hipSuccess) return false;
            return true;
        };
        while (rc >= 0 && uploads_done() && reader.next(c, 16 * wpb, 64u << 20, err)) {
            for (size_t b = 0; b < c.words() && rc >= 0; b += wpb) {
                Set& S = set[cur];
                if ((rc = drain(S)) < 0) break;  // its previous sub-batch, two sub-batches ago
                const size_t e = std::min(c.words(), b + wpb);
                S.words = e - b;
                S.hoff.resize(S.words + 1);
                for (size_t i = b; i <= e; i++) S.hoff[i - b] = c.off[i] - c.off[b];
                const size_t nbytes = c.off[e] - c.off[b];
                if (S.bytes.n < nbytes + 16 && S.bytes.ensure(nbytes + 16 + (nbytes >> 1))) { rc = DWPA_E_NOMEM; break; }
                if (hipMemcpyAsync(S.off.p, S.hoff.data(), S.hoff.size() * 8, hipMemcpyHostToDevice, S.s) != hipSuccess ||
                    (nbytes && hipMemcpyAsync(S.bytes.p, c.bytes.data() + c.off[b], nbytes, hipMemcpyHostToDevice,
                                              S.s) != hipSuccess) ||
                    hipEventRecord(S.up, S.s) != hipSuccess ||
                    launch_rules_expand((const uint64_t*)S.off.p, (const uint8_t*)S.bytes.p, (uint32_t)S.words,
                                        (const uint32_t*)dr.offs, (const uint32_t*)dr.code, (uint32_t)nr,
                                        (uint8_t*)S.out.p, (uint32_t*)S.len.p, S.s, (uint32_t*)S.tlen.p) != hipSuccess) {
                    rc = DWPA_E_HIP;
                    break;
                }
                if ((rc = pack(S)) < 0) break;
                S.busy = true;  // S.hoff is rewritten only after drain(S); the chunk only after uploads_done()
                words += S.words;
                cur ^= 1;
                if ((rc = drain(set[cur])) < 0) break;
            }
        }
        if (err && rc >= 0) rc = DWPA_E_IO;
        for (Set& S : set)
            if (rc >= 0) rc = drain(S);
    }
    for (Set& S : set) {
        if (S.s) (void)hipStreamSynchronize(S.s);
        for (DevBuf* b : {&S.off, &S.bytes, &S.out, &S.len, &S.tlen, &S.bsum, &S.bcnt, &S.tot, &S.text}) b->release();
        pinned_free(S.h_text, S.h_cap);
        pinned_free(S.h_tot, 8);
        if (S.done) (void)hipEventDestroy(S.done);
        if (S.up) (void)hipEventDestroy(S.up);
        if (S.s) (void)hipStreamDestroy(S.s);
    }
    rules_release(&dr);
    if (gz && gzclose(gz) != Z_OK && rc >= 0) rc = DWPA_E_IO;
    if (fo && fclose(fo) != 0 && rc >= 0) rc = DWPA_E_IO;
    if (words_out) *words_out = words;
    if (cands_out) *cands_out = cands;
    return rc < 0 ? rc : 0;
}

}  // namespace dwpa

extern "C" {

int dwpa_rules_expand_file(int device, const char* rules_file, const char* const* sources, size_t nsources,
                           const char* out_path, int gzip_level, uint64_t* words_out, uint64_t* cands_out) {
    return dwpa::guarded([&]() -> int {
        return dwpa::rules_expand_file_impl(device, rules_file, sources, nsources, out_path, gzip_level, words_out,
                                            cands_out);
    });
}

int dwpa_crack_files(const char* hash_file, const char* const* dicts, size_t ndicts, const char* rules_file,
                     int nonce_error_corrections, const char* out_file, const dwpa_config* cfg) {
    return dwpa::guarded([&]() -> int {
        return dwpa::crack_impl(hash_file, dicts, ndicts, rules_file, nonce_error_corrections, out_file, cfg, nullptr);
    }, DWPA_RC_ERROR, DWPA_RC_ERROR);
}

// Test hook (outside include/dwpa22000.h and the ABI version): out[0..3] = loads issued, overflowed and repeated, kept
// nothing, scanned, by the sizing loops of the dictionary, rules, hybrid and combinator runs of this process.
void dwpa_debug_crack_loads(uint64_t out[4], int reset) {
    std::atomic<uint64_t>* c[4] = {&dwpa::g_loads_issued, &dwpa::g_loads_overflowed, &dwpa::g_loads_empty,
                                   &dwpa::g_loads_scanned};
    for (int i = 0; i < 4; i++) {
        const uint64_t v = reset ? c[i]->exchange(0u, std::memory_order_relaxed)
                                 : c[i]->load(std::memory_order_relaxed);
        if (out) out[i] = v;
    }
}

int dwpa_crack_files_ex(const char* hash_file, const char* const* dicts, size_t ndicts, const char* rules_file,
                        int nonce_error_corrections, const char* out_file, const dwpa_config* cfg,
                        int32_t* dict_status) {
    return dwpa::guarded([&]() -> int {
        return dwpa::crack_impl(hash_file, dicts, ndicts, rules_file, nonce_error_corrections, out_file, cfg, dict_status);
    }, DWPA_RC_ERROR, DWPA_RC_ERROR);
}

int dwpa_crack_hybrid(const char* hash_file, const char* const* dicts, size_t ndicts, const char* mask,
                      const dwpa_bytes custom[4], int mode, int nonce_error_corrections, const char* out_file,
                      const dwpa_config* cfg, int32_t* dict_status) {
    return dwpa::guarded([&]() -> int {
        auto m = std::make_unique<dwpa::Mask>();
        dwpa::HybridSpec hy;
        hy.mask = m.get();
        hy.mode = mode;
        hy.valid = true;
        if (mode != DWPA_HYBRID_WORD_MASK && mode != DWPA_HYBRID_MASK_WORD) {
            fprintf(stderr, "[dwpa] hybrid mode %d: 6 (wordlist + mask) or 7 (mask + wordlist)\n", mode);
            hy.valid = false;
        }
        if (!mask || dwpa::mask_parse(mask, strlen(mask), custom, m.get()) < 0) {
            fprintf(stderr, "[dwpa] mask %s: invalid (syntax, an undefined custom set, more than 63 positions or a "
                            "keyspace above 2^64 - 1)\n", mask ? mask : "(null)");
            hy.valid = false;
        }
        return dwpa::crack_impl(hash_file, dicts, ndicts, nullptr, nonce_error_corrections, out_file, cfg, dict_status,
                                &hy);
    }, DWPA_RC_ERROR, DWPA_RC_ERROR);
}

int dwpa_crack_combinator(const char* hash_file, const char* left_dict, const char* right_dict, int amp_side,
                          int nonce_error_corrections, const char* out_file, const dwpa_config* cfg,
                          int32_t dict_status[2]) {
    return dwpa::guarded([&]() -> int {
        auto cb = std::make_unique<dwpa::CombiSpec>();
        cb->valid = true;
        if (amp_side != DWPA_COMBI_AMP_RIGHT && amp_side != DWPA_COMBI_AMP_LEFT) {
            fprintf(stderr, "[dwpa] amp_side %d: 0 (the right list is the amplifier) or 1 (the left list)\n", amp_side);
            cb->valid = false;
        } else {
            cb->side = amp_side;
        }
        const char* const dicts[2] = {left_dict, right_dict};
        return dwpa::crack_impl(hash_file, dicts, 2, nullptr, nonce_error_corrections, out_file, cfg, dict_status,
                                nullptr, cb.get());
    }, DWPA_RC_ERROR, DWPA_RC_ERROR);
}

// md5 over fields 1..7 of the hashline (web/common.php:310-315); a tiny host MD5 keeps this dependency-free.
static void md5_host(const uint8_t* msg, size_t len, uint8_t out[16]) {
    static const uint32_t K[64] = {
        0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501,
        0x698098d8, 0x8b44f7af, 0xffff5bb1, 0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821,
        0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d, 0x02441453, 0xd8a1e681, 0xe7d3fbc8,
        0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a,
        0xfffa3942, 0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70,
        0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05, 0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665,
        0xf4292244, 0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d, 0x85845dd1,
        0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391};
    static const int S[4][4] = {{7, 12, 17, 22}, {5, 9, 14, 20}, {4, 11, 16, 23}, {6, 10, 15, 21}};
    std::string b((const char*)msg, len);
    b.push_back((char)0x80);
    while (b.size() % 64 != 56) b.push_back('\0');
    const uint64_t bits = (uint64_t)len * 8;
    for (int i = 0; i < 8; i++) b.push_back((char)(bits >> (8 * i)));
    uint32_t h[4] = {0x67452301, 0xefcdab89, 0x98badcfe, 0x10325476};
    for (size_t o = 0; o < b.size(); o += 64) {
        uint32_t m[16];
        for (int j = 0; j < 16; j++)
            m[j] = (uint32_t)(uint8_t)b[o + 4 * j] | (uint32_t)(uint8_t)b[o + 4 * j + 1] << 8 |
                   (uint32_t)(uint8_t)b[o + 4 * j + 2] << 16 | (uint32_t)(uint8_t)b[o + 4 * j + 3] << 24;
        uint32_t a = h[0], bb = h[1], c = h[2], d = h[3];
        for (int i = 0; i < 64; i++) {
            uint32_t f;
            int g;
            if (i < 16) { f = (bb & c) | (~bb & d); g = i; }
            else if (i < 32) { f = (d & bb) | (~d & c); g = (5 * i + 1) & 15; }
            else if (i < 48) { f = bb ^ c ^ d; g = (3 * i + 5) & 15; }
            else { f = c ^ (bb | ~d); g = (7 * i) & 15; }
            uint32_t t = d;
            d = c;
            c = bb;
            uint32_t x = a + f + K[i] + m[g];
            int s = S[i >> 4][i & 3];
            bb = bb + ((x << s) | (x >> (32 - s)));
            a = t;
        }
        h[0] += a; h[1] += bb; h[2] += c; h[3] += d;
    }
    for (int k = 0; k < 4; k++)
        for (int i = 0; i < 4; i++) out[4 * k + i] = (uint8_t)(h[k] >> (8 * i));
}

int dwpa_hash_m22000(const char* line, size_t line_len, uint8_t out[16]) {
    return dwpa::guarded([&]() -> int {
        if (!line || !out) return DWPA_E_ARG;
        const char* f[9];
        size_t fl[9], cnt = 0, st = 0;
        for (size_t i = 0; i < line_len && cnt < 8; i++)
            if (line[i] == '*') { f[cnt] = line + st; fl[cnt] = i - st; cnt++; st = i + 1; }
        f[cnt] = line + st; fl[cnt] = line_len - st; cnt++;
        if (cnt != 9) return DWPA_E_FORMAT;
        std::string cat;
        for (int i = 1; i <= 7; i++) cat.append(f[i], fl[i]);
        md5_host((const uint8_t*)cat.data(), cat.size(), out);
        return 0;
    });
}

}  // extern "C"
