// crack_range.cpp -- the two attacks over a range of indices, with dwpa_crack_files' hash file, rc convention, outfile
// records, nc-mode default and cfg handling (crack_common.hpp):
//   dwpa_crack_mask():  hashcat -a 3.  The keyspace is a list of segments, one per mask length that runs: the mask
//                       itself, or with increment its prefixes, shortest first.
//   dwpa_crack_mask_markov(): the same in Markov order under a threshold (markov.hpp): the segments index the
//                       thresholded keyspace, and one model serves every prefix.
//   dwpa_crack_chain(): a chain of 1..4 word lists and masks (chain.hpp).  Every list is read whole through the
//                       dictionary reader once (plain or gzip, CRLF, $HEX[]), kept on the host to rebuild a hit's PSK
//                       and uploaded once per worker.  The keyspace is one segment of raw indices [skip, skip + limit).
//   dwpa_crack_chain_rules(): the same with a rules file on any list part (chain_rules_dev.hip): that part's choices
//                       are its (rule, word) pairs, rule-major, and a hit's PSK takes the rule through
//                       RuleSet::apply_host.
//   dwpa_crack_table(): one word list under a substitution table (table.hpp): every combination of the per-byte
//                       alternatives of every kept word.  The keyspace is a prefix sum over the words; one segment
//                       of raw indices [skip, skip + limit).
//   dwpa_crack_assoc(): every net (ESSID, MAC_AP) of the hash file against its own words x the rules (assoc.hpp): the
//                       keyspace is a prefix sum over the nets; one segment of raw indices [skip, skip + limit).  The
//                       host-only dwpa_assoc_single / _plan / _candidates share its set-up and live here with it.
//
// There is no dictionary feed, so none of crack.cpp's reader / item-queue machinery: every worker --
// DWPA_CRACK_SHARDS_PER_DEVICE per selected device -- takes batch-sized ascending index ranges from one shared cursor
// (crack_cursor.hpp), generates them on its device, scans them and reports.  A hit's PSK is rebuilt on the host from
// its index; the first hit of a line is written once, under the mutex, and the line is retired on every worker before
// its next launch.  A fully cracked file stops every worker.
//
// One driver runs both.  An attack is a type with the segments' meaning in it and a nested Worker, one per scan worker:
//   Worker(attack)            its state (the mask attack: the prefix its scan holds)
//   open(w)                   once, before any thread runs (the chain attack: upload the lists, scan_set_chain)
//   enter(w, seg)             before the first load of a segment
//   load(w, first, count)     generate indices [first, first + count) of the segment into w's scan
//   counted(w, count, &n)     the candidates of the load just scanned; the stream is idle
//   plain_of(id, &psk)        the PSK of candidate id of the segment; false for an id outside it
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "dwpa22000.h"
#include "assoc.hpp"
#include "chain.hpp"
#include "crack_common.hpp"
#include "crack_cursor.hpp"
#include "engine.hpp"
#include "markov.hpp"
#include "mask.hpp"
#include "rules.hpp"
#include "table.hpp"

namespace dwpa {

namespace {

template <class AttackWorker>
int range_worker(ScanWorker& w, AttackWorker& aw, CrackShared& sh, RangeCursor& cursor) {
    if (hipSetDevice(w.device) != hipSuccess) return DWPA_E_HIP;
    const uint32_t cap = scan_batch_cap(w.scan);
    size_t cur_seg = (size_t)-1, seg;
    uint64_t first;
    uint32_t count;
    std::vector<HitDev> hits;
    while (!sh.stop.load(std::memory_order_relaxed) && cursor.take(cap, &seg, &first, &count)) {
        const auto ts = std::chrono::steady_clock::now();
        int r;
        if (seg != cur_seg) {
            if ((r = aw.enter(w, seg)) < 0) return r;
            cur_seg = seg;
        }
        if ((r = aw.load(w, first, count)) < 0) return r;
        if ((r = scan_step(w, sh, hits, [&](uint64_t id, std::string* psk) { return aw.plain_of(id, psk); })) < 0)
            return r;
        uint64_t n = 0;
        if ((r = aw.counted(w, count, &n)) < 0) return r;
        w.items++;
        w.cands += n;
        w.scan_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - ts).count();
    }
    return 0;
}

// From the first device touched to the return code.  Everything an attack can refuse on the host has been refused.
template <class Attack>
int crack_range(CrackCall& call, const char* hash_file, int nec, const char* out_file, const dwpa_config* cfg,
                std::vector<RangeSegment> segs, const Attack& attack) {
    CrackPlan plan;
    if (!crack_plan(cfg, nec, &plan)) return DWPA_RC_ERROR;
    CrackShared sh;
    HashLines hl;
    if (!sh.load_hashes(hash_file, &hl) || !sh.open_out(out_file)) return DWPA_RC_ERROR;

    struct Work {
        ScanWorker scan;
        typename Attack::Worker attack;
        explicit Work(const Attack& a) : attack(a) {}
    };
    std::vector<std::unique_ptr<Work>> work;
    int rc = 0;
    for (int dev : plan.devs)
        for (size_t k = 0; k < plan.shards && rc >= 0; k++) {
            work.push_back(std::make_unique<Work>(attack));
            Work& w = *work.back();
            if ((rc = scan_worker_open(w.scan, dev, hl, plan)) >= 0) rc = w.attack.open(w.scan);
        }
    RangeCursor cursor(std::move(segs));
    if (rc >= 0)
        run_workers(sh, work.size(), [&](size_t k) { return range_worker(work[k]->scan, work[k]->attack, sh, cursor); });
    std::vector<dwpa_crack_worker> wst;
    for (auto& wp : work) {
        ScanWorker& w = wp->scan;
        scan_worker_close(w);  // waits for the device: what the attack's worker holds there is free after it
        wst.push_back(dwpa_crack_worker{w.device, (uint32_t)w.items, 0, w.cands, 0.0, w.scan_s});
    }
    return call.finish(sh, wst, rc < 0);
}

struct MaskAttack {
    const Mask& full;
    std::vector<uint32_t> npos;  // per segment: the positions of its prefix

    struct Worker {
        const MaskAttack& at;
        std::unique_ptr<Mask> cur = std::make_unique<Mask>();  // the prefix this worker's scan holds
        explicit Worker(const MaskAttack& a) : at(a) {}
        int open(ScanWorker&) { return 0; }
        int enter(ScanWorker& w, size_t seg) {
            mask_prefix(at.full, at.npos[seg], cur.get());
            return scan_set_mask(w.scan, *cur);
        }
        int load(ScanWorker& w, uint64_t first, uint32_t count) { return scan_load_mask(w.scan, first, count, w.stream); }
        int counted(ScanWorker&, uint32_t count, uint64_t* n) {
            *n = count;  // every index is a candidate: nothing to read back
            return 0;
        }
        bool plain_of(uint64_t id, std::string* psk) const {
            if (id >= cur->keyspace) return false;
            uint8_t m[64];
            mask_candidate(*cur, id, m);
            psk->assign((const char*)m, cur->npos);
            return true;
        }
    };
};

// The segments of a mask run: the mask itself over [skip, skip + limit), or with increment its prefixes of inc_min..
// inc_max positions, shortest first.  npos: the mask's positions, keyspace_of(n): the keyspace of its first n.  Fills
// npos_of (the positions of each segment's prefix) and segs; false after a message for what hashcat refuses.  Both
// empty: nothing is left to run.
template <class KeyspaceOf>
bool mask_segments(const char* mask, uint32_t npos, KeyspaceOf keyspace_of, uint64_t skip, uint64_t limit,
                   uint32_t inc_min, uint32_t inc_max, std::vector<uint32_t>* npos_of, std::vector<RangeSegment>* segs) {
    const bool increment = inc_min || inc_max;
    if (increment && (skip || limit)) {
        fprintf(stderr, "[dwpa] --increment cannot be combined with --skip / --limit\n");
        return false;
    }
    if (increment) {
        const uint32_t lo = std::max<uint32_t>(1, inc_min), hi = std::min(inc_max ? inc_max : npos, npos);
        if (lo > hi) return false;
        for (uint32_t n = lo; n <= hi; n++) {
            if (n < 8) {  // hashcat skips a mask shorter than the hash mode's shortest password
                fprintf(stderr, "[dwpa] skipping the mask's first %u positions: m22000 takes 8..63 characters\n", n);
                continue;
            }
            npos_of->push_back(n);
            segs->push_back(RangeSegment{0, keyspace_of(n)});
        }
    } else if (npos < 8) {
        fprintf(stderr, "[dwpa] skipping mask %s: %u positions, m22000 takes 8..63 characters\n", mask, npos);
    } else {
        const uint64_t K = keyspace_of(npos);
        if (skip >= K) {
            fprintf(stderr, "[dwpa] --skip is not below the keyspace\n");
            return false;
        }
        const uint64_t room = K - skip;
        npos_of->push_back(npos);
        segs->push_back(RangeSegment{skip, skip + (limit && limit < room ? limit : room)});
    }
    return true;
}

int crack_mask_impl(const char* hash_file, const char* mask, const dwpa_bytes* custom, uint64_t skip, uint64_t limit,
                    uint32_t inc_min, uint32_t inc_max, int nec, const char* out_file, const dwpa_config* cfg) {
    CrackCall call;
    if (!hash_file || !mask || !out_file) return DWPA_RC_ERROR;
    if (!crack_check_args(cfg, nec)) return DWPA_RC_ERROR;
    auto full = std::make_unique<Mask>();
    if (mask_parse(mask, strlen(mask), custom, full.get()) < 0) {
        fprintf(stderr, "[dwpa] mask %s: invalid (syntax, an undefined custom set, more than 63 positions or a keyspace "
                        "above 2^64 - 1)\n", mask);
        return DWPA_RC_ERROR;
    }
    MaskAttack attack{*full, {}};
    std::vector<RangeSegment> segs;
    auto pre = std::make_unique<Mask>();
    if (!mask_segments(mask, full->npos, [&](uint32_t n) {
            mask_prefix(*full, n, pre.get());
            return pre->keyspace;
        }, skip, limit, inc_min, inc_max, &attack.npos, &segs))
        return DWPA_RC_ERROR;
    if (segs.empty()) return DWPA_RC_ERROR;  // nothing left to run
    return crack_range(call, hash_file, nec, out_file, cfg, std::move(segs), attack);
}

struct MarkovAttack {
    const MarkovMask& full;
    const std::vector<uint8_t>& model;
    std::vector<uint32_t> npos;  // per segment: the positions of its prefix

    struct Worker {
        const MarkovAttack& at;
        std::unique_ptr<MarkovMask> cur = std::make_unique<MarkovMask>();  // the prefix this worker's scan holds
        explicit Worker(const MarkovAttack& a) : at(a) {}
        int open(ScanWorker&) { return 0; }
        int enter(ScanWorker& w, size_t seg) {
            markov_prefix(at.full, at.npos[seg], cur.get());
            return scan_set_mask_markov(w.scan, *cur, at.model.data());
        }
        int load(ScanWorker& w, uint64_t first, uint32_t count) { return scan_load_mask(w.scan, first, count, w.stream); }
        int counted(ScanWorker&, uint32_t count, uint64_t* n) {
            *n = count;  // every index is a candidate: nothing to read back
            return 0;
        }
        bool plain_of(uint64_t id, std::string* psk) const {
            if (id >= cur->keyspace) return false;
            uint8_t m[64];
            markov_candidate(*cur, at.model.data(), id, m);
            psk->assign((const char*)m, cur->npos);
            return true;
        }
    };
};

int crack_mask_markov_impl(const char* hash_file, const char* mask, const dwpa_bytes* custom, const char* markov_file,
                           uint32_t threshold, uint64_t skip, uint64_t limit, uint32_t inc_min, uint32_t inc_max,
                           int nec, const char* out_file, const dwpa_config* cfg) {
    CrackCall call;
    if (!hash_file || !mask || !markov_file || !out_file) return DWPA_RC_ERROR;
    if (!crack_check_args(cfg, nec)) return DWPA_RC_ERROR;
    auto sets = std::make_unique<Mask>();
    auto full = std::make_unique<MarkovMask>();
    if (threshold > 256) {
        fprintf(stderr, "[dwpa] the Markov threshold takes 0 (none) or 1..256\n");
        return DWPA_RC_ERROR;
    }
    if (mask_parse_sets(mask, strlen(mask), custom, sets.get()) < 0 || markov_mask(*sets, threshold, full.get()) < 0) {
        fprintf(stderr, "[dwpa] mask %s: invalid (syntax, an undefined custom set, more than 63 positions or a keyspace "
                        "above 2^64 - 1)\n", mask);
        return DWPA_RC_ERROR;
    }
    std::vector<uint8_t> model;
    const int mr = markov_read_file(markov_file, &model);
    if (mr < 0) {
        fprintf(stderr, "[dwpa] Markov model %s: %s\n", markov_file,
                mr == DWPA_E_IO ? "cannot be read" : "not a model file (size, header or a row that is no permutation)");
        return DWPA_RC_ERROR;
    }
    MarkovAttack attack{*full, model, {}};
    std::vector<RangeSegment> segs;
    auto pre = std::make_unique<MarkovMask>();
    if (!mask_segments(mask, full->npos, [&](uint32_t n) {
            markov_prefix(*full, n, pre.get());
            return pre->keyspace;
        }, skip, limit, inc_min, inc_max, &attack.npos, &segs))
        return DWPA_RC_ERROR;
    if (segs.empty()) return DWPA_RC_ERROR;  // nothing left to run
    return crack_range(call, hash_file, nec, out_file, cfg, std::move(segs), attack);
}

struct ChainPart {
    std::unique_ptr<Mask> mask;  // a mask part, else a list
    HostList list;
    std::unique_ptr<RuleSet> rules;  // a ruled list: radix = its word count x its rules
    uint64_t radix = 0;
};

struct ChainAttack {
    const dwpa_chain_spec* specs;
    const dwpa_bytes* custom;
    std::vector<ChainPart> parts;
    uint64_t radix[CHAIN_MAX_PARTS] = {};
    uint64_t K = 0;

    // Candidate `id` (< K) as its bytes: the parts' choices left to right.
    bool candidate(uint64_t id, std::string* psk) const {
        uint64_t digit[CHAIN_MAX_PARTS];
        if (chain_split(radix, (uint32_t)parts.size(), id, digit) < 0) return false;
        psk->clear();
        for (size_t p = 0; p < parts.size(); p++) {
            const ChainPart& cp = parts[p];
            if (cp.mask) {
                uint8_t m[64];
                mask_candidate(*cp.mask, digit[p], m);
                psk->append((const char*)m, cp.mask->npos);
            } else {
                const HostList& l = cp.list;
                if (cp.rules) {  // choice = rule * words + word
                    const uint64_t nw = l.words(), rule = digit[p] / nw, wi = digit[p] % nw;
                    std::string piece;
                    if (!cp.rules->apply_host((size_t)rule, l.bytes.substr((size_t)l.off[wi],
                                                                           (size_t)(l.off[wi + 1] - l.off[wi])), &piece))
                        return false;  // cannot happen for a hit: the GPU kept it
                    psk->append(piece);
                    continue;
                }
                psk->append(l.bytes, (size_t)l.off[digit[p]], (size_t)(l.off[digit[p] + 1] - l.off[digit[p]]));
            }
        }
        return true;
    }

    struct Worker {
        const ChainAttack& at;
        int device = 0;
        DevBuf off[CHAIN_MAX_PARTS], bytes[CHAIN_MAX_PARTS];  // the lists on this worker's device
        explicit Worker(const ChainAttack& a) : at(a) {}
        ~Worker() {
            (void)hipSetDevice(device);
            for (uint32_t p = 0; p < CHAIN_MAX_PARTS; p++) {
                off[p].release();
                bytes[p].release();
            }
        }
        int open(ScanWorker& w) {
            device = w.device;
            dwpa_chain_part cp[CHAIN_MAX_PARTS] = {};
            for (size_t p = 0; p < at.parts.size(); p++) {
                if (at.parts[p].mask) {
                    cp[p].kind = DWPA_CHAIN_MASK;
                    cp[p].mask = at.specs[p].text;
                    cp[p].mask_len = strlen(at.specs[p].text);
                    continue;
                }
                const int r = upload_list(at.parts[p].list, &off[p], &bytes[p]);
                if (r < 0) return r;
                cp[p].kind = DWPA_CHAIN_LIST;
                cp[p].d_offsets = (const uint64_t*)off[p].p;
                cp[p].d_bytes = (const uint8_t*)bytes[p].p;
                cp[p].nwords = at.parts[p].list.words();
            }
            int r = scan_set_chain(w.scan, cp, (uint32_t)at.parts.size(), at.custom, nullptr);
            for (size_t p = 0; p < at.parts.size() && r >= 0; p++)
                if (at.parts[p].rules) r = scan_set_chain_rules(w.scan, (uint32_t)p, at.parts[p].rules.get(), nullptr);
            return r < 0 ? r : 0;
        }
        int enter(ScanWorker&, size_t) { return 0; }
        // A load is `count` raw indices, so PBKDF2 runs over the kept ones only: a chain whose filter drops most
        // candidates runs short launches (filling a batch from several raw ranges is left for later).
        int load(ScanWorker& w, uint64_t first, uint32_t count) {
            return scan_load_chain(w.scan, first, count, 8, 63, w.stream);
        }
        int counted(ScanWorker& w, uint32_t, uint64_t* n) {
            uint32_t kept = 0;  // the stream is idle by now: this copy waits for nothing
            const int r = scan_counter_raw(w.scan, w.stream, &kept);
            *n = kept;
            return r;
        }
        bool plain_of(uint64_t id, std::string* psk) const { return id < at.K && at.candidate(id, psk); }
    };
};

int crack_chain_impl(const char* hash_file, const dwpa_chain_spec* specs, uint32_t nparts,
                     const char* const* part_rules /* nullable; nparts paths of rules files, nullptr: no rules */,
                     const dwpa_bytes* custom, uint64_t skip, uint64_t limit, int nec, const char* out_file,
                     const dwpa_config* cfg, int32_t* part_status) {
    CrackCall call;
    if (nparts == 0 || nparts > CHAIN_MAX_PARTS) {
        fprintf(stderr, "[dwpa] a chain takes 1..%u parts\n", CHAIN_MAX_PARTS);
        return DWPA_RC_ERROR;
    }
    if (part_status)
        for (uint32_t p = 0; p < nparts; p++) part_status[p] = DWPA_DICT_OK;
    if (!hash_file || !specs || !out_file) return DWPA_RC_ERROR;
    if (!crack_check_args(cfg, nec)) return DWPA_RC_ERROR;
    // every part is looked at before the call fails, so that each unreadable list is marked
    ChainAttack attack{specs, custom, {}};
    std::vector<ChainPart>& parts = attack.parts;
    parts.resize(nparts);
    bool bad = false;
    for (uint32_t p = 0; p < nparts; p++) {
        const char* text = specs[p].text;
        if (specs[p].kind == DWPA_CHAIN_MASK) {
            parts[p].mask = std::make_unique<Mask>();
            if (part_rules && part_rules[p]) {
                fprintf(stderr, "[dwpa] part %u: rules go with a list part, not with a mask\n", p + 1);
                bad = true;
            }
            if (!text || mask_parse(text, strlen(text), custom, parts[p].mask.get()) < 0) {
                fprintf(stderr, "[dwpa] part %u, mask %s: invalid (syntax, an undefined custom set, more than 63 "
                                "positions or a keyspace above 2^64 - 1)\n", p + 1, text ? text : "(null)");
                bad = true;
            } else {
                parts[p].radix = parts[p].mask->keyspace;
            }
        } else if (specs[p].kind == DWPA_CHAIN_LIST) {
            FILE* f = text ? fopen(text, "rb") : nullptr;
            if (!f) {
                if (part_status) part_status[p] = DWPA_E_IO;
                fprintf(stderr, "[dwpa] part %u, list %s: cannot be opened\n", p + 1, text ? text : "(null)");
                bad = true;
            } else {
                fclose(f);
            }
        } else {
            fprintf(stderr, "[dwpa] part %u: kind %d is neither a list nor a mask\n", p + 1, specs[p].kind);
            bad = true;
        }
    }
    if (bad) return DWPA_RC_ERROR;
    // rules files load under the process's rule mode, as dwpa_crack_files' -r (hashcat's loader unless DWPA_RULES_FULL);
    // the counts are sums over the parts and are published whatever becomes of the call
    const int want = DWPA_CFG_HAS(cfg, rule_mode) ? cfg->rule_mode : DWPA_RULES_DEFAULT;
    if (want != DWPA_RULES_DEFAULT && want != DWPA_RULES_HASHCAT && want != DWPA_RULES_FULL) return DWPA_RC_ERROR;
    for (uint32_t p = 0; p < nparts; p++) {
        if (!part_rules || !part_rules[p]) continue;
        parts[p].rules = std::make_unique<RuleSet>();
        parts[p].rules->mode = want == DWPA_RULES_DEFAULT ? engine_rule_mode() : want;
        const int lr = parts[p].rules->load_file(part_rules[p]);
        if (lr == DWPA_E_IO) fprintf(stderr, "[dwpa] part %u, rules %s: cannot be opened\n", p + 1, part_rules[p]);
        call.st.rules += (uint32_t)parts[p].rules->size();
        call.st.rules_skipped += (uint32_t)parts[p].rules->skipped.size();
        call.st.rules_rejmem += parts[p].rules->rejmem;
        bad |= lr < 0;
    }
    if (part_rules) crack_publish_stats(call.st, {});
    if (bad) return DWPA_RC_ERROR;
    {
        FILE* f = fopen(hash_file, "rb");
        if (!f) return DWPA_RC_ERROR;
        fclose(f);
    }
    for (uint32_t p = 0; p < nparts; p++) {
        if (!parts[p].mask) {
            const int r = read_list(specs[p].text, &parts[p].list);
            if (r == DWPA_E_OVERFLOW) {
                fprintf(stderr, "[dwpa] part %u, list %s: too large to hold (at most %llu bytes of text and offsets, "
                                "fewer than 2^32 words)\n", p + 1, specs[p].text,
                        (unsigned long long)DWPA_COMBI_AMP_MAX_BYTES);
                return DWPA_RC_ERROR;
            }
            if (r < 0) {
                if (part_status) part_status[p] = DWPA_E_IO;
                fprintf(stderr, "[dwpa] part %u, list %s: read error\n", p + 1, specs[p].text);
                return DWPA_RC_ERROR;
            }
            if (parts[p].list.damaged && part_status) part_status[p] = DWPA_DICT_DAMAGED;
            parts[p].radix = parts[p].list.words();
            call.st.words += parts[p].radix;
            if (parts[p].rules) {
                parts[p].radix *= parts[p].rules->size();  // < 2^32 words x a rule count that fits memory: no wrap
                if (parts[p].radix > UINT32_MAX) {
                    fprintf(stderr, "[dwpa] part %u: %llu words x %zu rules is 2^32 choices or more\n", p + 1,
                            (unsigned long long)parts[p].list.words(), parts[p].rules->size());
                    return DWPA_RC_ERROR;
                }
            }
        }
        attack.radix[p] = parts[p].radix;
    }
    if (chain_keyspace(attack.radix, nparts, &attack.K) < 0) {
        fprintf(stderr, "[dwpa] the chain's keyspace is above 2^64 - 1\n");
        return DWPA_RC_ERROR;
    }
    const uint64_t K = attack.K;
    if (K > 0 && skip >= K) {
        fprintf(stderr, "[dwpa] --skip is not below the keyspace\n");
        return DWPA_RC_ERROR;
    }
    std::vector<RangeSegment> segs;  // K = 0 (an empty list): nothing to run, the call exhausts
    if (K > 0) {
        const uint64_t room = K - skip;
        segs.push_back(RangeSegment{skip, skip + (limit && limit < room ? limit : room)});
    }
    return crack_range(call, hash_file, nec, out_file, cfg, std::move(segs), attack);
}

// The table attack (table.hpp): one list held whole, the table, and the kept-word index built on the host, which names
// the keyspace before any device is touched and rebuilds a hit's PSK.  Every worker's scan builds its own index on its
// device (scan_set_table); the two must agree.
struct TableAttack {
    Table table;
    TableFilter filter;
    HostList list;
    TableIndex index;

    struct Worker {
        const TableAttack& at;
        int device = 0;
        DevBuf off, bytes;  // the list on this worker's device
        explicit Worker(const TableAttack& a) : at(a) {}
        ~Worker() {
            (void)hipSetDevice(device);
            off.release();
            bytes.release();
        }
        int open(ScanWorker& w) {
            device = w.device;
            int r = upload_list(at.list, &off, &bytes);
            if (r < 0) return r;
            uint64_t K = 0, kept = 0;
            r = scan_set_table(w.scan, (const uint64_t*)off.p, (const uint8_t*)bytes.p, at.list.words(), at.table,
                               at.filter.minlen, at.filter.maxlen, at.filter.word_max, &K, &kept);
            if (r < 0) return r;
            return K == at.index.keyspace() && kept == at.index.kept() ? 0 : DWPA_E_HIP;
        }
        int enter(ScanWorker&, size_t) { return 0; }
        int load(ScanWorker& w, uint64_t first, uint32_t count) { return scan_load_table(w.scan, first, count, w.stream); }
        int counted(ScanWorker&, uint32_t count, uint64_t* n) {
            *n = count;  // every index is a candidate: nothing to read back
            return 0;
        }
        bool plain_of(uint64_t id, std::string* psk) const {
            uint8_t m[64];
            uint32_t len;
            if (!table_candidate(at.table, at.index, at.list.off.data(), (const uint8_t*)at.list.bytes.data(), id, m,
                                 &len))
                return false;
            psk->assign((const char*)m, len);
            return true;
        }
    };
};

int crack_table_impl(const char* hash_file, const char* dict, const char* table_file, uint32_t word_max, uint64_t skip,
                     uint64_t limit, int nec, const char* out_file, const dwpa_config* cfg) {
    CrackCall call;
    if (!hash_file || !dict || !table_file || !out_file) return DWPA_RC_ERROR;
    if (!crack_check_args(cfg, nec)) return DWPA_RC_ERROR;
    auto attack = std::make_unique<TableAttack>();
    attack->filter = table_filter(8, TABLE_MAX_LEN, word_max);
    uint32_t bad_line = 0;
    const int tr = table_read_file(table_file, &attack->table, &bad_line);
    if (tr == DWPA_E_IO) {
        fprintf(stderr, "[dwpa] table %s: cannot be read\n", table_file);
        return DWPA_RC_ERROR;
    }
    if (tr < 0) {
        fprintf(stderr, "[dwpa] table %s: line %u is not K=V (one byte or \\xHH each), is a 17th alternative for its "
                        "key, or the file holds no mapping\n", table_file, bad_line);
        return DWPA_RC_ERROR;
    }
    {
        FILE* f = fopen(hash_file, "rb");
        if (!f) {
            fprintf(stderr, "[dwpa] hash file %s: cannot be opened\n", hash_file);
            return DWPA_RC_ERROR;
        }
        fclose(f);
    }
    const int lr = read_list(dict, &attack->list);
    if (lr == DWPA_E_OVERFLOW) {
        fprintf(stderr, "[dwpa] list %s: too large to hold (at most %llu bytes of text and offsets, fewer than 2^32 "
                        "words)\n", dict, (unsigned long long)DWPA_COMBI_AMP_MAX_BYTES);
        return DWPA_RC_ERROR;
    }
    if (lr < 0) {
        fprintf(stderr, "[dwpa] list %s: cannot be read\n", dict);
        return DWPA_RC_ERROR;
    }
    const HostList& l = attack->list;
    call.st.words = l.words();
    if (table_index_list(attack->table, attack->filter, l.off.data(), (const uint8_t*)l.bytes.data(), (size_t)l.words(),
                         &attack->index) < 0) {
        fprintf(stderr, "[dwpa] the table attack's keyspace is above 2^64 - 1\n");
        return DWPA_RC_ERROR;
    }
    const TableIndex& ix = attack->index;
    fprintf(stderr, "[dwpa] table attack: %llu of %llu words kept, %llu dropped for length, %llu for more than %u "
                    "candidates\n", (unsigned long long)ix.kept(), (unsigned long long)l.words(),
            (unsigned long long)ix.dropped_len, (unsigned long long)ix.dropped_max, attack->filter.word_max);
    const uint64_t K = ix.keyspace();
    if (K > 0 && skip >= K) {
        fprintf(stderr, "[dwpa] --skip is not below the keyspace\n");
        return DWPA_RC_ERROR;
    }
    std::vector<RangeSegment> segs;  // K = 0 (no word kept): nothing to run, the call exhausts
    if (K > 0) {
        const uint64_t room = K - skip;
        segs.push_back(RangeSegment{skip, skip + (limit && limit < room ? limit : room)});
    }
    return crack_range(call, hash_file, nec, out_file, cfg, std::move(segs), *attack);
}

// The association attack (assoc.hpp): the plan -- nets, entries, start[] -- is built on the host from the parsed hash
// file before any device is touched; it names the keyspace and rebuilds a hit's PSK.  Every worker's scan takes the
// entries (scan_set_assoc) and builds its own index over its own nets; the two must agree on K.
struct AssocAttack {
    AssocPlan plan;
    std::unique_ptr<RuleSet> rules;

    struct Worker {
        const AssocAttack& at;
        explicit Worker(const AssocAttack& a) : at(a) {}
        int open(ScanWorker& w) {
            const AssocPlan& p = at.plan;
            if (scan_num_nets(w.scan) != p.nets.nets.size()) return DWPA_E_HIP;
            std::vector<dwpa_bytes> words((size_t)p.entries());
            for (size_t e = 0; e < words.size(); e++)
                words[e] = dwpa_bytes{(const uint8_t*)p.wbytes.data() + p.woff[e], (size_t)(p.woff[e + 1] - p.woff[e])};
            uint64_t K = 0;
            const int r = scan_set_assoc(w.scan, words.data(), p.wnet.data(), words.size(), at.rules.get(), 8, 63, &K);
            if (r < 0) return r;
            return K == p.keyspace() ? 0 : DWPA_E_HIP;
        }
        int enter(ScanWorker&, size_t) { return 0; }
        int load(ScanWorker& w, uint64_t first, uint32_t count) { return scan_load_assoc(w.scan, first, count, w.stream); }
        int counted(ScanWorker& w, uint32_t, uint64_t* n) {
            uint32_t kept = 0;  // the stream is idle by now: this copy waits for nothing
            const int r = scan_counter_raw(w.scan, w.stream, &kept);
            *n = std::min(kept, scan_batch_cap(w.scan));
            return r;
        }
        bool plain_of(uint64_t id, std::string* psk) const { return at.plan.candidate(id, psk); }
    };
};

// The hash file parsed, the rules file loaded under the process's rule mode and the plan built: what dwpa_assoc_plan,
// dwpa_assoc_candidates and dwpa_crack_assoc share.  A negative DWPA_E_* after one stderr line, else 0.
int assoc_prepare(const char* hash_file, const char* assoc_file, uint32_t flags, const char* rules_file, int rule_mode,
                  AssocAttack* at) {
    if (!hash_file || (flags & ~DWPA_ASSOC_SINGLE) || (!assoc_file && !(flags & DWPA_ASSOC_SINGLE))) {
        fprintf(stderr, "[dwpa] the association attack takes an association file, the single generator, or both\n");
        return DWPA_E_ARG;
    }
    if (rule_mode != DWPA_RULES_DEFAULT && rule_mode != DWPA_RULES_HASHCAT && rule_mode != DWPA_RULES_FULL)
        return DWPA_E_ARG;
    if (rules_file) {
        at->rules = std::make_unique<RuleSet>();
        at->rules->mode = rule_mode == DWPA_RULES_DEFAULT ? engine_rule_mode() : rule_mode;
        const int lr = at->rules->load_file(rules_file);
        if (lr == DWPA_E_IO) fprintf(stderr, "[dwpa] rules %s: cannot be opened\n", rules_file);
        if (lr < 0) return lr;
    }
    std::vector<std::string> lines;
    if (!read_hash_file(hash_file, lines)) {
        fprintf(stderr, "[dwpa] hash file %s: cannot be opened\n", hash_file);
        return DWPA_E_IO;
    }
    std::vector<ParsedLine> parsed(lines.size());
    for (size_t i = 0; i < lines.size(); i++) parsed[i] = parse_m22000(lines[i].data(), lines[i].size());
    const int r = assoc_plan(parsed, assoc_file, (flags & DWPA_ASSOC_SINGLE) != 0, rules_file ? 1u : 8u, at->rules.get(),
                             &at->plan);
    if (r == DWPA_E_IO) fprintf(stderr, "[dwpa] association file %s: cannot be read\n", assoc_file);
    else if (r < 0)
        fprintf(stderr, "[dwpa] the association attack's keyspace is above 2^64 - 1, or one net has 2^32 or more "
                        "word x rule choices\n");
    return r;
}

int crack_assoc_impl(const char* hash_file, const char* assoc_file, uint32_t flags, const char* rules_file,
                     uint64_t skip, uint64_t limit, int nec, const char* out_file, const dwpa_config* cfg) {
    CrackCall call;
    if (!hash_file || !out_file) return DWPA_RC_ERROR;
    if (!crack_check_args(cfg, nec)) return DWPA_RC_ERROR;
    auto attack = std::make_unique<AssocAttack>();
    const int pr = assoc_prepare(hash_file, assoc_file, flags, rules_file,
                                 DWPA_CFG_HAS(cfg, rule_mode) ? cfg->rule_mode : DWPA_RULES_DEFAULT, attack.get());
    if (attack->rules) {
        call.st.rules = (uint32_t)attack->rules->size();
        call.st.rules_skipped = (uint32_t)attack->rules->skipped.size();
        call.st.rules_rejmem = attack->rules->rejmem;
        crack_publish_stats(call.st, {});
    }
    if (pr < 0) return DWPA_RC_ERROR;
    const AssocPlan& p = attack->plan;
    call.st.words = p.entries();
    fprintf(stderr, "[dwpa] association attack: %llu nets, %llu entries, %u rules; association file: %llu lines, %llu "
                    "unmatched, %llu malformed; %llu words dropped\n", (unsigned long long)p.nets.nets.size(),
            (unsigned long long)p.entries(), p.R, (unsigned long long)p.file_lines, (unsigned long long)p.unmatched,
            (unsigned long long)p.malformed, (unsigned long long)p.dropped);
    const uint64_t K = p.keyspace();
    if (K > 0 && skip >= K) {
        fprintf(stderr, "[dwpa] --skip is not below the keyspace\n");
        return DWPA_RC_ERROR;
    }
    std::vector<RangeSegment> segs;  // K = 0 (no net has a word): nothing to run, the call exhausts
    if (K > 0) {
        const uint64_t room = K - skip;
        segs.push_back(RangeSegment{skip, skip + (limit && limit < room ? limit : room)});
    }
    return crack_range(call, hash_file, nec, out_file, cfg, std::move(segs), *attack);
}

}  // namespace

}  // namespace dwpa

extern "C" int dwpa_assoc_single(const char* line, size_t line_len, uint32_t minlen, uint8_t* out, size_t out_cap,
                                 uint32_t* lens, size_t lens_cap, size_t* nwords, size_t* nbytes) {
    return dwpa::guarded([&]() -> int {
        if (!line || !nwords || !nbytes) return DWPA_E_ARG;
        const dwpa::ParsedLine p = dwpa::parse_m22000(line, line_len);
        if (p.status) return p.status;
        std::vector<std::string> words;
        dwpa::assoc_single(p.mac_ap, p.essid, minlen, &words);
        size_t total = 0;
        for (const std::string& w : words) total += w.size();
        *nwords = words.size();
        *nbytes = total;
        if (words.size() > lens_cap || total > out_cap || (words.size() && (!out || !lens))) return DWPA_E_OVERFLOW;
        size_t at = 0;
        for (size_t k = 0; k < words.size(); k++) {
            memcpy(out + at, words[k].data(), words[k].size());
            at += words[k].size();
            lens[k] = (uint32_t)words[k].size();
        }
        return 0;
    });
}

extern "C" int dwpa_assoc_plan(const char* hash_file, const char* assoc_file, uint32_t flags, const char* rules_file,
                               dwpa_assoc_info* out) {
    return dwpa::guarded([&]() -> int {
        if (!out) return DWPA_E_ARG;
        dwpa::AssocAttack at;
        const int r = dwpa::assoc_prepare(hash_file, assoc_file, flags, rules_file, DWPA_RULES_DEFAULT, &at);
        if (r < 0) return r;
        const dwpa::AssocPlan& p = at.plan;
        *out = dwpa_assoc_info{p.keyspace(), p.nets.nets.size(), p.entries(), p.file_lines, p.unmatched, p.malformed,
                               p.dropped, p.R, 0};
        return 0;
    });
}

extern "C" int dwpa_assoc_candidates(const char* hash_file, const char* assoc_file, uint32_t flags,
                                     const char* rules_file, const uint64_t* indices, size_t n, uint8_t* out,
                                     uint32_t* out_len, uint32_t* first_line) {
    return dwpa::guarded([&]() -> int {
        if (n && (!indices || !out || !out_len)) return DWPA_E_ARG;
        dwpa::AssocAttack at;
        const int r = dwpa::assoc_prepare(hash_file, assoc_file, flags, rules_file, DWPA_RULES_DEFAULT, &at);
        if (r < 0) return r;
        const dwpa::AssocPlan& p = at.plan;
        std::string c;
        for (size_t k = 0; k < n; k++) {
            if (indices[k] >= p.keyspace()) return DWPA_E_ARG;
            size_t net = 0;
            memset(out + 64 * k, 0, 64);
            if (p.candidate(indices[k], &c, &net)) {
                memcpy(out + 64 * k, c.data(), c.size());
                out_len[k] = (uint32_t)c.size();
            } else {
                out_len[k] = 0xffffffffu;
            }
            if (first_line) first_line[k] = p.nets.nets[net].lines[0];
        }
        return 0;
    });
}

extern "C" int dwpa_crack_assoc(const char* hash_file, const char* assoc_file, uint32_t flags, const char* rules_file,
                                uint64_t skip, uint64_t limit, int nonce_error_corrections, const char* out_file,
                                const dwpa_config* cfg) {
    return dwpa::guarded([&]() -> int {
        return dwpa::crack_assoc_impl(hash_file, assoc_file, flags, rules_file, skip, limit, nonce_error_corrections,
                                      out_file, cfg);
    }, DWPA_RC_ERROR, DWPA_RC_ERROR);
}

extern "C" int dwpa_crack_table(const char* hash_file, const char* dict, const char* table_file, uint32_t word_max,
                                uint64_t skip, uint64_t limit, int nonce_error_corrections, const char* out_file,
                                const dwpa_config* cfg) {
    return dwpa::guarded([&]() -> int {
        return dwpa::crack_table_impl(hash_file, dict, table_file, word_max, skip, limit, nonce_error_corrections,
                                      out_file, cfg);
    }, DWPA_RC_ERROR, DWPA_RC_ERROR);
}

extern "C" int dwpa_crack_mask(const char* hash_file, const char* mask, const dwpa_bytes custom[4], uint64_t skip,
                               uint64_t limit, uint32_t increment_min, uint32_t increment_max,
                               int nonce_error_corrections, const char* out_file, const dwpa_config* cfg) {
    return dwpa::guarded([&]() -> int {
        return dwpa::crack_mask_impl(hash_file, mask, custom, skip, limit, increment_min, increment_max,
                                     nonce_error_corrections, out_file, cfg);
    }, DWPA_RC_ERROR, DWPA_RC_ERROR);
}

extern "C" int dwpa_crack_mask_markov(const char* hash_file, const char* mask, const dwpa_bytes custom[4],
                                      const char* markov_file, uint32_t threshold, uint64_t skip, uint64_t limit,
                                      uint32_t increment_min, uint32_t increment_max, int nonce_error_corrections,
                                      const char* out_file, const dwpa_config* cfg) {
    return dwpa::guarded([&]() -> int {
        return dwpa::crack_mask_markov_impl(hash_file, mask, custom, markov_file, threshold, skip, limit, increment_min,
                                            increment_max, nonce_error_corrections, out_file, cfg);
    }, DWPA_RC_ERROR, DWPA_RC_ERROR);
}

extern "C" int dwpa_crack_chain(const char* hash_file, const dwpa_chain_spec* parts, uint32_t nparts,
                                const dwpa_bytes custom[4], uint64_t skip, uint64_t limit,
                                int nonce_error_corrections, const char* out_file, const dwpa_config* cfg,
                                int32_t* part_status) {
    return dwpa::guarded([&]() -> int {
        return dwpa::crack_chain_impl(hash_file, parts, nparts, nullptr, custom, skip, limit,
                                      nonce_error_corrections, out_file, cfg, part_status);
    }, DWPA_RC_ERROR, DWPA_RC_ERROR);
}

extern "C" int dwpa_crack_chain_rules(const char* hash_file, const dwpa_chain_spec* parts, uint32_t nparts,
                                      const char* const* part_rules, const dwpa_bytes custom[4], uint64_t skip,
                                      uint64_t limit, int nonce_error_corrections, const char* out_file,
                                      const dwpa_config* cfg, int32_t* part_status) {
    return dwpa::guarded([&]() -> int {
        return dwpa::crack_chain_impl(hash_file, parts, nparts, part_rules, custom, skip, limit,
                                      nonce_error_corrections, out_file, cfg, part_status);
    }, DWPA_RC_ERROR, DWPA_RC_ERROR);
}
