// crack_chain.cpp -- dwpa_crack_chain(): a chain of 1..4 word lists and masks (chain.hpp) over an m22000 hash file,
// with dwpa_crack_mask's hash file, rc convention, outfile records, nc-mode default and cfg handling.
//
// Built like crack_mask.cpp, not like crack.cpp: nothing is streamed.  Every list is read whole through the
// dictionary reader once (plain or gzip, CRLF, $HEX[]), kept on the host to rebuild a hit's PSK and uploaded once per
// worker.  The keyspace is one range of raw indices [skip, skip + limit): every worker --
// DWPA_CRACK_SHARDS_PER_DEVICE per selected device -- takes batch-sized ascending ranges of it from one shared
// cursor, generates them on its device (dwpa_scan_load_chain: the 8..63 filter and the compaction run in
// k_prep_chain), scans them and reports.  A load is `batch` raw indices, so PBKDF2 runs over the kept ones only: a
// chain whose filter drops most candidates runs short launches (filling a batch from several raw ranges is left for
// later).  The first hit of a line is written once, under the mutex, and the line is retired on every worker before
// its next launch.  A fully cracked file stops every worker.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "dwpa22000.h"
#include "chain.hpp"
#include "dict_reader.hpp"
#include "engine.hpp"
#include "m22000_host.hpp"
#include "mask.hpp"

namespace dwpa {

namespace {

struct HostPart {
    bool is_mask = false;
    std::unique_ptr<Mask> mask;
    std::vector<uint64_t> off{0};  // N + 1 offsets into bytes
    std::string bytes;
    uint64_t radix = 0;
};

struct ChainShared {
    std::mutex mu;
    std::vector<uint8_t> cracked;  // per input line (1: cracked, or never usable)
    std::vector<ParsedLine> parsed;
    FILE* out = nullptr;
    size_t valid = 0, ncracked = 0;
    std::atomic<uint32_t> version{0};
    std::atomic<bool> stop{false};
    std::atomic<int> error{0};
    uint64_t next = 0, end = 0;  // the shared cursor (under mu): raw indices [next, end) are left
};

struct ChainWork {
    int device = 0;
    dwpa_scan* scan = nullptr;
    hipStream_t stream = nullptr;
    DevBuf off[CHAIN_MAX_PARTS], bytes[CHAIN_MAX_PARTS];  // the lists on this worker's device
    uint32_t seen_version = 0;
    uint32_t items = 0;
    uint64_t cands = 0;  // kept candidates derived
    double scan_s = 0;
};

// A list through the dictionary reader, whole.  DWPA_E_IO: a read error; DWPA_E_OVERFLOW: above the limits.
int read_list(const char* path, HostPart* hp, int32_t* status) {
    DictReader rd({std::string(path)});
    Chunk c;
    bool err = false;
    while (rd.next(c, (size_t)1 << 20, (size_t)64 << 20, err)) {
        const uint64_t at = hp->bytes.size();
        hp->bytes += c.bytes;
        for (size_t i = 1; i < c.off.size(); i++) hp->off.push_back(at + c.off[i]);
        if (hp->off.size() - 1 > UINT32_MAX || hp->bytes.size() + hp->off.size() * 8 > DWPA_COMBI_AMP_MAX_BYTES)
            return DWPA_E_OVERFLOW;
    }
    if (err) return DWPA_E_IO;
    if (rd.damaged() && status) *status = DWPA_DICT_DAMAGED;
    hp->radix = hp->off.size() - 1;
    return 0;
}

// Candidate `id` (< K) as its bytes: the parts' choices left to right.
std::string chain_candidate(const std::vector<HostPart>& parts, const uint64_t* radix, uint64_t id) {
    uint64_t digit[CHAIN_MAX_PARTS];
    std::string psk;
    if (chain_split(radix, (uint32_t)parts.size(), id, digit) < 0) return psk;
    for (size_t p = 0; p < parts.size(); p++) {
        const HostPart& hp = parts[p];
        if (hp.is_mask) {
            uint8_t m[64];
            mask_candidate(*hp.mask, digit[p], m);
            psk.append((const char*)m, hp.mask->npos);
        } else {
            psk.append(hp.bytes, (size_t)hp.off[digit[p]], (size_t)(hp.off[digit[p] + 1] - hp.off[digit[p]]));
        }
    }
    return psk;
}

// The next batch of the range: first index and count.  False at the end.
bool take(ChainShared& sh, uint32_t batch, uint64_t* first, uint32_t* count) {
    std::lock_guard<std::mutex> lk(sh.mu);
    if (sh.next >= sh.end) return false;
    *first = sh.next;
    *count = (uint32_t)std::min<uint64_t>(batch, sh.end - sh.next);
    sh.next += *count;
    return true;
}

int worker(ChainWork& w, ChainShared& sh, const std::vector<HostPart>& parts, const uint64_t* radix, uint64_t K) {
    if (hipSetDevice(w.device) != hipSuccess) return DWPA_E_HIP;
    const uint32_t cap = scan_batch_cap(w.scan);
    uint64_t first;
    uint32_t count;
    std::vector<HitDev> hits;
    while (!sh.stop.load(std::memory_order_relaxed) && take(sh, cap, &first, &count)) {
        const auto ts = std::chrono::steady_clock::now();
        int r;
        if ((r = scan_load_chain(w.scan, first, count, 8, 63, w.stream)) < 0) return r;
        const uint32_t v = sh.version.load(std::memory_order_acquire);
        if (v != w.seen_version) {  // retire every line cracked anywhere so far
            std::lock_guard<std::mutex> lk(sh.mu);
            for (size_t i = 0; i < sh.cracked.size(); i++)
                if (sh.cracked[i]) scan_mark_cracked(w.scan, (uint32_t)i);
            w.seen_version = v;
        }
        if ((r = scan_run(w.scan, w.stream)) < 0) return r;
        if ((r = scan_hits_raw(w.scan, hits, w.stream)) < 0) return r;
        uint32_t kept = 0;  // the stream is idle by now: this copy waits for nothing
        if ((r = scan_counter_raw(w.scan, w.stream, &kept)) < 0) return r;
        w.items++;
        w.cands += kept;
        w.scan_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - ts).count();
        if (hits.empty()) continue;
        std::sort(hits.begin(), hits.end(), [](const HitDev& x, const HitDev& y) { return x.cand < y.cand; });
        std::lock_guard<std::mutex> lk(sh.mu);
        for (const HitDev& h : hits) {
            dwpa_hit ph;
            hit_to_public(w.scan, h, ph);
            if (sh.cracked[ph.line] || h.cand >= K) continue;
            sh.cracked[ph.line] = 1;
            sh.ncracked++;
            sh.version.fetch_add(1, std::memory_order_acq_rel);
            const std::string rec = outfile_record(sh.parsed[ph.line], chain_candidate(parts, radix, h.cand));
            fwrite(rec.data(), 1, rec.size(), sh.out);
            fflush(sh.out);
        }
        if (sh.ncracked == sh.valid) sh.stop = true;
    }
    return 0;
}

int crack_chain_impl(const char* hash_file, const dwpa_chain_spec* specs, uint32_t nparts, const dwpa_bytes* custom,
                     uint64_t skip, uint64_t limit, int nec, const char* out_file, const dwpa_config* cfg,
                     int32_t* part_status) {
    const auto t_call = std::chrono::steady_clock::now();
    dwpa_crack_stats st{};
    std::vector<dwpa_crack_worker> wst;
    crack_publish_stats(st, wst);  // an early return reports zeros, never the previous call
    if (nparts == 0 || nparts > CHAIN_MAX_PARTS) {
        fprintf(stderr, "[dwpa] a chain takes 1..%u parts\n", CHAIN_MAX_PARTS);
        return DWPA_RC_ERROR;
    }
    if (part_status)
        for (uint32_t p = 0; p < nparts; p++) part_status[p] = DWPA_DICT_OK;
    if (!hash_file || !specs || !out_file) return DWPA_RC_ERROR;
    if (cfg && cfg->struct_size && cfg->struct_size < offsetof(dwpa_config, batch)) return DWPA_RC_ERROR;
    if (nec > DWPA_NC_MAX) {
        fprintf(stderr, "[dwpa] --nonce-error-corrections=%d is above the supported %d\n", nec, DWPA_NC_MAX);
        return DWPA_RC_ERROR;
    }
    // every part is looked at before the call fails, so that each unreadable list is marked
    std::vector<HostPart> parts(nparts);
    bool bad = false;
    for (uint32_t p = 0; p < nparts; p++) {
        const char* text = specs[p].text;
        if (specs[p].kind == DWPA_CHAIN_MASK) {
            parts[p].is_mask = true;
            parts[p].mask = std::make_unique<Mask>();
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
    {
        FILE* f = fopen(hash_file, "rb");
        if (!f) return DWPA_RC_ERROR;
        fclose(f);
    }
    uint64_t radix[CHAIN_MAX_PARTS] = {};
    for (uint32_t p = 0; p < nparts; p++) {
        if (!parts[p].is_mask) {
            const int r = read_list(specs[p].text, &parts[p], part_status ? &part_status[p] : nullptr);
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
            st.words += parts[p].radix;
        }
        radix[p] = parts[p].radix;
    }
    uint64_t K;
    if (chain_keyspace(radix, nparts, &K) < 0) {
        fprintf(stderr, "[dwpa] the chain's keyspace is above 2^64 - 1\n");
        return DWPA_RC_ERROR;
    }
    if (K > 0 && skip >= K) {
        fprintf(stderr, "[dwpa] --skip is not below the keyspace\n");
        return DWPA_RC_ERROR;
    }
    ChainShared sh;
    if (K > 0) {
        const uint64_t room = K - skip;
        sh.next = skip;
        sh.end = skip + (limit && limit < room ? limit : room);
    }

    if (engine_init() < 0) return DWPA_RC_ERROR;
    std::vector<int> devs = engine_devices(DWPA_CFG_HAS(cfg, device_mask) ? cfg->device_mask : 0);
    if (devs.empty()) return DWPA_RC_ERROR;
    const int nc_mode = DWPA_CFG_HAS(cfg, nc_mode) ? cfg->nc_mode : DWPA_NC_HASHCAT;

    std::vector<std::string> lines;
    if (!read_hash_file(hash_file, lines)) return DWPA_RC_ERROR;
    sh.parsed.resize(lines.size());
    sh.cracked.assign(lines.size(), 0);
    for (size_t i = 0; i < lines.size(); i++) {
        sh.parsed[i] = parse_m22000(lines[i].data(), lines[i].size());
        if (sh.parsed[i].status || !line_can_match(sh.parsed[i])) sh.cracked[i] = 1;  // as dwpa_crack_files
        else sh.valid++;
    }
    if (sh.valid == 0) return DWPA_RC_ERROR;  // hashcat: "No hashes loaded"
    sh.out = fopen(out_file, "ab");
    if (!sh.out) return DWPA_RC_ERROR;

    std::vector<const char*> lp(lines.size());
    std::vector<size_t> ll(lines.size());
    for (size_t i = 0; i < lines.size(); i++) { lp[i] = lines[i].data(); ll[i] = lines[i].size(); }
    const uint32_t batch = DWPA_CFG_HAS(cfg, batch) && cfg->batch ? cfg->batch : engine_batch();
    const size_t spd = crack_shards_per_device();
    std::vector<std::unique_ptr<ChainWork>> work;
    int rc = 0;
    for (int dev : devs)
        for (size_t k = 0; k < spd && rc >= 0; k++) {
            work.push_back(std::make_unique<ChainWork>());
            ChainWork& w = *work.back();
            w.device = dev;
            (void)hipSetDevice(dev);
            if (hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking) != hipSuccess) rc = DWPA_E_HIP;
            if (rc >= 0) rc = scan_create(dev, lp.data(), ll.data(), lines.size(), nec, nc_mode, batch, &w.scan);
            dwpa_chain_part cp[CHAIN_MAX_PARTS] = {};
            for (uint32_t p = 0; p < nparts && rc >= 0; p++) {
                const HostPart& hp = parts[p];
                if (hp.is_mask) {
                    cp[p].kind = DWPA_CHAIN_MASK;
                    cp[p].mask = specs[p].text;
                    cp[p].mask_len = strlen(specs[p].text);
                    continue;
                }
                if (w.off[p].ensure(hp.off.size() * 8) || w.bytes[p].ensure(hp.bytes.size() + 64)) {
                    rc = DWPA_E_NOMEM;
                } else if (hipMemcpy(w.off[p].p, hp.off.data(), hp.off.size() * 8, hipMemcpyHostToDevice) !=
                               hipSuccess ||
                           (!hp.bytes.empty() && hipMemcpy(w.bytes[p].p, hp.bytes.data(), hp.bytes.size(),
                                                           hipMemcpyHostToDevice) != hipSuccess)) {
                    rc = DWPA_E_HIP;
                }
                cp[p].kind = DWPA_CHAIN_LIST;
                cp[p].d_offsets = (const uint64_t*)w.off[p].p;
                cp[p].d_bytes = (const uint8_t*)w.bytes[p].p;
                cp[p].nwords = hp.radix;
            }
            if (rc >= 0) rc = scan_set_chain(w.scan, cp, nparts, custom, nullptr);
        }
    std::vector<std::thread> th;
    if (rc >= 0) try {
        for (auto& wp : work)
            th.emplace_back([&sh, &parts, &radix, K, w = wp.get()] {
                const int r = guarded([&] { return worker(*w, sh, parts, radix, K); });
                if (r < 0) {
                    int z = 0;
                    sh.error.compare_exchange_strong(z, r);
                    sh.stop = true;
                }
            });
    } catch (...) {  // a thread that cannot start stops the ones that did
        int z = 0;
        sh.error.compare_exchange_strong(z, DWPA_E_NOMEM);
        sh.stop = true;
    }
    for (auto& t : th) t.join();
    for (auto& wp : work) {
        if (wp->scan) scan_destroy(wp->scan);  // waits for the device: the lists are free after it
        (void)hipSetDevice(wp->device);
        for (uint32_t p = 0; p < CHAIN_MAX_PARTS; p++) {
            wp->off[p].release();
            wp->bytes[p].release();
        }
        if (wp->stream) (void)hipStreamDestroy(wp->stream);
        st.candidates += wp->cands;
        wst.push_back(dwpa_crack_worker{wp->device, wp->items, 0, wp->cands, 0.0, wp->scan_s});
    }
    fclose(sh.out);
    st.hashes = (uint32_t)sh.valid;
    st.cracked = (uint32_t)sh.ncracked;
    st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_call).count();
    crack_publish_stats(st, wst);
    if (rc < 0 || sh.error.load() < 0) return DWPA_RC_ERROR;
    return sh.ncracked == sh.valid ? DWPA_RC_CRACKED : DWPA_RC_EXHAUSTED;
}

}  // namespace

}  // namespace dwpa

extern "C" int dwpa_crack_chain(const char* hash_file, const dwpa_chain_spec* parts, uint32_t nparts,
                                const dwpa_bytes custom[4], uint64_t skip, uint64_t limit,
                                int nonce_error_corrections, const char* out_file, const dwpa_config* cfg,
                                int32_t* part_status) {
    return dwpa::guarded([&]() -> int {
        return dwpa::crack_chain_impl(hash_file, parts, nparts, custom, skip, limit, nonce_error_corrections,
                                      out_file, cfg, part_status);
    }, DWPA_RC_ERROR, DWPA_RC_ERROR);
}
