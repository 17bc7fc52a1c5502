// crack_mask.cpp -- dwpa_crack_mask(): hashcat -a 3 (mask attack) over an m22000 hash file, with dwpa_crack_files'
// hash file, rc convention, outfile records, nc-mode default and cfg handling.
//
// There is no dictionary feed, so none of crack.cpp's reader / item-queue machinery: the keyspace is a list of
// segments (one per mask length that runs: the mask itself, or with increment its prefixes, shortest first), and
// every worker -- DWPA_CRACK_SHARDS_PER_DEVICE per selected device -- takes batch-sized ascending index ranges from
// one shared cursor, generates them on its device (dwpa_scan_load_mask), scans them and reports.  A hit's PSK is
// rebuilt on the host from its index; the first hit of a line is written once, under the mutex, and the line is
// retired on every worker before its next launch.  A fully cracked file stops every worker.
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
#include "engine.hpp"
#include "m22000_host.hpp"
#include "mask.hpp"

namespace dwpa {

namespace {

struct Segment {
    uint32_t npos;          // positions of this prefix
    uint64_t begin, end;    // indices [begin, end) of its keyspace
};

struct MaskShared {
    std::mutex mu;
    std::vector<uint8_t> cracked;  // per input line (1: cracked, or never usable)
    std::vector<ParsedLine> parsed;
    FILE* out = nullptr;
    size_t valid = 0, ncracked = 0;
    std::atomic<uint32_t> version{0};
    std::atomic<bool> stop{false};
    std::atomic<int> error{0};
    // the shared cursor (under mu)
    std::vector<Segment> segs;
    size_t seg = 0;
    uint64_t next = 0;  // next index of segs[seg]
};

struct MaskWork {
    int device = 0;
    dwpa_scan* scan = nullptr;
    hipStream_t stream = nullptr;
    uint32_t seen_version = 0;
    uint32_t items = 0;
    uint64_t cands = 0;
    double scan_s = 0;
};

// The next batch of the keyspace: segment index, first index, count.  False at the end.
bool take(MaskShared& sh, uint32_t batch, size_t* seg, uint64_t* first, uint32_t* count) {
    std::lock_guard<std::mutex> lk(sh.mu);
    while (sh.seg < sh.segs.size() && sh.next >= sh.segs[sh.seg].end) {
        sh.seg++;
        if (sh.seg < sh.segs.size()) sh.next = sh.segs[sh.seg].begin;
    }
    if (sh.seg >= sh.segs.size()) return false;
    *seg = sh.seg;
    *first = sh.next;
    *count = (uint32_t)std::min<uint64_t>(batch, sh.segs[sh.seg].end - sh.next);
    sh.next += *count;
    return true;
}

int worker(MaskWork& w, MaskShared& sh, const Mask& full) {
    if (hipSetDevice(w.device) != hipSuccess) return DWPA_E_HIP;
    const uint32_t cap = scan_batch_cap(w.scan);
    auto cur = std::make_unique<Mask>();  // the prefix this worker's scan holds
    size_t cur_seg = (size_t)-1;
    size_t seg;
    uint64_t first;
    uint32_t count;
    std::vector<HitDev> hits;
    while (!sh.stop.load(std::memory_order_relaxed) && take(sh, cap, &seg, &first, &count)) {
        const auto ts = std::chrono::steady_clock::now();
        int r;
        if (seg != cur_seg) {
            mask_prefix(full, sh.segs[seg].npos, cur.get());
            if ((r = scan_set_mask(w.scan, *cur)) < 0) return r;
            cur_seg = seg;
        }
        if ((r = scan_load_mask(w.scan, first, count, w.stream)) < 0) return r;
        const uint32_t v = sh.version.load(std::memory_order_acquire);
        if (v != w.seen_version) {  // retire every line cracked anywhere so far
            std::lock_guard<std::mutex> lk(sh.mu);
            for (size_t i = 0; i < sh.cracked.size(); i++)
                if (sh.cracked[i]) scan_mark_cracked(w.scan, (uint32_t)i);
            w.seen_version = v;
        }
        if ((r = scan_run(w.scan, w.stream)) < 0) return r;
        if ((r = scan_hits_raw(w.scan, hits, w.stream)) < 0) return r;
        w.items++;
        w.cands += count;
        w.scan_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - ts).count();
        if (hits.empty()) continue;
        std::sort(hits.begin(), hits.end(), [](const HitDev& x, const HitDev& y) { return x.cand < y.cand; });
        std::lock_guard<std::mutex> lk(sh.mu);
        for (const HitDev& h : hits) {
            dwpa_hit ph;
            hit_to_public(w.scan, h, ph);
            if (sh.cracked[ph.line] || h.cand >= cur->keyspace) continue;
            uint8_t psk[64];
            mask_candidate(*cur, h.cand, psk);
            sh.cracked[ph.line] = 1;
            sh.ncracked++;
            sh.version.fetch_add(1, std::memory_order_acq_rel);
            const std::string rec = outfile_record(sh.parsed[ph.line], std::string((const char*)psk, cur->npos));
            fwrite(rec.data(), 1, rec.size(), sh.out);
            fflush(sh.out);
        }
        if (sh.ncracked == sh.valid) sh.stop = true;
    }
    return 0;
}

int crack_mask_impl(const char* hash_file, const char* mask, const dwpa_bytes* custom, uint64_t skip, uint64_t limit,
                    uint32_t inc_min, uint32_t inc_max, int nec, const char* out_file, const dwpa_config* cfg) {
    const auto t_call = std::chrono::steady_clock::now();
    dwpa_crack_stats st{};
    std::vector<dwpa_crack_worker> wst;
    crack_publish_stats(st, wst);  // an early return reports zeros, never the previous call
    if (!hash_file || !mask || !out_file) return DWPA_RC_ERROR;
    if (cfg && cfg->struct_size && cfg->struct_size < offsetof(dwpa_config, batch)) return DWPA_RC_ERROR;
    if (nec > DWPA_NC_MAX) {
        fprintf(stderr, "[dwpa] --nonce-error-corrections=%d is above the supported %d\n", nec, DWPA_NC_MAX);
        return DWPA_RC_ERROR;
    }
    auto full = std::make_unique<Mask>();
    if (mask_parse(mask, strlen(mask), custom, full.get()) < 0) {
        fprintf(stderr, "[dwpa] mask %s: invalid (syntax, an undefined custom set, more than 63 positions or a keyspace "
                        "above 2^64 - 1)\n", mask);
        return DWPA_RC_ERROR;
    }
    const bool increment = inc_min || inc_max;
    if (increment && (skip || limit)) {
        fprintf(stderr, "[dwpa] --increment cannot be combined with --skip / --limit\n");
        return DWPA_RC_ERROR;
    }
    MaskShared sh;
    if (increment) {
        const uint32_t lo = std::max<uint32_t>(1, inc_min), hi = std::min(inc_max ? inc_max : full->npos, full->npos);
        if (lo > hi) return DWPA_RC_ERROR;
        auto pre = std::make_unique<Mask>();
        for (uint32_t n = lo; n <= hi; n++) {
            if (n < 8) {  // hashcat skips a mask shorter than the hash mode's shortest password
                fprintf(stderr, "[dwpa] skipping the mask's first %u positions: m22000 takes 8..63 characters\n", n);
                continue;
            }
            mask_prefix(*full, n, pre.get());
            sh.segs.push_back(Segment{n, 0, pre->keyspace});
        }
    } else if (full->npos < 8) {
        fprintf(stderr, "[dwpa] skipping mask %s: %u positions, m22000 takes 8..63 characters\n", mask, full->npos);
    } else {
        if (skip >= full->keyspace) {
            fprintf(stderr, "[dwpa] --skip is not below the keyspace\n");
            return DWPA_RC_ERROR;
        }
        const uint64_t room = full->keyspace - skip;
        sh.segs.push_back(Segment{full->npos, skip, skip + (limit && limit < room ? limit : room)});
    }
    if (sh.segs.empty()) return DWPA_RC_ERROR;  // nothing left to run
    sh.next = sh.segs[0].begin;

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
    std::vector<std::unique_ptr<MaskWork>> work;
    int rc = 0;
    for (int dev : devs)
        for (size_t k = 0; k < spd && rc >= 0; k++) {
            work.push_back(std::make_unique<MaskWork>());
            MaskWork& w = *work.back();
            w.device = dev;
            (void)hipSetDevice(dev);
            if (hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking) != hipSuccess) rc = DWPA_E_HIP;
            if (rc >= 0) rc = scan_create(dev, lp.data(), ll.data(), lines.size(), nec, nc_mode, batch, &w.scan);
        }
    std::vector<std::thread> th;
    if (rc >= 0) try {
        for (auto& wp : work)
            th.emplace_back([&sh, &full, w = wp.get()] {
                const int r = guarded([&] { return worker(*w, sh, *full); });
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
        if (wp->scan) scan_destroy(wp->scan);
        (void)hipSetDevice(wp->device);
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

extern "C" int dwpa_crack_mask(const char* hash_file, const char* mask, const dwpa_bytes custom[4], uint64_t skip,
                               uint64_t limit, uint32_t increment_min, uint32_t increment_max,
                               int nonce_error_corrections, const char* out_file, const dwpa_config* cfg) {
    return dwpa::guarded([&]() -> int {
        return dwpa::crack_mask_impl(hash_file, mask, custom, skip, limit, increment_min, increment_max,
                                     nonce_error_corrections, out_file, cfg);
    }, DWPA_RC_ERROR, DWPA_RC_ERROR);
}
