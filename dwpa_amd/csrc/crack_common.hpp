// crack_common.hpp -- what the five crack calls share (crack.cpp: dwpa_crack_files, _hybrid, _combinator;
// crack_range.cpp: dwpa_crack_mask, _chain): the call's checks and statistics, the hash file and the outfile, a scan
// worker, line retirement and hit reporting, and a word list held whole.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "dwpa22000.h"
#include "engine.hpp"
#include "m22000_host.hpp"

namespace dwpa {

std::string outfile_record(const ParsedLine& p, const std::string& psk);
size_t crack_shards_per_device();  // DWPA_CRACK_SHARDS_PER_DEVICE, 1..8
bool read_hash_file(const char* path, std::vector<std::string>& lines);
// what dwpa_crack_last_stats / dwpa_crack_worker_stats report for the calling thread from now on
void crack_publish_stats(const dwpa_crack_stats& st, const std::vector<dwpa_crack_worker>& workers);

// Everything below is the library's own: it stays out of the dynamic symbol table.
#pragma GCC visibility push(hidden)

// The hash file as scan_create takes it.
struct HashLines {
    std::vector<std::string> lines;
    std::vector<const char*> ptr;
    std::vector<size_t> len;
};

// What the workers of one call share.
struct CrackShared {
    std::mutex mu;
    std::vector<uint8_t> cracked;         // per input line (1: cracked, or never usable)
    std::vector<ParsedLine> parsed;
    FILE* out = nullptr;
    size_t valid = 0, ncracked = 0;
    std::atomic<uint32_t> version{0};     // bumped for every newly cracked line: workers re-sync their scans
    std::atomic<bool> stop{false};        // every usable line cracked, or an error
    std::atomic<int> error{0};            // the first one

    ~CrackShared() { if (out) fclose(out); }
    // Read and parse the hash file.  False: it cannot be read, or no line of it is usable.
    bool load_hashes(const char* hash_file, HashLines* hl);
    bool open_out(const char* out_file);  // appending, as hashcat's outfile
    void fail(int r) {
        int z = 0;
        error.compare_exchange_strong(z, r);
        stop = true;
    }
};

// One crack call: its clock and its statistics, which an early return leaves at zero (never at the previous call's).
struct CrackCall {
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    dwpa_crack_stats st{};
    CrackCall() { crack_publish_stats(st, {}); }
    // The end of a call that got as far as its workers: their words and candidates summed into st, the lines and the
    // time filled in, all of it published.  DWPA_RC_ERROR if `failed` (set-up or I/O) or a worker failed, else
    // DWPA_RC_CRACKED or DWPA_RC_EXHAUSTED.
    int finish(const CrackShared& sh, const std::vector<dwpa_crack_worker>& workers, bool failed);
};

// cfg->struct_size and nonce_error_corrections, before anything else is looked at.  False: refused.
bool crack_check_args(const dwpa_config* cfg, int nec);

// Where and how a call runs: the config applies to this call only (dwpa_init's process-wide selection stays).
struct CrackPlan {
    std::vector<int> devs;
    int nec = 0, nc_mode = DWPA_NC_HASHCAT;
    uint32_t batch = 0;
    size_t shards = 1;  // workers per device
};
// Initialises the engine.  False: no device.
bool crack_plan(const dwpa_config* cfg, int nec, CrackPlan* plan);

// One scan on one device with its stream, and what it has done (DWPA_TRACE, dwpa_crack_worker_stats).
struct ScanWorker {
    int device = 0;
    dwpa_scan* scan = nullptr;
    hipStream_t stream = nullptr;
    uint32_t seen_version = 0;  // CrackShared::version this scan's retired lines reflect
    size_t items = 0;
    uint64_t cands = 0;         // candidates derived (inside the 8..63 filter, after rules)
    double scan_s = 0;
};
int scan_worker_open(ScanWorker& w, int device, const HashLines& hl, const CrackPlan& plan);
void scan_worker_close(ScanWorker& w);  // the scan first (it waits for the device), then the stream

// Retire on w's scan every line cracked anywhere so far (hashcat reports each hash once).
void sync_retired(ScanWorker& w, CrackShared& sh);

// The first hit of each line (lowest candidate id first) is written to the outfile once and the line retired;
// plain_of(id, &psk) rebuilds a candidate's PSK on the host from its id (false: no such candidate).
template <class F>
void report_hits(ScanWorker& w, CrackShared& sh, std::vector<HitDev>& hits, F&& plain_of) {
    std::sort(hits.begin(), hits.end(), [](const HitDev& x, const HitDev& y) { return x.cand < y.cand; });
    std::lock_guard<std::mutex> lk(sh.mu);
    std::string plain;
    for (const HitDev& h : hits) {
        dwpa_hit ph;
        hit_to_public(w.scan, h, ph);
        if (sh.cracked[ph.line]) continue;
        if (!plain_of(h.cand, &plain)) continue;
        sh.cracked[ph.line] = 1;
        sh.ncracked++;
        sh.version.fetch_add(1, std::memory_order_acq_rel);
        const std::string rec = outfile_record(sh.parsed[ph.line], plain);
        fwrite(rec.data(), 1, rec.size(), sh.out);
        fflush(sh.out);
    }
    if (sh.ncracked == sh.valid) sh.stop = true;
}

// Scan what was just loaded into w's scan (all ESSID groups, grouped per launch): retire, run, read the hits (the
// stream is idle afterwards) and report them.  The caller counts its candidates.
template <class F>
int scan_step(ScanWorker& w, CrackShared& sh, std::vector<HitDev>& hits, F&& plain_of) {
    sync_retired(w, sh);
    int r;
    if ((r = scan_run(w.scan, w.stream)) < 0) return r;
    if ((r = scan_hits_raw(w.scan, hits, w.stream)) < 0) return r;
    if (!hits.empty()) report_hits(w, sh, hits, plain_of);
    return 0;
}

// body(k) for k < n, each on its own thread, all joined.  The first negative return is the call's error and stops the
// others; a thread that cannot start (std::system_error, e.g. under RLIMIT_NPROC) stops the ones that did.
void run_workers(CrackShared& sh, size_t n, const std::function<int(size_t)>& body);

// A word list held whole on the host, to be uploaded once per worker and to rebuild a hit's PSK.
struct HostList {
    std::vector<uint64_t> off{0};  // words + 1 offsets into bytes
    std::string bytes;
    bool damaged = false;          // a gzip stream read up to its damage
    uint64_t words() const { return off.size() - 1; }
};
// Through the dictionary reader (plain or gzip, CRLF, $HEX[]).  DWPA_E_IO: a read error; DWPA_E_OVERFLOW: 2^32 words
// or more, or above DWPA_COMBI_AMP_MAX_BYTES.
int read_list(const char* path, HostList* l);
// To the current device, with the 64 bytes of padding a staged dictionary shard has.
int upload_list(const HostList& l, DevBuf* off, DevBuf* bytes);

#pragma GCC visibility pop

}  // namespace dwpa
