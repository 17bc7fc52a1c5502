// crack_common.cpp -- the call frame of the five crack calls (crack_common.hpp), and the two calls that report a crack
// call's statistics.
#include "crack_common.hpp"

#include <stddef.h>
#include <stdlib.h>

#include <thread>

#include "dict_reader.hpp"

namespace dwpa {

std::string outfile_record(const ParsedLine& p, const std::string& psk) {
    const std::string& target = p.kind == LINE_PMKID ? p.pmkid : p.keymic;
    return hex_lower(target.substr(0, 16)) + ":" + hex_lower(p.mac_ap) + ":" + hex_lower(p.mac_sta) + ":" +
           hashcat_plain(p.essid) + ":" + hashcat_plain(psk) + "\n";
}

// DWPA_CRACK_SHARDS_PER_DEVICE=k runs k shard workers per selected device (default 1).  On a one-GPU box k = 2
// rehearses the multi-device path -- per-worker queues, shard scans and cross-worker line retirement -- that a
// volunteer's 8-GPU node runs (hashcat uses every device, help_crack.py:773).
size_t crack_shards_per_device() {
    const char* e = getenv("DWPA_CRACK_SHARDS_PER_DEVICE");
    const long k = e ? strtol(e, nullptr, 10) : 1;
    return (size_t)std::min<long>(8, std::max<long>(1, k));
}

// dwpa_crack_last_stats / dwpa_crack_worker_stats: the calling thread's last crack call
static thread_local dwpa_crack_stats g_last_stats;
static thread_local std::vector<dwpa_crack_worker> g_last_workers;
static thread_local bool g_have_stats = false;

void crack_publish_stats(const dwpa_crack_stats& st, const std::vector<dwpa_crack_worker>& workers) {
    g_last_stats = st;
    g_last_workers = workers;
    g_have_stats = true;
}

// One m22000 line per line (LF or CRLF), empty lines dropped.
bool read_hash_file(const char* path, std::vector<std::string>& lines) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    std::string cur;
    int ch;
    while ((ch = fgetc(f)) != EOF) {
        if (ch == '\n') {
            if (!cur.empty() && cur.back() == '\r') cur.pop_back();
            if (!cur.empty()) lines.push_back(cur);
            cur.clear();
        } else cur.push_back((char)ch);
    }
    if (!cur.empty() && cur.back() == '\r') cur.pop_back();
    if (!cur.empty()) lines.push_back(cur);
    fclose(f);
    return true;
}

bool CrackShared::load_hashes(const char* hash_file, HashLines* hl) {
    if (!read_hash_file(hash_file, hl->lines)) return false;
    const size_t n = hl->lines.size();
    parsed.resize(n);
    cracked.assign(n, 0);
    hl->ptr.resize(n);
    hl->len.resize(n);
    for (size_t i = 0; i < n; i++) {
        hl->ptr[i] = hl->lines[i].data();
        hl->len[i] = hl->lines[i].size();
        parsed[i] = parse_m22000(hl->ptr[i], hl->len[i]);
        // rejected by the parser (hashcat: token exception), or a PMKID/MIC shorter than 16 bytes that can never
        // verify (hashcat refuses such a hash at load time): neither is counted, so rc 0 stays reachable
        if (parsed[i].status || !line_can_match(parsed[i])) cracked[i] = 1;
        else valid++;
    }
    return valid != 0;  // hashcat: "No hashes loaded"
}

bool CrackShared::open_out(const char* out_file) {
    out = fopen(out_file, "ab");
    return out != nullptr;
}

int CrackCall::finish(const CrackShared& sh, const std::vector<dwpa_crack_worker>& workers, bool failed) {
    for (const dwpa_crack_worker& w : workers) {
        st.words += w.words;
        st.candidates += w.candidates;
    }
    st.hashes = (uint32_t)sh.valid;
    st.cracked = (uint32_t)sh.ncracked;
    st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    crack_publish_stats(st, workers);
    if (failed || sh.error.load() < 0) return DWPA_RC_ERROR;
    return sh.ncracked == sh.valid ? DWPA_RC_CRACKED : DWPA_RC_EXHAUSTED;
}

bool crack_check_args(const dwpa_config* cfg, int nec) {
    if (cfg && cfg->struct_size && cfg->struct_size < offsetof(dwpa_config, batch)) return false;
    if (nec > DWPA_NC_MAX) {
        fprintf(stderr, "[dwpa] --nonce-error-corrections=%d is above the supported %d\n", nec, DWPA_NC_MAX);
        return false;
    }
    return true;
}

bool crack_plan(const dwpa_config* cfg, int nec, CrackPlan* plan) {
    if (engine_init() < 0) return false;
    plan->devs = engine_devices(DWPA_CFG_HAS(cfg, device_mask) ? cfg->device_mask : 0);
    plan->nec = nec;
    plan->nc_mode = DWPA_CFG_HAS(cfg, nc_mode) ? cfg->nc_mode : DWPA_NC_HASHCAT;
    plan->batch = DWPA_CFG_HAS(cfg, batch) && cfg->batch ? cfg->batch : engine_batch();
    plan->shards = crack_shards_per_device();
    return !plan->devs.empty();
}

int scan_worker_open(ScanWorker& w, int device, const HashLines& hl, const CrackPlan& plan) {
    w.device = device;
    (void)hipSetDevice(device);
    if (hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking) != hipSuccess) return DWPA_E_HIP;
    return scan_create(device, hl.ptr.data(), hl.len.data(), hl.lines.size(), plan.nec, plan.nc_mode, plan.batch, &w.scan);
}

void scan_worker_close(ScanWorker& w) {
    if (w.scan) scan_destroy(w.scan);
    (void)hipSetDevice(w.device);
    if (w.stream) (void)hipStreamDestroy(w.stream);
    w.scan = nullptr;
    w.stream = nullptr;
}

void sync_retired(ScanWorker& w, CrackShared& sh) {
    const uint32_t v = sh.version.load(std::memory_order_acquire);
    if (v == w.seen_version) return;
    std::lock_guard<std::mutex> lk(sh.mu);
    for (size_t i = 0; i < sh.cracked.size(); i++)
        if (sh.cracked[i]) scan_mark_cracked(w.scan, (uint32_t)i);
    w.seen_version = v;
}

void run_workers(CrackShared& sh, size_t n, const std::function<int(size_t)>& body) {
    std::vector<std::thread> th;  // never unwinds with joinable threads in it
    try {
        for (size_t k = 0; k < n; k++)
            th.emplace_back([&sh, &body, k] {
                const int r = guarded([&] { return body(k); });
                if (r < 0) sh.fail(r);
            });
    } catch (...) {
        sh.fail(DWPA_E_NOMEM);
    }
    for (auto& t : th) t.join();
}

int read_list(const char* path, HostList* l) {
    DictReader rd({std::string(path)});
    Chunk c;
    bool err = false;
    while (rd.next(c, (size_t)1 << 20, (size_t)64 << 20, err)) {
        const uint64_t at = l->bytes.size();
        l->bytes += c.bytes;
        for (size_t i = 1; i < c.off.size(); i++) l->off.push_back(at + c.off[i]);
        if (l->words() > UINT32_MAX || l->bytes.size() + l->off.size() * 8 > DWPA_COMBI_AMP_MAX_BYTES)
            return DWPA_E_OVERFLOW;
    }
    if (err) return DWPA_E_IO;
    l->damaged = rd.damaged();
    return 0;
}

int upload_list(const HostList& l, DevBuf* off, DevBuf* bytes) {
    if (off->ensure(l.off.size() * 8) || bytes->ensure(l.bytes.size() + 64)) return DWPA_E_NOMEM;
    if (hipMemcpy(off->p, l.off.data(), l.off.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
        (!l.bytes.empty() && hipMemcpy(bytes->p, l.bytes.data(), l.bytes.size(), hipMemcpyHostToDevice) != hipSuccess))
        return DWPA_E_HIP;
    return 0;
}

}  // namespace dwpa

extern "C" {

int dwpa_crack_last_stats(dwpa_crack_stats* out) {
    if (!out || !dwpa::g_have_stats) return DWPA_E_ARG;
    *out = dwpa::g_last_stats;
    return 0;
}

int dwpa_crack_worker_stats(dwpa_crack_worker* out, size_t cap, size_t* n) {
    if (!n || (!out && cap) || !dwpa::g_have_stats) return DWPA_E_ARG;
    *n = dwpa::g_last_workers.size();
    for (size_t i = 0; i < std::min(cap, *n); i++) out[i] = dwpa::g_last_workers[i];
    return 0;
}

}  // extern "C"
