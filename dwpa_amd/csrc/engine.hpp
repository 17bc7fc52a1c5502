// engine.hpp -- the engine's own interface inside libdwpa22000.so (engine.cpp), as the host backend, the rule engine
// and the crack calls (crack_common.hpp, crack.cpp, crack_range.cpp) use it.
#pragma once
#include <stdint.h>

#include <functional>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "dwpa22000.h"
#include "tables.hpp"

namespace dwpa {

struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
    int ensure(size_t bytes);
    void release();
};

// Per-batch device working set (cap candidate slots).
struct Batch {
    uint32_t cap = 0, hitcap = 0;
    DevBuf mid;       // [10][cap] u32 HMAC key midstates
    DevBuf pmk;       // [8][cap]  u32 PMKs
    DevBuf ids;       // [cap]     u64 candidate ids
    DevBuf hits;      // [hitcap]  HitDev
    DevBuf counters;  // [0] loaded slots, [1] hit count, [2] PBKDF2 work-queue counter
    int reserve(uint32_t cap, uint32_t hitcap);
};

// A field of the caller's dwpa_config counts only if its struct_size covers it (an older, shorter struct leaves the
// later fields at their documented defaults).  struct_size 0 = the full current struct.
#define DWPA_CFG_HAS(cfg, field) \
    ((cfg) && (!(cfg)->struct_size || (cfg)->struct_size >= offsetof(dwpa_config, field) + sizeof((cfg)->field)))

// No C++ exception crosses the C ABI (a PHP-FPM worker or a Python process would be aborted): every entry point that
// allocates host memory runs its body through guarded(), which maps std::bad_alloc / std::length_error (a host table
// for an input too large for the machine) to `nomem` and any other exception to `other`.  Locks, call contexts and
// in-flight device work are held by RAII objects in the bodies, so an unwound call leaves the library usable.
template <class F>
inline int guarded(F&& body, int nomem = DWPA_E_NOMEM, int other = DWPA_E_ARG) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return nomem;
    } catch (const std::length_error&) {
        return nomem;
    } catch (...) {
        return other;
    }
}

// The check path's host worker pool (engine.cpp HostPool): threads for n items of at least min_per_thread each (at
// most DWPA_HOST_THREADS), and fn(0..T-1) with part 0 on the calling thread.
size_t host_threads_for(size_t n, size_t min_per_thread);
void host_parallel(size_t T, const std::function<void(size_t)>& fn);

// Host (CPU) backend, host_check.cpp.  host_cost: the work of a check call in PMK-equivalents (PBKDF2 derives plus
// the nonce-correction attempts' verify compressions / 16,388), estimated from the jobs without parsing them.
struct HostCost {
    uint64_t keys = 0;      // non-null keys
    uint64_t derives = 0;   // keys whose PMK is derived (not the caller's $pmk)
    double pmk_equiv = 0;   // derives + verify work
};
HostCost host_cost(const dwpa_job* jobs, size_t njobs);
int host_check_batch(const dwpa_job* jobs, size_t njobs, dwpa_result* out, int* rcs, dwpa_check_stats& stats);
int host_pbkdf2(const dwpa_bytes* keys, size_t nkeys, const uint8_t* essid, size_t essid_len, uint8_t* out);
// PMKs the host backend derives in `seconds` on this CPU over `threads` threads (its measured per-chunk costs).
double host_pmks_in(double seconds, size_t threads);
// PBKDF2 of n keys on the host backend into SoA rows: pmk[w * stride + i] = big-endian word w of key i's PMK; key i
// salted with salt[i] (build_salt_blocks layout, nblk[i] blocks).  The device check path's remainder helper.
void host_derive_soa(size_t n, const uint8_t* const* key, const uint32_t* len, const uint32_t* const* salt,
                     const uint32_t* nblk, uint32_t* pmk, size_t stride);

// Pinned host memory (hipHostMalloc) counted in dwpa_resource_stats.pinned_host_bytes; free with the same size.
int pinned_alloc(void** p, size_t bytes);
void pinned_free(void* p, size_t bytes);

int engine_init();
// Rule-file loader mode of the process: dwpa_init's cfg->rule_mode when given, else DWPA_RULE_MODE=full|hashcat
// from the environment, else DWPA_RULES_HASHCAT.  Host only (no device needed).
int engine_rule_mode();
std::vector<int> engine_devices(uint32_t mask);  // mask 0 = the dwpa_init() selection
uint32_t engine_batch();

int scan_create(int device, const char* const* lines, const size_t* lens, size_t nlines, int nc, int nc_mode,
                uint32_t batch, dwpa_scan** out);
void scan_destroy(dwpa_scan* sc);
// fill = true (crack_files): count may exceed the batch; candidates beyond it are dropped by the compaction and
// counted, and scan_counter_raw tells the caller to retry with fewer words.
int scan_counter_raw(dwpa_scan* sc, void* stream, uint32_t* raw);
int scan_load_dict(dwpa_scan* sc, const uint64_t* off, const uint8_t* bytes, uint64_t first, uint32_t count,
                   uint32_t minlen, uint32_t maxlen, void* stream, bool fill = false);
int scan_load_numeric(dwpa_scan* sc, uint64_t first, uint32_t count, uint32_t digits, void* stream);
struct Mask;  // mask.hpp
int scan_set_mask(dwpa_scan* sc, const Mask& m);
// The scan's mask in Markov order (markov_dev.hip): replaces a mask of either kind, and scan_set_mask replaces it;
// scan_load_mask launches the kernel of whichever was set last.  model: a validated image.
struct MarkovMask;  // markov.hpp
int scan_set_mask_markov(dwpa_scan* sc, const MarkovMask& mm, const uint8_t* model);
int scan_load_mask(dwpa_scan* sc, uint64_t first, uint32_t count, void* stream);
// fill = true (crack_hybrid): nwords * mask_count may reach 16 batches (below 2^32), as for scan_load_dict
int scan_load_hybrid(dwpa_scan* sc, const uint64_t* off, const uint8_t* bytes, uint64_t first_word, uint32_t nwords,
                     uint64_t mask_first, uint32_t mask_count, int mode, uint32_t minlen, uint32_t maxlen,
                     void* stream, bool fill = false);
// base words x amplifier words (combi_dev.hip); fill = true (crack_combinator): nbase * amp_count may reach 16
// batches (below 2^32), as for scan_load_hybrid
int scan_load_combinator(dwpa_scan* sc, const uint64_t* base_off, const uint8_t* base_bytes, uint64_t first_base,
                         uint32_t nbase, const uint64_t* amp_off, const uint8_t* amp_bytes, uint64_t amp_words,
                         uint64_t amp_first, uint32_t amp_count, int amp_side, uint32_t minlen, uint32_t maxlen,
                         void* stream, bool fill = false);
// a chain of 1..4 lists and masks (chain_dev.hip); the lists' device pointers stay the caller's
int scan_set_chain(dwpa_scan* sc, const dwpa_chain_part* parts, uint32_t nparts, const dwpa_bytes* custom,
                   uint64_t* keyspace);
// rules on list part `part` of the chain (chain_rules_dev.hip); rs == nullptr takes them off.  Returns the number
// of rules; *keyspace (nullable) = the new K.  A later scan_set_chain clears every part's rules.
struct RuleSet;  // rules.hpp
int scan_set_chain_rules(dwpa_scan* sc, uint32_t part, const RuleSet* rs, uint64_t* keyspace);
int scan_load_chain(dwpa_scan* sc, uint64_t first, uint32_t count, uint32_t minlen, uint32_t maxlen, void* stream);
// the table attack (table_dev.hip): the list's device pointers stay the caller's, the scan owns the table image and
// the kept-word index it builds from the count kernel's output.  A refused call leaves the previous table set.
struct Table;  // table.hpp
int scan_set_table(dwpa_scan* sc, const uint64_t* d_off, const uint8_t* d_bytes, uint64_t nwords, const Table& t,
                   uint32_t minlen, uint32_t maxlen, uint32_t word_max, uint64_t* keyspace, uint64_t* kept);
int scan_load_table(dwpa_scan* sc, uint64_t first, uint32_t count, void* stream);
// the association attack (assoc_dev.hip, assoc.hpp): the scan's nets are the (ESSID, MAC_AP) pairs of its usable lines
// in order of first appearance.  scan_set_assoc takes the entries of all nets, net-major (net_of_word non-decreasing,
// every word 1..256 bytes; the scan copies them), builds the index over the nets with W_n x R > 0 and one salt entry per
// ESSID group; rs == nullptr: the identity.  A refused call leaves the previous association set.  scan_load_assoc
// generates indices [first, first + count); scan_run then derives each slot with its own net's ESSID and verifies it
// against that net's live lines only, and scan_pbkdf2 / scan_verify refuse until another kind of load.
uint32_t scan_num_nets(const dwpa_scan* sc);
int64_t scan_net_of_line(const dwpa_scan* sc, size_t input_line);  // DWPA_E_ARG: no such line or not usable
int scan_set_assoc(dwpa_scan* sc, const dwpa_bytes* words, const uint32_t* net_of_word, size_t count, const RuleSet* rs,
                   uint32_t minlen, uint32_t maxlen, uint64_t* keyspace);
int scan_load_assoc(dwpa_scan* sc, uint64_t first, uint32_t count, void* stream);
int scan_pbkdf2(dwpa_scan* sc, int group, void* stream);
int scan_verify(dwpa_scan* sc, int group, void* stream);
int scan_run(dwpa_scan* sc, void* stream);
int scan_hits_raw(dwpa_scan* sc, std::vector<HitDev>& out, void* stream);
void hit_to_public(const dwpa_scan* sc, const HitDev& h, dwpa_hit& o);
void scan_mark_cracked(dwpa_scan* sc, uint32_t input_line);
uint32_t scan_batch_cap(const dwpa_scan* sc);
Batch& scan_batch_ref(dwpa_scan* sc);
int scan_device(const dwpa_scan* sc);
void scan_rules_drop(const dwpa_scan* scan);

}  // namespace dwpa
