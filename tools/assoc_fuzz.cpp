// assoc_fuzz -- the association attack's host side (dwpa_amd/csrc/assoc.cpp) under AddressSanitizer + UBSan, as a
// stand-alone program (make tools/bin/assoc_fuzz_asan).
//
//   assoc_fuzz_asan HASHFILE ASSOCFILE|- RULESFILE|- [single]
//       builds the plan as dwpa_assoc_plan does and walks EVERY index through candidate(); prints the counts, the
//       number of indices that gave a candidate and an FNV-1a sum over (index, net, candidate), so two builds or two
//       runs can be compared.
//   assoc_fuzz_asan --fuzz [N] [SEED]
//       N random rounds: random bytes through assoc_parse_line; random MACs (0..8 bytes) and ESSIDs (0..40 bytes)
//       through assoc_single at random minlen with its documented counts checked; random nets and word lists with
//       duplicates, empty and over-long words through assoc_build and candidate() at every index, with split()'s
//       invariants checked.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "assoc.hpp"
#include "dwpa22000.h"

#include "engine.hpp"

// rules.cpp's device side (upload, scan loads, the expand kernels) is never reached here: stubbed as in rules_fuzz.cpp
namespace dwpa {
[[noreturn]] static void not_here() { abort(); }
uint32_t scan_batch_cap(const dwpa_scan*) { not_here(); }
Batch& scan_batch_ref(dwpa_scan*) { not_here(); }
int scan_device(const dwpa_scan*) { not_here(); }
int engine_init() { not_here(); }
hipError_t launch_rules_prep(const uint64_t*, const uint8_t*, uint64_t, uint32_t, const uint32_t*, const uint32_t*,
                             uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t*, uint64_t*, uint32_t*, uint32_t,
                             hipStream_t) {
    not_here();
}
hipError_t launch_rules_expand(const uint64_t*, const uint8_t*, uint32_t, const uint32_t*, const uint32_t*, uint32_t,
                               uint8_t*, uint32_t*, hipStream_t, uint32_t*) {
    not_here();
}
}  // namespace dwpa

using namespace dwpa;

#define CHECK(c)                                                       \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "assoc_fuzz: %s:%d: %s\n", __FILE__, __LINE__, #c); \
            exit(2);                                                    \
        }                                                               \
    } while (0)

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
    for (size_t i = 0; i < n; i++) h = (h ^ ((const uint8_t*)p)[i]) * 1099511628211ull;
    return h;
}

static uint64_t walk(const AssocPlan& p, uint64_t* kept) {
    uint64_t h = 14695981039346656037ull;
    std::string c;
    *kept = 0;
    for (uint64_t id = 0; id < p.keyspace(); id++) {
        size_t net = 0;
        uint32_t rule = 0;
        uint64_t e = 0;
        p.split(id, &net, &rule, &e);
        CHECK(net < p.nets.nets.size() && rule < p.R && e >= p.wfirst[net] && e < p.wfirst[net + 1]);
        CHECK(p.start[net] <= id && id < p.start[net + 1] && p.wnet[(size_t)e] == net);
        if (!p.candidate(id, &c, &net)) continue;
        CHECK(c.size() >= 8 && c.size() <= 63);
        (*kept)++;
        h = fnv(h, &id, 8);
        h = fnv(h, &net, sizeof net);
        h = fnv(h, c.data(), c.size());
    }
    std::string none;
    CHECK(!p.candidate(p.keyspace(), &none));
    return h;
}

static int run_files(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    std::vector<std::string> lines;
    std::string cur;
    for (int ch; (ch = fgetc(f)) != EOF;) {
        if (ch == '\n') {
            if (!cur.empty() && cur.back() == '\r') cur.pop_back();
            if (!cur.empty()) lines.push_back(cur);
            cur.clear();
        } else cur.push_back((char)ch);
    }
    if (!cur.empty()) lines.push_back(cur);
    fclose(f);
    std::vector<ParsedLine> parsed;
    for (const std::string& l : lines) parsed.push_back(parse_m22000(l.data(), l.size()));
    const char* assoc = argc > 2 && strcmp(argv[2], "-") ? argv[2] : nullptr;
    const char* rules = argc > 3 && strcmp(argv[3], "-") ? argv[3] : nullptr;
    const bool single = argc > 4 && !strcmp(argv[4], "single");
    RuleSet rs;
    rs.mode = DWPA_RULES_HASHCAT;
    rs.quiet = true;
    if (rules && rs.load_file(rules) < 0) return 1;
    AssocPlan p;
    const int r = assoc_plan(parsed, assoc, single, rules ? 1u : 8u, rules ? &rs : nullptr, &p);
    if (r < 0) {
        printf("refused %d\n", r);
        return 0;
    }
    uint64_t kept = 0;
    const uint64_t h = walk(p, &kept);
    printf("keyspace %llu nets %zu entries %llu lines %llu unmatched %llu malformed %llu dropped %llu rules %u kept %llu "
           "sum %016llx\n", (unsigned long long)p.keyspace(), p.nets.nets.size(), (unsigned long long)p.entries(),
           (unsigned long long)p.file_lines, (unsigned long long)p.unmatched, (unsigned long long)p.malformed,
           (unsigned long long)p.dropped, p.R, (unsigned long long)kept, (unsigned long long)h);
    return 0;
}

static std::string rnd_bytes(std::mt19937_64& g, size_t n, bool hexish) {
    static const char pool[] = "0123456789abcdefABCDEF:$HEX[]gz";
    std::string s(n, '\0');
    for (char& c : s) c = hexish ? pool[g() % (sizeof pool - 1)] : (char)(g() & 0xff);
    return s;
}

static int run_fuzz(uint64_t rounds, uint64_t seed) {
    std::mt19937_64 g(seed);
    RuleSet rs;
    rs.quiet = true;
    const char* text = ":\nu\n$1\nc $!\n^x\nd\n[ [ [\n!a\n>9\n";
    rs.load_text(text, strlen(text));
    CHECK(rs.size() == 9);
    for (uint64_t r = 0; r < rounds; r++) {
        std::string mac, word;
        const std::string line = rnd_bytes(g, g() % 40, g() % 4 != 0);
        if (assoc_parse_line(line.data(), line.size(), &mac, &word)) CHECK(mac.size() == 6 && line.size() >= 13);
        // the generator: 18 BSSID words for a 6-byte MAC, and per suffix 1..3 ESSID words of at least minlen
        const std::string m = rnd_bytes(g, g() % 9, false), e = rnd_bytes(g, g() % 41, g() % 2);
        const uint32_t minlen = (uint32_t)(g() % 45);
        std::vector<std::string> ws;
        assoc_single(m, e, minlen, &ws);
        size_t lo = m.size() == 6 ? 18 : 0, hi = lo;
        for (size_t extra : {0u, 1u, 3u, 1u})
            if (e.size() + extra >= minlen) lo += 1, hi += 3;
        CHECK(ws.size() >= lo && ws.size() <= hi);
        // a plan over random nets
        AssocNets nets;
        const size_t N = 1 + g() % 6;
        std::vector<std::vector<std::string>> words(N);
        for (size_t n = 0; n < N; n++) {
            nets.nets.push_back(AssocNet{rnd_bytes(g, g() % 33, false), rnd_bytes(g, 6, false), {(uint32_t)n}});
            const size_t W = g() % 7;
            for (size_t k = 0; k < W; k++) {
                const uint64_t pick = g() % 10;
                words[n].push_back(pick == 0 ? std::string() : pick == 1 ? std::string(257 + g() % 3, 'L')
                                   : pick == 2 && k ? words[n][0] : rnd_bytes(g, 1 + g() % 70, g() % 2));
            }
        }
        AssocPlan p;
        CHECK(assoc_build(nets, words, g() % 2 ? &rs : nullptr, &p) == 0);
        uint64_t kept = 0;
        walk(p, &kept);
        uint64_t in = 0;
        for (auto& w : words) in += w.size();
        CHECK(p.entries() + p.dropped == in && p.keyspace() == p.entries() * p.R);
    }
    printf("assoc_fuzz: %llu rounds clean\n", (unsigned long long)rounds);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "--fuzz"))
        return run_fuzz(argc > 2 ? strtoull(argv[2], nullptr, 10) : 20000, argc > 3 ? strtoull(argv[3], nullptr, 10) : 1);
    if (argc < 2) {
        fprintf(stderr, "usage: assoc_fuzz HASHFILE ASSOCFILE|- RULESFILE|- [single]  |  assoc_fuzz --fuzz [N] [SEED]\n");
        return 1;
    }
    return run_files(argc, argv);
}
