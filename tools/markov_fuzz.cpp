// markov_fuzz.cpp -- host fuzz of the Markov-ordered mask (dwpa_amd/csrc/markov.cpp with mask.cpp) under
// AddressSanitizer / UBSan: random masks, custom sets, thresholds, model images (valid and damaged) and indices
// through the host functions, checked against a second, naive implementation below.  For a mask that parses under
// its threshold, the candidates at index 0, K - 1 and random indices must equal the naive ones, index K must be
// refused, and walking the device table image as k_prep_markov does (in an exact-size heap block, so that a write or
// read past it is seen) must give the same bytes.  A damaged image must be refused by every call that takes one.
//   make tools/bin/markov_fuzz_asan && tools/bin/markov_fuzz_asan [iterations]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "dwpa22000.h"
#include "markov.hpp"
#include "mask.hpp"

namespace {

// Candidate `index` the slow way: no MarkovMask, no table.  sets: the parsed positions; t: the threshold.
bool naive(const dwpa::Mask& sets, uint32_t t, const uint8_t* model, unsigned __int128 index, uint8_t* out) {
    uint32_t digit[64];
    for (int p = (int)sets.npos - 1; p >= 0; p--) {
        const uint32_t n = sets.pos[p].radix, r = t == 0 || t > n ? n : t;
        digit[p] = (uint32_t)(index % r);
        index /= r;
    }
    if (index != 0) return false;
    uint32_t prev = 0;
    for (uint32_t p = 0; p < sets.npos; p++) {
        const uint8_t* row = model + 16 + ((size_t)p * 256 + prev) * 256;
        uint32_t seen = 0;
        bool found = false;
        for (int j = 0; j < 256 && !found; j++) {
            const uint8_t* e = sets.pos[p].bytes + sets.pos[p].radix;
            if (std::find(sets.pos[p].bytes, e, row[j]) == e) continue;
            if (seen++ == digit[p]) {
                out[p] = row[j];
                found = true;
            }
        }
        if (!found) return false;
        prev = out[p];
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const long iters = argc > 1 ? atol(argv[1]) : 20000;
    std::mt19937_64 rng(22000);
    // a few valid models: every row a random permutation, some rows left in byte order (unseen)
    std::vector<std::vector<uint8_t>> models(3, std::vector<uint8_t>(DWPA_MARKOV_BYTES));
    for (auto& m : models) {
        memcpy(m.data(), "DWPAMKV1\x3f\0\0\0\0\0\0\0", 16);
        for (size_t row = 0; row < (size_t)63 * 256; row++) {
            uint8_t* r = m.data() + 16 + row * 256;
            std::iota(r, r + 256, (uint8_t)0);
            if (rng() % 4) std::shuffle(r, r + 256, rng);
        }
        if (dwpa_markov_check(m.data(), m.size()) != 0) {
            fprintf(stderr, "a valid model was refused\n");
            return 1;
        }
    }
    const std::string builtin = "ludhHsab?", sets1234 = "1234";
    auto token = [&](std::string& s, bool refs) {  // refs: ?1..?4 now and then (often undefined: an error)
        const uint64_t r = rng() % 96;
        if (r < 56) {
            s.push_back('?');
            s.push_back(refs && rng() % 6 == 0 ? sets1234[rng() % 4] : builtin[rng() % builtin.size()]);
        } else if (r < 57) {
            s.push_back('?');
            s.push_back((char)(rng() % 256));  // mostly an unknown letter
        } else {
            s.push_back((char)(rng() % 4 ? 'a' + rng() % 26 : rng() % 256));
        }
    };
    long parsed = 0, refused = 0, cands = 0, damaged_refused = 0, tables = 0;
    auto sets = std::make_unique<dwpa::Mask>();
    auto mm = std::make_unique<dwpa::MarkovMask>();
    auto pre = std::make_unique<dwpa::MarkovMask>();
    for (long it = 0; it < iters; it++) {
        std::string mask;
        const int n = (int)(rng() % 8 == 0 ? 56 + rng() % 10 : 1 + rng() % 14);
        for (int i = 0; i < n; i++) token(mask, true);
        std::string cs[4];
        dwpa_bytes custom[4];
        for (int k = 0; k < 4; k++) {
            custom[k].ptr = nullptr;
            custom[k].len = 0;
            if (rng() % 8 == 0) continue;
            const int m = (int)(1 + rng() % 6);
            for (int i = 0; i < m; i++) token(cs[k], rng() % 8 == 0);
            uint8_t* p = (uint8_t*)malloc(cs[k].size());  // exact size: a read past the set is seen
            memcpy(p, cs[k].data(), cs[k].size());
            custom[k].ptr = p;
            custom[k].len = cs[k].size();
        }
        const uint32_t pick[] = {0, 1, 2, 3, 9, 10, 26, 95, 255, 256, 257, 1000};
        const uint32_t t = rng() % 3 ? pick[rng() % 12] : (uint32_t)(rng() % 300);
        const std::vector<uint8_t>& model = models[rng() % models.size()];
        std::vector<char> exact(mask.begin(), mask.end());  // no NUL behind the mask
        uint32_t npos = 0;
        uint64_t K = 0;
        const int r = dwpa_mask_keyspace_markov(exact.data(), exact.size(), custom, t, &npos, &K);
        const bool parses = dwpa::mask_parse_sets(exact.data(), exact.size(), custom, sets.get()) == 0;
        // the naive keyspace, in 128 bits
        unsigned __int128 k128 = 1;
        bool fits = parses && t <= 256;
        for (uint32_t p = 0; fits && p < sets->npos; p++) {
            const uint32_t np = sets->pos[p].radix;
            k128 *= t == 0 || t > np ? np : t;
            fits = k128 <= (unsigned __int128)UINT64_MAX;
        }
        if ((r == 0) != fits || (r != 0 && r != DWPA_E_ARG) || (r == 0 && (K != (uint64_t)k128 || npos != sets->npos))) {
            fprintf(stderr, "keyspace: rc %d, K %llu, fits %d\n", r, (unsigned long long)K, (int)fits);
            return 1;
        }
        if (r == 0) {
            parsed++;
            if (dwpa::markov_mask(*sets, t, mm.get()) != 0 || mm->keyspace != K) return 1;
            uint64_t idx[8] = {0, K - 1, K / 2, rng() % K, rng() % K, rng() % K, rng() % K, rng() % K};
            uint8_t got[8 * 64], want[64], one[64];
            uint32_t len = 0;
            const bool api = it % 8 == 0;  // the C calls validate the whole image: every eighth iteration
            if (api) {
                if (dwpa_mask_candidates_markov(exact.data(), exact.size(), custom, model.data(), model.size(), t, idx, 8,
                                                got, &len) != 0 || len != npos) {
                    fprintf(stderr, "candidates of a mask that parsed were refused\n");
                    return 1;
                }
                if (dwpa_mask_candidate_markov(exact.data(), exact.size(), custom, model.data(), model.size(), t, K, one,
                                               &len) != DWPA_E_ARG)
                    return 1;
            } else {
                memset(got, 0, sizeof got);
                for (int j = 0; j < 8; j++) dwpa::markov_candidate(*mm, model.data(), idx[j], got + 64 * j);
            }
            // the table image, walked as the kernel walks it; of a prefix now and then
            const dwpa::MarkovMask* tm = mm.get();
            if (rng() % 4 == 0) {
                dwpa::markov_prefix(*mm, 1 + (uint32_t)(rng() % npos), pre.get());
                tm = pre.get();
            }
            const size_t tbytes = dwpa::markov_table_bytes(tm->npos);
            uint8_t* table = (uint8_t*)calloc(tbytes, 1);
            dwpa::markov_table(*tm, model.data(), table);
            tables++;
            for (int j = 0; j < 8; j++) {
                memset(want, 0, 64);
                if (!naive(*sets, t, model.data(), idx[j], want) || memcmp(want, got + 64 * j, 64) != 0) {
                    fprintf(stderr, "candidate %llu differs from the naive one (threshold %u)\n",
                            (unsigned long long)idx[j], t);
                    return 1;
                }
                cands++;
                const uint64_t ti = tm == mm.get() ? idx[j] : idx[j] % tm->keyspace;
                uint8_t dg[64], walked[64];
                dwpa::markov_digits(*tm, ti, dg);
                dwpa::markov_candidate(*tm, model.data(), ti, one);
                uint32_t prev = 0;
                for (uint32_t p = 0; p < tm->npos; p++) {
                    uint32_t radix;
                    memcpy(&radix, table + 4 * p, 4);
                    if (radix != tm->radix[p] || dg[p] >= radix) return 1;
                    prev = table[dwpa::MARKOV_TABLE_NEXT + ((size_t)p * 256 + prev) * 256 + dg[p]];
                    walked[p] = (uint8_t)prev;
                }
                if (memcmp(walked, one, tm->npos) != 0) {
                    fprintf(stderr, "the table walk of index %llu differs\n", (unsigned long long)ti);
                    return 1;
                }
            }
            free(table);
            if (it % 4 == 0) {  // a damaged image: cut, grown, another header, a byte twice in a row
                std::vector<uint8_t> bad(model);
                switch (rng() % 4) {
                case 0: bad.resize(rng() % bad.size()); break;
                case 1: bad.push_back(0); break;
                case 2: bad[rng() % 16] ^= (uint8_t)(1 + rng() % 255); break;
                default: {
                    const size_t at = 16 + (size_t)(rng() % (63 * 256)) * 256;
                    const size_t a = rng() % 256, b = (a + 1 + rng() % 255) % 256;
                    bad[at + a] = bad[at + b];
                }
                }
                std::vector<uint8_t> tight(bad);  // exact-size copy
                tight.shrink_to_fit();
                if (dwpa_markov_check(tight.data(), tight.size()) != DWPA_E_ARG ||
                    dwpa_mask_candidate_markov(exact.data(), exact.size(), custom, tight.data(), tight.size(), t, 0, one,
                                               &len) != DWPA_E_ARG) {
                    fprintf(stderr, "a damaged image was taken\n");
                    return 1;
                }
                damaged_refused++;
            }
        } else {
            refused++;
        }
        for (int k = 0; k < 4; k++) free((void*)custom[k].ptr);
    }
    printf("{\"iterations\": %ld, \"masks_parsed\": %ld, \"refused\": %ld, \"candidates\": %ld, \"tables\": %ld, "
           "\"damaged_refused\": %ld}\n", iters, parsed, refused, cands, tables, damaged_refused);
    return 0;
}
