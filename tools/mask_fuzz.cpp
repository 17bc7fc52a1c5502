// mask_fuzz.cpp -- host fuzz of the mask language (dwpa_amd/csrc/mask.cpp alone) under AddressSanitizer / UBSan:
// random and mutated masks and custom sets through dwpa_mask_keyspace and dwpa_mask_candidate.  For a mask that
// parses, the candidates at index 0, K - 1 and a few random indices must have `positions` bytes, and index K must be
// refused; the internal table image must hold every set inside its 16 KiB.
//   make tools/bin/mask_fuzz_asan && tools/bin/mask_fuzz_asan [iterations]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "dwpa22000.h"
#include "mask.hpp"

int main(int argc, char** argv) {
    const long iters = argc > 1 ? atol(argv[1]) : 200000;
    std::mt19937_64 rng(22000);
    const std::string letters = "ludhHsab?1234";
    const std::string seeds[] = {"?d?d?d?d?d?d?d?d", "?1?1?1?1?1?1?1?1", "pre??x?1?2?l", "?b?b?b?b?b?b?b?a", "?a?a?a?a?a?a?a?a",
                                 "passw?1?1?1", "?h?H?s?u?d?l?3?4"};
    auto token = [&](std::string& s) {
        const uint64_t r = rng() % 48;
        if (r < 30) {
            s.push_back('?');
            s.push_back(letters[rng() % letters.size()]);
        } else if (r < 31) {
            s.push_back('?');
            s.push_back((char)(rng() % 256));  // mostly an unknown letter
        } else if (r < 32) {
            s.push_back('?');  // a lone '?': an error at the end, else it takes the next byte
        } else {
            s.push_back((char)(rng() % 4 ? 'a' + rng() % 26 : rng() % 256));
        }
    };
    long parsed = 0, refused = 0, cands = 0;
    std::vector<uint8_t> table(dwpa::MASK_TABLE_BYTES);
    for (long it = 0; it < iters; it++) {
        std::string mask;
        if (rng() % 3 == 0) {  // a mutated seed: bytes replaced, dropped, doubled
            mask = seeds[rng() % (sizeof seeds / sizeof seeds[0])];
            for (int m = (int)(rng() % 4); m > 0 && !mask.empty(); m--) {
                const size_t at = rng() % mask.size();
                switch (rng() % 3) {
                case 0: mask[at] = (char)(rng() % 256); break;
                case 1: mask.erase(at, 1); break;
                default: mask.insert(at, 1, mask[at]); break;
                }
            }
        } else {
            const int n = (int)(rng() % 8 == 0 ? 56 + rng() % 16 : rng() % 14);  // often around the 63-position limit
            for (int i = 0; i < n; i++) token(mask);
        }
        std::string cs[4];
        dwpa_bytes custom[4];
        for (int k = 0; k < 4; k++) {
            custom[k].ptr = nullptr;
            custom[k].len = 0;
            if (rng() % 3 == 0) continue;
            const int n = (int)(rng() % 10 == 0 ? 0 : 1 + rng() % 6);
            for (int i = 0; i < n; i++) token(cs[k]);
            // an exact-size heap copy, so that a read past the set is seen
            uint8_t* p = (uint8_t*)malloc(cs[k].size() ? cs[k].size() : 1);
            memcpy(p, cs[k].data(), cs[k].size());
            custom[k].ptr = p;
            custom[k].len = cs[k].size();
        }
        const dwpa_bytes* cu = rng() % 8 ? custom : nullptr;
        std::vector<char> exact(mask.begin(), mask.end());  // no NUL behind the mask
        uint32_t npos = 0;
        uint64_t K = 0;
        const int r = dwpa_mask_keyspace(exact.data(), exact.size(), cu, &npos, &K);
        if (r == 0) {
            parsed++;
            if (npos < 1 || npos > 63 || K == 0) {
                fprintf(stderr, "bad result: %u positions, keyspace %llu\n", npos, (unsigned long long)K);
                return 1;
            }
            dwpa::Mask m;
            if (dwpa::mask_parse(exact.data(), exact.size(), cu, &m) != 0 || m.keyspace != K) return 1;
            dwpa::mask_table(m, table.data());
            dwpa::Mask pre;
            dwpa::mask_prefix(m, 1 + (uint32_t)(rng() % npos), &pre);
            const uint64_t idx[5] = {0, K - 1, rng() % K, rng() % K, K / 2};
            for (uint64_t i : idx) {
                uint8_t out[64];
                uint32_t n = 0;
                if (dwpa_mask_candidate(exact.data(), exact.size(), cu, i, out, &n) != 0 || n != npos) {
                    fprintf(stderr, "candidate %llu of a mask that parsed was refused\n", (unsigned long long)i);
                    return 1;
                }
                cands++;
            }
            uint8_t out[64];
            uint32_t n = 0;
            if (dwpa_mask_candidate(exact.data(), exact.size(), cu, K, out, &n) != DWPA_E_ARG) return 1;
        } else if (r == DWPA_E_ARG) {
            refused++;
        } else {
            fprintf(stderr, "unexpected code %d\n", r);
            return 1;
        }
        for (int k = 0; k < 4; k++) free((void*)custom[k].ptr);
    }
    printf("{\"iterations\": %ld, \"masks_parsed\": %ld, \"refused\": %ld, \"candidates\": %ld}\n", iters, parsed, refused,
           cands);
    return 0;
}
