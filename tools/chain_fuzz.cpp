// chain_fuzz.cpp -- host fuzz of the chain attack's arithmetic (chain.cpp: dwpa_chain_keyspace / dwpa_chain_split)
// against 128-bit integers, built with AddressSanitizer + UBSan (make tools/bin/chain_fuzz_asan).  No device.
//   chain_fuzz_asan [iterations] [seed]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "dwpa22000.h"

typedef unsigned __int128 u128;

static int fail(const char* what, const uint64_t* r, uint32_t n, uint64_t index) {
    fprintf(stderr, "chain_fuzz: %s: nparts %u radices %llu %llu %llu %llu index %llu\n", what, n,
            (unsigned long long)r[0], (unsigned long long)r[1], (unsigned long long)r[2], (unsigned long long)r[3],
            (unsigned long long)index);
    return 1;
}

int main(int argc, char** argv) {
    const long iters = argc > 1 ? atol(argv[1]) : 200000;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x636861696eull);
    const uint64_t edge[] = {0, 1, 2, 3, 10, 255, 256, 65535, 65536, 65537, 641, 6700417, 0xffffffffull, 0x100000000ull,
                             0x100000001ull, 10000000000ull, 0x7fffffffffffffffull, 0x8000000000000000ull,
                             0xffffffffffffffffull};
    const size_t nedge = sizeof(edge) / sizeof(edge[0]);
    for (long it = 0; it < iters; it++) {
        uint64_t r[5] = {0, 0, 0, 0, 0};
        const uint32_t n = (uint32_t)(rng() % 6);  // 0 and 5 are refused
        for (uint32_t p = 0; p < n && p < 5; p++) {
            const uint64_t v = rng();
            r[p] = v % 4 == 0 ? edge[(v >> 8) % nedge] : v % 4 == 1 ? (v >> 8) % 1000 : v >> (8 + (v >> 2) % 56);
        }
        u128 k = 1;
        bool zero = false;
        for (uint32_t p = 0; p < n; p++) zero |= r[p] == 0;
        for (uint32_t p = 0; p < n && !zero; p++) {
            k *= r[p];
            if (k > (u128)UINT64_MAX) break;
        }
        if (zero) k = 0;
        const bool refused = n == 0 || n > DWPA_CHAIN_MAX_PARTS || k > (u128)UINT64_MAX;
        uint64_t got = 0x5a5a5a5a5a5a5a5aull;
        const int rc = dwpa_chain_keyspace(r, n, &got);
        if (refused ? rc != DWPA_E_ARG : (rc != 0 || got != (uint64_t)k)) return fail("keyspace", r, n, 0);
        uint64_t index = rng();
        if (!refused && k && rng() % 2) index %= (uint64_t)k;
        if (!refused && k && rng() % 8 == 0) index = (uint64_t)k - 1;
        uint64_t d[4] = {~0ull, ~0ull, ~0ull, ~0ull};
        const int rs = dwpa_chain_split(r, n, index, d);
        if (refused || (u128)index >= k) {
            if (rs != DWPA_E_ARG) return fail("split not refused", r, n, index);
            continue;
        }
        if (rs != 0) return fail("split refused", r, n, index);
        u128 back = 0;
        for (uint32_t p = 0; p < n; p++) {
            if (d[p] >= r[p]) return fail("digit out of range", r, n, index);
            back = back * r[p] + d[p];
        }
        if (back != (u128)index) return fail("digits do not give the index", r, n, index);
    }
    printf("chain_fuzz: %ld cases ok\n", iters);
    return 0;
}
