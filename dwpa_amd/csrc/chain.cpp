// chain.cpp -- the chain attack's host arithmetic (chain.hpp) and its C entry points.  Host only, no HIP.
#include "chain.hpp"

namespace dwpa {

int chain_keyspace(const uint64_t* radix, uint32_t nparts, uint64_t* keyspace) {
    if (!radix || nparts == 0 || nparts > CHAIN_MAX_PARTS) return DWPA_E_ARG;
    for (uint32_t p = 0; p < nparts; p++)
        if (radix[p] == 0) {  // an empty part: no candidate, however large the others are
            if (keyspace) *keyspace = 0;
            return 0;
        }
    uint64_t k = 1;
    for (uint32_t p = 0; p < nparts; p++)
        if (__builtin_mul_overflow(k, radix[p], &k)) return DWPA_E_ARG;
    if (keyspace) *keyspace = k;
    return 0;
}

int chain_split(const uint64_t* radix, uint32_t nparts, uint64_t index, uint64_t* digits) {
    uint64_t k;
    const int r = chain_keyspace(radix, nparts, &k);
    if (r < 0) return r;
    if (!digits || index >= k) return DWPA_E_ARG;
    for (uint32_t p = nparts; p-- > 0;) {
        digits[p] = index % radix[p];
        index /= radix[p];
    }
    return 0;
}

}  // namespace dwpa

extern "C" {

int dwpa_chain_keyspace(const uint64_t* radix, uint32_t nparts, uint64_t* keyspace) {
    return dwpa::chain_keyspace(radix, nparts, keyspace);
}

int dwpa_chain_split(const uint64_t* radix, uint32_t nparts, uint64_t index, uint64_t* digits) {
    return dwpa::chain_split(radix, nparts, index, digits);
}

}  // extern "C"
