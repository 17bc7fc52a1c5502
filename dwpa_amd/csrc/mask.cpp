// mask.cpp -- hashcat -a 3 mask language on the host (mask.hpp): no HIP, no heap, no exceptions.
#include "mask.hpp"

#include <string.h>

namespace dwpa {

namespace {

struct Set {
    uint32_t n = 0;
    uint8_t b[256];
    bool seen[256];
    Set() { memset(b, 0, sizeof b); memset(seen, 0, sizeof seen); }
    void add(uint8_t c) {  // duplicates dropped, first occurrence kept
        if (seen[c]) return;
        seen[c] = true;
        b[n++] = c;
    }
    void range(int lo, int hi) {
        for (int c = lo; c <= hi; c++) add((uint8_t)c);
    }
};

// Adds built-in set `c` to s; false if c names none.
bool add_builtin(Set& s, uint8_t c) {
    switch (c) {
    case 'l': s.range('a', 'z'); return true;
    case 'u': s.range('A', 'Z'); return true;
    case 'd': s.range('0', '9'); return true;
    case 'h': s.range('0', '9'); s.range('a', 'f'); return true;
    case 'H': s.range('0', '9'); s.range('A', 'F'); return true;
    case 's': s.range(0x20, 0x2f); s.range(0x3a, 0x40); s.range(0x5b, 0x60); s.range(0x7b, 0x7e); return true;
    case 'a': add_builtin(s, 'l'); add_builtin(s, 'u'); add_builtin(s, 'd'); add_builtin(s, 's'); return true;
    case 'b': s.range(0x00, 0xff); return true;
    default: return false;
    }
}

// One token of mask / custom-set text at p[i]: appended to s.  ncustom = how many custom sets (1..ncustom) the text
// may reference.  Returns the bytes consumed, or 0 on error.
size_t take(const uint8_t* p, size_t i, size_t len, const Set* custom, const bool* defined, int ncustom, Set& s) {
    if (p[i] != '?') {
        s.add(p[i]);
        return 1;
    }
    if (i + 1 >= len) return 0;  // a trailing lone '?'
    const uint8_t c = p[i + 1];
    if (c == '?') {
        s.add('?');
        return 2;
    }
    if (c >= '1' && c <= '4') {
        const int k = c - '1';
        if (k >= ncustom || !defined[k]) return 0;
        for (uint32_t j = 0; j < custom[k].n; j++) s.add(custom[k].b[j]);
        return 2;
    }
    return add_builtin(s, c) ? 2 : 0;
}

}  // namespace

int mask_parse_sets(const char* mask, size_t len, const dwpa_bytes* custom_in, Mask* out) {
    if (!mask || !out || len == 0) return DWPA_E_ARG;
    Set custom[4];
    bool defined[4] = {false, false, false, false};
    for (int k = 0; k < 4 && custom_in; k++) {
        if (!custom_in[k].ptr) continue;
        const uint8_t* p = custom_in[k].ptr;
        const size_t n = custom_in[k].len;
        for (size_t i = 0; i < n;) {
            const size_t used = take(p, i, n, custom, defined, k, custom[k]);  // lower-numbered sets only
            if (!used) return DWPA_E_ARG;
            i += used;
        }
        if (custom[k].n == 0) return DWPA_E_ARG;  // an empty set
        defined[k] = true;
    }
    out->npos = 0;
    out->keyspace = 0;
    const uint8_t* p = (const uint8_t*)mask;
    for (size_t i = 0; i < len;) {
        if (out->npos == MASK_MAX_POS) return DWPA_E_ARG;
        Set s;
        const size_t used = take(p, i, len, custom, defined, 4, s);
        if (!used || s.n == 0) return DWPA_E_ARG;
        i += used;
        MaskPos& mp = out->pos[out->npos++];
        mp.radix = s.n;
        memcpy(mp.bytes, s.b, 256);
    }
    return out->npos ? 0 : DWPA_E_ARG;
}

int mask_parse(const char* mask, size_t len, const dwpa_bytes* custom_in, Mask* out) {
    const int r = mask_parse_sets(mask, len, custom_in, out);
    if (r < 0) return r;
    out->keyspace = 1;
    for (uint32_t p = 0; p < out->npos; p++) {
        const uint32_t n = out->pos[p].radix;
        if (out->keyspace > UINT64_MAX / n) return DWPA_E_ARG;  // K above 2^64 - 1
        out->keyspace *= n;
    }
    return 0;
}

void mask_prefix(const Mask& m, uint32_t n, Mask* out) {
    out->npos = n;
    out->keyspace = 1;
    for (uint32_t p = 0; p < n; p++) {
        out->pos[p] = m.pos[p];
        out->keyspace *= m.pos[p].radix;
    }
}

void mask_digits(const Mask& m, uint64_t index, uint8_t digits[64]) {
    memset(digits, 0, 64);
    for (uint32_t p = m.npos; p-- > 0;) {
        const uint32_t r = m.pos[p].radix;
        digits[p] = (uint8_t)(index % r);
        index /= r;
    }
}

void mask_candidate(const Mask& m, uint64_t index, uint8_t* out) {
    uint8_t d[64];
    mask_digits(m, index, d);
    for (uint32_t p = 0; p < m.npos; p++) out[p] = m.pos[p].bytes[d[p]];
}

void mask_table(const Mask& m, uint8_t* table) {
    memset(table, 0, MASK_TABLE_BYTES);
    for (uint32_t p = 0; p < m.npos; p++) {
        const uint32_t r = m.pos[p].radix;
        memcpy(table + 4 * p, &r, 4);
        memcpy(table + MASK_TABLE_SETS + (size_t)p * 256, m.pos[p].bytes, 256);
    }
}

}  // namespace dwpa

extern "C" {

int dwpa_mask_keyspace(const char* mask, size_t mask_len, const dwpa_bytes custom[4], uint32_t* positions,
                       uint64_t* keyspace) {
    dwpa::Mask m;
    const int r = dwpa::mask_parse(mask, mask_len, custom, &m);
    if (r < 0) return r;
    if (positions) *positions = m.npos;
    if (keyspace) *keyspace = m.keyspace;
    return 0;
}

int dwpa_mask_candidate(const char* mask, size_t mask_len, const dwpa_bytes custom[4], uint64_t index,
                        uint8_t out[64], uint32_t* out_len) {
    if (!out || !out_len) return DWPA_E_ARG;
    dwpa::Mask m;
    const int r = dwpa::mask_parse(mask, mask_len, custom, &m);
    if (r < 0) return r;
    if (index >= m.keyspace) return DWPA_E_ARG;
    memset(out, 0, 64);
    dwpa::mask_candidate(m, index, out);
    *out_len = m.npos;
    return 0;
}

}  // extern "C"
