// table_fuzz.cpp -- host fuzz of the table attack (table.cpp: the parser, the saturating counts, the kept-word index
// and the candidates) against naive second implementations, built with AddressSanitizer + UBSan (make
// tools/bin/table_fuzz_asan).  No device.
//   table_fuzz_asan [iterations] [seed]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "dwpa22000.h"
#include "table.hpp"

typedef unsigned __int128 u128;
using dwpa::Table;

static int fail(const char* what, long it) {
    fprintf(stderr, "table_fuzz: %s (case %ld)\n", what, it);
    return 1;
}

// A text the parser may accept or refuse: bytes drawn from what its grammar cares about, or anything at all.
static std::string random_text(std::mt19937_64& rng) {
    static const char pool[] = "=\\x0123456789abcdefABCDEFgG#\r\n\n\naz";
    std::string t;
    const size_t n = rng() % 200;
    const bool wild = rng() % 4 == 0;
    for (size_t i = 0; i < n; i++) t += wild ? (char)(rng() & 0xff) : pool[rng() % (sizeof(pool) - 1)];
    return t;
}

// A valid text with chosen alternative counts: key c gets want[c] distinct values (0: the text never names it).
static std::string table_text(std::mt19937_64& rng, const uint8_t want[256], Table* ref) {
    std::string t;
    for (int c = 0; c < 256; c++) {
        ref->nalt[c] = want[c] ? want[c] : 1;
        memset(ref->alt[c], 0, sizeof(ref->alt[c]));
        if (!want[c]) ref->alt[c][0] = (uint8_t)c;
        const uint8_t base = (uint8_t)rng();
        for (uint32_t k = 0; k < want[c]; k++) {
            const uint8_t v = (uint8_t)(base + 7 * k);  // 7 is odd: distinct for k < 256
            ref->alt[c][k] = v;
            char line[16];
            if (rng() % 2 || c == '\n' || c == '\r' || v == '\n' || v == '\r' || c == '\\' || v == '\\')
                snprintf(line, sizeof(line), "\\x%02x=\\x%02X", c, v);
            else
                snprintf(line, sizeof(line), "%c=%c", c, v);
            // a literal NUL ends snprintf's output: such bytes take the hex form
            if (c == 0 || v == 0) snprintf(line, sizeof(line), "\\x%02x=\\x%02x", c, v);
            t += line;
            t += rng() % 3 ? "\n" : "\r\n";
            if (rng() % 8 == 0) t += rng() % 2 ? "\n" : "\r\n";  // an empty line
            if (rng() % 8 == 0) t += line + std::string("\n");   // a repeated (K, V) line
        }
    }
    return t;
}

int main(int argc, char** argv) {
    const long iters = argc > 1 ? atol(argv[1]) : 3000;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x7461626c65ull);
    for (long it = 0; it < iters; it++) {
        // 1. the parser on random bytes: it ends, and what it accepts is a table
        {
            const std::string t = random_text(rng);
            std::vector<char> exact(t.begin(), t.end());  // no terminator behind the text: ASan sees a read past it
            Table tab;
            uint32_t bad = 0;
            const int r = dwpa::table_parse(exact.data(), exact.size(), &tab, &bad);
            if (r < 0) {
                if (r != DWPA_E_ARG || bad == 0) return fail("a refusal without a line", it);
            } else {
                if (r == 0) return fail("a table without a mapping", it);
                for (int c = 0; c < 256; c++) {
                    if (tab.nalt[c] < 1 || tab.nalt[c] > 16) return fail("alternative count out of range", it);
                    for (int a = 0; a < tab.nalt[c]; a++)
                        for (int b = 0; b < a; b++)
                            if (tab.alt[c][a] == tab.alt[c][b]) return fail("a repeated alternative", it);
                }
            }
        }
        // 2. a generated table parses to what it was generated from
        uint8_t want[256];
        const int style = (int)(rng() % 3);  // 0: few keys, small counts; 1: many keys; 2: counts up to 16
        for (int c = 0; c < 256; c++) {
            const uint64_t v = rng();
            want[c] = style == 0 ? (v % 16 == 0 ? 1 + (v >> 8) % 3 : 0) : style == 1 ? (v >> 8) % 4 : (v >> 8) % 17;
        }
        want['a'] = 2;  // never an empty table
        Table ref, tab;
        const std::string text = table_text(rng, want, &ref);
        if (dwpa::table_parse(text.data(), text.size(), &tab, nullptr) <= 0) return fail("a valid table refused", it);
        if (memcmp(&ref, &tab, sizeof(tab)) != 0) return fail("the parsed table differs", it);
        // 3. counts against a 128-bit product, the filter, the index and every candidate against an odometer
        const uint32_t word_max = style == 2 ? 4096 : (uint32_t)(1 + rng() % 300);
        const dwpa::TableFilter f = dwpa::table_filter((uint32_t)(rng() % 4), (uint32_t)(4 + rng() % 70), word_max);
        std::vector<uint64_t> off{0};
        std::vector<uint8_t> bytes;
        std::vector<dwpa_bytes> words;
        const size_t nwords = rng() % 12;
        for (size_t w = 0; w < nwords; w++) {
            const size_t len = rng() % 8 == 0 ? rng() % 80 : rng() % 7;
            for (size_t i = 0; i < len; i++) bytes.push_back((uint8_t)(rng() % 3 ? 'a' + rng() % 4 : rng()));
            off.push_back(bytes.size());
        }
        bytes.push_back(0);
        for (size_t w = 0; w < nwords; w++) words.push_back(dwpa_bytes{bytes.data() + off[w], (size_t)(off[w + 1] - off[w])});
        std::vector<std::string> expect;
        uint64_t dl = 0, dm = 0, kept = 0;
        for (size_t w = 0; w < nwords; w++) {
            const uint8_t* p = bytes.data() + off[w];
            const size_t len = (size_t)(off[w + 1] - off[w]);
            u128 k = 1;
            bool sat = false;
            for (size_t i = 0; i < len && !sat; i++) {
                k *= tab.nalt[p[i]];
                sat = k > (u128)UINT64_MAX;
            }
            const uint64_t got = dwpa::table_word_count(tab, p, len);
            if (sat ? got != UINT64_MAX : got != (uint64_t)k) return fail("count differs from the 128-bit product", it);
            if (len < f.minlen || len > f.maxlen) {
                dl++;
                continue;
            }
            if (sat || k > f.word_max) {
                dm++;
                continue;
            }
            kept++;
            std::vector<uint32_t> d(len, 0);  // the odometer: last position fastest
            for (uint64_t n = 0; n < (uint64_t)k; n++) {
                std::string c;
                for (size_t i = 0; i < len; i++) c += (char)tab.alt[p[i]][d[i]];
                expect.push_back(c);
                for (size_t i = len; i-- > 0;) {
                    if (++d[i] < tab.nalt[p[i]]) break;
                    d[i] = 0;
                }
            }
        }
        uint64_t K = 0, gk = 0, gl = 0, gm = 0;
        if (dwpa_table_keyspace(text.data(), text.size(), words.data(), nwords, f.minlen, f.maxlen, word_max, &K, &gk,
                                &gl, &gm) != 0)
            return fail("keyspace refused", it);
        if (K != expect.size() || gk != kept || gl != dl || gm != dm) return fail("keyspace or drop counts differ", it);
        std::vector<uint64_t> idx(expect.size());
        for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
        std::vector<uint8_t> out(64 * idx.size() + 1);
        std::vector<uint32_t> lens(idx.size() + 1);
        if (dwpa_table_candidates(text.data(), text.size(), words.data(), nwords, f.minlen, f.maxlen, word_max,
                                  idx.data(), idx.size(), out.data(), lens.data()) != 0)
            return fail("candidates refused", it);
        for (size_t i = 0; i < idx.size(); i++)
            if (lens[i] != expect[i].size() || memcmp(out.data() + 64 * i, expect[i].data(), lens[i]) != 0)
                return fail("a candidate differs from the odometer", it);
        const uint64_t past = K;
        uint8_t one[64];
        uint32_t ol;
        if (dwpa_table_candidates(text.data(), text.size(), words.data(), nwords, f.minlen, f.maxlen, word_max, &past, 1,
                                  one, &ol) != DWPA_E_ARG)
            return fail("index K not refused", it);
    }
    printf("table_fuzz: %ld cases ok\n", iters);
    return 0;
}
