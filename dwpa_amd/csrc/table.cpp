// table.cpp -- table attack, host side: table.hpp's parser, counts, index and decoder, and their C entry points.
#include "table.hpp"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <stdexcept>

namespace dwpa {

namespace {

int hexval(uint8_t c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

// One byte of a K=V line at s[*i]: \xHH or the literal byte.  False at the end of the line.
bool take_byte(const uint8_t* s, size_t n, size_t* i, uint8_t* out) {
    if (*i >= n) return false;
    if (s[*i] == '\\' && *i + 3 < n && s[*i + 1] == 'x' && hexval(s[*i + 2]) >= 0 && hexval(s[*i + 3]) >= 0) {
        *out = (uint8_t)(hexval(s[*i + 2]) << 4 | hexval(s[*i + 3]));
        *i += 4;
        return true;
    }
    *out = s[(*i)++];
    return true;
}

// No exception crosses the C ABI (engine.hpp guarded(); this file stays free of the engine's headers so that it builds
// alone under the sanitizers).
template <class F>
int no_throw(F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return DWPA_E_NOMEM;
    } catch (const std::length_error&) {
        return DWPA_E_NOMEM;
    } catch (...) {
        return DWPA_E_ARG;
    }
}

// words[] as one list: offsets and bytes.  DWPA_E_ARG: a null pointer with a length.
int flatten(const dwpa_bytes* words, size_t nwords, std::vector<uint64_t>* off, std::vector<uint8_t>* bytes) {
    if (!words && nwords) return DWPA_E_ARG;
    off->assign(1, 0);
    off->reserve(nwords + 1);
    for (size_t i = 0; i < nwords; i++) {
        if (!words[i].ptr && words[i].len) return DWPA_E_ARG;
        if (words[i].len) bytes->insert(bytes->end(), words[i].ptr, words[i].ptr + words[i].len);
        off->push_back(bytes->size());
    }
    return 0;
}

}  // namespace

int table_parse(const char* text, size_t len, Table* out, uint32_t* bad_line) {
    if ((!text && len) || !out) return DWPA_E_ARG;
    const uint8_t* s = (const uint8_t*)text;
    bool keyed[256] = {};
    memset(out, 0, sizeof(*out));
    int mappings = 0;
    uint32_t line = 0;
    size_t pos = 0;
    auto fail = [&](uint32_t at) {
        if (bad_line) *bad_line = at;
        return DWPA_E_ARG;
    };
    while (pos < len) {
        const uint8_t* nl = (const uint8_t*)memchr(s + pos, '\n', len - pos);
        const size_t end = nl ? (size_t)(nl - s) : len;
        size_t n = end - pos;
        const uint8_t* l = s + pos;
        pos = nl ? end + 1 : len;
        line++;
        if (n && l[n - 1] == '\r') n--;
        if (n == 0) continue;
        size_t i = 0;
        uint8_t k, v;
        if (!take_byte(l, n, &i, &k) || i >= n || l[i++] != '=' || !take_byte(l, n, &i, &v) || i != n)
            return fail(line);
        keyed[k] = true;
        if (memchr(out->alt[k], v, out->nalt[k])) continue;  // a repeated (K, V) line
        if (out->nalt[k] == TABLE_MAX_ALT) return fail(line);
        out->alt[k][out->nalt[k]++] = v;
        mappings++;
    }
    if (mappings == 0) return fail(line + 1);
    for (int c = 0; c < 256; c++)
        if (!keyed[c]) {
            out->nalt[c] = 1;
            out->alt[c][0] = (uint8_t)c;
        }
    return mappings;
}

std::string table_builtin(const char* name) {
    std::string t;
    if (!name || strcmp(name, "toggle") != 0) return t;
    for (int c = 'a'; c <= 'z'; c++) {
        const char lo = (char)c, up = (char)(c - 32);
        t += {lo, '=', lo, '\n', lo, '=', up, '\n', up, '=', up, '\n', up, '=', lo, '\n'};
    }
    return t;
}

int table_read_file(const char* path, Table* out, uint32_t* bad_line) {
    FILE* f = path ? fopen(path, "rb") : nullptr;
    if (!f) return DWPA_E_IO;
    std::string text;
    char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, n);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) return DWPA_E_IO;
    return table_parse(text.data(), text.size(), out, bad_line);
}

uint64_t table_word_count(const Table& t, const uint8_t* w, size_t len) {
    uint64_t k = 1;
    for (size_t i = 0; i < len; i++)
        if (__builtin_mul_overflow(k, (uint64_t)t.nalt[w[i]], &k)) return UINT64_MAX;
    return k;
}

uint32_t table_kept_count(const Table& t, const TableFilter& f, const uint8_t* w, size_t len, int* why) {
    int reason = TABLE_KEPT;
    uint64_t k = 0;
    if (len < f.minlen || len > f.maxlen) {
        reason = TABLE_DROP_LEN;
    } else if ((k = table_word_count(t, w, len)) > f.word_max) {
        reason = TABLE_DROP_MAX;
    }
    if (why) *why = reason;
    return reason == TABLE_KEPT ? (uint32_t)k : 0u;
}

int table_index_counts(const uint32_t* counts, size_t nwords, TableIndex* ix) {
    if (nwords > UINT32_MAX) return DWPA_E_ARG;
    ix->start.assign(1, 0);
    ix->kword.clear();
    uint64_t K = 0;
    for (size_t i = 0; i < nwords; i++) {
        if (!counts[i]) continue;
        if (__builtin_add_overflow(K, (uint64_t)counts[i], &K)) return DWPA_E_ARG;
        ix->kword.push_back((uint32_t)i);
        ix->start.push_back(K);
    }
    return 0;
}

int table_index_list(const Table& t, const TableFilter& f, const uint64_t* off, const uint8_t* bytes, size_t nwords,
                     TableIndex* ix) {
    if (nwords > UINT32_MAX) return DWPA_E_ARG;
    std::vector<uint32_t> counts(nwords);
    ix->dropped_len = ix->dropped_max = 0;
    for (size_t i = 0; i < nwords; i++) {
        int why;
        counts[i] = table_kept_count(t, f, bytes + off[i], (size_t)(off[i + 1] - off[i]), &why);
        ix->dropped_len += why == TABLE_DROP_LEN;
        ix->dropped_max += why == TABLE_DROP_MAX;
    }
    return table_index_counts(counts.data(), nwords, ix);
}

bool table_candidate(const Table& t, const TableIndex& ix, const uint64_t* off, const uint8_t* bytes, uint64_t id,
                     uint8_t out[64], uint32_t* len) {
    if (id >= ix.keyspace()) return false;
    // the kept word j with start[j] <= id < start[j + 1]: counts are >= 1, so start is strictly increasing
    const size_t j = (size_t)(std::upper_bound(ix.start.begin(), ix.start.end(), id) - ix.start.begin()) - 1;
    const uint32_t wi = ix.kword[j];
    const uint8_t* w = bytes + off[wi];
    const uint32_t L = (uint32_t)(off[wi + 1] - off[wi]);  // <= 63: the word is kept
    uint64_t sub = id - ix.start[j];
    memset(out, 0, 64);
    for (uint32_t p = L; p-- > 0;) {
        const uint32_t n = t.nalt[w[p]];
        out[p] = t.alt[w[p]][sub % n];
        sub /= n;
    }
    *len = L;
    return true;
}

}  // namespace dwpa

using namespace dwpa;

extern "C" int dwpa_table_parse(const char* text, size_t len, uint8_t* image, uint32_t* bad_line) {
    return no_throw([&]() -> int {
        Table t;
        if (bad_line) *bad_line = 0;
        const int r = table_parse(text, len, &t, bad_line);
        if (r > 0 && image) memcpy(image, &t, sizeof(t));
        return r;
    });
}

extern "C" int dwpa_table_builtin(const char* name, char* out, size_t cap, size_t* len) {
    return no_throw([&]() -> int {
        const std::string t = table_builtin(name);
        if (t.empty() || !len) return DWPA_E_ARG;
        *len = t.size();
        if (out && cap >= t.size()) memcpy(out, t.data(), t.size());
        return 0;
    });
}

extern "C" int dwpa_table_keyspace(const char* table_text, size_t table_len, const dwpa_bytes* words, size_t nwords,
                                   uint32_t minlen, uint32_t maxlen, uint32_t word_max, uint64_t* keyspace,
                                   uint64_t* kept, uint64_t* dropped_len, uint64_t* dropped_max) {
    return no_throw([&]() -> int {
        Table t;
        int r = table_parse(table_text, table_len, &t, nullptr);
        if (r < 0) return r;
        std::vector<uint64_t> off;
        std::vector<uint8_t> bytes;
        if ((r = flatten(words, nwords, &off, &bytes)) < 0) return r;
        TableIndex ix;
        bytes.push_back(0);  // data() of an all-empty list is still a pointer
        if ((r = table_index_list(t, table_filter(minlen, maxlen, word_max), off.data(), bytes.data(), nwords, &ix)) < 0)
            return r;
        if (keyspace) *keyspace = ix.keyspace();
        if (kept) *kept = ix.kept();
        if (dropped_len) *dropped_len = ix.dropped_len;
        if (dropped_max) *dropped_max = ix.dropped_max;
        return 0;
    });
}

extern "C" int dwpa_table_candidates(const char* table_text, size_t table_len, const dwpa_bytes* words, size_t nwords,
                                     uint32_t minlen, uint32_t maxlen, uint32_t word_max, const uint64_t* indices,
                                     size_t n, uint8_t* out, uint32_t* out_len) {
    return no_throw([&]() -> int {
        if (n && (!indices || !out || !out_len)) return DWPA_E_ARG;
        Table t;
        int r = table_parse(table_text, table_len, &t, nullptr);
        if (r < 0) return r;
        std::vector<uint64_t> off;
        std::vector<uint8_t> bytes;
        if ((r = flatten(words, nwords, &off, &bytes)) < 0) return r;
        TableIndex ix;
        bytes.push_back(0);
        if ((r = table_index_list(t, table_filter(minlen, maxlen, word_max), off.data(), bytes.data(), nwords, &ix)) < 0)
            return r;
        for (size_t k = 0; k < n; k++)
            if (!table_candidate(t, ix, off.data(), bytes.data(), indices[k], out + 64 * k, &out_len[k]))
                return DWPA_E_ARG;
        return 0;
    });
}
