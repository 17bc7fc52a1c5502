// table.hpp -- table attack, host side (no HIP): the substitution table and its text, a word's candidate count, the
// kept-word index over a list, and candidate `id` (internal to libdwpa22000.so; the C entry points dwpa_table_parse /
// dwpa_table_builtin / dwpa_table_keyspace / dwpa_table_candidates are in table.cpp).
//
// Table: for every byte value c a list alt[c] of 1..16 distinct replacement bytes, in file order.  A byte the text
// never names as a key has alt[c] = [c]; a key keeps its original only if the text says so (a=a), as in
// hashcat-legacy's --table-file.  Text, strict: every non-empty line, after one trailing CR is removed, is K=V with K
// and V each one literal byte or \xHH; a repeated (K, V) line is ignored; any other line, a 17th alternative for one
// key, or a text without a mapping is an error that names the line.  Replacements are one byte each, so a candidate has
// its word's length.
//
// A word of L bytes is kept iff minlen <= L <= maxlen (maxlen clamped to 63) and its count k_w = the product of
// nalt[w[i]] is at most word_max (1..2^32 - 1; 0 means 2^32 - 1); the product saturates and never wraps.  Kept words
// stand in list order: start[j] = the exclusive prefix sum of their counts (u64), K = start[nkept] <= 2^64 - 1.
// Candidate id belongs to kept word j with start[j] <= id < start[j + 1]; sub = id - start[j] is the mixed-radix
// numeral over the word's positions, last position fastest (itertools.product over the alternative lists).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "dwpa22000.h"

namespace dwpa {

constexpr uint32_t TABLE_MAX_ALT = DWPA_TABLE_MAX_ALT;
constexpr uint32_t TABLE_MAX_LEN = 63;

// The device image as well: u8 nalt[256], then u8 alt[256][16] (unused entries 0).
struct Table {
    uint8_t nalt[256];
    uint8_t alt[256][TABLE_MAX_ALT];
};
static_assert(sizeof(Table) == DWPA_TABLE_IMAGE_BYTES, "the table image is 256 + 256 x 16 bytes");

// The number of mappings kept (>= 1), or DWPA_E_ARG with *bad_line (nullable) = the 1-based line at fault (for a text
// without any mapping: the number of lines + 1).
int table_parse(const char* text, size_t len, Table* out, uint32_t* bad_line);
// The text of a built-in table ("toggle": every ASCII letter -> itself, the other case); empty: no such table.
std::string table_builtin(const char* name);
// The file at `path` parsed: the number of mappings, DWPA_E_IO (unreadable) or DWPA_E_ARG.
int table_read_file(const char* path, Table* out, uint32_t* bad_line);

struct TableFilter {
    uint32_t minlen = 8, maxlen = TABLE_MAX_LEN, word_max = UINT32_MAX;
};
// minlen / maxlen / word_max as the calls take them: maxlen clamped to 63, word_max 0 = 2^32 - 1.
inline TableFilter table_filter(uint32_t minlen, uint32_t maxlen, uint32_t word_max) {
    return TableFilter{minlen, maxlen < TABLE_MAX_LEN ? maxlen : TABLE_MAX_LEN, word_max ? word_max : UINT32_MAX};
}

// The saturating product of nalt over the word: UINT64_MAX for 2^64 - 1 and above.
uint64_t table_word_count(const Table& t, const uint8_t* w, size_t len);

enum { TABLE_KEPT = 0, TABLE_DROP_LEN = 1, TABLE_DROP_MAX = 2 };
// The word's count as the count kernel writes it: 1..word_max, or 0 for a dropped word with *why (nullable) set.
uint32_t table_kept_count(const Table& t, const TableFilter& f, const uint8_t* w, size_t len, int* why);

struct TableIndex {
    std::vector<uint64_t> start{0};  // nkept + 1
    std::vector<uint32_t> kword;     // nkept list indices
    uint64_t dropped_len = 0, dropped_max = 0;
    uint64_t keyspace() const { return start.back(); }
    uint64_t kept() const { return kword.size(); }
};
// From per-word counts (0: dropped).  DWPA_E_ARG: K above 2^64 - 1; the drop counters are left alone.
int table_index_counts(const uint32_t* counts, size_t nwords, TableIndex* ix);
// From a host list (off: nwords + 1 byte offsets into bytes).  DWPA_E_ARG: nwords >= 2^32, K above 2^64 - 1.
int table_index_list(const Table& t, const TableFilter& f, const uint64_t* off, const uint8_t* bytes, size_t nwords,
                     TableIndex* ix);
// Candidate `id` into out[0..*len): false for id >= K.
bool table_candidate(const Table& t, const TableIndex& ix, const uint64_t* off, const uint8_t* bytes, uint64_t id,
                     uint8_t out[64], uint32_t* len);

}  // namespace dwpa
