// markov.cpp -- the Markov model of the mask attack on the host (markov.hpp): no HIP.  The trainer reads its word
// lists through the dictionary reader, so they are cut exactly as every attack cuts them.
#include "markov.hpp"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <numeric>
#include <string>

#include "dict_reader.hpp"
#include "engine.hpp"

namespace dwpa {

namespace {

const uint8_t MAGIC[MARKOV_HEADER] = {'D', 'W', 'P', 'A', 'M', 'K', 'V', '1', MARKOV_POS, 0, 0, 0, 0, 0, 0, 0};

}  // namespace

int markov_validate(const uint8_t* model, size_t len) {
    if (!model || len != MARKOV_FILE_BYTES || memcmp(model, MAGIC, MARKOV_HEADER) != 0) return DWPA_E_ARG;
    for (size_t row = 0; row < (size_t)MARKOV_POS * 256; row++) {
        const uint8_t* r = model + MARKOV_HEADER + row * 256;
        uint64_t seen[4] = {0, 0, 0, 0};  // 256 distinct bytes set all 256 bits
        for (int d = 0; d < 256; d++) seen[r[d] >> 6] |= 1ull << (r[d] & 63);
        if ((seen[0] & seen[1] & seen[2] & seen[3]) != ~0ull) return DWPA_E_ARG;
    }
    return 0;
}

int markov_read_file(const char* path, std::vector<uint8_t>* out) {
    FILE* f = path ? fopen(path, "rb") : nullptr;
    if (!f) return DWPA_E_IO;
    out->resize(MARKOV_FILE_BYTES + 1);  // one byte more: a longer file shows
    const size_t got = fread(out->data(), 1, out->size(), f);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) return DWPA_E_IO;
    out->resize(got);
    return markov_validate(out->data(), out->size());
}

int markov_mask(const Mask& sets, uint32_t threshold, MarkovMask* out) {
    if (threshold > 256 || sets.npos == 0 || sets.npos > MARKOV_POS) return DWPA_E_ARG;
    out->npos = sets.npos;
    out->keyspace = 1;
    memset(out->radix, 0, sizeof out->radix);
    memset(out->member, 0, sizeof out->member);
    for (uint32_t p = 0; p < sets.npos; p++) {
        const uint32_t n = sets.pos[p].radix, r = threshold && threshold < n ? threshold : n;
        for (uint32_t j = 0; j < n; j++) out->member[p][sets.pos[p].bytes[j]] = 1;
        out->radix[p] = r;
        if (out->keyspace > UINT64_MAX / r) return DWPA_E_ARG;  // K above 2^64 - 1
        out->keyspace *= r;
    }
    return 0;
}

void markov_prefix(const MarkovMask& mm, uint32_t n, MarkovMask* out) {
    *out = mm;
    out->npos = n;
    out->keyspace = 1;
    for (uint32_t p = 0; p < MARKOV_POS; p++) {
        if (p < n) {
            out->keyspace *= mm.radix[p];
        } else {
            out->radix[p] = 0;
            memset(out->member[p], 0, 256);
        }
    }
}

void markov_digits(const MarkovMask& mm, uint64_t index, uint8_t digits[64]) {
    memset(digits, 0, 64);
    for (uint32_t p = mm.npos; p-- > 0;) {
        const uint32_t r = mm.radix[p];
        digits[p] = (uint8_t)(index % r);
        index /= r;
    }
}

namespace {

// row(p, a)[0..r_p) into dst: order[p][a] filtered to the members of S_p.
void filtered_row(const MarkovMask& mm, const uint8_t* model, uint32_t p, uint32_t a, uint8_t* dst) {
    const uint8_t* row = markov_row(model, p, a);
    const uint32_t r = mm.radix[p];
    uint32_t k = 0;
    for (int j = 0; j < 256 && k < r; j++)
        if (mm.member[p][row[j]]) dst[k++] = row[j];
}

}  // namespace

void markov_candidate(const MarkovMask& mm, const uint8_t* model, uint64_t index, uint8_t* out) {
    uint8_t d[64], row[256];
    markov_digits(mm, index, d);
    uint32_t prev = 0;
    for (uint32_t p = 0; p < mm.npos; p++) {
        filtered_row(mm, model, p, prev, row);
        out[p] = row[d[p]];
        prev = out[p];
    }
}

void markov_table(const MarkovMask& mm, const uint8_t* model, uint8_t* table) {
    for (uint32_t p = 0; p < mm.npos; p++) memcpy(table + 4 * p, &mm.radix[p], 4);
    bool reach[256] = {};  // the predecessors that can occur at position p
    reach[0] = true;
    for (uint32_t p = 0; p < mm.npos; p++) {
        bool next[256] = {};
        for (uint32_t a = 0; a < 256; a++) {
            if (!reach[a]) continue;
            uint8_t* dst = table + MARKOV_TABLE_NEXT + ((size_t)p * 256 + a) * 256;
            filtered_row(mm, model, p, a, dst);
            for (uint32_t d = 0; d < mm.radix[p]; d++) next[dst[d]] = true;
        }
        memcpy(reach, next, sizeof reach);
    }
}

namespace {

int markov_train(const char* const* dicts, size_t ndicts, const char* out_file, uint64_t* words) {
    if (!dicts || !ndicts || !out_file) return DWPA_E_ARG;
    std::vector<std::string> paths;
    for (size_t i = 0; i < ndicts; i++) {
        if (!dicts[i]) return DWPA_E_ARG;
        paths.emplace_back(dicts[i]);
    }
    std::vector<uint64_t> n((size_t)MARKOV_POS * 256 * 256, 0);
    uint64_t counted = 0;
    bool err = false, damaged = false;
    {
        DictReader rd(paths);
        Chunk c;
        while (rd.next(c, (size_t)1 << 20, (size_t)64 << 20, err)) {
            for (size_t w = 0; w + 1 < c.off.size(); w++) {
                const uint8_t* s = (const uint8_t*)c.bytes.data() + c.off[w];
                const size_t len = std::min<size_t>(c.off[w + 1] - c.off[w], MARKOV_POS);
                if (!len) continue;
                counted++;
                uint32_t prev = 0;
                for (size_t p = 0; p < len; p++) {
                    n[(p * 256 + prev) * 256 + s[p]]++;
                    prev = s[p];
                }
            }
        }
        damaged = rd.damaged();
    }
    if (words) *words = counted;
    if (err || damaged) return DWPA_E_IO;  // a damaged gzip stream was counted up to the damage; no file is written
    std::vector<uint8_t> img(MARKOV_FILE_BYTES);
    memcpy(img.data(), MAGIC, MARKOV_HEADER);
    for (size_t row = 0; row < (size_t)MARKOV_POS * 256; row++) {
        const uint64_t* cnt = n.data() + row * 256;
        uint8_t* o = img.data() + MARKOV_HEADER + row * 256;
        std::iota(o, o + 256, (uint8_t)0);
        if (std::any_of(cnt, cnt + 256, [](uint64_t v) { return v != 0; }))
            std::stable_sort(o, o + 256, [cnt](uint8_t x, uint8_t y) { return cnt[x] > cnt[y]; });
    }
    FILE* f = fopen(out_file, "wb");
    if (!f) return DWPA_E_IO;
    const bool ok = fwrite(img.data(), 1, img.size(), f) == img.size();
    if (fclose(f) != 0 || !ok) {
        remove(out_file);
        return DWPA_E_IO;
    }
    return 0;
}

}  // namespace

}  // namespace dwpa

extern "C" {

int dwpa_markov_train(const char* const* dicts, size_t ndicts, const char* out_file, uint64_t* words) {
    return dwpa::guarded([&]() -> int { return dwpa::markov_train(dicts, ndicts, out_file, words); }, DWPA_E_NOMEM,
                         DWPA_E_IO);
}

int dwpa_markov_load(const char* path, uint8_t* out, size_t cap) {
    return dwpa::guarded([&]() -> int {
        std::vector<uint8_t> img;
        const int r = dwpa::markov_read_file(path, &img);
        if (r < 0) return r;
        if (!out || cap < img.size()) return DWPA_E_ARG;
        memcpy(out, img.data(), img.size());
        return 0;
    });
}

int dwpa_markov_check(const uint8_t* model, size_t model_len) { return dwpa::markov_validate(model, model_len); }

int dwpa_mask_keyspace_markov(const char* mask, size_t mask_len, const dwpa_bytes custom[4], uint32_t threshold,
                              uint32_t* positions, uint64_t* keyspace) {
    return dwpa::guarded([&]() -> int {
        if (threshold > 256) return DWPA_E_ARG;
        auto sets = std::make_unique<dwpa::Mask>();
        auto mm = std::make_unique<dwpa::MarkovMask>();
        int r = dwpa::mask_parse_sets(mask, mask_len, custom, sets.get());
        if (r < 0 || (r = dwpa::markov_mask(*sets, threshold, mm.get())) < 0) return r;
        if (positions) *positions = mm->npos;
        if (keyspace) *keyspace = mm->keyspace;
        return 0;
    });
}

int dwpa_mask_candidates_markov(const char* mask, size_t mask_len, const dwpa_bytes custom[4], const uint8_t* model,
                                size_t model_len, uint32_t threshold, const uint64_t* indices, size_t n, uint8_t* out,
                                uint32_t* out_len) {
    return dwpa::guarded([&]() -> int {
        if ((n && (!indices || !out)) || !out_len || threshold > 256) return DWPA_E_ARG;
        auto sets = std::make_unique<dwpa::Mask>();
        auto mm = std::make_unique<dwpa::MarkovMask>();
        int r = dwpa::mask_parse_sets(mask, mask_len, custom, sets.get());
        if (r < 0 || (r = dwpa::markov_mask(*sets, threshold, mm.get())) < 0) return r;
        if ((r = dwpa::markov_validate(model, model_len)) < 0) return r;
        for (size_t k = 0; k < n; k++)
            if (indices[k] >= mm->keyspace) return DWPA_E_ARG;
        memset(out, 0, n * 64);
        for (size_t k = 0; k < n; k++) dwpa::markov_candidate(*mm, model, indices[k], out + 64 * k);
        *out_len = mm->npos;
        return 0;
    });
}

int dwpa_mask_candidate_markov(const char* mask, size_t mask_len, const dwpa_bytes custom[4], const uint8_t* model,
                               size_t model_len, uint32_t threshold, uint64_t index, uint8_t out[64],
                               uint32_t* out_len) {
    if (!out) return DWPA_E_ARG;
    return dwpa_mask_candidates_markov(mask, mask_len, custom, model, model_len, threshold, &index, 1, out, out_len);
}

}  // extern "C"
