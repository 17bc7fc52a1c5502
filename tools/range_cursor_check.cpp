// range_cursor_check.cpp -- the range attacks' shared cursor (dwpa_amd/csrc/crack_cursor.hpp) on the host, built with
// -fsanitize=thread: every segment list below is drained with cap = 4 by 1 thread and by 8 threads.  The ranges taken
// must tile the segments exactly (no gap, no overlap, none crossing a segment), every count must be 1..cap, one thread
// must see ascending order within a segment and the segments in list order, and once the cursor is exhausted eight
// more take() calls must say so.  Indices near 2^64 and concurrent takers are what no GPU-less test reaches otherwise.
// Exit status 0 and one JSON line, or 1 and the first failure on stderr.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <thread>
#include <tuple>
#include <vector>

#include "crack_cursor.hpp"

using dwpa::RangeCursor;
using dwpa::RangeSegment;

namespace {

constexpr uint32_t CAP = 4;

struct Taken {
    size_t seg;
    uint64_t first;
    uint32_t count;
};

bool fail(const char* name, int threads, const char* what) {
    fprintf(stderr, "range_cursor_check: %s, %d thread(s): %s\n", name, threads, what);
    return false;
}

bool run_case(const char* name, const std::vector<RangeSegment>& segs, int threads, uint64_t* ranges) {
    RangeCursor cursor(segs);
    std::vector<std::vector<Taken>> per(threads);
    auto drain = [&](int t) {
        Taken k;
        while (cursor.take(CAP, &k.seg, &k.first, &k.count)) per[t].push_back(k);
    };
    std::vector<std::thread> th;
    for (int t = 1; t < threads; t++) th.emplace_back(drain, t);
    drain(0);
    for (auto& t : th) t.join();
    for (int i = 0; i < 8; i++) {
        Taken k;
        if (cursor.take(CAP, &k.seg, &k.first, &k.count)) return fail(name, threads, "take() after exhaustion");
    }
    if (threads == 1)
        for (size_t i = 1; i < per[0].size(); i++) {
            const Taken &a = per[0][i - 1], &b = per[0][i];
            if (b.seg < a.seg || (b.seg == a.seg && b.first <= a.first)) return fail(name, threads, "order");
        }
    std::vector<Taken> all;
    for (auto& p : per) all.insert(all.end(), p.begin(), p.end());
    std::sort(all.begin(), all.end(),
              [](const Taken& a, const Taken& b) { return std::tie(a.seg, a.first) < std::tie(b.seg, b.first); });
    // walk the segments and the sorted ranges together: each range must start where the one before it ended
    size_t i = 0;
    for (size_t s = 0; s < segs.size(); s++) {
        uint64_t at = segs[s].begin;
        while (at < segs[s].end) {
            if (i == all.size() || all[i].seg != s || all[i].first != at) return fail(name, threads, "gap or overlap");
            if (all[i].count < 1 || all[i].count > CAP) return fail(name, threads, "count outside 1..cap");
            if (all[i].count > segs[s].end - at) return fail(name, threads, "range crosses its segment");
            at += all[i++].count;
        }
    }
    if (i != all.size()) return fail(name, threads, "a range outside every segment");
    *ranges += all.size();
    return true;
}

}  // namespace

int main() {
    const uint64_t top = UINT64_MAX;  // 2^64 - 1
    const struct {
        const char* name;
        std::vector<RangeSegment> segs;
    } cases[] = {
        {"no segment", {}},
        {"an empty segment between two", {{0, 6}, {7, 7}, {3, 12}}},
        {"one index", {{5, 6}}},
        {"three batches and one", {{0, 3 * CAP + 1}}},
        {"the top of 2^64", {{top - 10, top}}},
    };
    uint64_t ranges = 0;
    for (const auto& c : cases)
        for (int threads : {1, 8})
            if (!run_case(c.name, c.segs, threads, &ranges)) return 1;
    printf("{\"cases\": %zu, \"ranges\": %llu}\n", sizeof cases / sizeof cases[0], (unsigned long long)ranges);
    return 0;
}
