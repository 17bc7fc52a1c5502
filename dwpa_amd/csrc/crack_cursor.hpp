// crack_cursor.hpp -- the shared cursor of the range attacks (crack_range.cpp): a list of segments of ascending
// indices, handed out in batch-sized ranges to whichever worker asks next.  Host only (no HIP header), so that
// tools/range_cursor_check.cpp can run it under ThreadSanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>

namespace dwpa {

struct RangeSegment {
    uint64_t begin, end;  // indices [begin, end)
};

class RangeCursor {
  public:
    explicit RangeCursor(std::vector<RangeSegment> segs) : segs_(std::move(segs)) {
        if (!segs_.empty()) next_ = segs_[0].begin;
    }
    // The next range: segment index, first index, count (1..cap; a range never crosses a segment).  False once the
    // segments are exhausted, and from then on.
    bool take(uint32_t cap, size_t* seg, uint64_t* first, uint32_t* count) {
        std::lock_guard<std::mutex> lk(mu_);
        while (seg_ < segs_.size() && next_ >= segs_[seg_].end)
            if (++seg_ < segs_.size()) next_ = segs_[seg_].begin;
        if (seg_ == segs_.size()) return false;
        *seg = seg_;
        *first = next_;
        *count = (uint32_t)std::min<uint64_t>(cap, segs_[seg_].end - next_);
        next_ += *count;  // at most end: no wrap, whatever the segment
        return true;
    }

  private:
    std::mutex mu_;
    const std::vector<RangeSegment> segs_;
    size_t seg_ = 0;
    uint64_t next_ = 0;  // next index of segs_[seg_]
};

}  // namespace dwpa
