// The guided chunk schedule of the persistent spectrogram kernels (stft1024_kernel over tiles,
// cstft4096_kernel over frames): workgroups draw chunks by ticket, each chunk 1 / (div * wgs) of
// what is left when it is cut.  Host only, no HIP types (host_check.cpp compiles it with g++).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace msd {

// bounds = {0, ..., total}: chunk i is [bounds[i], bounds[i + 1]).  A chunk is (total - pos) /
// (div * wgs) items, at least cmin, rounded up to a multiple of `multiple` (the last one ends at
// total); merge_short_tail: a remainder below cmin joins the chunk before it.
inline void guided_chunks(int64_t total, int64_t wgs, int64_t div, int64_t cmin, int64_t multiple,
                          bool merge_short_tail, std::vector<int64_t> &bounds) {
    bounds.assign(1, 0);
    for (int64_t pos = 0; pos < total;) {
        int64_t sz = std::max<int64_t>((total - pos) / (div * wgs), cmin);
        sz = (sz + multiple - 1) / multiple * multiple;
        pos = std::min(total, pos + sz);
        if (merge_short_tail && total - pos > 0 && total - pos < cmin) pos = total;
        bounds.push_back(pos);
    }
}

}  // namespace msd
