// remove_map.hpp -- the bookkeeping of sbo_remove: from the caller's indices
// to stored positions, and the renumbering of the rows left.  Host only, no
// HIP header: sbo_remove, sbo_debug_remove_map and a stand-alone program
// (tests/remove_map_main.cpp) compile the same code.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace sbo {

enum class RemoveMapStatus { kOk, kInval, kEmpty };

// order[i] = the caller's index of stored row i (a permutation of 0 .. n-1);
// idx: b caller indices to remove.
//   pos        the b stored positions, ascending
//   keep       the n - b stored positions left, ascending
//   new_order  their renumbered caller indices: the old index minus the number
//              of removed indices below it (numpy.delete's numbering)
// kInval: b < 0, an index outside [0, n) or a duplicate; kEmpty: b == n (a
// model needs a point).  b == 0: kOk, keep is every position.
struct RemoveMap {
    std::vector<int64_t> pos, keep, new_order;
    // the columns the chains cross: per removed point the live columns to its
    // right at the time its chain runs (ascending position, no compaction in
    // between: n - 1 - pos each)
    int64_t rotations = 0;
    // the removed points stored below `limit` (n_sorted's share)
    int64_t below(int64_t limit) const {
        return (int64_t)(std::lower_bound(pos.begin(), pos.end(), limit) - pos.begin());
    }
};

inline RemoveMapStatus remove_map(const int64_t *order, int64_t n, const int64_t *idx, int64_t b, RemoveMap &out) {
    out = RemoveMap{};
    if (n < 0 || b < 0 || (b > 0 && !idx) || (n > 0 && !order)) return RemoveMapStatus::kInval;
    // removed[c]: caller index c goes
    std::vector<char> removed((size_t)n, 0);
    for (int64_t j = 0; j < b; ++j) {
        const int64_t c = idx[j];
        if (c < 0 || c >= n || removed[(size_t)c]) return RemoveMapStatus::kInval;
        removed[(size_t)c] = 1;
    }
    if (b == n && n > 0) return RemoveMapStatus::kEmpty;
    // shift[c]: removed indices below caller index c
    std::vector<int64_t> shift((size_t)n);
    int64_t below = 0;
    for (int64_t c = 0; c < n; ++c) {
        shift[(size_t)c] = below;
        below += removed[(size_t)c];
    }
    out.pos.reserve((size_t)b);
    out.keep.reserve((size_t)(n - b));
    out.new_order.reserve((size_t)(n - b));
    for (int64_t i = 0; i < n; ++i) {
        const int64_t c = order[i];
        if (c < 0 || c >= n) return RemoveMapStatus::kInval;   // (not a permutation)
        if (removed[(size_t)c]) {
            out.pos.push_back(i);
            out.rotations += n - 1 - i;
        } else {
            out.keep.push_back(i);
            out.new_order.push_back(c - shift[(size_t)c]);
        }
    }
    if ((int64_t)out.pos.size() != b) return RemoveMapStatus::kInval;   // (order repeats an index)
    return RemoveMapStatus::kOk;
}

}  // namespace sbo
