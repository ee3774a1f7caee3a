// operand_state.hpp -- how much of an operand derived from the packed model is
// valid: the row blocks below `from`, in layout `layout`.  The owners of the two
// derived operands (sbo_ctx.hpp) keep one each; nobody else writes it.  Host
// only, no HIP header: a stand-alone program can compile it.
#pragma once

#include <algorithm>
#include <cstdint>

namespace sbo {

class OperandState {
public:
    // rows from row block I0 on changed / every row changed
    void touch(int64_t I0) { from_ = std::min(from_, std::max<int64_t>(I0, 0)); }
    void touch_all() { from_ = 0; }
    // the first row block a derivation in `layout` has to write: 0 after a
    // change of layout (nothing derived in another one is kept), and nI or
    // more when there is nothing to do for nI row blocks
    int64_t start(int layout) const { return layout == layout_ ? from_ : 0; }
    // derived up to date in `layout`
    void mark(int layout) {
        from_ = kNone;
        layout_ = layout;
    }
    bool current(int64_t nI, int layout) const { return start(layout) >= nI; }
    // the layout last derived (-1: never), and start() with -1 for "nothing stale"
    int layout() const { return layout_; }
    int64_t stale_from(int layout) const { return start(layout) == kNone ? -1 : start(layout); }

private:
    static constexpr int64_t kNone = INT64_MAX;
    int64_t from_ = 0;
    int layout_ = -1;
};

}  // namespace sbo
