// sbo_remove's bookkeeping (csrc/remove_map.hpp) at its edges: stored
// positions, numpy.delete's renumbering, the rotation count and every
// rejected input; built and run by tests/test_remove_map.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "remove_map.hpp"

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);     \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

int main() {
    using namespace sbo;
    using V = std::vector<int64_t>;
    const auto ok = RemoveMapStatus::kOk, inval = RemoveMapStatus::kInval, empty = RemoveMapStatus::kEmpty;
    RemoveMap m;
    {   // a shuffled order: caller indices 1 and 4 go
        const V order = {3, 1, 5, 0, 4, 2}, idx = {4, 1};
        CHECK(remove_map(order.data(), 6, idx.data(), 2, m) == ok);
        CHECK((m.pos == V{1, 4}));
        CHECK((m.keep == V{0, 2, 3, 5}));
        // numpy.delete: 0 2 3 5 -> 0 1 2 3
        CHECK((m.new_order == V{2, 3, 0, 1}));
        CHECK(m.rotations == (6 - 1 - 1) + (6 - 1 - 4));
        CHECK(m.below(0) == 0 && m.below(1) == 0 && m.below(2) == 1 && m.below(4) == 1 && m.below(5) == 2 &&
              m.below(6) == 2);
    }
    {   // first and last stored position, the identity order
        const V order = {0, 1, 2, 3}, first = {0}, last = {3};
        CHECK(remove_map(order.data(), 4, first.data(), 1, m) == ok);
        CHECK((m.pos == V{0}) && (m.new_order == V{0, 1, 2}) && m.rotations == 3);
        CHECK(remove_map(order.data(), 4, last.data(), 1, m) == ok);
        CHECK((m.pos == V{3}) && (m.new_order == V{0, 1, 2}) && m.rotations == 0);
    }
    {   // b == 0: nothing goes, with or without an idx pointer
        const V order = {1, 0};
        CHECK(remove_map(order.data(), 2, nullptr, 0, m) == ok);
        CHECK(m.pos.empty() && (m.keep == V{0, 1}) && (m.new_order == V{1, 0}) && m.rotations == 0);
    }
    {   // all but one
        const V order = {2, 0, 1}, idx = {0, 2};
        CHECK(remove_map(order.data(), 3, idx.data(), 2, m) == ok);
        CHECK((m.pos == V{0, 1}) && (m.keep == V{2}) && (m.new_order == V{0}));
    }
    {   // rejected: a duplicate, -1, n, b == n, b < 0, a null idx with b > 0
        const V order = {2, 0, 1};
        const V dup = {1, 1}, neg = {-1}, big = {3}, all = {0, 1, 2}, dup_all = {0, 1, 1};
        CHECK(remove_map(order.data(), 3, dup.data(), 2, m) == inval);
        CHECK(remove_map(order.data(), 3, neg.data(), 1, m) == inval);
        CHECK(remove_map(order.data(), 3, big.data(), 1, m) == inval);
        CHECK(remove_map(order.data(), 3, all.data(), 3, m) == empty);
        CHECK(remove_map(order.data(), 3, dup_all.data(), 3, m) == inval);
        CHECK(remove_map(order.data(), 3, all.data(), -1, m) == inval);
        CHECK(remove_map(order.data(), 3, nullptr, 1, m) == inval);
        CHECK(m.pos.empty() && m.keep.empty() && m.new_order.empty());
    }
    {   // an order that is no permutation is refused, not read past
        const V bad = {0, 0, 1}, far = {0, 7, 1}, idx = {0};
        CHECK(remove_map(bad.data(), 3, idx.data(), 1, m) == inval);
        CHECK(remove_map(far.data(), 3, idx.data(), 1, m) == inval);
    }
    std::puts("remove_map ok");
    return 0;
}
