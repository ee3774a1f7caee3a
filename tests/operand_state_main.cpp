// Walks sbo::OperandState (csrc/operand_state.hpp) through the rules the two
// derived operands rely on; built and run by tests/test_operand_state.py.
#include <cstdio>
#include <cstdlib>

#include "operand_state.hpp"

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);     \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

int main() {
    using sbo::OperandState;
    {   // a new record: everything stale, no layout
        OperandState s;
        CHECK(s.layout() == -1 && s.start(2) == 0 && s.stale_from(2) == 0);
        CHECK(!s.current(2, 2));
        CHECK(s.current(0, 2));   // (no row blocks: nothing to derive)
    }
    {   // touch then derive
        OperandState s;
        s.touch(1);
        CHECK(s.start(2) == 0);   // (never derived: the touch cannot raise it)
        s.mark(2);
        CHECK(s.layout() == 2 && s.current(3, 2) && s.stale_from(2) == -1);
        s.touch(1);
        CHECK(!s.current(3, 2) && s.start(2) == 1 && s.stale_from(2) == 1);
        s.touch(2);               // a later touch further up keeps the lower start
        CHECK(s.start(2) == 1);
        s.touch(0);
        CHECK(s.start(2) == 0);
        s.mark(2);
        CHECK(s.current(3, 2));
    }
    {   // a layout change forces 0, whatever was current or stale before
        OperandState s;
        s.mark(2);
        CHECK(s.current(3, 2) && !s.current(3, 0) && s.start(0) == 0 && s.stale_from(0) == 0);
        s.touch(2);
        CHECK(s.start(2) == 2 && s.start(1) == 0);
        s.mark(0);                // derived in the other layout: the old one is gone
        CHECK(s.layout() == 0 && s.current(3, 0) && s.start(2) == 0);
    }
    {   // touch below a current operand
        OperandState s;
        s.mark(1);
        s.touch(0);
        CHECK(!s.current(1, 1) && s.start(1) == 0);
        s.mark(1);
        s.touch_all();
        CHECK(!s.current(1, 1) && s.start(1) == 0 && s.layout() == 1);
        s.touch(-5);              // (clamped)
        CHECK(s.start(1) == 0);
    }
    {   // touch above nI: still current for nI row blocks
        OperandState s;
        s.mark(1);
        s.touch(4);
        CHECK(s.current(3, 1) && s.current(4, 1) && !s.current(5, 1) && s.stale_from(1) == 4);
    }
    {   // current, then a query with another nI
        OperandState s;
        s.mark(2);
        CHECK(s.current(2, 2) && s.current(1000000, 2) && s.current(0, 2));
        s.touch(2);               // an append that opens row block 2
        CHECK(s.current(2, 2) && !s.current(3, 2));
    }
    std::puts("operand_state ok");
    return 0;
}
