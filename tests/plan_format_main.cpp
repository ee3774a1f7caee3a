// Round-trips the tick plan's device format (csrc/plan_format.hpp) at the
// edges of every field and checks the capacity predicate at the first value
// past each; built and run by tests/test_plan_format.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "plan_format.hpp"

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);     \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

int main() {
    using namespace sbo;
    {   // item descriptors: every offset edge with every count edge
        const uint64_t offs[] = {0, (1ull << 32) - 1, 1ull << 32, (1ull << 48) - 1, (1ull << 47) | 5, (1ull << 47) - 1};
        const int cnts[] = {1, 0xffff, 0x8000, 0x7fff};
        const int Is[] = {0, 4095}, qbs[] = {0, 0x7fffffff};
        for (uint64_t off : offs)
            for (int cnt : cnts)
                for (int I : Is)
                    for (int qb : qbs) {
                        const PlanItemWords d = plan_item_pack(I, qb, off, cnt);
                        CHECK(d.x == I && d.y == qb);
                        CHECK(plan_item_count(d.w) == cnt);
                        CHECK(plan_item_offset(d.z, d.w) == off);
                    }
        // offset bit 47 lands in w's sign bit, offset bit 31 in z's: both words
        // are negative as ints and still decode
        const PlanItemWords n = plan_item_pack(1, 2, (1ull << 47) | (1ull << 31), 0xffff);
        CHECK(n.w < 0 && n.z < 0);
        CHECK(plan_item_count(n.w) == 0xffff && plan_item_offset(n.z, n.w) == ((1ull << 47) | (1ull << 31)));
        // the layout the kernels and sbo_debug_plan have always read
        const PlanItemWords l = plan_item_pack(3, 7, 0x123456789abcull, 0x0fed);
        CHECK((uint32_t)l.z == 0x56789abcu && (uint32_t)l.w == 0x12340fedu);
    }
    {   // tile-list entries: the tile field's ends under every level code
        const int tiles[] = {0, 1, kPlanMaxTiles / 2, kPlanMaxTiles - 1};
        for (int t : tiles)
            for (int lv = 0; lv < kPlanLevels; ++lv) {
                const unsigned short e = plan_entry_pack(t, lv);
                CHECK(plan_entry_tile(e) == t && plan_entry_level(e) == lv);
            }
        CHECK(plan_entry_pack(kPlanMaxTiles - 1, 2) == 0xbfff && plan_entry_pack(5, 1) == 0x4005);
        CHECK(kPlanMaxTiles == 1 << kLevelShift);
    }
    {   // plan keys and their scan
        CHECK(plan_key_pack(0) == 0ull);
        CHECK(plan_key_count(plan_key_pack(1)) == 1 && plan_key_items(plan_key_pack(1)) == 1);
        CHECK(plan_key_count(plan_key_pack(0xffff)) == 0xffff && plan_key_items(plan_key_pack(0xffff)) == 1);
        // a scan: the largest total beside the largest item count
        const unsigned long long s = kPlanCountMask | (((1ull << (64 - kPlanKeyShift)) - 1ull) << kPlanKeyShift);
        CHECK(plan_key_count(s) == kPlanCountMask && plan_key_items(s) == (1ll << (64 - kPlanKeyShift)) - 1);
    }
    {   // capacity: the last value each field holds, then the first it does not
        const int64_t nQ = 0x7fffffff, items = (1ll << (64 - kPlanKeyShift)) - 1, entries = (1ll << kPlanKeyShift) - 1,
                      ktiles = kPlanMaxTiles - 1;
        CHECK(plan_fits(1, 1, 1, 1));
        CHECK(plan_fits(nQ, items, entries, ktiles));
        CHECK(!plan_fits(nQ + 1, items, entries, ktiles));
        CHECK(!plan_fits(nQ, items + 1, entries, ktiles));
        CHECK(!plan_fits(nQ, items, entries + 1, ktiles));
        CHECK(!plan_fits(nQ, items, entries, ktiles + 1));
        // what fits packs: the largest count and offset a fitting plan can hold
        const PlanItemWords d = plan_item_pack(0, (int)nQ, (uint64_t)entries - 1, (int)ktiles);
        CHECK(plan_item_count(d.w) == ktiles && plan_item_offset(d.z, d.w) == (uint64_t)entries - 1);
    }
    {   // windows: one KiB each, and the padding covers the look-ahead
        CHECK(kPlanDescWindow * 16 == kPlanWindowBytes && kPlanListWindow * 2 == kPlanWindowBytes &&
              kPlanRecWindow * 16 == kPlanWindowBytes);
        // a reader at the last element of a buffer of n has requested at most
        // window n / W + 1 (one ahead of its own), the prologue windows w and w + 1
        const int64_t ns[] = {1, kPlanListWindow - 1, kPlanListWindow, kPlanListWindow + 1, 1000003};
        for (int64_t n : ns) {
            CHECK(plan_desc_slots(n) >= ((n - 1) / kPlanDescWindow + 2) * kPlanDescWindow);
            CHECK(plan_list_slots(n) >= ((n - 1) / kPlanListWindow + 2) * kPlanListWindow);
            CHECK(plan_rec_slots(n) >= ((n - 1) / kPlanRecWindow + 2) * kPlanRecWindow);
        }
    }
    std::puts("plan_format ok");
    return 0;
}
