// plan_format.hpp -- the tick plan's device format: what the plan kernels
// (kernels.hip) write and the persistent sweeps read through LDS windows
// (plan_walk.hpp).  Host and device; plain integers and no HIP header, so the
// format is tested by a program g++ alone builds (tests/plan_format_main.cpp).
//
//   item descriptor (four ints): x = row block I, y = query block, z = offset
//     of the item's first tile-list entry (low 32 bits), w = its entry count
//     (low 16 bits) | offset bits 32-47 << 16
//   tile-list entry (u16): k-tile index | precision level code << kLevelShift
//   plan key (u64): kept-tile count | non-empty << kPlanKeyShift; in the
//     inclusive scan the high field counts the non-empty items so far
//   step record of the split sweep (four ints, one per kept tile in sweep
//     order): x = the packed tile's offset in the split operand (KiB, two
//     stages of 48: the tile's halves), y = its k-tile's coordinate offset in
//     kc3 (floats), z = query block, w = row block | level code << 16 | first
//     / last tile of its item (kRecFirst, kRecLast)
#pragma once

#include <cstdint>

namespace sbo {

// The sweeps read descriptors, list entries and step records in 1 KiB LDS
// windows, two of each kind, one window ahead of use: a reader may request
// the two windows after the last one it uses, so every buffer is padded by
// kPlanWindowPad windows.
constexpr int kPlanWindowBytes = 1024;
constexpr int kPlanDescWindow = kPlanWindowBytes / 16;   // item descriptors per window
constexpr int kPlanListWindow = kPlanWindowBytes / 2;    // tile-list entries per window
constexpr int kPlanRecWindow = kPlanWindowBytes / 16;    // step records per window
constexpr int kPlanWindowPad = 2;
constexpr int64_t plan_desc_slots(int64_t items) { return items + kPlanWindowPad * kPlanDescWindow; }
constexpr int64_t plan_list_slots(int64_t entries) { return entries + kPlanWindowPad * kPlanListWindow; }
constexpr int64_t plan_rec_slots(int64_t entries) { return entries + kPlanWindowPad * kPlanRecWindow; }

// ---- item descriptor
constexpr int kPlanCountBits = 16, kPlanOffsetBits = 48;
struct PlanItemWords {
    int x, y, z, w;
};
constexpr PlanItemWords plan_item_pack(int I, int qb, uint64_t off, int cnt) {
    return {I, qb, (int)(uint32_t)off, (int)((uint32_t)cnt | ((uint32_t)(off >> 32) << kPlanCountBits))};
}
constexpr int plan_item_count(int w) { return w & ((1 << kPlanCountBits) - 1); }
constexpr uint64_t plan_item_offset(int z, int w) {
    return (uint64_t)(uint32_t)z | ((uint64_t)((uint32_t)w >> kPlanCountBits) << 32);
}

// ---- tile-list entry; level codes 0 (full precision), 1, 2
constexpr int kLevelShift = 14;
constexpr int kPlanLevels = 3;
constexpr int kPlanMaxTiles = 1 << kLevelShift;   // k-tile indices an entry can name
constexpr unsigned short plan_entry_pack(int tile, int level) {
    return (unsigned short)(tile | (level << kLevelShift));
}
constexpr int plan_entry_tile(int entry) { return entry & (kPlanMaxTiles - 1); }
constexpr int plan_entry_level(int entry) { return entry >> kLevelShift; }

// ---- plan key and its scan
constexpr int kPlanKeyShift = 40;
constexpr unsigned long long kPlanCountMask = (1ull << kPlanKeyShift) - 1ull;
constexpr unsigned long long plan_key_pack(int cnt) {
    return (unsigned long long)cnt | ((cnt > 0 ? 1ull : 0ull) << kPlanKeyShift);
}
constexpr uint64_t plan_key_count(unsigned long long key) { return key & kPlanCountMask; }
constexpr int64_t plan_key_items(unsigned long long key) { return (int64_t)(key >> kPlanKeyShift); }

// ---- step record flags
constexpr int kRecLevelShift = 16;
constexpr int kRecFirst = 1 << 20, kRecLast = 1 << 21;

// What the fields hold: query blocks in a descriptor's int, the non-empty
// item count above kPlanKeyShift of a scanned key, the plan's kept-tile total
// (at most `entries`, the dense sweep's) below it, a row block's k-tiles
// (`ktiles`, of the longest) in an entry's tile field.  An item's count is
// at most ktiles and its offset below entries, so the descriptor's 16 and 48
// bits hold them.
constexpr bool plan_fits(int64_t nQ, int64_t items, int64_t entries, int64_t ktiles) {
    return nQ <= 0x7fffffff && items < (1ll << (64 - kPlanKeyShift)) && entries < (1ll << kPlanKeyShift) &&
           ktiles < kPlanMaxTiles;
}
static_assert(kLevelShift <= kPlanCountBits && kPlanKeyShift <= kPlanOffsetBits, "plan_fits covers the descriptor");
static_assert((kPlanLevels - 1) >> (16 - kLevelShift) == 0, "an entry is 16 bits");

}  // namespace sbo
