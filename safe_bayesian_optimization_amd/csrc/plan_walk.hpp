// plan_walk.hpp -- how a persistent sweep workgroup walks its part of the
// tick plan (plan_format.hpp): predict_kernel (kernels.hip),
// predict_f64_kernel (predict_f64.hip) and predict_oz_kernel,
// predict_oz2_kernel, predict_oz3_kernel (predict_oz.hip).  Device only.
// (ozgemm.hip takes the LDS-DMA primitive lds_dma16 from here and nothing else.)
//
// Workgroup b owns the items seg[r(b)] .. seg[r(b) + 1] of the descriptor
// list.  It reads descriptors and tile-list entries from two 1 KiB LDS
// windows of each kind, refilled one window ahead by LDS-DMA from one wave,
// and retires every DMA with the vmcnt wait and barrier that end each step.
// Whatever the plan's buffers hold, the walk addresses nothing outside them:
// the range is clamped to the item count, a descriptor's row block to the
// operand's, an entry's k-tile to its row block's, and a window request goes
// at most kPlanWindowPad windows past the last one used, which the buffers
// are padded for.
#pragma once

#include <cstdint>

#include "sbo_internal.hpp"

namespace sbo {
namespace {

// LDS-DMA: global_load_lds_dwordx4 moves 16 B per lane, 1 KiB per wave
// instruction, lane-linear from the per-lane address gsrc to the
// wave-uniform LDS address ldst, with no staging registers.  It is issued
// from inline asm so that hipcc does not see an LDS write in flight: with a
// compiler-visible one pending it drains every ds_read wait to lgkmcnt(0)
// (waiting on reads issued one instruction earlier) instead of counting.  The
// callers therefore retire it themselves, by an explicit vmcnt wait and a
// barrier before the bytes are read (plan_dma_landed).  m0, the LDS base the
// instruction takes, is saved and restored around it.
__device__ __forceinline__ void lds_dma16(const void *gsrc, uint32_t ldst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(ldst)
                 : "memory");
}
__device__ __forceinline__ void plan_dma_landed() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// The workgroup's item range.  Consecutive ranges go to one XCD (workgroups
// are dealt to the 8 XCDs round-robin), so an XCD's L2 sees neighbouring
// items.
struct PlanRange {
    int k0, k1;
};
__device__ __forceinline__ PlanRange plan_range(const int *__restrict__ seg, int P, int n_items) {
    const int bid = blockIdx.x;
    const int rng = (P % 8 == 0) ? (bid % 8) * (P / 8) + bid / 8 : bid;
    return {max(seg[rng], 0), min(seg[rng + 1], n_items)};
}

constexpr int kPlanWalkLds = 4 * kPlanWindowBytes;   // two descriptor windows, then two list windows

// The workgroup's view of its windows: kPlanWalkLds bytes of LDS at `win`.
// Window w of a kind lives in slot w & 1.
struct PlanWindows {
    const int4 *dwin;
    const unsigned short *lwin;
    int nI;

    __device__ __forceinline__ PlanWindows(const char *win, int nI_)
        : dwin(reinterpret_cast<const int4 *>(win)),
          lwin(reinterpret_cast<const unsigned short *>(win + 2 * kPlanWindowBytes)), nI(nI_) {}

    // descriptor k from its (loaded) window, wave-uniform; w keeps the packed
    // count and offset bits (plan_item_count)
    __device__ __forceinline__ int4 desc_at(int k) const {
        const int4 d = dwin[((k / kPlanDescWindow) & 1) * kPlanDescWindow + k % kPlanDescWindow];
        const int I = min(max(__builtin_amdgcn_readfirstlane(d.x), 0), nI - 1);
        return make_int4(I, __builtin_amdgcn_readfirstlane(d.y), __builtin_amdgcn_readfirstlane(d.z),
                         __builtin_amdgcn_readfirstlane(d.w));
    }
    // the k-tile of tile-list entry e, an entry of row block I (the level
    // code is dropped: these sweeps run every tile at one precision)
    __device__ __forceinline__ int list_at(uint64_t e, int I) const {
        const int t = plan_entry_tile(
            __builtin_amdgcn_readfirstlane((int)lwin[((e / kPlanListWindow) & 1) * kPlanListWindow + e % kPlanListWindow]));
        return min(t, kTilesPerRowBlockStep * (I + 1) - 1);
    }
};
__device__ __forceinline__ uint64_t entry_off(const int4 &d) { return plan_item_offset(d.z, d.w); }

// The refills, by the m0-saving DMA: wave-uniform `fill_desc` / `fill_list`
// name the one wave that moves each kind.
struct PlanRefill {
    const char *gD, *gL;
    uint32_t lds_dwin, lds_lwin;
    bool fill_desc, fill_list;

    __device__ __forceinline__ PlanRefill(const char *win, const int4 *desc, const unsigned short *tl, int lane,
                                          bool fill_desc_, bool fill_list_)
        : gD(reinterpret_cast<const char *>(desc) + lane * 16), gL(reinterpret_cast<const char *>(tl) + lane * 16),
          lds_dwin((uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char *)(win)),
          lds_lwin(lds_dwin + 2u * kPlanWindowBytes), fill_desc(fill_desc_), fill_list(fill_list_) {}

    __device__ __forceinline__ void desc_window(int64_t w) const {
        if (fill_desc) lds_dma16(gD + w * kPlanWindowBytes, lds_dwin + (uint32_t)(w & 1) * kPlanWindowBytes);
    }
    __device__ __forceinline__ void list_window(int64_t w) const {
        if (fill_list) lds_dma16(gL + w * kPlanWindowBytes, lds_lwin + (uint32_t)(w & 1) * kPlanWindowBytes);
    }
    // entering item k / entry e: at a window's first element, request the
    // window after it
    __device__ __forceinline__ void enter_item(int k) const {
        if (k % kPlanDescWindow == 0) desc_window(k / kPlanDescWindow + 1);
    }
    __device__ __forceinline__ void enter_entry(uint64_t e) const {
        if (e % kPlanListWindow == 0) list_window(e / kPlanListWindow + 1);
    }
    // from entry e on to entry en > e, not necessarily the next one
    __device__ __forceinline__ void move_entry(uint64_t e, uint64_t en) const {
        if (en / kPlanListWindow != e / kPlanListWindow) list_window(en / kPlanListWindow + 1);
    }
    // The prologue, in two steps: the first two descriptor windows, landed
    // (then desc_at(k0) gives the first entry e), and the first two list
    // windows from e, landed.
    __device__ __forceinline__ void begin_items(int k0) const {
        desc_window(k0 / kPlanDescWindow);
        desc_window(k0 / kPlanDescWindow + 1);
        plan_dma_landed();
    }
    __device__ __forceinline__ void begin_entries(uint64_t e) const {
        list_window(e / kPlanListWindow);
        list_window(e / kPlanListWindow + 1);
        plan_dma_landed();
    }
};

}  // namespace
}  // namespace sbo
