// inverse.hpp -- the f64 inverse of the factor (inverse.cpp): the plan of its
// block recursion, the lanes it runs on, the reservation and the run stages.
// Host only.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "sbo_internal.hpp"

namespace sbo {

// Appends of at most kAppendInvRows points solve their factor rows and extend
// the inverse by matrix-vector products with the kept f64 inverse
// (bandwidth-bound, one pass over its lower triangle per point); up to
// kAppendInvGemm points the factor rows by one f64 GEMM with it (rocBLAS strsm
// of a b x n block ran as hundreds of small launches); alpha is updated from
// the kept z = L^-1 r up to kAppendInvGemm points too.  Larger batches: the
// blocked level-3 forms.
constexpr int64_t kAppendInvRows = 8;
constexpr int64_t kAppendInvGemm = 256;

// SBO_OPT_INV_LEAVES: the recursion's base cases one dtrtri each where the
// recursion reaches them, all up front in one batched rocSOLVER call, or up
// front by doubling from 128-column blocks (inverse.cpp, "the leaves").
enum class InvLeaves { kOneByOne = 0, kBatched = 1, kDoubling = 2 };

// What the recursion reads from the context, resolved once.
struct InvConfig {
    int64_t base = 2048;    // SBO_OPT_INV_BASE: the base-case size b, a multiple of 128
    int64_t panels = 16;    // SBO_OPT_INV_PANELS: dgemm panels per product
    InvLeaves leaves = InvLeaves::kOneByOne;
    int digits = 0;         // wanted for the sliced products (0: every product a dgemm)
    int64_t oz_min = 4096;  // the smallest split that slices (SBO_OPT_INV_OZ_MIN, resolved from the fit's n)
    bool two_lanes = false; // the top node's halves side by side (aux_ready)
};

// One node of the recursion [A 0; B C]^-1 over columns off .. off + n of the
// matrix: A its first h columns, C the other m = n - h.  h == 0: a base case.
struct InvNode {
    int64_t off = 0, n = 0, h = 0;
    int64_t s_off = -1;     // its S (m x h doubles) in the scratch; -1: a base case
    int slot = 0;           // its first rocSOLVER info slot (a base case's only one)
    bool sliced = false;    // its two products are the int8-sliced GEMM
    int lane = 0;           // which lane inverts it (the top node: lane 0 multiplies)
    int left = -1, right = -1;   // its children A and C in InvPlan::nodes
    size_t ws_bytes = 0;    // sliced: the workspace its larger product needs
    int64_t m() const { return n - h; }
    bool leaf() const { return h == 0; }
};

// The whole tree laid out once (plan_inverse).  Scratch: a node's S first, its
// subtrees' scratch after it -- A's and C's in the same place (C follows A),
// except under a two-lane top node, where C's comes after A's.  Info slots:
// slot 0 for single calls, the base case of block k (columns k b ..) in slot
// k + 1 (one each, so a later success cannot overwrite an earlier singular
// block), one slot per 128-column block of the leaves by doubling from
// info_leaf128 on, info_total in all.
struct InvPlan {
    InvConfig cfg;
    int64_t n = 0, ld = 0;
    std::vector<InvNode> nodes;     // in the recursion's order; nodes[0]: the top
    int64_t scratch = 0;            // doubles the recursion needs
    bool doubling = false;          // the leaves run by doubling ...
    int64_t leaf_scratch = 0;       // ... through this many doubles of scratch
    int64_t info_leaf128 = 0, info_total = 0;
    size_t ws_bytes[2] = {0, 0};    // per lane: the largest need of its sliced nodes
    bool split() const { return !nodes.empty() && !nodes[0].leaf(); }
    bool two_lane_top() const { return cfg.two_lanes && split(); }
    bool sliced() const { return !nodes.empty() && nodes[0].sliced; }
    // the info slots 1 .. half_slots of the top node's first half (A's base cases)
    int half_slots() const { return split() ? nodes[(size_t)nodes[0].right].slot - 1 : 0; }
    int64_t scratch_doubles() const { return scratch > leaf_scratch ? scratch : leaf_scratch; }
};

// The info slots of an n-column inverse: {first 128-column slot, total}.
struct InvInfo {
    int64_t leaf128, total;
};
InvInfo inv_info(int64_t n);

// The plan of the inverse of n columns at leading dimension ld.  Pure: no HIP
// call, no context.
InvPlan plan_inverse(const InvConfig &cfg, int64_t n, int64_t ld);

// A stream, the rocBLAS handle bound to it, and the sliced GEMM's workspace of
// the products that run there (null: this lane never slices).
struct InvLane {
    hipStream_t stream;
    rocblas_handle blas;
    DevBuf *ws;
};

}  // namespace sbo

// The config of this context's fit with `digits` wanted, and of the early half
// beside the Cholesky (dgemm products, base cases one by one, one lane).
sbo::InvConfig inv_config(const sbo_ctx *ctx, int digits);
sbo::InvConfig inv_config_early(const sbo_ctx *ctx);

// Everything a plan's run touches, sized before its first launch (a reserve
// that reallocates later would free memory in use, and waits for the device):
// Linv, the scratch, the info slots and the lanes' workspaces.
sbo_status inverse_reserve(sbo_ctx *ctx, const sbo::InvPlan &plan);

// The run stages.  Each reads the plan and nothing else about the tree.
//   inverse_full:        the whole inverse from the f32 factor (widened here unless it is already)
//   inverse_early_half:  A^-1 and S = B A^-1 of the top node on inv_stream, from the widened left h columns
//   inverse_finish_half: the rest of that plan on `stream`: widen C, C^-1, X21 = -C^-1 S
//   inverse_incremental: the new rows n_old .. n of an append, from the kept inverse
//   inverse_rocsolver:   rocSOLVER's dtrtri on the widened factor (SBO_OPT_INVERSE 0)
sbo_status inverse_full(sbo_ctx *ctx, const sbo::InvPlan &plan, bool widened);
sbo_status inverse_early_half(sbo_ctx *ctx, const sbo::InvPlan &plan);
sbo_status inverse_finish_half(sbo_ctx *ctx, const sbo::InvPlan &plan);
sbo_status inverse_incremental(sbo_ctx *ctx, int64_t n, int64_t ld, int64_t n_old);
sbo_status inverse_rocsolver(sbo_ctx *ctx, int64_t n, int64_t ld);
