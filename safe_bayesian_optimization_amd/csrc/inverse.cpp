// inverse.cpp -- the f64 inverse of the factor: X = L^-1 in place for the
// lower-triangular matrix in ctx->Linv (column-major, its strictly upper part
// zero), by the block recursion
//     [A 0; B C]^-1 = [A^-1 0; -C^-1 B A^-1  C^-1].
// rocSOLVER's dtrtri forms the two products with the triangular inverses as
// full dgemms (2n^3/3 flops at the top of its recursion); here each product
// is a row of dgemms over panels of width nb that leave out the zero part
// of the triangle (n^3/3 + O(n^2 nb) flops):
//     S[:, p] = B[:, p0:h] Ainv[p0:h, p]          (column panels p of A^-1)
//     X21[p, :] = -Cinv[p, 0:p1] S[0:p1, :]       (row panels p of C^-1)
// Each panel's diagonal block is multiplied in full; its strictly upper part
// is zero (widen() writes it, neither rocSOLVER nor this recursion touches
// it).  The first half (A^-1, then S) reads only the factor's left h
// columns, so the fit can run it beside the Cholesky's last steps
// (blocked_potrf, SBO_OPT_INV_OVERLAP); the second half (C^-1, X21) follows
// the factor.
//
// The tree is laid out once by plan_inverse (InvPlan: every node's columns,
// its S in the scratch, its info slot, whether its products slice, its lane);
// three pieces run a node on a lane (invert_subtree, product_s, product_x21),
// and the drivers below are sequences over them.
#include "inverse.hpp"

#include <rocsolver/rocsolver.h>

#include <algorithm>

#include "sbo_host.hpp"

using sbo::InvConfig;
using sbo::InvLane;
using sbo::InvLeaves;
using sbo::InvNode;
using sbo::InvPlan;

// ---- the plan ----

namespace sbo {

// One slot per base case needs ceil(n / b) + 1 <= n/512 + 2 slots at b >= 1024
// (SBO_OPT_INV_BASE's floor); the 128-column blocks of the leaves by doubling
// come after them.
InvInfo inv_info(int64_t n) {
    const int64_t leaf128 = std::max<int64_t>(64, n / 512 + 2);
    return {leaf128, leaf128 + n / 128 + 1};
}

namespace {

// The split lands on a multiple of the base size b (SBO_OPT_INV_BASE, a
// multiple of 128): every base case is then a b x b diagonal block at a
// multiple of b (the last one partial), so all of them can be inverted up
// front in one batched rocSOLVER call (inverse_leaves).
// (SBO_OPT_INV_BASE: the dtrtri base-case size, default 2048, >= 1024 so
// that inv_info holds)
int64_t inverse_split(int64_t n, int64_t b) { return ((n + b - 1) / b + 1) / 2 * b; }

// SBO_OPT_INV_OZ: a level of the recursion whose split is at least
// SBO_OPT_INV_OZ_MIN runs its two products as the sliced GEMM (K <= 16384);
// the levels below keep dgemms.  Automatic (0, default): 2048 in the inverses
// of N >= 12288 (C4: fit 42.0 -> 41.3 ms, profiles/r5_inv_oz_min_gz16.log),
// else 4096 (below that the 2048 level's products are too small to pay for
// their packs, and a sliced inverse brings the guard's check)
bool oz_level(const InvConfig &cfg, int64_t h, int64_t m) {
    return cfg.digits != 0 && h >= cfg.oz_min && h <= 16384 && m <= 16384;
}

// The subtree over columns off .. off + n with its scratch from s_off on;
// returns the doubles of scratch it uses.  side_by_side: the top node of a
// two-lane plan, whose C goes to lane 1 with scratch of its own.
int64_t plan_node(InvPlan &p, int64_t off, int64_t n, int64_t s_off, int lane, bool slicing, bool side_by_side) {
    const int64_t b = p.cfg.base;
    const size_t me = p.nodes.size();
    p.nodes.emplace_back();
    InvNode nd;
    nd.off = off;
    nd.n = n;
    nd.slot = (int)(off / b) + 1;
    nd.lane = lane;
    if (n <= b) {
        p.nodes[me] = nd;
        return 0;
    }
    const int64_t h = inverse_split(n, b), m = n - h;
    nd.h = h;
    nd.s_off = s_off;
    nd.sliced = slicing && oz_level(p.cfg, h, m);
    if (nd.sliced) {
        nd.ws_bytes = std::max(gz_workspace_bytes(m, h, h, p.cfg.digits), gz_workspace_bytes(h, m, m, p.cfg.digits));
        p.ws_bytes[lane] = std::max(p.ws_bytes[lane], nd.ws_bytes);
    }
    nd.left = (int)p.nodes.size();
    const int64_t left = plan_node(p, off, h, s_off + h * m, lane, slicing, false);
    nd.right = (int)p.nodes.size();
    const int64_t right = plan_node(p, off + h, m, s_off + h * m + (side_by_side ? left : 0),
                                    side_by_side ? 1 : lane, slicing, false);
    p.nodes[me] = nd;
    return h * m + (side_by_side ? left + right : std::max(left, right));
}

}  // namespace

// Nothing slices unless two lanes exist, the top node splits and passes
// oz_level (the sliced GEMM's workspaces belong to the two-lane path, and with
// the top split over 16384 it is all dgemm); then every node slices by
// oz_level alone.
InvPlan plan_inverse(const InvConfig &cfg, int64_t n, int64_t ld) {
    InvPlan p;
    p.cfg = cfg;
    p.n = n;
    p.ld = ld;
    const int64_t b = cfg.base;
    const bool splits = n > b;
    const int64_t h = splits ? inverse_split(n, b) : 0;
    const bool slicing = cfg.two_lanes && splits && oz_level(cfg, h, n - h);
    p.scratch = plan_node(p, 0, n, 0, 0, slicing, cfg.two_lanes && splits);
    // the leaves by doubling: with fewer than four full leaves the batches are
    // too small to fill the chip, and rocSOLVER keeps them
    p.doubling = cfg.leaves == InvLeaves::kDoubling && n / b >= 4 && b % 128 == 0 && ((b / 128) & (b / 128 - 1)) == 0;
    p.leaf_scratch = p.doubling ? (n / b) * b * b / 4 : 0;
    const InvInfo info = inv_info(n);
    p.info_leaf128 = info.leaf128;
    p.info_total = info.total;
    return p;
}

}  // namespace sbo

InvConfig inv_config(const sbo_ctx *ctx, int digits) {
    InvConfig c;
    c.base = ctx->opt.inv_base;
    c.panels = ctx->opt.inv_panels;
    c.leaves = !ctx->opt.inv_batched      ? InvLeaves::kOneByOne
               : ctx->opt.inv_leaves_own ? InvLeaves::kDoubling
                                     : InvLeaves::kBatched;
    c.digits = digits;
    c.oz_min = ctx->opt.inv_oz_min > 0 ? ctx->opt.inv_oz_min : (ctx->n >= 12288 ? 2048 : 4096);
    c.two_lanes = aux_ready(ctx);
    return c;
}

InvConfig inv_config_early(const sbo_ctx *ctx) {
    InvConfig c = inv_config(ctx, 0);
    c.leaves = InvLeaves::kOneByOne;
    c.two_lanes = false;
    return c;
}

sbo_status inverse_reserve(sbo_ctx *ctx, const InvPlan &plan) {
    SBO_HIP(ctx->Linv.reserve(sizeof(double) * (size_t)plan.ld * (size_t)plan.ld));
    SBO_HIP(ctx->ws.scratch.reserve(sizeof(double) * (size_t)std::max<int64_t>(plan.scratch_doubles(), 1)));
    SBO_HIP(ctx->info.reserve(sizeof(rocblas_int) * (size_t)plan.info_total));
    // one workspace per lane (SBO_OPT_INV_OZ: the sliced products on the int8
    // matrix cores)
    SBO_HIP(ctx->ws.gzws.reserve(plan.ws_bytes[0]));
    SBO_HIP(ctx->ws.gzws_aux.reserve(plan.ws_bytes[1]));
    return SBO_OK;
}

namespace {

InvLane lane_main(sbo_ctx *ctx) { return {ctx->stream, ctx->blas, &ctx->ws.gzws}; }
InvLane lane_aux(sbo_ctx *ctx) { return {ctx->aux_stream, ctx->blas_aux, &ctx->ws.gzws_aux}; }
InvLane lane_inv(sbo_ctx *ctx) { return {ctx->inv_stream, ctx->blas_inv, nullptr}; }

// ---- the pieces: one node on one lane ----

// dgemm panel width of a product of the recursion at split h: h / panels,
// at least 512 columns -- and at least 1024 for 2048 < h <= 6144, where
// rocBLAS dgemm with ~4096 rows and fewer than 1024 columns at K > 2048 ran
// at half speed (38.5 vs 76.5 TF at 4096 x 512 x 4096 against 4096 x 1024 x
// 4096, tools/r3_dgemm_probe.cpp, profiles/r3_dgemm_probe.log)
// (SBO_OPT_INV_PANELS: the products' panels per half, default 16, at least 512
// columns each: C4 warm fit 58.0 ms at 8 panels, 56.0 at 16; a 256-column
// floor: 59.8 at 16, 68 at 32, profiles/r3_fit_invtune*.log)
int64_t inverse_panel(const InvConfig &cfg, int64_t h) {
    int64_t nb = std::max<int64_t>(512, sbo::round_up(h / cfg.panels, 128));
    if (h > 2048 && h <= 6144) nb = std::max<int64_t>(nb, 1024);
    return nb;
}

// What a node's products read and write: its corner of Linv and its S.
struct NodeView {
    int64_t h, m, ld;
    double *A, *B, *C, *S;
};
NodeView view(const sbo_ctx *ctx, const InvPlan &plan, const InvNode &nd) {
    double *A = ctx->Linv.as<double>() + nd.off * (plan.ld + 1);
    return {nd.h, nd.m(), plan.ld, A, A + nd.h, A + nd.h * (plan.ld + 1), ctx->ws.scratch.as<double>() + nd.s_off};
}

// S = B A^-1 of a node whose A^-1 is done
sbo_status product_s(sbo_ctx *ctx, const InvPlan &plan, int node, const InvLane &lane) {
    const InvNode &nd = plan.nodes[(size_t)node];
    const NodeView v = view(ctx, plan, nd);
    if (nd.sliced) {   // S = L21 A^-1 in one sliced GEMM (A^-1 lower triangular)
        SBO_HIP(sbo::launch_gz_gemm(lane.stream, plan.cfg.digits, v.B, v.ld, v.A, v.ld, v.m, v.h, v.h, 1.0, v.S, v.m,
                                    sbo::kGzTriBLower, lane.ws->as<char>()));
        return SBO_OK;
    }
    SBO_BLAS(rocblas_set_pointer_mode(lane.blas, rocblas_pointer_mode_host));
    const double one = 1.0, zero = 0.0;
    const int64_t nb = inverse_panel(plan.cfg, v.h);
    for (int64_t p0 = 0; p0 < v.h; p0 += nb) {
        const int64_t w = std::min(nb, v.h - p0);
        SBO_BLAS(rocblas_dgemm(lane.blas, rocblas_operation_none, rocblas_operation_none, (rocblas_int)v.m,
                               (rocblas_int)w, (rocblas_int)(v.h - p0), &one, v.B + p0 * v.ld, (rocblas_int)v.ld,
                               v.A + p0 + p0 * v.ld, (rocblas_int)v.ld, &zero, v.S + p0 * v.m, (rocblas_int)v.m));
    }
    return SBO_OK;
}

// X21 = -C^-1 S of a node whose C^-1 and S are done
sbo_status product_x21(sbo_ctx *ctx, const InvPlan &plan, int node, const InvLane &lane) {
    const InvNode &nd = plan.nodes[(size_t)node];
    const NodeView v = view(ctx, plan, nd);
    if (nd.sliced) {
        // X21 = -C^-1 S in one sliced GEMM, as X21^T = -S^T C^-T: the
        // triangular operand then bounds the k loop per column tile, so the
        // workgroups of one column run in step as in S = L21 A^-1 (the direct
        // form, C^-1 as a lower-triangular op(A): 7.4 vs 5.x ms at C4)
        SBO_HIP(sbo::launch_gz_gemm(lane.stream, plan.cfg.digits, v.S, v.m, v.C, v.ld, v.h, v.m, v.m, -1.0, v.B, v.ld,
                                    sbo::kGzTransA | sbo::kGzTransB | sbo::kGzTriBUpper | sbo::kGzTransC,
                                    lane.ws->as<char>()));
        return SBO_OK;
    }
    SBO_BLAS(rocblas_set_pointer_mode(lane.blas, rocblas_pointer_mode_host));
    const double minus_one = -1.0, zero = 0.0;
    const int64_t nb = inverse_panel(plan.cfg, v.h);
    for (int64_t p0 = 0; p0 < v.m; p0 += nb) {
        const int64_t w = std::min(nb, v.m - p0);
        SBO_BLAS(rocblas_dgemm(lane.blas, rocblas_operation_none, rocblas_operation_none, (rocblas_int)w,
                               (rocblas_int)v.h, (rocblas_int)(p0 + w), &minus_one, v.C + p0, (rocblas_int)v.ld, v.S,
                               (rocblas_int)v.m, &zero, v.B + p0, (rocblas_int)v.ld));
    }
    return SBO_OK;
}

// The inverse of a node's whole subtree, in the recursion's order: A^-1, S,
// C^-1, X21.  A base case is one dtrtri with its own info slot -- unless the
// leaves ran up front (inverse_leaves), when base cases are not visited.
sbo_status invert_subtree(sbo_ctx *ctx, const InvPlan &plan, int node, const InvLane &lane) {
    const InvNode &nd = plan.nodes[(size_t)node];
    if (nd.leaf()) {
        SBO_BLAS(rocsolver_dtrtri(lane.blas, rocblas_fill_lower, rocblas_diagonal_non_unit, (rocblas_int)nd.n,
                                  ctx->Linv.as<double>() + nd.off * (plan.ld + 1), (rocblas_int)plan.ld,
                                  ctx->info.as<rocblas_int>() + nd.slot));
        return SBO_OK;
    }
    const bool leaves_done = plan.cfg.leaves != InvLeaves::kOneByOne;
    if (!(leaves_done && plan.nodes[(size_t)nd.left].leaf()))
        if (sbo_status st = invert_subtree(ctx, plan, nd.left, lane)) return st;
    if (sbo_status st = product_s(ctx, plan, node, lane)) return st;
    if (!(leaves_done && plan.nodes[(size_t)nd.right].leaf()))
        if (sbo_status st = invert_subtree(ctx, plan, nd.right, lane)) return st;
    return product_x21(ctx, plan, node, lane);
}

// ---- the leaves ----
//
// Every base case of the recursion -- the b x b diagonal blocks at multiples
// of b = cfg.base, the last one partial -- in one strided-batched rocSOLVER
// dtrtri (+ one call for the partial block), info slots as the plan's (block
// k: slot k + 1).  One at a time inside the recursion each 2048 block took
// ~0.46 ms of mostly idle chip (C4: eight of them;
// profiles/r3_fit_timeline_leaves.txt).
// SBO_OPT_INV_LEAVES 2 (b a power-of-two multiple of 128): the full leaves
// by doubling instead -- every 128-column diagonal block of them in one
// batched dtrtri, then per level s = 128, 256, .., b/2 all the 2s-column
// blocks at once, [A 0; B C]^-1 from A^-1 and C^-1 by two strided-batched
// dgemms through scratch T (T = B A^-1, X21 = -C^-1 T).  From s = 512 up
// each product is two dgemms that leave out the triangular factor's zero
// quarter (3/4 of the flops).  rocSOLVER's batched dtrtri runs its own
// doubling as ~100 launches with a copy of the leaves and mostly small
// tiles (C4: 1.74 ms for 8 leaves of 2048).  Warm fits: C4 29.1 -> 28.4 ms,
// C3 9.7 -> 9.5; with fewer than four leaves the batches are too small to
// fill the chip (C2's one leaf: 2.0 -> 2.3 ms) and rocSOLVER keeps them
// (profiles/r6_inv_leaves_doubling.log).  Scratch: plan.leaf_scratch doubles.
sbo_status leaves_doubling(sbo_ctx *ctx, const InvPlan &plan, rocblas_handle hb, double *Li, double *T) {
    const int64_t n = plan.n, ld = plan.ld, b = plan.cfg.base, nf = n / b, nb128 = nf * b / 128;
    rocblas_int *info128 = ctx->info.as<rocblas_int>() + plan.info_leaf128;
    SBO_BLAS(rocsolver_dtrtri_strided_batched(hb, rocblas_fill_lower, rocblas_diagonal_non_unit, 128, Li,
                                              (rocblas_int)ld, (rocblas_stride)(128 * (ld + 1)), info128,
                                              (rocblas_int)nb128));
    SBO_BLAS(rocblas_set_pointer_mode(hb, rocblas_pointer_mode_host));
    const double one = 1.0, minus_one = -1.0, zero = 0.0;
    const auto N_ = rocblas_operation_none;
    for (int64_t s = 128; s < b; s *= 2) {
        const rocblas_int cnt = (rocblas_int)(nf * b / (2 * s)), is = (rocblas_int)s, il = (rocblas_int)ld;
        const rocblas_stride st = (rocblas_stride)(2 * s * (ld + 1)), sT = (rocblas_stride)(s * s);
        const double *Ainv = Li, *Cinv = Li + s * (ld + 1);
        double *B = Li + s;
        if (s < 512) {
            SBO_BLAS(rocblas_dgemm_strided_batched(hb, N_, N_, is, is, is, &one, B, il, st, Ainv, il, st, &zero, T, is,
                                                   sT, cnt));
            SBO_BLAS(rocblas_dgemm_strided_batched(hb, N_, N_, is, is, is, &minus_one, Cinv, il, st, T, is, sT, &zero,
                                                   B, il, st, cnt));
            continue;
        }
        const int64_t h = s / 2;
        const rocblas_int ih = (rocblas_int)h;
        // T[:, 0:h] = B A^-1[:, 0:h]; T[:, h:s] = B[:, h:s] A^-1[h:s, h:s]
        SBO_BLAS(rocblas_dgemm_strided_batched(hb, N_, N_, is, ih, is, &one, B, il, st, Ainv, il, st, &zero, T, is, sT,
                                               cnt));
        SBO_BLAS(rocblas_dgemm_strided_batched(hb, N_, N_, is, ih, ih, &one, B + h * ld, il, st, Ainv + h * (ld + 1),
                                               il, st, &zero, T + h * s, is, sT, cnt));
        // X21[0:h, :] = -C^-1[0:h, 0:h] T[0:h, :]; X21[h:s, :] = -C^-1[h:s, :] T
        SBO_BLAS(rocblas_dgemm_strided_batched(hb, N_, N_, ih, is, ih, &minus_one, Cinv, il, st, T, is, sT, &zero, B,
                                               il, st, cnt));
        SBO_BLAS(rocblas_dgemm_strided_batched(hb, N_, N_, ih, is, is, &minus_one, Cinv + h, il, st, T, is, sT, &zero,
                                               B + h, il, st, cnt));
    }
    return SBO_OK;
}

sbo_status inverse_leaves(sbo_ctx *ctx, const InvPlan &plan, rocblas_handle hb) {
    const int64_t n = plan.n, ld = plan.ld, b = plan.cfg.base, nf = n / b, r = n - nf * b;
    double *Li = ctx->Linv.as<double>();
    rocblas_int *info = ctx->info.as<rocblas_int>() + 1;
    if (plan.doubling) {
        if (sbo_status st = leaves_doubling(ctx, plan, hb, Li, ctx->ws.scratch.as<double>()); st != SBO_OK) return st;
    } else if (nf > 0)
        SBO_BLAS(rocsolver_dtrtri_strided_batched(hb, rocblas_fill_lower, rocblas_diagonal_non_unit, (rocblas_int)b,
                                                  Li, (rocblas_int)ld, (rocblas_stride)(b * (ld + 1)), info,
                                                  (rocblas_int)nf));
    if (r > 0)
        SBO_BLAS(rocsolver_dtrtri(hb, rocblas_fill_lower, rocblas_diagonal_non_unit, (rocblas_int)r,
                                  Li + nf * b * (ld + 1), (rocblas_int)ld, info + nf));
    return SBO_OK;
}

// ---- the drivers ----

// The top of the recursion with its two independent halves side by side:
// C^-1 on aux_stream (the Cholesky's look-ahead stream and rocBLAS handle,
// idle by now) while `stream` computes A^-1 and S = B A^-1, then X21 once
// both are done.  The lower levels' GEMMs are too small to fill the chip on
// their own.  Enqueue order: A^-1 first, then C^-1, then S -- the host spends
// ~3 ms issuing a half's ~90 rocSOLVER/rocBLAS launches, and C^-1 is needed
// only after S (C4 trace: with C^-1 issued first, `stream` sat idle for
// those 3 ms; profiles/r3_fit_timeline_invorder.txt).
sbo_status inverse_two_lanes(sbo_ctx *ctx, const InvPlan &plan) {
    const InvNode &top = plan.nodes[0];
    const InvLane on_main = lane_main(ctx), on_aux = lane_aux(ctx);
    const bool leaves_done = plan.cfg.leaves != InvLeaves::kOneByOne;
    const auto invert_half = [&](int node, const InvLane &lane) {
        return leaves_done && plan.nodes[(size_t)node].leaf() ? SBO_OK : invert_subtree(ctx, plan, node, lane);
    };
    SBO_HIP(hipEventRecord(ctx->ev_panel, ctx->stream));            // Li widened
    if (sbo_status st = invert_half(top.left, on_main)) return st;
    SBO_HIP(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_panel, 0));
    SBO_BLAS(rocblas_set_pointer_mode(ctx->blas_aux, rocblas_pointer_mode_host));
    if (sbo_status st = invert_half(top.right, on_aux)) {
        (void)hipStreamSynchronize(ctx->aux_stream);
        return st;
    }
    SBO_HIP(hipEventRecord(ctx->ev_trail, ctx->aux_stream));
    if (sbo_status st = product_s(ctx, plan, 0, on_main)) {
        (void)hipStreamSynchronize(ctx->aux_stream);
        return st;
    }
    SBO_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_trail, 0));
    return product_x21(ctx, plan, 0, on_main);
}

}  // namespace

// The library's own recursion (SBO_OPT_INVERSE 1): the factor widened unless
// blocked_potrf did it, the base cases up front (SBO_OPT_INV_LEAVES), then
// the two halves side by side, or the whole tree on `stream` where there is
// one lane or nothing to split.
sbo_status inverse_full(sbo_ctx *ctx, const InvPlan &plan, bool widened) {
    if (!widened)
        SBO_HIP(sbo::launch_widen(ctx->stream, ctx->L.as<float>(), plan.ld, plan.n, plan.n, true,
                                  ctx->Linv.as<double>(), plan.ld));
    const bool leaves_first = plan.cfg.leaves != InvLeaves::kOneByOne;
    if (leaves_first)
        if (sbo_status st = inverse_leaves(ctx, plan, ctx->blas)) return st;
    if (plan.two_lane_top()) return inverse_two_lanes(ctx, plan);
    if (leaves_first && plan.nodes[0].leaf()) return SBO_OK;
    return invert_subtree(ctx, plan, 0, lane_main(ctx));
}

// The left h columns are widened: A^-1 and S = B A^-1 of the top node on
// inv_stream (half the inverse's flops).
sbo_status inverse_early_half(sbo_ctx *ctx, const InvPlan &plan) {
    const InvLane lane = lane_inv(ctx);
    if (sbo_status st = invert_subtree(ctx, plan, plan.nodes[0].left, lane)) return st;
    return product_s(ctx, plan, 0, lane);
}

// The inverse whose first half ran beside the Cholesky (blocked_potrf):
// A^-1 and S = B A^-1 are done: widen the right columns (their rows 0..h-1
// zero), then C^-1 and X21 = -C^-1 S
sbo_status inverse_finish_half(sbo_ctx *ctx, const InvPlan &plan) {
    const int64_t n = plan.n, ld = plan.ld, h = plan.nodes[0].h;
    float *L = ctx->L.as<float>();
    double *Li = ctx->Linv.as<double>();
    SBO_HIP(sbo::launch_widen(ctx->stream, L + h + h * ld, ld, n - h, n - h, true, Li + h + h * ld, ld));
    SBO_HIP(hipMemset2DAsync(Li + h * ld, sizeof(double) * (size_t)ld, 0, sizeof(double) * (size_t)h,
                             (size_t)(n - h), ctx->stream));
    const InvLane lane = lane_main(ctx);
    if (sbo_status st = invert_subtree(ctx, plan, plan.nodes[0].right, lane)) return st;
    return product_x21(ctx, plan, 0, lane);
}

// An append of rows n_old..n-1 to an unchanged leading factor: with the f64
// inverse of the leading block kept from the last refresh, only the new rows
// of L^-1 are computed,
//     [L11  0 ]^-1   [ L11^-1                  0     ]
//     [L21 L22]    = [ -L22^-1 L21 L11^-1   L22^-1 ]
// (one b x b dtrtri and two dtrmm, O(b n^2) instead of O(n^3)).
sbo_status inverse_incremental(sbo_ctx *ctx, int64_t n, int64_t ld, int64_t n_old) {
    const int64_t b = n - n_old;
    float *L = ctx->L.as<float>();
    double *Li = ctx->Linv.as<double>();
    const double one = 1.0, minus_one = -1.0;
    double *T = Li + n_old;                      // rows n_old.., columns 0..n_old-1
    double *L22i = Li + n_old + n_old * ld;      // rows n_old.., columns n_old..
    SBO_HIP(sbo::launch_widen(ctx->stream, L + n_old, ld, b, n_old, false, T, ld));
    SBO_HIP(sbo::launch_widen(ctx->stream, L + n_old + n_old * ld, ld, b, b, true, L22i, ld));
    SBO_BLAS(rocsolver_dtrtri(ctx->blas, rocblas_fill_lower, rocblas_diagonal_non_unit, (rocblas_int)b, L22i,
                              (rocblas_int)ld, ctx->info.as<rocblas_int>()));
    SBO_BLAS(rocblas_set_pointer_mode(ctx->blas, rocblas_pointer_mode_host));
    // S = L21 L11^-1, then T = -L22^-1 S, as two dgemms on the
    // triangles with their zero halves (one f64 MFMA GEMM each:
    // rocBLAS's in-place dtrmm ran as ~200 small launches per append).
    // The strictly upper part of L^-1 is zero: widen() writes it for
    // the initial inverse and for L22^-1, rocSOLVER dtrtri leaves it,
    // and the columns an append adds are zeroed above the new rows here.
    SBO_HIP(hipMemset2DAsync(Li + n_old * ld, sizeof(double) * (size_t)ld, 0, sizeof(double) * (size_t)n_old,
                             (size_t)b, ctx->stream));
    // (sized by the capacity, so that the appends of a streaming loop do not regrow it)
    SBO_HIP(ctx->ws.scratch.reserve(sizeof(double) * (size_t)sbo::round_up(b, 256) * (size_t)ld));
    double *S = ctx->ws.scratch.as<double>();
    const double zero = 0.0;
    if (b <= sbo::kAppendInvRows) {
        // row by row: S[r,:]^T = Li^T T[r,:]^T, one dtrmv over the
        // lower triangle (the dgemm read the whole n_old^2 square)
        for (int64_t r = 0; r < b; ++r) {
            SBO_BLAS(rocblas_dcopy(ctx->blas, (rocblas_int)n_old, T + r, (rocblas_int)ld, S + r, (rocblas_int)b));
            SBO_BLAS(rocblas_dtrmv(ctx->blas, rocblas_fill_lower, rocblas_operation_transpose,
                                   rocblas_diagonal_non_unit, (rocblas_int)n_old, Li, (rocblas_int)ld, S + r,
                                   (rocblas_int)b));
        }
    } else {
        SBO_BLAS(rocblas_dgemm(ctx->blas, rocblas_operation_none, rocblas_operation_none, (rocblas_int)b,
                               (rocblas_int)n_old, (rocblas_int)n_old, &one, T, (rocblas_int)ld, Li,
                               (rocblas_int)ld, &zero, S, (rocblas_int)b));
    }
    SBO_BLAS(rocblas_dgemm(ctx->blas, rocblas_operation_none, rocblas_operation_none, (rocblas_int)b,
                           (rocblas_int)n_old, (rocblas_int)b, &minus_one, L22i, (rocblas_int)ld, S,
                           (rocblas_int)b, &zero, T, (rocblas_int)ld));
    return SBO_OK;
}

// rocSOLVER's dtrtri on the widened factor (SBO_OPT_INVERSE 0)
sbo_status inverse_rocsolver(sbo_ctx *ctx, int64_t n, int64_t ld) {
    double *Li = ctx->Linv.as<double>();
    SBO_HIP(sbo::launch_widen(ctx->stream, ctx->L.as<float>(), ld, n, n, true, Li, ld));
    SBO_BLAS(rocsolver_dtrtri(ctx->blas, rocblas_fill_lower, rocblas_diagonal_non_unit, (rocblas_int)n, Li,
                              (rocblas_int)ld, ctx->info.as<rocblas_int>()));
    return SBO_OK;
}

// The plan of the inverse of n columns as int64 records of kRec values, for
// tests: record 0 the totals {nodes, scratch, leaf_scratch, doubling,
// info_leaf128, info_total, ws_bytes lane 0, ws_bytes lane 1, half_slots,
// two_lane_top, 0, 0}, then one record per node in the recursion's order {off,
// n, h, s_off, slot, sliced, lane, left, right, ws_bytes, 0, 0}.
SBO_API sbo_status sbo_debug_inverse_plan(int64_t n, int64_t ld, int64_t base, int64_t panels, int leaves, int digits,
                                          int64_t oz_min, int lanes, int64_t *out, int64_t cap, int64_t *count) {
    constexpr int64_t kRec = 12;
    if (n < 1 || ld < n || base < 128 || base % 128 != 0 || panels < 1 || leaves < 0 || leaves > 2 || digits < 0 ||
        oz_min < 1 || lanes < 1 || lanes > 2 || cap < 0 || (cap > 0 && !out) || !count)
        return SBO_E_INVAL;
    try {
        InvConfig c;
        c.base = base;
        c.panels = panels;
        c.leaves = (InvLeaves)leaves;
        c.digits = digits;
        c.oz_min = oz_min;
        c.two_lanes = lanes == 2;
        const InvPlan p = sbo::plan_inverse(c, n, ld);
        *count = kRec * (1 + (int64_t)p.nodes.size());
        if (cap < *count) return cap == 0 ? SBO_OK : SBO_E_INVAL;
        std::fill(out, out + *count, (int64_t)0);
        const int64_t head[] = {(int64_t)p.nodes.size(), p.scratch, p.leaf_scratch, p.doubling, p.info_leaf128,
                                p.info_total, (int64_t)p.ws_bytes[0], (int64_t)p.ws_bytes[1], p.half_slots(),
                                p.two_lane_top()};
        std::copy(std::begin(head), std::end(head), out);
        for (size_t i = 0; i < p.nodes.size(); ++i) {
            const InvNode &nd = p.nodes[i];
            const int64_t rec[] = {nd.off, nd.n, nd.h, nd.s_off, nd.slot, nd.sliced, nd.lane, nd.left, nd.right,
                                   (int64_t)nd.ws_bytes};
            std::copy(std::begin(rec), std::end(rec), out + kRec * (int64_t)(1 + i));
        }
    } catch (...) {
        return SBO_E_OOM;
    }
    return SBO_OK;
}
