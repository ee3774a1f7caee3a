// sbo_api.cpp -- the extern "C" entry points of libsbo.so (include/sbo.h).
//
// Host orchestration of the GP mapper (fit / append / predict) and the
// node's acquisition (ComputeSets, grid argmax).  Device work runs on the
// context's stream: HIP kernels (the tick's from kernels.hip, the operand
// build's from operand.hip), rocSOLVER for the factorisation.  No exception crosses the C boundary.
#include <rocsolver/rocsolver.h>

#include <algorithm>
#include <limits>
#include <cstddef>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "inverse.hpp"
#include "remove_map.hpp"
#include "sbo_host.hpp"

using sbo::DevBuf;
using sbo::kAppendInvGemm;
using sbo::kAppendInvRows;

namespace {

constexpr const char *kVersion = "sbo-mi355x 0.1.0";

sbo_status finish(sbo_ctx *ctx, uint32_t flags) {
    if (flags & SBO_ASYNC) return SBO_OK;
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    return SBO_OK;
}

// The guard's policy for the f64 inverse (inverse.cpp runs the inverse itself).
// The digits of the current fit's sliced products (SBO_OPT_INV_OZ_ADAPT:
// chosen per fit by choose_inv_digits; 0 with SBO_OPT_INV_OZ 0)
int inv_digits(const sbo_ctx *ctx) {
    return ctx->opt.inv_oz == 0 ? 0 : ctx->inv_oz_cur > 0 ? ctx->inv_oz_cur : ctx->opt.inv_oz;
}
// SBO_OPT_INV_OZ_ADAPT: the guard's readings of a sliced inverse (its
// effect on the variance and on the mean at 31 queries) grow ~256x per digit
// dropped -- the digits' truncation and the dropped digit products are 2^-8
// coarser each; the variance's measured 200x (C4) to 1000x (lpsc box) from
// six digits to five, tools/r5_inv_adapt.py -- so the last readings at d
// digits predict the next fit's at d' as err 256^(d - d').  The next fit
// takes five digits (never four) only when the prediction of both readings
// for five is within tol / kInvOzPredict, and only for the same
// hyper-parameters, N and training-box area within [0.8, 1.25] of the
// measured fit's.  That fit must then read both within tol / kInvOzReduced
// (a reduced inverse is a speed option, so it must sit well inside the
// bound): otherwise the fit redoes its inverse at SBO_OPT_INV_OZ digits,
// itself guarded, and this data keeps SBO_OPT_INV_OZ digits from then on.
// (Round 5 gated on the variance alone with a 1000x margin, since the mean
// went unwatched: at four digits on C4 it moved 240x the variance reading.)
// Measured (tools/guard_mean.py, profiles/r6_guard_mean.log; readings at
// six -> five -> four digits): C4 variance 1.4e-12 -> 2.5e-10 -> 5.2e-8,
// mean 1.2e-10 -> 2.3e-8 -> 4.4e-6 (the whole-grid mean moved 2.9e-6 at four
// digits: the variance reading alone passed it); the lpsc box 3.2e-9 ->
// 3.2e-6 (variance) and 2.1e-9 -> 9.6e-7 (mean); the mean grows 140-190x per
// digit from six to five on five workloads, the variance 180-1000x.  C4's
// refits take five digits (predicted 3.1e-8, read 2.3e-8 <= 6.25e-8), the
// box stays at six.
constexpr int kInvOzAdaptMin = 5;
constexpr double kInvOzReduced = 8.0;
constexpr double kInvOzPredict = 8.0;
// the fit's data is "the same" as the last guarded fit's: the same
// hyper-parameters, N and the training bounding box's area within [0.8,
// 1.25] of its (so the same density of points per length scale -- what sets
// cond(K) beside the noise; the bench's C4 data and the lpsc box differ 130x)
double bbox_area(const sbo_ctx *ctx) {
    return (double)(ctx->bbox[1] - ctx->bbox[0]) * (double)(ctx->bbox[3] - ctx->bbox[2]);
}
bool inv_same_data(const sbo_ctx *ctx) {
    const sbo_hyper &a = ctx->hyper, &b = ctx->inv_oz_hist_hyper;
    const double ar = bbox_area(ctx), ah = ctx->inv_oz_hist_area;
    return ctx->inv_oz_hist_n > 0 && a.length_scale == b.length_scale && a.sigma_f == b.sigma_f &&
           a.noise_level == b.noise_level && 5 * ctx->n >= 4 * ctx->inv_oz_hist_n &&
           4 * ctx->n <= 5 * ctx->inv_oz_hist_n && ah > 0.0 && 5.0 * ar >= 4.0 * ah && 4.0 * ar <= 5.0 * ah;
}
int choose_inv_digits(const sbo_ctx *ctx) {
#ifdef SBO_DIAG
    // (diagnostic build: SBO_INV_OZ_FORCE = d takes d digits for every fit
    // the pinning allows -- the pinning's test, test_diagnostic_only_variants)
    if (const char *e = getenv("SBO_INV_OZ_FORCE");
        e && ctx->opt.inv_oz_adapt && ctx->opt.inv_check != 0 && ctx->opt.inv_oz != 0 && !(ctx->inv_oz_pinned && inv_same_data(ctx)))
        return std::clamp(atoi(e), 4, ctx->opt.inv_oz);
#endif
    if (!ctx->opt.inv_oz_adapt || ctx->opt.inv_check == 0 || ctx->opt.inv_oz == 0 || ctx->inv_oz_next <= 0 ||
        !inv_same_data(ctx))
        return ctx->opt.inv_oz;
    return std::min(ctx->opt.inv_oz, ctx->inv_oz_next);
}
// the bound a checked inverse must meet on both readings: tol, and tol /
// kInvOzReduced for fewer than SBO_OPT_INV_OZ digits
double inv_check_bar(const sbo_ctx *ctx, const sbo_inv_check &r) {
    return (r.digits > 0 && r.digits < ctx->opt.inv_oz) ? r.tol / kInvOzReduced : r.tol;
}
bool inv_check_passed(const sbo_ctx *ctx, const sbo_inv_check &r) {
    const double bar = inv_check_bar(ctx, r);
    return r.err <= bar && r.err_mean <= bar;   // (NaN fails)
}
// after the guard read a fit's inverse: the next fit's digits
void record_inv_digits(sbo_ctx *ctx, const sbo_inv_check &r) {
    if (!inv_same_data(ctx)) ctx->inv_oz_pinned = false;
    ctx->inv_oz_hist_n = ctx->n;
    ctx->inv_oz_hist_area = bbox_area(ctx);
    ctx->inv_oz_hist_hyper = ctx->hyper;
    ctx->inv_oz_next = 0;
    if (!ctx->opt.inv_oz_adapt || !r.ran || r.digits <= 0) return;
    if (!inv_check_passed(ctx, r)) {
        // fired at reduced digits: this data keeps SBO_OPT_INV_OZ digits from
        // now on (no reduced fit that fires every other time)
        if (r.digits < ctx->opt.inv_oz) ctx->inv_oz_pinned = true;
        return;
    }
    if (ctx->inv_oz_pinned) return;
    const double e = std::max(r.err, r.err_mean);
    int nd = ctx->opt.inv_oz;
    for (int d = kInvOzAdaptMin; d < ctx->opt.inv_oz; ++d)
        if (e * std::ldexp(1.0, 8 * (r.digits - d)) <= r.tol / kInvOzPredict) {
            nd = d;
            break;
        }
    ctx->inv_oz_next = nd;
}

sbo_status check_hyper(sbo_ctx *ctx, const sbo_hyper &h) {
    SBO_CHECK(std::isfinite(h.length_scale) && h.length_scale > 0.0, SBO_E_INVAL,
              "length_scale must be > 0");
    SBO_CHECK(std::isfinite(h.sigma_f) && h.sigma_f > 0.0, SBO_E_INVAL, "sigma_f must be > 0");
    SBO_CHECK(std::isfinite(h.noise_level) && h.noise_level >= 0.0, SBO_E_INVAL,
              "noise_level must be >= 0");
    SBO_CHECK(std::isfinite(h.prior_mean), SBO_E_INVAL, "prior_mean must be finite");
    return SBO_OK;
}

// 32-bit Morton (Z-order) code of a point quantised to 16 bits per axis.
uint32_t morton2(uint32_t a, uint32_t b) {
    auto spread = [](uint32_t v) {
        v &= 0xFFFFu;
        v = (v | (v << 8)) & 0x00FF00FFu;
        v = (v | (v << 4)) & 0x0F0F0F0Fu;
        v = (v | (v << 2)) & 0x33333333u;
        v = (v | (v << 1)) & 0x55555555u;
        return v;
    };
    return spread(a) | (spread(b) << 1);
}

// 32-bit Hilbert index of a point quantised to 16 bits per axis (the
// classic xy -> d walk, one quadrant rotation per level).  Consecutive
// Hilbert indices are always adjacent cells, so 64 consecutive training
// points never straddle a Morton jump: the k-tile bounding boxes are
// tighter and 12 % fewer (k-tile, query block) pairs pass the cutoff at C3
// than with Morton order (counted on the C3 inputs).
uint32_t hilbert2(uint32_t a, uint32_t b) {
    constexpr uint32_t n = 1u << 16;
    uint32_t x = a & (n - 1), y = b & (n - 1), d = 0;
    for (uint32_t s = n >> 1; s > 0; s >>= 1) {
        const uint32_t rx = (x & s) ? 1u : 0u, ry = (y & s) ? 1u : 0u;
        d += s * s * ((3u * rx) ^ ry);
        if (ry == 0) {  // rotate the quadrant (only the bits below s matter from here on)
            if (rx == 1) {
                x = n - 1 - x;
                y = n - 1 - y;
            }
            const uint32_t t = x;
            x = y;
            y = t;
        }
    }
    return d;
}

// k-d order (SBO_OPT_SPATIAL_ORDER 3): recursive bisection of the points
// across the longer side of their box, each cut on a k-tile boundary of the
// stored array (off = the first point's position modulo kBK: an appended
// batch's first leaf fills the partial tile before it) and closest to half,
// down to single k-tiles, each leaf then in caller order (deterministic:
// the comparator is a total order on (coordinate, index), non-finite
// coordinates first).  Its 64-point k-tile boxes are ~16 % smaller in
// semi-perimeter than Hilbert's on scattered points (C4: 2.21 vs 2.65
// length units).  The points are sorted as (x, y, index) records, the two
// halves of the top three levels' cuts on their own threads (disjoint
// ranges: the same order as one thread; C4's 16384 points 2.0 -> 0.6 ms on
// the GPU box's host, part of the fit).
struct KdPoint {
    float x, y;
    int64_t i;
};
void kd_rec(KdPoint *p, int64_t cnt, int64_t off, int par) {
    if (off + cnt <= sbo::kBK) {
        std::sort(p, p + cnt, [](const KdPoint &a, const KdPoint &b) { return a.i < b.i; });
        return;
    }
    float x0 = std::numeric_limits<float>::max(), x1 = -x0, y0 = x0, y1 = -x0;
    for (int64_t i = 0; i < cnt; ++i) {
        x0 = std::min(x0, p[i].x); x1 = std::max(x1, p[i].x);
        y0 = std::min(y0, p[i].y); y1 = std::max(y1, p[i].y);
    }
    // the cut: a tile boundary (off + left a multiple of kBK) closest to half
    int64_t left = (off + cnt / 2 + sbo::kBK / 2) / sbo::kBK * sbo::kBK - off;
    left = std::min(std::max<int64_t>(left, sbo::kBK - off), cnt - 1);
    if ((double)x1 - x0 >= (double)y1 - y0)
        std::nth_element(p, p + left, p + cnt,
                         [](const KdPoint &a, const KdPoint &b) { return a.x < b.x || (a.x == b.x && a.i < b.i); });
    else
        std::nth_element(p, p + left, p + cnt,
                         [](const KdPoint &a, const KdPoint &b) { return a.y < b.y || (a.y == b.y && a.i < b.i); });
    const int64_t off2 = (off + left) % sbo::kBK;
    std::thread t;
    if (par > 0 && cnt >= 4096) {
        try {
            t = std::thread([=] { kd_rec(p, left, off, par - 1); });
        } catch (...) {  // no thread to be had: this one does both halves (same order)
        }
    }
    if (!t.joinable()) kd_rec(p, left, off, 0);
    kd_rec(p + left, cnt - left, off2, t.joinable() ? par - 1 : 0);
    if (t.joinable()) t.join();
}
void kd_order(const std::vector<float> &hx, const std::vector<float> &hy, int64_t *perm, int64_t cnt, int64_t off) {
    auto key = [](float v) { return std::isfinite(v) ? v : -std::numeric_limits<float>::max(); };
    std::vector<KdPoint> p((size_t)cnt);
    for (int64_t i = 0; i < cnt; ++i) p[(size_t)i] = {key(hx[(size_t)perm[i]]), key(hy[(size_t)perm[i]]), perm[i]};
    kd_rec(p.data(), cnt, off, 3);
    for (int64_t i = 0; i < cnt; ++i) perm[i] = p[(size_t)i].i;
}

// Copy `count` measurements into the context's training buffers at `dst`,
// in Hilbert (ctx->opt.spatial_order == 1) or Morton (2) order so that every
// 64-point k-tile is spatially compact and far tiles can be skipped, and
// record the caller's index of each internal row in ctx->order.
sbo_status stage_training(sbo_ctx *ctx, const float *x, const float *y, const float *obs, int64_t count,
                          int64_t dst, int64_t index_base, uint32_t flags) {
    std::vector<float> hx(count), hy(count), ho(count);
    const hipMemcpyKind k = dev(flags) ? hipMemcpyDeviceToHost : hipMemcpyHostToHost;
    SBO_HIP(hipMemcpyAsync(hx.data(), x, sizeof(float) * count, k, ctx->stream));
    SBO_HIP(hipMemcpyAsync(hy.data(), y, sizeof(float) * count, k, ctx->stream));
    SBO_HIP(hipMemcpyAsync(ho.data(), obs, sizeof(float) * count, k, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<int64_t> perm(count);
    for (int64_t i = 0; i < count; ++i) perm[i] = i;
    if (ctx->opt.spatial_order == 3 && count > 1) {
        kd_order(hx, hy, perm.data(), count, dst % sbo::kBK);
    } else if (ctx->opt.spatial_order && count > 1) {
        const auto mx = std::minmax_element(hx.begin(), hx.end());
        const auto my = std::minmax_element(hy.begin(), hy.end());
        const double x0 = *mx.first, sx = std::max(1e-30, (double)*mx.second - x0);
        const double y0 = *my.first, sy = std::max(1e-30, (double)*my.second - y0);
        std::vector<uint32_t> code(count);
        for (int64_t i = 0; i < count; ++i) {
            const double u = std::min(1.0, std::max(0.0, (hx[i] - x0) / sx));
            const double v = std::min(1.0, std::max(0.0, (hy[i] - y0) / sy));
            const uint32_t qu = (uint32_t)(u * 65535.0), qv = (uint32_t)(v * 65535.0);
            code[i] = !(std::isfinite(u) && std::isfinite(v)) ? 0
                      : ctx->opt.spatial_order == 2                ? morton2(qu, qv)
                                                               : hilbert2(qu, qv);
        }
        std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return code[a] < code[b]; });
    }
    std::vector<float> px(count), py(count), po(count);
    for (int64_t i = 0; i < count; ++i) {
        px[i] = hx[perm[i]];
        py[i] = hy[perm[i]];
        po[i] = ho[perm[i]];
    }
    SBO_HIP(hipMemcpyAsync(ctx->x.as<float>() + dst, px.data(), sizeof(float) * count, hipMemcpyHostToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(ctx->y.as<float>() + dst, py.data(), sizeof(float) * count, hipMemcpyHostToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(ctx->obs.as<float>() + dst, po.data(), sizeof(float) * count, hipMemcpyHostToDevice, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    ctx->order.resize((size_t)dst);
    for (int64_t i = 0; i < count; ++i) ctx->order.push_back(index_base + perm[i]);
    // running bounding box of all training points (query Morton frame)
    const auto mx = std::minmax_element(hx.begin(), hx.end());
    const auto my = std::minmax_element(hy.begin(), hy.end());
    if (dst == 0) {
        ctx->bbox[0] = *mx.first; ctx->bbox[1] = *mx.second;
        ctx->bbox[2] = *my.first; ctx->bbox[3] = *my.second;
    } else {
        ctx->bbox[0] = std::min(ctx->bbox[0], *mx.first); ctx->bbox[1] = std::max(ctx->bbox[1], *mx.second);
        ctx->bbox[2] = std::min(ctx->bbox[2], *my.first); ctx->bbox[3] = std::max(ctx->bbox[3], *my.second);
    }
    return SBO_OK;
}

void recycle_events(sbo_ctx *ctx) {
    for (auto *l : {&ctx->ev_predict, &ctx->ev_fill}) {
        for (auto &p : *l) {
            ctx->ev_pool.push_back(p.first);
            ctx->ev_pool.push_back(p.second);
        }
        l->clear();
    }
}

// Grow a device buffer to `bytes`, keeping its first `keep` bytes.
hipError_t grow_keep(sbo_ctx *ctx, DevBuf &buf, size_t bytes, size_t keep) {
    if (bytes <= buf.capacity()) return hipSuccess;
    DevBuf nb;
    hipError_t e = nb.reserve(bytes);
    if (e != hipSuccess) return e;
    if (keep) {
        e = hipMemcpyAsync(nb.as<void>(), buf.as<void>(), keep, hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) return e;
        e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return e;
    }
    buf.swap(nb);
    return hipSuccess;
}

// ------------------------------------------------------------ tick pipeline
// What a tick is asked for: the plan alone (sbo_debug_plan), the plan and its
// per-query cost (sbo_query_cost), or plan, sweep and acquisition.
enum class TickWant { kPlan, kCost, kTick };
// Which sweep: the context's (ctx->precise), the fast sweep, the precise
// sweep under its budget, or the precise sweep under a budget of
// 2^-kProbeRefBits of the probe's largest variance (the probe's reference).
enum class Sweep { kCtx, kFast, kPrecise, kProbeRef };
// The sweep order of one query set, as an earlier tick of the same queries
// returned it (TickPlan::perm, qx, qy: pointers into qwork, valid while qwork
// is untouched).  Empty: the tick orders the queries itself.
struct QueryOrder {
    const int32_t *perm = nullptr;
    const float *sx = nullptr, *sy = nullptr;
};
// One tick over m queries on the device.  Outputs not wanted stay null; key
// null leaves the argmax key behind the block keys in ctx->keys.
struct TickRequest {
    const float *qx = nullptr, *qy = nullptr;
    int64_t m = 0;
    double beta = 0.0, f_min = 0.0;
    int score = SBO_SCORE_WIDTH;
    int64_t index_offset = 0;
    float *mu = nullptr, *sd = nullptr;
    double *lo = nullptr, *hi = nullptr;
    uint8_t *safe = nullptr;
    sbo_key *key = nullptr;
    float *cost = nullptr;       // kCost: the per-query cost, in the caller's order
    TickWant want = TickWant::kTick;
    Sweep sweep = Sweep::kCtx;
    QueryOrder order;
    bool quiet = false;          // no profile events, no counters (the probe is not a tick)
    bool keep = false;           // sbo_tick_stream's full path: capture the posterior into ctx->keep
};
// What SBO_OPT_PRECISE_KERNEL's value selects: the operand's layout (0 f64
// tiles, 1 int8 digit tiles, 2 int8 with exponents shared by k-tile pairs),
// the int8 sweep, its K* table (the chunked tick), the pair exponents.
struct PreciseKernel {
    int layout;
    bool int8, table, pairs;
};
PreciseKernel precise_kernel_traits(int k) {
    const bool pairs = k == 4 || k == 10;
    return {k == 0 ? 0 : pairs ? 2 : 1, k >= 1, k >= 3 && k != 9, pairs};
}
// Everything a tick's stages read, computed once from (ctx, request) by
// tick_plan; tick_order_queries fills the second half.  A plan-only or cost
// request keeps its items row-block-major (the cost kernel and sbo_debug_plan
// index them so), is never chunked and counts nothing.
struct TickPlan {
    int64_t nI = 0;              // row blocks
    int P = 0;                   // sweep workgroups
    bool precise = false;
    PreciseKernel pk{};
    bool chunked = false;        // the K* table's sweep: each chunk of query blocks plans itself
    bool prof = false;           // record events and counters where sbo_profile is on
    sbo::SkipPlan skip;
    // the queries in sweep order: ms positions (>= m: padded patches), nQ
    // query blocks, partials' leading dimension; perm null: the caller's order
    int64_t ms = 0, nQ = 0, ldp = 0;
    const int32_t *perm = nullptr;
    const float *qx = nullptr, *qy = nullptr;
};
}  // namespace

// ---- the split operand (SplitOperand, sbo_ctx.hpp)
sbo_status SplitOperand::reserve(sbo_ctx *ctx, int64_t npad, int layout) {
    const int64_t I0 = std::min(st_.start(layout), npad / sbo::kBM);
    SBO_HIP(grow_keep(ctx, ax3, sbo::x3_operand_bytes(npad), sbo::x3_operand_bytes(I0 * sbo::kBM)));
    SBO_HIP(kc3.reserve(sbo::x3_coord_bytes(npad)));
    return SBO_OK;
}
sbo_status SplitOperand::update(sbo_ctx *ctx, int64_t npad, int layout, hipStream_t planes, bool coords) {
    if (st_.current(npad / sbo::kBM, layout)) return SBO_OK;
    if (sbo_status st = reserve(ctx, npad, layout)) return st;
    SBO_HIP(sbo::launch_pack_x3(planes, ctx->aug.as<float>(), coords ? ctx->kcoord.as<float>() : nullptr, npad,
                                st_.start(layout), layout, ax3.as<char>(), coords ? kc3.as<float>() : nullptr));
    st_.mark(layout);
    return SBO_OK;
}
sbo_status SplitOperand::pack_coords(sbo_ctx *ctx, int64_t npad, hipStream_t s) {
    SBO_HIP(sbo::launch_pack_x3(s, nullptr, ctx->kcoord.as<float>(), npad, 0, 0, nullptr, kc3.as<float>()));
    return SBO_OK;
}
namespace {
// The split operand of the current kernel variant's layout, up to date on
// ctx->stream (the tick's lazy derivation, sbo_debug_x3_operand).
sbo_status derive_x3(sbo_ctx *ctx) {
    return ctx->split.update(ctx, ctx->npad, sbo::x3_layout(ctx->opt.kernel_variant), ctx->stream, true);
}

sbo_status run_tick(sbo_ctx *ctx, const TickRequest &rq, TickPlan *plan_out = nullptr);
sbo_status probe_precision(sbo_ctx *ctx, int precision);
// the precision probe runs on this refresh (probe_precision): on a fresh fit,
// and on appends once N has grown by SBO_OPT_REPROBE percent (default 25)
// since the last probe -- or shrunk by as much (sbo_remove)
bool probe_due(const sbo_ctx *ctx) {
    return ctx->probe_n == 0 ||
           std::llabs((long long)(ctx->n - ctx->probe_n)) * 100 >= ctx->probe_n * (int64_t)ctx->opt.reprobe_pct;
}

// Wait (host) for an accuracy guard still running on chk_stream: it reads L,
// L^-1, x/y/obs and ctx->ws.chk, so whoever abandons a refresh waits for it
// before those buffers are regrown, freed or rewritten.
void drain_guard(sbo_ctx *ctx) {
    if (ctx->chk_stream) (void)hipStreamSynchronize(ctx->chk_stream);
}

// The context out of the fitted state, every buffer keeping its capacity: no
// model, nothing derived from one, no guard in flight.  The one list of what
// "fitted" stands on; the digit adaptation's history across fits
// (inv_oz_next, inv_oz_hist_*, inv_oz_pinned) is not part of it.
void unfit(sbo_ctx *ctx) {
    ++ctx->fit_epoch;   // (whatever follows is another model: a kept posterior is not updated into it)
    ctx->fitted = false;
    ctx->has_factor = false;
    ctx->n = 0;
    ctx->linv_n = 0;
    ctx->z_n = 0;
    ctx->probe_n = 0;
    ctx->precise = false;
    ctx->n_sorted = 0;
    ctx->removed_since_sort = 0;
    ctx->order.clear();
    ctx->chk_res = sbo_inv_check{};
    ctx->split.all_changed();
    ctx->pop.all_changed();
    drain_guard(ctx);
}

// The one commit point of the calls that rebuild the model (sbo_fit,
// sbo_append, sbo_import_state), armed once their arguments are accepted and
// the precise operand's pack is drained.  From then on the context counts as
// fitted only through commit(): every other way out -- an error return of any
// stage, the probe and the guard's reading included -- is unfit(), so that it
// accepts a new sbo_fit, an import or option calls and nothing else.
struct FitCommit {
    sbo_ctx *ctx;
    bool committed = false;
    explicit FitCommit(sbo_ctx *c) : ctx(c) {}
    sbo_status commit(sbo_status st) {
        if (st != SBO_OK) return st;
        ctx->fitted = true;
        committed = true;
        return SBO_OK;
    }
    ~FitCommit() {
        if (!committed) unfit(ctx);
    }
};

}  // namespace

// ---- the precise operand (PreciseOperand, sbo_ctx.hpp)
sbo_status PreciseOperand::drain(sbo_ctx *ctx) {
    if (pending_) {
        SBO_HIP(hipEventSynchronize(ev));
        pending_ = false;
    }
    return SBO_OK;
}
sbo_status PreciseOperand::wait_on(sbo_ctx *ctx, hipStream_t s) const {
    if (pending_) SBO_HIP(hipStreamWaitEvent(s, ev, 0));
    return SBO_OK;
}
// The buffers for npad rows, keeping the row blocks below the first stale one
// (grow_keep copies on `stream` and waits for it: the fit reserves them
// before it forks work onto aux_stream, so that the fork is not serialised).
sbo_status PreciseOperand::reserve(sbo_ctx *ctx, int64_t npad) {
    if (sbo_status st = drain(ctx)) return st;
    const PreciseKernel pk = precise_kernel_traits(ctx->opt.precise_kernel);
    const int64_t I0 = std::min(st_.start(pk.layout), npad / sbo::kBM);
    if (pk.int8) {
        SBO_HIP(grow_keep(ctx, aoz, sbo::oz_operand_bytes(npad), sbo::oz_operand_bytes(I0 * sbo::kBM)));
        SBO_HIP(grow_keep(ctx, eoz, sbo::oz_exp_bytes(npad), sbo::oz_exp_bytes(I0 * sbo::kBM)));
        SBO_HIP(koz.reserve(sbo::oz_coord_bytes(npad)));
    } else {
        SBO_HIP(grow_keep(ctx, a64, sbo::f64_operand_bytes(npad), sbo::f64_operand_bytes(I0 * sbo::kBM)));
        SBO_HIP(kc64.reserve(sbo::f64_coord_bytes(npad)));
    }
    return SBO_OK;
}
// The operand of SBO_OPT_PRECISE_KERNEL's layout (f64 tiles or int8 digit
// tiles) for npad rows from the first stale row block on, from the f64
// inverse and alpha64, on stream s; a pack on another stream than `stream`
// stays in flight (wait_on, drain).
sbo_status PreciseOperand::update(sbo_ctx *ctx, int64_t npad, hipStream_t s) {
    const PreciseKernel pk = precise_kernel_traits(ctx->opt.precise_kernel);
    if (st_.current(npad / sbo::kBM, pk.layout)) return SBO_OK;
    if (sbo_status st = reserve(ctx, npad)) return st;
    const int64_t I0 = st_.start(pk.layout);
    const double sf2 = ctx->hyper.sigma_f * ctx->hyper.sigma_f;
    if (pk.int8) {
        SBO_HIP(sbo::launch_pack_oz(s, ctx->Linv.as<double>(), ctx->cap, ctx->n, npad, I0, sf2, ctx->x.as<float>(),
                                    ctx->y.as<float>(), ctx->alpha64.as<double>(), aoz.as<char>(), eoz.as<int>(),
                                    koz.as<char>(), pk.pairs));
    } else {
        SBO_HIP(sbo::launch_pack_f64(s, ctx->Linv.as<double>(), ctx->cap, ctx->n, npad, I0, sf2, ctx->x.as<float>(),
                                     ctx->y.as<float>(), ctx->alpha64.as<double>(), a64.as<double>(),
                                     kc64.as<double>()));
    }
    st_.mark(pk.layout);
    if (s != ctx->stream) {
        SBO_HIP(hipEventRecord(ev, s));
        pending_ = true;
    }
    return SBO_OK;
}

namespace {
// The inverse's accuracy guard (SBO_OPT_INV_CHECK; inv_check.hip).  Launch:
// on chk_stream once `stream` has finished the inverse, beside the operand
// packs that follow it (it only reads L, L^-1 and the observations).  The
// guard set: a 4 x 4 lattice over the training box (its corners included:
// the largest variances, which the contract normalises by) and kChkTrain
// training locations, every (n / kChkTrain)-th stored point (the k-d order
// spreads them over the data in proportion to its density; where the data
// is dense the variance is smallest and sf2 - |V|^2 cancels hardest, and the
// mean is largest); the last right-hand side is the residual (the mean's
// reading).
// kInvCheckTol = 5e-7: a twentieth of the 1e-5 contract -- the inverse's share
// adds to the sweeps' own errors, which the probe holds to 5e-6 x the largest
// whole-grid / probe ratio measured.
constexpr int kChkGrid = 4, kChkQueries = sbo::kChkQ - 1, kChkTrain = kChkQueries - kChkGrid * kChkGrid;
constexpr double kInvCheckTol = 5e-7;
// The two ingredients the guard's and the probe's query sets share: a g x g
// lattice over the training box, corners included (x at hx[i g + j], y at
// hy[i g + j]), and every stride-th stored point from stride / 2 on (count of
// them, a strided 2-D copy on stream s).
void bbox_lattice(const float bbox[4], int g, float *hx, float *hy) {
    for (int i = 0; i < g; ++i)
        for (int j = 0; j < g; ++j) {
            hx[i * g + j] = bbox[0] + (bbox[1] - bbox[0]) * (float)j / (float)(g - 1);
            hy[i * g + j] = bbox[2] + (bbox[3] - bbox[2]) * (float)i / (float)(g - 1);
        }
}
sbo_status copy_strided_points(sbo_ctx *ctx, hipStream_t s, int64_t stride, int64_t count, float *qx, float *qy) {
    SBO_HIP(hipMemcpy2DAsync(qx, sizeof(float), ctx->x.as<float>() + stride / 2, sizeof(float) * stride,
                             sizeof(float), (size_t)count, hipMemcpyDeviceToDevice, s));
    SBO_HIP(hipMemcpy2DAsync(qy, sizeof(float), ctx->y.as<float>() + stride / 2, sizeof(float) * stride,
                             sizeof(float), (size_t)count, hipMemcpyDeviceToDevice, s));
    return SBO_OK;
}
sbo_status inverse_check_launch(sbo_ctx *ctx) {
    const int64_t n = ctx->n;
    if (!ctx->chk_stream) {
        SBO_HIP(hipStreamCreateWithFlags(&ctx->chk_stream, hipStreamNonBlocking));
        SBO_HIP(hipEventCreate(&ctx->ev_chk0));
        SBO_HIP(hipEventCreate(&ctx->ev_chk1));
    }
    SBO_HIP(ctx->ws.chk.reserve(sbo::inv_check_bytes(n)));
    float *q = nullptr;
    double *cs = nullptr;
    SBO_HIP(sbo::launch_inv_check(ctx->chk_stream, nullptr, nullptr, 0, n, nullptr, nullptr, nullptr, 0.0, 0.0,
                                  0.0, ctx->ws.chk.as<void>(), &q, &cs));
    static thread_local std::vector<float> hq;   // (lives until the copy below has run)
    hq.assign(2 * kChkGrid * kChkGrid, 0.0f);
    bbox_lattice(ctx->bbox, kChkGrid, hq.data(), hq.data() + kChkGrid * kChkGrid);
    SBO_HIP(hipEventRecord(ctx->ev_panel, ctx->stream));   // the inverse is done
    SBO_HIP(hipStreamWaitEvent(ctx->chk_stream, ctx->ev_panel, 0));
    SBO_HIP(hipEventRecord(ctx->ev_chk0, ctx->chk_stream));
    constexpr int G = kChkGrid * kChkGrid, Q = sbo::kChkQ;
    SBO_HIP(hipMemcpyAsync(q, hq.data(), sizeof(float) * G, hipMemcpyHostToDevice, ctx->chk_stream));
    SBO_HIP(hipMemcpyAsync(q + Q, hq.data() + G, sizeof(float) * G, hipMemcpyHostToDevice, ctx->chk_stream));
    // training locations: every stride-th stored point (n > kChkTrain here;
    // fewer points repeat the last one)
    const int64_t stride = std::max<int64_t>(1, n / kChkTrain);
    const int64_t mt = std::min<int64_t>(kChkTrain, (n - stride / 2 + stride - 1) / stride);
    if (sbo_status st = copy_strided_points(ctx, ctx->chk_stream, stride, mt, q + G, q + Q + G)) return st;
    for (int64_t c = G + mt; c < kChkQueries; ++c) {
        SBO_HIP(hipMemcpyAsync(q + c, q + G + mt - 1, sizeof(float), hipMemcpyDeviceToDevice, ctx->chk_stream));
        SBO_HIP(hipMemcpyAsync(q + Q + c, q + Q + G + mt - 1, sizeof(float), hipMemcpyDeviceToDevice,
                               ctx->chk_stream));
    }
    const double sf2 = ctx->hyper.sigma_f * ctx->hyper.sigma_f;
    SBO_HIP(sbo::launch_inv_check(ctx->chk_stream, ctx->Linv.as<double>(), ctx->L.as<float>(), ctx->cap, n,
                                  ctx->x.as<float>(), ctx->y.as<float>(), ctx->obs.as<float>(),
                                  ctx->hyper.prior_mean, sf2, ctx->hyper.length_scale, ctx->ws.chk.as<void>(), nullptr,
                                  nullptr));
    SBO_HIP(hipEventRecord(ctx->ev_chk1, ctx->chk_stream));
    return SBO_OK;
}
// Wait for the launched check and fill r (err, err_grid, err_train, var_max,
// err_mean, mean_max, ms).
sbo_status inverse_check_read(sbo_ctx *ctx, sbo_inv_check &r) {
    float *q = nullptr;
    double *cs = nullptr;
    SBO_HIP(sbo::launch_inv_check(ctx->chk_stream, nullptr, nullptr, 0, ctx->n, nullptr, nullptr, nullptr, 0.0, 0.0,
                                  0.0, ctx->ws.chk.as<void>(), &q, &cs));
    constexpr int G = kChkGrid * kChkGrid, Q = kChkQueries;
    double h[4 * Q];
    SBO_HIP(hipMemcpyAsync(h, cs, sizeof(h), hipMemcpyDeviceToHost, ctx->chk_stream));
    SBO_HIP(hipStreamSynchronize(ctx->chk_stream));
    float ms = 0.0f;
    SBO_HIP(hipEventElapsedTime(&ms, ctx->ev_chk0, ctx->ev_chk1));
    const double sf2 = ctx->hyper.sigma_f * ctx->hyper.sigma_f, m0 = ctx->hyper.prior_mean;
    double dmax[2] = {0.0, 0.0}, vmax[2] = {0.0, 0.0}, dmu = 0.0, mumax = 0.0;
    bool finite = true;
    for (int c = 0; c < Q; ++c) {
        const double *e = h + 4 * c;
        const int part = c < G ? 0 : 1;
        finite = finite && std::isfinite(e[0]) && std::isfinite(e[1]) && std::isfinite(e[2]) && std::isfinite(e[3]);
        dmax[part] = std::max(dmax[part], std::fabs(e[0]));        // |d var| = ||V1|^2 - |V0|^2|
        vmax[part] = std::max(vmax[part], sf2 - e[1]);              // var from the refined V1
        dmu = std::max(dmu, std::fabs(e[3]));                       // |d mu| = |V1^T z1 - V0^T z0|
        mumax = std::max(mumax, std::fabs(m0 + e[2] + e[3]));       // mu from the refined V1, z1
    }
    auto rel = [](double d, double v) { return v > 0.0 ? d / v : (d > 0.0 ? HUGE_VAL : 0.0); };
    r.ran = 1;
    r.m = Q;
    r.err_mean = finite ? rel(dmu, mumax) : HUGE_VAL;
    r.mean_max = mumax;
    r.err = finite ? rel(std::max(dmax[0], dmax[1]), std::max(vmax[0], vmax[1])) : HUGE_VAL;
    r.err_grid = finite ? rel(dmax[0], vmax[0]) : HUGE_VAL;
    r.err_train = finite ? rel(dmax[1], vmax[1]) : HUGE_VAL;
    r.var_max = std::max(vmax[0], vmax[1]);
    r.tol = kInvCheckTol;
    r.ms = ms;
    return SBO_OK;
}

// What blocked_potrf hands to the refresh of the factor it just wrote.
struct FactorHandover {
    int64_t widened_n = 0;   // the factor (n columns) is already widened into Linv
    int64_t half_n = 0;      // n of a factor whose inverse's first half is done (inverse_finish_half ends it) ...
    sbo::InvPlan half;       // ... by this plan: its layout, its reservation, the info slots that half used
    rocblas_int *info = nullptr;   // the info slots the factorization wrote (slot 0: the leading minor)
};

// The guard's ladder (refresh_operand): the digits chosen for this fit, then
// SBO_OPT_INV_OZ digits, then dgemm products.
enum InvAttempt { kInvChosen, kInvFullDigits, kInvDgemm };

// Everything one refresh decides, once, before its first launch: the stages
// below read it and none of them looks the conditions up again.
struct RefreshPlan {
    int64_t n, ld, npad, nI;
    double sf2;
    bool f64;            // SBO_OPT_INVERSE_BITS 64 (else the f32 strtri path, refresh_f32)
    bool incr;           // an append with the leading block's f64 inverse kept: only rows n_old.. are new
    bool removed;        // sbo_remove's rotations: rows from first_row on changed, the f64 inverse is already current, n went down
    int64_t n_old, I0;   // (I0: first row block holding new or changed rows)
    size_t old_tiles;    // packed tiles of the row blocks below I0, kept
    bool half_done;      // the inverse's first half ran beside the Cholesky (blocked_potrf) ...
    int half_slots;      // ... its info slots 1 .. half_slots stay, the rest are cleared
    sbo::InvPlan inv;    // the recursion's plan (half_done: the one that half ran by; empty: no recursion)
    int64_t info_slots;  // the rocSOLVER info slots of an n-column refresh
    bool widened;        // the factor is already widened into Linv
    int digits;          // of this inverse's sliced products (0: dgemm)
    bool guard;          // the accuracy guard runs on this inverse
    bool inc_alpha;      // alpha updated from the kept z instead of solved in full
    bool aux;            // alpha and the derived operands go to aux_stream
    bool eager_x3, eager_f64;   // the derived operands brought up to date on aux_stream beside the packs
    int x3_layout;
};
RefreshPlan plan_refresh(const sbo_ctx *ctx, int64_t n_old, const FactorHandover &ho, InvAttempt attempt,
                         int64_t removed_from = -1) {
    const sbo_options &o = ctx->opt;
    RefreshPlan p{};
    p.n = ctx->n;
    p.ld = ctx->cap;
    p.npad = sbo::round_up(p.n, sbo::kBM);
    p.nI = p.npad / sbo::kBM;
    p.sf2 = ctx->hyper.sigma_f * ctx->hyper.sigma_f;
    p.f64 = o.inverse_bits == 64;
    p.incr = n_old > 0 && inverse_current(ctx, n_old) && ctx->npad > 0;
    p.removed = removed_from >= 0 && n_old == 0 && inverse_current(ctx, p.n) && ctx->npad > 0;
    p.n_old = p.incr ? n_old : 0;
    // (a removal that ends on a row block's edge still repacks the last block: no stage meets an empty range)
    p.I0 = p.removed ? std::min(removed_from / sbo::kBM, p.nI - 1) : p.n_old / sbo::kBM;
    p.old_tiles = (size_t)sbo::total_tiles(p.I0);
    p.half_done = p.f64 && o.inverse_rec && !p.incr && !p.removed && ho.half_n == p.n;
    p.widened = ho.widened_n == p.n;
    const int want = attempt == kInvDgemm ? 0 : attempt == kInvFullDigits ? o.inv_oz : inv_digits(ctx);
    if (p.half_done)
        p.inv = ho.half;
    else if (p.f64 && !p.incr && !p.removed && o.inverse_rec)
        p.inv = sbo::plan_inverse(inv_config(ctx, want), p.n, p.ld);
    p.half_slots = p.half_done ? p.inv.half_slots() : 0;
    p.info_slots = sbo::inv_info(p.n).total;
    const bool sliced = p.inv.sliced();
    p.digits = sliced ? want : 0;
    p.guard = p.f64 && !p.incr && !p.removed &&
              (o.inv_check == 2 || attempt == kInvDgemm || (o.inv_check == 1 && sliced));
    p.inc_alpha = p.incr && ctx->z_n == n_old && p.n - n_old <= kAppendInvGemm;
    p.aux = p.f64 && aux_ready(ctx);
    p.eager_x3 = p.aux && o.kernel_variant >= 2;
    p.eager_f64 =
        p.aux && o.precision_opt != 0 && (probe_due(ctx) || ctx->precise || o.precision_opt == 1);
    p.x3_layout = sbo::x3_layout(o.kernel_variant);
    return p;
}

// The buffers every refresh writes, and the rocSOLVER info slots cleared (a
// first half that ran beside the Cholesky keeps its own).
sbo_status refresh_begin(sbo_ctx *ctx, const RefreshPlan &p) {
    const int64_t nslots = p.info_slots;
    SBO_HIP(ctx->info.reserve(sizeof(rocblas_int) * (size_t)nslots));
    rocblas_int *info = ctx->info.as<rocblas_int>();
    SBO_HIP(grow_keep(ctx, ctx->aug, sizeof(float) * (size_t)sbo::total_tiles(p.nI) * sbo::kTileFloats,
                      sizeof(float) * p.old_tiles * sbo::kTileFloats));
    SBO_HIP(ctx->kcoord.reserve(sizeof(float) * (size_t)(p.npad / sbo::kBK) * 3 * sbo::kBK));
    if (p.half_done) {
        SBO_HIP(hipMemsetAsync(info, 0, sizeof(rocblas_int), ctx->stream));
        SBO_HIP(hipMemsetAsync(info + 1 + p.half_slots, 0, sizeof(rocblas_int) * (size_t)(nslots - 1 - p.half_slots),
                               ctx->stream));
    } else {
        SBO_HIP(hipMemsetAsync(info, 0, sizeof(rocblas_int) * (size_t)nslots, ctx->stream));
    }
    return SBO_OK;
}

// L^-1 (lower, non-unit) in f64: widen L and invert (f64 MFMA), then round
// sf2 * L^-1 to f32 once while packing -- the f32 strtri path adds its own
// inversion error on top of the f32 representation error
// (SBO_OPT_INVERSE_BITS = 32 selects it, refresh_f32).
sbo_status refresh_inverse(sbo_ctx *ctx, const RefreshPlan &p) {
    sbo_status st;
    if (p.incr) {
        st = inverse_incremental(ctx, p.n, p.ld, p.n_old);
    } else if (!p.inv.nodes.empty()) {
        if (sbo_status sr = inverse_reserve(ctx, p.inv)) return sr;
        st = p.half_done ? inverse_finish_half(ctx, p.inv) : inverse_full(ctx, p.inv, p.widened);
    } else {
        SBO_HIP(ctx->Linv.reserve(sizeof(double) * (size_t)p.ld * (size_t)p.ld));
        st = inverse_rocsolver(ctx, p.n, p.ld);
    }
    if (st != SBO_OK) return st;
    ctx->linv_n = p.n;
    return SBO_OK;
}

// the inverse's accuracy guard, on its own stream beside what follows
sbo_status refresh_guard_launch(sbo_ctx *ctx, const RefreshPlan &p) {
    if (p.incr || p.removed) return SBO_OK;
    ctx->chk_res = sbo_inv_check{};
    if (!p.guard) return SBO_OK;
    ctx->chk_res.digits = p.digits;
    return inverse_check_launch(ctx);
}

// alpha = K^-1 (y - m0) = L^-T L^-1 (y - m0), in f64 from the f64
// inverse: two triangular matrix-vector products (bandwidth-bound and
// parallel, unlike the two sequential triangular solves of spotrs),
// into alpha64 (the precise sweep's mean uses alpha in f64).  They
// only feed the coordinate pack: on aux_stream (blas_aux) beside the
// operand pack, row sums and tile norms, which read only L^-1 (C4:
// 0.75 ms off the fit's critical path).
// An append of a few points updates alpha instead (z = L^-1 r kept from
// the last refresh): z's new entries are the inverse's new rows times
// r, and alpha += (new rows)^T z_new over all n -- two dgemv over b
// rows instead of two passes over the whole triangle (0.8 ms at C4).
sbo_status refresh_alpha(sbo_ctx *ctx, const RefreshPlan &p) {
    const int64_t n = p.n, ld = p.ld, n_old = p.n_old;
    double *Li = ctx->Linv.as<double>();
    SBO_HIP(grow_keep(ctx, ctx->alpha64, sizeof(double) * (size_t)std::max(p.npad, ld),
                      p.inc_alpha ? sizeof(double) * (size_t)n_old : 0));
    SBO_HIP(grow_keep(ctx, ctx->zvec, sizeof(double) * (size_t)std::max(p.npad, ld),
                      p.inc_alpha ? sizeof(double) * (size_t)n_old : 0));
    ctx->z_n = 0;
    double *d = ctx->alpha64.as<double>(), *zv = ctx->zvec.as<double>();
    hipStream_t sa = p.aux ? ctx->aux_stream : ctx->stream;
    rocblas_handle ha = p.aux ? ctx->blas_aux : ctx->blas;
    if (p.aux) {
        SBO_HIP(hipEventRecord(ctx->ev_panel, ctx->stream));
        SBO_HIP(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_panel, 0));
    }
    if (p.inc_alpha) {
        const int64_t b = n - n_old;
        const double one = 1.0;
        SBO_HIP(ctx->rvec.reserve(sizeof(double) * (size_t)n));
        double *rv = ctx->rvec.as<double>();
        SBO_HIP(sbo::launch_widen_sub(sa, ctx->obs.as<float>(), ctx->hyper.prior_mean, n, rv));
        SBO_BLAS(rocblas_set_pointer_mode(ha, rocblas_pointer_mode_host));
        SBO_HIP(sbo::launch_row_dot(sa, Li + n_old, ld, b, n, rv, zv + n_old));
        SBO_HIP(hipMemsetAsync(d + n_old, 0, sizeof(double) * (size_t)b, sa));
        SBO_BLAS(rocblas_dgemv(ha, rocblas_operation_transpose, (rocblas_int)b, (rocblas_int)n, &one, Li + n_old,
                               (rocblas_int)ld, zv + n_old, 1, &one, d, 1));
    } else {
        // z = L^-1 r and alpha = L^-T z by the own two-pass kernels (one
        // read of the triangle each; rocBLAS dtrmv took 1.4 ms at C4)
        SBO_HIP(ctx->ws.awork.reserve(sbo::alpha_work_bytes(n)));
        SBO_HIP(sbo::launch_alpha_f64(sa, Li, ld, n, ctx->obs.as<float>(), ctx->hyper.prior_mean, zv, d,
                                      ctx->ws.awork.as<double>()));
    }
    ctx->z_n = n;
    SBO_HIP(sbo::launch_narrow(sa, d, n, ctx->alpha.as<float>()));
    if (p.aux) SBO_HIP(hipEventRecord(ctx->ev_trail, ctx->aux_stream));
    return SBO_OK;
}

// The packed f32 tiles from L^-1 on `stream`, and the fork: the sweeps'
// operands, derived from the packed f32 tiles (the split bf16 planes) and
// from L^-1 (the f64 operand, when the precision probe or the precise sweep
// will read it), on aux_stream beside the row sums and tile norms, instead
// of lazily at the first tick (HBM-bound beside MFMA-bound; C4: 0.22 + 0.41
// ms off the fit's critical path).  refresh_join waits for them.
sbo_status refresh_packs(sbo_ctx *ctx, const RefreshPlan &p) {
    const int64_t n = p.n, ld = p.ld, npad = p.npad, I0 = p.I0;
    double *Li = ctx->Linv.as<double>();
    // (before the fork: a growing operand copies and waits on `stream`)
    if (p.eager_x3)
        if (sbo_status st = ctx->split.reserve(ctx, npad, p.x3_layout)) return st;
    if (p.eager_f64)
        if (sbo_status st = ctx->pop.reserve(ctx, npad)) return st;
    // the pack and the tile norms in one pass over L^-1 (tile_norm_kernel<true>)
    SBO_HIP(grow_keep(ctx, ctx->tile_lgn, 2 * sizeof(float4) * (size_t)sbo::total_tiles(p.nI),
                      2 * sizeof(float4) * p.old_tiles));
    SBO_HIP(sbo::launch_pack_tile_norms(ctx->stream, Li, ld, n, npad, I0, p.sf2, ctx->aug.as<float>(),
                                        ctx->tile_lgn.as<float4>()));
    if (!p.eager_x3 && !p.eager_f64) return SBO_OK;
    SBO_HIP(hipEventRecord(ctx->ev_panel, ctx->stream));
    SBO_HIP(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_panel, 0));
    if (p.eager_x3)   // (its coordinates: refresh_join)
        if (sbo_status st = ctx->split.update(ctx, npad, p.x3_layout, ctx->aux_stream, false)) return st;
    // the row sums too (the skip budget's, read by the host after the
    // tile norms): the tile norms start right after the pack
    SBO_HIP(ctx->ws.scratch.reserve(sizeof(double) * (size_t)npad));
    SBO_HIP(sbo::launch_row_l1(ctx->aux_stream, ctx->aug.as<float>(), npad, I0, ctx->ws.scratch.as<double>()));
    SBO_HIP(hipEventRecord(ctx->ev_pack, ctx->aux_stream));   // what the host reads in refresh_skip_budget
    // the precise operand after it, left running past this fit's host
    // sync: only the probe's precise sweep reads it, on the device,
    // after its event (round 6: 1.7 ms at C4 off the fit's critical path)
    if (p.eager_f64)
        if (sbo_status st = ctx->pop.update(ctx, npad, ctx->aux_stream)) return st;
    return SBO_OK;
}

// SBO_OPT_INVERSE_BITS 32: alpha = K^-1 (y - m0) by the f32 triangular
// solves, L^-1 by rocSOLVER strtri, packed with the coordinates in one launch
sbo_status refresh_f32(sbo_ctx *ctx, const RefreshPlan &p) {
    const int64_t n = p.n, ld = p.ld;
    float *L = ctx->L.as<float>(), *alpha = ctx->alpha.as<float>();
    ctx->linv_n = 0;
    SBO_HIP(sbo::launch_sub_scalar(ctx->stream, ctx->obs.as<float>(), (float)ctx->hyper.prior_mean, n, alpha));
    SBO_BLAS(rocsolver_spotrs(ctx->blas, rocblas_fill_lower, (rocblas_int)n, 1, L, (rocblas_int)ld, alpha,
                              (rocblas_int)n));
    SBO_HIP(ctx->Linv.reserve(sizeof(float) * (size_t)ld * (size_t)n));
    float *Li = ctx->Linv.as<float>();
    SBO_HIP(hipMemcpyAsync(Li, L, sizeof(float) * (size_t)ld * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
    SBO_BLAS(rocsolver_strtri(ctx->blas, rocblas_fill_lower, rocblas_diagonal_non_unit, (rocblas_int)n, Li,
                              (rocblas_int)ld, ctx->info.as<rocblas_int>()));
    SBO_HIP(sbo::launch_pack_operand(ctx->stream, Li, ld, n, p.npad, 0, p.sf2, ctx->x.as<float>(), ctx->y.as<float>(),
                                     alpha, ctx->aug.as<float>(), ctx->kcoord.as<float>()));
    return SBO_OK;
}

// The plan's column prefilter (SkipPlan::colmax) from the tile norms on
// `stream`, whole: an append changes the columns of every k-tile.
sbo_status refresh_colmax(sbo_ctx *ctx, int64_t npad) {
    SBO_HIP(ctx->tile_colmax.reserve(sizeof(float) * (size_t)(npad / sbo::kBK)));
    SBO_HIP(sbo::launch_tile_colmax(ctx->stream, ctx->tile_lgn.as<float4>(), npad, ctx->tile_colmax.as<float>()));
    return SBO_OK;
}

// What is left of the packs on `stream` -- the row sums and tile norms that
// did not run with the fork, the coordinate pack once alpha is there -- and
// the join with aux_stream.
sbo_status refresh_join(sbo_ctx *ctx, const RefreshPlan &p) {
    const int64_t npad = p.npad;
    const bool packs_aux = p.eager_x3 || p.eager_f64;
    if (!packs_aux) {
        SBO_HIP(ctx->ws.scratch.reserve(sizeof(double) * (size_t)npad));
        SBO_HIP(sbo::launch_row_l1(ctx->stream, ctx->aug.as<float>(), npad, p.I0, ctx->ws.scratch.as<double>()));
    }
    if (!p.f64) {   // (the f64 inverse's tile norms ran with its pack, refresh_packs)
        SBO_HIP(grow_keep(ctx, ctx->tile_lgn, 2 * sizeof(float4) * (size_t)sbo::total_tiles(p.nI),
                          2 * sizeof(float4) * p.old_tiles));
        SBO_HIP(sbo::launch_tile_norms(ctx->stream, ctx->aug.as<float>(), npad, p.I0, ctx->tile_lgn.as<float4>()));
    }
    if (sbo_status st = refresh_colmax(ctx, npad)) return st;
    if (p.f64) {   // (refresh_f32's pack wrote the coordinates)
        if (p.aux) SBO_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_trail, 0));
        SBO_HIP(sbo::launch_pack_kcoord(ctx->stream, ctx->x.as<float>(), ctx->y.as<float>(), ctx->alpha.as<float>(),
                                        p.n, npad, p.sf2, ctx->kcoord.as<float>()));
        if (p.eager_x3)  // the split sweep's coordinates (its planes are on aux_stream)
            if (sbo_status st = ctx->split.pack_coords(ctx, npad, ctx->stream)) return st;
    }
    if (packs_aux) SBO_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_pack, 0));  // row sums and packs
    return SBO_OK;
}

// The cutoff exponent L that keeps 2^-L `need` below one (16 .. 160), and the
// two cutoffs of a |dV(q)|_2 budget tau2: every K* entry of a dropped tile is
// below 2^-L, so each V_i moves by at most 2^-L max_i |A_i|_1 and |dV|_2 by
// sqrt(N) times that; lg_tau: log2 of each row block's share tau2 / sqrt(nI).
int skip_cut(double need) {
    const double l2 = std::log2(std::max(need, 1.0));
    return std::isfinite(l2) ? std::min(160, std::max(16, (int)std::ceil(l2))) : 160;
}
void skip_cutoffs(double max_row_l1, int64_t n, int64_t nI, double tau2, int &L, float &lg_tau) {
    L = skip_cut(max_row_l1 * std::sqrt((double)n) / tau2);
    lg_tau = (float)std::log2(tau2 / std::sqrt((double)nI));
}

// Error budget of the automatic K* tile cutoff (SBO_OPT_TILE_SKIP = -1),
// B = SBO_OPT_SKIP_BUDGET: sigma^2 = sf2 - |V|^2 moves by at most
// 2 |V|_2 |dV|_2 + |dV|_2^2 with |V|_2 <= sf2^(1/2), so |dV(q)|_2 <=
// tau2 = 2^-B sf2^(1/2) / 2 (less 1 %) keeps it below 2^-B sf2.
//  - tile-norm test (one row block per workgroup): row block I may lose
//    |dV_I|_2 <= tau2 / sqrt(nI); a dropped tile t costs at most
//    nu_It K*max(t), nu_It = min(16 max row sum, 8 |A_It|_F) (the tile's
//    2-norm gain bound), and the kernel drops the smallest first.
//  - distance cutoff (row-block chunks, and the reported L): every K*
//    entry of a dropped tile is below 2^-L, so each V_i moves by at most
//    2^-L max_i |A_i|_1 and |dV|_2 by sqrt(N) times that; L keeps it
//    below tau2.
// The mean (last row block) drops only tiles below 2^-L_mean, with
// 2^-L_mean |sf2 alpha|_1 <= 2^-B sf2^(1/2).  Rows of earlier row blocks
// are unchanged by an append: only the repacked row blocks are measured.
sbo_status refresh_skip_budget(sbo_ctx *ctx, const RefreshPlan &p) {
    const int64_t n = p.n, r0 = p.I0 * sbo::kBM;
    std::vector<double> rl1((size_t)(p.npad - r0));
    std::vector<float> ha((size_t)n);
    SBO_HIP(hipMemcpyAsync(rl1.data(), ctx->ws.scratch.as<double>() + r0, sizeof(double) * (p.npad - r0),
                           hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipMemcpyAsync(ha.data(), ctx->alpha.as<float>(), sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    double mx = *std::max_element(rl1.begin(), rl1.end());
    if (p.incr || p.removed) mx = std::max(mx, ctx->max_row_l1);   // (the rows below I0 are the ones it was taken over)
    ctx->max_row_l1 = mx;
    double al1 = 0.0;
    for (float v : ha) al1 += std::fabs((double)v);
    ctx->alpha_l1 = al1 * p.sf2;
    const double tol = std::ldexp(1.0, -ctx->opt.skip_budget), sf = std::sqrt(p.sf2);
    const double tau2 = tol * sf / 2.0 * 0.99;  // 1 % for the dV^2 term
    skip_cutoffs(ctx->max_row_l1, n, p.nI, tau2, ctx->auto_skip_log2, ctx->lg_tau_v);
    ctx->auto_skip_mean_log2 = skip_cut(ctx->alpha_l1 / (tol * sf));
    return SBO_OK;
}

// The tile boxes, then every rocSOLVER info slot read in one sync: a singular
// block anywhere (the first non-zero slot) is NOT_SPD.  Past that check the
// packed operand is the context's: npad.
sbo_status refresh_read_info(sbo_ctx *ctx, const RefreshPlan &p) {
    SBO_HIP(ctx->kbox.reserve(sizeof(float4) * (size_t)(p.npad / sbo::kBK)));
    SBO_HIP(sbo::launch_tile_boxes(ctx->stream, ctx->x.as<float>(), ctx->y.as<float>(), p.n, p.npad,
                                   ctx->kbox.as<float4>()));
    const int64_t nslots = p.info_slots;
    std::vector<rocblas_int> hinfos((size_t)nslots);
    SBO_HIP(hipMemcpyAsync(hinfos.data(), ctx->info.as<rocblas_int>(), sizeof(rocblas_int) * (size_t)nslots,
                           hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    rocblas_int hinfo = 0;
    for (rocblas_int v : hinfos)
        if (hinfo == 0) hinfo = v;
    if (hinfo != 0) ctx->linv_n = 0;
    SBO_CHECK(hinfo == 0, SBO_E_NOT_SPD, "trtri: singular factor (info=" + std::to_string(hinfo) + ")");
    ctx->npad = p.npad;
    return SBO_OK;
}

// The guard's reading of this attempt's inverse, kept in chk_res; true when
// the inverse has to be redone.
sbo_status refresh_guard_verdict(sbo_ctx *ctx, InvAttempt attempt, bool &redo) {
    sbo_inv_check r = ctx->chk_res;
    if (sbo_status st = inverse_check_read(ctx, r)) return st;
    r.err_fallback = r.err_mean_fallback = -1.0;
    r.kept_digits = r.digits;
    ctx->chk_res = r;
    if (attempt != kInvDgemm) record_inv_digits(ctx, r);
    redo = !inv_check_passed(ctx, r) && r.digits != 0 && attempt != kInvDgemm;
    return SBO_OK;
}

// Rebuild alpha, L^-1 and the packed predictive operand from the current L
// (n_old > 0: an append of rows n_old..n-1, inverse_incremental -- only the
// row blocks that hold new rows are repacked; alpha, the per-k coordinates
// and the tile boxes are rebuilt in full, O(n^2) and O(n)).  ho: what the
// factorization that just ran handed over (blocked_potrf).
// The guard's redo: a sliced inverse that misses the guard's bound on the
// variance or the mean is redone -- a reduced-digit one at SBO_OPT_INV_OZ
// digits, a full one with dgemm products; the redone inverse is checked too
// (and a six-digit redo that misses tol goes on to dgemm products) -- and
// reported as fired with the kept inverse's readings.
// The caller's FitCommit waits for a guard still in flight when a stage fails.
// removed_from >= 0: sbo_remove's rotations left L and the f64 inverse current
// for the n points that remain; rows from removed_from on changed, so the
// packs of the row blocks from removed_from / kBM on are redone for the new
// npad (which may have lost a row block), alpha and z are solved in full and
// the guard does not run, as on appends.
sbo_status refresh_operand(sbo_ctx *ctx, int64_t n_old = 0, FactorHandover ho = {}, int64_t removed_from = -1) {
    sbo_inv_check first{};   // the reading that fired, and the rejected attempts' guard time
    bool fired = false;
    float ms_rejected = 0.0f;
    for (InvAttempt attempt = kInvChosen;;) {
        if (sbo_status st = ctx->pop.drain(ctx)) return st;
        const RefreshPlan p = plan_refresh(ctx, n_old, ho, attempt, removed_from);
        // what this refresh rewrites, for the derived operands: the row blocks from
        // I0 on (a full refresh: I0 = 0, everything); refresh_packs or the tick derives them
        ctx->split.rows_changed(p.I0);
        ctx->pop.rows_changed(p.I0);
        if (sbo_status st = refresh_begin(ctx, p)) return st;
        if (p.f64) {
            if (!p.removed)
                if (sbo_status st = refresh_inverse(ctx, p)) return st;
            if (sbo_status st = refresh_guard_launch(ctx, p)) return st;
            if (sbo_status st = refresh_alpha(ctx, p)) return st;
            if (sbo_status st = refresh_packs(ctx, p)) return st;
        } else {
            if (sbo_status st = refresh_f32(ctx, p)) return st;
        }
        if (sbo_status st = refresh_join(ctx, p)) return st;
        if (sbo_status st = refresh_skip_budget(ctx, p)) return st;
        if (sbo_status st = refresh_read_info(ctx, p)) return st;
        // The precision probe before the guard's reading (round 6): the guard's
        // three products on chk_stream run beside the probe's sweeps instead of
        // ahead of them (C4: the guard finished ~0.7 ms after the tail's last
        // kernel).  If the guard then fires, the fit's inverse is redone, and the
        // probe with it only because probe_n is reset first (as fill_and_factor
        // does for new data): probe_precision has just set it to n, and
        // probe_due() would keep the rejected inverse's readings.
        if (sbo_status st = probe_precision(ctx, ctx->opt.precision_opt)) return st;
        if (!p.guard) break;
        bool redo = false;
        if (sbo_status st = refresh_guard_verdict(ctx, attempt, redo)) return st;
        if (!redo) break;
        if (!fired) first = ctx->chk_res;
        fired = true;
        ms_rejected += ctx->chk_res.ms;
        if (ctx->chk_res.digits < ctx->opt.inv_oz) {
            attempt = kInvFullDigits;
            ctx->inv_oz_cur = ctx->opt.inv_oz;   // (the digits this fit's inverse ends up with)
        } else {
            attempt = kInvDgemm;
        }
        ctx->probe_n = 0;   // the probe above read the rejected inverse: measure the kept one
        n_old = 0;          // the redo is a full refresh, with nothing handed over
        removed_from = -1;
        ho = FactorHandover{};
    }
    if (fired) {
        const sbo_inv_check f = ctx->chk_res;   // the kept inverse's reading
        ctx->chk_res = first;
        ctx->chk_res.fired = 1;
        ctx->chk_res.err_fallback = f.ran ? f.err : -1.0;
        ctx->chk_res.err_mean_fallback = f.ran ? f.err_mean : -1.0;
        ctx->chk_res.kept_digits = f.ran ? f.kept_digits : 0;
        ctx->chk_res.ms = ms_rejected + f.ms;
    }
    return SBO_OK;
}

// The precise sweep's budget: the same construction as the automatic cutoff
// (refresh_skip_budget) with the tolerance 2^-B times the smallest variance the
// probe saw inside the training box instead of 2^-B sf2 -- the 1e-5 contract
// is relative to the largest variance of a query set, and in the dense
// regime that is orders below sf2.
// (cutoff exponent, log2 of the row blocks' |dV_I|_2 share) keeping the
// dropped tiles' effect on any variance below tol (absolute)
void skip_budget_for(const sbo_ctx *ctx, double tol, int &L, float &lg_tau) {
    const double sf2 = ctx->hyper.sigma_f * ctx->hyper.sigma_f, sf = std::sqrt(sf2);
    skip_cutoffs(ctx->max_row_l1, ctx->n, ctx->npad / sbo::kBM, tol / (2.0 * sf) * 0.99, L, lg_tau);
}
void precise_budget(sbo_ctx *ctx) {
    const double sf2 = ctx->hyper.sigma_f * ctx->hyper.sigma_f;
    const double floor_v = std::max(ctx->probe_vmin, 1e-12 * sf2);
    skip_budget_for(ctx, std::ldexp(1.0, -ctx->opt.skip_budget) * std::min(floor_v, sf2), ctx->p_skip_log2,
                    ctx->p_lg_tau_v);
}

// SBO_OPT_PRECISION (-1 auto): which sweep the ticks run.  The probe sweeps
// its query set twice -- the fast split sweep and the precise sweep (the
// kernel SBO_OPT_PRECISE_KERNEL names; default 3, the int8-sliced one with
// K*'s digit table) under a budget of 2^-kProbeRefBits of the largest probe
// variance -- and measures the fast sweep's normwise variance error against
// it, max |d var| / max var (the contract's metric); above kPreciseTol the
// context's ticks use the precise sweep.  The query set (round 4, VERDICT r3
// next-1): a 32 x 32 grid over the training box AND at most 512 training
// locations: the stored points at stride / 2 + i stride over all of [0, n),
// stride = ceil(n / 512) -- every point of the k-d order up to n = 512, 500 of
// 1000, 512 of 16384 -- so dense clusters are sampled in proportion to their
// points wherever they are stored (a floor stride stopped at position
// 511 (n / 512): up to half of the points, the appended ones among them, went
// unprobed): where the data is dense the variance is
// smallest and sf2 - |V|^2 cancels hardest, and a narrow dense path (the
// publisher's data, turtlesim_spatial_publisher.py:151-183) falls between the
// grid's points.  The error is normalised by the largest variance of the whole
// set, as the contract normalises by its query set's (a grid over the data's
// bounds holds both kinds of points); each part's own normwise error is kept
// for sbo_get_probe.
// kPreciseTol = 5e-6 (round 4; 7e-6 before) rests on the envelope whole-grid
// error <= 1.62 probe + 1e-6 (docs/DESIGN_HISTORY.md 5a: 24 workloads at
// N = 8192, the fast sweep over the whole grid against the precise one; single
// ratios up to 1.77 / 2.47 occur only at probe readings below 1.4e-6): 9.1e-6
// at the threshold, inside the 1e-5 contract.  Measured probe errors: C2
// 2.1e-6, C3 4.2e-6, C4 4.4e-6, C5 4.4e-6, path 4.6e-7 -- fast; the lpsc box
// from N = 320 on (5.6e-6; 1.8e-5 / 8.9e-5 / 3.3e-4 at 1024 / 4096 / 16384) --
// precise.  tests/test_gpu_probe_decision.py holds the contract against the
// fp64 oracle on three ladders of readings from 1.5e-6 to 1.7e-5 across the
// threshold; every rung lies inside the envelope (profiles/probe_decision.log).
// Re-probed at every fit, and on appends once N has grown by
// SBO_OPT_REPROBE percent (default 25) since the last probe (probe_due).  A
// verdict just under the threshold stands over that growth: the same test
// grows the highest fast rungs by 24 % (uniform appends and appends into one
// l x l square) and the fast sweep stays inside the contract (the fresh
// reading at the end is logged beside the stale one).  Needs the f64 inverse
// (SBO_OPT_INVERSE_BITS 64) and a factor (not an imported state).
constexpr double kPreciseTol = 5e-6;
constexpr int kProbeRefBits = 24;
sbo_status probe_precision(sbo_ctx *ctx, int precision) {
    const bool avail = ctx->has_factor && inverse_current(ctx, ctx->n);
    if (!avail || precision == 0) {
        ctx->precise = false;
        if (!avail) ctx->probe_n = 0;
        return SBO_OK;
    }
    const bool fresh = probe_due(ctx);
    if (fresh) {
        const int G = ctx->opt.probe_grid, MG = G * G;
        const int64_t n = ctx->n;
        // the training part spans [0, n): positions stride / 2 + i stride with
        // the smallest stride that needs at most probe_train of them, and as
        // many as fit (512 at n = 16384, 500 at n = 1000; every point up to 512)
        const int64_t want = ctx->opt.probe_train;
        const int64_t stride = (n + want - 1) / want;     // >= 1
        const int MT = (int)((n - stride / 2 + stride - 1) / stride), M = MG + MT;
        std::vector<float> h(2 * (size_t)M);
        bbox_lattice(ctx->bbox, G, h.data(), h.data() + M);
        SBO_HIP(ctx->qprobe.reserve(sizeof(float) * 2 * M));
        SBO_HIP(ctx->oprobe.reserve(sizeof(float) * 2 * M + sizeof(sbo_key)));
        float *qx = ctx->qprobe.as<float>(), *qy = qx + M, *sdf = ctx->oprobe.as<float>(), *sdp = sdf + M;
        sbo_key *key = reinterpret_cast<sbo_key *>(sdp + M);
        SBO_HIP(hipMemcpyAsync(qx, h.data(), sizeof(float) * MG, hipMemcpyHostToDevice, ctx->stream));
        SBO_HIP(hipMemcpyAsync(qy, h.data() + M, sizeof(float) * MG, hipMemcpyHostToDevice, ctx->stream));
        // the training part: every stride-th stored point
        if (sbo_status cst = copy_strided_points(ctx, ctx->stream, stride, MT, qx + MG, qy + MG)) return cst;
        // the two sweeps: the same queries, each its own sweep and output
        TickRequest fast;
        fast.qx = qx;
        fast.qy = qy;
        fast.m = M;
        fast.sd = sdf;
        fast.key = key;
        fast.sweep = Sweep::kFast;
        fast.quiet = true;
        TickPlan fast_plan;
        sbo_status st = run_tick(ctx, fast, &fast_plan);
        if (st == SBO_OK) {
            // the reference's budget: 2^-kProbeRefBits of the largest variance
            // the fast sweep sees (its own error is orders below that: any
            // estimate within 2x serves), so the reference moves the measured
            // error by < 2^-23 of max var (1.7 % of the 7e-6 threshold); at
            // most 2^-kProbeRefBits sf2, at least 2^-(2 kProbeRefBits) sf2 (was
            // a fixed 2^-44 sf2, then 2^-30 of max var: DESIGN.md section 5a)
            const double sf2 = ctx->hyper.sigma_f * ctx->hyper.sigma_f;
            if (hipMemcpyAsync(h.data(), sdf, sizeof(float) * M, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                hipStreamSynchronize(ctx->stream) != hipSuccess)
                st = SBO_E_DEVICE;
            double vf = 0.0;
            for (int i = 0; i < M; ++i) vf = std::max(vf, (double)h[i] * h[i]);
            ctx->probe_ref_tol = std::ldexp(
                std::clamp(std::isfinite(vf) ? vf : sf2, std::ldexp(sf2, -kProbeRefBits), sf2), -kProbeRefBits);
        }
        if (st == SBO_OK) {
            // the same queries as the fast sweep's: its Morton order again
            // (qwork untouched in between)
            TickRequest ref = fast;
            ref.sd = sdp;
            ref.sweep = Sweep::kProbeRef;
            ref.order = QueryOrder{fast_plan.perm, fast_plan.qx, fast_plan.qy};
            st = run_tick(ctx, ref);
        }
        if (st != SBO_OK) return st;
        SBO_HIP(hipMemcpyAsync(h.data(), sdf, sizeof(float) * 2 * M, hipMemcpyDeviceToHost, ctx->stream));
        SBO_HIP(hipStreamSynchronize(ctx->stream));
        double dmax[2] = {0.0, 0.0}, vmax[2] = {0.0, 0.0}, vmin = HUGE_VAL;
        for (int i = 0; i < M; ++i) {
            const double vf = (double)h[i] * h[i], vp = (double)h[M + i] * h[M + i];
            const int part = i < MG ? 0 : 1;
            dmax[part] = std::max(dmax[part], std::fabs(vf - vp));
            vmax[part] = std::max(vmax[part], vp);
            vmin = std::min(vmin, vp);
        }
        auto rel = [](double d, double v) { return v > 0.0 ? d / v : 0.0; };
        const double va = std::max(vmax[0], vmax[1]);
        ctx->probe_err = rel(std::max(dmax[0], dmax[1]), va);
        ctx->probe_err_grid = rel(dmax[0], vmax[0]);
        ctx->probe_err_train = rel(dmax[1], vmax[1]);
        ctx->probe_vmax_grid = vmax[0];
        ctx->probe_vmax_train = vmax[1];
        ctx->probe_m_grid = MG;
        ctx->probe_m_train = MT;
        ctx->probe_vmin = vmin;
        ctx->probe_vmax = va;
        ctx->probe_n = ctx->n;
    }
    precise_budget(ctx);
    // a looser skip budget than the default (B < 20: the caller trades
    // accuracy for speed) loosens the threshold by the same factor
    const double tol = kPreciseTol * std::ldexp(1.0, std::max(0, 20 - ctx->opt.skip_budget));
    ctx->precise = precision == 1 || ctx->probe_err > tol;
    return SBO_OK;
}

// ---- the blocked Cholesky (SBO_OPT_CHOLESKY 1 / 2) ----
//
// Everything one factorization decides, once, before its first launch
// (chol_plan): the stages below read it and none of them looks the conditions
// up again.  SBO_OPT_CHOL_GEMM and SBO_OPT_CHOLESKY are decoded here only.
struct CholPlan {
    int64_t n, ld;       // the n x n lower triangle, leading dimension ld
    int64_t NB, NB2;     // the chain's block (kCholNB) and the outer panel (SBO_OPT_CHOL_OUTER; NB: one level)
    // SBO_OPT_CHOL_GEMM 0 rocBLAS; 1 chol_update_kernel for trailing updates of
    // at most 8192 rows (where it measured faster than rocBLAS); 2 for every
    // update; 3 the outer panel split into bf16 planes; 4 / 5 the outer
    // panel's updates as the int8-sliced GEMM with that many digits
    enum Update { kRocblas, kOwnSmall, kOwn, kX3, kOz } update;
    int oz_digits;       // kOz: 4 or 5
    int chain;           // SBO_OPT_CHOL_DIAG: the version of the chain's two kernels
    bool own_trsm;       // the panel solve by chol_trsm_kernel (SBO_OPT_CHOLESKY 1), else rocBLAS strsm (2)
    bool early;          // the inverse's first half runs beside the last steps (SBO_OPT_INV_OVERLAP) ...
    int64_t h_inv;       // ... once the factor's left h_inv columns are final (-1: never) ...
    sbo::InvPlan inv;    // ... by this plan (the refresh finishes it: FactorHandover)
    bool widen;          // the f64 copy of the factor is written panel by panel into Linv
    rocblas_int *info;   // rocSOLVER-style info: slot 0 the leading minor, with `early` the first half's after it
    int64_t info_slots;
};

// Which of the three updates of a step chol_update runs.  The inner update (the
// outer panel's remaining columns, after each 128-column block) never reads
// the packed panel; only the trailing update (everything right of the next
// outer panel) writes the lower triangle alone, and only it has the size rules
// of kOwnSmall and kSmallTrail.
enum class UpdateSite { kInner, kLookahead, kTrailing };

// Below this size the trailing update is one sgemm over the full square
// (rocBLAS ssyrk: 82 vs 49 us at m = 4000, 67 vs 20 at 2000, k = 128;
// tools/r3_gemm_probe.cpp); the upper triangle it also writes is never read.
constexpr int64_t kSmallTrail = 6144;

// The outer panel's rows below it (m3 x W), packed once per outer step for the
// look-ahead and the trailing update (chol_pack_panel): int8 digits (kOz, W a
// multiple of 64 and the next panel's width W2 of 128; the last panels are
// rocBLAS's) or bf16 planes (kX3, W a multiple of 32).  Two buffers alternate
// across steps: the trailing update on aux_stream may still read the previous
// one until the next look-ahead has waited for it.
struct PanelPack {
    bool oz = false, x3 = false;
    int buffer = 0;                // which of ctx->ws.cholx3
    const char *planes = nullptr;
};

// Failures of the launched stages carry no text of their own: blocked_potrf
// gives them one (the set-up stages keep SBO_HIP's, which names the call and
// tells out-of-memory apart).
#define CHOL_HIP(expr)                               \
    do {                                             \
        if ((expr) != hipSuccess) return SBO_E_DEVICE; \
    } while (0)
#define CHOL_BLAS(expr)                                           \
    do {                                                          \
        if ((expr) != rocblas_status_success) return SBO_E_DEVICE; \
    } while (0)

// The plan, and the info slots it points at (sized here, so that the pointer
// is final before the first launch).
sbo_status chol_plan(sbo_ctx *ctx, int64_t n, int64_t ld, bool early_inv, CholPlan &p) {
    const sbo_options &o = ctx->opt;
    p.n = n;
    p.ld = ld;
    p.NB = sbo::kCholNB;
    p.NB2 = std::max<int64_t>(p.NB, (int64_t)o.chol_outer / p.NB * p.NB);
    const int g = o.chol_gemm_own;
    p.update = g == 1   ? CholPlan::kOwnSmall
               : g == 2 ? CholPlan::kOwn
               : g == 3 ? CholPlan::kX3
               : g >= 4 ? CholPlan::kOz
                        : CholPlan::kRocblas;
    p.oz_digits = p.update == CholPlan::kOz ? g : 0;
    p.chain = o.chol_diag;
    p.own_trsm = o.chol_trsm_own;
    // early_inv: a fit with the recursive f64 inverse.  Its first half beside
    // the Cholesky with SBO_OPT_INV_OVERLAP = R > 0; otherwise the factor is
    // widened for it on the way.
    p.early = early_inv && o.inv_overlap > 0 && n > o.inv_base;
    if (p.early) p.inv = sbo::plan_inverse(inv_config_early(ctx), n, ld);
    p.h_inv = p.early ? p.inv.nodes[0].h : -1;
    p.widen = early_inv && !p.early;
    p.info_slots = p.early ? p.inv.info_total : 1;
    SBO_HIP(ctx->info.reserve(sizeof(rocblas_int) * (size_t)p.info_slots));
    p.info = ctx->info.as<rocblas_int>();
    return SBO_OK;
}

// *s, with the rocBLAS handle *hb bound to it: a stream that stays off the
// first `reserve` CUs (0: an ordinary non-blocking stream), made on first use
// and made again when the mask changed.
sbo_status forked_stream(sbo_ctx *ctx, hipStream_t *s, rocblas_handle *hb, int *reserved, int reserve) {
    if (*s && *reserved != reserve) {
        SBO_HIP(hipStreamSynchronize(*s));
        SBO_HIP(hipStreamDestroy(*s));
        *s = nullptr;
    }
    if (*s && *hb) return SBO_OK;
    if (!*s) {
        if (reserve > 0) {
            std::vector<uint32_t> mask((size_t)(ctx->num_cu + 31) / 32, 0u);
            for (int c = reserve; c < ctx->num_cu; ++c) mask[(size_t)c / 32] |= 1u << (c % 32);
            SBO_HIP(hipExtStreamCreateWithCUMask(s, (uint32_t)mask.size(), mask.data()));
        } else {
            SBO_HIP(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
        }
        *reserved = reserve;
    }
    if (!*hb) SBO_BLAS(rocblas_create_handle(hb));
    SBO_BLAS(rocblas_set_stream(*hb, *s));
    return SBO_OK;
}

// The lazy set-up: aux_stream for the trailing updates, off the first
// SBO_OPT_CHOL_RESERVE CUs so that the latency-bound chain finds them free,
// and for an early half inv_stream, which leaves SBO_OPT_INV_OVERLAP CUs to
// the chain (its kernels would otherwise queue behind the long dgemm
// workgroups); each with its handle and its events.  aux_ready() is true from
// here on.
sbo_status chol_streams(sbo_ctx *ctx, const CholPlan &p) {
    if (p.early) {
        sbo_status st = forked_stream(ctx, &ctx->inv_stream, &ctx->blas_inv, &ctx->inv_reserved, ctx->opt.inv_overlap);
        if (st != SBO_OK) return st;
        if (!ctx->ev_half) {
            SBO_HIP(hipEventCreateWithFlags(&ctx->ev_half, hipEventDisableTiming));
            SBO_HIP(hipEventCreateWithFlags(&ctx->ev_inv, hipEventDisableTiming));
        }
    }
    if (sbo_status st = forked_stream(ctx, &ctx->aux_stream, &ctx->blas_aux, &ctx->aux_reserved, ctx->opt.chol_reserve))
        return st;
    if (!ctx->ev_panel) {   // (all four together: aux_ready tests the first)
        SBO_HIP(hipEventCreateWithFlags(&ctx->ev_panel, hipEventDisableTiming));
        SBO_HIP(hipEventCreateWithFlags(&ctx->ev_trail, hipEventDisableTiming));
        SBO_HIP(hipEventCreateWithFlags(&ctx->ev_pack, hipEventDisableTiming));
        SBO_HIP(hipEventCreateWithFlags(&ctx->pop.ev, hipEventDisableTiming));
    }
    SBO_BLAS(rocblas_set_pointer_mode(ctx->blas, rocblas_pointer_mode_host));
    SBO_BLAS(rocblas_set_pointer_mode(ctx->blas_aux, rocblas_pointer_mode_host));
    return SBO_OK;
}

// Every buffer the early half touches, sized before it starts (a reserve that
// reallocates later would free memory in use), and its info slots cleared.
sbo_status chol_reserve_early(sbo_ctx *ctx, const CholPlan &p) {
    if (sbo_status st = inverse_reserve(ctx, p.inv)) return st;
    SBO_HIP(hipMemsetAsync(p.info, 0, sizeof(rocblas_int) * (size_t)p.info_slots, ctx->stream));
    return SBO_OK;
}

// The widened factor's place, and both pack buffers at the first outer
// panel's size, up front.
sbo_status chol_reserve_panels(sbo_ctx *ctx, const CholPlan &p) {
    if (p.widen) SBO_HIP(ctx->Linv.reserve(sizeof(double) * (size_t)p.ld * (size_t)p.ld));
    if (p.n <= p.NB2) return SBO_OK;
    for (sbo::DevBuf &pb : ctx->ws.cholx3) {
        if (p.update == CholPlan::kX3) SBO_HIP(pb.reserve(sbo::chol_x3_bytes(p.n - p.NB2, p.NB2)));
        if (p.update == CholPlan::kOz) SBO_HIP(pb.reserve(sbo::gz_pack_bytes(p.n - p.NB2, p.NB2, p.oz_digits)));
    }
    return SBO_OK;
}

// One step of the chain on `stream`: the kb x kb diagonal block at L11 (step
// k) in one workgroup, then the m2 rows below it, A21 := A21 L11^-T.
sbo_status chol_chain_step(sbo_ctx *ctx, const CholPlan &p, float *L11, int64_t kb, int64_t k, int64_t m2) {
    CHOL_HIP(sbo::launch_chol_diag(ctx->stream, L11, p.ld, (int)kb, k, p.info, p.chain));
    if (m2 <= 0) return SBO_OK;
    if (p.own_trsm) {
        CHOL_HIP(sbo::launch_chol_trsm(ctx->stream, L11, p.ld, (int)kb, L11 + kb, m2, p.chain));
    } else {
        const float one = 1.0f;
        CHOL_BLAS(rocblas_strsm(ctx->blas, rocblas_side_right, rocblas_fill_lower, rocblas_operation_transpose,
                                rocblas_diagonal_non_unit, (rocblas_int)m2, (rocblas_int)kb, &one, L11,
                                (rocblas_int)p.ld, L11 + kb, (rocblas_int)p.ld));
    }
    return SBO_OK;
}

// C (mr x nc, lda ld) -= P[r0 .. r0 + mr) P[c0 .. c0 + nc)^T for row ranges of
// the m x k panel P, on stream s (hb: the rocBLAS handle bound to it), by the
// plan's back end for this site.
sbo_status chol_update(const CholPlan &p, const PanelPack &pk, UpdateSite site, hipStream_t s, rocblas_handle hb,
                       const float *P, int64_t m, int64_t k, int64_t r0, int64_t mr, int64_t c0, int64_t nc,
                       float *C) {
    const bool trailing = site == UpdateSite::kTrailing;
    const bool packed = site != UpdateSite::kInner;
    if (packed && pk.oz) {
        CHOL_HIP(sbo::launch_gz_gemm_packed_f32(s, p.oz_digits, pk.planes, m, k, r0, mr, c0, nc, -1.0, C, p.ld,
                                                sbo::kGzBeta1 | (trailing ? sbo::kGzLowerC : 0u)));
    } else if (packed && pk.x3) {
        CHOL_HIP(sbo::launch_chol_update_x3(s, pk.planes, m, k, r0, mr, c0, nc, trailing, C, p.ld));
    } else if (p.update == CholPlan::kOwn || (p.update == CholPlan::kOwnSmall && trailing && mr <= 8192)) {
        CHOL_HIP(sbo::launch_chol_update(s, P + r0, P + c0, p.ld, mr, nc, k, trailing, C));
    } else if (trailing && mr > kSmallTrail) {
        const float one = 1.0f, minus_one = -1.0f;
        CHOL_BLAS(rocblas_ssyrk(hb, rocblas_fill_lower, rocblas_operation_none, (rocblas_int)mr, (rocblas_int)k,
                                &minus_one, P + r0, (rocblas_int)p.ld, &one, C, (rocblas_int)p.ld));
    } else {
        const float one = 1.0f, minus_one = -1.0f;
        CHOL_BLAS(rocblas_sgemm(hb, rocblas_operation_none, rocblas_operation_transpose, (rocblas_int)mr,
                                (rocblas_int)nc, (rocblas_int)k, &minus_one, P + r0, (rocblas_int)p.ld, P + c0,
                                (rocblas_int)p.ld, &one, C, (rocblas_int)p.ld));
    }
    return SBO_OK;
}

// Joins the streams blocked_potrf forked if it returns early: aux_stream, and
// inv_stream once the early half has started.  Dismissed on success (the
// joins are then events on `stream`, chol_join).
struct CholJoin {
    sbo_ctx *ctx;
    bool early_started = false, dismissed = false;
    ~CholJoin() {
        if (dismissed) return;
        (void)hipStreamSynchronize(ctx->aux_stream);
        if (early_started) (void)hipStreamSynchronize(ctx->inv_stream);
    }
};

// The left h_inv columns are final: the inverse's first half on inv_stream
// (widen them, A^-1, S = B A^-1: half its flops) beside the Cholesky's last
// steps, which leave most CUs idle.  refresh_operand finishes the inverse.
sbo_status chol_early_half(sbo_ctx *ctx, const CholPlan &p, const float *L, CholJoin &join, FactorHandover &ho) {
    double *Li = ctx->Linv.as<double>();
    CHOL_HIP(hipEventRecord(ctx->ev_half, ctx->stream));
    CHOL_HIP(hipStreamWaitEvent(ctx->inv_stream, ctx->ev_half, 0));
    CHOL_HIP(sbo::launch_widen(ctx->inv_stream, L, p.ld, p.n, p.h_inv, true, Li, p.ld));
    join.early_started = true;
    if (sbo_status st = inverse_early_half(ctx, p.inv)) return st;
    ho.half = p.inv;
    CHOL_HIP(hipEventRecord(ctx->ev_inv, ctx->inv_stream));
    return SBO_OK;
}

// The pack of the outer panel's m3 x W rows below it, where this step's
// shapes allow the plan's packed update (else an empty PanelPack: rocBLAS or
// chol_update_kernel read P itself).
sbo_status chol_pack_panel(sbo_ctx *ctx, const CholPlan &p, const float *P, int64_t m3, int64_t W, int64_t W2,
                           int buffer, PanelPack &pk) {
    pk = PanelPack{};
    pk.buffer = buffer;
    pk.oz = p.update == CholPlan::kOz && W % 64 == 0 && W2 % 128 == 0;
    pk.x3 = p.update == CholPlan::kX3 && W % 32 == 0;
    if (!pk.oz && !pk.x3) return SBO_OK;
    sbo::DevBuf &pb = ctx->ws.cholx3[buffer];
    if (pk.oz) {
        CHOL_HIP(sbo::launch_gz_pack_f32(ctx->stream, p.oz_digits, P, p.ld, m3, W, pb.as<char>()));
    } else {
        CHOL_HIP(pb.reserve(sbo::chol_x3_bytes(m3, W)));
        CHOL_HIP(sbo::launch_chol_split(ctx->stream, P, p.ld, m3, W, pb.as<char>()));
    }
    pk.planes = pb.as<char>();
    return SBO_OK;
}

// The outer panel at columns [K, K + W) is factored: its rank-W update of the
// trailing matrix, in two parts.  The look-ahead -- the next outer panel's W2
// columns -- on `stream`, followed at once by that panel's chain, so that the
// one-CU diagonal kernels run beside the big update instead of between
// updates; the rest on aux_stream.  ev_panel: the panel (and its pack) is
// ready; ev_trail: the trailing update is done, which the next look-ahead
// waits for (it wrote those columns too) and the final join.
sbo_status chol_outer_update(sbo_ctx *ctx, const CholPlan &p, float *L, int64_t K, int64_t W, bool &trail_pending) {
    const int64_t m3 = p.n - K - W, W2 = std::min(p.NB2, m3), m4 = m3 - W2;
    const float *P = L + (K + W) + K * p.ld;   // the panel's rows below it: m3 x W
    float *C1 = L + (K + W) + (K + W) * p.ld;
    PanelPack pk;
    if (sbo_status st = chol_pack_panel(ctx, p, P, m3, W, W2, (int)((K / p.NB2) & 1), pk)) return st;
    CHOL_HIP(hipEventRecord(ctx->ev_panel, ctx->stream));
    if (trail_pending) CHOL_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_trail, 0));
    if (sbo_status st = chol_update(p, pk, UpdateSite::kLookahead, ctx->stream, ctx->blas, P, m3, W, 0, m3, 0, W2, C1))
        return st;
    trail_pending = false;
    if (m4 <= 0) return SBO_OK;
    CHOL_HIP(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_panel, 0));
    if (sbo_status st = chol_update(p, pk, UpdateSite::kTrailing, ctx->aux_stream, ctx->blas_aux, P, m3, W, W2, m4, W2,
                                    m4, C1 + W2 + W2 * p.ld))
        return st;
    trail_pending = true;
    CHOL_HIP(hipEventRecord(ctx->ev_trail, ctx->aux_stream));
    return SBO_OK;
}

// The f64 copy of the factor the inverse starts from (refresh_operand),
// widened panel by panel as outer panels become final: on aux_stream after
// each trailing update, beside the chain's latency-bound second half, instead
// of one 0.7 ms pass between the factorization and the inverse (C4).  The
// strictly upper part is zeroed with it.  The panel's columns are final at
// ev_panel, which aux_stream has waited for if it took a trailing update;
// coming after ev_trail's record, the widen stays off the look-ahead's
// dependency chain.
sbo_status chol_widen_panel(sbo_ctx *ctx, const CholPlan &p, const float *L, int64_t K, int64_t W, bool waited) {
    double *Lw = ctx->Linv.as<double>();
    if (!waited) CHOL_HIP(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_panel, 0));
    CHOL_HIP(sbo::launch_widen(ctx->aux_stream, L + K + K * p.ld, p.ld, p.n - K, W, true, Lw + K + K * p.ld, p.ld));
    if (K > 0)
        CHOL_HIP(hipMemset2DAsync(Lw + K * p.ld, sizeof(double) * (size_t)p.ld, 0, sizeof(double) * (size_t)K,
                                  (size_t)W, ctx->aux_stream));
    return SBO_OK;
}

// `stream` waits for what was forked: the last trailing update, the widened
// panels (after widening the last outer panel, columns Kw.., itself) and the
// early half; and says in `ho` what is there for the refresh.
sbo_status chol_join(sbo_ctx *ctx, const CholPlan &p, const float *L, int64_t Kw, bool trail_pending,
                     bool early_started, FactorHandover &ho) {
    if (trail_pending) CHOL_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_trail, 0));
    if (p.widen) {
        double *Lw = ctx->Linv.as<double>();
        const int64_t r = p.n - Kw;
        CHOL_HIP(sbo::launch_widen(ctx->stream, L + Kw + Kw * p.ld, p.ld, r, r, true, Lw + Kw + Kw * p.ld, p.ld));
        if (Kw > 0)
            CHOL_HIP(hipMemset2DAsync(Lw + Kw * p.ld, sizeof(double) * (size_t)p.ld, 0, sizeof(double) * (size_t)Kw,
                                      (size_t)r, ctx->stream));
        CHOL_HIP(hipEventRecord(ctx->ev_trail, ctx->aux_stream));
        CHOL_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_trail, 0));
        ho.widened_n = p.n;
    }
    if (early_started) {
        CHOL_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_inv, 0));
        ho.half_n = p.n;
    }
    return SBO_OK;
}

// Right-looking blocked Cholesky of the n x n lower triangle at L (lda = ld),
// in two levels.  Outer panels of NB2 columns; each is factored by the chain
// of NB = 128 columns (chol_chain_step: diagonal block, panel below it) with
// the updates after each block kept inside the outer panel (chol_update,
// kInner), and the rest of the trailing matrix takes one rank-NB2 update per
// outer panel, split into the look-ahead on `stream` and the rest on
// aux_stream (chol_outer_update).  NB2 = NB is the one-level factorization.
// The same factorization as spotrf without its unblocked potf2 panels; info
// as rocSOLVER's.  early_inv: a fit whose recursive f64 inverse follows.
// Either its first half runs on inv_stream as soon as the columns it reads
// are final (chol_early_half), or the factor is widened to f64 for it panel
// by panel (chol_widen_panel).  ho: what is handed to the refresh, and the
// info slots used.  Nothing here waits on the host; after a failure the
// forked streams are joined (CholJoin) before the error is returned.
sbo_status blocked_potrf(sbo_ctx *ctx, float *L, int64_t n, int64_t ld, bool early_inv, FactorHandover &ho) {
    CholPlan p;
    if (sbo_status st = chol_plan(ctx, n, ld, early_inv, p)) return st;
    ho = FactorHandover{};
    ho.info = p.info;
    SBO_HIP(hipMemsetAsync(p.info, 0, sizeof(rocblas_int), ctx->stream));
    if (sbo_status st = chol_streams(ctx, p)) return st;
    if (p.early)
        if (sbo_status st = chol_reserve_early(ctx, p)) return st;
    if (sbo_status st = chol_reserve_panels(ctx, p)) return st;
    CholJoin join{ctx};
    const auto fail = [ctx](sbo_status st) {
        ctx->err = "blocked Cholesky: a rocBLAS or HIP call failed";
        return st;
    };
    bool trail_pending = false;
    int64_t Kw = 0;   // columns [0, Kw) widened (enqueued)
    for (int64_t K = 0; K < n; K += p.NB2) {
        const int64_t W = std::min(p.NB2, n - K);
        for (int64_t k = K; k < K + W; k += p.NB) {
            const int64_t kb = std::min(p.NB, n - k), m2 = n - k - kb;
            float *L11 = L + k + k * ld;
            if (sbo_status st = chol_chain_step(ctx, p, L11, kb, k, m2)) return fail(st);
            if (m2 <= 0) break;
            if (k + kb == p.h_inv)
                if (sbo_status st = chol_early_half(ctx, p, L, join, ho)) return fail(st);
            const int64_t rem = K + W - (k + kb);   // the outer panel's remaining columns (rows below this block)
            if (rem > 0)
                if (sbo_status st = chol_update(p, PanelPack{}, UpdateSite::kInner, ctx->stream, ctx->blas, L11 + kb,
                                                m2, kb, 0, m2, 0, rem, L11 + kb + kb * ld))
                    return fail(st);
        }
        if (n - K - W <= 0) break;
        if (sbo_status st = chol_outer_update(ctx, p, L, K, W, trail_pending)) return fail(st);
        if (p.widen) {   // (a trailing update pending: aux_stream has waited for this panel)
            if (sbo_status st = chol_widen_panel(ctx, p, L, K, W, trail_pending)) return fail(st);
            Kw = K + W;
        }
    }
    if (sbo_status st = chol_join(ctx, p, L, Kw, trail_pending, join.early_started, ho)) return fail(st);
    join.dismissed = true;
    return SBO_OK;
}
#undef CHOL_HIP
#undef CHOL_BLAS

// The leading minor rocSOLVER's or blocked_potrf's info slot 0 reports, read
// back (the factorization's one host sync); non-zero: SBO_E_NOT_SPD.
enum class FactorOf { kFit, kAppendedBlock };
sbo_status factor_info(sbo_ctx *ctx, const rocblas_int *info, FactorOf what) {
    rocblas_int hinfo = 0;
    SBO_HIP(hipMemcpyAsync(&hinfo, info, sizeof(hinfo), hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    if (hinfo == 0) return SBO_OK;
    ctx->err = what == FactorOf::kFit
                   ? "spotrf: leading minor " + std::to_string(hinfo) + " not positive definite"
                   : "sbo_append: updated block not positive definite (info=" + std::to_string(hinfo) + ")";
    return SBO_E_NOT_SPD;
}

// The n x n lower triangle at L (already filled, lda = ld) factored in place
// by the blocked Cholesky or rocSOLVER's spotrf (SBO_OPT_CHOLESKY 0), and its
// info read.  Only blocked_potrf hands anything to refresh_operand.
sbo_status factor_block(sbo_ctx *ctx, float *L, int64_t n, int64_t ld, bool early_inv, FactorOf what,
                        FactorHandover &ho) {
    ho = FactorHandover{};
    ho.info = ctx->info.as<rocblas_int>();
    if (ctx->opt.chol_blocked) {
        if (sbo_status st = blocked_potrf(ctx, L, n, ld, early_inv, ho)) return st;
    } else {
        SBO_BLAS(rocsolver_spotrf(ctx->blas, rocblas_fill_lower, (rocblas_int)n, L, (rocblas_int)ld, ho.info));
    }
    return factor_info(ctx, ho.info, what);
}

// Factor K in L (already filled, lda = cap) and refresh the operand.
sbo_status factor_and_refresh(sbo_ctx *ctx) {
    ctx->inv_oz_cur = choose_inv_digits(ctx);
    FactorHandover ho;
    if (sbo_status st = factor_block(ctx, ctx->L.as<float>(), ctx->n, ctx->cap, ctx->opt.inverse_bits == 64 && ctx->opt.inverse_rec,
                                     FactorOf::kFit, ho))
        return st;
    ctx->has_factor = true;
    return refresh_operand(ctx, 0, ho);
}

// The tile cutoff of one sweep (sbo::SkipPlan): the fields every regime shares,
// then one branch per regime -- the probe's reference, the automatic cutoff of
// the fast and of the precise sweep (SBO_OPT_TILE_SKIP -1), the fixed cutoff.
sbo::SkipPlan skip_rule(const sbo_ctx *ctx, Sweep sweep) {
    const bool precise = sweep != Sweep::kFast;
    const bool split = !precise && ctx->opt.kernel_variant >= 2;
    sbo::SkipPlan s;
    s.prod_full = split ? 6 : 1;
    s.records = split;
    s.wide = precise;
    // the tile-norm test's tables (the automatic cutoffs)
    auto tile_norms = [&] {
        s.lgn = ctx->tile_lgn.as<float4>();
        s.colmax = ctx->tile_colmax.as<float>();
        s.kcoord = ctx->kcoord.as<float>();
    };
    if (sweep == Sweep::kProbeRef) {
        // the precise sweep under a budget of 2^-kProbeRefBits of the largest
        // variance the probe's fast sweep saw (probe_precision)
        skip_budget_for(ctx, ctx->probe_ref_tol, s.L, s.lg_tau_v);
        s.L_mean = ctx->auto_skip_mean_log2;
        tile_norms();
    } else if (ctx->opt.skip_log2 < 0 && !precise) {
        s.L = ctx->auto_skip_log2;
        s.L_mean = ctx->auto_skip_mean_log2;
        s.lg_tau_v = ctx->lg_tau_v;
        s.levels = sbo::x3_levels(ctx->opt.kernel_variant) ? 1 : 0;
        tile_norms();
    } else if (ctx->opt.skip_log2 < 0) {
        s.L = ctx->p_skip_log2;
        // the precise sweep's mean 2^8 tighter than the budget's 2^-B sf
        // (absolute): its tiles are the last row block's only, and the mean
        // of an ill-conditioned fit (large |alpha|_1) otherwise sits right at
        // its budget
        s.L_mean = std::min(160, ctx->auto_skip_mean_log2 + 8);
        s.lg_tau_v = ctx->p_lg_tau_v;
        tile_norms();
    } else {
        s.L = ctx->opt.skip_log2;
    }
    return s;
}

#ifdef SBO_DIAG
// The diagnostic build's environment overrides of a tick's plan,
// applied once to the finished rule.
void diag_skip_overrides(sbo::SkipPlan &s) {
    // timing diagnostic: the drop-only plan with every kept tile at level
    // SBO_LVL_FORCE -- outside the error budget
    if (const char *e = getenv("SBO_LVL_FORCE"); e && s.levels) s.levels = 2 + std::clamp(atoi(e), 0, 2);
    // the level increments' rank keys (SkipPlan::lvl_key), "k0,k1" -- re-calibration A/B
    if (const char *e = getenv("SBO_LVL_KEY")) (void)sscanf(e, "%f,%f", &s.lvl_key[0], &s.lvl_key[1]);
    // the reference plan builder: every pair's bounds evaluated in every
    // pass, empty items' partials written and read
    if (const char *e = getenv("SBO_PLAN_REF"); e && atoi(e)) {
        s.colmax = nullptr;
        s.zero_empty = true;
        s.ref_chain = true;
    }
}
#endif

// The plan's first half: what the request and the context's options decide
// before the queries are looked at.
sbo_status tick_plan(sbo_ctx *ctx, const TickRequest &rq, TickPlan &p) {
    const sbo_options &o = ctx->opt;
    const Sweep sweep = rq.sweep != Sweep::kCtx ? rq.sweep : ctx->precise ? Sweep::kPrecise : Sweep::kFast;
    SBO_CHECK(sweep == Sweep::kFast || (ctx->has_factor && inverse_current(ctx, ctx->n)),
              SBO_E_STATE, "precise sweep: needs the fit's f64 inverse (not an imported state, INVERSE_BITS 64)");
    const bool full = rq.want == TickWant::kTick;
    p.nI = ctx->npad / sbo::kBM;
    p.P = o.sweep_groups > 0 ? o.sweep_groups : std::max(1, ctx->num_cu);
    p.precise = sweep != Sweep::kFast;
    p.pk = precise_kernel_traits(o.precise_kernel);
    // plan only => row-block-major item order, unchunked, no counters
    p.chunked = full && p.precise && p.pk.table;
    p.prof = full && ctx->prof && !rq.quiet;
    p.skip = skip_rule(ctx, sweep);
    p.skip.order_blk = full && p.precise ? o.plan_block : 0;
    // (a chunk's plan is gone by the acquisition: its empty items' partials are written)
    p.skip.zero_empty = p.chunked;
#ifdef SBO_DIAG
    diag_skip_overrides(p.skip);
#endif
    return SBO_OK;
}

// The queries in sweep order: grid patches or Morton order (compact 128-query
// blocks skip more k-tiles), the request's own order where it brings one.
sbo_status tick_order_queries(sbo_ctx *ctx, const TickRequest &rq, TickPlan &p) {
    const float *qx = rq.qx, *qy = rq.qy;
    const int64_t m = rq.m;
    QueryOrder o{nullptr, qx, qy};
    int64_t ms = m;
    if (ctx->opt.query_order && p.skip.L > 0 && m > sbo::kBN) {
        int32_t *perm = nullptr;
        float *sx = nullptr, *sy = nullptr;
        if (ctx->opt.query_order == 1) {
            // a raster grid's shape, read once per query buffer (one stream
            // sync); the patch layout is valid for any data, so a reused
            // buffer holding other points still gets correct outputs
            SBO_HIP(ctx->qgwork.reserve(sbo::query_grid_bytes(m)));
            if (qx != ctx->qgrid_x || qy != ctx->qgrid_y || m != ctx->qgrid_m) {
                unsigned long long g[6];
                SBO_HIP(sbo::launch_grid_detect(ctx->stream, qx, qy, m, ctx->qgwork.as<void>(), g));
                sbo::grid_layout(g, m, ctx->qgrid);
                ctx->qgrid_x = qx;
                ctx->qgrid_y = qy;
                ctx->qgrid_m = m;
            }
        }
        if (ctx->opt.query_order == 1 && ctx->qgrid.ok) {
            SBO_HIP(sbo::launch_query_grid(ctx->stream, qx, qy, m, ctx->qgrid, ctx->qgwork.as<void>(), &perm, &sx,
                                           &sy));
            o = QueryOrder{perm, sx, sy};
            ms = ctx->qgrid.ms;
        } else if (rq.order.perm) {
            o = rq.order;    // (the probe's second sweep: the same queries, already ordered)
        } else {
            const size_t wb = sbo::query_order_bytes(m);
            SBO_HIP(ctx->qwork.reserve(wb));
            SBO_HIP(sbo::launch_query_order(ctx->stream, qx, qy, m, ctx->bbox, ctx->qwork.as<void>(), wb, &perm, &sx,
                                            &sy));
            o = QueryOrder{perm, sx, sy};
        }
    }
    p.ms = ms;
    p.nQ = (ms + sbo::kBN - 1) / sbo::kBN;
    p.ldp = sbo::round_up(ms, 64);
    p.perm = o.perm;
    p.qx = o.sx;
    p.qy = o.sy;
    return SBO_OK;
}

// The tick's workspaces: partials and mean, block keys, the plan.
sbo_status tick_reserve(sbo_ctx *ctx, const TickPlan &p) {
    const size_t pw = p.precise ? sizeof(double) : sizeof(float);   // the precise sweep's partials are f64
    SBO_HIP(ctx->part.reserve(pw * (size_t)p.nI * (size_t)p.ldp));
    SBO_HIP(ctx->mean.reserve(pw * (size_t)p.ldp));
    SBO_HIP(ctx->keys.reserve(sizeof(sbo_key) * (size_t)(sbo::acq_blocks(p.ms) + 1)));
    // the plan's tile lists and step records are sized for the dense sweep
    // (every tile of every item) and indexed by 32-bit list positions
    // (predict_x3.hip reads an item's first entry from desc.z alone)
    SBO_CHECK((double)2 * p.nI * (p.nI + 1) * (double)p.nQ < 4294967296.0, SBO_E_INVAL,
              "sbo_tick: N x M too large for one tick plan (2 nI (nI + 1) nQ >= 2^32 tile entries); "
              "split the queries into shards");
    SBO_HIP(ctx->plan_work.reserve(sbo::predict_work_bytes(ctx->npad, p.ms, p.P)));
    return SBO_OK;
}

// The plan of mc sweep positions from c0 on (all of them, or one chunk), in plan_work.
sbo_status tick_build_plan(sbo_ctx *ctx, const TickPlan &p, int64_t c0, int64_t mc) {
    // (an f64 plan writes its empty items' outputs as doubles: SkipPlan::wide)
    const size_t pw = p.precise ? sizeof(double) : sizeof(float);
    SBO_HIP(sbo::launch_plan(ctx->stream, ctx->kbox.as<float4>(), ctx->npad, p.qx + c0, p.qy + c0, mc, p.ldp,
                             (float)ctx->hyper.length_scale, (float)ctx->hyper.prior_mean, p.skip,
                             reinterpret_cast<float *>(ctx->part.as<char>() + pw * (size_t)c0),
                             reinterpret_cast<float *>(ctx->mean.as<char>() + pw * (size_t)c0),
                             p.prof ? ctx->counters.as<unsigned long long>() : nullptr, p.P,
                             ctx->plan_work.as<void>(), ctx->plan_work.capacity()));
    return SBO_OK;
}

// sbo_query_cost: the plan's work per query, no sweep.
sbo_status tick_cost(sbo_ctx *ctx, const TickPlan &p, float *cost) {
    SBO_HIP(ctx->ws.qcost.reserve(sizeof(float) * (size_t)p.nQ));
    SBO_HIP(sbo::launch_plan_cost(ctx->stream, ctx->npad, p.ms, p.P, ctx->plan_work.as<void>(), p.perm,
                                  ctx->ws.qcost.as<float>(), cost));
    return SBO_OK;
}

// The precise operand up to date on ctx->stream: the fit's pack may still be
// running on aux_stream, and row blocks repacked since (or all of them, after
// a change of SBO_OPT_PRECISE_KERNEL's layout) are derived from the f64 inverse.
sbo_status precise_operand(sbo_ctx *ctx, const TickPlan &p) {
    if (sbo_status st = ctx->pop.wait_on(ctx, ctx->stream)) return st;
    return ctx->pop.update(ctx, p.nI * sbo::kBM, ctx->stream);
}

// The int8 sweep over mc positions (nq query blocks) from c0 on under the plan
// in plan_work; a chunked plan's sweep reads the K* table of those blocks in kzt.
sbo_status launch_oz(sbo_ctx *ctx, const TickPlan &p, int64_t c0, int64_t mc, int64_t nq) {
    const int4 *desc = nullptr;
    const unsigned short *tl = nullptr;
    const int *seg = nullptr;
    sbo::plan_views(ctx->npad, mc, p.P, ctx->plan_work.as<void>(), &desc, &tl, &seg);
    SBO_HIP(sbo::launch_predict_oz(ctx->stream, ctx->pop.aoz.as<char>(), ctx->pop.eoz.as<int>(),
                                   ctx->pop.koz.as<char>(), desc, tl, seg, p.P, (int)(p.nI * nq), (int)p.nI, p.qx + c0,
                                   p.qy + c0, mc, p.ldp, ctx->hyper.length_scale, ctx->hyper.prior_mean,
                                   ctx->part.as<double>() + c0, ctx->mean.as<double>() + c0, ctx->opt.precise_kernel,
                                   p.chunked ? ctx->ws.kzt.as<char>() : nullptr));
    return SBO_OK;
}

// SBO_OPT_PRECISE_KERNEL 3: the queries in chunks of Qc blocks -- each
// chunk's plan, its K* table (every k-tile of its query blocks, once) and the
// sweep reading it; the table is sized by SBO_OPT_TABLE_MB (2 GiB: a
// 10^6-point grid at N = 16384 runs in 33 chunks of 244 query blocks).  An
// item's result does not depend on the chunking (plans are per query block).
sbo_status sweep_precise_chunked(sbo_ctx *ctx, const TickPlan &p) {
    const size_t per_qb = sbo::oz_table_bytes(ctx->npad, p.pk.pairs);
    size_t budget = (size_t)ctx->opt.table_mb << 20;
    if (budget == 0) {
        // auto: 1/32 of the free device memory, within [256 MiB, 8 GiB]
        // (8 GiB: 9 chunks on the lpsc grid, 1.4 % faster than 2 GiB's 33)
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = size_t(64) << 30;
        budget = std::clamp(fr / 32 + ctx->ws.kzt.capacity() / 32, size_t(256) << 20, size_t(8) << 30);
    }
    const int64_t Qc = std::clamp<int64_t>((int64_t)(budget / per_qb), 1, p.nQ);
    SBO_HIP(ctx->ws.kzt.reserve(per_qb * (size_t)Qc));
    Bracket br(ctx, ctx->ev_predict, p.prof);
    for (int64_t qb0 = 0; qb0 < p.nQ; qb0 += Qc) {
        const int64_t c0 = qb0 * sbo::kBN, mc = std::min<int64_t>(Qc * sbo::kBN, p.ms - c0);
        const int64_t nq = std::min(Qc, p.nQ - qb0);
        if (sbo_status st = tick_build_plan(ctx, p, c0, mc)) return st;
        SBO_HIP(sbo::launch_kstar_table(ctx->stream, ctx->pop.koz.as<char>(), p.qx + c0, p.qy + c0, mc, ctx->npad,
                                        ctx->hyper.length_scale, nq, ctx->ws.kzt.as<char>(), p.pk.pairs));
        if (sbo_status st = launch_oz(ctx, p, c0, mc, nq)) return st;
    }
    return SBO_OK;
}

// The precise sweep over the whole plan: the int8 sliced kernel or the f64 one.
sbo_status sweep_precise(sbo_ctx *ctx, const TickPlan &p) {
    Bracket br(ctx, ctx->ev_predict, p.prof);
    if (p.pk.int8) return launch_oz(ctx, p, 0, p.ms, p.nQ);
    const int4 *desc = nullptr;
    const unsigned short *tl = nullptr;
    const int *seg = nullptr;
    sbo::plan_views(ctx->npad, p.ms, p.P, ctx->plan_work.as<void>(), &desc, &tl, &seg);
    SBO_HIP(sbo::launch_predict_f64(ctx->stream, ctx->pop.a64.as<double>(), ctx->pop.kc64.as<double>(), desc, tl, seg,
                                    p.P, (int)(p.nI * p.nQ), (int)p.nI, p.qx, p.qy, p.ms, p.ldp, ctx->hyper.length_scale,
                                    ctx->hyper.prior_mean, ctx->part.as<double>(), ctx->mean.as<double>()));
    return SBO_OK;
}

// The split-operand sweep: derive the bf16 planes of any repacked row block,
// and give the kernel whole 128-query blocks to read (m: the caller's queries).
sbo_status sweep_fast_x3(sbo_ctx *ctx, const TickPlan &p, int64_t m) {
    if (sbo_status st = derive_x3(ctx)) return st;
    const float *qx = p.qx, *qy = p.qy;
    if (!p.perm) {
        const int64_t mp = sbo::round_up(m, sbo::kBN);
        SBO_HIP(ctx->qpad.reserve(sizeof(float) * 2 * (size_t)mp));
        float *px = ctx->qpad.as<float>(), *py = px + mp;
        SBO_HIP(hipMemcpyAsync(px, qx, sizeof(float) * (size_t)m, hipMemcpyDeviceToDevice, ctx->stream));
        SBO_HIP(hipMemcpyAsync(py, qy, sizeof(float) * (size_t)m, hipMemcpyDeviceToDevice, ctx->stream));
        qx = px;
        qy = py;
    }
    const int4 *desc = nullptr;
    const unsigned short *tl = nullptr;
    const int *seg = nullptr;
    const int4 *rec = nullptr;
    sbo::plan_views(ctx->npad, p.ms, p.P, ctx->plan_work.as<void>(), &desc, &tl, &seg, &rec);
    Bracket br(ctx, ctx->ev_predict, p.prof);
    SBO_HIP(sbo::launch_predict_x3(ctx->stream, ctx->split.ax3.as<char>(), ctx->split.kc3.as<float>(), desc, rec, seg,
                                   p.P, (int)(p.nI * p.nQ), (int)p.nI, qx, qy, p.ms, p.ldp,
                                   sbo::exp2_coef_f((float)ctx->hyper.length_scale), (float)ctx->hyper.prior_mean,
                                   ctx->part.as<float>(), ctx->mean.as<float>(), ctx->opt.kernel_variant));
    return SBO_OK;
}

sbo_status sweep_fast_f32(sbo_ctx *ctx, const TickPlan &p) {
    Bracket br(ctx, ctx->ev_predict, p.prof);
    SBO_HIP(sbo::launch_predict(ctx->stream, ctx->aug.as<float>(), ctx->kcoord.as<float>(), ctx->npad, p.qx, p.qy,
                                p.ms, p.ldp, (float)ctx->hyper.length_scale, (float)ctx->hyper.prior_mean,
                                ctx->part.as<float>(), ctx->mean.as<float>(), ctx->opt.kernel_variant, p.P,
                                ctx->plan_work.as<void>()));
    return SBO_OK;
}

// The acquisition over the partials and the key reduction.  The plan's
// non-empty view only where the plan outlives the sweep (SkipPlan::zero_empty).
sbo_status tick_acquire(sbo_ctx *ctx, const TickRequest &rq, const TickPlan &p) {
    const unsigned long long *pkey = nullptr, *pscan = nullptr, *nonempty = nullptr;
    const unsigned char *pthr = nullptr;
    if (!p.skip.zero_empty)
        sbo::plan_item_views(ctx->npad, p.ms, p.P, ctx->plan_work.as<void>(), &pkey, &pscan, &pthr, &nonempty);
    const int64_t nb = sbo::acq_blocks(p.ms);
    sbo_key *bkeys = ctx->keys.as<sbo_key>();
    const double sf2 = ctx->hyper.sigma_f * ctx->hyper.sigma_f;
    double *kmu = rq.keep ? ctx->keep.mu64.as<double>() : nullptr;
    double *kvar = rq.keep ? ctx->keep.var64.as<double>() : nullptr;
    if (p.precise)
        SBO_HIP(sbo::launch_acquire(ctx->stream, ctx->part.as<double>(), ctx->mean.as<double>(), (int)p.nI, p.ldp,
                                    p.ms, sf2, rq.beta, rq.f_min, rq.score, rq.index_offset, p.perm, rq.mu, rq.sd,
                                    rq.lo, rq.hi, rq.safe, bkeys, nonempty, kmu, kvar));
    else
        SBO_HIP(sbo::launch_acquire(ctx->stream, ctx->part.as<float>(), ctx->mean.as<float>(), (int)p.nI, p.ldp,
                                    p.ms, (float)sf2, rq.beta, rq.f_min, rq.score, rq.index_offset, p.perm, rq.mu,
                                    rq.sd, rq.lo, rq.hi, rq.safe, bkeys, nonempty, kmu, kvar));
    SBO_HIP(sbo::launch_reduce_keys(ctx->stream, bkeys, nb, rq.key ? rq.key : bkeys + nb));
    return SBO_OK;
}

// The kept posterior's buffers for a full sweep of p (sbo_tick_stream), and,
// after the acquisition wrote mu64 / var64, its sweep order, block boxes and
// bookkeeping.  The state counts as kept only once both ran.
sbo_status stream_reserve(sbo_ctx *ctx, const TickPlan &p) {
    sbo::StreamKeep &k = ctx->keep;
    k.valid = false;
    const size_t ms = (size_t)p.ms;
    SBO_HIP(k.mu64.reserve(sizeof(double) * ms));
    SBO_HIP(k.var64.reserve(sizeof(double) * ms));
    SBO_HIP(k.qx.reserve(sizeof(float) * ms));
    SBO_HIP(k.qy.reserve(sizeof(float) * ms));
    SBO_HIP(k.perm.reserve(sizeof(int32_t) * ms));
    SBO_HIP(k.qbox.reserve(sizeof(float4) * (size_t)p.nQ));
    SBO_HIP(k.head.reserve(sizeof(sbo::StreamHead) + sizeof(unsigned long long)));
    // (padded positions, perm < 0, are never written by the acquisition and never read by anyone)
    return SBO_OK;
}
sbo_status stream_capture(sbo_ctx *ctx, const TickRequest &rq, const TickPlan &p) {
    sbo::StreamKeep &k = ctx->keep;
    SBO_HIP(sbo::launch_stream_keep(ctx->stream, p.qx, p.qy, p.perm, p.ms, k.qx.as<float>(), k.qy.as<float>(),
                                    k.perm.as<int32_t>(), k.qbox.as<float4>()));
    k.m = rq.m;
    k.ms = p.ms;
    k.n_map = ctx->n;
    k.epoch = ctx->fit_epoch;
    k.precise = p.precise;
    k.err_var = k.err_mean = 0.0;
    k.updates = 0;
    k.valid = true;
    k.was_reset = false;
    return SBO_OK;
}

// Plan, sweep and acquisition over queries already on the device (or the
// plan alone, or the plan and its cost: TickWant); plan_out, where given,
// receives the plan as built (plan_views / plan_item_views of ms and P on
// plan_work read an unchunked one).
sbo_status run_tick(sbo_ctx *ctx, const TickRequest &rq, TickPlan *plan_out) {
    TickPlan p;
    if (sbo_status st = tick_plan(ctx, rq, p)) return st;
    if (sbo_status st = tick_order_queries(ctx, rq, p)) return st;
    if (sbo_status st = tick_reserve(ctx, p)) return st;
    // (the K* table's precise sweep plans each chunk of query blocks itself)
    if (!p.chunked)
        if (sbo_status st = tick_build_plan(ctx, p, 0, p.ms)) return st;
    if (plan_out) *plan_out = p;
    if (rq.want == TickWant::kPlan) return SBO_OK;
    if (rq.want == TickWant::kCost) return tick_cost(ctx, p, rq.cost);
    sbo_status st;
    if (p.precise) {
        st = precise_operand(ctx, p);
        if (st == SBO_OK) st = p.chunked ? sweep_precise_chunked(ctx, p) : sweep_precise(ctx, p);
    } else if (ctx->opt.kernel_variant >= 2) {
        st = sweep_fast_x3(ctx, p, rq.m);
    } else {
        st = sweep_fast_f32(ctx, p);
    }
    if (st != SBO_OK) return st;
    if (!rq.keep) return tick_acquire(ctx, rq, p);
    if ((st = stream_reserve(ctx, p)) != SBO_OK) return st;
    if ((st = tick_acquire(ctx, rq, p)) != SBO_OK) return st;
    return stream_capture(ctx, rq, p);
}

// ------------------------------------------------------------ streaming tick
static_assert(sizeof(sbo_stream_info) == 96, "sbo_stream_info: the bindings mirror this layout");

// The skip budget of the sweep in effect (absolute, on any variance / mean):
// skip_budget_for's tolerance of the fast sweep and of the precise plan
// (precise_budget).  (Declared in sbo_host.hpp: sbo_whatif spends it too.)
}  // namespace
void stream_budget(const sbo_ctx *ctx, double &var, double &mean) {
    const double sf2 = ctx->hyper.sigma_f * ctx->hyper.sigma_f;
    const double share = std::ldexp(1.0, -ctx->opt.skip_budget);
    var = share * (ctx->precise ? std::min(std::max(ctx->probe_vmin, 1e-12 * sf2), sf2) : sf2);
    mean = share * std::sqrt(sf2);
}
namespace {

// Worst-case effect of dropping K* entries below 2^-L on an update over rows
// whose 1-norms give sum_l1sq and sum_l1z (sbo::StreamHead): with
// d_r = sf2 2^-L |L^-1_r|_1 bounding |dv_r|, and |v|_2^2 <= var_old <= sf2,
//   |d var| <= 2 sqrt(sf2) |d|_2 + |d|_2^2,   |d mu| <= sum_r d_r |z_r|.
void stream_bounds(double sf2, int L, const sbo::StreamHead &h, double &var, double &mean) {
    const double s = sf2 * std::ldexp(1.0, -L), d2 = s * s * h.sum_l1sq;
    var = 2.0 * std::sqrt(sf2) * std::sqrt(d2) + d2;
    mean = s * h.sum_l1z;
}

// The cutoff of one update and the bounds it spends: the context's fixed
// cutoff, or (SBO_OPT_TILE_SKIP -1) the smallest L whose bounds stay within
// 2^-SBO_OPT_STREAM_SHARE of the budget.  L = 0: dense (also where only
// L >= 150 would do, which drops nothing but exact zeros).
int stream_cutoff(const sbo_ctx *ctx, const sbo::StreamHead &h, double budget_var, double budget_mean, double &var,
                  double &mean) {
    const double sf2 = ctx->hyper.sigma_f * ctx->hyper.sigma_f;
    var = mean = 0.0;
    if (ctx->opt.skip_log2 >= 0) {
        if (ctx->opt.skip_log2 > 0 && ctx->opt.skip_log2 < 150) stream_bounds(sf2, ctx->opt.skip_log2, h, var, mean);
        return ctx->opt.skip_log2;
    }
    const double share = std::ldexp(1.0, -ctx->opt.stream_share);
    for (int L = 16; L < 150; ++L) {
        stream_bounds(sf2, L, h, var, mean);
        if (var <= share * budget_var && mean <= share * budget_mean) return L;
    }
    var = mean = 0.0;
    return 0;
}

// One sbo_tick_stream call: the report it leaves (info.reason is the verdict so
// far), and for an update the cutoff and the bounds it spends.
struct StreamTurn {
    sbo_stream_info info{};
    int64_t R = 0;   // rows appended since the kept posterior was computed
    int L = 0;
    double spend_var = 0.0, spend_mean = 0.0;
};

// The part of the path decision that needs no device (include/sbo.h), in its order.
int stream_decide(const sbo_ctx *ctx, int64_t m, int64_t R) {
    const sbo::StreamKeep &k = ctx->keep;
    if (!k.valid) return k.was_reset ? SBO_STREAM_RESET : SBO_STREAM_FIRST;
    if (k.epoch != ctx->fit_epoch || k.precise != ctx->precise) return SBO_STREAM_REFIT;
    if (k.m != m) return SBO_STREAM_QUERIES_CHANGED;
    if (!(fit_state_complete(ctx, ctx->n) && R >= 0)) return SBO_STREAM_NO_INVERSE;
    if (R > ctx->opt.stream_max_rows) return SBO_STREAM_ROWS_OVER_CAP;
    return SBO_STREAM_UPDATED;
}

// The queries against the kept ones and the appended rows' norms (one readback,
// one sync), then the cutoff and whether the budget still covers its bounds.
sbo_status stream_read_head(sbo_ctx *ctx, const TickRequest &rq, StreamTurn &t) {
    sbo::StreamKeep &k = ctx->keep;
    sbo::StreamHead h{};
    sbo::StreamHead *dh = k.head.as<sbo::StreamHead>();
    SBO_HIP(hipMemsetAsync(dh, 0, sizeof(sbo::StreamHead) + sizeof(unsigned long long), ctx->stream));
    SBO_HIP(sbo::launch_stream_compare(ctx->stream, rq.qx, rq.qy, k.qx.as<float>(), k.qy.as<float>(),
                                       k.perm.as<int32_t>(), k.ms, dh));
    if (t.R > 0) {
        SBO_HIP(k.l1.reserve(sbo::update_l1_bytes(t.R)));
        SBO_HIP(sbo::launch_update_bound_sums(ctx->stream, ctx->Linv.as<double>(), ctx->cap, k.n_map, ctx->n,
                                              ctx->zvec.as<double>(), k.l1.as<double>(), dh));
    }
    SBO_HIP(hipMemcpyAsync(&h, dh, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    if (h.mismatch) {
        t.info.reason = SBO_STREAM_QUERIES_CHANGED;
    } else if (t.R > 0) {
        t.L = stream_cutoff(ctx, h, t.info.budget_var, t.info.budget_mean, t.spend_var, t.spend_mean);
        if (k.err_var + t.spend_var > t.info.budget_var || k.err_mean + t.spend_mean > t.info.budget_mean)
            t.info.reason = SBO_STREAM_BUDGET;
    }
    return SBO_OK;
}

// Path 0: the full tick, its posterior kept.
sbo_status stream_fallback(sbo_ctx *ctx, TickRequest rq, StreamTurn &t) {
    rq.keep = true;
    if (sbo_status st = run_tick(ctx, rq)) return st;
    t.info.path = 0;
    ctx->keep.last = t.info;
    return SBO_OK;
}

// Path 1: the rank-R update of the kept posterior, the acquisition from it,
// and the kept state's bookkeeping.
sbo_status stream_update(sbo_ctx *ctx, const TickRequest &rq, StreamTurn &t) {
    sbo::StreamKeep &k = ctx->keep;
    const int64_t n = ctx->n;
    sbo::StreamHead *dh = k.head.as<sbo::StreamHead>();
    const int64_t nb = sbo::acq_blocks(k.ms);
    SBO_HIP(ctx->keys.reserve(sizeof(sbo_key) * (size_t)(nb + 1)));
    if (t.R > 0) {
        const double sf2 = ctx->hyper.sigma_f * ctx->hyper.sigma_f;
        Bracket br(ctx, ctx->ev_predict);
        SBO_HIP(sbo::launch_predict_update(ctx->stream, ctx->Linv.as<double>(), ctx->cap, k.n_map, n,
                                           ctx->zvec.as<double>(), ctx->x.as<float>(), ctx->y.as<float>(),
                                           ctx->kbox.as<float4>(), k.qbox.as<float4>(), k.qx.as<float>(),
                                           k.qy.as<float>(), k.perm.as<int32_t>(), k.ms, ctx->hyper.length_scale, sf2,
                                           t.L, k.mu64.as<double>(), k.var64.as<double>(),
                                           reinterpret_cast<unsigned long long *>(dh + 1)));
        t.info.tiles_total = kept_tiles_total(k.ms, n);
    }
    sbo_key *bkeys = ctx->keys.as<sbo_key>();
    SBO_HIP(sbo::launch_acquire_kept(ctx->stream, k.mu64.as<double>(), k.var64.as<double>(), k.ms, rq.beta, rq.f_min,
                                     rq.score, rq.index_offset, k.perm.as<int32_t>(), rq.mu, rq.sd, rq.lo, rq.hi,
                                     rq.safe, bkeys));
    SBO_HIP(sbo::launch_reduce_keys(ctx->stream, bkeys, nb, rq.key ? rq.key : bkeys + nb));
    k.n_map = n;
    k.err_var += t.spend_var;
    k.err_mean += t.spend_mean;
    ++k.updates;
    t.info.path = 1;
    t.info.cutoff_log2 = t.L;
    k.last = t.info;
    return SBO_OK;
}

// sbo_tick_stream over queries already on the device: the path decision
// (include/sbo.h), then either the update of the kept posterior and the
// acquisition from it, or run_tick with the capture.
sbo_status run_tick_stream(sbo_ctx *ctx, TickRequest rq) {
    const sbo::StreamKeep &k = ctx->keep;
    StreamTurn t;
    t.R = k.valid ? ctx->n - k.n_map : 0;
    t.info.struct_size = (uint32_t)sizeof(t.info);
    t.info.m = rq.m;
    t.info.rows = std::max<int64_t>(t.R, 0);
    t.info.n_map = k.valid ? k.n_map : 0;
    stream_budget(ctx, t.info.budget_var, t.info.budget_mean);
    t.info.reason = stream_decide(ctx, rq.m, t.R);
    if (t.info.reason == SBO_STREAM_UPDATED)
        if (sbo_status st = stream_read_head(ctx, rq, t)) return st;
    return t.info.reason == SBO_STREAM_UPDATED ? stream_update(ctx, rq, t) : stream_fallback(ctx, rq, t);
}

// Host queries staged for a tick: hq sized for them and `rest` more bytes,
// the two coordinate arrays carved first and copied over on ctx->stream; the
// caller carves its outputs from c.
sbo_status stage_queries(sbo_ctx *ctx, const float *qx, const float *qy, int64_t m, size_t rest, TickRequest &rq,
                         Carve &c) {
    SBO_HIP(ctx->hq.reserve(Carve::need(m, 4) * 2 + rest));
    c = Carve(ctx->hq.as<void>());
    float *dqx = c.take<float>(m), *dqy = c.take<float>(m);
    SBO_HIP(hipMemcpyAsync(dqx, qx, sizeof(float) * m, hipMemcpyHostToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(dqy, qy, sizeof(float) * m, hipMemcpyHostToDevice, ctx->stream));
    rq.qx = dqx;
    rq.qy = dqy;
    return SBO_OK;
}

}  // namespace

namespace {
// ComputeSets on f32 (the tick's own outputs) or f64 (the node's mu_/std_)
template <typename T>
sbo_status compute_sets_impl(sbo_ctx *ctx, const T *mu, const T *sd, int64_t m, double beta, double f_min,
                             double *lo, double *hi, uint8_t *safe, uint32_t flags) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(mu && sd, SBO_E_INVAL, "sbo_compute_sets: null mu/sd");
    SBO_CHECK(m >= 0, SBO_E_INVAL, "sbo_compute_sets: m must be >= 0");
    if (m == 0) return SBO_OK;
    SBO_HIP(hipSetDevice(ctx->device));
    if (dev(flags)) {
        SBO_HIP(sbo::launch_sets(ctx->stream, mu, sd, m, beta, f_min, lo, hi, safe));
        return finish(ctx, flags);
    }
    const size_t need = Carve::need(m, sizeof(T)) * 2 + Carve::need(m, 8) * 2 + Carve::need(m, 1);
    SBO_HIP(ctx->hq.reserve(need));
    Carve c(ctx->hq.as<void>());
    T *dmu = c.take<T>(m), *dsd = c.take<T>(m);
    double *dlo = c.take<double>(m), *dhi = c.take<double>(m);
    uint8_t *ds = c.take<uint8_t>(m);
    SBO_HIP(hipMemcpyAsync(dmu, mu, sizeof(T) * m, hipMemcpyHostToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(dsd, sd, sizeof(T) * m, hipMemcpyHostToDevice, ctx->stream));
    SBO_HIP(sbo::launch_sets(ctx->stream, (const T *)dmu, (const T *)dsd, m, beta, f_min, lo ? dlo : nullptr,
                             hi ? dhi : nullptr, safe ? ds : nullptr));
    if (lo) SBO_HIP(hipMemcpyAsync(lo, dlo, sizeof(double) * m, hipMemcpyDeviceToHost, ctx->stream));
    if (hi) SBO_HIP(hipMemcpyAsync(hi, dhi, sizeof(double) * m, hipMemcpyDeviceToHost, ctx->stream));
    if (safe) SBO_HIP(hipMemcpyAsync(safe, ds, m, hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    return SBO_OK;
}
}  // namespace

extern "C" {

SBO_API const char *sbo_version(void) { return kVersion; }

SBO_API const char *sbo_status_string(sbo_status s) {
    switch (s) {
        case SBO_OK: return "SBO_OK";
        case SBO_E_INVAL: return "SBO_E_INVAL";
        case SBO_E_NOT_SPD: return "SBO_E_NOT_SPD";
        case SBO_E_DEVICE: return "SBO_E_DEVICE";
        case SBO_E_OOM: return "SBO_E_OOM";
        case SBO_E_EMPTY: return "SBO_E_EMPTY";
        case SBO_E_STATE: return "SBO_E_STATE";
    }
    return "SBO_E_UNKNOWN";
}

SBO_API sbo_status sbo_create(int device, sbo_ctx **out) {
    if (!out) return SBO_E_INVAL;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return SBO_E_DEVICE;
    sbo_ctx *ctx = new (std::nothrow) sbo_ctx();
    if (!ctx) return SBO_E_OOM;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess ||
        rocblas_create_handle(&ctx->blas) != rocblas_status_success ||
        hipHostMalloc(reinterpret_cast<void **>(&ctx->host_key), sizeof(sbo_key)) != hipSuccess ||
        ctx->info.reserve(256) != hipSuccess ||
        hipDeviceGetAttribute(&ctx->num_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
        sbo_destroy(ctx);
        return SBO_E_DEVICE;
    }
    ctx->stream = ctx->own_stream;
    rocblas_set_stream(ctx->blas, ctx->stream);
    *out = ctx;
    return SBO_OK;
}

SBO_API void sbo_destroy(sbo_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    recycle_events(ctx);
    for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
    if (ctx->aux_stream) (void)hipStreamSynchronize(ctx->aux_stream);
    if (ctx->ev_panel) (void)hipEventDestroy(ctx->ev_panel);
    if (ctx->ev_trail) (void)hipEventDestroy(ctx->ev_trail);
    if (ctx->ev_pack) (void)hipEventDestroy(ctx->ev_pack);
    if (ctx->pop.ev) (void)hipEventDestroy(ctx->pop.ev);
    if (ctx->blas_aux) rocblas_destroy_handle(ctx->blas_aux);
    if (ctx->aux_stream) (void)hipStreamDestroy(ctx->aux_stream);
    if (ctx->inv_stream) (void)hipStreamSynchronize(ctx->inv_stream);
    if (ctx->ev_half) (void)hipEventDestroy(ctx->ev_half);
    if (ctx->ev_inv) (void)hipEventDestroy(ctx->ev_inv);
    if (ctx->blas_inv) rocblas_destroy_handle(ctx->blas_inv);
    if (ctx->inv_stream) (void)hipStreamDestroy(ctx->inv_stream);
    if (ctx->chk_stream) (void)hipStreamSynchronize(ctx->chk_stream);
    if (ctx->ev_chk0) (void)hipEventDestroy(ctx->ev_chk0);
    if (ctx->ev_chk1) (void)hipEventDestroy(ctx->ev_chk1);
    if (ctx->chk_stream) (void)hipStreamDestroy(ctx->chk_stream);
    if (ctx->blas) rocblas_destroy_handle(ctx->blas);
    if (ctx->host_key) (void)hipHostFree(ctx->host_key);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

SBO_API sbo_status sbo_set_stream(sbo_ctx *ctx, void *hip_stream) {
    if (!ctx) return SBO_E_INVAL;
    ctx->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    SBO_BLAS(rocblas_set_stream(ctx->blas, ctx->stream));
    return SBO_OK;
}

SBO_API const char *sbo_last_error(const sbo_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

SBO_API int64_t sbo_num_train(const sbo_ctx *ctx) { return ctx && ctx->fitted ? ctx->n : 0; }

namespace {
// Fill K of the ctx->n staged points (lda = ctx->cap) and factor it, with the
// SBO_OPT_JITTER_RETRIES policy: a factorization that fails (NOT_SPD) is
// retried up to R times with sf2 * 10^(r-7) added to the diagonal (r = 1..R);
// the jitter that succeeded stays part of the noise term, so appends and
// exported state use the same K (sbo_get_jitter).  base_noise: the noise
// variance without jitter.
sbo_status fill_and_factor(sbo_ctx *ctx, double base_noise) {
    const int64_t n = ctx->n;
    ++ctx->fit_epoch;   // a model from scratch (sbo_fit, the append's re-sort, each jitter retry)
    ctx->probe_n = 0;   // new data: the precision probe runs again (appends re-probe by growth)
    const double sf2 = ctx->hyper.sigma_f * ctx->hyper.sigma_f;
    ctx->jitter = 0.0;
    for (int r = 0;; ++r) {
        const double jit = r == 0 ? 0.0 : sf2 * std::pow(10.0, r - 7);
        {
            Bracket br(ctx, ctx->ev_fill);
            SBO_HIP(sbo::launch_rbf_fill(ctx->stream, ctx->x.as<float>(), ctx->y.as<float>(), n, ctx->x.as<float>(),
                                         ctx->y.as<float>(), n, ctx->cap, (float)ctx->hyper.length_scale, (float)sf2,
                                         (float)(base_noise + jit), true, ctx->L.as<float>()));
        }
        ctx->hyper.noise_level = base_noise + jit;
        const sbo_status st = factor_and_refresh(ctx);
        if (st == SBO_OK) {
            ctx->jitter = jit;
            ctx->n_sorted = n;
            ctx->removed_since_sort = 0;
            return SBO_OK;
        }
        ctx->hyper.noise_level = base_noise;
        if (st != SBO_E_NOT_SPD || r >= ctx->opt.jitter_retries) return st;
        drain_guard(ctx);   // (the retry rewrites L)
    }
}

// SBO_OPT_RESORT: the points appended since the last k-d sort (n - n_sorted)
// and those removed since then exceed resort_pct % of the sorted ones
bool resort_due(const sbo_ctx *ctx, int64_t n, int64_t n_sorted, int64_t removed) {
    return ctx->opt.resort_pct > 0 && ctx->opt.spatial_order != 0 &&
           (n - n_sorted + removed) * 100 > n_sorted * ctx->opt.resort_pct;
}

// sbo_append's re-sort (SBO_OPT_RESORT): all n0 + b points staged again in
// k-d order and factored from scratch, the caller's indices kept
// (order[i] = the caller index of internal row i, appends numbered after
// the fit).  Appended batches are k-d sorted only among themselves, so a
// stream of scattered batches leaves k-tiles whose boxes span the domain and
// defeat the sweep's tile skipping (C5: 50 batches of ~143 uniform points);
// re-sorting once the unsorted tail exceeds a share of N restores compact
// tiles for a fit amortised over that many appends.
sbo_status resort_append(sbo_ctx *ctx, const float *x, const float *y, const float *obs, int64_t b, uint32_t flags) {
    const int64_t n0 = ctx->n, n1 = n0 + b;
    SBO_HIP(ctx->ws.restage.reserve(sizeof(float) * 3 * (size_t)n1));
    float *tx = ctx->ws.restage.as<float>(), *ty = tx + n1, *to = ty + n1;
    const hipMemcpyKind k = dev(flags) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    SBO_HIP(hipMemcpyAsync(tx, ctx->x.as<float>(), sizeof(float) * n0, hipMemcpyDeviceToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(ty, ctx->y.as<float>(), sizeof(float) * n0, hipMemcpyDeviceToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(to, ctx->obs.as<float>(), sizeof(float) * n0, hipMemcpyDeviceToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(tx + n0, x, sizeof(float) * b, k, ctx->stream));
    SBO_HIP(hipMemcpyAsync(ty + n0, y, sizeof(float) * b, k, ctx->stream));
    SBO_HIP(hipMemcpyAsync(to + n0, obs, sizeof(float) * b, k, ctx->stream));
    std::vector<int64_t> prev(ctx->order.begin(), ctx->order.begin() + n0);
    for (int64_t i = n0; i < n1; ++i) prev.push_back(i);
    if (n1 > ctx->cap) {  // geometric growth, as the block append does (contents are rebuilt)
        const int64_t ncap = std::max<int64_t>(n1, sbo::round_up(ctx->cap + ctx->cap / 2, 256));
        SBO_HIP(hipStreamSynchronize(ctx->stream));
        ctx->x.release();
        ctx->y.release();
        ctx->obs.release();
        ctx->L.release();
        ctx->Linv.release();
        SBO_HIP(ctx->x.reserve(sizeof(float) * ncap));
        SBO_HIP(ctx->y.reserve(sizeof(float) * ncap));
        SBO_HIP(ctx->obs.reserve(sizeof(float) * ncap));
        SBO_HIP(ctx->alpha.reserve(sizeof(float) * ncap));
        SBO_HIP(ctx->L.reserve(sizeof(float) * (size_t)ncap * (size_t)ncap));
        ctx->cap = ncap;
    }
    ctx->n = n1;
    ctx->linv_n = 0;
    if (sbo_status st = stage_training(ctx, tx, ty, to, n1, 0, 0, SBO_DEVICE_PTRS)) return st;
    for (int64_t i = 0; i < n1; ++i) ctx->order[(size_t)i] = prev[(size_t)ctx->order[(size_t)i]];
    return fill_and_factor(ctx, ctx->hyper.noise_level - ctx->jitter);
}

// sbo_append's block update of the lower factor (column-major, lda = cap), n0
// points there and b staged behind them:
//   [L11  0 ]   K21 = k(Xnew, X)  -> L21 = K21 L11^-T        (append_panel)
//   [L21 L22]   K22 = k(Xnew, Xnew) + sn2 I - L21 L21^T      (append_schur)
//               L22 = chol(K22)                              (factor_block)
// L21: rows n0.., columns 0..n0-1; L22: rows n0.., columns n0..
float *append_L21(const sbo_ctx *ctx, int64_t n0) { return ctx->L.as<float>() + n0; }
float *append_L22(const sbo_ctx *ctx, int64_t n0) { return ctx->L.as<float>() + n0 + n0 * ctx->cap; }

// Storage for n1 > cap points: geometric growth that keeps the points, the
// factor and, where the incremental refresh will use it, the f64 inverse.
sbo_status append_grow(sbo_ctx *ctx, int64_t n1) {
    const int64_t n0 = ctx->n;
    const int64_t ncap = std::max<int64_t>(n1, sbo::round_up(ctx->cap + ctx->cap / 2, 256));
    DevBuf nx, ny, no, nL;
    SBO_HIP(nx.reserve(sizeof(float) * ncap));
    SBO_HIP(ny.reserve(sizeof(float) * ncap));
    SBO_HIP(no.reserve(sizeof(float) * ncap));
    SBO_HIP(nL.reserve(sizeof(float) * (size_t)ncap * (size_t)ncap));
    SBO_HIP(hipMemcpyAsync(nx.as<float>(), ctx->x.as<float>(), sizeof(float) * n0, hipMemcpyDeviceToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(ny.as<float>(), ctx->y.as<float>(), sizeof(float) * n0, hipMemcpyDeviceToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(no.as<float>(), ctx->obs.as<float>(), sizeof(float) * n0, hipMemcpyDeviceToDevice, ctx->stream));
    SBO_HIP(hipMemcpy2DAsync(nL.as<float>(), sizeof(float) * ncap, ctx->L.as<float>(), sizeof(float) * ctx->cap,
                             sizeof(float) * n0, n0, hipMemcpyDeviceToDevice, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    if (inverse_current(ctx, n0)) {  // keep the f64 inverse for the incremental refresh
        DevBuf nLi;
        SBO_HIP(nLi.reserve(sizeof(double) * (size_t)ncap * (size_t)ncap));
        SBO_HIP(hipMemcpy2DAsync(nLi.as<double>(), sizeof(double) * ncap, ctx->Linv.as<double>(),
                                 sizeof(double) * ctx->cap, sizeof(double) * n0, n0, hipMemcpyDeviceToDevice,
                                 ctx->stream));
        SBO_HIP(hipStreamSynchronize(ctx->stream));
        ctx->Linv.swap(nLi);
    } else {
        ctx->linv_n = 0;
    }
    ctx->x.swap(nx);
    ctx->y.swap(ny);
    ctx->obs.swap(no);
    ctx->L.swap(nL);
    ctx->cap = ncap;
    SBO_HIP(ctx->alpha.reserve(sizeof(float) * ncap));
    return SBO_OK;
}

// K21 and K22 (with the noise on its diagonal) in their places in L
sbo_status append_fill(sbo_ctx *ctx, int64_t n0, int64_t b) {
    const int64_t ld = ctx->cap;
    const float *xs = ctx->x.as<float>(), *ys = ctx->y.as<float>();
    const float ell = (float)ctx->hyper.length_scale, sn2 = (float)ctx->hyper.noise_level;
    const float sf2 = (float)(ctx->hyper.sigma_f * ctx->hyper.sigma_f);
    SBO_HIP(sbo::launch_rbf_fill(ctx->stream, xs + n0, ys + n0, b, xs, ys, n0, ld, ell, sf2, sn2, false,
                                 append_L21(ctx, n0)));
    SBO_HIP(sbo::launch_rbf_fill(ctx->stream, xs + n0, ys + n0, b, xs + n0, ys + n0, b, ld, ell, sf2, sn2, true,
                                 append_L22(ctx, n0)));
    return SBO_OK;
}

// L21 = K21 L11^-T in place, one branch per regime (kAppendInvRows,
// kAppendInvGemm, the level-3 solve).
sbo_status append_panel(sbo_ctx *ctx, int64_t n0, int64_t b) {
    const int64_t ld = ctx->cap;
    float *L21 = append_L21(ctx, n0);
    const bool inv_kept = inverse_current(ctx, n0);
    SBO_BLAS(rocblas_set_pointer_mode(ctx->blas, rocblas_pointer_mode_host));
    if (inv_kept && b <= kAppendInvRows) {
        // a few points (the node's one per change): L21 row by row from the
        // kept f64 inverse, L21[r,:]^T = L11^-1 K21[r,:]^T, one dtrmv over its
        // lower triangle per point, rounded to f32 once -- rocBLAS strsm ran
        // the 1 x n0 solve as ~250 small launches (6.3 ms at C4)
        SBO_HIP(ctx->rvec.reserve(sizeof(double) * (size_t)n0));
        double *w = ctx->rvec.as<double>();
        for (int64_t r = 0; r < b; ++r) {
            SBO_HIP(sbo::launch_widen(ctx->stream, L21 + r, ld, 1, n0, false, w, 1));
            SBO_BLAS(rocblas_dtrmv(ctx->blas, rocblas_fill_lower, rocblas_operation_none, rocblas_diagonal_non_unit,
                                   (rocblas_int)n0, ctx->Linv.as<double>(), (rocblas_int)ld, w, 1));
            SBO_HIP(sbo::launch_narrow_strided(ctx->stream, w, n0, L21 + r, ld));
        }
    } else if (inv_kept && b <= kAppendInvGemm) {
        // a batch: L21 = K21 L11^-T as one f64 GEMM with the kept inverse
        // (its strict upper part is zero), rounded to f32 once
        SBO_HIP(ctx->rvec.reserve(sizeof(double) * (size_t)n0 * (size_t)b * 2));
        double *kw = ctx->rvec.as<double>(), *cw = kw + (size_t)n0 * (size_t)b;
        const double done = 1.0, dzero = 0.0;
        SBO_HIP(sbo::launch_widen(ctx->stream, L21, ld, b, n0, false, kw, b));
        SBO_BLAS(rocblas_dgemm(ctx->blas, rocblas_operation_none, rocblas_operation_transpose, (rocblas_int)b,
                               (rocblas_int)n0, (rocblas_int)n0, &done, kw, (rocblas_int)b, ctx->Linv.as<double>(),
                               (rocblas_int)ld, &dzero, cw, (rocblas_int)b));
        SBO_HIP(sbo::launch_narrow_2d(ctx->stream, cw, b, b, n0, L21, ld));
    } else {
        const float one = 1.0f;
        SBO_BLAS(rocblas_strsm(ctx->blas, rocblas_side_right, rocblas_fill_lower, rocblas_operation_transpose,
                               rocblas_diagonal_non_unit, (rocblas_int)b, (rocblas_int)n0, &one, ctx->L.as<float>(),
                               (rocblas_int)ld, L21, (rocblas_int)ld));
    }
    return SBO_OK;
}

// K22 -= L21 L21^T as a full b x b sgemm (rocBLAS's ssyrk ran its small-n
// kernels at ~250 us here; the strict upper half it also writes is never
// read).  Host pointer mode: append_panel set it.
sbo_status append_schur(sbo_ctx *ctx, int64_t n0, int64_t b) {
    const float one = 1.0f, minus_one = -1.0f;
    const float *L21 = append_L21(ctx, n0);
    SBO_BLAS(rocblas_sgemm(ctx->blas, rocblas_operation_none, rocblas_operation_transpose, (rocblas_int)b,
                           (rocblas_int)b, (rocblas_int)n0, &minus_one, L21, (rocblas_int)ctx->cap, L21,
                           (rocblas_int)ctx->cap, &one, append_L22(ctx, n0), (rocblas_int)ctx->cap));
    return SBO_OK;
}
}  // namespace

SBO_API sbo_status sbo_fit(sbo_ctx *ctx, const float *x, const float *y, const float *obs, int64_t n,
                           sbo_hyper hyper, uint32_t flags) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(x && y && obs, SBO_E_INVAL, "sbo_fit: null input");
    SBO_CHECK(n > 0, SBO_E_EMPTY, "sbo_fit: n must be > 0");
    SBO_CHECK(n < (int64_t)1 << 30, SBO_E_INVAL, "sbo_fit: n too large");
    if (sbo_status st = check_hyper(ctx, hyper)) return st;
    SBO_HIP(hipSetDevice(ctx->device));
    if (sbo_status st = ctx->pop.drain(ctx)) return st;   // (a precise pack may still read x, y, L^-1, alpha64)
    FitCommit fc(ctx);
    ctx->hyper = hyper;
    ctx->n = n;
    ctx->cap = n;
    ctx->linv_n = 0;
    SBO_HIP(ctx->x.reserve(sizeof(float) * n));
    SBO_HIP(ctx->y.reserve(sizeof(float) * n));
    SBO_HIP(ctx->obs.reserve(sizeof(float) * n));
    SBO_HIP(ctx->alpha.reserve(sizeof(float) * n));
    SBO_HIP(ctx->L.reserve(sizeof(float) * (size_t)n * (size_t)n));
    if (sbo_status st = stage_training(ctx, x, y, obs, n, 0, 0, flags)) return st;
    if (sbo_status st = fill_and_factor(ctx, hyper.noise_level)) return st;
    return fc.commit(finish(ctx, flags));
}

SBO_API sbo_status sbo_get_jitter(const sbo_ctx *ctx, double *jitter) {
    if (!ctx || !jitter) return SBO_E_INVAL;
    if (!ctx->fitted) return SBO_E_STATE;
    *jitter = ctx->jitter;
    return SBO_OK;
}

SBO_API sbo_status sbo_append(sbo_ctx *ctx, const float *x, const float *y, const float *obs, int64_t b,
                              uint32_t flags) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(ctx->fitted, SBO_E_STATE, "sbo_append: call sbo_fit first");
    SBO_CHECK(ctx->has_factor, SBO_E_STATE, "sbo_append: imported predict-only state has no factor; refit");
    SBO_CHECK(x && y && obs, SBO_E_INVAL, "sbo_append: null input");
    SBO_CHECK(b >= 0, SBO_E_INVAL, "sbo_append: b must be >= 0");
    if (b == 0) return SBO_OK;
    SBO_HIP(hipSetDevice(ctx->device));
    if (sbo_status st = ctx->pop.drain(ctx)) return st;   // (a precise pack may still read x, y, L^-1, alpha64)
    const int64_t n0 = ctx->n, n1 = n0 + b;
    SBO_CHECK(n1 < (int64_t)1 << 30, SBO_E_INVAL, "sbo_append: n too large");
    FitCommit fc(ctx);
    // SBO_OPT_RESORT: once the points appended since the last k-d sort exceed
    // resort_pct % of the sorted ones, re-sort and refactor all of them
    // (points sbo_remove rotated out since then count as well: resort_due)
    if (resort_due(ctx, n1, ctx->n_sorted, ctx->removed_since_sort)) {
        if (sbo_status st = resort_append(ctx, x, y, obs, b, flags)) return st;
        return fc.commit(finish(ctx, flags));
    }
    // the block update (append_L21): storage, the new points, K21 and K22,
    // L21, the Schur complement, its factorization, the operand's new rows
    if (n1 > ctx->cap)
        if (sbo_status st = append_grow(ctx, n1)) return st;
    if (sbo_status st = stage_training(ctx, x, y, obs, b, n0, n0, flags)) return st;
    if (sbo_status st = append_fill(ctx, n0, b)) return st;
    if (sbo_status st = append_panel(ctx, n0, b)) return st;
    if (sbo_status st = append_schur(ctx, n0, b)) return st;
    FactorHandover ho;   // (nothing but the info: a block's factorization starts no inverse)
    if (sbo_status st = factor_block(ctx, append_L22(ctx, n0), b, ctx->cap, false, FactorOf::kAppendedBlock, ho))
        return st;
    ctx->n = n1;
    if (sbo_status st = refresh_operand(ctx, n0)) return st;
    return fc.commit(finish(ctx, flags));
}

namespace {
// sbo_remove's rotation path, beside the append_* stages: per removed point
// (ascending stored position, no compaction in between -- a later chain only
// touches columns to the right of its own position, the dead rows and columns
// of earlier ones are to its left or harmless to rotate) remove_chain over L
// and remove_rows over the f64 inverse, then one remove_compact, then
// refresh_operand.  One point rotates the f32 factor in place; a batch
// rotates an f64 copy of its columns from the first removed one on, so that
// the factor is rounded to f32 once per call.
struct RemoveRun {
    sbo::RemoveMap map;
    int64_t n0 = 0, n1 = 0, first = 0;
    sbo::RemoveWork wk;
    double *W = nullptr;          // the batch's f64 columns of L (null: one point, in place)
    std::vector<int> keep32;      // (lives until the stream has taken it)
};

// the workspaces, the kept positions on the device, the flag cleared, and the batch's f64 columns
sbo_status remove_begin(sbo_ctx *ctx, RemoveRun &run) {
    const int64_t n0 = run.n0, ld = ctx->cap, f = run.first;
    SBO_HIP(ctx->ws.rmws.reserve(sbo::remove_work_bytes(n0)));
    run.wk = sbo::remove_work(ctx->ws.rmws.as<void>(), n0);
    run.keep32.assign(run.map.keep.begin(), run.map.keep.end());
    SBO_HIP(hipMemsetAsync(run.wk.flag, 0, sizeof(int), ctx->stream));
    SBO_HIP(hipMemcpyAsync(run.wk.keep, run.keep32.data(), sizeof(int) * run.keep32.size(), hipMemcpyHostToDevice,
                           ctx->stream));
    if (run.map.pos.size() > 1) {
        SBO_HIP(ctx->ws.rmw64.reserve(sizeof(double) * (size_t)ld * (size_t)(n0 - f)));
        run.W = ctx->ws.rmw64.as<double>();
        SBO_HIP(sbo::launch_widen(ctx->stream, ctx->L.as<float>() + f + f * ld, ld, n0 - f, n0 - f, true, run.W + f, ld));
    }
    return SBO_OK;
}
sbo_status remove_chain(sbo_ctx *ctx, const RemoveRun &run, int64_t i) {
    SBO_HIP(sbo::launch_remove_chain(ctx->stream, ctx->L.as<float>(), run.W, ctx->cap, run.first, run.n0, i, run.wk));
    return SBO_OK;
}
sbo_status remove_rows(sbo_ctx *ctx, const RemoveRun &run, int64_t i) {
    SBO_HIP(sbo::launch_remove_rows(ctx->stream, ctx->Linv.as<double>(), ctx->cap, run.n0, i, run.wk));
    return SBO_OK;
}
// The rows and columns left move up (only positions >= the first removed one
// move), and the chains' pivots are read: one that was not positive and finite
// is NOT_SPD.
sbo_status remove_compact(sbo_ctx *ctx, const RemoveRun &run) {
    SBO_HIP(ctx->ws.rmmove.reserve(sbo::remove_compact_bytes(run.n1, run.first)));
    SBO_HIP(sbo::launch_remove_compact(ctx->stream, ctx->L.as<float>(), run.W, run.first, ctx->Linv.as<double>(),
                                       ctx->cap, ctx->x.as<float>(), ctx->y.as<float>(), ctx->obs.as<float>(), run.n1,
                                       run.first, run.wk, ctx->ws.rmmove.as<void>()));
    int flag = 0;
    SBO_HIP(hipMemcpyAsync(&flag, run.wk.flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    SBO_CHECK(flag == 0, SBO_E_NOT_SPD, "sbo_remove: a rotation met a pivot that is not positive and finite");
    return SBO_OK;
}

// sbo_remove's refit of the remaining points: staged again in k-d order and
// factored from scratch, the way resort_append does, the caller's (renumbered)
// indices kept.  The bounding box stays the one of every point seen.
sbo_status remove_refit(sbo_ctx *ctx, const RemoveRun &run) {
    const int64_t n0 = run.n0, n1 = run.n1;
    std::vector<float> h[3], p[3];
    const float *src[3] = {ctx->x.as<float>(), ctx->y.as<float>(), ctx->obs.as<float>()};
    for (int a = 0; a < 3; ++a) {
        h[a].resize((size_t)n0);
        SBO_HIP(hipMemcpyAsync(h[a].data(), src[a], sizeof(float) * n0, hipMemcpyDeviceToHost, ctx->stream));
    }
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    for (int a = 0; a < 3; ++a) {
        p[a].resize((size_t)n1);
        for (int64_t r = 0; r < n1; ++r) p[a][(size_t)r] = h[a][(size_t)run.map.keep[(size_t)r]];
    }
    float bbox[4];
    std::copy(ctx->bbox, ctx->bbox + 4, bbox);
    ctx->n = n1;
    ctx->linv_n = 0;
    if (sbo_status st = stage_training(ctx, p[0].data(), p[1].data(), p[2].data(), n1, 0, 0, 0)) return st;
    std::copy(bbox, bbox + 4, ctx->bbox);
    for (int64_t r = 0; r < n1; ++r) ctx->order[(size_t)r] = run.map.new_order[(size_t)ctx->order[(size_t)r]];
    return fill_and_factor(ctx, ctx->hyper.noise_level - ctx->jitter);
}
}  // namespace

SBO_API sbo_status sbo_remove(sbo_ctx *ctx, const int64_t *idx, int64_t b, sbo_remove_info *info, uint32_t flags) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(ctx->fitted, SBO_E_STATE, "sbo_remove: call sbo_fit first");
    SBO_CHECK(ctx->has_factor, SBO_E_STATE, "sbo_remove: imported predict-only state has no factor; refit");
    SBO_CHECK(b >= 0, SBO_E_INVAL, "sbo_remove: b must be >= 0");
    SBO_CHECK(idx || b == 0, SBO_E_INVAL, "sbo_remove: null idx");
    sbo_remove_info r{};
    r.path = 1;
    r.reason = SBO_REMOVE_DOWNDATED;
    r.n = ctx->n;
    r.first_row = -1;
    if (b == 0) {
        if (info) copy_info(info, r);
        return SBO_OK;
    }
    RemoveRun run;
    run.n0 = ctx->n;
    const sbo::RemoveMapStatus ms = sbo::remove_map(ctx->order.data(), run.n0, idx, b, run.map);
    SBO_CHECK(ms != sbo::RemoveMapStatus::kInval, SBO_E_INVAL, "sbo_remove: an index outside [0, n) or a duplicate");
    SBO_CHECK(ms != sbo::RemoveMapStatus::kEmpty, SBO_E_EMPTY, "sbo_remove: a model needs at least one point");
    run.n1 = run.n0 - b;
    run.first = run.map.pos.front();
    SBO_HIP(hipSetDevice(ctx->device));
    if (sbo_status st = ctx->pop.drain(ctx)) return st;   // (a precise pack may still read x, y, L^-1, alpha64)
    hipEvent_t ev0 = take_event(ctx), ev1 = take_event(ctx);
    struct Back {   // the events go back to the pool on every path
        sbo_ctx *c;
        hipEvent_t a, b;
        ~Back() {
            if (a) c->ev_pool.push_back(a);
            if (b) c->ev_pool.push_back(b);
        }
    } back{ctx, ev0, ev1};
    SBO_CHECK(ev0 && ev1, SBO_E_DEVICE, "sbo_remove: hipEventCreate failed");
    FitCommit fc(ctx);
    drain_guard(ctx);
    // rotations, or a refit of the remaining points
    const int64_t sorted_left = ctx->n_sorted - run.map.below(ctx->n_sorted);
    if (!fit_state_complete(ctx, run.n0)) {
        r.path = 0;
        r.reason = SBO_REMOVE_NO_INVERSE;
    } else if (b > ctx->opt.remove_max) {
        r.path = 0;
        r.reason = SBO_REMOVE_OVER_CAP;
    } else if (resort_due(ctx, run.n1, sorted_left, ctx->removed_since_sort + b)) {
        r.path = 0;
        r.reason = SBO_REMOVE_RESORT;
    }
    r.removed = b;
    r.n = run.n1;
    r.first_row = run.first;
    r.rotations = r.path ? run.map.rotations : 0;
    SBO_HIP(hipEventRecord(ev0, ctx->stream));
    if (r.path == 0) {
        if (sbo_status st = remove_refit(ctx, run)) return st;
    } else {
        if (sbo_status st = remove_begin(ctx, run)) return st;
        for (int64_t i : run.map.pos) {
            if (sbo_status st = remove_chain(ctx, run, i)) return st;
            if (sbo_status st = remove_rows(ctx, run, i)) return st;
        }
        if (sbo_status st = remove_compact(ctx, run)) return st;
        ++ctx->fit_epoch;   // another model: a kept posterior is not updated into it
        ctx->n = run.n1;
        ctx->linv_n = run.n1;
        ctx->z_n = 0;
        ctx->order = run.map.new_order;
        ctx->n_sorted = sorted_left;
        ctx->removed_since_sort += b;
        if (sbo_status st = refresh_operand(ctx, 0, {}, run.first)) return st;
    }
    SBO_HIP(hipEventRecord(ev1, ctx->stream));
    SBO_HIP(hipEventSynchronize(ev1));
    float msf = 0.0f;
    SBO_HIP(hipEventElapsedTime(&msf, ev0, ev1));
    r.ms = msf;
    if (info) copy_info(info, r);
    return fc.commit(finish(ctx, flags));
}

SBO_API sbo_status sbo_debug_inverse64(sbo_ctx *ctx, double *X, int64_t cap) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(ctx->fitted && inverse_current(ctx, ctx->n), SBO_E_STATE, "sbo_debug_inverse64: no current f64 inverse");
    const int64_t n = ctx->n;
    SBO_CHECK(X && cap >= n * n, SBO_E_INVAL, "sbo_debug_inverse64: X must hold n * n doubles");
    SBO_HIP(hipSetDevice(ctx->device));
    std::vector<double> cm((size_t)n * (size_t)n);
    SBO_HIP(hipMemcpy2DAsync(cm.data(), sizeof(double) * n, ctx->Linv.as<double>(), sizeof(double) * ctx->cap,
                             sizeof(double) * n, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < n; ++j) X[i * n + j] = j <= i ? cm[(size_t)(j * n + i)] : 0.0;
    return SBO_OK;
}

SBO_API sbo_status sbo_debug_remove_map(const int64_t *order, int64_t n, const int64_t *idx, int64_t b, int64_t *pos,
                                        int64_t *new_order) {
    if (n <= 0 || !order) return SBO_E_INVAL;
    try {
        sbo::RemoveMap m;
        const sbo::RemoveMapStatus st = sbo::remove_map(order, n, idx, b, m);
        if (st == sbo::RemoveMapStatus::kInval) return SBO_E_INVAL;
        if (st == sbo::RemoveMapStatus::kEmpty) return SBO_E_EMPTY;
        if (pos) std::copy(m.pos.begin(), m.pos.end(), pos);
        if (new_order) std::copy(m.new_order.begin(), m.new_order.end(), new_order);
    } catch (...) {
        return SBO_E_OOM;
    }
    return SBO_OK;
}

SBO_API sbo_status sbo_predict(sbo_ctx *ctx, const float *qx, const float *qy, int64_t m, float *mu, float *sd,
                               uint32_t flags) {
    return sbo_tick(ctx, qx, qy, m, 0.0, 0.0, SBO_SCORE_WIDTH, 0, mu, sd, nullptr, nullptr, nullptr, nullptr,
                    flags);
}

SBO_API sbo_status sbo_query_cost(sbo_ctx *ctx, const float *qx, const float *qy, int64_t m, float *cost,
                                  uint32_t flags) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(ctx->fitted, SBO_E_STATE, "sbo_query_cost: call sbo_fit first");
    SBO_CHECK(qx && qy && cost, SBO_E_INVAL, "sbo_query_cost: null pointer");
    SBO_CHECK(m > 0, SBO_E_EMPTY, "sbo_query_cost: m must be > 0");
    SBO_HIP(hipSetDevice(ctx->device));
    TickRequest rq;
    rq.m = m;
    rq.want = TickWant::kCost;
    if (dev(flags)) {
        rq.qx = qx;
        rq.qy = qy;
        rq.cost = cost;
        if (sbo_status st = run_tick(ctx, rq)) return st;
        return finish(ctx, flags);
    }
    Carve c;
    if (sbo_status st = stage_queries(ctx, qx, qy, m, Carve::need(m, 4), rq, c)) return st;
    rq.cost = c.take<float>(m);
    if (sbo_status st = run_tick(ctx, rq)) return st;
    SBO_HIP(hipMemcpyAsync(cost, rq.cost, sizeof(float) * m, hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    return SBO_OK;
}

// sbo_tick and sbo_tick_stream: one argument check, one staging of host
// pointers; `stream` selects run_tick_stream over run_tick.
static sbo_status tick_entry(bool stream, sbo_ctx *ctx, const float *qx, const float *qy, int64_t m, double beta,
                             double f_min, sbo_score score, int64_t index_offset, float *mu, float *sd, double *lo,
                             double *hi, uint8_t *safe, sbo_key *out, uint32_t flags) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(ctx->fitted, SBO_E_STATE, "sbo_tick: call sbo_fit first");
    SBO_CHECK(qx && qy, SBO_E_INVAL, "sbo_tick: null query coordinates");
    SBO_CHECK(m > 0, SBO_E_EMPTY, "sbo_tick: m must be > 0");
    SBO_CHECK(score == SBO_SCORE_WIDTH || score == SBO_SCORE_UCB, SBO_E_INVAL, "sbo_tick: bad score kind");
    SBO_CHECK(std::isfinite(beta) && !std::isnan(f_min), SBO_E_INVAL, "sbo_tick: beta/f_min must be finite");
    SBO_HIP(hipSetDevice(ctx->device));
    TickRequest rq;
    rq.m = m;
    rq.beta = beta;
    rq.f_min = f_min;
    rq.score = (int)score;
    rq.index_offset = index_offset;
    if (dev(flags)) {
        rq.qx = qx;
        rq.qy = qy;
        rq.mu = mu;
        rq.sd = sd;
        rq.lo = lo;
        rq.hi = hi;
        rq.safe = safe;
        rq.key = out;
        if (sbo_status st = stream ? run_tick_stream(ctx, rq) : run_tick(ctx, rq)) return st;
        return finish(ctx, flags);
    }
    // host pointers: stage through device scratch
    Carve c;
    if (sbo_status st = stage_queries(ctx, qx, qy, m,
                                      Carve::need(m, 4) * 2 + Carve::need(m, 8) * 2 + Carve::need(m, 1) +
                                          Carve::need(1, sizeof(sbo_key)),
                                      rq, c))
        return st;
    float *dmu = c.take<float>(m), *dsd = c.take<float>(m);
    double *dlo = c.take<double>(m), *dhi = c.take<double>(m);
    uint8_t *dsafe = c.take<uint8_t>(m);
    sbo_key *dkey = c.take<sbo_key>(1);
    rq.mu = mu ? dmu : nullptr;
    rq.sd = sd ? dsd : nullptr;
    rq.lo = lo ? dlo : nullptr;
    rq.hi = hi ? dhi : nullptr;
    rq.safe = safe ? dsafe : nullptr;
    rq.key = dkey;
    if (sbo_status st = stream ? run_tick_stream(ctx, rq) : run_tick(ctx, rq)) return st;
    if (mu) SBO_HIP(hipMemcpyAsync(mu, dmu, sizeof(float) * m, hipMemcpyDeviceToHost, ctx->stream));
    if (sd) SBO_HIP(hipMemcpyAsync(sd, dsd, sizeof(float) * m, hipMemcpyDeviceToHost, ctx->stream));
    if (lo) SBO_HIP(hipMemcpyAsync(lo, dlo, sizeof(double) * m, hipMemcpyDeviceToHost, ctx->stream));
    if (hi) SBO_HIP(hipMemcpyAsync(hi, dhi, sizeof(double) * m, hipMemcpyDeviceToHost, ctx->stream));
    if (safe) SBO_HIP(hipMemcpyAsync(safe, dsafe, m, hipMemcpyDeviceToHost, ctx->stream));
    if (out) SBO_HIP(hipMemcpyAsync(ctx->host_key, dkey, sizeof(sbo_key), hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    if (out) *out = *ctx->host_key;
    return SBO_OK;
}

SBO_API sbo_status sbo_tick(sbo_ctx *ctx, const float *qx, const float *qy, int64_t m, double beta, double f_min,
                            sbo_score score, int64_t index_offset, float *mu, float *sd, double *lo, double *hi,
                            uint8_t *safe, sbo_key *out, uint32_t flags) {
    return tick_entry(false, ctx, qx, qy, m, beta, f_min, score, index_offset, mu, sd, lo, hi, safe, out, flags);
}

SBO_API sbo_status sbo_tick_stream(sbo_ctx *ctx, const float *qx, const float *qy, int64_t m, double beta,
                                   double f_min, sbo_score score, int64_t index_offset, float *mu, float *sd,
                                   double *lo, double *hi, uint8_t *safe, sbo_key *out, uint32_t flags) {
    return tick_entry(true, ctx, qx, qy, m, beta, f_min, score, index_offset, mu, sd, lo, hi, safe, out, flags);
}

SBO_API sbo_status sbo_get_stream(const sbo_ctx *ctx, sbo_stream_info *out) {
    if (!ctx || !out || out->struct_size < sizeof(uint32_t)) return SBO_E_INVAL;
    const sbo::StreamKeep &k = ctx->keep;
    sbo_stream_info info = k.last;
    info.updates_since_full = k.updates;
    info.err_var = k.err_var;
    info.err_mean = k.err_mean;
    if (info.path == 1 && info.tiles_total > 0) {
        // the update's own count of the tiles it multiplied (waits for the stream)
        unsigned long long kept = 0;
        if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
            hipMemcpy(&kept, k.head.as<sbo::StreamHead>() + 1, sizeof(kept), hipMemcpyDeviceToHost) != hipSuccess)
            return SBO_E_DEVICE;
        info.tiles_kept = (int64_t)kept;
    }
    copy_info(out, info);
    return SBO_OK;
}

SBO_API sbo_status sbo_stream_reset(sbo_ctx *ctx) {
    if (!ctx) return SBO_E_INVAL;
    SBO_HIP(hipSetDevice(ctx->device));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    ctx->keep.release();
    ctx->keep.was_reset = true;
    ctx->keep.last = sbo_stream_info{};
    ctx->keep.err_var = ctx->keep.err_mean = 0.0;
    ctx->keep.updates = 0;
    return SBO_OK;
}

SBO_API sbo_status sbo_debug_stream_state(sbo_ctx *ctx, double *mu64, double *var64, int64_t cap) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(mu64 && var64, SBO_E_INVAL, "sbo_debug_stream_state: null output");
    const sbo::StreamKeep &k = ctx->keep;
    SBO_CHECK(k.valid, SBO_E_STATE, "sbo_debug_stream_state: no kept posterior (call sbo_tick_stream first)");
    SBO_CHECK(cap >= k.m, SBO_E_INVAL, "sbo_debug_stream_state: cap below the kept posterior's m");
    SBO_HIP(hipSetDevice(ctx->device));
    const size_t bytes = sizeof(double) * (size_t)k.m;
    SBO_HIP(ctx->hout.reserve(2 * bytes));
    double *dmu = ctx->hout.as<double>(), *dvar = dmu + k.m;
    SBO_HIP(sbo::launch_stream_scatter(ctx->stream, k.mu64.as<double>(), k.var64.as<double>(), k.perm.as<int32_t>(),
                                       k.ms, dmu, dvar));
    SBO_HIP(hipMemcpyAsync(mu64, dmu, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipMemcpyAsync(var64, dvar, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    return SBO_OK;
}

SBO_API sbo_status sbo_compute_sets(sbo_ctx *ctx, const float *mu, const float *sd, int64_t m, double beta,
                                    double f_min, double *lo, double *hi, uint8_t *safe, uint32_t flags) {
    return compute_sets_impl(ctx, mu, sd, m, beta, f_min, lo, hi, safe, flags);
}

SBO_API sbo_status sbo_compute_sets_f64(sbo_ctx *ctx, const double *mu, const double *sd, int64_t m, double beta,
                                        double f_min, double *lo, double *hi, uint8_t *safe, uint32_t flags) {
    return compute_sets_impl(ctx, mu, sd, m, beta, f_min, lo, hi, safe, flags);
}

SBO_API sbo_status sbo_argmax(sbo_ctx *ctx, const double *score, const uint8_t *mask, int64_t m,
                              int64_t index_offset, sbo_key *out, uint32_t flags) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(score && out, SBO_E_INVAL, "sbo_argmax: null score/out");
    SBO_CHECK(m >= 0, SBO_E_INVAL, "sbo_argmax: m must be >= 0");
    SBO_HIP(hipSetDevice(ctx->device));
    if (m == 0) {
        const sbo_key none{0.0, -1};
        if (dev(flags)) {
            SBO_HIP(hipMemcpyAsync(out, &none, sizeof(none), hipMemcpyHostToDevice, ctx->stream));
            return finish(ctx, flags);
        }
        *out = none;
        return SBO_OK;
    }
    const int64_t nb = sbo::acq_blocks(m);
    SBO_HIP(ctx->keys.reserve(sizeof(sbo_key) * (size_t)(nb + 1)));
    sbo_key *bk = ctx->keys.as<sbo_key>();
    if (dev(flags)) {
        SBO_HIP(sbo::launch_argmax_blocks(ctx->stream, score, mask, m, index_offset, bk));
        SBO_HIP(sbo::launch_reduce_keys(ctx->stream, bk, nb, out));
        return finish(ctx, flags);
    }
    const size_t need = Carve::need(m, 8) + Carve::need(m, 1);
    SBO_HIP(ctx->hq.reserve(need));
    Carve c(ctx->hq.as<void>());
    double *ds = c.take<double>(m);
    uint8_t *dm = c.take<uint8_t>(m);
    SBO_HIP(hipMemcpyAsync(ds, score, sizeof(double) * m, hipMemcpyHostToDevice, ctx->stream));
    if (mask) SBO_HIP(hipMemcpyAsync(dm, mask, m, hipMemcpyHostToDevice, ctx->stream));
    SBO_HIP(sbo::launch_argmax_blocks(ctx->stream, ds, mask ? dm : nullptr, m, index_offset, bk));
    SBO_HIP(sbo::launch_reduce_keys(ctx->stream, bk, nb, bk + nb));
    SBO_HIP(hipMemcpyAsync(ctx->host_key, bk + nb, sizeof(sbo_key), hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    *out = *ctx->host_key;
    return SBO_OK;
}

SBO_API sbo_key sbo_key_combine(sbo_key a, sbo_key b) {
    if (a.idx < 0) return b;
    if (b.idx < 0) return a;
    if (a.score > b.score) return a;
    if (b.score > a.score) return b;
    return a.idx <= b.idx ? a : b;
}

SBO_API sbo_status sbo_keys_reduce(sbo_ctx *ctx, const sbo_key *keys, int64_t n, sbo_key *out, uint32_t flags) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(out && (keys || n == 0), SBO_E_INVAL, "sbo_keys_reduce: null keys/out");
    SBO_CHECK(n >= 0 && n <= ((int64_t)1 << 31), SBO_E_INVAL, "sbo_keys_reduce: n out of range");
    if (!dev(flags)) {
        sbo_key r{0.0, -1};
        for (int64_t i = 0; i < n; ++i) r = sbo_key_combine(r, keys[i]);
        *out = r;
        return SBO_OK;
    }
    SBO_HIP(hipSetDevice(ctx->device));
    // one workgroup, the tick's own final reduction (reduce_keys_kernel:
    // highest score, lowest index on ties, idx -1 = none); n = 0 writes the
    // empty key
    SBO_HIP(sbo::launch_reduce_keys(ctx->stream, keys, n, out));
    return finish(ctx, flags);
}

SBO_API sbo_status sbo_rbf_fill(sbo_ctx *ctx, const float *x, const float *y, int64_t n, sbo_hyper hyper, float *K,
                                uint32_t flags) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(x && y && K, SBO_E_INVAL, "sbo_rbf_fill: null argument");
    SBO_CHECK(n > 0, SBO_E_EMPTY, "sbo_rbf_fill: n must be > 0");
    if (sbo_status st = check_hyper(ctx, hyper)) return st;
    SBO_HIP(hipSetDevice(ctx->device));
    const float sf2 = (float)(hyper.sigma_f * hyper.sigma_f);
    if (dev(flags)) {
        Bracket br(ctx, ctx->ev_fill);
        SBO_HIP(sbo::launch_rbf_fill(ctx->stream, x, y, n, x, y, n, n, (float)hyper.length_scale, sf2,
                                     (float)hyper.noise_level, true, K));
        return finish(ctx, flags);
    }
    const size_t need = Carve::need(n, 4) * 2 + Carve::need((size_t)n * n, 4);
    SBO_HIP(ctx->hq.reserve(need));
    Carve c(ctx->hq.as<void>());
    float *dx = c.take<float>(n), *dy = c.take<float>(n), *dK = c.take<float>((size_t)n * n);
    SBO_HIP(hipMemcpyAsync(dx, x, sizeof(float) * n, hipMemcpyHostToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(dy, y, sizeof(float) * n, hipMemcpyHostToDevice, ctx->stream));
    SBO_HIP(sbo::launch_rbf_fill(ctx->stream, dx, dy, n, dx, dy, n, n, (float)hyper.length_scale, sf2,
                                 (float)hyper.noise_level, true, dK));
    SBO_HIP(hipMemcpyAsync(K, dK, sizeof(float) * (size_t)n * n, hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    return SBO_OK;
}

SBO_API sbo_status sbo_get_factor(sbo_ctx *ctx, float *L, float *alpha, uint32_t flags) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(ctx->fitted && ctx->has_factor, SBO_E_STATE, "sbo_get_factor: call sbo_fit first");
    SBO_HIP(hipSetDevice(ctx->device));
    const int64_t n = ctx->n;
    const hipMemcpyKind k = dev(flags) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (L) {
        if (dev(flags)) {
            SBO_HIP(sbo::launch_copy_lower(ctx->stream, ctx->L.as<float>(), ctx->cap, n, L, n));
        } else {
            SBO_HIP(ctx->hq.reserve(sizeof(float) * (size_t)n * n));
            SBO_HIP(sbo::launch_copy_lower(ctx->stream, ctx->L.as<float>(), ctx->cap, n, ctx->hq.as<float>(), n));
            SBO_HIP(hipMemcpyAsync(L, ctx->hq.as<float>(), sizeof(float) * (size_t)n * n, k, ctx->stream));
        }
    }
    if (alpha) SBO_HIP(hipMemcpyAsync(alpha, ctx->alpha.as<float>(), sizeof(float) * n, k, ctx->stream));
    if (!dev(flags)) {
        SBO_HIP(hipStreamSynchronize(ctx->stream));
        return SBO_OK;
    }
    return finish(ctx, flags);
}

SBO_API sbo_status sbo_profile(sbo_ctx *ctx, int enable) {
    if (!ctx) return SBO_E_INVAL;
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    recycle_events(ctx);
    ctx->prof = enable != 0;
    SBO_HIP(ctx->counters.reserve(64));
    SBO_HIP(hipMemsetAsync(ctx->counters.as<void>(), 0, 64, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    return SBO_OK;
}

SBO_API sbo_status sbo_profile_work(sbo_ctx *ctx, double *predict_flops) {
    if (!ctx || !predict_flops) return SBO_E_INVAL;
    unsigned long long t = 0;
    if (ctx->counters.capacity()) {
        SBO_HIP(hipMemcpyAsync(&t, ctx->counters.as<void>(), sizeof(t), hipMemcpyDeviceToHost, ctx->stream));
        SBO_HIP(hipStreamSynchronize(ctx->stream));
    }
    *predict_flops = 2.0 * sbo::kBM * sbo::kBN * sbo::kBK * (double)t;
    return SBO_OK;
}

SBO_API sbo_status sbo_debug_x3_stamps(sbo_ctx *ctx, double *cycles, int n) {
    if (!ctx || !cycles || n <= 0) return SBO_E_INVAL;
    SBO_HIP(hipSetDevice(ctx->device));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    SBO_HIP(sbo::read_x3_stamps(cycles, n));
    return SBO_OK;
}

SBO_API sbo_status sbo_debug_x3_operand(sbo_ctx *ctx, void *host_buf, int64_t cap, int64_t *bytes) {
    if (!ctx || !bytes || cap < 0) return SBO_E_INVAL;
    if (!ctx->fitted || ctx->opt.kernel_variant < 2) return SBO_E_INVAL;
    SBO_HIP(hipSetDevice(ctx->device));
    // (the eager derivation of a fit or an append runs on aux_stream)
    SBO_HIP(hipStreamSynchronize(ctx->aux_stream));
    if (sbo_status st = derive_x3(ctx)) return st;
    const int64_t need = (int64_t)sbo::x3_operand_bytes(ctx->npad);
    *bytes = need;
    if (!host_buf) return SBO_OK;
    if (cap < need) return SBO_E_INVAL;
    SBO_HIP(hipMemcpyAsync(host_buf, ctx->split.ax3.as<char>(), (size_t)need, hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    return SBO_OK;
}

SBO_API sbo_status sbo_debug_state(const sbo_ctx *ctx, int64_t *out, int cap) {
    if (!ctx || !out || cap < 0) return SBO_E_INVAL;
    const int xl = sbo::x3_layout(ctx->opt.kernel_variant), pl = precise_kernel_traits(ctx->opt.precise_kernel).layout;
    const sbo::OperandState &xs = ctx->split.state(), &ps = ctx->pop.state();
    const int64_t v[13] = {ctx->n, ctx->npad, ctx->fitted, ctx->has_factor, ctx->linv_n, ctx->z_n, ctx->probe_n,
                           xs.stale_from(xl), xs.layout(), ps.stale_from(pl), ps.layout(), ctx->pop.in_flight(),
                           (int64_t)ctx->fit_epoch};
    std::copy(v, v + std::min(cap, 13), out);
    return SBO_OK;
}

SBO_API sbo_status sbo_debug_plan(sbo_ctx *ctx, const float *qx, const float *qy, int64_t m, int32_t *host_buf,
                                  int64_t cap, int64_t *n_out) {
    if (!ctx || !n_out || cap < 0) return SBO_E_INVAL;
    SBO_CHECK(ctx->fitted, SBO_E_STATE, "sbo_debug_plan: call sbo_fit first");
    SBO_CHECK(qx && qy, SBO_E_INVAL, "sbo_debug_plan: null pointer");
    SBO_CHECK(m > 0, SBO_E_EMPTY, "sbo_debug_plan: m must be > 0");
    SBO_HIP(hipSetDevice(ctx->device));
    // the plan sbo_query_cost builds (no sweep), then its items and lists read back
    TickRequest rq;
    rq.m = m;
    rq.want = TickWant::kPlan;
    Carve c;
    if (sbo_status st = stage_queries(ctx, qx, qy, m, 0, rq, c)) return st;
    TickPlan p;
    if (sbo_status st = run_tick(ctx, rq, &p)) return st;
    const int64_t nI = p.nI, nQ = p.nQ, items = nI * nQ;
    const unsigned long long *key = nullptr, *scan = nullptr;
    const unsigned char *thr = nullptr;
    const int4 *desc = nullptr;
    const unsigned short *tl = nullptr;
    const int *seg = nullptr;
    sbo::plan_item_views(ctx->npad, p.ms, p.P, ctx->plan_work.as<void>(), &key, &scan, &thr);
    sbo::plan_views(ctx->npad, p.ms, p.P, ctx->plan_work.as<void>(), &desc, &tl, &seg);
    std::vector<unsigned long long> hkey((size_t)items);
    std::vector<unsigned char> hthr((size_t)items);
    unsigned long long last = 0;
    SBO_HIP(hipMemcpyAsync(hkey.data(), key, 8 * (size_t)items, hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipMemcpyAsync(hthr.data(), thr, (size_t)items, hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipMemcpyAsync(&last, scan + items - 1, 8, hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t total = (int64_t)sbo::plan_key_count(last), nne = sbo::plan_key_items(last);
    const int64_t need = 4 + 2 * items + 4 * total;
    *n_out = need;
    if (!host_buf) return SBO_OK;
    if (cap < need) return SBO_E_INVAL;
    std::vector<int4> hdesc((size_t)nne);
    std::vector<unsigned short> htl((size_t)total);
    if (nne) SBO_HIP(hipMemcpyAsync(hdesc.data(), desc, 16 * (size_t)nne, hipMemcpyDeviceToHost, ctx->stream));
    if (total) SBO_HIP(hipMemcpyAsync(htl.data(), tl, 2 * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    host_buf[0] = (int32_t)nI;
    host_buf[1] = (int32_t)nQ;
    host_buf[2] = (int32_t)total;
    host_buf[3] = (int32_t)nne;
    int32_t *it = host_buf + 4, *rec = it + 2 * items;
    for (int64_t I = 0; I < nI; ++I)
        for (int64_t qb = 0; qb < nQ; ++qb) {
            const int64_t item = (nI - 1 - I) * nQ + qb;   // plan_item, row-block-major
            it[2 * (I * nQ + qb)] = (int32_t)hthr[(size_t)item];
            it[2 * (I * nQ + qb) + 1] = (int32_t)sbo::plan_key_count(hkey[(size_t)item]);
        }
    int64_t r = 0;
    for (int64_t k = 0; k < nne; ++k) {
        const int4 d = hdesc[(size_t)k];
        const int cnt = sbo::plan_item_count(d.w);
        const uint64_t off = sbo::plan_item_offset(d.z, d.w);
        SBO_CHECK(off + (uint64_t)cnt <= (uint64_t)total && r + cnt <= total, SBO_E_DEVICE,
                  "sbo_debug_plan: a descriptor points outside the tile list");
        for (int i = 0; i < cnt; ++i, ++r) {
            const unsigned short te = htl[(size_t)off + i];
            rec[4 * r] = d.x;
            rec[4 * r + 1] = d.y;
            rec[4 * r + 2] = sbo::plan_entry_tile(te);
            rec[4 * r + 3] = sbo::plan_entry_level(te);
        }
    }
    SBO_CHECK(r == total, SBO_E_DEVICE, "sbo_debug_plan: the descriptors' counts do not sum to the plan's total");
    return SBO_OK;
}

namespace {
static_assert(SBO_GZ_TRI_A == sbo::kGzTriA && SBO_GZ_TRANS_A == sbo::kGzTransA &&
                  SBO_GZ_TRI_B_LOWER == sbo::kGzTriBLower && SBO_GZ_TRI_B_UPPER == sbo::kGzTriBUpper &&
                  SBO_GZ_TRANS_B == sbo::kGzTransB && SBO_GZ_TRANS_C == sbo::kGzTransC &&
                  SBO_GZ_BETA1 == sbo::kGzBeta1 && SBO_GZ_LOWER_C == sbo::kGzLowerC,
              "include/sbo.h documents the sliced GEMM's flags");
// the sliced GEMM's own argument errors (hipErrorInvalidValue) are the caller's
sbo_status gz_status(sbo_ctx *ctx, hipError_t e, const char *what) {
    if (e == hipSuccess) return SBO_OK;
    ctx->err = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorInvalidValue ? SBO_E_INVAL : e == hipErrorOutOfMemory ? SBO_E_OOM : SBO_E_DEVICE;
}
}  // namespace

SBO_API sbo_status sbo_debug_gz_gemm(sbo_ctx *ctx, int nd, int is_f32, const void *A, int64_t lda, int64_t a_cols,
                                     const void *B, int64_t ldb, int64_t b_cols, int64_t m, int64_t n, int64_t K,
                                     double alpha, void *C, int64_t ldc, int64_t c_cols, uint32_t flags) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(A && B && C, SBO_E_INVAL, "sbo_debug_gz_gemm: null operand");
    SBO_CHECK(m >= 0 && n >= 0 && K >= 0 && lda >= 1 && ldb >= 1 && ldc >= 1 && a_cols >= 1 && b_cols >= 1 &&
                  c_cols >= 1,
              SBO_E_INVAL, "sbo_debug_gz_gemm: negative size or empty buffer");
    SBO_CHECK((flags & ~255u) == 0, SBO_E_INVAL, "sbo_debug_gz_gemm: unknown flag");
    // the logical operands lie inside the buffers given (A is K x m with
    // kGzTransA, B n x K with kGzTransB, C n x m with kGzTransC)
    const bool tA = flags & sbo::kGzTransA, tB = flags & sbo::kGzTransB, tC = flags & sbo::kGzTransC;
    SBO_CHECK((tA ? K : m) <= lda && (tA ? m : K) <= a_cols && (tB ? n : K) <= ldb && (tB ? K : n) <= b_cols &&
                  (tC ? n : m) <= ldc && (tC ? m : n) <= c_cols,
              SBO_E_INVAL, "sbo_debug_gz_gemm: operand larger than its buffer");
    SBO_HIP(hipSetDevice(ctx->device));
    const size_t es = is_f32 ? sizeof(float) : sizeof(double);
    const size_t ab = es * (size_t)lda * (size_t)a_cols, bb = es * (size_t)ldb * (size_t)b_cols,
                 cb = es * (size_t)ldc * (size_t)c_cols;
    DevBuf dA, dB, dC, ws;
    SBO_HIP(dA.reserve(ab));
    SBO_HIP(dB.reserve(bb));
    SBO_HIP(dC.reserve(cb));
    SBO_HIP(ws.reserve(sbo::gz_workspace_bytes(std::max<int64_t>(m, 1), std::max<int64_t>(n, 1),
                                               std::max<int64_t>(K, 1), std::min(std::max(nd, 4), 6))));
    SBO_HIP(hipMemcpyAsync(dA.as<void>(), A, ab, hipMemcpyHostToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(dB.as<void>(), B, bb, hipMemcpyHostToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(dC.as<void>(), C, cb, hipMemcpyHostToDevice, ctx->stream));
    const hipError_t e =
        is_f32 ? sbo::launch_gz_gemm_f32(ctx->stream, nd, dA.as<float>(), lda, dB.as<float>(), ldb, m, n, K, alpha,
                                         dC.as<float>(), ldc, flags, ws.as<char>())
               : sbo::launch_gz_gemm(ctx->stream, nd, dA.as<double>(), lda, dB.as<double>(), ldb, m, n, K, alpha,
                                     dC.as<double>(), ldc, flags, ws.as<char>());
    if (e == hipSuccess) SBO_HIP(hipMemcpyAsync(C, dC.as<void>(), cb, hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    return gz_status(ctx, e, "sbo_debug_gz_gemm");
}

SBO_API sbo_status sbo_debug_gz_gemm_packed(sbo_ctx *ctx, int nd, const float *P, int64_t ld, int64_t mpack,
                                            int64_t K, int64_t a0, int64_t m, int64_t b0, int64_t n, double alpha,
                                            float *C, int64_t ldc, int64_t c_cols, uint32_t flags) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(P && C, SBO_E_INVAL, "sbo_debug_gz_gemm_packed: null operand");
    SBO_CHECK(mpack >= 1 && K >= 1 && ld >= mpack && a0 >= 0 && b0 >= 0 && m >= 0 && n >= 0 && ldc >= 1 &&
                  c_cols >= 1 && m <= ldc && n <= c_cols,
              SBO_E_INVAL, "sbo_debug_gz_gemm_packed: size out of range or C larger than its buffer");
    SBO_CHECK((flags & ~255u) == 0, SBO_E_INVAL, "sbo_debug_gz_gemm_packed: unknown flag");
    SBO_HIP(hipSetDevice(ctx->device));
    const size_t pb = sizeof(float) * (size_t)ld * (size_t)K, cb = sizeof(float) * (size_t)ldc * (size_t)c_cols;
    DevBuf dP, dC, pack;
    SBO_HIP(dP.reserve(pb));
    SBO_HIP(dC.reserve(cb));
    SBO_HIP(pack.reserve(sbo::gz_pack_bytes(mpack, K, std::min(std::max(nd, 4), 5))));
    SBO_HIP(hipMemcpyAsync(dP.as<void>(), P, pb, hipMemcpyHostToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(dC.as<void>(), C, cb, hipMemcpyHostToDevice, ctx->stream));
    hipError_t e = sbo::launch_gz_pack_f32(ctx->stream, nd, dP.as<float>(), ld, mpack, K, pack.as<char>());
    if (e == hipSuccess)
        e = sbo::launch_gz_gemm_packed_f32(ctx->stream, nd, pack.as<char>(), mpack, K, a0, m, b0, n, alpha,
                                           dC.as<float>(), ldc, flags);
    if (e == hipSuccess) SBO_HIP(hipMemcpyAsync(C, dC.as<void>(), cb, hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    return gz_status(ctx, e, "sbo_debug_gz_gemm_packed");
}

SBO_API sbo_status sbo_profile_mfma(sbo_ctx *ctx, double *mfma_flops, int64_t *tiles_by_level) {
    if (!ctx || !mfma_flops) return SBO_E_INVAL;
    unsigned long long t[4] = {0, 0, 0, 0};
    if (ctx->counters.capacity()) {
        SBO_HIP(hipMemcpyAsync(t, ctx->counters.as<void>(), sizeof(t), hipMemcpyDeviceToHost, ctx->stream));
        SBO_HIP(hipStreamSynchronize(ctx->stream));
    }
    *mfma_flops = 2.0 * sbo::kBM * sbo::kBN * sbo::kBK * (double)t[1];
    if (tiles_by_level) {
        tiles_by_level[1] = (int64_t)t[2];
        tiles_by_level[2] = (int64_t)t[3];
        tiles_by_level[0] = (int64_t)t[0] - (int64_t)(t[2] + t[3]);
    }
    return SBO_OK;
}

SBO_API sbo_status sbo_profile_read(sbo_ctx *ctx, double *predict_ms, int64_t *predict_launches, double *fill_ms,
                                    int64_t *fill_launches) {
    if (!ctx) return SBO_E_INVAL;
    auto sum = [&](const std::vector<std::pair<hipEvent_t, hipEvent_t>> &l, double *ms, int64_t *cnt) -> sbo_status {
        double t = 0.0;
        for (const auto &p : l) {
            SBO_HIP(hipEventSynchronize(p.second));
            float e = 0.f;
            SBO_HIP(hipEventElapsedTime(&e, p.first, p.second));
            t += e;
        }
        if (ms) *ms = t;
        if (cnt) *cnt = (int64_t)l.size();
        return SBO_OK;
    };
    if (sbo_status st = sum(ctx->ev_predict, predict_ms, predict_launches)) return st;
    return sum(ctx->ev_fill, fill_ms, fill_launches);
}

SBO_API sbo_status sbo_set_option(sbo_ctx *ctx, int option, int64_t value) {
    if (!ctx) return SBO_E_INVAL;
    switch (option) {
        case SBO_OPT_CHOLESKY:
            SBO_CHECK(value >= 0 && value <= 2, SBO_E_INVAL, "SBO_OPT_CHOLESKY must be 0, 1 or 2");
            ctx->opt.chol_blocked = value != 0;
            ctx->opt.chol_trsm_own = value == 1;
            return SBO_OK;
        case SBO_OPT_JITTER_RETRIES:
            SBO_CHECK(value >= 0 && value <= 8, SBO_E_INVAL, "SBO_OPT_JITTER_RETRIES must be in [0, 8]");
            ctx->opt.jitter_retries = (int)value;
            return SBO_OK;
        case SBO_OPT_INVERSE:
            SBO_CHECK(value == 0 || value == 1, SBO_E_INVAL, "SBO_OPT_INVERSE must be 0 or 1");
            ctx->opt.inverse_rec = value != 0;
            return SBO_OK;
        case SBO_OPT_INVERSE_BITS:
            SBO_CHECK(value == 32 || value == 64, SBO_E_INVAL, "SBO_OPT_INVERSE_BITS must be 32 or 64");
            ctx->opt.inverse_bits = (int)value;
            return SBO_OK;
        case SBO_OPT_SPATIAL_ORDER:
            SBO_CHECK(value >= 0 && value <= 3, SBO_E_INVAL, "SBO_OPT_SPATIAL_ORDER must be 0, 1, 2 or 3");
            ctx->opt.spatial_order = (int)value;
            return SBO_OK;
        case SBO_OPT_QUERY_ORDER:
            SBO_CHECK(value >= 0 && value <= 2, SBO_E_INVAL, "SBO_OPT_QUERY_ORDER must be 0, 1 or 2");
            ctx->opt.query_order = (int)value;
            return SBO_OK;
        case SBO_OPT_SKIP_BUDGET:
            SBO_CHECK(value >= 10 && value <= 60, SBO_E_INVAL, "SBO_OPT_SKIP_BUDGET must be in [10, 60]");
            ctx->opt.skip_budget = (int)value;
            return SBO_OK;
        case SBO_OPT_SWEEP_GROUPS:
            SBO_CHECK(value >= 0 && value <= 65536, SBO_E_INVAL, "SBO_OPT_SWEEP_GROUPS must be in [0, 65536]");
            ctx->opt.sweep_groups = (int)value;
            return SBO_OK;
        case SBO_OPT_KERNEL_VARIANT:
            SBO_CHECK(sbo::variant_allowed((int)value), SBO_E_INVAL,
                      "SBO_OPT_KERNEL_VARIANT: not a sweep of this build (product: 0, 1, 3, 22)");
            ctx->opt.kernel_variant = (int)value;
            return SBO_OK;
        case SBO_OPT_INV_BASE:
            SBO_CHECK(value >= 1024 && value <= 8192, SBO_E_INVAL, "SBO_OPT_INV_BASE must be in [1024, 8192]");
            ctx->opt.inv_base = value / 128 * 128;   // (the split lands on multiples of it: Cholesky block columns)
            return SBO_OK;
        case SBO_OPT_INV_LEAVES:
            SBO_CHECK(value >= 0 && value <= 2, SBO_E_INVAL, "SBO_OPT_INV_LEAVES must be 0, 1 or 2");
            ctx->opt.inv_batched = value >= 1;
            ctx->opt.inv_leaves_own = value == 2;
            return SBO_OK;
        case SBO_OPT_INV_PANELS:
            SBO_CHECK(value >= 1 && value <= 64, SBO_E_INVAL, "SBO_OPT_INV_PANELS must be in [1, 64]");
            ctx->opt.inv_panels = value;
            return SBO_OK;
        case SBO_OPT_CHOL_GEMM:
#ifdef SBO_DIAG
            SBO_CHECK(value >= 0 && value <= 5, SBO_E_INVAL, "SBO_OPT_CHOL_GEMM must be in [0, 5] (diagnostics)");
#else
            // (3, the split-bf16 updates, only in the diagnostic build: a worse
            // factor on ill-conditioned K)
            SBO_CHECK(value >= 0 && value <= 5 && value != 3, SBO_E_INVAL,
                      "SBO_OPT_CHOL_GEMM must be 0, 1, 2, 4 or 5");
#endif
            ctx->opt.chol_gemm_own = (int)value;
            return SBO_OK;
        case SBO_OPT_CHOL_DIAG:
            SBO_CHECK(value >= 0 && value <= 2, SBO_E_INVAL, "SBO_OPT_CHOL_DIAG must be 0, 1 or 2");
            ctx->opt.chol_diag = (int)value;
            return SBO_OK;
        case SBO_OPT_CHOL_OUTER:
            SBO_CHECK(value >= sbo::kCholNB && value <= 4096 && value % sbo::kCholNB == 0, SBO_E_INVAL,
                      "SBO_OPT_CHOL_OUTER must be a multiple of 128 in [128, 4096]");
            ctx->opt.chol_outer = (int)value;
            return SBO_OK;
        case SBO_OPT_INV_OVERLAP:
            SBO_CHECK(value >= 0 && value < ctx->num_cu, SBO_E_INVAL,
                      "SBO_OPT_INV_OVERLAP must be in [0, compute units)");
            ctx->opt.inv_overlap = (int)value;
            return SBO_OK;
        case SBO_OPT_CHOL_RESERVE:
            SBO_CHECK(value >= 0 && value < ctx->num_cu, SBO_E_INVAL,
                      "SBO_OPT_CHOL_RESERVE must be in [0, compute units)");
            ctx->opt.chol_reserve = (int)value;
            return SBO_OK;
        case SBO_OPT_PRECISE_KERNEL:
#ifdef SBO_DIAG
            SBO_CHECK(value == 0 || value == 1 || (value >= 3 && value <= 5) || (value >= 9 && value <= 12),
                      SBO_E_INVAL, "SBO_OPT_PRECISE_KERNEL: 0, 1, 3, 4, 5 or 9-12 (diagnostics)");
#else
            SBO_CHECK(value == 0 || value == 1 || value == 3 || value == 4, SBO_E_INVAL,
                      "SBO_OPT_PRECISE_KERNEL must be 0 (f64 MFMA), 1 (int8), 3 (int8, K* table) or 4 (int8, "
                      "k-tile pairs)");
#endif
            ctx->opt.precise_kernel = (int)value;   // (another layout: the operand derives all of it, PreciseOperand)
            return SBO_OK;
        case SBO_OPT_INV_OZ:
            SBO_CHECK(value == 0 || (value >= 4 && value <= 6), SBO_E_INVAL, "SBO_OPT_INV_OZ must be 0, 4, 5 or 6");
            ctx->opt.inv_oz = (int)value;
            ctx->inv_oz_cur = ctx->inv_oz_next = 0;
            ctx->inv_oz_pinned = false;
            return SBO_OK;
        case SBO_OPT_INV_OZ_ADAPT:
            SBO_CHECK(value == 0 || value == 1, SBO_E_INVAL, "SBO_OPT_INV_OZ_ADAPT must be 0 or 1");
            ctx->opt.inv_oz_adapt = (int)value;
            ctx->inv_oz_next = 0;
            ctx->inv_oz_pinned = false;
            return SBO_OK;
        case SBO_OPT_INV_OZ_MIN:
            SBO_CHECK(value == 0 || value == 2048 || value == 4096 || value == 8192, SBO_E_INVAL,
                      "SBO_OPT_INV_OZ_MIN must be 0 (automatic), 2048, 4096 or 8192");
            ctx->opt.inv_oz_min = value;
            return SBO_OK;
        case SBO_OPT_PROBE_SIZE:
            SBO_CHECK(value >= 0 && (value >> 16) >= 4 && (value >> 16) <= 256 && (value & 0xffff) >= 1 &&
                          (value & 0xffff) <= 16384,
                      SBO_E_INVAL, "SBO_OPT_PROBE_SIZE must be grid << 16 | train (grid 4..256, train 1..16384)");
            ctx->opt.probe_grid = (int)(value >> 16);
            ctx->opt.probe_train = (int)(value & 0xffff);
            ctx->probe_n = 0;   // probe again at the next refresh
            return SBO_OK;
        case SBO_OPT_PLAN_BLOCK:
            SBO_CHECK(value == 0 || ((value >> 8) >= 1 && (value >> 8) <= 64 && (value & 255) >= 1), SBO_E_INVAL,
                      "SBO_OPT_PLAN_BLOCK must be 0 or bi << 8 | bq with 1 <= bi <= 64, 1 <= bq <= 255");
            ctx->opt.plan_block = (int)value;
            return SBO_OK;
        case SBO_OPT_INV_CHECK:
            SBO_CHECK(value >= 0 && value <= 2, SBO_E_INVAL, "SBO_OPT_INV_CHECK must be 0, 1 or 2");
            ctx->opt.inv_check = (int)value;
            return SBO_OK;
        case SBO_OPT_TABLE_MB:
            SBO_CHECK(value >= 0 && value <= (int64_t(1) << 20), SBO_E_INVAL,
                      "SBO_OPT_TABLE_MB must be in [0, 2^20] (0: automatic)");
            ctx->opt.table_mb = value;
            return SBO_OK;
        case SBO_OPT_REPROBE:
            SBO_CHECK(value >= 0 && value <= 1000, SBO_E_INVAL, "SBO_OPT_REPROBE must be in [0, 1000] (percent)");
            ctx->opt.reprobe_pct = (int)value;
            return SBO_OK;
        case SBO_OPT_RESORT:
            SBO_CHECK(value >= 0 && value <= 1000, SBO_E_INVAL, "SBO_OPT_RESORT must be in [0, 1000] (percent)");
            ctx->opt.resort_pct = (int)value;
            return SBO_OK;
        case SBO_OPT_PRECISION:
            SBO_CHECK(value >= -1 && value <= 1, SBO_E_INVAL, "SBO_OPT_PRECISION must be -1 (auto), 0 or 1");
            if (ctx->fitted) {
                // takes effect at once: a first auto probe now, or the forced choice
                const bool avail = ctx->has_factor && inverse_current(ctx, ctx->n);
                SBO_CHECK(value != 1 || avail, SBO_E_STATE,
                          "SBO_OPT_PRECISION 1: needs the fit's f64 inverse (not an imported state)");
                ctx->opt.precision_opt = (int)value;
                if (value != 0 && avail) {
                    SBO_HIP(hipSetDevice(ctx->device));
                    if (sbo_status st = probe_precision(ctx, ctx->opt.precision_opt)) return st;
                } else {
                    ctx->precise = false;
                }
                return SBO_OK;
            }
            ctx->opt.precision_opt = (int)value;
            return SBO_OK;
        case SBO_OPT_STREAM_SHARE:
            SBO_CHECK(value >= 0 && value <= 20, SBO_E_INVAL, "SBO_OPT_STREAM_SHARE must be in [0, 20]");
            ctx->opt.stream_share = (int)value;
            return SBO_OK;
        case SBO_OPT_STREAM_MAX_ROWS:
            SBO_CHECK(value >= 0 && value <= 65536, SBO_E_INVAL, "SBO_OPT_STREAM_MAX_ROWS must be in [0, 65536]");
            ctx->opt.stream_max_rows = value;
            return SBO_OK;
        case SBO_OPT_EVIDENCE_BUDGET:
            SBO_CHECK(value == 0 || (value >= 10 && value <= 60), SBO_E_INVAL,
                      "SBO_OPT_EVIDENCE_BUDGET must be 0 (dense) or in [10, 60]");
            ctx->opt.evidence_budget = (int)value;
            return SBO_OK;
        case SBO_OPT_WHATIF_GEMM:
            SBO_CHECK(value == 0 || value == 1, SBO_E_INVAL, "SBO_OPT_WHATIF_GEMM must be 0 (dtrmm) or 1 (dgemm)");
            ctx->opt.whatif_gemm = (int)value;
            return SBO_OK;
        case SBO_OPT_REMOVE_MAX:
            SBO_CHECK(value >= 0 && value <= 65536, SBO_E_INVAL, "SBO_OPT_REMOVE_MAX must be in [0, 65536]");
            ctx->opt.remove_max = value;
            return SBO_OK;
        case SBO_OPT_TILE_SKIP:
            SBO_CHECK(value == -1 || value == 0 || (value >= 16 && value <= 1000), SBO_E_INVAL,
                      "SBO_OPT_TILE_SKIP must be -1 (auto), 0 (dense) or a cutoff exponent in [16, 1000]");
            ctx->opt.skip_log2 = (int)value;
            return SBO_OK;
    }
    ctx->err = "unknown option " + std::to_string(option);
    return SBO_E_INVAL;
}

SBO_API sbo_status sbo_get_precision(const sbo_ctx *ctx, int *precise, double *probe_err, double *probe_var_min,
                                     double *probe_var_max) {
    if (!ctx) return SBO_E_INVAL;
    if (!ctx->fitted) return SBO_E_STATE;
    if (precise) *precise = ctx->precise ? 1 : 0;
    if (probe_err) *probe_err = ctx->probe_n ? ctx->probe_err : -1.0;
    if (probe_var_min) *probe_var_min = ctx->probe_n ? ctx->probe_vmin : -1.0;
    if (probe_var_max) *probe_var_max = ctx->probe_n ? ctx->probe_vmax : -1.0;
    return SBO_OK;
}

SBO_API sbo_status sbo_trim(sbo_ctx *ctx) {
    if (!ctx) return SBO_E_INVAL;
    SBO_HIP(hipSetDevice(ctx->device));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->aux_stream) SBO_HIP(hipStreamSynchronize(ctx->aux_stream));
    if (ctx->inv_stream) SBO_HIP(hipStreamSynchronize(ctx->inv_stream));
    if (ctx->chk_stream) SBO_HIP(hipStreamSynchronize(ctx->chk_stream));
    ctx->ws.release();
    return SBO_OK;
}

SBO_API sbo_status sbo_warmup(sbo_ctx *ctx, int64_t n_cap, int64_t m_cap, sbo_hyper hyper) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(n_cap > 0 && m_cap > 0, SBO_E_EMPTY, "sbo_warmup: n_cap and m_cap must be > 0");
    SBO_CHECK(n_cap < (int64_t)1 << 30 && m_cap < (int64_t)1 << 31, SBO_E_INVAL, "sbo_warmup: sizes too large");
    if (sbo_status st = check_hyper(ctx, hyper)) return st;
    SBO_HIP(hipSetDevice(ctx->device));
    // n_cap points uniform over a square of about 8 points per l^2 (the C2-C5
    // density: a well-conditioned fit), a smooth field as observations
    const double side = hyper.length_scale * std::sqrt((double)n_cap / 8.0);
    std::vector<float> hx((size_t)n_cap), hy((size_t)n_cap), ho((size_t)n_cap);
    uint64_t z = 0x9E3779B97F4A7C15ull;
    auto next = [&z]() {   // SplitMix64 -> [0, 1)
        uint64_t v = (z += 0x9E3779B97F4A7C15ull);
        v = (v ^ (v >> 30)) * 0xBF58476D1CE4E5B9ull;
        v = (v ^ (v >> 27)) * 0x94D049BB133111EBull;
        return (double)((v ^ (v >> 31)) >> 11) * 0x1.0p-53;
    };
    for (int64_t i = 0; i < n_cap; ++i) {
        hx[(size_t)i] = (float)(next() * side);
        hy[(size_t)i] = (float)(next() * side);
        ho[(size_t)i] = (float)(std::sin(hx[(size_t)i] / hyper.length_scale) +
                                std::cos(0.7 * hy[(size_t)i] / hyper.length_scale));
    }
    sbo_status st = sbo_fit(ctx, hx.data(), hy.data(), ho.data(), n_cap, hyper, 0);
    // an m_cap-point raster over the square (the grid-patch query path), swept
    // with both sweeps; device buffers so that the tick's own workspaces are
    // what gets sized
    const int64_t w = std::max<int64_t>(1, (int64_t)std::ceil(std::sqrt((double)m_cap)));
    const int64_t h = (m_cap + w - 1) / w, m = w * h;
    DevBuf dq, dk;
    if (st == SBO_OK) {
        std::vector<float> gq(2 * (size_t)m);
        for (int64_t i = 0; i < h; ++i)
            for (int64_t j = 0; j < w; ++j) {
                gq[(size_t)(i * w + j)] = (float)(side * (double)j / (double)std::max<int64_t>(w - 1, 1));
                gq[(size_t)(m + i * w + j)] = (float)(side * (double)i / (double)std::max<int64_t>(h - 1, 1));
            }
        if (dq.reserve(sizeof(float) * 2 * (size_t)m) != hipSuccess || dk.reserve(sizeof(sbo_key)) != hipSuccess ||
            hipMemcpy(dq.as<float>(), gq.data(), sizeof(float) * 2 * (size_t)m, hipMemcpyHostToDevice) != hipSuccess)
            st = SBO_E_OOM;
    }
    for (int prec = 0; prec <= 1 && st == SBO_OK; ++prec) {
        if (prec == 1 && !inverse_current(ctx, ctx->n)) break;
        if ((st = probe_precision(ctx, prec)) != SBO_OK) break;
        st = sbo_tick(ctx, dq.as<float>(), dq.as<float>() + m, m, 2.0, 0.0, SBO_SCORE_WIDTH, 0, nullptr, nullptr,
                      nullptr, nullptr, nullptr, dk.as<sbo_key>(), SBO_DEVICE_PTRS);
    }
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    // unfitted again; the workspaces keep their sizes (the query buffers go:
    // forget the grid layout cached by their addresses)
    unfit(ctx);
    ctx->inv_oz_next = 0;   // (the synthetic fit's guard reading says nothing about the real data)
    ctx->inv_oz_hist_n = 0;
    ctx->inv_oz_pinned = false;
    ctx->qgrid_x = ctx->qgrid_y = nullptr;
    ctx->qgrid_m = -1;
    ctx->hyper = sbo_hyper{0.4, 1.0, 0.1, 0.0};
    return st;
}

SBO_API sbo_status sbo_get_inverse_check(const sbo_ctx *ctx, sbo_inv_check *out) {
    if (!ctx || !out) return SBO_E_INVAL;
    if (!ctx->fitted) return SBO_E_STATE;
    *out = ctx->chk_res;
    return SBO_OK;
}

SBO_API sbo_status sbo_get_probe(const sbo_ctx *ctx, sbo_probe *out) {
    if (!ctx || !out) return SBO_E_INVAL;
    if (!ctx->fitted) return SBO_E_STATE;
    *out = sbo_probe{};
    out->precise = ctx->precise ? 1 : 0;
    out->precise_kernel = ctx->opt.precise_kernel;
    out->n_at_probe = ctx->probe_n;
    if (ctx->probe_n == 0) {
        out->err = out->err_grid = out->err_train = -1.0;
        return SBO_OK;
    }
    out->m_grid = ctx->probe_m_grid;
    out->m_train = ctx->probe_m_train;
    out->err = ctx->probe_err;
    out->err_grid = ctx->probe_err_grid;
    out->err_train = ctx->probe_err_train;
    out->var_min = ctx->probe_vmin;
    out->var_max = ctx->probe_vmax;
    out->var_max_grid = ctx->probe_vmax_grid;
    out->var_max_train = ctx->probe_vmax_train;
    return SBO_OK;
}

SBO_API sbo_status sbo_get_skip(const sbo_ctx *ctx, int *cutoff_log2, double *max_row_l1, double *alpha_l1) {
    if (!ctx) return SBO_E_INVAL;
    if (cutoff_log2) *cutoff_log2 = ctx->opt.skip_log2 < 0 ? ctx->auto_skip_log2 : ctx->opt.skip_log2;
    if (max_row_l1) *max_row_l1 = ctx->max_row_l1;
    if (alpha_l1) *alpha_l1 = ctx->alpha_l1;
    return SBO_OK;
}

SBO_API sbo_status sbo_get_order(const sbo_ctx *ctx, int64_t *order) {
    if (!ctx || !order) return SBO_E_INVAL;
    if (!ctx->fitted) return SBO_E_STATE;
    std::copy(ctx->order.begin(), ctx->order.begin() + ctx->n, order);
    return SBO_OK;
}

SBO_API sbo_status sbo_kd_order(const float *x, const float *y, int64_t n, int64_t first_offset, int64_t *perm) {
    if (n < 0 || (n > 0 && (!x || !y || !perm)) || first_offset < 0) return SBO_E_INVAL;
    if (n == 0) return SBO_OK;
    try {
        std::vector<float> hx(x, x + n), hy(y, y + n);
        for (int64_t i = 0; i < n; ++i) perm[i] = i;
        kd_order(hx, hy, perm, n, first_offset % sbo::kBK);
    } catch (...) {
        return SBO_E_OOM;
    }
    return SBO_OK;
}

SBO_API sbo_status sbo_get_inverse(sbo_ctx *ctx, float *Linv) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(ctx->fitted && Linv, SBO_E_STATE, "sbo_get_inverse: call sbo_fit first");
    SBO_HIP(hipSetDevice(ctx->device));
    const int64_t n = ctx->n, npad = ctx->npad;
    // unpack the packed operand tiles (rows of sf2 * L^-1) on the host
    const int64_t nI = npad / sbo::kBM;
    const size_t tiles = (size_t)sbo::total_tiles(nI);
    std::vector<float> h(tiles * sbo::kTileFloats);
    SBO_HIP(hipMemcpyAsync(h.data(), ctx->aug.as<float>(), sizeof(float) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    for (int64_t I = 0; I < nI; ++I)
        for (int64_t kb = 0; kb < (I + 1) * sbo::kTilesPerRowBlockStep; ++kb) {
            const float *t = h.data() + (sbo::tile_start(I) + kb) * sbo::kTileFloats;
            for (int k = 0; k < sbo::kBK; ++k)
                for (int r = 0; r < sbo::kBM; ++r) {
                    const int64_t row = I * sbo::kBM + r, col = kb * sbo::kBK + k;
                    if (row < n && col < n) Linv[row * n + col] = t[sbo::tile_offset(k, r)];
                }
        }
    return SBO_OK;
}

SBO_API sbo_status sbo_get_tile_bounds(sbo_ctx *ctx, float *bounds, int64_t cap) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(ctx->fitted && bounds, SBO_E_STATE, "sbo_get_tile_bounds: call sbo_fit first");
    const int64_t need = 8 * sbo::total_tiles(ctx->npad / sbo::kBM);
    SBO_CHECK(cap >= need, SBO_E_INVAL, "sbo_get_tile_bounds: cap < 8 floats per packed tile");
    SBO_HIP(hipSetDevice(ctx->device));
    SBO_HIP(hipMemcpyAsync(bounds, ctx->tile_lgn.as<void>(), sizeof(float) * (size_t)need, hipMemcpyDeviceToHost,
                           ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    return SBO_OK;
}

}  // extern "C"

// ----------------------------------------------------------- frontier 8(f)1
namespace {

// Device raster + host border following; F = frontier grid indices in the
// node's order.  Returns SBO_OK with F filled (possibly empty).
sbo_status device_frontier(sbo_ctx *ctx, const double *Dx, const double *Dy, const uint8_t *safe, int64_t m,
                           int width, int height, const double *lo, const double *hi, std::vector<int32_t> &F,
                           std::vector<double> &cols) {
    F.clear();
    cols.clear();
    if (m <= 0 || width <= 0 || height <= 0) return SBO_OK;  // "D_ or S_ is empty" (:419-422)
    SBO_CHECK(m <= INT32_MAX, SBO_E_INVAL, "frontier: m must fit int32 (grid indices)");
    const int64_t npx = (int64_t)width * height;
    SBO_HIP(ctx->fwork.reserve(sbo::frontier_work_bytes(m)));
    SBO_HIP(ctx->fowner.reserve(sizeof(int32_t) * (size_t)npx));
    SBO_HIP(ctx->fimg.reserve((size_t)npx));
    SBO_HIP(sbo::launch_frontier_raster(ctx->stream, Dx, Dy, safe, m, width, height, ctx->fwork.as<void>(),
                                        ctx->fowner.as<int32_t>(), ctx->fimg.as<uint8_t>()));
    std::vector<uint8_t> img((size_t)npx);
    SBO_HIP(hipMemcpyAsync(img.data(), ctx->fimg.as<uint8_t>(), (size_t)npx, hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<int32_t> pix;
    sbo::trace_external_pixels(img.data(), width, height, pix);
    const int64_t nf = (int64_t)pix.size();
    if (nf == 0) return SBO_OK;
    SBO_HIP(ctx->fpix.reserve(sizeof(int32_t) * (size_t)nf));
    const size_t fbytes = (size_t)sbo::round_up((int64_t)sizeof(int32_t) * nf, 8);
    SBO_HIP(ctx->fout.reserve(fbytes + 4 * sizeof(double) * (size_t)nf));
    int32_t *dF = ctx->fout.as<int32_t>();
    double *dcols = reinterpret_cast<double *>(ctx->fout.as<char>() + fbytes);
    SBO_HIP(hipMemcpyAsync(ctx->fpix.as<int32_t>(), pix.data(), sizeof(int32_t) * nf, hipMemcpyHostToDevice,
                           ctx->stream));
    SBO_HIP(sbo::launch_frontier_gather(ctx->stream, ctx->fpix.as<int32_t>(), nf, ctx->fowner.as<int32_t>(), Dx, Dy,
                                        lo, hi, dF, dcols));
    F.resize((size_t)nf);
    SBO_HIP(hipMemcpyAsync(F.data(), dF, sizeof(int32_t) * nf, hipMemcpyDeviceToHost, ctx->stream));
    if (lo) {
        cols.resize((size_t)(4 * nf));
        SBO_HIP(hipMemcpyAsync(cols.data(), dcols, sizeof(double) * 4 * nf, hipMemcpyDeviceToHost, ctx->stream));
    }
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    return SBO_OK;
}

}  // namespace

extern "C" {

SBO_API sbo_status sbo_frontier(sbo_ctx *ctx, const double *Dx, const double *Dy, const uint8_t *safe, int64_t m,
                                int width_cells, int height_cells, int32_t *out, int64_t out_cap, int64_t *count,
                                uint32_t flags) {
    if (!ctx || !count) return SBO_E_INVAL;
    *count = 0;
    SBO_CHECK(m >= 0, SBO_E_INVAL, "sbo_frontier: m must be >= 0");
    if (m == 0) return SBO_OK;
    SBO_CHECK(Dx && Dy && safe, SBO_E_INVAL, "sbo_frontier: null input");
    if (!dev(flags))
        return sbo_find_safety_contour_indices(Dx, Dy, safe, m, width_cells, height_cells, out, out_cap, count);
    SBO_HIP(hipSetDevice(ctx->device));
    std::vector<int32_t> F;
    std::vector<double> cols;
    if (sbo_status st = device_frontier(ctx, Dx, Dy, safe, m, width_cells, height_cells, nullptr, nullptr, F, cols))
        return st;
    *count = (int64_t)F.size();
    SBO_CHECK((int64_t)F.size() <= out_cap && (out || F.empty()), SBO_E_INVAL,
              "sbo_frontier: out_cap too small (count holds the size)");
    std::copy(F.begin(), F.end(), out);
    return SBO_OK;
}

SBO_API sbo_status sbo_subgoal(sbo_ctx *ctx, const double *Dx, const double *Dy, const double *lo, const double *hi,
                               const uint8_t *safe, int64_t m, int width_cells, int height_cells, double goal_x,
                               double goal_y, int64_t *index, uint32_t flags) {
    if (!ctx || !index) return SBO_E_INVAL;
    *index = -1;
    SBO_CHECK(m >= 0, SBO_E_INVAL, "sbo_subgoal: m must be >= 0");
    if (m == 0) return SBO_OK;
    SBO_CHECK(Dx && Dy && lo && hi && safe, SBO_E_INVAL, "sbo_subgoal: null input");
    if (!dev(flags)) {
        *index = sbo_next_subgoal(Dx, Dy, lo, hi, safe, m, width_cells, height_cells, goal_x, goal_y);
        return SBO_OK;
    }
    SBO_HIP(hipSetDevice(ctx->device));
    std::vector<int32_t> F;
    std::vector<double> cols;
    if (sbo_status st = device_frontier(ctx, Dx, Dy, safe, m, width_cells, height_cells, lo, hi, F, cols)) return st;
    const size_t nf = F.size();
    const int64_t b = sbo::select_subgoal(nf, cols.data(), cols.data() + nf, cols.data() + 2 * nf,
                                          cols.data() + 3 * nf, goal_x, goal_y);
    *index = b >= 0 ? F[(size_t)b] : -1;
    return SBO_OK;
}

}  // extern "C"

// ------------------------------------------------- fitted state, 8(e)
namespace {

constexpr uint64_t kStateMagic = 0x3553544154534253ull;  // "SBSTATS5" (tile and piece norms, 32 B per tile)

struct StateHeader {
    uint64_t magic;
    int64_t n, npad;
    double hyper[4];
    double max_row_l1, alpha_l1;
    float bbox[4];
    int32_t auto_skip_log2, spatial_order, auto_skip_mean_log2;
    float lg_tau_v;
    int64_t off_order, off_aug, off_kcoord, off_kbox, off_lgn, total;
};

static_assert(offsetof(StateHeader, off_aug) == 112 && sizeof(StateHeader) <= 256,
              "state blob header layout (tests/test_gpu_parity.py tampers off_aug at byte 112)");

// Section offsets of a blob holding n points (npad = round_up(n, kBM)):
// export writes them, import recomputes them from (n, npad) and rejects any
// blob whose stored offsets disagree.
void state_offsets(StateHeader &h) {
    const int64_t nt = h.npad / sbo::kBK;
    h.off_order = 256;
    h.off_aug = sbo::round_up(h.off_order + 8 * h.n, 256);
    h.off_kcoord = sbo::round_up(h.off_aug + 4 * sbo::total_tiles(h.npad / sbo::kBM) * sbo::kTileFloats, 256);
    h.off_kbox = sbo::round_up(h.off_kcoord + 4 * nt * 3 * sbo::kBK, 256);
    h.off_lgn = sbo::round_up(h.off_kbox + 16 * nt, 256);
    h.total = sbo::round_up(h.off_lgn + 32 * sbo::total_tiles(h.npad / sbo::kBM), 256);
}

StateHeader state_layout(const sbo_ctx *ctx) {
    StateHeader h{};
    h.magic = kStateMagic;
    h.n = ctx->n;
    h.npad = ctx->npad;
    h.hyper[0] = ctx->hyper.length_scale;
    h.hyper[1] = ctx->hyper.sigma_f;
    h.hyper[2] = ctx->hyper.noise_level;
    h.hyper[3] = ctx->hyper.prior_mean;
    h.max_row_l1 = ctx->max_row_l1;
    h.alpha_l1 = ctx->alpha_l1;
    for (int i = 0; i < 4; ++i) h.bbox[i] = ctx->bbox[i];
    h.auto_skip_log2 = ctx->auto_skip_log2;
    h.auto_skip_mean_log2 = ctx->auto_skip_mean_log2;
    h.lg_tau_v = ctx->lg_tau_v;
    h.spatial_order = ctx->opt.spatial_order;
    state_offsets(h);
    return h;
}

}  // namespace

extern "C" {

SBO_API sbo_status sbo_get_bounds(const sbo_ctx *ctx, double *bounds) {
    if (!ctx || !bounds) return SBO_E_INVAL;
    if (!ctx->fitted) return SBO_E_STATE;
    for (int i = 0; i < 4; ++i) bounds[i] = (double)ctx->bbox[i];
    return SBO_OK;
}

SBO_API sbo_status sbo_state_bytes(sbo_ctx *ctx, int64_t *bytes) {
    if (!ctx || !bytes) return SBO_E_INVAL;
    SBO_CHECK(ctx->fitted, SBO_E_STATE, "sbo_state_bytes: call sbo_fit first");
    *bytes = state_layout(ctx).total;
    return SBO_OK;
}

SBO_API sbo_status sbo_export_state(sbo_ctx *ctx, void *dev_buf, int64_t cap) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(ctx->fitted, SBO_E_STATE, "sbo_export_state: call sbo_fit first");
    const StateHeader h = state_layout(ctx);
    SBO_CHECK(dev_buf && cap >= h.total, SBO_E_INVAL, "sbo_export_state: buffer smaller than sbo_state_bytes");
    SBO_HIP(hipSetDevice(ctx->device));
    char *b = static_cast<char *>(dev_buf);
    const int64_t nt = ctx->npad / sbo::kBK;
    SBO_HIP(hipMemcpyAsync(b, &h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(b + h.off_order, ctx->order.data(), 8 * (size_t)h.n, hipMemcpyHostToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(b + h.off_aug, ctx->aug.as<void>(),
                           4 * (size_t)sbo::total_tiles(ctx->npad / sbo::kBM) * sbo::kTileFloats,
                           hipMemcpyDeviceToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(b + h.off_kcoord, ctx->kcoord.as<void>(), 4 * (size_t)nt * 3 * sbo::kBK,
                           hipMemcpyDeviceToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(b + h.off_kbox, ctx->kbox.as<void>(), 16 * (size_t)nt, hipMemcpyDeviceToDevice,
                           ctx->stream));
    SBO_HIP(hipMemcpyAsync(b + h.off_lgn, ctx->tile_lgn.as<void>(),
                           32 * (size_t)sbo::total_tiles(ctx->npad / sbo::kBM), hipMemcpyDeviceToDevice, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));  // the header and order live on this host stack
    return SBO_OK;
}

SBO_API sbo_status sbo_import_state(sbo_ctx *ctx, const void *dev_buf, int64_t bytes) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(dev_buf && bytes >= (int64_t)sizeof(StateHeader), SBO_E_INVAL, "sbo_import_state: bad buffer");
    SBO_HIP(hipSetDevice(ctx->device));
    if (sbo_status st = ctx->pop.drain(ctx)) return st;   // (a precise pack may still read x, y, L^-1, alpha64)
    const char *b = static_cast<const char *>(dev_buf);
    StateHeader h;
    SBO_HIP(hipMemcpyAsync(&h, b, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    SBO_CHECK(h.magic == kStateMagic && h.n > 0 && h.n <= (int64_t)1 << 32 && h.npad == sbo::round_up(h.n, sbo::kBM),
              SBO_E_INVAL, "sbo_import_state: not an sbo state blob");
    {
        StateHeader e = h;
        state_offsets(e);
        SBO_CHECK(e.off_order == h.off_order && e.off_aug == h.off_aug && e.off_kcoord == h.off_kcoord &&
                      e.off_kbox == h.off_kbox && e.off_lgn == h.off_lgn && e.total == h.total,
                  SBO_E_INVAL, "sbo_import_state: section offsets do not match the blob's (n, npad)");
        SBO_CHECK(h.total <= bytes, SBO_E_INVAL, "sbo_import_state: truncated blob");
        SBO_CHECK(h.spatial_order >= 0 && h.spatial_order <= 3 && std::isfinite(h.lg_tau_v) &&
                      h.bbox[0] <= h.bbox[1] && h.bbox[2] <= h.bbox[3],
                  SBO_E_INVAL, "sbo_import_state: header fields out of range");
        // the hyper-parameters (noise_level carries the exporter's jitter) pass the fit's own checks
        const sbo_hyper hh{h.hyper[0], h.hyper[1], h.hyper[2], h.hyper[3]};
        if (sbo_status st = check_hyper(ctx, hh)) {
            ctx->err = "sbo_import_state: " + ctx->err;
            return st;
        }
    }
    FitCommit fc(ctx);
    // no factor and no f64 inverse travel: an imported state ticks with the
    // fast sweep and derives its split operand at the first tick
    unfit(ctx);
    const int64_t nt = h.npad / sbo::kBK;
    const size_t aug_bytes = 4 * (size_t)sbo::total_tiles(h.npad / sbo::kBM) * sbo::kTileFloats;
    SBO_HIP(ctx->aug.reserve(aug_bytes));
    SBO_HIP(ctx->kcoord.reserve(4 * (size_t)nt * 3 * sbo::kBK));
    SBO_HIP(ctx->kbox.reserve(16 * (size_t)nt));
    SBO_HIP(ctx->tile_lgn.reserve(32 * (size_t)sbo::total_tiles(h.npad / sbo::kBM)));
    ctx->order.resize((size_t)h.n);
    SBO_HIP(hipMemcpyAsync(ctx->order.data(), b + h.off_order, 8 * (size_t)h.n, hipMemcpyDeviceToHost, ctx->stream));
    SBO_HIP(hipMemcpyAsync(ctx->aug.as<void>(), b + h.off_aug, aug_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(ctx->kcoord.as<void>(), b + h.off_kcoord, 4 * (size_t)nt * 3 * sbo::kBK,
                           hipMemcpyDeviceToDevice, ctx->stream));
    SBO_HIP(hipMemcpyAsync(ctx->kbox.as<void>(), b + h.off_kbox, 16 * (size_t)nt, hipMemcpyDeviceToDevice,
                           ctx->stream));
    SBO_HIP(hipMemcpyAsync(ctx->tile_lgn.as<void>(), b + h.off_lgn, 32 * (size_t)sbo::total_tiles(h.npad / sbo::kBM),
                           hipMemcpyDeviceToDevice, ctx->stream));
    if (sbo_status st = refresh_colmax(ctx, h.npad)) return st;
    SBO_HIP(hipStreamSynchronize(ctx->stream));
    {   // the order must be a permutation of 0..n-1 (it indexes the caller's arrays)
        std::vector<uint8_t> seen((size_t)h.n, 0);
        for (int64_t v : ctx->order) {
            if (v < 0 || v >= h.n || seen[(size_t)v]) {
                ctx->err = "sbo_import_state: training order is not a permutation";
                return SBO_E_INVAL;
            }
            seen[(size_t)v] = 1;
        }
    }
    ctx->n = h.n;
    ctx->npad = h.npad;
    ctx->hyper = sbo_hyper{h.hyper[0], h.hyper[1], h.hyper[2], h.hyper[3]};
    ctx->jitter = 0.0;  // an exporter's jitter is already part of the imported noise term
    ctx->max_row_l1 = h.max_row_l1;
    ctx->alpha_l1 = h.alpha_l1;
    for (int i = 0; i < 4; ++i) ctx->bbox[i] = h.bbox[i];
    ctx->auto_skip_log2 = h.auto_skip_log2;
    ctx->auto_skip_mean_log2 = h.auto_skip_mean_log2;
    ctx->lg_tau_v = h.lg_tau_v;
    if (sbo_status st = sbo_set_option(ctx, SBO_OPT_SPATIAL_ORDER, h.spatial_order)) return st;
    return fc.commit(SBO_OK);
}

}  // extern "C"
