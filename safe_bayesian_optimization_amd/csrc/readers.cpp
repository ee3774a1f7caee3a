// readers.cpp -- sbo_evidence (csrc/evidence.hip), sbo_whatif (csrc/whatif.hip) and sbo_sample (csrc/sample.hip) with
// their debug entry points: the readers of the fitted and the kept state.  Each call is a sequence of stages over a
// plan (readers.hpp): checks and reservation, a device phase with one readback, the host's choice from it, a second
// device phase, the copy-out.
#include "readers.hpp"

#include <algorithm>
#include <cmath>
#include <new>

#include "sbo_host.hpp"

using sbo::EvidencePlan;
using sbo::WhatifPlan;

// ------------------------------------------------------------ model evidence
// Phase 1: the column norms, per-tile sums and LOO outputs.  Then the host chooses the kept k-tile pairs from the
// tiles' norms and boxes; phase 2 is the Gram contraction of grad[0] over (pair, row chunk) items.  Reads the fitted
// state only; evws / evitems are its own workspaces.
void sbo::evidence_totals(const double *sums, int64_t T, int64_t n, double sn, double noise, sbo_evidence_info &r,
                          double *al1, double *sl1) {
    double tot[kEvSums] = {};
    for (int64_t t = 0; t < T; ++t) {
        for (int j = 0; j < kEvSums; ++j) tot[j] += sums[t * kEvSums + j];
        al1[t] = sums[t * kEvSums];
        sl1[t] = sums[t * kEvSums + 1];
    }
    const double sum_c = tot[2], aa = tot[3], ar = tot[4];
    r.n = n;
    r.data_fit = -0.5 * tot[7];
    r.log_det = tot[6];
    r.lml = r.data_fit - r.log_det - 0.5 * (double)n * kEvLog2Pi;
    r.grad[1] = (ar - sn * aa) - ((double)n - sn * sum_c);
    r.grad[2] = 0.5 * noise * (aa - sum_c);
    r.grad[3] = tot[5];
    r.loo_log_pred = tot[8];
}

std::vector<int4> sbo::evidence_items(const uint8_t *drop, int64_t T, int64_t n, sbo_evidence_info &r) {
    std::vector<int4> items;
    r.pairs_total = T * (T + 1) / 2;
    for (int64_t J = 0; J < T; ++J)
        for (int64_t I = 0; I <= J; ++I) r.pairs_kept += drop[I * T + J] ? 0 : 1;
    // the workgroups in flight read one band of X -- kEvChunk x n doubles, which the last-level
    // cache holds -- and share the J block
    constexpr int64_t kBand = kEvChunk / kBK;   // k-tiles per chunk
    for (int64_t g = 0; g * kEvChunk < n; ++g)
        for (int64_t J = 0; J < T && J / kBand <= g; ++J) {
            const int64_t k0 = J * kBK + (g - J / kBand) * kEvChunk;
            if (k0 >= n) continue;
            for (int64_t I = 0; I <= J; ++I)
                if (!drop[I * T + J]) items.push_back(make_int4((int)I, (int)J, (int)k0, k0 == J * kBK ? 1 : 0));
        }
    r.dropped = r.pairs_kept < r.pairs_total ? 1 : 0;
    return items;
}

namespace {

// Stage 1: the checks, evws reserved and carved.
sbo_status evidence_plan(sbo_ctx *ctx, const sbo_evidence_info *out, uint32_t flags, EvidencePlan &p) {
    SBO_CHECK(out->struct_size >= sizeof(uint32_t), SBO_E_INVAL, "sbo_evidence: struct_size not set");
    const int64_t n = p.n = ctx->n;
    SBO_CHECK(ctx->fitted && n > 0, SBO_E_STATE, "sbo_evidence: call sbo_fit first");
    SBO_CHECK(fit_state_complete(ctx, n), SBO_E_STATE,
              "sbo_evidence: needs the fit's factor, f64 inverse and z (not an imported state, SBO_OPT_INVERSE_BITS 64)");
    SBO_HIP(hipSetDevice(ctx->device));
    p.T = (n + sbo::kBK - 1) / sbo::kBK;
    p.want_loo = p.out_mean || p.out_var;
    p.host_loo = p.want_loo && !dev(flags);
    SBO_HIP(ctx->ws.evws.reserve(Carve::need(n, 8) + Carve::need(p.T * sbo::kEvSums, 8) + Carve::need(1, 8) +
                              (p.want_loo ? Carve::need(n, 8) : 0) + (p.host_loo ? 2 * Carve::need(n, 8) : 0)));
    Carve cv(ctx->ws.evws.as<void>());
    p.c = cv.take<double>(n), p.sums = cv.take<double>(p.T * sbo::kEvSums), p.res = cv.take<double>(1);
    if (!p.want_loo) return SBO_OK;
    p.order = cv.take<int64_t>(n);
    double *dm = p.out_mean, *dv = p.out_var;
    if (p.host_loo) dm = cv.take<double>(n), dv = cv.take<double>(n);
    p.loo_mean = p.out_mean ? dm : nullptr;
    p.loo_var = p.out_var ? dv : nullptr;
    return SBO_OK;
}

// Stage 2 (phase 1): c_i, the per-tile sums, the LOO outputs; the sums and the k-tile boxes read back.
sbo_status evidence_phase1(sbo_ctx *ctx, const EvidencePlan &p, PhaseEvents &pe, std::vector<double> &sums,
                           std::vector<float> &boxes) {
    hipStream_t s = ctx->stream;
    const int64_t n = p.n;
    const double *dalpha = ctx->alpha64.as<double>();
    SBO_HIP(pe.record(0));
    SBO_HIP(sbo::launch_evidence_norms(s, ctx->Linv.as<double>(), ctx->cap, n, dalpha, ctx->zvec.as<double>(),
                                       ctx->obs.as<float>(), ctx->L.as<float>(), ctx->cap, ctx->hyper.prior_mean, p.c,
                                       p.sums));
    if (p.want_loo) {
        SBO_HIP(hipMemcpyAsync(p.order, ctx->order.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, s));
        SBO_HIP(sbo::launch_evidence_loo(s, p.c, dalpha, ctx->obs.as<float>(), p.order, n, p.loo_mean, p.loo_var));
        if (p.host_loo && p.out_mean)
            SBO_HIP(hipMemcpyAsync(p.out_mean, p.loo_mean, sizeof(double) * n, hipMemcpyDeviceToHost, s));
        if (p.host_loo && p.out_var)
            SBO_HIP(hipMemcpyAsync(p.out_var, p.loo_var, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    }
    SBO_HIP(pe.record(1));
    SBO_HIP(hipMemcpyAsync(sums.data(), p.sums, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, s));
    SBO_HIP(hipMemcpyAsync(boxes.data(), ctx->kbox.as<void>(), sizeof(float) * boxes.size(), hipMemcpyDeviceToHost, s));
    SBO_HIP(hipStreamSynchronize(s));
    return SBO_OK;
}

// Stage 5 (phase 2): the Gram contraction over the items; grad[0] and the phases' time into r.
sbo_status evidence_gram(sbo_ctx *ctx, const EvidencePlan &p, PhaseEvents &pe, const std::vector<int4> &items,
                         sbo_evidence_info &r) {
    hipStream_t s = ctx->stream;
    const int64_t ni = (int64_t)items.size();
    SBO_HIP(ctx->ws.evitems.reserve(Carve::need(ni, sizeof(int4)) + Carve::need(ni, 8)));
    Carve ci(ctx->ws.evitems.as<void>());
    int4 *ditems = ci.take<int4>(ni);
    double *dslots = ci.take<double>(ni);
    SBO_HIP(hipMemcpyAsync(ditems, items.data(), sizeof(int4) * (size_t)ni, hipMemcpyHostToDevice, s));
    SBO_HIP(pe.record(2));
    SBO_HIP(sbo::launch_evidence_gram(s, ctx->Linv.as<double>(), ctx->cap, p.n, ctx->x.as<float>(), ctx->y.as<float>(),
                                      ctx->alpha64.as<double>(), ditems, ni, ctx->hyper.length_scale,
                                      ctx->hyper.sigma_f * ctx->hyper.sigma_f, dslots, p.res));
    SBO_HIP(pe.record(3));
    SBO_HIP(hipMemcpyAsync(&r.grad[0], p.res, sizeof(double), hipMemcpyDeviceToHost, s));
    SBO_HIP(hipStreamSynchronize(s));   // (the slots carry the 1/2: a diagonal pair halved, an off-diagonal one for both orders)
    SBO_HIP(pe.elapsed());
    r.ms = pe.ms;
    return SBO_OK;
}

sbo_status evidence_run(sbo_ctx *ctx, sbo_evidence_info *out, double *loo_mean, double *loo_var, uint32_t flags) {
    EvidencePlan p;
    p.out_mean = loo_mean, p.out_var = loo_var;
    if (sbo_status st = evidence_plan(ctx, out, flags, p)) return st;
    PhaseEvents pe(ctx);
    SBO_CHECK(pe.ok(), SBO_E_DEVICE, "sbo_evidence: hipEventCreate failed");
    const int64_t T = p.T;
    std::vector<double> sums((size_t)T * sbo::kEvSums), al1(T), sl1(T);
    std::vector<float> boxes((size_t)4 * T);
    if (sbo_status st = evidence_phase1(ctx, p, pe, sums, boxes)) return st;
    sbo_evidence_info r{};
    const double sn = ctx->hyper.noise_level;   // (hyper.noise_level holds the jitter too)
    sbo::evidence_totals(sums.data(), T, p.n, sn, sn - ctx->jitter, r, al1.data(), sl1.data());
    // the cutoff, then the items.  Host cost per call, T = n / 64: the T x T drop map (64 KiB at n = 16384, 1 MiB at
    // 65536), inside evidence_pairs up to T^2 / 2 candidates of 16 B (0.5 / 8 MiB) and their sort, and 16 B per item
    // (about n^2 / 1400 items: 3 MiB at 16384, 47 MiB at 65536)
    r.grad_budget = ctx->opt.evidence_budget > 0 ? std::ldexp((double)p.n, -ctx->opt.evidence_budget) : 0.0;
    std::vector<uint8_t> drop((size_t)T * T);
    sbo::evidence_pairs(boxes.data(), al1.data(), sl1.data(), T, ctx->hyper.length_scale,
                        ctx->hyper.sigma_f * ctx->hyper.sigma_f, r.grad_budget, drop.data(), &r.grad_err_bound);
    if (sbo_status st = evidence_gram(ctx, p, pe, sbo::evidence_items(drop.data(), T, p.n, r), r)) return st;
    copy_info(out, r);
    return SBO_OK;
}

}  // namespace

SBO_API sbo_status sbo_evidence(sbo_ctx *ctx, sbo_evidence_info *out, double *loo_mean, double *loo_var,
                                uint32_t flags) {
    if (!ctx || !out) return SBO_E_INVAL;
    try {
        return evidence_run(ctx, out, loo_mean, loo_var, flags);
    } catch (const std::bad_alloc &) {   // (the host-side tile and item lists)
        ctx->err = "sbo_evidence: host allocation failed";
        return SBO_E_OOM;
    }
}

SBO_API sbo_status sbo_debug_evidence_pairs(const float *boxes, const double *alpha_l1, const double *sqrtc_l1,
                                            int64_t T, sbo_hyper hyper, double budget, uint8_t *drop, double *bound) {
    if (T < 0 || !bound || (T > 0 && (!boxes || !alpha_l1 || !sqrtc_l1 || !drop))) return SBO_E_INVAL;
    if (!(hyper.length_scale > 0.0) || !(hyper.sigma_f > 0.0)) return SBO_E_INVAL;
    try {
        sbo::evidence_pairs(boxes, alpha_l1, sqrtc_l1, T, hyper.length_scale, hyper.sigma_f * hyper.sigma_f, budget,
                            drop, bound);
    } catch (...) {
        return SBO_E_OOM;
    }
    return SBO_OK;
}

// ------------------------------------------------------------ what-if posterior
// The candidate weights W = K^-1 K_c by two triangular products on the f64 inverse, the candidates' sums, one
// readback (var_c and |w_j|_1: the host chooses the cutoff from them), then the sweep over the kept posterior.
// Reads the fitted and the kept state only; wiws is its own workspace.
static_assert(sizeof(sbo_whatif_info) == 80, "sbo_whatif_info: the bindings mirror this layout");

namespace {

// What sbo_whatif and sbo_sample (`who`) read: a kept posterior of the current epoch that has seen every fitted row,
// and the fit's f64 inverse and z.
sbo_status kept_reader_state(sbo_ctx *ctx, const std::string &who) {
    const int64_t n = ctx->n;
    const sbo::StreamKeep &k = ctx->keep;
    SBO_CHECK(ctx->fitted && n > 0, SBO_E_STATE, who + ": call sbo_fit first");
    SBO_CHECK(k.valid, SBO_E_STATE, who + ": no kept posterior (call sbo_tick_stream first)");
    SBO_CHECK(k.epoch == ctx->fit_epoch && k.n_map == n, SBO_E_STATE,
              who + ": the kept posterior has not seen every fitted row (call sbo_tick_stream again)");
    SBO_CHECK(fit_state_complete(ctx, n), SBO_E_STATE,
              who + ": needs the fit's f64 inverse and z (not an imported state, SBO_OPT_INVERSE_BITS 64)");
    return SBO_OK;
}

// U^T = B^T X^T and W^T = U^T X for `rows` right-hand sides stored as rows (rows x n column-major each at leading
// dimension ldb; Wt may be Bt): W = K^-1 B by two triangular products on the f64 inverse X.
sbo_status inverse_products(sbo_ctx *ctx, const double *Bt, double *Ut, double *Wt, int64_t rows, int64_t ldb,
                            int64_t n_) {
    const double *X = ctx->Linv.as<double>();
    const double one = 1.0, zero = 0.0;
    const rocblas_int pp = (rocblas_int)rows, lb = (rocblas_int)ldb, n = (rocblas_int)n_, ld = (rocblas_int)ctx->cap;
    SBO_BLAS(rocblas_set_pointer_mode(ctx->blas, rocblas_pointer_mode_host));
    if (ctx->opt.whatif_gemm) {   // (the inverse's strict upper half is stored as zeros)
        SBO_BLAS(rocblas_dgemm(ctx->blas, rocblas_operation_none, rocblas_operation_transpose, pp, n, n, &one, Bt, lb, X,
                               ld, &zero, Ut, lb));
        SBO_BLAS(rocblas_dgemm(ctx->blas, rocblas_operation_none, rocblas_operation_none, pp, n, n, &one, Ut, lb, X, ld,
                               &zero, Wt, lb));
    } else {
        SBO_BLAS(rocblas_dtrmm(ctx->blas, rocblas_side_right, rocblas_fill_lower, rocblas_operation_transpose,
                               rocblas_diagonal_non_unit, pp, n, &one, X, ld, Bt, lb, Ut, lb));
        SBO_BLAS(rocblas_dtrmm(ctx->blas, rocblas_side_right, rocblas_fill_lower, rocblas_operation_none,
                               rocblas_diagonal_non_unit, pp, n, &one, X, ld, Ut, lb, Wt, lb));
    }
    return SBO_OK;
}

// Stage 1: the checks, wiws reserved and carved, a host caller's candidates staged.
sbo_status whatif_plan(sbo_ctx *ctx, const float *cx, const float *cy, const sbo_whatif_info *info, uint32_t flags,
                       WhatifPlan &w) {
    const int64_t p = w.p, n = w.n = ctx->n;
    SBO_CHECK(cx && cy && w.out_gain, SBO_E_INVAL, "sbo_whatif: null candidates or gain");
    SBO_CHECK(p > 0 && p <= 1024, SBO_E_INVAL, "sbo_whatif: p must be in [1, 1024]");
    SBO_CHECK(std::isfinite(w.beta) && !std::isnan(w.f_min), SBO_E_INVAL, "sbo_whatif: beta/f_min must be finite");
    SBO_CHECK(!info || info->struct_size >= sizeof(uint32_t), SBO_E_INVAL, "sbo_whatif: struct_size not set");
    if (sbo_status st = kept_reader_state(ctx, "sbo_whatif")) return st;
    const sbo::StreamKeep &k = ctx->keep;
    SBO_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t pp = w.pp = sbo::round_up(p, 16);
    w.m = k.m;
    w.host = !dev(flags);
    w.mat = (size_t)p * (size_t)w.m;
    SBO_HIP(ctx->ws.wiws.reserve(2 * Carve::need((size_t)pp * (size_t)n, 8) + Carve::need(sbo::whatif_part_bytes(pp), 1) +
                              3 * Carve::need(p, 8) + Carve::need(2 * pp, 8) + Carve::need(p + 1, 8) +
                              (w.host ? 2 * Carve::need(p, 4) + (w.out_cov ? Carve::need(w.mat, 8) : 0) +
                                            (w.out_lo ? Carve::need(w.mat, 8) : 0)
                                      : 0)));
    Carve cv(ctx->ws.wiws.as<void>());
    w.Wt = w.Kt = cv.take<double>((size_t)pp * (size_t)n), w.Ut = cv.take<double>((size_t)pp * (size_t)n);
    w.part = cv.take<double>(sbo::whatif_part_bytes(pp) / 8);
    w.mu = cv.take<double>(p), w.var = cv.take<double>(p), w.l1 = cv.take<double>(p);
    w.par = cv.take<double>(2 * pp);
    w.gain = cv.take<unsigned long long>(p + 1), w.kept = w.gain + p;
    w.cx = cx, w.cy = cy, w.cov = w.out_cov, w.lo = w.out_lo;
    if (!w.host) return SBO_OK;
    float *sx = cv.take<float>(p), *sy = cv.take<float>(p);
    SBO_HIP(hipMemcpyAsync(sx, cx, sizeof(float) * p, hipMemcpyHostToDevice, s));
    SBO_HIP(hipMemcpyAsync(sy, cy, sizeof(float) * p, hipMemcpyHostToDevice, s));
    w.cx = sx, w.cy = sy;
    if (w.out_cov) w.cov = cv.take<double>(w.mat);
    if (w.out_lo) w.lo = cv.take<double>(w.mat);
    return SBO_OK;
}

// Stage 2 (phase 1): K_c^T, U^T = K_c^T X^T, W^T = U^T X (over K_c^T), the candidates' sums; var_c and |w_j|_1 read back.
sbo_status whatif_weights(sbo_ctx *ctx, const WhatifPlan &w, PhaseEvents &pe, std::vector<double> &hvar,
                          std::vector<double> &hl1) {
    hipStream_t s = ctx->stream;
    const double sf2 = ctx->hyper.sigma_f * ctx->hyper.sigma_f, noise = ctx->hyper.noise_level;   // (holds the jitter too)
    SBO_HIP(pe.record(0));
    {
        Bracket br(ctx, ctx->ev_fill);
        SBO_HIP(sbo::launch_whatif_fill(s, ctx->x.as<float>(), ctx->y.as<float>(), w.n, w.cx, w.cy, w.p, w.pp,
                                        ctx->hyper.length_scale, sf2, w.Kt));
        if (sbo_status st = inverse_products(ctx, w.Kt, w.Ut, w.Wt, w.pp, w.pp, w.n)) return st;
        SBO_HIP(sbo::launch_whatif_stats(s, w.Ut, w.Wt, w.p, w.pp, w.n, ctx->zvec.as<double>(), ctx->hyper.prior_mean,
                                         sf2, noise, w.beta, w.part, w.mu, w.var, w.l1, w.par));
    }
    SBO_HIP(pe.record(1));
    SBO_HIP(hipMemcpyAsync(hvar.data(), w.var, sizeof(double) * w.p, hipMemcpyDeviceToHost, s));
    SBO_HIP(hipMemcpyAsync(hl1.data(), w.l1, sizeof(double) * w.p, hipMemcpyDeviceToHost, s));
    SBO_HIP(hipStreamSynchronize(s));
    return SBO_OK;
}

// Stage 3: the cutoff -- the context's fixed one, or the smallest L within the sweep's budgets -- and its bound on
// |cov error|.
int whatif_choose_cutoff(const sbo_ctx *ctx, const WhatifPlan &w, const std::vector<double> &hvar,
                         const std::vector<double> &hl1, double &err_cov) {
    const double sf2 = ctx->hyper.sigma_f * ctx->hyper.sigma_f;
    int L = ctx->opt.skip_log2;
    if (L < 0) {
        double bvar = 0.0, bmean = 0.0;
        stream_budget(ctx, bvar, bmean);
        sbo::whatif_cutoff(w.p, hl1.data(), hvar.data(), ctx->hyper.noise_level, w.beta, sf2, bvar, bmean, &L, &err_cov);
    } else {
        err_cov = sbo::whatif_err_cov(L, sf2, *std::max_element(hl1.begin(), hl1.end()));
    }
    return L;
}

// Stage 4 (phase 2): the sweep over the kept posterior at cutoff L.
sbo_status whatif_sweep(sbo_ctx *ctx, const WhatifPlan &w, PhaseEvents &pe, int L) {
    hipStream_t s = ctx->stream;
    const sbo::StreamKeep &k = ctx->keep;
    SBO_HIP(hipMemsetAsync(w.gain, 0, sizeof(unsigned long long) * (size_t)(w.p + 1), s));
    SBO_HIP(pe.record(2));
    {
        Bracket br(ctx, ctx->ev_predict);
        SBO_HIP(sbo::launch_whatif(s, w.Wt, w.pp, w.p, w.n, ctx->x.as<float>(), ctx->y.as<float>(),
                                   ctx->kbox.as<float4>(), k.qbox.as<float4>(), k.qx.as<float>(), k.qy.as<float>(),
                                   k.perm.as<int32_t>(), k.ms, w.m, ctx->hyper.length_scale,
                                   ctx->hyper.sigma_f * ctx->hyper.sigma_f, L, k.mu64.as<double>(),
                                   k.var64.as<double>(), w.cx, w.cy, w.par, w.beta, w.f_min, w.gain, w.cov, w.lo,
                                   w.kept));
    }
    SBO_HIP(pe.record(3));
    return SBO_OK;
}

// Stage 5: the outputs to the caller; with `info` wanted the best candidate's gain, the sizes, the tile counts and
// the phases' time into r.
sbo_status whatif_read_out(sbo_ctx *ctx, const WhatifPlan &w, PhaseEvents &pe, bool info, sbo_whatif_info &r) {
    hipStream_t s = ctx->stream;
    const int64_t p = w.p;
    std::vector<unsigned long long> hgain((size_t)p + 1);
    SBO_HIP(hipMemcpyAsync(hgain.data(), w.gain, sizeof(unsigned long long) * (size_t)(p + 1), hipMemcpyDeviceToHost, s));
    const hipMemcpyKind out = w.host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (!w.host) SBO_HIP(hipMemcpyAsync(w.out_gain, w.gain, sizeof(int64_t) * p, out, s));
    if (w.out_mu) SBO_HIP(hipMemcpyAsync(w.out_mu, w.mu, sizeof(double) * p, out, s));
    if (w.out_var) SBO_HIP(hipMemcpyAsync(w.out_var, w.var, sizeof(double) * p, out, s));
    if (w.host && w.out_cov) SBO_HIP(hipMemcpyAsync(w.out_cov, w.cov, sizeof(double) * w.mat, out, s));
    if (w.host && w.out_lo) SBO_HIP(hipMemcpyAsync(w.out_lo, w.lo, sizeof(double) * w.mat, out, s));
    SBO_HIP(hipStreamSynchronize(s));
    r.best = 0;
    for (int64_t j = 0; j < p; ++j) {
        if (w.host) w.out_gain[j] = (int64_t)hgain[(size_t)j];
        if (hgain[(size_t)j] > hgain[(size_t)r.best]) r.best = j;   // (the lowest j on ties)
    }
    if (!info) return SBO_OK;
    r.best_gain = (int64_t)hgain[(size_t)r.best];
    r.p = p, r.m = w.m, r.n = w.n;
    r.tiles_total = kept_tiles_total(ctx->keep.ms, w.n);
    r.tiles_kept = (int64_t)hgain[(size_t)p];
    SBO_HIP(pe.elapsed());
    r.ms = pe.ms;
    return SBO_OK;
}

sbo_status whatif_run(sbo_ctx *ctx, const float *cx, const float *cy, WhatifPlan &w, sbo_whatif_info *info,
                      uint32_t flags) {
    if (sbo_status st = whatif_plan(ctx, cx, cy, info, flags, w)) return st;
    PhaseEvents pe(ctx);
    SBO_CHECK(pe.ok(), SBO_E_DEVICE, "sbo_whatif: hipEventCreate failed");
    std::vector<double> hvar((size_t)w.p), hl1((size_t)w.p);
    if (sbo_status st = whatif_weights(ctx, w, pe, hvar, hl1)) return st;
    sbo_whatif_info r{};
    r.cutoff_log2 = whatif_choose_cutoff(ctx, w, hvar, hl1, r.err_cov);
    if (sbo_status st = whatif_sweep(ctx, w, pe, r.cutoff_log2)) return st;
    if (sbo_status st = whatif_read_out(ctx, w, pe, info != nullptr, r)) return st;
    if (info) copy_info(info, r);
    return SBO_OK;
}

}  // namespace

SBO_API sbo_status sbo_whatif(sbo_ctx *ctx, const float *cx, const float *cy, int64_t p, double beta, double f_min,
                              int64_t *gain, double *cand_mu, double *cand_var, double *cov, double *lo_new,
                              sbo_whatif_info *info, uint32_t flags) {
    if (!ctx) return SBO_E_INVAL;
    try {
        WhatifPlan w;
        w.p = p, w.beta = beta, w.f_min = f_min;
        w.out_gain = gain, w.out_mu = cand_mu, w.out_var = cand_var, w.out_cov = cov, w.out_lo = lo_new;
        return whatif_run(ctx, cx, cy, w, info, flags);
    } catch (const std::bad_alloc &) {   // (the host copies of the candidates' sums and counts)
        ctx->err = "sbo_whatif: host allocation failed";
        return SBO_E_OOM;
    }
}

SBO_API sbo_status sbo_debug_whatif_cutoff(int64_t p, const double *w_l1, const double *cand_var, double s,
                                           double beta, double sf2, double budget_var, double budget_mean,
                                           int32_t *cutoff_log2, double *err_cov) {
    if (p <= 0 || !w_l1 || !cand_var || !cutoff_log2 || !err_cov || !(sf2 > 0.0)) return SBO_E_INVAL;
    int L = 0;
    sbo::whatif_cutoff(p, w_l1, cand_var, s, beta, sf2, budget_var, budget_mean, &L, err_cov);
    *cutoff_log2 = L;
    return SBO_OK;
}

// ------------------------------------------------------------ posterior sample paths
// The draws (frequencies, feature weights, sqrt(s) eps), T^T += the prior paths at the training points, the weights
// W = K^-1 T by the what-if's two triangular products, |w_j|_1 and the feature kernel's error, one readback (the host
// chooses the cutoff from |w_j|_1), then the sweep over the kept posterior and the key reduction.  Reads the fitted
// and the kept state only; smws is its own workspace.
//
// rocBLAS chooses a product's blocking, and with it the order of a row's sums, from the number of rows (measured at
// n = 700: 17 + 133 rows in two calls against 150 in one differ in the last place).  A path must not depend on how a
// range of samples is cut into calls, so T^T, U^T and W^T have kSampleChunk-row chunks (leading dimension pw, the
// rows past the samples zero) and every product runs on one chunk: rocBLAS sees one shape, whatever `samples` is.
constexpr int64_t kSampleChunk = 128;
static_assert(sizeof(sbo_sample_info) == 96, "sbo_sample_info: the bindings mirror this layout");

using sbo::SamplePlan;

namespace {

// The sizes every entry point of the sampler takes.
sbo_status sample_sizes(sbo_ctx *ctx, int64_t first, int64_t samples, int64_t features, const std::string &who) {
    SBO_CHECK(samples >= 1 && samples <= 1024, SBO_E_INVAL, who + ": samples must be in [1, 1024]");
    SBO_CHECK(first >= 0 && first + samples <= ((int64_t)1 << 20), SBO_E_INVAL,
              who + ": first must be >= 0 and first + samples <= 2^20");
    SBO_CHECK(features >= 1 && features <= 4096, SBO_E_INVAL, who + ": features must be in [1, 4096]");
    return SBO_OK;
}

// Stage 1: the checks, smws reserved and carved.
sbo_status sample_plan(sbo_ctx *ctx, const sbo_sample_info *info, uint32_t flags, SamplePlan &p) {
    SBO_CHECK(p.out_keys, SBO_E_INVAL, "sbo_sample: null keys");
    if (sbo_status st = sample_sizes(ctx, p.first, p.S, p.F, "sbo_sample")) return st;
    SBO_CHECK(std::isfinite(p.beta) && !std::isnan(p.f_min), SBO_E_INVAL, "sbo_sample: beta/f_min must be finite");
    SBO_CHECK(!info || info->struct_size >= sizeof(uint32_t), SBO_E_INVAL, "sbo_sample: struct_size not set");
    if (sbo_status st = kept_reader_state(ctx, "sbo_sample")) return st;
    const int64_t n = p.n = ctx->n, S = p.S;
    SBO_CHECK(n <= ((int64_t)1 << 24), SBO_E_INVAL, "sbo_sample: more than 2^24 training points");
    SBO_HIP(hipSetDevice(ctx->device));
    const sbo::StreamKeep &k = ctx->keep;
    const int64_t pp = p.pp = sbo::round_up(S, 16), Fp = p.Fp = sbo::round_up(p.F, 4);
    const int64_t pw = p.pw = sbo::round_up(S, kSampleChunk);
    p.m = k.m;
    p.nb = sbo::sample_blocks(k.ms);
    p.host = !dev(flags);
    p.mat = (size_t)S * (size_t)p.m;
    p.cx0 = 0.5 * ((double)ctx->bbox[0] + (double)ctx->bbox[1]);
    p.cy0 = 0.5 * ((double)ctx->bbox[2] + (double)ctx->bbox[3]);
    const size_t pn = (size_t)pw * (size_t)n, pf = (size_t)pp * (size_t)(2 * Fp), pk = (size_t)S * (size_t)p.nb;
    SBO_HIP(ctx->ws.smws.reserve(2 * Carve::need(pn, 8) + Carve::need(pf, 8) + 2 * Carve::need(Fp, 8) + Carve::need(n, 8) +
                              Carve::need(sbo::whatif_part_bytes(pw), 1) + Carve::need(S, 8) +
                              Carve::need(2 * S + 2 * pw, 8) + Carve::need(S + 2, 8) + Carve::need(pk, sizeof(sbo_key)) +
                              Carve::need(S, sizeof(sbo_key)) + (p.host && p.out_paths ? Carve::need(p.mat, 8) : 0)));
    Carve cv(ctx->ws.smws.as<void>());
    p.Wt = p.Tt = cv.take<double>(pn), p.Ut = cv.take<double>(pn), p.Theta = cv.take<double>(pf);
    p.wx = cv.take<double>(Fp), p.wy = cv.take<double>(Fp);
    p.order = cv.take<int64_t>(n);
    p.part = cv.take<double>(sbo::whatif_part_bytes(pw) / 8);
    p.l1 = cv.take<double>(S), p.junk = cv.take<double>(2 * S + 2 * pw);
    p.count = cv.take<unsigned long long>(S + 2), p.kept = p.count + S, p.kerr = p.kept + 1;
    p.pkeys = cv.take<sbo_key>(pk), p.keys = cv.take<sbo_key>(S);
    p.paths = p.out_paths;
    if (p.host && p.out_paths) p.paths = cv.take<double>(p.mat);
    return SBO_OK;
}

// Stage 2 (phase 1): the draws, T^T += g(train), U^T = T^T X^T, W^T = U^T X (over T^T), |w_j|_1 by the what-if's
// chunked sums, the feature kernel's error; |w_j|_1 and the error read back.
sbo_status sample_weights(sbo_ctx *ctx, const SamplePlan &p, PhaseEvents &pe, std::vector<double> &hl1,
                          double &kernel_err) {
    hipStream_t s = ctx->stream;
    const sbo_hyper &h = ctx->hyper;   // (noise_level holds the jitter too)
    SBO_HIP(hipMemcpyAsync(p.order, ctx->order.data(), sizeof(int64_t) * p.n, hipMemcpyHostToDevice, s));
    SBO_HIP(hipMemsetAsync(p.kerr, 0, sizeof(unsigned long long), s));
    SBO_HIP(pe.record(0));
    {
        Bracket br(ctx, ctx->ev_fill);
        SBO_HIP(sbo::launch_sample_draw(s, p.seed, p.first, p.S, p.pp, p.pw, p.F, p.Fp, p.n, p.order, h.length_scale,
                                        h.sigma_f, h.noise_level, p.wx, p.wy, p.Theta, p.Tt, nullptr, nullptr, nullptr));
        SBO_HIP(sbo::launch_sample_train(s, p.Theta, p.pp, p.n, ctx->x.as<float>(), ctx->y.as<float>(), p.wx, p.wy,
                                         p.Fp, p.cx0, p.cy0, p.Tt, p.pw));
        for (int64_t r0 = 0; r0 < p.pw; r0 += kSampleChunk)
            if (sbo_status st = inverse_products(ctx, p.Tt + r0, p.Ut + r0, p.Wt + r0, kSampleChunk, p.pw, p.n))
                return st;
        // (the candidates' u . z and |u|^2 of the what-if mean nothing here: junk)
        double *jmu = p.junk, *jvar = jmu + p.S, *jpar = jvar + p.S;
        SBO_HIP(sbo::launch_whatif_stats(s, p.Ut, p.Wt, p.S, p.pw, p.n, ctx->zvec.as<double>(), h.prior_mean,
                                         h.sigma_f * h.sigma_f, h.noise_level, p.beta, p.part, jmu, jvar, p.l1, jpar));
        SBO_HIP(sbo::launch_sample_kernel_err(s, p.wx, p.wy, p.F, h.length_scale, p.kerr));
    }
    SBO_HIP(pe.record(1));
    unsigned long long bits = 0;
    SBO_HIP(hipMemcpyAsync(hl1.data(), p.l1, sizeof(double) * p.S, hipMemcpyDeviceToHost, s));
    SBO_HIP(hipMemcpyAsync(&bits, p.kerr, sizeof(bits), hipMemcpyDeviceToHost, s));
    SBO_HIP(hipStreamSynchronize(s));
    memcpy(&kernel_err, &bits, sizeof(double));
    return SBO_OK;
}

// Stage 3: the cutoff -- the context's fixed one, or the smallest L within the sweep's mean budget -- and its bound
// on |path error|.
int sample_choose_cutoff(const sbo_ctx *ctx, const std::vector<double> &hl1, double &err_path) {
    const double sf2 = ctx->hyper.sigma_f * ctx->hyper.sigma_f;
    int L = ctx->opt.skip_log2;
    if (L < 0) {
        double bvar = 0.0, bmean = 0.0;
        stream_budget(ctx, bvar, bmean);
        sbo::sample_cutoff((int64_t)hl1.size(), hl1.data(), sf2, bmean, &L, &err_path);
    } else {
        err_path = sbo::whatif_err_cov(L, sf2, *std::max_element(hl1.begin(), hl1.end()));
    }
    return L;
}

// Stage 4 (phase 2): the sweep over the kept posterior at cutoff L, then the samples' keys.
sbo_status sample_sweep(sbo_ctx *ctx, const SamplePlan &p, PhaseEvents &pe, int L) {
    hipStream_t s = ctx->stream;
    const sbo::StreamKeep &k = ctx->keep;
    SBO_HIP(hipMemsetAsync(p.count, 0, sizeof(unsigned long long) * (size_t)(p.S + 1), s));
    SBO_HIP(pe.record(2));
    {
        Bracket br(ctx, ctx->ev_predict);
        SBO_HIP(sbo::launch_sample(s, p.Wt, p.pw, p.Theta, p.pp, p.S, p.n, ctx->x.as<float>(), ctx->y.as<float>(),
                                   ctx->kbox.as<float4>(), k.qbox.as<float4>(), k.qx.as<float>(), k.qy.as<float>(),
                                   k.perm.as<int32_t>(), k.ms, p.m, ctx->hyper.length_scale,
                                   ctx->hyper.sigma_f * ctx->hyper.sigma_f, L, k.mu64.as<double>(),
                                   k.var64.as<double>(), p.wx, p.wy, p.Fp, p.cx0, p.cy0, p.beta, p.f_min,
                                   p.index_offset, p.count, p.paths, p.pkeys, p.keys, p.kept));
    }
    SBO_HIP(pe.record(3));
    return SBO_OK;
}

// Stage 5: the outputs to the caller; with `info` wanted the sizes, the tile counts and the phases' time into r.
sbo_status sample_read_out(sbo_ctx *ctx, const SamplePlan &p, PhaseEvents &pe, bool info, sbo_sample_info &r) {
    hipStream_t s = ctx->stream;
    const hipMemcpyKind out = p.host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    unsigned long long kept = 0;
    SBO_HIP(hipMemcpyAsync(&kept, p.kept, sizeof(kept), hipMemcpyDeviceToHost, s));
    SBO_HIP(hipMemcpyAsync(p.out_keys, p.keys, sizeof(sbo_key) * (size_t)p.S, out, s));
    if (p.out_count) SBO_HIP(hipMemcpyAsync(p.out_count, p.count, sizeof(int64_t) * (size_t)p.S, out, s));
    if (p.host && p.out_paths) SBO_HIP(hipMemcpyAsync(p.out_paths, p.paths, sizeof(double) * p.mat, out, s));
    SBO_HIP(hipStreamSynchronize(s));
    if (!info) return SBO_OK;
    r.samples = p.S, r.first = p.first, r.m = p.m, r.n = p.n, r.features = p.F;
    r.tiles_total = kept_tiles_total(ctx->keep.ms, p.n);
    r.tiles_kept = (int64_t)kept;
    SBO_HIP(pe.elapsed());
    r.ms = pe.ms;
    return SBO_OK;
}

sbo_status sample_run(sbo_ctx *ctx, SamplePlan &p, sbo_sample_info *info, uint32_t flags) {
    if (sbo_status st = sample_plan(ctx, info, flags, p)) return st;
    PhaseEvents pe(ctx);
    SBO_CHECK(pe.ok(), SBO_E_DEVICE, "sbo_sample: hipEventCreate failed");
    std::vector<double> hl1((size_t)p.S);
    sbo_sample_info r{};
    if (sbo_status st = sample_weights(ctx, p, pe, hl1, r.kernel_err)) return st;
    r.w_l1_max = *std::max_element(hl1.begin(), hl1.end());
    r.cutoff_log2 = sample_choose_cutoff(ctx, hl1, r.err_path);
    if (sbo_status st = sample_sweep(ctx, p, pe, r.cutoff_log2)) return st;
    if (sbo_status st = sample_read_out(ctx, p, pe, info != nullptr, r)) return st;
    if (info) copy_info(info, r);
    return SBO_OK;
}

}  // namespace

SBO_API sbo_status sbo_sample(sbo_ctx *ctx, uint64_t seed, int64_t first, int64_t samples, int64_t features,
                              double beta, double f_min, int64_t index_offset, sbo_key *keys, int64_t *count_above,
                              double *paths, sbo_sample_info *info, uint32_t flags) {
    if (!ctx) return SBO_E_INVAL;
    try {
        SamplePlan p;
        p.seed = seed, p.first = first, p.S = samples, p.F = features, p.beta = beta, p.f_min = f_min;
        p.index_offset = index_offset;
        p.out_keys = keys, p.out_count = count_above, p.out_paths = paths;
        return sample_run(ctx, p, info, flags);
    } catch (const std::bad_alloc &) {   // (the host copy of the samples' sums)
        ctx->err = "sbo_sample: host allocation failed";
        return SBO_E_OOM;
    }
}

SBO_API sbo_status sbo_debug_sample_cutoff(int64_t samples, const double *w_l1, double sf2, double budget_mean,
                                           int32_t *cutoff_log2, double *err_path) {
    if (samples <= 0 || !w_l1 || !cutoff_log2 || !err_path || !(sf2 > 0.0)) return SBO_E_INVAL;
    int L = 0;
    sbo::sample_cutoff(samples, w_l1, sf2, budget_mean, &L, err_path);
    *cutoff_log2 = L;
    return SBO_OK;
}

SBO_API sbo_status sbo_debug_sample_draws(sbo_ctx *ctx, uint64_t seed, int64_t first, int64_t samples,
                                          int64_t features, double *nu, double *ab, double *eps) {
    if (!ctx) return SBO_E_INVAL;
    SBO_CHECK(nu && ab && eps, SBO_E_INVAL, "sbo_debug_sample_draws: null output");
    if (sbo_status st = sample_sizes(ctx, first, samples, features, "sbo_debug_sample_draws")) return st;
    const int64_t n = ctx->n, S = samples, F = features;
    SBO_CHECK(ctx->fitted && n > 0, SBO_E_STATE, "sbo_debug_sample_draws: call sbo_fit first");
    SBO_CHECK(n <= ((int64_t)1 << 24), SBO_E_INVAL, "sbo_debug_sample_draws: more than 2^24 training points");
    SBO_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t pp = sbo::round_up(S, 16), Fp = sbo::round_up(F, 4);
    SBO_HIP(ctx->ws.smws.reserve(2 * Carve::need(Fp, 8) + Carve::need(n, 8) + Carve::need(2 * F, 8) +
                              Carve::need(S * 2 * F, 8) + Carve::need(S * n, 8)));
    Carve cv(ctx->ws.smws.as<void>());
    double *wx = cv.take<double>(Fp), *wy = cv.take<double>(Fp);
    int64_t *order = cv.take<int64_t>(n);
    double *dnu = cv.take<double>(2 * F), *dab = cv.take<double>(S * 2 * F), *deps = cv.take<double>(S * n);
    SBO_HIP(hipMemcpyAsync(order, ctx->order.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, s));
    SBO_HIP(sbo::launch_sample_draw(s, seed, first, S, pp, pp, F, Fp, n, order, ctx->hyper.length_scale, ctx->hyper.sigma_f,
                                    ctx->hyper.noise_level, wx, wy, nullptr, nullptr, dnu, dab, deps));
    SBO_HIP(hipMemcpyAsync(nu, dnu, sizeof(double) * 2 * F, hipMemcpyDeviceToHost, s));
    SBO_HIP(hipMemcpyAsync(ab, dab, sizeof(double) * S * 2 * F, hipMemcpyDeviceToHost, s));
    SBO_HIP(hipMemcpyAsync(eps, deps, sizeof(double) * S * n, hipMemcpyDeviceToHost, s));
    SBO_HIP(hipStreamSynchronize(s));
    return SBO_OK;
}
