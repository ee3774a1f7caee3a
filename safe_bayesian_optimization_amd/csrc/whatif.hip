// whatif.hip -- the what-if posterior (sbo_whatif): the posterior
// cross-covariance of the kept grid with p candidate points, and each
// candidate's expander count -- the currently unsafe grid points whose lower
// bound would clear f_min after an optimistic observation at the candidate
// (SafeOpt's GP-defined expanders, Berkenkamp et al. 2016; no Lipschitz
// constant).  Nothing is appended: the fitted and the kept state are read only.
//
// Fitted state: K = K_f + s I with s = noise_level + jitter, X = L^-1 in f64,
// z = X (y - m0), the training points in the factor's order; f32 coordinates
// are widened to f64 wherever a kernel value is formed.  For the candidates
// c_j (f32 coordinates cx, cy), j < p:
//     k_j   = k(train, c_j)                      (n)
//     u_j   = X k_j            w_j = X^T u_j      (= K^-1 k_j)
//     mu_c  = m0 + u_j . z     var_c = sf2 - |u_j|^2      d_j = var_c + s
//     cov(q, c_j) = k(q, c_j) - k*(q) . w_j      for every kept query q
// The optimistic observation is y_j = mu_c + beta sd_c, sd_c = sqrt(max(var_c, 0)).
// Conditioning the kept posterior (mu, var) on it gives, all in f64,
//     mu'(q)  = mu(q)  + cov(q, c_j) beta sd_c / d_j
//     var'(q) = var(q) - cov(q, c_j)^2 / d_j
//     lo'(q)  = mu'(q) - beta sqrt(max(var'(q), 0))
//     gain_j  = #{ q : not safe(q) and lo'(q) > f_min }
// where safe(q) is recomputed from the kept state by acquire_kept_kernel's
// arithmetic (mean and sd narrowed to f32, the sets in IEEE f64 without FMA):
// it equals the `safe` output of the sbo_tick_stream call that left the state.
//
// Candidate weights: whatif_fill_kernel writes K_c^T (pp x n, pp = p rounded
// up to 16, the padding rows zero); the host runs the two triangular products
// U^T = K_c^T X^T and W^T = U^T X on rocBLAS; whatif_stats_kernel and
// whatif_cand_kernel reduce u_j . z, |u_j|^2 and |w_j|_1 in a fixed order
// (column chunks, then the chunks ascending; no floating-point atomics).
//
// The sweep (whatif_kernel) is the k-tile walk of kstar_walk.hpp, shared with
// predict_update_kernel, with another left operand and another epilogue: W^T
// is stored pp x n column-major, so the sixteen candidates of a column are one
// 128-byte segment and a lane's A operand is one 8-byte load of it.  NJ
// candidate blocks share the K* of a step; more candidates than 16 NJ go in
// further passes over the tiles.  L >= 150 is bitwise the dense call.
// The epilogue forms, per (candidate, position), the direct term k(q, c_j),
// cov, mu', var', lo' and the newly-safe predicate; a candidate's count over a
// wave's sixteen positions comes from one ballot and is added with an integer
// atomic (order-independent); cov and lo' go out through perm in the caller's
// order.  Padding positions (perm < 0) contribute nothing.  Each cov entry is
// one wave's sum over the tiles in ascending order: nothing depends on the
// launch grid, and two calls agree bitwise.
//
// Cutoff: dropping K* entries below 2^-L moves cov(q, c_j) by at most
// e_j = sf2 2^-L |w_j|_1, hence (|cov| <= sqrt(sf2 max(var_c, 0)))
//     mean:     beta sd_c e_j / d_j
//     variance: (2 sqrt(sf2 max(var_c, 0)) e_j + e_j^2) / d_j.
// whatif_cutoff (host) picks the smallest L in [16, 149] that keeps both within
// the budgets for every candidate, else 150.
#include <cmath>
#include <cstdint>

#include "kstar_walk.hpp"
#include "sbo_internal.hpp"

namespace sbo {
namespace {

constexpr int kWChunks = 32;        // column chunks of the candidate sums
constexpr int kWSums = 3;           // u . z, |u|^2, |w|_1

// Kt[j + k pp] = k(train_k, c_j) for j < p, 0 for the padding rows p <= j < pp.
__global__ __launch_bounds__(256) void whatif_fill_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                          int64_t n, const float *__restrict__ cx,
                                                          const float *__restrict__ cy, int64_t p, int64_t pp,
                                                          double cexp, double sf2, double *__restrict__ Kt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * pp) return;
    const int64_t j = i % pp, k = i / pp;
    Kt[i] = j < p ? rbf64((double)x[k], (double)y[k], (double)cx[j], (double)cy[j], cexp, sf2) : 0.0;
}

// Workgroup (candidate block b, column chunk c): thread (candidate r = tid & 15,
// k lane tid >> 4) strides its chunk's columns by 16 (sixteen candidates of a
// column are one 128-byte segment); part[(j kWChunks + c) kWSums + ..] = the
// chunk's u_j . z, |u_j|^2 and |w_j|_1, the sixteen k lanes added in ascending order.
__global__ __launch_bounds__(256) void whatif_stats_kernel(const double *__restrict__ Ut, const double *__restrict__ Wt,
                                                           int64_t pp, int64_t n, const double *__restrict__ z,
                                                           double *__restrict__ part) {
    __shared__ double red[kWSums][256];
    const int tid = threadIdx.x, r = tid & 15;
    const int64_t j = (int64_t)blockIdx.x * 16 + r;
    const int64_t span = round_up((n + kWChunks - 1) / kWChunks, 16);
    const int64_t k0 = (int64_t)blockIdx.y * span, k1 = k0 + span < n ? k0 + span : n;
    double uz = 0.0, uu = 0.0, w1 = 0.0;
    for (int64_t k = k0 + (tid >> 4); k < k1; k += 16) {
        const double u = Ut[j + k * pp];
        uz = fma(u, z[k], uz);
        uu = fma(u, u, uu);
        w1 += fabs(Wt[j + k * pp]);
    }
    red[0][tid] = uz;
    red[1][tid] = uu;
    red[2][tid] = w1;
    __syncthreads();
    if (tid < 16) {
        double *out = part + (j * kWChunks + blockIdx.y) * kWSums;
        for (int q = 0; q < kWSums; ++q) {
            double t = 0.0;
            for (int l = 0; l < 16; ++l) t += red[q][l * 16 + tid];
            out[q] = t;
        }
    }
}

// One thread per candidate: the chunks' sums in ascending order, then mu_c,
// var_c, |w_j|_1 and what the sweep's epilogue multiplies by:
// cpar[2 j] = beta sd_c / d_j, cpar[2 j + 1] = 1 / d_j.
__global__ __launch_bounds__(256) void whatif_cand_kernel(const double *__restrict__ part, int64_t p, double m0,
                                                          double sf2, double s, double beta,
                                                          double *__restrict__ cand_mu, double *__restrict__ cand_var,
                                                          double *__restrict__ w_l1, double *__restrict__ cpar) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= p) return;
    double uz = 0.0, uu = 0.0, w1 = 0.0;
    for (int c = 0; c < kWChunks; ++c) {
        const double *in = part + (j * kWChunks + c) * kWSums;
        uz += in[0];
        uu += in[1];
        w1 += in[2];
    }
    const double var = sf2 - uu, d = var + s;
    cand_mu[j] = m0 + uz;
    cand_var[j] = var;
    w_l1[j] = w1;
    cpar[2 * j] = beta * sqrt(fmax(var, 0.0)) / d;
    cpar[2 * j + 1] = 1.0 / d;
}

// Rows are candidates, columns the wave's positions.
template <int NJ>
__global__ __launch_bounds__(kWalkThreads) void whatif_kernel(
    const double *__restrict__ Wt, int64_t pp, int64_t p, int64_t n, const float *__restrict__ x,
    const float *__restrict__ y, const float4 *__restrict__ kbox, const float4 *__restrict__ qbox,
    const float *__restrict__ qx, const float *__restrict__ qy, const int32_t *__restrict__ perm, int64_t ms, int64_t m,
    double cexp, double sf2, float skip_L, const double *__restrict__ mu64, const double *__restrict__ var64,
    const float *__restrict__ cx, const float *__restrict__ cy, const double *__restrict__ cpar, double beta,
    double f_min, unsigned long long *__restrict__ gain, double *__restrict__ cov, double *__restrict__ lo_new,
    unsigned long long *__restrict__ tiles_kept) {
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int64_t pos = (int64_t)blockIdx.x * kBN + wave * 16 + r;
    const bool live = pos < ms;
    const double xq = live ? (double)qx[pos] : 0.0, yq = live ? (double)qy[pos] : 0.0;
    const int64_t o = live ? (int64_t)perm[pos] : -1;   // the caller's index (-1: padding)
    const bool real = o >= 0;
    // the kept posterior of this position and its safe flag, as acquire_kept_kernel forms it
    double muq = 0.0, varq = 0.0;
    bool safe = false;
    if (real) {
        muq = mu64[pos];
        varq = var64[pos];
        const float sdf = __fsqrt_rn(varq > 0.0 ? (float)varq : 0.0f);
        safe = __dsub_rn((double)(float)muq, __dmul_rn(beta, (double)sdf)) > f_min;
    }
    const float4 qb = qbox[blockIdx.x];
    const WalkRows A{Wt, pp, pp};
    const int nrb = (int)(pp / 16);
    int kept = 0;
    for (int rb0 = 0; rb0 < nrb; rb0 += NJ) {
        f64x4 acc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
        kstar_walk<NJ>(A, rb0, r, g, xq, yq, x, y, kbox, qb, n, cexp, sf2, skip_L, acc, kept);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t cand = (int64_t)(rb0 + j) * 16 + g + 4 * c;
                const bool on = cand < p && real;
                bool newly = false;
                if (on) {
                    const double cv = rbf64((double)cx[cand], (double)cy[cand], xq, yq, cexp, sf2) - acc[j][c];
                    const double mu1 = muq + cv * cpar[2 * cand];
                    const double var1 = varq - cv * cv * cpar[2 * cand + 1];
                    const double lo1 = mu1 - beta * sqrt(fmax(var1, 0.0));
                    newly = !safe && lo1 > f_min;
                    if (cov) cov[cand * m + o] = cv;
                    if (lo_new) lo_new[cand * m + o] = lo1;
                }
                // the sixteen lanes of group g hold candidate `cand` at the wave's sixteen positions
                const unsigned long long b = __ballot(newly);
                const int cnt = __popcll((b >> (16 * g)) & 0xffffull);
                if (r == 0 && cnt > 0) atomicAdd(gain + cand, (unsigned long long)cnt);
            }
        }
    }
    if (tid == 0 && tiles_kept) atomicAdd(tiles_kept, (unsigned long long)kept);
}

}  // namespace

size_t whatif_part_bytes(int64_t pp) { return sizeof(double) * (size_t)pp * kWChunks * kWSums; }

hipError_t launch_whatif_fill(hipStream_t s, const float *x, const float *y, int64_t n, const float *cx,
                              const float *cy, int64_t p, int64_t pp, double ell, double sf2, double *Kt) {
    if (n <= 0 || pp <= 0) return hipSuccess;
    const double cexp = exp2_coef64(ell);
    hipLaunchKernelGGL(whatif_fill_kernel, dim3((unsigned)((n * pp + 255) / 256)), dim3(256), 0, s, x, y, n, cx, cy, p,
                       pp, cexp, sf2, Kt);
    return hipGetLastError();
}

hipError_t launch_whatif_stats(hipStream_t s, const double *Ut, const double *Wt, int64_t p, int64_t pp, int64_t n,
                               const double *z, double m0, double sf2, double noise, double beta, double *part,
                               double *cand_mu, double *cand_var, double *w_l1, double *cpar) {
    if (n <= 0 || p <= 0) return hipSuccess;
    hipLaunchKernelGGL(whatif_stats_kernel, dim3((unsigned)(pp / 16), kWChunks), dim3(256), 0, s, Ut, Wt, pp, n, z,
                       part);
    hipLaunchKernelGGL(whatif_cand_kernel, dim3((unsigned)((p + 255) / 256)), dim3(256), 0, s, part, p, m0, sf2, noise,
                       beta, cand_mu, cand_var, w_l1, cpar);
    return hipGetLastError();
}

hipError_t launch_whatif(hipStream_t s, const double *Wt, int64_t pp, int64_t p, int64_t n, const float *x,
                         const float *y, const float4 *kbox, const float4 *qbox, const float *kqx, const float *kqy,
                         const int32_t *kperm, int64_t ms, int64_t m, double ell, double sf2, int skip_L,
                         const double *mu64, const double *var64, const float *cx, const float *cy, const double *cpar,
                         double beta, double f_min, unsigned long long *gain, double *cov, double *lo_new,
                         unsigned long long *tiles_kept) {
    if (p <= 0 || ms <= 0 || n <= 0) return hipSuccess;
    const double cexp = exp2_coef64(ell);
    const dim3 grid((unsigned)((ms + kBN - 1) / kBN)), block(kWalkThreads);
#define SBO_WHATIF(NJ)                                                                                              \
    hipLaunchKernelGGL(whatif_kernel<NJ>, grid, block, 0, s, Wt, pp, p, n, x, y, kbox, qbox, kqx, kqy, kperm, ms, m, \
                       cexp, sf2, (float)skip_L, mu64, var64, cx, cy, cpar, beta, f_min, gain, cov, lo_new, tiles_kept)
    SBO_WALK_DISPATCH(pp / 16, SBO_WHATIF);
#undef SBO_WHATIF
    return hipGetLastError();
}

void whatif_cutoff(int64_t p, const double *w_l1, const double *cand_var, double s, double beta, double sf2,
                   double budget_var, double budget_mean, int *L_out, double *err_cov) {
    double l1max = 0.0;
    for (int64_t j = 0; j < p; ++j) l1max = std::max(l1max, w_l1[j]);
    *L_out = 0;
    *err_cov = 0.0;
    if (!(budget_var > 0.0) || !(budget_mean > 0.0)) return;   // dense
    int L = 16;
    for (; L < 150; ++L) {
        const double scale = sf2 * std::ldexp(1.0, -L);
        bool ok = true;
        for (int64_t j = 0; j < p && ok; ++j) {
            const double v = std::max(cand_var[j], 0.0), d = cand_var[j] + s, e = scale * w_l1[j];
            ok = std::fabs(beta) * std::sqrt(v) * e / d <= budget_mean &&
                 (2.0 * std::sqrt(sf2 * v) * e + e * e) / d <= budget_var;
        }
        if (ok) break;
    }
    *L_out = L;   // (150: no L in range qualified -- only exact zeros are dropped)
    *err_cov = whatif_err_cov(L, sf2, l1max);
}

double whatif_err_cov(int L, double sf2, double l1max) { return L > 0 ? sf2 * std::ldexp(1.0, -L) * l1max : 0.0; }

}  // namespace sbo
