// evidence.hip -- model evidence from the fitted state (sbo_evidence): the log
// marginal likelihood, its gradient in (log length_scale, log sigma_f,
// log noise_level, prior_mean) and the leave-one-out predictive, read off what
// sbo_fit / sbo_append leave on the device.  Nothing here writes fitted state.
//
// With X = L^-1 (f64, column-major, lower), z = X r, alpha = X^T z, r = y - m0,
// s = noise_level + jitter and c_i = (K^-1)_ii = sum_{k >= i} X_ki^2:
//     lml      = -1/2 z'z - sum_i log L_ii - n/2 log 2 pi
//     grad[1]  = (alpha'r - s alpha'alpha) - (n - s sum c)
//     grad[2]  = 1/2 noise_level (alpha'alpha - sum c)
//     grad[3]  = sum alpha
//     grad[0]  = 1/2 sum_ij (alpha_i alpha_j - (X'X)_ij) G_ij,
//                G_ij = sf2 exp(-d_ij^2 / 2 l^2) d_ij^2 / l^2
//     loo_mean = y_i - alpha_i / c_i,  loo_var = 1 / c_i
//
// Kernels.  ev_colnorm_kernel: c_i, one workgroup per column of X (memory
// bound, one pass over the stored triangle).  ev_tile_sums_kernel: one wave
// per 64-point k-tile, the nine per-tile sums (kEvSums) the host adds up in
// tile order; two of them, a_I = sum |alpha_i| and s_I = sum sqrt(c_i), feed
// the cutoff.  ev_loo_kernel: the LOO outputs through the training order.
// ev_gram_kernel (the hot path): a work item is a kept k-tile pair I <= J and
// a chunk of kEvChunk rows k >= 64 J of X; it forms the partial 64 x 64
// product P = X[k, I]^T X[k, J] on v_mfma_f64_16x16x4_f64 from k-slabs of the
// two column blocks staged through LDS (coalesced column runs in, fragment
// reads out), evaluates G in f64 in the epilogue in the f64 C/D map (row =
// (lane >> 4) + 4 reg, column = lane & 15) and writes its contraction with
// -P (chunk 0: with alpha_i alpha_j - P) to the item's own slot.
// ev_slot_sum_kernel: one workgroup adds the slots in a fixed order.  No
// floating-point atomics: the result does not depend on the launch grid.
//
// Cutoff (evidence_pairs, host): |K^-1_ij| <= sqrt(c_i c_j), so dropping the
// pair (I, J) moves grad[0] by at most 1/2 g_max (a_I a_J + s_I s_J) per
// order, g_max = g(d_min) for boxes at least sqrt(2) l apart (g(d) = sf2
// exp(-d^2 / 2 l^2) d^2 / l^2 decreases from there on; closer pairs are kept).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "sbo_internal.hpp"

namespace sbo {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kEvThreads = 256;
constexpr int kEvSlab = 32;       // rows of X per LDS stage
// doubles per staged column: a fragment read's half wave (16 columns x 2 rows) lands on 34 c + k, 32 distinct banks
constexpr int kEvStride = 34;

__device__ __forceinline__ f64x4 mfma_f64(double a, double b, f64x4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// sum over the wave, the same value (and summation order) in every lane
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// c[i] = sum_{k = i}^{n - 1} X[k + i ld]^2: thread t adds rows i + t, i + t + 256, ..
// in ascending order, then a fixed tree over the 256 partial sums.
__global__ __launch_bounds__(kEvThreads) void ev_colnorm_kernel(const double *__restrict__ X, int64_t ld, int64_t n,
                                                                double *__restrict__ c) {
    __shared__ double red[kEvThreads];
    const int tid = threadIdx.x;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const double *col = X + i * ld;
        double s = 0.0;
        for (int64_t k = i + tid; k < n; k += kEvThreads) {
            const double v = col[k];
            s = fma(v, v, s);
        }
        red[tid] = s;
        __syncthreads();
        for (int w = kEvThreads / 2; w >= 1; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        if (tid == 0) c[i] = red[0];
        __syncthreads();
    }
}

// sums[t * kEvSums + q] over the points i of k-tile t:
//   0 |alpha_i|   1 sqrt(c_i)   2 c_i   3 alpha_i^2   4 alpha_i r_i   5 alpha_i
//   6 log L_ii    7 z_i^2       8 -1/2 log(2 pi / c_i) - 1/2 alpha_i^2 / c_i
__global__ __launch_bounds__(64) void ev_tile_sums_kernel(const double *__restrict__ c,
                                                          const double *__restrict__ alpha,
                                                          const double *__restrict__ z, const float *__restrict__ obs,
                                                          const float *__restrict__ L, int64_t ldl, double m0,
                                                          int64_t n, double *__restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * kBK + threadIdx.x;
    double q[kEvSums];
#pragma unroll
    for (int j = 0; j < kEvSums; ++j) q[j] = 0.0;
    if (i < n) {
        const double ci = c[i], a = alpha[i], zi = z[i], r = (double)obs[i] - m0;
        q[0] = fabs(a);
        q[1] = sqrt(ci);
        q[2] = ci;
        q[3] = a * a;
        q[4] = a * r;
        q[5] = a;
        q[6] = log((double)L[i + i * ldl]);
        q[7] = zi * zi;
        q[8] = -0.5 * (kEvLog2Pi - log(ci)) - 0.5 * a * a / ci;
    }
#pragma unroll
    for (int j = 0; j < kEvSums; ++j) q[j] = wave_sum(q[j]);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < kEvSums; ++j) sums[(int64_t)blockIdx.x * kEvSums + j] = q[j];
    }
}

// LOO predictive of internal row i, written at the caller's index order[i]
__global__ void ev_loo_kernel(const double *__restrict__ c, const double *__restrict__ alpha,
                              const float *__restrict__ obs, const int64_t *__restrict__ order, int64_t n,
                              double *__restrict__ loo_mean, double *__restrict__ loo_var) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t o = order[i];
    if (o < 0 || o >= n) return;
    const double ci = c[i];
    if (loo_mean) loo_mean[o] = (double)obs[i] - alpha[i] / ci;
    if (loo_var) loo_var[o] = 1.0 / ci;
}

// One item: slots[item] = w sum_ij (first alpha_i alpha_j - P_ij) G_ij over the
// 64 x 64 entries of pair (I, J), P from rows [k0, min(k0 + kEvChunk, n)) of X,
// w = 1/2 for I == J and 1 for I < J (both orders of the pair).
// Four waves; wave w owns columns 16 w .. 16 w + 15 of the J block and all four
// 16-row blocks of the I block (four accumulators).
__global__ __launch_bounds__(kEvThreads) void ev_gram_kernel(const double *__restrict__ X, int64_t ld, int64_t n,
                                                             const float *__restrict__ x, const float *__restrict__ y,
                                                             const double *__restrict__ alpha,
                                                             const int4 *__restrict__ items, double inv_l2, double sf2,
                                                             double *__restrict__ slots) {
    __shared__ double sA[kBK * kEvStride], sB[kBK * kEvStride];
    __shared__ double red[kEvThreads / 64];
    const int4 it = items[blockIdx.x];
    const int64_t colI = (int64_t)it.x * kBK, colJ = (int64_t)it.y * kBK;
    const int64_t k0 = it.z, k1 = k0 + kEvChunk < n ? k0 + kEvChunk : n;
    const bool first = it.w != 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fk = lane >> 4;
    // staging: thread (kk, cq) carries row kb + kk of columns cq + 8 m of both blocks
    const int kk = tid & (kEvSlab - 1), cq = tid / kEvSlab;
    double ra[8], rb[8];
    auto fetch = [&](int64_t kb) {
        const int64_t row = kb + kk;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int64_t ci = colI + cq + 8 * m, cj = colJ + cq + 8 * m;
            // (the stored triangle only: rows below n, columns below n, row >= column)
            ra[m] = (row < k1 && ci < n && row >= ci) ? X[row + ci * ld] : 0.0;
            rb[m] = (row < k1 && cj < n && row >= cj) ? X[row + cj * ld] : 0.0;
        }
    };
    f64x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = f64x4{0.0, 0.0, 0.0, 0.0};
    fetch(k0);
    for (int64_t kb = k0; kb < k1; kb += kEvSlab) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            sA[(cq + 8 * m) * kEvStride + kk] = ra[m];
            sB[(cq + 8 * m) * kEvStride + kk] = rb[m];
        }
        __syncthreads();
        if (kb + kEvSlab < k1) fetch(kb + kEvSlab);
#pragma unroll
        for (int s = 0; s < kEvSlab / 4; ++s) {
            const int k = 4 * s + fk;
            const double b = sB[(16 * wave + fr) * kEvStride + k];
            double a[4];
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) a[mb] = sA[(16 * mb + fr) * kEvStride + k];
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) acc[mb] = mfma_f64(a[mb], b, acc[mb]);
        }
        __syncthreads();
    }
    // epilogue: acc[mb][reg] is P[16 mb + fk + 4 reg][16 wave + fr]
    const int64_t j = colJ + 16 * wave + fr;
    const bool jin = j < n;
    const double xj = jin ? (double)x[j] : 0.0, yj = jin ? (double)y[j] : 0.0, aj = jin ? alpha[j] : 0.0;
    double sum = 0.0;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t i = colI + 16 * mb + fk + 4 * reg;
            if (jin && i < n) {
                const double dx = (double)x[i] - xj, dy = (double)y[i] - yj;
                const double u = (dx * dx + dy * dy) * inv_l2;
                const double G = sf2 * exp(-0.5 * u) * u;
                const double w = first ? alpha[i] * aj - acc[mb][reg] : -acc[mb][reg];
                sum += w * G;
            }
        }
    }
    sum = wave_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        const double t = (red[0] + red[1]) + (red[2] + red[3]);
        slots[blockIdx.x] = it.x == it.y ? 0.5 * t : t;
    }
}

// *out = sum of the slots: thread t adds slots t, t + 256, .. in ascending
// order, then a fixed tree (one workgroup, whatever the item count).
__global__ __launch_bounds__(kEvThreads) void ev_slot_sum_kernel(const double *__restrict__ slots, int64_t count,
                                                                 double *__restrict__ out) {
    __shared__ double red[kEvThreads];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int64_t i = tid; i < count; i += kEvThreads) s += slots[i];
    red[tid] = s;
    __syncthreads();
    for (int w = kEvThreads / 2; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) *out = red[0];
}

}  // namespace

hipError_t launch_evidence_norms(hipStream_t s, const double *X, int64_t ld, int64_t n, const double *alpha,
                                 const double *z, const float *obs, const float *L, int64_t ldl, double m0, double *c,
                                 double *sums) {
    if (n <= 0) return hipSuccess;
    const unsigned cols = (unsigned)std::min<int64_t>(n, 1 << 20);
    hipLaunchKernelGGL(ev_colnorm_kernel, dim3(cols), dim3(kEvThreads), 0, s, X, ld, n, c);
    hipLaunchKernelGGL(ev_tile_sums_kernel, dim3((unsigned)((n + kBK - 1) / kBK)), dim3(64), 0, s, c, alpha, z, obs, L,
                       ldl, m0, n, sums);
    return hipGetLastError();
}

hipError_t launch_evidence_loo(hipStream_t s, const double *c, const double *alpha, const float *obs,
                               const int64_t *order, int64_t n, double *loo_mean, double *loo_var) {
    if (n <= 0 || (!loo_mean && !loo_var)) return hipSuccess;
    hipLaunchKernelGGL(ev_loo_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c, alpha, obs, order, n,
                       loo_mean, loo_var);
    return hipGetLastError();
}

hipError_t launch_evidence_gram(hipStream_t s, const double *X, int64_t ld, int64_t n, const float *x, const float *y,
                                const double *alpha, const int4 *items, int64_t n_items, double ell, double sf2,
                                double *slots, double *out) {
    if (n_items > 0)
        hipLaunchKernelGGL(ev_gram_kernel, dim3((unsigned)n_items), dim3(kEvThreads), 0, s, X, ld, n, x, y, alpha, items,
                           1.0 / (ell * ell), sf2, slots);
    hipLaunchKernelGGL(ev_slot_sum_kernel, dim3(1), dim3(kEvThreads), 0, s, slots, n_items, out);
    return hipGetLastError();
}

// ------------------------------------------------------------ host: cutoff
void evidence_pairs(const float *boxes, const double *alpha_l1, const double *sqrtc_l1, int64_t T, double ell,
                    double sf2, double budget, uint8_t *drop, double *bound) {
    std::fill(drop, drop + T * T, (uint8_t)0);
    *bound = 0.0;
    if (!(budget > 0.0)) return;
    struct Cand {
        double b;
        int32_t I, J;
    };
    std::vector<Cand> cand;
    const double l2 = ell * ell;
    for (int64_t I = 0; I < T; ++I) {
        const float *p = boxes + 4 * I;
        for (int64_t J = I + 1; J < T; ++J) {
            const float *q = boxes + 4 * J;
            const double dx = std::max(0.0, std::max((double)p[0] - (double)q[1], (double)q[0] - (double)p[1]));
            const double dy = std::max(0.0, std::max((double)p[2] - (double)q[3], (double)q[2] - (double)p[3]));
            const double d2 = dx * dx + dy * dy;
            if (!(d2 >= 2.0 * l2) || !std::isfinite(d2)) continue;   // g is not yet decreasing: always kept
            const double g = sf2 * std::exp(-d2 / (2.0 * l2)) * (d2 / l2);
            // 1/2 g (a_I a_J + s_I s_J) for (I, J) and the same for (J, I)
            const double b = g * (alpha_l1[I] * alpha_l1[J] + sqrtc_l1[I] * sqrtc_l1[J]);
            if (!(b <= budget)) continue;
            cand.push_back({b, (int32_t)I, (int32_t)J});
        }
    }
    std::sort(cand.begin(), cand.end(), [](const Cand &u, const Cand &v) {
        return u.b != v.b ? u.b < v.b : u.I != v.I ? u.I < v.I : u.J < v.J;
    });
    // every pair with a bound <= tau, tau the largest bound whose pairs still fit (equal bounds go together)
    double sum = 0.0;
    size_t e = 0;
    while (e < cand.size()) {
        size_t f = e;
        double t = sum;
        while (f < cand.size() && cand[f].b == cand[e].b) t += cand[f++].b;
        if (!(t <= budget)) break;
        sum = t;
        e = f;
    }
    for (size_t i = 0; i < e; ++i) {
        drop[(int64_t)cand[i].I * T + cand[i].J] = 1;
        drop[(int64_t)cand[i].J * T + cand[i].I] = 1;
    }
    *bound = sum;
}

}  // namespace sbo
