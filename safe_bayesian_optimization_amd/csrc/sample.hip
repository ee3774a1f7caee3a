// sample.hip -- posterior sample paths on the kept grid (sbo_sample): joint
// draws of the GP posterior at every kept query by pathwise conditioning
// (Matheron's rule; Wilson et al., ICML 2020), each draw's maximiser over the
// safe set (a Thompson key) and the size of its region above f_min.  Nothing is
// appended: the fitted and the kept state are read only.  All f64.
//
// Fitted state as in whatif.hip: s = noise_level + jitter, X = L^-1 in f64, the
// training points in the factor's order, the kept f64 mean mu(q).  With F
// random Fourier features, arguments in turns:
//     g_j(x)  = sf / sqrt(F) sum_{f < F} [ a_fj cos(2 pi t_f(x)) + b_fj sin(2 pi t_f(x)) ]
//     t_f(x)  = w_f . (x - c),  w_f = nu_f / (2 pi l),  c the centre of the training bounding box
//     t_j     = g_j(train) + sqrt(s) eps_j                                   (n)
//     u_j     = X t_j,  w_j = X^T u_j  (= K^-1 t_j)
//     path_j(q) = mu(q) + g_j(q) - k*(q) . w_j          for every kept query q
// nu, a, b, eps are standard normals of the counter-based SplitMix64 /
// Box-Muller generator of terrain.py (normal_at below; the streams and their
// element numbers: include/sbo.h), so a path depends on (seed, J, F, the fit)
// only -- not on how a range of samples is cut into calls, on the training
// order or on the rank that holds a query.
//
// Layouts.  Theta^T is pp x 2 Fp column-major (pp = samples rounded up to 16,
// Fp = F rounded up to 4; column f the cos weight of feature f, column Fp + f
// its sin weight; padding rows and columns zero), stored times -sf / sqrt(F);
// T^T and W^T are column-major as whatif.hip's K_c^T and W^T, at a leading
// dimension ldw >= pp (the host runs the triangular products in row chunks of
// one fixed size, so that a sample's weights do not depend on how many samples
// share its call: readers.cpp).  So the sixteen samples of a column are one
// 128-byte segment and a lane's A operand is one 8-byte load, in the k-tile walk (kstar_walk.hpp, over W^T) and in the
// feature walk (feature_walk below, over Theta^T) alike, and both add into one
// accumulator set: acc = k* . w_j - g_j, path = mu - acc.
//
// The feature walk has the k-tile walk's workgroup shape.  A step takes four
// frequencies: lane (g = lane >> 4, r = lane & 15) forms t of frequency 4 s + g
// at its position, reduces it to [-1/2, 1/2] turns (t -= rint(t): no
// large-argument path), takes one sincospi(2 t), and the cos and the sin value
// are the B operands of NJ v_mfma_f64_16x16x4_f64 each.  It runs once with
// positions = training points (sample_train_kernel: T^T += g) and once inside
// the sweep (sample_kernel).
//
// The sweep's epilogue writes path through perm in the caller's order, counts
// path > f_min with one ballot per (sample, wave) and an integer atomic, and
// reduces (path, caller index) over the safe positions to one partial key per
// (sample, block); sample_keys_kernel combines a sample's blocks by the
// sbo_key_combine rule (a total order on (score, index): the result does not
// depend on the order of the combination).  safe(q) is whatif_kernel's.  No
// floating-point atomics anywhere: two calls agree bitwise, on any launch grid.
//
// Cutoff: dropping K* entries below 2^-L moves path_j(q) by at most
// e_j = sf2 2^-L |w_j|_1 (rigorous; sample_cutoff picks L from it).  The
// feature approximation of the prior is not bounded but measured:
// sample_kerr_kernel reports max |k^(d) / sf2 - exp(-|d|^2 / 2 l^2)| over the
// lattice d = (a, +-b) 4 l / 32, a, b = 0 .. 32, with
// k^(d) / sf2 = (1 / F) sum_f cos(2 pi w_f . d).
#include <cmath>
#include <cstdint>

#include "kstar_walk.hpp"
#include "sbo_internal.hpp"

namespace sbo {
namespace {

constexpr int kErrSide = 33;                              // lattice points a (and b) of kernel_err
constexpr int kErrOffsets = 2 * kErrSide * kErrSide;      // (a, b, sign of b)

// Output ctr (1-based) of a SplitMix64 stream started at `seed` (terrain.splitmix64).
__device__ __forceinline__ double uniform_at(uint64_t seed, uint64_t ctr) {
    uint64_t z = seed + ctr * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// Element e of terrain.normal(seed, .): Box-Muller on the uniforms 2 e and 2 e + 1.
__device__ __forceinline__ double normal_at(uint64_t seed, uint64_t e) {
    const double u1 = fmax(uniform_at(seed, 2 * e + 1), 1e-300);
    const double u2 = uniform_at(seed, 2 * e + 2);
    return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}

// w_f = nu_f / (2 pi l) in turns, zero for the padding f >= F; raw_nu (may be null): the normals themselves.
__global__ __launch_bounds__(256) void sample_freq_kernel(uint64_t seed, int64_t F, int64_t Fp, double two_pi_l,
                                                          double *__restrict__ wx, double *__restrict__ wy,
                                                          double *__restrict__ raw_nu) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= Fp) return;
    double nx = 0.0, ny = 0.0;
    if (f < F) {
        nx = normal_at(seed, 2 * (uint64_t)f);
        ny = normal_at(seed, 2 * (uint64_t)f + 1);
        if (raw_nu) raw_nu[2 * f] = nx, raw_nu[2 * f + 1] = ny;
    }
    wx[f] = nx / two_pi_l;
    wy[f] = ny / two_pi_l;
}

// Theta[j + c pp] = scale x (a_fj for c = f, b_fj for c = Fp + f) of sample J = first + j; raw_ab (may be null):
// samples x 2 F row-major, the normals themselves.
__global__ __launch_bounds__(256) void sample_theta_kernel(uint64_t seed, int64_t first, int64_t S, int64_t pp,
                                                           int64_t F, int64_t Fp, double scale,
                                                           double *__restrict__ Theta, double *__restrict__ raw_ab) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= pp * 2 * Fp) return;
    const int64_t j = i % pp, c = i / pp;
    const int64_t half = c >= Fp ? 1 : 0, f = c - half * Fp;
    double v = 0.0;
    if (j < S && f < F) {
        const uint64_t e = (uint64_t)(first + j) * (uint64_t)(2 * F) + (uint64_t)(half * F + f);
        const double nrm = normal_at(seed, e);
        v = scale * nrm;
        if (raw_ab) raw_ab[j * 2 * F + half * F + f] = nrm;
    }
    if (Theta) Theta[i] = v;
}

// Tt[j + k ldw] = sqrt(s) eps of sample J = first + j at the training point of factor row k, whose counter is its
// caller index order[k], zero for the rows S <= j < ldw; raw_eps (may be null): samples x n row-major in the
// caller's training order.
__global__ __launch_bounds__(256) void sample_eps_kernel(uint64_t seed, int64_t first, int64_t S, int64_t ldw,
                                                         int64_t n, const int64_t *__restrict__ order, double sqrt_s,
                                                         double *__restrict__ Tt, double *__restrict__ raw_eps) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ldw * n) return;
    const int64_t j = i % ldw, k = i / ldw;
    double v = 0.0;
    if (j < S) {
        const int64_t ci = order[k];
        const double nrm = normal_at(seed, ((uint64_t)(first + j) << 24) + (uint64_t)ci);
        v = sqrt_s * nrm;
        if (raw_eps) raw_eps[j * n + ci] = nrm;
    }
    if (Tt) Tt[i] = v;
}

// acc[j] += Theta[16 (rb0 + j) .. + 16, :] phi(the wave's positions), j < NJ, phi = (cos 2 pi t_f, f < Fp; sin 2 pi
// t_f, f < Fp): the steps ascending, a step's cos products before its sin products, j ascending.  (r, g) as in
// kstar_walk; (dx, dy) the lane's position less the centre c.
template <int NJ>
__device__ __forceinline__ void feature_walk(const double *__restrict__ Theta, int64_t pp, int rb0, int r, int g,
                                             double dx, double dy, const double *__restrict__ wx,
                                             const double *__restrict__ wy, int64_t Fp, f64x4 (&acc)[NJ]) {
    for (int64_t f = g; f < Fp; f += 4) {
        double t = fma(wy[f], dy, wx[f] * dx);
        t -= rint(t);
        double sn, cs;
        sincospi(2.0 * t, &sn, &cs);
        double ac[NJ], as[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int64_t row = (int64_t)(rb0 + j) * 16 + r;
            ac[j] = row < pp ? Theta[row + f * pp] : 0.0;
            as[j] = row < pp ? Theta[row + (Fp + f) * pp] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = mfma_f64(ac[j], cs, acc[j]);
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = mfma_f64(as[j], sn, acc[j]);
    }
}

// Positions are the training points in the factor's order: Tt[j + k ldw] -= (Theta phi)(j, k), i.e. T^T += g.
template <int NJ>
__global__ __launch_bounds__(kWalkThreads) void sample_train_kernel(const double *__restrict__ Theta, int64_t pp,
                                                                    int64_t n, const float *__restrict__ x,
                                                                    const float *__restrict__ y,
                                                                    const double *__restrict__ wx,
                                                                    const double *__restrict__ wy, int64_t Fp,
                                                                    double cx0, double cy0, double *__restrict__ Tt,
                                                                    int64_t ldw) {
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int64_t k = (int64_t)blockIdx.x * kBN + wave * 16 + r;
    const bool live = k < n;
    const double dx = live ? (double)x[k] - cx0 : 0.0, dy = live ? (double)y[k] - cy0 : 0.0;
    const int nrb = (int)(pp / 16);
    for (int rb0 = 0; rb0 < nrb; rb0 += NJ) {
        f64x4 acc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
        feature_walk<NJ>(Theta, pp, rb0, r, g, dx, dy, wx, wy, Fp, acc);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t row = (int64_t)(rb0 + j) * 16 + g + 4 * c;
                if (live && row < pp) Tt[row + k * ldw] -= acc[j][c];
            }
        }
    }
}

// (value a, index ai) before (b, bi) in the keys' order: sbo_key_combine's rule, ai / bi < 0 meaning none.
__device__ __forceinline__ bool path_better(double a, int64_t ai, double b, int64_t bi) {
    if (ai < 0) return false;
    if (bi < 0) return true;
    if (a > b) return true;
    if (a < b) return false;
    return ai < bi;
}

// Rows are samples, columns the wave's positions.
template <int NJ>
__global__ __launch_bounds__(kWalkThreads) void sample_kernel(
    const double *__restrict__ Wt, int64_t ldw, const double *__restrict__ Theta, int64_t pp, int64_t S, int64_t n,
    const float *__restrict__ x, const float *__restrict__ y, const float4 *__restrict__ kbox,
    const float4 *__restrict__ qbox, const float *__restrict__ qx, const float *__restrict__ qy,
    const int32_t *__restrict__ perm, int64_t ms, int64_t m, double cexp, double sf2, float skip_L,
    const double *__restrict__ mu64, const double *__restrict__ var64, const double *__restrict__ wx,
    const double *__restrict__ wy, int64_t Fp, double cx0, double cy0, double beta, double f_min,
    unsigned long long *__restrict__ count, double *__restrict__ paths, sbo_key *__restrict__ pkeys,
    unsigned long long *__restrict__ tiles_kept) {
    __shared__ double red_v[kBN / 16][16 * NJ];
    __shared__ int32_t red_i[kBN / 16][16 * NJ];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int64_t pos = (int64_t)blockIdx.x * kBN + wave * 16 + r;
    const bool live = pos < ms;
    const double xq = live ? (double)qx[pos] : 0.0, yq = live ? (double)qy[pos] : 0.0;
    const int64_t o = live ? (int64_t)perm[pos] : -1;   // the caller's index (-1: padding)
    const bool real = o >= 0;
    // the kept mean of this position and its safe flag, as whatif_kernel forms it
    double muq = 0.0;
    bool safe = false;
    if (real) {
        muq = mu64[pos];
        const double varq = var64[pos];
        const float sdf = __fsqrt_rn(varq > 0.0 ? (float)varq : 0.0f);
        safe = __dsub_rn((double)(float)muq, __dmul_rn(beta, (double)sdf)) > f_min;
    }
    const float4 qb = qbox[blockIdx.x];
    const WalkRows A{Wt, ldw, pp};
    const int nrb = (int)(pp / 16);
    int kept = 0;
    for (int rb0 = 0; rb0 < nrb; rb0 += NJ) {
        f64x4 acc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
        kstar_walk<NJ>(A, rb0, r, g, xq, yq, x, y, kbox, qb, n, cexp, sf2, skip_L, acc, kept);
        feature_walk<NJ>(Theta, pp, rb0, r, g, xq - cx0, yq - cy0, wx, wy, Fp, acc);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t smp = (int64_t)(rb0 + j) * 16 + g + 4 * c;
                const bool on = smp < S && real;
                const double v = muq - acc[j][c];
                if (on && paths) paths[smp * m + o] = v;
                // the sixteen lanes of group g hold sample `smp` at the wave's sixteen positions
                const unsigned long long b = __ballot(on && v > f_min);
                const int cnt = __popcll((b >> (16 * g)) & 0xffffull);
                if (r == 0 && cnt > 0) atomicAdd(count + smp, (unsigned long long)cnt);
                double bv = v;
                int32_t bi = (on && safe && v == v) ? (int32_t)o : -1;   // (a NaN never wins)
#pragma unroll
                for (int off = 8; off >= 1; off >>= 1) {
                    const double ov = __shfl_xor(bv, off);
                    const int32_t oi = __shfl_xor(bi, off);
                    if (path_better(ov, oi, bv, bi)) bv = ov, bi = oi;
                }
                if (r == 0) red_v[wave][j * 16 + g + 4 * c] = bv, red_i[wave][j * 16 + g + 4 * c] = bi;
            }
        }
        __syncthreads();
        if (tid < 16 * NJ) {
            double bv = red_v[0][tid];
            int32_t bi = red_i[0][tid];
            for (int w = 1; w < kBN / 16; ++w)
                if (path_better(red_v[w][tid], red_i[w][tid], bv, bi)) bv = red_v[w][tid], bi = red_i[w][tid];
            const int64_t smp = (int64_t)rb0 * 16 + tid;
            if (smp < S) pkeys[smp * gridDim.x + blockIdx.x] = sbo_key{bi < 0 ? 0.0 : bv, (int64_t)bi};
        }
        __syncthreads();
    }
    if (tid == 0 && tiles_kept) atomicAdd(tiles_kept, (unsigned long long)kept);
}

// One wave per sample: its nb partial keys combined, index_offset added.
__global__ __launch_bounds__(64) void sample_keys_kernel(const sbo_key *__restrict__ pkeys, int64_t nb,
                                                         int64_t index_offset, sbo_key *__restrict__ keys) {
    const sbo_key *in = pkeys + (int64_t)blockIdx.x * nb;
    double bv = 0.0;
    int64_t bi = -1;
    for (int64_t b = threadIdx.x; b < nb; b += 64) {
        const sbo_key k = in[b];
        if (path_better(k.score, k.idx, bv, bi)) bv = k.score, bi = k.idx;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int64_t oi = __shfl_xor(bi, off);
        if (path_better(ov, oi, bv, bi)) bv = ov, bi = oi;
    }
    if (threadIdx.x == 0) keys[blockIdx.x] = sbo_key{bi < 0 ? 0.0 : bv, bi < 0 ? -1 : bi + index_offset};
}

// Workgroup o = ((a kErrSide + b) << 1 | sign): |(1 / F) sum_f cos(2 pi w_f . d) - exp(-|d|^2 / 2 l^2)| at
// d = (a, +-b) 4 l / 32, each thread's features ascending, then the threads by a fixed tree; the maximum over the
// workgroups through the bit pattern of the non-negative double (an integer maximum; *out zeroed by the caller).
__global__ __launch_bounds__(256) void sample_kerr_kernel(const double *__restrict__ wx, const double *__restrict__ wy,
                                                          int64_t F, double ell, unsigned long long *__restrict__ out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int o = blockIdx.x, ab = o >> 1;
    const double h = 4.0 * ell / 32.0;
    const double dx = (double)(ab / kErrSide) * h, dy = ((o & 1) ? -1.0 : 1.0) * (double)(ab % kErrSide) * h;
    double sum = 0.0;
    for (int64_t f = tid; f < F; f += 256) {
        double t = fma(wy[f], dy, wx[f] * dx);
        t -= rint(t);
        sum += cospi(2.0 * t);
    }
    red[tid] = sum;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        const double e = fabs(red[0] / (double)F - exp(-fma(dy, dy, dx * dx) / (2.0 * ell * ell)));
        atomicMax(out, (unsigned long long)__double_as_longlong(e));
    }
}

}  // namespace

hipError_t launch_sample_draw(hipStream_t s, uint64_t seed, int64_t first, int64_t S, int64_t pp, int64_t ldw, int64_t F,
                              int64_t Fp, int64_t n, const int64_t *order, double ell, double sf, double noise, double *wx,
                              double *wy, double *Theta, double *Tt, double *raw_nu, double *raw_ab, double *raw_eps) {
    if (S <= 0 || F <= 0 || n <= 0) return hipSuccess;
    const auto blocks = [](int64_t items) { return dim3((unsigned)((items + 255) / 256)); };
    hipLaunchKernelGGL(sample_freq_kernel, blocks(Fp), dim3(256), 0, s, seed, F, Fp, 2.0 * M_PI * ell, wx, wy, raw_nu);
    hipLaunchKernelGGL(sample_theta_kernel, blocks(pp * 2 * Fp), dim3(256), 0, s, seed + 1, first, S, pp, F, Fp,
                       -sf / sqrt((double)F), Theta, raw_ab);
    hipLaunchKernelGGL(sample_eps_kernel, blocks(ldw * n), dim3(256), 0, s, seed + 2, first, S, ldw, n, order,
                       sqrt(noise), Tt, raw_eps);
    return hipGetLastError();
}

hipError_t launch_sample_train(hipStream_t s, const double *Theta, int64_t pp, int64_t n, const float *x,
                               const float *y, const double *wx, const double *wy, int64_t Fp, double cx0, double cy0,
                               double *Tt, int64_t ldw) {
    if (pp <= 0 || n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n + kBN - 1) / kBN)), block(kWalkThreads);
#define SBO_SAMPLE_TRAIN(NJ) \
    hipLaunchKernelGGL(sample_train_kernel<NJ>, grid, block, 0, s, Theta, pp, n, x, y, wx, wy, Fp, cx0, cy0, Tt, ldw)
    SBO_WALK_DISPATCH(pp / 16, SBO_SAMPLE_TRAIN);
#undef SBO_SAMPLE_TRAIN
    return hipGetLastError();
}

hipError_t launch_sample_kernel_err(hipStream_t s, const double *wx, const double *wy, int64_t F, double ell,
                                    unsigned long long *out) {
    hipLaunchKernelGGL(sample_kerr_kernel, dim3(kErrOffsets), dim3(256), 0, s, wx, wy, F, ell, out);
    return hipGetLastError();
}

int64_t sample_blocks(int64_t ms) { return (ms + kBN - 1) / kBN; }

hipError_t launch_sample(hipStream_t s, const double *Wt, int64_t ldw, const double *Theta, int64_t pp, int64_t S, int64_t n,
                         const float *x, const float *y, const float4 *kbox, const float4 *qbox, const float *kqx,
                         const float *kqy, const int32_t *kperm, int64_t ms, int64_t m, double ell, double sf2,
                         int skip_L, const double *mu64, const double *var64, const double *wx, const double *wy,
                         int64_t Fp, double cx0, double cy0, double beta, double f_min, int64_t index_offset,
                         unsigned long long *count, double *paths, sbo_key *pkeys, sbo_key *keys,
                         unsigned long long *tiles_kept) {
    if (S <= 0 || ms <= 0 || n <= 0) return hipSuccess;
    const double cexp = exp2_coef64(ell);
    const dim3 grid((unsigned)sample_blocks(ms)), block(kWalkThreads);
#define SBO_SAMPLE(NJ)                                                                                                \
    hipLaunchKernelGGL(sample_kernel<NJ>, grid, block, 0, s, Wt, ldw, Theta, pp, S, n, x, y, kbox, qbox, kqx, kqy, kperm, \
                       ms, m, cexp, sf2, (float)skip_L, mu64, var64, wx, wy, Fp, cx0, cy0, beta, f_min, count, paths, pkeys, \
                       tiles_kept)
    SBO_WALK_DISPATCH(pp / 16, SBO_SAMPLE);
#undef SBO_SAMPLE
    hipLaunchKernelGGL(sample_keys_kernel, dim3((unsigned)S), dim3(64), 0, s, pkeys, (int64_t)grid.x, index_offset,
                       keys);
    return hipGetLastError();
}

void sample_cutoff(int64_t S, const double *w_l1, double sf2, double budget_mean, int *L_out, double *err_path) {
    double l1max = 0.0;
    for (int64_t j = 0; j < S; ++j) l1max = std::max(l1max, w_l1[j]);
    *L_out = 0;
    *err_path = 0.0;
    if (!(budget_mean > 0.0)) return;   // dense
    int L = 16;
    while (L < 150 && !(whatif_err_cov(L, sf2, l1max) <= budget_mean)) ++L;
    *L_out = L;   // (150: no L in range qualified -- only exact zeros are dropped)
    *err_path = whatif_err_cov(L, sf2, l1max);
}

}  // namespace sbo
