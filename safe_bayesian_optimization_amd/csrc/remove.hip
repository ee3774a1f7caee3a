// remove.hip -- sbo_remove's kernels: a training point leaves the lower
// Cholesky factor L and its f64 inverse X = L^-1 by a chain of Givens
// rotations, and one compaction per call drops the dead rows and columns.
// The host sequence is remove_chain / remove_rows / remove_compact
// (sbo_api.cpp); the f64 model is tests/remove_model.py.
//
// Removing stored position i of n: the carry column w = L[i+1:n, i] and the
// carry row x = X[i, :]; for k = i+1 .. n-1 in this order
//     r = sqrt(L_kk^2 + w_k^2),  c = L_kk / r,  s = w_k / r
//     (L_jk, w_j) <- (c L_jk + s w_j, -s L_jk + c w_j)   rows j >= k
//     (X_kq, x_q) <- (c X_kq + s x_q, -s X_kq + c x_q)   every column q
// (r by sqrt, not hypot: the pivots of a factor of K + sn2 I are O(sf) and
// neither square leaves the f64 range.)
//
// Everything is f64: L is widened on load and rounded to f32 once per call
// on store -- one point rotates the f32 factor in place (each element is
// loaded and stored once), a batch rotates an f64 copy of the columns from the
// first removed one on, which the compaction rounds.  The carry column lives
// in an f64 workspace across the whole chain.
//
// Dependencies are stream order only: per 128 columns one diagonal-block
// launch (one workgroup: the dependent rotations, their (c, s) to the
// coefficient buffer) and one panel launch (a thread per row below the
// block), as blocked_potrf drives chol_chain.hip; the pass over X runs once
// the chain's coefficients are all there.
//
// Compiled with -ffp-contract=off: every fused multiply-add below is explicit,
// so that two contexts fed the same calls agree bit for bit.
#include "sbo_internal.hpp"

namespace sbo {
namespace {

constexpr int kRmNB = 128;     // columns of one chain step
constexpr int kRmStrip = 64;   // columns of X a workgroup owns, and rows of one tile of them
constexpr int kRmAhead = 16;   // panel loads in flight per thread

// A column-major matrix whose storage starts at column col0 (the f32 factor:
// col0 = 0; the batch's f64 copy: col0 = the first removed position).
template <class T> struct RmMat {
    T *p;
    int64_t ld, col0;
    __device__ __forceinline__ T *at(int64_t r, int64_t c) const { return p + (c - col0) * ld + r; }
};

// One rotation of the pair (v, w): v' = c v + s w, w' = c w - s v.
__device__ __forceinline__ void rotate(double c, double s, double &v, double &w) {
    const double nv = fma(c, v, s * w);
    w = fma(c, w, -(s * v));
    v = nv;
}

// w[j] = L[j, i] for j = i+1 .. n-1: the carry column.
template <class T> __global__ void remove_carry_kernel(RmMat<T> A, int64_t i, int64_t n, double *__restrict__ w) {
    const int64_t j = i + 1 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) w[j] = (double)*A.at(j, i);
}

// The diagonal step: the kb x kb block at (k0, k0), kb <= 128, and the carry's
// entries of its rows.  All four waves load the block's lower triangle into
// LDS (column c at B[c][.]: a column's rows are adjacent lanes in memory and
// in LDS alike), wave 0 runs the kb dependent rotations -- lane l owns rows l
// and l + 64 with their carry entries in registers, the pivot's carry entry is
// a lane broadcast, so the chain needs no barrier -- and all four store.  The
// pivot L_kk is read before its own column's rotation touches it: column k is
// rotated by step k alone.  A pivot that is not positive and finite raises
// *flag; the data it leaves is not used (the caller unfits the context).
template <class T>
__global__ __launch_bounds__(256) void remove_diag_kernel(RmMat<T> A, int64_t k0, int kb, double *__restrict__ w,
                                                          double *__restrict__ coef, int *__restrict__ flag) {
    __shared__ double B[kRmNB][kRmNB + 1];
    const int tid = threadIdx.x, r = tid & (kRmNB - 1);
    for (int c = tid >> 7; c < kb; c += 2)
        if (r < kb && r >= c) B[c][r] = (double)*A.at(k0 + r, k0 + c);
    __syncthreads();
    if (tid < 64) {
        const int l = tid;
        double w0 = l < kb ? w[k0 + l] : 0.0, w1 = l + 64 < kb ? w[k0 + l + 64] : 0.0;
        bool bad = false;
        for (int j = 0; j < kb; ++j) {
            const double a = B[j][j];
            const double b = __shfl(j < 64 ? w0 : w1, j & 63);
            const double rr = sqrt(fma(a, a, b * b));
            bad = bad || !(a > 0.0) || !(rr < __builtin_huge_val());
            const double c = a / rr, s = b / rr;
            if (l == 0) {
                coef[2 * (k0 + j)] = c;
                coef[2 * (k0 + j) + 1] = s;
            }
            if (l >= j && l < kb) {
                double v = B[j][l];
                rotate(c, s, v, w0);
                B[j][l] = v;
            }
            if (l + 64 >= j && l + 64 < kb) {
                double v = B[j][l + 64];
                rotate(c, s, v, w1);
                B[j][l + 64] = v;
            }
        }
        if (l < kb) w[k0 + l] = w0;
        if (l + 64 < kb) w[k0 + l + 64] = w1;
        if (bad && l == 0) *flag = 1;
    }
    __syncthreads();
    for (int c = tid >> 7; c < kb; c += 2)
        if (r < kb && r >= c) *A.at(k0 + r, k0 + c) = (T)B[c][r];
}

// The panel step: the rows below the block, one thread each, its carry entry
// in a register across the step's kb columns.  Adjacent threads read adjacent
// rows of a column-major column; the loads do not depend on the recurrence, so
// kRmAhead of them are in flight.
template <class T>
__global__ __launch_bounds__(256) void remove_panel_kernel(RmMat<T> A, int64_t k0, int kb, int64_t n,
                                                           double *__restrict__ w, const double *__restrict__ coef) {
    __shared__ double cs[2 * kRmNB];
    for (int t = threadIdx.x; t < 2 * kb; t += blockDim.x) cs[t] = coef[2 * k0 + t];
    __syncthreads();
    const int64_t j = k0 + kb + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double wj = w[j];
    T *p = A.at(j, k0);
    const int64_t ld = A.ld;
    for (int c0 = 0; c0 < kb; c0 += kRmAhead) {
        double v[kRmAhead];
#pragma unroll
        for (int u = 0; u < kRmAhead; ++u)
            if (c0 + u < kb) v[u] = (double)p[(c0 + u) * ld];
#pragma unroll
        for (int u = 0; u < kRmAhead; ++u)
            if (c0 + u < kb) {
                rotate(cs[2 * (c0 + u)], cs[2 * (c0 + u) + 1], v[u], wj);
                p[(c0 + u) * ld] = (T)v[u];
            }
    }
    w[j] = wj;
}

// The row pass over X (column-major, lower): a workgroup owns a strip of 64
// columns and walks the rows k = max(i + 1, c0) .. n-1 in tiles of 64 (a
// column above its diagonal is zero, and so is its carry until then).  All
// four waves load a tile along the columns (contiguous), wave 0 runs the
// recurrences -- lane l owns column c0 + l and its carry x -- and all four
// store.  Elements above the diagonal are neither read nor written.
__global__ __launch_bounds__(256) void remove_rows_kernel(double *__restrict__ X, int64_t ld, int64_t n, int64_t i,
                                                          const double *__restrict__ coef) {
    __shared__ double T[kRmStrip][kRmStrip + 1];   // T[column][row]
    __shared__ double cs[2 * kRmStrip];
    const int tid = threadIdx.x, tr = tid & 63, tc = tid >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * kRmStrip;
    const int64_t mycol = c0 + tid;   // (wave 0)
    double x = 0.0;
    if (tid < 64 && mycol <= i) x = X[mycol * ld + i];
    for (int64_t kt = i + 1 > c0 ? i + 1 : c0; kt < n; kt += kRmStrip) {
        const int64_t k = kt + tr;
        for (int cc = tc; cc < kRmStrip; cc += 4) {
            const int64_t col = c0 + cc;
            if (col < n && k < n && k >= col) T[cc][tr] = X[col * ld + k];
        }
        if (tid < 2 * kRmStrip && kt + (tid >> 1) < n) cs[tid] = coef[2 * kt + tid];
        __syncthreads();
        if (tid < 64 && mycol < n) {
            const int rows = (int)(n - kt < kRmStrip ? n - kt : kRmStrip);
            for (int t = 0; t < rows; ++t)
                if (kt + t >= mycol) {
                    double v = T[tid][t];
                    rotate(cs[2 * t], cs[2 * t + 1], v, x);
                    T[tid][t] = v;
                }
        }
        __syncthreads();
        for (int cc = tc; cc < kRmStrip; cc += 4) {
            const int64_t col = c0 + cc;
            if (col < n && k < n && k >= col) X[col * ld + k] = T[cc][tr];
        }
    }
}

// Compaction, first half: the elements that move -- kept row r' >= f of kept
// column c', r' >= c', f the smallest removed position -- gathered into a
// dense workspace of n1 - f rows per column.  Columns from wcol0 on come from
// the batch's f64 copy W when there is one.
template <class S>
__global__ void remove_gather_kernel(const S *__restrict__ A, int64_t lda, const double *__restrict__ W, int64_t wcol0,
                                     const int *__restrict__ keep, int64_t n1, int64_t f, S *__restrict__ ws) {
    const int64_t r = f + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n1) return;
    const int64_t sr = keep[r], rows = n1 - f;
    for (int64_t c = blockIdx.y; c <= r; c += gridDim.y) {
        const int64_t sc = keep[c];
        ws[c * rows + (r - f)] = W && sc >= wcol0 ? (S)W[(sc - wcol0) * lda + sr] : A[sc * lda + sr];
    }
}
// Second half, after the first in stream order: back to their new places.  No
// element is overwritten before its reader has read it, because every reader
// ran in the launch before.
template <class S>
__global__ void remove_scatter_kernel(S *__restrict__ A, int64_t lda, int64_t n1, int64_t f, const S *__restrict__ ws) {
    const int64_t r = f + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n1) return;
    const int64_t rows = n1 - f;
    for (int64_t c = blockIdx.y; c <= r; c += gridDim.y) A[c * lda + r] = ws[c * rows + (r - f)];
}
// The points: x, y and obs of the kept rows from f on, into ws (3 x (n1 - f)).
__global__ void remove_gather_points_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                            const float *__restrict__ obs, const int *__restrict__ keep, int64_t n1,
                                            int64_t f, float *__restrict__ ws) {
    const int64_t r = f + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n1) return;
    const int64_t sr = keep[r], rows = n1 - f;
    ws[r - f] = x[sr];
    ws[rows + r - f] = y[sr];
    ws[2 * rows + r - f] = obs[sr];
}

template <class T>
hipError_t chain_steps(hipStream_t s, RmMat<T> A, int64_t n, int64_t i, const RemoveWork &wk) {
    const int64_t below = n - 1 - i;
    if (below <= 0) return hipSuccess;
    hipLaunchKernelGGL(remove_carry_kernel<T>, dim3((unsigned)((below + 255) / 256)), dim3(256), 0, s, A, i, n, wk.w);
    for (int64_t k0 = i + 1; k0 < n; k0 += kRmNB) {
        const int kb = (int)std::min<int64_t>(kRmNB, n - k0);
        hipLaunchKernelGGL(remove_diag_kernel<T>, dim3(1), dim3(256), 0, s, A, k0, kb, wk.w, wk.coef, wk.flag);
        const int64_t rows = n - k0 - kb;
        if (rows > 0)
            hipLaunchKernelGGL(remove_panel_kernel<T>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, A, k0,
                               kb, n, wk.w, wk.coef);
    }
    return hipGetLastError();
}

template <class S>
hipError_t compact_matrix(hipStream_t s, S *A, int64_t lda, const double *W, int64_t wcol0, const int *keep,
                          int64_t n1, int64_t f, void *ws) {
    const int64_t rows = n1 - f;
    if (rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)((rows + 255) / 256), (unsigned)std::min<int64_t>(n1, kMaxGridY));
    hipLaunchKernelGGL(remove_gather_kernel<S>, grid, dim3(256), 0, s, (const S *)A, lda, W, wcol0, keep, n1, f,
                       static_cast<S *>(ws));
    hipLaunchKernelGGL(remove_scatter_kernel<S>, grid, dim3(256), 0, s, A, lda, n1, f, (const S *)ws);
    return hipGetLastError();
}

}  // namespace

size_t remove_work_bytes(int64_t n) {
    return (size_t)round_up(sizeof(double) * 3 * (size_t)n + 256, 256) + sizeof(int) * (size_t)n;
}
RemoveWork remove_work(void *base, int64_t n) {
    RemoveWork wk;
    char *p = static_cast<char *>(base);
    wk.w = reinterpret_cast<double *>(p);
    wk.coef = wk.w + n;
    wk.flag = reinterpret_cast<int *>(wk.coef + 2 * n);
    wk.keep = reinterpret_cast<int *>(p + round_up(sizeof(double) * 3 * (size_t)n + 256, 256));
    return wk;
}
size_t remove_compact_bytes(int64_t n1, int64_t f) {
    return sizeof(double) * (size_t)(n1 - f) * (size_t)std::max<int64_t>(n1, 3);
}

hipError_t launch_remove_chain(hipStream_t s, float *L, double *W, int64_t ld, int64_t wcol0, int64_t n, int64_t i,
                               const RemoveWork &wk) {
    if (W) return chain_steps(s, RmMat<double>{W, ld, wcol0}, n, i, wk);
    return chain_steps(s, RmMat<float>{L, ld, 0}, n, i, wk);
}

hipError_t launch_remove_rows(hipStream_t s, double *X, int64_t ld, int64_t n, int64_t i, const RemoveWork &wk) {
    if (n - 1 - i <= 0) return hipSuccess;
    hipLaunchKernelGGL(remove_rows_kernel, dim3((unsigned)((n + kRmStrip - 1) / kRmStrip)), dim3(256), 0, s, X, ld, n, i,
                       wk.coef);
    return hipGetLastError();
}

hipError_t launch_remove_compact(hipStream_t s, float *L, const double *W, int64_t wcol0, double *X, int64_t ld,
                                 float *x, float *y, float *obs, int64_t n1, int64_t f, const RemoveWork &wk,
                                 void *ws) {
    const int64_t rows = n1 - f;
    if (rows <= 0) return hipSuccess;
    if (hipError_t e = compact_matrix<float>(s, L, ld, W, wcol0, wk.keep, n1, f, ws)) return e;
    if (hipError_t e = compact_matrix<double>(s, X, ld, nullptr, 0, wk.keep, n1, f, ws)) return e;
    float *pw = static_cast<float *>(ws);
    hipLaunchKernelGGL(remove_gather_points_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s,
                       (const float *)x, (const float *)y, (const float *)obs, wk.keep, n1, f, pw);
    float *dst[3] = {x, y, obs};
    for (int a = 0; a < 3; ++a)
        if (hipError_t e = hipMemcpyAsync(dst[a] + f, pw + a * rows, sizeof(float) * (size_t)rows,
                                          hipMemcpyDeviceToDevice, s))
            return e;
    return hipGetLastError();
}

}  // namespace sbo
