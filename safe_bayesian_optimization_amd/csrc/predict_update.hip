// predict_update.hip -- the streaming tick (sbo_tick_stream): the rank-R
// update of a kept f64 posterior after a block append, and the small kernels
// that keep, compare and bound it.
//
// A block append leaves the old rows of L^-1 and the old entries of
// z = L^-1 (y - m0) as they were.  With R = n - n_map rows appended since the
// kept posterior was computed, every query q moves by
//     v      = L^-1[n_map:n, 0:n] k*(q)            (R values)
//     var   -= sum_r v_r^2
//     mu    += sum_r v_r z_r
// so the update costs R n multiply-adds and n kernel evaluations per query
// instead of the sweep's n^2 / 2.  Both operands are what sbo_append leaves on
// the device in f64: the new rows of ctx->Linv (column-major, lda = cap, zero
// above the diagonal) and the new entries of ctx->zvec.
//
// Work layout: the k-tile walk of kstar_walk.hpp, shared with the what-if
// sweep, over the new rows of L^-1: the rows of a column are contiguous, so a
// lane's A operand is one 8-byte load of a 128-byte segment.  NJ row blocks
// share the K* of a step; more rows than 16 NJ go in further passes over the
// tiles.  A cutoff of L >= 150 drops only exact zeros and is bitwise the dense
// update.  The epilogue sums v^2 and v z in a fixed order (row block, register,
// then the four lane groups) and applies them in place: no atomics on the
// state, and nothing depends on the launch grid.
#include <cstdint>

#include "kstar_walk.hpp"
#include "sbo_internal.hpp"

namespace sbo {
namespace {

// Rows are the appended rows n_map .. n of L^-1, columns the wave's positions.
template <int NJ>
__global__ __launch_bounds__(kWalkThreads) void predict_update_kernel(
    const double *__restrict__ Linv, int64_t ld, int64_t n_map, int64_t n, const double *__restrict__ z,
    const float *__restrict__ x, const float *__restrict__ y, const float4 *__restrict__ kbox,
    const float4 *__restrict__ qbox, const float *__restrict__ qx, const float *__restrict__ qy,
    const int32_t *__restrict__ perm, int64_t ms, double cexp, double sf2, float skip_L,
    double *__restrict__ mu64, double *__restrict__ var64, unsigned long long *__restrict__ tiles_kept) {
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int64_t pos = (int64_t)blockIdx.x * kBN + wave * 16 + r;
    const bool live = pos < ms;
    const double xq = live ? (double)qx[pos] : 0.0, yq = live ? (double)qy[pos] : 0.0;
    const float4 qb = qbox[blockIdx.x];
    const WalkRows A{Linv + n_map, ld, n - n_map};
    const int nrb = (int)((A.rows + 15) / 16);
    double dvar = 0.0, dmu = 0.0;
    int kept = 0;
    for (int rb0 = 0; rb0 < nrb; rb0 += NJ) {
        f64x4 acc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
        kstar_walk<NJ>(A, rb0, r, g, xq, yq, x, y, kbox, qb, n, cexp, sf2, skip_L, acc, kept);
        double s2 = 0.0, sz = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t row = n_map + (int64_t)(rb0 + j) * 16 + g + 4 * c;
                const double v = acc[j][c];
                s2 = fma(v, v, s2);
                sz = fma(v, row < n ? z[row] : 0.0, sz);
            }
        }
        s2 += __shfl_xor(s2, 16);
        s2 += __shfl_xor(s2, 32);
        sz += __shfl_xor(sz, 16);
        sz += __shfl_xor(sz, 32);
        dvar += s2;
        dmu += sz;
    }
    if (g == 0 && live && perm[pos] >= 0) {
        var64[pos] -= dvar;
        mu64[pos] += dmu;
    }
    if (tid == 0 && tiles_kept) atomicAdd(tiles_kept, (unsigned long long)kept);
}

// The new rows' 1-norms, |L^-1_r|_1 = sum_k |L^-1[n_map + r][k]| over k < n, in
// two steps with a fixed summation order.  First, workgroup (row group,
// column chunk c of kL1Chunks): thread (row r & 15, k lane tid >> 4) strides
// its chunk's columns by 16 (16 rows of a column are one 128-byte segment);
// part[r * kL1Chunks + c] = the chunk's sum.
constexpr int kL1Chunks = 32;
__global__ __launch_bounds__(256) void update_row_l1_kernel(const double *__restrict__ Linv, int64_t ld,
                                                            int64_t n_map, int64_t n, double *__restrict__ part) {
    __shared__ double red[256];
    const int tid = threadIdx.x, r = tid & 15;
    const int64_t i = (int64_t)blockIdx.x * 16 + r, row = n_map + i;
    const int64_t span = round_up((n + kL1Chunks - 1) / kL1Chunks, 16);
    const int64_t k0 = (int64_t)blockIdx.y * span, k1 = k0 + span < n ? k0 + span : n;
    double s = 0.0;
    if (row < n)
        for (int64_t k = k0 + (tid >> 4); k < k1; k += 16) s += fabs(Linv[row + k * ld]);
    red[tid] = s;
    __syncthreads();
    if (tid < 16 && row < n) {
        double t = 0.0;
        for (int j = 0; j < 16; ++j) t += red[j * 16 + tid];
        part[i * kL1Chunks + blockIdx.y] = t;
    }
}

// Then one workgroup: l1_r = its chunks' sums in ascending order, and
// head->sum_l1sq = sum_r l1_r^2, head->sum_l1z = sum_r l1_r |z_(n_map + r)| over
// the R new rows in ascending r.
__global__ __launch_bounds__(256) void update_bound_sums_kernel(const double *__restrict__ part,
                                                                const double *__restrict__ z, int64_t n_map,
                                                                int64_t R, StreamHead *__restrict__ head) {
    __shared__ double sq[256], sz[256];
    const int tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int64_t base = 0; base < R; base += 256) {
        const int64_t i = base + tid;
        double l1 = 0.0;
        if (i < R)
            for (int c = 0; c < kL1Chunks; ++c) l1 += part[i * kL1Chunks + c];
        sq[tid] = l1 * l1;
        sz[tid] = i < R ? l1 * fabs(z[n_map + i]) : 0.0;
        __syncthreads();
        if (tid == 0)
            for (int j = 0; j < 256; ++j) {
                a += sq[j];
                b += sz[j];
            }
        __syncthreads();
    }
    if (tid == 0) {
        head->sum_l1sq = a;
        head->sum_l1z = b;
    }
}

// The sweep order of a full tick, kept: coordinates and the permutation
// (identity where the tick swept in the caller's order).
__global__ void stream_keep_kernel(const float *__restrict__ qx, const float *__restrict__ qy,
                                   const int32_t *__restrict__ perm, int64_t ms, float *__restrict__ kqx,
                                   float *__restrict__ kqy, int32_t *__restrict__ kperm) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ms) return;
    kqx[i] = qx[i];
    kqy[i] = qy[i];
    kperm[i] = perm ? perm[i] : (int32_t)i;
}

// Bounding box (x0, x1, y0, y1) of each 128-position block of the kept order.
__global__ __launch_bounds__(kBN) void stream_box_kernel(const float *__restrict__ kqx, const float *__restrict__ kqy,
                                                         int64_t ms, float4 *__restrict__ qbox) {
    __shared__ float red[4 * (kBN / 64)];
    const int64_t i = (int64_t)blockIdx.x * kBN + threadIdx.x;
    float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    if (i < ms) {
        x0 = x1 = kqx[i];
        y0 = y1 = kqy[i];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        x0 = fminf(x0, __shfl_xor(x0, off));
        x1 = fmaxf(x1, __shfl_xor(x1, off));
        y0 = fminf(y0, __shfl_xor(y0, off));
        y1 = fmaxf(y1, __shfl_xor(y1, off));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[4 * w] = x0;
        red[4 * w + 1] = x1;
        red[4 * w + 2] = y0;
        red[4 * w + 3] = y1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kBN / 64; ++k) {
            x0 = fminf(x0, red[4 * k]);
            x1 = fmaxf(x1, red[4 * k + 1]);
            y0 = fminf(y0, red[4 * k + 2]);
            y1 = fmaxf(y1, red[4 * k + 3]);
        }
        qbox[blockIdx.x] = make_float4(x0, x1, y0, y1);
    }
}

// head->mismatch != 0 when a caller's query differs (bitwise) from the kept one
// of its sweep position.
__global__ void stream_compare_kernel(const float *__restrict__ qx, const float *__restrict__ qy,
                                      const float *__restrict__ kqx, const float *__restrict__ kqy,
                                      const int32_t *__restrict__ kperm, int64_t ms, StreamHead *__restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ms) return;
    const int32_t o = kperm[i];
    if (o < 0) return;
    if (__float_as_uint(qx[o]) != __float_as_uint(kqx[i]) || __float_as_uint(qy[o]) != __float_as_uint(kqy[i]))
        atomicOr(&head->mismatch, 1);
}

// The caller's order of the kept state (sbo_debug_stream_state).
__global__ void stream_scatter_kernel(const double *__restrict__ mu64, const double *__restrict__ var64,
                                      const int32_t *__restrict__ kperm, int64_t ms, double *__restrict__ mu_out,
                                      double *__restrict__ var_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ms) return;
    const int32_t o = kperm[i];
    if (o < 0) return;
    mu_out[o] = mu64[i];
    var_out[o] = var64[i];
}

}  // namespace

hipError_t launch_stream_keep(hipStream_t s, const float *qx, const float *qy, const int32_t *perm, int64_t ms,
                              float *kqx, float *kqy, int32_t *kperm, float4 *qbox) {
    if (ms <= 0) return hipSuccess;
    hipLaunchKernelGGL(stream_keep_kernel, dim3((unsigned)((ms + 255) / 256)), dim3(256), 0, s, qx, qy, perm, ms, kqx,
                       kqy, kperm);
    hipLaunchKernelGGL(stream_box_kernel, dim3((unsigned)((ms + kBN - 1) / kBN)), dim3(kBN), 0, s, kqx, kqy, ms, qbox);
    return hipGetLastError();
}

hipError_t launch_stream_compare(hipStream_t s, const float *qx, const float *qy, const float *kqx, const float *kqy,
                                 const int32_t *kperm, int64_t ms, StreamHead *head) {
    if (ms <= 0) return hipSuccess;
    hipLaunchKernelGGL(stream_compare_kernel, dim3((unsigned)((ms + 255) / 256)), dim3(256), 0, s, qx, qy, kqx, kqy,
                       kperm, ms, head);
    return hipGetLastError();
}

size_t update_l1_bytes(int64_t R) { return sizeof(double) * (size_t)R * kL1Chunks; }

hipError_t launch_update_bound_sums(hipStream_t s, const double *Linv, int64_t ld, int64_t n_map, int64_t n,
                                    const double *z, double *l1, StreamHead *head) {
    const int64_t R = n - n_map;
    if (R <= 0) return hipSuccess;
    hipLaunchKernelGGL(update_row_l1_kernel, dim3((unsigned)((R + 15) / 16), kL1Chunks), dim3(256), 0, s, Linv, ld,
                       n_map, n, l1);
    hipLaunchKernelGGL(update_bound_sums_kernel, dim3(1), dim3(256), 0, s, l1, z, n_map, R, head);
    return hipGetLastError();
}

hipError_t launch_predict_update(hipStream_t s, const double *Linv, int64_t ld, int64_t n_map, int64_t n,
                                 const double *z, const float *x, const float *y, const float4 *kbox,
                                 const float4 *qbox, const float *kqx, const float *kqy, const int32_t *kperm,
                                 int64_t ms, double ell, double sf2, int skip_L, double *mu64, double *var64,
                                 unsigned long long *tiles_kept) {
    const int64_t R = n - n_map;
    if (R <= 0 || ms <= 0) return hipSuccess;
    const double cexp = exp2_coef64(ell);
    const dim3 grid((unsigned)((ms + kBN - 1) / kBN)), block(kWalkThreads);
#define SBO_UPDATE(NJ)                                                                                          \
    hipLaunchKernelGGL(predict_update_kernel<NJ>, grid, block, 0, s, Linv, ld, n_map, n, z, x, y, kbox, qbox, kqx, \
                       kqy, kperm, ms, cexp, sf2, (float)skip_L, mu64, var64, tiles_kept)
    SBO_WALK_DISPATCH((R + 15) / 16, SBO_UPDATE);
#undef SBO_UPDATE
    return hipGetLastError();
}

hipError_t launch_stream_scatter(hipStream_t s, const double *mu64, const double *var64, const int32_t *kperm,
                                 int64_t ms, double *mu_out, double *var_out) {
    if (ms <= 0) return hipSuccess;
    hipLaunchKernelGGL(stream_scatter_kernel, dim3((unsigned)((ms + 255) / 256)), dim3(256), 0, s, mu64, var64, kperm,
                       ms, mu_out, var_out);
    return hipGetLastError();
}

}  // namespace sbo
