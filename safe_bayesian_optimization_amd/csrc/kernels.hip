// kernels.hip -- CDNA4 (gfx950) kernels of the planning-tick hot path.
//
//   rbf_fill      a1  K = sf2 exp(-|xi-xj|^2 / 2l^2) + sn2 I      (HBM-write bound)
//   (operand.hip)     A = sf2 L^-1 into [BK][BM] tiles, the per-k-tile coordinates and the
//                     per-tile gain bounds the plan reads
//   predict       a3+a4  V = A K*^T on f32 MFMA with K* generated in registers;
//                    per row block: sum_rows V^2 (-> variance), sf2 alpha^T K* (-> mean)
//   acquire       a6+a7+a10  sum partials, sd, ComputeSets in f64, masked argmax
//
// The reference has no device code; the math contract is
// SURVEY.md 7, the acquisition restates
// /root/reference/src/safe_bayesian_optimization_node.cpp:409-416.
//
// Compiled with -ffp-contract=off: every fused multiply-add below is explicit,
// so the f64 acquisition arithmetic is the node's plain IEEE double sequence.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "plan_walk.hpp"

namespace sbo {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float fast_exp2(float v) { return __builtin_amdgcn_exp2f(v); }

// ------------------------------------------------------------------ a1 fill
// One workgroup: 1024 rows (4 per lane, one 16-B store) x kFillCols columns.
constexpr int kFillCols = 8;

// K[i + j*ld] = sf2 exp(c |a_i - b_j|^2) (+ sn2 where diag && i == j), i < ma, j < mb.
template <bool VEC>
__global__ __launch_bounds__(256) void rbf_fill_kernel(const float *__restrict__ xa,
                                                       const float *__restrict__ ya, int64_t ma,
                                                       const float *__restrict__ xb,
                                                       const float *__restrict__ yb, int64_t mb,
                                                       int64_t ld, float c, float sf2, float sn2,
                                                       int diag, float *__restrict__ K) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const int64_t j0 = (int64_t)blockIdx.y * kFillCols;
    if (i0 >= ma) return;
    const bool full = i0 + 3 < ma;
    float xi[4], yi[4];
    if (VEC && full) {
        const float4 a = *reinterpret_cast<const float4 *>(xa + i0);
        const float4 b = *reinterpret_cast<const float4 *>(ya + i0);
        xi[0] = a.x; xi[1] = a.y; xi[2] = a.z; xi[3] = a.w;
        yi[0] = b.x; yi[1] = b.y; yi[2] = b.z; yi[3] = b.w;
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t i = i0 + r < ma ? i0 + r : ma - 1;
            xi[r] = xa[i];
            yi[r] = ya[i];
        }
    }
#pragma unroll
    for (int cc = 0; cc < kFillCols; ++cc) {
        const int64_t j = j0 + cc;
        if (j >= mb) break;
        const float xj = xb[j], yj = yb[j];
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float dx = xi[r] - xj, dy = yi[r] - yj;
            v[r] = sf2 * expf(c * fmaf(dy, dy, dx * dx));
            if (diag && i0 + r == j) v[r] += sn2;
        }
        float *col = K + j * ld;
        if (VEC && full) {
            *reinterpret_cast<float4 *>(col + i0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (i0 + r < ma) col[i0 + r] = v[r];
        }
    }
}

__global__ void sub_scalar_kernel(const float *__restrict__ in, float v, int64_t n,
                                  float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] - v;
}

// (columns j = blockIdx.y + c gridDim.y: grid.y is capped at kMaxGridY)
__global__ void copy_lower_kernel(const float *__restrict__ src, int64_t lds, int64_t n,
                                  float *__restrict__ dst, int64_t ldd) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int64_t j = blockIdx.y; j < n; j += gridDim.y) dst[i + j * ldd] = i >= j ? src[i + j * lds] : 0.0f;
}

// dst[i + j*ldd] = src[i + j*lds] (f32 -> f64), i < m, j < n; lower: zero above the diagonal.
// out[r] = sum_c A[r + c * ld] x[c], c < n, for a few rows r of a column-major
// f64 matrix (one workgroup per row; strided lanes, then a fixed-order tree:
// deterministic) -- rocBLAS dgemv ran a 1 x 16384 strided row in ~300 us
__global__ __launch_bounds__(256) void row_dot_kernel(const double *__restrict__ A, int64_t ld, int64_t n,
                                                      const double *__restrict__ x, double *__restrict__ out) {
    __shared__ double red[256];
    const int64_t r = blockIdx.x;
    double s = 0.0;
    for (int64_t c = threadIdx.x; c < n; c += 256) s = fma(A[r + c * ld], x[c], s);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[r] = red[0];
}

// alpha = K^-1 r = X^T (X r) from the fit's f64 inverse X (lower, column-major,
// lda ld, its strictly upper part zero), r = obs - m0 (round 6; was two
// rocBLAS dtrmv: 0.93 + 0.48 ms at C4 for two passes over a 1 GiB triangle).
// Pass 1, z = X r: workgroup (row block of kAlRows rows, k chunk of kAlK
// columns), each thread two consecutive rows (one 16-B load per k: a wave
// reads 1 KiB of a column), r's chunk in LDS; the partial sums of chunk kc go
// to P[kc][row] and alpha_z_reduce_kernel adds them in chunk order.  Pass 2,
// alpha_k = sum_{i >= k} X[i][k] z_i: one wave per column (a contiguous read
// of rows k .. n-1), a fixed-order shuffle tree.  Both deterministic.
constexpr int kAlRows = 512, kAlK = 512;
__global__ __launch_bounds__(256) void alpha_z_kernel(const double *__restrict__ X, int64_t ld, int64_t n,
                                                      const float *__restrict__ obs, double m0,
                                                      double *__restrict__ P) {
    __shared__ double rs[kAlK];
    const int64_t r0 = (int64_t)blockIdx.x * kAlRows, k0 = (int64_t)blockIdx.y * kAlK;
    if (k0 >= r0 + kAlRows || k0 >= n) return;                       // above the diagonal: nothing
    for (int j = threadIdx.x; j < kAlK; j += 256) rs[j] = k0 + j < n ? (double)obs[k0 + j] - m0 : 0.0;
    __syncthreads();
    const int64_t row = r0 + 2 * (int64_t)threadIdx.x;
    const int64_t kend = min(min(k0 + kAlK, n), row + 2);             // k <= row + 1 (the pair's last row)
    double s0 = 0.0, s1 = 0.0;
    if (row < n) {
        const double *col = X + row;
        // (X's strictly upper part is zero: X[row][row + 1] adds nothing).  A
        // 16-B load per k when every (row, k) pair is 16-B aligned (ld even),
        // else two 8-B loads
        if (row + 1 < n && (ld & 1) == 0) {
#pragma unroll 8
            for (int64_t k = k0; k < kend; ++k) {
                const double2 v = *reinterpret_cast<const double2 *>(col + k * ld);
                s0 = fma(v.x, rs[k - k0], s0);
                s1 = fma(v.y, rs[k - k0], s1);
            }
        } else {
            const bool two = row + 1 < n;
#pragma unroll 8
            for (int64_t k = k0; k < kend; ++k) {
                s0 = fma(col[k * ld], rs[k - k0], s0);
                if (two) s1 = fma(col[k * ld + 1], rs[k - k0], s1);
            }
        }
    }
    const int64_t kc = blockIdx.y;
    if (row < n) P[kc * n + row] = s0;
    if (row + 1 < n) P[kc * n + row + 1] = s1;
}
__global__ __launch_bounds__(256) void alpha_z_reduce_kernel(const double *__restrict__ P, int64_t n,
                                                             double *__restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t nkc = i / kAlK + 1;                                 // chunks at or left of the diagonal
    double s = 0.0;
    for (int64_t kc = 0; kc < nkc; ++kc) s += P[kc * n + i];
    z[i] = s;
}
__global__ __launch_bounds__(256) void alpha_xtz_kernel(const double *__restrict__ X, int64_t ld, int64_t n,
                                                        const double *__restrict__ z, double *__restrict__ alpha) {
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n) return;
    const int lane = threadIdx.x & 63;
    const double *col = X + k * ld;
    double s = 0.0;
    // rows k .. n-1; lane l takes rows i = k + l, k + l + 64, ... (coalesced)
#pragma unroll 4
    for (int64_t i = k + lane; i < n; i += 64) s = fma(col[i], z[i], s);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) alpha[k] = s;
}

// out[i + j * ldo] = (float)d[i + j * ldd] (i < m, j = blockIdx.y)
__global__ void narrow_2d_kernel(const double *__restrict__ d, int64_t ldd, int64_t m, int64_t n,
                                 float *__restrict__ out, int64_t ldo) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    for (int64_t j = blockIdx.y; j < n; j += gridDim.y) out[i + j * ldo] = (float)d[i + j * ldd];
}

// out[j * stride] = (float)d[j]: a row of the f32 factor from an f64 vector
__global__ void narrow_strided_kernel(const double *__restrict__ d, int64_t n, float *__restrict__ out,
                                      int64_t stride) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j * stride] = (float)d[j];
}

__global__ void widen_kernel(const float *__restrict__ src, int64_t lds, int64_t m, int64_t n, int lower,
                             double *__restrict__ dst, int64_t ldd) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    for (int64_t j = blockIdx.y; j < n; j += gridDim.y)
        dst[i + j * ldd] = (!lower || i >= j) ? (double)src[i + j * lds] : 0.0;
}

// d[i] = (double)in[i] - v
__global__ void widen_sub_kernel(const float *__restrict__ in, double v, int64_t n, double *__restrict__ d) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = (double)in[i] - v;
}

__global__ void narrow_kernel(const double *__restrict__ d, int64_t n, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)d[i];
}

// ---------------------------------------------------------- a3+a4 predict
// Work item (I, qb): the BN = 128 queries [qb*BN, qb*BN+BN) against row
// block I = rows [I*BM, I*BM+BM) of A = sf2 L^-1 (BM = 256), over the k-tiles
// t < 4(I+1) the tick's plan keeps.  A workgroup has eight waves, two per
// SIMD; wave w owns the 16 queries qb*BN + 16w + (l&15) and ALL 256 rows as
// sixteen 16-row blocks: sixteen accumulators of v_mfma_f32_16x16x4_f32
// (exact f32, 64 FLOP/clk/SIMD).  The B operand K*[k][q] is generated per
// lane -- lane l holds k = l>>4, q = l&15, exactly the MFMA B-fragment map --
// so K* never touches LDS or HBM.
//
// Why this shape: on gfx950 the VALU work of a wave does not overlap the
// matrix pipe (measured, tools/mfma_probe.hip: four 32x32x2 MFMAs per K*
// value run at 86 % of peak, sixteen 16x16x4 MFMAs per K* value at 91 %), so
// the K* chain (2 sub, mul, fma, mul, exp) must be amortised over as many
// MFMAs as the register file allows.  256 rows x 16 queries per wave is 64
// accumulator registers plus 64 (f32) or 128 (f64) for the cross-tile sum,
// which leaves two waves per SIMD.
//
// The A tile [BK = 64][BM = 256] is staged through LDS by LDS-DMA (double
// buffered, one barrier per stage).  tile_offset puts the four A operands of
// row blocks 4jj..4jj+3 of one (k, row&15) side by side, so a k step is four
// conflict-free ds_read_b128 per lane.  The mean rides along in the last row
// block (every kept k visited) as an f64 FMA per k step.
//
// Plan, then sweep.  plan_count_kernel decides, per work item, which k-tiles
// run (error-budgeted, see below) and counts them; a scan turns the counts
// into offsets; plan_write_kernel writes the kept tile indices (ascending)
// and a descriptor per non-empty item, in row-block-major order, heaviest
// row block first; plan_seg_kernel cuts that item list into one contiguous,
// tile-balanced range per workgroup.  predict_kernel is persistent (one
// workgroup per CU): it walks its range as one flat stream of (item, tile)
// steps, so the LDS-DMA pipeline runs across item boundaries, and neither
// the selection nor empty items nor workgroup launches cost sweep time
// (measured on a launch-per-item kernel: selection 5.9 %, empty items 3 %,
// launch gaps ~6 % of the C4 sweep).
//
// Tile selection: with the tile-norm table (automatic cutoff) each item
// bounds tile t's share of |dV_I(q)|_2 by nu_It * K*max(box distance) and
// drops tiles smallest bound first while the dropped bounds stay within the
// row block's budget (binned, fixed point: order-independent); otherwise a
// tile whose bounding box is farther from the query block's box than the
// cutoff radius (every K* < 2^-L) is dropped.  The last row block also keeps
// every tile within the mean's cutoff.  Kept tiles run in ascending t, the
// dense order, so L >= 150 (only exact zeros dropped) is bitwise identical
// to the dense sweep.
//
// Accuracy: a single f32 MFMA chain over all N training points accumulates
// ~sqrt(N) roundings on large cancelling terms (2.2e-5 normwise variance
// error at N = 8192, measured).  Each k-tile's chain therefore starts from
// zero and is added into an outer accumulator; the K* evaluation error
// (f32 coordinate differences and exp2), amplified by A, dominates what is
// left (tools/variant_accuracy.py: 5e-6 at N = 16384 for either outer type).
constexpr int kStageFloats = kTileFloats + 3 * kBK;
constexpr int kPredictWaves = kBN / 16;
constexpr int kPredictThreads = 64 * kPredictWaves;
constexpr int kSmemFloats = 2 * kStageFloats + kPlanWalkLds / 4;  // stages + the plan's windows
constexpr int kBudgetFloor = 40;        // bounds below 2^-40 of the budget share bin 0
constexpr int kBinsPerBit = 4;
constexpr int kBudgetBins = kBudgetFloor * kBinsPerBit + 2;
constexpr int kPlanThreads = 256;       // plan kernels: one query block, one row block per wave
constexpr int kPlanWaves = kPlanThreads / 64;
constexpr int kPlanD2 = 2048;           // k-tile distances cached in LDS (N <= 131072; beyond: recomputed)
constexpr int kPlanBinCache = 256;
constexpr int kPlanWriteBlocks = 4096;  // plan_write grid cap (four waves each, grid-stride over items)      // per wave: the increment bins of a row block's first tiles (nI <= 64: all)
// Sweep time of a kept tile by precision level, in 1/64 of a full tile
// (forced-level C4 sweeps: 20.6, 13.5, 10.6 ns per tile): the weight the
// workgroup ranges and sbo_query_cost balance
constexpr unsigned kLevelWeight0 = 64, kLevelWeight1 = 42, kLevelWeight2 = 33;
// The mean's row block (the last) sweeps slower per tile than the others --
// stamp build at C4 with every tile forced to one level: the XCD chunk that
// holds it balanced at 125 / 107 / 100 % of the six- / three- / one-product
// weights -- and lower row blocks somewhat faster (their A operand fits the
// XCD's L2): tile weights of the mean's row block, and the slope, percent at
// I = nI - 1 over I = 0, of a linear per-row-block factor (diagnostic build:
// SBO_MEAN_W = "w0,w1,w2", SBO_RB_SLOPE)
constexpr unsigned kMeanWeight0 = 80, kMeanWeight1 = 45, kMeanWeight2 = 33;
__device__ unsigned g_mean_w[3] = {kMeanWeight0, kMeanWeight1, kMeanWeight2};
__device__ unsigned g_rb_slope = 0;
#ifdef SBO_DIAG
// SBO_PLAN_STATS: [0], [1] near / all (query block, k-tile) pairs of the column
// prefilter; [2..8] plan_count's wall clock (100 MHz ticks) summed over
// workgroups: setup, near list, water-filling totals, its serial part,
// thresholds, levels, the rest of the item loop
__device__ unsigned long long g_plan_near[9] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
#define SBO_PLAN_LAP(acc)                                \
    if (threadIdx.x == 0) {                              \
        const unsigned long long now_ = wall_clock64(); \
        (acc) += now_ - tprev_;                          \
        tprev_ = now_;                                   \
    }
#else
#define SBO_PLAN_LAP(acc)
#endif
constexpr int kSteps = kBK / 4;          // 16x16x4 k steps per tile
constexpr int kRowBlocks = kBM / 16;     // 16-row MFMA blocks per wave

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The sixteen k steps of one staged tile: acc = A_tile * K*_tile (fresh
// chain), mean += sf2 alpha^T K* when MEAN.
//
// Software pipeline, pinned with scheduling fences (left alone, the compiler
// minimises registers by issuing each A read right before its MFMA and then
// waiting on it): step p first issues the LDS reads of the A operands of
// step p+1 (four ds_read_b128 = the sixteen row blocks, tile_offset layout);
// every even step also reads the coordinate pairs of steps p+4, p+5 and
// evaluates K* of steps p+2, p+3 as one packed pair (v_pk_add/mul/fma_f32,
// then two v_exp_f32) beside the sixteen MFMAs of step p.  No MFMA or exp
// waits on a read issued in its own step.  pc = this lane group's
// coordinate row (operand.hip's kcoord_slot layout: step p of x at pc[p], y at
// pc[kBK + p], sf2*alpha at pc[2*kBK + p]).
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x2 kstar_pair(f32x2 x, f32x2 y, float xq, float yq, float cexp) {
    const f32x2 dx = x - xq, dy = y - yq;
    const f32x2 d2 = __builtin_elementwise_fma(dy, dy, dx * dx);
    const f32x2 a = d2 * cexp;
    f32x2 b;
    b.x = fast_exp2(a.x);
    b.y = fast_exp2(a.y);
    return b;
}

template <bool MEAN>
__device__ __forceinline__ void tile_steps(const float4 *__restrict__ pa, const float *__restrict__ pc, float xq,
                                           float yq, float cexp, f32x4 (&acc)[kRowBlocks], double &mu) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x2 *pc2 = reinterpret_cast<const f32x2 *>(pc);
    float4 a_cur[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) a_cur[jj] = pa[jj * 1024];
    f32x2 b_cur = kstar_pair(pc2[0], pc2[kBK / 2], xq, yq, cexp);  // steps 0, 1
    f32x2 x1 = pc2[1], y1 = pc2[kBK / 2 + 1];                         // steps 2, 3
    f32x2 b_nxt = b_cur;
#pragma unroll
    for (int p = 0; p < kSteps; ++p) {
        float4 a_nxt[4];
        f32x2 x2 = x1, y2 = y1;
        if (p + 1 < kSteps) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) a_nxt[jj] = pa[jj * 1024 + (p + 1) * 64];
        }
        if ((p & 1) == 0 && p + 4 < kSteps) {
            x2 = pc2[(p + 4) / 2];
            y2 = pc2[kBK / 2 + (p + 4) / 2];
        }
        const float alpha = MEAN ? pc[2 * kBK + p] : 0.0f;
        __builtin_amdgcn_sched_barrier(0);
        if ((p & 1) == 0 && p + 2 < kSteps) b_nxt = kstar_pair(x1, y1, xq, yq, cexp);
        const float b = (p & 1) ? b_cur.y : b_cur.x;
        if (MEAN) mu = fma((double)alpha, (double)b, mu);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            acc[4 * jj + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[jj].x, b, p == 0 ? zero : acc[4 * jj + 0], 0, 0, 0);
            acc[4 * jj + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[jj].y, b, p == 0 ? zero : acc[4 * jj + 1], 0, 0, 0);
            acc[4 * jj + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[jj].z, b, p == 0 ? zero : acc[4 * jj + 2], 0, 0, 0);
            acc[4 * jj + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[jj].w, b, p == 0 ? zero : acc[4 * jj + 3], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (p + 1 < kSteps) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) a_cur[jj] = a_nxt[jj];
        }
        if ((p & 1) == 0) {
            x1 = x2;
            y1 = y2;
        } else {
            b_cur = b_nxt;
        }
    }
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// ---- plan: which k-tiles each work item (I, qb) multiplies
struct QBox {
    float x0, x1, y0, y1;
};

__device__ __forceinline__ float tile_box_d2(const float4 b, const QBox &q) {
    // b = (xmin, xmax, ymin, ymax); an empty tile (+inf, -inf, ..) is infinitely far
    const float dx = fmaxf(0.0f, fmaxf(b.x - q.x1, q.x0 - b.y));
    const float dy = fmaxf(0.0f, fmaxf(b.z - q.y1, q.y0 - b.w));
    return fmaf(dy, dy, dx * dx);
}

// A kept tile runs at one of three precision levels: all six split
// products (code 0), the three largest a1 k0 + a0 k1 + a0 k0 (code 1), or
// a0 k0 alone (code 2).  With A = A0 + A1 + A2 and K = K0 + K1 + K2 the
// bf16 pieces (round to nearest at each step, so |K1| <= 2^-9 (1 + 2^-9) |K|
// and |K2| <= 2^-18 (1 + 2^-9)^2 |K| entrywise), the products code 1 leaves
// out are A2 K0 + A1 K1 + A0 K2 and code 2 also A1 K0 + A0 K1; each is
// bounded plane by plane, |A_p K_j|_2 <= min(R_p K*max, S_p |k|_2) rho_j with
// R_p = 16 max row 1-norm and S_p the spectral bound of piece p (lgn[2T+1];
// for A0: R = R_A (1 + 2^-9), S = S_A + 2^-9 |A|_F).  Lowering a tile's
// level, or dropping it, costs part of the row block's error budget; the
// three increments
//     code 0 -> 1:  c3 = |A2 K0| + |A1 K1| + |A0 K2|   (bounds as above)
//     code 1 -> 2:  c1 = |A1 K0| + |A0 K1|
//     code 2 -> drop:  b - c3 - c1,  b = min(R_A K*max, S_A |k|_2) >= |A_It k_t|_2
// sum to the tile's drop bound and are spent greedily over all tiles of the
// row block, cheapest first by error per sweep time saved (the increments
// are ranked by log2(error) + kLvlKey[j], kLvlKey from the measured per-tile
// time of the three levels and of the drop; a tile's keys never go down, so
// its spent increments are a prefix).  (Earlier rule, still an upper bound
// of these: c3 <= 3.1 2^-16 |A|_F |k|_2, c3 + c1 <= 2.03 2^-8 |A|_F |k|_2 --
// far_tile relies on it.)
// For each increment: its bin relative to the budget 2^lg_tau (bin 0 = below
// 2^-kBudgetFloor of it, bin kBudgetBins-1 = over the whole budget, never
// spent) and its weight in fixed point (2^32 = the budget), rounded up.
constexpr float kLg3 = -14.36f;  // log2(3.1 2^-16), rounded up
constexpr float kLg1 = -6.96f;   // log2(2.03 2^-8 + 3.1 2^-16), rounded up
constexpr float kRho0 = 0.0029f;          // log2(1 + 2^-9), rounded up
constexpr float kRho1 = -9.0f + 0.0029f;  // log2(2^-9 (1 + 2^-9))
constexpr float kRho2 = -18.0f + 0.0058f; // log2(2^-18 (1 + 2^-9)^2)

__device__ __forceinline__ int inc_bin(float l, unsigned long long &w, float key = 0.0f) {  // l = log2(inc / budget)
    const float f = (l + key + (float)kBudgetFloor) * (float)kBinsPerBit + 1.0f;
    const int bi = f < 0.0f ? 0 : (f >= (float)(kBudgetBins - 1) ? kBudgetBins - 1 : (int)f);
    w = bi < kBudgetBins - 1 ? (unsigned long long)ceilf(exp2f(l + 32.0f) * 1.0001f) + 1ull : 0ull;
    return bi;
}

// log2(2^a + 2^b), rounded up
__device__ __forceinline__ float lg_add(float a, float b) {
    const float hi = fmaxf(a, b), lo = fminf(a, b);
    return hi + __log2f(1.0f + exp2f(lo - hi)) + 1e-4f;
}

__device__ __forceinline__ void tile_increments(float d2, float kn, float4 lgn_t, float4 lgp_t, float cexp,
                                                float lg_tau, float2 key, int (&bi)[3],
                                                unsigned long long (&w)[3]) {
    const float kmax = cexp * d2 * 0.999f;
    const float b = fminf(lgn_t.x + kmax, lgn_t.y + kn) - lg_tau + 0.01f;
    // |A_p k|_2 bounds of the three pieces (relative to the budget)
    const float n0 = fminf(lgn_t.x + kRho0 + kmax, lg_add(lgn_t.y, lgn_t.z - 9.0f) + kn) - lg_tau + 0.01f;
    const float n1 = fminf(lgp_t.x + kmax, lgp_t.y + kn) - lg_tau + 0.01f;
    const float n2 = fminf(lgp_t.z + kmax, lgp_t.w + kn) - lg_tau + 0.01f;
    const float r3 = lg_add(lg_add(n2 + kRho0, n1 + kRho1), n0 + kRho2);   // A2 K0 + A1 K1 + A0 K2
    const float r1 = lg_add(n1 + kRho0, n0 + kRho1);                       // A1 K0 + A0 K1
    const float r31 = lg_add(r3, r1);
    bi[0] = inc_bin(r3, w[0], key.x);
    bi[1] = inc_bin(r1, w[1], key.y);
    const float dl = r31 - b;
    bi[2] = dl < -0.01f ? inc_bin(b + __log2f(1.0f - exp2f(dl)), w[2]) : inc_bin(b, w[2]);
    // monotone: the three bins never go down (so a tile's spent increments are a prefix)
    bi[1] = max(bi[1], bi[0]);
    bi[2] = max(bi[2], bi[1]);
}

// Everything the two plan kernels share: the query block's box, the box
// distance of every k-tile, and the per-item selection rule.
struct PlanRule {
    const float4 *kbox;
    const float4 *lgn;  // per packed tile log2 gain bounds, two float4 (null: distance test)
    float cexp, skip_d2, skip_d2_mean, lg_tau;
    int nI;
    QBox box;
    const float *d2s;   // LDS cache of tile distances (t < kPlanD2)
    const float *kns;   // LDS cache of the tiles' log2 |k|_2 bounds (t < kPlanD2)
    int levels;         // 0: every kept tile at full precision; 1: budgeted levels; 2 + l: timing
                        // diagnostic, the drop-only plan with every kept tile at level l
    float2 key;         // rank keys of the two level increments (SkipPlan::lvl_key)

    __device__ __forceinline__ float d2(int t) const { return t < kPlanD2 ? d2s[t] : tile_box_d2(kbox[t], box); }
    // beyond the cache: |k|_2 <= 8 K*max
    __device__ __forceinline__ float kn(int t) const { return t < kPlanD2 ? kns[t] : 3.0f + cexp * d2(t) * 0.999f; }

    // A tile whose largest possible increment (the drop bound by K*max, plus
    // the larger level rank key) is below bin 0's upper edge: all three of
    // its increments go to bin 0 with weight <= 2 each (exp2(l + 32) < 2^-8
    // rounds up to at most 1, plus 1), so the plan books 6 for it without
    // evaluating the bounds -- most candidate tiles of a row block.
    __device__ __forceinline__ bool far_lg(float l, float dd) const {
        const float kf = fmaxf(0.0f, fmaxf(key.x + kLg3, key.y + kLg1));
        return l + cexp * dd * 0.999f - lg_tau + 0.01f + kf < -(float)kBudgetFloor;
    }
    __device__ __forceinline__ bool far_tile(int I, int t, float dd) const {
        return far_lg(lgn[2 * (tile_start(I) + t)].x, dd);
    }

    // Column prefilter (near != null).  far_lg is non-decreasing in l (every
    // rounded step of it is; the build forbids contraction), so a k-tile that
    // is far by colmax[t] = max over row blocks of lgn[..].x is far for every
    // row block: the query block tests each k-tile once, and the passes below
    // walk only the ascending list of the others (nearl; bitmap nearm, its
    // prefix counts per 64 tiles nearp) and book the rest as far_tile would.
    const unsigned long long *nearm = nullptr;
    const int *nearp = nullptr;
    const unsigned short *nearl = nullptr;
    __device__ __forceinline__ int near_count(int T) const {  // near k-tiles t < T
        const int c = T >> 6, r = T & 63;
        return nearp[c] + (r ? __popcll(nearm[c] & ((1ull << r) - 1ull)) : 0);
    }

    __device__ __forceinline__ void incs(int I, int t, int (&bi)[3], unsigned long long (&w)[3]) const {
        const int64_t T = tile_start(I) + t;
        tile_increments(d2(t), kn(t), lgn[2 * T], lgn[2 * T + 1], cexp, lg_tau, key, bi, w);
        if (levels != 1) {  // only the whole drop: the first two increments free, the third the whole drop bound
            bi[0] = bi[1] = 0;
            w[0] = w[1] = 0ull;
            const float kmax = cexp * d2(t) * 0.999f;
            const float4 l = lgn[2 * T];
            bi[2] = inc_bin(fminf(l.x + kmax, l.y + kn(t)) - lg_tau + 0.01f, w[2]);
        }
    }

    // Total weight of every increment of row block I (wave-wide): what the
    // row block would spend dropping all its tiles; `over` is set when some
    // increment is larger than the whole reference budget (it never drops
    // everything).  The same increments and fixed-point weights as threshold.
    __device__ unsigned long long total_weight(int I, int lane, bool &over) const {
        const int T = kTilesPerRowBlockStep * (I + 1);
        // (prefilter: the far k-tiles booked at once, the loop over the near list)
        const int n = nearl ? near_count(T) : T;
        unsigned long long wsum = lane == 0 ? 6ull * (unsigned long long)(T - n) : 0ull;
        int ov = 0;
        for (int t0 = 0; t0 < n; t0 += 64) {
            if (t0 + lane < n) {
                const int t = nearl ? (int)nearl[t0 + lane] : t0 + lane;
                if (far_tile(I, t, d2(t))) {
                    wsum += 6ull;
                } else {
                    int bi[3];
                    unsigned long long w[3];
                    incs(I, t, bi, w);
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        if (bi[j] < kBudgetBins - 1) wsum += w[j];
                        else ov = 1;
                    }
                }
            }
            // an increment over the whole budget decides the row block (never
            // cheap): the rest of its tiles cannot change that
            if (__ballot(ov)) break;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            wsum += __shfl_xor(wsum, o);
            ov |= __shfl_xor(ov, o);
        }
        over = ov != 0;
        return wsum;
    }

    // Greedy budget threshold of row block I (wave-wide; bins is wave-private
    // LDS): the largest prefix of bins, smallest increments first, whose
    // summed weights (integer adds: order-independent) stay within the
    // row block's budget (fixed point, 2^32 = the reference budget 2^lg_tau).
    // Returns the last spent bin (-1: none).
    __device__ int threshold(int I, unsigned long long *bins, int lane, unsigned long long budget,
                             unsigned *bc = nullptr) const {
        if (!lgn) return -1;
        const int T = kTilesPerRowBlockStep * (I + 1);
        for (int i = lane; i < kBudgetBins; i += 64) bins[i] = 0ull;
        __builtin_amdgcn_wave_barrier();
        // (prefilter: a far k-tile's bc entry is not written; level_far does not read it)
        const int n = nearl ? near_count(T) : T;
        unsigned long long nfar = lane == 0 ? (unsigned long long)(T - n) : 0ull;
        for (int i = lane; i < n; i += 64) {
            const int t = nearl ? (int)nearl[i] : i;
            if (far_tile(I, t, d2(t))) {
                ++nfar;
                if (bc && t < kPlanBinCache) bc[t] = 0u;  // all three increments in bin 0
                continue;
            }
            int bi[3];
            unsigned long long w[3];
            incs(I, t, bi, w);
            if (bc && t < kPlanBinCache) bc[t] = (unsigned)bi[0] | ((unsigned)bi[1] << 8) | ((unsigned)bi[2] << 16);
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (bi[j] < kBudgetBins - 1) atomicAdd(bins + bi[j], w[j]);
        }
        if (nfar) atomicAdd(bins, 6ull * nfar);
        __builtin_amdgcn_wave_barrier();
        constexpr int per = (kBudgetBins + 63) / 64;
        unsigned long long v[per], run = 0;
#pragma unroll
        for (int j = 0; j < per; ++j) {
            const int i = lane * per + j;
            v[j] = i < kBudgetBins - 1 ? bins[i] : (1ull << 40);
            run += v[j];
        }
        unsigned long long incl = run;  // inclusive scan over lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long u = __shfl_up(incl, o);
            if (lane >= o) incl += u;
        }
        unsigned long long pre = incl - run;
        int ok = 0;
#pragma unroll
        for (int j = 0; j < per; ++j) {
            pre += v[j];
            ok += pre <= budget ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ok += __shfl_xor(ok, o);
        __builtin_amdgcn_wave_barrier();
        return ok - 1;
    }

    // The tile's level code (0 full, 1 three products, 2 one product) or -1
    // (dropped) under the row block's threshold.  bc: the bins threshold()
    // cached for this row block (a far tile's are all 0, as booked there).
    __device__ __forceinline__ int level(int I, int t, int drop_max, const unsigned *bc = nullptr) const {
        const float dd = d2(t);
        int code;
        if (lgn) {
            int spent;
            if (bc && t < kPlanBinCache) {
                const unsigned c = bc[t];
                spent = ((int)(c & 0xffu) <= drop_max) + ((int)((c >> 8) & 0xffu) <= drop_max) +
                        ((int)(c >> 16) <= drop_max);
            } else if (far_tile(I, t, dd)) {
                spent = drop_max >= 0 ? 3 : 0;
            } else {
                int bi[3];
                unsigned long long w[3];
                incs(I, t, bi, w);
                spent = (bi[0] <= drop_max) + (bi[1] <= drop_max) + (bi[2] <= drop_max);
            }
            code = spent_code(spent);
        } else {
            code = (skip_d2 <= 0.0f || dd <= skip_d2) ? 0 : -1;  // skip_d2 <= 0: dense
        }
        return mean_keep(I, dd, code);
    }
    __device__ __forceinline__ int spent_code(int spent) const {
        return spent == 3 ? -1 : (levels == 1 ? spent : (levels > 1 ? levels - 2 : 0));
    }
    // the mean's own cutoff (last row block): keep at the cheapest level
    // (its V error is below the drop bound already spent)
    __device__ __forceinline__ int mean_keep(int I, float dd, int code) const {
        if (code < 0 && I == nI - 1 && dd <= skip_d2_mean) code = lgn && levels ? 2 : 0;
        return code;
    }
    // level() of a k-tile the column prefilter found far (lgn != null)
    __device__ __forceinline__ int level_far(int I, int t, int drop_max) const {
        return mean_keep(I, d2(t), spent_code(drop_max >= 0 ? 3 : 0));
    }
};

// The plan's reference budget 2^lg_ref = tau2, the whole query block's
// |dV|_2 budget, from lg_tau = log2(tau2 / sqrt(nI)) (the even share).
__device__ __forceinline__ float plan_ref(float lg_tau, int nI) { return lg_tau + 0.5f * __log2f((float)nI) - 1e-4f; }
constexpr int kDropAll = 64 * ((kBudgetBins + 63) / 64) - 1;  // threshold() under an unlimited budget
constexpr int kPlanMaxI = 512;   // water-filling of the budget for nI <= this (N <= 131072), else even shares

// Query box of block qb (threads 0..127 hold its queries, 128..255 repeat
// them) and the distance cache.
// Bound on log2 |k_t(q)|_2 for every query q of the box: the tile's points p
// (kcoord; padding points count too, which only raises the bound) give
// K*(p, q) <= 2^(cexp dist(p, box)^2), so |k|_2^2 <= sum_p 2^(2 cexp dist^2)
// (summed scaled by 2^120 against underflow; 0.999 / 1.002 margins over the
// kernel's f32 rounding); if even that underflows, the box bound 8 K*max.
__device__ __forceinline__ float tile_knorm(const float *__restrict__ kc, const QBox &b, float cexp, float d2box) {
    float sum = 0.0f;
    // (four points per load, their loads in flight together; summed in point order)
    const float4 *kx = reinterpret_cast<const float4 *>(kc), *ky = reinterpret_cast<const float4 *>(kc + kBK);
#pragma unroll 4
    for (int i = 0; i < kBK / 4; ++i) {
        const float4 vx = kx[i], vy = ky[i];
        const float pxs[4] = {vx.x, vx.y, vx.z, vx.w}, pys[4] = {vy.x, vy.y, vy.z, vy.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float px = pxs[j], py = pys[j];
            const float dx = fmaxf(0.0f, fmaxf(b.x0 - px, px - b.x1));
            const float dy = fmaxf(0.0f, fmaxf(b.y0 - py, py - b.y1));
            sum += __builtin_amdgcn_exp2f(fmaf(2.0f * cexp, fmaf(dy, dy, dx * dx) * 0.999f, 120.0f));
        }
    }
    return sum > 0.0f ? 0.5f * (__log2f(sum * 1.002f) - 120.0f) + 0.001f : 3.0f + cexp * d2box * 0.999f;
}

__device__ QBox plan_setup(const float *__restrict__ qx, const float *__restrict__ qy, int64_t m, int64_t qb,
                           const float4 *__restrict__ kbox, const float *__restrict__ kcoord, float cexp, int nkt,
                           float *d2s, float *kns, float *red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = qb * kBN + (tid & (kBN - 1));
    const int64_t qc = q < m ? q : m - 1;
    const float xq = qx[qc], yq = qy[qc];
    const float bx0 = wave_min(xq), bx1 = wave_max(xq), by0 = wave_min(yq), by1 = wave_max(yq);
    if (lane == 0) {
        red[wave * 4 + 0] = bx0; red[wave * 4 + 1] = bx1;
        red[wave * 4 + 2] = by0; red[wave * 4 + 3] = by1;
    }
    __syncthreads();
    QBox b = {red[0], red[1], red[2], red[3]};
#pragma unroll
    for (int w = 1; w < kPlanWaves; ++w) {
        b.x0 = fminf(b.x0, red[w * 4 + 0]); b.x1 = fmaxf(b.x1, red[w * 4 + 1]);
        b.y0 = fminf(b.y0, red[w * 4 + 2]); b.y1 = fmaxf(b.y1, red[w * 4 + 3]);
    }
    for (int t = tid; t < nkt && t < kPlanD2; t += kPlanThreads) {
        const float d = tile_box_d2(kbox[t], b);
        d2s[t] = d;
        // only tiles whose box bound can reach the budget floors need the point sum
        kns[t] = (kcoord && cexp * d > -400.0f) ? tile_knorm(kcoord + (int64_t)t * (3 * kBK), b, cexp, d)
                                                : 3.0f + cexp * d * 0.999f;
    }
    __syncthreads();
    return b;
}

// Item index of (I, qb): row-block major, heaviest (last) row block first.
// Item order (round 5): row-block-major, heaviest row block first; with
// blk = bi << 8 | bq (> 0, the precise sweep's SBO_OPT_PLAN_BLOCK) in blocks
// of bi row blocks x bq query blocks, so that the sweep workgroups of one XCD,
// which run consecutive items at once, share the K* table pieces of a query
// block (bi of them) as well as the A tiles of a row block (bq of them) in
// their L2 -- instead of 32-fold A sharing and no table sharing.  A bijection
// of [0, nI nQ); plan_item_inv inverts it.
__device__ __forceinline__ int64_t plan_item(int I, int nI, int64_t nQ, int64_t qb, int blk = 0) {
    const int64_t r = nI - 1 - I;
    if (blk == 0) return r * nQ + qb;
    const int64_t bi = blk >> 8, bq = blk & 255;
    const int64_t IB = r / bi, ii = r % bi, QB = qb / bq, qq = qb % bq;
    const int64_t bie = min(bi, (int64_t)nI - IB * bi), bqe = min(bq, nQ - QB * bq);
    return IB * bi * nQ + QB * bie * bq + ii * bqe + qq;
}
__device__ __forceinline__ void plan_item_inv(int64_t item, int nI, int64_t nQ, int blk, int &I, int64_t &qb) {
    if (blk == 0) {
        I = nI - 1 - (int)(item / nQ);
        qb = item % nQ;
        return;
    }
    const int64_t bi = blk >> 8, bq = blk & 255;
    const int64_t IB = item / (bi * nQ), r0 = item - IB * bi * nQ;
    const int64_t bie = min(bi, (int64_t)nI - IB * bi);
    const int64_t QB = r0 / (bie * bq), r1 = r0 - QB * bie * bq;
    const int64_t bqe = min(bq, nQ - QB * bq);
    I = nI - 1 - (int)(IB * bi + r1 / bqe);
    qb = QB * bq + r1 % bqe;
}
// 64-tile chunks of the longest item (the code bitmap's stride per item)
__host__ __device__ __forceinline__ int plan_chunks(int nI) { return (kTilesPerRowBlockStep * nI + 63) / 64; }

// Pass 1, one workgroup per query block, one row block per wave at a time:
// the budget threshold and the kept-tile count of every item.  key packs
// (count, non-empty) for the scan; empty items get their (exactly zero)
// outputs here, so the sweep never visits them.
// With colmax (the product's path; null: the reference builder the
// diagnostic build keeps, SBO_PLAN_REF) the kernel is organised by what it
// costs -- wave-level steps, not pairs: the near list of the column
// prefilter, the water-filling totals over the flat list of near pairs, and
// no wave for the cheap row blocks.  Every shortcut
// is an integer identity or a monotone bound: the plan is the reference's.
__global__ __launch_bounds__(kPlanThreads) void plan_count_kernel(
    const float4 *__restrict__ kbox, const float *__restrict__ kcoord, const float4 *__restrict__ lgn, int levels,
    float2 lvl_key, int nI,
    int64_t nQ,
    const float *__restrict__ qx, const float *__restrict__ qy, int64_t m, float cexp, float skip_d2,
    float skip_d2_mean, float lg_tau, float m0, int64_t ldp, float *__restrict__ part, float *__restrict__ mean,
    unsigned long long *__restrict__ key, unsigned char *__restrict__ thr, unsigned long long *__restrict__ wkey,
    unsigned long long *__restrict__ bits, int wide, int blk, const float *__restrict__ colmax, int zero_empty,
    unsigned long long *__restrict__ nemask) {
    // dynamic LDS: the increment-bin cache [kPlanWaves][kPlanBinCache], then
    // the distance and |k|_2 caches of min(nkt, kPlanD2) tiles each, then the
    // near list (u16) of as many
    extern __shared__ unsigned plan_dyn[];
    __shared__ float red[4 * kPlanWaves];
    __shared__ unsigned long long nearm[kPlanD2 / 64];
    __shared__ int nearp[kPlanD2 / 64 + 1];
    __shared__ unsigned long long nem[kPlanMaxTiles / kTilesPerRowBlockStep / 64];  // bit I: item (I, qb) keeps a tile
    __shared__ unsigned long long bins[kPlanWaves][kBudgetBins];
    __shared__ unsigned long long wtot[kPlanMaxI];
    __shared__ unsigned long long budget_exp;
    __shared__ int cumn[kPlanMaxI + 1];
    __shared__ unsigned short todo[kPlanMaxI];
    __shared__ int ntodo;
    __shared__ unsigned ovm[kPlanMaxI / 32];
    const int64_t qb = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nkt = kTilesPerRowBlockStep * nI;
    const int nem_words = (nI + 63) >> 6;
    for (int i = threadIdx.x; i < nem_words; i += kPlanThreads) nem[i] = 0ull;   // (plan_setup's barriers order it)
    unsigned *bc = plan_dyn + wave * kPlanBinCache;
    float *d2s = reinterpret_cast<float *>(plan_dyn + kPlanWaves * kPlanBinCache);
    float *kns = d2s + min(nkt, kPlanD2);
    PlanRule R{kbox, lgn, cexp, skip_d2, skip_d2_mean, plan_ref(lg_tau, nI), nI, {}, d2s, kns, levels, lvl_key};
#ifdef SBO_DIAG
    unsigned long long tprev_ = wall_clock64(), lap[7] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
#endif
    R.box = plan_setup(qx, qy, m, qb, kbox, lgn ? kcoord : nullptr, cexp, nkt, d2s, kns, red);
    SBO_PLAN_LAP(lap[0])
    // The column prefilter's near list (PlanRule::nearl).  Beyond the distance
    // cache (N > 131072) every pair is tested on its own, as without colmax.
    const bool pre = lgn && colmax && nkt <= kPlanD2;
    if (pre) {
        unsigned short *nearl = reinterpret_cast<unsigned short *>(kns + nkt);
        const int nch = (nkt + 63) >> 6;
        for (int c = wave; c < nch; c += kPlanWaves) {
            const int t = c * 64 + lane;
            const unsigned long long b = __ballot(t < nkt && !R.far_lg(colmax[t < nkt ? t : 0], d2s[t < nkt ? t : 0]));
            if (lane == 0) nearm[c] = b;
        }
        __syncthreads();
        if (wave == 0) {  // nch <= 32: exclusive prefix of the chunks' near counts
            const int cnt = lane < nch ? __popcll(nearm[lane]) : 0;
            int incl = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(incl, o);
                if (lane >= o) incl += u;
            }
            if (lane < nch) nearp[lane + 1] = incl;
            if (lane == 0) nearp[0] = 0;
        }
        __syncthreads();
        for (int c = wave; c < nch; c += kPlanWaves) {
            const unsigned long long b = nearm[c];
            if ((b >> lane) & 1ull)
                nearl[nearp[c] + __popcll(b & ((1ull << lane) - 1ull))] = (unsigned short)(c * 64 + lane);
        }
        __syncthreads();
        R.nearm = nearm;
        R.nearp = nearp;
        R.nearl = nearl;
#ifdef SBO_DIAG
        if (threadIdx.x == 0) {  // SBO_PLAN_STATS: near (query block, k-tile) pairs over all
            atomicAdd(&g_plan_near[0], (unsigned long long)nearp[nch]);
            atomicAdd(&g_plan_near[1], (unsigned long long)nkt);
        }
#endif
    }
    SBO_PLAN_LAP(lap[1])
    // The error budget of the query block, |dV(q)|_2^2 = sum_I |dV_I(q)|_2^2
    // <= tau2^2 = 2^(2 lg_ref) for every query q of the block, shared over
    // its row blocks by water-filling instead of evenly (tau2 / sqrt(nI)
    // each): a row block whose tiles can all be dropped within the common
    // share drops them and spends only what they cost; the rest of tau2^2 is
    // split evenly over the others (iterated: a larger share can make more
    // row blocks cheap).  Fixed point, 2^32 = 2^lg_ref.
    const bool fill = lgn && nI <= kPlanMaxI;
    if (fill && pre) {
        // The totals over the flat list of (row block, near k-tile) pairs,
        // 256 at a time whatever row block they belong to (a row block has
        // fewer near k-tiles than a wave has lanes): pair p is near k-tile
        // p - cumn[I] of the row block I with cumn[I] <= p < cumn[I + 1].
        // Integer sums: the same totals as total_weight's.
        for (int I = threadIdx.x; I < nI; I += kPlanThreads) {
            const int T = kTilesPerRowBlockStep * (I + 1), n = R.near_count(T);
            cumn[I + 1] = n;
            wtot[I] = 6ull * (unsigned long long)(T - n);
        }
        if (threadIdx.x < kPlanMaxI / 32) ovm[threadIdx.x] = 0u;
        if (threadIdx.x == 0) cumn[0] = 0;
        __syncthreads();
        if (wave == 0) {  // cumn[1..nI]: inclusive scan, (nI + 63) / 64 entries per lane
            const int per = (nI + 63) >> 6, base = 1 + lane * per;
            int sum = 0;
            for (int j = 0; j < per; ++j) sum += base + j <= nI ? cumn[base + j] : 0;
            int incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(incl, o);
                if (lane >= o) incl += u;
            }
            int run = incl - sum;
            for (int j = 0; j < per; ++j)
                if (base + j <= nI) {
                    run += cumn[base + j];
                    cumn[base + j] = run;
                }
        }
        __syncthreads();
        const int ptot = cumn[nI];
        for (int p = threadIdx.x; p < ptot; p += kPlanThreads) {
            int lo = 0, hi = nI - 1;  // the last I with cumn[I] <= p
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (cumn[mid] <= p) lo = mid;
                else hi = mid - 1;
            }
            const int I = lo, t = (int)R.nearl[p - cumn[I]];
            if (R.far_tile(I, t, R.d2(t))) {
                atomicAdd(&wtot[I], 6ull);
            } else {
                int bi[3];
                unsigned long long w[3], ws = 0ull;
                R.incs(I, t, bi, w);
                bool ov = false;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if (bi[j] < kBudgetBins - 1) ws += w[j];
                    else ov = true;
                }
                atomicAdd(&wtot[I], ws);
                if (ov) atomicOr(&ovm[I >> 5], 1u << (I & 31));
            }
        }
        __syncthreads();
        for (int I = threadIdx.x; I < nI; I += kPlanThreads)
            if ((ovm[I >> 5] >> (I & 31)) & 1u) wtot[I] = ~0ull;
        __syncthreads();
    } else if (fill) {
        for (int I = wave; I < nI; I += kPlanWaves) {
            bool over;
            const unsigned long long w = R.total_weight(I, lane, over);
            if (lane == 0) wtot[I] = over ? ~0ull : w;
        }
        __syncthreads();
    }
    if (fill) {
        SBO_PLAN_LAP(lap[2])
        if (threadIdx.x == 0) {
            const double one = 4294967296.0;
            double share = 1.0 / sqrt((double)nI);   // the even split, in units of 2^lg_ref
            for (int it = 0; it < 4; ++it) {
                double cheap2 = 0.0;
                int nexp = 0;
                for (int I = 0; I < nI; ++I) {
                    const double w = wtot[I] == ~0ull ? 2.0 : (double)wtot[I] / one;
                    if (w <= share) cheap2 += w * w;
                    else ++nexp;
                }
                if (nexp == 0) break;
                const double s2 = fmax(0.0, (1.0 - cheap2) * (1.0 - 1e-9)) / (double)nexp;
                const double sn = sqrt(s2) * (1.0 - 1e-9);
                if (!(sn > share)) break;
                share = sn;
            }
            budget_exp = (unsigned long long)floor(share * one);
        }
        __syncthreads();
        SBO_PLAN_LAP(lap[3])
    }
    // Under the prefilter the cheap row blocks but the mean's need no wave:
    // their items are empty with the threshold of an unlimited budget
    // (kDropAll, see below), written here by one thread each -- their code
    // bitmaps are not (plan_write reads a non-empty item's only) -- and the
    // waves share the list of the others.  (zero_empty: the item loop also
    // writes the empty items' partials.)
    const bool flat = pre && fill && !zero_empty;
    if (flat) {
        if (wave == 0) {
            int base = 0;
            for (int I0 = 0; I0 < nI; I0 += 64) {
                const int I = I0 + lane;
                const bool work = I < nI && (I == nI - 1 || wtot[I] > budget_exp);
                const unsigned long long b = __ballot(work);
                if (work) todo[base + __popcll(b & ((1ull << lane) - 1ull))] = (unsigned short)I;
                base += __popcll(b);
            }
            if (lane == 0) ntodo = base;
        }
        for (int I = threadIdx.x; I < nI - 1; I += kPlanThreads)
            if (wtot[I] <= budget_exp) {
                const int64_t item = plan_item(I, nI, nQ, qb, blk);
                key[item] = 0ull;
                thr[item] = (unsigned char)(kDropAll + 1);
                wkey[item] = 0ull;
            }
        __syncthreads();
    }
    const int nwork = flat ? ntodo : nI;
    for (int idx = wave; idx < nwork; idx += kPlanWaves) {
        const int I = flat ? (int)todo[idx] : idx;
        const int T = kTilesPerRowBlockStep * (I + 1);
        // a cheap row block (everything within the share) spends its own total
        const unsigned long long bud = !fill ? (unsigned long long)floor(4294967296.0 / sqrt((double)nI))
                                       : (wtot[I] <= budget_exp ? ~0ull : budget_exp);
        // A cheap row block under the prefilter: threshold() with the budget
        // ~0 counts every slot of its scan, whatever the bins hold, and every
        // tile is dropped (but for the mean's cutoff) -- nothing to evaluate.
        const bool cheap = pre && bud == ~0ull;
        const int drop_max = cheap ? kDropAll : R.threshold(I, bins[wave], lane, bud, bc);
        SBO_PLAN_LAP(lap[4])
        const int64_t item = plan_item(I, nI, nQ, qb, blk);
        // the item's codes, 64 tiles per chunk: kept / level 1 / level 2 masks (read by plan_write)
        unsigned long long *ib = bits + item * (int64_t)plan_chunks(nI) * 3;
        int cnt = 0;
        unsigned wsum = 0;
#pragma unroll 1
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int t = t0 + lane;
            int code;
            if (cheap) {
                if (I != nI - 1) {
                    if (lane < 3) ib[(t0 >> 6) * 3 + lane] = 0ull;
                    continue;
                }
                code = t < T ? R.mean_keep(I, R.d2(t), -1) : -1;
            } else if (pre) {
                const unsigned long long nm = nearm[t0 >> 6];
                // no near k-tile in the chunk, and a far one is dropped: all dropped
                if (nm == 0ull && drop_max >= 0 && I != nI - 1) {
                    if (lane < 3) ib[(t0 >> 6) * 3 + lane] = 0ull;
                    continue;
                }
                code = t < T ? (((nm >> lane) & 1ull) ? R.level(I, t, drop_max, bc) : R.level_far(I, t, drop_max)) : -1;
            } else {
                code = t < T ? R.level(I, t, drop_max, bc) : -1;
            }
            const unsigned long long b0 = __ballot(code == 0), b1 = __ballot(code == 1), b2 = __ballot(code == 2);
            if (lane < 3) ib[(t0 >> 6) * 3 + lane] = lane == 0 ? (b0 | b1 | b2) : (lane == 1 ? b1 : b2);
            const int n0 = __popcll(b0), n1 = __popcll(b1), n2 = __popcll(b2);
            cnt += n0 + n1 + n2;
            wsum += I == nI - 1 ? g_mean_w[0] * n0 + g_mean_w[1] * n1 + g_mean_w[2] * n2
                                : kLevelWeight0 * n0 + kLevelWeight1 * n1 + kLevelWeight2 * n2;
        }
        SBO_PLAN_LAP(lap[5])
        if (g_rb_slope)
            wsum = (unsigned)((unsigned long long)wsum * (100u * (unsigned)nI + g_rb_slope * (unsigned)I) /
                              (100u * (unsigned)nI));
        if (lane == 0) {
            key[item] = plan_key_pack(cnt);
            thr[item] = (unsigned char)(drop_max + 1);
            wkey[item] = wsum;
            if (cnt > 0) atomicOr(&nem[I >> 6], 1ull << (I & 63));
        }
        if (cnt == 0)
            for (int j = lane; j < kBN; j += 64) {
                const int64_t q = qb * kBN + j;
                if (q < m) {
                    // (wide: the precise sweep's f64 partials and mean)
                    // (zero_empty == 0: the acquisition skips an empty item's partial by nemask)
                    if (wide) {
                        if (zero_empty) reinterpret_cast<double *>(part)[(int64_t)I * ldp + q] = 0.0;
                        if (I == nI - 1) reinterpret_cast<double *>(mean)[q] = (double)m0;
                    } else {
                        if (zero_empty) part[(int64_t)I * ldp + q] = 0.0f;
                        if (I == nI - 1) mean[q] = m0;
                    }
                }
            }
        SBO_PLAN_LAP(lap[6])
    }
#ifdef SBO_DIAG
    if (threadIdx.x == 0)
        for (int i = 0; i < 7; ++i) atomicAdd(&g_plan_near[2 + i], lap[i]);
#endif
    __syncthreads();
    for (int i = threadIdx.x; i < nem_words; i += kPlanThreads) nemask[qb * nem_words + i] = nem[i];
}

// Pass 2 (after the inclusive scan of key): the kept tile indices of every
// non-empty item, ascending, at its offset, and its descriptor
// (I, qb, offset low 32 bits, count | offset high bits << 16) -- from the
// code bitmap plan_count left (bits: per item and 64-tile chunk, the kept /
// level-1 / level-2 masks), so no tile's bounds are evaluated twice.  Each
// wave walks items gw, gw + W, .. (W = all waves of the grid).
__global__ __launch_bounds__(256) void plan_write_kernel(
    int nI, int64_t nQ, const unsigned long long *__restrict__ key, const unsigned long long *__restrict__ scan,
    const unsigned long long *__restrict__ bits, int4 *__restrict__ desc, unsigned short *__restrict__ tl,
    int prod_full, unsigned long long *__restrict__ partial, int blk) {
    // partial (may be null): per wave [MFMA products, tiles at level 1, at level 2]
    // (summed by plan_counts_reduce_kernel: no contended global atomics)
    const int lane = threadIdx.x & 63;
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
    const int64_t items = (int64_t)nI * nQ;
    unsigned long long prod = 0, nl1 = 0, nl2 = 0;
    for (int64_t item = gw; item < items; item += nw) {
        const unsigned long long k = key[item];
        const int cnt = (int)plan_key_count(k);
        if (cnt > 0) {
            int I;
            int64_t qb;
            plan_item_inv(item, nI, nQ, blk, I, qb);
            const unsigned long long ex = scan[item] - k;
            const uint64_t off = plan_key_count(ex);
            const int64_t ne = plan_key_items(ex);
            const int T = kTilesPerRowBlockStep * (I + 1);
            const unsigned long long *ib = bits + item * (int64_t)plan_chunks(nI) * 3;
            uint64_t base = off;
            for (int t0 = 0; t0 < T; t0 += 64) {
                const unsigned long long kept = ib[(t0 >> 6) * 3], l1 = ib[(t0 >> 6) * 3 + 1],
                                         l2 = ib[(t0 >> 6) * 3 + 2];
                if ((kept >> lane) & 1ull) {
                    const int code = ((l1 >> lane) & 1ull) ? 1 : (((l2 >> lane) & 1ull) ? 2 : 0);
                    tl[base + __popcll(kept & ((1ull << lane) - 1ull))] = plan_entry_pack(t0 + lane, code);
                    prod += code == 0 ? prod_full : (code == 1 ? 3 : 1);
                    nl1 += code == 1 ? 1 : 0;
                    nl2 += code == 2 ? 1 : 0;
                }
                base += __popcll(kept);
            }
            if (lane == 0) desc[ne] = plan_item_int4(I, (int)qb, off, cnt);
        }
    }
    if (partial) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            prod += __shfl_xor(prod, o);
            nl1 += __shfl_xor(nl1, o);
            nl2 += __shfl_xor(nl2, o);
        }
        if (lane == 0) {
            unsigned long long *p = partial + 3 * gw;
            p[0] = prod;
            p[1] = nl1;
            p[2] = nl2;
        }
    }
}

// One workgroup: the per-wave level counts of plan_write into the profile counters.
__global__ __launch_bounds__(256) void plan_counts_reduce_kernel(const unsigned long long *__restrict__ partial,
                                                                 int64_t n, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long red[3][256];
    unsigned long long v[3] = {0, 0, 0};
    for (int64_t i = threadIdx.x; i < n; i += 256)
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] += partial[3 * i + j];
#pragma unroll
    for (int j = 0; j < 3; ++j) red[j][threadIdx.x] = v[j];
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o)
#pragma unroll
            for (int j = 0; j < 3; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0)
#pragma unroll
        for (int j = 0; j < 3; ++j) out[j] += red[j][0];
}

// One thread per sweep workgroup: cut the non-empty item list into P
// contiguous ranges of about equal sweep time -- the level-weighted tile
// count (wkey, inclusive scan wscan) -- (seg[r] .. seg[r+1]).
__global__ void plan_seg_kernel(const unsigned long long *__restrict__ scan, int64_t n_items,
                                const int4 *__restrict__ desc, int P, int *__restrict__ seg,
                                unsigned long long *__restrict__ tiles_done, const unsigned long long *__restrict__ wkey,
                                const unsigned long long *__restrict__ wscan, int nI, int64_t nQ, int blk) {
    const unsigned long long last = scan[n_items - 1];
    const uint64_t total = plan_key_count(last);
    const uint64_t wtotal = wscan[n_items - 1];
    const int64_t nne = plan_key_items(last);
    for (int w = threadIdx.x; w <= P; w += blockDim.x) {
        if (w == P) {
            seg[P] = (int)nne;
            continue;
        }
        const uint64_t target = wtotal * (uint64_t)w / (uint64_t)P;
        int64_t lo = 0, hi = nne;  // first item whose weighted offset >= target
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            const int4 d = desc[mid];
            const int64_t it = plan_item(d.x, nI, nQ, d.y, blk);
            const uint64_t off = wscan[it] - wkey[it];
            if (off < target) lo = mid + 1; else hi = mid;
        }
        seg[w] = (int)lo;
    }
    if (threadIdx.x == 0 && tiles_done) atomicAdd(tiles_done, (unsigned long long)total);
}

// XCD-interleaved item order (P a multiple of 8).  The sweep's workgroup b
// runs on XCD b % 8, and an XCD's 32 CUs share one L2: with contiguous
// per-workgroup ranges they work on 32 far-apart items at once and share no
// A tile (the staged bytes all come from beyond L2).  Instead each XCD takes
// one tile-balanced contiguous chunk [a, b) of the item list (plan_seg with
// 8 ranges, xseg), and its G = P/8 workgroups take the chunk's items
// round-robin -- slot c runs items a + c, a + c + G, ... -- so at any time
// they sweep G neighbouring items (same row block, Morton-adjacent query
// blocks, mostly the same k-tiles).  The descriptors and tile lists are
// permuted so that every workgroup's items stay contiguous (the sweep walks
// one contiguous range either way).
__device__ __forceinline__ int64_t xcd_position(int64_t k, const int *__restrict__ xseg, int G) {
    int x = 0;
#pragma unroll
    for (int i = 1; i < 8; ++i) x += k >= xseg[i] ? 1 : 0;
    const int64_t a = xseg[x], n = xseg[x + 1] - a, q = n / G, rm = n % G, c = (k - a) % G, j = (k - a) / G;
    return a + c * q + (c < rm ? c : rm) + j;
}

__global__ void plan_perm_kernel(const unsigned long long *__restrict__ scan, int64_t n_items,
                                 const int4 *__restrict__ desc, const int *__restrict__ xseg, int G,
                                 int *__restrict__ pos_of, unsigned long long *__restrict__ cnt2) {
    const int64_t nne = plan_key_items(scan[n_items - 1]);
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nne) {
        // (the permutation maps [0, nne) onto itself: the positions past it count 0 for the scan)
        if (k < n_items) cnt2[k] = 0ull;
        return;
    }
    const int64_t p = xcd_position(k, xseg, G);
    pos_of[k] = (int)p;
    cnt2[p] = (unsigned long long)plan_item_count(desc[k].w);
}

__device__ __forceinline__ int4 step_record(int64_t ts, int I, int qb, int te, int i, int cnt);

// one wave per item: its tile list to the new offset, its descriptor to its
// new position, and (rec != nullptr) the split sweep's step records of the
// moved list -- what plan_rec_kernel would write from desc2 / tl2
__global__ __launch_bounds__(256) void plan_move_kernel(const unsigned long long *__restrict__ scan, int64_t n_items,
                                                        const int4 *__restrict__ desc,
                                                        const unsigned short *__restrict__ tl,
                                                        const int *__restrict__ pos_of,
                                                        const unsigned long long *__restrict__ off2,
                                                        int4 *__restrict__ desc2, unsigned short *__restrict__ tl2,
                                                        int4 *__restrict__ rec) {
    const int64_t nne = plan_key_items(scan[n_items - 1]);
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (k >= nne) return;
    const int4 d = desc[k];
    const int cnt = plan_item_count(d.w);
    const uint64_t off = plan_item_offset(d.z, d.w);
    const int p = pos_of[k];
    const uint64_t o2 = off2[p];
    const int64_t ts = tile_start(d.x);
    for (int i = lane; i < cnt; i += 64) {
        const unsigned short te = tl[off + i];
        tl2[o2 + i] = te;
        if (rec) rec[o2 + i] = step_record(ts, d.x, d.y, te, i, cnt);
    }
    if (lane == 0) desc2[p] = plan_item_int4(d.x, d.y, o2, cnt);
}

// Step records of the split sweep (plan_format.hpp), one
// wave per non-empty item, in the order the sweep walks the list (after the
// XCD permutation, where plan_move_kernel writes them): the kernel then
// stages a tile from one record instead of re-deriving offsets from the
// descriptor and tile list in every wave.
__device__ __forceinline__ int4 step_record(int64_t ts, int I, int qb, int te, int i, int cnt) {
    const int t = plan_entry_tile(te);
    const int w = I | (plan_entry_level(te) << kRecLevelShift) | (i == 0 ? kRecFirst : 0) | (i == cnt - 1 ? kRecLast : 0);
    return make_int4((int)(uint32_t)((ts + t) * 96), t * 256, qb, w);
}

__global__ __launch_bounds__(256) void plan_rec_kernel(const unsigned long long *__restrict__ scan, int64_t n_items,
                                                       const int4 *__restrict__ desc,
                                                       const unsigned short *__restrict__ tl, int4 *__restrict__ rec) {
    const int64_t nne = plan_key_items(scan[n_items - 1]);
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (k >= nne) return;
    const int4 d = desc[k];
    const int cnt = plan_item_count(d.w);
    const uint64_t off = plan_item_offset(d.z, d.w);
    const int64_t ts = tile_start(d.x);
    for (int i = lane; i < cnt; i += 64) rec[off + i] = step_record(ts, d.x, d.y, tl[off + i], i, cnt);
}

__global__ void plan_seg2_kernel(const int *__restrict__ xseg, int G, int P, int *__restrict__ seg2) {
    for (int r = threadIdx.x; r <= P; r += blockDim.x) {
        if (r == P) {
            seg2[P] = xseg[8];
            continue;
        }
        const int x = r / G, c = r % G;
        const int a = xseg[x], n = xseg[x + 1] - a, q = n / G, rm = n % G;
        seg2[r] = a + c * q + (c < rm ? c : rm);
    }
}

// Sweep work per query from a plan (load balancing across ranks): the kept
// tiles of its 128-query block summed over row blocks, shared by the block's
// queries; written in the caller's order (perm: sweep position -> caller).
__global__ void plan_block_cost_kernel(const unsigned long long *__restrict__ wkey, int nI, int64_t nQ,
                                       float *__restrict__ bcost) {
    const int64_t qb = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (qb >= nQ) return;
    unsigned long long c = 0;
    for (int I = 0; I < nI; ++I) c += wkey[plan_item(I, nI, nQ, qb)];
    bcost[qb] = (float)((double)c / (double)kLevelWeight0);  // in full-precision tiles
}

// a block's cost is shared by its queries (a grid patch's padded positions,
// perm -1, take no share): one block per workgroup of kBN threads
__global__ __launch_bounds__(kBN) void plan_query_cost_kernel(const float *__restrict__ bcost, int64_t m,
                                                              const int32_t *__restrict__ perm,
                                                              float *__restrict__ cost) {
    __shared__ int nv;
    const int64_t qb = blockIdx.x, i = qb * kBN + threadIdx.x;
    const int64_t o = i < m ? (perm ? (int64_t)perm[i] : i) : -1;  // (-1: padding)
    if (threadIdx.x == 0) nv = 0;
    __syncthreads();
    if (o >= 0) atomicAdd(&nv, 1);
    __syncthreads();
    if (o >= 0) cost[o] = bcost[qb] / (float)nv;
}

// ---- the sweep (persistent: one workgroup per CU)
// OT: outer (cross-tile) accumulator type.  Workgroup b walks the item range
// r(b) of the plan; consecutive ranges go to one XCD (blocks are dealt to the
// 8 XCDs round-robin), so an XCD's L2 sees neighbouring items.
template <class OT, int LOADERS = kPredictWaves / 2>
__global__ __launch_bounds__(kPredictThreads, 1) void predict_kernel(
    const float *__restrict__ aug, const float *__restrict__ kcoord, const int4 *__restrict__ desc,
    const unsigned short *__restrict__ tl, const int *__restrict__ seg, int P, int n_items, int nI,
    const float *__restrict__ qx, const float *__restrict__ qy, int64_t m, int64_t ldp, float cexp, float m0,
    float *__restrict__ part, float *__restrict__ mean) {
    __shared__ __attribute__((aligned(16))) float smem[kSmemFloats];
    const PlanRange range = plan_range(seg, P, n_items);
    const int k0 = range.k0, k1 = range.k1;
    if (k0 >= k1) return;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int g = lane >> 4;   // k within the step
    const int r = lane & 15;   // row within a 16-row block / query within the wave

    // LDS: two stages, then the plan's windows.  A stage = the 64 KiB
    // [BK][BM] tile (16 LDS-DMA instructions per loader wave, lds_dma16) +
    // 768 B of per-k coordinates.  Every stage and window is retired by the
    // explicit vmcnt(0) + barrier at the end of each step.
    typedef __attribute__((address_space(3))) char lds_char;
    constexpr int kTileBytes = kTileFloats * 4, kStageBytes = kStageFloats * 4, kCBytes = 3 * kBK * 4;
    // Only the last LOADERS waves (one per SIMD) issue the stage, 16 pieces
    // each; the first four go straight from the barrier into their MFMAs
    // (1.8 % over every wave issuing 8, measured at C4).
    constexpr int kWaveStride = kTileBytes / LOADERS;  // bytes per loader wave per stage
    const int lw = wave - (kPredictWaves - LOADERS);    // loader index (< 0: not a loader)
    const bool loader = lw >= 0;
    const char *gA = reinterpret_cast<const char *>(aug) + (loader ? lw : 0) * 1024 + lane * 16;
    const char *gC = reinterpret_cast<const char *>(kcoord) + lane * 16;
    const uint32_t lds_smem = (uint32_t)(uintptr_t)(lds_char *)(smem);
    const uint32_t lds_wave = lds_smem + (uint32_t)__builtin_amdgcn_readfirstlane(loader ? lw : 0) * 1024u;
    const char *wbase = reinterpret_cast<const char *>(smem + 2 * kStageFloats);
    const PlanWindows win(wbase, nI);
    const PlanRefill refill(wbase, desc, tl, lane, lw == 1, lw == 2);
#define SBO_STAGE(I_, t_, buf)                                                                          \
    do {                                                                                                \
        if (loader) {                                                                                   \
            const char *s_ = gA + (tile_start(I_) + (t_)) * (int64_t)kTileBytes;                       \
            const uint32_t d_ = lds_wave + (uint32_t)(buf) * kStageBytes;                               \
            _Pragma("unroll") for (int j = 0; j < kWaveStride / 1024; ++j)                              \
                lds_dma16(s_ + j * LOADERS * 1024, d_ + (uint32_t)(j * LOADERS * 1024));                \
        }                                                                                               \
        if (lw == 0 && lane < kCBytes / 16)                                                             \
            lds_dma16(gC + (int64_t)(t_) * kCBytes, lds_smem + (uint32_t)((buf) * kStageBytes + kTileBytes)); \
    } while (0)

    // ---- prologue: the first two windows of each kind, the first stage
    refill.begin_items(k0);
    int4 dc = win.desc_at(k0);
    uint64_t e = entry_off(dc);
    refill.begin_entries(e);
    SBO_STAGE(dc.x, win.list_at(e, dc.x), 0);
    int64_t q = (int64_t)dc.y * kBN + wave * 16 + r;
    float xq = qx[q < m ? q : m - 1], yq = qy[q < m ? q : m - 1];
    plan_dma_landed();

    OT outer[kRowBlocks][4];
#pragma unroll
    for (int rb = 0; rb < kRowBlocks; ++rb)
#pragma unroll
        for (int c = 0; c < 4; ++c) outer[rb][c] = (OT)0;
    double mu = 0.0;
    f32x4 acc[kRowBlocks];
    int k = k0, j = 0, cur = 0;
    for (;;) {
        const int cnt = plan_item_count(dc.w);
        // the next step: (k, j+1), or the first tile of item k+1
        int kn = k, jn = j + 1;
        if (jn >= cnt) {
            kn = k + 1;
            jn = 0;
        }
        const bool more = kn < k1;
        int4 dn = dc;
        float xqn = xq, yqn = yq;
        if (more) {
            if (kn != k) {
                dn = win.desc_at(kn);
                refill.enter_item(kn);
                const int64_t qn = (int64_t)dn.y * kBN + wave * 16 + r;
                xqn = qx[qn < m ? qn : m - 1];
                yqn = qy[qn < m ? qn : m - 1];
            }
            const uint64_t en = e + 1;
            refill.enter_entry(en);
            SBO_STAGE(dn.x, win.list_at(en, dn.x), cur ^ 1);
        }
        // per-lane bases; every k step is a constant offset from them
        const float4 *pa = reinterpret_cast<const float4 *>(smem + cur * kStageFloats) + g * 16 + r;
        const float *pc = smem + cur * kStageFloats + kTileFloats + g * (kBK / 4);
        const int I = dc.x;
        if (I == nI - 1)
            tile_steps<true>(pa, pc, xq, yq, cexp, acc, mu);
        else
            tile_steps<false>(pa, pc, xq, yq, cexp, acc, mu);
#pragma unroll
        for (int rb = 0; rb < kRowBlocks; ++rb)
#pragma unroll
            for (int c = 0; c < 4; ++c) outer[rb][c] += (OT)acc[rb][c];
        if (j == cnt - 1) {
            // item done: column sums of V^2 over its rows; lanes l, l+16,
            // l+32, l+48 hold four row quarters of column l&15 of every block
            double s = 0.0;
#pragma unroll
            for (int rb = 0; rb < kRowBlocks; ++rb)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    s = fma((double)outer[rb][c], (double)outer[rb][c], s);
                    outer[rb][c] = (OT)0;
                }
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            const bool writer = lane < 16 && q < m;
            if (writer) part[(int64_t)I * ldp + q] = (float)s;
            if (I == nI - 1) {
                mu += __shfl_xor(mu, 16);
                mu += __shfl_xor(mu, 32);
                if (writer) mean[q] = (float)((double)m0 + mu);
                mu = 0.0;
            }
        }
        plan_dma_landed();
        if (!more) break;
        if (kn != k) {
            k = kn;
            dc = dn;
            xq = xqn;
            yq = yqn;
            q = (int64_t)dc.y * kBN + wave * 16 + r;
        }
        j = jn;
        ++e;
        cur ^= 1;
    }
#undef SBO_STAGE
}

// ------------------------------------------------------ a6+a7+a10 acquire
__device__ __forceinline__ bool key_better(double as, int64_t ai, double bs, int64_t bi) {
    if (ai < 0) return false;
    if (bi < 0) return true;
    if (as > bs) return true;
    if (as < bs) return false;
    return ai < bi;
}

__device__ __forceinline__ void block_reduce_key(double &s, int64_t &i, sbo_key *out) {
    __shared__ double ss[kAcqThreads / 64];
    __shared__ int64_t si[kAcqThreads / 64];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double os = __shfl_xor(s, off);
        const int64_t oi = __shfl_xor(i, off);
        if (key_better(os, oi, s, i)) { s = os; i = oi; }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { ss[w] = s; si[w] = i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < (int)(blockDim.x >> 6); ++k)
            if (key_better(ss[k], si[k], s, i)) { s = ss[k]; i = si[k]; }
        out->score = s;
        out->idx = i;
    }
}

// node.cpp:411-416 and :409 in IEEE double, no contraction:
//   confidence = beta * std;  lo = mu - confidence;  hi = mu + confidence;  S = lo > f_min
// T = float (the tick's own f32 outputs, widened exactly) or double (the
// node's f64 mu_/std_, node.cpp:129-130, :641-643)
template <typename T>
__device__ __forceinline__ void compute_sets_one(T mu, T sd, double beta, double f_min,
                                                 double &lo, double &hi, bool &safe) {
    const double c = __dmul_rn(beta, (double)sd);
    lo = __dsub_rn((double)mu, c);
    hi = __dadd_rn((double)mu, c);
    safe = lo > f_min;
}

// One position's acquisition from its variance before the clamp (f64) and its
// mean (f32): the outputs at caller index o and the thread's argmax candidate.
__device__ __forceinline__ void acquire_one(double vd, float mu, int64_t o, double beta, double f_min, int score_kind,
                                            int64_t index_offset, float *__restrict__ mu_out,
                                            float *__restrict__ sd_out, double *__restrict__ lo_out,
                                            double *__restrict__ hi_out, uint8_t *__restrict__ safe_out, double &bs,
                                            int64_t &bi) {
    float var = vd > 0.0 ? (float)vd : 0.0f;
    const float sd = __fsqrt_rn(var);
    if (mu_out) mu_out[o] = mu;
    if (sd_out) sd_out[o] = sd;
    double lo, hi;
    bool safe;
    compute_sets_one(mu, sd, beta, f_min, lo, hi, safe);
    if (lo_out) lo_out[o] = lo;
    if (hi_out) hi_out[o] = hi;
    if (safe_out) safe_out[o] = safe ? 1 : 0;
    const double score = score_kind == SBO_SCORE_UCB ? hi : __dsub_rn(hi, lo);
    if (safe && score == score) { bs = score; bi = index_offset + o; }
}

// The acquisition from a kept posterior (sbo_tick_stream's update path).
__global__ __launch_bounds__(kAcqThreads) void acquire_kept_kernel(
    const double *__restrict__ mu64, const double *__restrict__ var64, int64_t ms, double beta, double f_min,
    int score_kind, int64_t index_offset, const int32_t *__restrict__ perm, float *__restrict__ mu_out,
    float *__restrict__ sd_out, double *__restrict__ lo_out, double *__restrict__ hi_out,
    uint8_t *__restrict__ safe_out, sbo_key *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * kAcqThreads + threadIdx.x;
    double bs = 0.0;
    int64_t bi = -1;
    if (i < ms && perm[i] >= 0)
        acquire_one(var64[i], (float)mu64[i], (int64_t)perm[i], beta, f_min, score_kind, index_offset, mu_out, sd_out,
                    lo_out, hi_out, safe_out, bs, bi);
    block_reduce_key(bs, bi, keys + blockIdx.x);
}

template <class PT>
__global__ __launch_bounds__(kAcqThreads) void acquire_kernel(
    const PT *__restrict__ part, const PT *__restrict__ mean, int nI, int64_t ldp, int64_t m,
    double sf2, double beta, double f_min, int score_kind, int64_t index_offset,
    const int32_t *__restrict__ perm, float *__restrict__ mu_out, float *__restrict__ sd_out,
    double *__restrict__ lo_out, double *__restrict__ hi_out, uint8_t *__restrict__ safe_out,
    sbo_key *__restrict__ keys, const unsigned long long *__restrict__ nemask, double *__restrict__ keep_mu,
    double *__restrict__ keep_var) {
    const int64_t i = (int64_t)blockIdx.x * kAcqThreads + threadIdx.x;
    double bs = 0.0;
    int64_t bi = -1;
    // (perm -1: a padded grid-patch position, no output)
    if (i < m && (!perm || perm[i] >= 0)) {
        // the row blocks' partials, summed in f64 in ascending I; read eight
        // at a time so their loads are in flight together (same sum order).
        // nemask (the plan's non-empty items, bit I of the query block's
        // words; may be null): an empty item's partial is not read -- nobody
        // wrote it, and it would add +0.0 to a sum that is never -0.0
        const unsigned long long *ne = nemask ? nemask + (i / kBN) * (int64_t)((nI + 63) >> 6) : nullptr;
        double s = 0.0;
        int I = 0;
        for (; I + 8 <= nI; I += 8) {
            const unsigned b = ne ? (unsigned)(ne[I >> 6] >> (I & 63)) & 0xffu : 0xffu;   // (I % 8 == 0: one word)
            PT v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = ((b >> u) & 1u) ? part[(int64_t)(I + u) * ldp + i] : (PT)0;
#pragma unroll
            for (int u = 0; u < 8; ++u) s += (double)v[u];
        }
        for (; I < nI; ++I)
            if (!ne || ((ne[I >> 6] >> (I & 63)) & 1ull)) s += (double)part[(int64_t)I * ldp + i];
        const double vd = sf2 - s;
        const PT mean_i = mean[i];
        if (keep_var) keep_var[i] = vd;
        if (keep_mu) keep_mu[i] = (double)mean_i;
        const int64_t o = perm ? (int64_t)perm[i] : i;  // caller's index of sweep position i
        acquire_one(vd, (float)mean_i, o, beta, f_min, score_kind, index_offset, mu_out, sd_out, lo_out, hi_out,
                    safe_out, bs, bi);
    }
    block_reduce_key(bs, bi, keys + blockIdx.x);
}

template <typename T>
__global__ __launch_bounds__(kAcqThreads) void sets_kernel(const T *__restrict__ mu,
                                                           const T *__restrict__ sd, int64_t m,
                                                           double beta, double f_min,
                                                           double *__restrict__ lo,
                                                           double *__restrict__ hi,
                                                           uint8_t *__restrict__ safe) {
    const int64_t i = (int64_t)blockIdx.x * kAcqThreads + threadIdx.x;
    if (i >= m) return;
    double l, h;
    bool s;
    compute_sets_one(mu[i], sd[i], beta, f_min, l, h, s);
    if (lo) lo[i] = l;
    if (hi) hi[i] = h;
    if (safe) safe[i] = s ? 1 : 0;
}

__global__ __launch_bounds__(kAcqThreads) void argmax_kernel(const double *__restrict__ score,
                                                             const uint8_t *__restrict__ mask,
                                                             int64_t m, int64_t index_offset,
                                                             sbo_key *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * kAcqThreads + threadIdx.x;
    double bs = 0.0;
    int64_t bi = -1;
    if (i < m && (!mask || mask[i])) {
        const double v = score[i];
        if (v == v) { bs = v; bi = index_offset + i; }
    }
    block_reduce_key(bs, bi, keys + blockIdx.x);
}

__global__ __launch_bounds__(kAcqThreads) void reduce_keys_kernel(const sbo_key *__restrict__ keys,
                                                                  int64_t nb,
                                                                  sbo_key *__restrict__ out) {
    double bs = 0.0;
    int64_t bi = -1;
    for (int64_t k = threadIdx.x; k < nb; k += kAcqThreads) {
        const sbo_key v = keys[k];
        if (key_better(v.score, v.idx, bs, bi)) { bs = v.score; bi = v.idx; }
    }
    block_reduce_key(bs, bi, out);
}

}  // namespace

// ---------------------------------------------------------------- launchers
hipError_t launch_rbf_fill(hipStream_t s, const float *xa, const float *ya, int64_t ma, const float *xb,
                           const float *yb, int64_t mb, int64_t ld, float ell, float sf2, float sn2, bool diag,
                           float *K) {
    const float c = -1.0f / (2.0f * ell * ell);
    const dim3 grid((unsigned)((ma + 1023) / 1024), (unsigned)((mb + kFillCols - 1) / kFillCols));
    const bool vec = (ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(K) & 15) == 0) &&
                     ((reinterpret_cast<uintptr_t>(xa) & 15) == 0) &&
                     ((reinterpret_cast<uintptr_t>(ya) & 15) == 0);
    if (vec)
        hipLaunchKernelGGL(rbf_fill_kernel<true>, grid, dim3(256), 0, s, xa, ya, ma, xb, yb, mb, ld, c, sf2, sn2,
                           (int)diag, K);
    else
        hipLaunchKernelGGL(rbf_fill_kernel<false>, grid, dim3(256), 0, s, xa, ya, ma, xb, yb, mb, ld, c, sf2, sn2,
                           (int)diag, K);
    return hipGetLastError();
}

hipError_t launch_sub_scalar(hipStream_t s, const float *in, float v, int64_t n, float *out) {
    hipLaunchKernelGGL(sub_scalar_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, v, n, out);
    return hipGetLastError();
}

hipError_t launch_copy_lower(hipStream_t s, const float *src, int64_t ld_src, int64_t n, float *dst,
                             int64_t ld_dst) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(copy_lower_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)std::min<int64_t>(n, kMaxGridY)),
                       dim3(256), 0, s, src, ld_src, n, dst, ld_dst);
    return hipGetLastError();
}

hipError_t launch_widen(hipStream_t s, const float *src, int64_t ld_src, int64_t m, int64_t n, bool lower,
                        double *dst, int64_t ld_dst) {
    if (m <= 0 || n <= 0) return hipSuccess;
    hipLaunchKernelGGL(widen_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)std::min<int64_t>(n, kMaxGridY)),
                       dim3(256), 0, s, src, ld_src, m, n, lower ? 1 : 0, dst, ld_dst);
    return hipGetLastError();
}

hipError_t launch_widen_sub(hipStream_t s, const float *in, double v, int64_t n, double *d) {
    hipLaunchKernelGGL(widen_sub_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, v, n, d);
    return hipGetLastError();
}

hipError_t launch_narrow(hipStream_t s, const double *d, int64_t n, float *out) {
    hipLaunchKernelGGL(narrow_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, n, out);
    return hipGetLastError();
}

size_t alpha_work_bytes(int64_t n) { return sizeof(double) * (size_t)((n + kAlK - 1) / kAlK) * (size_t)n; }

hipError_t launch_alpha_f64(hipStream_t s, const double *X, int64_t ld, int64_t n, const float *obs, double m0,
                            double *z, double *alpha, double *work) {
    if (n <= 0) return hipSuccess;
    const dim3 g1((unsigned)((n + kAlRows - 1) / kAlRows), (unsigned)((n + kAlK - 1) / kAlK));
    hipLaunchKernelGGL(alpha_z_kernel, g1, dim3(256), 0, s, X, ld, n, obs, m0, work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(alpha_z_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, work, n, z);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(alpha_xtz_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, X, ld, n, z, alpha);
    return hipGetLastError();
}

hipError_t launch_row_dot(hipStream_t s, const double *A, int64_t ld, int64_t rows, int64_t n, const double *x,
                          double *out) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(row_dot_kernel, dim3((unsigned)rows), dim3(256), 0, s, A, ld, n, x, out);
    return hipGetLastError();
}

hipError_t launch_narrow_2d(hipStream_t s, const double *d, int64_t ldd, int64_t m, int64_t n, float *out,
                            int64_t ldo) {
    if (m <= 0 || n <= 0) return hipSuccess;
    hipLaunchKernelGGL(narrow_2d_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)std::min<int64_t>(n, kMaxGridY)),
                       dim3(256), 0, s, d, ldd, m, n, out, ldo);
    return hipGetLastError();
}

hipError_t launch_narrow_strided(hipStream_t s, const double *d, int64_t n, float *out, int64_t stride) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(narrow_strided_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, n, out, stride);
    return hipGetLastError();
}

namespace {
struct PlanLayout {
    size_t key, scan, thr, desc, tl, seg, temp, temp_bytes, wkey, wscan, lvcnt, rec, bits, nemask;
    // XCD-interleaved order (P % 8 == 0): the sweep reads desc2 / tl2 / seg2
    bool xcd;
    size_t xseg, pos_of, cnt2, off2, desc2, tl2, seg2, temp2, temp2_bytes;
    size_t total;
};

bool xcd_interleave(int P) { return P >= 8 && P % 8 == 0; }

PlanLayout plan_layout(int64_t nI, int64_t nQ, int P) {
    const int64_t items = nI * nQ;
    const int64_t cap = 2 * nI * (nI + 1) * nQ;  // every tile of every item (the dense sweep)
    PlanLayout L{};
    size_t o = 0;
    auto take = [&](size_t b) {
        const size_t at = o;
        o = (o + b + 255) / 256 * 256;
        return at;
    };
    L.key = take(8 * (size_t)items);
    L.scan = take(8 * (size_t)items);
    L.thr = take((size_t)items);
    L.wkey = take(8 * (size_t)items);
    L.wscan = take(8 * (size_t)items);
    L.nemask = take(8 * (size_t)nQ * (size_t)((nI + 63) / 64));
    L.lvcnt = take(8 * 3 * 4 * (size_t)kPlanWriteBlocks);
    L.bits = take(8 * 3 * (size_t)items * (size_t)plan_chunks((int)nI));
    L.desc = take(16 * (size_t)plan_desc_slots(items));
    L.tl = take(2 * (size_t)plan_list_slots(cap));
    L.seg = take(4 * (size_t)(P + 1));
    L.rec = take(16 * (size_t)plan_rec_slots(cap));
    size_t tb = 0;
    (void)rocprim::inclusive_scan(nullptr, tb, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                  (size_t)items, rocprim::plus<unsigned long long>());
    L.temp = take(tb);
    L.temp_bytes = tb;
    L.xcd = xcd_interleave(P);
    if (L.xcd) {
        L.xseg = take(4 * 9);
        L.pos_of = take(4 * (size_t)items);
        L.cnt2 = take(8 * (size_t)items);
        L.off2 = take(8 * (size_t)items);
        L.desc2 = take(16 * (size_t)plan_desc_slots(items));
        L.tl2 = take(2 * (size_t)plan_list_slots(cap));
        L.seg2 = take(4 * (size_t)(P + 1));
        size_t t2 = 0;
        (void)rocprim::exclusive_scan(nullptr, t2, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                      0ull, (size_t)items, rocprim::plus<unsigned long long>());
        L.temp2 = take(t2);
        L.temp2_bytes = t2;
    }
    L.total = o;
    return L;
}

// k-tiles farther than this squared distance give c*d^2 < -L, i.e. every K*
// entry < 2^-L (0.1% margin over the kernel's rounding); L >= 150 means every
// such entry is exactly +0.0 in f32
float cutoff_d2(int L, double ce) { return L > 0 ? (float)((double)L / -ce * 1.001) : -1.0f; }
double exp2_coef(float ell) { return -1.0 / (2.0 * (double)ell * (double)ell * 0.69314718055994530942); }
}  // namespace

size_t predict_work_bytes(int64_t npad, int64_t m, int P) {
    return plan_layout(npad / kBM, (m + kBN - 1) / kBN, P).total;
}

hipError_t launch_plan(hipStream_t s, const float4 *kbox, int64_t npad, const float *qx, const float *qy, int64_t m,
                       int64_t ldp, float ell, float m0, const SkipPlan &skip, float *part, float *mean,
                       unsigned long long *tiles_done, int P, void *work, size_t work_bytes) {
    const int nI = (int)(npad / kBM);
    const int64_t nQ = (m + kBN - 1) / kBN;
    const int64_t items = (int64_t)nI * nQ;
    if (m <= 0 || nI <= 0) return hipSuccess;
    if (!plan_fits(nQ, items, 2 * (int64_t)nI * (nI + 1) * nQ, kTilesPerRowBlockStep * (int64_t)nI))
        return hipErrorInvalidValue;
    const PlanLayout L = plan_layout(nI, nQ, P);
    if (work_bytes < L.total) return hipErrorInvalidValue;
    if (skip.order_blk != 0 && ((skip.order_blk >> 8) < 1 || (skip.order_blk & 255) < 1 || (skip.order_blk >> 16) != 0))
        return hipErrorInvalidValue;
    char *w = static_cast<char *>(work);
    auto *key = reinterpret_cast<unsigned long long *>(w + L.key);
    auto *scan = reinterpret_cast<unsigned long long *>(w + L.scan);
    auto *thr = reinterpret_cast<unsigned char *>(w + L.thr);
    auto *desc = reinterpret_cast<int4 *>(w + L.desc);
    auto *tl = reinterpret_cast<unsigned short *>(w + L.tl);
    auto *seg = reinterpret_cast<int *>(w + L.seg);
    auto *wkey = reinterpret_cast<unsigned long long *>(w + L.wkey);
    auto *wscan = reinterpret_cast<unsigned long long *>(w + L.wscan);
#ifdef SBO_DIAG
    if (const char *ev = getenv("SBO_MEAN_W")) {
        unsigned v[3] = {kMeanWeight0, kMeanWeight1, kMeanWeight2};
        if (sscanf(ev, "%u,%u,%u", &v[0], &v[1], &v[2]) == 3)
            (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_mean_w), v, sizeof(v), 0, hipMemcpyHostToDevice, s);
    }
    if (const char *ev = getenv("SBO_RB_SLOPE")) {
        const unsigned v = (unsigned)std::max(0, atoi(ev));
        (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_rb_slope), &v, sizeof(v), 0, hipMemcpyHostToDevice, s);
    }
#endif
    const double ce = exp2_coef(ell);
    const float cexp = (float)ce;
    const float skip_d2 = cutoff_d2(skip.L, ce);
    const float skip_d2_mean = skip.L > 0 && skip.L_mean > skip.L ? cutoff_d2(skip.L_mean, ce) : skip_d2;
    const float4 *lgn = skip.L > 0 ? skip.lgn : nullptr;
    const int levels = lgn ? skip.levels : 0;
    auto *bits = reinterpret_cast<unsigned long long *>(w + L.bits);
    const int nc = std::min(kTilesPerRowBlockStep * nI, kPlanD2);
    const size_t plan_lds = 4 * (size_t)kPlanWaves * kPlanBinCache + 8 * (size_t)nc + 2 * (size_t)nc;
    hipLaunchKernelGGL(plan_count_kernel, dim3((unsigned)nQ), dim3(kPlanThreads), plan_lds, s, kbox, skip.kcoord, lgn,
                       levels, make_float2(skip.lvl_key[0], skip.lvl_key[1]), nI,
                       nQ, qx, qy,
                       m, cexp, skip_d2, skip_d2_mean, skip.lg_tau_v, m0, ldp, part, mean, key, thr, wkey, bits,
                       skip.wide ? 1 : 0, skip.order_blk, lgn ? skip.colmax : nullptr, skip.zero_empty ? 1 : 0,
                       reinterpret_cast<unsigned long long *>(w + L.nemask));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
#ifdef SBO_DIAG
    if (getenv("SBO_PLAN_STATS")) {  // the column prefilter's near fraction of this plan, to stderr
        unsigned long long h[9] = {}, z[9] = {};
        (void)hipStreamSynchronize(s);
        (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_plan_near), sizeof(h));
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_plan_near), z, sizeof(z));
        fprintf(stderr, "plan stats: near (qb, t) pairs %llu of %llu; clock setup %llu near %llu totals %llu fill %llu "
                        "thresholds %llu levels %llu rest %llu\n", h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8]);
    }
#endif
    size_t tb = L.temp_bytes;
    e = rocprim::inclusive_scan(w + L.temp, tb, key, scan, (size_t)items, rocprim::plus<unsigned long long>(), s);
    if (e != hipSuccess) return e;
    tb = L.temp_bytes;
    e = rocprim::inclusive_scan(w + L.temp, tb, wkey, wscan, (size_t)items, rocprim::plus<unsigned long long>(), s);
    if (e != hipSuccess) return e;
    const int64_t wblocks = std::min<int64_t>((items + 3) / 4, kPlanWriteBlocks);
    hipLaunchKernelGGL(plan_write_kernel, dim3((unsigned)wblocks), dim3(256), 0, s, nI, nQ, key, scan, bits,
                       desc, tl, skip.prod_full, tiles_done ? reinterpret_cast<unsigned long long *>(w + L.lvcnt) : nullptr,
                       skip.order_blk);
    if (tiles_done)
        hipLaunchKernelGGL(plan_counts_reduce_kernel, dim3(1), dim3(256), 0, s,
                           reinterpret_cast<const unsigned long long *>(w + L.lvcnt), wblocks * 4, tiles_done + 1);
    auto *rec = reinterpret_cast<int4 *>(w + L.rec);
    if (!L.xcd) {
        hipLaunchKernelGGL(plan_seg_kernel, dim3(1), dim3(256), 0, s, scan, items, desc, P, seg, tiles_done, wkey,
                           wscan, nI, nQ, skip.order_blk);
        if (skip.records)
            hipLaunchKernelGGL(plan_rec_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, scan, items, desc,
                               tl, rec);
        return hipGetLastError();
    }
    auto *xseg = reinterpret_cast<int *>(w + L.xseg);
    auto *pos_of = reinterpret_cast<int *>(w + L.pos_of);
    auto *cnt2 = reinterpret_cast<unsigned long long *>(w + L.cnt2);
    auto *off2 = reinterpret_cast<unsigned long long *>(w + L.off2);
    auto *desc2 = reinterpret_cast<int4 *>(w + L.desc2);
    auto *tl2 = reinterpret_cast<unsigned short *>(w + L.tl2);
    auto *seg2 = reinterpret_cast<int *>(w + L.seg2);
    const int G = P / 8;
    // (positions past the last non-empty item count 0 for the scan: plan_perm writes them)
    if (skip.ref_chain) {  // (the diagnostic build's reference chain clears them as before)
        e = hipMemsetAsync(cnt2, 0, 8 * (size_t)items, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(plan_seg_kernel, dim3(1), dim3(256), 0, s, scan, items, desc, 8, xseg, tiles_done, wkey, wscan,
                       nI, nQ, skip.order_blk);
    hipLaunchKernelGGL(plan_perm_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, scan, items, desc,
                       xseg, G, pos_of, cnt2);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t t2 = L.temp2_bytes;
    e = rocprim::exclusive_scan(w + L.temp2, t2, cnt2, off2, 0ull, (size_t)items,
                                rocprim::plus<unsigned long long>(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(plan_move_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, scan, items, desc, tl,
                       pos_of, off2, desc2, tl2, skip.records ? rec : nullptr);
    hipLaunchKernelGGL(plan_seg2_kernel, dim3(1), dim3(256), 0, s, xseg, G, P, seg2);
    return hipGetLastError();
}

void plan_views(int64_t npad, int64_t m, int P, const void *work, const int4 **desc, const unsigned short **tl,
                const int **seg, const int4 **rec) {
    const PlanLayout L = plan_layout(npad / kBM, (m + kBN - 1) / kBN, P);
    const char *w = static_cast<const char *>(work);
    *desc = reinterpret_cast<const int4 *>(w + (L.xcd ? L.desc2 : L.desc));
    *tl = reinterpret_cast<const unsigned short *>(w + (L.xcd ? L.tl2 : L.tl));
    *seg = reinterpret_cast<const int *>(w + (L.xcd ? L.seg2 : L.seg));
    if (rec) *rec = reinterpret_cast<const int4 *>(w + L.rec);
}

void plan_item_views(int64_t npad, int64_t m, int P, const void *work, const unsigned long long **key,
                     const unsigned long long **scan, const unsigned char **thr, const unsigned long long **nonempty) {
    const PlanLayout L = plan_layout(npad / kBM, (m + kBN - 1) / kBN, P);
    const char *w = static_cast<const char *>(work);
    *key = reinterpret_cast<const unsigned long long *>(w + L.key);
    *scan = reinterpret_cast<const unsigned long long *>(w + L.scan);
    *thr = reinterpret_cast<const unsigned char *>(w + L.thr);
    if (nonempty) *nonempty = reinterpret_cast<const unsigned long long *>(w + L.nemask);
}

float exp2_coef_f(float ell) { return (float)exp2_coef(ell); }

hipError_t launch_plan_cost(hipStream_t s, int64_t npad, int64_t m, int P, const void *work, const int32_t *perm,
                            float *bcost, float *cost) {
    const int nI = (int)(npad / kBM);
    const int64_t nQ = (m + kBN - 1) / kBN;
    if (m <= 0 || nI <= 0) return hipSuccess;
    const PlanLayout L = plan_layout(nI, nQ, P);
    const auto *wkey = reinterpret_cast<const unsigned long long *>(static_cast<const char *>(work) + L.wkey);
    hipLaunchKernelGGL(plan_block_cost_kernel, dim3((unsigned)((nQ + 255) / 256)), dim3(256), 0, s, wkey, nI, nQ,
                       bcost);
    hipLaunchKernelGGL(plan_query_cost_kernel, dim3((unsigned)nQ), dim3(kBN), 0, s, bcost, m, perm, cost);
    return hipGetLastError();
}

hipError_t launch_predict(hipStream_t s, const float *aug, const float *kcoord, int64_t npad, const float *qx,
                          const float *qy, int64_t m, int64_t ldp, float ell, float m0, float *part, float *mean,
                          int variant, int P, const void *work) {
    const int nI = (int)(npad / kBM);
    const int64_t nQ = (m + kBN - 1) / kBN;
    if (m <= 0 || nI <= 0) return hipSuccess;
    const int4 *desc = nullptr;
    const unsigned short *tl = nullptr;
    const int *seg = nullptr;
    plan_views(npad, m, P, work, &desc, &tl, &seg);
    const float cexp = (float)exp2_coef(ell);
#define SBO_PREDICT_ARGS aug, kcoord, desc, tl, seg, P, (int)(nI * nQ), nI, qx, qy, m, ldp, cexp, m0, part, mean
    switch (variant) {
        case 1: hipLaunchKernelGGL((predict_kernel<double>), dim3((unsigned)P), dim3(kPredictThreads), 0, s, SBO_PREDICT_ARGS); break;
        default: hipLaunchKernelGGL((predict_kernel<float>), dim3((unsigned)P), dim3(kPredictThreads), 0, s, SBO_PREDICT_ARGS); break;
    }
#undef SBO_PREDICT_ARGS
    return hipGetLastError();
}

hipError_t launch_acquire(hipStream_t s, const float *part, const float *mean, int nI, int64_t ldp,
                          int64_t m, float sf2, double beta, double f_min, int score_kind,
                          int64_t index_offset, const int32_t *perm, float *mu, float *sd, double *lo,
                          double *hi, uint8_t *safe, sbo_key *block_keys, const unsigned long long *nonempty,
                          double *keep_mu, double *keep_var) {
    hipLaunchKernelGGL(acquire_kernel<float>, dim3((unsigned)acq_blocks(m)), dim3(kAcqThreads), 0, s, part, mean,
                       nI, ldp, m, (double)sf2, beta, f_min, score_kind, index_offset, perm, mu, sd, lo, hi, safe,
                       block_keys, nonempty, keep_mu, keep_var);
    return hipGetLastError();
}

hipError_t launch_acquire(hipStream_t s, const double *part, const double *mean, int nI, int64_t ldp,
                          int64_t m, double sf2, double beta, double f_min, int score_kind,
                          int64_t index_offset, const int32_t *perm, float *mu, float *sd, double *lo,
                          double *hi, uint8_t *safe, sbo_key *block_keys, const unsigned long long *nonempty,
                          double *keep_mu, double *keep_var) {
    hipLaunchKernelGGL(acquire_kernel<double>, dim3((unsigned)acq_blocks(m)), dim3(kAcqThreads), 0, s, part, mean,
                       nI, ldp, m, sf2, beta, f_min, score_kind, index_offset, perm, mu, sd, lo, hi, safe,
                       block_keys, nonempty, keep_mu, keep_var);
    return hipGetLastError();
}

hipError_t launch_acquire_kept(hipStream_t s, const double *mu64, const double *var64, int64_t ms, double beta,
                               double f_min, int score_kind, int64_t index_offset, const int32_t *perm, float *mu,
                               float *sd, double *lo, double *hi, uint8_t *safe, sbo_key *block_keys) {
    hipLaunchKernelGGL(acquire_kept_kernel, dim3((unsigned)acq_blocks(ms)), dim3(kAcqThreads), 0, s, mu64, var64, ms,
                       beta, f_min, score_kind, index_offset, perm, mu, sd, lo, hi, safe, block_keys);
    return hipGetLastError();
}

hipError_t launch_sets(hipStream_t s, const float *mu, const float *sd, int64_t m, double beta,
                       double f_min, double *lo, double *hi, uint8_t *safe) {
    hipLaunchKernelGGL(sets_kernel<float>, dim3((unsigned)acq_blocks(m)), dim3(kAcqThreads), 0, s, mu, sd, m, beta,
                       f_min, lo, hi, safe);
    return hipGetLastError();
}

hipError_t launch_sets(hipStream_t s, const double *mu, const double *sd, int64_t m, double beta,
                       double f_min, double *lo, double *hi, uint8_t *safe) {
    hipLaunchKernelGGL(sets_kernel<double>, dim3((unsigned)acq_blocks(m)), dim3(kAcqThreads), 0, s, mu, sd, m,
                       beta, f_min, lo, hi, safe);
    return hipGetLastError();
}

hipError_t launch_argmax_blocks(hipStream_t s, const double *score, const uint8_t *mask, int64_t m,
                                int64_t index_offset, sbo_key *block_keys) {
    hipLaunchKernelGGL(argmax_kernel, dim3((unsigned)acq_blocks(m)), dim3(kAcqThreads), 0, s, score, mask,
                       m, index_offset, block_keys);
    return hipGetLastError();
}

hipError_t launch_reduce_keys(hipStream_t s, const sbo_key *keys, int64_t nblocks, sbo_key *out) {
    hipLaunchKernelGGL(reduce_keys_kernel, dim3(1), dim3(kAcqThreads), 0, s, keys, nblocks, out);
    return hipGetLastError();
}

}  // namespace sbo
