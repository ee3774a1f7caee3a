// kstar_walk.hpp -- the k-tile walk of the two sweeps over a kept posterior:
// predict_update_kernel (predict_update.hip) and whatif_kernel (whatif.hip).
// Device only; included by those two files.
//
// One workgroup per 128-position query block of the kept order, eight waves,
// wave w owns positions 16 w .. 16 w + 15.  A pass walks the 64-column k-tiles
// in ascending order and skips a tile when the block's box and the tile's box
// put every K* entry below 2^-L.  Kept tiles evaluate K* = sf2 exp2(cexp d^2)
// in f64 from the f32 coordinates, one entry per lane in the MFMA B-fragment
// map (k = l >> 4, q = l & 15), and multiply it by NJ blocks of sixteen rows
// of the left operand on v_mfma_f64_16x16x4_f64.  The left operand is
// column-major, so the sixteen rows of a column are one 128-byte segment and
// a lane's A operand is one 8-byte load of it.  Entries below 2^-150 are exact
// zeros in every mode, so a cutoff of L >= 150 drops only zeros.
#pragma once

#include <cstdint>

#include "sbo_internal.hpp"

namespace sbo {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kWalkThreads = 64 * (kBN / 16);   // eight waves of sixteen positions
constexpr double kKstarZero = -150.0;           // K* exponents below it: the entry is +0.0

// C/D map of v_mfma_f64_16x16x4_f64: register c of lane l is row (l >> 4) + 4 c,
// column l & 15.
__device__ __forceinline__ f64x4 mfma_f64(double a, double b, f64x4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// squared distance of two boxes (x0, x1, y0, y1); an empty k-tile box
// (+inf, -inf, ..) is infinitely far
__device__ __forceinline__ float box_d2(float4 k, float4 q) {
    const float dx = fmaxf(0.0f, fmaxf(k.x - q.y, q.x - k.y));
    const float dy = fmaxf(0.0f, fmaxf(k.z - q.w, q.z - k.w));
    return dx * dx + dy * dy;
}

__device__ __forceinline__ double rbf64(double ax, double ay, double bx, double by, double cexp, double sf2) {
    const double dx = ax - bx, dy = ay - by;
    const double a = cexp * fma(dy, dy, dx * dx);
    return a < kKstarZero ? 0.0 : sf2 * exp2(a);
}

// K* = sf2 exp2(cexp d^2): cexp = -1 / (2 ell^2 ln 2), from the f64 length scale.
inline double exp2_coef64(double ell) { return -1.0 / (2.0 * ell * ell * 0.69314718055994530942); }

// The left operand of a walk: `rows` rows from `base`, column-major at leading
// dimension `ld`; rows past the last read as zero.
struct WalkRows {
    const double *__restrict__ base;
    int64_t ld, rows;
};

// One pass: acc[j] += A[16 (rb0 + j) .. + 16, 0:n] K*[0:n, the wave's positions]
// for j < NJ, over the kept tiles ascending, their sixteen steps ascending, j
// ascending.  (r, g) = (lane & 15, lane >> 4), (xq, yq) the lane's query, qb
// the block's box.  The first pass (rb0 == 0) adds the tiles it kept to `kept`
// (the same in every lane of the workgroup).
//
// The kernel zeroes acc before the call and the count goes through `kept`
// rather than a return value: with the zeroing in here, or with the count
// returned and selected on rb0 by the caller, the NJ = 8 what-if sweep takes
// 191 VGPRs instead of 145 and loses a wave per SIMD (ROCm 7.2 hipcc, gfx950).
template <int NJ>
__device__ __forceinline__ void kstar_walk(WalkRows A, int rb0, int r, int g, double xq, double yq,
                                           const float *__restrict__ x, const float *__restrict__ y,
                                           const float4 *__restrict__ kbox, float4 qb, int64_t n, double cexp,
                                           double sf2, float skip_L, f64x4 (&acc)[NJ], int &kept) {
    const float cexp_f = (float)cexp;
    const int ntiles = (int)((n + kBK - 1) / kBK);
    for (int t = 0; t < ntiles; ++t) {
        // (the same decision in every lane of the workgroup)
        if (skip_L > 0.0f && cexp_f * box_d2(kbox[t], qb) * 0.999f < -skip_L) continue;
        if (rb0 == 0) ++kept;
        for (int s = 0; s < kBK / 4; ++s) {
            const int64_t k = (int64_t)t * kBK + 4 * s + g;
            const bool kin = k < n;
            const double e = kin ? rbf64((double)x[k], (double)y[k], xq, yq, cexp, sf2) : 0.0;
            double a[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int64_t row = (int64_t)(rb0 + j) * 16 + r;
                a[j] = (kin && row < A.rows) ? A.base[row + k * A.ld] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = mfma_f64(a[j], e, acc[j]);
        }
    }
}

// NJ of a sweep over nrb blocks of sixteen rows: the smallest of 1, 2, 4, 8
// that takes them in one pass, else 8 and further passes.  LAUNCH(NJ) is the
// caller's launch of its kernel<NJ>.
#define SBO_WALK_DISPATCH(nrb, LAUNCH) \
    do {                               \
        if ((nrb) <= 1) LAUNCH(1);     \
        else if ((nrb) <= 2) LAUNCH(2); \
        else if ((nrb) <= 4) LAUNCH(4); \
        else LAUNCH(8);                \
    } while (0)

}  // namespace
}  // namespace sbo
