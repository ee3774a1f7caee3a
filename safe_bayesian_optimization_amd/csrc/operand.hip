// operand.hip -- the fit-side operand build: what a refresh derives from L^-1
// and the training points for the sweeps and the tick plan to read.
//
//   product                                   kernel               read by
//   aug     A = sf2 L^-1 as packed f32        pack_operand_kernel  the f32 sweep (kernels.hip), the split
//           [BK][BM] tiles, lower triangle    (f32 inverse) or     operand's pack (predict_x3.hip), the
//           (tile_start / tile_offset)        tile_norm_kernel     row sums and the tile norms below
//                                             <true> (f64 inverse)
//   kcoord  per k-tile x, y, sf2 alpha        pack_kcoord_kernel   the f32 sweep, the plan's |k|_2 bound,
//                                                                  the split sweep's coordinate pack
//   row_l1  |A_r|_1 per row (f64)             row_l1_kernel        the host's skip budget (sbo_api.cpp)
//   lgn     per tile log2 gain bounds of A    tile_norm_kernel     the plan builder (kernels.hip), the
//           and of its bf16 pieces A1, A2                          column prefilter, sbo_get_tile_bounds
//   kbox    per k-tile box of the points      tile_box_kernel      the plan builder
//   colmax  per k-tile max of lgn[..].x       tile_colmax_kernel   the plan builder's column prefilter
//
// The tiles, row sums and tile bounds are per row block and are built for the
// row blocks I >= I0 only: an append or a removal leaves the rows of earlier
// blocks, and so their products, as they were.  The coordinates, boxes and the
// prefilter are per k-tile (every row block's columns) and are built whole.
//
// (-ffp-contract=off: every fused multiply-add below is explicit.)
#include <cstdint>
#include <type_traits>

#include "bf16_split.hpp"
#include "sbo_internal.hpp"

namespace sbo {
namespace {

// ------------------------------------------------------------ operand pack
// The f32 inverse's pack (SBO_OPT_INVERSE_BITS 32; the f64 inverse is packed
// by tile_norm_kernel<true>).  grid.x = k-tiles of the longest row block,
// grid.y = row block I.
__global__ __launch_bounds__(256) void pack_operand_kernel(const float *__restrict__ Linv, int64_t ld, int64_t n,
                                                           float sf2, int64_t I0, float *__restrict__ aug) {
    const int64_t I = I0 + blockIdx.y;
    const int64_t kb = blockIdx.x;
    if (kb >= (I + 1) * kTilesPerRowBlockStep) return;
    float *tile = aug + (tile_start(I) + kb) * kTileFloats;
    // (unrolled: 16 independent loads in flight per thread -- the kernel is a pure stream)
#pragma unroll 16
    for (int e = threadIdx.x; e < kTileFloats; e += 256) {
        // inverse of tile_offset: e = ((jj*BK + k)*16 + r)*4 + j3, row = 64 jj + 16 j3 + r
        const int j3 = e & 3, r16 = (e >> 2) & 15, k = (e >> 6) & (kBK - 1), jj = e >> 12;
        const int r = jj * 64 + j3 * 16 + r16;
        const int64_t row = I * kBM + r, col = kb * kBK + k;
        float v = 0.0f;
        if (row < n && col < n && col <= row) v = (float)(sf2 * Linv[row + col * ld]);
        tile[e] = v;
    }
}

// Per k-tile coordinates, step-major per lane group: k = 4p + g is stored at
// g*16 + p (x, then y, then sf2*alpha), so lane group g reads the values of
// consecutive k steps p, p+1 as one 8-byte pair.
__device__ __forceinline__ int kcoord_slot(int o) { return (o & 3) * 16 + (o >> 2); }

__global__ void pack_kcoord_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                   const float *__restrict__ alpha, int64_t n, int64_t npad,
                                   float sf2, float *__restrict__ kcoord) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= npad) return;
    const int64_t t = k / kBK;
    const int o = kcoord_slot((int)(k % kBK));
    float *c = kcoord + t * (3 * kBK);
    const bool in = k < n;
    c[o] = in ? x[k] : x[0];
    c[kBK + o] = in ? y[k] : y[0];
    c[2 * kBK + o] = in ? sf2 * alpha[k] : 0.0f;
}

// Row 1-norms of the packed operand, |A[I*BM + r][:]|_1: block (c, I)
// sums row r over k-tiles [c*kRowL1Tiles, (c+1)*kRowL1Tiles) of row block I
// and adds into row_l1 (zeroed by the launcher).
constexpr int kRowL1Tiles = 4;
__global__ __launch_bounds__(kBM) void row_l1_kernel(const float *__restrict__ aug, int64_t I0,
                                                     double *__restrict__ row_l1) {
    const int64_t I = I0 + blockIdx.y;
    const int64_t kb0 = (int64_t)blockIdx.x * kRowL1Tiles;
    const int64_t nkb = (I + 1) * kTilesPerRowBlockStep;
    if (kb0 >= nkb) return;
    const int r = threadIdx.x;
    const float *t = aug + (tile_start(I) + kb0) * kTileFloats;
    double s = 0.0;
    for (int64_t kb = 0; kb < kRowL1Tiles && kb0 + kb < nkb; ++kb)
        for (int k = 0; k < kBK; ++k) s += fabs((double)t[kb * kTileFloats + tile_offset(k, r)]);
    atomicAdd(row_l1 + I * kBM + r, s);
}

// --------------------------------------------------------------- tile norms
// Per packed tile A_It (256 rows x 64 k), gain bounds as log2 rounded up, two
// float4 per tile; -1000 stands for an all-zero matrix.
//   lgn[2T]   .x  log2(16 max_r |A_r|_1):  |A k|_2 <= sqrt(256) |A k|_inf <= 16 max_r |A_r|_1 max|k|
//             .y  log2 of a bound on the spectral norm:  |A k|_2 <= ||A||_2 |k|_2
//             .z  log2 |A|_F, which also bounds || |A| ||_2
//   lgn[2T+1] .x, .y the first two for the bf16 piece A1, .z, .w for A2, of
//             the split A = A0 + A1 + A2 the split sweep multiplies
//             (bf16_split.hpp).  The products a tile's lower precision levels
//             leave out are A2 K0 + A1 K1 + A0 K2 (three products) and also
//             A1 K0 + A0 K1 (one product); the plan bounds them plane by plane.
// The plan pairs the row-sum bounds with the largest K* of the tile and the
// spectral ones with a bound on |k|_2 from the tile's points.
//
// One workgroup of four waves per tile.  FUSED: the tile is first packed here
// from the f64 inverse, (float)(sf2 L^-1) written to aug -- the f64 path's
// only pack, so that the pack and the norms are one pass over L^-1.
//
// The chain of bounds for a plane P (A, A1, A2), in the kernel's order; each
// phase below carries its part of the argument:
//   1-2  the pieces of every entry, cut as the sweep cuts them, each piece
//        scaled by a power of two so that nothing below underflows in f32;
//   3-4  row sums and |P|_F^2 in f64 from the pieces, and the 64 x 64 Gram
//        matrix G_c of P on the bf16 matrix cores, ||G_c - G||_2 <= delta |P|_F^2;
//   5    ||P||_2^2 = lambda_max(G) <= lambda_max(G_c) + delta |P|_F^2 (Weyl; at
//        most 64 delta = 1e-3 relative, since ||P||_2^2 >= |P|_F^2 / 64), and
//        lambda_max(G_c) <= ||G_c^16||_inf^(1/16) (any induced norm bounds the
//        spectral radius; at most 64^(1/32) = 1.14 x over for a 64 x 64 G_c)
//        by four squarings with an error term each; the bound is the smaller
//        of that and |P|_F.
constexpr int kTnGmLd = kBK + 4;               // LDS row stride (floats) of the powers of G: the row-sum pass's
                                               // 16-B reads and the mirrored stores on distinct banks
constexpr int kTnPq = kBK + 8;                 // bf16 per staged k row: 144 B, conflict-free b128 reads
constexpr double kTnDelta = 1.0 / 65536.0;     // 2^-16
constexpr int kGramSquarings = 4;
constexpr double kSqEta = 64.0 / 32768.0;      // 64 eps, eps = 2^-15 (the squarings)
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned short TnPlanes[3][kBK * kTnPq];   // the three pieces of a 64 x 64 block, [piece][k][c]
template <bool FUSED> using TilePtr = std::conditional_t<FUSED, float *, const float *>;

__device__ __forceinline__ f32x4_t mfma_bf16(uint4 a, uint4 b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b),
                                                   c, 0, 0, 0);
}

// Four-wave block reductions, fixed order (deterministic): a wave's value by
// a butterfly, lane 0 puts it into the wave's slot, and after the caller's
// barrier every thread combines the four slots.
template <class T> __device__ __forceinline__ T wave_max(T v) {   // (float or double: fmax's overloads)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <class T> __device__ __forceinline__ void wave_put(T (&slot)[4], T v) {
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
}
template <class T> __device__ __forceinline__ T slots_max(const T (&s)[4]) {
    return fmax(fmax(s[0], s[1]), fmax(s[2], s[3]));
}
__device__ __forceinline__ double slots_sum(const double (&s)[4]) { return ((s[0] + s[1]) + s[2]) + s[3]; }
// put, barrier, combine: every thread gets the block's maximum
__device__ __forceinline__ double block_max(double (&slot)[4], double wave_value) {
    wave_put(slot, wave_value);
    __syncthreads();
    return slots_max(slot);
}

// The ten lower 16 x 16 blocks (bi >= bj) of a symmetric 64 x 64 product, two or three per wave:
//        bj 0   1   2   3
//   bi 0    w0
//      1    w0  w0
//      2    w1  w1  w1
//      3    w2  w2  w3  w3
struct WaveBlocks { int nb, bi[3], bj[3]; };
__device__ __forceinline__ WaveBlocks wave_blocks(int wave) {
    return {wave < 2 ? 3 : 2,
            {wave < 2 ? 2 * wave : 3, wave < 2 ? 2 * wave + (wave == 0 ? 1 : 0) : 3, wave == 0 ? 1 : 2},
            {wave < 3 ? 0 : 2, wave == 0 ? 0 : (wave == 1 ? 1 : (wave == 2 ? 1 : 3)), wave == 0 ? 1 : 2}};
}

// 16 consecutive floats (16-B aligned)
__device__ __forceinline__ void load_row16(const float *p, float (&v)[16]) {
    const float4 *src = reinterpret_cast<const float4 *>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 f = src[j];
        v[4 * j] = f.x, v[4 * j + 1] = f.y, v[4 * j + 2] = f.z, v[4 * j + 3] = f.w;
    }
}

// FUSED: the row block and k-tile of a packed tile, tile = tile_start(I) + kb
__device__ __forceinline__ void tile_decode(int64_t tile, int64_t &I, int64_t &kb) {
    I = (int64_t)((sqrt(1.0 + 2.0 * (double)tile) - 1.0) * 0.5);
    while (I > 0 && tile_start(I) > tile) --I;
    while (tile_start(I + 1) <= tile) ++I;
    kb = tile - tile_start(I);
}
// FUSED: the thread's 16 floats of quarter q of tile (I, kb) from the f64
// inverse, stored to the tile.  Element 16 tid + j of the quarter
// (tile_offset): k = tid / 4, row 64 q + 16 (j & 3) + 4 (tid & 3) + j / 4.
__device__ __forceinline__ void pack_row16(const double *__restrict__ Linv, int64_t ld, int64_t n, double sf2,
                                           int64_t I, int64_t kb, int q, int tid, float *dst16, float (&v)[16]) {
    const int64_t col = kb * kBK + (tid >> 2);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int64_t row = I * kBM + 64 * q + 16 * (j & 3) + 4 * (tid & 3) + (j >> 2);
        v[j] = (row < n && col < n && col <= row) ? (float)(sf2 * Linv[row + col * ld]) : 0.0f;
    }
    float4 *dst = reinterpret_cast<float4 *>(dst16);
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
}

// Split 16 values, scale piece p by up[p] (a power of two: exact), and store
// them as columns sc .. sc + 15 of row sk of the three planes: two 16-B
// stores per plane.
__device__ __forceinline__ void stage_row16(TnPlanes &pq, int sk, int sc, const float (&v)[16], const float (&up)[3]) {
    uint32_t w[3][8];
#pragma unroll
    for (int j = 0; j < 16; j += 2) {
        uint32_t h[3][2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float a0, a1, a2;
            bf16s::split3(v[j + e], a0, a1, a2);
            h[0][e] = __float_as_uint(a0 * up[0]) >> 16;
            h[1][e] = __float_as_uint(a1 * up[1]) >> 16;
            h[2][e] = __float_as_uint(a2 * up[2]) >> 16;
        }
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) w[pc][j / 2] = h[pc][0] | (h[pc][1] << 16);
    }
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) {
        uint4 *dst = reinterpret_cast<uint4 *>(pq[pc] + sk * kTnPq + sc);
        dst[0] = make_uint4(w[pc][0], w[pc][1], w[pc][2], w[pc][3]);
        dst[1] = make_uint4(w[pc][4], w[pc][5], w[pc][6], w[pc][7]);
    }
}

// The MFMA fragments of this wave's blocks for one 32-deep contraction step
// ks over the staged planes: fa[piece][block] the block's rows, fb its columns.
struct TnFrags { uint4 a[3][3], b[3][3]; };
__device__ __forceinline__ void load_frags(const TnPlanes &pq, const WaveBlocks &wb, int lane, int ks, TnFrags &f) {
    const int co = 32 * ks + 8 * (lane >> 4);
#pragma unroll
    for (int b = 0; b < 3; ++b)
        if (b < wb.nb)
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) {
                f.a[pc][b] = *reinterpret_cast<const uint4 *>(pq[pc] + (16 * wb.bi[b] + (lane & 15)) * kTnPq + co);
                f.b[pc][b] = *reinterpret_cast<const uint4 *>(pq[pc] + (16 * wb.bj[b] + (lane & 15)) * kTnPq + co);
            }
}

// The Gram accumulators of a wave's blocks: G_A's terms A0^T A0, A1^T A0 +
// A0^T A1, A2^T A0 + A0^T A2 (scaled 2^(s0 + s_p)), then G1 and G2
struct GramAcc { f32x4_t a00[3], a01[3], a02[3], a1[3], a2[3]; };
__device__ __forceinline__ void gram_step(GramAcc &g, const TnFrags &f, const WaveBlocks &wb) {
#pragma unroll
    for (int b = 0; b < 3; ++b)
        if (b < wb.nb) {
            g.a02[b] = mfma_bf16(f.a[0][b], f.b[2][b], mfma_bf16(f.a[2][b], f.b[0][b], g.a02[b]));
            g.a01[b] = mfma_bf16(f.a[0][b], f.b[1][b], mfma_bf16(f.a[1][b], f.b[0][b], g.a01[b]));
            g.a00[b] = mfma_bf16(f.a[0][b], f.b[0][b], g.a00[b]);
            g.a1[b] = mfma_bf16(f.a[1][b], f.b[1][b], g.a1[b]);
            g.a2[b] = mfma_bf16(f.a[2][b], f.b[2][b], g.a2[b]);
        }
}
// M M of a symmetric M split into the staged planes, as the six products a2 b0
// + a1 b1 + a0 b2 + a1 b0 + a0 b1 + a0 b0 (smallest first)
__device__ __forceinline__ void square_step(f32x4_t (&sq)[3], const TnFrags &f, const WaveBlocks &wb) {
#pragma unroll
    for (int b = 0; b < 3; ++b)
        if (b < wb.nb) {
            sq[b] = mfma_bf16(f.a[2][b], f.b[0][b], sq[b]);
            sq[b] = mfma_bf16(f.a[1][b], f.b[1][b], sq[b]);
            sq[b] = mfma_bf16(f.a[0][b], f.b[2][b], sq[b]);
            sq[b] = mfma_bf16(f.a[1][b], f.b[0][b], sq[b]);
            sq[b] = mfma_bf16(f.a[0][b], f.b[1][b], sq[b]);
            sq[b] = mfma_bf16(f.a[0][b], f.b[0][b], sq[b]);
        }
}

// Row sums of a staged quarter (its 64 rows = its 64 storage columns) and
// |.|_F^2, in f64 from the pieces unscaled by dn[p] = 2^-s_p (exact): thread
// (rk, rc) sums column rc over k in [16 rk, 16 rk + 16) into rpart[.][rk][rc]
// and adds to its |.|_F^2 sums.  Plane 0 is A = A0 + A1 + A2 (exact in f64:
// three bf16 values of one f32's split).
__device__ __forceinline__ void quarter_sums(const TnPlanes &pq, const double (&dn)[3], int rk, int rc,
                                             double (&rpart)[3][4][kBK], double (&fro)[3]) {
    double s[3] = {0.0, 0.0, 0.0};
#pragma unroll 4
    for (int k = 16 * rk; k < 16 * rk + 16; ++k) {
        const double b0 = (double)__uint_as_float((uint32_t)pq[0][k * kTnPq + rc] << 16) * dn[0];
        const double b1 = (double)__uint_as_float((uint32_t)pq[1][k * kTnPq + rc] << 16) * dn[1];
        const double b2 = (double)__uint_as_float((uint32_t)pq[2][k * kTnPq + rc] << 16) * dn[2];
        const double a = b0 + b1 + b2;
        s[0] += fabs(a);
        s[1] += fabs(b1);
        s[2] += fabs(b2);
        fro[0] = fma(a, a, fro[0]);
        fro[1] = fma(b1, b1, fro[1]);
        fro[2] = fma(b2, b2, fro[2]);
    }
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) rpart[pc][rk][rc] = s[pc];
}

// a 16 x 16 block (bi >= bj) of plane pi's symmetric 64 x 64 Gram matrix,
// scaled 2^(2 sp[pi]), from the f32 MFMA accumulators (lane l, element v:
// row 16 bi + 4 (l>>4) + v, column 16 bj + (l&15)): G_A = a00 + 2^(s0 - s1)
// a01 + 2^(s0 - s2) a02 + 2^(2 (s0 - s1)) a1 in f64 (exact scalings); the
// entries above the diagonal of a diagonal block are left 0 (the stores
// mirror the lower ones)
__device__ __forceinline__ void gram_values(double (&x)[4], int bi, int bj, int lane, int pi, f32x4_t a00,
                                            f32x4_t a01, f32x4_t a02, f32x4_t a1, f32x4_t a2,
                                            const int (&sp)[3]) {
    const double c01 = ldexp(1.0, sp[0] - sp[1]), c02 = ldexp(1.0, sp[0] - sp[2]), c11 = c01 * c01;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int i = 16 * bi + 4 * (lane >> 4) + v, j = 16 * bj + (lane & 15);
        x[v] = (bi != bj || i >= j)
                   ? (pi == 0 ? (((double)a00[v] + c01 * (double)a01[v]) + c02 * (double)a02[v]) + c11 * (double)a1[v]
                              : (pi == 1 ? (double)a1[v] : (double)a2[v]))
                   : 0.0;
    }
}
// an f32 block (bi >= bj) of a symmetric matrix into gf (stride kTnGmLd):
// the lower entries and their mirror (a diagonal block's upper entries from
// its lower ones, so the stored matrix is exactly symmetric); the mirror of
// a lane's four rows is one 16-B store
__device__ __forceinline__ void store_sym_f32(float *gf, int bi, int bj, int lane, const float (&x)[4]) {
    const int i0 = 16 * bi + 4 * (lane >> 4), j = 16 * bj + (lane & 15);
    if (bi != bj) {
#pragma unroll
        for (int v = 0; v < 4; ++v) gf[(i0 + v) * kTnGmLd + j] = x[v];
        *reinterpret_cast<float4 *>(gf + j * kTnGmLd + i0) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (i0 + v >= j) {
                gf[(i0 + v) * kTnGmLd + j] = x[v];
                gf[j * kTnGmLd + i0 + v] = x[v];
            }
    }
}

template <bool FUSED>
__global__ __launch_bounds__(kBM, 2) void tile_norm_kernel(TilePtr<FUSED> aug, int64_t t0, float4 *__restrict__ lgn,
                                                           const double *__restrict__ Linv, int64_t ld, int64_t n,
                                                           double sf2) {
    __shared__ __attribute__((aligned(16))) TnPlanes pq;                 // a quarter's pieces, then M_k's (27 KiB)
    __shared__ __attribute__((aligned(16))) float gm[kBK * kTnGmLd];     // G, then its powers, normalised f32 (17 KiB)
    __shared__ double rpart[3][4][kBK];          // row-sum partials of a quarter (6 KiB)
    // the block reductions' slots, one per wave
    __shared__ float pmax[3][4];                 // the pieces' largest |entry|
    __shared__ double rwm[3][4], fred[3][4];     // per plane: row-sum maxima, |.|_F^2 sums
    __shared__ double red[2][4];                 // [0] a squaring's largest entry; [1] G_c's largest entry, then M4's row sums
    __shared__ float out[6];                     // (rows, spectral) of A; of A1; of A2 (LDS: a plane-indexed array)
    const int64_t tile = t0 + blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const WaveBlocks wb = wave_blocks(wave);
    const int sk = tid >> 2, sc = 16 * (tid & 3);   // staging: k row sk, storage columns sc .. sc + 15
    const int rc = tid & 63, rk = tid >> 6;         // row sums: column rc, k in [16 rk, 16 rk + 16)
    // the thread's 16 floats of quarter q: a quarter is one contiguous 64 x 64
    // block in k-major order (tile_offset)
    TilePtr<FUSED> mine = aug + tile * kTileFloats + 16 * tid;

    // 1. Pack (FUSED) and the pieces' maxima.  (The tile is read twice, the
    //    second time from L2 -- FUSED: the thread's own stores: this pass for
    //    the maxima, then the staging.)
    float amax[3] = {0.0f, 0.0f, 0.0f};
    int64_t fI = 0, fkb = 0;
    if constexpr (FUSED) tile_decode(tile, fI, fkb);
#pragma unroll
    for (int q = 0; q < kBM / 64; ++q) {
        float tv[16];
        if constexpr (FUSED)
            pack_row16(Linv, ld, n, sf2, fI, fkb, q, tid, mine + q * 64 * kBK, tv);
        else
            load_row16(mine + q * 64 * kBK, tv);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            float a0, a1, a2;
            bf16s::split3(tv[j], a0, a1, a2);
            amax[0] = fmaxf(amax[0], fabsf(a0));
            amax[1] = fmaxf(amax[1], fabsf(a1));
            amax[2] = fmaxf(amax[2], fabsf(a2));
        }
    }
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) wave_put(pmax[pc], wave_max(amax[pc]));
    __syncthreads();

    // 2. The pieces' scales: 2^sp max |piece| in [1, 2); up = 2^sp, dn = 2^-sp
    //    (exact).  f32 products and sums of the scaled pieces stay far above
    //    f32's underflow; unscaled, A2^T A2 of a tile of 2^-60 entries
    //    underflows and the bound is no bound.
    int sp[3];
    float up[3];
    double dn[3];
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) {
        const float m = slots_max(pmax[pc]);
        sp[pc] = m > 0.0f ? -ilogbf(m) : 0;
        up[pc] = ldexpf(1.0f, sp[pc]);
        dn[pc] = ldexp(1.0, -sp[pc]);
    }

    // 3. Per quarter (64 rows): stage the scaled pieces, one Gram step over
    //    the quarter's 64 storage columns (the contraction runs over the
    //    storage order: any order of the rows serves), the row sums.  Exact
    //    products, f32 accumulation: G1 = A1^T A1, G2 = A2^T A2, and G = A^T A
    //    taken as A0^T A0 + (A0^T A1 + A1^T A0) + (A0^T A2 + A2^T A0) + G1.
    //    |G_c - G| <= delta |A|^T |A| entrywise, delta = 2^-16 (<= 80 f32
    //    roundings of partial sums of |A|^T |A|, 4.8e-6, plus the dropped A1^T
    //    A2 + A2^T A1 + A2^T A2 and the split's remainder, < 2^-22 |A|^T |A|),
    //    so ||G_c - G||_2 <= delta |A|_F^2.  Row sums and |.|_F^2 come from the
    //    pieces in f64 (A0 + A1 + A2 = A to 2^-24: inside the outputs' 1e-5
    //    log2 margin).
    GramAcc g;
#pragma unroll
    for (int b = 0; b < 3; ++b) g.a00[b] = g.a01[b] = g.a02[b] = g.a1[b] = g.a2[b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    double rmax[3] = {0.0, 0.0, 0.0}, fro[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
    for (int q = 0; q < kBM / 64; ++q) {
        float tv[16];
        load_row16(mine + q * 64 * kBK, tv);
        stage_row16(pq, sk, sc, tv, up);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            TnFrags f;
            load_frags(pq, wb, lane, ks, f);
            gram_step(g, f, wb);
        }
        quarter_sums(pq, dn, rk, rc, rpart, fro);
        __syncthreads();   // (pq restaged next quarter; rpart complete)
        if (rk == 0)
#pragma unroll
            for (int pc = 0; pc < 3; ++pc)
                rmax[pc] = fmax(rmax[pc], ((rpart[pc][0][rc] + rpart[pc][1][rc]) + rpart[pc][2][rc]) + rpart[pc][3][rc]);
    }

    // 4. Block totals: the row sums' maxima and the sums of |.|_F^2, unscaled (exact: powers of two)
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) {
        wave_put(fred[pc], wave_sum(fro[pc]));
        wave_put(rwm[pc], wave_max(rmax[pc]));
    }
    __syncthreads();
    const double rowmax_all[3] = {slots_max(rwm[0]), slots_max(rwm[1]), slots_max(rwm[2])};

    // 5. Per plane (A itself, then A1, A2): Gram values, four squarings, the bound
    double lg_fro_a = -1000.0;
#pragma unroll 1
    for (int pi = 0; pi < 3; ++pi) {
        // 5a. The plane's Gram matrix G_c (f64, registers), normalised by its
        //     largest entry's power of two 2^e0 and rounded to f32: M0, stored
        //     symmetric (lower blocks mirrored).  ||G_c||_2 <= 2^e0 ||M0||_2 /
        //     (1 - 2^-21).
        double gv[3][4], gmx = 0.0;
#pragma unroll
        for (int b = 0; b < 3; ++b)
            if (b < wb.nb) {
                gram_values(gv[b], wb.bi[b], wb.bj[b], lane, pi, g.a00[b], g.a01[b], g.a02[b], g.a1[b], g.a2[b], sp);
#pragma unroll
                for (int v = 0; v < 4; ++v) gmx = fmax(gmx, fabs(gv[b][v]));
            }
        const double mx0 = block_max(red[1], wave_max(gmx));
        const int e0 = mx0 > 0.0 ? ilogb(mx0) : 0;
#pragma unroll
        for (int b = 0; b < 3; ++b)
            if (b < wb.nb) {
                float xf[4];
#pragma unroll
                for (int v = 0; v < 4; ++v) xf[v] = (float)ldexp(gv[b][v], -e0);
                store_sym_f32(gm, wb.bi[b], wb.bj[b], lane, xf);
            }
        const double fro2 = slots_sum(fred[pi]);
        const double s = rowmax_all[pi];
        // 5b. Four squarings on the bf16 matrix cores: M_k is split into three
        //     bf16 planes (pq, free after the Gram), S_k = M_k M_k is taken as
        //     six products (exact products, f32 accumulation) on the ten lower
        //     blocks, and M_(k+1) = 2^-e S_k (e: S_k's largest entry's
        //     exponent, exact) is stored mirrored, so every M_k is exactly
        //     symmetric.  |S_k - M_k^2| <= eps |M_k| |M_k| entrywise with eps =
        //     2^-15 (the dropped a1 b2 + a2 b1 + a2 b2 and the split's
        //     remainder < 2^-22, <= 396 f32 roundings of partial sums of the
        //     |terms| < 2.4e-5), so ||S_k - M_k^2||_2 <= eta ||M_k||_2^2 with
        //     eta = 64 eps (|| |M| |M| ||_2 <= |M|_F^2 <= 64 ||M||_2^2) and
        //     ||M_k||_2^2 <= ||S_k||_2 / (1 - eta).  Chained: log2 ||G_c||_2 <=
        //     e0 + (T + log2 ||M4||_inf + 15 log2(1 / (1 - eta))) / 16 +
        //     log2(1 / (1 - 2^-21)), T = 8 e1 + 4 e2 + 2 e3 + e4 (||M4||_2 <=
        //     ||M4||_inf: symmetric).  Underflow (entries below 2^-110 of the
        //     largest) costs < 2^-90 of ||S_k||_2 >= 1, inside eps's slack.
        int T = 0;
        bool live = mx0 > 0.0;
        for (int it = 0; it < kGramSquarings && live; ++it) {
            __syncthreads();   // M_k stored (and every read of pq by the last products done)
            float tv[16];   // row sk, columns sc .. sc + 15 of M_k into the planes, unscaled
            load_row16(gm + sk * kTnGmLd + sc, tv);
            stage_row16(pq, sk, sc, tv, {1.0f, 1.0f, 1.0f});
            __syncthreads();
            f32x4_t sq[3];
#pragma unroll
            for (int b = 0; b < 3; ++b) sq[b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                TnFrags f;
                load_frags(pq, wb, lane, ks, f);
                square_step(sq, f, wb);
            }
            float qmx = 0.0f;
#pragma unroll
            for (int b = 0; b < 3; ++b)
                if (b < wb.nb)
#pragma unroll
                    for (int v = 0; v < 4; ++v) qmx = fmaxf(qmx, fabsf(sq[b][v]));
            // (the barrier inside: every read of gm by the split is done too)
            const double mk = block_max(red[0], (double)wave_max(qmx));
            live = mk > 0.0;
            const int ek = live ? ilogb(mk) : 0;
            T = 2 * T + ek;
#pragma unroll
            for (int b = 0; b < 3; ++b)
                if (b < wb.nb) {
                    // (the diagonal block's upper entries are computed too; only the lower are kept)
                    const float xf[4] = {ldexpf(sq[b][0], -ek), ldexpf(sq[b][1], -ek), ldexpf(sq[b][2], -ek),
                                         ldexpf(sq[b][3], -ek)};
                    store_sym_f32(gm, wb.bi[b], wb.bj[b], lane, xf);
                }
        }
        __syncthreads();   // the last power stored
        // ||M4||_inf: largest absolute row sum (f64)
        double rs = 0.0;
        if (tid < kBK)
            for (int j = 0; j < kBK; ++j) rs += fabs((double)gm[tid * kTnGmLd + j]);
        rs = block_max(red[1], wave_max(rs));
        if (!live) rs = 0.0;   // (a zero Gram matrix)
        // 5c. log2 ||P||_2 (the plane scaled by 2^sp: G_c = 2^(2 sp) G) from
        //     the chain above, 1e-6 for the f64 row sums and logs; then
        //     ||P||_2^2 <= that^2 + delta |P|_F^2 (G_c's own error) + the
        //     absolute underflow term: 2^-110 per accumulator at its own
        //     scale, five for G_A, all at most 2^(-2 sp) unscaled
        const int spl = sp[pi];
        const double lg_g = (double)e0 +
                            ((double)T + log2(rs) - (double)((1 << kGramSquarings) - 1) * log2(1.0 - kSqEta)) /
                                (double)(1 << kGramSquarings) -
                            log2(1.0 - 0x1p-21);
        const double lg_pow = rs > 0.0 ? 0.5 * lg_g + 1e-6 - spl : -1000.0;
        const double spec2 = (rs > 0.0 ? exp2(2.0 * lg_pow) : 0.0) + kTnDelta * fro2 + ldexp(5.0, -110 - 2 * spl);
        const double lg_spec = spec2 > 0.0 ? 0.5 * log2(spec2) : -1000.0;
        const double lg_fro = fro2 > 0.0 ? 0.5 * log2(fro2) : -1000.0;
        if (tid == 0) {
            out[2 * pi] = s > 0.0 ? (float)log2(16.0 * s) + 1e-5f : -1000.0f;
            out[2 * pi + 1] = (float)fmin(lg_spec, lg_fro) + 1e-5f;
        }
        if (pi == 0) lg_fro_a = lg_fro;
        __syncthreads();   // gm and the slots are rewritten for the next plane
    }

    // 6. Store
    if (tid == 0) {
        lgn[2 * tile] = make_float4(out[0], out[1], (float)lg_fro_a + 1e-5f, 0.0f);
        lgn[2 * tile + 1] = make_float4(out[2], out[3], out[4], out[5]);
    }
}

// Bounding box of each k-tile's valid training points: (xmin, xmax, ymin, ymax);
// a tile with no valid point gets an empty box (+inf, -inf, +inf, -inf).
__global__ void tile_box_kernel(const float *__restrict__ x, const float *__restrict__ y, int64_t n,
                                int64_t ntiles, float4 *__restrict__ kbox) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles) return;
    float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int64_t k = t * kBK; k < (t + 1) * kBK && k < n; ++k) {
        x0 = fminf(x0, x[k]); x1 = fmaxf(x1, x[k]);
        y0 = fminf(y0, y[k]); y1 = fmaxf(y1, y[k]);
    }
    kbox[t] = make_float4(x0, x1, y0, y1);
}

// colmax[t] = max over the row blocks I that hold k-tile t of lgn[2 (tile_start(I) + t)].x
// (+inf if one is NaN: such a pair is never far)
__global__ void tile_colmax_kernel(const float4 *__restrict__ lgn, int nI, float *__restrict__ colmax) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= kTilesPerRowBlockStep * nI) return;
    float mx = -INFINITY;
    for (int I = t / kTilesPerRowBlockStep; I < nI; ++I) {
        const float v = lgn[2 * (tile_start(I) + t)].x;
        mx = v != v ? INFINITY : fmaxf(mx, v);
    }
    colmax[t] = mx;
}

}  // namespace

// ---------------------------------------------------------------- launchers
hipError_t launch_pack_kcoord(hipStream_t s, const float *x, const float *y, const float *alpha, int64_t n,
                              int64_t npad, double sf2, float *kcoord) {
    hipLaunchKernelGGL(pack_kcoord_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, s, x, y, alpha, n, npad,
                       (float)sf2, kcoord);
    return hipGetLastError();
}

hipError_t launch_pack_operand(hipStream_t s, const float *Linv, int64_t ld, int64_t n, int64_t npad, int64_t I0,
                               double sf2, const float *x, const float *y, const float *alpha, float *aug,
                               float *kcoord) {
    const int64_t nI = npad / kBM;
    if (I0 < nI) {
        hipLaunchKernelGGL(pack_operand_kernel, dim3((unsigned)(nI * kTilesPerRowBlockStep), (unsigned)(nI - I0)),
                           dim3(256), 0, s, Linv, ld, n, (float)sf2, I0, aug);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return launch_pack_kcoord(s, x, y, alpha, n, npad, sf2, kcoord);
}

hipError_t launch_row_l1(hipStream_t s, const float *aug, int64_t npad, int64_t I0, double *row_l1) {
    const int64_t nI = npad / kBM;
    if (I0 >= nI) return hipSuccess;
    hipError_t e = hipMemsetAsync(row_l1 + I0 * kBM, 0, sizeof(double) * (size_t)((nI - I0) * kBM), s);
    if (e != hipSuccess) return e;
    const int64_t chunks = (nI * kTilesPerRowBlockStep + kRowL1Tiles - 1) / kRowL1Tiles;
    hipLaunchKernelGGL(row_l1_kernel, dim3((unsigned)chunks, (unsigned)(nI - I0)), dim3(kBM), 0, s, aug, I0, row_l1);
    return hipGetLastError();
}

hipError_t launch_pack_tile_norms(hipStream_t s, const double *Linv, int64_t ld, int64_t n, int64_t npad, int64_t I0,
                                  double sf2, float *aug, float4 *lgn) {
    const int64_t nI = npad / kBM;
    const int64_t t0 = tile_start(I0), t1 = tile_start(nI);
    if (t1 <= t0) return hipSuccess;
    hipLaunchKernelGGL(tile_norm_kernel<true>, dim3((unsigned)(t1 - t0)), dim3(kBM), 0, s, aug, t0, lgn, Linv, ld, n,
                       sf2);
    return hipGetLastError();
}

hipError_t launch_tile_norms(hipStream_t s, const float *aug, int64_t npad, int64_t I0, float4 *lgn) {
    const int64_t nI = npad / kBM;
    const int64_t t0 = tile_start(I0), t1 = tile_start(nI);
    if (t1 <= t0) return hipSuccess;
    hipLaunchKernelGGL(tile_norm_kernel<false>, dim3((unsigned)(t1 - t0)), dim3(kBM), 0, s, aug, t0, lgn,
                       static_cast<const double *>(nullptr), (int64_t)0, (int64_t)0, 0.0);
    return hipGetLastError();
}

hipError_t launch_tile_boxes(hipStream_t s, const float *x, const float *y, int64_t n, int64_t npad, float4 *kbox) {
    const int64_t nt = npad / kBK;
    hipLaunchKernelGGL(tile_box_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, x, y, n, nt, kbox);
    return hipGetLastError();
}

hipError_t launch_tile_colmax(hipStream_t s, const float4 *lgn, int64_t npad, float *colmax) {
    const int nI = (int)(npad / kBM);
    if (nI <= 0) return hipSuccess;
    hipLaunchKernelGGL(tile_colmax_kernel, dim3((unsigned)((kTilesPerRowBlockStep * nI + 255) / 256)), dim3(256), 0, s,
                       lgn, nI, colmax);
    return hipGetLastError();
}

}  // namespace sbo
