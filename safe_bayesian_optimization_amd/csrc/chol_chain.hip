// chol_chain.hip -- the blocked Cholesky's chain (a2): per 128 columns, the
// kb x kb diagonal block's factorization (launch_chol_diag) and the solve of
// the panel below it (launch_chol_trsm), the factorization step rocSOLVER's
// spotrf spends most of its time in; and the f32 trailing update
// (launch_chol_update).  The host sequence is blocked_potrf (sbo_api.cpp).
//
// Three versions of each chain kernel (SBO_OPT_CHOL_DIAG), bitwise equal:
//   0  chol_diag_kernel      / chol_trsm_kernel       VALU, the plain reference
//   1  chol_diag_ll_kernel   / chol_trsm_ll_kernel    left-looking MFMA (default)
//   2  chol_diag_mfma_kernel / chol_trsm_mfma_kernel  right-looking MFMA
// The contract that lets them check each other: every element of the factor
// sees fmaf(-L[i][j], L[l][j], a) with j ascending, as the column-by-column
// right-looking Cholesky does, and every element of the panel its terms
// fmaf(-x_u, L[j][u], s) with u ascending, as the plain forward substitution.
// A v_mfma_f32_16x16x4_f32 is bit for bit a k-ordered fmaf chain, so the
// versions differ in who does the updates and when, never in their order.
// Versions 1 and 2 share the block load and store, the register panel step,
// the panel solve's prologue, 16 x 16 solve and store below; version 0 keeps
// its own masked 8-column panel and its own loads.
//
// f32 as spotrf.  A failed pivot (SBO_PIVOT_FAILS) stops the factorization:
// info = k0 + j + 1 (the leading minor, rocSOLVER's convention); later blocks
// see info != 0 and leave their data alone.  Column-major, lda = ld; only
// i >= j is written.
//
// Compiled with -ffp-contract=off: every fused multiply-add below is explicit.
#include "sbo_internal.hpp"

namespace sbo {
namespace {

#ifdef SBO_CHOL_STAMPS
// tools/chol_micro.hip only: s_memtime phase stamps of workgroup 0.  Slots
// 0-3 the diagonal block's entry / loaded / factored / stored, 4 and 5 its
// panels' and its updates' summed time, 8-11 the panel solve's entry / loaded
// / solved / stored.
__device__ unsigned long long g_chol_stamps[16];
#define SBO_CSTAMP(i) do { if (threadIdx.x == 0 && blockIdx.x == 0) g_chol_stamps[i] = __builtin_amdgcn_s_memtime(); } while (0)
#define SBO_CSTAMP_ZERO(i) do { if (threadIdx.x == 0 && blockIdx.x == 0) g_chol_stamps[i] = 0; } while (0)
#define SBO_CSTAMP_BEGIN(t0) const unsigned long long t0 = __builtin_amdgcn_s_memtime()
#define SBO_CSTAMP_ADD(i, t0) do { if (threadIdx.x == 0 && blockIdx.x == 0) g_chol_stamps[i] += __builtin_amdgcn_s_memtime() - (t0); } while (0)
#else
#define SBO_CSTAMP(i) do { } while (0)
#define SBO_CSTAMP_ZERO(i) do { } while (0)
#define SBO_CSTAMP_BEGIN(t0) do { } while (0)
#define SBO_CSTAMP_ADD(i, t0) do { } while (0)
#endif

typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float lane_value(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// Not positive definite: a pivot that is not > 0, NaN or infinite -- and one
// below FLT_MIN (denormal, flushed or zero) too, its v_rsq_f32 may overflow.
// A macro over a plain variable: as a function hipcc folds the test before it
// inlines it, and the record of the first failure then runs as lane-mask
// operations inside the unrolled panels (profiles/chol_chain.log, section 3).
#define SBO_PIVOT_FAILS(djj) (!((djj) >= 1.17549435e-38f) || !((djj) < __builtin_huge_valf()))

// Row ti of element q of a lower triangle counted row by row, q = ti (ti + 1) / 2 + tl
// with tl <= ti (the two loops correct the f32 guess's rounding).
__device__ __forceinline__ int tri_row(int q) {
    int ti = (int)((sqrtf(8.0f * (float)q + 1.0f) - 1.0f) * 0.5f);
    while ((ti + 1) * (ti + 2) / 2 <= q) ++ti;
    while (ti * (ti + 1) / 2 > q) --ti;
    return ti;
}

// ------------------------------------------------------- the diagonal block
// The block in LDS, row-major; row stride 132: a row's panel columns are
// aligned float4 reads.
typedef float CholBlock[kCholNB][kCholNB + 4];
constexpr int kCholPanel = 8;    // version 0's panel width
constexpr int kCholPW = 16;      // versions 1 and 2

// The kb x kb block in, padded to 128 x 128 with the identity (pivots 1, zero
// coupling: the real part sees exactly the arithmetic of the kb x kb
// factorization) and zero above the diagonal.  Thread (i, h): row i = tid &
// 127 of columns h, h + 2, ... (coalesced over i), 16 loads in flight per
// batch: every load is unconditional, from inside the kb x kb block -- rows
// and columns past kb read its last row / column and are replaced after.
__device__ __forceinline__ void chol_block_load(const float *__restrict__ A, int64_t ld, int kb, CholBlock &a) {
    const int li = threadIdx.x & (kCholNB - 1), lh = threadIdx.x >> 7;
    const float *colp = A + min(li, kb - 1);
    for (int j0 = 0; j0 < kCholNB; j0 += 32) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = colp[(int64_t)min(j0 + 2 * u + lh, kb - 1) * ld];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int j = j0 + 2 * u + lh;
            a[li][j] = (li < kb && j < kb && li >= j) ? v[u] : (li == j ? 1.0f : 0.0f);
        }
    }
}

// Its lower triangle out, the same thread map, 64 stores per thread issued back to back.
__device__ __forceinline__ void chol_block_store(float *__restrict__ A, int64_t ld, int kb, const CholBlock &a) {
    const int li = threadIdx.x & (kCholNB - 1), lh = threadIdx.x >> 7;
    float *colw = A + li + (int64_t)lh * ld;
    for (int j0 = 0; j0 < kCholNB; j0 += 32) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = a[li][j0 + 2 * u + lh];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int j = j0 + 2 * u + lh;
            if (li < kb && j < kb && li >= j) colw[(int64_t)(j0 + 2 * u) * ld] = v[u];
        }
    }
}

// A lane's R rows of the 16-column panel at jb between LDS and registers
// (rows past the block, clamped, are read and not stored).
template <int R>
__device__ __forceinline__ void chol_panel_load(const CholBlock &a, const int (&row)[R], int jb, float (&p)[R][kCholPW]) {
#pragma unroll
    for (int c4 = 0; c4 < kCholPW / 4; ++c4)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float4 u = reinterpret_cast<const float4 *>(&a[min(row[r], kCholNB - 1)][jb])[c4];
            p[r][4 * c4] = u.x; p[r][4 * c4 + 1] = u.y; p[r][4 * c4 + 2] = u.z; p[r][4 * c4 + 3] = u.w;
        }
}
__device__ __forceinline__ void chol_panel_store(CholBlock &a, int row, int jb, const float (&p)[kCholPW]) {
#pragma unroll
    for (int c = 0; c < kCholPW; ++c) a[row][jb + c] = p[c];
}

// The 16-column panel at jb factored in registers: lane l < 16 holds panel
// row jb + l in p[0] (the pivot rows: their values reach the other lanes by
// v_readlane, no barrier per column), every lane R rows in all.  Per column:
// 1 / sqrt(djj) once (v_rsq_f32), the column scaled by it and the pivot as
// djj * (1 / sqrt(djj)) -- one transcendental on the serial chain instead of
// a sqrt and two divisions -- then fmaf(-L[i][j], L[c2][j], .) on every later
// column c2.  Every lane, no row tests: the lanes above the diagonal (row <
// column) compute values of the upper triangle that nothing reads (a lane
// mask per column and row would be 136 live SGPR pairs).  No early exit
// either: the first failed pivot is returned (its leading minor within the
// block, else 0) and the rest of the panel computes garbage that the block
// never stores.
template <int R>
__device__ __forceinline__ int chol_panel_step(float (&rows)[R][kCholPW], int jb) {
    // (on a copy of its own: hipcc schedules the caller's array through one SGPR, profiles/chol_chain.log section 3)
    float p[R][kCholPW];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < kCholPW; ++c) p[r][c] = rows[r][c];
    int bad = 0;
#pragma unroll
    for (int c = 0; c < kCholPW; ++c) {
        const float djj = lane_value(p[0][c], c);
        if (bad == 0 && SBO_PIVOT_FAILS(djj)) bad = jb + c + 1;
        const float rs = __builtin_amdgcn_rsqf(djj);
#pragma unroll
        for (int r = 0; r < R; ++r) p[r][c] = p[r][c] * rs;
#pragma unroll
        for (int c2 = c + 1; c2 < kCholPW; ++c2) {
            const float lc2 = lane_value(p[0][c], c2);   // L[jb + c2][jb + c], lane c2's (already scaled)
#pragma unroll
            for (int r = 0; r < R; ++r) p[r][c2] = fmaf(-p[r][c], lc2, p[r][c2]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < kCholPW; ++c) rows[r][c] = p[r][c];
    return bad;
}

// Version 0: right-looking in 8-column panels, all of it on the VALU and
// masked to the kb x kb block (no padding).  A panel is factored by wave 0
// alone in registers (lane l holds rows jb + l and jb + 64 + l), the steps of
// chol_panel_step with row and width tests; the trailing lower triangle then
// takes the panel's rank-8 update from all four waves in 4 x 4 element tiles.
__global__ __launch_bounds__(256) void chol_diag_kernel(float *__restrict__ A, int64_t ld, int kb, int64_t k0,
                                                        int *__restrict__ info) {
    static_assert(kCholNB <= 128, "two panel rows per lane of wave 0");
    __shared__ __attribute__((aligned(16))) CholBlock a;
    __shared__ int s_bad;
    if (*info != 0) return;
    SBO_CSTAMP(0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the block in, kCholLoad independent loads per thread in flight at a time
    // (one at a time, the reads' latency was most of this kernel)
    constexpr int kCholLoad = 16;
    for (int e0 = 0; e0 < kb * kb; e0 += 256 * kCholLoad) {
        float v[kCholLoad];
#pragma unroll
        for (int u = 0; u < kCholLoad; ++u) {
            const int e = e0 + u * 256 + tid;
            const int i = e % kb, j = e / kb;
            v[u] = (e < kb * kb && i >= j) ? A[i + (int64_t)j * ld] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kCholLoad; ++u) {
            const int e = e0 + u * 256 + tid;
            const int i = e % kb, j = e / kb;
            if (e < kb * kb && i >= j) a[i][j] = v[u];
        }
    }
    if (tid == 0) s_bad = 0;
    __syncthreads();
    SBO_CSTAMP(1);
    SBO_CSTAMP_ZERO(4);
    SBO_CSTAMP_ZERO(5);
    for (int jb = 0; jb < kb; jb += kCholPanel) {
        const int w = min(kCholPanel, kb - jb);
        SBO_CSTAMP_BEGIN(tp0);
        if (wave == 0) {
            const int r0 = jb + lane, r1 = jb + 64 + lane;
            float p0[kCholPanel], p1[kCholPanel];
#pragma unroll
            for (int c = 0; c < kCholPanel; ++c) {
                p0[c] = (r0 < kb && c < w) ? a[r0][jb + c] : 0.0f;
                p1[c] = (r1 < kb && c < w) ? a[r1][jb + c] : 0.0f;
            }
            int bad = 0;
#pragma unroll
            for (int c = 0; c < kCholPanel; ++c) {
                if (c >= w || bad) continue;   // uniform
                const int j = jb + c;
                const float djj = lane_value(p0[c], c);   // row j is lane c's first row
                if (SBO_PIVOT_FAILS(djj)) {
                    bad = j + 1;
                    continue;
                }
                const float rs = __builtin_amdgcn_rsqf(djj);
                if (r0 > j) p0[c] = p0[c] * rs;
                else if (r0 == j) p0[c] = djj * rs;
                p1[c] = p1[c] * rs;   // r1 > j always
#pragma unroll
                for (int c2 = c + 1; c2 < kCholPanel; ++c2) {
                    if (c2 >= w) continue;
                    const float lc2 = lane_value(p0[c], c2);   // L[jb + c2][j], lane c2's (already scaled)
                    if (r0 >= jb + c2) p0[c2] = fmaf(-p0[c], lc2, p0[c2]);
                    p1[c2] = fmaf(-p1[c], lc2, p1[c2]);
                }
            }
#pragma unroll
            for (int c = 0; c < kCholPanel; ++c) {
                if (c < w && r0 < kb && r0 >= jb + c) a[r0][jb + c] = p0[c];
                if (c < w && r1 < kb) a[r1][jb + c] = p1[c];
            }
            if (lane == 0 && bad) s_bad = bad;
        }
        __syncthreads();
        SBO_CSTAMP_ADD(4, tp0);
        if (s_bad) break;
        SBO_CSTAMP_BEGIN(tu0);
        // rank-w update of the trailing lower triangle [t0, kb) in 4 x 4 tiles
        const int t0 = jb + w, n2 = kb - t0;
        const int nt = (n2 + 3) >> 2, ntiles = nt * (nt + 1) / 2;
        for (int q = tid; q < ntiles; q += 256) {
            const int ti = tri_row(q), tl = q - ti * (ti + 1) / 2;
            const int i0 = t0 + 4 * ti, l0 = t0 + 4 * tl;
            float li[4][kCholPanel], ll[4][kCholPanel];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // rows past kb read (finite) padding rows of the array; columns
                // past w are masked below
                const float4 *pi = reinterpret_cast<const float4 *>(&a[min(i0 + r, kCholNB - 1)][jb]);
                const float4 *pl = reinterpret_cast<const float4 *>(&a[min(l0 + r, kCholNB - 1)][jb]);
                const float4 i0v = pi[0], i1v = pi[1], l0v = pl[0], l1v = pl[1];
                const float iv[8] = {i0v.x, i0v.y, i0v.z, i0v.w, i1v.x, i1v.y, i1v.z, i1v.w};
                const float lv[8] = {l0v.x, l0v.y, l0v.z, l0v.w, l1v.x, l1v.y, l1v.z, l1v.w};
#pragma unroll
                for (int c = 0; c < kCholPanel; ++c) {
                    li[r][c] = (i0 + r < kb && c < w) ? iv[c] : 0.0f;
                    ll[r][c] = (l0 + r < kb && c < w) ? lv[c] : 0.0f;
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + r, l = l0 + u;
                    if (i < kb && l <= i) {
                        float v = a[i][l];
#pragma unroll
                        for (int c = 0; c < kCholPanel; ++c)
                            if (c < w) v = fmaf(-li[r][c], ll[u][c], v);
                        a[i][l] = v;
                    }
                }
        }
        __syncthreads();
        SBO_CSTAMP_ADD(5, tu0);
    }
    SBO_CSTAMP(2);
    if (s_bad) {
        if (tid == 0) atomicCAS(info, 0, (int)(k0 + s_bad));
        return;
    }
    for (int e = tid; e < kb * kb; e += 256) {
        const int i = e % kb, j = e / kb;
        if (i >= j) A[i + (int64_t)j * ld] = a[i][j];
    }
    SBO_CSTAMP(3);
}

// Version 2: right-looking.  Wave 0 factors each 16-column panel, two rows
// per lane (jb + l and jb + 64 + l); the lower triangle of 16 x 16 blocks
// behind the panel, spread over the four waves, then takes C -= L_i L_l^T as
// four MFMAs per block over the panel's 16 columns, through LDS.
__global__ __launch_bounds__(256) void chol_diag_mfma_kernel(float *__restrict__ A, int64_t ld, int kb, int64_t k0,
                                                             int *__restrict__ info) {
    static_assert(kCholNB == 128, "two panel rows per lane of wave 0, 8 x 16 blocks");
    __shared__ __attribute__((aligned(16))) CholBlock a;
    __shared__ int s_bad;
    if (*info != 0) return;
    SBO_CSTAMP(0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    chol_block_load(A, ld, kb, a);
    if (tid == 0) s_bad = 0;
    __syncthreads();
    SBO_CSTAMP(1);
    SBO_CSTAMP_ZERO(4);
    SBO_CSTAMP_ZERO(5);
    for (int jb = 0; jb < kCholNB; jb += kCholPW) {
        SBO_CSTAMP_BEGIN(tp0);
        if (wave == 0) {
            const int row[2] = {jb + lane, jb + 64 + lane};
            float p[2][kCholPW];
            chol_panel_load<2>(a, row, jb, p);
            const int bad = chol_panel_step<2>(p, jb);
#pragma unroll
            for (int r = 0; r < 2; ++r)
                if (row[r] < kCholNB) chol_panel_store(a, row[r], jb, p[r]);
            if (lane == 0 && bad) s_bad = bad;
        }
        __syncthreads();
        SBO_CSTAMP_ADD(4, tp0);
        if (s_bad) break;
        SBO_CSTAMP_BEGIN(tu0);
        // rank-16 update of the trailing lower triangle, 16 x 16 blocks
        const int t0 = jb + kCholPW, nbt = (kCholNB - t0) / 16, nblk = nbt * (nbt + 1) / 2;
        const int fi = lane & 15, fk = lane >> 4;   // operand lane map: A[fi][fk], B[fk][fi]; C row 4 fk + v, col fi
        for (int q = wave; q < nblk; q += 4) {
            int bi = 0, r = q;
            while (r > bi) { r -= bi + 1; ++bi; }
            const int i0 = t0 + 16 * bi, l0 = t0 + 16 * r;
            f32x4_t acc;
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[v] = a[i0 + 4 * fk + v][l0 + fi];
#pragma unroll
            for (int kk = 0; kk < kCholPW / 4; ++kk) {
                const float av = -a[i0 + fi][jb + 4 * kk + fk];
                const float bv = a[l0 + fi][jb + 4 * kk + fk];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) a[i0 + 4 * fk + v][l0 + fi] = acc[v];
        }
        __syncthreads();
        SBO_CSTAMP_ADD(5, tu0);
    }
    SBO_CSTAMP(2);
    if (s_bad) {
        if (tid == 0) atomicCAS(info, 0, (int)(k0 + s_bad));
        return;
    }
    chol_block_store(A, ld, kb, a);
    SBO_CSTAMP(3);
}

// Version 1: left-looking.  Before a 16-column panel is factored, the four
// waves bring its columns up to date with every factored column in one MFMA
// chain per 16 x 16 block, the accumulator in registers, instead of updating
// the whole trailing triangle through LDS after every panel; and the panel
// itself runs on all four waves, one row per lane.
__global__ __launch_bounds__(256) void chol_diag_ll_kernel(float *__restrict__ A, int64_t ld, int kb, int64_t k0,
                                                           int *__restrict__ info) {
    static_assert(kCholNB == 128, "8 x 16 blocks");
    __shared__ __attribute__((aligned(16))) CholBlock a;
    __shared__ int s_bad;
    if (*info != 0) return;
    SBO_CSTAMP(0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    chol_block_load(A, ld, kb, a);
    if (tid == 0) s_bad = 0;
    __syncthreads();
    SBO_CSTAMP(1);
    SBO_CSTAMP_ZERO(4);
    SBO_CSTAMP_ZERO(5);
    const int fi = lane & 15, fk = lane >> 4;   // operand lane map: A[fi][fk], B[fk][fi]; C row 4 fk + v, col fi
    for (int jb = 0; jb < kCholNB; jb += kCholPW) {
        if (jb > 0) {
            SBO_CSTAMP_BEGIN(tu0);
            // the panel's columns jb .. jb + 15, rows jb .. 127, from every
            // factored column 0 .. jb - 1
            for (int q = wave; q < (kCholNB - jb) / 16; q += 4) {
                const int i0 = jb + 16 * q;
                f32x4_t acc;
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[v] = a[i0 + 4 * fk + v][jb + fi];
                for (int k16 = 0; k16 < jb; k16 += 16) {
                    float av[4], bv[4];
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        av[kk] = -a[i0 + fi][k16 + 4 * kk + fk];
                        bv[kk] = a[jb + fi][k16 + 4 * kk + fk];
                    }
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk], bv[kk], acc, 0, 0, 0);
                }
#pragma unroll
                for (int v = 0; v < 4; ++v) a[i0 + 4 * fk + v][jb + fi] = acc[v];
            }
            __syncthreads();
            SBO_CSTAMP_ADD(5, tu0);
        }
        SBO_CSTAMP_BEGIN(tp0);
        {
            // every wave factors the panel's top 16 x 16 triangle in lanes
            // 0-15 (the pivot rows its other lanes need) and 48 of the rows
            // below it in lanes 16-63; wave 0 writes the triangle.  Each row
            // sees the same operations as on one wave.
            const int row[1] = {lane < 16 ? jb + lane : jb + 16 + 48 * wave + (lane - 16)};
            float p[1][kCholPW];
            chol_panel_load<1>(a, row, jb, p);
            __syncthreads();   // (every wave has read the triangle before wave 0 writes it)
            const int bad = chol_panel_step<1>(p, jb);
            if (row[0] < kCholNB && (lane >= 16 || wave == 0)) chol_panel_store(a, row[0], jb, p[0]);
            if (tid == 0 && bad) s_bad = bad;
        }
        __syncthreads();
        SBO_CSTAMP_ADD(4, tp0);
        if (s_bad) break;
    }
    SBO_CSTAMP(2);
    if (s_bad) {
        if (tid == 0) atomicCAS(info, 0, (int)(k0 + s_bad));
        return;
    }
    chol_block_store(A, ld, kb, a);
    SBO_CSTAMP(3);
}

// ------------------------------------------------------ the trailing update
// C[r][c] -= sum_k P[r][k] Q[c][k] over 128 x 128 tiles of C (all tiles of an
// m x nc block, or, lower != 0, the tiles on and below the diagonal of an
// m x m block), f32 in and out, column-major with leading dimension ld, K
// columns of P and Q.  The products on the matrix cores with C itself as the
// accumulator's start, so every element sees fmaf(-P[r][k], Q[c][k], C) in k
// order, as in a right-looking factorization.  rocBLAS ssyrk / sgemm ran
// these at 55-75 TF.  Workgroup: 4 waves as 2 x 2 of 64 x 64; the MFMA's A
// side takes Q (the tile's columns) and its B side P (rows), so a lane's
// result column is a row of C: the stores run down C's columns.  K in chunks
// of 32 staged through LDS as [k][row] (row stride 144 floats: the 16 rows x
// 4 k of one fragment read hit 64 distinct banks), double buffered, the next
// chunk's global loads in flight during the MFMAs.
constexpr int kUpBM = 128, kUpBK = 32, kUpLd = kUpBM + 16;
__global__ __launch_bounds__(256, 2) void chol_update_kernel(const float *__restrict__ P, const float *__restrict__ Q,
                                                             int64_t ld, int m, int nc, int K, int lower,
                                                             float *__restrict__ C) {
    __shared__ float Ps[2][kUpBK][kUpLd], Qs[2][kUpBK][kUpLd];
    int ti, tj;
    if (lower) {
        const int q = blockIdx.x;
        ti = tri_row(q);
        tj = q - ti * (ti + 1) / 2;
    } else {
        const int ntj = (nc + kUpBM - 1) / kUpBM;
        ti = blockIdx.x / ntj;
        tj = blockIdx.x % ntj;
    }
    const int r0 = ti * kUpBM, c0 = tj * kUpBM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    // loader: row (tid & 127) of the chunk's k = (tid >> 7) + 2 u, u < 16, for P and Q
    const int lrow = tid & (kUpBM - 1), lk = tid >> 7;
    const bool prow = r0 + lrow < m, qrow = c0 + lrow < nc;
    const float *pp = P + (prow ? r0 + lrow : 0), *qp = Q + (qrow ? c0 + lrow : 0);
    float vp[16], vq[16];
    auto gload = [&](int k0) {
        // (K is a multiple of kUpBK: every k in range; rows past m / nc read
        // row 0 and are zeroed)
        const float *p0 = pp + (int64_t)(k0 + lk) * ld, *q0 = qp + (int64_t)(k0 + lk) * ld;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const float a = p0[(int64_t)(2 * u) * ld], c = q0[(int64_t)(2 * u) * ld];
            vp[u] = prow ? a : 0.0f;
            vq[u] = qrow ? c : 0.0f;
        }
    };
    auto lstore = [&](int b) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            Ps[b][lk + 2 * u][lrow] = vp[u];
            Qs[b][lk + 2 * u][lrow] = vq[u];
        }
    };
    // accumulators from C: acc[cb][rb] holds C[r0 + 64 wr + 16 rb + (lane & 15)][c0 + 64 wc + 16 cb + 4 (lane >> 4) + v]
    const int fr = lane & 15, fg = lane >> 4;
    // a tile inside the block (uniform) needs no per-element tests
    const bool interior = r0 + kUpBM <= m && c0 + kUpBM <= nc;
    float *cw = C + (int64_t)(r0 + 64 * wr + fr) + (int64_t)(c0 + 64 * wc + 4 * fg) * ld;
    f32x4_t acc[4][4];
    if (interior) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[cb][rb][v] = cw[16 * rb + (int64_t)(16 * cb + v) * ld];
    } else {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const int r = r0 + 64 * wr + 16 * rb + fr;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int c = c0 + 64 * wc + 16 * cb + 4 * fg + v;
                    acc[cb][rb][v] = (r < m && c < nc) ? cw[16 * rb + (int64_t)(16 * cb + v) * ld] : 0.0f;
                }
            }
    }
    gload(0);
    lstore(0);
    __syncthreads();
    const int nchunk = K / kUpBK;
    for (int ch = 0; ch < nchunk; ++ch) {
        const int b = ch & 1;
        if (ch + 1 < nchunk) gload((ch + 1) * kUpBK);
#pragma unroll
        for (int kk = 0; kk < kUpBK / 4; ++kk) {
            const int k = 4 * kk + fg;
            float qa[4], pb[4];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) qa[cb] = Qs[b][k][64 * wc + 16 * cb + fr];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) pb[rb] = -Ps[b][k][64 * wr + 16 * rb + fr];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
                    acc[cb][rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[cb], pb[rb], acc[cb][rb], 0, 0, 0);
        }
        if (ch + 1 < nchunk) lstore(b ^ 1);
        __syncthreads();
    }
    if (interior) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int v = 0; v < 4; ++v) cw[16 * rb + (int64_t)(16 * cb + v) * ld] = acc[cb][rb][v];
    } else {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const int r = r0 + 64 * wr + 16 * rb + fr;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int c = c0 + 64 * wc + 16 * cb + 4 * fg + v;
                    if (r < m && c < nc) cw[16 * rb + (int64_t)(16 * cb + v) * ld] = acc[cb][rb][v];
                }
            }
    }
}

// ---------------------------------------------------------- the panel solve
// A21 := A21 L11^-T for the m2 x kb panel below a factored kb x kb diagonal
// block (rocBLAS strsm right / lower / transpose ran as ~10 launches, ~100 us
// per step, on the factorization's critical path).  Forward substitution row
// by row, x L11^T = a, in 16-column blocks: 128 panel rows per workgroup, two
// threads per row (t and t + 128, one wave per SIMD); L11 row-major in LDS
// (stride 132: a row's 16-column blocks are aligned float4 reads, every lane
// reading the same address -- broadcast), the rows being solved in LDS
// column-major (lane-linear, conflict-free).  The reciprocal of the pivot is
// the one extra rounding strsm's inverted diagonal has too.  kb < 128 (the
// last step) pads L11 with the identity.
constexpr int kTrsmLd = 132;
constexpr int kTrX = kCholNB + 4;   // versions 1 and 2: X's stride, conflict-free MFMA result reads and writes
typedef float TrsmL[kCholNB * kTrsmLd];
typedef float TrsmX[kCholNB * kTrX];

// Versions 1 and 2, the prologue: L11's lower triangle into Ls (zero above,
// identity past kb), the workgroup's 128 panel rows into X (zero past m2 and
// past kb), the pivots' reciprocals, once per workgroup, into rinv.  Thread
// (t, h) takes columns h, h + 2, ... of L11's row t and of panel row t, two
// batches of 64 loads in flight: every load unconditional, clamped into the
// block, the padding replaced after.
__device__ __forceinline__ void trsm_panel_load(const float *__restrict__ L11, int64_t ld, int kb,
                                                const float *__restrict__ A21, int64_t m2, TrsmL &Ls, TrsmX &X,
                                                float (&rinv)[kCholNB]) {
    const int tid = threadIdx.x, t = tid & (kCholNB - 1), h = tid >> 7;
    const int64_t row = (int64_t)blockIdx.x * kCholNB + t;
    const bool in = row < m2, lin = t < kb;
    const float *lp = L11 + min(t, kb - 1);
    const float *xp = A21 + (in ? row : 0);
    for (int jb = 0; jb < kCholNB; jb += 64) {
        float lv[32], xv[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            const int64_t off = (int64_t)min(jb + 2 * u + h, kb - 1) * ld;
            lv[u] = lp[off];
            xv[u] = xp[off];
        }
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            const int j = jb + 2 * u + h;
            Ls[t * kTrsmLd + j] = (j < kb && lin && t >= j) ? lv[u] : (t == j && j >= kb ? 1.0f : 0.0f);
            X[j * kTrX + t] = (in && j < kb) ? xv[u] : 0.0f;
        }
    }
    __syncthreads();
    if (tid < kCholNB) rinv[tid] = __fdiv_rn(1.0f, Ls[tid * kTrsmLd + tid]);
    __syncthreads();
}

// Versions 1 and 2: panel row t solves the 16 columns at j0 in registers,
// right-looking -- after x_q, every later s_q' of the block takes
// fmaf(-x_q, L[q'][q], s_q') -- the block's 16 x 16 lower triangle of L read
// into registers first (broadcast reads) so that the chain waits on no LDS
// read.
__device__ __forceinline__ void trsm_block_solve(const TrsmL &Ls, TrsmX &X, const float (&rinv)[kCholNB], int j0, int t) {
    float4 lb[16][4];
#pragma unroll
    for (int q = 0; q < 16; ++q)
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (4 * v <= q) lb[q][v] = reinterpret_cast<const float4 *>(Ls + (j0 + q) * kTrsmLd + j0)[v];
    float sb[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) sb[q] = X[(j0 + q) * kTrX + t];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        sb[q] = sb[q] * rinv[j0 + q];
#pragma unroll
        for (int q2 = q + 1; q2 < 16; ++q2) {
            const float4 l4 = lb[q2][q >> 2];
            const float l = (q & 3) == 0 ? l4.x : (q & 3) == 1 ? l4.y : (q & 3) == 2 ? l4.z : l4.w;
            sb[q2] = fmaf(-sb[q], l, sb[q2]);
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) X[(j0 + q) * kTrX + t] = sb[q];
}

// Versions 1 and 2: the solved rows out, thread (t, h) every other column.
__device__ __forceinline__ void trsm_panel_store(float *__restrict__ A21, int64_t ld, int kb, int64_t m2, const TrsmX &X) {
    const int t = threadIdx.x & (kCholNB - 1), h = threadIdx.x >> 7;
    const int64_t row = (int64_t)blockIdx.x * kCholNB + t;
    if (row < m2)
        for (int j = h; j < kb; j += 2) A21[row + (int64_t)j * ld] = X[j * kTrX + t];
}

// Version 0, on the VALU: both threads of a row solve the block's 16 values,
// x_j = (a_j - sum_{u<j} x_u L_ju) * (1 / L_jj) (ascending u), then each
// takes every other later column and subtracts the block's 16 terms.
__global__ __launch_bounds__(256) void chol_trsm_kernel(const float *__restrict__ L11, int64_t ld, int kb,
                                                        float *__restrict__ A21, int64_t m2) {
    __shared__ __attribute__((aligned(16))) float Ls[kCholNB * kTrsmLd];
    __shared__ float X[kCholNB * kCholNB];
    SBO_CSTAMP(8);
    const int tid = threadIdx.x, t = tid & (kCholNB - 1), h = tid >> 7;
    const int64_t row = (int64_t)blockIdx.x * kCholNB + t;
    const bool in = row < m2;
    // columns of L11 and of the panel rows (coalesced over t), 16 columns of
    // loads in flight at a time, half the columns per thread of the pair
    // (one predicate per thread for the loads, so all 16 of a batch are in
    // flight together; the upper triangle and the padding are fixed up after)
    const bool lin = t < kb;
    for (int j0 = 8 * h; j0 < kCholNB; j0 += 16) {
        float lv[8], xv[8];
        if (j0 + 8 <= kb) {
            if (lin) {
#pragma unroll
                for (int u = 0; u < 8; ++u) lv[u] = L11[t + (int64_t)(j0 + u) * ld];
            }
            if (in) {
#pragma unroll
                for (int u = 0; u < 8; ++u) xv[u] = A21[row + (int64_t)(j0 + u) * ld];
            }
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                lv[u] = (lin && j0 + u < kb) ? L11[t + (int64_t)(j0 + u) * ld] : 0.0f;
                xv[u] = (in && j0 + u < kb) ? A21[row + (int64_t)(j0 + u) * ld] : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = j0 + u;
            Ls[t * kTrsmLd + j] = (j < kb && lin && t >= j) ? lv[u] : (t == j && j >= kb ? 1.0f : 0.0f);
            X[j * kCholNB + t] = (in && j < kb) ? xv[u] : 0.0f;
        }
    }
    __syncthreads();
    SBO_CSTAMP(9);
    for (int B = 0; B < kCholNB / 16; ++B) {
        const int j0 = 16 * B;
        // the 16 x 16 diagonal block of L (lower: row q needs q + 1 values)
        float4 lb[16][4];
#pragma unroll
        for (int q = 0; q < 16; ++q)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (4 * v <= q) lb[q][v] = reinterpret_cast<const float4 *>(Ls + (j0 + q) * kTrsmLd + j0)[v];
        float xb[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) xb[u] = X[(j0 + u) * kCholNB + t];
        float rinv[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float4 d = lb[q][q >> 2];
            rinv[q] = __fdiv_rn(1.0f, (q & 3) == 0 ? d.x : (q & 3) == 1 ? d.y : (q & 3) == 2 ? d.z : d.w);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            float s = xb[q];
#pragma unroll
            for (int u = 0; u < q; ++u) {
                const float4 l4 = lb[q][u >> 2];
                const float l = (u & 3) == 0 ? l4.x : (u & 3) == 1 ? l4.y : (u & 3) == 2 ? l4.z : l4.w;
                s = fmaf(-xb[u], l, s);
            }
            xb[q] = s * rinv[q];
        }
        __syncthreads();   // every read of this block's columns is done
        if (h == 0) {
#pragma unroll
            for (int u = 0; u < 16; ++u) X[(j0 + u) * kCholNB + t] = xb[u];
        }
        // later columns of this thread (every other one), four at a time:
        // four independent FMA chains in flight instead of one
        for (int c0 = j0 + 16 + h; c0 < kCholNB; c0 += 8) {
            float v[4];
            float lv[4][16];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = min(c0 + 2 * k, kCholNB - 1);
                const float4 *lr = reinterpret_cast<const float4 *>(Ls + c * kTrsmLd + j0);
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const float4 l4 = lr[q4];
                    lv[k][4 * q4] = l4.x;
                    lv[k][4 * q4 + 1] = l4.y;
                    lv[k][4 * q4 + 2] = l4.z;
                    lv[k][4 * q4 + 3] = l4.w;
                }
                v[k] = X[c * kCholNB + t];
            }
#pragma unroll
            for (int u = 0; u < 16; ++u)
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = fmaf(-xb[u], lv[k][u], v[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c0 + 2 * k < kCholNB) X[(c0 + 2 * k) * kCholNB + t] = v[k];
        }
        __syncthreads();
    }
    SBO_CSTAMP(10);
    if (in)
        for (int j = h; j < kb; j += 2) A21[row + (int64_t)j * ld] = X[j * kCholNB + t];
    SBO_CSTAMP(11);
}

// Version 2: right-looking.  After the rows solve a 16-column block, its
// rank-16 update of every later column, X[c][t] -= sum_u L[c][u] x_u(t), runs
// as MFMAs through LDS: the A side takes L (result rows = columns c of X),
// the B side the solved x (result columns = panel rows t, contiguous in X's
// [c][t] layout).
__global__ __launch_bounds__(256) void chol_trsm_mfma_kernel(const float *__restrict__ L11, int64_t ld, int kb,
                                                             float *__restrict__ A21, int64_t m2) {
    __shared__ __attribute__((aligned(16))) TrsmL Ls;
    __shared__ TrsmX X;
    __shared__ float rinv[kCholNB];
    SBO_CSTAMP(8);
    const int tid = threadIdx.x, t = tid & (kCholNB - 1), h = tid >> 7;
    const int lane = tid & 63, wave = tid >> 6;
    trsm_panel_load(L11, ld, kb, A21, m2, Ls, X, rinv);
    SBO_CSTAMP(9);
    const int fr = lane & 15, fg = lane >> 4;
    for (int B = 0; B < kCholNB / 16; ++B) {
        const int j0 = 16 * B;
        if (h == 0) trsm_block_solve(Ls, X, rinv, j0, t);
        __syncthreads();
        // rank-16 update of the later columns: 16 x 16 result blocks (column
        // block ci, row block ri), spread over the four waves
        const int c1 = j0 + 16, nci = (kCholNB - c1) / 16, nblk = nci * (kCholNB / 16);
        for (int qb = wave; qb < nblk; qb += 4) {
            const int ci = qb / (kCholNB / 16), ri = qb % (kCholNB / 16);
            const int cb0 = c1 + 16 * ci, rb0 = 16 * ri;
            f32x4_t acc;
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[v] = X[(cb0 + 4 * fg + v) * kTrX + rb0 + fr];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int u = 4 * kk + fg;
                const float av = -Ls[(cb0 + fr) * kTrsmLd + j0 + u];
                const float bv = X[(j0 + u) * kTrX + rb0 + fr];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) X[(cb0 + 4 * fg + v) * kTrX + rb0 + fr] = acc[v];
        }
        __syncthreads();
    }
    SBO_CSTAMP(10);
    trsm_panel_store(A21, ld, kb, m2, X);
    SBO_CSTAMP(11);
}

// Version 1: left-looking.  Before the rows solve 16-column block B, the four
// waves bring its columns up to date with every solved column 0 .. 16B - 1 in
// one MFMA chain per 16 x 16 result block, the accumulator in registers from
// X itself; the right-looking kernel reads and writes every later block's
// accumulators through LDS after every block (56 16 x 16 updates per wave,
// each a four-MFMA chain) where this issues 8B MFMAs per wave as two
// interleaved chains.  Wave w owns row blocks 2w and 2w + 1 (rows 32w ..
// 32w + 31).
__global__ __launch_bounds__(256) void chol_trsm_ll_kernel(const float *__restrict__ L11, int64_t ld, int kb,
                                                           float *__restrict__ A21, int64_t m2) {
    __shared__ __attribute__((aligned(16))) TrsmL Ls;
    __shared__ TrsmX X;
    __shared__ float rinv[kCholNB];
    SBO_CSTAMP(8);
    const int tid = threadIdx.x, t = tid & (kCholNB - 1), h = tid >> 7;
    const int lane = tid & 63, wave = tid >> 6;
    trsm_panel_load(L11, ld, kb, A21, m2, Ls, X, rinv);
    SBO_CSTAMP(9);
    const int fr = lane & 15, fg = lane >> 4;
    const int rb0 = 32 * wave, rb1 = rb0 + 16;
    for (int B = 0; B < kCholNB / 16; ++B) {
        const int j0 = 16 * B;
        if (B > 0) {
            f32x4_t acc0, acc1;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                acc0[v] = X[(j0 + 4 * fg + v) * kTrX + rb0 + fr];
                acc1[v] = X[(j0 + 4 * fg + v) * kTrX + rb1 + fr];
            }
            for (int k16 = 0; k16 < B; ++k16) {   // (16 columns at a time: operand reads batched)
                float av[4], b0[4], b1[4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int u = 16 * k16 + 4 * kk + fg;
                    av[kk] = -Ls[(j0 + fr) * kTrsmLd + u];
                    b0[kk] = X[u * kTrX + rb0 + fr];
                    b1[kk] = X[u * kTrX + rb1 + fr];
                }
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk], b0[kk], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk], b1[kk], acc1, 0, 0, 0);
                }
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                X[(j0 + 4 * fg + v) * kTrX + rb0 + fr] = acc0[v];
                X[(j0 + 4 * fg + v) * kTrX + rb1 + fr] = acc1[v];
            }
            __syncthreads();
        }
        if (h == 0) trsm_block_solve(Ls, X, rinv, j0, t);
        __syncthreads();
    }
    SBO_CSTAMP(10);
    trsm_panel_store(A21, ld, kb, m2, X);
    SBO_CSTAMP(11);
}

}  // namespace

hipError_t launch_chol_diag(hipStream_t s, float *A, int64_t ld, int kb, int64_t k0, int *info, int version) {
    if (kb <= 0 || kb > kCholNB) return hipErrorInvalidValue;
    if (version == 1)
        hipLaunchKernelGGL(chol_diag_ll_kernel, dim3(1), dim3(256), 0, s, A, ld, kb, k0, info);
    else if (version == 2)
        hipLaunchKernelGGL(chol_diag_mfma_kernel, dim3(1), dim3(256), 0, s, A, ld, kb, k0, info);
    else
        hipLaunchKernelGGL(chol_diag_kernel, dim3(1), dim3(256), 0, s, A, ld, kb, k0, info);
    return hipGetLastError();
}

hipError_t launch_chol_update(hipStream_t s, const float *P, const float *Q, int64_t ld, int64_t m, int64_t nc,
                              int64_t K, bool lower, float *C) {
    if (m < 0 || nc < 0 || K < 0 || m > INT32_MAX / 2 || nc > INT32_MAX / 2 || K > INT32_MAX / 2 || (lower && nc != m) ||
        K % kUpBK != 0)
        return hipErrorInvalidValue;
    if (m == 0 || nc == 0 || K == 0) return hipSuccess;
    const int64_t nti = (m + kUpBM - 1) / kUpBM, ntj = (nc + kUpBM - 1) / kUpBM;
    const int64_t tiles = lower ? nti * (nti + 1) / 2 : nti * ntj;
    if (tiles > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(chol_update_kernel, dim3((unsigned)tiles), dim3(256), 0, s, P, Q, ld, (int)m, (int)nc, (int)K,
                       lower ? 1 : 0, C);
    return hipGetLastError();
}

hipError_t launch_chol_trsm(hipStream_t s, const float *L11, int64_t ld, int kb, float *A21, int64_t m2, int version) {
    if (kb <= 0 || kb > kCholNB || m2 < 0) return hipErrorInvalidValue;
    if (m2 == 0) return hipSuccess;
    const dim3 grid((unsigned)((m2 + kCholNB - 1) / kCholNB)), block(2 * kCholNB);
    if (version == 1)
        hipLaunchKernelGGL(chol_trsm_ll_kernel, grid, block, 0, s, L11, ld, kb, A21, m2);
    else if (version == 2)
        hipLaunchKernelGGL(chol_trsm_mfma_kernel, grid, block, 0, s, L11, ld, kb, A21, m2);
    else
        hipLaunchKernelGGL(chol_trsm_kernel, grid, block, 0, s, L11, ld, kb, A21, m2);
    return hipGetLastError();
}

}  // namespace sbo
