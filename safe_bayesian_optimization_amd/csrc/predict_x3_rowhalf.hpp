// predict_x3_rowhalf.hpp -- the split sweep's kernel and the pack of its
// operand, in the row-half layout (x3_layout 2).  Included by predict_x3.hip
// (the product) and by diag/predict_x3_diag.hip (whose variants 3 and 22 are
// this kernel), so the two libraries run the same code by construction.
//
// A stage is 64 k x 128 rows: row half R of a 64-k tile, three bf16 planes
// of 16 KiB, each plane eight row blocks x two k halves of one 1 KiB
// lane-fragment piece.  A step is (tile, row half): every row block's MFMA
// chain starts from zero, runs over k half 0 and then k half 1 in the level's
// product order and ends inside its step.  The eight finished chains of a
// step stay in registers (fin[R]); the R = 0 step hands its eight across the
// barrier to the R = 1 step, and one tile end (x3_tile_end) after the R = 1
// body adds all sixteen into the f32 outer sums, one add per block per tile.
// (The compiler sank the adds there from wherever the source placed them; the
// source now says so, and spends 32 packed adds on them instead of 64.)  Per
// 16 x 16 block this is the sequence of MFMAs of the k-half stages it
// replaces (chain over k half 0, continued over k half 1) and the same one
// add, so the results are bitwise the same.
//
// K* is built once per tile for all 64 k (kb[2]: one set of pieces per k
// half) and serves both row-half steps; the next tile's K* and its mean terms
// are built beside the MFMAs, k half R during step R (nx[R]).  The next
// tile's coordinates (1 KiB, once per tile) and, with an item's first tile,
// its 128 queries arrive in small LDS rings of their own, one tile ahead of
// the A stages: issued at the top of step (t, 1) for tile t + 2, read during
// the two steps of tile t + 1.
#pragma once
#include <cstdint>
#include <type_traits>

#include "bf16_split.hpp"
#include "sbo_internal.hpp"

namespace sbo {
namespace x3r {
namespace {

using bf16s::hi_f32;
using bf16s::lo_f32;
using bf16s::pk_bf16;
using bf16s::split3;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// The translation units of this kernel are built without packed f32 VALU
// (v_pk_* beside bf16 MFMAs costs more issue cycles than the scalar pair).
// The kernel turns it on again for itself, for the tile end alone: the step
// bodies hold no vector-typed f32 arithmetic and the units are built without
// SLP vectorisation, so nothing between a step's first and last MFMA is
// packed.  (A device-only attribute: the host pass does not know the feature.)
#if defined(__HIP_DEVICE_COMPILE__)
#define SBO_X3_PACKED_F32 __attribute__((target("packed-fp32-ops")))
#else
#define SBO_X3_PACKED_F32
#endif

constexpr int kXH = 32;                  // k per K* piece set (a k half)
constexpr int kXPlane = (kBM / 2) * kBK * 2;  // one bf16 plane of a row half: 16 KiB
constexpr int kXA = 3 * kXPlane;         // the A stage: 48 KiB
constexpr int kXSlot = kXA;
constexpr int kXSlots = 3;
constexpr int kXWin = kXSlots * kXSlot;  // the step-record windows follow the slots (2 x 1 KiB)
constexpr int kXCrd = kXWin + 2048;      // the coordinate ring: 2 x (2 k halves x x[32], y[32], sf2 alpha[32], pad)
constexpr int kXQry = kXCrd + 2048;      // the query ring: 2 x (qx[128], qy[128])
constexpr int kXSmem = kXQry + 2048;
constexpr int kRecWin = 64;              // step records (int4) per 1 KiB LDS window
constexpr int kLoaders = 8;              // every wave loads an eighth of each A stage
constexpr int kPieces = (kXA / 1024) / kLoaders;  // 6 A pieces per wave per stage (2 per plane)
constexpr int kStride = kLoaders * 1024;          // a wave's consecutive pieces
static_assert(kPieces == 6, "the end-of-step wait below counts 2, 4 or 6 pieces");
static_assert(kXPlane == 16 * 1024 && kBM == 256 && kBK == 64 && kBN == 128, "the stage is 64 k x 128 rows");

__device__ __forceinline__ float fast_exp2(float v) { return __builtin_amdgcn_exp2f(v); }

__device__ __forceinline__ bf16x8 as_bf16x8(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }

__device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(a), as_bf16x8(b), c, 0, 0, 0);
}

typedef __attribute__((address_space(3))) char lds_char;

__device__ __forceinline__ u32x4 lds_b128(const lds_char *p) {
    return *reinterpret_cast<const __attribute__((address_space(3))) u32x4 *>(p);
}
__device__ __forceinline__ float lds_f(const lds_char *p) {
    return *reinterpret_cast<const __attribute__((address_space(3))) float *>(p);
}
typedef float f32x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2v lds_f2(const lds_char *p) {
    return *reinterpret_cast<const __attribute__((address_space(3))) f32x2v *>(p);
}

// One LDS-DMA piece: 64 lanes x 16 B from sbase + voff to LDS at M0 = ldst
// (+ lane x 16).  s_nop: the M0 write -> LDS-DMA hazard.
__device__ __forceinline__ void dma16(uint32_t voff, const void *sbase, uint32_t ldst) {
    asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "{m0}"(ldst) : "memory");
}

// K* pieces of one k half (lane (g, r): k = 8g + j of the half, query 16 w + r)
struct KPieces {
    u32x4 h, m, l;
};

__device__ __forceinline__ float kstar1(float xk, float yk, float xq, float yq, float cexp) {
    const float dx = xk - xq, dy = yk - yq;
    return fast_exp2(fmaf(dy, dy, dx * dx) * cexp);
}

// Pin a value's computation to this point of the instruction stream (the
// IR-level sinking passes ignore sched_barrier and would otherwise bunch the
// next tile's K* work after the last MFMA), in an arch VGPR.
#define SBO_X3R_PIN(v) asm volatile("" : "+v"(v))

// One step of one wave: row half R of a tile, as 16 pieces u = 2 rb + h (row
// block rb of the half, k half h) x 6, 3 or 1 MFMA(s) (the tile's precision
// level LV) on this slot's A planes and the tile's K* pieces kb[h], with k
// half R of the next tile's K* pieces (nx) and its mean terms built beside
// them: pair i of the lane's eight k over pieces 4i .. 4i+3 (evaluate at
// u = 4i, 4i+1, split at 4i+2, mean terms at 4i+3; the next pair's
// coordinates are read at 4i+1).
//   A row block's chain starts from zero at h = 0, continues over h = 1 and
//   is left in fin[rb]: the step adds nothing into the outer sums (the tile
//   end does, x3_tile_end), so all eight chains are live at its end.
//   LV: 0 all six products, 1 the three largest (a1 kh + a0 km + a0 kh), 2 a0
//   kh alone; the A planes a level leaves out are not read from LDS, and A
//   fragments are read AH = 1 / 2 / 4 pieces ahead so the LDS latency stays
//   covered however few MFMAs a piece has.
//   NS: the next tile's level as the number of K* pieces and A planes it
//   reads (3: kh, km, kl; 2: kh, km; 1: kh alone) -- the split stops there (a
//   level reads no other piece, so the results are bitwise those of the full
//   split).
//   MEAN: the next tile is in the mean's row block.
// The stage two steps ahead (asrc -> adst: row half R of that same next
// tile) is issued here: this wave's A piece j between pieces j and j + 1, the
// 2 NS pieces of the planes its level reads and no others.
template <int R, int LV, int NS, bool MEAN>
__device__ __forceinline__ void x3_step(const lds_char *pa, const lds_char *pcn, float xq, float yq, int g, float cexp,
                                        const KPieces (&kb)[2], f32x4 (&fin)[8], KPieces &nx, double &mu,
                                        uint32_t voff, const char *asrc, uint32_t adst) {
    // the pieces the next tile's level does not read: no value to keep alive
    if constexpr (NS < 3) nx.l = __builtin_nondeterministic_value(nx.l);
    if constexpr (NS < 2) nx.m = __builtin_nondeterministic_value(nx.m);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    constexpr bool P1 = LV <= 1, P2 = LV == 0;  // planes a1, a2 in use
    constexpr int NPROD = LV == 0 ? 6 : (LV == 1 ? 3 : 1);
    constexpr int AH = LV == 2 ? 4 : (LV == 1 ? 2 : 1);
    u32x4 f0[16], f1[16], f2[16];
#pragma unroll
    for (int r = 0; r < AH; ++r) {
        f0[r] = lds_b128(pa + r * 1024);
        if constexpr (P1) f1[r] = lds_b128(pa + kXPlane + r * 1024);
        if constexpr (P2) f2[r] = lds_b128(pa + 2 * kXPlane + r * 1024);
    }
    // coordinates of pair 0 (sf2 alpha only before the mean's row block)
    f32x2v xk = lds_f2(pcn + g * 32), yk = lds_f2(pcn + 128 + g * 32), ak = {0.f, 0.f};
    if constexpr (MEAN) ak = lds_f2(pcn + 256 + g * 32);
    f32x2v e;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int rb = u >> 1, h = u & 1;
        if (u + AH < 16) {
            f0[u + AH] = lds_b128(pa + (u + AH) * 1024);
            if constexpr (P1) f1[u + AH] = lds_b128(pa + kXPlane + (u + AH) * 1024);
            if constexpr (P2) f2[u + AH] = lds_b128(pa + 2 * kXPlane + (u + AH) * 1024);
        }
        const u32x4 a0 = f0[u];
        u32x4 a1 = {}, a2 = {};
        if constexpr (P1) a1 = f1[u];
        if constexpr (P2) a2 = f2[u];
        // ---- the next tile's K* (k half R), pair i over pieces 4i .. 4i+3
        const int i = u >> 2, ph = u & 3;
        if (ph <= 1) {
            float ev = kstar1(ph == 0 ? xk.x : xk.y, ph == 0 ? yk.x : yk.y, xq, yq, cexp);
            SBO_X3R_PIN(ev);
            if (ph == 0) e.x = ev; else e.y = ev;
            if (ph == 1 && i < 3) {  // the next pair's x, y
                xk = lds_f2(pcn + g * 32 + (i + 1) * 8);
                yk = lds_f2(pcn + 128 + g * 32 + (i + 1) * 8);
            }
        } else if (ph == 2) {
            if constexpr (NS == 1) {
                uint32_t w0 = pk_bf16(e.x, e.y);
                SBO_X3R_PIN(w0);
                nx.h[i] = w0;
            } else {
                uint32_t w0, w1, w2;
                split3(e.x, e.y, w0, w1, w2);
                SBO_X3R_PIN(w0);
                SBO_X3R_PIN(w1);
                nx.h[i] = w0;
                nx.m[i] = w1;
                if constexpr (NS == 3) {
                    SBO_X3R_PIN(w2);
                    nx.l[i] = w2;
                }
            }
        } else {
            if constexpr (MEAN) {
                // the pair's terms in f32 (one rounding of a two-term sum,
                // the order of K*'s own), accumulated in f64
                mu += (double)fmaf(ak.x, e.x, ak.y * e.y);
                SBO_X3R_PIN(mu);
                if (i < 3) ak = lds_f2(pcn + 256 + g * 32 + (i + 1) * 8);
            }
        }
        if (u >= 1 && u <= 2 * NS) dma16(voff, asrc + (u - 1) * kStride, adst + (u - 1) * kStride);
        f32x4 v = h == 0 ? zero : fin[rb];
        if constexpr (P2) {
            v = mfma(a2, kb[h].h, v);
            v = mfma(a1, kb[h].m, v);
            v = mfma(a0, kb[h].l, v);
        }
        if constexpr (P1) {
            v = mfma(a1, kb[h].h, v);
            v = mfma(a0, kb[h].m, v);
        }
        v = mfma(a0, kb[h].h, v);
        fin[rb] = v;
        // interleave: each MFMA followed by two VALU and one LDS read, so the
        // vector work issues in the matrix pipe's shadow (a bf16 MFMA holds
        // the SIMD's issue for 8 of its 16 cycles)
#pragma unroll
        for (int j = 0; j < NPROD; ++j) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);  // VALU
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The tile end, once per tile after the R = 1 body: every block's one f32 add
// of the tile, outer[8 R + rb] += fin[R][rb], R = 0's blocks first.  Written
// on the f32x2 halves, so that with packed f32 enabled for the kernel
// (SBO_X3_PACKED_F32) the 64 adds are 32 v_pk_add_f32: an IEEE add per
// element, the same bits.  No MFMA of this wave runs beside them.
__device__ __forceinline__ void x3_tile_end(f32x4 (&outer)[16], const f32x4 (&fin)[2][8]) {
#pragma unroll
    for (int R = 0; R < 2; ++R)
#pragma unroll
        for (int rb = 0; rb < 8; ++rb) {
            outer[8 * R + rb].lo += fin[R][rb].lo;
            outer[8 * R + rb].hi += fin[R][rb].hi;
        }
}

// K* pieces of one k half directly (the prologue's first tile)
__device__ __forceinline__ void x3_kstar(const lds_char *pc, float xq, float yq, int g, float cexp, bool mean,
                                         KPieces &kb, double &mu) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x2v xk = lds_f2(pc + g * 32 + i * 8), yk = lds_f2(pc + 128 + g * 32 + i * 8);
        const f32x2v ak = lds_f2(pc + 256 + g * 32 + i * 8);
        const float e0 = kstar1(xk.x, yk.x, xq, yq, cexp), e1 = kstar1(xk.y, yk.y, xq, yq, cexp);
        uint32_t w0, w1, w2;
        split3(e0, e1, w0, w1, w2);
        kb.h[i] = w0;
        kb.m[i] = w1;
        kb.l[i] = w2;
        if (mean) mu += (double)fmaf(ak.x, e0, ak.y * e1);  // as in x3_step
    }
}

// a kept tile of the sweep (its step record, decoded): row block, query
// block, flags, precision level, the packed tile's offset in the split
// operand (KiB) and its coordinates' offset in kc3 (floats)
struct XTile {
    int I, qb, flags, lv;
    uint32_t akib, kcf;
};
constexpr int kFirst = 2, kLast = 4, kValid = 8;  // first / last tile of its item

// The persistent sweep: eight waves (two per SIMD), wave w owns queries
// 16w .. 16w+15; every wave loads an eighth of each stage's A planes.
__global__ __launch_bounds__(512, 1) SBO_X3_PACKED_F32 void predict_x3_kernel(
    const char *__restrict__ ax3, const float *__restrict__ kc3, const int4 *__restrict__ desc,
    const int4 *__restrict__ rec, const int *__restrict__ seg, int P, int n_items, int nI, uint32_t a_max,
    const float *__restrict__ qx, const float *__restrict__ qy, int64_t m, int64_t ldp, float cexp, float m0,
    float *__restrict__ part, float *__restrict__ mean) {
    __shared__ __attribute__((aligned(16))) char smem[kXSmem];
    const int bid = blockIdx.x;
    // XCD b % 8 sweeps chunk b % 8 of the plan's XCD-interleaved ranges
    const int rng = (P % 8 == 0) ? (bid % 8) * (P / 8) + bid / 8 : bid;
    const int k0 = max(seg[rng], 0), k1 = min(seg[rng + 1], n_items);
    if (k0 >= k1) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int lw = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave = loader index
    const int g = lane >> 4, r = lane & 15;

    const lds_char *lds = (const lds_char *)smem;
    const int4 *rwin = reinterpret_cast<const int4 *>(smem + kXWin);
    // LDS-DMA with an SGPR base (global_load_lds_dwordx4 v_off, s_base): the
    // only per-lane operand is the byte offset lane*16
    const uint32_t voff = (uint32_t)lane * 16u;
    const uint32_t lds_smem = (uint32_t)(uintptr_t)(lds_char *)(smem);
    const uint32_t lds_wave = lds_smem + (uint32_t)lw * 1024u;
    const uint32_t lds_rwin = lds_smem + (uint32_t)kXWin;
#define SBO_DMA16(sbase, ldst)                                                                          \
    asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"((const void *)(sbase)),     \
                 "{m0}"(ldst)                                                                           \
                 : "memory")
    // the range's step records (plan_rec_kernel: one int4 per kept tile, in
    // sweep order) arrive in 1 KiB LDS windows of kRecWin, one window ahead
#define SBO_REC_WINDOW(w_)                                                                              \
    do {                                                                                                \
        if (lw == 1) SBO_DMA16(reinterpret_cast<const char *>(rec) + (uint64_t)(w_) * 1024u, lds_rwin + (uint32_t)((w_) & 1) * 1024u); \
    } while (0)
    auto tile_at = [&](uint32_t e) {
        const int4 d = rwin[((e / kRecWin) & 1) * kRecWin + e % kRecWin];
        const int rx = __builtin_amdgcn_readfirstlane(d.x), ry = __builtin_amdgcn_readfirstlane(d.y),
                  rz = __builtin_amdgcn_readfirstlane(d.z), rw = __builtin_amdgcn_readfirstlane(d.w);
        XTile t;
        t.I = min(rw & 0xffff, nI - 1);
        t.qb = rz;
        t.flags = ((rw & kRecFirst) ? kFirst : 0) | ((rw & kRecLast) ? kLast : 0) | kValid;
        t.lv = min((rw >> 16) & 3, 2);
        t.akib = min((uint32_t)rx, a_max);
        t.kcf = (uint32_t)ry;
        return t;
    };
    // the range's first and one-past-last list entries
    uint32_t e_rd, e_end;  // e_rd: the entry read last
    {
        const int4 da = desc[k0], db = desc[k1 - 1];
        e_rd = (uint32_t)__builtin_amdgcn_readfirstlane(da.z);
        e_end = (uint32_t)__builtin_amdgcn_readfirstlane(db.z) + (uint32_t)(__builtin_amdgcn_readfirstlane(db.w) & 0xffff);
    }
    SBO_REC_WINDOW(e_rd / kRecWin);
    SBO_REC_WINDOW(e_rd / kRecWin + 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // A tile's coordinates (all 64 k: 1 KiB) go to the coordinate ring and,
    // with an item's first tile, the item's queries (lanes 0-31 qx, 32-63 qy)
    // to the query ring, by wave 0; both rings alternate between two buffers.
    int cw = 0, qw = 0;  // the buffers written next
    auto issue_aux = [&](const XTile &t) {
        const bool first = (t.flags & kFirst) != 0;
        if (lw == 0) {
            if (first) {
                const uint32_t dq = lds_smem + (uint32_t)kXQry + (uint32_t)qw * 1024u;
                if (lane < 32) SBO_DMA16(qx + (int64_t)t.qb * kBN, dq);
                else SBO_DMA16(qy + (int64_t)t.qb * kBN - 128, dq);
            }
            SBO_DMA16(kc3 + t.kcf, lds_smem + (uint32_t)kXCrd + (uint32_t)cw * 1024u);
        }
        if (first) qw ^= 1;
        cw ^= 1;
    };
    // the next entry of the range (flags 0: none left).  Window w + 1 goes
    // into the buffer of window w - 1 once entry 64 w + 1 is read: every wave
    // read that buffer's last entry (64 w - 1) two tiles (four barriers) ago.
    auto read_next = [&]() {
        ++e_rd;
        if (e_rd % kRecWin == 1) SBO_REC_WINDOW(e_rd / kRecWin + 1);
        XTile t = {0, 0, 0, 0, 0, 0};
        if (e_rd < e_end) {
            t = tile_at(e_rd);
            issue_aux(t);
        }
        return t;
    };

    // this wave's share of every A stage starts at a_base (+ the stage's offset)
    const char *a_base = ax3 + lw * 1024;
    const char *a_src = ax3;  // this wave's A pieces of the last staged step
    // the prologue: the first tile's coordinates, queries and both its stages
    // (in a burst), the second tile's coordinates (and queries)
    XTile t0 = tile_at(e_rd);
    issue_aux(t0);
#pragma unroll
    for (int R = 0; R < 2; ++R) {
        const char *s_ = a_base + (uint64_t)(t0.akib + R * (kXA / 1024)) * 1024u;
        const uint32_t w_ = lds_wave + (uint32_t)R * kXSlot;
#pragma unroll
        for (int j = 0; j < kPieces; ++j) SBO_DMA16(s_ + j * kStride, w_ + (uint32_t)(j * kStride));
    }
    XTile t1 = read_next();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // The lane's query in the block, 16 w + (lane & 15): recomputed where it
    // is needed (item starts and ends) from a lane id the compiler cannot
    // hoist, so that it holds no VGPR through the MFMA region.
    auto lane_now = [&]() {
        uint32_t z = 0;
        asm volatile("" : "+v"(z));
        return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
    };
    f32x4 outer[16];
#pragma unroll
    for (int rb = 0; rb < 16; ++rb) outer[rb] = f32x4{};
    f32x4 fin[2][8];
    double mu = 0.0;
    KPieces kb[2], nx[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) nx[h].h = nx[h].m = nx[h].l = u32x4{};
    // the lane's query coordinates of the item whose K* is being built, and
    // the rings' buffers read next
    int cr = 1, qr = 0;
    float xq, yq;
    {
        const lds_char *pq = lds + kXQry;
        const int qo = lw * 16 + r;
        xq = lds_f(pq + qo * 4);
        yq = lds_f(pq + (kBN + qo) * 4);
        qr ^= 1;
        x3_kstar(lds + kXCrd, xq, yq, g, cexp, t0.I == nI - 1, kb[0], mu);
        x3_kstar(lds + kXCrd + 4 * kXH * 4, xq, yq, g, cexp, t0.I == nI - 1, kb[1], mu);
    }
    // deferred outputs of the item finished in the previous step (stored at
    // the top of the next step, before its DMA, so that the vmcnt count at
    // the end of every step is the A pieces of one stage)
    bool pend = false, pend_mean = false;
    float pend_s = 0.0f, pend_mu = 0.0f;
    int pend_qb = 0, pend_I = 0;
    auto flush = [&]() {
        if (pend) {
            const int l = lane_now();
            const int64_t q = (int64_t)pend_qb * kBN + lw * 16 + (l & 15);
            if (l < 16 && q < m) {
                part[(int64_t)pend_I * ldp + q] = pend_s;
                if (pend_mean) mean[q] = pend_mu;
            }
        }
        pend = false;
    };
    int cur = 0;
    bool more = true;
    // one step: row half R of tile t0; items are whole tiles, so the steps
    // alternate R = 0 and R = 1 (which may end an item)
    auto step = [&](auto r_tag) {
        constexpr int R = decltype(r_tag)::value;
        const bool nvalid = (t1.flags & kValid) != 0;
        if (R == 0) {
            flush();
            // this tile may end its item: the item's mean terms are all in
            // (its K* were built during the tile before); close it before
            // the next item's terms start
            if ((t0.flags & kLast) && t0.I == nI - 1) {
                double u = mu;
                u += __shfl_xor(u, 16);
                u += __shfl_xor(u, 32);
                float m0s = m0;
                asm volatile("" : "+v"(m0s));  // (the conversion here, not held in VGPRs through the loop)
                pend_mu = (float)((double)m0s + u);
            }
            if (nvalid && (t1.flags & kFirst)) {
                mu = 0.0;
                const lds_char *pq = lds + kXQry + qr * 1024;
                const int qo = lw * 16 + (lane_now() & 15);
                xq = lds_f(pq + qo * 4);
                yq = lds_f(pq + (kBN + qo) * 4);
                qr ^= 1;
            }
        }
        // the stage two steps ahead: row half R of the next tile, into the
        // slot of the step before this one; with none left, a harmless
        // re-stage of the last staged pieces into that free slot
        const int nslot = cur == 0 ? 2 : cur - 1;  // (cur + 2) % 3
        const uint32_t a_dst = lds_wave + (uint32_t)nslot * kXSlot;
        if (nvalid) a_src = a_base + (uint64_t)(t1.akib + R * (kXA / 1024)) * 1024u;
        XTile t2 = {0, 0, 0, 0, 0, 0};
        if (R == 1) t2 = read_next();  // and its coordinates (queries), one tile ahead of its stages
        const lds_char *pa = lds + cur * kXSlot + lane * 16;
        const lds_char *pcn = lds + kXCrd + cr * 1024 + R * (4 * kXH * 4);
        const bool mn = nvalid && t1.I == nI - 1;
        // the body by the tile's level, the next tile's (the K* pieces it
        // reads) and whether the next tile is in the mean's row block (all
        // uniform: one branch here, none inside the body's MFMA region)
        const int ns = nvalid ? 3 - t1.lv : 1;
#define SBO_X3R_BODY(LV_, NS_, MN_)                                                                              \
    x3_step<R, LV_, NS_, MN_>(pa, pcn, xq, yq, g, cexp, kb, fin[R], nx[R], mu, voff, a_src, a_dst)
#define SBO_X3R_BY_NEXT(LV_)                                                                                     \
    do {                                                                                                        \
        if (mn) {                                                                                               \
            if (ns == 1) SBO_X3R_BODY(LV_, 1, true);                                                            \
            else if (ns == 2) SBO_X3R_BODY(LV_, 2, true);                                                       \
            else SBO_X3R_BODY(LV_, 3, true);                                                                    \
        } else {                                                                                                \
            if (ns == 1) SBO_X3R_BODY(LV_, 1, false);                                                           \
            else if (ns == 2) SBO_X3R_BODY(LV_, 2, false);                                                      \
            else SBO_X3R_BODY(LV_, 3, false);                                                                   \
        }                                                                                                       \
    } while (0)
        if (t0.lv == 2) SBO_X3R_BY_NEXT(2);
        else if (t0.lv == 1) SBO_X3R_BY_NEXT(1);
        else SBO_X3R_BY_NEXT(0);
#undef SBO_X3R_BY_NEXT
#undef SBO_X3R_BODY
        if (R == 1) x3_tile_end(outer, fin);
        if (R == 1 && (t0.flags & kLast)) {
            // item done: column sums of V^2 over its rows (lanes l, l+16, l+32,
            // l+48 hold four row quarters of column l&15 of every block)
            pend = true;
            pend_I = t0.I;
            pend_qb = t0.qb;
            pend_mean = t0.I == nI - 1;
            // four independent f64 chains (element e of every block), then
            // combined: the 64-term sum off one dependent fma chain
            double sq[4] = {};
#pragma unroll
            for (int rb = 0; rb < 16; ++rb)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    sq[e] = fma((double)outer[rb][e], (double)outer[rb][e], sq[e]);
                    outer[rb][e] = 0.0f;
                }
            double sv = (sq[0] + sq[1]) + (sq[2] + sq[3]);
            sv += __shfl_xor(sv, 16);
            sv += __shfl_xor(sv, 32);
            pend_s = (float)sv;
        }
        // Retire stage i + 1.  A wave's vector-memory operations of step i, in
        // issue order: the flush's stores (R = 0), then wave 0's queries and
        // coordinates and wave 1's record window (R = 1), then -- always, an
        // item's or the range's last step included (ns = 1 then) -- the
        // 2 ns A pieces of stage i + 2 from inside the body just run.  So all
        // but the 2 ns youngest done means: stage i + 1's pieces (issued in
        // step i - 1, however many) and this step's coordinates, queries and
        // records have landed, and stage i + 2's pieces stay in flight.
        // (This counts on vmcnt retiring in issue order across kinds: the
        // flush's global stores with the LDS-DMA loads after them, as the
        // k-half kernel before this one did.)
        if (ns == 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else if (ns == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        cur = cur == 2 ? 0 : cur + 1;
        if (R == 1) {
            more = nvalid;
            t0 = t1;
            t1 = t2;
            kb[0] = nx[0];
            kb[1] = nx[1];
            cr ^= 1;
        }
    };
    do {
        step(std::integral_constant<int, 0>{});
        step(std::integral_constant<int, 1>{});
    } while (more);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no LDS-DMA may land after the workgroup ends
    flush();
#undef SBO_REC_WINDOW
#undef SBO_DMA16
}

// Split the f32 packed operand (tiles T0 .. T0+nt-1, tile_offset layout) into
// the three bf16 planes of the row-half layout: tile T, row half R, plane p,
// row block rb of the half, k half h, lane l = 16 g + r holds
// A[16 (8R + rb) + r][32 h + 8 g + j], j = 0..7, at byte
// T*2*kXA + R*kXA + p*kXPlane + (2 rb + h)*1024 + l*16 + 2j.
__global__ __launch_bounds__(256) void pack_x3_kernel(const float *__restrict__ aug, int64_t T0, int64_t nt,
                                                      char *__restrict__ ax3) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= nt * 2048) return;
    const int lane = (int)(id & 63), h = (int)((id >> 6) & 1), rb = (int)((id >> 7) & 7), R = (int)((id >> 10) & 1);
    const int64_t T = T0 + (id >> 11);
    const int row = (8 * R + rb) * 16 + (lane & 15);
    const int k0 = kXH * h + 8 * (lane >> 4);
    const float *src = aug + T * kTileFloats;
    u32x4 w0, w1, w2;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int k = k0 + 2 * d;
        uint32_t a, b, c;
        split3(src[tile_offset(k, row)], src[tile_offset(k + 1, row)], a, b, c);
        w0[d] = a;
        w1[d] = b;
        w2[d] = c;
    }
    char *dst = ax3 + T * (2 * kXA) + R * kXA + (2 * rb + h) * 1024 + lane * 16;
    *reinterpret_cast<u32x4 *>(dst) = w0;
    *reinterpret_cast<u32x4 *>(dst + kXPlane) = w1;
    *reinterpret_cast<u32x4 *>(dst + 2 * kXPlane) = w2;
}

#undef SBO_X3R_PIN
#undef SBO_X3_PACKED_F32

}  // namespace

inline hipError_t launch_pack(hipStream_t s, const float *aug, int64_t T0, int64_t nt, char *ax3) {
    hipLaunchKernelGGL(pack_x3_kernel, dim3((unsigned)((nt * 2048 + 255) / 256)), dim3(256), 0, s, aug, T0, nt, ax3);
    return hipGetLastError();
}

inline hipError_t launch_sweep(hipStream_t s, const char *ax3, const float *kc3, const int4 *desc, const int4 *rec,
                               const int *seg, int P, int n_items, int nI, uint32_t a_max, const float *qx,
                               const float *qy, int64_t m, int64_t ldp, float cexp, float m0, float *part,
                               float *mean) {
    hipLaunchKernelGGL(predict_x3_kernel, dim3((unsigned)P), dim3(512), 0, s, ax3, kc3, desc, rec, seg, P, n_items, nI,
                       a_max, qx, qy, m, ldp, cexp, m0, part, mean);
    return hipGetLastError();
}

}  // namespace x3r
}  // namespace sbo
