// predict_x3.hip -- the predictive sweep (a3+a4) on bf16 MFMA with split
// operands: f32-accurate V = A K*^T at 6/16 of the f32 MFMA cycles.
//
// Every f32 operand value v is split into three bf16 pieces, v = v0 + v1 + v2
// (round to nearest at each step: |v1| <= 2^-8 |v|, |v2| <= 2^-16 |v|, the
// remainder below 2^-24 |v|), and a product a*k is taken as the six terms
//     a2 k0 + a1 k1 + a0 k2 + a1 k0 + a0 k1 + a0 k0
// (smallest first; the dropped a1 k2, a2 k1, a2 k2 are below 2^-23 |a k|,
// the order of an f32 rounding).  Each term is one v_mfma_f32_16x16x32_bf16
// (exact bf16 products, f32 accumulation): 6 x 16 cycles per 16x16x32
// block against 8 x 32 cycles of v_mfma_f32_16x16x4_f32, and unlike the f32
// MFMA, a bf16 MFMA leaves the SIMD's vector issue free for 8 of its 16
// cycles, so the K* chain and its split run in the matrix pipe's shadow.
//
// A = sf2 L^-1 is split once per fit/append/import (pack_x3_kernel, from the
// f32 packed operand); K* is split in registers as it is generated.
//
// Work items, the tick plan and the persistent walk are those of
// predict_kernel (kernels.hip): workgroup = 256 rows x 128 queries, eight
// waves, wave w owns queries 16w..16w+15 and all 256 rows as sixteen 16-row
// MFMA blocks; each 64-k tile is two steps of 128 rows (an LDS stage of
// 3 planes x 128 rows x 64 k bf16 = 48 KiB), every block's MFMA chain starts
// from zero, ends inside its step and is added into an f32 outer sum.  Every
// tile runs at the precision level its plan entry names (six, three or one
// product(s)).
//
// Staging: three LDS slots, stage i+2 issued during step i by LDS-DMA
// (global_load_lds_dwordx4 from inline asm: this wave's A pieces one per
// piece between the MFMAs), retired by a counted vmcnt at the end of step
// i+1; a tile's coordinates, sf2 alpha and an item's 128 query coordinates
// arrive in LDS rings of their own one tile earlier, so the K* of tile t+1 is
// computed during the two steps of tile t, beside their MFMAs.
//
// This is the product build's one code path (SBO_OPT_KERNEL_VARIANT 3, and 22
// = the same kernel over a plan without precision levels).  The kernel and
// the pack of its operand are in predict_x3_rowhalf.hpp, which
// diag/predict_x3_diag.hip includes as well: its variants 3 and 22 are this
// kernel.  Every A/B and timing variant of rounds 1-3 (the DIAG template
// mask: other shapes, stage burst, phase stamps, work left out; on the
// k-half layout) lives there, built only into lib/libsbo_diag.so.
#include <cstdint>
#include <vector>

#include "predict_x3_rowhalf.hpp"

namespace sbo {
namespace {

constexpr int kXH = x3r::kXH;
constexpr int kXA = x3r::kXA;
// the split sweep reads its step records by windows of its own; the plan's
// buffers are padded for plan_format.hpp's
static_assert(x3r::kRecWin == kPlanRecWindow, "the record window the plan pads for");

// Per k-tile coordinates in natural order per half: kc3[t*256 + h*128 + c*32 + i]
// = (x, y, sf2 alpha, 0)[c] of k = 64t + 32h + i, from the kcoord layout
// (k = 4p + g of a tile at g*16 + p).
__global__ void pack_kc3_kernel(const float *__restrict__ kcoord, int64_t nkt, float *__restrict__ kc3) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= nkt * 256) return;
    const int64_t t = id >> 8;
    const int o = (int)(id & 255), h = o >> 7, c = (o >> 5) & 3, i = o & 31;
    const int kk = kXH * h + i;
    kc3[id] = c < 3 ? kcoord[t * (3 * kBK) + c * kBK + (kk & 3) * 16 + (kk >> 2)] : 0.0f;
}

}  // namespace

size_t x3_operand_bytes(int64_t npad) { return (size_t)total_tiles(npad / kBM) * 2 * kXA; }
size_t x3_coord_bytes(int64_t npad) { return (size_t)(npad / kBK) * 256 * sizeof(float); }

hipError_t launch_pack_x3(hipStream_t s, const float *aug, const float *kcoord, int64_t npad, int64_t I0, int wide,
                          char *ax3, float *kc3) {
    if (ax3 && wide != 2) return hipErrorInvalidValue;   // the row-half layout alone (others: the diagnostic build's)
    const int64_t nI = npad / kBM;
    const int64_t T0 = tile_start(I0), T1 = tile_start(nI);
    if (ax3 && T1 > T0) {
        hipError_t e = x3r::launch_pack(s, aug, T0, T1 - T0, ax3);
        if (e != hipSuccess) return e;
    }
    if (!kc3) return hipSuccess;
    const int64_t nkt = npad / kBK;
    hipLaunchKernelGGL(pack_kc3_kernel, dim3((unsigned)((nkt * 256 + 255) / 256)), dim3(256), 0, s, kcoord, nkt, kc3);
    return hipGetLastError();
}

// The product build has no phase stamps (diag/predict_x3_diag.hip): zeros.
hipError_t read_x3_stamps(double *out, int n) {
    for (int j = 0; j < n; ++j) out[j] = 0.0;
    return hipSuccess;
}

hipError_t launch_predict_x3(hipStream_t s, const char *ax3, const float *kc3, const int4 *desc, const int4 *rec,
                             const int *seg, int P, int n_items, int nI, const float *qx, const float *qy, int64_t m,
                             int64_t ldp, float cexp, float m0, float *part, float *mean, int variant) {
    // the largest tile offset a record may name (KiB): keeps every staged address inside ax3
    const int64_t amax = (total_tiles(nI) - 1) * (2 * kXA / 1024);
    if (nI <= 0 || amax > 0xffffffffll) return hipErrorInvalidValue;
    if (variant != 3 && variant != 22) return hipErrorInvalidValue;   // (22: the same kernel, the plan has no levels)
    return x3r::launch_sweep(s, ax3, kc3, desc, rec, seg, P, n_items, nI, (uint32_t)amax, qx, qy, m, ldp, cexp, m0, part,
                             mean);
}

}  // namespace sbo
