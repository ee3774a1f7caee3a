// sbo_internal.hpp -- geometry, device buffers and kernel launchers of
// libsbo.so, shared by the .hip files and the host (the context: sbo_ctx.hpp).
// Not part of the public ABI (include/sbo.h is).
#pragma once

#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sbo.h"
#include "plan_format.hpp"

namespace sbo {

// ---------------------------------------------------------------- geometry
// Predictive operand tiling (see DESIGN.md "predictive sweep").
//   BM rows of A = sf2 * L^-1 per workgroup, BN queries per workgroup
//   (8 waves x 16), BK training points per LDS stage.
constexpr int kBM = 256;
constexpr int kBN = 128;
constexpr int kBK = 64;
constexpr int kTileFloats = kBM * kBK;           // one packed [BK][BM] tile
constexpr int kTilesPerRowBlockStep = kBM / kBK;  // k-tiles added per row block
constexpr int kAcqThreads = 256;
// grid.y / grid.z of a launch stay below the device limit (65535 on gfx950);
// kernels that index columns by blockIdx.y loop over j += gridDim.y
constexpr int64_t kMaxGridY = 65535;

__host__ __device__ inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// First packed tile of row block I: sum_{I'<I} (I'+1)*(BM/BK).
__host__ __device__ inline int64_t tile_start(int64_t I) { return kTilesPerRowBlockStep * I * (I + 1) / 2; }
inline int64_t total_tiles(int64_t nI) { return tile_start(nI); }
// raster-grid query blocks (query_order.hip): kGridPatchFast points along
// the grid's fast axis x kGridPatchSlow rows
constexpr int kGridPatchFast = 8, kGridPatchSlow = 16;
static_assert(kGridPatchFast * kGridPatchSlow == kBN, "a grid patch is one query block");
struct QueryGrid {
    bool ok = false;
    int64_t W = 0, c0 = 0, R = 0, npf = 0, ms = 0;  // row length, first row's column, rows, patches per row, positions
    int64_t nfull = 0, wl = 0;  // whole patch rows; the last rows' patch width (kBN / the next power of two >= R % 16)
};
inline int64_t grid_max_positions(int64_t m) { return round_up(m + m / 8 + kBN, kBN); }
// Element offset inside a packed [BK][BM] tile of A[row][k] (row < BM, k < BK).
// The MFMA is 16x16x4: lane (k&3, row&15) of a k step needs A of the sixteen
// 16-row blocks of its row; blocks 4jj..4jj+3 sit side by side, so four
// conflict-free ds_read_b128 per lane fetch the A operands of all sixteen
// MFMAs of a step.
__host__ __device__ constexpr int tile_offset(int k, int row) {
    return (((row >> 6) * kBK + k) * 16 + (row & 15)) * 4 + ((row >> 4) & 3);
}

// ----------------------------------------------------------- device buffer
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    // Grow-only; contents are NOT preserved on growth.
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap_) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&ptr_, bytes);
        if (e != hipSuccess) { ptr_ = nullptr; return e; }
        cap_ = bytes;
        return hipSuccess;
    }
    void release() {
        if (ptr_) (void)hipFree(ptr_);
        ptr_ = nullptr;
        cap_ = 0;
    }
    template <class T> T *as() const { return static_cast<T *>(ptr_); }
    void swap(DevBuf &o) {
        std::swap(ptr_, o.ptr_);
        std::swap(cap_, o.cap_);
    }
    size_t capacity() const { return cap_; }

private:
    void *ptr_ = nullptr;
    size_t cap_ = 0;
};

// ------------------------------------------------------- streaming tick
// What one sbo_tick_stream reads back before it decides its path, in one copy.
struct StreamHead {
    int mismatch;        // a caller's query differs from the kept one of its sweep position
    int pad;
    double sum_l1sq;     // sum over the new rows r of |L^-1_r|_1^2
    double sum_l1z;      // sum over the new rows r of |L^-1_r|_1 |z_r|
};
// The kept posterior of sbo_tick_stream: state, not workspace (sbo_trim leaves
// it; sbo_stream_reset frees it).  Everything per sweep position is in the
// order tick_order_queries produced for the full sweep that captured it.
struct StreamKeep {
    DevBuf mu64, var64;          // f64 mean and variance (sf2 - sum of partials, unclamped), ms each
    DevBuf qx, qy, perm;         // the ordered queries (f32) and their caller index (int32; -1: padding)
    DevBuf qbox;                 // per 128-position block: bounding box (float4 x0, x1, y0, y1)
    DevBuf l1;                   // the new rows' 1-norms of one update
    DevBuf head;                 // StreamHead, then the kept-tile counter of the last update
    bool valid = false, was_reset = false;
    int64_t m = 0, ms = 0, n_map = 0;   // caller's queries, sweep positions, training rows the state has seen
    uint64_t epoch = 0;          // ctx->fit_epoch at capture
    bool precise = false;        // the sweep that captured it
    double err_var = 0.0, err_mean = 0.0;   // cutoff bounds spent since the last full sweep
    int64_t updates = 0;
    sbo_stream_info last{};      // what the last call did (sbo_get_stream)
    void release() {
        for (DevBuf *b : {&mu64, &var64, &qx, &qy, &perm, &qbox, &l1, &head}) b->release();
        valid = false;
    }
};

// ---------------------------------------------------------- kernel launchers
// All launchers enqueue on `s` and return hipGetLastError().
// K[i + j*ld] = sf2 exp(-|a_i - b_j|^2 / 2l^2) (+ sn2 on i == j when diag).
hipError_t launch_rbf_fill(hipStream_t s, const float *xa, const float *ya, int64_t ma, const float *xb,
                           const float *yb, int64_t mb, int64_t ld, float ell, float sf2, float sn2, bool diag,
                           float *K);
hipError_t launch_sub_scalar(hipStream_t s, const float *in, float v, int64_t n, float *out);
hipError_t launch_copy_lower(hipStream_t s, const float *src, int64_t ld_src, int64_t n,
                             float *dst, int64_t ld_dst);
// The fit-side operand build (csrc/operand.hip): what a refresh derives from
// L^-1 (lower, column-major) and the points; per row block for the row blocks
// I >= I0 (earlier row blocks are left as they are), per k-tile whole.
// The per-k-tile coordinates and sf2 * alpha for all k
hipError_t launch_pack_kcoord(hipStream_t s, const float *x, const float *y, const float *alpha, int64_t n,
                              int64_t npad, double sf2, float *kcoord);
// The f32 inverse: A = sf2 * L^-1 into [BK][BM] tiles, and the coordinates
hipError_t launch_pack_operand(hipStream_t s, const float *Linv, int64_t ld, int64_t n, int64_t npad, int64_t I0,
                               double sf2, const float *x, const float *y, const float *alpha, float *aug,
                               float *kcoord);
// lgn[2 (tile_start(I) + t)] = log2 bounds (16 max row 1-norm, spectral,
// Frobenius) of A_It, lgn[2 (..) + 1] = (16 max row 1-norm, spectral) of its
// bf16 pieces A1 and A2 (f64 sums, rounded up; -1000 for an all-zero matrix).
hipError_t launch_tile_norms(hipStream_t s, const float *aug, int64_t npad, int64_t I0, float4 *lgn);
// The f64 inverse: its tiles packed and their norms taken in one pass over L^-1
hipError_t launch_pack_tile_norms(hipStream_t s, const double *Linv, int64_t ld, int64_t n, int64_t npad, int64_t I0,
                                  double sf2, float *aug, float4 *lgn);
// row_l1[i] = sum_j |A_ij| over the packed operand (f64)
hipError_t launch_row_l1(hipStream_t s, const float *aug, int64_t npad, int64_t I0, double *row_l1);
// Per k-tile bounding boxes of the (internally ordered) training points
hipError_t launch_tile_boxes(hipStream_t s, const float *x, const float *y, int64_t n, int64_t npad,
                             float4 *kbox);
// colmax[t], t < npad / kBK: the largest lgn[2 (tile_start(I) + t)].x over the row blocks I that hold k-tile t
hipError_t launch_tile_colmax(hipStream_t s, const float4 *lgn, int64_t npad, float *colmax);
// dst (m x n, f64, ld_dst) = src (f32, ld_src); lower: zero above the diagonal.
hipError_t launch_widen(hipStream_t s, const float *src, int64_t ld_src, int64_t m, int64_t n, bool lower,
                        double *dst, int64_t ld_dst);
// Predictive sweep: part[I][q] = sum over rows of block I of (sf2 L^-1 k_q)^2,
// mean[q] = m0 + sf2 alpha^T k_q.
// Tile cutoff (SkipPlan).  With a tile-norm table (automatic cutoff, one row
// block per workgroup) a workgroup (row block I, query block) bounds tile t's
// share of |dV_I(q)|_2 by 2^(lgn[t]) * K*max(box distance) and drops tiles
// smallest bound first while the dropped bounds sum to at most 2^lg_tau_v
// (binned, fixed point: order-independent); otherwise it drops tile t when
// every K* entry is below 2^-L.  The last row block (which also accumulates
// the mean) keeps every tile within 2^-L_mean.  L >= 150 drops only exact
// zeros (bitwise identical to the dense sweep); L = 0: dense.
// tiles_done (may be null): [0] += number of (BM x BN x BK) tiles multiplied,
// [1] += MFMA products issued on them (prod_full per full tile, 3 / 1 per
// tile at the reduced levels).
struct SkipPlan {
    int L = 0;                  // 0: dense
    int L_mean = 0;             // last row block; <= L means "same as L"
    const float4 *lgn = nullptr;   // per packed tile log2 gain bounds (null: distance test only)
    const float *kcoord = nullptr; // per k-tile coordinates (the |k|_2 bound of the tile-norm test)
    float lg_tau_v = 0.0f;
    int levels = 0;     // with lgn: tiles may run at the reduced precision levels (split sweep)
    int prod_full = 1;  // MFMA products per full-precision tile (6: split sweep), for the counter
    bool records = false;  // also write the split sweep's step records (plan_views' rec)
    bool wide = false;     // empty items' outputs as f64 (the precise sweep's partials and mean)
    int order_blk = 0;     // item order: 0 row-block-major, else blocks of (bi << 8 | bq) -- plan_item
    // with lgn: per k-tile max over row blocks of lgn[..].x (launch_tile_colmax), the plan's
    // column prefilter; null: every (row block, k-tile) pair is tested on its own
    const float *colmax = nullptr;
    // write an empty item's partial (0) instead of leaving it to the acquisition to skip
    // (launch_acquire's nonempty): for plans that do not live until then
    bool zero_empty = false;
    // diagnostic build's reference: cnt2 cleared by a memset, as before plan_perm wrote every position
    bool ref_chain = false;
    // rank of a tile's two level increments against drops: log2(time a drop
    // saves / time the level step saves), per-tile sweep time at C4 of six,
    // three, one product(s) 18.6, 12.9, 9.9 ns (variants 22, 20, 21)
    float lvl_key[2] = {0.80f, 1.72f};
};
// The tick's plan (which k-tiles each (row block, query block) item runs,
// non-empty items in row-block-major order, one balanced item range per
// sweep workgroup) in `work` (predict_work_bytes); empty items' outputs are
// written here.  P = sweep workgroups (one per CU).
size_t predict_work_bytes(int64_t npad, int64_t m, int P);
hipError_t launch_plan(hipStream_t s, const float4 *kbox, int64_t npad, const float *qx, const float *qy, int64_t m,
                       int64_t ldp, float ell, float m0, const SkipPlan &skip, float *part, float *mean,
                       unsigned long long *tiles_done, int P, void *work, size_t work_bytes);
// The sweep over the plan in `work` (persistent, P workgroups).
hipError_t launch_predict(hipStream_t s, const float *aug, const float *kcoord, int64_t npad, const float *qx,
                          const float *qy, int64_t m, int64_t ldp, float ell, float m0, float *part, float *mean,
                          int variant, int P, const void *work);
// exp2 coefficient of the RBF kernel: k = exp2(cexp d^2), cexp = -1/(2 l^2 ln 2)
float exp2_coef_f(float ell);
// Per-query sweep work of the plan in `work` (kept k-tiles of the query's
// block summed over row blocks / block size), in the caller's order.
// bcost: (m + kBN - 1) / kBN floats of scratch.
hipError_t launch_plan_cost(hipStream_t s, int64_t npad, int64_t m, int P, const void *work, const int32_t *perm,
                            float *bcost, float *cost);
// The plan's descriptors, tile lists and per-workgroup ranges inside `work`.
void plan_views(int64_t npad, int64_t m, int P, const void *work, const int4 **desc, const unsigned short **tl,
                const int **seg, const int4 **rec = nullptr);
// Per item of the plan in `work` (index: plan_item order, row-block-major for
// order_blk 0: (nI - 1 - I) * nQ + qb): the plan key (plan_key_pack), its
// inclusive scan, and the budget threshold + 1.
// nonempty (may be null): per query block (nI + 63) / 64 words, bit I set when
// item (I, qb) keeps a tile (launch_acquire).
void plan_item_views(int64_t npad, int64_t m, int P, const void *work, const unsigned long long **key,
                     const unsigned long long **scan, const unsigned char **thr,
                     const unsigned long long **nonempty = nullptr);
// Split-operand (bf16 x3) predictive sweep, predict_x3.hip: the packed
// operand split into three bf16 planes per row half of a tile (48 KiB stages,
// predict_x3_rowhalf.hpp) and the per-k-tile coordinates in natural order,
// for row blocks >= I0 (coordinates: all).
size_t x3_operand_bytes(int64_t npad);
size_t x3_coord_bytes(int64_t npad);
// (ax3 null: the coordinates only; kc3 null: the planes only)
hipError_t launch_pack_x3(hipStream_t s, const float *aug, const float *kcoord, int64_t npad, int64_t I0, int layout,
                          char *ax3, float *kc3);
// (the plan's descriptors, tile-list entries, keys and the split sweep's step
// records: plan_format.hpp)
__host__ __device__ inline int4 plan_item_int4(int I, int qb, uint64_t off, int cnt) {
    const PlanItemWords p = plan_item_pack(I, qb, off, cnt);
    return make_int4(p.x, p.y, p.z, p.w);
}
// the split sweeps that honour the plan's precision levels
inline bool x3_levels(int variant) { return variant == 3 || variant == 23 || variant == 24 || variant == 30 || variant == 32 || variant == 33 || variant == 39 || variant == 41 || variant == 42 || variant == 43 || variant == 46 || variant == 47 || variant == 48 || variant == 49 || variant == 51 || variant == 52 || variant == 53 || variant == 54 || variant == 55 || variant == 56 || variant == 57 || (variant >= 58 && variant <= 62); }
// Sweeps the product library accepts (all compute the full result; 3 is the
// default).  The timing diagnostics (parts of the work left out, forced
// precision levels, phase stamps) exist only in the diagnostic build
// (-DSBO_DIAG, lib/libsbo_diag.so, selected by SBO_LIB for tools/).
inline bool variant_allowed(int v) {
#ifdef SBO_DIAG
    return v >= 0 && v <= 62;
#else
    return v == 0 || v == 1 || v == 3 || v == 22;
#endif
}
// the split operand's layout a kernel variant reads (2: row-half stages, the product's; 0: k-half stages and
// 1: the wide 32x32x16 shape, the diagnostic build's other variants)
inline int x3_layout(int variant) { return (variant == 13 || variant == 14) ? 1 : (variant == 3 || variant == 22) ? 2 : 0; }
// The sweep over the plan with the split operand; qx/qy must be readable in
// whole 128-query blocks (padded to round_up(m, kBN)).  variant: 3 (the
// default, honouring the plan's precision levels) or 22 (every kept tile at
// six products); the diagnostic build's timing variants go through
// csrc/diag/predict_x3_diag.hip.
// Diagnostic build (SBO_OPT_KERNEL_VARIANT 39): summed phase cycles of the
// split sweep since the last read (see g_x3_stamps), then reset.
hipError_t read_x3_stamps(double *out, int n);
hipError_t launch_predict_x3(hipStream_t s, const char *ax3, const float *kc3, const int4 *desc, const int4 *rec,
                             const int *seg, int P, int n_items, int nI, const float *qx, const float *qy, int64_t m,
                             int64_t ldp, float cexp, float m0, float *part, float *mean, int variant);
// Blocked Cholesky, the chain (csrc/chol_chain.hip): factor the kb x kb
// diagonal block at A (column-major, lda = ld) of step k0 in place (kb <=
// kCholNB); info as rocSOLVER's.
constexpr int kCholNB = 128;
// version (SBO_OPT_CHOL_DIAG) 1: left-looking MFMA (default), 2: right-looking MFMA, 0: VALU; bitwise equal
hipError_t launch_chol_diag(hipStream_t s, float *A, int64_t ld, int kb, int64_t k0, int *info, int version = 1);
// C -= P Q^T over 128 x 128 tiles (lower: the tiles on and below the diagonal of an m x m C), f32, lda ld, K columns
hipError_t launch_chol_update(hipStream_t s, const float *P, const float *Q, int64_t ld, int64_t m, int64_t nc,
                              int64_t K, bool lower, float *C);
// SBO_OPT_CHOL_GEMM 3 (csrc/chol_x3.hip): the outer panel P (m x K f32, lda ld,
// K a multiple of 32) into three bf16 planes in MFMA fragment order
// (chol_x3_bytes), then C (rows x cols, lda ld) -= P[r0 ..] P[c0 ..]^T on the bf16
// matrix cores with six split products per f32 product (lower: the tiles on and
// below the diagonal of a square region with r0 == c0)
size_t chol_x3_bytes(int64_t m, int64_t K);
hipError_t launch_chol_split(hipStream_t s, const float *P, int64_t ld, int64_t m, int64_t K, char *planes);
hipError_t launch_chol_update_x3(hipStream_t s, const char *planes, int64_t m, int64_t K, int64_t r0, int64_t rows,
                                 int64_t c0, int64_t cols, bool lower, float *C, int64_t ld);
// The panel below it (csrc/chol_chain.hip): A21 (m2 x kb, lda ld) := A21 L11^-T (forward substitution, f32);
// version as launch_chol_diag's
hipError_t launch_chol_trsm(hipStream_t s, const float *L11, int64_t ld, int kb, float *A21, int64_t m2, int version = 1);
// sbo_remove (csrc/remove.hip): a point leaves the factor and the f64 inverse
// by Givens rotations.  The chain's workspace for n points: the f64 carry
// column w, the rotations' (c_k, s_k) at coef[2k], the failed-pivot flag
// (zeroed by the caller), and the kept stored positions (n1 of them,
// ascending) for the compaction.
struct RemoveWork {
    double *w = nullptr, *coef = nullptr;
    int *flag = nullptr, *keep = nullptr;
};
size_t remove_work_bytes(int64_t n);
RemoveWork remove_work(void *base, int64_t n);
// the compaction's staging of the elements that move (n1 points left, f the smallest removed position)
size_t remove_compact_bytes(int64_t n1, int64_t f);
// Stored position i (of n, dead rows and columns of earlier chains included)
// out of the factor: the f32 L in place (W null), or the f64 copy W of its
// columns from wcol0 on (same ld; column c at W + (c - wcol0) ld).  One
// diagonal and one panel launch per 128 columns right of i.
hipError_t launch_remove_chain(hipStream_t s, float *L, double *W, int64_t ld, int64_t wcol0, int64_t n, int64_t i,
                               const RemoveWork &wk);
// The same rotations (wk.coef) applied to rows i+1 .. n-1 of X with row i as the carry
hipError_t launch_remove_rows(hipStream_t s, double *X, int64_t ld, int64_t n, int64_t i, const RemoveWork &wk);
// The kept rows and columns (wk.keep) of L (columns from wcol0 on rounded from
// W when there is one), X and the points moved to positions 0 .. n1-1; only
// positions >= f move, through ws (remove_compact_bytes)
hipError_t launch_remove_compact(hipStream_t s, float *L, const double *W, int64_t wcol0, double *X, int64_t ld,
                                 float *x, float *y, float *obs, int64_t n1, int64_t f, const RemoveWork &wk, void *ws);
// d = (double)in - v;  out = (float)d
hipError_t launch_widen_sub(hipStream_t s, const float *in, double v, int64_t n, double *d);
// alpha = X^T X (obs - m0) from the f64 inverse X (lower, lda ld), z = X (obs -
// m0) kept; work: alpha_work_bytes(n) (the first pass's per-chunk partials)
size_t alpha_work_bytes(int64_t n);
hipError_t launch_alpha_f64(hipStream_t s, const double *X, int64_t ld, int64_t n, const float *obs, double m0,
                            double *z, double *alpha, double *work);
hipError_t launch_narrow(hipStream_t s, const double *d, int64_t n, float *out);
// out[r] = sum_c A[r + c ld] x[c] (c < n) for rows r < rows of a column-major f64 matrix
hipError_t launch_row_dot(hipStream_t s, const double *A, int64_t ld, int64_t rows, int64_t n, const double *x,
                          double *out);
// out[i + j ldo] = (float)d[i + j ldd], i < m, j < n
hipError_t launch_narrow_2d(hipStream_t s, const double *d, int64_t ldd, int64_t m, int64_t n, float *out,
                            int64_t ldo);
// out[j * stride] = (float)d[j], j < n
hipError_t launch_narrow_strided(hipStream_t s, const double *d, int64_t n, float *out, int64_t stride);
// Acquisition over predictive partials (fused reduce + sets + block argmax).
// perm (may be null): sweep position i holds caller query perm[i]; outputs and
// key indices are written in the caller's order.  nonempty (may be null): the
// non-empty items of the plan the partials were swept under (plan_item_views):
// the partial of an empty item is not read (SkipPlan::zero_empty).
// keep_mu / keep_var (may be null): the streaming tick's capture, per sweep
// position the mean widened to f64 and sf2 - the summed partials before the
// clamp at zero; the other outputs do not depend on them.
hipError_t launch_acquire(hipStream_t s, const float *part, const float *mean, int nI, int64_t ldp,
                          int64_t m, float sf2, double beta, double f_min, int score_kind,
                          int64_t index_offset, const int32_t *perm, float *mu, float *sd, double *lo,
                          double *hi, uint8_t *safe, sbo_key *block_keys,
                          const unsigned long long *nonempty = nullptr, double *keep_mu = nullptr,
                          double *keep_var = nullptr);
// the same over the precise sweep's f64 partials and mean (sf2 in f64)
hipError_t launch_acquire(hipStream_t s, const double *part, const double *mean, int nI, int64_t ldp,
                          int64_t m, double sf2, double beta, double f_min, int score_kind,
                          int64_t index_offset, const int32_t *perm, float *mu, float *sd, double *lo,
                          double *hi, uint8_t *safe, sbo_key *block_keys,
                          const unsigned long long *nonempty = nullptr, double *keep_mu = nullptr,
                          double *keep_var = nullptr);
// Acquisition from a kept posterior (sbo_tick_stream's update path): per sweep
// position mu = (float)mu64, sd = sqrt((float)max(var64, 0)), then the sets
// and the block argmax exactly as launch_acquire's; perm as there (never null).
hipError_t launch_acquire_kept(hipStream_t s, const double *mu64, const double *var64, int64_t ms, double beta,
                               double f_min, int score_kind, int64_t index_offset, const int32_t *perm, float *mu,
                               float *sd, double *lo, double *hi, uint8_t *safe, sbo_key *block_keys);
// Streaming tick (predict_update.hip).  launch_stream_keep: the sweep order of
// a full tick copied into the kept buffers (perm null: identity) and each
// 128-position block's bounding box.  launch_stream_compare: head->mismatch
// |= 1 when a caller's query is not bitwise the kept one (head zeroed by the
// caller).  launch_update_bound_sums: the 1-norms of rows n_map .. n - 1 of
// the f64 inverse (l1: scratch of update_l1_bytes) and the two sums of StreamHead.
// launch_predict_update: the rank-(n - n_map) update of mu64 / var64 in place;
// skip_L 0: dense, else tiles whose K* entries are all below 2^-skip_L are
// skipped; *tiles_kept += the (query block, k-tile) pairs multiplied.
// launch_stream_scatter: the kept state in the caller's order.
hipError_t launch_stream_keep(hipStream_t s, const float *qx, const float *qy, const int32_t *perm, int64_t ms,
                              float *kqx, float *kqy, int32_t *kperm, float4 *qbox);
hipError_t launch_stream_compare(hipStream_t s, const float *qx, const float *qy, const float *kqx, const float *kqy,
                                 const int32_t *kperm, int64_t ms, StreamHead *head);
size_t update_l1_bytes(int64_t R);   // launch_update_bound_sums' l1 scratch for R new rows
hipError_t launch_update_bound_sums(hipStream_t s, const double *Linv, int64_t ld, int64_t n_map, int64_t n,
                                    const double *z, double *l1, StreamHead *head);
hipError_t launch_predict_update(hipStream_t s, const double *Linv, int64_t ld, int64_t n_map, int64_t n,
                                 const double *z, const float *x, const float *y, const float4 *kbox,
                                 const float4 *qbox, const float *kqx, const float *kqy, const int32_t *kperm,
                                 int64_t ms, double ell, double sf2, int skip_L, double *mu64, double *var64,
                                 unsigned long long *tiles_kept);
hipError_t launch_stream_scatter(hipStream_t s, const double *mu64, const double *var64, const int32_t *kperm,
                                 int64_t ms, double *mu_out, double *var_out);
// What-if posterior (whatif.hip, sbo_whatif), pp = p rounded up to 16.
// launch_whatif_fill: Kt = K_c^T (pp x n column-major, padding rows zero).
// launch_whatif_stats: from U^T and W^T (pp x n each) the candidates' mu_c,
// var_c, |w_j|_1 and the sweep's per-candidate factors cpar (2 pp doubles:
// beta sd_c / d_j, 1 / d_j, d_j = var_c + noise); part: scratch of
// whatif_part_bytes(pp).  launch_whatif: the sweep over the kept posterior --
// gain[j] += candidate j's newly safe positions (zeroed by the caller), cov /
// lo_new (p x m row-major, the caller's query order; either may be null),
// *tiles_kept += the (query block, k-tile) pairs multiplied; skip_L as
// launch_predict_update's.  whatif_cutoff (host): the auto cutoff L and its
// bound on |cov error| (whatif_err_cov of the largest |w_j|_1).
size_t whatif_part_bytes(int64_t pp);
hipError_t launch_whatif_fill(hipStream_t s, const float *x, const float *y, int64_t n, const float *cx,
                              const float *cy, int64_t p, int64_t pp, double ell, double sf2, double *Kt);
hipError_t launch_whatif_stats(hipStream_t s, const double *Ut, const double *Wt, int64_t p, int64_t pp, int64_t n,
                               const double *z, double m0, double sf2, double noise, double beta, double *part,
                               double *cand_mu, double *cand_var, double *w_l1, double *cpar);
hipError_t launch_whatif(hipStream_t s, const double *Wt, int64_t pp, int64_t p, int64_t n, const float *x,
                         const float *y, const float4 *kbox, const float4 *qbox, const float *kqx, const float *kqy,
                         const int32_t *kperm, int64_t ms, int64_t m, double ell, double sf2, int skip_L,
                         const double *mu64, const double *var64, const float *cx, const float *cy, const double *cpar,
                         double beta, double f_min, unsigned long long *gain, double *cov, double *lo_new,
                         unsigned long long *tiles_kept);
void whatif_cutoff(int64_t p, const double *w_l1, const double *cand_var, double s, double beta, double sf2,
                   double budget_var, double budget_mean, int *L_out, double *err_cov);
double whatif_err_cov(int L, double sf2, double l1max);
// Posterior sample paths (sample.hip, sbo_sample), pp = samples rounded up to
// 16, Fp = features rounded up to 4.  launch_sample_draw: the frequencies
// (wx, wy: Fp each, in turns), Theta^T (pp x 2 Fp column-major, times
// -sf / sqrt(F)) and T^T = sqrt(noise) eps (ldw x n column-major, ldw >= pp,
// the rows from S on zero; order: the rows' caller indices on the device) of samples first .. first + S - 1 from
// the streams seed, seed + 1, seed + 2; Theta / Tt may be null, and raw_nu
// (2 F), raw_ab (S x 2 F), raw_eps (S x n, the caller's training order) take
// the standard normals themselves when not null.  launch_sample_train:
// T^T += g(train).  launch_sample_kernel_err: *out (zeroed by the caller) =
// the bits of the feature kernel's largest error on the lattice.
// launch_sample: the sweep over the kept posterior -- count[j] += the positions
// with path_j > f_min (zeroed by the caller), paths (S x m row-major, the
// caller's query order; may be null), pkeys: S x sample_blocks(ms) partial keys,
// keys[j] = the argmax of path_j over the safe positions with index_offset
// added; skip_L and tiles_kept as launch_whatif's.  sample_cutoff (host): the
// auto cutoff L and its bound on |path error| (whatif_err_cov of the largest
// |w_j|_1).
hipError_t launch_sample_draw(hipStream_t s, uint64_t seed, int64_t first, int64_t S, int64_t pp, int64_t ldw, int64_t F,
                              int64_t Fp, int64_t n, const int64_t *order, double ell, double sf, double noise, double *wx,
                              double *wy, double *Theta, double *Tt, double *raw_nu, double *raw_ab, double *raw_eps);
hipError_t launch_sample_train(hipStream_t s, const double *Theta, int64_t pp, int64_t n, const float *x,
                               const float *y, const double *wx, const double *wy, int64_t Fp, double cx0, double cy0,
                               double *Tt, int64_t ldw);
hipError_t launch_sample_kernel_err(hipStream_t s, const double *wx, const double *wy, int64_t F, double ell,
                                    unsigned long long *out);
int64_t sample_blocks(int64_t ms);
hipError_t launch_sample(hipStream_t s, const double *Wt, int64_t ldw, const double *Theta, int64_t pp, int64_t S, int64_t n,
                         const float *x, const float *y, const float4 *kbox, const float4 *qbox, const float *kqx,
                         const float *kqy, const int32_t *kperm, int64_t ms, int64_t m, double ell, double sf2,
                         int skip_L, const double *mu64, const double *var64, const double *wx, const double *wy,
                         int64_t Fp, double cx0, double cy0, double beta, double f_min, int64_t index_offset,
                         unsigned long long *count, double *paths, sbo_key *pkeys, sbo_key *keys,
                         unsigned long long *tiles_kept);
void sample_cutoff(int64_t S, const double *w_l1, double sf2, double budget_mean, int *L_out, double *err_path);
// Precise sweep (predict_f64.hip, SBO_OPT_PRECISION): A = sf2 L^-1 packed in
// f64 from the fit's f64 inverse for row blocks >= I0 (tile (I, t) at
// tile_start(I) + t, two 64 KiB stages in MFMA fragment order), and per k-tile
// half the f64 x, y, sf2 alpha (alpha from the f64 solve).
size_t f64_operand_bytes(int64_t npad);
size_t f64_coord_bytes(int64_t npad);
hipError_t launch_pack_f64(hipStream_t s, const double *Linv, int64_t ld, int64_t n, int64_t npad, int64_t I0,
                           double sf2, const float *x, const float *y, const double *alpha, double *a64,
                           double *kc64);
// The sweep over the plan (descriptors and tile lists of plan_views; every
// kept tile in f64): part[I][q] (f64) = sum over row block I of V^2, mean[q]
// (f64) = m0 + sf2 alpha^T k_q.
hipError_t launch_predict_f64(hipStream_t s, const double *a64, const double *kc64, const int4 *desc,
                              const unsigned short *tl, const int *seg, int P, int n_items, int nI, const float *qx,
                              const float *qy, int64_t m, int64_t ldp, double ell, double m0, double *part,
                              double *mean);
// The int8 sliced precise sweep (predict_oz.hip, SBO_OPT_PRECISE_KERNEL 1):
// A = sf2 L^-1 from the fit's f64 inverse as five balanced base-256 int8
// digit slices per 16-row block and k-tile (80 KiB per packed tile) with a
// power-of-two exponent per block (oz_exp_bytes: 16 int32 per tile), per
// k-tile x, y (f64 and f32) and sf2 alpha (f64).  The sweep reads the same plan as launch_predict_f64 and
// writes the same f64 partials and mean.
size_t oz_operand_bytes(int64_t npad);
size_t oz_exp_bytes(int64_t npad);
size_t oz_coord_bytes(int64_t npad);
hipError_t launch_pack_oz(hipStream_t s, const double *Linv, int64_t ld, int64_t n, int64_t npad, int64_t I0,
                          double sf2, const float *x, const float *y, const double *alpha, char *aoz, int *eoz,
                          char *koz, bool pairs = false);
hipError_t launch_predict_oz(hipStream_t s, const char *aoz, const int *eoz, const char *koz, const int4 *desc,
                             const unsigned short *tl, const int *seg, int P, int n_items, int nI, const float *qx,
                             const float *qy, int64_t m, int64_t ldp, double ell, double m0, double *part,
                             double *mean, int variant = 1, const char *kzt = nullptr);
// The K* table (SBO_OPT_PRECISE_KERNEL 3): bytes per query block, and the
// table of nq query blocks of the queries qx/qy (m of them) for every k-tile.
// pairs (SBO_OPT_PRECISE_KERNEL 4): exponents shared by k-tile pairs (2p,
// 2p + 1) -- the operand (launch_pack_oz), the table and the sweep (variant 4)
size_t oz_table_bytes(int64_t npad, bool pairs = false);
hipError_t launch_kstar_table(hipStream_t s, const char *koz, const float *qx, const float *qy, int64_t m,
                              int64_t npad, double ell, int64_t nq, char *kzt, bool pairs = false);
// The int8-sliced f64 GEMM (ozgemm.hip): C (m x n, ldc) = alpha op(A) op(B)
// (+ C), column-major f64, op(A) m x K (A itself K x m with kGzTransA), op(B)
// K x n (n x K with kGzTransB); a triangular operand's zero part is not read;
// kGzTransC stores C^T (C then points at n x m storage, ldc its leading
// dimension); nd digits (5, 6); K <= 16384; workspace of
// gz_workspace_bytes(m, n, K, nd).
constexpr unsigned kGzTriA = 1;        // op(A) lower triangular: a_ik = 0 for k > i
constexpr unsigned kGzTransA = 2;
constexpr unsigned kGzTriBLower = 4;   // op(B) lower triangular: b_kj = 0 for k < j
constexpr unsigned kGzTriBUpper = 8;   // op(B) upper triangular: b_kj = 0 for k > j
constexpr unsigned kGzTransB = 16;
constexpr unsigned kGzTransC = 32;
constexpr unsigned kGzBeta1 = 64;      // C += instead of C =
constexpr unsigned kGzLowerC = 128;    // (f32 form) only tiles that meet C's lower triangle
size_t gz_workspace_bytes(int64_t m, int64_t n, int64_t K, int nd);
hipError_t launch_gz_gemm(hipStream_t s, int nd, const double *A, int64_t lda, const double *B, int64_t ldb,
                          int64_t m, int64_t n, int64_t K, double alpha, double *C, int64_t ldc, unsigned flags,
                          char *ws);
// The same product on f32 operands and an f32 C (4 or 5 digits: the Cholesky's
// updates, SBO_OPT_CHOL_GEMM 4 / 5); kGzLowerC skips the tiles above C's diagonal.
hipError_t launch_gz_gemm_f32(hipStream_t s, int nd, const float *A, int64_t lda, const float *B, int64_t ldb,
                              int64_t m, int64_t n, int64_t K, double alpha, float *C, int64_t ldc, unsigned flags,
                              char *ws);
// ... and with one pack of the panel's m rows shared by every product of an
// outer step: op(A) its rows a0 .., op(B)^T its rows b0 .. (multiples of 128)
size_t gz_pack_bytes(int64_t m, int64_t K, int nd);
hipError_t launch_gz_pack_f32(hipStream_t s, int nd, const float *P, int64_t ld, int64_t m, int64_t K, char *pack);
hipError_t launch_gz_gemm_packed_f32(hipStream_t s, int nd, const char *pack, int64_t mpack, int64_t K, int64_t a0,
                                     int64_t m, int64_t b0, int64_t n, double alpha, float *C, int64_t ldc,
                                     unsigned flags);
// The fit's accuracy guard of the f64 inverse (inv_check.hip): on kChkQ - 1
// queries (coordinates at *qxy: x[kChkQ] then y[kChkQ], filled by the caller
// before the launch) plus the residual r = obs - m0 as the last right-hand
// side, V0 = Linv Kq and one refinement against the f32 factor L, dV = Linv
// (Kq - L V0), both lower-triangular column-major with lda ld; *colsums = per
// query column (sum dV (2 V0 + dV), sum (V0 + dV)^2, sum V0 z0, sum V0 dz +
// dV z0 + dV dz) with z0 / dz the residual's columns.  work:
// inv_check_bytes(n); with Linv null only the pointers are set.
constexpr int kChkQ = 32;
int64_t inv_check_rows(int64_t n);
size_t inv_check_bytes(int64_t n);
hipError_t launch_inv_check(hipStream_t s, const double *Linv, const float *L, int64_t ld, int64_t n,
                            const float *x, const float *y, const float *obs, double m0, double sf2, double ell,
                            void *work, float **qxy, double **colsums);
// Morton ordering of the queries (query_order.hip): workspace of
// query_order_bytes(m); returns the permutation and the gathered coordinates
// (all inside the workspace).
size_t query_order_bytes(int64_t m);
hipError_t launch_query_order(hipStream_t s, const float *qx, const float *qy, int64_t m, const float bbox[4],
                              void *work, size_t work_bytes, int32_t **perm, float **sqx, float **sqy);
// Raster-grid queries (query_order.hip): blocks of kGridPatchFast points
// along the grid's fast axis x kGridPatchSlow rows, patches in raster order,
// padded positions with perm = -1.  launch_grid_detect (workspace
// query_grid_bytes(m), synchronizes the stream) reads the raster's shape;
// grid_layout turns it into a layout (false: not a raster, or more padding
// than grid_max_positions allows -- Morton then); launch_query_grid
// gathers the q.ms sweep positions.
size_t query_grid_bytes(int64_t m);
hipError_t launch_grid_detect(hipStream_t s, const float *qx, const float *qy, int64_t m, void *work,
                              unsigned long long host_g[6]);
bool grid_layout(const unsigned long long g[6], int64_t m, QueryGrid &q);
hipError_t launch_query_grid(hipStream_t s, const float *qx, const float *qy, int64_t m, const QueryGrid &q,
                             void *work, int32_t **perm, float **sqx, float **sqy);
// ComputeSets from given mu/sd (staged API).
hipError_t launch_sets(hipStream_t s, const float *mu, const float *sd, int64_t m, double beta,
                       double f_min, double *lo, double *hi, uint8_t *safe);
hipError_t launch_sets(hipStream_t s, const double *mu, const double *sd, int64_t m, double beta,
                       double f_min, double *lo, double *hi, uint8_t *safe);
// Masked argmax over f64 scores -> block keys.
hipError_t launch_argmax_blocks(hipStream_t s, const double *score, const uint8_t *mask, int64_t m,
                                int64_t index_offset, sbo_key *block_keys);
// Reduce nblocks keys into *out (device pointer).
hipError_t launch_reduce_keys(hipStream_t s, const sbo_key *keys, int64_t nblocks, sbo_key *out);

// Model evidence (evidence.hip).  launch_evidence_norms: c[i] = (K^-1)_ii =
// sum_{k >= i} X_ki^2 from the f64 inverse X (lower, lda ld), and per 64-point
// k-tile t the kEvSums sums at sums[t kEvSums ..]: |alpha|, sqrt(c), c, alpha^2,
// alpha r, alpha, log L_ii (L: the f32 factor, lda ldl), z^2 and the LOO log
// predictive, r = obs - m0.  launch_evidence_loo: y_i - alpha_i / c_i and 1 / c_i
// at order[i] (device array; either output may be null).  launch_evidence_gram:
// per item (int4: k-tile I, k-tile J >= I, first row k0, k0 == 64 J) the
// contraction of (alpha_I alpha_J^T [k0 == 64 J] - X[k0 .. k0 + kEvChunk, I]^T
// X[.., J]) with G_ij = sf2 exp(-d^2 / 2 l^2) d^2 / l^2 into slots[item] (halved
// for I == J), then *out = the slots' sum in a fixed order.
// evidence_pairs (host): the cutoff's drop set (T x T, symmetric) over the
// k-tile boxes (x0, x1, y0, y1) under `budget`, and the summed bound.
constexpr int kEvSums = 9;
constexpr int kEvChunk = 1024;
constexpr double kEvLog2Pi = 1.8378770664093454836;   // log 2 pi
hipError_t launch_evidence_norms(hipStream_t s, const double *X, int64_t ld, int64_t n, const double *alpha,
                                 const double *z, const float *obs, const float *L, int64_t ldl, double m0, double *c,
                                 double *sums);
hipError_t launch_evidence_loo(hipStream_t s, const double *c, const double *alpha, const float *obs,
                               const int64_t *order, int64_t n, double *loo_mean, double *loo_var);
hipError_t launch_evidence_gram(hipStream_t s, const double *X, int64_t ld, int64_t n, const float *x, const float *y,
                                const double *alpha, const int4 *items, int64_t n_items, double ell, double sf2,
                                double *slots, double *out);
void evidence_pairs(const float *boxes, const double *alpha_l1, const double *sqrtc_l1, int64_t T, double ell,
                    double sf2, double budget, uint8_t *drop, double *bound);

inline int64_t acq_blocks(int64_t m) { return (m + kAcqThreads - 1) / kAcqThreads; }

// ------------------------------------------------------ frontier (8(f)1)
// Device raster of FindSafetyContourIndices (:425-475): the node's
// int-truncated bounds from a device min/max, each grid point's pixel
// (scaled by width/height, out-of-range dropped), last writer (highest
// index) wins -- atomicMax on a dense owner map, which replaces the node's
// unordered_map (:468-475) -- and owner[k] = that point if it is safe, else
// -1 (a pixel is foreground exactly when its last writer is safe).
// img[k] = 1 on foreground pixels.  Workspace: frontier_work_bytes(m);
// owner: width*height int32; img: width*height bytes.
size_t frontier_work_bytes(int64_t m);
hipError_t launch_frontier_raster(hipStream_t s, const double *Dx, const double *Dy, const uint8_t *safe, int64_t m,
                                  int width, int height, void *work, int32_t *owner, uint8_t *img);
// F[i] = owner[pix[i]]; when lo is non-null also out[c*nf + i] = (Dx, Dy, lo, hi)[F[i]].
hipError_t launch_frontier_gather(hipStream_t s, const int32_t *pix, int64_t nf, const int32_t *owner,
                                  const double *Dx, const double *Dy, const double *lo, const double *hi, int32_t *F,
                                  double *out);
// host side (frontier.cpp)
void trace_external_pixels(const uint8_t *img, int w, int h, std::vector<int32_t> &pix);
int64_t select_subgoal(size_t nf, const double *fx, const double *fy, const double *flo, const double *fhi,
                       double goal_x, double goal_y);

}  // namespace sbo
