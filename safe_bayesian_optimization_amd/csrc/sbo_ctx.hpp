// sbo_ctx.hpp -- the context of libsbo.so: what it holds and who may write
// each part ("the context").  Host only; no .hip file
// includes it.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "operand_state.hpp"
#include "sbo_internal.hpp"

// ------------------------------------------------------------------ options
// The SBO_OPT_* settings.  Written by sbo_set_option alone; every stage reads
// them (plan_refresh, chol_plan, tick_plan, inv_config take them const).
struct sbo_options {
    int chol_reserve = 0;        // SBO_OPT_CHOL_RESERVE: CUs the trailing updates leave free (CU-masked aux stream)
    int chol_gemm_own = 4;       // SBO_OPT_CHOL_GEMM: 4 (default) / 5 the outer panels' updates int8-sliced, 3 split bf16, 2 every update by chol_update_kernel, 1 the small trailing ones, 0 rocBLAS
    int chol_diag = 1;           // SBO_OPT_CHOL_DIAG: the chain kernels (diagonal block, panel): 1 left-looking MFMA, 2 right-looking MFMA, 0 VALU (bitwise equal)
    int chol_outer = 1024;       // SBO_OPT_CHOL_OUTER: outer panel width of the two-level Cholesky (128: one level)
    int inv_overlap = 0;         // SBO_OPT_INV_OVERLAP = R > 0: the inverse's first half on inv_stream, CU-masked to leave R CUs free
    int64_t inv_base = 2048;     // SBO_OPT_INV_BASE: dtrtri base case of the recursive inverse
    int64_t inv_panels = 16;     // SBO_OPT_INV_PANELS: dgemm panels per product of the recursion
    int inv_oz = 6;              // SBO_OPT_INV_OZ: digits of the int8-sliced top-level products (0: dgemm)
    int64_t inv_oz_min = 0;      // SBO_OPT_INV_OZ_MIN: the smallest sliced split (0: 2048 at N >= 12288, else 4096)
    int inv_oz_adapt = 1;        // SBO_OPT_INV_OZ_ADAPT: the digits chosen per fit from the last guard reading
    int inv_check = 1;           // SBO_OPT_INV_CHECK: 0 off, 1 after sliced inverses, 2 after every full inverse
    int inverse_bits = 64;       // SBO_OPT_INVERSE_BITS: precision of the L^-1 computation
    int jitter_retries = 0;      // SBO_OPT_JITTER_RETRIES: NOT_SPD fits retried with diagonal jitter
    bool inverse_rec = true;     // SBO_OPT_INVERSE: 1 own recursive f64 inverse (panelled dgemms), 0 rocSOLVER dtrtri
    bool chol_blocked = true;    // SBO_OPT_CHOLESKY: 1 own blocked factorization, 0 rocSOLVER spotrf
    bool chol_trsm_own = true;   //   1: its panels by chol_trsm_kernel, 2: by rocBLAS strsm
    int spatial_order = 3;       // SBO_OPT_SPATIAL_ORDER: 0 caller order, 1 Hilbert, 2 Morton, 3 k-d
    int skip_log2 = -1;          // SBO_OPT_TILE_SKIP: skip K* tiles with every entry < 2^-L (-1: auto)
    int skip_budget = 20;        // SBO_OPT_SKIP_BUDGET: the auto cutoff keeps the skip error below 2^-B
    int query_order = 1;         // SBO_OPT_QUERY_ORDER: 0 caller order, 1 grid patches or Morton, 2 Morton
    int kernel_variant = 3;      // SBO_OPT_KERNEL_VARIANT: predictive kernel (3: split-operand bf16 sweep)
    int sweep_groups = 0;        // SBO_OPT_SWEEP_GROUPS: persistent sweep workgroups (0: one per CU)
    int precision_opt = -1;      // SBO_OPT_PRECISION: -1 auto (fit-time probe), 0 the fast split sweep, 1 always f64
    int resort_pct = 25;         // SBO_OPT_RESORT: re-sort + refactor on append past this share of unsorted points
    int precise_kernel = 3;      // SBO_OPT_PRECISE_KERNEL: 0 the f64 MFMA sweep, 1 the int8 sliced sweep, 3 the same reading the K* table
    int64_t table_mb = 0;        // SBO_OPT_TABLE_MB: the K* table's memory budget (SBO_OPT_PRECISE_KERNEL 3; 0: auto)
    int probe_grid = 32, probe_train = 512;  // SBO_OPT_PROBE_SIZE: the probe's grid side and training locations
    int plan_block = 0;          // SBO_OPT_PLAN_BLOCK: the precise plans' item blocks (bi << 8 | bq; 0: row-block-major)
    int reprobe_pct = 25;        // SBO_OPT_REPROBE: appends re-probe once N grew by this share (0: every append)
    bool inv_batched = true;     // SBO_OPT_INV_LEAVES: the recursion's base cases inverted up front, batched
    bool inv_leaves_own = true;  // (SBO_OPT_INV_LEAVES 2, default: by doubling from 128-column blocks, inverse_leaves)
    int stream_share = 10;       // SBO_OPT_STREAM_SHARE: an update's cutoff may spend 2^-s of the sweep's skip budget
    int64_t stream_max_rows = 64;   // SBO_OPT_STREAM_MAX_ROWS: more appended rows than this take the full sweep
    int evidence_budget = 20;    // SBO_OPT_EVIDENCE_BUDGET: the pair cutoff may move grad[0] by 2^-B n (0: dense)
    int whatif_gemm = 0;         // SBO_OPT_WHATIF_GEMM: the candidate weights' two products by 0 dtrmm, 1 dgemm over the zero half
    int64_t remove_max = 2;      // SBO_OPT_REMOVE_MAX: sbo_remove refits the remaining points above this many removed ones
};

// --------------------------------------------------------- derived operands
// Two operands are derived from the model's packed tiles and f64 inverse, row
// block by row block.  Each owns its buffers and the record of how much of
// them is valid (sbo::OperandState).  The rules, the same for both:
//  - the refresh says what changed, once per RefreshPlan (refresh_operand): a
//    full refresh everything, an incremental one the row blocks from I0 on;
//    unfit() says everything;
//  - update() derives from the first stale row block on -- from 0 when the
//    layout wanted is not the one last derived -- keeping the row blocks below
//    it when a buffer grows, and marks the operand current in that layout;
//  - the refresh calls update() beside its own packs where it has a second
//    stream (eagerly), the tick calls it on `stream` (lazily): they differ in
//    the streams they pass and in nothing else.
// Their member functions are in sbo_api.cpp.

// The split (bf16 x3) operand of the fast sweep and its coordinates (kernel
// variants 2, 3); layouts: sbo::x3_layout.
class SplitOperand {
public:
    sbo::DevBuf ax3, kc3;
    const sbo::OperandState &state() const { return st_; }
    void rows_changed(int64_t I0) { st_.touch(I0); }
    void all_changed() { st_.touch_all(); }
    // the buffers for npad rows (a growing one copies on `stream` and waits
    // for it: the refresh reserves before it forks, update() does otherwise)
    sbo_status reserve(sbo_ctx *ctx, int64_t npad, int layout);
    // the planes on `planes`, with the coordinates in the same launch, or
    // without: pack_coords then writes them once alpha is there
    sbo_status update(sbo_ctx *ctx, int64_t npad, int layout, hipStream_t planes, bool coords);
    sbo_status pack_coords(sbo_ctx *ctx, int64_t npad, hipStream_t s);

private:
    sbo::OperandState st_;
};

// The precise sweep's operand: f64 tiles (layout 0: a64, kc64) or int8 digit
// tiles with their exponents (layouts 1, 2: aoz, eoz, koz), from the f64
// inverse and alpha64.  A pack on another stream than `stream` is left running
// past the call: the precise sweep waits for it on the device (wait_on), and
// whoever rewrites L^-1, alpha64, the points or the operand first on the host
// (drain).
class PreciseOperand {
public:
    sbo::DevBuf a64, kc64;
    sbo::DevBuf aoz, eoz, koz;
    hipEvent_t ev = nullptr;     // (made with aux_stream: chol_streams)
    const sbo::OperandState &state() const { return st_; }
    bool in_flight() const { return pending_; }
    void rows_changed(int64_t I0) { st_.touch(I0); }
    void all_changed() { st_.touch_all(); }
    sbo_status drain(sbo_ctx *ctx);
    sbo_status wait_on(sbo_ctx *ctx, hipStream_t s) const;
    sbo_status reserve(sbo_ctx *ctx, int64_t npad);
    sbo_status update(sbo_ctx *ctx, int64_t npad, hipStream_t s);

private:
    sbo::OperandState st_;
    bool pending_ = false;
};

// Workspaces that carry nothing from one call to the next: sbo_trim frees
// exactly these (a new one goes into release()'s list).
struct Workspaces {
    sbo::DevBuf scratch;         // append workspace, the refresh's row sums
    sbo::DevBuf gzws;            // the int8-sliced GEMM's packed operands (SBO_OPT_INV_OZ)
    sbo::DevBuf gzws_aux;        //   and those of the products on aux_stream (the inverse's second half)
    sbo::DevBuf chk;             // the accuracy guard's (inv_check.hip)
    sbo::DevBuf restage;         // the re-sort's staging copy of all points
    sbo::DevBuf kzt;             // the int8 sweep's K* table of one chunk of query blocks (SBO_OPT_PRECISE_KERNEL 3)
    sbo::DevBuf qcost;           // sbo_query_cost scratch
    sbo::DevBuf awork;           // launch_alpha_f64's partial sums
    sbo::DevBuf evws, evitems;   // sbo_evidence: column norms, tile sums, order, LOO staging; the work items and their slots
    sbo::DevBuf wiws;            // sbo_whatif: K_c^T / W^T, U^T, the candidates' sums and factors, counts, host staging
    sbo::DevBuf smws;            // sbo_sample: T^T / W^T, U^T, Theta^T, the frequencies, the sums, counts, keys, host staging
    sbo::DevBuf cholx3[2];       // the Cholesky's outer panels split into bf16 planes (SBO_OPT_CHOL_GEMM 3), alternating
    sbo::DevBuf rmws, rmw64, rmmove;   // sbo_remove: the chain's carry, coefficients and kept positions; a batch's f64 columns of L; the compaction's staging
    void release() {
        for (sbo::DevBuf *b : {&scratch, &gzws, &gzws_aux, &chk, &restage, &kzt, &qcost, &awork, &evws, &evitems, &wiws,
                               &smws, &cholx3[0], &cholx3[1], &rmws, &rmw64, &rmmove})
            b->release();
    }
};

struct sbo_ctx {
    // ---- streams, handles, events: made once, by sbo_create and the first
    // blocked factorization (chol_streams)
    int device = 0;
    int num_cu = 0;              // compute units of the device
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    rocblas_handle blas = nullptr;
    // the blocked Cholesky's look-ahead: trailing updates on a second stream
    // (created on first use: chol_streams, aux_ready), ordered against `stream` by two events, with a
    // rocBLAS handle of its own (a handle's device workspace must not be
    // shared by kernels in flight on two streams)
    hipStream_t aux_stream = nullptr;
    rocblas_handle blas_aux = nullptr;
    int aux_reserved = 0;        // the mask the current aux stream was created with
    hipEvent_t ev_panel = nullptr, ev_trail = nullptr;
    hipEvent_t ev_pack = nullptr;  // the fit's operand packs on aux_stream (refresh_operand)
    // the recursive inverse's first half beside the Cholesky's last steps (SBO_OPT_INV_OVERLAP)
    hipStream_t inv_stream = nullptr;
    rocblas_handle blas_inv = nullptr;
    int inv_reserved = 0;
    hipEvent_t ev_half = nullptr, ev_inv = nullptr;
    // the inverse's accuracy guard (SBO_OPT_INV_CHECK, inv_check.hip)
    hipStream_t chk_stream = nullptr;
    hipEvent_t ev_chk0 = nullptr, ev_chk1 = nullptr;
    std::string err;

    // ---- options: sbo_set_option
    sbo_options opt;

    // ---- the fitted model: written by the fit pipeline (sbo_fit, sbo_append,
    // sbo_import_state) under a FitCommit; unfit() is the one way out of it
    int64_t n = 0;       // training points
    int64_t cap = 0;     // allocated leading dimension of L (>= n, for appends)
    sbo_hyper hyper{0.4, 1.0, 0.1, 0.0};
    bool fitted = false;         // written true only by FitCommit::commit (sbo_api.cpp)
    bool has_factor = false;     // false after sbo_import_state: predict-only (no L to append to)
    uint64_t fit_epoch = 0;      // counts every event that rebuilds the model from scratch (a block append keeps it)
    sbo::DevBuf x, y, obs;       // training data, f32, capacity cap
    sbo::DevBuf L;               // lower Cholesky factor, column-major, lda = cap
    sbo::DevBuf Linv;            // L^-1 (strtri f32 workspace, or dtrtri f64 kept for appends), lda = cap
    int64_t linv_n = 0;          // rows of the f64 L^-1 held in Linv (0: none; appends extend it)
    double jitter = 0.0;         // the diagonal jitter of the current fit (0 unless a retry succeeded)
    int auto_skip_log2 = 160;    // auto K* cutoff for V (half the budget), computed at fit (refresh_operand)
    int auto_skip_mean_log2 = 160;  // auto cutoff the last row block keeps for the mean
    float lg_tau_v = -1000.0f;   // log2 of each row block's |dV_I|_2 budget (tile-norm test)
    sbo::DevBuf tile_lgn;        // per packed tile: log2 gain bounds of A_It and of its bf16 pieces (2 x float4)
    sbo::DevBuf tile_colmax;     // per k-tile: the largest tile_lgn[..].x of its column (the plan's prefilter)
    double max_row_l1 = 0.0;     // max_i sum_j |A_ij|, A = sf2 L^-1
    double alpha_l1 = 0.0;       // sum_j |sf2 alpha_j|
    std::vector<int64_t> order;  // internal row -> caller's training index
    float bbox[4] = {0.f, 0.f, 0.f, 0.f};  // training bounding box (x0, x1, y0, y1)
    sbo::DevBuf kbox;            // per k-tile bounding boxes (float4)
    sbo::DevBuf alpha;           // K^-1 (y - m0), length cap
    sbo::DevBuf aug;             // packed sf2 * L^-1 tiles
    sbo::DevBuf kcoord;          // per k-tile: x[BK], y[BK], sf2*alpha[BK]
    int64_t npad = 0;            // rows/cols of the packed operand (multiple of BM)
    int64_t n_sorted = 0;        // points of the last k-d sort (fit / re-sort) still stored
    int64_t removed_since_sort = 0;   // points sbo_remove rotated out since then (SBO_OPT_RESORT counts them with the appended ones)
    sbo::DevBuf alpha64;         // alpha from the f64 solve (length cap)
    sbo::DevBuf zvec, rvec;      // z = L^-1 (y - m0) (f64, valid for z_n points: appends update alpha from it), r scratch
    int64_t z_n = 0;
    sbo_inv_check chk_res{};     // the guard's last result (ran = 0: none since the last fit)
    // SBO_OPT_INV_OZ_ADAPT: the digits of the current fit's sliced products
    // (inv_digits), those the last guard reading allows for the next fit of
    // the same hyper-parameters, about the same N and box area (0: inv_oz), that
    // reading's N and hyper-parameters, and whether a reduced fit of this data
    // fired (then it keeps inv_oz digits).  A history across fits: unfit()
    // leaves it.
    int inv_oz_cur = 0, inv_oz_next = 0;
    int64_t inv_oz_hist_n = 0;
    double inv_oz_hist_area = 0.0;   // (the training bounding box's area: N / area the density)
    sbo_hyper inv_oz_hist_hyper{};
    bool inv_oz_pinned = false;
    // precise sweep (SBO_OPT_PRECISION, predict_f64.hip): the probe's verdict and readings
    bool precise = false;        // the sweep ticks run in effect
    int64_t probe_n = 0;         // training points at the last probe (0: none)
    double probe_err = -1.0, probe_vmin = 0.0, probe_vmax = 0.0;  // fast sweep's error on the probe, var range
    // the probe's two parts: its grid over the training box, and training
    // locations (where the variance is smallest); each part's own normwise error
    double probe_err_grid = -1.0, probe_err_train = -1.0, probe_vmax_grid = 0.0, probe_vmax_train = 0.0;
    int probe_m_grid = 0, probe_m_train = 0;
    double probe_ref_tol = 0.0;  // the probe reference sweep's skip budget (absolute variance)
    int p_skip_log2 = 160;       // the precise plan's cutoffs and budget (2^-B of the probe's smallest variance)
    float p_lg_tau_v = -1000.0f;

    // ---- the operands derived from the model: their owners
    SplitOperand split;
    PreciseOperand pop;

    // ---- the kept posterior of sbo_tick_stream: state, not workspace
    sbo::StreamKeep keep;

    // ---- workspaces: sized by whoever uses them, nothing in them outlives a call
    Workspaces ws;               // ... and these sbo_trim frees
    sbo::DevBuf info;            // rocSOLVER info
    // grid layout of the last query buffers seen (the layout depends on (m, W, c0) only)
    const float *qgrid_x = nullptr, *qgrid_y = nullptr;
    int64_t qgrid_m = -1;
    sbo::QueryGrid qgrid;
    sbo::DevBuf qgwork;          // grid detection + patch layout workspace
    sbo::DevBuf plan_work;       // the tick's tile plan (launch_plan)
    sbo::DevBuf fwork, fowner, fimg, fpix, fout;  // device frontier (sbo_frontier / sbo_subgoal)
    sbo::DevBuf qwork;           // query ordering workspace
    sbo::DevBuf qpad;            // queries padded to whole blocks (split sweep without query ordering)
    sbo::DevBuf qprobe, oprobe;  // probe grid and outputs
    sbo::DevBuf part, mean;      // predictive partial sums [nI][ldp], mean [ldp]
    sbo::DevBuf hq;              // host-input staging (queries, mu/sd, ...)
    sbo::DevBuf hout;            // host-output staging
    sbo::DevBuf keys;            // per-block argmax keys + final key
    sbo_key *host_key = nullptr; // pinned readback

    // kernel timing (sbo_profile)
    bool prof = false;
    std::vector<hipEvent_t> ev_pool;               // free events
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_predict, ev_fill;
    sbo::DevBuf counters;                          // [0]: predictive tiles multiplied

    bool fail(const std::string &m) { err = m; return false; }
};
