/*
 * sbo.h -- C ABI of the MI355X safe-BO planning-tick library (libsbo.so).
 *
 * The reference has no plugin/FFI API for this path.  Its
 * boundary is (i) the GetTerrainMapWithUncertainty service between the
 * external GP mapper and the node, consumed at
 * src/safe_bayesian_optimization_node.cpp:576-647 (request resolution[2] f32
 * :580-581; response success, message, n_width_cells, n_height_cells,
 * x_coords[], y_coords[], values[] (= mu), uncertainties[] (= sigma)
 * :606-644), and (ii) the node's private calls ComputeSets() (:399-416),
 * FindSafetyContourIndices() (:418-497) and GetNextSubgoal() (:499-550).
 * Each entry point below names the reference interface it replaces.
 *
 * Conventions (mirroring the reference, :129-177, :503-506, :1503):
 *   - the caller owns every buffer; no exceptions cross this boundary;
 *   - one context per thread; a context is not thread-safe;
 *   - calls are synchronous with respect to the context's HIP stream unless
 *     SBO_ASYNC is passed (then results are ready when the stream drains);
 *   - array pointers are host pointers unless SBO_DEVICE_PTRS is passed, in
 *     which case EVERY array argument of that call is a device pointer;
 *   - coordinates are SoA (all x, then all y), like the column-major
 *     Eigen::Matrix<double,Dynamic,2> D_ (:132);
 *   - "no subgoal" is -1 (:503-506).
 */
#ifndef SBO_H_
#define SBO_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBO_API __attribute__((visibility("default")))

typedef enum sbo_status {
    SBO_OK = 0,
    SBO_E_INVAL = 1,    /* bad argument (null pointer, n <= 0, bad hyper-parameter) */
    SBO_E_NOT_SPD = 2,  /* the Cholesky's leading minor (rocSOLVER info convention): K not positive definite */
    SBO_E_DEVICE = 3,   /* HIP / rocBLAS / rocSOLVER runtime error */
    SBO_E_OOM = 4,      /* device allocation failed */
    SBO_E_EMPTY = 5,    /* nothing to operate on (no fit yet, empty input) */
    SBO_E_STATE = 6     /* call out of order (e.g. predict before fit) */
} sbo_status;

/* flags */
#define SBO_DEVICE_PTRS 0x1u  /* all array arguments are device pointers */
#define SBO_ASYNC 0x2u        /* do not synchronise the stream before returning */

/* GP hyper-parameters (config/lpsc.yaml:35-37: noise_level 0.1,
 * length_scale 0.4, sigma_f 1.0).  noise_level is a noise VARIANCE. */
typedef struct sbo_hyper {
    double length_scale;
    double sigma_f;
    double noise_level;
    double prior_mean;
} sbo_hyper;

/* Acquisition score for the grid argmax (a10). */
typedef enum sbo_score {
    SBO_SCORE_WIDTH = 0,  /* Q(:,1) - Q(:,0), the width GetNextSubgoal ranks (:516) */
    SBO_SCORE_UCB = 1     /* Q(:,1) = mu + beta*sigma */
} sbo_score;

/* Result of a masked argmax: highest score, lowest global index on ties.
 * idx = -1 when no point is eligible.  Keys from different shards combine
 * with sbo_key_combine (this is what crosses ranks). */
typedef struct sbo_key {
    double score;
    int64_t idx;
} sbo_key;

typedef struct sbo_ctx sbo_ctx;

/* Library / context ------------------------------------------------------ */
SBO_API const char *sbo_version(void);
SBO_API const char *sbo_status_string(sbo_status s);
/* Replaces the node's service client (:75-77): binds a HIP device.  */
SBO_API sbo_status sbo_create(int device, sbo_ctx **out);
SBO_API void sbo_destroy(sbo_ctx *ctx);
/* Run on the caller's HIP stream (hipStream_t), e.g. torch's current stream.
 * NULL restores the context's own stream. */
SBO_API sbo_status sbo_set_stream(sbo_ctx *ctx, void *hip_stream);
SBO_API const char *sbo_last_error(const sbo_ctx *ctx);

/* GP mapper (the external terrain_mapping_node, a1+a2) -------------------
 * Fit the posterior to n measurements (x, y, obs): RBF fill (HIP kernel),
 * the library's blocked Cholesky (SBO_OPT_CHOLESKY), L^-1 in f64 by its block
 * recursion (SBO_OPT_INVERSE), alpha = L^-T L^-1 (y - m0) from that inverse,
 * the packed predictive operand and its tile bounds, and the precision probe
 * (SBO_OPT_PRECISION).  Replaces the mapper's fit behind the service.
 * Rejected arguments (SBO_E_INVAL, SBO_E_EMPTY) leave a fitted context as it
 * was.  Any error after argument validation (SBO_E_NOT_SPD included) leaves
 * the context unfitted: sbo_num_train is 0, and it accepts a new sbo_fit,
 * sbo_import_state or option calls only (everything else: SBO_E_STATE). */
SBO_API sbo_status sbo_fit(sbo_ctx *ctx, const float *x, const float *y, const float *obs,
                           int64_t n, sbo_hyper hyper, uint32_t flags);

/* Streaming update (C5): append b measurements with a block Cholesky update
 * (L21 = K21 L11^-T, L22 = chol(K22 - L21 L21^T)), then re-solve alpha.
 * Replaces a full re-fit on each spatial_data_size change (:552-566).
 * Rejected arguments leave the fitted context as it was.  Any error after
 * argument validation (SBO_E_NOT_SPD of the updated block included, in the
 * block update and in the SBO_OPT_RESORT re-sort alike) leaves the context
 * unfitted, as a failed sbo_fit does: refit all the points. */
SBO_API sbo_status sbo_append(sbo_ctx *ctx, const float *x, const float *y, const float *obs,
                              int64_t b, uint32_t flags);

/* The inverse of sbo_append: drop b training points without a refit.  Deleting
 * a row of a Cholesky factor is a chain of Givens rotations, and the same
 * rotations applied to the rows of the f64 inverse give the new inverse:
 * O(n (n - i)) per point stored at position i, against n^3 / 3 for a refit
 * (csrc/remove.hip; all arithmetic f64, the factor rounded to f32 once per
 * call).  idx: a HOST array (also with SBO_DEVICE_PTRS) of b caller indices in
 * sbo_get_order's numbering -- positions in the fit's input, appends numbered
 * after the fit.  Afterwards the remaining points keep their relative order
 * and are renumbered densely: new index = old index minus the number of
 * removed indices below it (numpy.delete); sbo_get_order, sbo_evidence's LOO
 * arrays and sbo_sample's eps counter use the new numbering, and a later
 * sbo_append numbers its points from the new n.
 *
 * SBO_E_STATE before a fit or on an imported state; SBO_E_INVAL for a NULL idx
 * with b > 0, b < 0, an index outside [0, n) or a duplicate; SBO_E_EMPTY for
 * b == n (a model needs a point); b == 0 is SBO_OK and nothing happens.
 * Rejected arguments leave the context exactly as it was; any error after
 * validation (SBO_E_NOT_SPD of a pivot the chain meets that is not positive
 * and finite included) leaves it unfitted, as a failed sbo_append does.
 *
 * sbo_get_bounds is unchanged by a removal.  A removal starts a new fit epoch:
 * the next sbo_tick_stream runs the full sweep (reason REFIT), and sbo_whatif
 * and sbo_sample return SBO_E_STATE until that tick.
 *
 * The rotations run unless (reason): there is no current f64 inverse and z
 * (SBO_OPT_INVERSE_BITS 32: NO_INVERSE); b > SBO_OPT_REMOVE_MAX (OVER_CAP); or,
 * with spatial order on, the points appended plus the points removed since the
 * last k-d sort would exceed SBO_OPT_RESORT percent of the sorted points still
 * stored (RESORT; sbo_append counts removals the same way).  Then the
 * remaining points are staged again in k-d order and factored from scratch
 * (path 0), the renumbered indices kept.  info may be NULL; the caller sets
 * info->struct_size to sizeof(sbo_remove_info) and no more than that many
 * bytes are written.  SBO_ASYNC as sbo_append (the refresh's own
 * synchronisations stay). */
typedef enum sbo_remove_reason { SBO_REMOVE_DOWNDATED = 0, SBO_REMOVE_NO_INVERSE = 1,
                                 SBO_REMOVE_OVER_CAP = 2, SBO_REMOVE_RESORT = 3 } sbo_remove_reason;
typedef struct sbo_remove_info {
    uint32_t struct_size; int32_t path;      /* 1 rotations, 0 refit of the remaining points */
    int32_t reason, reserved;
    int64_t removed, n;                      /* n: points left */
    int64_t first_row;                       /* smallest stored position removed (-1: b == 0) */
    int64_t rotations;                       /* sum over removed points of the columns their chain crossed (0 on path 0) */
    double ms;                               /* device time from the call's first kernel to its last */
} sbo_remove_info;
SBO_API sbo_status sbo_remove(sbo_ctx *ctx, const int64_t *idx, int64_t b, sbo_remove_info *info, uint32_t flags);
/* Test accessor: the current f64 inverse L^-1 as a dense n x n ROW-major host
 * array (cap >= n * n doubles), the upper triangle zeroed.  SBO_E_STATE without
 * a current f64 inverse. */
SBO_API sbo_status sbo_debug_inverse64(sbo_ctx *ctx, double *X, int64_t cap);
/* Test accessor, host only, no context: sbo_remove's bookkeeping
 * (csrc/remove_map.hpp).  order (n, as sbo_get_order) and idx (b) give pos,
 * the b stored positions in ascending order, and new_order, the renumbered
 * order of the n - b rows left (either may be NULL).  SBO_E_INVAL / SBO_E_EMPTY
 * as sbo_remove. */
SBO_API sbo_status sbo_debug_remove_map(const int64_t *order, int64_t n, const int64_t *idx, int64_t b, int64_t *pos,
                                        int64_t *new_order);

/* Number of training points currently fitted (0 before sbo_fit). */
SBO_API int64_t sbo_num_train(const sbo_ctx *ctx);

/* Predict (a3+a4): posterior mean and latent std at m query points
 * (the service's values[] and uncertainties[], :642-643).  mu/sd may be NULL
 * to skip that output. */
SBO_API sbo_status sbo_predict(sbo_ctx *ctx, const float *qx, const float *qy, int64_t m,
                               float *mu, float *sd, uint32_t flags);

/* ComputeSets() (:399-416) == ComputeConfidenceIntervals + UpdateSafeSet:
 *   c = beta*sd;  lo = mu - c;  hi = mu + c;  safe = lo > f_min
 * evaluated in IEEE double exactly as the node's Eigen code (no FMA).
 * lo/hi are Q_.col(0)/Q_.col(1) (f64), safe is S_ (1 byte per point). */
SBO_API sbo_status sbo_compute_sets(sbo_ctx *ctx, const float *mu, const float *sd, int64_t m,
                                    double beta, double f_min, double *lo, double *hi,
                                    uint8_t *safe, uint32_t flags);
/* The same on f64 inputs: the node's own mu_/std_ (Eigen::VectorXd,
 * node.cpp:129-130, filled at :641-643) passed as they are -- lossless for
 * any service value, bit-exact with ComputeSets() (:411-416). */
SBO_API sbo_status sbo_compute_sets_f64(sbo_ctx *ctx, const double *mu, const double *sd, int64_t m,
                                        double beta, double f_min, double *lo, double *hi,
                                        uint8_t *safe, uint32_t flags);

/* Grid acquisition argmax (a10): argmax of score over mask (mask may be NULL),
 * lowest index on ties, NaN never wins.  index_offset is added to local
 * indices (the first global row of this rank's shard). */
SBO_API sbo_status sbo_argmax(sbo_ctx *ctx, const double *score, const uint8_t *mask, int64_t m,
                              int64_t index_offset, sbo_key *out, uint32_t flags);

/* The whole planning tick on one shard of the grid, fused on the device:
 * predict -> ComputeSets -> masked argmax of `score` over the safe set.
 * Output arrays may be NULL to skip writing them (the key is always produced).
 * This is the headline step measured by bench.py. */
SBO_API sbo_status sbo_tick(sbo_ctx *ctx, const float *qx, const float *qy, int64_t m,
                            double beta, double f_min, sbo_score score, int64_t index_offset,
                            float *mu, float *sd, double *lo, double *hi, uint8_t *safe,
                            sbo_key *out, uint32_t flags);

/* sbo_tick with a kept posterior: the node's steady state, "one measurement
 * arrived (sbo_append), give me the map and the subgoal".  Arguments,
 * outputs, flags, status codes and error strings are sbo_tick's.
 *
 * The first call runs sbo_tick's full sweep and keeps, per sweep position, the
 * f64 mean and variance (about 28 B per query, owned by the context: state,
 * not workspace -- sbo_trim leaves it, sbo_stream_reset frees it).  A later
 * call with the same queries after block appends adds only the R appended
 * rows' share to the kept posterior,
 *     v = L^-1[n_map:n, 0:n] k*(q),  var -= sum_r v_r^2,  mu += sum_r v_r z_r
 * (R n multiply-adds per query instead of n^2 / 2), and runs the acquisition
 * from it.  That path needs: a kept posterior of the same fit epoch (sbo_fit,
 * a re-sorting append, sbo_import_state, a failed fit or append start a new
 * one; a block append does not), of the same sweep (fast / precise) and the
 * same m; bitwise equal queries; the fit's f64 inverse current
 * (SBO_OPT_INVERSE_BITS 64, not an imported state);
 * R <= SBO_OPT_STREAM_MAX_ROWS; and the accumulated cutoff bound within the
 * sweep's skip budget.  Anything else takes the full sweep and keeps its
 * posterior; on that path every output is bitwise sbo_tick's.  No call is
 * refused for streaming reasons; sbo_get_stream says what the last one did.
 *
 * Synchronisation: before an update the queries are compared on the device
 * with the kept ones and the appended rows' norms are reduced; their result
 * (24 bytes) is read back with one synchronisation of the context's stream,
 * also under SBO_ASYNC.  The full path synchronises as sbo_tick does.
 *
 * The update skips a (128-query block, 64-column k-tile) pair when the two
 * bounding boxes put every K* entry below 2^-L.  With SBO_OPT_TILE_SKIP -1, L
 * is the smallest exponent whose worst-case effect, from
 * d_r = sf2 2^-L |L^-1_r|_1 over the appended rows r,
 *     variance: 2 sqrt(sf2) sqrt(sum d_r^2) + sum d_r^2,   mean: sum d_r |z_r|,
 * stays within 2^-s (s = SBO_OPT_STREAM_SHARE) of the budget of the sweep in
 * effect: 2^-B sf2 and 2^-B sf for the fast sweep, 2^-B times the smallest
 * probe variance (and 2^-B sf) for the precise one.  The bounds spent add up
 * in err_var / err_mean until the next full sweep, which a call takes
 * (reason BUDGET) before they would exceed the budget.  SBO_OPT_TILE_SKIP 0:
 * dense; a fixed L spends its own bound; L >= 150 drops only exact zeros
 * (bitwise the dense update). */
SBO_API sbo_status sbo_tick_stream(sbo_ctx *ctx, const float *qx, const float *qy, int64_t m, double beta,
                                   double f_min, sbo_score score, int64_t index_offset, float *mu, float *sd,
                                   double *lo, double *hi, uint8_t *safe, sbo_key *out, uint32_t flags);

/* What the last sbo_tick_stream did and why.  The caller sets struct_size to
 * sizeof(sbo_stream_info); the library writes no more than that many bytes. */
typedef enum sbo_stream_reason {
    SBO_STREAM_FIRST = 0,            /* no kept posterior yet */
    SBO_STREAM_UPDATED = 1,          /* the update path ran (rows = 0: acquisition only) */
    SBO_STREAM_QUERIES_CHANGED = 2,  /* another m, or a query not bitwise the kept one */
    SBO_STREAM_REFIT = 3,            /* another fit epoch, or another sweep (fast / precise) in effect */
    SBO_STREAM_NO_INVERSE = 4,       /* no current f64 inverse / z to read the appended rows from */
    SBO_STREAM_ROWS_OVER_CAP = 5,    /* more appended rows than SBO_OPT_STREAM_MAX_ROWS */
    SBO_STREAM_BUDGET = 6,           /* the accumulated cutoff bound would exceed the skip budget */
    SBO_STREAM_RESET = 7             /* first call after sbo_stream_reset */
} sbo_stream_reason;
typedef struct sbo_stream_info {
    uint32_t struct_size;
    int32_t path;                 /* 0 full sweep, 1 update */
    int32_t reason;               /* sbo_stream_reason */
    int32_t cutoff_log2;          /* the update's L (0: dense) */
    int64_t rows;                 /* R: rows appended since the kept posterior's last tick */
    int64_t n_map;                /* training rows the kept posterior had seen before this call */
    int64_t m;
    int64_t updates_since_full;
    int64_t tiles_total;          /* (query block, k-tile) pairs of the last update */
    int64_t tiles_kept;           /* ... and those it multiplied */
    double err_var, err_mean;     /* worst-case bounds spent since the last full sweep */
    double budget_var, budget_mean;
} sbo_stream_info;
SBO_API sbo_status sbo_get_stream(const sbo_ctx *ctx, sbo_stream_info *out);
/* Drop the kept posterior and free its memory; the next sbo_tick_stream runs
 * the full sweep (reason RESET). */
SBO_API sbo_status sbo_stream_reset(sbo_ctx *ctx);
/* Test accessor: the kept f64 mean and variance (sf2 - |V|^2, not clamped) in
 * the caller's order, host buffers of cap >= m doubles each.  SBO_E_STATE
 * without a kept posterior. */
SBO_API sbo_status sbo_debug_stream_state(sbo_ctx *ctx, double *mu64, double *var64, int64_t cap);

/* Model evidence of the current fit: the log marginal likelihood of the
 * training data under the fitted hyper-parameters, its gradient, and the
 * leave-one-out predictive -- whether length_scale / sigma_f / noise_level
 * suit the data (no reference counterpart: the node copies them from
 * config/lpsc.yaml:35-37).  Read off what sbo_fit / sbo_append leave on the
 * device: the f32 factor L, the f64 inverse X = L^-1, z = X (y - m0) and
 * alpha = X^T z.  With r = y - m0, s = noise_level + jitter (the jitter held
 * constant in the derivatives), c_i = (K^-1)_ii = sum_{k >= i} X_ki^2:
 *   lml      = -1/2 z'z - sum_i log L_ii - n/2 log 2 pi
 *   grad[0]  = 1/2 sum_ij (alpha_i alpha_j - (X'X)_ij) G_ij,
 *              G_ij = sf2 exp(-d_ij^2 / 2 l^2) d_ij^2 / l^2
 *   grad[1]  = (alpha'r - s alpha'alpha) - (n - s sum_i c_i)
 *   grad[2]  = 1/2 noise_level (alpha'alpha - sum_i c_i)
 *   grad[3]  = sum_i alpha_i
 *   loo_mean_i = y_i - alpha_i / c_i,  loo_var_i = 1 / c_i,
 *   loo_log_pred = sum_i -1/2 log(2 pi / c_i) - 1/2 alpha_i^2 / c_i.
 * grad[0]'s trace is a contraction of K^-1 = X'X with a matrix that decays as
 * exp(-d^2 / 2 l^2): per pair of 64-point k-tiles (I <= J) a tall-skinny f64
 * Gram product on the f64 matrix cores.  With SBO_OPT_EVIDENCE_BUDGET B > 0 a
 * pair whose bounding boxes are at least sqrt(2) l apart may be dropped: by
 * |K^-1_ij| <= sqrt(c_i c_j) that moves grad[0] by at most
 * g(d_min) (sum_I |alpha| sum_J |alpha| + sum_I sqrt(c) sum_J sqrt(c)) for both
 * orders of the pair; pairs are dropped smallest bound first while the bounds
 * sum to at most 2^-B n (grad_budget); the sum spent is grad_err_bound.  Every
 * other field, and the LOO arrays, do not depend on the cutoff.  All sums run
 * in a fixed order (no floating-point atomics): two calls on the same state
 * agree bitwise.
 *
 * loo_mean / loo_var: n doubles each in the caller's training order
 * (sbo_get_order), or NULL; host pointers, device pointers with
 * SBO_DEVICE_PTRS.  The caller sets out->struct_size to
 * sizeof(sbo_evidence_info); the library writes no more than that many bytes.
 * Synchronous (the per-tile norms are read back; SBO_ASYNC is ignored).
 * Needs a fit with a factor and a current f64 inverse and z: SBO_E_STATE
 * before a fit, after a failed one, on an imported state and with
 * SBO_OPT_INVERSE_BITS 32.  Alters no fitted state; its workspace is freed by
 * sbo_trim. */
typedef struct sbo_evidence_info {
    uint32_t struct_size;          /* caller sets; the library writes no more than this many bytes */
    int32_t  dropped;              /* 1 if the cutoff dropped at least one tile pair */
    int64_t  n;
    double   lml;                  /* log p(y | X, theta) = data_fit - log_det - n/2 log 2pi */
    double   data_fit;             /* -1/2 z'z */
    double   log_det;              /* sum_i log L_ii  (the f32 factor's diagonal, widened) */
    double   grad[4];              /* d lml / d (log length_scale, log sigma_f, log noise_level, prior_mean) */
    double   grad_err_bound;       /* rigorous bound on |error of grad[0]| from dropped pairs (0 when dense) */
    double   grad_budget;          /* what the bound was allowed to be */
    int64_t  pairs_total, pairs_kept;   /* k-tile pairs I <= J */
    double   loo_log_pred;         /* sum_i log p(y_i | y_-i) */
    double   ms;                   /* device time of the call's kernels */
} sbo_evidence_info;
SBO_API sbo_status sbo_evidence(sbo_ctx *ctx, sbo_evidence_info *out,
                                double *loo_mean, double *loo_var, uint32_t flags);

/* Test accessor: sbo_evidence's pair cutoff alone, on the host (no context, no
 * device).  boxes: per k-tile x0, x1, y0, y1; alpha_l1 / sqrtc_l1: per k-tile
 * sum |alpha_i| / sum sqrt(c_i); budget: what the summed bound may be (<= 0:
 * nothing is dropped).  drop[I * T + J] = 1 for a dropped pair (symmetric, the
 * diagonal never); *bound = the dropped pairs' summed bound, both orders. */
SBO_API sbo_status sbo_debug_evidence_pairs(const float *boxes /* 4 T: x0,x1,y0,y1 */,
        const double *alpha_l1, const double *sqrtc_l1, int64_t T, sbo_hyper hyper,
        double budget, uint8_t *drop /* T*T, row-major, symmetric */, double *bound);

/* What-if posterior: for p candidate points c_j, the posterior cross-covariance
 * Cov(f(q), f(c_j)) with every query q of the kept posterior, and each
 * candidate's expander count -- the currently unsafe queries whose lower bound
 * would clear f_min after an optimistic observation at c_j (SafeOpt's
 * GP-defined expanders, Berkenkamp et al. 2016; the reference node ranks its
 * frontier by distance and width instead, node.cpp:499-550).  Nothing is
 * appended.  Read off what a streaming tick leaves on the device: the f64
 * inverse X = L^-1, z = X (y - m0), and sbo_tick_stream's kept f64 posterior
 * (mu, var).  With s = noise_level + jitter:
 *   k_j = k(train, c_j),  u_j = X k_j,  w_j = X^T u_j  (= K^-1 k_j)
 *   mu_c = m0 + u_j . z,  var_c = sf2 - |u_j|^2,  d_j = var_c + s
 *   cov(q, c_j) = k(q, c_j) - k*(q) . w_j
 * and, conditioning on y_j = mu_c + beta sd_c, sd_c = sqrt(max(var_c, 0)):
 *   mu'(q)  = mu(q) + cov(q, c_j) beta sd_c / d_j
 *   var'(q) = var(q) - cov(q, c_j)^2 / d_j
 *   lo'(q)  = mu'(q) - beta sqrt(max(var'(q), 0))                  (all f64)
 *   gain_j  = #{ q : not safe(q) and lo'(q) > f_min }
 * safe(q) is recomputed from the kept state exactly as sbo_tick_stream forms
 * its `safe` output (for the same beta and f_min).  That is the posterior of a
 * refit with (c_j, y_j) added, without the refit.
 *
 * cx, cy: p candidates, 1 <= p <= 1024.  gain: p counts.  cand_mu, cand_var:
 * p doubles each, or NULL.  cov, lo_new: p x m row-major in the caller's query
 * order (m = the kept posterior's), or NULL.  Host pointers; device pointers
 * (every array) with SBO_DEVICE_PTRS.  Synchronous (var_c and |w_j|_1 are read
 * back for the cutoff; SBO_ASYNC is ignored).  info may be NULL; the caller
 * sets info->struct_size to sizeof(sbo_whatif_info) and the library writes no
 * more than that many bytes.
 *
 * The sweep skips a (128-query block, 64-column k-tile) pair when the two
 * bounding boxes put every K* entry below 2^-L, which moves cov(q, c_j) by at
 * most e_j = sf2 2^-L |w_j|_1.  SBO_OPT_TILE_SKIP 0: dense; a fixed L spends
 * its own bound; L >= 150 drops only exact zeros (bitwise the dense result);
 * -1 (auto): the smallest L in [16, 149] for which every candidate keeps
 *   mean:     beta sd_c e_j / d_j                                  <= budget_mean
 *   variance: (2 sqrt(sf2 max(var_c, 0)) e_j + e_j^2) / d_j        <= budget_var
 * (the budgets sbo_get_stream reports; nothing accumulates, so a call may use
 * all of them), else 150.  err_cov = max_j e_j.  All floating-point sums run in
 * a fixed order and the counts are integer sums: two calls agree bitwise.
 *
 * SBO_E_STATE without a kept posterior, when the kept posterior has not seen
 * every fitted row (an append without a following sbo_tick_stream, another fit
 * epoch), and without a current f64 inverse and z (SBO_OPT_INVERSE_BITS 32, an
 * imported state).  SBO_E_INVAL for p <= 0, p > 1024 or a NULL gain.  Alters
 * no fitted or kept state; its workspace is freed by sbo_trim. */
typedef struct sbo_whatif_info {
    uint32_t struct_size;      /* caller sets; no more than this many bytes are written */
    int32_t  cutoff_log2;      /* L (0: dense) */
    int64_t  p, m, n;
    int64_t  tiles_total, tiles_kept;   /* (query block, k-tile) pairs */
    double   err_cov;          /* rigorous bound on |cov error| from the cutoff (0 when dense) */
    int64_t  best;             /* argmax gain, lowest j on ties */
    int64_t  best_gain;
    double   ms;               /* device time of the call's kernels */
} sbo_whatif_info;
SBO_API sbo_status sbo_whatif(sbo_ctx *ctx, const float *cx, const float *cy, int64_t p,
                              double beta, double f_min,
                              int64_t *gain,                        /* p */
                              double *cand_mu, double *cand_var,    /* p each, may be NULL */
                              double *cov, double *lo_new,          /* p x m row-major, caller's query order, may be NULL */
                              sbo_whatif_info *info, uint32_t flags);

/* Test accessor: sbo_whatif's auto cutoff alone, on the host (no context, no
 * device).  w_l1 / cand_var: per candidate |w_j|_1 / var_c; s = noise_level +
 * jitter.  *cutoff_log2 = the smallest L in [16, 149] within both budgets, 150
 * if none is, 0 (dense) when a budget is <= 0; *err_cov = max_j sf2 2^-L |w_j|_1
 * (0 when dense). */
SBO_API sbo_status sbo_debug_whatif_cutoff(int64_t p, const double *w_l1, const double *cand_var, double s,
                                           double beta, double sf2, double budget_var, double budget_mean,
                                           int32_t *cutoff_log2, double *err_cov);

/* Posterior sample paths on the kept grid: `samples` joint draws of the GP
 * posterior at every kept query, each draw's maximiser over the safe set
 * (Thompson sampling's key) and the size of its region above f_min.  Nothing
 * is appended.  The method is pathwise conditioning (Matheron's rule; Wilson
 * et al., ICML 2020): a prior path from F random Fourier features, and the
 * data-dependent correction exactly, through the fit's f64 inverse.  With
 * s = noise_level + jitter, X = L^-1 (f64), the kept f64 mean mu(q):
 *   g_j(x)  = sf / sqrt(F) sum_{f < F} [ a_fj cos(2 pi t_f(x)) + b_fj sin(2 pi t_f(x)) ]
 *   t_f(x)  = w_f . (x - c) in turns,  w_f = nu_f / (2 pi l),  nu_f ~ N(0, I2),
 *             c the centre of the training bounding box (sbo_get_bounds)
 *   t_j     = g_j(train) + sqrt(s) eps_j          (n)        a, b, eps ~ N(0, 1)
 *   u_j     = X t_j,  w_j = X^T u_j  (= K^-1 t_j)
 *   path_j(q) = mu(q) + g_j(q) - k*(q) . w_j      for every kept query q
 * E[path] = mu exactly; the covariance is the posterior's up to the feature
 * approximation of the prior kernel (pointwise standard error about
 * 1 / sqrt(2 F) of sf2), which is measured, not bounded: kernel_err is the
 * maximum over d = (a, +-b) 4 l / 32, a, b = 0 .. 32, of
 * |k^(d) / sf2 - exp(-|d|^2 / 2 l^2)|, k^(d) / sf2 = (1 / F) sum_f cos(2 pi w_f . d).
 *
 * The random numbers are part of the interface.  With normal(seed_t, e) =
 * element e of the counter-based SplitMix64 / Box-Muller stream started at
 * seed_t (uniform u_i = (output i + 1 of SplitMix64(seed_t) >> 11) 2^-53;
 * normal e = sqrt(-2 log max(u_2e, 1e-300)) cos(2 pi u_2e+1)), sample
 * J = first + j uses
 *   nu_f       = (normal(seed, 2 f), normal(seed, 2 f + 1))
 *   a_fJ, b_fJ = normal(seed + 1, J 2 F + f), normal(seed + 1, J 2 F + F + f)
 *   eps_J at the training point with caller index i = normal(seed + 2, J 2^24 + i)
 * (seeds mod 2^64).  So a path depends on (seed, J, F, the fit) only: not on
 * `samples` or how a range of J is cut into calls, not on
 * SBO_OPT_SPATIAL_ORDER, and not on the rank -- every rank of a sharded grid
 * draws the same global path on its rows, and the per-sample keys combine with
 * sbo_keys_reduce.
 *
 * keys: `samples` keys; keys[j].score = path_j at its maximiser over the safe
 * queries, idx = index_offset + the caller's index of it (the lowest index on
 * ties; a NaN never wins; idx -1 and score 0 when nothing is safe).  safe(q)
 * is recomputed from the kept state exactly as sbo_tick_stream forms its
 * `safe` output (for the same beta and f_min); f_min = -inf gives the
 * unconstrained maximiser.  count_above: samples counts #{q : path_j(q) >
 * f_min}, or NULL.  paths: samples x m row-major in the caller's query order
 * (m = the kept posterior's), or NULL.  Host pointers; device pointers (every
 * array) with SBO_DEVICE_PTRS.  Synchronous (|w_j|_1 is read back for the
 * cutoff; SBO_ASYNC is ignored).  info may be NULL; the caller sets
 * info->struct_size to sizeof(sbo_sample_info) and the library writes no more
 * than that many bytes.
 *
 * The sweep's K* cutoff is sbo_whatif's: dropping entries below 2^-L moves
 * path_j(q) by at most e_j = sf2 2^-L |w_j|_1 (rigorous).  SBO_OPT_TILE_SKIP 0:
 * dense; a fixed L spends its own bound; L >= 150 drops only exact zeros
 * (bitwise the dense result); -1 (auto): the smallest L in [16, 149] with
 * max_j e_j <= budget_mean (sbo_get_stream's; nothing accumulates), else 150.
 * All floating-point sums run in a fixed order, the counts are integer sums
 * and the keys' order is total: two calls agree bitwise.
 *
 * SBO_E_STATE exactly as sbo_whatif.  SBO_E_INVAL for samples outside
 * [1, 1024], first < 0, first + samples > 2^20, features outside [1, 4096],
 * NULL keys, or a fit of more than 2^24 points (eps's counter).  Alters no fitted or kept state; its workspace is freed by
 * sbo_trim. */
typedef struct sbo_sample_info {
    uint32_t struct_size;            /* caller sets; no more than this many bytes are written */
    int32_t  cutoff_log2;            /* L (0: dense) */
    int64_t  samples, first, m, n, features;
    int64_t  tiles_total, tiles_kept;   /* (query block, k-tile) pairs */
    double   err_path;               /* rigorous bound on |path error| from the cutoff: max_j sf2 2^-L |w_j|_1 */
    double   kernel_err;             /* measured: max |k^(d)/sf2 - exp(-|d|^2 / 2 l^2)| on the lattice above */
    double   w_l1_max;               /* max_j |w_j|_1 */
    double   ms;                     /* device time of the call's kernels */
} sbo_sample_info;
SBO_API sbo_status sbo_sample(sbo_ctx *ctx, uint64_t seed, int64_t first, int64_t samples, int64_t features,
                              double beta, double f_min, int64_t index_offset,
                              sbo_key *keys,          /* samples: argmax of path_j over the safe set */
                              int64_t *count_above,   /* samples: #{q : path_j(q) > f_min}; may be NULL */
                              double *paths,          /* samples x m row-major, caller's query order; may be NULL */
                              sbo_sample_info *info, uint32_t flags);

/* Test accessor: sbo_sample's auto cutoff alone, on the host (no context, no
 * device).  w_l1: per sample |w_j|_1.  *cutoff_log2 = the smallest L in
 * [16, 149] with sf2 2^-L max_j |w_j|_1 <= budget_mean, 150 if none is, 0
 * (dense) when budget_mean <= 0; *err_path = sf2 2^-L max_j |w_j|_1 (0 when
 * dense). */
SBO_API sbo_status sbo_debug_sample_cutoff(int64_t samples, const double *w_l1, double sf2, double budget_mean,
                                           int32_t *cutoff_log2, double *err_path);

/* Test accessor: the standard normals the device generates for sbo_sample, to
 * host buffers: nu (2 features), ab (samples x 2 features row-major: a then b
 * of each sample) and eps (samples x n row-major, the caller's training
 * order).  Needs a fitted context. */
SBO_API sbo_status sbo_debug_sample_draws(sbo_ctx *ctx, uint64_t seed, int64_t first, int64_t samples,
                                          int64_t features, double *nu, double *ab, double *eps);

/* Sweep work of each query under the current fit: builds the tick's tile
 * plan for these queries (no sweep) and writes cost[i] = the k-tiles its
 * 128-query block multiplies, summed over row blocks and weighted by their
 * precision level's sweep time (1, 42/64, 33/64 for six, three, one
 * product(s)), / the block's size, in the caller's order.  For cost-balanced M-sharding across ranks (every
 * rank computes the same costs from the same inputs: the plan is
 * deterministic); no reference counterpart. */
SBO_API sbo_status sbo_query_cost(sbo_ctx *ctx, const float *qx, const float *qy, int64_t m, float *cost,
                                  uint32_t flags);

/* Combine two shard keys (the cross-rank reduction of sbo_tick / sbo_argmax). */
SBO_API sbo_key sbo_key_combine(sbo_key a, sbo_key b);

/* Reduce n keys (e.g. the P keys of a cross-rank all-gather) to one by the
 * sbo_key_combine rule.  With SBO_DEVICE_PTRS keys and out are device
 * pointers and the reduction is one workgroup on the context's stream (with
 * SBO_ASYNC nothing synchronises: the combined key stays on the device, so a
 * sharded tick needs no host round trip per step); otherwise host memory. */
SBO_API sbo_status sbo_keys_reduce(sbo_ctx *ctx, const sbo_key *keys, int64_t n, sbo_key *out, uint32_t flags);

/* Host-side node logic (no device needed) ---------------------------------
 * FindSafetyContourIndices() (:418-497): rasterise safe into a
 * height x width image with the node's int-truncated bounds, trace external
 * contours (cv::findContours RETR_EXTERNAL, CHAIN_APPROX_NONE restated) and
 * map contour pixels back to grid indices (last writer wins, duplicates kept).
 * Dx/Dy are D_.col(0)/D_.col(1) (f64).  Writes at most out_cap indices,
 * stores the total in *count; returns SBO_E_INVAL if out_cap was too small. */
SBO_API sbo_status sbo_find_safety_contour_indices(const double *Dx, const double *Dy,
                                                   const uint8_t *safe, int64_t m,
                                                   int width_cells, int height_cells,
                                                   int32_t *out, int64_t out_cap, int64_t *count);

/* GetNextSubgoal() (:499-550): frontier, distance sort to the goal, top
 * max(1, F/4), strict-> argmax of Q(:,1)-Q(:,0).  Returns the grid index or -1. */
SBO_API int64_t sbo_next_subgoal(const double *Dx, const double *Dy, const double *lo,
                                 const double *hi, const uint8_t *safe, int64_t m,
                                 int width_cells, int height_cells, double goal_x, double goal_y);

/* The same two steps on device-resident grid data: with
 * SBO_DEVICE_PTRS, Dx/Dy/lo/hi/safe are device arrays (e.g. the tick's own
 * outputs); the O(M) raster -- bounds, pixel arithmetic, the last-writer
 * maps -- runs on the GPU and only the width x height image crosses to the
 * host for the border follow.  Results are identical to the host functions
 * above for finite coordinates (non-finite ones: the device bounds ignore
 * them).  Without the flag they call the host functions.  `out` is host
 * memory; count receives the frontier size even when out_cap is too small
 * (SBO_E_INVAL).  *index = -1 when there is no frontier. */
SBO_API sbo_status sbo_frontier(sbo_ctx *ctx, const double *Dx, const double *Dy, const uint8_t *safe,
                                int64_t m, int width_cells, int height_cells, int32_t *out,
                                int64_t out_cap, int64_t *count, uint32_t flags);
SBO_API sbo_status sbo_subgoal(sbo_ctx *ctx, const double *Dx, const double *Dy, const double *lo,
                               const double *hi, const uint8_t *safe, int64_t m, int width_cells,
                               int height_cells, double goal_x, double goal_y, int64_t *index,
                               uint32_t flags);

/* Post-selection geometry, host, f64.  Rings are the
 * exterior ring as Boost stores it: x[] / y[], closing point included.
 * sbo_polygon_correct: bg::correct for polygon<point, false, true> (the
 * node's :682): closes an open ring (needs cap >= n + 1) and reverses a
 * clockwise one; *n_out = new length.
 * sbo_polydist: polydist (src/libraries/polygeom_lib.cpp:401-474) including
 * its nearest-vertex quirk (:439-440); SBO_E_EMPTY for fewer than 2 ring
 * points, with the reference's intended dist 1e8 and point (0, 0).
 * sbo_point_within: bg::within(point, polygon) (:657), 1 strictly inside,
 * 0 outside or on the boundary.
 * sbo_project_subgoal: the node's step after GetNextSubgoal (:651-704): the
 * goal when within the ring (returns 1); else (Dx, Dy)[subgoal_index]
 * projected by polydist onto the corrected ring (returns 0); -1 when there
 * is no subgoal (index < 0) or the ring is empty. */
SBO_API sbo_status sbo_polygon_correct(double *rx, double *ry, int64_t n, int64_t cap, int64_t *n_out);
SBO_API sbo_status sbo_polydist(const double *rx, const double *ry, int64_t n, double px, double py,
                                double *proj_x, double *proj_y, double *dist);
SBO_API int sbo_point_within(const double *rx, const double *ry, int64_t n, double px, double py);
SBO_API int sbo_project_subgoal(const double *rx, const double *ry, int64_t n, double goal_x, double goal_y,
                                int64_t subgoal_index, const double *Dx, const double *Dy, int64_t m,
                                double *out_x, double *out_y, double *out_dist);

/* Bounding box of the fitted training points (x0, x1, y0, y1), widened by
 * every sbo_append and carried through sbo_export_state / sbo_import_state:
 * the extent the service grid spans by default (mapper side of :583-586).
 * Unchanged by sbo_remove, on either of its paths: it remains a box that
 * contains the points, and the probe lattice and the centre sbo_sample uses
 * stay put.  SBO_E_STATE before the first fit. */
SBO_API sbo_status sbo_get_bounds(const sbo_ctx *ctx, double *bounds);

/* The diagonal jitter added by SBO_OPT_JITTER_RETRIES to the current fit
 * (0.0 when the first factorization succeeded).  SBO_E_STATE before a fit. */
SBO_API sbo_status sbo_get_jitter(const sbo_ctx *ctx, double *jitter);

/* Fitted predictive state as one device blob (fit on one
 * rank, broadcast the operand to the others instead of refitting there).
 * sbo_state_bytes gives the size (the packed sf2 L^-1 tiles dominate:
 * ~2 N^2 B), sbo_export_state writes it into a caller device buffer,
 * sbo_import_state restores it into another context on any device.  An
 * imported context predicts, ticks and reports like the original (bitwise
 * identical sweeps) but holds no factor: sbo_append / sbo_get_factor return
 * SBO_E_STATE until the next sbo_fit.  sbo_import_state rejects
 * (SBO_E_INVAL) a blob whose magic, size, section offsets, header fields
 * or training order do not match what (n, npad) implies.  A rejected buffer
 * or header leaves a fitted context as it was; any error after the header is
 * accepted (a failed copy, a training order that is no permutation) leaves
 * the context unfitted, as a failed sbo_fit does. */
SBO_API sbo_status sbo_state_bytes(sbo_ctx *ctx, int64_t *bytes);
SBO_API sbo_status sbo_export_state(sbo_ctx *ctx, void *dev_buf, int64_t cap);
SBO_API sbo_status sbo_import_state(sbo_ctx *ctx, const void *dev_buf, int64_t bytes);

/* Raw border follower used by the frontier: img is height x width u8
 * row-major; points (x,y) pairs; start[c]..start[c+1] bound contour c.
 * Returns the number of contours, or -1 if a capacity was exceeded. */
SBO_API int64_t sbo_find_contours_external(const uint8_t *img, int width, int height,
                                           int32_t *pts, int64_t pts_cap,
                                           int64_t *start, int64_t contours_cap);

/* Staged-parity accessors (tests) ----------------------------------------
 * RBF fill alone (a1): writes the n x n column-major K (lda = n). */
SBO_API sbo_status sbo_rbf_fill(sbo_ctx *ctx, const float *x, const float *y, int64_t n,
                                sbo_hyper hyper, float *K, uint32_t flags);
/* Copy out the current factor L (n x n column-major, lower; upper part
 * zeroed) and alpha (n), both in the internal training order (sbo_get_order). */
SBO_API sbo_status sbo_get_factor(sbo_ctx *ctx, float *L, float *alpha, uint32_t flags);

/* The k-d order sbo_fit stores host points in (SBO_OPT_SPATIAL_ORDER 3):
 * perm[j] = the caller's index of stored row j, for n points whose first lands
 * at position first_offset of a 64-point k-tile (0 for a fit; sbo_append's
 * batch starts at the current N).  Host pointers, no context, no device. */
SBO_API sbo_status sbo_kd_order(const float *x, const float *y, int64_t n, int64_t first_offset, int64_t *perm);

/* The layout of the recursive f64 inverse of an n-column factor (leading
 * dimension ld) as the fit plans it, for base size `base`, `panels`, leaves
 * mode 0 / 1 / 2 (SBO_OPT_INV_LEAVES), `digits` wanted, the effective smallest
 * sliced split oz_min and 1 or 2 lanes: int64 records of 12 values.  Record 0:
 * {nodes, scratch doubles, leaves-by-doubling scratch doubles, leaves by
 * doubling, first 128-column info slot, info slots, workspace bytes of lane 0,
 * of lane 1, info slots of the top node's first half, two-lane top, 0, 0};
 * then one record per node in the recursion's order: {first column, n, split
 * h (0: a base case), offset of its S in the scratch (-1: none), first info
 * slot, sliced, lane, left child, right child (node indices, -1: none),
 * workspace bytes its products need, 0, 0}.  *count: the values the plan
 * takes; they are written when cap >= *count (cap 0 only asks for the count).
 * No context, no device. */
SBO_API sbo_status sbo_debug_inverse_plan(int64_t n, int64_t ld, int64_t base, int64_t panels, int leaves, int digits,
                                          int64_t oz_min, int lanes, int64_t *out, int64_t cap, int64_t *count);

/* Options.  SBO_OPT_INVERSE_BITS (32 | 64, default 64): precision in which
 * L^-1 is computed before sf2 * L^-1 is rounded to f32 for the predictive
 * sweep (64 = widen L, rocsolver_dtrtri; 32 = rocsolver_strtri).  Takes
 * effect at the next sbo_fit / sbo_append. */
#define SBO_OPT_INVERSE_BITS 1
/* SBO_OPT_SPATIAL_ORDER (0 caller order | 1 Hilbert | 2 Morton | 3 k-d,
 * default 3): store the training points spatially sorted (sbo_fit sorts all
 * points, sbo_append sorts each batch), so every 64-point k-tile of the
 * predictive sweep is spatially compact -- Hilbert: no Morton jumps inside
 * a tile (12 % fewer tiles pass the cutoff at C3 than Morton); k-d:
 * recursive bisection across the longer side into whole k-tiles, 16 %
 * smaller tile boxes than Hilbert on scattered points (C4 sweep 23.5 ->
 * 22.4 ms).  The
 * posterior does not depend on the order; sbo_get_factor returns the factor
 * of the internally ordered K and sbo_get_order the caller's index of each
 * internal row.  Takes effect at the next sbo_fit / sbo_append. */
#define SBO_OPT_SPATIAL_ORDER 2
/* SBO_OPT_TILE_SKIP (-1 | 0 | L in [16, 1000], default -1): skip a k-tile
 * for a workgroup of queries when the two bounding boxes are so far apart
 * that every K* entry of the block is below 2^-L (|d| > l sqrt(2 L ln 2)).
 * 0: dense sweep.  L >= 150: the dropped entries are exactly +0.0 in f32 and
 * the result is bitwise identical to the dense sweep.  -1 (auto): L is the
 * smallest exponent whose worst-case effect -- 2^-L max_i |(sf2 L^-1)_i|_1 on
 * any V entry, hence 2 sqrt(N sf2) times that on sigma^2, and
 * 2^-L |sf2 alpha|_1 on any mean -- stays below 2^-B sf2 (resp. 2^-B
 * sqrt(sf2)), B = SBO_OPT_SKIP_BUDGET, computed from the fitted factor
 * (sbo_get_skip reports it). */
#define SBO_OPT_TILE_SKIP 3
/* SBO_OPT_QUERY_ORDER (0 | 1 | 2, default 1): the order the queries of a
 * tick are swept in, so that each workgroup's 128 queries are spatially
 * compact and skip more k-tiles -- 0 the caller's order; 2 Morton order
 * (device radix sort, ~0.1 ms per 10^6 points); 1 (default) 8 x 16 grid
 * patches when the queries are a raster grid (rows of one coordinate, the
 * other repeating row by row; a contiguous run of rows cut anywhere
 * qualifies; detected with one stream synchronization per new query
 * buffer, and the patch layout is a valid order for whatever the buffer
 * later holds), else Morton order.  Outputs and argmax indices stay in the
 * caller's order. */
#define SBO_OPT_QUERY_ORDER 4
/* SBO_OPT_KERNEL_VARIANT, the predictive sweep: 3 (default) = split
 * operands on bf16 MFMA -- sf2 L^-1 and K* as three bf16 pieces each, up to
 * six v_mfma_f32_16x16x32_bf16 products per f32 product, f32 accumulation,
 * eight waves per CU; with the automatic cutoff the tile plan runs tiles
 * whose share of the variance is small at three or one product(s), charged
 * to the same error budget as the skipped tiles (SBO_OPT_SKIP_BUDGET);
 * 22 = variant 3 with every kept tile at six products (f32-accurate:
 * variance error vs a host f64 sweep 5.07e-6 at N = 16384 against 5.00e-6
 * for variant 0); 0 = f32 MFMA (16x16x4) with an f32 cross-tile
 * accumulator; 1 = variant 0 with an f64 one.  Any other value: SBO_E_INVAL.
 * (The other shapes and the timing diagnostics -- some leave parts of the
 * work out -- exist only in the diagnostic build lib/libsbo_diag.so, never
 * in this library.) */
#define SBO_OPT_KERNEL_VARIANT 5
/* SBO_OPT_SWEEP_GROUPS: workgroups of the persistent predictive sweep, each
 * walking one tile-balanced range of the tick's plan; 0 = default (one per
 * CU).  Results do not depend on it (bitwise). */
#define SBO_OPT_SWEEP_GROUPS 6
/* SBO_OPT_SKIP_BUDGET (B in [10, 60], default 20): the automatic K* cutoff
 * (SBO_OPT_TILE_SKIP = -1) keeps its worst-case error below 2^-B sf2 on any
 * variance and 2^-B sf2^(1/2) on any mean (2^-20 = 9.5e-7: under 10 % of the
 * 1e-5 contract; the measured effect at B = 18..27 is below the f32
 * rounding of the sweep itself).  Takes effect at the next sbo_fit /
 * sbo_append. */
#define SBO_OPT_SKIP_BUDGET 7
/* SBO_OPT_CHOLESKY (1 default | 2 | 0): the fit's factorization -- 1 the
 * library's blocked right-looking Cholesky (a one-workgroup kernel per
 * 128-column diagonal block, its own panel triangular solve, rocBLAS sgemm +
 * ssyrk for the trailing update with a look-ahead column), 2 the same with
 * rocBLAS strsm for the panel, 0 rocSOLVER spotrf.  Same f32 algorithm class
 * and the same NOT_SPD reporting (leading minor). */
#define SBO_OPT_CHOLESKY 8
/* SBO_OPT_INVERSE (1 default | 0): how the fit computes the f64 L^-1 of
 * SBO_OPT_INVERSE_BITS = 64 -- 1 the library's block recursion (rocSOLVER
 * dtrtri on diagonal blocks of <= 2048, the off-diagonal products as
 * panelled dgemms that leave out the zero half of each triangular factor:
 * n^3/3 flops), 0 rocsolver_dtrtri on the whole factor (its recursion
 * multiplies the triangles as full matrices: 2n^3/3).  Same algorithm
 * class; results agree to f64 rounding.  Takes effect at the next sbo_fit. */
#define SBO_OPT_INVERSE 9
/* SBO_OPT_JITTER_RETRIES (R in [0, 8], default 0): an sbo_fit whose
 * factorization fails (SBO_E_NOT_SPD: duplicate points with no noise, or a
 * kernel matrix singular in f32) is retried up to R times with
 * sf2 * 10^(r-7) added to the diagonal at retry r (1e-6 sf2, 1e-5 sf2, ...).
 * The jitter that succeeded becomes part of the noise term (appends and
 * exported state use it too) and sbo_get_jitter reports it; 0 keeps the
 * reference's behaviour of reporting the failure. */
#define SBO_OPT_JITTER_RETRIES 10
/* SBO_OPT_PRECISION (-1 auto default | 0 fast | 1 precise): the predictive
 * sweep's arithmetic.  0: the split-operand bf16 sweep (f32-accurate products,
 * f32 accumulation, A = sf2 L^-1 rounded to f32).  1: the precise sweep -- A
 * in f64 from the fit's f64 inverse, products and sums to f64 accuracy by
 * the kernel SBO_OPT_PRECISE_KERNEL names (default 3: int8 digit slices on
 * the int8 matrix cores, K*'s digits from a table; 0: f64 MFMA); about 3-5x
 * the fast sweep's time on the same tiles.  -1: every sbo_fit, and an
 * sbo_append once N has grown by SBO_OPT_REPROBE percent (default 25) since
 * the last probe, sweeps a probe set both ways -- a 32 x 32 lattice over the
 * training box and at most 512 training locations, the stored points at
 * positions stride / 2 + i stride over all of [0, n) with stride =
 * ceil(n / 512) (SBO_OPT_PROBE_SIZE, sbo_get_probe) -- and ticks with the
 * precise sweep when the fast sweep's variance error there, max |d var| /
 * max var, exceeds 5e-6 (5e-6 * 2^(20 - B) for a looser SBO_OPT_SKIP_BUDGET
 * B < 20).  The threshold rests on the envelope whole-grid error <=
 * 1.62 * probe + 1e-6 (9.1e-6 at the threshold, inside the 1e-5 contract),
 * calibrated at N = 8192 and held at the threshold itself by
 * tests/test_gpu_probe_decision.py: dense data, where the
 * variance is orders below sf2 and sf2 - |V|^2 cancels (config/lpsc.yaml's
 * own box from a few hundred points on), runs precise.  The precise sweep's
 * skip budget is 2^-B times the smallest probe variance
 * (SBO_OPT_SKIP_BUDGET = B).  Needs
 * SBO_OPT_INVERSE_BITS 64 and a fitted factor: an imported state always runs
 * the fast sweep.  Setting it on a fitted context takes effect at once. */
#define SBO_OPT_PRECISION 11
/* SBO_OPT_RESORT (percent, default 25; 0: never): sbo_append sorts each
 * batch only among itself (k-d), so scattered batches leave k-tiles whose
 * boxes span the domain and defeat the sweep's tile skipping.  Once the
 * points appended since the last sort exceed this share of the sorted ones,
 * the append re-sorts all points and refactors (a fit's cost, amortised over
 * the appends in between); otherwise it is the block Cholesky update.  The
 * posterior is the same either way (to f32 factorization rounding); caller
 * indices (sbo_get_order) are kept. */
#define SBO_OPT_RESORT 12
/* SBO_OPT_CHOL_RESERVE (CUs, default 0): the blocked Cholesky's trailing
 * updates (the look-ahead's second stream) run on a CU-masked stream that
 * leaves this many CUs free for the latency-bound chain of diagonal blocks and
 * panels.  Results do not depend on it (bitwise). */
#define SBO_OPT_CHOL_RESERVE 13
/* SBO_OPT_INV_OVERLAP (CUs, default 0: off): with the recursive f64 inverse,
 * its first half (the inverse of the factor's leading half and the product
 * below it: half the inverse's flops) starts as soon as the factor's left
 * half is final and runs beside the Cholesky's last steps, on a CU-masked
 * stream that leaves this many CUs to the factorization's latency-bound
 * chain.  Results do not depend on it (bitwise). */
#define SBO_OPT_INV_OVERLAP 14
/* SBO_OPT_CHOL_OUTER (columns, default 1024 since round 6; a multiple of
 * 128 in [128, 4096]): the blocked Cholesky's outer panel.  Each outer panel
 * is factored by the 128-column chain with its updates kept inside the
 * panel, and the rest of the trailing matrix takes one rank-1024 update per
 * outer panel; 128 is the one-level factorization (a rank-128 update per 128
 * columns).  1024 against 512: C4 fit -0.4 ms, the factor's backward error
 * 1.38e-7 -> 1.43e-7 (synthetic) and 8.7e-8 -> 9.5e-8 (lpsc box) at
 * N = 8192.  (Round 5 kept 512 when test_tile_skip_exact_and_bounded failed
 * at 1024; that leg compared a refit taking five inverse digits with the
 * first fit's dense sweep -- inverse drift, not the factor's -- and is fixed.) */
#define SBO_OPT_CHOL_OUTER 15
/* SBO_OPT_CHOL_DIAG (default 1): the blocked Cholesky's chain kernels -- the
 * 128 x 128 diagonal blocks (16-column panels) and the panel solves below
 * them -- with their inner updates on the matrix cores, left-looking (1: one
 * MFMA chain per block from every finished column, in registers) or
 * right-looking (2: each finished panel's update through LDS), or on the VALU
 * (0); the factor is bitwise the same. */
#define SBO_OPT_CHOL_DIAG 16
/* SBO_OPT_CHOL_GEMM (default 4): the blocked Cholesky's updates.  4 / 5: the
 * outer panels' two big updates (the look-ahead block column and the lower
 * trailing triangle, k = 512) as the int8-sliced GEMM of csrc/ozgemm.hip with
 * 4 / 5 base-256 digits per row (exact int32 digit products, one f64
 * combination per element, f32 out), from one pack of the panel per outer
 * step; the chain's small updates by rocBLAS.  C4 fit 41.3 -> 37.3 ms (5
 * digits: 39.0); the factor's backward error 1.64e-7 -> 1.38e-7 (synthetic,
 * N = 8192) and 2.51e-7 -> 8.7e-8 on the lpsc box against rocBLAS's f32
 * GEMMs.  0: rocBLAS sgemm / ssyrk; 1 / 2: the library's f32 matrix-core
 * kernel for the small trailing updates / every update (exact f32 products;
 * the factors agree to f32 rounding).  (3, the outer updates on the bf16
 * matrix cores with each operand split in three -- faster than rocBLAS, but
 * the factor's backward error 2.6x worse on the box -- exists only in the
 * diagnostic build; SBO_E_INVAL here.) */
#define SBO_OPT_CHOL_GEMM 17
/* SBO_OPT_INV_BASE (default 2048, in [1024, 8192], rounded down to a multiple
 * of 128) and SBO_OPT_INV_PANELS (default 16, in [1, 64]): the recursive f64
 * inverse's base-case size (rocSOLVER dtrtri on the diagonal blocks at
 * multiples of it) and the number of dgemm panels each of its products is cut
 * into (fewer panels: larger GEMMs, more multiplied zeros).  SBO_OPT_INV_LEAVES
 * (default 2): every base case up front -- with four or more full base cases
 * by doubling from 128-column blocks (one batched dtrtri, then two
 * strided-batched dgemms per product and level), else in one strided-batched
 * dtrtri (1: always the latter; 0: one call per base case inside the
 * recursion).  Tuning only; the inverse agrees to f64 rounding. */
#define SBO_OPT_INV_BASE 18
#define SBO_OPT_INV_PANELS 19
#define SBO_OPT_INV_LEAVES 20
/* SBO_OPT_REPROBE (percent, default 25; 0: every append): with
 * SBO_OPT_PRECISION -1, an sbo_append runs the precision probe again once N
 * has grown by this share since the last probe (every sbo_fit probes). */
#define SBO_OPT_REPROBE 21
/* SBO_OPT_PRECISE_KERNEL (3 default | 1 | 0): the precise sweep's arithmetic --
 * 1 A = sf2 L^-1 as five and K* as four balanced base-256 int8 digit slices, the 14
 * leading slice products on the int8 matrix cores (v_mfma_i32_16x16x64_i8,
 * exact int32 sums), combined in f64 per k-tile (an Ozaki-style sliced
 * product; predict_oz.hip), K*'s digits built in the sweep for every row
 * block that reads a k-tile; 3 the same products with K*'s digits read from a
 * table built once per (128-query block, k-tile) (the queries in chunks that
 * fit SBO_OPT_TABLE_MB; sigma bitwise kernel 1's); 0 every product and sum in
 * f64 on the f64 matrix cores (v_mfma_f64_16x16x4_f64; predict_f64.hip).  All
 * meet the 1e-5 contract where the fast sweep cannot (SBO_OPT_PRECISION). */
#define SBO_OPT_PRECISE_KERNEL 22
/* SBO_OPT_TABLE_MB (default 0 = automatic: 1/32 of the free device memory,
 * within [256 MiB, 8 GiB]): device memory budget, MiB, of the K* table
 * SBO_OPT_PRECISE_KERNEL 3 sweeps through (the queries run in chunks of as
 * many 128-query blocks as fit it; at least one). */
#define SBO_OPT_TABLE_MB 23
/* SBO_OPT_INV_OZ (default 6; 5, 4; 0: rocBLAS dgemm): the recursive f64
 * inverse's products at splits of 4096 and more (S = L21 A^-1, X21 = -C^-1 S;
 * N <= 32768)
 * as an f64 GEMM emulated on the int8 matrix cores -- each row / column cut
 * into that many base-256 digits under its own power of two, the digit
 * products summed exactly in int32, combined in f64 (csrc/ozgemm.hip).  Its
 * error is relative to a row's and a column's largest entries (2^-40 / 2^-48
 * of them for 5 / 6 digits), not to each product's: six digits move the
 * posterior by < 5e-7 against the dgemm fit, five by up to 4e-6 (not for the
 * precise regime).  With SBO_OPT_INV_OZ_ADAPT the value is the most digits a
 * fit uses.  The SBO_OPT_INV_OVERLAP fit keeps the dgemm products. */
#define SBO_OPT_INV_OZ 24
/* SBO_OPT_INV_CHECK (default 1; 0 off; 2 after every full inverse): the
 * fit's run-time accuracy guard of its f64 inverse X.  On 32 queries (a 4 x 4
 * lattice over the training box and 16 training locations) it forms V0 = X k
 * and one refinement against the f32 factor, V1 = V0 + X (k - L V0), in f64,
 * and takes err = max |(sf2 - |V0|^2) - (sf2 - |V1|^2)| / max (sf2 - |V1|^2):
 * the inverse's own share of the variance error, which the precision probe
 * cannot see (its two sweeps read the same inverse).  With 1 it runs after an
 * inverse whose products were int8-sliced (SBO_OPT_INV_OZ); when err exceeds
 * 5e-7 (a twentieth of the 1e-5 contract) the fit recomputes the inverse with
 * dgemm products and checks it again (sbo_get_inverse_check).  Runs on a
 * stream of its own beside the fit's operand packs. */
#define SBO_OPT_INV_CHECK 25
/* SBO_OPT_PLAN_BLOCK (0 = row-block-major; bi << 8 | bq): the item order of
 * the precise sweep's plans -- blocks of bi row blocks x bq query blocks, so
 * that the sweep workgroups of one XCD share the K* table pieces of a query
 * block in their L2 as well as the A tiles of a row block.  Results do not
 * depend on it (items are computed independently). */
#define SBO_OPT_PLAN_BLOCK 26
/* SBO_OPT_PROBE_SIZE (grid << 16 | train; default 32 << 16 | 512): the
 * precision probe's query set -- a grid x grid lattice over the training box
 * and `train` training locations (SBO_OPT_PRECISION); the next fit or append
 * probes again. */
#define SBO_OPT_PROBE_SIZE 27
/* SBO_OPT_INV_OZ_MIN (0 automatic, default; 2048, 4096, 8192): the smallest
 * split of the recursive inverse whose two products run as the int8-sliced
 * GEMM (SBO_OPT_INV_OZ); the levels below keep dgemm products.  Automatic:
 * 2048 for N >= 12288, else 4096. */
#define SBO_OPT_INV_OZ_MIN 28
/* SBO_OPT_INV_OZ_ADAPT (default 1; 0 off): the sliced inverse's digits per
 * fit from the guard's last readings (SBO_OPT_INV_CHECK must be on).  Both
 * grow ~256x per digit dropped (200-1000x measured), so a fit at d digits
 * with readings e (variance) and e_mu (mean) lets the next fit -- same
 * hyper-parameters, N and training bounding-box area within [0.8, 1.25] of
 * its -- take five digits when max(e, e_mu) 256^(d - 5) <= tol / 8 (never
 * four).  That fit must read both within tol / 8: otherwise it is redone at
 * SBO_OPT_INV_OZ digits (fired = 1) and the data keeps SBO_OPT_INV_OZ digits
 * from then on.  The first fit after sbo_create / sbo_warmup, after an
 * option change or a hyper-parameter change takes SBO_OPT_INV_OZ digits.
 * sbo_get_inverse_check's digits say which ran. */
#define SBO_OPT_INV_OZ_ADAPT 29
/* SBO_OPT_STREAM_SHARE (s in [0, 20], default 10): each update of
 * sbo_tick_stream may spend 2^-s of the sweep's skip budget on its K* cutoff
 * (2^-10: a thousand updates before the bounds alone force a full sweep). */
#define SBO_OPT_STREAM_SHARE 30
/* SBO_OPT_STREAM_MAX_ROWS (R in [0, 65536], default 64): an sbo_tick_stream
 * with more rows appended since its last tick than this takes the full sweep
 * (0: every call after an append does). */
#define SBO_OPT_STREAM_MAX_ROWS 31
/* SBO_OPT_EVIDENCE_BUDGET (B in [10, 60], default 20; 0: dense): sbo_evidence's
 * k-tile pair cutoff may move grad[0] by at most 2^-B n (grad_err_bound says
 * what it spent). */
#define SBO_OPT_EVIDENCE_BUDGET 32
/* SBO_OPT_WHATIF_GEMM (0 default, 1): sbo_whatif's two products with the
 * triangular inverse run as rocBLAS dtrmm (0) or as dgemm over the stored zero
 * half (1: twice the arithmetic, rocBLAS's general kernels; measured slower at
 * N = 16384 for p = 16 .. 256, 3.5-4.1 against 2.5-3.5 ms). */
#define SBO_OPT_WHATIF_GEMM 33
/* SBO_OPT_REMOVE_MAX (b in [0, 65536], default 2): an sbo_remove of more
 * points than this refits the remaining ones instead of rotating them out one
 * chain after another (reason OVER_CAP; 0: always).  The default is the
 * largest power of two whose removal at uniformly random stored positions
 * takes at most 0.8 of the warm refit of the points left (the refit also
 * restores k-d-compact tiles): at N = 16384, b = 2 takes 13.9 ms against
 * 32.2 ms (0.43), b = 4 35.3 ms against 30.5 ms (1.16).  One point at the
 * first stored position, the worst case, takes 25.5 ms [25.4, 26.5] against
 * 32.3 ms [32.1, 32.5]: it wins by more than the run's spread, so the
 * rotations are not capped by their count (profiles/remove.log). */
#define SBO_OPT_REMOVE_MAX 34
SBO_API sbo_status sbo_set_option(sbo_ctx *ctx, int option, int64_t value);

/* The last inverse check (SBO_OPT_INV_CHECK) of the current fit, on m = 31
 * guard queries (a 4 x 4 lattice over the training box, 15 training
 * locations).  ran = 1 if it ran; digits = the SBO_OPT_INV_OZ digits of the
 * checked inverse (0: dgemm).  Two readings, each the inverse's own share of
 * the posterior measured by one f64 refinement against the f32 factor:
 *   err       the variance's, max |d var| / max var (err_grid / err_train:
 *             over the lattice / the training locations, each normalised by
 *             its own largest variance; var_max the largest variance);
 *   err_mean  the mean's, max |d mu| / max |mu| (mean_max = max |mu|), from
 *             the residual y - m0 refined the same way (round 6: alpha, and
 *             so mu_ of src/safe_bayesian_optimization_node.cpp:642, comes
 *             from the same inverse).
 * fired = 1 if a reading exceeded its bound and the inverse was recomputed:
 * a six-digit (SBO_OPT_INV_OZ) inverse whose err or err_mean exceeds tol is
 * recomputed with dgemm products; a reduced-digit one (SBO_OPT_INV_OZ_ADAPT)
 * already above tol / 8 with SBO_OPT_INV_OZ digits, itself checked (and
 * recomputed with dgemm products if that one exceeds tol).  err_fallback /
 * err_mean_fallback: the readings of the recomputed inverse (-1 when none
 * was); kept_digits: the digits of the inverse the fit kept (0: dgemm); ms
 * the checks' device time.  Appends keep the fit's result (their new rows
 * are dgemm / dtrmv products). */
typedef struct sbo_inv_check {
    int32_t ran, fired, digits, m;
    double err, err_grid, err_train, err_fallback, tol, var_max, ms;
    double err_mean, mean_max, err_mean_fallback;
    int32_t kept_digits, reserved;
} sbo_inv_check;
SBO_API sbo_status sbo_get_inverse_check(const sbo_ctx *ctx, sbo_inv_check *out);

/* Release the fit-time and tick-time workspaces the context keeps between
 * calls for speed (the recursive inverse's scratch and the int8-sliced GEMM's
 * packed operands -- about 2.1 GB at N = 16384, 8.5 GB at 32768 -- the inverse
 * check's, the append re-sort's staging copy, sbo_evidence's column norms and
 * work items, sbo_whatif's candidate weights, sbo_sample's weights and keys
 * and the precise sweep's K* table, up to SBO_OPT_TABLE_MB); they
 * are allocated again on the next call that needs them.  The fitted state
 * (factor, inverse, operands) stays, and so does sbo_tick_stream's kept
 * posterior (sbo_stream_reset frees that).  Waits for the context's streams. */
SBO_API sbo_status sbo_trim(sbo_ctx *ctx);

/* Startup warm-up for the node's first map (no reference counterpart: the
 * node pays its first request_terrain_map, node.cpp:568-623, on a cold
 * process): fits n_cap synthetic points with `hyper` and the context's
 * options, then sweeps an m_cap-point raster grid with the fast and the
 * precise sweep, so that every code object a fit and a tick load (the
 * library's kernels, rocBLAS / rocSOLVER / Tensile) is loaded and the
 * workspaces are sized for fits of up to n_cap points and ticks of up to
 * m_cap queries.  The context is left unfitted (as after sbo_create); its
 * options are unchanged.  Synchronous. */
SBO_API sbo_status sbo_warmup(sbo_ctx *ctx, int64_t n_cap, int64_t m_cap, sbo_hyper hyper);

/* The sweep the ticks run (precise = 1: the precise sweep) and the last probe
 * (SBO_OPT_PRECISION): the fast sweep's normwise variance error against the
 * precise one on the probe set (lattice and training locations) and that
 * set's smallest and largest variance (-1 when no probe ran).  SBO_E_STATE
 * before a fit. */
SBO_API sbo_status sbo_get_precision(const sbo_ctx *ctx, int *precise, double *probe_err, double *probe_var_min,
                                     double *probe_var_max);

/* The last precision probe in detail (SBO_OPT_PRECISION): its query set is a
 * 32 x 32 grid over the training box (m_grid points) and m_train training
 * locations (every ceil(n / 512)-th stored point over all n); err = the fast sweep's
 * max |d var| over both / the largest variance of both (the decision's
 * number, also sbo_get_precision's probe_err), err_grid / err_train = each
 * part's own max |d var| / its own largest variance.  err* = -1 when no
 * probe ran.  SBO_E_STATE before a fit. */
typedef struct sbo_probe {
    int32_t precise, m_grid, m_train, precise_kernel;   /* precise_kernel: SBO_OPT_PRECISE_KERNEL in effect */
    int64_t n_at_probe;
    double err, err_grid, err_train;
    double var_min, var_max, var_max_grid, var_max_train;
} sbo_probe;
SBO_API sbo_status sbo_get_probe(const sbo_ctx *ctx, sbo_probe *out);

/* The K* tile cutoff in effect (auto or fixed) and the norms it was derived from. */
SBO_API sbo_status sbo_get_skip(const sbo_ctx *ctx, int *cutoff_log2, double *max_row_l1, double *alpha_l1);

/* order[i] = the caller's index (position in the sbo_fit / sbo_append
 * inputs, appends numbered after the fit) of internal training row i. */
SBO_API sbo_status sbo_get_order(const sbo_ctx *ctx, int64_t *order);

/* Test accessor: the packed predictive operand A = sf2 * L^-1 unpacked into a
 * dense n x n ROW-major f32 host array (upper triangle left untouched). */
SBO_API sbo_status sbo_get_inverse(sbo_ctx *ctx, float *Linv);

/* Test accessor: the plan's per packed tile gain bounds, 8 floats per tile in
 * packed-tile order (row block I, k-tile t at tile_start(I) + t):
 * log2 of (16 max row 1-norm, spectral-norm bound, Frobenius norm, 0) of
 * A_It, then (16 max row 1-norm, spectral-norm bound) of its bf16 pieces A1
 * and A2 (-1000 for an all-zero matrix).  cap >= 8 * tiles. */
SBO_API sbo_status sbo_get_tile_bounds(sbo_ctx *ctx, float *bounds, int64_t cap);

/* Kernel timing (bench.py): when enabled, hipEvents are recorded on the
 * context's stream around every predictive-sweep and RBF-fill launch.
 * sbo_profile(ctx, 1) enables and resets; sbo_profile_read sums the elapsed
 * device time of the launches recorded so far (it synchronises on them). */
SBO_API sbo_status sbo_profile(sbo_ctx *ctx, int enable);
SBO_API sbo_status sbo_profile_read(sbo_ctx *ctx, double *predict_ms, int64_t *predict_launches,
                                    double *fill_ms, int64_t *fill_launches);
/* MFMA flops the predictive sweep actually executed since sbo_profile(ctx, 1)
 * (2*BM*BN*BK per multiplied tile; skipped exactly-zero tiles excluded). */
SBO_API sbo_status sbo_profile_work(sbo_ctx *ctx, double *predict_flops);
/* Matrix-core flops the predictive sweep issued since sbo_profile(ctx, 1):
 * 2*BM*BN*BK per MFMA product per multiplied tile -- six products per tile
 * for the split sweeps at full precision, three / one at the reduced
 * precision levels (variant 3), one for the f32 sweeps (variants 0, 1) and
 * the precise f64 sweep; tiles_by_level (may be NULL): the multiplied tiles
 * at six, three, one product(s). */
SBO_API sbo_status sbo_profile_mfma(sbo_ctx *ctx, double *mfma_flops, int64_t *tiles_by_level /* [3] or NULL */);
/* Diagnostic build only (libsbo_diag.so; the product returns zeros): with
 * SBO_OPT_KERNEL_VARIANT 39 (the default sweep with phase stamps,
 * s_memtime; never timed as the product) the summed cycles of every
 * sweep wave since the last call, cycles[0..11]: step top, half-step body,
 * item end, vmcnt wait, barrier, whole half-steps, body at six / three / one
 * product(s), half-steps at six / three / one product(s); then reset. */
SBO_API sbo_status sbo_debug_x3_stamps(sbo_ctx *ctx, double *cycles, int n);

/* Test accessor: the split (bf16 x3) operand of the fitted state, brought up
 * to date and copied to host memory, in the layout the split sweep stages
 * (csrc/predict_x3_rowhalf.hpp): packed tile T (the order of the f32 packed
 * operand), row half R, plane p, row block rb of the half, k half h, lane
 * l = 16 g + r holds A[16 (8R + rb) + r][32 h + 8 g + j], j = 0..7, as bf16 at
 * byte T*98304 + R*49152 + p*16384 + (2 rb + h)*1024 + l*16 + 2j.  *bytes is
 * the operand's size; host_buf may be null to ask for it alone. */
SBO_API sbo_status sbo_debug_x3_operand(sbo_ctx *ctx, void *host_buf, int64_t cap, int64_t *bytes);

/* Test accessor: which parts of the context's model are valid, as the first
 * min(cap, 13) of: [0] n, [1] npad, [2] fitted, [3] has_factor, [4] rows of the
 * f64 inverse, [5] rows of z, [6] N at the last probe, [7] the first row block
 * the split operand must be derived from for the kernel variant in effect (-1:
 * current), [8] the layout it was last derived in (-1: never), [9] / [10] the
 * same for the precise operand and SBO_OPT_PRECISE_KERNEL, [11] a precise pack
 * is in flight that the host has not waited for, [12] fit_epoch.  Nothing is
 * launched or waited for; valid on an unfitted context. */
SBO_API sbo_status sbo_debug_state(const sbo_ctx *ctx, int64_t *out, int cap);

/* Test accessor: the plan a tick of these m queries (host pointers) would
 * sweep under the context's options -- the plan sbo_query_cost builds; no
 * sweep runs -- as int32 in host_buf: [0] nI row blocks, [1] nQ query blocks
 * of 128 sweep positions (the queries in the tick's sweep order, padded grid
 * patches included), [2] the kept tiles, [3] the non-empty items; then per
 * item, at 4 + 2 (I nQ + qb): the budget threshold + 1 (thr) and the kept-tile
 * count; then per kept tile, in the order the sweep walks them, four ints: row
 * block I, query block qb, k-tile t, precision level (0 six, 1 three, 2 one
 * product(s)).  *n_out is the number of ints; host_buf may be null to ask for
 * it alone.  Diagnostic build only: with SBO_PLAN_REF=1 in the environment the
 * plan comes from the reference builder (every (row block, k-tile) pair's
 * bounds evaluated in every pass, no column prefilter), and ticks write and
 * read the partials of empty items. */
SBO_API sbo_status sbo_debug_plan(sbo_ctx *ctx, const float *qx, const float *qy, int64_t m, int32_t *host_buf,
                                  int64_t cap, int64_t *n_out);

/* Test accessors: the int8-sliced GEMM under the fit (csrc/ozgemm.hip), run
 * alone on the context's stream so that tests/test_gpu_ozgemm.py can hold the
 * product's object code bit for bit to an integer model (tests/oz_model.py).
 * C (m x n) = alpha op(A) op(B) (+ C), HOST pointers, column-major; op(A) is
 * m x K (A itself K x m with SBO_GZ_TRANS_A), op(B) K x n (B itself n x K with
 * SBO_GZ_TRANS_B).  Each row of op(A) and each column of op(B) is scaled by a
 * power of two above 1.01 times its largest magnitude, rounded to an integer
 * of 8 nd - 1 bits and cut into nd balanced base-256 digits; digit products of
 * level s + u < nd are summed exactly.  K in [1, 16384]; m == 0 or n == 0 is
 * SBO_OK and writes nothing; bad sizes, digits or flag combinations are
 * SBO_E_INVAL.  No inf, NaN or subnormal inside the logical operands. */
#define SBO_GZ_TRI_A 1u        /* op(A) lower triangular: a_ik = 0 for k > i; the zero part is not read */
#define SBO_GZ_TRANS_A 2u
#define SBO_GZ_TRI_B_LOWER 4u  /* op(B) lower triangular: b_kj = 0 for k < j; the zero part is not read */
#define SBO_GZ_TRI_B_UPPER 8u  /* op(B) upper triangular: b_kj = 0 for k > j; the zero part is not read */
#define SBO_GZ_TRANS_B 16u
#define SBO_GZ_TRANS_C 32u     /* C^T is stored: C points at n x m storage, ldc its leading dimension */
#define SBO_GZ_BETA1 64u       /* C += instead of C = */
#define SBO_GZ_LOWER_C 128u    /* (f32 only, not with SBO_GZ_TRANS_C) 128 x 128 tiles wholly above C's diagonal
                                  are left alone; tiles that meet the diagonal are written whole */
/* The f64 form (is_f32 == 0: double operands, nd 4, 5 or 6 -- the L^-1
 * recursion's) or the f32 form (is_f32 != 0: float operands, nd 4 or 5).  The
 * whole lda x a_cols, ldb x b_cols and ldc x c_cols buffers go to the device
 * and the whole C buffer comes back, padding included. */
SBO_API sbo_status sbo_debug_gz_gemm(sbo_ctx *ctx, int nd, int is_f32, const void *A, int64_t lda, int64_t a_cols,
                                     const void *B, int64_t ldb, int64_t b_cols, int64_t m, int64_t n, int64_t K,
                                     double alpha, void *C, int64_t ldc, int64_t c_cols, uint32_t flags);
/* The Cholesky's form: the mpack x K f32 panel P (leading dimension ld) is cut
 * into digits once, then C (m x n f32) = alpha P[a0 .. a0 + m) P[b0 .. b0 + n)^T
 * (+ C) is read from that pack.  nd 4 or 5; a0 and b0 multiples of 128, both
 * row ranges inside the pack; flags: SBO_GZ_BETA1, SBO_GZ_LOWER_C.  A
 * 16-byte-aligned C with ldc % 4 == 0 takes the vector epilogue, any other the
 * scalar one; the whole ld x K and ldc x c_cols buffers travel as above. */
SBO_API sbo_status sbo_debug_gz_gemm_packed(sbo_ctx *ctx, int nd, const float *P, int64_t ld, int64_t mpack,
                                            int64_t K, int64_t a0, int64_t m, int64_t b0, int64_t n, double alpha,
                                            float *C, int64_t ldc, int64_t c_cols, uint32_t flags);

#ifdef __cplusplus
}
#endif

#endif /* SBO_H_ */
