// readers.hpp -- sbo_evidence, sbo_whatif and sbo_sample (readers.cpp) as stages over a
// plan: the call's sizes, the caller's pointers and the device pointers carved
// for it.  The stages between the device phases are pure.  Host only.
#pragma once

#include <cstdint>
#include <vector>

#include "sbo_internal.hpp"

namespace sbo {

struct EvidencePlan {
    int64_t n = 0, T = 0;                        // rows, k-tiles
    bool want_loo = false, host_loo = false;     // any LOO output; staged on the device for a host caller
    double *out_mean = nullptr, *out_var = nullptr;         // the caller's
    double *c = nullptr, *sums = nullptr, *res = nullptr;   // (K^-1)_ii, the tiles' kEvSums sums, grad[0]
    int64_t *order = nullptr;                               // want_loo: the rows' caller indices
    double *loo_mean = nullptr, *loo_var = nullptr;         // where the device writes them (null: not wanted)
};

// The tiles' sums (T x kEvSums) added in tile order into lml, data_fit, log_det, grad[1..3] and loo_log_pred
// (sn: noise_level with the jitter, noise: without); al1 / sl1: the tiles' |alpha|_1 and |sqrt(c)|_1.
void evidence_totals(const double *sums, int64_t T, int64_t n, double sn, double noise, sbo_evidence_info &r,
                     double *al1, double *sl1);
// The Gram phase's items from the drop map (T x T): kept pair I <= J x chunk of kEvChunk rows from 64 J, as
// (I, J, k0, first chunk of the pair), by the band of kEvChunk rows of k0, then J, then I; r's pair counts.
std::vector<int4> evidence_items(const uint8_t *drop, int64_t T, int64_t n, sbo_evidence_info &r);

struct WhatifPlan {
    int64_t n = 0, p = 0, pp = 0, m = 0;         // rows, candidates (rounded up to 16), kept queries
    bool host = false;                           // the caller's pointers are host memory
    size_t mat = 0;                              // p m: the entries of cov / lo_new
    double beta = 0.0, f_min = 0.0;
    int64_t *out_gain = nullptr;                 // the caller's
    double *out_mu = nullptr, *out_var = nullptr, *out_cov = nullptr, *out_lo = nullptr;
    double *Kt = nullptr, *Ut = nullptr, *Wt = nullptr, *part = nullptr;   // K_c^T, U^T, W^T (over K_c^T); the sums' chunks
    double *mu = nullptr, *var = nullptr, *l1 = nullptr, *par = nullptr;   // mu_c, var_c, |w_j|_1, the epilogue's factors
    unsigned long long *gain = nullptr, *kept = nullptr;                   // p counts, then the sweep's tiles
    const float *cx = nullptr, *cy = nullptr;    // the candidates on the device
    double *cov = nullptr, *lo = nullptr;        // where the sweep writes them (null: not wanted)
};

struct SamplePlan {
    int64_t n = 0, S = 0, pp = 0, F = 0, Fp = 0, m = 0;   // rows, samples (rounded up to 16), features (to 4), kept queries
    int64_t pw = 0;                              // samples rounded up to the products' row chunk: T^T, U^T, W^T's leading dimension
    int64_t first = 0, index_offset = 0, nb = 0;          // the first sample's number; the sweep's query blocks
    uint64_t seed = 0;
    bool host = false;                           // the caller's pointers are host memory
    size_t mat = 0;                              // S m: the entries of paths
    double beta = 0.0, f_min = 0.0, cx0 = 0.0, cy0 = 0.0;   // (cx0, cy0): the centre of the training bounding box
    sbo_key *out_keys = nullptr;                 // the caller's
    int64_t *out_count = nullptr;
    double *out_paths = nullptr;
    double *Tt = nullptr, *Ut = nullptr, *Wt = nullptr, *Theta = nullptr;   // T^T, U^T, W^T (over T^T), Theta^T
    double *wx = nullptr, *wy = nullptr;         // the frequencies in turns
    int64_t *order = nullptr;                    // the rows' caller indices
    double *part = nullptr, *l1 = nullptr, *junk = nullptr;   // the sums' chunks, |w_j|_1, the sums sbo_sample does not use
    unsigned long long *count = nullptr, *kept = nullptr, *kerr = nullptr;   // S counts, the sweep's tiles, kernel_err's bits
    sbo_key *pkeys = nullptr, *keys = nullptr;   // S x nb partial keys, S keys
    double *paths = nullptr;                     // where the sweep writes them (null: not wanted)
};

}  // namespace sbo
