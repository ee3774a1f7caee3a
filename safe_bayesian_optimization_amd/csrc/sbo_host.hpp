// sbo_host.hpp -- what the host sources of libsbo.so share beside the context
// (sbo_internal.hpp): the status macros of a function that has `ctx` in scope
// and returns sbo_status, and the test for the second lane.  Host only.
#pragma once

#include <string>

#include "sbo_internal.hpp"

#define SBO_HIP(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            ctx->err = std::string(#expr) + ": " + hipGetErrorString(e_);               \
            return e_ == hipErrorOutOfMemory ? SBO_E_OOM : SBO_E_DEVICE;                \
        }                                                                               \
    } while (0)

#define SBO_BLAS(expr)                                                                  \
    do {                                                                                \
        rocblas_status s_ = (expr);                                                     \
        if (s_ != rocblas_status_success) {                                             \
            ctx->err = std::string(#expr) + ": " + rocblas_status_to_string(s_);        \
            return s_ == rocblas_status_memory_error ? SBO_E_OOM : SBO_E_DEVICE;        \
        }                                                                               \
    } while (0)

#define SBO_CHECK(cond, code, msg)                                                      \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            ctx->err = (msg);                                                           \
            return (code);                                                              \
        }                                                                               \
    } while (0)

// Has a blocked factorization run on this context?  Its set-up (chol_streams)
// leaves aux_stream, its rocBLAS handle and the events ev_panel, ev_trail,
// ev_pack, ev_poz, which the inverse's two-lane top level and the refresh's
// side work use without making them.  The four events are created together,
// so ev_panel stands for all of them.  The answer depends on history, not on
// the options now: a context whose fits so far all ran rocSOLVER's spotrf
// (SBO_OPT_CHOLESKY 0) has no aux stream and its refresh stays single-stream;
// one that has run the blocked factorization once keeps it.
inline bool aux_ready(const sbo_ctx *ctx) { return ctx->blas_aux && ctx->aux_stream && ctx->ev_panel; }
