// sbo_host.hpp -- what the host sources of libsbo.so share beside the context
// (sbo_ctx.hpp): the status macros of a function that has `ctx` in scope
// and returns sbo_status, the tests of the fitted state, the scratch carver,
// the pooled events and the copy-out of a versioned info struct.  Host only.
#pragma once

#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "sbo_ctx.hpp"

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
// ev_pack, pop.ev, which the inverse's two-lane top level and the refresh's
// side work use without making them.  The four events are created together,
// so ev_panel stands for all of them.  The answer depends on history, not on
// the options now: a context whose fits so far all ran rocSOLVER's spotrf
// (SBO_OPT_CHOLESKY 0) has no aux stream and its refresh stays single-stream;
// one that has run the blocked factorization once keeps it.
inline bool aux_ready(const sbo_ctx *ctx) { return ctx->blas_aux && ctx->aux_stream && ctx->ev_panel; }

inline bool dev(uint32_t flags) { return (flags & SBO_DEVICE_PTRS) != 0; }

// The fit's f64 inverse holds exactly n rows: L^-1 in Linv, computed in f64
// (SBO_OPT_INVERSE_BITS 64), current for the first n training points.
inline bool inverse_current(const sbo_ctx *ctx, int64_t n) { return ctx->opt.inverse_bits == 64 && ctx->linv_n == n; }

// The fit's factor, f64 inverse and z = L^-1 (y - m0) hold all n rows: what the
// readers of the fitted state (the streaming update, sbo_evidence, sbo_whatif)
// need.  Not so for an imported state or below SBO_OPT_INVERSE_BITS 64.
inline bool fit_state_complete(const sbo_ctx *ctx, int64_t n) {
    return ctx->has_factor && inverse_current(ctx, n) && ctx->z_n == n;
}

// The skip budget of the sweep in effect (sbo_api.cpp, the streaming tick).
void stream_budget(const sbo_ctx *ctx, double &var, double &mean);

// tiles_total of a sweep over a kept posterior of ms positions and n columns
inline int64_t kept_tiles_total(int64_t ms, int64_t n) {
    return (ms + sbo::kBN - 1) / sbo::kBN * ((n + sbo::kBK - 1) / sbo::kBK);
}

// Sub-allocator over one scratch buffer (16-B aligned pieces).
struct Carve {
    char *base;
    size_t off = 0;
    explicit Carve(void *b = nullptr) : base(static_cast<char *>(b)) {}
    template <class T> T *take(size_t count) {
        T *p = reinterpret_cast<T *>(base + off);
        off += (count * sizeof(T) + 255) & ~size_t(255);
        return p;
    }
    static size_t need(size_t count, size_t sz) { return (count * sz + 255) & ~size_t(255); }
};

// An event from the context's pool (a new one when it is empty; null: hipEventCreate failed).
inline hipEvent_t take_event(sbo_ctx *ctx) {
    if (!ctx->ev_pool.empty()) {
        hipEvent_t e = ctx->ev_pool.back();
        ctx->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// Event bracket around one launch when profiling is on.
struct Bracket {
    sbo_ctx *ctx;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> *list;
    hipEvent_t a = nullptr, b = nullptr;
    // (on: a caller's own switch beside sbo_profile's, TickPlan::prof)
    Bracket(sbo_ctx *c, std::vector<std::pair<hipEvent_t, hipEvent_t>> &l, bool on = true) : ctx(c), list(&l) {
        if (!ctx->prof || !on) return;
        a = take_event(ctx);
        b = take_event(ctx);
        if (a) (void)hipEventRecord(a, ctx->stream);
    }
    ~Bracket() {
        if (!a || !b) return;
        (void)hipEventRecord(b, ctx->stream);
        list->emplace_back(a, b);
    }
};

// The four pooled events around the two device phases of a reader: ev[0] ..
// ev[1] the first, ev[2] .. ev[3] the second.  They go back to the pool on
// every path.
struct PhaseEvents {
    sbo_ctx *ctx;
    hipEvent_t ev[4];
    double ms = 0.0;   // after elapsed(): the two phases' device time
    explicit PhaseEvents(sbo_ctx *c) : ctx(c), ev{take_event(c), take_event(c), take_event(c), take_event(c)} {}
    PhaseEvents(const PhaseEvents &) = delete;
    PhaseEvents &operator=(const PhaseEvents &) = delete;
    ~PhaseEvents() {
        for (hipEvent_t e : ev)
            if (e) ctx->ev_pool.push_back(e);
    }
    bool ok() const { return ev[0] && ev[1] && ev[2] && ev[3]; }
    hipError_t record(int i) { return hipEventRecord(ev[i], ctx->stream); }
    hipError_t elapsed() {   // (all four recorded and the stream synchronized)
        float ms1 = 0.0f, ms2 = 0.0f;
        if (hipError_t e = hipEventElapsedTime(&ms1, ev[0], ev[1])) return e;
        if (hipError_t e = hipEventElapsedTime(&ms2, ev[2], ev[3])) return e;
        ms = (double)ms1 + (double)ms2;
        return hipSuccess;
    }
};

// A versioned info struct to the caller: as many bytes as the caller's
// struct_size names, struct_size set to what was written.
template <class Info> void copy_info(Info *out, Info r) {
    r.struct_size = (uint32_t)std::min<size_t>(out->struct_size, sizeof(r));
    memcpy(out, &r, r.struct_size);
}
