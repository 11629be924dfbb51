// Host plumbing shared by the iterative solvers on the Toeplitz normal operator (cg.cpp, fista.cpp, tv.cpp, lps.cpp; dcf.cpp and
// precond.cpp use the generic pieces): the argument checks at the head of every *_solve, the outcome block of the proximal solvers
// (ProxScalars of solver_decide.h: its layout, its allocation and its copy-out), the check_every poll and the entries that read an
// outcome back.  Host only; DESIGN.md section 23.  Everything here has internal linkage: the library exports nothing new.
#pragma once

#include <cmath>

#include "host_common.h"
#include "solver_decide.h"

namespace nufft {

static inline bool weight_ok(double v) { return std::isfinite(v) && v >= 0.0; }

static inline int toeplitz_info(const nufft_toeplitz* tz, nufft_toeplitz_info& ti) {
    std::memset(&ti, 0, sizeof(ti));
    ti.struct_size = (int32_t)sizeof(ti);
    return nufft_toeplitz_get_info(tz, &ti);
}

// The number of compute units that sizes the streaming grids; 256 where the query fails.
static inline int device_cus(int device) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) return cus;
    (void)hipGetLastError();
    return 256;
}

// A solve that polls its done flags synchronises the stream.
static inline int refuse_polling_capture(int check_every, hipStream_t stream) {
    if (check_every > 0 && capturing(stream))
        return fail(NUFFT_ERR_INVALID_ARG, "check_every > 0 synchronises the stream: not on a capturing stream (use check_every = 0)");
    return NUFFT_OK;
}

// The head of every *_solve, under the caller's DeviceGuard: the operator has its spectrum, x and b are tables of C aligned vectors of n
// complex elements, x is apart from b and from itself, and a solve that polls is not captured.
static inline int check_solve_args(const nufft_toeplitz* tz, const char* entry, int C, int64_t n, int dtype, void* const* x, const void* const* b,
                            int check_every, hipStream_t stream) {
    nufft_toeplitz_info ti;
    if (int rc = toeplitz_info(tz, ti)) return rc;
    if (!ti.has_spectrum)
        return fail(NUFFT_ERR_NO_POINTS, std::string("nufft_toeplitz_set_spectrum or nufft_toeplitz_set_points must be called before ") + entry);
    if (!x || !b) return fail(NUFFT_ERR_INVALID_ARG, "null table");
    const size_t bytes = (size_t)n * 2 * real_bytes(dtype);
    for (int c = 0; c < C; ++c) {
        if (!x[c] || !b[c]) return fail(NUFFT_ERR_INVALID_ARG, "null data vector");
        if (((uintptr_t)x[c] | (uintptr_t)b[c]) & 15) return fail(NUFFT_ERR_INVALID_ARG, "x and b must be 16-byte aligned");
    }
    for (int c = 0; c < C; ++c)
        for (int k = 0; k < C; ++k) {
            if (overlap(x[c], b[k], bytes)) return fail(NUFFT_ERR_INVALID_ARG, "x overlaps b: the right-hand side is read while x is written");
            if (k != c && overlap(x[c], x[k], bytes)) return fail(NUFFT_ERR_INVALID_ARG, "two components of x overlap");
        }
    return refuse_polling_capture(check_every, stream);
}

// ProxScalars in one block of `count` slots: double change[count]; int32 flag[count], iters[count], status[count]
static inline size_t prox_scal_bytes(int count) { return (size_t)count * (sizeof(double) + 3 * sizeof(int32_t)); }

static inline ProxScalars prox_scalars_at(void* base, int count, void* hist) {
    ProxScalars k{};
    k.change = static_cast<double*>(base);
    k.flag = reinterpret_cast<int32_t*>(k.change + count);
    k.iters = k.flag + count;
    k.status = k.flag + 2 * count;
    k.history = static_cast<double*>(hist);
    return k;
}

// The history and the mirrored scalars of a solver, with a defined answer from its get_result / history before the first solve: zeros
// and NaN.  `scal_bytes`: prox_scal_bytes(count), or the size of a solver's own block.  The caller releases what was allocated when this
// fails.
static inline int create_outcome(int64_t& own_bytes, const char* noun, ScalarMirror& scal, void** d_hist, size_t scal_bytes, size_t hist_bytes) {
    int rc;
    if ((rc = alloc_buffer(own_bytes, noun, d_hist, hist_bytes)) ||
        (rc = scal.create(own_bytes, noun, scal_bytes, "hipHostMalloc of the solver's host mirror failed")))
        return rc;
    if (scal.zero() != hipSuccess || hipMemset(*d_hist, 0xFF, hist_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(NUFFT_ERR_HIP, "hipMemset of the solver's scalars failed");
    }
    return NUFFT_OK;
}

// The check_every poll: the scalars come to the host (the stream is synchronised); done when all `count` flags are set.
static inline int all_done(ScalarMirror& scal, hipStream_t stream, const int32_t* flags, int count, bool* done) {
    if (int rc = scal.fetch(stream)) return rc;
    *done = true;
    for (int c = 0; c < count; ++c) *done = *done && flags[c] != 0;
    return NUFFT_OK;
}

// The entries that read an outcome back synchronise the stream.
static inline int refuse_capture(const char* entry, hipStream_t stream) {
    if (capturing(stream)) return fail(NUFFT_ERR_INVALID_ARG, std::string(entry) + " synchronises: not on a capturing stream");
    return NUFFT_OK;
}

static inline int fetch_history(const char* entry, double* host_out, const void* d_hist, size_t hist_bytes, hipStream_t stream) {
    if (int rc = refuse_capture(entry, stream)) return rc;
    NUFFT_HIP(hipMemcpyAsync(host_out, d_hist, hist_bytes, hipMemcpyDeviceToHost, stream));
    NUFFT_HIP(hipStreamSynchronize(stream));
    return NUFFT_OK;
}

// nufft_*_get_result of a proximal solver: component c reads slot c * stride (stride 0: one system, its slot for every component).
static inline int copy_result(const char* entry, ScalarMirror& scal, int count, int C, int stride, int32_t* iterations, int32_t* status, double* change,
                       hipStream_t stream) {
    int rc;
    if ((rc = refuse_capture(entry, stream)) || (rc = scal.fetch(stream))) return rc;
    const ProxScalars host = prox_scalars_at(scal.host, count, nullptr);
    for (int c = 0; c < C; ++c) {
        if (iterations) iterations[c] = host.iters[c * stride];
        if (status) status[c] = host.status[c * stride];
        if (change) change[c] = host.change[c * stride];
    }
    return NUFFT_OK;
}

}  // namespace nufft
