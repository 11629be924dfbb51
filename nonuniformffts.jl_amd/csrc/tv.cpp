// Total variation on the Toeplitz normal operator: the periodic difference operator (nufft_tv_*) and the primal-dual solver
// (nufft_tvpd_*) of include/nufft_mi355x.h; DESIGN.md section 25.
//
// Minimises, per component c (jointly over all components on a coupled operator),
//
//     ½ <x, (G + μ I) x> − Re<b, x> + tv_c · Σ_i |(∇x)_i|₂
//
// (∇x)_d[i] = x[i + e_d] − x[i], indices mod N_d, on the array as stored;  |(∇x)_i|₂ = sqrt(Σ_d |(∇x)_d[i]|²);
// (∇ᴴy)[i] = Σ_d (y_d[i − e_d] − y_d[i]).  Condat–Vũ / Chambolle–Pock with the smooth term taken by its gradient:
//
//     start:  x = x0 (or 0),  y_d = 0
//     per iteration:
//         q  = G x                                        the operator's apply, unchanged
//         x⁺ = x − τ (q + μ x − b + ∇ᴴ y)                 tv_primal kernel: stores x <- x⁺ and q <- x̄ = 2x⁺ − x,
//                                                         partials of ‖x⁺ − x‖², ‖x⁺‖²
//         y  <- P_tv(y + σ ∇x̄)                            tv_dual kernel, in place: P_t(v)_i = v_i · min(1, t / |v_i|₂);
//                                                         partial of Σ_i |(∇x⁺)_i|₂ (reads x⁺ too)
//         decide: change = ‖x⁺ − x‖ / ‖x⁺‖ (0 when both are 0); history row (change, Σ_i |(∇x⁺)_i|₂);
//                 done <- change <= tol, or change not finite (BREAKDOWN)
//
// τ = step, σ = sigma (0: 1 / (8 D τ)); with ‖∇‖² <= 4 D that gives 1/τ − σ ‖∇‖² >= L / 2 for τ <= 1 / L, the convergence condition.
//
// The host side only enqueues: per iteration one nufft_toeplitz_apply, the two stencil kernels and the decision kernel.  Every scalar
// lives on the device; with check_every > 0 the host looks at the done flags now and then, and at nothing else.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "host_common.h"
#include "stream_kernels.h"
#include "tv.h"

using namespace nufft;

struct nufft_tv {
    int dtype = NUFFT_F64, D = 1, C = 1, device = -1, wide = 0;
    int64_t N[3] = {1, 1, 1};
    int64_t n = 1, G = 1;
    int tile[3] = {1, 1, 1}, tiles[3] = {1, 1, 1};
    void* d_part = nullptr;               // double[C][G]
    int64_t own_bytes = 0;
};

struct nufft_tvpd {
    nufft_toeplitz* tz = nullptr;
    nufft_tv* tv = nullptr;
    int dtype = NUFFT_F64, C = 1, D = 1, device = -1, G0 = 1;
    int max_iter = 1, check_every = 0, enqueued = -1;
    double tol = 0.0, step = 1.0, sigma = 1.0, lambda = 0.0;
    std::vector<double> weight;
    int64_t n = 0, stride = 0;            // complex cells per component; reals between two of the solver's arrays
    void* d_q = nullptr;                  // [C] arrays
    void* d_y = nullptr;                  // [C][D] arrays
    void* d_part = nullptr;               // double[C][G][2] of the primal kernel
    ScalarMirror scal;                    // double change[C]; int32 flag[C], iters[C], status[C]
    void* d_hist = nullptr;               // double[max_iter][C][2]
    int64_t array_bytes = 0, own_bytes = 0;
    std::vector<void*> qtab;
};

namespace {

void release(nufft_tv* t) {
    if (!t) return;
    if (t->device >= 0) {
        DeviceGuard g(t->device);
        if (t->d_part) (void)hipFree(t->d_part);
    }
    delete t;
}

void release(nufft_tvpd* s) {
    if (!s) return;
    release(s->tv);
    if (s->device >= 0) {
        DeviceGuard g(s->device);
        for (void* p : {s->d_q, s->d_y, s->d_part, s->d_hist})
            if (p) (void)hipFree(p);
        s->scal.release();
    }
    delete s;
}

int create_geometry(nufft_tv** out, int dtype, int D, const int64_t* N, int C, int device) {
    const int64_t most[3] = {(int64_t)1 << 30, (int64_t)1 << (D == 2 ? 20 : 17), (int64_t)1 << 18};      // grid limits of the tiling
    for (int d = 0; d < D; ++d)
        if (N[d] > most[d])
            return fail(NUFFT_ERR_UNSUPPORTED, "N[" + std::to_string(d) + "] = " + std::to_string(N[d]) + " is more than the " + std::to_string(most[d]) +
                                                   " cells the total-variation kernels tile along this dimension");
    // the decision and sum kernels count the rows of partial sums (workgroups of all components of a joint system) in an int
    const bool f32 = dtype == NUFFT_F32, wide = f32 && N[0] % 2 == 0;      // ComplexF32 rows of odd length are not 16-byte aligned
    int64_t G = 1;
    for (int d = 0; d < D; ++d) G *= (N[d] + tv_tile(f32, wide, D, d) - 1) / tv_tile(f32, wide, D, d);
    if (G > (int64_t)INT_MAX / std::max(C, 1))
        return fail(NUFFT_ERR_UNSUPPORTED, std::to_string(G) + " workgroups for each of " + std::to_string(C) + " components: more than 2^31 - 1 rows of partial sums");
    if (device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only plan (device = -1): the total-variation kernels run on the device");
    nufft_tv* t = new (std::nothrow) nufft_tv();
    if (!t) return fail(NUFFT_ERR_ALLOC, "out of host memory");
    t->dtype = dtype;
    t->D = D;
    t->C = C;
    t->device = device;
    for (int d = 0; d < D; ++d) {
        t->N[d] = N[d];
        t->n *= N[d];
    }
    t->wide = wide ? 1 : 0;
    for (int d = 0; d < 3; ++d) {
        t->tile[d] = tv_tile(f32, t->wide != 0, D, d);
        t->tiles[d] = (int)((t->N[d] + t->tile[d] - 1) / t->tile[d]);
        t->G *= t->tiles[d];
    }
    DeviceGuard guard(device);
    if (int rc = alloc_buffer(t->own_bytes, "total-variation", &t->d_part, (size_t)C * t->G * sizeof(double))) {
        const std::string keep = nufft_last_error_message();
        release(t);
        return fail(rc, keep);
    }
    *out = t;
    return NUFFT_OK;
}

TvLaunch launch_template(const nufft_tv* t) {
    TvLaunch a{};
    a.dtype = t->dtype;
    a.D = t->D;
    a.wide = t->wide;
    a.C = t->C;
    for (int d = 0; d < 3; ++d) {
        a.N[d] = (int)t->N[d];
        a.tiles[d] = t->tiles[d];
    }
    a.G = t->G;
    a.part = static_cast<double*>(t->d_part);
    return a;
}

// components per launch: the callers' pointers travel as kernel arguments, and gridDim.z = tiles[2] · components stays below 2^16
int batch_of(const nufft_tv* t) { return std::max(1, std::min(kTvBatch, 65535 / t->tiles[2])); }

bool overlap(const void* a, const void* b, size_t bytes) {
    const char* x = static_cast<const char*>(a);
    const char* y = static_cast<const char*>(b);
    return x < y + bytes && y < x + bytes;
}

// `count` device pointers, 16-byte aligned
int check_table(const void* const* tab, int count) {
    if (!tab) return fail(NUFFT_ERR_INVALID_ARG, "null table");
    for (int k = 0; k < count; ++k) {
        if (!tab[k]) return fail(NUFFT_ERR_INVALID_ARG, "null data vector");
        if ((uintptr_t)tab[k] & 15) return fail(NUFFT_ERR_INVALID_ARG, "the arrays must be 16-byte aligned");
    }
    return NUFFT_OK;
}

// no output may overlap an input or another output
int check_overlap(const nufft_tv* t, void* const* out, int nout, const void* const* in, int nin) {
    const size_t bytes = (size_t)t->n * 2 * real_bytes(t->dtype);
    for (int o = 0; o < nout; ++o) {
        for (int i = 0; i < nin; ++i)
            if (overlap(out[o], in[i], bytes))
                return fail(NUFFT_ERR_INVALID_ARG, "an output overlaps an input: a cell's neighbours are read while other workgroups store");
        for (int k = 0; k < o; ++k)
            if (overlap(out[o], out[k], bytes)) return fail(NUFFT_ERR_INVALID_ARG, "two outputs overlap");
    }
    return NUFFT_OK;
}

// One operator launch per batch of components: x[c] and the D arrays y[c · D + d]
int run_operator(nufft_tv* t, TvMode mode, void* const* x, void* const* y, hipStream_t stream) {
    TvLaunch a = launch_template(t);
    const int B = batch_of(t);
    for (int c0 = 0; c0 < t->C; c0 += B) {
        a.c0 = c0;
        a.nc = std::min(B, t->C - c0);
        for (int k = 0; k < a.nc; ++k) {
            a.x[k] = x[c0 + k];
            for (int d = 0; d < t->D; ++d) a.y[k][d] = y ? y[(size_t)(c0 + k) * t->D + d] : nullptr;
        }
        hipError_t e = launch_tv(a, mode, stream);
        if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a total-variation kernel: ") + hipGetErrorString(e));
    }
    return NUFFT_OK;
}

size_t scal_bytes(const nufft_tvpd* s) { return (size_t)s->C * (sizeof(double) + 3 * sizeof(int32_t)); }
size_t hist_bytes(const nufft_tvpd* s) { return (size_t)s->max_iter * s->C * 2 * sizeof(double); }

TvScalars scalars_at(const nufft_tvpd* s, void* base) {
    TvScalars k{};
    double* d = static_cast<double*>(base);
    k.change = d;
    int32_t* i = reinterpret_cast<int32_t*>(d + s->C);
    k.flag = i;
    k.iters = i + s->C;
    k.status = i + 2 * s->C;
    k.history = static_cast<double*>(s->d_hist);
    return k;
}

bool weight_ok(double v) { return std::isfinite(v) && v >= 0.0; }

int toeplitz_info(const nufft_toeplitz* tz, nufft_toeplitz_info& ti) {
    std::memset(&ti, 0, sizeof(ti));
    ti.struct_size = (int32_t)sizeof(ti);
    return nufft_toeplitz_get_info(tz, &ti);
}

}  // namespace

extern "C" {

int64_t nufft_sizeof_tv_info(void) { return (int64_t)sizeof(nufft_tv_info); }
int64_t nufft_sizeof_tvpd_params(void) { return (int64_t)sizeof(nufft_tvpd_params); }
int64_t nufft_sizeof_tvpd_info(void) { return (int64_t)sizeof(nufft_tvpd_info); }

int nufft_tv_create(nufft_tv** out, const nufft_plan* plan) {
    if (!out || !plan) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!plan->is_complex)
        return fail(NUFFT_ERR_UNSUPPORTED, "the total-variation operator needs a complex plan: its arrays are those of the Toeplitz normal "
                                           "operator, which a real-data plan cannot have");
    return create_geometry(out, plan->dtype, plan->D, plan->N, plan->C, plan->device);
}

int nufft_tv_create_for_operator(nufft_tv** out, const nufft_toeplitz* tz) {
    if (!out || !tz) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    nufft_toeplitz_info ti;
    if (int rc = toeplitz_info(tz, ti)) return rc;
    return create_geometry(out, ti.dtype, ti.ndim, ti.N, ti.ntransforms, ti.device);
}

int nufft_tv_destroy(nufft_tv* tv) {
    release(tv);
    return NUFFT_OK;
}

int nufft_tv_get_info(const nufft_tv* t, nufft_tv_info* o) {
    if (!t || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    nufft_tv_info i;
    std::memset(&i, 0, sizeof(i));
    i.ndim = t->D;
    i.dtype = t->dtype;
    i.ntransforms = t->C;
    i.device = t->device;
    for (int d = 0; d < 3; ++d) {
        i.tile[d] = t->tile[d];
        i.N[d] = t->N[d];
    }
    i.workgroups = t->G;
    i.workspace_bytes = t->own_bytes;
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_tv_gradient(nufft_tv* t, void* const* y_out, const void* const* x, void* stream) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = check_table(y_out, t->C * t->D)) || (rc = check_table(x, t->C)) || (rc = check_overlap(t, y_out, t->C * t->D, x, t->C))) return rc;
    DeviceGuard guard(t->device);
    return run_operator(t, TV_GRADIENT, const_cast<void* const*>(x), y_out, static_cast<hipStream_t>(stream));
}

int nufft_tv_adjoint(nufft_tv* t, void* const* x_out, const void* const* y, void* stream) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = check_table(x_out, t->C)) || (rc = check_table(y, t->C * t->D)) || (rc = check_overlap(t, x_out, t->C, y, t->C * t->D))) return rc;
    DeviceGuard guard(t->device);
    return run_operator(t, TV_ADJOINT, x_out, const_cast<void* const*>(y), static_cast<hipStream_t>(stream));
}

int nufft_tv_norm(nufft_tv* t, const void* const* x, double* sums_out_device, void* stream) {
    if (!t || !sums_out_device) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (int rc = check_table(x, t->C)) return rc;
    DeviceGuard guard(t->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = run_operator(t, TV_NORM, const_cast<void* const*>(x), nullptr, s)) return rc;
    hipError_t e = launch_tv_sum(static_cast<const double*>(t->d_part), t->G, t->C, sums_out_device, s);
    if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a total-variation kernel: ") + hipGetErrorString(e));
    return NUFFT_OK;
}

int nufft_tvpd_create(nufft_tvpd** out, nufft_toeplitz* tz, const nufft_tvpd_params* params) {
    if (!out || !tz || !params) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    nufft_toeplitz_info ti;
    int rc = toeplitz_info(tz, ti);
    if (rc) return rc;
    nufft_tvpd_params p;
    if ((rc = read_params(p, params, "nufft_tvpd_params"))) return rc;
    if (p.max_iter < 1) return fail(NUFFT_ERR_INVALID_ARG, "max_iter must be at least 1");
    if (p.max_iter > (1 << 24)) return fail(NUFFT_ERR_INVALID_ARG, "max_iter beyond 2^24");
    if (p.check_every < 0) return fail(NUFFT_ERR_INVALID_ARG, "check_every must not be negative");
    if (!weight_ok(p.tol)) return fail(NUFFT_ERR_INVALID_ARG, "tol must be finite and not negative");
    if (!weight_ok(p.tv)) return fail(NUFFT_ERR_INVALID_ARG, "tv must be finite and not negative");
    if (!weight_ok(p.lambda)) return fail(NUFFT_ERR_INVALID_ARG, "lambda must be finite and not negative");
    if (!std::isfinite(p.step) || !(p.step > 0.0))
        return fail(NUFFT_ERR_INVALID_ARG, "step must be finite and positive (1 / (lambda_max + lambda): nufft_toeplitz_max_eigenvalue)");
    if (!weight_ok(p.sigma)) return fail(NUFFT_ERR_INVALID_ARG, "sigma must be finite and positive (0: 1 / (8 ndim step))");

    nufft_tvpd* s = new (std::nothrow) nufft_tvpd();
    if (!s) return fail(NUFFT_ERR_ALLOC, "out of host memory");
    if ((rc = create_geometry(&s->tv, ti.dtype, ti.ndim, ti.N, ti.ntransforms, ti.device))) {      // host-only: refused here
        delete s;
        return rc;
    }
    s->tz = tz;
    s->dtype = ti.dtype;
    s->C = ti.ntransforms;
    s->D = ti.ndim;
    s->device = ti.device;
    s->max_iter = p.max_iter;
    s->check_every = p.check_every;
    s->tol = p.tol;
    s->step = p.step;
    s->sigma = p.sigma > 0.0 ? p.sigma : 1.0 / (8.0 * s->D * p.step);
    s->lambda = p.lambda;
    s->weight.assign(s->C, p.tv);
    s->n = s->tv->n;
    const size_t rb = real_bytes(s->dtype), comp = padded((size_t)s->n * 2 * rb);
    s->stride = (int64_t)(comp / rb);
    s->array_bytes = (int64_t)(1 + s->D) * s->C * (int64_t)comp;

    DeviceGuard guard(s->device);
    int cus = 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device) != hipSuccess || cus <= 0) {
        (void)hipGetLastError();
        cus = 256;
    }
    s->G0 = stream::stream_workgroups((int64_t)(comp / 16), cus);
    auto alloc = [&](void** ptr, size_t bytes) { return alloc_buffer(s->own_bytes, "TV solver", ptr, bytes); };
    if ((rc = alloc(&s->d_q, (size_t)s->C * comp)) || (rc = alloc(&s->d_y, (size_t)s->C * s->D * comp)) ||
        (rc = alloc(&s->d_part, (size_t)s->C * s->tv->G * 2 * sizeof(double))) || (rc = alloc(&s->d_hist, hist_bytes(s))) ||
        (rc = s->scal.create(s->own_bytes, "TV solver", scal_bytes(s), "hipHostMalloc of the solver's host mirror failed"))) {
        const std::string keep = nufft_last_error_message();
        release(s);
        return fail(rc, keep);
    }
    // a defined answer from nufft_tvpd_get_result / nufft_tvpd_history before the first solve
    if (s->scal.zero() != hipSuccess || hipMemset(s->d_hist, 0xFF, hist_bytes(s)) != hipSuccess) {
        (void)hipGetLastError();
        release(s);
        return fail(NUFFT_ERR_HIP, "hipMemset of the solver's scalars failed");
    }
    for (int c = 0; c < s->C; ++c) s->qtab.push_back(static_cast<char*>(s->d_q) + (size_t)c * comp);
    *out = s;
    return NUFFT_OK;
}

int nufft_tvpd_destroy(nufft_tvpd* s) {
    release(s);
    return NUFFT_OK;
}

int nufft_tvpd_set_tv(nufft_tvpd* s, const double* weights, int64_t count) {
    if (!s || !weights) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (count != s->C) return fail(NUFFT_ERR_INVALID_ARG, "count must be ntransforms");
    for (int c = 0; c < s->C; ++c)
        if (!weight_ok(weights[c])) return fail(NUFFT_ERR_INVALID_ARG, "tv must be finite and not negative");
    s->weight.assign(weights, weights + s->C);
    return NUFFT_OK;
}

int nufft_tvpd_get_info(const nufft_tvpd* s, nufft_tvpd_info* o) {
    if (!s || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    nufft_tvpd_info i;
    std::memset(&i, 0, sizeof(i));
    i.ntransforms = s->C;
    i.dtype = s->dtype;
    i.ndim = s->D;
    i.max_iter = s->max_iter;
    i.check_every = s->check_every;
    i.iterations_enqueued = s->enqueued;
    i.tol = s->tol;
    i.step = s->step;
    i.sigma = s->sigma;
    i.lambda = s->lambda;
    i.array_bytes = s->array_bytes;
    i.workspace_bytes = s->own_bytes + s->tv->own_bytes;
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_tvpd_solve(nufft_tvpd* s, void* const* x, const void* const* b, int use_x0, void* stream_) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    nufft_toeplitz_info ti;
    int rc = toeplitz_info(s->tz, ti);
    if (rc) return rc;
    if (!ti.has_spectrum)
        return fail(NUFFT_ERR_NO_POINTS, "nufft_toeplitz_set_spectrum or nufft_toeplitz_set_points must be called before nufft_tvpd_solve");
    if (!x || !b) return fail(NUFFT_ERR_INVALID_ARG, "null table");
    const size_t bytes = (size_t)s->n * 2 * real_bytes(s->dtype);
    for (int c = 0; c < s->C; ++c) {
        if (!x[c] || !b[c]) return fail(NUFFT_ERR_INVALID_ARG, "null data vector");
        if (((uintptr_t)x[c] | (uintptr_t)b[c]) & 15) return fail(NUFFT_ERR_INVALID_ARG, "x and b must be 16-byte aligned");
    }
    for (int c = 0; c < s->C; ++c)
        for (int k = 0; k < s->C; ++k) {
            if (overlap(x[c], b[k], bytes)) return fail(NUFFT_ERR_INVALID_ARG, "x overlaps b: the right-hand side is read while x is written");
            if (k != c && overlap(x[c], x[k], bytes)) return fail(NUFFT_ERR_INVALID_ARG, "two components of x overlap");
        }
    DeviceGuard guard(s->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (s->check_every > 0 && capturing(stream))
        return fail(NUFFT_ERR_INVALID_ARG, "check_every > 0 synchronises the stream: not on a capturing stream (use check_every = 0)");

    const size_t rb = real_bytes(s->dtype), comp = (size_t)s->stride * rb;
    TvSolve h{};
    h.dtype = s->dtype;
    h.C = s->C;
    h.G = s->G0;
    h.n = s->n;
    h.ystride = s->stride * s->D;
    h.y = s->d_y;
    h.max_iter = s->max_iter;
    h.joint = nufft_toeplitz_num_coupled(s->tz) > 0 ? 1 : 0;
    h.tol = s->tol;
    h.part_p = static_cast<const double*>(s->d_part);
    h.part_d = static_cast<const double*>(s->tv->d_part);
    h.P = s->tv->G;
    h.s = scalars_at(s, s->scal.dev);
    TvLaunch a = launch_template(s->tv);
    a.step = s->step;
    a.sigma = s->sigma;
    a.lambda = s->lambda;
    a.flag = h.s.flag;
    const int B = batch_of(s->tv);
    // one launch per batch of components; the solver's q and y, the callers' x and b
    auto for_batches = [&](auto&& launch) -> int {
        for (int c0 = 0; c0 < s->C; c0 += B) {
            h.c0 = a.c0 = c0;
            h.nc = a.nc = std::min(B, s->C - c0);
            for (int k = 0; k < a.nc; ++k) {
                const int c = c0 + k;
                h.x[k] = a.x[k] = x[c];
                a.b[k] = b[c];
                a.q[k] = s->qtab[c];
                for (int d = 0; d < s->D; ++d) a.y[k][d] = static_cast<char*>(s->d_y) + ((size_t)c * s->D + d) * comp;
                a.tv[k] = s->weight[c];
            }
            hipError_t e = launch();
            if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a TV solver kernel: ") + hipGetErrorString(e));
        }
        return NUFFT_OK;
    };

    s->enqueued = 0;
    const bool warm = use_x0 != 0;
    if ((rc = for_batches([&]() { return launch_tv_start(h, warm, stream); }))) return rc;
    const TvScalars host = scalars_at(s, s->scal.host);
    for (int it = 1; it <= s->max_iter; ++it) {
        h.it = it;
        if ((rc = nufft_toeplitz_apply(s->tz, s->qtab.data(), const_cast<const void* const*>(x), stream))) return rc;      // q = G x
        a.part = static_cast<double*>(s->d_part);
        if ((rc = for_batches([&]() { return launch_tv(a, TV_PRIMAL, stream); }))) return rc;
        a.part = static_cast<double*>(s->tv->d_part);
        if ((rc = for_batches([&]() { return launch_tv(a, TV_DUAL, stream); }))) return rc;
        if ((rc = for_batches([&]() { return launch_tv_decide(h, stream); }))) return rc;
        s->enqueued = it;
        if (s->check_every > 0 && it % s->check_every == 0 && it < s->max_iter) {
            if ((rc = s->scal.fetch(stream))) return rc;
            bool all = true;
            for (int c = 0; c < s->C; ++c) all = all && host.flag[c] != 0;
            if (all) break;
        }
    }
    return NUFFT_OK;
}

int nufft_tvpd_get_result(nufft_tvpd* s, int32_t* iterations, int32_t* status, double* change, int64_t capacity, void* stream_) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (capacity < s->C) return fail(NUFFT_ERR_INVALID_ARG, "capacity is smaller than ntransforms");
    DeviceGuard guard(s->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (capturing(stream)) return fail(NUFFT_ERR_INVALID_ARG, "nufft_tvpd_get_result synchronises: not on a capturing stream");
    int rc = s->scal.fetch(stream);
    if (rc) return rc;
    const TvScalars host = scalars_at(s, s->scal.host);
    for (int c = 0; c < s->C; ++c) {
        if (iterations) iterations[c] = host.iters[c];
        if (status) status[c] = host.status[c];
        if (change) change[c] = host.change[c];
    }
    return NUFFT_OK;
}

int nufft_tvpd_history(nufft_tvpd* s, double* host_out, int64_t capacity, void* stream_) {
    if (!s || !host_out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (capacity < (int64_t)s->max_iter * s->C * 2) return fail(NUFFT_ERR_INVALID_ARG, "capacity is smaller than max_iter * ntransforms * 2");
    DeviceGuard guard(s->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (capturing(stream)) return fail(NUFFT_ERR_INVALID_ARG, "nufft_tvpd_history synchronises: not on a capturing stream");
    NUFFT_HIP(hipMemcpyAsync(host_out, s->d_hist, hist_bytes(s), hipMemcpyDeviceToHost, stream));
    NUFFT_HIP(hipStreamSynchronize(stream));
    return NUFFT_OK;
}

}  // extern "C"
