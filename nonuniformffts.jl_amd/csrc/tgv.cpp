// Second-order total generalized variation on the Toeplitz normal operator: the primal-dual solver (nufft_tgv_*) of
// include/nufft_mi355x.h; DESIGN.md section 31.  The operator alone (nufft_tv_sym_*) is in tv.cpp, on the nufft_tv object.
//
// Minimises, per component (jointly over all components on a coupled operator), over an image x and a vector field v,
//
//     ½ <x, (G + μ I) x> − Re<b, x> + α1 Σ_i |(∇x − v)_i|₂ + α0 Σ_i |(E v)_i|_F
//
// ∇ the periodic forward difference of tv.cpp, E the symmetrised gradient from periodic backward differences (tgv_kernels.hip).
// Condat–Vũ on K(x, v) = (∇x − v, E v), Kᴴ(p, r) = (∇ᴴp, −p + Eᴴr):
//
//     start:  x = x0 (or 0),  v = p = r = 0
//     per iteration:
//         q  = G x                                        the operator's apply, unchanged
//         x⁺ = x − τ (q + μ x − b + ∇ᴴ p)                 tv_primal kernel with p for y: stores x <- x⁺ and q <- x̄
//         v⁺ = v − τ (−p + Eᴴ r)                          tgv_field kernel: stores v <- v⁺ and v̄
//         p  <- P_α1(p + σ (∇x̄ − v̄))                      tgv_p kernel, in place; partial of Σ_i |(∇x⁺ − v⁺)_i|₂
//         r  <- P_α0(r + σ E v̄)                           tgv_r kernel, in place; partial of Σ_i |(E v⁺)_i|_F
//         decide: change = ‖x⁺ − x‖ / ‖x⁺‖; history row (change, the two sums); done <- change <= tol, or change not finite
//
// τ = step, σ = sigma (0: 1 / (16 D τ)); with ‖K‖² <= 8 D that gives 1/τ − σ ‖K‖² >= 1 / (2 τ) >= L / 2 for τ <= 1 / L.
//
// The host side only enqueues, as in tv.cpp: every scalar lives on the device, and with check_every > 0 the host looks at the done
// flags now and then.  The geometry (tiles, workgroups) is that of a nufft_tv object made for the operator.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "solver_common.h"
#include "stream_kernels.h"
#include "tgv.h"

using namespace nufft;

struct nufft_tgv {
    nufft_toeplitz* tz = nullptr;
    nufft_tv_info geo;                    // of a nufft_tv made for the operator (not kept): tiles and workgroups
    int dtype = NUFFT_F64, C = 1, D = 1, S = 1, device = -1, G0 = 1;
    int max_iter = 1, check_every = 0, enqueued = -1;
    double tol = 0.0, step = 1.0, sigma = 1.0, lambda = 0.0;
    std::vector<double> alpha1, alpha0;
    int64_t n = 0, stride = 0;            // complex cells per component; reals between two of the solver's arrays
    int na = 1;                           // arrays per component in d_w: v (D), p (D), r (S), v̄ (D)
    void* d_q = nullptr;                  // [C] arrays
    void* d_w = nullptr;                  // [C][na] arrays
    void* d_part_x = nullptr;             // double[C][G][2] of the primal kernel
    void* d_part_p = nullptr;             // double[C][G]
    void* d_part_r = nullptr;             // double[C][G]
    ScalarMirror scal;                    // double change[C]; int32 flag[C], iters[C], status[C]
    void* d_hist = nullptr;               // double[max_iter][C][3]
    int64_t array_bytes = 0, own_bytes = 0;
    std::vector<void*> qtab;
};

namespace {

void release(nufft_tgv* s) {
    if (!s) return;
    if (s->device >= 0) {
        DeviceGuard g(s->device);
        for (void* p : {s->d_q, s->d_w, s->d_part_x, s->d_part_p, s->d_part_r, s->d_hist})
            if (p) (void)hipFree(p);
        s->scal.release();
    }
    delete s;
}

size_t hist_bytes(const nufft_tgv* s) { return (size_t)s->max_iter * s->C * 3 * sizeof(double); }

// array `k` of component c in d_w
void* work_array(const nufft_tgv* s, int c, int k) {
    return static_cast<char*>(s->d_w) + ((size_t)c * s->na + k) * (size_t)s->stride * real_bytes(s->dtype);
}

}  // namespace

extern "C" {

int64_t nufft_sizeof_tgv_params(void) { return (int64_t)sizeof(nufft_tgv_params); }
int64_t nufft_sizeof_tgv_info(void) { return (int64_t)sizeof(nufft_tgv_info); }

int nufft_tgv_create(nufft_tgv** out, nufft_toeplitz* tz, const nufft_tgv_params* params) {
    if (!out || !tz || !params) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    nufft_toeplitz_info ti;
    int rc = toeplitz_info(tz, ti);
    if (rc) return rc;
    nufft_tgv_params p;
    if ((rc = read_params(p, params, "nufft_tgv_params"))) return rc;
    if (p.max_iter < 1) return fail(NUFFT_ERR_INVALID_ARG, "max_iter must be at least 1");
    if (p.max_iter > (1 << 24)) return fail(NUFFT_ERR_INVALID_ARG, "max_iter beyond 2^24");
    if (p.check_every < 0) return fail(NUFFT_ERR_INVALID_ARG, "check_every must not be negative");
    if (!weight_ok(p.tol)) return fail(NUFFT_ERR_INVALID_ARG, "tol must be finite and not negative");
    if (!weight_ok(p.alpha1) || !weight_ok(p.alpha0)) return fail(NUFFT_ERR_INVALID_ARG, "alpha1 and alpha0 must be finite and not negative");
    if (!weight_ok(p.lambda)) return fail(NUFFT_ERR_INVALID_ARG, "lambda must be finite and not negative");
    if (!std::isfinite(p.step) || !(p.step > 0.0))
        return fail(NUFFT_ERR_INVALID_ARG, "step must be finite and positive (1 / (lambda_max + lambda): nufft_toeplitz_max_eigenvalue)");
    if (!weight_ok(p.sigma)) return fail(NUFFT_ERR_INVALID_ARG, "sigma must be finite and positive (0: 1 / (16 ndim step))");

    // the geometry of the stencil kernels, with the refusals of nufft_tv_create (a host-only operator among them)
    nufft_tv* tv = nullptr;
    if ((rc = nufft_tv_create_for_operator(&tv, tz))) return rc;
    nufft_tgv* s = new (std::nothrow) nufft_tgv();
    if (!s) {
        nufft_tv_destroy(tv);
        return fail(NUFFT_ERR_ALLOC, "out of host memory");
    }
    std::memset(&s->geo, 0, sizeof(s->geo));
    s->geo.struct_size = (int32_t)sizeof(s->geo);
    rc = nufft_tv_get_info(tv, &s->geo);
    nufft_tv_destroy(tv);
    if (rc) {
        delete s;
        return rc;
    }
    s->tz = tz;
    s->dtype = ti.dtype;
    s->C = ti.ntransforms;
    s->D = ti.ndim;
    s->S = tgv_sym(s->D);
    s->device = ti.device;
    s->max_iter = p.max_iter;
    s->check_every = p.check_every;
    s->tol = p.tol;
    s->step = p.step;
    s->sigma = p.sigma > 0.0 ? p.sigma : 1.0 / (16.0 * s->D * p.step);
    s->lambda = p.lambda;
    s->alpha1.assign(s->C, p.alpha1);
    s->alpha0.assign(s->C, p.alpha0);
    s->n = 1;
    for (int d = 0; d < s->D; ++d) s->n *= ti.N[d];
    s->na = 3 * s->D + s->S;
    const size_t rb = real_bytes(s->dtype), comp = padded((size_t)s->n * 2 * rb);
    s->stride = (int64_t)(comp / rb);
    s->array_bytes = (int64_t)(1 + s->na) * s->C * (int64_t)comp;

    DeviceGuard guard(s->device);
    s->G0 = stream::stream_workgroups((int64_t)(comp / 16), device_cus(s->device));
    auto alloc = [&](void** ptr, size_t bytes) { return alloc_buffer(s->own_bytes, "TGV solver", ptr, bytes); };
    const size_t rows = (size_t)s->C * (size_t)s->geo.workgroups;
    if ((rc = alloc(&s->d_q, (size_t)s->C * comp)) || (rc = alloc(&s->d_w, (size_t)s->C * s->na * comp)) ||
        (rc = alloc(&s->d_part_x, rows * 2 * sizeof(double))) || (rc = alloc(&s->d_part_p, rows * sizeof(double))) ||
        (rc = alloc(&s->d_part_r, rows * sizeof(double))) ||
        (rc = create_outcome(s->own_bytes, "TGV solver", s->scal, &s->d_hist, prox_scal_bytes(s->C), hist_bytes(s)))) {
        const std::string keep = nufft_last_error_message();
        release(s);
        return fail(rc, keep);
    }
    for (int c = 0; c < s->C; ++c) s->qtab.push_back(static_cast<char*>(s->d_q) + (size_t)c * comp);
    *out = s;
    return NUFFT_OK;
}

int nufft_tgv_destroy(nufft_tgv* s) {
    release(s);
    return NUFFT_OK;
}

int nufft_tgv_set_weights(nufft_tgv* s, const double* alpha1, const double* alpha0, int64_t count) {
    if (!s || !alpha1 || !alpha0) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (count != s->C) return fail(NUFFT_ERR_INVALID_ARG, "count must be ntransforms");
    for (int c = 0; c < s->C; ++c)
        if (!weight_ok(alpha1[c]) || !weight_ok(alpha0[c])) return fail(NUFFT_ERR_INVALID_ARG, "alpha1 and alpha0 must be finite and not negative");
    s->alpha1.assign(alpha1, alpha1 + s->C);
    s->alpha0.assign(alpha0, alpha0 + s->C);
    return NUFFT_OK;
}

int nufft_tgv_get_info(const nufft_tgv* s, nufft_tgv_info* o) {
    if (!s || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    nufft_tgv_info i;
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
    i.workspace_bytes = s->own_bytes;
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_tgv_solve(nufft_tgv* s, void* const* x, const void* const* b, int use_x0, void* stream_) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    DeviceGuard guard(s->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc = check_solve_args(s->tz, "nufft_tgv_solve", s->C, s->n, s->dtype, x, b, s->check_every, stream);
    if (rc) return rc;

    const int D = s->D, S = s->S;
    const bool f32 = s->dtype == NUFFT_F32;
    TgvSolve h{};
    h.dtype = s->dtype;
    h.C = s->C;
    h.G = s->G0;
    h.n = s->n;
    h.wstride = s->stride * s->na;
    h.w = s->d_w;
    h.max_iter = s->max_iter;
    h.joint = nufft_toeplitz_num_coupled(s->tz) > 0 ? 1 : 0;
    h.tol = s->tol;
    h.part_x = static_cast<const double*>(s->d_part_x);
    h.part_p = static_cast<const double*>(s->d_part_p);
    h.part_r = static_cast<const double*>(s->d_part_r);
    h.P = s->geo.workgroups;
    h.s = prox_scalars_at(s->scal.dev, s->C, s->d_hist);
    TvLaunch a{};      // the x-update: the TV solver's primal kernel with p in the place of y
    TgvLaunch g{};
    a.dtype = g.dtype = s->dtype;
    a.D = g.D = D;
    a.wide = g.wide = f32 && s->geo.N[0] % 2 == 0 ? 1 : 0;
    a.C = g.C = s->C;
    for (int d = 0; d < 3; ++d) {
        a.N[d] = g.N[d] = (int)s->geo.N[d];
        a.tiles[d] = g.tiles[d] = (int)((s->geo.N[d] + s->geo.tile[d] - 1) / s->geo.tile[d]);
    }
    a.G = g.G = s->geo.workgroups;
    a.step = g.step = s->step;
    a.sigma = g.sigma = s->sigma;
    a.lambda = s->lambda;
    a.part = static_cast<double*>(s->d_part_x);
    a.flag = g.flag = h.s.flag;
    const int B = std::max(1, std::min(kTvBatch, 65535 / a.tiles[2]));      // gridDim.z = tiles[2] · components stays below 2^16
    // one launch per batch of components; the solver's q, v, p, r, v̄, the callers' x and b
    auto for_batches = [&](auto&& launch) -> int {
        for (int c0 = 0; c0 < s->C; c0 += B) {
            h.c0 = a.c0 = g.c0 = c0;
            h.nc = a.nc = g.nc = std::min(B, s->C - c0);
            for (int k = 0; k < a.nc; ++k) {
                const int c = c0 + k;
                h.x[k] = a.x[k] = x[c];
                g.x[k] = x[c];
                a.b[k] = b[c];
                a.q[k] = s->qtab[c];
                g.q[k] = s->qtab[c];
                for (int d = 0; d < D; ++d) {
                    g.v[k][d] = work_array(s, c, d);
                    a.y[k][d] = g.p[k][d] = work_array(s, c, D + d);
                    g.vb[k][d] = work_array(s, c, 2 * D + S + d);
                }
                for (int e = 0; e < S; ++e) g.r[k][e] = work_array(s, c, 2 * D + e);
                g.alpha1[k] = s->alpha1[c];
                g.alpha0[k] = s->alpha0[c];
            }
            hipError_t e = launch();
            if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a TGV solver kernel: ") + hipGetErrorString(e));
        }
        return NUFFT_OK;
    };

    s->enqueued = 0;
    const bool warm = use_x0 != 0;
    if ((rc = for_batches([&]() { return launch_tgv_start(h, warm, stream); }))) return rc;
    const ProxScalars host = prox_scalars_at(s->scal.host, s->C, nullptr);
    for (int it = 1; it <= s->max_iter; ++it) {
        h.it = it;
        if ((rc = nufft_toeplitz_apply(s->tz, s->qtab.data(), const_cast<const void* const*>(x), stream))) return rc;      // q = G x
        if ((rc = for_batches([&]() { return launch_tv(a, TV_PRIMAL, stream); }))) return rc;
        if ((rc = for_batches([&]() { return launch_tgv(g, TGV_FIELD, stream); }))) return rc;
        g.part = static_cast<double*>(s->d_part_p);
        if ((rc = for_batches([&]() { return launch_tgv(g, TGV_P, stream); }))) return rc;
        g.part = static_cast<double*>(s->d_part_r);
        if ((rc = for_batches([&]() { return launch_tgv(g, TGV_R, stream); }))) return rc;
        if ((rc = for_batches([&]() { return launch_tgv_decide(h, stream); }))) return rc;
        s->enqueued = it;
        if (s->check_every > 0 && it % s->check_every == 0 && it < s->max_iter) {
            bool all;
            if ((rc = all_done(s->scal, stream, host.flag, s->C, &all))) return rc;
            if (all) break;
        }
    }
    return NUFFT_OK;
}

int nufft_tgv_get_result(nufft_tgv* s, int32_t* iterations, int32_t* status, double* change, int64_t capacity, void* stream_) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (capacity < s->C) return fail(NUFFT_ERR_INVALID_ARG, "capacity is smaller than ntransforms");
    DeviceGuard guard(s->device);
    return copy_result("nufft_tgv_get_result", s->scal, s->C, s->C, 1, iterations, status, change, static_cast<hipStream_t>(stream_));
}

int nufft_tgv_history(nufft_tgv* s, double* host_out, int64_t capacity, void* stream_) {
    if (!s || !host_out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (capacity < (int64_t)s->max_iter * s->C * 3) return fail(NUFFT_ERR_INVALID_ARG, "capacity is smaller than max_iter * ntransforms * 3");
    DeviceGuard guard(s->device);
    return fetch_history("nufft_tgv_history", host_out, s->d_hist, hist_bytes(s), static_cast<hipStream_t>(stream_));
}

int nufft_tgv_copy_field(nufft_tgv* s, void* const* v_out, void* stream_) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (int rc = check_table(v_out, s->C * s->D)) return rc;
    DeviceGuard guard(s->device);
    const size_t bytes = (size_t)s->n * 2 * real_bytes(s->dtype);
    for (int c = 0; c < s->C; ++c)
        for (int d = 0; d < s->D; ++d)
            NUFFT_HIP(hipMemcpyAsync(v_out[(size_t)c * s->D + d], work_array(s, c, d), bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream_)));
    return NUFFT_OK;
}

}  // extern "C"
