// FISTA with an l1-wavelet prior on the Toeplitz normal operator (include/nufft_mi355x.h, FISTA section).
//
// The host side only enqueues: per iteration one nufft_toeplitz_apply (unchanged), the gradient kernel, the wavelet object's analysis
// levels (threshold and ‖·‖₁ partials on store), its synthesis levels (the momentum step and the partials of ‖x⁺ − x‖², ‖x⁺‖² on the
// last level's store) and the decision kernel.  Every scalar lives on the device; with check_every > 0 the host looks at the done flags
// now and then, and at nothing else.
//
// With the locally low-rank prior (nufft_fista_create_llr) an iteration is the apply, llr.h's kernel (gradient
// step on load, proximal map, momentum step on store) and the decision kernel of one joint system; the wavelet path is untouched by it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "fista.h"
#include "llr.h"
#include "solver_common.h"
#include "wavelet.h"

using namespace nufft;

struct nufft_fista {
    nufft_toeplitz* tz = nullptr;
    nufft_wavelet* wav = nullptr;
    nufft_llr* llr = nullptr;         // the locally low-rank prior instead of the wavelet one
    double nuc = 0.0;
    int dtype = NUFFT_F64, C = 1, device = -1, num_cus = 256, G = 1, G0 = 1;
    int max_iter = 1, check_every = 0, enqueued = -1, wavelet = 0, levels = 1;
    double tol = 0.0, step = 1.0, lambda = 0.0;
    std::vector<double> l1, thr;
    int64_t n = 0, stride = 0;
    void* d_z = nullptr;
    void* d_q = nullptr;
    void* d_c = nullptr;
    void* d_mom = nullptr;            // double[C][G0][2]
    ScalarMirror scal;                // double change[C]; int32 flag[C], iters[C], status[C]
    void* d_hist = nullptr;           // double[max_iter][C][2]
    int64_t array_bytes = 0, own_bytes = 0;
    std::vector<void*> ztab, qtab, ctab;
};

namespace {

size_t hist_bytes(const nufft_fista* s) { return (size_t)s->max_iter * s->C * 2 * sizeof(double); }

void release(nufft_fista* s) {
    if (!s) return;
    if (s->wav) (void)nufft_wavelet_destroy(s->wav);
    if (s->llr) (void)nufft_llr_destroy(s->llr);
    if (s->device >= 0) {
        DeviceGuard g(s->device);
        for (void* p : {s->d_z, s->d_q, s->d_c, s->d_mom, s->d_hist})
            if (p) (void)hipFree(p);
        s->scal.release();
    }
    delete s;
}

template <typename F>
int for_batches(const nufft_fista* s, FistaLaunch& a, void* const* x, const void* const* b, F&& launch) {
    for (int c0 = 0; c0 < s->C; c0 += kFistaBatch) {
        a.c0 = c0;
        a.nc = std::min(kFistaBatch, s->C - c0);
        for (int k = 0; k < a.nc; ++k) {
            a.x[k] = x[c0 + k];
            a.b[k] = b[c0 + k];
        }
        hipError_t e = launch(a);
        if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a FISTA kernel: ") + hipGetErrorString(e));
    }
    return NUFFT_OK;
}

// nufft_fista_create (lp null) and nufft_fista_create_llr
int create(nufft_fista** out, nufft_toeplitz* tz, const nufft_fista_params* params, const nufft_llr_params* lp, double nuc) {
    nufft_toeplitz_info ti;
    int rc = toeplitz_info(tz, ti);
    if (rc) return rc;
    nufft_fista_params p;
    if ((rc = read_params(p, params, "nufft_fista_params"))) return rc;
    if (p.max_iter < 1) return fail(NUFFT_ERR_INVALID_ARG, "max_iter must be at least 1");
    if (p.max_iter > (1 << 24)) return fail(NUFFT_ERR_INVALID_ARG, "max_iter beyond 2^24");
    if (p.check_every < 0) return fail(NUFFT_ERR_INVALID_ARG, "check_every must not be negative");
    if (!weight_ok(p.tol)) return fail(NUFFT_ERR_INVALID_ARG, "tol must be finite and not negative");
    if (!weight_ok(p.l1)) return fail(NUFFT_ERR_INVALID_ARG, "l1 must be finite and not negative");
    if (!weight_ok(p.lambda)) return fail(NUFFT_ERR_INVALID_ARG, "lambda must be finite and not negative");
    if (lp && (p.wavelet != 0 || p.levels != 0 || p.l1 != 0.0))
        return fail(NUFFT_ERR_INVALID_ARG, "wavelet, levels and l1 must be 0 for the locally low-rank prior");
    if (lp && !weight_ok(nuc)) return fail(NUFFT_ERR_INVALID_ARG, "nuc must be finite and not negative");
    if (!std::isfinite(p.step) || !(p.step > 0.0))
        return fail(NUFFT_ERR_INVALID_ARG, "step must be finite and positive (1 / (lambda_max + lambda): nufft_toeplitz_max_eigenvalue)");

    nufft_fista* s = new (std::nothrow) nufft_fista();
    if (!s) return fail(NUFFT_ERR_ALLOC, "out of host memory");
    nufft_wavelet_params wp;
    std::memset(&wp, 0, sizeof(wp));
    wp.struct_size = (int32_t)sizeof(wp);
    wp.wavelet = p.wavelet;
    wp.levels = p.levels;
    rc = lp ? llr_create_geometry(&s->llr, ti.dtype, ti.ndim, ti.N, ti.ntransforms, ti.device, lp)
            : wavelet_create_geometry(&s->wav, ti.dtype, ti.ndim, ti.N, ti.ntransforms, ti.device, &wp);      // host-only: refused here
    if (rc) {
        delete s;
        return rc;
    }
    s->nuc = nuc;
    s->tz = tz;
    s->dtype = ti.dtype;
    s->C = ti.ntransforms;
    s->device = ti.device;
    s->max_iter = p.max_iter;
    s->check_every = p.check_every;
    s->wavelet = p.wavelet;
    s->levels = p.levels;
    s->tol = p.tol;
    s->step = p.step;
    s->lambda = p.lambda;
    s->l1.assign(s->C, p.l1);
    s->thr.assign(s->C, 0.0);
    s->n = ti.N[0] * ti.N[1] * ti.N[2];
    const size_t rb = real_bytes(s->dtype), comp = padded((size_t)s->n * 2 * rb);
    s->stride = (int64_t)(comp / rb);
    s->array_bytes = (lp ? 2 : 3) * (int64_t)s->C * (int64_t)comp;      // the locally low-rank kernel needs no coefficient array

    DeviceGuard guard(s->device);
    s->num_cus = device_cus(s->device);
    s->G = fista_workgroups(s->dtype, s->n, s->num_cus);
    s->G0 = lp ? 1 : wavelet_level0_workgroups(s->wav);
    auto alloc = [&](void** ptr, size_t bytes) { return alloc_buffer(s->own_bytes, "FISTA", ptr, bytes); };
    if ((rc = alloc(&s->d_z, (size_t)s->C * comp)) || (rc = alloc(&s->d_q, (size_t)s->C * comp)) ||
        (!lp && ((rc = alloc(&s->d_c, (size_t)s->C * comp)) || (rc = alloc(&s->d_mom, (size_t)s->C * s->G0 * 2 * sizeof(double))))) ||
        (rc = create_outcome(s->own_bytes, "FISTA", s->scal, &s->d_hist, prox_scal_bytes(s->C), hist_bytes(s)))) {
        const std::string keep = nufft_last_error_message();
        release(s);
        return fail(rc, keep);
    }
    for (int c = 0; c < s->C; ++c) {
        s->ztab.push_back(static_cast<char*>(s->d_z) + (size_t)c * comp);
        s->qtab.push_back(static_cast<char*>(s->d_q) + (size_t)c * comp);
        if (s->d_c) s->ctab.push_back(static_cast<char*>(s->d_c) + (size_t)c * comp);
    }
    *out = s;
    return NUFFT_OK;
}

// One solve with the locally low-rank prior: the components are one system.
int solve_llr(nufft_fista* s, FistaLaunch& a, void* const* x, const void* const* b, hipStream_t stream) {
    int rc;
    LlrLaunch l = llr_launch_template(s->llr);
    l.mode = LLR_FISTA;
    l.t = s->step * s->nuc;
    l.z = s->d_z;
    l.q = s->d_q;
    l.stride = s->stride;
    l.step = s->step;
    l.lambda = s->lambda;
    l.flag = a.s.flag;
    for (int c = 0; c < s->C; ++c) {
        l.in[c] = b[c];
        l.out[c] = x[c];
    }
    const int64_t G = llr_workgroups(l);
    const ProxScalars host = prox_scalars_at(s->scal.host, s->C, nullptr);
    uint64_t state = llr_seed(s->llr);
    double t = 1.0;
    for (int it = 1; it <= s->max_iter; ++it) {
        a.it = it;
        const double t_next = 0.5 * (1.0 + std::sqrt(1.0 + 4.0 * t * t));
        l.beta = (t - 1.0) / t_next;
        t = t_next;
        if (llr_shifts(s->llr))
            for (int d = 0; d < l.D; ++d) {
                state = state * 6364136223846793005ull + 1442695040888963407ull;
                l.shift[d] = (int)((state >> 33) % (uint64_t)llr_block_side(s->llr, d));
            }
        if ((rc = nufft_toeplitz_apply(s->tz, s->qtab.data(), s->ztab.data(), stream))) return rc;                        // q = G z
        hipError_t e = launch_llr(l, stream);
        if (e == hipSuccess) e = launch_fista_decide_llr(a, l.part, G, stream);
        if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a FISTA kernel: ") + hipGetErrorString(e));
        s->enqueued = it;
        if (s->check_every > 0 && it % s->check_every == 0 && it < s->max_iter) {
            bool done;
            if ((rc = all_done(s->scal, stream, host.flag, 1, &done))) return rc;
            if (done) break;
        }
    }
    return NUFFT_OK;
}

}  // namespace

extern "C" {

int64_t nufft_sizeof_fista_params(void) { return (int64_t)sizeof(nufft_fista_params); }
int64_t nufft_sizeof_fista_info(void) { return (int64_t)sizeof(nufft_fista_info); }

int nufft_fista_create(nufft_fista** out, nufft_toeplitz* tz, const nufft_fista_params* params) {
    if (!out || !tz || !params) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    return create(out, tz, params, nullptr, 0.0);
}

int nufft_fista_create_llr(nufft_fista** out, nufft_toeplitz* tz, const nufft_fista_params* params, const nufft_llr_params* llr, double nuc) {
    if (!out || !tz || !params || !llr) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    return create(out, tz, params, llr, nuc);
}

int nufft_fista_set_nuc(nufft_fista* s, double nuc) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (!s->llr) return fail(NUFFT_ERR_INVALID_ARG, "nufft_fista_set_nuc on a solver with the wavelet prior (nufft_fista_set_l1)");
    if (!weight_ok(nuc)) return fail(NUFFT_ERR_INVALID_ARG, "nuc must be finite and not negative");
    s->nuc = nuc;
    return NUFFT_OK;
}

int nufft_fista_destroy(nufft_fista* f) {
    release(f);
    return NUFFT_OK;
}

int nufft_fista_set_l1(nufft_fista* s, const double* l1, int64_t count) {
    if (!s || !l1) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (s->llr) return fail(NUFFT_ERR_INVALID_ARG, "nufft_fista_set_l1 on a solver with the locally low-rank prior (nufft_fista_set_nuc)");
    if (count != s->C) return fail(NUFFT_ERR_INVALID_ARG, "count must be ntransforms");
    for (int c = 0; c < s->C; ++c)
        if (!weight_ok(l1[c])) return fail(NUFFT_ERR_INVALID_ARG, "l1 must be finite and not negative");
    s->l1.assign(l1, l1 + s->C);
    return NUFFT_OK;
}

int nufft_fista_get_info(const nufft_fista* s, nufft_fista_info* o) {
    if (!s || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    int64_t prior_bytes = 0;
    if (s->llr) {
        nufft_llr_info li;
        std::memset(&li, 0, sizeof(li));
        li.struct_size = (int32_t)sizeof(li);
        if (int rc = nufft_llr_get_info(s->llr, &li)) return rc;
        prior_bytes = li.workspace_bytes;
    } else {
        nufft_wavelet_info wi;
        std::memset(&wi, 0, sizeof(wi));
        wi.struct_size = (int32_t)sizeof(wi);
        if (int rc = nufft_wavelet_get_info(s->wav, &wi)) return rc;
        prior_bytes = wi.workspace_bytes;
    }
    nufft_fista_info i;
    std::memset(&i, 0, sizeof(i));
    i.ntransforms = s->C;
    i.dtype = s->dtype;
    i.max_iter = s->max_iter;
    i.check_every = s->check_every;
    i.wavelet = s->wavelet;
    i.levels = s->levels;
    i.iterations_enqueued = s->enqueued;
    i.tol = s->tol;
    i.step = s->step;
    i.lambda = s->lambda;
    i.array_bytes = s->array_bytes;
    i.workspace_bytes = s->own_bytes + prior_bytes;
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_fista_solve(nufft_fista* s, void* const* x, const void* const* b, int use_x0, void* stream_) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    DeviceGuard guard(s->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc = check_solve_args(s->tz, "nufft_fista_solve", s->C, s->n, s->dtype, x, b, s->check_every, stream);
    if (rc) return rc;

    FistaLaunch a{};
    a.dtype = s->dtype;
    a.C = s->C;
    a.G = s->G;
    a.n = s->n;
    a.stride = s->stride;
    a.z = s->d_z;
    a.q = s->d_q;
    a.step = s->step;
    a.lambda = s->lambda;
    a.tol = s->tol;
    a.max_iter = s->max_iter;
    a.joint = nufft_toeplitz_num_coupled(s->tz) > 0 ? 1 : 0;
    a.mom_part = static_cast<const double*>(s->d_mom);
    a.G0 = s->G0;
    if (s->wav) a.l1_part = wavelet_partials(s->wav, &a.P);
    a.s = prox_scalars_at(s->scal.dev, s->C, s->d_hist);
    for (int c = 0; c < s->C; ++c) s->thr[c] = s->step * s->l1[c];

    s->enqueued = 0;
    const bool warm = use_x0 != 0;
    if ((rc = for_batches(s, a, x, b, [&](const FistaLaunch& l) { return launch_fista_start(l, warm, stream); }))) return rc;
    if (s->llr) return solve_llr(s, a, x, b, stream);
    const ProxScalars host = prox_scalars_at(s->scal.host, s->C, nullptr);
    double t = 1.0;
    for (int it = 1; it <= s->max_iter; ++it) {
        a.it = it;
        const double t_next = 0.5 * (1.0 + std::sqrt(1.0 + 4.0 * t * t));
        WaveletFista wf;
        wf.momentum = 1;
        wf.beta = (t - 1.0) / t_next;
        wf.x = x;
        wf.mom_part = static_cast<double*>(s->d_mom);
        t = t_next;
        if ((rc = nufft_toeplitz_apply(s->tz, s->qtab.data(), s->ztab.data(), stream))) return rc;                        // q = G z
        if ((rc = for_batches(s, a, x, b, [&](const FistaLaunch& l) { return launch_fista_gradient(l, stream); }))) return rc;
        if ((rc = wavelet_forward(s->wav, s->ctab.data(), s->qtab.data(), s->thr.data(), a.s.flag, stream))) return rc;
        if ((rc = wavelet_inverse(s->wav, s->ztab.data(), s->ctab.data(), &wf, a.s.flag, stream))) return rc;
        if ((rc = for_batches(s, a, x, b, [&](const FistaLaunch& l) { return launch_fista_decide(l, stream); }))) return rc;
        s->enqueued = it;
        if (s->check_every > 0 && it % s->check_every == 0 && it < s->max_iter) {
            bool all;
            if ((rc = all_done(s->scal, stream, host.flag, s->C, &all))) return rc;
            if (all) break;
        }
    }
    return NUFFT_OK;
}

int nufft_fista_get_result(nufft_fista* s, int32_t* iterations, int32_t* status, double* change, int64_t capacity, void* stream_) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (capacity < s->C) return fail(NUFFT_ERR_INVALID_ARG, "capacity is smaller than ntransforms");
    DeviceGuard guard(s->device);
    return copy_result("nufft_fista_get_result", s->scal, s->C, s->C, 1, iterations, status, change, static_cast<hipStream_t>(stream_));
}

int nufft_fista_history(nufft_fista* s, double* host_out, int64_t capacity, void* stream_) {
    if (!s || !host_out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (capacity < (int64_t)s->max_iter * s->C * 2) return fail(NUFFT_ERR_INVALID_ARG, "capacity is smaller than max_iter * ntransforms * 2");
    DeviceGuard guard(s->device);
    return fetch_history("nufft_fista_history", host_out, s->d_hist, hist_bytes(s), static_cast<hipStream_t>(stream_));
}

// Power iteration on what nufft_toeplitz_apply computes (header: largest eigenvalue).  Lives here, above the operator's public entry
// points, with the other users of the streaming reductions.
int nufft_toeplitz_max_eigenvalue(nufft_toeplitz* tz, const void* const* v0, int32_t iters, double* out_host, void* stream_) {
    if (!tz || !v0 || !out_host) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (iters < 1) return fail(NUFFT_ERR_INVALID_ARG, "iters must be at least 1");
    nufft_toeplitz_info ti;
    int rc = toeplitz_info(tz, ti);
    if (rc) return rc;
    if (ti.device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only Toeplitz object (device = -1)");
    if (!ti.has_spectrum)
        return fail(NUFFT_ERR_NO_POINTS, "nufft_toeplitz_set_spectrum or nufft_toeplitz_set_points must be called before nufft_toeplitz_max_eigenvalue");
    const int C = ti.ntransforms;
    for (int c = 0; c < C; ++c) {
        if (!v0[c]) return fail(NUFFT_ERR_INVALID_ARG, "null data vector");
        if ((uintptr_t)v0[c] & 15) return fail(NUFFT_ERR_INVALID_ARG, "the start vectors must be 16-byte aligned");
    }
    DeviceGuard guard(ti.device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (capturing(stream)) return fail(NUFFT_ERR_INVALID_ARG, "nufft_toeplitz_max_eigenvalue synchronises: not on a capturing stream");

    PowerLaunch a{};
    a.dtype = ti.dtype;
    a.C = C;
    a.joint = nufft_toeplitz_num_coupled(tz) > 0 ? 1 : 0;
    a.n = ti.N[0] * ti.N[1] * ti.N[2];
    const size_t rb = real_bytes(a.dtype), bytes = (size_t)a.n * 2 * rb, comp = padded(bytes);
    a.stride = (int64_t)(comp / rb);
    a.G = fista_workgroups(a.dtype, a.n, device_cus(ti.device));
    int64_t own = 0;
    void* d_part = nullptr;
    void* d_rho = nullptr;
    auto cleanup = [&]() {
        for (void* p : {a.v, a.g, d_part, d_rho})
            if (p) (void)hipFree(p);
    };
    if ((rc = alloc_buffer(own, "power-iteration", &a.v, (size_t)C * comp)) || (rc = alloc_buffer(own, "power-iteration", &a.g, (size_t)C * comp)) ||
        (rc = alloc_buffer(own, "power-iteration", &d_part, (size_t)C * a.G * 3 * sizeof(double))) ||
        (rc = alloc_buffer(own, "power-iteration", &d_rho, (size_t)C * sizeof(double)))) {
        const std::string keep = nufft_last_error_message();
        cleanup();
        return fail(rc, keep);
    }
    a.part = static_cast<double*>(d_part);
    a.rho = static_cast<double*>(d_rho);
    std::vector<void*> vtab, gtab;
    for (int c = 0; c < C; ++c) {
        vtab.push_back(static_cast<char*>(a.v) + (size_t)c * comp);
        gtab.push_back(static_cast<char*>(a.g) + (size_t)c * comp);
    }
    auto run = [&]() -> int {
        for (int c = 0; c < C; ++c) NUFFT_HIP(hipMemcpyAsync(vtab[c], v0[c], bytes, hipMemcpyDeviceToDevice, stream));
        for (int it = 0; it < iters; ++it) {
            if (int r = nufft_toeplitz_apply(tz, gtab.data(), vtab.data(), stream)) return r;
            hipError_t e = launch_power_dot(a, stream);
            if (e == hipSuccess) e = launch_power_scale(a, stream);
            if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a power-iteration kernel: ") + hipGetErrorString(e));
        }
        NUFFT_HIP(hipMemcpyAsync(out_host, d_rho, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, stream));
        NUFFT_HIP(hipStreamSynchronize(stream));
        return NUFFT_OK;
    };
    rc = run();
    if (rc) {
        const std::string keep = nufft_last_error_message();
        (void)hipStreamSynchronize(stream);
        cleanup();
        return fail(rc, keep);
    }
    cleanup();
    return NUFFT_OK;
}

}  // extern "C"
