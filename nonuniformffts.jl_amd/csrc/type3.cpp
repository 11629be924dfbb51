// Type-3 plan (nonuniform to nonuniform): parameter rule, buffers and the C ABI of include/nufft_mi355x.h's type-3 section.
//
// f_k = Σ_j c_j exp(sign i s_k·x_j).  With y = x - C (source centre) and t = s - D (target centre), s·x = s·C + D·y + t·y, so
//   f_k = exp(sign i s_k·C) Σ_j [c_j exp(sign i D·y_j)] exp(sign i t_k·y_j)
// (Barnett, Magland & af Klinteberg, SISC 2019, section 3.3).  The inner sum is a type-3 sum between centred boxes: the prephased
// values are spread at y / γ onto a grid of nf cells (the spreading plan), that grid is the input spectrum of a type-2 transform
// (the type-2 plan, N = nf) at θ = sign γ h t, and the window is divided out per target at the real wavenumber γ t.  DESIGN.md
// section 13 has the derivation of the constants and the measurements.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "host_common.h"
#include "type3.h"

using namespace nufft;

struct nufft_plan3 {
    nufft_plan* sp = nullptr;          // spreading plan: N_over = nf, window of the requested σ and M
    nufft_plan* t2 = nullptr;          // type-2 plan: complex, N = nf, fftshift = false
    int dtype = NUFFT_F64, D = 1, C = 1, M = 4, kernel = 0, evalmode = 0, device = -1, sign = -1;
    double sigma = 2.0;
    double src_c[3] = {0, 0, 0}, src_w[3] = {0, 0, 0};     // declared boxes (the caller's half-widths: what points_outside counts)
    double tgt_c[3] = {0, 0, 0}, tgt_w[3] = {0, 0, 0};
    double X[3] = {1, 1, 1}, S[3] = {1, 1, 1};             // half-widths of the rule (zero ones replaced)
    int64_t nf[3] = {1, 1, 1}, inner_nover[3] = {1, 1, 1};
    double gamma[3] = {1, 1, 1}, h[3] = {0, 0, 0}, beta[3] = {0, 0, 0};
    int num_cus = 256;
    // device buffers (capacity in points; they move only when a point set outgrows them)
    void* d_xr = nullptr;              // T[D][src_cap]: rescaled source coordinates
    void* d_phase = nullptr;           // complex<T>[src_cap]
    void* d_cvals = nullptr;           // complex<T>[C][src_cap]: prephased values
    void* d_theta = nullptr;           // T[D][tgt_cap]
    void* d_post = nullptr;            // complex<T>[tgt_cap]
    unsigned long long* d_outside = nullptr;   // [2]: sources, targets outside the declared boxes
    int64_t src_cap = 0, tgt_cap = 0, own_bytes = 0;
    int64_t Np = -1, Nk = -1;
    bool timing = false;
    hipEvent_t ev_begin[NUFFT3_NUM_STAGES] = {}, ev_end[NUFFT3_NUM_STAGES] = {};
    bool ev_valid[NUFFT3_NUM_STAGES] = {};
};

namespace {

struct Timer {
    nufft_plan3* p;
    int stage;
    hipStream_t stream;
    Timer(nufft_plan3* plan, int st, hipStream_t s) : p(plan), stage(st), stream(s) {
        if (p->timing) (void)hipEventRecord(p->ev_begin[stage], stream);
    }
    ~Timer() {
        if (p->timing) {
            (void)hipEventRecord(p->ev_end[stage], stream);
            p->ev_valid[stage] = true;
        }
    }
};

int alloc(nufft_plan3* p, void** ptr, size_t bytes) { return alloc_buffer(p->own_bytes, "type-3", ptr, bytes); }

size_t src_bytes(const nufft_plan3* p, int64_t n, int which) {      // 0: coordinates, 1: phase, 2: values
    const size_t rb = real_bytes(p->dtype);
    return which == 0 ? (size_t)n * rb * p->D : which == 1 ? (size_t)n * rb * 2 : (size_t)n * rb * 2 * p->C;
}
size_t tgt_bytes(const nufft_plan3* p, int64_t n, int which) {      // 0: θ, 1: post factor
    const size_t rb = real_bytes(p->dtype);
    return which == 0 ? (size_t)n * rb * p->D : (size_t)n * rb * 2;
}

void release(nufft_plan3* p) {
    if (!p) return;
    if (p->device >= 0) {
        DeviceGuard g(p->device);
        free_buffer(p->own_bytes, p->d_xr, src_bytes(p, p->src_cap, 0));
        free_buffer(p->own_bytes, p->d_phase, src_bytes(p, p->src_cap, 1));
        free_buffer(p->own_bytes, p->d_cvals, src_bytes(p, p->src_cap, 2));
        free_buffer(p->own_bytes, p->d_theta, tgt_bytes(p, p->tgt_cap, 0));
        free_buffer(p->own_bytes, p->d_post, tgt_bytes(p, p->tgt_cap, 1));
        free_buffer(p->own_bytes, p->d_outside, 16);
        for (int s = 0; s < NUFFT3_NUM_STAGES; ++s) {
            if (p->ev_begin[s]) (void)hipEventDestroy(p->ev_begin[s]);
            if (p->ev_end[s]) (void)hipEventDestroy(p->ev_end[s]);
        }
    }
    if (p->sp) nufft_plan_destroy(p->sp);
    if (p->t2) nufft_plan_destroy(p->t2);
    delete p;
}

// Optimal window shape for the requested σ (plan.cpp: build_host, with σ in the plan's precision): the spreading plan's grid is nf,
// whatever σ its N_over implies, so its shape parameter is passed explicitly.
double optimal_param(int kernel, int M, double sigma, int dtype) {
    const double s = dtype == NUFFT_F32 ? (double)(float)sigma : sigma;
    if (kernel == NUFFT_KERNEL_BACKWARDS_KAISER_BESSEL) return nufft::bkb_beta(M, s);
    if (kernel == NUFFT_KERNEL_KAISER_BESSEL) return nufft::kb_beta(M, s);
    if (kernel == NUFFT_KERNEL_GAUSSIAN) return nufft::gaussian_ell(M, s);
    return 0.0;
}

// The grid rule: the smallest multiple of 4 that is 2,3,5-smooth and >= 2σXS/π + 2M + 2 (the +2 a margin on X/γ + M h <= π; multiples
// of 4 keep the 3-D engines of 4-cell bins eligible).  Returns 0 beyond 2^30.
int64_t fine_grid(double sigma, int M, double X, double S) {
    const double bound = 2.0 * sigma * X * S / M_PI + 2.0 * M + 2.0;
    if (!(bound <= (double)((int64_t)1 << 30))) return 0;
    const int64_t n = 4 * nufft::nextprod235((int64_t)std::ceil(bound / 4.0));
    return n <= ((int64_t)1 << 30) ? n : 0;
}

// The stages exec_type3 and exec_type3_grad share: premultiply c' = c · phase, then the completing spread of c'; `us` receives the
// spread grid of every component (the type-2 plan's input spectrum).
int prephase_and_spread(nufft_plan3* p, const void* const* c_in, std::vector<const void*>& us, hipStream_t stream) {
    const size_t cb = 2 * real_bytes(p->dtype);
    std::vector<const void*> cv(p->C);
    for (int c = 0; c < p->C; ++c) cv[c] = static_cast<char*>(p->d_cvals) + (size_t)c * p->Np * cb;
    {
        Timer tm(p, NUFFT3_STAGE_PREMULTIPLY, stream);
        for (int c0 = 0; c0 < p->C; c0 += nufft::kMaxCompPerLaunch) {
            nufft::T3MultArgs m{};
            m.dtype = p->dtype;
            m.n = p->Np;
            m.ncomp = std::min(nufft::kMaxCompPerLaunch, p->C - c0);
            m.factor = p->d_phase;
            for (int i = 0; i < m.ncomp; ++i) { m.in[i] = c_in[c0 + i]; m.out[i] = const_cast<void*>(cv[c0 + i]); }
            NUFFT_HIP(nufft::launch_t3_multiply(m, p->num_cus, stream));
        }
    }
    int rc;
    {
        Timer tm(p, NUFFT3_STAGE_SPREAD, stream);
        // the completing spread: `us` holds the whole field (the halo variant's side buffer added) before the type-2 plan reads it
        if ((rc = nufft_spread(p->sp, cv.data(), stream))) return rc;
    }
    us.assign(p->C, nullptr);
    for (int c = 0; c < p->C; ++c) {
        void* ptr = nullptr;
        if ((rc = nufft_grid_ptr(p->sp, 0, c, &ptr, nullptr))) return rc;
        us[c] = ptr;
    }
    return NUFFT_OK;
}

}  // namespace

extern "C" {

int64_t nufft_sizeof_type3_params(void) { return (int64_t)sizeof(nufft_type3_params); }
int64_t nufft_sizeof_info3(void) { return (int64_t)sizeof(nufft_info3); }

int nufft_plan3_create(nufft_plan3** out, const nufft_params* params_in, const nufft_type3_params* t3_in) {
    if (!out || !params_in || !t3_in) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    // the prefix of nufft_params the caller knows (nufft_plan_create_ex's rule)
    nufft_params prm;
    std::memset(&prm, 0, sizeof(prm));
    size_t known = params_in->struct_size > 0 ? (size_t)params_in->struct_size : offsetof(nufft_params, kernel_param_dim);
    if (known < offsetof(nufft_params, kernel_param_dim)) return fail(NUFFT_ERR_INVALID_ARG, "nufft_params.struct_size is smaller than any published layout");
    std::memcpy(&prm, params_in, std::min(known, sizeof(prm)));
    nufft_type3_params t3;
    std::memset(&t3, 0, sizeof(t3));
    const size_t known3 = t3_in->struct_size > 0 ? (size_t)t3_in->struct_size : sizeof(t3);
    std::memcpy(&t3, t3_in, std::min(known3, sizeof(t3)));

    if (prm.dtype != NUFFT_F32 && prm.dtype != NUFFT_F64) return fail(NUFFT_ERR_INVALID_ARG, "dtype must be NUFFT_F32 or NUFFT_F64");
    if (prm.is_complex != 1) return fail(NUFFT_ERR_INVALID_ARG, "type-3 plans are complex (is_complex = 1)");
    if (prm.ndim < 1 || prm.ndim > 3) return fail(NUFFT_ERR_UNSUPPORTED, "ndim must be 1, 2 or 3");
    for (int d = 0; d < 3; ++d)
        if (prm.N[d] != 0 || prm.N_over[d] != 0)
            return fail(NUFFT_ERR_INVALID_ARG, "type-3 plans take their grids from the boxes: N and N_over must be 0");
    if (prm.fftshift != 0) return fail(NUFFT_ERR_INVALID_ARG, "fftshift has no meaning for a type-3 plan (must be 0)");
    if (prm.point_transform != NUFFT_POINT_TRANSFORM_IDENTITY) return fail(NUFFT_ERR_INVALID_ARG, "point_transform must be identity for a type-3 plan");
    const int sign = t3.sign == 0 ? -1 : t3.sign;
    if (sign != -1 && sign != 1) return fail(NUFFT_ERR_INVALID_ARG, "sign must be -1 or +1");
    const int D = prm.ndim;
    for (int d = 0; d < D; ++d) {
        const double v[4] = {t3.source_center[d], t3.source_halfwidth[d], t3.target_center[d], t3.target_halfwidth[d]};
        for (double x : v)
            if (!std::isfinite(x)) return fail(NUFFT_ERR_INVALID_ARG, "box centres and half-widths must be finite");
        if (t3.source_halfwidth[d] < 0.0 || t3.target_halfwidth[d] < 0.0) return fail(NUFFT_ERR_INVALID_ARG, "half-widths must be >= 0");
    }

    nufft_plan3* p = new (std::nothrow) nufft_plan3();
    if (!p) return fail(NUFFT_ERR_ALLOC, "out of host memory");
    p->dtype = prm.dtype;
    p->D = D;
    p->C = prm.ntransforms > 0 ? prm.ntransforms : 1;
    p->M = prm.half_support > 0 ? prm.half_support : 4;
    p->sigma = prm.sigma > 0 ? prm.sigma : 2.0;
    p->kernel = prm.kernel;
    p->evalmode = prm.evalmode;
    p->device = prm.device;
    p->sign = sign;
    if (p->M < nufft::kMinM || p->M > nufft::kMaxM) { release(p); return fail(NUFFT_ERR_UNSUPPORTED, "half-support M must be in 2..10"); }
    if (!(p->sigma >= 1.0)) { release(p); return fail(NUFFT_ERR_INVALID_ARG, "sigma must be >= 1"); }
    if (p->kernel < NUFFT_KERNEL_BACKWARDS_KAISER_BESSEL || p->kernel > NUFFT_KERNEL_BSPLINE) {
        release(p);
        return fail(NUFFT_ERR_UNSUPPORTED, "kernel must be one of NUFFT_KERNEL_*");
    }
    double grid_bytes = 0.0;
    for (int d = 0; d < D; ++d) {
        p->src_c[d] = t3.source_center[d];
        p->src_w[d] = t3.source_halfwidth[d];
        p->tgt_c[d] = t3.target_center[d];
        p->tgt_w[d] = t3.target_halfwidth[d];
        double X = p->src_w[d], S = p->tgt_w[d];
        if (X == 0.0 && S == 0.0) X = S = 1.0;
        else if (X == 0.0) X = 1.0 / S;
        else if (S == 0.0) S = 1.0 / X;
        p->X[d] = X;
        p->S[d] = S;
        p->nf[d] = fine_grid(p->sigma, p->M, X, S);
        const double inner = p->nf[d] > 0 ? (double)nufft::nextprod235((int64_t)std::floor(p->sigma * (double)p->nf[d])) : 0.0;
        if (p->nf[d] == 0 || inner > (double)((int64_t)1 << 30)) {
            const double want = 2.0 * p->sigma * X * S / M_PI + 2.0 * p->M + 2.0;
            release(p);
            return fail(NUFFT_ERR_UNSUPPORTED, "type-3 fine grid nf = " + std::to_string(want) + " (dimension " + std::to_string(d + 1) +
                                                   ") and its oversampled type-2 grid must stay within 2^30 cells per axis: narrow the boxes");
        }
        p->inner_nover[d] = (int64_t)inner;
        p->h[d] = 2.0 * M_PI / (double)p->nf[d];
        p->gamma[d] = (double)p->nf[d] / (2.0 * p->sigma * S);
    }
    {
        double outer = 1.0, inner = 1.0;
        for (int d = 0; d < D; ++d) { outer *= (double)p->nf[d]; inner *= (double)p->inner_nover[d]; }
        grid_bytes = (outer + inner) * 2.0 * (double)real_bytes(p->dtype) * p->C;
    }
    const double user_param = prm.kernel_param;
    for (int d = 0; d < D; ++d) p->beta[d] = user_param > 0.0 ? user_param : optimal_param(p->kernel, p->M, p->sigma, p->dtype);

    if (p->device >= 0) {
        DeviceGuard g(p->device);
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, p->device) != hipSuccess) {
            (void)hipGetLastError();
            release(p);
            return fail(NUFFT_ERR_HIP, "hipGetDeviceProperties failed");
        }
        p->num_cus = std::max(1, prop.multiProcessorCount);
        if (grid_bytes > (double)prop.totalGlobalMem) {
            std::string msg = "type-3 grids need " + std::to_string(grid_bytes / 1e9) + " GB (nf =";
            for (int d = 0; d < D; ++d) msg += " " + std::to_string(p->nf[d]);
            msg += ") but the device holds " + std::to_string((double)prop.totalGlobalMem / 1e9) + " GB: narrow the boxes";
            release(p);
            return fail(NUFFT_ERR_UNSUPPORTED, msg);
        }
        // the spreading plan: grid nf, window of the requested σ; N only sizes the type-1 stages this plan never runs
        nufft_params a = prm;
        a.struct_size = (int32_t)sizeof(nufft_params);
        a.is_complex = 1;
        a.fftshift = 0;
        a.point_transform = NUFFT_POINT_TRANSFORM_IDENTITY;
        a.kernel_param = 0.0;
        for (int d = 0; d < 3; ++d) { a.N[d] = 0; a.N_over[d] = 0; a.kernel_param_dim[d] = 0.0; }
        for (int d = 0; d < D; ++d) {
            a.N_over[d] = p->nf[d];
            a.N[d] = std::max<int64_t>(1, (int64_t)std::floor((double)p->nf[d] / p->sigma));
            if (p->kernel != NUFFT_KERNEL_BSPLINE) a.kernel_param_dim[d] = p->beta[d];
        }
        int rc = nufft_plan_create_ex(&p->sp, &a);
        if (rc) { const std::string keep = nufft_last_error_message(); release(p); return fail(rc, "type-3 spreading plan: " + keep); }
        // the type-2 plan: N = nf, the same σ, M and kernel, frequencies in FFT order
        nufft_params b = prm;
        b.struct_size = (int32_t)sizeof(nufft_params);
        b.is_complex = 1;
        b.fftshift = 0;
        b.point_transform = NUFFT_POINT_TRANSFORM_IDENTITY;
        for (int d = 0; d < 3; ++d) { b.N[d] = d < D ? p->nf[d] : 0; b.N_over[d] = 0; b.kernel_param_dim[d] = 0.0; }
        rc = nufft_plan_create_ex(&p->t2, &b);
        if (rc) { const std::string keep = nufft_last_error_message(); release(p); return fail(rc, "type-3 type-2 plan: " + keep); }
        for (int d = 0; d < D; ++d) p->beta[d] = p->sp->beta[d];
        for (int s = 0; s < NUFFT3_NUM_STAGES; ++s) {
            if (hipEventCreate(&p->ev_begin[s]) != hipSuccess || hipEventCreate(&p->ev_end[s]) != hipSuccess) {
                (void)hipGetLastError();
                release(p);
                return fail(NUFFT_ERR_HIP, "hipEventCreate failed");
            }
        }
        void* o = nullptr;
        if ((rc = alloc(p, &o, 16))) { release(p); return rc; }
        p->d_outside = static_cast<unsigned long long*>(o);
        if (hipMemset(p->d_outside, 0, 16) != hipSuccess) { (void)hipGetLastError(); release(p); return fail(NUFFT_ERR_HIP, "hipMemset failed"); }
    }
    *out = p;
    return NUFFT_OK;
}

int nufft_plan3_destroy(nufft_plan3* p) {
    release(p);
    return NUFFT_OK;
}

int nufft_plan3_info(const nufft_plan3* p, nufft_info3* o) {
    if (!p || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    std::memset(o, 0, sizeof(*o));
    o->ndim = p->D;
    o->ntransforms = p->C;
    o->dtype = p->dtype;
    o->half_support = p->M;
    o->sign = p->sign;
    o->kernel = p->kernel;
    o->evalmode = p->evalmode;
    o->device = p->device;
    for (int d = 0; d < 3; ++d) {
        const bool in = d < p->D;
        o->nf[d] = in ? p->nf[d] : 1;
        o->gamma[d] = in ? p->gamma[d] : 0.0;
        o->h[d] = in ? p->h[d] : 0.0;
        o->source_halfwidth[d] = in ? p->X[d] : 0.0;
        o->target_halfwidth[d] = in ? p->S[d] : 0.0;
        o->inner_N_over[d] = in ? p->inner_nover[d] : 1;
        o->beta[d] = in ? p->beta[d] : 0.0;
    }
    o->sigma = p->sigma;
    o->spread_method = p->sp ? p->sp->spread_method : 0;
    o->num_sources = p->Np;
    o->num_targets = p->Nk;
    o->workspace_bytes = p->own_bytes + (p->sp ? p->sp->workspace_bytes : 0) + (p->t2 ? p->t2->workspace_bytes : 0);
    return NUFFT_OK;
}

int nufft_plan3_internal(const nufft_plan3* p, int which, nufft_plan** out) {
    if (!p || !out || (which != 0 && which != 1)) return fail(NUFFT_ERR_INVALID_ARG, "bad argument");
    if (p->device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only type-3 plan: no internal plans");
    *out = which == 0 ? p->sp : p->t2;
    return NUFFT_OK;
}

int nufft_set_points3(nufft_plan3* p, int64_t np, const void* const* x, int64_t nk, const void* const* s, void* stream_) {
    if (!p) return fail(NUFFT_ERR_INVALID_ARG, "null plan");
    if (p->device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only plan (device = -1)");
    if (np < 0 || nk < 0) return fail(NUFFT_ERR_INVALID_ARG, "negative number of points");
    if (np >= ((int64_t)1 << 31) - 1 || nk >= ((int64_t)1 << 31) - 1) return fail(NUFFT_ERR_UNSUPPORTED, "number of points exceeds 2^31 - 2");
    for (int d = 0; d < p->D; ++d) {
        if (np > 0 && (!x || !x[d])) return fail(NUFFT_ERR_INVALID_ARG, "null source coordinate vector");
        if (nk > 0 && (!s || !s[d])) return fail(NUFFT_ERR_INVALID_ARG, "null target coordinate vector");
    }
    DeviceGuard guard(p->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    p->Np = p->Nk = -1;       // no valid point sets until everything below has been enqueued
    int rc;
    if (np > p->src_cap || nk > p->tgt_cap) {
        if (capturing(stream))
            return fail(NUFFT_ERR_INVALID_ARG, "nufft_set_points3 would have to grow its buffers on a capturing stream: "
                                               "run it once eagerly with the largest point sets before capturing");
        if (np > p->src_cap) {
            free_buffer(p->own_bytes, p->d_xr, src_bytes(p, p->src_cap, 0));
            free_buffer(p->own_bytes, p->d_phase, src_bytes(p, p->src_cap, 1));
            free_buffer(p->own_bytes, p->d_cvals, src_bytes(p, p->src_cap, 2));
            p->src_cap = 0;
            if ((rc = alloc(p, &p->d_xr, src_bytes(p, np, 0))) || (rc = alloc(p, &p->d_phase, src_bytes(p, np, 1))) ||
                (rc = alloc(p, &p->d_cvals, src_bytes(p, np, 2))))
                return rc;
            p->src_cap = np;
        }
        if (nk > p->tgt_cap) {
            free_buffer(p->own_bytes, p->d_theta, tgt_bytes(p, p->tgt_cap, 0));
            free_buffer(p->own_bytes, p->d_post, tgt_bytes(p, p->tgt_cap, 1));
            p->tgt_cap = 0;
            if ((rc = alloc(p, &p->d_theta, tgt_bytes(p, nk, 0))) || (rc = alloc(p, &p->d_post, tgt_bytes(p, nk, 1)))) return rc;
            p->tgt_cap = nk;
        }
    }
    const size_t rb = real_bytes(p->dtype);
    NUFFT_HIP(hipMemsetAsync(p->d_outside, 0, 2 * sizeof(unsigned long long), stream));
    if (np > 0) {
        nufft::T3SourceArgs a{};
        a.dtype = p->dtype;
        a.D = p->D;
        a.n = np;
        a.phase = p->d_phase;
        a.outside = p->d_outside;
        a.sign = (double)p->sign;
        const void* xr[3] = {nullptr, nullptr, nullptr};
        for (int d = 0; d < p->D; ++d) {
            a.x[d] = x[d];
            a.xr[d] = static_cast<char*>(p->d_xr) + (size_t)d * np * rb;
            xr[d] = a.xr[d];
            a.center[d] = p->src_c[d];
            a.halfwidth[d] = p->src_w[d];
            a.inv_gamma[d] = 1.0 / p->gamma[d];
            a.target_center[d] = p->tgt_c[d];
        }
        {
            Timer tm(p, NUFFT3_STAGE_PREP_SOURCES, stream);
            NUFFT_HIP(nufft::launch_t3_source_prep(a, p->num_cus, stream));
        }
        if ((rc = nufft_set_points(p->sp, np, xr, stream))) return rc;
    }
    if (nk > 0) {
        nufft::T3TargetArgs a{};
        a.dtype = p->dtype;
        a.D = p->D;
        a.n = nk;
        a.post = p->d_post;
        a.outside = p->d_outside + 1;
        a.sign = (double)p->sign;
        a.kernel = p->kernel;
        a.M = p->M;
        const void* th[3] = {nullptr, nullptr, nullptr};
        for (int d = 0; d < p->D; ++d) {
            a.s[d] = s[d];
            a.theta[d] = static_cast<char*>(p->d_theta) + (size_t)d * nk * rb;
            th[d] = a.theta[d];
            a.center[d] = p->tgt_c[d];
            a.halfwidth[d] = p->tgt_w[d];
            a.theta_scale[d] = (double)p->sign * p->gamma[d] * p->h[d];      // = sign π / (σ S_d)
            a.gamma[d] = p->gamma[d];
            a.source_center[d] = p->src_c[d];
            // the spreading plan's window: ϕ̂ parameter as its type-1 deconvolution uses it (plan.cpp: build_host), and its scale 2^k
            a.dx[d] = p->h[d];
            a.param[d] = p->kernel == NUFFT_KERNEL_GAUSSIAN ? p->sp->tau[d] : p->sp->beta[d];
            a.h_scaled[d] = std::ldexp(p->h[d], -p->sp->scale_exp[d]);
        }
        {
            Timer tm(p, NUFFT3_STAGE_PREP_TARGETS, stream);
            NUFFT_HIP(nufft::launch_t3_target_prep(a, p->num_cus, stream));
        }
        if ((rc = nufft_set_points(p->t2, nk, th, stream))) return rc;
    }
    p->Np = np;
    p->Nk = nk;
    return NUFFT_OK;
}

int nufft_exec_type3(nufft_plan3* p, void* const* f_out, const void* const* c_in, void* stream_) {
    if (!p) return fail(NUFFT_ERR_INVALID_ARG, "null plan");
    if (p->device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only plan (device = -1)");
    if (p->Np < 0 || p->Nk < 0) return fail(NUFFT_ERR_NO_POINTS, "nufft_set_points3 must be called before nufft_exec_type3");
    if (p->Nk == 0) return NUFFT_OK;
    if (!f_out || (p->Np > 0 && !c_in)) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    for (int c = 0; c < p->C; ++c)
        if (!f_out[c] || (p->Np > 0 && !c_in[c])) return fail(NUFFT_ERR_INVALID_ARG, "null data vector");
    DeviceGuard guard(p->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const size_t cb = 2 * real_bytes(p->dtype);
    if (p->Np == 0) {
        for (int c = 0; c < p->C; ++c) NUFFT_HIP(hipMemsetAsync(f_out[c], 0, (size_t)p->Nk * cb, stream));
        return NUFFT_OK;
    }
    std::vector<const void*> us;
    int rc = prephase_and_spread(p, c_in, us, stream);
    if (rc) return rc;
    {
        Timer tm(p, NUFFT3_STAGE_TYPE2, stream);
        if ((rc = nufft_exec_type2(p->t2, f_out, us.data(), stream))) return rc;
    }
    {
        Timer tm(p, NUFFT3_STAGE_POSTMULTIPLY, stream);
        for (int c0 = 0; c0 < p->C; c0 += nufft::kMaxCompPerLaunch) {
            nufft::T3MultArgs m{};
            m.dtype = p->dtype;
            m.n = p->Nk;
            m.ncomp = std::min(nufft::kMaxCompPerLaunch, p->C - c0);
            m.factor = p->d_post;
            for (int i = 0; i < m.ncomp; ++i) { m.in[i] = f_out[c0 + i]; m.out[i] = f_out[c0 + i]; }
            NUFFT_HIP(nufft::launch_t3_multiply(m, p->num_cus, stream));
        }
    }
    return NUFFT_OK;
}

// Gradient with respect to the targets: the same premultiply and spread, the inner type-2 gradient straight into
// the caller's vectors, then the finish kernel in place (f = P v, ∂f/∂s_d from ∂v/∂θ_d, v and the window's ln-derivative).
int nufft_exec_type3_grad(nufft_plan3* p, void* const* f_out, void* const* grad_out, const void* const* c_in, void* stream_) {
    if (!p) return fail(NUFFT_ERR_INVALID_ARG, "null plan");
    if (p->device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only plan (device = -1)");
    if (p->Np < 0 || p->Nk < 0) return fail(NUFFT_ERR_NO_POINTS, "nufft_set_points3 must be called before nufft_exec_type3_grad");
    if (p->Nk == 0) return NUFFT_OK;
    if (!f_out || !grad_out || (p->Np > 0 && !c_in)) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    for (int c = 0; c < p->C; ++c) {
        if (!f_out[c] || (p->Np > 0 && !c_in[c])) return fail(NUFFT_ERR_INVALID_ARG, "null data vector");
        for (int d = 0; d < p->D; ++d)
            if (!grad_out[c * p->D + d]) return fail(NUFFT_ERR_INVALID_ARG, "null gradient vector");
    }
    DeviceGuard guard(p->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const size_t cb = 2 * real_bytes(p->dtype);
    if (p->Np == 0) {
        for (int c = 0; c < p->C; ++c) {
            NUFFT_HIP(hipMemsetAsync(f_out[c], 0, (size_t)p->Nk * cb, stream));
            for (int d = 0; d < p->D; ++d) NUFFT_HIP(hipMemsetAsync(grad_out[c * p->D + d], 0, (size_t)p->Nk * cb, stream));
        }
        return NUFFT_OK;
    }
    std::vector<const void*> us;
    int rc = prephase_and_spread(p, c_in, us, stream);
    if (rc) return rc;
    {
        Timer tm(p, NUFFT3_STAGE_TYPE2, stream);
        if ((rc = nufft_exec_type2_grad(p->t2, f_out, grad_out, us.data(), stream))) return rc;
    }
    {
        Timer tm(p, NUFFT3_STAGE_POSTMULTIPLY, stream);
        const size_t rb = real_bytes(p->dtype);
        for (int c0 = 0; c0 < p->C; c0 += nufft::kMaxCompPerLaunch) {
            nufft::T3GradArgs g{};
            g.dtype = p->dtype;
            g.D = p->D;
            g.n = p->Nk;
            g.ncomp = std::min(nufft::kMaxCompPerLaunch, p->C - c0);
            g.post = p->d_post;
            g.sign = (double)p->sign;
            g.kernel = p->kernel;
            g.M = p->M;
            for (int d = 0; d < p->D; ++d) {
                g.theta[d] = static_cast<const char*>(p->d_theta) + (size_t)d * p->Nk * rb;
                g.theta_scale[d] = (double)p->sign * p->gamma[d] * p->h[d];      // as nufft_set_points3 forms θ
                g.gamma[d] = p->gamma[d];
                g.source_center[d] = p->src_c[d];
                g.dx[d] = p->h[d];
                g.param[d] = p->kernel == NUFFT_KERNEL_GAUSSIAN ? p->sp->tau[d] : p->sp->beta[d];
            }
            for (int i = 0; i < g.ncomp; ++i) {
                g.f[i] = f_out[c0 + i];
                for (int d = 0; d < p->D; ++d) g.grad[i][d] = grad_out[(c0 + i) * p->D + d];
            }
            NUFFT_HIP(nufft::launch_t3_grad_finish(g, p->num_cus, stream));
        }
    }
    return NUFFT_OK;
}

int nufft_type3_points_outside(nufft_plan3* p, int64_t* sources_out, int64_t* targets_out, void* stream_) {
    if (!p) return fail(NUFFT_ERR_INVALID_ARG, "null plan");
    if (p->device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only plan (device = -1)");
    if (p->Np < 0 || p->Nk < 0) return fail(NUFFT_ERR_NO_POINTS, "nufft_set_points3 must be called first");
    DeviceGuard guard(p->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    unsigned long long h[2] = {0, 0};
    NUFFT_HIP(hipMemcpyAsync(h, p->d_outside, sizeof(h), hipMemcpyDeviceToHost, stream));
    NUFFT_HIP(hipStreamSynchronize(stream));
    if (sources_out) *sources_out = (int64_t)h[0];
    if (targets_out) *targets_out = (int64_t)h[1];
    return NUFFT_OK;
}

int nufft_set_timing3(nufft_plan3* p, int enable) {
    if (!p) return fail(NUFFT_ERR_INVALID_ARG, "null plan");
    if (p->device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only plan (device = -1)");
    p->timing = enable != 0;
    return NUFFT_OK;
}

int nufft_get_stage_times3(nufft_plan3* p, float* ms_out) {
    if (!p || !ms_out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (p->device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only plan (device = -1)");
    DeviceGuard guard(p->device);
    for (int s = 0; s < NUFFT3_NUM_STAGES; ++s) {
        ms_out[s] = -1.0f;
        if (!p->ev_valid[s]) continue;
        NUFFT_HIP(hipEventSynchronize(p->ev_end[s]));
        float ms = 0.0f;
        NUFFT_HIP(hipEventElapsedTime(&ms, p->ev_begin[s], p->ev_end[s]));
        ms_out[s] = ms;
    }
    return NUFFT_OK;
}

}  // extern "C"
