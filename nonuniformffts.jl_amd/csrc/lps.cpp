// Low-rank plus sparse reconstruction of a series of frames (include/nufft_mi355x.h, L+S section): the global
// low-rank map (nufft_glr_*), the temporal transform (nufft_tsparse_*) and the solver (nufft_lps_*).
//
// The host side only enqueues.  A global low-rank apply is three launches (Gram, eigen, apply: glr_kernels.hip), a temporal transform
// one (tsparse_kernels.hip).  A solver iteration is one nufft_toeplitz_apply (unchanged), those four kernels in their solver variants
// and the decision kernel; every scalar lives on the device, and with check_every > 0 the host looks at the done flag now and then, and
// at nothing else.  The frame pointers travel as kernel arguments: no device table is written, so a solve is free of copies.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "lps.h"
#include "solver_common.h"
#include "stream_kernels.h"

using namespace nufft;

struct nufft_glr {
    int dtype = NUFFT_F64, D = 1, C = 1, device = -1;
    int64_t N[3] = {1, 1, 1};
    int64_t n = 1;
    FlatTiling tl{}, tla{};       // of the Gram kernel, of the apply kernel (the same tiles, more workgroups)
    void* d_gram = nullptr;      // complex double [G][K (K + 1) / 2]
    void* d_P = nullptr;         // complex double [K][K]
    void* d_words = nullptr;     // double nuc; int32 sweeps
    void* d_part = nullptr;      // double[tla.G][2]: the solver's variant of the apply kernel
    int64_t own_bytes = 0;
};

struct nufft_tsparse {
    int dtype = NUFFT_F64, D = 1, C = 1, device = -1, transform = NUFFT_TSPARSE_DFT;
    int64_t N[3] = {1, 1, 1};
    int64_t n = 1;
    FlatTiling tl{};
    double tw[2 * kLpsMaxK] = {};
    void* d_part = nullptr;      // double[G][3]
    int64_t own_bytes = 0;
};

struct nufft_lps {
    nufft_toeplitz* tz = nullptr;
    nufft_glr* glr = nullptr;
    nufft_tsparse* ts = nullptr;
    int dtype = NUFFT_F64, C = 1, device = -1, G0 = 1;
    int max_iter = 1, check_every = 0, enqueued = -1, transform = NUFFT_TSPARSE_DFT, momentum = 1;
    double tol = 0.0, step = 1.0, lambda = 0.0, nuc = 0.0, l1 = 0.0;
    int64_t n = 0;
    void* d_arrays = nullptr;    // L, S, zL, zS, q: [5][C] arrays
    ScalarMirror scal;           // double change; int32 flag, iters, status
    void* d_hist = nullptr;      // double[max_iter][3]
    int64_t array_bytes = 0, own_bytes = 0;
    std::vector<void*> Ltab, Stab, zLtab, zStab, qtab;
};

namespace {

void release(nufft_glr* g) {
    if (!g) return;
    if (g->device >= 0) {
        DeviceGuard guard(g->device);
        for (void* p : {g->d_gram, g->d_P, g->d_words, g->d_part})
            if (p) (void)hipFree(p);
    }
    delete g;
}

void release(nufft_tsparse* t) {
    if (!t) return;
    if (t->device >= 0 && t->d_part) {
        DeviceGuard guard(t->device);
        (void)hipFree(t->d_part);
    }
    delete t;
}

void release(nufft_lps* s) {
    if (!s) return;
    release(s->glr);
    release(s->ts);
    if (s->device >= 0) {
        DeviceGuard guard(s->device);
        for (void* p : {s->d_arrays, s->d_hist})
            if (p) (void)hipFree(p);
        s->scal.release();
    }
    delete s;
}

int check_frames(int C) {
    if (C > kLpsMaxK)
        return fail(NUFFT_ERR_UNSUPPORTED, std::to_string(C) + " transforms: more than the " + std::to_string(kLpsMaxK) +
                                               " frames of a one-wave Jacobi team and of K x K matrices in LDS");
    return NUFFT_OK;
}

int64_t cells_of(int D, const int64_t* N) {
    int64_t n = 1;
    for (int d = 0; d < D; ++d) n *= N[d];
    return n;
}

int glr_geometry(nufft_glr** out, int dtype, int D, const int64_t* N, int C, int device) {
    if (int rc = check_frames(C)) return rc;
    if (device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only plan (device = -1): the global low-rank map runs on the device");
    nufft_glr* g = new (std::nothrow) nufft_glr();
    if (!g) return fail(NUFFT_ERR_ALLOC, "out of host memory");
    g->dtype = dtype;
    g->D = D;
    g->C = C;
    g->device = device;
    for (int d = 0; d < D; ++d) g->N[d] = N[d];
    g->n = cells_of(D, N);
    g->tl = lps_tiling(C, g->n, kGlrTileElems, kGlrGramGroups);
    g->tla = lps_tiling(C, g->n, kGlrTileElems, kLpsStreamGroups);
    const size_t np = (size_t)C * (C + 1) / 2;
    DeviceGuard guard(device);
    int rc;
    if ((rc = alloc_buffer(g->own_bytes, "global low-rank", &g->d_gram, (size_t)g->tl.G * np * 16)) ||
        (rc = alloc_buffer(g->own_bytes, "global low-rank", &g->d_P, (size_t)C * C * 16)) ||
        (rc = alloc_buffer(g->own_bytes, "global low-rank", &g->d_words, 16)) ||
        (rc = alloc_buffer(g->own_bytes, "global low-rank", &g->d_part, (size_t)g->tla.G * 2 * sizeof(double)))) {
        const std::string keep = nufft_last_error_message();
        release(g);
        return fail(rc, keep);
    }
    if (hipMemset(g->d_words, 0, 16) != hipSuccess) {
        (void)hipGetLastError();
        release(g);
        return fail(NUFFT_ERR_HIP, "hipMemset of the global low-rank scalars failed");
    }
    *out = g;
    return NUFFT_OK;
}

int transform_ok(int32_t transform) {
    if (transform != NUFFT_TSPARSE_IDENTITY && transform != NUFFT_TSPARSE_DFT)
        return fail(NUFFT_ERR_INVALID_ARG, "transform must be NUFFT_TSPARSE_IDENTITY or NUFFT_TSPARSE_DFT");
    return NUFFT_OK;
}

int tsparse_geometry(nufft_tsparse** out, int dtype, int D, const int64_t* N, int C, int device, int transform) {
    if (int rc = check_frames(C)) return rc;
    if (device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only plan (device = -1): the temporal transform runs on the device");
    nufft_tsparse* t = new (std::nothrow) nufft_tsparse();
    if (!t) return fail(NUFFT_ERR_ALLOC, "out of host memory");
    t->dtype = dtype;
    t->D = D;
    t->C = C;
    t->device = device;
    t->transform = transform;
    for (int d = 0; d < D; ++d) t->N[d] = N[d];
    t->n = cells_of(D, N);
    t->tl = lps_tiling(C, t->n, kTsTileElems, kLpsStreamGroups);
    const double scale = 1.0 / std::sqrt((double)C);
    for (int m = 0; m < C; ++m) {
        const double ang = -2.0 * M_PI * (double)m / (double)C;
        t->tw[2 * m] = scale * std::cos(ang);
        t->tw[2 * m + 1] = scale * std::sin(ang);
    }
    DeviceGuard guard(device);
    if (int rc = alloc_buffer(t->own_bytes, "temporal transform", &t->d_part, (size_t)t->tl.G * 3 * sizeof(double))) {
        const std::string keep = nufft_last_error_message();
        release(t);
        return fail(rc, keep);
    }
    *out = t;
    return NUFFT_OK;
}

int real_plan() {
    return fail(NUFFT_ERR_UNSUPPORTED, "the low-rank plus sparse objects need a complex plan: their arrays are those of the Toeplitz normal operator, "
                                       "which a real-data plan cannot have");
}

// C outputs and C inputs, 16-byte aligned; out[c] may be exactly in[c], nothing else may overlap
int check_tables(int C, int64_t n, int dtype, void* const* out, const void* const* in) {
    return nufft::check_tables(C, (size_t)n * 2 * real_bytes(dtype), out, in, true, "the output overlaps the input: out[c] may be exactly in[c], nothing else");
}

GlrLaunch glr_template(const nufft_glr* g) {
    GlrLaunch a{};
    a.dtype = g->dtype;
    a.K = g->C;
    a.mode = GLR_PLAIN;
    a.tl = g->tl;
    a.n = g->n;
    a.gram = static_cast<double*>(g->d_gram);
    a.P = static_cast<double*>(g->d_P);
    a.nuc = static_cast<double*>(g->d_words);
    a.sweeps = reinterpret_cast<int32_t*>(static_cast<char*>(g->d_words) + 8);
    a.part = static_cast<double*>(g->d_part);
    return a;
}

TsLaunch ts_template(const nufft_tsparse* t) {
    TsLaunch a{};
    a.dtype = t->dtype;
    a.K = t->C;
    a.transform = t->transform;
    a.tl = t->tl;
    a.n = t->n;
    std::memcpy(a.tw, t->tw, sizeof(a.tw));
    a.part = static_cast<double*>(t->d_part);
    return a;
}

template <typename Ptr>
void fill(LpsFrames& f, Ptr const* tab, int C) {
    for (int c = 0; c < C; ++c) f.p[c] = const_cast<void*>(static_cast<const void*>(tab[c]));
}

int run_transform(nufft_tsparse* t, int mode, void* const* out, const void* const* in, double thr, double* l1_out, void* stream_) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (int rc = check_tables(t->C, t->n, t->dtype, out, in)) return rc;
    if (!weight_ok(thr)) return fail(NUFFT_ERR_INVALID_ARG, "the threshold must be finite and not negative");
    TsLaunch a = ts_template(t);
    a.mode = mode;
    a.t = thr;
    fill(a.f0, in, t->C);
    fill(a.f1, out, t->C);
    DeviceGuard guard(t->device);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipError_t e = launch_tsparse(a, s);
    if (e == hipSuccess && l1_out) e = launch_tsparse_sum(a.part, t->tl.G, l1_out, s);
    if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a temporal-transform kernel: ") + hipGetErrorString(e));
    return NUFFT_OK;
}

size_t hist_bytes(const nufft_lps* s) { return (size_t)s->max_iter * 3 * sizeof(double); }

}  // namespace

extern "C" {

int64_t nufft_sizeof_glr_info(void) { return (int64_t)sizeof(nufft_glr_info); }
int64_t nufft_sizeof_tsparse_info(void) { return (int64_t)sizeof(nufft_tsparse_info); }
int64_t nufft_sizeof_lps_params(void) { return (int64_t)sizeof(nufft_lps_params); }
int64_t nufft_sizeof_lps_info(void) { return (int64_t)sizeof(nufft_lps_info); }

/* ---- the global low-rank map ---- */

int nufft_glr_create(nufft_glr** out, const nufft_plan* plan) {
    if (!out || !plan) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!plan->is_complex) return real_plan();
    return glr_geometry(out, plan->dtype, plan->D, plan->N, plan->C, plan->device);
}

int nufft_glr_create_for_operator(nufft_glr** out, const nufft_toeplitz* tz) {
    if (!out || !tz) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    nufft_toeplitz_info ti;
    if (int rc = toeplitz_info(tz, ti)) return rc;
    return glr_geometry(out, ti.dtype, ti.ndim, ti.N, ti.ntransforms, ti.device);
}

int nufft_glr_destroy(nufft_glr* g) {
    release(g);
    return NUFFT_OK;
}

int nufft_glr_get_info(const nufft_glr* g, nufft_glr_info* o) {
    if (!g || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    nufft_glr_info i;
    std::memset(&i, 0, sizeof(i));
    i.ndim = g->D;
    i.dtype = g->dtype;
    i.ntransforms = g->C;
    i.device = g->device;
    i.tile_cells = g->tl.TC;
    i.jacobi_sweeps_max = jacobi_team::kSweepsMax;
    for (int d = 0; d < 3; ++d) i.N[d] = g->N[d];
    i.cells = g->n;
    i.workgroups = g->tl.G;
    i.workspace_bytes = g->own_bytes;
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_glr_apply(nufft_glr* g, void* const* out, const void* const* in, double t, double* nuc_out_device, void* stream_) {
    if (!g) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (int rc = check_tables(g->C, g->n, g->dtype, out, in)) return rc;
    if (!weight_ok(t)) return fail(NUFFT_ERR_INVALID_ARG, "the threshold must be finite and not negative");
    GlrLaunch a = glr_template(g);
    a.t = t;
    a.nuc_out = nuc_out_device;
    fill(a.f0, in, g->C);
    fill(a.f1, out, g->C);
    DeviceGuard guard(g->device);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipError_t e = launch_glr_gram(a, s);
    if (e == hipSuccess) e = launch_glr_eigen(a, s);
    a.tl = g->tla;
    if (e == hipSuccess) e = launch_glr_apply(a, s);
    if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a global low-rank kernel: ") + hipGetErrorString(e));
    return NUFFT_OK;
}

int nufft_glr_last_sweeps(nufft_glr* g, int32_t* sweeps_out, void* stream_) {
    if (!g || !sweeps_out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    DeviceGuard guard(g->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (capturing(stream)) return fail(NUFFT_ERR_INVALID_ARG, "nufft_glr_last_sweeps synchronises: not on a capturing stream");
    NUFFT_HIP(hipMemcpyAsync(sweeps_out, static_cast<char*>(g->d_words) + 8, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    NUFFT_HIP(hipStreamSynchronize(stream));
    return NUFFT_OK;
}

/* ---- the temporal transform ---- */

int nufft_tsparse_create(nufft_tsparse** out, const nufft_plan* plan, int32_t transform) {
    if (!out || !plan) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (int rc = transform_ok(transform)) return rc;
    if (!plan->is_complex) return real_plan();
    return tsparse_geometry(out, plan->dtype, plan->D, plan->N, plan->C, plan->device, transform);
}

int nufft_tsparse_create_for_operator(nufft_tsparse** out, const nufft_toeplitz* tz, int32_t transform) {
    if (!out || !tz) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (int rc = transform_ok(transform)) return rc;
    nufft_toeplitz_info ti;
    if (int rc = toeplitz_info(tz, ti)) return rc;
    return tsparse_geometry(out, ti.dtype, ti.ndim, ti.N, ti.ntransforms, ti.device, transform);
}

int nufft_tsparse_destroy(nufft_tsparse* t) {
    release(t);
    return NUFFT_OK;
}

int nufft_tsparse_get_info(const nufft_tsparse* t, nufft_tsparse_info* o) {
    if (!t || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    nufft_tsparse_info i;
    std::memset(&i, 0, sizeof(i));
    i.ndim = t->D;
    i.dtype = t->dtype;
    i.ntransforms = t->C;
    i.device = t->device;
    i.transform = t->transform;
    i.tile_cells = t->tl.TC;
    for (int d = 0; d < 3; ++d) i.N[d] = t->N[d];
    i.cells = t->n;
    i.workgroups = t->tl.G;
    i.workspace_bytes = t->own_bytes;
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_tsparse_forward(nufft_tsparse* t, void* const* out, const void* const* in, void* stream) {
    return run_transform(t, TS_FORWARD, out, in, 0.0, nullptr, stream);
}

int nufft_tsparse_inverse(nufft_tsparse* t, void* const* out, const void* const* in, void* stream) {
    return run_transform(t, TS_INVERSE, out, in, 0.0, nullptr, stream);
}

int nufft_tsparse_shrink(nufft_tsparse* t, void* const* coeff_out, const void* const* in, double thr, double* l1_out_device, void* stream) {
    return run_transform(t, TS_SHRINK, coeff_out, in, thr, l1_out_device, stream);
}

/* ---- the solver ---- */

int nufft_lps_create(nufft_lps** out, nufft_toeplitz* tz, const nufft_lps_params* params) {
    if (!out || !tz || !params) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    nufft_toeplitz_info ti;
    int rc = toeplitz_info(tz, ti);
    if (rc) return rc;
    nufft_lps_params p;
    if ((rc = read_params(p, params, "nufft_lps_params"))) return rc;
    if (p.max_iter < 1) return fail(NUFFT_ERR_INVALID_ARG, "max_iter must be at least 1");
    if (p.max_iter > (1 << 24)) return fail(NUFFT_ERR_INVALID_ARG, "max_iter beyond 2^24");
    if (p.check_every < 0) return fail(NUFFT_ERR_INVALID_ARG, "check_every must not be negative");
    if ((rc = transform_ok(p.transform))) return rc;
    if (p.momentum != 0 && p.momentum != 1) return fail(NUFFT_ERR_INVALID_ARG, "momentum must be 0 or 1");
    if (!weight_ok(p.tol)) return fail(NUFFT_ERR_INVALID_ARG, "tol must be finite and not negative");
    if (!weight_ok(p.lambda)) return fail(NUFFT_ERR_INVALID_ARG, "lambda must be finite and not negative");
    if (!weight_ok(p.nuc)) return fail(NUFFT_ERR_INVALID_ARG, "nuc must be finite and not negative");
    if (!weight_ok(p.l1)) return fail(NUFFT_ERR_INVALID_ARG, "l1 must be finite and not negative");
    if (!std::isfinite(p.step) || !(p.step > 0.0))
        return fail(NUFFT_ERR_INVALID_ARG, "step must be finite and positive (1 / (2 (lambda_max + lambda)): nufft_toeplitz_max_eigenvalue)");

    nufft_lps* s = new (std::nothrow) nufft_lps();
    if (!s) return fail(NUFFT_ERR_ALLOC, "out of host memory");
    if ((rc = glr_geometry(&s->glr, ti.dtype, ti.ndim, ti.N, ti.ntransforms, ti.device)) ||      // more than 32 frames, host-only: refused here
        (rc = tsparse_geometry(&s->ts, ti.dtype, ti.ndim, ti.N, ti.ntransforms, ti.device, p.transform))) {
        const std::string keep = nufft_last_error_message();
        release(s);
        return fail(rc, keep);
    }
    s->tz = tz;
    s->dtype = ti.dtype;
    s->C = ti.ntransforms;
    s->device = ti.device;
    s->max_iter = p.max_iter;
    s->check_every = p.check_every;
    s->transform = p.transform;
    s->momentum = p.momentum;
    s->tol = p.tol;
    s->step = p.step;
    s->lambda = p.lambda;
    s->nuc = p.nuc;
    s->l1 = p.l1;
    s->n = s->glr->n;
    const size_t rb = real_bytes(s->dtype), comp = padded((size_t)s->n * 2 * rb);
    s->array_bytes = 5 * (int64_t)s->C * (int64_t)comp;

    DeviceGuard guard(s->device);
    s->G0 = (int)stream::grid_for(s->n, device_cus(s->device));
    if ((rc = alloc_buffer(s->own_bytes, "L+S solver", &s->d_arrays, (size_t)5 * s->C * comp)) ||
        (rc = create_outcome(s->own_bytes, "L+S solver", s->scal, &s->d_hist, prox_scal_bytes(1), hist_bytes(s)))) {
        const std::string keep = nufft_last_error_message();
        release(s);
        return fail(rc, keep);
    }
    // a defined answer from nufft_lps_get_parts before the first solve
    if (hipMemset(s->d_arrays, 0, (size_t)5 * s->C * comp) != hipSuccess) {
        (void)hipGetLastError();
        release(s);
        return fail(NUFFT_ERR_HIP, "hipMemset of the solver's arrays failed");
    }
    std::vector<void*>* tabs[5] = {&s->Ltab, &s->Stab, &s->zLtab, &s->zStab, &s->qtab};
    for (int a = 0; a < 5; ++a)
        for (int c = 0; c < s->C; ++c) tabs[a]->push_back(static_cast<char*>(s->d_arrays) + ((size_t)a * s->C + c) * comp);
    *out = s;
    return NUFFT_OK;
}

int nufft_lps_destroy(nufft_lps* s) {
    release(s);
    return NUFFT_OK;
}

int nufft_lps_set_weights(nufft_lps* s, double nuc, double l1) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (!weight_ok(nuc)) return fail(NUFFT_ERR_INVALID_ARG, "nuc must be finite and not negative");
    if (!weight_ok(l1)) return fail(NUFFT_ERR_INVALID_ARG, "l1 must be finite and not negative");
    s->nuc = nuc;
    s->l1 = l1;
    return NUFFT_OK;
}

int nufft_lps_get_info(const nufft_lps* s, nufft_lps_info* o) {
    if (!s || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    nufft_lps_info i;
    std::memset(&i, 0, sizeof(i));
    i.ntransforms = s->C;
    i.dtype = s->dtype;
    i.max_iter = s->max_iter;
    i.check_every = s->check_every;
    i.transform = s->transform;
    i.momentum = s->momentum;
    i.iterations_enqueued = s->enqueued;
    i.tol = s->tol;
    i.step = s->step;
    i.lambda = s->lambda;
    i.nuc = s->nuc;
    i.l1 = s->l1;
    i.array_bytes = s->array_bytes;
    i.workspace_bytes = s->own_bytes + s->glr->own_bytes + s->ts->own_bytes;
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_lps_solve(nufft_lps* s, void* const* x, const void* const* b, int use_x0, void* stream_) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    DeviceGuard guard(s->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc = check_solve_args(s->tz, "nufft_lps_solve", s->C, s->n, s->dtype, x, b, s->check_every, stream);
    if (rc) return rc;

    const int C = s->C;
    LpsSolve h{};
    h.dtype = s->dtype;
    h.K = C;
    h.G = s->G0;
    h.n = s->n;
    h.max_iter = s->max_iter;
    h.tol = s->tol;
    h.part_l = static_cast<const double*>(s->glr->d_part);
    h.part_s = static_cast<const double*>(s->ts->d_part);
    h.Gl = s->glr->tla.G;
    h.Gs = s->ts->tl.G;
    h.nuc = static_cast<const double*>(s->glr->d_words);
    h.s = prox_scalars_at(s->scal.dev, 1, s->d_hist);
    fill(h.x, x, C);
    fill(h.L, s->Ltab.data(), C);
    fill(h.S, s->Stab.data(), C);
    fill(h.zL, s->zLtab.data(), C);
    fill(h.zS, s->zStab.data(), C);

    GlrLaunch gram = glr_template(s->glr);
    gram.mode = GLR_SOLVER;
    gram.t = s->step * s->nuc;
    gram.step = s->step;
    gram.lambda = s->lambda;
    gram.flag = h.s.flag;
    GlrLaunch apply = gram;
    apply.tl = s->glr->tla;
    fill(gram.f0, s->zLtab.data(), C);
    fill(gram.f1, s->zStab.data(), C);
    fill(gram.f2, s->qtab.data(), C);
    fill(gram.f3, b, C);
    fill(apply.f0, s->zLtab.data(), C);
    fill(apply.f1, s->Ltab.data(), C);
    fill(apply.f2, s->qtab.data(), C);
    TsLaunch ts = ts_template(s->ts);
    ts.mode = TS_SOLVER;
    ts.t = s->step * s->l1;
    ts.flag = h.s.flag;
    fill(ts.f0, s->zStab.data(), C);
    fill(ts.f1, s->qtab.data(), C);
    fill(ts.f2, s->Stab.data(), C);
    fill(ts.f3, s->zLtab.data(), C);
    fill(ts.f4, x, C);

    s->enqueued = 0;
    hipError_t e = launch_lps_start(h, use_x0 != 0, stream);
    if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of an L+S solver kernel: ") + hipGetErrorString(e));
    const ProxScalars host = prox_scalars_at(s->scal.host, 1, nullptr);
    double t = 1.0;
    for (int it = 1; it <= s->max_iter; ++it) {
        h.it = it;
        const double t_next = 0.5 * (1.0 + std::sqrt(1.0 + 4.0 * t * t));
        apply.beta = ts.beta = s->momentum ? (t - 1.0) / t_next : 0.0;
        t = t_next;
        if ((rc = nufft_toeplitz_apply(s->tz, s->qtab.data(), const_cast<const void* const*>(x), stream))) return rc;      // q = G u
        e = launch_glr_gram(gram, stream);
        if (e == hipSuccess) e = launch_glr_eigen(gram, stream);
        if (e == hipSuccess) e = launch_glr_apply(apply, stream);
        if (e == hipSuccess) e = launch_tsparse(ts, stream);
        if (e == hipSuccess) e = launch_lps_decide(h, stream);
        if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of an L+S solver kernel: ") + hipGetErrorString(e));
        s->enqueued = it;
        if (s->check_every > 0 && it % s->check_every == 0 && it < s->max_iter) {
            bool done;
            if ((rc = all_done(s->scal, stream, host.flag, 1, &done))) return rc;
            if (done) break;
        }
    }
    e = launch_lps_sum(h, stream);                                                                                           // x = L + S
    if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of an L+S solver kernel: ") + hipGetErrorString(e));
    return NUFFT_OK;
}

int nufft_lps_get_parts(nufft_lps* s, void* const* L_out, void* const* S_out, void* stream_) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    for (void* const* tab : {L_out, S_out})
        for (int c = 0; tab && c < s->C; ++c)
            if (!tab[c]) return fail(NUFFT_ERR_INVALID_ARG, "null data vector");
    const size_t bytes = (size_t)s->n * 2 * real_bytes(s->dtype);
    // every destination apart from every other one, and from the solver's five arrays per frame (one allocation)
    std::vector<const void*> dst;
    for (void* const* tab : {L_out, S_out})
        for (int c = 0; tab && c < s->C; ++c) dst.push_back(tab[c]);
    for (size_t i = 0; i < dst.size(); ++i) {
        for (size_t k = 0; k < i; ++k)
            if (overlap(dst[i], dst[k], bytes)) return fail(NUFFT_ERR_INVALID_ARG, "two of the output arrays overlap");
        const char* own = static_cast<const char*>(s->d_arrays);
        const char* d = static_cast<const char*>(dst[i]);
        if (d < own + s->array_bytes && own < d + bytes) return fail(NUFFT_ERR_INVALID_ARG, "an output array overlaps the solver's own arrays");
    }
    DeviceGuard guard(s->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    for (int c = 0; c < s->C; ++c) {
        if (L_out) NUFFT_HIP(hipMemcpyAsync(L_out[c], s->Ltab[c], bytes, hipMemcpyDeviceToDevice, stream));
        if (S_out) NUFFT_HIP(hipMemcpyAsync(S_out[c], s->Stab[c], bytes, hipMemcpyDeviceToDevice, stream));
    }
    return NUFFT_OK;
}

int nufft_lps_get_result(nufft_lps* s, int32_t* iterations, int32_t* status, double* change, int64_t capacity, void* stream_) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (capacity < s->C) return fail(NUFFT_ERR_INVALID_ARG, "capacity is smaller than ntransforms");
    DeviceGuard guard(s->device);
    return copy_result("nufft_lps_get_result", s->scal, 1, s->C, 0, iterations, status, change, static_cast<hipStream_t>(stream_));
}

int nufft_lps_history(nufft_lps* s, double* host_out, int64_t capacity, void* stream_) {
    if (!s || !host_out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (capacity < (int64_t)s->max_iter * 3) return fail(NUFFT_ERR_INVALID_ARG, "capacity is smaller than max_iter * 3");
    DeviceGuard guard(s->device);
    return fetch_history("nufft_lps_history", host_out, s->d_hist, hist_bytes(s), static_cast<hipStream_t>(stream_));
}

}  // extern "C"
