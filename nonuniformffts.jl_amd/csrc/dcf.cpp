// Sample-density compensation weights by the iteration of Pipe & Menon (include/nufft_mi355x.h, density compensation section;
// DESIGN.md section 18).
//
// The host side only enqueues: per iteration nufft_fill_zeros, nufft_spread_deferred and nufft_interpolate of an internal real-data
// plan (unchanged: interpolation completes the deferred spread by itself) and the two kernels of dcf_kernels.hip.  Every scalar lives
// on the device; with check_every > 0 the host looks at the done flag now and then, and at nothing else.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "dcf.h"
#include "solver_common.h"

using namespace nufft;

struct nufft_dcf {
    nufft_plan* plan = nullptr;       // the internal real-data plan (host-only when the parent is)
    int dtype = NUFFT_F64, D = 1, device = -1, num_cus = 256, G = 0;
    int max_iter = 1, check_every = 0, normalize = NUFFT_DCF_NORMALIZE_SUM, enqueued = -1;
    int kappa = 0;                    // the device's C is 2^kappa times the mathematical one
    double tol = 0.0;
    int64_t Np = -1, capacity = 0;
    void* d_v = nullptr;              // T[capacity]
    void* d_part = nullptr;           // double[kDcfMaxGroups][2]
    ScalarMirror scal;                // double res, sum; int32 flag[2], iters, status
    void* d_hist = nullptr;           // double[max_iter]
    int64_t own_bytes = 0;
};

namespace {

constexpr size_t kScalBytes = 2 * sizeof(double) + 4 * sizeof(int32_t);
constexpr size_t kPartBytes = (size_t)kDcfMaxGroups * 2 * sizeof(double);
size_t hist_bytes(const nufft_dcf* s) { return (size_t)s->max_iter * sizeof(double); }
size_t v_bytes(const nufft_dcf* s, int64_t capacity) { return capacity > 0 ? padded((size_t)capacity * real_bytes(s->dtype)) : 0; }
// what a device object of these parameters and this capacity owns next to its plan
size_t own_bytes_of(const nufft_dcf* s) { return padded(kPartBytes) + padded(kScalBytes) + padded(hist_bytes(s)) + v_bytes(s, s->capacity); }

int alloc(nufft_dcf* s, void** ptr, size_t bytes) { return alloc_buffer(s->own_bytes, "density-compensation", ptr, bytes); }

void release(nufft_dcf* s) {
    if (!s) return;
    if (s->device >= 0) {
        DeviceGuard g(s->device);
        for (void* p : {s->d_v, s->d_part, s->d_hist})
            if (p) (void)hipFree(p);
        s->scal.release();
    }
    if (s->plan) nufft_plan_destroy(s->plan);
    delete s;
}

DcfScalars scalars_at(const nufft_dcf* s, void* base) {
    DcfScalars k{};
    double* d = static_cast<double*>(base);
    k.res = d;
    k.sum = d + 1;
    int32_t* i = reinterpret_cast<int32_t*>(d + 2);
    k.flag = i;
    k.iters = i + 2;
    k.status = i + 3;
    k.history = static_cast<double*>(s->d_hist);
    k.part = static_cast<double*>(s->d_part);
    return k;
}

int launched(hipError_t e) {
    return e == hipSuccess ? NUFFT_OK : fail(NUFFT_ERR_HIP, std::string("launch of a density-compensation kernel: ") + hipGetErrorString(e));
}

}  // namespace

extern "C" {

int64_t nufft_sizeof_dcf_params(void) { return (int64_t)sizeof(nufft_dcf_params); }
int64_t nufft_sizeof_dcf_info(void) { return (int64_t)sizeof(nufft_dcf_info); }

int nufft_dcf_create(nufft_dcf** out, const nufft_plan* plan, const nufft_dcf_params* params) {
    if (!out || !plan || !params) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    nufft_dcf_params p;
    int rc = read_params(p, params, "nufft_dcf_params");
    if (rc) return rc;
    if (p.max_iter < 1) return fail(NUFFT_ERR_INVALID_ARG, "max_iter must be at least 1");
    if (p.max_iter > (1 << 24)) return fail(NUFFT_ERR_INVALID_ARG, "max_iter beyond 2^24");
    if (p.check_every < 0) return fail(NUFFT_ERR_INVALID_ARG, "check_every must not be negative");
    if (!std::isfinite(p.tol) || p.tol < 0) return fail(NUFFT_ERR_INVALID_ARG, "tol must be finite and not negative");
    if (p.normalize != NUFFT_DCF_NORMALIZE_SUM && p.normalize != NUFFT_DCF_NORMALIZE_NONE)
        return fail(NUFFT_ERR_INVALID_ARG, "normalize must be NUFFT_DCF_NORMALIZE_SUM or NUFFT_DCF_NORMALIZE_NONE");

    nufft_dcf* s = new (std::nothrow) nufft_dcf();
    if (!s) return fail(NUFFT_ERR_ALLOC, "out of host memory");
    s->dtype = plan->dtype;
    s->D = plan->D;
    s->device = plan->device;
    s->num_cus = plan->num_cus;
    s->max_iter = p.max_iter;
    s->check_every = p.check_every;
    s->normalize = p.normalize;
    s->tol = p.tol;

    // the real-data plan of the parent's parameters; the shape parameter per dimension verbatim
    nufft_params prm;
    std::memset(&prm, 0, sizeof(prm));
    prm.struct_size = (int32_t)sizeof(prm);
    prm.dtype = plan->dtype;
    prm.is_complex = 0;
    prm.ndim = plan->D;
    for (int d = 0; d < plan->D; ++d) {
        prm.N[d] = plan->N[d];
        prm.kernel_param_dim[d] = plan->kernel == NUFFT_KERNEL_BSPLINE ? 0.0 : plan->beta[d];
    }
    prm.half_support = plan->M;
    prm.sigma = plan->sigma_req;
    prm.kernel = plan->kernel;
    prm.evalmode = plan->evalmode;
    prm.ntransforms = 1;
    prm.fftshift = 0;
    prm.point_transform = plan->point_transform;
    prm.device = plan->device;
    const std::string options = plan->opts.str();
    prm.options = options.empty() ? nullptr : options.c_str();
    rc = nufft_plan_create_ex(&s->plan, &prm);
    if (rc) {
        const std::string keep = nufft_last_error_message();
        s->plan = nullptr;
        release(s);
        return fail(rc, "internal real-data plan of the density compensation: " + keep);
    }
    for (int d = 0; d < s->D; ++d) s->kappa += 2 * s->plan->scale_exp[d];

    if (s->device >= 0) {
        DeviceGuard guard(s->device);
        if ((rc = alloc(s, &s->d_part, kPartBytes)) || (rc = alloc(s, &s->d_hist, hist_bytes(s))) ||
            (rc = s->scal.create(s->own_bytes, "density-compensation", kScalBytes,
                                 "hipHostMalloc of the host mirror of the density compensation failed"))) {
            const std::string keep = nufft_last_error_message();
            release(s);
            return fail(rc, keep);
        }
        // a defined answer from nufft_dcf_get_result / nufft_dcf_history before the first compute
        if (s->scal.zero() != hipSuccess || hipMemset(s->d_hist, 0xFF, hist_bytes(s)) != hipSuccess ||
            hipMemset(s->d_part, 0, kPartBytes) != hipSuccess) {
            (void)hipGetLastError();
            release(s);
            return fail(NUFFT_ERR_HIP, "hipMemset of the scalars of the density compensation failed");
        }
    }
    *out = s;
    return NUFFT_OK;
}

int nufft_dcf_destroy(nufft_dcf* dcf) {
    release(dcf);
    return NUFFT_OK;
}

int nufft_dcf_get_info(const nufft_dcf* s, nufft_dcf_info* o) {
    if (!s || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    nufft_dcf_info i;
    std::memset(&i, 0, sizeof(i));
    i.ndim = s->D;
    i.dtype = s->dtype;
    i.device = s->device;
    i.max_iter = s->max_iter;
    i.check_every = s->check_every;
    i.normalize = s->normalize;
    i.workgroups = s->G;
    i.iterations_enqueued = s->enqueued;
    i.window_scale_log2 = s->kappa;
    for (int d = 0; d < 3; ++d) {
        i.N_over[d] = d < s->D ? s->plan->Nover[d] : 1;
        i.beta[d] = d < s->D ? s->plan->beta[d] : 0.0;
    }
    i.tol = s->tol;
    i.capacity = s->capacity;
    i.num_points = s->Np;
    i.workspace_bytes = s->device >= 0 ? s->own_bytes : (int64_t)own_bytes_of(s);
    i.plan_bytes = s->plan->workspace_bytes;
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_dcf_set_points(nufft_dcf* s, int64_t np, const void* const* coords, void* stream_) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (s->device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only density-compensation object (device = -1)");
    if (np < 0) return fail(NUFFT_ERR_INVALID_ARG, "negative number of points");
    if (!coords) return fail(NUFFT_ERR_INVALID_ARG, "null coordinate table");
    for (int d = 0; d < s->D; ++d)
        if (np > 0 && !coords[d]) return fail(NUFFT_ERR_INVALID_ARG, "null coordinate vector");
    DeviceGuard guard(s->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (np > s->capacity) {
        if (capturing(stream)) return fail(NUFFT_ERR_INVALID_ARG, "nufft_dcf_set_points grows a buffer: not on a capturing stream");
        NUFFT_HIP(hipStreamSynchronize(stream));      // an earlier compute may still read v
        free_buffer(s->own_bytes, s->d_v, (size_t)s->capacity * real_bytes(s->dtype));
        s->capacity = 0;
        s->Np = -1;
        const int rc = alloc(s, &s->d_v, (size_t)np * real_bytes(s->dtype));
        if (rc) return rc;
        s->capacity = np;
    }
    s->Np = -1;
    const int rc = nufft_set_points(s->plan, np, coords, stream);
    if (rc) return rc;
    s->Np = np;
    s->G = np > 0 ? dcf_workgroups(s->dtype, np, s->num_cus) : 0;
    return NUFFT_OK;
}

int nufft_dcf_compute(nufft_dcf* s, void* w, int use_w0, void* stream_) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (s->device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only density-compensation object (device = -1)");
    if (s->Np < 0) return fail(NUFFT_ERR_NO_POINTS, "nufft_dcf_set_points must be called before nufft_dcf_compute");
    if (s->Np == 0) return NUFFT_OK;
    if (!w) return fail(NUFFT_ERR_INVALID_ARG, "null weight vector");
    if ((uintptr_t)w & 15) return fail(NUFFT_ERR_INVALID_ARG, "the weight vector must be 16-byte aligned");
    DeviceGuard guard(s->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int prc = refuse_polling_capture(s->check_every, stream)) return prc;

    DcfLaunch a{};
    a.dtype = s->dtype;
    a.G = s->G;
    a.n = s->Np;
    a.w = w;
    a.v = s->d_v;
    a.tol = s->tol;
    a.vscale = 1.0;
    a.gamma = std::ldexp(1.0, s->kappa);
    a.max_iter = s->max_iter;
    a.normalize = s->normalize;
    a.s = scalars_at(s, s->scal.dev);

    s->enqueued = 0;
    const bool warm = use_w0 != 0;
    int rc;
    if ((rc = launched(launch_dcf_start(a, warm, stream)))) return rc;
    if ((rc = launched(launch_dcf_begin(a, stream)))) return rc;
    const DcfScalars host = scalars_at(s, s->scal.host);
    const void* in[1] = {w};
    void* outv[1] = {s->d_v};
    for (int k = 0; k < s->max_iter; ++k) {
        a.k = k;
        a.report = (k >= 1 || warm) ? 1 : 0;
        // the caller's w0 is in true units: its C w0 is what the device computes, divided by 2^κ; from the first division on the state
        // is u = w / 2^κ, whose C w is what the device computes
        a.vscale = (k == 0 && warm) ? std::ldexp(1.0, -s->kappa) : 1.0;
        if ((rc = nufft_fill_zeros(s->plan, stream))) return rc;
        if ((rc = nufft_spread_deferred(s->plan, in, stream))) return rc;
        if ((rc = nufft_interpolate(s->plan, outv, stream))) return rc;
        if ((rc = launched(launch_dcf_check(a, stream)))) return rc;
        if ((rc = launched(launch_dcf_update(a, stream)))) return rc;
        s->enqueued = k + 1;
        if (s->check_every > 0 && (k + 1) % s->check_every == 0 && k + 1 < s->max_iter) {
            bool done;
            if ((rc = all_done(s->scal, stream, host.flag + ((k + 1) & 1), 1, &done))) return rc;
            if (done) break;
        }
    }
    if (s->normalize == NUFFT_DCF_NORMALIZE_SUM) {
        if ((rc = launched(launch_dcf_sum(a, stream)))) return rc;
        if ((rc = launched(launch_dcf_scale(a, stream)))) return rc;
    } else if (s->kappa != 0) {
        if ((rc = launched(launch_dcf_scale(a, stream)))) return rc;
    }
    return NUFFT_OK;
}

int nufft_dcf_get_result(nufft_dcf* s, int32_t* iterations, int32_t* status, double* residual, void* stream_) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (s->device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only density-compensation object (device = -1)");
    DeviceGuard guard(s->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc;
    if ((rc = refuse_capture("nufft_dcf_get_result", stream)) || (rc = s->scal.fetch(stream))) return rc;
    const DcfScalars host = scalars_at(s, s->scal.host);
    if (iterations) *iterations = host.iters[0];
    if (status) *status = host.status[0];
    if (residual) *residual = host.res[0];
    return NUFFT_OK;
}

int nufft_dcf_history(nufft_dcf* s, double* host_out, int64_t capacity, void* stream_) {
    if (!s || !host_out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (s->device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only density-compensation object (device = -1)");
    if (capacity < (int64_t)s->max_iter) return fail(NUFFT_ERR_INVALID_ARG, "capacity is smaller than max_iter");
    DeviceGuard guard(s->device);
    return fetch_history("nufft_dcf_history", host_out, s->d_hist, hist_bytes(s), static_cast<hipStream_t>(stream_));
}

}  // extern "C"
