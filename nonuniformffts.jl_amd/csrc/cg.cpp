// Conjugate gradients on (G + λI) x = b, G a Toeplitz normal operator (include/nufft_mi355x.h, CG section).
//
// The host side only enqueues: per iteration one nufft_toeplitz_apply (unchanged) and the three kernels of cg_kernels.hip.  Every
// scalar lives on the device; with check_every > 0 the host looks at the done flags now and then, and at nothing else.
//
// With a preconditioner set (nufft_cg_set_preconditioner, DESIGN.md sections 21 and 22) an iteration is the apply, the dot kernel, pcg_update_kernel,
// the preconditioner's apply, the dot kernel on (r, z) and pcg_direction_kernel; without one, exactly the launches above.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "cg.h"
#include "precond.h"
#include "solver_common.h"

using namespace nufft;

struct nufft_cg {
    nufft_toeplitz* tz = nullptr;
    int dtype = NUFFT_F64, C = 1, device = -1, num_cus = 256, G = 1;
    int max_iter = 1, check_every = 0, enqueued = -1;
    double rtol = 0.0, lambda = 0.0;
    int64_t n = 0;                    // complex elements per component
    int64_t stride = 0;               // reals between components of r, p, q
    void* d_r = nullptr;
    void* d_p = nullptr;
    void* d_q = nullptr;
    void* d_z = nullptr;              // with a preconditioner: z = M⁻¹ r
    nufft_precond* pc = nullptr;      // borrowed
    void* d_part = nullptr;           // double[C][G][2] + double[C][G]
    ScalarMirror scal;                // double rho[2][C], beta0[C], res[C], rhoz[2][C]; int32 flag[2][C], brk[C], iters[C], status[C]
    void* d_hist = nullptr;           // double[max_iter + 1][C]
    int64_t array_bytes = 0, own_bytes = 0;
    std::vector<void*> ptab, qtab;    // the pointer tables nufft_toeplitz_apply takes
    std::vector<void*> rtab, ztab;    // ... and nufft_precond_apply
};

namespace {

size_t scal_bytes(const nufft_cg* s) { return (size_t)s->C * (6 * sizeof(double) + 5 * sizeof(int32_t)); }
size_t part_bytes(const nufft_cg* s) { return (size_t)s->C * s->G * 3 * sizeof(double); }
size_t hist_bytes(const nufft_cg* s) { return (size_t)(s->max_iter + 1) * s->C * sizeof(double); }

int alloc(nufft_cg* s, void** ptr, size_t bytes) { return alloc_buffer(s->own_bytes, "CG", ptr, bytes); }

void release(nufft_cg* s) {
    if (!s) return;
    if (s->device >= 0) {
        DeviceGuard g(s->device);
        for (void* p : {s->d_r, s->d_p, s->d_q, s->d_z, s->d_part, s->d_hist})
            if (p) (void)hipFree(p);
        s->scal.release();
    }
    delete s;
}

CgScalars scalars_at(const nufft_cg* s, void* base) {
    const int C = s->C;
    CgScalars k{};
    double* d = static_cast<double*>(base);
    k.rho = d;
    k.beta0 = d + 2 * C;
    k.res = d + 3 * C;
    k.rhoz = d + 4 * C;
    int32_t* i = reinterpret_cast<int32_t*>(d + 6 * C);
    k.flag = i;
    k.brk = i + 2 * C;
    k.iters = i + 3 * C;
    k.status = i + 4 * C;
    k.history = static_cast<double*>(s->d_hist);
    k.part1 = static_cast<double*>(s->d_part);
    k.part2 = k.part1 + (size_t)C * s->G * 2;
    return k;
}

// One kernel over all components, kCgBatch at a time.
template <typename F>
int for_batches(const nufft_cg* s, CgLaunch& a, void* const* x, const void* const* b, F&& launch) {
    for (int c0 = 0; c0 < s->C; c0 += kCgBatch) {
        a.c0 = c0;
        a.nc = std::min(kCgBatch, s->C - c0);
        for (int k = 0; k < a.nc; ++k) {
            a.x[k] = x[c0 + k];
            a.b[k] = b ? b[c0 + k] : nullptr;
        }
        hipError_t e = launch(a);
        if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a CG kernel: ") + hipGetErrorString(e));
    }
    return NUFFT_OK;
}

}  // namespace

extern "C" {

int64_t nufft_sizeof_cg_params(void) { return (int64_t)sizeof(nufft_cg_params); }
int64_t nufft_sizeof_cg_info(void) { return (int64_t)sizeof(nufft_cg_info); }

int nufft_cg_create(nufft_cg** out, nufft_toeplitz* tz, const nufft_cg_params* params) {
    if (!out || !tz || !params) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    nufft_toeplitz_info ti;
    int rc = toeplitz_info(tz, ti);
    if (rc) return rc;
    if (ti.device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only Toeplitz object (device = -1): the solver runs on the device");
    nufft_cg_params p;
    if ((rc = read_params(p, params, "nufft_cg_params"))) return rc;
    if (p.max_iter < 1) return fail(NUFFT_ERR_INVALID_ARG, "max_iter must be at least 1");
    if (p.max_iter > (1 << 24)) return fail(NUFFT_ERR_INVALID_ARG, "max_iter beyond 2^24");
    if (p.check_every < 0) return fail(NUFFT_ERR_INVALID_ARG, "check_every must not be negative");
    if (!std::isfinite(p.rtol) || p.rtol < 0) return fail(NUFFT_ERR_INVALID_ARG, "rtol must be finite and not negative");
    if (!std::isfinite(p.lambda) || p.lambda < 0) return fail(NUFFT_ERR_INVALID_ARG, "lambda must be finite and not negative");

    nufft_cg* s = new (std::nothrow) nufft_cg();
    if (!s) return fail(NUFFT_ERR_ALLOC, "out of host memory");
    s->tz = tz;
    s->dtype = ti.dtype;
    s->C = ti.ntransforms;
    s->device = ti.device;
    s->max_iter = p.max_iter;
    s->check_every = p.check_every;
    s->rtol = p.rtol;
    s->lambda = p.lambda;
    s->n = ti.N[0] * ti.N[1] * ti.N[2];
    const size_t rb = real_bytes(s->dtype), comp = padded((size_t)s->n * 2 * rb);
    s->stride = (int64_t)(comp / rb);
    s->array_bytes = 3 * (int64_t)s->C * (int64_t)comp;

    DeviceGuard guard(s->device);
    s->num_cus = device_cus(s->device);
    s->G = cg_workgroups(s->dtype, s->n, s->num_cus);
    if ((rc = alloc(s, &s->d_r, (size_t)s->C * comp)) || (rc = alloc(s, &s->d_p, (size_t)s->C * comp)) ||
        (rc = alloc(s, &s->d_q, (size_t)s->C * comp)) || (rc = alloc(s, &s->d_part, part_bytes(s))) ||
        (rc = create_outcome(s->own_bytes, "CG", s->scal, &s->d_hist, scal_bytes(s), hist_bytes(s)))) {
        const std::string keep = nufft_last_error_message();
        release(s);
        return fail(rc, keep);
    }
    for (int c = 0; c < s->C; ++c) {
        s->ptab.push_back(static_cast<char*>(s->d_p) + (size_t)c * comp);
        s->qtab.push_back(static_cast<char*>(s->d_q) + (size_t)c * comp);
        s->rtab.push_back(static_cast<char*>(s->d_r) + (size_t)c * comp);
    }
    *out = s;
    return NUFFT_OK;
}

int nufft_cg_destroy(nufft_cg* cg) {
    release(cg);
    return NUFFT_OK;
}

int nufft_cg_set_preconditioner(nufft_cg* s, nufft_precond* pc) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (!pc) {
        s->pc = nullptr;
        return NUFFT_OK;
    }
    if (nufft::precond_operator(pc) != s->tz)
        return fail(NUFFT_ERR_INVALID_ARG, "the preconditioner was created for another operator (element type, shape and ntransforms follow the operator)");
    if (!s->d_z) {
        DeviceGuard guard(s->device);
        const size_t comp = (size_t)s->stride * real_bytes(s->dtype);
        if (int rc = alloc(s, &s->d_z, (size_t)s->C * comp)) return rc;
        for (int c = 0; c < s->C; ++c) s->ztab.push_back(static_cast<char*>(s->d_z) + (size_t)c * comp);
        s->array_bytes += (int64_t)s->C * (int64_t)comp;
    }
    s->pc = pc;
    return NUFFT_OK;
}

int nufft_cg_get_info(const nufft_cg* s, nufft_cg_info* o) {
    if (!s || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    nufft_cg_info i;
    std::memset(&i, 0, sizeof(i));
    i.ntransforms = s->C;
    i.dtype = s->dtype;
    i.max_iter = s->max_iter;
    i.check_every = s->check_every;
    i.workgroups = s->G;
    i.iterations_enqueued = s->enqueued;
    i.rtol = s->rtol;
    i.lambda = s->lambda;
    i.array_bytes = s->array_bytes;
    i.workspace_bytes = s->own_bytes;
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_cg_solve(nufft_cg* s, void* const* x, const void* const* b, int use_x0, void* stream_) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    DeviceGuard guard(s->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc = check_solve_args(s->tz, "nufft_cg_solve", s->C, s->n, s->dtype, x, b, s->check_every, stream);
    if (rc) return rc;

    CgLaunch a{};
    a.dtype = s->dtype;
    a.C = s->C;
    a.G = s->G;
    a.n = s->n;
    a.stride = s->stride;
    a.r = s->d_r;
    a.p = s->d_p;
    a.q = s->d_q;
    a.lambda = s->lambda;
    a.rtol = s->rtol;
    a.max_iter = s->max_iter;
    a.it = 0;
    a.joint = nufft_toeplitz_num_coupled(s->tz) > 0 ? 1 : 0;      // coupled components are one system: one α, one β, one done flag
    a.s = scalars_at(s, s->scal.dev);
    if (s->pc) {
        // a coupled operator takes the block preconditioner created for its K, independent components the scalar one
        const int K = nufft_toeplitz_num_coupled(s->tz);
        if (nufft_precond_num_coupled(s->pc) != K)
            return fail(NUFFT_ERR_UNSUPPORTED, K > 0 ? "the operator couples its components: the preconditioner must be a block preconditioner created for this coupling "
                                                       "(nufft_precond_create_block; clear the one set with nufft_cg_set_preconditioner(cg, NULL))"
                                                     : "the block preconditioner was created for a coupled operator, and the operator no longer couples its components "
                                                       "(clear it with nufft_cg_set_preconditioner(cg, NULL))");
        a.z = s->d_z;
    }

    s->enqueued = 0;
    const bool warm = use_x0 != 0;
    if (warm && (rc = nufft_toeplitz_apply(s->tz, s->qtab.data(), x, stream))) return rc;      // q = G x0
    if ((rc = for_batches(s, a, x, b, [&](const CgLaunch& l) { return launch_cg_residual(l, warm, stream); }))) return rc;
    if ((rc = for_batches(s, a, x, b, [&](const CgLaunch& l) { return launch_cg_start(l, stream); }))) return rc;
    const CgScalars host = scalars_at(s, s->scal.host);
    // z = M⁻¹ r, the partials of Re<r, z> (the dot kernel with p = r, q = z) and the direction kernel: the tail of a preconditioned
    // iteration, and with it = 0 the start of the solve
    auto precondition = [&]() -> int {
        int prc = nufft_precond_apply(s->pc, s->ztab.data(), s->rtab.data(), stream);
        if (prc) return prc;
        CgLaunch d = a;
        d.p = s->d_r;
        d.q = s->d_z;
        if ((prc = for_batches(s, d, x, nullptr, [&](const CgLaunch& l) { return launch_cg_dot(l, stream); }))) return prc;
        return for_batches(s, a, x, nullptr, [&](const CgLaunch& l) { return launch_pcg_direction(l, stream); });
    };
    if (s->pc && (rc = precondition())) return rc;
    for (int it = 1; it <= s->max_iter; ++it) {
        a.it = it;
        if ((rc = nufft_toeplitz_apply(s->tz, s->qtab.data(), s->ptab.data(), stream))) return rc;
        if ((rc = for_batches(s, a, x, nullptr, [&](const CgLaunch& l) { return launch_cg_dot(l, stream); }))) return rc;
        if (s->pc) {
            if ((rc = for_batches(s, a, x, nullptr, [&](const CgLaunch& l) { return launch_pcg_update(l, stream); }))) return rc;
            if ((rc = precondition())) return rc;
        } else {
            if ((rc = for_batches(s, a, x, nullptr, [&](const CgLaunch& l) { return launch_cg_update(l, stream); }))) return rc;
            if ((rc = for_batches(s, a, x, nullptr, [&](const CgLaunch& l) { return launch_cg_direction(l, stream); }))) return rc;
        }
        s->enqueued = it;
        if (s->check_every > 0 && it % s->check_every == 0 && it < s->max_iter) {
            bool all;
            if ((rc = all_done(s->scal, stream, host.flag + ((it + 1) & 1) * s->C, s->C, &all))) return rc;
            if (all) break;
        }
    }
    return NUFFT_OK;
}

int nufft_cg_get_result(nufft_cg* s, int32_t* iterations, int32_t* status, double* residual, int64_t capacity, void* stream_) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (capacity < s->C) return fail(NUFFT_ERR_INVALID_ARG, "capacity is smaller than ntransforms");
    DeviceGuard guard(s->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc;
    if ((rc = refuse_capture("nufft_cg_get_result", stream)) || (rc = s->scal.fetch(stream))) return rc;
    const CgScalars host = scalars_at(s, s->scal.host);
    for (int c = 0; c < s->C; ++c) {
        if (iterations) iterations[c] = host.iters[c];
        if (status) status[c] = host.status[c];
        if (residual) residual[c] = host.res[c];
    }
    return NUFFT_OK;
}

int nufft_cg_history(nufft_cg* s, double* host_out, int64_t capacity, void* stream_) {
    if (!s || !host_out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (capacity < (int64_t)(s->max_iter + 1) * s->C) return fail(NUFFT_ERR_INVALID_ARG, "capacity is smaller than (max_iter + 1) * ntransforms");
    DeviceGuard guard(s->device);
    return fetch_history("nufft_cg_history", host_out, s->d_hist, hist_bytes(s), static_cast<hipStream_t>(stream_));
}

}  // extern "C"
