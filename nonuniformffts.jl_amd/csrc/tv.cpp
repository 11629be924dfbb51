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
//
// With the temporal term (nufft_tvpd_create_temporal) the objective gains tv_t ‖∇_t x‖₁, the difference along the
// components, and the solver one more dual array z_c per component.  Without the spatial term the two kernels of tvt_kernels.hip are the
// whole iteration (x⁺ = x − τ (q + μ x − b + ∇_tᴴz), then z <- P_{tv_t}(z + σ ∇_t x̄)) and y does not exist.  With it, one launch adds ∇_tᴴz
// to q = G x, the spatial kernels run as they are (on q + ∇_tᴴz in place of q: the same x⁺), and the temporal dual kernel follows.  The
// decision is always joint.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "solver_common.h"
#include "stream_kernels.h"
#include "tgv.h"
#include "tv.h"

using namespace nufft;

struct nufft_tv {
    int dtype = NUFFT_F64, D = 1, C = 1, device = -1, wide = 0;
    int64_t N[3] = {1, 1, 1};
    int64_t n = 1, G = 1;
    int tile[3] = {1, 1, 1}, tiles[3] = {1, 1, 1};
    void* d_part = nullptr;               // double[C][G]
    int64_t own_bytes = 0;
    // the difference along the components: flat over the n cells of a frame (tvt_kernels.hip)
    int wide_t = 0;                       // two ComplexF32 per lane: n is even
    int64_t Gt = 1;                       // workgroups per frame
    void* d_part_t = nullptr;             // double[C][Gt], allocated by the first nufft_tv_norm_t
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
    // the temporal term (nufft_tvpd_create_temporal); without it nd = D and d_y holds [C][D] arrays as ever
    bool temporal = false;
    int periodic = 0, spatial = 1;
    int nd = 1;                           // arrays per component in d_y: y_1 ... y_D (spatial term on), then z
    double tv_t = 0.0;
    void* d_part_t = nullptr;             // double[C][Gt] of the temporal dual kernel
};

namespace {

void release(nufft_tv* t) {
    if (!t) return;
    if (t->device >= 0) {
        DeviceGuard g(t->device);
        if (t->d_part) (void)hipFree(t->d_part);
        if (t->d_part_t) (void)hipFree(t->d_part_t);
    }
    delete t;
}

void release(nufft_tvpd* s) {
    if (!s) return;
    release(s->tv);
    if (s->device >= 0) {
        DeviceGuard g(s->device);
        for (void* p : {s->d_q, s->d_y, s->d_part, s->d_hist, s->d_part_t})
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
    t->wide_t = f32 && t->n % 2 == 0 ? 1 : 0;
    t->Gt = (t->n / (t->wide_t ? 2 : 1) + (int64_t)stream::kThreads * kTvtPacks - 1) / ((int64_t)stream::kThreads * kTvtPacks);
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

// One launch of a symmetrised-gradient kernel (tgv_kernels.hip) per batch of components: the D arrays v[c · D + d] and the
// S = D (D + 1) / 2 arrays r[c · S + s]
int run_sym_operator(nufft_tv* t, TgvMode mode, void* const* v, void* const* r, hipStream_t stream) {
    TgvLaunch a{};
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
    const int B = batch_of(t), S = tgv_sym(t->D);
    for (int c0 = 0; c0 < t->C; c0 += B) {
        a.c0 = c0;
        a.nc = std::min(B, t->C - c0);
        for (int k = 0; k < a.nc; ++k) {
            for (int d = 0; d < t->D; ++d) a.v[k][d] = v[(size_t)(c0 + k) * t->D + d];
            for (int e = 0; e < S; ++e) a.r[k][e] = r ? r[(size_t)(c0 + k) * S + e] : nullptr;
        }
        hipError_t e = launch_tgv(a, mode, stream);
        if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a symmetrised-gradient kernel: ") + hipGetErrorString(e));
    }
    return NUFFT_OK;
}

TvtLaunch launch_template_t(const nufft_tv* t) {
    TvtLaunch a{};
    a.dtype = t->dtype;
    a.wide = t->wide_t;
    a.C = t->C;
    a.n = t->n;
    a.G = t->Gt;
    return a;
}

// Frame c of the axis: itself inside 0 ... C − 1, the other end on a periodic axis, −1 (no such frame) otherwise.
int frame_of(int c, int C, int periodic) {
    if (c >= 0 && c < C) return c;
    if (!periodic) return -1;
    return c < 0 ? C - 1 : 0;
}

// The slots of one batch (slot j: frame c0 + j − 1).  `zero_last`: the table is the z a ∇_tᴴ reads, whose last frame is zero by
// definition on the non-periodic axis.
template <typename Ptr>
void fill_slots(Ptr* slots, int c0, int nc, int C, int periodic, bool zero_last, const std::function<Ptr(int)>& at) {
    for (int j = 0; j < nc + 2; ++j) {
        const int c = frame_of(c0 + j - 1, C, periodic);
        slots[j] = c < 0 || (zero_last && !periodic && c == C - 1) ? nullptr : at(c);
    }
}

// One temporal operator launch per batch of components
int run_operator_t(nufft_tv* t, TvtMode mode, void* const* x, void* const* z, int periodic, hipStream_t stream) {
    TvtLaunch a = launch_template_t(t);
    a.part = static_cast<double*>(t->d_part_t);
    for (int c0 = 0; c0 < t->C; c0 += kTvBatch) {
        a.c0 = c0;
        a.nc = std::min(kTvBatch, t->C - c0);
        fill_slots<void*>(a.x, c0, a.nc, t->C, periodic, false, [&](int c) { return x[c]; });
        if (z) fill_slots<void*>(a.z, c0, a.nc, t->C, periodic, mode == TVT_ADJOINT, [&](int c) { return z[c]; });
        hipError_t e = launch_tvt(a, mode, stream);
        if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a total-variation kernel: ") + hipGetErrorString(e));
    }
    return NUFFT_OK;
}

int check_temporal(const nufft_tv* t, int periodic) {
    if (t->C < 2) return fail(NUFFT_ERR_INVALID_ARG, "the difference along the components needs ntransforms >= 2");
    if (periodic != 0 && periodic != 1) return fail(NUFFT_ERR_INVALID_ARG, "periodic must be 0 or 1");
    return NUFFT_OK;
}

size_t hist_bytes(const nufft_tvpd* s) { return (size_t)s->max_iter * s->C * 2 * sizeof(double); }

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

int nufft_tv_sym_gradient(nufft_tv* t, void* const* r_out, const void* const* v, void* stream) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    const int S = tgv_sym(t->D);
    int rc;
    if ((rc = check_table(r_out, t->C * S)) || (rc = check_table(v, t->C * t->D)) || (rc = check_overlap(t, r_out, t->C * S, v, t->C * t->D))) return rc;
    DeviceGuard guard(t->device);
    return run_sym_operator(t, TGV_SYM_GRADIENT, const_cast<void* const*>(v), r_out, static_cast<hipStream_t>(stream));
}

int nufft_tv_sym_adjoint(nufft_tv* t, void* const* v_out, const void* const* r, void* stream) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    const int S = tgv_sym(t->D);
    int rc;
    if ((rc = check_table(v_out, t->C * t->D)) || (rc = check_table(r, t->C * S)) || (rc = check_overlap(t, v_out, t->C * t->D, r, t->C * S))) return rc;
    DeviceGuard guard(t->device);
    return run_sym_operator(t, TGV_SYM_ADJOINT, v_out, const_cast<void* const*>(r), static_cast<hipStream_t>(stream));
}

int nufft_tv_sym_norm(nufft_tv* t, const void* const* v, double* sums_out_device, void* stream) {
    if (!t || !sums_out_device) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (int rc = check_table(v, t->C * t->D)) return rc;
    DeviceGuard guard(t->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = run_sym_operator(t, TGV_SYM_NORM, const_cast<void* const*>(v), nullptr, s)) return rc;
    hipError_t e = launch_tv_sum(static_cast<const double*>(t->d_part), t->G, t->C, sums_out_device, s);
    if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a total-variation kernel: ") + hipGetErrorString(e));
    return NUFFT_OK;
}

int nufft_tv_gradient_t(nufft_tv* t, void* const* z_out, const void* const* x, int periodic, void* stream) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = check_temporal(t, periodic)) || (rc = check_table(z_out, t->C)) || (rc = check_table(x, t->C)) || (rc = check_overlap(t, z_out, t->C, x, t->C)))
        return rc;
    DeviceGuard guard(t->device);
    return run_operator_t(t, TVT_GRADIENT, const_cast<void* const*>(x), z_out, periodic, static_cast<hipStream_t>(stream));
}

int nufft_tv_adjoint_t(nufft_tv* t, void* const* x_out, const void* const* z, int periodic, void* stream) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = check_temporal(t, periodic)) || (rc = check_table(x_out, t->C)) || (rc = check_table(z, t->C)) || (rc = check_overlap(t, x_out, t->C, z, t->C)))
        return rc;
    DeviceGuard guard(t->device);
    return run_operator_t(t, TVT_ADJOINT, x_out, const_cast<void* const*>(z), periodic, static_cast<hipStream_t>(stream));
}

int nufft_tv_norm_t(nufft_tv* t, const void* const* x, int periodic, double* sums_out_device, void* stream) {
    if (!t || !sums_out_device) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = check_temporal(t, periodic)) || (rc = check_table(x, t->C))) return rc;
    DeviceGuard guard(t->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!t->d_part_t) {
        if (capturing(s)) return fail(NUFFT_ERR_INVALID_ARG, "the first nufft_tv_norm_t allocates the partial sums: not on a capturing stream");
        if ((rc = alloc_buffer(t->own_bytes, "total-variation", &t->d_part_t, (size_t)t->C * t->Gt * sizeof(double)))) return rc;
    }
    if ((rc = run_operator_t(t, TVT_NORM, const_cast<void* const*>(x), nullptr, periodic, s))) return rc;
    hipError_t e = launch_tv_sum(static_cast<const double*>(t->d_part_t), t->Gt, t->C, sums_out_device, s);
    if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a total-variation kernel: ") + hipGetErrorString(e));
    return NUFFT_OK;
}

}  // extern "C"

namespace {

// nufft_tvpd_create (tp = null) and nufft_tvpd_create_temporal
int create_solver(nufft_tvpd** out, nufft_toeplitz* tz, const nufft_tvpd_params* params, const nufft_tvt_params* tparams) {
    nufft_toeplitz_info ti;
    int rc = toeplitz_info(tz, ti);
    if (rc) return rc;
    nufft_tvt_params tp;
    std::memset(&tp, 0, sizeof(tp));
    tp.spatial = 1;
    if (tparams) {
        if ((rc = read_params(tp, tparams, "nufft_tvt_params"))) return rc;
        if (ti.ntransforms < 2) return fail(NUFFT_ERR_INVALID_ARG, "the temporal term needs ntransforms >= 2 (the frames are the components)");
        if (!weight_ok(tp.tv_t)) return fail(NUFFT_ERR_INVALID_ARG, "tv_t must be finite and not negative");
        if ((tp.spatial != 0 && tp.spatial != 1) || (tp.periodic != 0 && tp.periodic != 1))
            return fail(NUFFT_ERR_INVALID_ARG, "spatial and periodic must be 0 or 1");
    }
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
    s->temporal = tparams != nullptr;
    s->periodic = tp.periodic;
    s->spatial = tp.spatial;
    s->tv_t = tp.tv_t;
    s->nd = s->temporal ? (s->spatial ? s->D : 0) + 1 : s->D;
    const int differences = s->temporal ? s->nd : s->D;      // ‖[∇; ∇_t]‖² <= 4 (D + 1), ‖∇_t‖² <= 4, ‖∇‖² <= 4 D
    s->sigma = p.sigma > 0.0 ? p.sigma : 1.0 / (8.0 * differences * p.step);
    s->lambda = p.lambda;
    s->weight.assign(s->C, s->spatial ? p.tv : 0.0);
    s->n = s->tv->n;
    const size_t rb = real_bytes(s->dtype), comp = padded((size_t)s->n * 2 * rb);
    s->stride = (int64_t)(comp / rb);
    s->array_bytes = (int64_t)(1 + s->nd) * s->C * (int64_t)comp;
    if (s->temporal && s->tv->Gt > (int64_t)INT_MAX / s->C) {
        release(s);
        return fail(NUFFT_ERR_UNSUPPORTED, std::to_string(s->tv->Gt) + " workgroups for each of " + std::to_string(s->C) + " frames: more than 2^31 - 1 rows of partial sums");
    }

    DeviceGuard guard(s->device);
    s->G0 = stream::stream_workgroups((int64_t)(comp / 16), device_cus(s->device));
    auto alloc = [&](void** ptr, size_t bytes) { return alloc_buffer(s->own_bytes, "TV solver", ptr, bytes); };
    const int64_t primal_rows = s->temporal && !s->spatial ? s->tv->Gt : s->tv->G;      // of the kernel that forms x⁺
    if ((rc = alloc(&s->d_q, (size_t)s->C * comp)) || (rc = alloc(&s->d_y, (size_t)s->C * s->nd * comp)) ||
        (rc = alloc(&s->d_part, (size_t)s->C * primal_rows * 2 * sizeof(double))) ||
        (s->temporal && (rc = alloc(&s->d_part_t, (size_t)s->C * s->tv->Gt * sizeof(double)))) ||
        (rc = create_outcome(s->own_bytes, "TV solver", s->scal, &s->d_hist, prox_scal_bytes(s->C), hist_bytes(s)))) {
        const std::string keep = nufft_last_error_message();
        release(s);
        return fail(rc, keep);
    }
    for (int c = 0; c < s->C; ++c) s->qtab.push_back(static_cast<char*>(s->d_q) + (size_t)c * comp);
    *out = s;
    return NUFFT_OK;
}

}  // namespace

extern "C" {

int64_t nufft_sizeof_tvt_params(void) { return (int64_t)sizeof(nufft_tvt_params); }

int nufft_tvpd_create(nufft_tvpd** out, nufft_toeplitz* tz, const nufft_tvpd_params* params) {
    if (!out || !tz || !params) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    return create_solver(out, tz, params, nullptr);
}

int nufft_tvpd_create_temporal(nufft_tvpd** out, nufft_toeplitz* tz, const nufft_tvpd_params* params, const nufft_tvt_params* temporal) {
    if (!out || !tz || !params || !temporal) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    return create_solver(out, tz, params, temporal);
}

int nufft_tvpd_set_tv_t(nufft_tvpd* s, double tv_t) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (!s->temporal) return fail(NUFFT_ERR_INVALID_ARG, "the solver has no temporal term (nufft_tvpd_create_temporal makes one)");
    if (!weight_ok(tv_t)) return fail(NUFFT_ERR_INVALID_ARG, "tv_t must be finite and not negative");
    s->tv_t = tv_t;
    return NUFFT_OK;
}

int nufft_tvpd_get_temporal(const nufft_tvpd* s, nufft_tvt_params* o) {
    if (!s || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (!s->temporal) return fail(NUFFT_ERR_INVALID_ARG, "the solver has no temporal term (nufft_tvpd_create_temporal makes one)");
    nufft_tvt_params i;
    std::memset(&i, 0, sizeof(i));
    i.periodic = s->periodic;
    i.spatial = s->spatial;
    i.tv_t = s->tv_t;
    write_info(o, i);
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
    for (int c = 0; c < s->C && !s->spatial; ++c)
        if (weights[c] != 0.0) return fail(NUFFT_ERR_INVALID_ARG, "the solver was created without the spatial term (spatial = 0): tv must be 0");
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
    DeviceGuard guard(s->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int rc = check_solve_args(s->tz, "nufft_tvpd_solve", s->C, s->n, s->dtype, x, b, s->check_every, stream);
    if (rc) return rc;

    const size_t rb = real_bytes(s->dtype), comp = (size_t)s->stride * rb;
    TvSolve h{};
    h.dtype = s->dtype;
    h.C = s->C;
    h.G = s->G0;
    h.n = s->n;
    h.ystride = s->stride * s->nd;
    h.y = s->d_y;
    h.max_iter = s->max_iter;
    h.joint = nufft_toeplitz_num_coupled(s->tz) > 0 ? 1 : 0;
    h.tol = s->tol;
    h.part_p = static_cast<const double*>(s->d_part);
    h.part_d = static_cast<const double*>(s->tv->d_part);
    h.P = s->tv->G;
    h.s = prox_scalars_at(s->scal.dev, s->C, s->d_hist);
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
                for (int d = 0; d < s->D && s->spatial; ++d) a.y[k][d] = static_cast<char*>(s->d_y) + ((size_t)c * s->nd + d) * comp;
                a.tv[k] = s->weight[c];
            }
            hipError_t e = launch();
            if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a TV solver kernel: ") + hipGetErrorString(e));
        }
        return NUFFT_OK;
    };

    // the temporal term: z_c is the last of component c's arrays in d_y; one launch per batch of kTvBatch frames
    TvtLaunch ta = launch_template_t(s->tv);
    ta.tv_t = s->tv_t;
    ta.step = s->step;
    ta.sigma = s->sigma;
    ta.lambda = s->lambda;
    ta.flag = h.s.flag;
    auto for_frames = [&](TvtMode mode) -> int {
        const bool reads_z = mode != TVT_DUAL;      // ∇_tᴴz: the last frame's z is zero by definition on the non-periodic axis
        for (int c0 = 0; c0 < s->C; c0 += kTvBatch) {
            ta.c0 = c0;
            ta.nc = std::min(kTvBatch, s->C - c0);
            fill_slots<void*>(ta.x, c0, ta.nc, s->C, s->periodic, false, [&](int c) { return x[c]; });
            fill_slots<void*>(ta.q, c0, ta.nc, s->C, s->periodic, false, [&](int c) { return s->qtab[c]; });
            fill_slots<void*>(ta.z, c0, ta.nc, s->C, s->periodic, reads_z,
                              [&](int c) { return static_cast<void*>(static_cast<char*>(s->d_y) + ((size_t)c * s->nd + s->nd - 1) * comp); });
            for (int k = 0; k < ta.nc; ++k) ta.b[k] = b[c0 + k];
            hipError_t e = launch_tvt(ta, mode, stream);
            if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a TV solver kernel: ") + hipGetErrorString(e));
        }
        return NUFFT_OK;
    };
    TvtDecide td{};
    td.C = s->C;
    td.tol = s->tol;
    td.tv_t = s->tv_t;
    td.part_p = static_cast<const double*>(s->d_part);
    td.part_s = s->spatial ? static_cast<const double*>(s->tv->d_part) : nullptr;
    td.part_t = static_cast<const double*>(s->d_part_t);
    td.Pp = s->spatial ? s->tv->G : s->tv->Gt;
    td.Ps = s->tv->G;
    td.Pt = s->tv->Gt;
    td.s = h.s;
    auto decide_frames = [&](int it) -> int {
        td.it = it;
        for (int c0 = 0; c0 < s->C; c0 += kTvBatch) {
            td.c0 = c0;
            td.nc = std::min(kTvBatch, s->C - c0);
            for (int k = 0; k < td.nc; ++k) td.tv[k] = s->weight[c0 + k];
            hipError_t e = launch_tvt_decide(td, stream);
            if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a TV solver kernel: ") + hipGetErrorString(e));
        }
        return NUFFT_OK;
    };

    s->enqueued = 0;
    const bool warm = use_x0 != 0;
    if ((rc = for_batches([&]() { return launch_tv_start(h, warm, stream); }))) return rc;
    const ProxScalars host = prox_scalars_at(s->scal.host, s->C, nullptr);
    for (int it = 1; it <= s->max_iter; ++it) {
        h.it = it;
        if ((rc = nufft_toeplitz_apply(s->tz, s->qtab.data(), const_cast<const void* const*>(x), stream))) return rc;      // q = G x
        if (s->temporal && !s->spatial) {
            ta.part = static_cast<double*>(s->d_part);
            if ((rc = for_frames(TVT_PRIMAL))) return rc;
        } else {
            if (s->temporal && (rc = for_frames(TVT_ADD))) return rc;      // q <- q + ∇_tᴴz
            a.part = static_cast<double*>(s->d_part);
            if ((rc = for_batches([&]() { return launch_tv(a, TV_PRIMAL, stream); }))) return rc;
            a.part = static_cast<double*>(s->tv->d_part);
            if ((rc = for_batches([&]() { return launch_tv(a, TV_DUAL, stream); }))) return rc;
        }
        if (s->temporal) {
            ta.part = static_cast<double*>(s->d_part_t);
            if ((rc = for_frames(TVT_DUAL)) || (rc = decide_frames(it))) return rc;
        } else if ((rc = for_batches([&]() { return launch_tv_decide(h, stream); }))) return rc;
        s->enqueued = it;
        if (s->check_every > 0 && it % s->check_every == 0 && it < s->max_iter) {
            bool all;
            if ((rc = all_done(s->scal, stream, host.flag, s->C, &all))) return rc;
            if (all) break;
        }
    }
    return NUFFT_OK;
}

int nufft_tvpd_get_result(nufft_tvpd* s, int32_t* iterations, int32_t* status, double* change, int64_t capacity, void* stream_) {
    if (!s) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (capacity < s->C) return fail(NUFFT_ERR_INVALID_ARG, "capacity is smaller than ntransforms");
    DeviceGuard guard(s->device);
    return copy_result("nufft_tvpd_get_result", s->scal, s->C, s->C, 1, iterations, status, change, static_cast<hipStream_t>(stream_));
}

int nufft_tvpd_history(nufft_tvpd* s, double* host_out, int64_t capacity, void* stream_) {
    if (!s || !host_out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (capacity < (int64_t)s->max_iter * s->C * 2) return fail(NUFFT_ERR_INVALID_ARG, "capacity is smaller than max_iter * ntransforms * 2");
    DeviceGuard guard(s->device);
    return fetch_history("nufft_tvpd_history", host_out, s->d_hist, hist_bytes(s), static_cast<hipStream_t>(stream_));
}

}  // extern "C"
