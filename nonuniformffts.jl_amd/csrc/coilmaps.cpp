// Coil sensitivity maps from coil images (include/nufft_mi355x.h, coil map section).
//
// The host side only enqueues: the main kernel, the one-workgroup maximum and, with crop > 0, the streaming crop pass
// (coilmaps_kernels.hip).  The object owns the per-workgroup partials, two words and, with crop > 0, an array for λ1 that is used when
// the caller passes none.  The coil pointers and the phase reference travel as kernel arguments: no device table is written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "coilmaps.h"
#include "host_common.h"
#include "jacobi.h"

using namespace nufft;

struct nufft_coilmaps {
    int dtype = NUFFT_F64, D = 1, C = 1, device = -1, num_cus = 256;
    int box[3] = {1, 1, 1};
    double crop = 0.0;
    int64_t N[3] = {1, 1, 1};
    int64_t n = 1;
    CoilmapsLayout L{};
    void* d_part = nullptr;      // double[G]
    void* d_sweeps = nullptr;    // int32[G]
    void* d_words = nullptr;     // double max λ1; int32 max sweeps
    void* d_lambda1 = nullptr;   // real T [n], crop > 0 only
    int64_t own_bytes = 0;
};

namespace {

void release(nufft_coilmaps* h) {
    if (!h) return;
    if (h->device >= 0) {
        DeviceGuard guard(h->device);
        for (void* p : {h->d_part, h->d_sweeps, h->d_words, h->d_lambda1})
            if (p) (void)hipFree(p);
    }
    delete h;
}

// The argument checks of a create call, in the documented order, and the geometry they lead to; no device is touched.
int describe(nufft_coilmaps& g, int dtype, int D, const int64_t* N, int C, const nufft_coilmaps_params* params) {
    nufft_coilmaps_params p;
    if (int rc = read_params(p, params, "nufft_coilmaps_params")) return rc;
    if (dtype != NUFFT_F32 && dtype != NUFFT_F64) return fail(NUFFT_ERR_INVALID_ARG, "dtype must be NUFFT_F32 or NUFFT_F64");
    if (D < 1 || D > 3) return fail(NUFFT_ERR_INVALID_ARG, "1, 2 or 3 dimensions");
    for (int d = 0; d < D; ++d)
        if (N[d] < 1) return fail(NUFFT_ERR_INVALID_ARG, "N[" + std::to_string(d) + "] must be positive");
    if (C < 1) return fail(NUFFT_ERR_INVALID_ARG, "ncoils = " + std::to_string(C) + " must be at least 1");
    for (int d = 0; d < 3; ++d) {
        const int b = p.box[d];
        if (d >= D) {
            if (b != 1 && b != 0) return fail(NUFFT_ERR_INVALID_ARG, "box[" + std::to_string(d) + "] must be 1 beyond the dimensions of the arrays");
            p.box[d] = 1;
            continue;
        }
        if (b < 1 || b % 2 == 0) return fail(NUFFT_ERR_INVALID_ARG, "box[" + std::to_string(d) + "] = " + std::to_string(b) + " must be odd and positive");
    }
    if (!(p.crop >= 0.0) || !std::isfinite(p.crop)) return fail(NUFFT_ERR_INVALID_ARG, "crop must be finite and not negative");
    if (C > kCmMaxCoils)
        return fail(NUFFT_ERR_UNSUPPORTED, std::to_string(C) + " coils: more than the " + std::to_string(kCmMaxCoils) + " lanes of a one-wave Jacobi team");
    for (int d = 0; d < D; ++d) {
        if (p.box[d] > kCmMaxBox || p.box[d] > N[d])
            return fail(NUFFT_ERR_UNSUPPORTED, "box[" + std::to_string(d) + "] = " + std::to_string(p.box[d]) + " exceeds " + std::to_string(kCmMaxBox) +
                                                   " or N[" + std::to_string(d) + "] = " + std::to_string(N[d]));
        if (N[d] > ((int64_t)1 << 30)) return fail(NUFFT_ERR_UNSUPPORTED, "more than 2^30 cells per axis");
    }
    const CoilmapsLayout L = coilmaps_layout(dtype == NUFFT_F32, C, D, p.box, N);
    if (L.G > INT_MAX) return fail(NUFFT_ERR_UNSUPPORTED, "more than 2^31 - 1 tiles");
    g.dtype = dtype;
    g.D = D;
    g.C = C;
    g.crop = p.crop;
    g.L = L;
    g.n = 1;
    for (int d = 0; d < 3; ++d) {
        g.box[d] = p.box[d];
        g.N[d] = d < D ? N[d] : 1;
        g.n *= g.N[d];
    }
    return NUFFT_OK;
}

// what create allocates on the device: the partials, the words and, with crop > 0, n reals
int64_t device_bytes(const nufft_coilmaps& g) {
    int64_t b = (int64_t)(padded((size_t)g.L.G * sizeof(double)) + padded((size_t)g.L.G * sizeof(int32_t)) + padded(16));
    if (g.crop > 0.0) b += (int64_t)padded((size_t)g.n * real_bytes(g.dtype));
    return b;
}

void describe_info(const nufft_coilmaps& g, nufft_coilmaps_info& i) {
    std::memset(&i, 0, sizeof(i));
    i.ndim = g.D;
    i.dtype = g.dtype;
    i.ncoils = g.C;
    i.device = g.device;
    for (int d = 0; d < 3; ++d) {
        i.box[d] = g.box[d];
        i.tile[d] = g.L.tile[d];
        i.N[d] = g.N[d];
    }
    i.tile_cells = g.L.tcells;
    i.team_lanes = g.L.TW;
    i.teams = g.L.teams;
    i.staged = g.L.staged;
    i.lds_bytes = (int32_t)g.L.bytes;
    i.jacobi_sweeps_max = jacobi_team::kSweepsMax;
    i.crop = g.crop;
    i.cells = g.n;
    i.workgroups = g.L.G;
    i.workspace_bytes = g.device >= 0 ? g.own_bytes : device_bytes(g);
}

int geometry(nufft_coilmaps** out, int dtype, int D, const int64_t* N, int C, int device, const nufft_coilmaps_params* params) {
    nufft_coilmaps g;
    if (int rc = describe(g, dtype, D, N, C, params)) return rc;
    if (device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only plan (device = -1): the coil map estimate runs on the device");
    nufft_coilmaps* h = new (std::nothrow) nufft_coilmaps(g);
    if (!h) return fail(NUFFT_ERR_ALLOC, "out of host memory");
    h->device = device;
    const CoilmapsLayout& L = h->L;
    DeviceGuard guard(device);
    if (hipDeviceGetAttribute(&h->num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
        (void)hipGetLastError();
        h->num_cus = 256;
    }
    if (hipError_t e = coilmaps_allow_lds(); e != hipSuccess) {
        (void)hipGetLastError();
        delete h;
        return fail(NUFFT_ERR_HIP, std::string("hipFuncSetAttribute of the coil map kernels: ") + hipGetErrorString(e));
    }
    int rc;
    if ((rc = alloc_buffer(h->own_bytes, "coil map", &h->d_part, (size_t)L.G * sizeof(double))) ||
        (rc = alloc_buffer(h->own_bytes, "coil map", &h->d_sweeps, (size_t)L.G * sizeof(int32_t))) ||
        (rc = alloc_buffer(h->own_bytes, "coil map", &h->d_words, 16)) ||
        (h->crop > 0.0 && (rc = alloc_buffer(h->own_bytes, "coil map", &h->d_lambda1, (size_t)h->n * real_bytes(dtype))))) {
        const std::string keep = nufft_last_error_message();
        release(h);
        return fail(rc, keep);
    }
    if (hipMemset(h->d_words, 0, 16) != hipSuccess) {
        (void)hipGetLastError();
        release(h);
        return fail(NUFFT_ERR_HIP, "hipMemset of the coil map words");
    }
    *out = h;
    return NUFFT_OK;
}

}  // namespace

extern "C" {

int64_t nufft_sizeof_coilmaps_params(void) { return (int64_t)sizeof(nufft_coilmaps_params); }
int64_t nufft_sizeof_coilmaps_info(void) { return (int64_t)sizeof(nufft_coilmaps_info); }

int nufft_coilmaps_create(nufft_coilmaps** out, int dtype, int ndim, const int64_t* N, int32_t ncoils, int device, const nufft_coilmaps_params* params) {
    if (!out || !N || !params) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    return geometry(out, dtype, ndim, N, ncoils, device, params);
}

int nufft_coilmaps_create_for_operator(nufft_coilmaps** out, const nufft_toeplitz* tz, int32_t ncoils, const nufft_coilmaps_params* params) {
    if (!out || !tz || !params) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    nufft_toeplitz_info ti;
    std::memset(&ti, 0, sizeof(ti));
    ti.struct_size = (int32_t)sizeof(ti);
    if (int rc = nufft_toeplitz_get_info(tz, &ti)) return rc;
    return geometry(out, ti.dtype, ti.ndim, ti.N, ncoils, ti.device, params);
}

int nufft_coilmaps_layout(int dtype, int ndim, const int64_t* N, int32_t ncoils, const nufft_coilmaps_params* params, nufft_coilmaps_info* o) {
    if (!N || !params || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    nufft_coilmaps g;
    if (int rc = describe(g, dtype, ndim, N, ncoils, params)) return rc;
    nufft_coilmaps_info i;
    describe_info(g, i);
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_coilmaps_destroy(nufft_coilmaps* h) {
    release(h);
    return NUFFT_OK;
}

int nufft_coilmaps_get_info(const nufft_coilmaps* h, nufft_coilmaps_info* o) {
    if (!h || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    nufft_coilmaps_info i;
    describe_info(*h, i);
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_coilmaps_estimate(nufft_coilmaps* h, void* const* maps_out, const void* const* images_in, const double* phase_ref, void* lambda1, void* lambda2,
                            void* stream_) {
    if (!h || !maps_out || !images_in) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    const int C = h->C;
    for (int c = 0; c < C && phase_ref; ++c)
        if (!std::isfinite(phase_ref[2 * c]) || !std::isfinite(phase_ref[2 * c + 1])) return fail(NUFFT_ERR_INVALID_ARG, "phase_ref must be finite");
    const size_t bytes = (size_t)h->n * 2 * real_bytes(h->dtype), lbytes = (size_t)h->n * real_bytes(h->dtype);
    for (int c = 0; c < C; ++c) {
        if (!maps_out[c] || !images_in[c]) return fail(NUFFT_ERR_INVALID_ARG, "null data vector");
        if (((uintptr_t)maps_out[c] | (uintptr_t)images_in[c]) & 15) return fail(NUFFT_ERR_INVALID_ARG, "the arrays must be 16-byte aligned");
    }
    if ((((uintptr_t)lambda1 | (uintptr_t)lambda2) & (real_bytes(h->dtype) - 1)) != 0) return fail(NUFFT_ERR_INVALID_ARG, "lambda1 / lambda2 are not aligned");
    // every output, the eigenvalue arrays included, against every other output and every input: neighbours are read
    const void* outs[kCmMaxCoils + 2];
    size_t sizes[kCmMaxCoils + 2];
    int no = 0;
    for (int c = 0; c < C; ++c) {
        outs[no] = maps_out[c];
        sizes[no++] = bytes;
    }
    for (void* l : {lambda1, lambda2})
        if (l) {
            outs[no] = l;
            sizes[no++] = lbytes;
        }
    for (int i = 0; i < no; ++i) {
        for (int j = i + 1; j < no; ++j)
            if (overlap(outs[i], sizes[i], outs[j], sizes[j])) return fail(NUFFT_ERR_INVALID_ARG, "two outputs overlap");
        for (int c = 0; c < C; ++c)
            if (overlap(outs[i], sizes[i], images_in[c], bytes))
                return fail(NUFFT_ERR_INVALID_ARG, "an output overlaps an input: every cell reads its neighbours, nothing runs in place");
    }

    CoilmapsLaunch a{};
    a.dtype = h->dtype;
    a.D = h->D;
    a.C = C;
    for (int d = 0; d < 3; ++d) {
        a.N[d] = (int)h->N[d];
        a.box[d] = h->box[d];
    }
    a.pitch[0] = 1;
    a.pitch[1] = h->N[0];
    a.pitch[2] = h->N[0] * h->N[1];
    a.n = h->n;
    for (int c = 0; c < C; ++c) {
        a.in[c] = images_in[c];
        a.out[c] = maps_out[c];
        a.p[2 * c] = phase_ref ? phase_ref[2 * c] : (c == 0 ? 1.0 : 0.0);
        a.p[2 * c + 1] = phase_ref ? phase_ref[2 * c + 1] : 0.0;
    }
    a.lambda1 = lambda1 ? lambda1 : h->d_lambda1;       // null without crop: the kernel then stores no λ1
    a.lambda2 = lambda2;
    a.part = static_cast<double*>(h->d_part);
    a.sweeps_part = static_cast<int32_t*>(h->d_sweeps);
    a.words = static_cast<double*>(h->d_words);
    a.crop2 = h->crop * h->crop;
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipError_t e = launch_coilmaps(a, h->L, s);
    if (e == hipSuccess) e = launch_coilmaps_max(a, h->L.G, s);
    if (e == hipSuccess && h->crop > 0.0) e = launch_coilmaps_crop(a, h->num_cus, s);
    if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a coil map kernel: ") + hipGetErrorString(e));
    return NUFFT_OK;
}

int nufft_coilmaps_apply_crop(nufft_coilmaps* h, void* const* maps_inout, const void* lambda1, double crop, void* stream_) {
    if (!h || !maps_inout) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (!(crop >= 0.0) || !std::isfinite(crop)) return fail(NUFFT_ERR_INVALID_ARG, "crop must be finite and not negative");
    if (!lambda1) lambda1 = h->d_lambda1;
    if (!lambda1) return fail(NUFFT_ERR_INVALID_ARG, "no lambda1: the object keeps one of its own only when it was created with crop > 0");
    if ((uintptr_t)lambda1 & (real_bytes(h->dtype) - 1)) return fail(NUFFT_ERR_INVALID_ARG, "lambda1 is not aligned");
    const size_t bytes = (size_t)h->n * 2 * real_bytes(h->dtype), lbytes = (size_t)h->n * real_bytes(h->dtype);
    for (int c = 0; c < h->C; ++c) {
        if (!maps_inout[c]) return fail(NUFFT_ERR_INVALID_ARG, "null data vector");
        if ((uintptr_t)maps_inout[c] & 15) return fail(NUFFT_ERR_INVALID_ARG, "the arrays must be 16-byte aligned");
        if (overlap(maps_inout[c], bytes, lambda1, lbytes)) return fail(NUFFT_ERR_INVALID_ARG, "a map overlaps lambda1");
        for (int k = c + 1; k < h->C; ++k)
            if (maps_inout[k] && overlap(maps_inout[c], bytes, maps_inout[k], bytes)) return fail(NUFFT_ERR_INVALID_ARG, "two maps overlap");
    }
    CoilmapsLaunch a{};
    a.dtype = h->dtype;
    a.C = h->C;
    a.n = h->n;
    for (int c = 0; c < h->C; ++c) a.out[c] = maps_inout[c];
    a.lambda1 = const_cast<void*>(lambda1);
    a.words = static_cast<double*>(h->d_words);
    a.crop2 = crop * crop;
    DeviceGuard guard(h->device);
    if (crop > 0.0)
        if (hipError_t e = launch_coilmaps_crop(a, h->num_cus, static_cast<hipStream_t>(stream_)); e != hipSuccess)
            return fail(NUFFT_ERR_HIP, std::string("launch of the coil map crop pass: ") + hipGetErrorString(e));
    return NUFFT_OK;
}

int nufft_coilmaps_last_sweeps(nufft_coilmaps* h, int32_t* sweeps_out, void* stream_) {
    if (!h || !sweeps_out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    DeviceGuard guard(h->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (capturing(stream)) return fail(NUFFT_ERR_INVALID_ARG, "nufft_coilmaps_last_sweeps synchronises: not on a capturing stream");
    NUFFT_HIP(hipMemcpyAsync(sweeps_out, static_cast<char*>(h->d_words) + 8, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    NUFFT_HIP(hipStreamSynchronize(stream));
    return NUFFT_OK;
}

}  // extern "C"
