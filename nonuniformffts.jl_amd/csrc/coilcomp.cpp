// Coil compression and noise pre-whitening (include/nufft_mi355x.h, coil compression section).
//
// The host side only enqueues (coilcomp_kernels.hip): reset is a memset node, accumulate the Gram kernel and its fold, finish one to
// three one-workgroup launches, apply one launch per 16 virtual coils.  The object owns the per-workgroup partials, R, W, A, λ and two
// words; the vector pointers travel as kernel arguments: no device table is written.  The Cholesky factor of a noise covariance and
// its inverse are formed here, on the host, in FP64.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "coilcomp.h"
#include "jacobi.h"
#include "solver_common.h"

using namespace nufft;

struct nufft_coilcomp {
    int dtype = NUFFT_F64, C = 1, device = -1, num_cus = 256;
    int rows = 0;                // rows of the matrix apply uses: 0 before the first finish / set_matrix
    bool noise = false;
    void* d_part = nullptr;      // complex double [kCcMaxGroups][C (C + 1) / 2]
    void* d_R = nullptr;         // complex double [C][C]
    void* d_W = nullptr;
    void* d_T = nullptr;         // W R W^H
    void* d_Uh = nullptr;
    void* d_A = nullptr;         // complex double [C + kCcApplyChunk][C]: the rows behind C stay zero
    void* d_lambda = nullptr;    // double [C]
    void* d_words = nullptr;     // int32 sweeps, status
    int64_t own_bytes = 0;
};

namespace {

using cd = std::complex<double>;

void release(nufft_coilcomp* h) {
    if (!h) return;
    if (h->device >= 0) {
        DeviceGuard guard(h->device);
        for (void* p : {h->d_part, h->d_R, h->d_W, h->d_T, h->d_Uh, h->d_A, h->d_lambda, h->d_words})
            if (p) (void)hipFree(p);
    }
    delete h;
}

size_t matrix_bytes(int C) { return (size_t)C * C * 16; }
size_t apply_matrix_bytes(int C) { return (size_t)(C + kCcApplyChunk) * C * 16; }
size_t part_bytes(int C) { return (size_t)kCcMaxGroups * (C * (C + 1) / 2) * 16; }

// the argument checks shared by create and layout, in the documented order
int describe(int dtype, int C) {
    if (dtype != NUFFT_F32 && dtype != NUFFT_F64) return fail(NUFFT_ERR_INVALID_ARG, "dtype must be NUFFT_F32 or NUFFT_F64");
    if (C < 1) return fail(NUFFT_ERR_INVALID_ARG, "ncoils = " + std::to_string(C) + " must be at least 1");
    if (C > kCcMaxCoils)
        return fail(NUFFT_ERR_UNSUPPORTED, std::to_string(C) + " coils: more than the " + std::to_string(kCcMaxCoils) + " lanes of a one-wave Jacobi team");
    return NUFFT_OK;
}

int64_t device_bytes(int C) {
    return (int64_t)(padded(part_bytes(C)) + 4 * padded(matrix_bytes(C)) + padded(apply_matrix_bytes(C)) + padded((size_t)C * 8) + padded(16));
}

void describe_info(nufft_coilcomp_info& i, int dtype, int C, int64_t n, const nufft_coilcomp* h) {
    std::memset(&i, 0, sizeof(i));
    const CcTiling tl = coilcomp_tiling(dtype == NUFFT_F32, C, n);
    const int np = C * (C + 1) / 2;
    i.dtype = dtype;
    i.ncoils = C;
    i.device = h ? h->device : -1;
    i.threads = kCcThreads;
    i.tile_samples = tl.TC;
    i.segments = tl.S;
    i.pairs = np;
    i.pairs_per_thread = (np + kCcThreads - 1) / kCcThreads;
    i.max_workgroups = kCcMaxGroups;
    i.apply_chunk = kCcApplyChunk;
    i.jacobi_team_lanes = 1;
    while (i.jacobi_team_lanes < C) i.jacobi_team_lanes *= 2;
    i.jacobi_sweeps_max = jacobi_team::kSweepsMax;
    i.lds_bytes_gram = (int32_t)tl.bytes;
    i.lds_bytes_eigen = (int32_t)coilcomp_eigen_lds(C);
    i.matrix_rows = h ? h->rows : 0;
    i.has_noise = h && h->noise ? 1 : 0;
    i.n = n;
    i.tiles = tl.tiles;
    i.tiles_per_workgroup = tl.tpw;
    i.workgroups = tl.G;
    i.workspace_bytes = h ? h->own_bytes : device_bytes(C);
}

// Ψ = L L^H, W = L^-1; `psi` and `w` are C x C complex doubles, row-major
int whitening(int C, const double* psi_, cd* w) {
    const cd* psi = reinterpret_cast<const cd*>(psi_);
    double big = 0.0;
    for (int e = 0; e < C * C; ++e) {
        if (!std::isfinite(psi[e].real()) || !std::isfinite(psi[e].imag())) return fail(NUFFT_ERR_INVALID_ARG, "the noise covariance is not finite");
        big = std::max(big, std::abs(psi[e]));
    }
    for (int i = 0; i < C; ++i)
        for (int j = 0; j <= i; ++j)
            if (std::abs(psi[i * C + j] - std::conj(psi[j * C + i])) > 1e-12 * big)
                return fail(NUFFT_ERR_INVALID_ARG, "the noise covariance is not Hermitian (entry " + std::to_string(i) + ", " + std::to_string(j) + ")");
    std::vector<cd> L((size_t)C * C, cd(0.0, 0.0));
    for (int j = 0; j < C; ++j) {
        double d = psi[j * C + j].real();
        for (int k = 0; k < j; ++k) d -= std::norm(L[j * C + k]);
        if (!(d > 0.0) || !std::isfinite(d))
            return fail(NUFFT_ERR_INVALID_ARG, "the noise covariance is not positive definite (pivot " + std::to_string(j) + ")");
        const double ljj = std::sqrt(d);
        L[j * C + j] = ljj;
        for (int i = j + 1; i < C; ++i) {
            cd s = psi[i * C + j];
            for (int k = 0; k < j; ++k) s -= L[i * C + k] * std::conj(L[j * C + k]);
            L[i * C + j] = s / ljj;
        }
    }
    std::fill(w, w + (size_t)C * C, cd(0.0, 0.0));
    for (int j = 0; j < C; ++j) {
        w[j * C + j] = 1.0 / L[j * C + j].real();
        for (int i = j + 1; i < C; ++i) {
            cd s(0.0, 0.0);
            for (int k = j; k < i; ++k) s += L[i * C + k] * w[k * C + j];
            w[i * C + j] = -s / L[i * C + i].real();
        }
    }
    return NUFFT_OK;
}

// a table of `count` vectors of n complex elements: no null entry, 16-byte aligned
int check_table(const void* const* t, int count, const char* what) {
    for (int c = 0; c < count; ++c) {
        if (!t[c]) return fail(NUFFT_ERR_INVALID_ARG, std::string("null ") + what + " vector");
        if ((uintptr_t)t[c] & 15) return fail(NUFFT_ERR_INVALID_ARG, std::string("the ") + what + " vectors must be 16-byte aligned");
    }
    return NUFFT_OK;
}

int upload(void* dst, const void* src, size_t bytes, hipStream_t stream) {
    NUFFT_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
    NUFFT_HIP(hipStreamSynchronize(stream));
    return NUFFT_OK;
}

int download(void* dst, const void* src, size_t bytes, hipStream_t stream) {
    NUFFT_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
    NUFFT_HIP(hipStreamSynchronize(stream));
    return NUFFT_OK;
}

}  // namespace

extern "C" {

int64_t nufft_sizeof_coilcomp_info(void) { return (int64_t)sizeof(nufft_coilcomp_info); }

int nufft_coilcomp_create(nufft_coilcomp** out, int dtype, int32_t ncoils, int device) {
    if (!out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (int rc = describe(dtype, ncoils)) return rc;
    if (device < 0) return fail(NUFFT_ERR_NO_DEVICE, "device = -1: coil compression runs on the device");
    nufft_coilcomp* h = new (std::nothrow) nufft_coilcomp;
    if (!h) return fail(NUFFT_ERR_ALLOC, "out of host memory");
    h->dtype = dtype;
    h->C = ncoils;
    h->device = device;
    DeviceGuard guard(device);
    h->num_cus = device_cus(device);
    if (hipError_t e = coilcomp_allow_lds(); e != hipSuccess) {
        (void)hipGetLastError();
        delete h;
        return fail(NUFFT_ERR_HIP, std::string("hipFuncSetAttribute of the coil compression kernels: ") + hipGetErrorString(e));
    }
    const int C = ncoils;
    int rc;
    if ((rc = alloc_buffer(h->own_bytes, "coil compression", &h->d_part, part_bytes(C))) ||
        (rc = alloc_buffer(h->own_bytes, "coil compression", &h->d_R, matrix_bytes(C))) ||
        (rc = alloc_buffer(h->own_bytes, "coil compression", &h->d_W, matrix_bytes(C))) ||
        (rc = alloc_buffer(h->own_bytes, "coil compression", &h->d_T, matrix_bytes(C))) ||
        (rc = alloc_buffer(h->own_bytes, "coil compression", &h->d_Uh, matrix_bytes(C))) ||
        (rc = alloc_buffer(h->own_bytes, "coil compression", &h->d_A, apply_matrix_bytes(C))) ||
        (rc = alloc_buffer(h->own_bytes, "coil compression", &h->d_lambda, (size_t)C * 8)) ||
        (rc = alloc_buffer(h->own_bytes, "coil compression", &h->d_words, 16))) {
        const std::string keep = nufft_last_error_message();
        release(h);
        return fail(rc, keep);
    }
    if (hipMemset(h->d_R, 0, matrix_bytes(C)) != hipSuccess || hipMemset(h->d_A, 0, apply_matrix_bytes(C)) != hipSuccess ||
        hipMemset(h->d_lambda, 0, (size_t)C * 8) != hipSuccess || hipMemset(h->d_words, 0, 16) != hipSuccess) {
        (void)hipGetLastError();
        release(h);
        return fail(NUFFT_ERR_HIP, "hipMemset of the coil compression matrices");
    }
    *out = h;
    return NUFFT_OK;
}

int nufft_coilcomp_destroy(nufft_coilcomp* h) {
    release(h);
    return NUFFT_OK;
}

int nufft_coilcomp_layout(int dtype, int32_t ncoils, int64_t n, nufft_coilcomp_info* o) {
    if (!o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (dtype != NUFFT_F32 && dtype != NUFFT_F64) return fail(NUFFT_ERR_INVALID_ARG, "dtype must be NUFFT_F32 or NUFFT_F64");
    if (ncoils < 1) return fail(NUFFT_ERR_INVALID_ARG, "ncoils = " + std::to_string(ncoils) + " must be at least 1");
    if (n < 1) return fail(NUFFT_ERR_INVALID_ARG, "n must be at least 1");
    if (int rc = describe(dtype, ncoils)) return rc;
    nufft_coilcomp_info i;
    describe_info(i, dtype, ncoils, n, nullptr);
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_coilcomp_get_info(const nufft_coilcomp* h, int64_t n, nufft_coilcomp_info* o) {
    if (!h || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (n < 1) return fail(NUFFT_ERR_INVALID_ARG, "n must be at least 1");
    nufft_coilcomp_info i;
    describe_info(i, h->dtype, h->C, n, h);
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_coilcomp_whitening_matrix(int32_t ncoils, const double* psi, double* w_out) {
    if (!psi || !w_out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (int rc = describe(NUFFT_F64, ncoils)) return rc;
    return whitening(ncoils, psi, reinterpret_cast<cd*>(w_out));
}

int nufft_coilcomp_set_noise_covariance(nufft_coilcomp* h, const double* psi, void* stream_) {
    if (!h) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (!psi) {
        h->noise = false;
        return NUFFT_OK;
    }
    std::vector<cd> w((size_t)h->C * h->C);
    if (int rc = whitening(h->C, psi, w.data())) return rc;
    DeviceGuard guard(h->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = refuse_capture("nufft_coilcomp_set_noise_covariance", stream)) return rc;
    if (int rc = upload(h->d_W, w.data(), matrix_bytes(h->C), stream)) return rc;
    h->noise = true;
    return NUFFT_OK;
}

int nufft_coilcomp_reset(nufft_coilcomp* h, void* stream_) {
    if (!h) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    DeviceGuard guard(h->device);
    NUFFT_HIP(hipMemsetAsync(h->d_R, 0, matrix_bytes(h->C), static_cast<hipStream_t>(stream_)));
    return NUFFT_OK;
}

int nufft_coilcomp_accumulate(nufft_coilcomp* h, const void* const* y, const void* weights, int64_t n, void* stream_) {
    if (!h || !y) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (n < 1) return fail(NUFFT_ERR_INVALID_ARG, "n must be at least 1");
    if (int rc = check_table(y, h->C, "data")) return rc;
    if ((uintptr_t)weights & (real_bytes(h->dtype) - 1)) return fail(NUFFT_ERR_INVALID_ARG, "the weights are not aligned");
    CcGramLaunch a{};
    a.dtype = h->dtype;
    a.C = h->C;
    a.n = n;
    a.tl = coilcomp_tiling(h->dtype == NUFFT_F32, h->C, n);
    for (int c = 0; c < h->C; ++c) a.y.p[c] = y[c];
    a.weights = weights;
    a.part = static_cast<double*>(h->d_part);
    a.R = static_cast<double*>(h->d_R);
    DeviceGuard guard(h->device);
    if (hipError_t e = launch_coilcomp_gram(a, static_cast<hipStream_t>(stream_)); e != hipSuccess)
        return fail(NUFFT_ERR_HIP, std::string("launch of the coil compression Gram kernels: ") + hipGetErrorString(e));
    return NUFFT_OK;
}

int nufft_coilcomp_finish(nufft_coilcomp* h, void* stream_) {
    if (!h) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    CcFinishLaunch a{};
    a.C = h->C;
    a.whiten = h->noise ? 1 : 0;
    a.R = static_cast<const double*>(h->d_R);
    a.W = static_cast<const double*>(h->d_W);
    a.T = static_cast<double*>(h->d_T);
    a.Uh = static_cast<double*>(h->d_Uh);
    a.A = static_cast<double*>(h->d_A);
    a.lambda = static_cast<double*>(h->d_lambda);
    a.words = static_cast<int32_t*>(h->d_words);
    DeviceGuard guard(h->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // a matrix of fewer rows may have been installed: the rows behind it are zero, and finish writes all C
    if (hipError_t e = launch_coilcomp_finish(a, stream); e != hipSuccess)
        return fail(NUFFT_ERR_HIP, std::string("launch of the coil compression eigen kernels: ") + hipGetErrorString(e));
    h->rows = h->C;
    return NUFFT_OK;
}

int nufft_coilcomp_set_matrix(nufft_coilcomp* h, const double* A_host, int32_t rows, void* stream_) {
    if (!h || !A_host) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (rows < 1 || rows > h->C) return fail(NUFFT_ERR_INVALID_ARG, "rows = " + std::to_string(rows) + " must be 1 ... " + std::to_string(h->C));
    for (int64_t e = 0; e < (int64_t)rows * h->C * 2; ++e)
        if (!std::isfinite(A_host[e])) return fail(NUFFT_ERR_INVALID_ARG, "the matrix is not finite");
    DeviceGuard guard(h->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = refuse_capture("nufft_coilcomp_set_matrix", stream)) return rc;
    std::vector<double> full(apply_matrix_bytes(h->C) / 8, 0.0);
    std::memcpy(full.data(), A_host, (size_t)rows * h->C * 16);
    if (int rc = upload(h->d_A, full.data(), apply_matrix_bytes(h->C), stream)) return rc;
    h->rows = rows;
    return NUFFT_OK;
}

int nufft_coilcomp_apply(nufft_coilcomp* h, void* const* out, int32_t nvirtual, const void* const* in, int64_t n, void* stream_) {
    if (!h || !out || !in) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (h->rows < 1) return fail(NUFFT_ERR_INVALID_ARG, "nufft_coilcomp_finish or nufft_coilcomp_set_matrix must be called before nufft_coilcomp_apply");
    if (nvirtual < 1 || nvirtual > h->rows)
        return fail(NUFFT_ERR_INVALID_ARG, "nvirtual = " + std::to_string(nvirtual) + " must be 1 ... " + std::to_string(h->rows) + ", the rows of the matrix");
    if (n < 1) return fail(NUFFT_ERR_INVALID_ARG, "n must be at least 1");
    const int C = h->C, V = nvirtual;
    if (int rc = check_table(in, C, "input")) return rc;
    if (int rc = check_table(out, V, "output")) return rc;
    const size_t bytes = (size_t)n * 2 * real_bytes(h->dtype);
    for (int v = 0; v < V; ++v) {
        for (int c = 0; c < C; ++c)
            if (overlap(out[v], in[c], bytes)) return fail(NUFFT_ERR_INVALID_ARG, "an output overlaps an input: the inputs are read once per 16 virtual coils");
        for (int k = v + 1; k < V; ++k)
            if (overlap(out[v], out[k], bytes)) return fail(NUFFT_ERR_INVALID_ARG, "two outputs overlap");
    }
    CcApplyLaunch a{};
    a.dtype = h->dtype;
    a.C = C;
    a.n = n;
    for (int c = 0; c < C; ++c) a.in.p[c] = in[c];
    DeviceGuard guard(h->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    for (int v0 = 0; v0 < V; v0 += kCcApplyChunk) {
        a.v0 = v0;
        a.V = std::min(kCcApplyChunk, V - v0);
        for (int v = 0; v < kCcApplyChunk; ++v) a.out[v] = v < a.V ? out[v0 + v] : nullptr;
        a.A = static_cast<const double*>(h->d_A) + (size_t)v0 * C * 2;
        if (hipError_t e = launch_coilcomp_apply(a, h->num_cus, stream); e != hipSuccess)
            return fail(NUFFT_ERR_HIP, std::string("launch of the coil compression apply kernel: ") + hipGetErrorString(e));
    }
    return NUFFT_OK;
}

int nufft_coilcomp_get_gram(nufft_coilcomp* h, double* host_out, void* stream_) {
    if (!h || !host_out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    DeviceGuard guard(h->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = refuse_capture("nufft_coilcomp_get_gram", stream)) return rc;
    return download(host_out, h->d_R, matrix_bytes(h->C), stream);
}

int nufft_coilcomp_get_matrix(nufft_coilcomp* h, double* host_out, void* stream_) {
    if (!h || !host_out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (h->rows < 1) return fail(NUFFT_ERR_INVALID_ARG, "nufft_coilcomp_finish or nufft_coilcomp_set_matrix must be called before nufft_coilcomp_get_matrix");
    DeviceGuard guard(h->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = refuse_capture("nufft_coilcomp_get_matrix", stream)) return rc;
    return download(host_out, h->d_A, matrix_bytes(h->C), stream);
}

int nufft_coilcomp_get_spectrum(nufft_coilcomp* h, double* lambda_out, int32_t* sweeps_out, int32_t* status_out, void* stream_) {
    if (!h) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    DeviceGuard guard(h->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = refuse_capture("nufft_coilcomp_get_spectrum", stream)) return rc;
    int32_t words[2] = {0, 0};
    if (lambda_out) NUFFT_HIP(hipMemcpyAsync(lambda_out, h->d_lambda, (size_t)h->C * 8, hipMemcpyDeviceToHost, stream));
    NUFFT_HIP(hipMemcpyAsync(words, h->d_words, sizeof(words), hipMemcpyDeviceToHost, stream));
    NUFFT_HIP(hipStreamSynchronize(stream));
    if (sweeps_out) *sweeps_out = words[0];
    if (status_out) *status_out = words[1];
    return NUFFT_OK;
}

}  // extern "C"
