// Time segmentation of a field map (include/nufft_mi355x.h, field-map section): the histogram least-squares fit of
// Sutton, Noll & Fessler (IEEE TMI 2003).
//
// fit is set-up: two reductions on the device (range, histogram), then the L × L normal matrix at the bin centres, its Cholesky factor
// and inverse on the host in FP64, and the upload of what the interpolator kernel reads.  interpolators and factors only enqueue.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "field.h"
#include "solver_common.h"

using namespace nufft;

struct nufft_fieldseg {
    int dtype = NUFFT_F64, L = 1, nbins = 1, device = -1, num_cus = 256;
    int nb = 0;                  // bins in use: 0 before the first fit, 1 for a constant ω, else nbins
    double delta = 0.0;          // spacing of the centres
    std::vector<double> tau;     // [L] of the last fit
    void* d_part = nullptr;      // FsRange [kFsMaxGroups + 1]: the rows and, behind them, their fold
    void* d_counts = nullptr;    // uint32 [nbins]
    void* d_centres = nullptr;   // double [nbins]
    void* d_table = nullptr;     // complex double [nbins][tier]: h_b exp(i ω_b τ_l)
    void* d_G = nullptr;         // complex double [L][L]: the normal matrix (without the ridge)
    void* d_P = nullptr;         // complex double [L][L]: (G + ridge tr(G) / L I)^-1
    int64_t own_bytes = 0;
};

namespace {

using cd = std::complex<double>;

void release(nufft_fieldseg* h) {
    if (!h) return;
    if (h->device >= 0) {
        DeviceGuard guard(h->device);
        for (void* p : {h->d_part, h->d_counts, h->d_centres, h->d_table, h->d_G, h->d_P})
            if (p) (void)hipFree(p);
    }
    delete h;
}

size_t part_bytes() { return (size_t)(kFsMaxGroups + 1) * sizeof(FsRange); }
size_t table_bytes(int L, int nbins) { return (size_t)nbins * fieldseg_tier(L) * 16; }
size_t matrix_bytes(int L) { return (size_t)L * L * 16; }

// the argument checks shared by create and layout, in the documented order
int describe(int dtype, int L, int nbins) {
    if (dtype != NUFFT_F32 && dtype != NUFFT_F64) return fail(NUFFT_ERR_INVALID_ARG, "dtype must be NUFFT_F32 or NUFFT_F64");
    if (L < 1) return fail(NUFFT_ERR_INVALID_ARG, "nsegments = " + std::to_string(L) + " must be at least 1");
    if (nbins < 1 || nbins > kFsMaxBins)
        return fail(NUFFT_ERR_INVALID_ARG, "nbins = " + std::to_string(nbins) + " must be 1 ... " + std::to_string(kFsMaxBins));
    if (L > kFsMaxSegments)
        return fail(NUFFT_ERR_UNSUPPORTED, std::to_string(L) + " segments: more than the " + std::to_string(kFsMaxSegments) + " a segmented Toeplitz operator takes");
    return NUFFT_OK;
}

int64_t device_bytes(int L, int nbins) {
    return (int64_t)(padded(part_bytes()) + padded((size_t)nbins * 4) + padded((size_t)nbins * 8) + padded(table_bytes(L, nbins)) + 2 * padded(matrix_bytes(L)));
}

void describe_info(nufft_fieldseg_info& i, int dtype, int L, int nbins, const nufft_fieldseg* h) {
    std::memset(&i, 0, sizeof(i));
    i.dtype = dtype;
    i.nsegments = L;
    i.nbins = nbins;
    i.device = h ? h->device : -1;
    i.threads = kFsThreads;
    i.segment_tier = fieldseg_tier(L);
    i.reseed_bins = kFsReseed;
    i.max_workgroups = kFsMaxGroups;
    i.lds_bytes_interpolators = (int32_t)fieldseg_interp_lds(L);
    i.lds_bytes_histogram = (int32_t)fieldseg_hist_lds(nbins);
    i.bins_used = h ? h->nb : 0;
    i.workspace_bytes = h ? h->own_bytes : device_bytes(L, nbins);
}

// A = L L^H in place of the lower triangle of `a` (n × n, row-major); the index of the pivot that is not positive, or −1
int cholesky(int n, std::vector<cd>& a) {
    for (int j = 0; j < n; ++j) {
        double d = a[(size_t)j * n + j].real();
        for (int k = 0; k < j; ++k) d -= std::norm(a[(size_t)j * n + k]);
        if (!(d > 0.0) || !std::isfinite(d)) return j;
        const double ljj = std::sqrt(d);
        a[(size_t)j * n + j] = ljj;
        for (int i = j + 1; i < n; ++i) {
            cd s = a[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) s -= a[(size_t)i * n + k] * std::conj(a[(size_t)j * n + k]);
            a[(size_t)i * n + j] = s / ljj;
        }
    }
    return -1;
}

// P = (L L^H)^-1 = W^H W with W = L^-1
void inverse_from_factor(int n, const std::vector<cd>& l, std::vector<cd>& p) {
    std::vector<cd> w((size_t)n * n, cd(0.0, 0.0));
    for (int j = 0; j < n; ++j) {
        w[(size_t)j * n + j] = 1.0 / l[(size_t)j * n + j].real();
        for (int i = j + 1; i < n; ++i) {
            cd s(0.0, 0.0);
            for (int k = j; k < i; ++k) s += l[(size_t)i * n + k] * w[(size_t)k * n + j];
            w[(size_t)i * n + j] = -s / l[(size_t)i * n + i].real();
        }
    }
    p.assign((size_t)n * n, cd(0.0, 0.0));
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            cd s(0.0, 0.0);
            for (int k = std::max(r, c); k < n; ++k) s += std::conj(w[(size_t)k * n + r]) * w[(size_t)k * n + c];
            p[(size_t)r * n + c] = s;
        }
}

int check_rows(const void* const* rows, int L, const char* what) {
    for (int l = 0; l < L; ++l) {
        if (!rows[l]) return fail(NUFFT_ERR_INVALID_ARG, std::string("null ") + what);
        if ((uintptr_t)rows[l] & 15) return fail(NUFFT_ERR_INVALID_ARG, std::string("every ") + what + " must be 16-byte aligned");
    }
    return NUFFT_OK;
}

int download(void* dst, const void* src, size_t bytes, hipStream_t stream) {
    NUFFT_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
    NUFFT_HIP(hipStreamSynchronize(stream));
    return NUFFT_OK;
}

}  // namespace

extern "C" {

int64_t nufft_sizeof_fieldseg_info(void) { return (int64_t)sizeof(nufft_fieldseg_info); }

int nufft_fieldseg_create(nufft_fieldseg** out, int dtype, int32_t nsegments, int32_t nbins, int device) {
    if (!out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (int rc = describe(dtype, nsegments, nbins)) return rc;
    if (device < 0) return fail(NUFFT_ERR_NO_DEVICE, "device = -1: the segment fit runs on the device");
    nufft_fieldseg* h = new (std::nothrow) nufft_fieldseg;
    if (!h) return fail(NUFFT_ERR_ALLOC, "out of host memory");
    h->dtype = dtype;
    h->L = nsegments;
    h->nbins = nbins;
    h->device = device;
    DeviceGuard guard(device);
    h->num_cus = device_cus(device);
    int rc;
    if ((rc = alloc_buffer(h->own_bytes, "segment fit", &h->d_part, part_bytes())) ||
        (rc = alloc_buffer(h->own_bytes, "segment fit", &h->d_counts, (size_t)nbins * 4)) ||
        (rc = alloc_buffer(h->own_bytes, "segment fit", &h->d_centres, (size_t)nbins * 8)) ||
        (rc = alloc_buffer(h->own_bytes, "segment fit", &h->d_table, table_bytes(h->L, nbins))) ||
        (rc = alloc_buffer(h->own_bytes, "segment fit", &h->d_G, matrix_bytes(h->L))) ||
        (rc = alloc_buffer(h->own_bytes, "segment fit", &h->d_P, matrix_bytes(h->L)))) {
        const std::string keep = nufft_last_error_message();
        release(h);
        return fail(rc, keep);
    }
    *out = h;
    return NUFFT_OK;
}

int nufft_fieldseg_destroy(nufft_fieldseg* h) {
    release(h);
    return NUFFT_OK;
}

int nufft_fieldseg_layout(int dtype, int32_t nsegments, int32_t nbins, nufft_fieldseg_info* o) {
    if (!o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (int rc = describe(dtype, nsegments, nbins)) return rc;
    nufft_fieldseg_info i;
    describe_info(i, dtype, nsegments, nbins, nullptr);
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_fieldseg_get_info(const nufft_fieldseg* h, nufft_fieldseg_info* o) {
    if (!h || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    nufft_fieldseg_info i;
    describe_info(i, h->dtype, h->L, h->nbins, h);
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_fieldseg_fit(nufft_fieldseg* h, const void* omega, const uint8_t* mask, int64_t n, const double* tau, double ridge, void* stream_) {
    if (!h || !omega || !tau) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (n < 1) return fail(NUFFT_ERR_INVALID_ARG, "n must be at least 1");
    if ((uintptr_t)omega & (real_bytes(h->dtype) - 1)) return fail(NUFFT_ERR_INVALID_ARG, "the field map is not aligned");
    const int L = h->L;
    for (int l = 0; l < L; ++l) {
        if (!std::isfinite(tau[l])) return fail(NUFFT_ERR_INVALID_ARG, "tau is not finite");
        if (l > 0 && !(tau[l] > tau[l - 1])) return fail(NUFFT_ERR_INVALID_ARG, "tau must be strictly increasing");
    }
    if (!std::isfinite(ridge) || ridge < 0) return fail(NUFFT_ERR_INVALID_ARG, "ridge must be finite and not negative");
    DeviceGuard guard(h->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = refuse_capture("nufft_fieldseg_fit", stream)) return rc;
    h->nb = 0;

    FsRange* part = static_cast<FsRange*>(h->d_part);
    if (hipError_t e = launch_fieldseg_range(h->dtype, omega, mask, n, part, part + kFsMaxGroups, h->num_cus, stream); e != hipSuccess)
        return fail(NUFFT_ERR_HIP, std::string("launch of the range kernels of the segment fit: ") + hipGetErrorString(e));
    FsRange range{};
    if (int rc = download(&range, part + kFsMaxGroups, sizeof(range), stream)) return rc;
    if (range.counted == 0) return fail(NUFFT_ERR_INVALID_ARG, "the mask is empty: no value of the field map is counted");
    if (range.bad > 0) return fail(NUFFT_ERR_INVALID_ARG, std::to_string(range.bad) + " counted values of the field map are not finite");

    const bool constant = range.hi == range.lo;
    const int nb = constant ? 1 : h->nbins;
    const double width = range.hi - range.lo;
    const double scale = constant ? 0.0 : (double)h->nbins / width;
    if (!constant && !std::isfinite(scale)) return fail(NUFFT_ERR_INVALID_ARG, "the range of the field map is too small or too large to be binned");
    NUFFT_HIP(hipMemsetAsync(h->d_counts, 0, (size_t)h->nbins * 4, stream));
    if (hipError_t e = launch_fieldseg_histogram(h->dtype, omega, mask, n, range.lo, scale, nb, static_cast<uint32_t*>(h->d_counts), h->num_cus, stream);
        e != hipSuccess)
        return fail(NUFFT_ERR_HIP, std::string("launch of the histogram kernel of the segment fit: ") + hipGetErrorString(e));
    std::vector<uint32_t> counts((size_t)nb);
    if (int rc = download(counts.data(), h->d_counts, (size_t)nb * 4, stream)) return rc;

    // the centres, equally spaced, and the normal matrix at them
    const double delta = constant ? 0.0 : width / (double)h->nbins;
    std::vector<double> centres((size_t)nb);
    for (int b = 0; b < nb; ++b) centres[(size_t)b] = constant ? range.lo : range.lo + ((double)b + 0.5) * delta;
    std::vector<cd> G((size_t)L * L, cd(0.0, 0.0));
    for (int r = 0; r < L; ++r)
        for (int c = r; c < L; ++c) {
            cd s(0.0, 0.0);
            const double dt = tau[c] - tau[r];
            for (int b = 0; b < nb; ++b)
                if (counts[(size_t)b]) s += (double)counts[(size_t)b] * std::polar(1.0, -centres[(size_t)b] * dt);
            G[(size_t)r * L + c] = s;
            G[(size_t)c * L + r] = std::conj(s);
        }
    double trace = 0.0;
    for (int l = 0; l < L; ++l) trace += G[(size_t)l * L + l].real();
    std::vector<cd> F = G, P;
    for (int l = 0; l < L; ++l) F[(size_t)l * L + l] += ridge * trace / (double)L;
    if (const int bad = cholesky(L, F); bad >= 0)
        return fail(NUFFT_ERR_INVALID_ARG, "the normal matrix of the segment fit is not positive definite (pivot " + std::to_string(bad) +
                                               "): the histogram does not tell the segments apart; raise ridge (now " + std::to_string(ridge) +
                                               ") or use fewer segments");
    inverse_from_factor(L, F, P);

    // what the interpolator kernel reads: h_b exp(i ω_b τ_l), zero behind L
    const int tier = fieldseg_tier(L);
    std::vector<cd> table((size_t)nb * tier, cd(0.0, 0.0));
    for (int b = 0; b < nb; ++b)
        for (int l = 0; l < L; ++l) table[(size_t)b * tier + l] = (double)counts[(size_t)b] * std::polar(1.0, centres[(size_t)b] * tau[l]);
    NUFFT_HIP(hipMemcpyAsync(h->d_centres, centres.data(), (size_t)nb * 8, hipMemcpyHostToDevice, stream));
    NUFFT_HIP(hipMemcpyAsync(h->d_table, table.data(), table.size() * 16, hipMemcpyHostToDevice, stream));
    NUFFT_HIP(hipMemcpyAsync(h->d_G, G.data(), matrix_bytes(L), hipMemcpyHostToDevice, stream));
    NUFFT_HIP(hipMemcpyAsync(h->d_P, P.data(), matrix_bytes(L), hipMemcpyHostToDevice, stream));
    NUFFT_HIP(hipStreamSynchronize(stream));      // the host vectors go away on return
    h->tau.assign(tau, tau + L);
    h->delta = delta;
    h->nb = nb;
    return NUFFT_OK;
}

int nufft_fieldseg_interpolators(nufft_fieldseg* h, const void* times, int64_t np, void* const* phi_rows, void* stream_) {
    if (!h || !times || !phi_rows) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (h->nb < 1) return fail(NUFFT_ERR_INVALID_ARG, "nufft_fieldseg_fit must be called before nufft_fieldseg_interpolators");
    if (np < 1) return fail(NUFFT_ERR_INVALID_ARG, "num_points must be at least 1");
    if (np > ((int64_t)1 << 38)) return fail(NUFFT_ERR_UNSUPPORTED, "more than 2^38 points in one call");
    if ((uintptr_t)times & (real_bytes(h->dtype) - 1)) return fail(NUFFT_ERR_INVALID_ARG, "the times are not aligned");
    if (int rc = check_rows(phi_rows, h->L, "row of interpolators")) return rc;
    FsPointers rows{};
    for (int l = 0; l < h->L; ++l) rows.p[l] = phi_rows[l];
    DeviceGuard guard(h->device);
    if (hipError_t e = launch_fieldseg_interpolators(h->dtype, h->L, h->nb, times, np, static_cast<const double*>(h->d_table),
                                                     static_cast<const double*>(h->d_centres), h->delta, static_cast<const double*>(h->d_P), rows,
                                                     static_cast<hipStream_t>(stream_));
        e != hipSuccess)
        return fail(NUFFT_ERR_HIP, std::string("launch of the interpolator kernel: ") + hipGetErrorString(e));
    return NUFFT_OK;
}

int nufft_fieldseg_factors(nufft_fieldseg* h, const void* omega, int64_t n, void* const* B, void* stream_) {
    if (!h || !omega || !B) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (h->nb < 1) return fail(NUFFT_ERR_INVALID_ARG, "nufft_fieldseg_fit must be called before nufft_fieldseg_factors (it sets tau)");
    if (n < 1) return fail(NUFFT_ERR_INVALID_ARG, "n must be at least 1");
    if ((uintptr_t)omega & (real_bytes(h->dtype) - 1)) return fail(NUFFT_ERR_INVALID_ARG, "the field map is not aligned");
    if (int rc = check_rows(B, h->L, "factor")) return rc;
    FsPointers rows{};
    FsTau tau{};
    for (int l = 0; l < h->L; ++l) {
        rows.p[l] = B[l];
        tau.v[l] = h->tau[(size_t)l];
    }
    DeviceGuard guard(h->device);
    if (hipError_t e = launch_fieldseg_factors(h->dtype, h->L, omega, n, tau, rows, h->num_cus, static_cast<hipStream_t>(stream_)); e != hipSuccess)
        return fail(NUFFT_ERR_HIP, std::string("launch of the factor kernel: ") + hipGetErrorString(e));
    return NUFFT_OK;
}

int nufft_fieldseg_get_histogram(nufft_fieldseg* h, uint32_t* counts_out, double* centres_out, void* stream_) {
    if (!h) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (h->nb < 1) return fail(NUFFT_ERR_INVALID_ARG, "nufft_fieldseg_fit must be called before nufft_fieldseg_get_histogram");
    DeviceGuard guard(h->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = refuse_capture("nufft_fieldseg_get_histogram", stream)) return rc;
    if (counts_out) NUFFT_HIP(hipMemcpyAsync(counts_out, h->d_counts, (size_t)h->nb * 4, hipMemcpyDeviceToHost, stream));
    if (centres_out) NUFFT_HIP(hipMemcpyAsync(centres_out, h->d_centres, (size_t)h->nb * 8, hipMemcpyDeviceToHost, stream));
    NUFFT_HIP(hipStreamSynchronize(stream));
    return NUFFT_OK;
}

int nufft_fieldseg_get_gram(nufft_fieldseg* h, double* host_out, void* stream_) {
    if (!h || !host_out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (h->nb < 1) return fail(NUFFT_ERR_INVALID_ARG, "nufft_fieldseg_fit must be called before nufft_fieldseg_get_gram");
    DeviceGuard guard(h->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = refuse_capture("nufft_fieldseg_get_gram", stream)) return rc;
    return download(host_out, h->d_G, matrix_bytes(h->L), stream);
}

int nufft_fieldseg_get_solver_matrix(nufft_fieldseg* h, double* host_out, void* stream_) {
    if (!h || !host_out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (h->nb < 1) return fail(NUFFT_ERR_INVALID_ARG, "nufft_fieldseg_fit must be called before nufft_fieldseg_get_solver_matrix");
    DeviceGuard guard(h->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = refuse_capture("nufft_fieldseg_get_solver_matrix", stream)) return rc;
    return download(host_out, h->d_P, matrix_bytes(h->L), stream);
}

int nufft_fieldseg_get_tau(nufft_fieldseg* h, double* host_out, void* stream_) {
    if (!h || !host_out) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (h->nb < 1) return fail(NUFFT_ERR_INVALID_ARG, "nufft_fieldseg_fit must be called before nufft_fieldseg_get_tau");
    DeviceGuard guard(h->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = refuse_capture("nufft_fieldseg_get_tau", stream)) return rc;
    NUFFT_HIP(hipStreamSynchronize(stream));
    std::memcpy(host_out, h->tau.data(), (size_t)h->L * 8);
    return NUFFT_OK;
}

}  // extern "C"
