// Periodic orthogonal wavelet transform with its proximal map (include/nufft_mi355x.h, wavelet section).
//
// The host side only enqueues: one kernel of wavelet_kernels.hip per level.  Level l reads the low-pass corner that level l − 1 left
// in a scratch array and writes its own into the other scratch array (tiles with halos would race on a corner transformed in place):
// A holds n / 2^D elements per component, B n / 4^D.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "host_common.h"
#include "wavelet.h"

using namespace nufft;

struct nufft_wavelet {
    int dtype = NUFFT_F64, D = 1, C = 1, device = -1;
    int wavelet = NUFFT_WAVELET_HAAR, taps = 2, levels = 1;
    int64_t N[3] = {1, 1, 1};
    int64_t n = 1;
    size_t strideA = 0, strideB = 0;      // bytes between the components' scratch arrays
    void* d_A = nullptr;
    void* d_B = nullptr;
    void* d_part = nullptr;               // double[C][P]
    int P = 0;
    std::vector<int> part_off;            // per level
    int64_t own_bytes = 0, scratch_bytes = 0;
};

namespace {

void release(nufft_wavelet* w) {
    if (!w) return;
    if (w->device >= 0) {
        DeviceGuard g(w->device);
        for (void* p : {w->d_A, w->d_B, w->d_part})
            if (p) (void)hipFree(p);
    }
    delete w;
}

size_t elem_bytes(const nufft_wavelet* w) { return 2 * real_bytes(w->dtype); }

// The geometry of level `l` (everything but the pointers); the tile is wavelet_tile's whatever the level's box (a box smaller than the
// tile wraps on load and masks on store).
WaveletLevel geometry(const nufft_wavelet* w, int l) {
    WaveletLevel g{};
    g.dtype = w->dtype;
    g.D = w->D;
    g.taps = w->taps;
    const bool f32 = w->dtype == NUFFT_F32;
    const int to[3] = {wavelet_tile(f32, w->D, 0), wavelet_tile(f32, w->D, 1), wavelet_tile(f32, w->D, 2)};
    for (int d = 0; d < 3; ++d) {
        g.m[d] = d < w->D ? (int)(w->N[d] >> l) : 1;
        g.h[d] = d < w->D ? g.m[d] / 2 : 1;
        g.to[d] = to[d];
        g.tiles[d] = (g.h[d] + g.to[d] - 1) / g.to[d];
    }
    g.pitch[0] = 1;
    g.pitch[1] = w->N[0];
    g.pitch[2] = w->N[0] * w->N[1];
    return g;
}

int64_t workgroups(const WaveletLevel& g) { return (int64_t)g.tiles[0] * g.tiles[1] * g.tiles[2]; }

int check_tables(const nufft_wavelet* w, void* const* out, const void* const* in) {
    return nufft::check_tables(w->C, (size_t)w->n * elem_bytes(w), out, in, false,
                               "the output overlaps the input: a level reads its sub-box while other tiles store into it");
}

char* at(void* base, size_t stride, int c) { return static_cast<char*>(base) + stride * (size_t)c; }

}  // namespace

namespace nufft {

int wavelet_create_geometry(nufft_wavelet** out, int dtype, int D, const int64_t* N, int C, int device, const nufft_wavelet_params* params) {
    nufft_wavelet_params p;
    if (int rc = read_params(p, params, "nufft_wavelet_params")) return rc;
    if (p.wavelet != NUFFT_WAVELET_HAAR && p.wavelet != NUFFT_WAVELET_DB2)
        return fail(NUFFT_ERR_INVALID_ARG, "unknown wavelet (NUFFT_WAVELET_HAAR or NUFFT_WAVELET_DB2)");
    if (p.levels < 1 || p.levels > 30) return fail(NUFFT_ERR_INVALID_ARG, "levels must lie in 1 ... 30");
    for (int d = 0; d < D; ++d) {
        if (N[d] % ((int64_t)1 << p.levels) != 0)
            return fail(NUFFT_ERR_INVALID_ARG, "N[" + std::to_string(d) + "] = " + std::to_string(N[d]) + " is not a multiple of 2^levels = " +
                                                   std::to_string((int64_t)1 << p.levels));
        if (p.wavelet == NUFFT_WAVELET_DB2 && (N[d] >> p.levels) < 2)
            return fail(NUFFT_ERR_INVALID_ARG, "N[" + std::to_string(d) + "] / 2^levels must be at least 2 for the 4-tap filter: the deepest level's input "
                                                   "must be one filter long");
        if (N[d] > ((int64_t)1 << 30)) return fail(NUFFT_ERR_UNSUPPORTED, "more than 2^30 cells per axis");
    }
    if (device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only plan (device = -1): the wavelet transform runs on the device");

    nufft_wavelet* w = new (std::nothrow) nufft_wavelet();
    if (!w) return fail(NUFFT_ERR_ALLOC, "out of host memory");
    w->dtype = dtype;
    w->D = D;
    w->C = C;
    w->device = device;
    w->wavelet = p.wavelet;
    w->taps = p.wavelet == NUFFT_WAVELET_HAAR ? 2 : 4;
    w->levels = p.levels;
    for (int d = 0; d < D; ++d) {
        w->N[d] = N[d];
        w->n *= N[d];
    }
    for (int l = 0; l < w->levels; ++l) {
        w->part_off.push_back(w->P);
        w->P += (int)workgroups(geometry(w, l));
    }
    DeviceGuard guard(device);
    const size_t eb = elem_bytes(w);
    w->strideA = padded((size_t)(w->n >> D) * eb);
    w->strideB = padded((size_t)(w->n >> (2 * D)) * eb);
    int rc = alloc_buffer(w->own_bytes, "wavelet", &w->d_A, (size_t)C * w->strideA);
    if (!rc && w->levels > 1) rc = alloc_buffer(w->own_bytes, "wavelet", &w->d_B, (size_t)C * w->strideB);
    w->scratch_bytes = w->own_bytes;
    if (!rc) rc = alloc_buffer(w->own_bytes, "wavelet", &w->d_part, (size_t)C * w->P * sizeof(double));
    if (rc) {
        const std::string keep = nufft_last_error_message();
        release(w);
        return fail(rc, keep);
    }
    *out = w;
    return NUFFT_OK;
}

// Level l reads its fine side from the callers' array (l = 0) or from the scratch level l − 1 wrote, and writes its low-pass corner to
// the other scratch array, the last level into the output's corner.  Level l − 1 wrote A for even l − 1.
int wavelet_forward(nufft_wavelet* w, void* const* out, const void* const* in, const double* thr_host, const int32_t* flag, hipStream_t stream) {
    for (int l = 0; l < w->levels; ++l) {
        WaveletLevel g = geometry(w, l);
        g.shrink = thr_host ? 1 : 0;
        g.part = thr_host ? static_cast<double*>(w->d_part) : nullptr;
        g.P = w->P;
        g.part_off = w->part_off[l];
        g.flag = flag;
        g.fine_dense = l > 0;
        g.low_dense = l + 1 < w->levels;
        void* src_base = (l - 1) % 2 == 0 ? w->d_A : w->d_B;
        const size_t src_stride = (l - 1) % 2 == 0 ? w->strideA : w->strideB;
        void* low_base = l % 2 == 0 ? w->d_A : w->d_B;
        const size_t low_stride = l % 2 == 0 ? w->strideA : w->strideB;
        for (int c0 = 0; c0 < w->C; c0 += kWaveletBatch) {
            g.c0 = c0;
            g.nc = std::min(kWaveletBatch, w->C - c0);
            for (int k = 0; k < g.nc; ++k) {
                const int c = c0 + k;
                g.fine_in[k] = l == 0 ? in[c] : at(src_base, src_stride, c);
                g.coef[k] = out[c];
                g.low[k] = g.low_dense ? (void*)at(low_base, low_stride, c) : out[c];
                g.thr[k] = thr_host ? thr_host[c] : 0.0;
            }
            hipError_t e = launch_wavelet_analysis(g, stream);
            if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a wavelet kernel: ") + hipGetErrorString(e));
        }
    }
    return NUFFT_OK;
}

// Level l (from the deepest up) reads its low-pass corner from the input's corner (deepest) or from the scratch level l + 1 wrote, and
// writes its fine side into the scratch array of its parity (A for odd l: level 1 needs n / 2^D elements), level 0 into the output.
int wavelet_inverse(nufft_wavelet* w, void* const* out, const void* const* in, const WaveletFista* f, const int32_t* flag, hipStream_t stream) {
    for (int l = w->levels - 1; l >= 0; --l) {
        WaveletLevel g = geometry(w, l);
        g.flag = flag;
        g.fine_dense = l > 0;
        g.low_dense = l + 1 < w->levels;
        void* low_base = (l + 1) % 2 == 1 ? w->d_A : w->d_B;
        const size_t low_stride = (l + 1) % 2 == 1 ? w->strideA : w->strideB;
        void* dst_base = l % 2 == 1 ? w->d_A : w->d_B;
        const size_t dst_stride = l % 2 == 1 ? w->strideA : w->strideB;
        if (l == 0 && f && f->momentum) {
            g.momentum = 1;
            g.beta = f->beta;
            g.mom_part = f->mom_part;
            g.G0 = (int)workgroups(g);
        }
        for (int c0 = 0; c0 < w->C; c0 += kWaveletBatch) {
            g.c0 = c0;
            g.nc = std::min(kWaveletBatch, w->C - c0);
            for (int k = 0; k < g.nc; ++k) {
                const int c = c0 + k;
                g.fine_out[k] = l == 0 ? out[c] : at(dst_base, dst_stride, c);
                g.coef[k] = const_cast<void*>(in[c]);
                g.low[k] = g.low_dense ? (void*)at(low_base, low_stride, c) : const_cast<void*>(in[c]);
                g.x[k] = g.momentum ? f->x[c] : nullptr;
            }
            hipError_t e = launch_wavelet_synthesis(g, stream);
            if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a wavelet kernel: ") + hipGetErrorString(e));
        }
    }
    return NUFFT_OK;
}

const double* wavelet_partials(const nufft_wavelet* w, int* P) {
    *P = w->P;
    return static_cast<const double*>(w->d_part);
}

int wavelet_level0_workgroups(const nufft_wavelet* w) { return (int)workgroups(geometry(w, 0)); }

}  // namespace nufft

extern "C" {

int64_t nufft_sizeof_wavelet_params(void) { return (int64_t)sizeof(nufft_wavelet_params); }
int64_t nufft_sizeof_wavelet_info(void) { return (int64_t)sizeof(nufft_wavelet_info); }

int nufft_wavelet_create(nufft_wavelet** out, const nufft_plan* plan, const nufft_wavelet_params* params) {
    if (!out || !plan || !params) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!plan->is_complex)
        return fail(NUFFT_ERR_UNSUPPORTED, "the wavelet transform needs a complex plan: its arrays are those of the Toeplitz normal operator, "
                                           "which a real-data plan cannot have");
    return wavelet_create_geometry(out, plan->dtype, plan->D, plan->N, plan->C, plan->device, params);
}

int nufft_wavelet_create_for_operator(nufft_wavelet** out, const nufft_toeplitz* tz, const nufft_wavelet_params* params) {
    if (!out || !tz || !params) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    nufft_toeplitz_info ti;
    std::memset(&ti, 0, sizeof(ti));
    ti.struct_size = (int32_t)sizeof(ti);
    if (int rc = nufft_toeplitz_get_info(tz, &ti)) return rc;
    return wavelet_create_geometry(out, ti.dtype, ti.ndim, ti.N, ti.ntransforms, ti.device, params);
}

int nufft_wavelet_destroy(nufft_wavelet* w) {
    release(w);
    return NUFFT_OK;
}

int nufft_wavelet_get_info(const nufft_wavelet* w, nufft_wavelet_info* o) {
    if (!w || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    nufft_wavelet_info i;
    std::memset(&i, 0, sizeof(i));
    i.ndim = w->D;
    i.dtype = w->dtype;
    i.ntransforms = w->C;
    i.device = w->device;
    i.wavelet = w->wavelet;
    i.taps = w->taps;
    i.levels = w->levels;
    for (int d = 0; d < 3; ++d) i.N[d] = w->N[d];
    i.scratch_bytes = w->scratch_bytes;
    i.workspace_bytes = w->own_bytes;
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_wavelet_forward(nufft_wavelet* w, void* const* out, const void* const* in, void* stream) {
    if (!w) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (int rc = check_tables(w, out, in)) return rc;
    DeviceGuard guard(w->device);
    return wavelet_forward(w, out, in, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int nufft_wavelet_inverse(nufft_wavelet* w, void* const* out, const void* const* in, void* stream) {
    if (!w) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (int rc = check_tables(w, out, in)) return rc;
    DeviceGuard guard(w->device);
    return wavelet_inverse(w, out, in, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int nufft_wavelet_shrink(nufft_wavelet* w, void* const* out, const void* const* in, const double* t, double* l1_out_device, void* stream) {
    if (!w || !t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (int rc = check_tables(w, out, in)) return rc;
    for (int c = 0; c < w->C; ++c)
        if (!(t[c] >= 0.0) || !std::isfinite(t[c])) return fail(NUFFT_ERR_INVALID_ARG, "thresholds must be finite and not negative");
    DeviceGuard guard(w->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = wavelet_forward(w, out, in, t, nullptr, s)) return rc;
    if (l1_out_device) {
        hipError_t e = launch_wavelet_sum(static_cast<const double*>(w->d_part), w->P, w->C, l1_out_device, s);
        if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a wavelet kernel: ") + hipGetErrorString(e));
    }
    return NUFFT_OK;
}

}  // extern "C"
