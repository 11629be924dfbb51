// The locally low-rank proximal map (include/nufft_mi355x.h, LLR section).
//
// The host side only enqueues: one launch of llr_kernels.hip's kernel for all components and, when the caller wants the nuclear norm, the
// fixed-order sum of the per-workgroup partials.  The object owns those partials and nothing else.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "host_common.h"
#include "llr.h"

using namespace nufft;

struct nufft_llr {
    int dtype = NUFFT_F64, D = 1, C = 1, device = -1;
    int block[3] = {1, 1, 1}, bshift[3] = {0, 0, 0};
    int shifts = 0;
    uint64_t seed = 0;
    int64_t N[3] = {1, 1, 1};
    int64_t n = 1, blocks = 1, G = 1;
    int B = 1;
    void* d_part = nullptr;      // double[G][3]
    int64_t own_bytes = 0;
};

namespace {

void release(nufft_llr* l) {
    if (!l) return;
    if (l->device >= 0 && l->d_part) {
        DeviceGuard g(l->device);
        (void)hipFree(l->d_part);
    }
    delete l;
}

int check_tables(const nufft_llr* l, void* const* out, const void* const* in) {
    return nufft::check_tables(l->C, (size_t)l->n * 2 * real_bytes(l->dtype), out, in, true,
                               "the output overlaps the input: out[c] may be exactly in[c], nothing else");
}

}  // namespace

namespace nufft {

int llr_create_geometry(nufft_llr** out, int dtype, int D, const int64_t* N, int C, int device, const nufft_llr_params* params) {
    nufft_llr_params p;
    if (int rc = read_params(p, params, "nufft_llr_params")) return rc;
    int B = 1;
    for (int d = 0; d < 3; ++d) {
        const int b = p.block[d];
        if (d >= D) {
            if (b != 1 && b != 0) return fail(NUFFT_ERR_INVALID_ARG, "block[" + std::to_string(d) + "] must be 1 beyond the plan's dimensions");
            p.block[d] = 1;
            continue;
        }
        if (b < 1 || b > 16 || (b & (b - 1)) != 0)
            return fail(NUFFT_ERR_INVALID_ARG, "block[" + std::to_string(d) + "] = " + std::to_string(b) + " must be a power of two in 1 ... 16");
        B *= b;
    }
    if (p.shifts != 0 && p.shifts != 1) return fail(NUFFT_ERR_INVALID_ARG, "shifts must be 0 or 1");
    for (int d = 0; d < D; ++d) {
        if (N[d] % p.block[d] != 0)
            return fail(NUFFT_ERR_INVALID_ARG, "N[" + std::to_string(d) + "] = " + std::to_string(N[d]) + " is not a multiple of block[" + std::to_string(d) +
                                                   "] = " + std::to_string(p.block[d]));
        if (N[d] > ((int64_t)1 << 30)) return fail(NUFFT_ERR_UNSUPPORTED, "more than 2^30 cells per axis");
    }
    if (C > kLlrMaxK) return fail(NUFFT_ERR_UNSUPPORTED, "more than " + std::to_string(kLlrMaxK) + " transforms: all components of a block share one workgroup");
    if (B * C > kLlrMaxElems)
        return fail(NUFFT_ERR_UNSUPPORTED, "block cells x ntransforms = " + std::to_string(B * C) + " exceeds the limit of " + std::to_string(kLlrMaxElems) +
                                               " elements a workgroup keeps in LDS");
    if (device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only plan (device = -1): the locally low-rank map runs on the device");

    nufft_llr* l = new (std::nothrow) nufft_llr();
    if (!l) return fail(NUFFT_ERR_ALLOC, "out of host memory");
    l->dtype = dtype;
    l->D = D;
    l->C = C;
    l->device = device;
    l->shifts = p.shifts;
    l->seed = p.seed;
    l->B = B;
    for (int d = 0; d < 3; ++d) {
        l->block[d] = p.block[d];
        while ((1 << l->bshift[d]) < p.block[d]) ++l->bshift[d];
        l->N[d] = d < D ? N[d] : 1;
        l->n *= l->N[d];
        l->blocks *= l->N[d] / l->block[d];
    }
    const int nb = llr_layout(dtype == NUFFT_F32, C, B).nb;
    l->G = (l->blocks + nb - 1) / nb;
    DeviceGuard guard(device);
    if (hipError_t e = llr_allow_lds(); e != hipSuccess) {
        (void)hipGetLastError();
        delete l;
        return fail(NUFFT_ERR_HIP, std::string("hipFuncSetAttribute of the locally low-rank kernels: ") + hipGetErrorString(e));
    }
    if (int rc = alloc_buffer(l->own_bytes, "locally low-rank", &l->d_part, (size_t)l->G * 3 * sizeof(double))) {
        const std::string keep = nufft_last_error_message();
        release(l);
        return fail(rc, keep);
    }
    *out = l;
    return NUFFT_OK;
}

LlrLaunch llr_launch_template(const nufft_llr* l) {
    LlrLaunch a{};
    a.dtype = l->dtype;
    a.D = l->D;
    a.K = l->C;
    a.mode = LLR_PLAIN;
    for (int d = 0; d < 3; ++d) {
        a.bshift[d] = l->bshift[d];
        a.nblk[d] = (int)(l->N[d] / l->block[d]);
        a.N[d] = (int)l->N[d];
    }
    a.pitch[0] = 1;
    a.pitch[1] = l->N[0];
    a.pitch[2] = l->N[0] * l->N[1];
    a.blocks = l->blocks;
    a.part = static_cast<double*>(l->d_part);
    return a;
}

int llr_block_side(const nufft_llr* l, int d) { return l->block[d]; }
int llr_shifts(const nufft_llr* l) { return l->shifts; }
uint64_t llr_seed(const nufft_llr* l) { return l->seed; }

}  // namespace nufft

extern "C" {

int64_t nufft_sizeof_llr_params(void) { return (int64_t)sizeof(nufft_llr_params); }
int64_t nufft_sizeof_llr_info(void) { return (int64_t)sizeof(nufft_llr_info); }

int nufft_llr_create(nufft_llr** out, const nufft_plan* plan, const nufft_llr_params* params) {
    if (!out || !plan || !params) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (params->struct_size > 0 && (size_t)params->struct_size < sizeof(nufft_llr_params))
        return fail(NUFFT_ERR_INVALID_ARG, "nufft_llr_params.struct_size is smaller than the published layout");
    if (!plan->is_complex)
        return fail(NUFFT_ERR_UNSUPPORTED, "the locally low-rank map needs a complex plan: its arrays are those of the Toeplitz normal operator, "
                                           "which a real-data plan cannot have");
    return llr_create_geometry(out, plan->dtype, plan->D, plan->N, plan->C, plan->device, params);
}

int nufft_llr_create_for_operator(nufft_llr** out, const nufft_toeplitz* tz, const nufft_llr_params* params) {
    if (!out || !tz || !params) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    nufft_toeplitz_info ti;
    std::memset(&ti, 0, sizeof(ti));
    ti.struct_size = (int32_t)sizeof(ti);
    if (int rc = nufft_toeplitz_get_info(tz, &ti)) return rc;
    return llr_create_geometry(out, ti.dtype, ti.ndim, ti.N, ti.ntransforms, ti.device, params);
}

int nufft_llr_destroy(nufft_llr* l) {
    release(l);
    return NUFFT_OK;
}

int nufft_llr_get_info(const nufft_llr* l, nufft_llr_info* o) {
    if (!l || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    nufft_llr_info i;
    std::memset(&i, 0, sizeof(i));
    i.ndim = l->D;
    i.dtype = l->dtype;
    i.ntransforms = l->C;
    i.device = l->device;
    i.shifts = l->shifts;
    for (int d = 0; d < 3; ++d) {
        i.block[d] = l->block[d];
        i.N[d] = l->N[d];
    }
    i.blocks = l->blocks;
    i.workspace_bytes = l->own_bytes;
    i.jacobi_sweeps_max = kLlrSweepsMax;
    // 160 KiB of LDS per compute unit, at most 8 workgroups of 4 waves
    const size_t lds = llr_layout(l->dtype == NUFFT_F32, l->C, l->B).bytes;
    i.waves_per_cu = (int)std::min<size_t>(8, (160u << 10) / lds) * (kLlrThreads / 64);
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_llr_apply(nufft_llr* l, void* const* out, const void* const* in, double t, const int32_t* shift, double* nuc_out_device, void* stream_) {
    if (!l) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (int rc = check_tables(l, out, in)) return rc;
    if (!(t >= 0.0) || !std::isfinite(t)) return fail(NUFFT_ERR_INVALID_ARG, "the threshold must be finite and not negative");
    LlrLaunch a = llr_launch_template(l);
    for (int d = 0; d < l->D && shift; ++d) {
        if (shift[d] < 0 || shift[d] >= l->block[d])
            return fail(NUFFT_ERR_INVALID_ARG, "shift[" + std::to_string(d) + "] = " + std::to_string(shift[d]) + " must lie in [0, block[" + std::to_string(d) + "])");
        a.shift[d] = shift[d];
    }
    a.t = t;
    for (int c = 0; c < l->C; ++c) {
        a.in[c] = in[c];
        a.out[c] = out[c];
    }
    DeviceGuard guard(l->device);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipError_t e = launch_llr(a, s);
    if (e == hipSuccess && nuc_out_device) e = launch_llr_sum(a.part, l->G, nuc_out_device, s);
    if (e != hipSuccess) return fail(NUFFT_ERR_HIP, std::string("launch of a locally low-rank kernel: ") + hipGetErrorString(e));
    return NUFFT_OK;
}

}  // extern "C"
