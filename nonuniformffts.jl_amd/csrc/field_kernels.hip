// Kernels of the time-segment fit of a field map (field.h).
//
// range:          FP64 minimum and maximum of ω over the mask and the number of values that are not finite: one row per workgroup, folded
//                 by one workgroup in index order (minimum, maximum and integer counts do not depend on the order anyway).
// histogram:      integer counts, LDS atomics per workgroup, then one global integer atomic per occupied bin: exact in any order.
// interpolators:  one thread per sample, the L accumulators of r = Σ_b h_b exp(i ω_b τ_l) exp(−i ω_b t) in registers.  The bin centres are
//                 equally spaced, so exp(−i ω_b t) is a geometric sequence in b: one sincos for its ratio, one exact sincos at the head of
//                 every piece of kFsReseed bins, a complex multiply per bin in between.  The factor h_b exp(i ω_b τ_l) does not depend
//                 on the sample: the host tabulates it at the fit, a workgroup stages the piece in LDS and every lane reads the same
//                 word (a broadcast).  Per bin and segment that leaves the four FP64 FMAs of one complex multiply-add.
// factors:        streaming, ω read once, L stores per element, one FP64 sincos per stored value.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "field.h"
#include "stream_kernels.h"

namespace nufft {
namespace {

using stream::grid_for;

struct alignas(16) Cd {
    double re, im;
};
template <typename T>
struct alignas(2 * sizeof(T)) Cx {
    T re, im;
};

__device__ __forceinline__ FsRange merge(const FsRange& a, const FsRange& b) {
    return FsRange{fmin(a.lo, b.lo), fmax(a.hi, b.hi), a.bad + b.bad, a.counted + b.counted};
}

// The fold of the workgroup's kFsThreads ranges, left in lds[0]
__device__ __forceinline__ void block_fold(FsRange v, FsRange* lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int half = kFsThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) lds[threadIdx.x] = merge(lds[threadIdx.x], lds[threadIdx.x + half]);
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(kFsThreads) void fs_range_kernel(const T* __restrict__ omega, const uint8_t* __restrict__ mask, int64_t n,
                                                              FsRange* __restrict__ part) {
    __shared__ FsRange lds[kFsThreads];
    FsRange v{INFINITY, -INFINITY, 0ull, 0ull};
    const int64_t step = (int64_t)gridDim.x * kFsThreads;
    for (int64_t i = (int64_t)blockIdx.x * kFsThreads + threadIdx.x; i < n; i += step) {
        if (mask && !mask[i]) continue;
        const double w = (double)omega[i];
        ++v.counted;
        if (isfinite(w)) {
            v.lo = fmin(v.lo, w);
            v.hi = fmax(v.hi, w);
        } else {
            ++v.bad;
        }
    }
    block_fold(v, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = lds[0];
}

__global__ __launch_bounds__(kFsThreads) void fs_range_fold_kernel(const FsRange* __restrict__ part, int G, FsRange* __restrict__ out) {
    __shared__ FsRange lds[kFsThreads];
    FsRange v{INFINITY, -INFINITY, 0ull, 0ull};
    for (int g = threadIdx.x; g < G; g += kFsThreads) v = merge(v, part[g]);
    block_fold(v, lds);
    if (threadIdx.x == 0) out[0] = lds[0];
}

template <typename T>
__global__ __launch_bounds__(kFsThreads) void fs_histogram_kernel(const T* __restrict__ omega, const uint8_t* __restrict__ mask, int64_t n,
                                                                  double lo, double scale, int nb, uint32_t* __restrict__ counts) {
    extern __shared__ uint32_t hist[];
    for (int b = threadIdx.x; b < nb; b += kFsThreads) hist[b] = 0u;
    __syncthreads();
    const int64_t step = (int64_t)gridDim.x * kFsThreads;
    for (int64_t i = (int64_t)blockIdx.x * kFsThreads + threadIdx.x; i < n; i += step) {
        if (mask && !mask[i]) continue;
        const double d = ((double)omega[i] - lo) * scale;
        // (the fit refuses values that are not finite before this kernel runs: d lies in [0, nbins])
        const int bin = min(nb - 1, max(0, (int)d));
        atomicAdd(&hist[bin], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += kFsThreads)
        if (hist[b]) atomicAdd(&counts[b], hist[b]);
}

// LDS: tab [kFsReseed][TIER] complex double, cen [kFsReseed] double, P [TIER][TIER] complex double (rows and columns behind L zero)
template <typename T, int TIER>
__global__ __launch_bounds__(kFsThreads) void fs_interp_kernel(const T* __restrict__ times, int64_t np, int L, int nb,
                                                               const double* __restrict__ table, const double* __restrict__ centres, double delta,
                                                               const double* __restrict__ P, FsPointers phi) {
    extern __shared__ double lds_raw[];
    Cd* tab = reinterpret_cast<Cd*>(lds_raw);
    double* cen = lds_raw + (size_t)kFsReseed * TIER * 2;
    Cd* Pm = reinterpret_cast<Cd*>(cen + kFsReseed);

    const int64_t j = (int64_t)blockIdx.x * kFsThreads + threadIdx.x;
    const bool live = j < np;
    const double t = live ? (double)times[j] : 0.0;

    for (int e = threadIdx.x; e < TIER * TIER; e += kFsThreads) {
        const int r = e / TIER, c = e % TIER;
        Pm[e] = (r < L && c < L) ? Cd{P[2 * (r * L + c)], P[2 * (r * L + c) + 1]} : Cd{0.0, 0.0};
    }

    // the ratio of the sequence: exp(−i Δ t)
    double qs, qc;
    sincos(delta * t, &qs, &qc);
    const Cd q{qc, -qs};

    Cd acc[TIER];
#pragma unroll
    for (int l = 0; l < TIER; ++l) acc[l] = Cd{0.0, 0.0};

    for (int b0 = 0; b0 < nb; b0 += kFsReseed) {
        const int cnt = min(kFsReseed, nb - b0);
        __syncthreads();       // the piece before this one has been read (first trip: nothing to wait for but P's stores)
        for (int e = threadIdx.x; e < cnt * TIER; e += kFsThreads)
            tab[e] = Cd{table[2 * ((size_t)b0 * TIER + e)], table[2 * ((size_t)b0 * TIER + e) + 1]};
        if ((int)threadIdx.x < cnt) cen[threadIdx.x] = centres[b0 + threadIdx.x];
        __syncthreads();
        // the head of the piece, exact: exp(−i ω_b0 t)
        double zs, zc;
        sincos(cen[0] * t, &zs, &zc);
        Cd z{zc, -zs};
        for (int k = 0; k < cnt; ++k) {
#pragma unroll
            for (int l = 0; l < TIER; ++l) {
                const Cd g = tab[k * TIER + l];        // one address for the whole wave: a broadcast
                acc[l].re = fma(g.re, z.re, fma(-g.im, z.im, acc[l].re));
                acc[l].im = fma(g.re, z.im, fma(g.im, z.re, acc[l].im));
            }
            const double zr = z.re * q.re - z.im * q.im;
            z.im = z.re * q.im + z.im * q.re;
            z.re = zr;
        }
    }
    if (!live) return;
    for (int l = 0; l < L; ++l) {
        double re = 0.0, im = 0.0;
#pragma unroll
        for (int m = 0; m < TIER; ++m) {
            const Cd p = Pm[l * TIER + m];
            re = fma(p.re, acc[m].re, fma(-p.im, acc[m].im, re));
            im = fma(p.re, acc[m].im, fma(p.im, acc[m].re, im));
        }
        static_cast<Cx<T>*>(phi.p[l])[j] = Cx<T>{(T)re, (T)im};
    }
}

template <typename T>
__global__ __launch_bounds__(kFsThreads) void fs_factors_kernel(const T* __restrict__ omega, int64_t n, int L, FsTau tau, FsPointers B) {
    const int64_t step = (int64_t)gridDim.x * kFsThreads;
    for (int64_t i = (int64_t)blockIdx.x * kFsThreads + threadIdx.x; i < n; i += step) {
        const double w = (double)omega[i];
        for (int l = 0; l < L; ++l) {
            double s, c;
            sincos(w * tau.v[l], &s, &c);
            static_cast<Cx<T>*>(B.p[l])[i] = Cx<T>{(T)c, (T)(-s)};
        }
    }
}

template <typename T, int TIER>
hipError_t launch_interp_tier(int L, int nb, const void* times, int64_t np, const double* table, const double* centres, double delta,
                              const double* P, const FsPointers& phi, hipStream_t stream) {
    const unsigned grid = (unsigned)((np + kFsThreads - 1) / kFsThreads);
    hipLaunchKernelGGL((fs_interp_kernel<T, TIER>), dim3(grid), dim3(kFsThreads), fieldseg_interp_lds(TIER), stream, static_cast<const T*>(times), np, L,
                       nb, table, centres, delta, P, phi);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_interp_t(int L, int nb, const void* times, int64_t np, const double* table, const double* centres, double delta, const double* P,
                           const FsPointers& phi, hipStream_t stream) {
    switch (fieldseg_tier(L)) {
        case 1: return launch_interp_tier<T, 1>(L, nb, times, np, table, centres, delta, P, phi, stream);
        case 2: return launch_interp_tier<T, 2>(L, nb, times, np, table, centres, delta, P, phi, stream);
        case 4: return launch_interp_tier<T, 4>(L, nb, times, np, table, centres, delta, P, phi, stream);
        case 8: return launch_interp_tier<T, 8>(L, nb, times, np, table, centres, delta, P, phi, stream);
        default: return launch_interp_tier<T, 16>(L, nb, times, np, table, centres, delta, P, phi, stream);
    }
}

}  // namespace

hipError_t launch_fieldseg_range(int dtype, const void* omega, const uint8_t* mask, int64_t n, FsRange* part, FsRange* out, int num_cus,
                                 hipStream_t stream) {
    const int G = (int)std::min<int64_t>(kFsMaxGroups, std::min<int64_t>((n + kFsThreads - 1) / kFsThreads, (int64_t)std::max(num_cus, 1)));
    if (dtype == NUFFT_F32)
        hipLaunchKernelGGL(fs_range_kernel<float>, dim3(G), dim3(kFsThreads), 0, stream, static_cast<const float*>(omega), mask, n, part);
    else
        hipLaunchKernelGGL(fs_range_kernel<double>, dim3(G), dim3(kFsThreads), 0, stream, static_cast<const double*>(omega), mask, n, part);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(fs_range_fold_kernel, dim3(1), dim3(kFsThreads), 0, stream, part, G, out);
    return hipGetLastError();
}

hipError_t launch_fieldseg_histogram(int dtype, const void* omega, const uint8_t* mask, int64_t n, double lo, double scale, int nb,
                                     uint32_t* counts, int num_cus, hipStream_t stream) {
    const unsigned grid = grid_for(n, num_cus);
    if (dtype == NUFFT_F32)
        hipLaunchKernelGGL(fs_histogram_kernel<float>, dim3(grid), dim3(kFsThreads), fieldseg_hist_lds(nb), stream, static_cast<const float*>(omega),
                           mask, n, lo, scale, nb, counts);
    else
        hipLaunchKernelGGL(fs_histogram_kernel<double>, dim3(grid), dim3(kFsThreads), fieldseg_hist_lds(nb), stream, static_cast<const double*>(omega),
                           mask, n, lo, scale, nb, counts);
    return hipGetLastError();
}

hipError_t launch_fieldseg_interpolators(int dtype, int L, int nb, const void* times, int64_t np, const double* table, const double* centres,
                                         double delta, const double* P, const FsPointers& phi, hipStream_t stream) {
    return dtype == NUFFT_F32 ? launch_interp_t<float>(L, nb, times, np, table, centres, delta, P, phi, stream)
                              : launch_interp_t<double>(L, nb, times, np, table, centres, delta, P, phi, stream);
}

hipError_t launch_fieldseg_factors(int dtype, int L, const void* omega, int64_t n, const FsTau& tau, const FsPointers& B, int num_cus,
                                   hipStream_t stream) {
    const unsigned grid = grid_for(n, num_cus);
    if (dtype == NUFFT_F32)
        hipLaunchKernelGGL(fs_factors_kernel<float>, dim3(grid), dim3(kFsThreads), 0, stream, static_cast<const float*>(omega), n, L, tau, B);
    else
        hipLaunchKernelGGL(fs_factors_kernel<double>, dim3(grid), dim3(kFsThreads), 0, stream, static_cast<const double*>(omega), n, L, tau, B);
    return hipGetLastError();
}

}  // namespace nufft
