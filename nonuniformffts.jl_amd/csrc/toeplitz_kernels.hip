// Streaming kernels of the Toeplitz normal operator (toeplitz.cpp): the pad / multiply / crop of the dense
// apply, and the two passes around the dense transform that builds the multiplier K (load with the Nyquist planes zeroed, real
// part with the normalisation), plus the real-to-complex copy of the weights.
//
// All of them are HBM-bound and in the style of type3_kernels.hip: a thread moves whole 16-byte packs of the embedding grid (one
// ComplexF64 or two ComplexF32 cells; rows of 2 N_1 cells are even, so a pack never crosses a row), grid-stride loops over a grid
// sized to the device.  The gathers through the index maps (pad, crop) touch the caller's array element by element.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "nufft_mi355x.h"
#include "stream_kernels.h"
#include "toeplitz.h"

namespace nufft {
using namespace stream;
namespace {

int64_t cells(const TzGrid& g) { return (int64_t)g.n2[0] * g.n2[1] * g.n2[2]; }

// MODE 0: grid = zero-padded û (gather through inv);  MODE 1: grid = T with the Nyquist planes zeroed
template <typename T, int MODE>
__global__ __launch_bounds__(kThreads) void tz_fill_kernel(TzGrid g, T* grid, const T* src, int64_t npacks) {
    constexpr int CW = Pack<T>::W / 2;          // cells per pack
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < npacks; q += (int64_t)gridDim.x * kThreads) {
        const int64_t cell = q * CW;
        const int j1 = (int)(cell % g.n2[0]);
        const int64_t r = cell / g.n2[0];
        const int j2 = (int)(r % g.n2[1]), j3 = (int)(r / g.n2[1]);
        Pack<T> pk;
        if (MODE == 0) {
            const int k2 = g.inv[1][j2], k3 = g.inv[2][j3];
#pragma unroll
            for (int w = 0; w < CW; ++w) {
                const int k1 = g.inv[0][j1 + w];
                T re = T(0), im = T(0);
                if (k1 >= 0 && k2 >= 0 && k3 >= 0) {
                    const int64_t s = k1 + (int64_t)g.nk[0] * (k2 + (int64_t)g.nk[1] * k3);
                    re = src[2 * s];
                    im = src[2 * s + 1];
                }
                pk.v[2 * w] = re;
                pk.v[2 * w + 1] = im;
            }
        } else {
            pk = *reinterpret_cast<const Pack<T>*>(src + 2 * cell);
            const bool nyq23 = (g.D > 1 && j2 == g.nk[1]) || (g.D > 2 && j3 == g.nk[2]);
#pragma unroll
            for (int w = 0; w < CW; ++w) {
                if (nyq23 || j1 + w == g.nk[0]) { pk.v[2 * w] = T(0); pk.v[2 * w + 1] = T(0); }
            }
        }
        *reinterpret_cast<Pack<T>*>(grid + 2 * cell) = pk;
    }
}

// MODE 0: grid *= K;  MODE 1: K = scale * Re(grid)
template <typename T, int MODE>
__global__ __launch_bounds__(kThreads) void tz_real_kernel(T* grid, T* K, T scale, int64_t npacks) {
    constexpr int CW = Pack<T>::W / 2;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < npacks; q += (int64_t)gridDim.x * kThreads) {
        const int64_t cell = q * CW;
        Pack<T> pk = *reinterpret_cast<const Pack<T>*>(grid + 2 * cell);
        if (MODE == 0) {
#pragma unroll
            for (int w = 0; w < CW; ++w) {
                const T k = K[cell + w];
                pk.v[2 * w] *= k;
                pk.v[2 * w + 1] *= k;
            }
            *reinterpret_cast<Pack<T>*>(grid + 2 * cell) = pk;
        } else {
#pragma unroll
            for (int w = 0; w < CW; ++w) K[cell + w] = scale * pk.v[2 * w];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void tz_crop_kernel(TzGrid g, T* out, const T* grid, int64_t nmodes) {
    typedef T T2 __attribute__((ext_vector_type(2)));
    for (int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x; s < nmodes; s += (int64_t)gridDim.x * kThreads) {
        const int k1 = (int)(s % g.nk[0]);
        const int64_t r = s / g.nk[0];
        const int k2 = (int)(r % g.nk[1]), k3 = (int)(r / g.nk[1]);
        const int64_t cell = g.map[0][k1] + (int64_t)g.n2[0] * (g.map[1][k2] + (int64_t)g.n2[1] * g.map[2][k3]);
        reinterpret_cast<T2*>(out)[s] = reinterpret_cast<const T2*>(grid)[cell];
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void tz_weights_kernel(T* values, const T* weights, int64_t n) {
    typedef T T2 __attribute__((ext_vector_type(2)));
    for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kThreads) {
        T2 v;
        v.x = weights ? weights[j] : T(1);
        v.y = T(0);
        reinterpret_cast<T2*>(values)[j] = v;
    }
}

int64_t packs(const TzGrid& g) { return cells(g) / (g.dtype == NUFFT_F32 ? 2 : 1); }

}  // namespace

hipError_t launch_tz_pad(const TzGrid& g, void* grid, const void* u, int num_cus, hipStream_t stream) {
    const int64_t np = packs(g);
    return launch_by_dtype(g.dtype, dim3(grid_for(np, num_cus)), dim3(kThreads), stream, tz_fill_kernel<float, 0>, tz_fill_kernel<double, 0>, g, grid, u, np);
}

hipError_t launch_tz_spectrum_load(const TzGrid& g, void* grid, const void* T_modes, int num_cus, hipStream_t stream) {
    const int64_t np = packs(g);
    return launch_by_dtype(g.dtype, dim3(grid_for(np, num_cus)), dim3(kThreads), stream, tz_fill_kernel<float, 1>, tz_fill_kernel<double, 1>, g, grid, T_modes,
                           np);
}

hipError_t launch_tz_multiply(const TzGrid& g, void* grid, const void* K, int num_cus, hipStream_t stream) {
    const int64_t np = packs(g);
    // the scale is a T in the kernel: launch_by_dtype narrows the double for Float32 (1.0 is exact)
    return launch_by_dtype(g.dtype, dim3(grid_for(np, num_cus)), dim3(kThreads), stream, tz_real_kernel<float, 0>, tz_real_kernel<double, 0>, grid,
                           const_cast<void*>(K), 1.0, np);
}

hipError_t launch_tz_real_part(const TzGrid& g, void* K, const void* grid, double scale, int num_cus, hipStream_t stream) {
    const int64_t np = packs(g);
    // `scale` is rounded to Float32 for the Float32 kernel, as (float)scale
    return launch_by_dtype(g.dtype, dim3(grid_for(np, num_cus)), dim3(kThreads), stream, tz_real_kernel<float, 1>, tz_real_kernel<double, 1>,
                           const_cast<void*>(grid), K, scale, np);
}

hipError_t launch_tz_crop(const TzGrid& g, void* out, const void* grid, int num_cus, hipStream_t stream) {
    const int64_t nm = (int64_t)g.nk[0] * g.nk[1] * g.nk[2];
    return launch_by_dtype(g.dtype, dim3(grid_for(nm, num_cus)), dim3(kThreads), stream, tz_crop_kernel<float>, tz_crop_kernel<double>, g, out, grid, nm);
}

hipError_t launch_tz_weights(int dtype, void* values, const void* weights, int64_t n, int num_cus, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    return launch_by_dtype(dtype, dim3(grid_for(n, num_cus)), dim3(kThreads), stream, tz_weights_kernel<float>, tz_weights_kernel<double>, values, weights, n);
}

}  // namespace nufft
