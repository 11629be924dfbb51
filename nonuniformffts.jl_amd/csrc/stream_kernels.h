// The toolkit of the streaming kernels (cg_kernels.hip, dcf_kernels.hip; packs, grid rule and launch dispatch also for
// type3_kernels.hip and toeplitz_kernels.hip): 16-byte packs, the fixed-order reduction, the loop shape, the grid rules and the
// float / double launch dispatch.  DESIGN.md section 17 describes the scheme.
//
// The kernels pass over vectors of reals in 16-byte packs (two Float64 or four Float32), grid-stride, two packs per thread and trip.
//
// No workgroup hands anything to another inside a launch and there are no floating-point atomics: a kernel leaves one row of partials
// per workgroup (plain stores), and every workgroup of the NEXT kernel reduces the rows itself, in one fixed order (thread t takes rows
// t, t + 256, ...; then the wave shuffles; then four LDS words).  The kernel boundary is the only synchronisation: it makes the partials
// visible.  The fixed order makes every workgroup, every run and every graph replay get the same bits.  Sums and maxima are FP64 for
// both element types.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <initializer_list>

#include "nufft_mi355x.h"

namespace nufft {
namespace stream {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

template <typename T>
struct alignas(16) Pack {
    static constexpr int W = 16 / sizeof(T);
    T v[W];
};

template <typename T>
__device__ __forceinline__ Pack<T> load(const T* a, int64_t pack) {
    return *reinterpret_cast<const Pack<T>*>(a + pack * Pack<T>::W);
}
template <typename T>
__device__ __forceinline__ void store(T* a, int64_t pack, const Pack<T>& v) {
    *reinterpret_cast<Pack<T>*>(a + pack * Pack<T>::W) = v;
}

struct Sum {
    __device__ static double op(double a, double b) { return a + b; }
};
struct Max {      // fmax: a NaN partial never wins
    __device__ static double op(double a, double b) { return fmax(a, b); }
};

template <typename Op>
__device__ __forceinline__ double wave_reduce(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = Op::op(v, __shfl_down(v, off, 64));
    return v;
}

// Reduction over the workgroup, returned to every thread.  The trailing barrier lets the caller reuse `lds` (kWaves words) at once.
template <typename Op>
__device__ __forceinline__ double block_reduce(double v, double* lds) {
    v = wave_reduce<Op>(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = lds[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t = Op::op(t, lds[w]);
    __syncthreads();
    return t;
}

// Reduction of row[g * pitch], g < G, in the fixed order described at the top (both identities are 0 here: the sums start empty, the
// maxima are of non-negative numbers).
template <typename Op>
__device__ __forceinline__ double row_reduce(const double* row, int G, int pitch, double* lds) {
    double v = 0.0;
    for (int g = threadIdx.x; g < G; g += kThreads) v = Op::op(v, row[(int64_t)g * pitch]);
    return block_reduce<Op>(v, lds);
}

// The loop shape shared by all kernels: the body runs for whole packs i (and i + step__ where that is < npacks__: two packs per trip);
// the reals behind the last whole pack are left to one thread after the loop.
#define NUFFT_FOR_EACH_PACK(T, nreal, i)                                                                     \
    const int64_t npacks__ = (nreal) / nufft::stream::Pack<T>::W;                                            \
    const int64_t step__ = (int64_t)gridDim.x * nufft::stream::kThreads;                                     \
    for (int64_t i = (int64_t)blockIdx.x * nufft::stream::kThreads + threadIdx.x; i < npacks__; i += 2 * step__)

// Workgroups of a NUFFT_FOR_EACH_PACK kernel: two packs per thread and trip, at most 4 workgroups of 4 waves per CU (32 – 128 B in flight
// per thread) and at most `cap`.
inline int stream_workgroups(int64_t packs, int num_cus, int cap = INT_MAX) {
    const int64_t need = (packs + 2 * kThreads - 1) / (2 * kThreads);
    const int64_t most = std::min<int64_t>((int64_t)std::max(num_cus, 1) * 4, cap);
    return (int)std::max<int64_t>(1, std::min(need, most));
}

// Workgroups of a one-pack-per-thread grid-stride kernel (type 3, Toeplitz).
inline unsigned grid_for(int64_t chunks, int num_cus) {
    const int64_t cap = (int64_t)num_cus * 8;      // 8 workgroups of 4 waves per CU: enough bytes in flight for HBM
    const int64_t need = (chunks + kThreads - 1) / kThreads;
    return (unsigned)std::max<int64_t>(1, std::min(need, cap));
}

// Byte counts and offsets of the LDS layouts are whole 16-byte packs.
inline size_t up16(size_t v) { return (v + 15) / 16 * 16; }

// Workgroups above 64 KiB of dynamic LDS must be allowed per kernel (and device): called when an object is created.
inline hipError_t allow_large_lds(std::initializer_list<const void*> kernels) {
    for (const void* k : kernels)
        if (hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 << 10); e != hipSuccess) return e;
    return hipSuccess;
}

// Launches the Float32 or the Float64 instantiation of a kernel; every argument is converted to the parameter type of the kernel that
// runs (void* to T*, and a double to T: for Float32 that narrows it).
template <typename... PF, typename... PD, typename... Args>
hipError_t launch_by_dtype(int dtype, dim3 grid, dim3 block, hipStream_t stream, void (*kernel_f32)(PF...), void (*kernel_f64)(PD...),
                           const Args&... args) {
    static_assert(sizeof...(PF) == sizeof...(Args) && sizeof...(PD) == sizeof...(Args), "one argument per kernel parameter");
    if (dtype == NUFFT_F32) hipLaunchKernelGGL(kernel_f32, grid, block, 0, stream, static_cast<PF>(args)...);
    else hipLaunchKernelGGL(kernel_f64, grid, block, 0, stream, static_cast<PD>(args)...);
    return hipGetLastError();
}

}  // namespace stream
}  // namespace nufft
