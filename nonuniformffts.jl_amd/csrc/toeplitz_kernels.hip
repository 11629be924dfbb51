// Streaming kernels of the Toeplitz normal operator (toeplitz.cpp): the pad / multiply / crop of the dense
// apply, and the two passes around the dense transform that builds the multiplier K (load with the Nyquist planes zeroed, real
// part with the normalisation), plus the real-to-complex copy of the weights, and the coil passes of the multi-coil operator
// (DESIGN.md section 19): the pad and crop with a sensitivity map, and coil expand / combine over whole arrays.
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

// MODE 0: grid = zero-padded û (gather through inv);  MODE 1: grid = T with the Nyquist planes zeroed;
// MODE 2: grid = zero-padded S ⊙ û (smap: the coil's sensitivity map, laid out like û)
template <typename T, int MODE>
__global__ __launch_bounds__(kThreads) void tz_fill_kernel(TzGrid g, T* grid, const T* src, int64_t npacks, const T* smap) {
    constexpr int CW = Pack<T>::W / 2;          // cells per pack
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < npacks; q += (int64_t)gridDim.x * kThreads) {
        const int64_t cell = q * CW;
        const int j1 = (int)(cell % g.n2[0]);
        const int64_t r = cell / g.n2[0];
        const int j2 = (int)(r % g.n2[1]), j3 = (int)(r / g.n2[1]);
        Pack<T> pk;
        if (MODE == 0 || MODE == 2) {
            const int k2 = g.inv[1][j2], k3 = g.inv[2][j3];
#pragma unroll
            for (int w = 0; w < CW; ++w) {
                const int k1 = g.inv[0][j1 + w];
                T re = T(0), im = T(0);
                if (k1 >= 0 && k2 >= 0 && k3 >= 0) {
                    const int64_t s = k1 + (int64_t)g.nk[0] * (k2 + (int64_t)g.nk[1] * k3);
                    re = src[2 * s];
                    im = src[2 * s + 1];
                    if constexpr (MODE == 2) {
                        const T sr = smap[2 * s], si = smap[2 * s + 1];
                        const T pr = re * sr - im * si;
                        im = re * si + im * sr;
                        re = pr;
                    }
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

// SMAP: out = conj(S) ⊙ (grid at the kept modes), added to what out holds when `accumulate`
template <typename T, bool SMAP>
__global__ __launch_bounds__(kThreads) void tz_crop_kernel(TzGrid g, T* out, const T* grid, int64_t nmodes, const T* smap, int accumulate) {
    typedef T T2 __attribute__((ext_vector_type(2)));
    for (int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x; s < nmodes; s += (int64_t)gridDim.x * kThreads) {
        const int k1 = (int)(s % g.nk[0]);
        const int64_t r = s / g.nk[0];
        const int k2 = (int)(r % g.nk[1]), k3 = (int)(r / g.nk[1]);
        const int64_t cell = g.map[0][k1] + (int64_t)g.n2[0] * (g.map[1][k2] + (int64_t)g.n2[1] * g.map[2][k3]);
        if constexpr (SMAP) {
            const T2 v = reinterpret_cast<const T2*>(grid)[cell], m = reinterpret_cast<const T2*>(smap)[s];
            T2 r;
            r.x = v.x * m.x + v.y * m.y;
            r.y = v.y * m.x - v.x * m.y;
            if (accumulate) {
                const T2 o = reinterpret_cast<const T2*>(out)[s];
                r.x = o.x + r.x;
                r.y = o.y + r.y;
            }
            reinterpret_cast<T2*>(out)[s] = r;
        } else {
            reinterpret_cast<T2*>(out)[s] = reinterpret_cast<const T2*>(grid)[cell];
        }
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

// Coupled components.  values[j] = w_j conj(φ_a(j)) φ_b(j): the weights of the type 1 that builds T_ab.
// The complex arrays pass as 2n reals in 16-byte packs, two per thread and trip; the weights are read element by element.
template <typename T>
__global__ __launch_bounds__(kThreads) void tz_pair_weights_kernel(T* values, const T* weights, const T* pa, const T* pb, int64_t n) {
    constexpr int W = Pack<T>::W, CW = W / 2;
    auto one = [&](T ar, T ai, T br, T bi, int64_t j, T& re, T& im) {
        const T w = weights ? weights[j] : T(1);
        re = w * (ar * br + ai * bi);
        im = w * (ar * bi - ai * br);
    };
    auto pack = [&](int64_t i) {
        const Pack<T> a = load(pa, i), b = load(pb, i);
        Pack<T> r;
#pragma unroll
        for (int w = 0; w < CW; ++w) one(a.v[2 * w], a.v[2 * w + 1], b.v[2 * w], b.v[2 * w + 1], i * CW + w, r.v[2 * w], r.v[2 * w + 1]);
        store(values, i, r);
    };
    NUFFT_FOR_EACH_PACK(T, 2 * n, i) {
        pack(i);
        if (i + step__ < npacks__) pack(i + step__);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t j = npacks__ * CW; j < n; ++j) one(pa[2 * j], pa[2 * j + 1], pb[2 * j], pb[2 * j + 1], j, values[2 * j], values[2 * j + 1]);
}

// Kc = scale * grid (complex): the multiplier of a pair a < b, the sibling of tz_real_kernel's MODE 1
template <typename T>
__global__ __launch_bounds__(kThreads) void tz_complex_part_kernel(const T* grid, T* K, T scale, int64_t npacks) {
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < npacks; q += (int64_t)gridDim.x * kThreads) {
        Pack<T> pk = load(grid, q);
#pragma unroll
        for (int w = 0; w < Pack<T>::W; ++w) pk.v[w] *= scale;
        store(K, q, pk);
    }
}

// grids[a] = Σ_b K_ab ⊙ grids[b] per cell, in place: a thread holds the K packs of its cells, so every grid and every multiplier
// grid is read once.  KT: the compile-time bound of the run-time K (the register arrays).  kd: T[K][cells]; kc: complex<T>[pairs a < b,
// row-major][cells]; the pair (b, a), b < a, applies conjugated.
template <typename T, int KT>
__global__ __launch_bounds__(kThreads) void tz_multiply_coupled_kernel(T* grids, int64_t stride, int K, const T* kd, const T* kc, int64_t ncells,
                                                                       int64_t npacks) {
    constexpr int CW = Pack<T>::W / 2;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < npacks; q += (int64_t)gridDim.x * kThreads) {
        const int64_t cell = q * CW;
        Pack<T> v[KT], acc[KT];
#pragma unroll
        for (int a = 0; a < KT; ++a) {
            if (a < K) {
                v[a] = load(grids + a * stride, q);
#pragma unroll
                for (int w = 0; w < CW; ++w) {
                    const T d = kd[a * ncells + cell + w];
                    acc[a].v[2 * w] = d * v[a].v[2 * w];
                    acc[a].v[2 * w + 1] = d * v[a].v[2 * w + 1];
                }
            }
        }
#pragma unroll
        for (int a = 0; a < KT; ++a) {
#pragma unroll
            for (int b = a + 1; b < KT; ++b) {
                if (b < K) {
                    const Pack<T> k = load(kc + 2 * (int64_t)(a * (K - 1) - a * (a - 1) / 2 + (b - a - 1)) * ncells, q);
#pragma unroll
                    for (int w = 0; w < CW; ++w) {
                        const T kr = k.v[2 * w], ki = k.v[2 * w + 1];
                        acc[a].v[2 * w] += kr * v[b].v[2 * w] - ki * v[b].v[2 * w + 1];
                        acc[a].v[2 * w + 1] += kr * v[b].v[2 * w + 1] + ki * v[b].v[2 * w];
                        acc[b].v[2 * w] += kr * v[a].v[2 * w] + ki * v[a].v[2 * w + 1];
                        acc[b].v[2 * w + 1] += kr * v[a].v[2 * w + 1] - ki * v[a].v[2 * w];
                    }
                }
            }
        }
#pragma unroll
        for (int a = 0; a < KT; ++a)
            if (a < K) store(grids + a * stride, q, acc[a]);
    }
}

int64_t packs(const TzGrid& g) { return cells(g) / (g.dtype == NUFFT_F32 ? 2 : 1); }

// Coil expand (EXPAND: data[c] = S_c ⊙ x for every coil of the table) and combine (y = Σ_c conj(S_c) ⊙ data[c], summed in coil order in
// registers, started from what y holds when `accumulate`), over n complex elements in 16-byte packs; the ComplexF32 element behind the
// last pack of an odd n is left to one thread.  Each array is read once and written once per launch.
template <typename T, bool EXPAND>
__global__ __launch_bounds__(kThreads) void coil_kernel(CoilTable tab, int ncoils, T* y, const T* x, int64_t n, int accumulate) {
    constexpr int CW = Pack<T>::W / 2;          // elements per pack
    const int64_t npacks = n / CW;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < npacks; q += (int64_t)gridDim.x * kThreads) {
        if constexpr (EXPAND) {
            const Pack<T> v = load(x, q);
            for (int c = 0; c < ncoils; ++c) {
                const Pack<T> m = load(static_cast<const T*>(tab.maps[c]), q);
                Pack<T> r;
#pragma unroll
                for (int w = 0; w < CW; ++w) {
                    r.v[2 * w] = v.v[2 * w] * m.v[2 * w] - v.v[2 * w + 1] * m.v[2 * w + 1];
                    r.v[2 * w + 1] = v.v[2 * w] * m.v[2 * w + 1] + v.v[2 * w + 1] * m.v[2 * w];
                }
                store(static_cast<T*>(tab.data[c]), q, r);
            }
        } else {
            Pack<T> acc;
#pragma unroll
            for (int w = 0; w < 2 * CW; ++w) acc.v[w] = T(0);
            if (accumulate) acc = load(static_cast<const T*>(y), q);
            for (int c = 0; c < ncoils; ++c) {
                const Pack<T> m = load(static_cast<const T*>(tab.maps[c]), q);
                const Pack<T> v = load(static_cast<const T*>(tab.data[c]), q);
#pragma unroll
                for (int w = 0; w < CW; ++w) {
                    acc.v[2 * w] += v.v[2 * w] * m.v[2 * w] + v.v[2 * w + 1] * m.v[2 * w + 1];
                    acc.v[2 * w + 1] += v.v[2 * w + 1] * m.v[2 * w] - v.v[2 * w] * m.v[2 * w + 1];
                }
            }
            store(y, q, acc);
        }
    }
    if (CW > 1 && (n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t e = 2 * (n - 1);
        if constexpr (EXPAND) {
            const T vr = x[e], vi = x[e + 1];
            for (int c = 0; c < ncoils; ++c) {
                const T* m = static_cast<const T*>(tab.maps[c]);
                T* d = static_cast<T*>(tab.data[c]);
                d[e] = vr * m[e] - vi * m[e + 1];
                d[e + 1] = vr * m[e + 1] + vi * m[e];
            }
        } else {
            T ar = T(0), ai = T(0);
            if (accumulate) { ar = y[e]; ai = y[e + 1]; }
            for (int c = 0; c < ncoils; ++c) {
                const T* m = static_cast<const T*>(tab.maps[c]);
                const T* d = static_cast<const T*>(tab.data[c]);
                ar += d[e] * m[e] + d[e + 1] * m[e + 1];
                ai += d[e + 1] * m[e] - d[e] * m[e + 1];
            }
            y[e] = ar;
            y[e + 1] = ai;
        }
    }
}

}  // namespace

hipError_t launch_tz_pad(const TzGrid& g, void* grid, const void* u, int num_cus, hipStream_t stream) {
    const int64_t np = packs(g);
    return launch_by_dtype(g.dtype, dim3(grid_for(np, num_cus)), dim3(kThreads), stream, tz_fill_kernel<float, 0>, tz_fill_kernel<double, 0>, g, grid, u, np,
                           nullptr);
}

hipError_t launch_tz_pad_map(const TzGrid& g, void* grid, const void* u, const void* smap, int num_cus, hipStream_t stream) {
    const int64_t np = packs(g);
    return launch_by_dtype(g.dtype, dim3(grid_for(np, num_cus)), dim3(kThreads), stream, tz_fill_kernel<float, 2>, tz_fill_kernel<double, 2>, g, grid, u, np,
                           smap);
}

hipError_t launch_tz_spectrum_load(const TzGrid& g, void* grid, const void* T_modes, int num_cus, hipStream_t stream) {
    const int64_t np = packs(g);
    return launch_by_dtype(g.dtype, dim3(grid_for(np, num_cus)), dim3(kThreads), stream, tz_fill_kernel<float, 1>, tz_fill_kernel<double, 1>, g, grid, T_modes,
                           np, nullptr);
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
    return launch_by_dtype(g.dtype, dim3(grid_for(nm, num_cus)), dim3(kThreads), stream, tz_crop_kernel<float, false>, tz_crop_kernel<double, false>, g, out, grid,
                           nm, nullptr, 0);
}

hipError_t launch_tz_crop_map(const TzGrid& g, void* out, const void* grid, const void* smap, bool accumulate, int num_cus, hipStream_t stream) {
    const int64_t nm = (int64_t)g.nk[0] * g.nk[1] * g.nk[2];
    return launch_by_dtype(g.dtype, dim3(grid_for(nm, num_cus)), dim3(kThreads), stream, tz_crop_kernel<float, true>, tz_crop_kernel<double, true>, g, out, grid,
                           nm, smap, accumulate ? 1 : 0);
}

hipError_t launch_coil_expand(int dtype, int64_t n, int ncoils, void* const* out, const void* const* maps, const void* in, int num_cus,
                              hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int64_t np = n / (dtype == NUFFT_F32 ? 2 : 1);
    for (int c0 = 0; c0 < ncoils; c0 += kCoilChunk) {
        CoilTable tab{};
        const int nc = std::min(kCoilChunk, ncoils - c0);
        for (int c = 0; c < nc; ++c) { tab.maps[c] = maps[c0 + c]; tab.data[c] = out[c0 + c]; }
        hipError_t e = launch_by_dtype(dtype, dim3(grid_for(np, num_cus)), dim3(kThreads), stream, coil_kernel<float, true>, coil_kernel<double, true>, tab, nc,
                                       nullptr, in, n, 0);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_coil_combine(int dtype, int64_t n, int ncoils, void* out, const void* const* maps, const void* const* in, bool accumulate,
                               int num_cus, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int64_t np = n / (dtype == NUFFT_F32 ? 2 : 1);
    for (int c0 = 0; c0 < ncoils; c0 += kCoilChunk) {
        CoilTable tab{};
        const int nc = std::min(kCoilChunk, ncoils - c0);
        for (int c = 0; c < nc; ++c) { tab.maps[c] = maps[c0 + c]; tab.data[c] = const_cast<void*>(in[c0 + c]); }
        hipError_t e = launch_by_dtype(dtype, dim3(grid_for(np, num_cus)), dim3(kThreads), stream, coil_kernel<float, false>, coil_kernel<double, false>, tab,
                                       nc, out, nullptr, n, (accumulate || c0 > 0) ? 1 : 0);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_tz_pair_weights(int dtype, void* values, const void* weights, const void* phi_a, const void* phi_b, int64_t n, int num_cus,
                                  hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int64_t np = (2 * n) / (dtype == NUFFT_F32 ? 4 : 2);
    return launch_by_dtype(dtype, dim3(stream_workgroups(np, num_cus)), dim3(kThreads), stream, tz_pair_weights_kernel<float>,
                           tz_pair_weights_kernel<double>, values, weights, phi_a, phi_b, n);
}

hipError_t launch_tz_complex_part(const TzGrid& g, void* Kc, const void* grid, double scale, int num_cus, hipStream_t stream) {
    const int64_t np = packs(g);
    return launch_by_dtype(g.dtype, dim3(grid_for(np, num_cus)), dim3(kThreads), stream, tz_complex_part_kernel<float>, tz_complex_part_kernel<double>,
                           grid, Kc, scale, np);
}

hipError_t launch_tz_multiply_coupled(const TzGrid& g, void* grids, int64_t grid_stride, int K, const void* kd, const void* kc, int num_cus,
                                      hipStream_t stream) {
    if (K < 1 || K > kMaxCoupled) return hipErrorInvalidValue;
    const int64_t np = packs(g), nc = cells(g), stride = 2 * grid_stride;
    const dim3 gr(grid_for(np, num_cus)), bl(kThreads);
    if (K <= 2) return launch_by_dtype(g.dtype, gr, bl, stream, tz_multiply_coupled_kernel<float, 2>, tz_multiply_coupled_kernel<double, 2>, grids, stride, K, kd, kc, nc, np);
    if (K <= 4) return launch_by_dtype(g.dtype, gr, bl, stream, tz_multiply_coupled_kernel<float, 4>, tz_multiply_coupled_kernel<double, 4>, grids, stride, K, kd, kc, nc, np);
    if (K <= 8) return launch_by_dtype(g.dtype, gr, bl, stream, tz_multiply_coupled_kernel<float, 8>, tz_multiply_coupled_kernel<double, 8>, grids, stride, K, kd, kc, nc, np);
    return launch_by_dtype(g.dtype, gr, bl, stream, tz_multiply_coupled_kernel<float, 16>, tz_multiply_coupled_kernel<double, 16>, grids, stride, K, kd, kc, nc, np);
}

hipError_t launch_tz_weights(int dtype, void* values, const void* weights, int64_t n, int num_cus, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    return launch_by_dtype(dtype, dim3(grid_for(n, num_cus)), dim3(kThreads), stream, tz_weights_kernel<float>, tz_weights_kernel<double>, values, weights, n);
}

}  // namespace nufft
