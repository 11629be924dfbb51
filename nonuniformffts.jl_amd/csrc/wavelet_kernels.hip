// Kernels of the periodic orthogonal wavelet transform (wavelet.cpp).
//
// One launch per level handles all D dimensions: a workgroup owns a tile of to[d] coarse positions per dimension, loads the fine cells
// it needs (analysis: 2 to[d] + taps − 2 per dimension, the halo wrapping periodically; synthesis: to[d] + taps / 2 − 1 coefficients per
// band and dimension) into LDS once, runs the D one-dimensional filter passes between two LDS buffers and stores every result once.
// All loads wrap (index mod the sub-box side), so sub-boxes smaller than a tile and sides that are no multiple of the tile need no
// special case: the stores are masked instead.
//
// Analysis:   lo[i] = Σ_k h[k] a[(2i + k) mod n],  hi[i] = Σ_k g[k] a[(2i + k) mod n],  g[k] = (−1)^k h[L − 1 − k]
// Synthesis:  a[j] = Σ_{2i + k ≡ j} h[k] lo[i] + g[k] hi[i]      (the transpose: the transform is orthogonal)
//
// The detail bands of a level are final when the level stores them: the soft threshold of `shrink` (and the partial sum of what it
// leaves) and, in the last synthesis level of a FISTA iteration, the momentum step with its two partial sums, ride on those stores.
// Partial sums go through stream_kernels.h: one plain store per workgroup, reduced later in one fixed order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "stream_kernels.h"
#include "wavelet.h"

namespace nufft {
using namespace stream;

extern __shared__ __align__(16) unsigned char wavelet_lds[];      // the two tile buffers (wavelet_lds_bytes)

namespace {

static_assert(kWaveletThreads == kThreads, "the reduction helpers assume their own workgroup size");

template <typename T>
struct alignas(2 * sizeof(T)) Cx {
    T re, im;
};

// h and g of the 2-tap (Haar) and 4-tap (Daubechies, two vanishing moments) filters: FP64 constants cast to T
template <typename T, int TAPS>
__device__ __forceinline__ void filters(T* h, T* g) {
    if (TAPS == 2) {
        h[0] = (T)0.70710678118654752440;
        h[1] = (T)0.70710678118654752440;
    } else {
        h[0] = (T)0.48296291314453414337;       // (1 + √3) / (4 √2)
        h[1] = (T)0.83651630373780790558;       // (3 + √3) / (4 √2)
        h[2] = (T)0.22414386804201338103;       // (3 − √3) / (4 √2)
        h[3] = (T)-0.12940952255126038117;      // (1 − √3) / (4 √2)
    }
#pragma unroll
    for (int k = 0; k < TAPS; ++k) g[k] = (k & 1) ? -h[TAPS - 1 - k] : h[TAPS - 1 - k];
}

// i mod n for i >= −1: the tile's indices leave [0, n) rarely, and by more than n only where the box is smaller than the tile
__device__ __forceinline__ int wrap(int i, int n) {
    if (i < 0) i += n;
    return i >= n ? i % n : i;
}

// The tile of this (element type, D): every extent below is a compile-time constant, so the index arithmetic is shifts and multiplies.
template <typename T, int D>
struct TileOf {
    static constexpr bool F32 = sizeof(T) == 4;
    static constexpr int TO0 = wavelet_tile(F32, D, 0), TO1 = wavelet_tile(F32, D, 1), TO2 = wavelet_tile(F32, D, 2);
};

struct Tile {
    int c, o0[3];
};

template <typename T, int D>
__device__ __forceinline__ Tile tile_of(const WaveletLevel& a) {
    using TL = TileOf<T, D>;
    Tile t;
    t.c = a.c0 + blockIdx.y;
    int b = blockIdx.x;
    t.o0[0] = (b % a.tiles[0]) * TL::TO0;
    b /= a.tiles[0];
    t.o0[1] = (b % a.tiles[1]) * TL::TO1;
    t.o0[2] = (b / a.tiles[1]) * TL::TO2;
    return t;
}

// One analysis pass along AXIS: extents (X0, X1, X2) -> the same with the extent of AXIS replaced by 2 TO (lo at [0, TO), hi at [TO, 2 TO))
template <typename T, int TAPS, int AXIS, int X0, int X1, int X2, int TO>
__device__ __forceinline__ void analysis_pass(const Cx<T>* src, Cx<T>* dst, const T* h, const T* g) {
    constexpr int SIN[3] = {1, X0, X0 * X1};
    constexpr int I0 = AXIS == 0 ? TO : X0, I1 = AXIS == 1 ? TO : X1, I2 = AXIS == 2 ? TO : X2;
    constexpr int Y0 = AXIS == 0 ? 2 * TO : X0, Y1 = AXIS == 1 ? 2 * TO : X1;
    constexpr int SOUT[3] = {1, Y0, Y0 * Y1};
    constexpr int ITEMS = I0 * I1 * I2;
    for (int it = threadIdx.x; it < ITEMS; it += kThreads) {
        int i[3] = {it % I0, (it / I0) % I1, it / (I0 * I1)};
        const int ob = i[0] * SOUT[0] + i[1] * SOUT[1] + i[2] * SOUT[2];
        i[AXIS] *= 2;
        const int ib = i[0] * SIN[0] + i[1] * SIN[1] + i[2] * SIN[2];
        T lr = 0, li = 0, hr = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
            const Cx<T> v = src[ib + k * SIN[AXIS]];
            lr += h[k] * v.re;
            li += h[k] * v.im;
            hr += g[k] * v.re;
            hi += g[k] * v.im;
        }
        dst[ob] = Cx<T>{lr, li};
        dst[ob + TO * SOUT[AXIS]] = Cx<T>{hr, hi};
    }
}

template <typename T, int TAPS, int D>
__global__ __launch_bounds__(kThreads) void wavelet_analysis_kernel(WaveletLevel a) {
    using TL = TileOf<T, D>;
    constexpr int TO[3] = {TL::TO0, TL::TO1, TL::TO2};
    constexpr int E0 = 2 * TL::TO0 + TAPS - 2, E1 = D >= 2 ? 2 * TL::TO1 + TAPS - 2 : 1, E2 = D >= 3 ? 2 * TL::TO2 + TAPS - 2 : 1;
    constexpr int F0 = 2 * TL::TO0, F1 = D >= 2 ? 2 * TL::TO1 : 1, F2 = D >= 3 ? 2 * TL::TO2 : 1;      // after all passes
    constexpr int CELLS = E0 * E1 * E2;
    __shared__ double red[kWaves];
    const Tile t = tile_of<T, D>(a);
    if (a.flag && a.flag[t.c]) return;
    T h[4], g[4];
    filters<T, TAPS>(h, g);
    Cx<T>* bufA = reinterpret_cast<Cx<T>*>(wavelet_lds);
    Cx<T>* bufB = bufA + CELLS;
    {
        const Cx<T>* src = static_cast<const Cx<T>*>(a.fine_in[blockIdx.y]);
        const int64_t p1 = a.fine_dense ? a.m[0] : a.pitch[1], p2 = a.fine_dense ? (int64_t)a.m[0] * a.m[1] : a.pitch[2];
        for (int e = threadIdx.x; e < CELLS; e += kThreads) {
            const int e0 = e % E0, e1 = (e / E0) % E1, e2 = e / (E0 * E1);
            const int f0 = wrap(2 * t.o0[0] + e0, a.m[0]), f1 = wrap(2 * t.o0[1] + e1, a.m[1]), f2 = wrap(2 * t.o0[2] + e2, a.m[2]);
            bufA[e] = src[f0 + f1 * p1 + f2 * p2];
        }
    }
    __syncthreads();
    analysis_pass<T, TAPS, 0, E0, E1, E2, TL::TO0>(bufA, bufB, h, g);
    __syncthreads();
    Cx<T>* cur = bufB;
    if (D >= 2) {
        analysis_pass<T, TAPS, 1, F0, E1, E2, TL::TO1>(bufB, bufA, h, g);
        __syncthreads();
        cur = bufA;
    }
    if (D >= 3) {
        analysis_pass<T, TAPS, 2, F0, F1, E2, TL::TO2>(bufA, bufB, h, g);
        __syncthreads();
        cur = bufB;
    }
    // the stores: 2 TO per transformed dimension, band per dimension from the position
    Cx<T>* coef = static_cast<Cx<T>*>(a.coef[blockIdx.y]);
    Cx<T>* low = static_cast<Cx<T>*>(a.low[blockIdx.y]);
    const int64_t l1 = a.low_dense ? a.h[0] : a.pitch[1], l2 = a.low_dense ? (int64_t)a.h[0] * a.h[1] : a.pitch[2];
    const T thr = (T)a.thr[blockIdx.y];
    const bool shrink = a.shrink != 0 && thr > T(0);
    double sum = 0.0;
    constexpr int OUTS = F0 * F1 * F2;
    for (int e = threadIdx.x; e < OUTS; e += kThreads) {
        const int j[3] = {e % F0, (e / F0) % F1, e / (F0 * F1)};
        int gpos[3] = {0, 0, 0}, band[3] = {0, 0, 0};
        bool inside = true;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            band[d] = j[d] >= TO[d] ? 1 : 0;
            gpos[d] = t.o0[d] + j[d] - band[d] * TO[d];
            inside = inside && gpos[d] < a.h[d];
        }
        if (!inside) continue;
        Cx<T> v = cur[e];
        if (band[0] | band[1] | band[2]) {
            if (shrink) {
                const T mag = sqrt(v.re * v.re + v.im * v.im);
                const T s = mag > thr ? T(1) - thr / mag : T(0);
                v.re *= s;
                v.im *= s;
            }
            if (a.shrink) sum += (double)sqrt(v.re * v.re + v.im * v.im);
            coef[(band[0] * a.h[0] + gpos[0]) + (band[1] * a.h[1] + gpos[1]) * a.pitch[1] + (band[2] * a.h[2] + gpos[2]) * a.pitch[2]] = v;
        } else {
            low[gpos[0] + gpos[1] * l1 + gpos[2] * l2] = v;
        }
    }
    if (a.part) {
        sum = block_reduce<Sum>(sum, red);
        if (threadIdx.x == 0) a.part[(int64_t)t.c * a.P + a.part_off + blockIdx.x] = sum;
    }
}

// One synthesis pass along AXIS: its extent is 2 CN (lo coefficients at [0, CN), hi at [CN, 2 CN), CN = TO + TAPS / 2 − 1, the first
// coefficient one before the tile for the 4-tap filter) -> 2 TO fine cells
template <typename T, int TAPS, int AXIS, int X0, int X1, int X2, int TO>
__device__ __forceinline__ void synthesis_pass(const Cx<T>* src, Cx<T>* dst, const T* h, const T* g) {
    constexpr int HAL = TAPS / 2 - 1, CN = TO + HAL;
    constexpr int SIN[3] = {1, X0, X0 * X1};
    constexpr int Y0 = AXIS == 0 ? 2 * TO : X0, Y1 = AXIS == 1 ? 2 * TO : X1, Y2 = AXIS == 2 ? 2 * TO : X2;
    constexpr int SOUT[3] = {1, Y0, Y0 * Y1};
    constexpr int ITEMS = Y0 * Y1 * Y2;
    for (int it = threadIdx.x; it < ITEMS; it += kThreads) {
        int i[3] = {it % Y0, (it / Y0) % Y1, it / (Y0 * Y1)};
        const int ob = i[0] * SOUT[0] + i[1] * SOUT[1] + i[2] * SOUT[2];
        const int j = i[AXIS], p = j & 1;
        i[AXIS] = (j >> 1) + HAL;
        const int ib = i[0] * SIN[0] + i[1] * SIN[1] + i[2] * SIN[2];
        const Cx<T> lo = src[ib], hi = src[ib + CN * SIN[AXIS]];
        T re = h[p] * lo.re + g[p] * hi.re, im = h[p] * lo.im + g[p] * hi.im;
        if (TAPS == 4) {
            const Cx<T> lo1 = src[ib - SIN[AXIS]], hi1 = src[ib + (CN - 1) * SIN[AXIS]];
            re += h[p + 2] * lo1.re + g[p + 2] * hi1.re;
            im += h[p + 2] * lo1.im + g[p + 2] * hi1.im;
        }
        dst[ob] = Cx<T>{re, im};
    }
}

template <typename T, int TAPS, int D>
__global__ __launch_bounds__(kThreads) void wavelet_synthesis_kernel(WaveletLevel a) {
    using TL = TileOf<T, D>;
    constexpr int HAL = TAPS / 2 - 1;
    constexpr int CN[3] = {TL::TO0 + HAL, D >= 2 ? TL::TO1 + HAL : 1, D >= 3 ? TL::TO2 + HAL : 1};
    constexpr int E0 = 2 * CN[0], E1 = D >= 2 ? 2 * CN[1] : 1, E2 = D >= 3 ? 2 * CN[2] : 1;
    constexpr int F0 = 2 * TL::TO0, F1 = D >= 2 ? 2 * TL::TO1 : 1, F2 = D >= 3 ? 2 * TL::TO2 : 1;
    constexpr int CELLS = E0 * E1 * E2;
    __shared__ double red[kWaves];
    const Tile t = tile_of<T, D>(a);
    if (a.flag && a.flag[t.c]) return;
    T h[4], g[4];
    filters<T, TAPS>(h, g);
    Cx<T>* bufA = reinterpret_cast<Cx<T>*>(wavelet_lds);
    Cx<T>* bufB = bufA + CELLS;
    {
        const Cx<T>* coef = static_cast<const Cx<T>*>(a.coef[blockIdx.y]);
        const Cx<T>* low = static_cast<const Cx<T>*>(a.low[blockIdx.y]);
        const int64_t l1 = a.low_dense ? a.h[0] : a.pitch[1], l2 = a.low_dense ? (int64_t)a.h[0] * a.h[1] : a.pitch[2];
        for (int e = threadIdx.x; e < CELLS; e += kThreads) {
            const int j[3] = {e % E0, (e / E0) % E1, e / (E0 * E1)};
            int gpos[3] = {0, 0, 0}, band[3] = {0, 0, 0};
#pragma unroll
            for (int d = 0; d < D; ++d) {
                band[d] = j[d] >= CN[d] ? 1 : 0;
                gpos[d] = wrap(t.o0[d] - HAL + j[d] - band[d] * CN[d], a.h[d]);
            }
            if (band[0] | band[1] | band[2])
                bufA[e] = coef[(band[0] * a.h[0] + gpos[0]) + (band[1] * a.h[1] + gpos[1]) * a.pitch[1] + (band[2] * a.h[2] + gpos[2]) * a.pitch[2]];
            else
                bufA[e] = low[gpos[0] + gpos[1] * l1 + gpos[2] * l2];
        }
    }
    __syncthreads();
    // dimension 3 first, dimension 1 last
    Cx<T>* cur = bufA;
    if (D >= 3) {
        synthesis_pass<T, TAPS, 2, E0, E1, E2, TL::TO2>(bufA, bufB, h, g);
        __syncthreads();
        cur = bufB;
    }
    if (D >= 2) {
        synthesis_pass<T, TAPS, 1, E0, E1, F2, TL::TO1>(cur, cur == bufA ? bufB : bufA, h, g);
        __syncthreads();
        cur = cur == bufA ? bufB : bufA;
    }
    {
        Cx<T>* nxt = cur == bufA ? bufB : bufA;
        synthesis_pass<T, TAPS, 0, E0, F1, F2, TL::TO0>(cur, nxt, h, g);
        __syncthreads();
        cur = nxt;
    }
    Cx<T>* dst = static_cast<Cx<T>*>(a.fine_out[blockIdx.y]);
    const int64_t p1 = a.fine_dense ? a.m[0] : a.pitch[1], p2 = a.fine_dense ? (int64_t)a.m[0] * a.m[1] : a.pitch[2];
    Cx<T>* x = a.momentum ? static_cast<Cx<T>*>(a.x[blockIdx.y]) : nullptr;
    const T beta = (T)a.beta;
    double sdd = 0.0, sxx = 0.0;
    constexpr int OUTS = F0 * F1 * F2;
    for (int e = threadIdx.x; e < OUTS; e += kThreads) {
        const int f0 = 2 * t.o0[0] + e % F0, f1 = 2 * t.o0[1] + (e / F0) % F1, f2 = 2 * t.o0[2] + e / (F0 * F1);
        if (f0 >= a.m[0] || f1 >= a.m[1] || f2 >= a.m[2]) continue;
        const int64_t at = f0 + f1 * p1 + f2 * p2;
        const Cx<T> v = cur[e];
        if (a.momentum) {
            const Cx<T> old = x[at];
            const T dr = v.re - old.re, di = v.im - old.im;
            sdd += (double)dr * (double)dr + (double)di * (double)di;
            sxx += (double)v.re * (double)v.re + (double)v.im * (double)v.im;
            x[at] = v;
            dst[at] = Cx<T>{v.re + beta * dr, v.im + beta * di};
        } else {
            dst[at] = v;
        }
    }
    if (a.momentum) {
        sdd = block_reduce<Sum>(sdd, red);
        sxx = block_reduce<Sum>(sxx, red);
        if (threadIdx.x == 0) {
            double* out = a.mom_part + ((int64_t)t.c * a.G0 + blockIdx.x) * 2;
            out[0] = sdd;
            out[1] = sxx;
        }
    }
}

__global__ __launch_bounds__(kThreads) void wavelet_sum_kernel(const double* part, int P, double* out) {
    __shared__ double red[kWaves];
    const double s = row_reduce<Sum>(part + (int64_t)blockIdx.x * P, P, 1, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

template <typename KF, typename KD>
hipError_t launch(const WaveletLevel& l, bool synthesis, KF kf, KD kd, hipStream_t stream) {
    const dim3 grid((unsigned)(l.tiles[0] * l.tiles[1] * l.tiles[2]), (unsigned)l.nc);
    const size_t lds = wavelet_lds_bytes(l, synthesis);
    if (l.dtype == NUFFT_F32) hipLaunchKernelGGL(kf, grid, dim3(kThreads), lds, stream, l);
    else hipLaunchKernelGGL(kd, grid, dim3(kThreads), lds, stream, l);
    return hipGetLastError();
}

// the instantiation for (taps, D); the element type is chosen in launch()
#define NUFFT_WAVELET_DISPATCH(kernel, synthesis)                                                                        \
    if (l.taps == 2) {                                                                                                   \
        if (l.D == 1) return launch(l, synthesis, kernel<float, 2, 1>, kernel<double, 2, 1>, stream);                    \
        if (l.D == 2) return launch(l, synthesis, kernel<float, 2, 2>, kernel<double, 2, 2>, stream);                    \
        return launch(l, synthesis, kernel<float, 2, 3>, kernel<double, 2, 3>, stream);                                  \
    }                                                                                                                    \
    if (l.D == 1) return launch(l, synthesis, kernel<float, 4, 1>, kernel<double, 4, 1>, stream);                        \
    if (l.D == 2) return launch(l, synthesis, kernel<float, 4, 2>, kernel<double, 4, 2>, stream);                        \
    return launch(l, synthesis, kernel<float, 4, 3>, kernel<double, 4, 3>, stream)

}  // namespace

size_t wavelet_lds_bytes(const WaveletLevel& l, bool synthesis) {
    size_t cells = 1;
    for (int d = 0; d < l.D; ++d) cells *= synthesis ? 2 * (size_t)(l.to[d] + l.taps / 2 - 1) : (size_t)(2 * l.to[d] + l.taps - 2);
    return 2 * cells * 2 * (l.dtype == NUFFT_F32 ? 4 : 8);
}

hipError_t launch_wavelet_analysis(const WaveletLevel& l, hipStream_t stream) {
    NUFFT_WAVELET_DISPATCH(wavelet_analysis_kernel, false);
}

hipError_t launch_wavelet_synthesis(const WaveletLevel& l, hipStream_t stream) {
    NUFFT_WAVELET_DISPATCH(wavelet_synthesis_kernel, true);
}

hipError_t launch_wavelet_sum(const double* part, int P, int C, double* out, hipStream_t stream) {
    hipLaunchKernelGGL(wavelet_sum_kernel, dim3(C), dim3(kThreads), 0, stream, part, P, out);
    return hipGetLastError();
}

}  // namespace nufft
