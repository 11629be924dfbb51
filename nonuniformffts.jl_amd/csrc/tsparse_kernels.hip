// The temporal sparsifying transform of the low-rank plus sparse model and the solver's small kernels (lps.h, lps.cpp; DESIGN.md
// section 27).
//
//     NUFFT_TSPARSE_DFT:       (T x)_k[i] = K^-1/2 Σ_c x_c[i] w^(k c mod K),  w = exp(−2πi / K);   Tᴴ with conj(w)
//     NUFFT_TSPARSE_IDENTITY:  T = I
//
// One kernel, flat over the n cells.  A workgroup stages a tile [frame][cell] in LDS (FlatTiles of hermitian.h); one thread per (frequency, cell)
// forms the direct sum of K terms in the element type (any K in 1 ... 32), with the K twiddles (K^-1/2 folded in, FP64 on the host,
// rounded once) in LDS.  The thread soft-thresholds the coefficient where it is produced: c · (1 − t / |c|) for |c| > t, else 0, nothing
// divided.  TS_SOLVER writes the coefficients to a second LDS tile and runs the inverse from there: S⁺ = Tᴴ soft_t(T (zS − g)),
// S <- S⁺, zS <- S⁺ + β (S⁺ − S), u <- zL + zS (the next apply's input), and the partials of ‖S⁺ − S‖², ‖S⁺‖², ‖T S⁺‖₁.
//
// Sums are FP64, one plain store per workgroup, reduced later in one fixed order (stream_kernels.h).  Every kernel but the start and the
// final sum reads the done flag before its first data load.
#include <hip/hip_runtime.h>

#include <cmath>

#include "hermitian.h"
#include "lps.h"
#include "stream_kernels.h"

namespace nufft {
using namespace stream;

static_assert(kLpsThreads == kThreads, "the reductions of stream_kernels.h");

namespace {

using namespace jacobi_team;

template <typename T>
__device__ __forceinline__ const Cx<T>* frame(const LpsFrames& f, int k) {
    return static_cast<const Cx<T>*>(f.p[k]);
}
template <typename T>
__device__ __forceinline__ Cx<T>* frame_w(const LpsFrames& f, int k) {
    return static_cast<Cx<T>*>(f.p[k]);
}

// The complex soft threshold, every operation rounded on its own (tests/lps_reference.py, tshrink, restates it); `l1` gains |result|.
template <typename T>
__device__ __forceinline__ Cx<T> soft(Cx<T> c, T t, double& l1) {
#pragma clang fp contract(off)
    const T mag = sqrt(c.re * c.re + c.im * c.im);
    if (!(mag > t)) return Cx<T>{T(0), T(0)};
    const T s = T(1) - t / mag;
    const Cx<T> r{c.re * s, c.im * s};
    l1 += sqrt((double)r.re * (double)r.re + (double)r.im * (double)r.im);
    return r;
}

// Σ_m src[m][v] tw[(m · k) mod K] (CONJ: the conjugate twiddle), in the element type
template <typename T, bool CONJ>
__device__ __forceinline__ Cx<T> dft_sum(const Cx<T>* src, int TCP, int v, const Cx<T>* tw, int K, int k) {
    T sr = T(0), si = T(0);
    int idx = 0;
    for (int m = 0; m < K; ++m) {
        const Cx<T> x = src[m * TCP + v];
        const T wr = tw[idx].re, wi = CONJ ? -tw[idx].im : tw[idx].im;
        sr += x.re * wr - x.im * wi;
        si += x.re * wi + x.im * wr;
        idx += k;
        if (idx >= K) idx -= K;
    }
    return Cx<T>{sr, si};
}

template <typename T, int MODE, bool DFT>
__global__ __launch_bounds__(kLpsThreads) void tsparse_kernel(TsLaunch a, int off_B, int off_tw) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ double red[kWaves];
    if (a.flag && a.flag[0]) return;
    const int K = a.K, tid = threadIdx.x;
    const FlatTiles ft(a.tl);
    const int TCP = ft.TCP;
    Cx<T>* A = reinterpret_cast<Cx<T>*>(smem);
    Cx<T>* B = reinterpret_cast<Cx<T>*>(smem + off_B);
    Cx<T>* tw = reinterpret_cast<Cx<T>*>(smem + off_tw);
    if (DFT && tid < K) tw[tid] = Cx<T>{(T)a.tw[2 * tid], (T)a.tw[2 * tid + 1]};
    const T t = (T)a.t, beta = (T)a.beta;
    double sdd = 0.0, sxx = 0.0, l1 = 0.0;
    for (int64_t tile = ft.tile0; tile < ft.tile1; ++tile) {
        const int64_t cell0 = ft.first_cell(tile);
        const int nc = ft.cells(tile, a.n);
        for_tile<kLpsThreads>(ft, K, nc, [&](int c, int v) {
            const int64_t at = cell0 + v;
            Cx<T> val = frame<T>(a.f0, c)[at];
            if (MODE == TS_SOLVER) {
                const Cx<T> g = frame<T>(a.f1, c)[at];
                val = Cx<T>{val.re - g.re, val.im - g.im};
            }
            A[c * TCP + v] = val;
        });
        __syncthreads();                                                        // also: the twiddles are in LDS
        if (MODE != TS_INVERSE) {
            for_tile<kLpsThreads>(ft, K, nc, [&](int k, int v) {
                Cx<T> cf = DFT ? dft_sum<T, false>(A, TCP, v, tw, K, k) : A[k * TCP + v];
                if (MODE != TS_FORWARD) cf = soft<T>(cf, t, l1);
                if (MODE == TS_SOLVER) B[k * TCP + v] = cf;
                else frame_w<T>(a.f1, k)[cell0 + v] = cf;
            });
        }
        if (MODE == TS_SOLVER) __syncthreads();
        if (MODE == TS_INVERSE || MODE == TS_SOLVER) {
            const Cx<T>* src = MODE == TS_INVERSE ? A : B;
            for_tile<kLpsThreads>(ft, K, nc, [&](int c, int v) {
                const int64_t at = cell0 + v;
                const Cx<T> res = DFT ? dft_sum<T, true>(src, TCP, v, tw, K, c) : src[c * TCP + v];
                if (MODE == TS_INVERSE) {
                    frame_w<T>(a.f1, c)[at] = res;
                } else {
                    const Cx<T> zs = solver_epilogue(frame_w<T>(a.f2, c), frame_w<T>(a.f0, c), at, res, beta, sdd, sxx);
                    const Cx<T> zl = frame<T>(a.f3, c)[at];
                    frame_w<T>(a.f4, c)[at] = Cx<T>{zl.re + zs.re, zl.im + zs.im};
                }
            });
        }
        __syncthreads();
    }
    if (MODE == TS_SHRINK || MODE == TS_SOLVER) {
        sdd = block_reduce<Sum>(sdd, red);
        sxx = block_reduce<Sum>(sxx, red);
        l1 = block_reduce<Sum>(l1, red);
        if (tid == 0) {
            double* out = a.part + (int64_t)blockIdx.x * 3;
            out[0] = sdd;
            out[1] = sxx;
            out[2] = l1;
        }
    }
}

__global__ __launch_bounds__(kThreads) void tsparse_sum_kernel(const double* part, int G, double* out) {
    __shared__ double lds[kWaves];
    const double v = row_reduce<Sum>(part + 2, G, 3, lds);
    if (threadIdx.x == 0) out[0] = v;
}

// L = zL = x (WARM) or 0 (then x = 0 too), S = zS = 0: u = zL + zS is x itself.  The first workgroup resets the scalars and fills the
// history with NaN.
template <typename T, bool WARM>
__global__ __launch_bounds__(kThreads) void lps_start_kernel(LpsSolve a) {
    const int c = blockIdx.y;
    Cx<T>* x = frame_w<T>(a.x, c);
    Cx<T>* L = frame_w<T>(a.L, c);
    Cx<T>* S = frame_w<T>(a.S, c);
    Cx<T>* zL = frame_w<T>(a.zL, c);
    Cx<T>* zS = frame_w<T>(a.zS, c);
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads) {
        const Cx<T> v = WARM ? x[i] : Cx<T>{T(0), T(0)};
        if (!WARM) x[i] = v;
        L[i] = v;
        zL[i] = v;
        S[i] = Cx<T>{T(0), T(0)};
        zS[i] = Cx<T>{T(0), T(0)};
    }
    if (blockIdx.x == 0 && c == 0) reset_outcome<3>(a.s, 0, 1, a.max_iter);
}

// One workgroup: the change, the history row and the done flag of iteration a.it
__global__ __launch_bounds__(kThreads) void lps_decide_kernel(LpsSolve a) {
    __shared__ double lds[kWaves];
    if (a.s.flag[0]) return;
    const double dl = row_reduce<Sum>(a.part_l, a.Gl, 2, lds);
    const double xl = row_reduce<Sum>(a.part_l + 1, a.Gl, 2, lds);
    const double ds = row_reduce<Sum>(a.part_s, a.Gs, 3, lds);
    const double xs = row_reduce<Sum>(a.part_s + 1, a.Gs, 3, lds);
    const double l1 = row_reduce<Sum>(a.part_s + 2, a.Gs, 3, lds);
    if (threadIdx.x == 0) {
        const int64_t row = (int64_t)(a.it - 1) * 3;
        store_decision(a.s, 0, row, dl + ds, xl + xs, a.tol, a.it);
        a.s.history[row + 1] = a.nuc[0];
        a.s.history[row + 2] = l1;
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void lps_sum_kernel(LpsSolve a) {
    const int c = blockIdx.y;
    Cx<T>* x = frame_w<T>(a.x, c);
    const Cx<T>* L = frame<T>(a.L, c);
    const Cx<T>* S = frame<T>(a.S, c);
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads)
        x[i] = Cx<T>{L[i].re + S[i].re, L[i].im + S[i].im};
}

template <typename T, int MODE>
hipError_t launch_ts(const TsLaunch& a, hipStream_t stream) {
    const size_t tile = up16((size_t)a.K * (a.tl.TC + 1) * sizeof(T) * 2);
    const size_t off_B = tile, off_tw = MODE == TS_SOLVER ? 2 * tile : tile;
    const size_t bytes = off_tw + (size_t)a.K * sizeof(T) * 2;
    const dim3 gr((unsigned)a.tl.G), bl(kLpsThreads);
    if (a.transform == NUFFT_TSPARSE_DFT) hipLaunchKernelGGL((tsparse_kernel<T, MODE, true>), gr, bl, bytes, stream, a, (int)off_B, (int)off_tw);
    else hipLaunchKernelGGL((tsparse_kernel<T, MODE, false>), gr, bl, bytes, stream, a, (int)off_B, (int)off_tw);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_ts_mode(const TsLaunch& a, hipStream_t stream) {
    switch (a.mode) {
        case TS_FORWARD: return launch_ts<T, TS_FORWARD>(a, stream);
        case TS_INVERSE: return launch_ts<T, TS_INVERSE>(a, stream);
        case TS_SHRINK: return launch_ts<T, TS_SHRINK>(a, stream);
        default: return launch_ts<T, TS_SOLVER>(a, stream);
    }
}

}  // namespace

hipError_t launch_tsparse(const TsLaunch& a, hipStream_t stream) {
    return a.dtype == NUFFT_F32 ? launch_ts_mode<float>(a, stream) : launch_ts_mode<double>(a, stream);
}

hipError_t launch_tsparse_sum(const double* part, int G, double* out, hipStream_t stream) {
    hipLaunchKernelGGL(tsparse_sum_kernel, dim3(1), dim3(kThreads), 0, stream, part, G, out);
    return hipGetLastError();
}

hipError_t launch_lps_start(const LpsSolve& a, bool warm, hipStream_t stream) {
    const dim3 gr(a.G, a.K), bl(kThreads);
    if (a.dtype == NUFFT_F32) {
        if (warm) hipLaunchKernelGGL((lps_start_kernel<float, true>), gr, bl, 0, stream, a);
        else hipLaunchKernelGGL((lps_start_kernel<float, false>), gr, bl, 0, stream, a);
    } else {
        if (warm) hipLaunchKernelGGL((lps_start_kernel<double, true>), gr, bl, 0, stream, a);
        else hipLaunchKernelGGL((lps_start_kernel<double, false>), gr, bl, 0, stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_lps_decide(const LpsSolve& a, hipStream_t stream) {
    hipLaunchKernelGGL(lps_decide_kernel, dim3(1), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_lps_sum(const LpsSolve& a, hipStream_t stream) {
    const dim3 gr(a.G, a.K), bl(kThreads);
    if (a.dtype == NUFFT_F32) hipLaunchKernelGGL(lps_sum_kernel<float>, gr, bl, 0, stream, a);
    else hipLaunchKernelGGL(lps_sum_kernel<double>, gr, bl, 0, stream, a);
    return hipGetLastError();
}

}  // namespace nufft
