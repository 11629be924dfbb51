// The global low-rank proximal map: singular-value soft-thresholding of the n x K space-time (Casorati) matrix M whose column c is
// frame c, through the K x K Gram matrix (lps.h, lps.cpp).
//
//     H = M^H M  (FP64)      H = V Λ V^H  (jacobi.h, FP64)      σ_i = sqrt(max(λ_i, 0))      f_i = σ_i > t ? 1 − t / σ_i : 0
//     P = V diag(f) V^H      M <- M P                           nuc = Σ_i f_i σ_i
//
// Three launches.  The Gram and apply kernels are flat over the n cells: a workgroup takes `tpw` consecutive tiles of TC cells x K frames
// into LDS (FlatTiles of hermitian.h, which also holds the Gram, fold, shrink, projector and apply steps named below).
//
//   gram   every entry i <= j of a tile is summed in FP64 in cell order over S fixed segments, the segments are added in segment order
//          into the thread that owns the entry, tile after tile; a workgroup leaves K (K + 1) / 2 complex partials with plain stores.
//          GLR_SOLVER forms g = τ (q + μ (zL + zS) − b) while it loads, stores g over q and takes zL − g as the matrix.
//   eigen  one workgroup adds the partial sets in workgroup order, a team of 2^ceil(log2 K) lanes of its first wave diagonalises H, and
//          P, the nuclear norm and the sweep count go to device memory.
//   apply  P in LDS; Σ_i M_vi P_ij in FP64, one store.  GLR_SOLVER reads the old L and writes L, zL = L⁺ + β (L⁺ − L) and the partials of
//          ‖L⁺ − L‖², ‖L⁺‖².  The output may be the input: a tile is loaded whole before it is stored, and tiles are disjoint.
//
// Every kernel reads the done flag before its first data load.  No atomics, every sum in one fixed order: two runs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "hermitian.h"
#include "lps.h"
#include "stream_kernels.h"

namespace nufft {
using namespace stream;

static_assert(kLpsThreads == kThreads, "the reductions of stream_kernels.h");
static_assert(kLpsMaxK * (kLpsMaxK + 1) / 2 <= kGlrPairsPerThread * kLpsThreads, "every Gram entry has an owner");

namespace {

using namespace jacobi_team;

// g = τ (q + μ u − b), every operation rounded on its own: the apply and temporal kernels subtract the STORED g, and the Gram kernel
// must see the same zL − g
template <typename T>
__device__ __forceinline__ Cx<T> gradient(Cx<T> q, Cx<T> u, Cx<T> b, T tau, T mu) {
#pragma clang fp contract(off)
    return Cx<T>{tau * (q.re + mu * u.re - b.re), tau * (q.im + mu * u.im - b.im)};
}

template <typename T>
__device__ __forceinline__ const Cx<T>* frame(const LpsFrames& f, int k) {
    return static_cast<const Cx<T>*>(f.p[k]);
}
template <typename T>
__device__ __forceinline__ Cx<T>* frame_w(const LpsFrames& f, int k) {
    return static_cast<Cx<T>*>(f.p[k]);
}

template <typename T, int MODE>
__global__ __launch_bounds__(kLpsThreads) void glr_gram_kernel(GlrLaunch a, int off_gp, int off_ij) {
    extern __shared__ __align__(16) unsigned char smem[];
    if (a.flag && a.flag[0]) return;
    const int K = a.K, S = a.tl.S, np = K * (K + 1) / 2, tid = threadIdx.x;
    const FlatTiles ft(a.tl);
    Cx<T>* data = reinterpret_cast<Cx<T>*>(smem);
    Cd* gp = reinterpret_cast<Cd*>(smem + off_gp);                                // [segment][entry]
    unsigned short* ij = reinterpret_cast<unsigned short*>(smem + off_ij);      // [entry]: i << 8 | j
    for (int pr = tid; pr < np; pr += kLpsThreads) {
        int i, j;
        pair_of(pr, K, i, j);
        ij[pr] = (unsigned short)(i << 8 | j);
    }
    Cd acc[kGlrPairsPerThread];
#pragma unroll
    for (int m = 0; m < kGlrPairsPerThread; ++m) acc[m] = Cd{0.0, 0.0};
    const T tau = (T)a.step, mu = (T)a.lambda;
    const int seg_len = ft.TC / S;
    for (int64_t tile = ft.tile0; tile < ft.tile1; ++tile) {
        stage_padded<kLpsThreads>(data, ft, K, ft.first_cell(tile), ft.cells(tile, a.n), [&](int k, int64_t at, bool live) {
            Cx<T> val = frame<T>(a.f0, k)[at];
            if (MODE == GLR_SOLVER && live) {
                const Cx<T> zs = frame<T>(a.f1, k)[at];
                const Cx<T> g = gradient<T>(frame<T>(a.f2, k)[at], Cx<T>{val.re + zs.re, val.im + zs.im}, frame<T>(a.f3, k)[at], tau, mu);
                frame_w<T>(a.f2, k)[at] = g;
                val = Cx<T>{val.re - g.re, val.im - g.im};
            }
            return val;
        });
        __syncthreads();
        for (int u = tid; u < S * np; u += kLpsThreads) {
            const int pr = u % np, seg = u / np;
            const int i = ij[pr] >> 8, j = ij[pr] & 255;
            gp[u] = gram_segment<false>(data + i * ft.TCP + seg * seg_len, data + j * ft.TCP + seg * seg_len, seg_len);
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < kGlrPairsPerThread; ++m) {
            const int pr = tid + m * kLpsThreads;
            if (pr < np)
                for (int seg = 0; seg < S; ++seg) {
                    const Cd g = gp[seg * np + pr];
                    acc[m].re += g.re;
                    acc[m].im += g.im;
                }
        }
        // the next tile's loads overwrite `data` only after every thread has passed the barrier above, and its `gp` only after the
        // barrier that follows those loads: no third barrier
    }
    Cd* out = reinterpret_cast<Cd*>(a.gram) + (int64_t)blockIdx.x * np;
#pragma unroll
    for (int m = 0; m < kGlrPairsPerThread; ++m) {
        const int pr = tid + m * kLpsThreads;
        if (pr < np) out[pr] = acc[m];
    }
}

// One workgroup.  LDS: H, V (K x K complex double each), f (K double)
__global__ __launch_bounds__(kLpsThreads) void glr_eigen_kernel(GlrLaunch a) {
    extern __shared__ __align__(16) unsigned char smem[];
    if (a.flag && a.flag[0]) return;
    const int K = a.K, np = K * (K + 1) / 2, tid = threadIdx.x, G = a.tl.G;
    Cd* H = reinterpret_cast<Cd*>(smem);
    Cd* V = H + K * K;
    double* fs = reinterpret_cast<double*>(V + K * K);
    const Cd* gram = reinterpret_cast<const Cd*>(a.gram);
    for (int pr = tid; pr < np; pr += kLpsThreads) {
        int i, j;
        pair_of(pr, K, i, j);
        store_hermitian(H, K, i, j, fold(gram + pr, G, np));
    }
    for (int e = tid; e < K * K; e += kLpsThreads) V[e] = identity_entry(e / K, e % K);
    __syncthreads();
    int sweeps = 0;
    if (K > 1 && tid < team_width(K)) sweeps = jacobi(H, V, K, tid);
    __syncthreads();
    if (tid == 0) {
        double nuc = 0.0;
        for (int i = 0; i < K; ++i) fs[i] = shrink_factor(H[i * K + i].re, a.t, nuc);
        a.nuc[0] = nuc;
        if (a.nuc_out) a.nuc_out[0] = nuc;
        a.sweeps[0] = sweeps;
    }
    __syncthreads();
    Cd* P = reinterpret_cast<Cd*>(a.P);
    for (int e = tid; e < K * K; e += kLpsThreads) P[e] = projector_entry(V, fs, K, e / K, e % K);
}

template <typename T, int MODE>
__global__ __launch_bounds__(kLpsThreads) void glr_apply_kernel(GlrLaunch a, int off_P) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ double red[kWaves];
    if (a.flag && a.flag[0]) return;
    const int K = a.K, tid = threadIdx.x;
    const FlatTiles ft(a.tl);
    Cx<T>* data = reinterpret_cast<Cx<T>*>(smem);
    Cd* P = reinterpret_cast<Cd*>(smem + off_P);
    for (int e = tid; e < K * K; e += kLpsThreads) P[e] = reinterpret_cast<const Cd*>(a.P)[e];
    const T beta = (T)a.beta;
    double sdd = 0.0, sxx = 0.0;
    for (int64_t tile = ft.tile0; tile < ft.tile1; ++tile) {
        const int64_t cell0 = ft.first_cell(tile);
        const int nc = ft.cells(tile, a.n);
        for_tile<kLpsThreads>(ft, K, nc, [&](int k, int v) {
            const int64_t at = cell0 + v;
            Cx<T> val = frame<T>(a.f0, k)[at];
            if (MODE == GLR_SOLVER) {
                const Cx<T> g = frame<T>(a.f2, k)[at];
                val = Cx<T>{val.re - g.re, val.im - g.im};
            }
            data[k * ft.TCP + v] = val;
        });
        __syncthreads();                                                        // also: P is in LDS
        for_tile<kLpsThreads>(ft, K, nc, [&](int j, int v) {
            const int64_t at = cell0 + v;
            double rr = 0.0, ri = 0.0;
            for (int i = 0; i < K; ++i) {
                const double mr = (double)data[i * ft.TCP + v].re, mi = (double)data[i * ft.TCP + v].im;
                const Cd p = P[i * K + j];
                rr += mr * p.re - mi * p.im;
                ri += mr * p.im + mi * p.re;
            }
            const Cx<T> res{(T)rr, (T)ri};
            if (MODE == GLR_SOLVER) solver_epilogue(frame_w<T>(a.f1, j), frame_w<T>(a.f0, j), at, res, beta, sdd, sxx);
            else frame_w<T>(a.f1, j)[at] = res;
        });
        __syncthreads();
    }
    if (MODE == GLR_SOLVER) {
        sdd = block_reduce<Sum>(sdd, red);
        sxx = block_reduce<Sum>(sxx, red);
        if (tid == 0) {
            a.part[(int64_t)blockIdx.x * 2] = sdd;
            a.part[(int64_t)blockIdx.x * 2 + 1] = sxx;
        }
    }
}

size_t tile_bytes(bool f32, int K, const FlatTiling& tl) { return up16((size_t)K * (tl.TC + 1) * (f32 ? 8 : 16)); }

template <typename T, int MODE>
hipError_t launch_gram(const GlrLaunch& a, hipStream_t stream) {
    const int np = a.K * (a.K + 1) / 2;
    const size_t off_gp = tile_bytes(sizeof(T) == 4, a.K, a.tl), off_ij = off_gp + (size_t)a.tl.S * np * 16;
    hipLaunchKernelGGL((glr_gram_kernel<T, MODE>), dim3((unsigned)a.tl.G), dim3(kLpsThreads), up16(off_ij + (size_t)np * 2), stream, a, (int)off_gp, (int)off_ij);
    return hipGetLastError();
}

template <typename T, int MODE>
hipError_t launch_apply(const GlrLaunch& a, hipStream_t stream) {
    const size_t off_P = tile_bytes(sizeof(T) == 4, a.K, a.tl);
    hipLaunchKernelGGL((glr_apply_kernel<T, MODE>), dim3((unsigned)a.tl.G), dim3(kLpsThreads), off_P + (size_t)a.K * a.K * 16, stream, a, (int)off_P);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_glr_gram(const GlrLaunch& a, hipStream_t stream) {
    const bool f32 = a.dtype == NUFFT_F32;
    if (a.mode == GLR_SOLVER) return f32 ? launch_gram<float, GLR_SOLVER>(a, stream) : launch_gram<double, GLR_SOLVER>(a, stream);
    return f32 ? launch_gram<float, GLR_PLAIN>(a, stream) : launch_gram<double, GLR_PLAIN>(a, stream);
}

hipError_t launch_glr_eigen(const GlrLaunch& a, hipStream_t stream) {
    hipLaunchKernelGGL(glr_eigen_kernel, dim3(1), dim3(kLpsThreads), (size_t)a.K * a.K * 32 + (size_t)a.K * 8, stream, a);
    return hipGetLastError();
}

hipError_t launch_glr_apply(const GlrLaunch& a, hipStream_t stream) {
    const bool f32 = a.dtype == NUFFT_F32;
    if (a.mode == GLR_SOLVER) return f32 ? launch_apply<float, GLR_SOLVER>(a, stream) : launch_apply<double, GLR_SOLVER>(a, stream);
    return f32 ? launch_apply<float, GLR_PLAIN>(a, stream) : launch_apply<double, GLR_PLAIN>(a, stream);
}

}  // namespace nufft
