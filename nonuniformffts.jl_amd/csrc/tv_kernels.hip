// Kernels of the total-variation prior and of its primal-dual solver (tv.cpp).
//
//     (∇x)_d[i] = x[i + e_d] − x[i]          (∇ᴴy)[i] = Σ_d (y_d[i − e_d] − y_d[i])          indices mod N_d, on the array as stored
//
// Two stencil kernels, both bound by memory.  The "primal" one reads y at i and i − e_d and writes only x[i] and q[i]; the "dual" one
// reads x̄ and x⁺ at i and i + e_d and writes only y_d[i]: no launch reads at a neighbour an array it writes, so nothing races, nothing is
// double-buffered and no workgroup hands anything to another.
//
// A lane owns one 16-byte pack along dimension 1 (one ComplexF64, two ComplexF32; one ComplexF32 where N_1 is odd and the rows are not
// 16-byte aligned).  For D >= 2 it marches kTvMarch cells along the outermost dimension and keeps the pack of the previous (primal) or
// next (dual) cell of that dimension in registers; the neighbours along the other dimensions come through the caches.  The tile
// (tv_tile) is a compile-time constant per (element type, D): block and lane indices give the coordinates by multiplies, the periodic
// neighbour is one compare and one select, and there is no division per cell.  Lanes outside the box do nothing (the stores are
// masked), so sides below a tile and sides that are no multiple of it need no special case.
//
// Sums are FP64, one plain store per workgroup, reduced later in one fixed order (stream_kernels.h).  A component whose done flag is set
// is frozen: its workgroups leave after reading the flag.  The flags change only in tv_decide_kernel, a launch of its own.
#include <hip/hip_runtime.h>

#include <cmath>

#include "nufft_mi355x.h"
#include "stream_kernels.h"
#include "tv.h"
#include "tv_cells.h"
#include "tv_walk.h"

namespace nufft {
using namespace stream;
using namespace tvcells;
namespace {

// x⁺ = x − τ (q + μ x − b + ∇ᴴy);  x <- x⁺;  q <- x̄ = x⁺ + (x⁺ − x);  partials of ‖x⁺ − x‖², ‖x⁺‖²      (TV_PRIMAL)
// x <- ∇ᴴy                                                                                              (TV_ADJOINT)
template <typename T, int D, int V, int MODE>
__global__ __launch_bounds__(kThreads) void tv_primal_kernel(TvLaunch a) {
    using P = Cells<T, V>;
    __shared__ double red[kWaves];
    Walk w = walk_of<D, V>(a);
    if (a.flag && a.flag[w.c]) return;
    Cx<T>* x = static_cast<Cx<T>*>(a.x[w.k]);
    Cx<T>* q = static_cast<Cx<T>*>(a.q[w.k]);
    const Cx<T>* b = static_cast<const Cx<T>*>(a.b[w.k]);
    const Cx<T>* y[3] = {static_cast<const Cx<T>*>(a.y[w.k][0]), static_cast<const Cx<T>*>(a.y[w.k][D >= 2 ? 1 : 0]),
                         static_cast<const Cx<T>*>(a.y[w.k][D >= 3 ? 2 : 0])};
    const T tau = (T)a.step, mu = (T)a.lambda;
    const int N0 = a.N[0], N1 = a.N[1], N2 = a.N[2];
    constexpr int MD = D - 1;                                        // the marching dimension
    const int64_t SM = D == 2 ? (int64_t)N0 : (int64_t)N0 * N1;      // its stride
    const int NM = D == 2 ? N1 : N2;
    double sdd = 0.0, sxx = 0.0;
    if (w.inside) {
        int im = D == 2 ? w.i1 : w.i2;
        int64_t at = w.at;
        // neighbours that do not move with the march: i0 − 1 (one cell), and for D = 3 row i1 − 1
        const int64_t left = w.i0 == 0 ? (int64_t)N0 - 1 : -1;
        const int64_t up = w.i1 == 0 ? (int64_t)N0 * (N1 - 1) : -(int64_t)N0;
        P prev{};                                                    // y_MD at the previous cell of the march
        if (D >= 2) prev = load_cells<T, V>(y[MD], im == 0 ? at + SM * (NM - 1) : at - SM);
        for (int m = 0; m < w.steps; ++m) {
            P div;
            {
                const P y0 = load_cells<T, V>(y[0], at);
                const Cx<T> l = y[0][at + left];
                div.v[0] = sub(l, y0.v[0]);
                if (V == 2) div.v[V - 1] = sub(y0.v[0], y0.v[V - 1]);
            }
            if (D == 3) {
                const P d1 = sub(load_cells<T, V>(y[1], at + up), load_cells<T, V>(y[1], at));
#pragma unroll
                for (int e = 0; e < V; ++e) div.v[e] = Cx<T>{div.v[e].re + d1.v[e].re, div.v[e].im + d1.v[e].im};
            }
            if (D >= 2) {
                const P cur = load_cells<T, V>(y[MD], at);
                const P dm = sub(prev, cur);
#pragma unroll
                for (int e = 0; e < V; ++e) div.v[e] = Cx<T>{div.v[e].re + dm.v[e].re, div.v[e].im + dm.v[e].im};
                prev = cur;
            }
            if (MODE == TV_ADJOINT) {
                store_cells<T, V>(x, at, div);
            } else {
                const P xv = load_cells<T, V>(x, at), qv = load_cells<T, V>(q, at), bv = load_cells<T, V>(b, at);
                P xn, xb;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    xn.v[e].re = xv.v[e].re - tau * (qv.v[e].re + mu * xv.v[e].re - bv.v[e].re + div.v[e].re);
                    xn.v[e].im = xv.v[e].im - tau * (qv.v[e].im + mu * xv.v[e].im - bv.v[e].im + div.v[e].im);
                    const T dr = xn.v[e].re - xv.v[e].re, di = xn.v[e].im - xv.v[e].im;
                    xb.v[e] = Cx<T>{xn.v[e].re + dr, xn.v[e].im + di};
                    sdd += (double)dr * (double)dr + (double)di * (double)di;
                    sxx += (double)xn.v[e].re * (double)xn.v[e].re + (double)xn.v[e].im * (double)xn.v[e].im;
                }
                store_cells<T, V>(x, at, xn);
                store_cells<T, V>(q, at, xb);
            }
            ++im;
            at += SM;
        }
    }
    if (MODE == TV_PRIMAL) {
        sdd = block_reduce<Sum>(sdd, red);
        sxx = block_reduce<Sum>(sxx, red);
        if (threadIdx.x == 0) {
            double* out = a.part + ((int64_t)w.c * a.G + w.g) * 2;
            out[0] = sdd;
            out[1] = sxx;
        }
    }
}

// y_d <- P_tv(y_d + σ (∇x̄)_d),  P_t(v)_i = v_i · min(1, t / |v_i|₂);  partial of Σ_i |(∇x⁺)_i|₂      (TV_DUAL: x̄ in q, x⁺ in x)
// y_d <- (∇x)_d                                                                                      (TV_GRADIENT)
// partial of Σ_i |(∇x)_i|₂                                                                            (TV_NORM)
template <typename T, int D, int V, int MODE>
__global__ __launch_bounds__(kThreads) void tv_dual_kernel(TvLaunch a) {
    using P = Cells<T, V>;
    __shared__ double red[kWaves];
    Walk w = walk_of<D, V>(a);
    if (a.flag && a.flag[w.c]) return;
    constexpr bool BAR = MODE == TV_DUAL;                            // a second array (x̄) takes part
    constexpr bool SUM = MODE != TV_GRADIENT;
    const Cx<T>* x = static_cast<const Cx<T>*>(a.x[w.k]);
    const Cx<T>* q = BAR ? static_cast<const Cx<T>*>(a.q[w.k]) : x;
    Cx<T>* y[3] = {static_cast<Cx<T>*>(a.y[w.k][0]), static_cast<Cx<T>*>(a.y[w.k][D >= 2 ? 1 : 0]), static_cast<Cx<T>*>(a.y[w.k][D >= 3 ? 2 : 0])};
    const T sigma = (T)a.sigma, t = (T)a.tv[w.k];
    const int N0 = a.N[0], N1 = a.N[1], N2 = a.N[2];
    const int64_t SM = D == 2 ? (int64_t)N0 : (int64_t)N0 * N1;
    const int NM = D == 2 ? N1 : N2;
    double sum = 0.0;
    if (w.inside) {
        int im = D == 2 ? w.i1 : w.i2;
        int64_t at = w.at;
        // neighbours that do not move with the march: i0 + V (one cell), and for D = 3 row i1 + 1
        const int64_t right = w.i0 + V == N0 ? (int64_t)V - N0 : V;
        const int64_t down = w.i1 + 1 == N1 ? -(int64_t)N0 * (N1 - 1) : (int64_t)N0;
        P xc = load_cells<T, V>(x, at), qc{};
        if (BAR) qc = load_cells<T, V>(q, at);
        for (int m = 0; m < w.steps; ++m) {
            P gx[D], gq[D];                                          // (∇x⁺)_d and (∇x̄)_d of the lane's cells
            {
                P n;
                n.v[V - 1] = x[at + right];
                if (V == 2) n.v[0] = xc.v[V - 1];
                gx[0] = sub(n, xc);
                if (BAR) {
                    n.v[V - 1] = q[at + right];
                    if (V == 2) n.v[0] = qc.v[V - 1];
                    gq[0] = sub(n, qc);
                }
            }
            if (D == 3) {
                gx[1] = sub(load_cells<T, V>(x, at + down), xc);
                if (BAR) gq[1] = sub(load_cells<T, V>(q, at + down), qc);
            }
            if (D >= 2) {
                const int64_t nx = im + 1 == NM ? at - SM * (NM - 1) : at + SM;
                const P xn = load_cells<T, V>(x, nx);
                gx[D - 1] = sub(xn, xc);
                xc = xn;
                if (BAR) {
                    const P qn = load_cells<T, V>(q, nx);
                    gq[D - 1] = sub(qn, qc);
                    qc = qn;
                }
            }
            if (SUM) {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    double s2 = 0.0;
#pragma unroll
                    for (int d = 0; d < D; ++d) s2 += (double)gx[d].v[e].re * (double)gx[d].v[e].re + (double)gx[d].v[e].im * (double)gx[d].v[e].im;
                    sum += sqrt(s2);
                }
            }
            if (MODE == TV_GRADIENT) {
#pragma unroll
                for (int d = 0; d < D; ++d) store_cells<T, V>(y[d], at, gx[d]);
            }
            if (MODE == TV_DUAL) {
                P v[D];
                T s2[V];
#pragma unroll
                for (int e = 0; e < V; ++e) s2[e] = T(0);
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    v[d] = load_cells<T, V>(y[d], at);
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        v[d].v[e].re += sigma * gq[d].v[e].re;
                        v[d].v[e].im += sigma * gq[d].v[e].im;
                        s2[e] += v[d].v[e].re * v[d].v[e].re + v[d].v[e].im * v[d].v[e].im;
                    }
                }
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const T nrm = sqrt(s2[e]);
                    s2[e] = nrm > t ? t / nrm : T(1);
                }
#pragma unroll
                for (int d = 0; d < D; ++d) {
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        v[d].v[e].re *= s2[e];
                        v[d].v[e].im *= s2[e];
                    }
                    store_cells<T, V>(y[d], at, v[d]);
                }
            }
            ++im;
            at += SM;
        }
    }
    if (SUM) {
        sum = block_reduce<Sum>(sum, red);
        if (threadIdx.x == 0) a.part[(int64_t)w.c * a.G + w.g] = sum;
    }
}

// x = 0 unless WARM;  y = 0;  the first workgroup of a component resets its scalars and fills its history with NaN
template <typename T, bool WARM>
__global__ __launch_bounds__(kThreads) void tv_start_kernel(TvSolve a) {
    constexpr int W = Pack<T>::W;
    const int c = a.c0 + blockIdx.y;
    {
        T* y = static_cast<T*>(a.y) + c * a.ystride;                 // whole packs: the arrays are padded to 256 bytes
        NUFFT_FOR_EACH_PACK(T, a.ystride, i) {
            store(y, i, Pack<T>{});
            if (i + step__ < npacks__) store(y, i + step__, Pack<T>{});
        }
    }
    if (!WARM) {
        T* x = static_cast<T*>(a.x[blockIdx.y]);
        const int64_t nreal = 2 * a.n;
        NUFFT_FOR_EACH_PACK(T, nreal, i) {
            store(x, i, Pack<T>{});
            if (i + step__ < npacks__) store(x, i + step__, Pack<T>{});
        }
        if (blockIdx.x == 0 && threadIdx.x == 0)
            for (int64_t e = npacks__ * W; e < nreal; ++e) x[e] = T(0);
    }
    if (blockIdx.x == 0) reset_outcome<2>(a.s, c, a.C, a.max_iter);
}

// One workgroup per component: change, Σ_i |(∇x⁺)_i|₂, the history row and the done flag of iteration a.it.  Coupled components are one
// system: the sums run over all components' rows (contiguous), and every component stores the same outcome in its own slots.
__global__ __launch_bounds__(kThreads) void tv_decide_kernel(TvSolve a) {
    __shared__ double lds[kWaves];
    const int c = a.c0 + blockIdx.y;
    if (a.s.flag[c]) return;
    const int sc = a.joint ? 0 : c;
    const int rows = (int)((a.joint ? a.C : 1) * a.P);
    const double* pp = a.part_p + (int64_t)sc * a.P * 2;
    const double dd = row_reduce<Sum>(pp, rows, 2, lds);
    const double xx = row_reduce<Sum>(pp + 1, rows, 2, lds);
    const double tv = row_reduce<Sum>(a.part_d + (int64_t)sc * a.P, rows, 1, lds);
    if (threadIdx.x == 0) {
        const int64_t row = ((int64_t)(a.it - 1) * a.C + c) * 2;
        store_decision(a.s, c, row, dd, xx, a.tol, a.it);
        a.s.history[row + 1] = tv;
    }
}

__global__ __launch_bounds__(kThreads) void tv_sum_kernel(const double* part, int64_t P, double* out) {
    __shared__ double red[kWaves];
    const double s = row_reduce<Sum>(part + (int64_t)blockIdx.x * P, (int)P, 1, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

template <typename K>
hipError_t launch(const TvLaunch& a, K kernel, hipStream_t stream) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)a.tiles[0], (unsigned)a.tiles[1], (unsigned)(a.tiles[2] * a.nc)), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

// the instantiation for (element type, row alignment, D)
#define NUFFT_TV_DISPATCH(kernel, MODE)                                                         \
    if (a.dtype == NUFFT_F64) {                                                                 \
        if (a.D == 1) return launch(a, kernel<double, 1, 1, MODE>, stream);                     \
        if (a.D == 2) return launch(a, kernel<double, 2, 1, MODE>, stream);                     \
        return launch(a, kernel<double, 3, 1, MODE>, stream);                                   \
    }                                                                                           \
    if (a.wide) {                                                                               \
        if (a.D == 1) return launch(a, kernel<float, 1, 2, MODE>, stream);                      \
        if (a.D == 2) return launch(a, kernel<float, 2, 2, MODE>, stream);                      \
        return launch(a, kernel<float, 3, 2, MODE>, stream);                                    \
    }                                                                                           \
    if (a.D == 1) return launch(a, kernel<float, 1, 1, MODE>, stream);                          \
    if (a.D == 2) return launch(a, kernel<float, 2, 1, MODE>, stream);                          \
    return launch(a, kernel<float, 3, 1, MODE>, stream)

}  // namespace

hipError_t launch_tv(const TvLaunch& a, TvMode mode, hipStream_t stream) {
    switch (mode) {
        case TV_PRIMAL: NUFFT_TV_DISPATCH(tv_primal_kernel, TV_PRIMAL);
        case TV_ADJOINT: NUFFT_TV_DISPATCH(tv_primal_kernel, TV_ADJOINT);
        case TV_DUAL: NUFFT_TV_DISPATCH(tv_dual_kernel, TV_DUAL);
        case TV_GRADIENT: NUFFT_TV_DISPATCH(tv_dual_kernel, TV_GRADIENT);
        default: NUFFT_TV_DISPATCH(tv_dual_kernel, TV_NORM);
    }
}

hipError_t launch_tv_start(const TvSolve& a, bool warm, hipStream_t stream) {
    const dim3 gr(a.G, a.nc), bl(kThreads);
    if (warm) return launch_by_dtype(a.dtype, gr, bl, stream, tv_start_kernel<float, true>, tv_start_kernel<double, true>, a);
    return launch_by_dtype(a.dtype, gr, bl, stream, tv_start_kernel<float, false>, tv_start_kernel<double, false>, a);
}

hipError_t launch_tv_decide(const TvSolve& a, hipStream_t stream) {
    hipLaunchKernelGGL(tv_decide_kernel, dim3(1, a.nc), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_tv_sum(const double* part, int64_t P, int C, double* out, hipStream_t stream) {
    hipLaunchKernelGGL(tv_sum_kernel, dim3(C), dim3(kThreads), 0, stream, part, P, out);
    return hipGetLastError();
}

}  // namespace nufft
