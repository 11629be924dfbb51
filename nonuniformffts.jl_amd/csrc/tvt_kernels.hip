// Kernels of the total variation along the components ("frames") and of its part in the primal-dual solver (tv.cpp; DESIGN.md
// section 26).
//
//     (∇_t x)_c[i]  = x_{c+1}[i] − x_c[i]        c < K − 1;   c = K − 1:  x_0[i] − x_{K−1}[i] if periodic, else 0
//     (∇_tᴴ z)_c[i] = z_{c−1}[i] − z_c[i]        z_{−1} = z_{K−1} if periodic, else z_{−1} = z_{K−1} = 0
//
// The neighbour of a cell is the same index of another array, so nothing here knows the shape: the kernels are flat over the n cells of
// a frame.  The "primal" kernel reads z at frames c and c − 1 and writes only x_c and q_c; the "dual" one reads x̄ and x⁺ at frames c and
// c + 1 and writes only z_c: as in tv_kernels.hip no launch reads at a neighbour an array it writes, so nothing races, nothing is
// double-buffered and there are no atomics.  The pointers are kernel arguments widened by one frame on each side of the batch
// (TvtLaunch): a null slot is a frame that is zero or absent on the non-periodic axis, decided per workgroup, never per cell.
//
// A lane owns kTvtPacks 16-byte packs, 256 lanes apart.  Sums are FP64, one plain store per workgroup, reduced later in one fixed order.
// A frozen system's workgroups leave after reading the flag, before the first data load.
#include <hip/hip_runtime.h>

#include <cmath>

#include "nufft_mi355x.h"
#include "stream_kernels.h"
#include "tv.h"
#include "tv_cells.h"

namespace nufft {
using namespace stream;
using namespace tvcells;
namespace {

// x⁺ = x − τ (q + μ x − b + ∇_tᴴz);  x <- x⁺;  q <- x̄ = x⁺ + (x⁺ − x);  partials of ‖x⁺ − x‖², ‖x⁺‖²      (TVT_PRIMAL)
// x <- ∇_tᴴz                                                                                              (TVT_ADJOINT)
// q <- q + ∇_tᴴz   (the spatial primal kernel then takes q as it takes G x)                                (TVT_ADD)
template <typename T, int V, int MODE>
__global__ __launch_bounds__(kThreads) void tvt_primal_kernel(TvtLaunch a) {
    using P = Cells<T, V>;
    __shared__ double red[kWaves];
    const int k = blockIdx.y, c = a.c0 + k;
    if (a.flag && a.flag[c]) return;
    Cx<T>* x = static_cast<Cx<T>*>(a.x[k + 1]);
    Cx<T>* q = static_cast<Cx<T>*>(a.q[k + 1]);
    const Cx<T>* b = static_cast<const Cx<T>*>(a.b[k]);
    const Cx<T>* zc = static_cast<const Cx<T>*>(a.z[k + 1]);         // null: zero
    const Cx<T>* zp = static_cast<const Cx<T>*>(a.z[k]);             // frame c − 1; null: zero
    const T tau = (T)a.step, mu = (T)a.lambda;
    double sdd = 0.0, sxx = 0.0;
#pragma unroll
    for (int u = 0; u < kTvtPacks; ++u) {
        const int64_t at = (((int64_t)blockIdx.x * kTvtPacks + u) * kThreads + threadIdx.x) * V;
        if (at >= a.n) break;                                        // n is a multiple of V: a pack is inside or outside as a whole
        P div{};
        if (zp) div = load_cells<T, V>(zp, at);
        if (zc) div = sub(div, load_cells<T, V>(zc, at));
        if (MODE == TVT_ADJOINT) {
            store_cells<T, V>(x, at, div);
        } else if (MODE == TVT_ADD) {
            P qv = load_cells<T, V>(q, at);
#pragma unroll
            for (int e = 0; e < V; ++e) qv.v[e] = Cx<T>{qv.v[e].re + div.v[e].re, qv.v[e].im + div.v[e].im};
            store_cells<T, V>(q, at, qv);
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
    }
    if (MODE == TVT_PRIMAL) {
        sdd = block_reduce<Sum>(sdd, red);
        sxx = block_reduce<Sum>(sxx, red);
        if (threadIdx.x == 0) {
            double* out = a.part + ((int64_t)c * a.G + blockIdx.x) * 2;
            out[0] = sdd;
            out[1] = sxx;
        }
    }
}

// z_c <- P_{tv_t}(z_c + σ (∇_t x̄)_c),  P_t(v) = v · min(1, t / |v|) per cell;  partial of Σ_i |(∇_t x⁺)_c[i]|      (TVT_DUAL: x̄ in q, x⁺ in x)
// z_c <- (∇_t x)_c                                                                                                (TVT_GRADIENT)
// partial of Σ_i |(∇_t x)_c[i]|                                                                                   (TVT_NORM)
template <typename T, int V, int MODE>
__global__ __launch_bounds__(kThreads) void tvt_dual_kernel(TvtLaunch a) {
    using P = Cells<T, V>;
    __shared__ double red[kWaves];
    const int k = blockIdx.y, c = a.c0 + k;
    if (a.flag && a.flag[c]) return;
    constexpr bool SUM = MODE != TVT_GRADIENT;
    const Cx<T>* x = static_cast<const Cx<T>*>(a.x[k + 1]);
    const Cx<T>* xn = static_cast<const Cx<T>*>(a.x[k + 2]);         // frame c + 1; null: the difference is zero
    const Cx<T>* q = static_cast<const Cx<T>*>(a.q[k + 1]);
    const Cx<T>* qn = static_cast<const Cx<T>*>(a.q[k + 2]);
    Cx<T>* z = static_cast<Cx<T>*>(a.z[k + 1]);
    const T sigma = (T)a.sigma, t = (T)a.tv_t;
    double sum = 0.0;
#pragma unroll
    for (int u = 0; u < kTvtPacks; ++u) {
        const int64_t at = (((int64_t)blockIdx.x * kTvtPacks + u) * kThreads + threadIdx.x) * V;
        if (at >= a.n) break;
        P gx{}, gq{};
        if (xn) gx = sub(load_cells<T, V>(xn, at), load_cells<T, V>(x, at));
        if (MODE == TVT_DUAL && qn) gq = sub(load_cells<T, V>(qn, at), load_cells<T, V>(q, at));
        if (SUM) {
#pragma unroll
            for (int e = 0; e < V; ++e) sum += sqrt((double)gx.v[e].re * (double)gx.v[e].re + (double)gx.v[e].im * (double)gx.v[e].im);
        }
        if (MODE == TVT_GRADIENT) store_cells<T, V>(z, at, gx);
        if (MODE == TVT_DUAL) {
            P v = load_cells<T, V>(z, at);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                v.v[e].re += sigma * gq.v[e].re;
                v.v[e].im += sigma * gq.v[e].im;
                const T nrm = sqrt(v.v[e].re * v.v[e].re + v.v[e].im * v.v[e].im);
                const T s = nrm > t ? t / nrm : T(1);
                v.v[e].re *= s;
                v.v[e].im *= s;
            }
            store_cells<T, V>(z, at, v);
        }
    }
    if (SUM) {
        sum = block_reduce<Sum>(sum, red);
        if (threadIdx.x == 0) a.part[(int64_t)c * a.G + blockIdx.x] = sum;
    }
}

// One workgroup per component.  The frames are one system: the change comes from the rows of all components (contiguous), and every
// component stores the same outcome next to its own share of the prior.
__global__ __launch_bounds__(kThreads) void tvt_decide_kernel(TvtDecide a) {
    __shared__ double lds[kWaves];
    const int k = blockIdx.y, c = a.c0 + k;
    if (a.s.flag[c]) return;
    const int rows = (int)(a.C * a.Pp);
    const double dd = row_reduce<Sum>(a.part_p, rows, 2, lds);
    const double xx = row_reduce<Sum>(a.part_p + 1, rows, 2, lds);
    const double tt = row_reduce<Sum>(a.part_t + (int64_t)c * a.Pt, (int)a.Pt, 1, lds);
    double ts = 0.0;
    if (a.part_s) ts = row_reduce<Sum>(a.part_s + (int64_t)c * a.Ps, (int)a.Ps, 1, lds);
    if (threadIdx.x == 0) {
        const int64_t row = ((int64_t)(a.it - 1) * a.C + c) * 2;
        store_decision(a.s, c, row, dd, xx, a.tol, a.it);
        a.s.history[row + 1] = a.part_s ? a.tv[k] * ts + a.tv_t * tt : a.tv_t * tt;
    }
}

template <typename K>
hipError_t launch(const TvtLaunch& a, K kernel, hipStream_t stream) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)a.G, (unsigned)a.nc), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

// the instantiation for (element type, pack)
#define NUFFT_TVT_DISPATCH(kernel, MODE)                                                \
    if (a.dtype == NUFFT_F64) return launch(a, kernel<double, 1, MODE>, stream);        \
    if (a.wide) return launch(a, kernel<float, 2, MODE>, stream);                       \
    return launch(a, kernel<float, 1, MODE>, stream)

}  // namespace

hipError_t launch_tvt(const TvtLaunch& a, TvtMode mode, hipStream_t stream) {
    switch (mode) {
        case TVT_PRIMAL: NUFFT_TVT_DISPATCH(tvt_primal_kernel, TVT_PRIMAL);
        case TVT_ADJOINT: NUFFT_TVT_DISPATCH(tvt_primal_kernel, TVT_ADJOINT);
        case TVT_ADD: NUFFT_TVT_DISPATCH(tvt_primal_kernel, TVT_ADD);
        case TVT_DUAL: NUFFT_TVT_DISPATCH(tvt_dual_kernel, TVT_DUAL);
        case TVT_GRADIENT: NUFFT_TVT_DISPATCH(tvt_dual_kernel, TVT_GRADIENT);
        default: NUFFT_TVT_DISPATCH(tvt_dual_kernel, TVT_NORM);
    }
}

hipError_t launch_tvt_decide(const TvtDecide& a, hipStream_t stream) {
    hipLaunchKernelGGL(tvt_decide_kernel, dim3(1, a.nc), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace nufft
