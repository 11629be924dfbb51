// Streaming kernels of the FISTA solver and of the power iteration (fista.cpp, toeplitz.cpp).
//
// Every scalar here is real, so the kernels treat a component as a vector of 2n reals, gridDim.y = component.  Packs, the loop shape and
// the fixed-order reduction of per-workgroup partials are those of stream_kernels.h.  A component whose done flag is set is frozen: its
// workgroups leave after reading the flag.  The flags change only in fista_decide_kernel, a launch of its own.
#include <hip/hip_runtime.h>

#include <cmath>

#include "fista.h"
#include "nufft_mi355x.h"
#include "solver_decide.h"
#include "stream_kernels.h"

namespace nufft {
using namespace stream;

// one decision step for the three solvers (solver_decide.h)
static_assert(NUFFT_FISTA_MAX_ITER == kProxMaxIter && NUFFT_FISTA_CONVERGED == kProxConverged && NUFFT_FISTA_BREAKDOWN == kProxBreakdown, "status values");
static_assert(NUFFT_TVPD_MAX_ITER == kProxMaxIter && NUFFT_TVPD_CONVERGED == kProxConverged && NUFFT_TVPD_BREAKDOWN == kProxBreakdown, "status values");
static_assert(NUFFT_LPS_MAX_ITER == kProxMaxIter && NUFFT_LPS_CONVERGED == kProxConverged && NUFFT_LPS_BREAKDOWN == kProxBreakdown, "status values");

namespace {

// z = x (WARM) or x = z = 0;  the first workgroup of a component resets its scalars and fills its history with NaN
template <typename T, bool WARM>
__global__ __launch_bounds__(kThreads) void fista_start_kernel(FistaLaunch a) {
    constexpr int W = Pack<T>::W;
    const int c = a.c0 + blockIdx.y;
    T* x = static_cast<T*>(a.x[blockIdx.y]);
    T* z = static_cast<T*>(a.z) + c * a.stride;
    const int64_t nreal = 2 * a.n;
    NUFFT_FOR_EACH_PACK(T, nreal, i) {
        const int64_t j = i + step__;
        const bool two = j < npacks__;
        if (WARM) {
            store(z, i, load(x, i));
            if (two) store(z, j, load(x, j));
        } else {
            store(x, i, Pack<T>{});
            store(z, i, Pack<T>{});
            if (two) {
                store(x, j, Pack<T>{});
                store(z, j, Pack<T>{});
            }
        }
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0)
            for (int64_t e = npacks__ * W; e < nreal; ++e) {
                if (!WARM) x[e] = T(0);
                z[e] = WARM ? x[e] : T(0);
            }
        reset_outcome<2>(a.s, c, a.C, a.max_iter);
    }
}

// q <- z − τ (q + μ z − b)
template <typename T>
__global__ __launch_bounds__(kThreads) void fista_gradient_kernel(FistaLaunch a) {
    constexpr int W = Pack<T>::W;
    const int c = a.c0 + blockIdx.y;
    if (a.s.flag[c]) return;
    const T* z = static_cast<const T*>(a.z) + c * a.stride;
    T* q = static_cast<T*>(a.q) + c * a.stride;
    const T* b = static_cast<const T*>(a.b[blockIdx.y]);
    const T tau = (T)a.step, mu = (T)a.lambda;
    const int64_t nreal = 2 * a.n;
    auto one = [&](T zv, T qv, T bv) { return zv - tau * (qv + mu * zv - bv); };
    NUFFT_FOR_EACH_PACK(T, nreal, i) {
        const int64_t j = i + step__;
        const bool two = j < npacks__;
        Pack<T> z0 = load(z, i), q0 = load(q, i), b0 = load(b, i), z1{}, q1{}, b1{};
        if (two) { z1 = load(z, j); q1 = load(q, j); b1 = load(b, j); }
#pragma unroll
        for (int w = 0; w < W; ++w) q0.v[w] = one(z0.v[w], q0.v[w], b0.v[w]);
        store(q, i, q0);
        if (two) {
#pragma unroll
            for (int w = 0; w < W; ++w) q1.v[w] = one(z1.v[w], q1.v[w], b1.v[w]);
            store(q, j, q1);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t e = npacks__ * W; e < nreal; ++e) q[e] = one(z[e], q[e], b[e]);
}

// One workgroup per component: change, ‖D W x‖₁, the history row and the done flag of iteration a.it
__global__ __launch_bounds__(kThreads) void fista_decide_kernel(FistaLaunch a) {
    __shared__ double lds[kWaves];
    const int c = a.c0 + blockIdx.y;
    if (a.s.flag[c]) return;
    const int sc = a.joint ? 0 : c;
    const int rows = a.joint ? a.C : 1;
    const double* mp = a.mom_part + (int64_t)sc * a.G0 * 2;
    const double dd = row_reduce<Sum>(mp, rows * a.G0, 2, lds);
    const double xx = row_reduce<Sum>(mp + 1, rows * a.G0, 2, lds);
    const double l1 = row_reduce<Sum>(a.l1_part + (int64_t)sc * a.P, rows * a.P, 1, lds);
    if (threadIdx.x == 0) {
        const int64_t row = ((int64_t)(a.it - 1) * a.C + c) * 2;
        store_decision(a.s, c, row, dd, xx, a.tol, a.it);
        a.s.history[row + 1] = l1;
    }
}

// The decision of a solver with the locally low-rank prior: ONE system whatever the operator, so one workgroup sums the rows
// part[g][3] (‖x⁺ − x‖², ‖x⁺‖², Σ kept singular values) of the fused kernel's workgroups and stores the same outcome for every component
__global__ __launch_bounds__(kThreads) void fista_decide_llr_kernel(FistaLaunch a, const double* part, int64_t G) {
    __shared__ double lds[kWaves];
    if (a.s.flag[0]) return;
    double dd = 0.0, xx = 0.0, nuc = 0.0;
    for (int64_t g = threadIdx.x; g < G; g += kThreads) {
        dd += part[g * 3];
        xx += part[g * 3 + 1];
        nuc += part[g * 3 + 2];
    }
    dd = block_reduce<Sum>(dd, lds);
    xx = block_reduce<Sum>(xx, lds);
    nuc = block_reduce<Sum>(nuc, lds);
    if (threadIdx.x == 0)
        for (int c = 0; c < a.C; ++c) {
            const int64_t row = ((int64_t)(a.it - 1) * a.C + c) * 2;
            store_decision(a.s, c, row, dd, xx, a.tol, a.it);
            a.s.history[row + 1] = nuc;
        }
}

// partial sums of Re<v, g>, <v, v>, <g, g>
template <typename T>
__global__ __launch_bounds__(kThreads) void power_dot_kernel(PowerLaunch a) {
    __shared__ double lds[kWaves];
    constexpr int W = Pack<T>::W;
    const int c = blockIdx.y;
    const T* v = static_cast<const T*>(a.v) + c * a.stride;
    const T* g = static_cast<const T*>(a.g) + c * a.stride;
    const int64_t nreal = 2 * a.n;
    double svg = 0.0, svv = 0.0, sgg = 0.0;
    auto one = [&](T vv, T gv) {
        svg += (double)vv * (double)gv;
        svv += (double)vv * (double)vv;
        sgg += (double)gv * (double)gv;
    };
    NUFFT_FOR_EACH_PACK(T, nreal, i) {
        const int64_t j = i + step__;
        const bool two = j < npacks__;
        Pack<T> v0 = load(v, i), g0 = load(g, i), v1{}, g1{};
        if (two) { v1 = load(v, j); g1 = load(g, j); }
#pragma unroll
        for (int w = 0; w < W; ++w) one(v0.v[w], g0.v[w]);
#pragma unroll
        for (int w = 0; w < W; ++w) one(v1.v[w], g1.v[w]);      // zeros when there is no second pack
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t e = npacks__ * W; e < nreal; ++e) one(v[e], g[e]);
    svg = block_reduce<Sum>(svg, lds);
    svv = block_reduce<Sum>(svv, lds);
    sgg = block_reduce<Sum>(sgg, lds);
    if (threadIdx.x == 0) {
        double* out = a.part + ((int64_t)c * a.G + blockIdx.x) * 3;
        out[0] = svg;
        out[1] = svv;
        out[2] = sgg;
    }
}

// rho = Re<v, g> / <v, v> (0 for v = 0);  v = g / ‖g‖ (g = 0: v = 0)
template <typename T>
__global__ __launch_bounds__(kThreads) void power_scale_kernel(PowerLaunch a) {
    __shared__ double lds[kWaves];
    constexpr int W = Pack<T>::W;
    const int c = blockIdx.y;
    const int sc = a.joint ? 0 : c, GR = a.joint ? a.C * a.G : a.G;
    const double* row = a.part + (int64_t)sc * a.G * 3;
    const double vg = row_reduce<Sum>(row, GR, 3, lds);
    const double vv = row_reduce<Sum>(row + 1, GR, 3, lds);
    const double gg = row_reduce<Sum>(row + 2, GR, 3, lds);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.rho[c] = vv > 0.0 ? vg / vv : 0.0;
    const T s = gg > 0.0 ? (T)(1.0 / sqrt(gg)) : T(0);
    T* v = static_cast<T*>(a.v) + c * a.stride;
    const T* g = static_cast<const T*>(a.g) + c * a.stride;
    const int64_t nreal = 2 * a.n;
    NUFFT_FOR_EACH_PACK(T, nreal, i) {
        const int64_t j = i + step__;
        const bool two = j < npacks__;
        Pack<T> g0 = load(g, i), g1{};
        if (two) g1 = load(g, j);
#pragma unroll
        for (int w = 0; w < W; ++w) g0.v[w] *= s;
        store(v, i, g0);
        if (two) {
#pragma unroll
            for (int w = 0; w < W; ++w) g1.v[w] *= s;
            store(v, j, g1);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t e = npacks__ * W; e < nreal; ++e) v[e] = g[e] * s;
}

}  // namespace

int fista_workgroups(int dtype, int64_t n, int num_cus) { return stream_workgroups((2 * n) / (dtype == NUFFT_F32 ? 4 : 2), num_cus); }

hipError_t launch_fista_start(const FistaLaunch& a, bool warm, hipStream_t stream) {
    const dim3 gr(a.G, a.nc), bl(kThreads);
    if (warm) return launch_by_dtype(a.dtype, gr, bl, stream, fista_start_kernel<float, true>, fista_start_kernel<double, true>, a);
    return launch_by_dtype(a.dtype, gr, bl, stream, fista_start_kernel<float, false>, fista_start_kernel<double, false>, a);
}

hipError_t launch_fista_gradient(const FistaLaunch& a, hipStream_t stream) {
    return launch_by_dtype(a.dtype, dim3(a.G, a.nc), dim3(kThreads), stream, fista_gradient_kernel<float>, fista_gradient_kernel<double>, a);
}

hipError_t launch_fista_decide(const FistaLaunch& a, hipStream_t stream) {
    hipLaunchKernelGGL(fista_decide_kernel, dim3(1, a.nc), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_fista_decide_llr(const FistaLaunch& a, const double* part, int64_t G, hipStream_t stream) {
    hipLaunchKernelGGL(fista_decide_llr_kernel, dim3(1), dim3(kThreads), 0, stream, a, part, G);
    return hipGetLastError();
}

hipError_t launch_power_dot(const PowerLaunch& a, hipStream_t stream) {
    return launch_by_dtype(a.dtype, dim3(a.G, a.C), dim3(kThreads), stream, power_dot_kernel<float>, power_dot_kernel<double>, a);
}

hipError_t launch_power_scale(const PowerLaunch& a, hipStream_t stream) {
    return launch_by_dtype(a.dtype, dim3(a.G, a.C), dim3(kThreads), stream, power_scale_kernel<float>, power_scale_kernel<double>, a);
}

}  // namespace nufft
