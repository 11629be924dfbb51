// Kernels of the conjugate-gradient solver on the Toeplitz normal operator (cg.cpp).
//
// Every scalar of CG here is real (α, ρ'/ρ, λ) and Re<p, q> = Σ over the 2n reals of p ⊙ q, so the kernels treat a component as a
// vector of 2n reals, gridDim.y = component.  Packs, the loop shape and the fixed-order reduction of the per-workgroup partials, which
// makes every run and every graph replay get the same bits, are those of stream_kernels.h.
//
// A component whose done flag is set is frozen: its workgroups leave after reading the flag.  The first workgroup of the last
// kernel of an iteration writes the scalars of the next one into the other parity slot (every workgroup of that kernel still reads
// the current slot); for a frozen component it only carries flag and ρ over.
//
// Joint mode (CgLaunch::joint: the operator couples its components): the components are one system.  The
// partial-sum rows of all components are contiguous, so every reduction runs over C * G entries from component 0's row, in the same
// fixed order; every component reads the scalars of slot 0 — all components then take the same decisions — and writes the values it
// computed, the same in every component, to its own slot, which is what the host reads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cg.h"
#include "nufft_mi355x.h"
#include "stream_kernels.h"

namespace nufft {
using namespace stream;
namespace {

__device__ __forceinline__ double relative(double rho, double beta0) {
    return beta0 > 0.0 ? sqrt(rho / beta0) : (rho == 0.0 ? 0.0 : INFINITY);
}

// r = b − (q + λ x) (WARM; q = G x) or r = b, x = 0;  p = r;  partial sums of |r|² and |b|²
template <typename T, bool WARM>
__global__ __launch_bounds__(kThreads) void cg_residual_kernel(CgLaunch a) {
    __shared__ double lds[kWaves];
    constexpr int W = Pack<T>::W;
    const int c = a.c0 + blockIdx.y;
    T* x = static_cast<T*>(a.x[blockIdx.y]);
    const T* b = static_cast<const T*>(a.b[blockIdx.y]);
    T* r = static_cast<T*>(a.r) + c * a.stride;
    T* p = static_cast<T*>(a.p) + c * a.stride;
    const T* q = static_cast<const T*>(a.q) + c * a.stride;
    const T lam = (T)a.lambda;
    const int64_t nreal = 2 * a.n;
    double srr = 0.0, sbb = 0.0;
    auto one = [&](T bv, T qv, T xv) {
        const T rv = WARM ? bv - (qv + lam * xv) : bv;
        srr += (double)rv * (double)rv;
        sbb += (double)bv * (double)bv;
        return rv;
    };
    NUFFT_FOR_EACH_PACK(T, nreal, i) {
        const int64_t j = i + step__;
        const bool two = j < npacks__;
        Pack<T> b0 = load(b, i), b1{}, q0{}, q1{}, x0{}, x1{};
        if (two) b1 = load(b, j);
        if (WARM) {
            q0 = load(q, i);
            x0 = load(x, i);
            if (two) { q1 = load(q, j); x1 = load(x, j); }
        }
        Pack<T> r0, r1;
#pragma unroll
        for (int w = 0; w < W; ++w) r0.v[w] = one(b0.v[w], q0.v[w], x0.v[w]);
        store(r, i, r0);
        store(p, i, r0);
        if (!WARM) store(x, i, Pack<T>{});
        if (two) {
#pragma unroll
            for (int w = 0; w < W; ++w) r1.v[w] = one(b1.v[w], q1.v[w], x1.v[w]);
            store(r, j, r1);
            store(p, j, r1);
            if (!WARM) store(x, j, Pack<T>{});
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t e = npacks__ * W; e < nreal; ++e) {
            const T rv = one(b[e], WARM ? q[e] : T(0), WARM ? x[e] : T(0));
            r[e] = rv;
            p[e] = rv;
            if (!WARM) x[e] = T(0);
        }
    srr = block_reduce<Sum>(srr, lds);
    sbb = block_reduce<Sum>(sbb, lds);
    if (threadIdx.x == 0) {
        double* out = a.s.part1 + ((int64_t)c * a.G + blockIdx.x) * 2;
        out[0] = srr;
        out[1] = sbb;
    }
}

// One workgroup per component: the scalars before the first iteration, and NaN into the history rows no iteration has written.
__global__ __launch_bounds__(kThreads) void cg_start_kernel(CgLaunch a) {
    __shared__ double lds[kWaves];
    const int c = a.c0 + blockIdx.y;
    const int GR = a.joint ? a.C * a.G : a.G;      // joint: one sum over all components
    const double* row = a.s.part1 + (int64_t)(a.joint ? 0 : c) * a.G * 2;
    const double rr = row_reduce<Sum>(row, GR, 2, lds);
    const double bb = row_reduce<Sum>(row + 1, GR, 2, lds);
    for (int it = 1 + threadIdx.x; it <= a.max_iter; it += kThreads) a.s.history[(int64_t)it * a.C + c] = NAN;
    if (threadIdx.x == 0) {
        const int done = rr <= a.rtol * a.rtol * bb ? 1 : 0;
        a.s.rho[c] = rr;
        a.s.rho[a.C + c] = rr;
        a.s.beta0[c] = bb;
        a.s.res[c] = relative(rr, bb);
        a.s.history[c] = relative(rr, bb);
        a.s.flag[c] = done;
        a.s.flag[a.C + c] = done;
        a.s.brk[c] = 0;
        a.s.iters[c] = 0;
        a.s.status[c] = done ? NUFFT_CG_CONVERGED : NUFFT_CG_MAX_ITER;
    }
}

// Kernel 1: partial sums of Re<p, q> and |p|²
template <typename T>
__global__ __launch_bounds__(kThreads) void cg_dot_kernel(CgLaunch a) {
    __shared__ double lds[kWaves];
    constexpr int W = Pack<T>::W;
    const int c = a.c0 + blockIdx.y;
    if (a.s.flag[(a.it & 1) * a.C + (a.joint ? 0 : c)]) return;
    const T* p = static_cast<const T*>(a.p) + c * a.stride;
    const T* q = static_cast<const T*>(a.q) + c * a.stride;
    const int64_t nreal = 2 * a.n;
    double spq = 0.0, spp = 0.0;
    NUFFT_FOR_EACH_PACK(T, nreal, i) {
        const int64_t j = i + step__;
        const bool two = j < npacks__;
        Pack<T> p0 = load(p, i), q0 = load(q, i), p1{}, q1{};
        if (two) { p1 = load(p, j); q1 = load(q, j); }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            spq += (double)p0.v[w] * (double)q0.v[w];
            spp += (double)p0.v[w] * (double)p0.v[w];
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {      // zeros when there is no second pack
            spq += (double)p1.v[w] * (double)q1.v[w];
            spp += (double)p1.v[w] * (double)p1.v[w];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t e = npacks__ * W; e < nreal; ++e) {
            spq += (double)p[e] * (double)q[e];
            spp += (double)p[e] * (double)p[e];
        }
    spq = block_reduce<Sum>(spq, lds);
    spp = block_reduce<Sum>(spp, lds);
    if (threadIdx.x == 0) {
        double* out = a.s.part1 + ((int64_t)c * a.G + blockIdx.x) * 2;
        out[0] = spq;
        out[1] = spp;
    }
}

// Kernel 2: γ = Re<p, q> + λ|p|² from kernel 1's partials, α = ρ / γ;  x += α p;  r −= α (q + λ p);  partial sums of |r|²
template <typename T>
__global__ __launch_bounds__(kThreads) void cg_update_kernel(CgLaunch a) {
    __shared__ double lds[kWaves];
    constexpr int W = Pack<T>::W;
    const int c = a.c0 + blockIdx.y;
    const int sc = a.joint ? 0 : c, GR = a.joint ? a.C * a.G : a.G;
    const int slot = (a.it & 1) * a.C + sc;
    if (a.s.flag[slot]) return;
    const double* row = a.s.part1 + (int64_t)sc * a.G * 2;
    const double pq = row_reduce<Sum>(row, GR, 2, lds);
    const double pp = row_reduce<Sum>(row + 1, GR, 2, lds);
    const double gamma = pq + a.lambda * pp;
    const bool bad = !(gamma > 0.0) || !isfinite(gamma);      // the same bits in every workgroup: they all leave, or none does
    if (blockIdx.x == 0 && threadIdx.x == 0) a.s.brk[c] = bad ? 1 : 0;
    if (bad) return;
    const T al = (T)(a.s.rho[slot] / gamma), lam = (T)a.lambda;
    T* x = static_cast<T*>(a.x[blockIdx.y]);
    T* r = static_cast<T*>(a.r) + c * a.stride;
    const T* p = static_cast<const T*>(a.p) + c * a.stride;
    const T* q = static_cast<const T*>(a.q) + c * a.stride;
    const int64_t nreal = 2 * a.n;
    double srr = 0.0;
    auto one = [&](T& xv, T& rv, T pv, T qv) {
        xv += al * pv;
        rv -= al * (qv + lam * pv);
        srr += (double)rv * (double)rv;
    };
    NUFFT_FOR_EACH_PACK(T, nreal, i) {
        const int64_t j = i + step__;
        const bool two = j < npacks__;
        Pack<T> x0 = load(x, i), r0 = load(r, i), p0 = load(p, i), q0 = load(q, i), x1{}, r1{}, p1{}, q1{};
        if (two) { x1 = load(x, j); r1 = load(r, j); p1 = load(p, j); q1 = load(q, j); }
#pragma unroll
        for (int w = 0; w < W; ++w) one(x0.v[w], r0.v[w], p0.v[w], q0.v[w]);
        store(x, i, x0);
        store(r, i, r0);
        if (two) {
#pragma unroll
            for (int w = 0; w < W; ++w) one(x1.v[w], r1.v[w], p1.v[w], q1.v[w]);
            store(x, j, x1);
            store(r, j, r1);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t e = npacks__ * W; e < nreal; ++e) one(x[e], r[e], p[e], q[e]);
    srr = block_reduce<Sum>(srr, lds);
    if (threadIdx.x == 0) a.s.part2[(int64_t)c * a.G + blockIdx.x] = srr;
}

// Kernel 3: ρ' from kernel 2's partials;  p = r + (ρ'/ρ) p;  the first workgroup writes the scalars of the next iteration
template <typename T>
__global__ __launch_bounds__(kThreads) void cg_direction_kernel(CgLaunch a) {
    __shared__ double lds[kWaves];
    constexpr int W = Pack<T>::W;
    const int c = a.c0 + blockIdx.y;
    const int sc = a.joint ? 0 : c, GR = a.joint ? a.C * a.G : a.G;
    const int slot = (a.it & 1) * a.C + sc, next = ((a.it + 1) & 1) * a.C + c;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    const bool frozen = a.s.flag[slot] != 0, bad = !frozen && a.s.brk[sc] != 0;
    if (frozen || bad) {
        if (first) {
            a.s.flag[next] = 1;
            a.s.rho[next] = a.s.rho[slot];
            if (bad) a.s.status[c] = NUFFT_CG_BREAKDOWN;
        }
        return;
    }
    const double rr = row_reduce<Sum>(a.s.part2 + (int64_t)sc * a.G, GR, 1, lds);
    const T bt = (T)(rr / a.s.rho[slot]);           // ρ > 0: the component is not done
    const T* r = static_cast<const T*>(a.r) + c * a.stride;
    T* p = static_cast<T*>(a.p) + c * a.stride;
    const int64_t nreal = 2 * a.n;
    NUFFT_FOR_EACH_PACK(T, nreal, i) {
        const int64_t j = i + step__;
        const bool two = j < npacks__;
        Pack<T> r0 = load(r, i), p0 = load(p, i), r1{}, p1{};
        if (two) { r1 = load(r, j); p1 = load(p, j); }
#pragma unroll
        for (int w = 0; w < W; ++w) p0.v[w] = r0.v[w] + bt * p0.v[w];
        store(p, i, p0);
        if (two) {
#pragma unroll
            for (int w = 0; w < W; ++w) p1.v[w] = r1.v[w] + bt * p1.v[w];
            store(p, j, p1);
        }
    }
    if (first) {
        for (int64_t e = npacks__ * W; e < nreal; ++e) p[e] = r[e] + bt * p[e];
        const double bb = a.s.beta0[sc];
        const int done = rr <= a.rtol * a.rtol * bb ? 1 : 0;
        a.s.rho[next] = rr;
        a.s.flag[next] = done;
        a.s.res[c] = relative(rr, bb);
        a.s.history[(int64_t)a.it * a.C + c] = relative(rr, bb);
        a.s.iters[c] = a.it;
        a.s.status[c] = done ? NUFFT_CG_CONVERGED : NUFFT_CG_MAX_ITER;
    }
}

// The preconditioned iteration (joint mode as in the plain kernels, for the block preconditioner of section 22).  Kernel 2': as cg_update_kernel with α = ρ_z / γ, ρ_z = Re<r, z> of the iteration before.
template <typename T>
__global__ __launch_bounds__(kThreads) void pcg_update_kernel(CgLaunch a) {
    __shared__ double lds[kWaves];
    constexpr int W = Pack<T>::W;
    const int c = a.c0 + blockIdx.y;
    const int sc = a.joint ? 0 : c, GR = a.joint ? a.C * a.G : a.G;
    const int slot = (a.it & 1) * a.C + sc;
    if (a.s.flag[slot]) return;
    const double* row = a.s.part1 + (int64_t)sc * a.G * 2;
    const double pq = row_reduce<Sum>(row, GR, 2, lds);
    const double pp = row_reduce<Sum>(row + 1, GR, 2, lds);
    const double gamma = pq + a.lambda * pp;
    const bool bad = !(gamma > 0.0) || !isfinite(gamma);      // the same bits in every workgroup: they all leave, or none does
    if (blockIdx.x == 0 && threadIdx.x == 0) a.s.brk[c] = bad ? 1 : 0;
    if (bad) return;
    const T al = (T)(a.s.rhoz[slot] / gamma), lam = (T)a.lambda;
    T* x = static_cast<T*>(a.x[blockIdx.y]);
    T* r = static_cast<T*>(a.r) + c * a.stride;
    const T* p = static_cast<const T*>(a.p) + c * a.stride;
    const T* q = static_cast<const T*>(a.q) + c * a.stride;
    const int64_t nreal = 2 * a.n;
    double srr = 0.0;
    auto one = [&](T& xv, T& rv, T pv, T qv) {
        xv += al * pv;
        rv -= al * (qv + lam * pv);
        srr += (double)rv * (double)rv;
    };
    NUFFT_FOR_EACH_PACK(T, nreal, i) {
        const int64_t j = i + step__;
        const bool two = j < npacks__;
        Pack<T> x0 = load(x, i), r0 = load(r, i), p0 = load(p, i), q0 = load(q, i), x1{}, r1{}, p1{}, q1{};
        if (two) { x1 = load(x, j); r1 = load(r, j); p1 = load(p, j); q1 = load(q, j); }
#pragma unroll
        for (int w = 0; w < W; ++w) one(x0.v[w], r0.v[w], p0.v[w], q0.v[w]);
        store(x, i, x0);
        store(r, i, r0);
        if (two) {
#pragma unroll
            for (int w = 0; w < W; ++w) one(x1.v[w], r1.v[w], p1.v[w], q1.v[w]);
            store(x, j, x1);
            store(r, j, r1);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t e = npacks__ * W; e < nreal; ++e) one(x[e], r[e], p[e], q[e]);
    srr = block_reduce<Sum>(srr, lds);
    if (threadIdx.x == 0) a.s.part2[(int64_t)c * a.G + blockIdx.x] = srr;
}

// Kernel 3': ρ' = ‖r‖² from the update's partials (the stopping test and the history, as in cg_direction_kernel), ρ_z' = Re<r, z> from the
// dot kernel's partials on (r, z);  p = z + (ρ_z'/ρ_z) p;  the first workgroup writes the scalars of the next iteration.  it = 0 is the
// start of a solve: p = z, ρ and the done flag are those cg_start_kernel left in both slots.  A ρ_z' that is not positive and finite while
// the component is not done is a breakdown (M⁻¹ is positive definite: it means r or m is not finite): p stays, the component freezes.
template <typename T>
__global__ __launch_bounds__(kThreads) void pcg_direction_kernel(CgLaunch a) {
    __shared__ double lds[kWaves];
    constexpr int W = Pack<T>::W;
    const int c = a.c0 + blockIdx.y;
    const int sc = a.joint ? 0 : c, GR = a.joint ? a.C * a.G : a.G;
    const int slot = (a.it & 1) * a.C + sc, next = ((a.it + 1) & 1) * a.C + c;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    const bool start = a.it == 0;
    const bool frozen = a.s.flag[slot] != 0, bad = !frozen && !start && a.s.brk[sc] != 0;
    if (frozen || bad) {
        if (first) {
            a.s.flag[next] = 1;
            a.s.rho[next] = a.s.rho[slot];
            a.s.rhoz[next] = start ? 0.0 : a.s.rhoz[slot];
            if (bad) a.s.status[c] = NUFFT_CG_BREAKDOWN;
        }
        return;
    }
    const double rr = start ? a.s.rho[slot] : row_reduce<Sum>(a.s.part2 + (int64_t)sc * a.G, GR, 1, lds);
    const double rz = row_reduce<Sum>(a.s.part1 + (int64_t)sc * a.G * 2, GR, 2, lds);
    const double bb = a.s.beta0[sc];
    const int done = rr <= a.rtol * a.rtol * bb ? 1 : 0;      // (start: not done, or the component would be frozen)
    const bool broke = !done && (!(rz > 0.0) || !isfinite(rz));
    if (first) {
        a.s.rho[next] = rr;
        a.s.rhoz[next] = rz;
        a.s.flag[next] = done || broke ? 1 : 0;
        if (!start) {
            a.s.res[c] = relative(rr, bb);
            a.s.history[(int64_t)a.it * a.C + c] = relative(rr, bb);
            a.s.iters[c] = a.it;
        }
        a.s.status[c] = broke ? NUFFT_CG_BREAKDOWN : (done ? NUFFT_CG_CONVERGED : NUFFT_CG_MAX_ITER);
    }
    if (broke) return;
    const T bt = start ? T(0) : (T)(rz / a.s.rhoz[slot]);      // ρ_z > 0: checked when it was written
    const T* z = static_cast<const T*>(a.z) + c * a.stride;
    T* p = static_cast<T*>(a.p) + c * a.stride;
    const int64_t nreal = 2 * a.n;
    NUFFT_FOR_EACH_PACK(T, nreal, i) {
        const int64_t j = i + step__;
        const bool two = j < npacks__;
        Pack<T> z0 = load(z, i), p0 = load(p, i), z1{}, p1{};
        if (two) { z1 = load(z, j); p1 = load(p, j); }
#pragma unroll
        for (int w = 0; w < W; ++w) p0.v[w] = start ? z0.v[w] : z0.v[w] + bt * p0.v[w];
        store(p, i, p0);
        if (two) {
#pragma unroll
            for (int w = 0; w < W; ++w) p1.v[w] = start ? z1.v[w] : z1.v[w] + bt * p1.v[w];
            store(p, j, p1);
        }
    }
    if (first)
        for (int64_t e = npacks__ * W; e < nreal; ++e) p[e] = start ? z[e] : z[e] + bt * p[e];
}

}  // namespace

int cg_workgroups(int dtype, int64_t n, int num_cus) { return stream_workgroups((2 * n) / (dtype == NUFFT_F32 ? 4 : 2), num_cus); }

hipError_t launch_cg_residual(const CgLaunch& a, bool warm, hipStream_t stream) {
    const dim3 gr(a.G, a.nc), bl(kThreads);
    if (warm) return launch_by_dtype(a.dtype, gr, bl, stream, cg_residual_kernel<float, true>, cg_residual_kernel<double, true>, a);
    return launch_by_dtype(a.dtype, gr, bl, stream, cg_residual_kernel<float, false>, cg_residual_kernel<double, false>, a);
}

hipError_t launch_cg_start(const CgLaunch& a, hipStream_t stream) {
    hipLaunchKernelGGL(cg_start_kernel, dim3(1, a.nc), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_cg_dot(const CgLaunch& a, hipStream_t stream) {
    return launch_by_dtype(a.dtype, dim3(a.G, a.nc), dim3(kThreads), stream, cg_dot_kernel<float>, cg_dot_kernel<double>, a);
}

hipError_t launch_cg_update(const CgLaunch& a, hipStream_t stream) {
    return launch_by_dtype(a.dtype, dim3(a.G, a.nc), dim3(kThreads), stream, cg_update_kernel<float>, cg_update_kernel<double>, a);
}

hipError_t launch_cg_direction(const CgLaunch& a, hipStream_t stream) {
    return launch_by_dtype(a.dtype, dim3(a.G, a.nc), dim3(kThreads), stream, cg_direction_kernel<float>, cg_direction_kernel<double>, a);
}

hipError_t launch_pcg_update(const CgLaunch& a, hipStream_t stream) {
    return launch_by_dtype(a.dtype, dim3(a.G, a.nc), dim3(kThreads), stream, pcg_update_kernel<float>, pcg_update_kernel<double>, a);
}

hipError_t launch_pcg_direction(const CgLaunch& a, hipStream_t stream) {
    return launch_by_dtype(a.dtype, dim3(a.G, a.nc), dim3(kThreads), stream, pcg_direction_kernel<float>, pcg_direction_kernel<double>, a);
}

}  // namespace nufft
