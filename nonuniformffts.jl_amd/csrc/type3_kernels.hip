// Streaming kernels of the type-3 transform (type3.cpp): source preparation, target preparation, the
// complex multiply that prephases the values before the spread and corrects the targets after the type-2 stage, and the finish of
// the type-3 gradient.
//
// All of them are HBM-bound (the target prep and the gradient finish are bound by their FP64 window terms): every thread moves whole 16-byte packs (2 Float64 / 4 Float32 coordinates, 1 ComplexF64 / 2 ComplexF32
// values) with global_load_dwordx4 / global_store_dwordx4; a pack that runs past the end (or an unaligned caller array) takes the
// scalar path.  Grid-stride loops over a grid sized to the device.  Phase arguments and rescaled coordinates are formed in Float64
// from the caller's values (s·C reaches 1e5 rad with ordinary centres, where a Float32 sincos alone is off by 1e-2); the results
// are stored in the plan's precision.
#include <hip/hip_runtime.h>

#include "stream_kernels.h"
#include "type3.h"

namespace nufft {
using namespace stream;
namespace {

constexpr double kTwoPi = 6.283185307179586476925286766559;
constexpr double kPi = 3.1415926535897932384626433832795;

__device__ inline double fold_2pi(double r) { return r - kTwoPi * floor(r * (1.0 / kTwoPi)); }

template <typename T>
__device__ inline T to_plan(double r) {      // folded coordinate in T, kept < 2π after rounding
    T t = (T)r;
    return t >= (T)kTwoPi ? (T)0 : t;
}

// Wave-level sum of the per-thread counts, one atomic per wave (points outside the box are rare).
__device__ inline void count_outside(unsigned long long* dst, uint32_t v) {
    for (int off = warpSize / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & (warpSize - 1)) == 0 && v) atomicAdd(dst, (unsigned long long)v);
}

__device__ double bessel_i0_dev(double x) {   // plan_math.cpp: bessel_i0 (all terms positive)
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

__device__ double bessel_j0_dev(double x) {   // only beyond the window's band (targets outside the declared box): finite, not accurate
    if (x > 25.0) return sqrt(2.0 / (kPi * x)) * cos(x - 0.25 * kPi);
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= -q / ((double)k * (double)k);
        sum += term;
        if (fabs(term) < 1e-17) break;
    }
    return sum;
}

// ϕ̂ of plan_math.cpp: fourier_coefficients_kernel at a real wavenumber k on a grid of spacing dx; past the band of the Kaiser-Bessel
// windows the square root turns imaginary: I0(i a) = J0(a), sinh(i a) / (i a) = sin(a) / a.
__device__ double phihat_dev(int kernel, int M, double dx, double param, double k) {
    if (kernel == NUFFT_KERNEL_BACKWARDS_KAISER_BESSEL || kernel == NUFFT_KERNEL_KAISER_BESSEL) {
        const double w = M * dx, q = w * k;
        const double z = param * param - q * q;
        if (kernel == NUFFT_KERNEL_BACKWARDS_KAISER_BESSEL) return z >= 0.0 ? w * bessel_i0_dev(sqrt(z)) : w * bessel_j0_dev(sqrt(-z));
        if (z > 0.0) { const double s = sqrt(z); return 2.0 * w * sinh(s) / s; }
        if (z < 0.0) { const double s = sqrt(-z); return 2.0 * w * sin(s) / s; }
        return 2.0 * w;
    }
    if (kernel == NUFFT_KERNEL_GAUSSIAN) return exp(-param * k * k * 0.25) * sqrt(kPi * param);
    const double kh = k * dx * 0.5;
    if (kh == 0.0) return dx;
    const double sn = sin(kh) / kh;
    double r = 1.0;
    for (int i = 0; i < 2 * M; ++i) r *= sn;
    return r * dx;
}

// Σ_n 2n/(2n+1)! z^(n−1) over Σ_n z^n/(2n+1)!: (s coth s − 1)/s² at z = s², (1 − u cot u)/u² at z = −u² (both → 1/3 at z → 0).
__device__ __forceinline__ double kb_dlog_series(double z) {
    double num = 0.0, den = 1.0, fac = 1.0, zn = 1.0;     // fac = (2n+1)!, zn = z^(n−1), then z^n
    for (int n = 1; n < 12; ++n) {
        fac *= (2.0 * n) * (2.0 * n + 1.0);
        num += 2.0 * n / fac * zn;
        zn *= z;
        den += zn / fac;
    }
    return num / den;
}

// d ln ϕ̂ / dk of phihat_dev at the same arguments.  Past the Kaiser-Bessel band and past the sinc zeros of
// the B-spline (targets outside the declared box) the value is finite and undefined, as ϕ̂ is there.
__device__ __forceinline__ double dlogphihat_dev(int kernel, int M, double dx, double param, double k) {
    if (kernel == NUFFT_KERNEL_BACKWARDS_KAISER_BESSEL || kernel == NUFFT_KERNEL_KAISER_BESSEL) {
        const double w = M * dx, q = w * k;
        const double z = param * param - q * q;
        double r;                                          // d ln ϕ̂ / dk = −w² k r
        if (kernel == NUFFT_KERNEL_BACKWARDS_KAISER_BESSEL) {
            if (z < -625.0) {                              // u > 25: J0, J1 asymptotics (as bessel_j0_dev)
                const double u = sqrt(-z);
                r = cos(u - 0.75 * kPi) / (u * cos(u - 0.25 * kPi));
            } else {                                       // I1(√z) / (√z I0(√z)) = ½ Σ q^n/(n!(n+1)!) / Σ q^n/(n!)², q = z/4
                const double qq = 0.25 * z;
                double t0 = 1.0, t1 = 0.5, s0 = 1.0, s1 = 0.5;
                for (int n = 1; n < 500; ++n) {
                    t0 *= qq / ((double)n * (double)n);
                    t1 *= qq / ((double)n * (double)(n + 1));
                    s0 += t0;
                    s1 += t1;
                    if (fabs(t0) < 1e-17 * fabs(s0) && fabs(t1) < 1e-17 * fabs(s1)) break;
                }
                r = s1 / s0;
            }
        } else if (fabs(z) < 1.0) {
            r = kb_dlog_series(z);
        } else if (z > 0.0) {
            const double s = sqrt(z);
            r = (s / tanh(s) - 1.0) / z;
        } else {
            const double u = sqrt(-z);
            r = (1.0 - u * cos(u) / sin(u)) / (-z);
        }
        const double out = -w * w * k * r;
        return isfinite(out) ? out : 0.0;
    }
    if (kernel == NUFFT_KERNEL_GAUSSIAN) return -0.5 * param * k;
    const double a = k * dx * 0.5;                         // 2M (dx/2) (cot a − 1/a)
    double g;
    if (fabs(a) < 1e-3) {
        const double a2 = a * a;
        g = -a * (1.0 / 3.0 + a2 * (1.0 / 45.0 + a2 * (2.0 / 945.0)));
    } else {
        g = cos(a) / sin(a) - 1.0 / a;
    }
    const double out = M * dx * g;
    return isfinite(out) ? out : 0.0;
}

template <typename T, int D>
__global__ __launch_bounds__(kThreads) void t3_source_prep_kernel(T3SourceArgs a, int vec) {
    constexpr int W = Pack<T>::W;
    const int64_t nchunks = (a.n + W - 1) / W;
    uint32_t outside = 0;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < nchunks; q += (int64_t)gridDim.x * kThreads) {
        const int64_t i0 = q * W;
        const bool full = i0 + W <= a.n;
        T xv[D][W];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const T* x = static_cast<const T*>(a.x[d]);
            if (full && vec) {
                const Pack<T> pk = *reinterpret_cast<const Pack<T>*>(x + i0);
#pragma unroll
                for (int w = 0; w < W; ++w) xv[d][w] = pk.v[w];
            } else {
#pragma unroll
                for (int w = 0; w < W; ++w) xv[d][w] = i0 + w < a.n ? x[i0 + w] : (T)a.center[d];
            }
        }
        Pack<T> xo[D], ph[2];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            double arg = 0.0;
            bool out = false;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const double y = (double)xv[d][w] - a.center[d];
                out |= fabs(y) > a.halfwidth[d];
                arg += a.target_center[d] * y;
                xo[d].v[w] = to_plan<T>(fold_2pi(y * a.inv_gamma[d]));
            }
            double sn, cs;
            sincos(a.sign * arg, &sn, &cs);
            ph[(2 * w) / W].v[(2 * w) % W] = (T)cs;
            ph[(2 * w + 1) / W].v[(2 * w + 1) % W] = (T)sn;
            outside += (out && i0 + w < a.n) ? 1u : 0u;
        }
        T* phase = static_cast<T*>(a.phase) + 2 * i0;
        if (full) {
#pragma unroll
            for (int d = 0; d < D; ++d) *reinterpret_cast<Pack<T>*>(static_cast<T*>(a.xr[d]) + i0) = xo[d];
            reinterpret_cast<Pack<T>*>(phase)[0] = ph[0];
            reinterpret_cast<Pack<T>*>(phase)[1] = ph[1];
        } else {
            for (int w = 0; w < W && i0 + w < a.n; ++w) {
#pragma unroll
                for (int d = 0; d < D; ++d) static_cast<T*>(a.xr[d])[i0 + w] = xo[d].v[w];
                phase[2 * w] = ph[(2 * w) / W].v[(2 * w) % W];
                phase[2 * w + 1] = ph[(2 * w + 1) / W].v[(2 * w + 1) % W];
            }
        }
    }
    count_outside(a.outside, outside);
}

template <typename T, int D>
__global__ __launch_bounds__(kThreads) void t3_target_prep_kernel(T3TargetArgs a, int vec) {
    constexpr int W = Pack<T>::W;
    const int64_t nchunks = (a.n + W - 1) / W;
    uint32_t outside = 0;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < nchunks; q += (int64_t)gridDim.x * kThreads) {
        const int64_t i0 = q * W;
        const bool full = i0 + W <= a.n;
        T sv[D][W];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const T* s = static_cast<const T*>(a.s[d]);
            if (full && vec) {
                const Pack<T> pk = *reinterpret_cast<const Pack<T>*>(s + i0);
#pragma unroll
                for (int w = 0; w < W; ++w) sv[d][w] = pk.v[w];
            } else {
#pragma unroll
                for (int w = 0; w < W; ++w) sv[d][w] = i0 + w < a.n ? s[i0 + w] : (T)a.center[d];
            }
        }
        Pack<T> th[D], pf[2];
        for (int w = 0; w < W; ++w) {
            double arg = 0.0, fac = 1.0;
            bool out = false;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const double sd = (double)sv[d][w];
                const double t = sd - a.center[d];
                out |= fabs(t) > a.halfwidth[d];
                arg += sd * a.source_center[d];
                th[d].v[w] = to_plan<T>(fold_2pi(a.theta_scale[d] * t));
                fac *= a.h_scaled[d] / phihat_dev(a.kernel, a.M, a.dx[d], a.param[d], a.gamma[d] * t);
            }
            double sn, cs;
            sincos(a.sign * arg, &sn, &cs);
            pf[(2 * w) / W].v[(2 * w) % W] = (T)(fac * cs);
            pf[(2 * w + 1) / W].v[(2 * w + 1) % W] = (T)(fac * sn);
            outside += (out && i0 + w < a.n) ? 1u : 0u;
        }
        T* post = static_cast<T*>(a.post) + 2 * i0;
        if (full) {
#pragma unroll
            for (int d = 0; d < D; ++d) *reinterpret_cast<Pack<T>*>(static_cast<T*>(a.theta[d]) + i0) = th[d];
            reinterpret_cast<Pack<T>*>(post)[0] = pf[0];
            reinterpret_cast<Pack<T>*>(post)[1] = pf[1];
        } else {
            for (int w = 0; w < W && i0 + w < a.n; ++w) {
#pragma unroll
                for (int d = 0; d < D; ++d) static_cast<T*>(a.theta[d])[i0 + w] = th[d].v[w];
                post[2 * w] = pf[(2 * w) / W].v[(2 * w) % W];
                post[2 * w + 1] = pf[(2 * w + 1) / W].v[(2 * w + 1) % W];
            }
        }
    }
    count_outside(a.outside, outside);
}

// out[c][i] = in[c][i] * factor[i] (complex), component c = blockIdx.y; in == out is allowed (postmultiply in place).
template <typename T>
__global__ __launch_bounds__(kThreads) void t3_multiply_kernel(T3MultArgs a, int vec) {
    constexpr int W = Pack<T>::W / 2;      // complex values per pack
    const int c = blockIdx.y;
    const T* in = static_cast<const T*>(a.in[c]);
    T* out = static_cast<T*>(a.out[c]);
    const T* f = static_cast<const T*>(a.factor);
    const int64_t nchunks = (a.n + W - 1) / W;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < nchunks; q += (int64_t)gridDim.x * kThreads) {
        const int64_t i0 = q * W;
        if (i0 + W <= a.n && vec) {
            const Pack<T> u = *reinterpret_cast<const Pack<T>*>(in + 2 * i0);
            const Pack<T> g = *reinterpret_cast<const Pack<T>*>(f + 2 * i0);
            Pack<T> r;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                r.v[2 * w] = u.v[2 * w] * g.v[2 * w] - u.v[2 * w + 1] * g.v[2 * w + 1];
                r.v[2 * w + 1] = u.v[2 * w] * g.v[2 * w + 1] + u.v[2 * w + 1] * g.v[2 * w];
            }
            *reinterpret_cast<Pack<T>*>(out + 2 * i0) = r;
        } else {
            for (int64_t i = i0; i < i0 + W && i < a.n; ++i) {
                const T ur = in[2 * i], ui = in[2 * i + 1], gr = f[2 * i], gi = f[2 * i + 1];
                out[2 * i] = ur * gr - ui * gi;
                out[2 * i + 1] = ur * gi + ui * gr;
            }
        }
    }
}

// Finish of the type-3 gradient, in place on the outputs of the inner type-2 gradient (component c = blockIdx.y): v_c -> f_c = P v_c,
// ∂_θd v_c -> ∂f_c/∂s_d = P [sign γ_d h_d ∂_θd v_c + (sign i C_d − ρ_d(t_d)) v_c] with ρ_d = γ_d (d ln ϕ̂_d / dk)(γ_d t_d).  t_d comes
// back from the stored θ (r = θ or θ − 2π, t = r / (sign γ_d h_d)): no per-target table beyond the ones set_points3 wrote.
template <typename T, int D, int K>     // K: the window (a.kernel), a template parameter so that one branch of dlogphihat_dev is inlined
__global__ __launch_bounds__(kThreads) void t3_grad_finish_kernel(T3GradArgs a, int vec_theta, int vec_io) {
    constexpr int W = Pack<T>::W;          // targets per thread: one pack of θ per dimension, two packs of each complex vector
    const int c = blockIdx.y;
    T* fv = static_cast<T*>(a.f[c]);
    T* gv[D];
#pragma unroll
    for (int d = 0; d < D; ++d) gv[d] = static_cast<T*>(a.grad[c][d]);
    const T* post = static_cast<const T*>(a.post);
    const int64_t nchunks = (a.n + W - 1) / W;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < nchunks; q += (int64_t)gridDim.x * kThreads) {
        const int64_t i0 = q * W;
        const bool full = i0 + W <= a.n;
        T th[D][W];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const T* x = static_cast<const T*>(a.theta[d]);
            if (full && vec_theta) {
                const Pack<T> pk = *reinterpret_cast<const Pack<T>*>(x + i0);
#pragma unroll
                for (int w = 0; w < W; ++w) th[d][w] = pk.v[w];
            } else {
#pragma unroll
                for (int w = 0; w < W; ++w) th[d][w] = i0 + w < a.n ? x[i0 + w] : (T)0;
            }
        }
        Pack<T> pf[2], vv[2], gg[D][2];
        if (full && vec_io) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                pf[h] = reinterpret_cast<const Pack<T>*>(post + 2 * i0)[h];
                vv[h] = reinterpret_cast<const Pack<T>*>(fv + 2 * i0)[h];
#pragma unroll
                for (int d = 0; d < D; ++d) gg[d][h] = reinterpret_cast<const Pack<T>*>(gv[d] + 2 * i0)[h];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 2 * W; ++e) {
                const bool in = i0 + e / 2 < a.n;
                pf[e / W].v[e % W] = in ? post[2 * i0 + e] : (T)0;
                vv[e / W].v[e % W] = in ? fv[2 * i0 + e] : (T)0;
#pragma unroll
                for (int d = 0; d < D; ++d) gg[d][e / W].v[e % W] = in ? gv[d][2 * i0 + e] : (T)0;
            }
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const int h = (2 * w) / W, e = (2 * w) % W;
            const double pr = (double)pf[h].v[e], pi = (double)pf[h].v[e + 1];
            const double vr = (double)vv[h].v[e], vi = (double)vv[h].v[e + 1];
            vv[h].v[e] = (T)(pr * vr - pi * vi);
            vv[h].v[e + 1] = (T)(pr * vi + pi * vr);
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const double theta = (double)th[d][w];
                const double t = (theta <= kPi ? theta : theta - kTwoPi) / a.theta_scale[d];
                const double rho = a.gamma[d] * dlogphihat_dev(K, a.M, a.dx[d], a.param[d], a.gamma[d] * t);
                const double sc = a.sign * a.source_center[d];
                const double xr = a.theta_scale[d] * (double)gg[d][h].v[e] - rho * vr - sc * vi;
                const double xi = a.theta_scale[d] * (double)gg[d][h].v[e + 1] - rho * vi + sc * vr;
                gg[d][h].v[e] = (T)(pr * xr - pi * xi);
                gg[d][h].v[e + 1] = (T)(pr * xi + pi * xr);
            }
        }
        if (full && vec_io) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                reinterpret_cast<Pack<T>*>(fv + 2 * i0)[h] = vv[h];
#pragma unroll
                for (int d = 0; d < D; ++d) reinterpret_cast<Pack<T>*>(gv[d] + 2 * i0)[h] = gg[d][h];
            }
        } else {
            for (int e = 0; e < 2 * W && i0 + e / 2 < a.n; ++e) {
                fv[2 * i0 + e] = vv[e / W].v[e % W];
#pragma unroll
                for (int d = 0; d < D; ++d) gv[d][2 * i0 + e] = gg[d][e / W].v[e % W];
            }
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

hipError_t launch_t3_source_prep(const T3SourceArgs& a, int num_cus, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    int vec = 1;
    for (int d = 0; d < a.D; ++d) vec &= aligned16(a.x[d]);
    const int W = a.dtype == NUFFT_F32 ? 4 : 2;
    const dim3 grid(grid_for((a.n + W - 1) / W, num_cus)), block(kThreads);
    switch (a.D) {
        case 1: return launch_by_dtype(a.dtype, grid, block, stream, t3_source_prep_kernel<float, 1>, t3_source_prep_kernel<double, 1>, a, vec);
        case 2: return launch_by_dtype(a.dtype, grid, block, stream, t3_source_prep_kernel<float, 2>, t3_source_prep_kernel<double, 2>, a, vec);
        default: return launch_by_dtype(a.dtype, grid, block, stream, t3_source_prep_kernel<float, 3>, t3_source_prep_kernel<double, 3>, a, vec);
    }
}

hipError_t launch_t3_target_prep(const T3TargetArgs& a, int num_cus, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    int vec = 1;
    for (int d = 0; d < a.D; ++d) vec &= aligned16(a.s[d]);
    const int W = a.dtype == NUFFT_F32 ? 4 : 2;
    const dim3 grid(grid_for((a.n + W - 1) / W, num_cus)), block(kThreads);
    switch (a.D) {
        case 1: return launch_by_dtype(a.dtype, grid, block, stream, t3_target_prep_kernel<float, 1>, t3_target_prep_kernel<double, 1>, a, vec);
        case 2: return launch_by_dtype(a.dtype, grid, block, stream, t3_target_prep_kernel<float, 2>, t3_target_prep_kernel<double, 2>, a, vec);
        default: return launch_by_dtype(a.dtype, grid, block, stream, t3_target_prep_kernel<float, 3>, t3_target_prep_kernel<double, 3>, a, vec);
    }
}

hipError_t launch_t3_multiply(const T3MultArgs& a, int num_cus, hipStream_t stream) {
    if (a.n <= 0 || a.ncomp <= 0) return hipSuccess;
    int vec = aligned16(a.factor);
    for (int c = 0; c < a.ncomp; ++c) vec &= (aligned16(a.in[c]) && aligned16(a.out[c])) ? 1 : 0;
    const int W = a.dtype == NUFFT_F32 ? 2 : 1;
    const dim3 grid(grid_for((a.n + W - 1) / W, std::max(1, num_cus / a.ncomp)), a.ncomp), block(kThreads);
    return launch_by_dtype(a.dtype, grid, block, stream, t3_multiply_kernel<float>, t3_multiply_kernel<double>, a, vec);
}

namespace {

template <int D>
hipError_t launch_grad_finish_d(const T3GradArgs& a, dim3 grid, hipStream_t stream, int vec_theta, int vec_io) {
    const dim3 block(kThreads);
    switch (a.kernel) {
        case NUFFT_KERNEL_BACKWARDS_KAISER_BESSEL:
            return launch_by_dtype(a.dtype, grid, block, stream, t3_grad_finish_kernel<float, D, NUFFT_KERNEL_BACKWARDS_KAISER_BESSEL>,
                                   t3_grad_finish_kernel<double, D, NUFFT_KERNEL_BACKWARDS_KAISER_BESSEL>, a, vec_theta, vec_io);
        case NUFFT_KERNEL_KAISER_BESSEL:
            return launch_by_dtype(a.dtype, grid, block, stream, t3_grad_finish_kernel<float, D, NUFFT_KERNEL_KAISER_BESSEL>,
                                   t3_grad_finish_kernel<double, D, NUFFT_KERNEL_KAISER_BESSEL>, a, vec_theta, vec_io);
        case NUFFT_KERNEL_GAUSSIAN:
            return launch_by_dtype(a.dtype, grid, block, stream, t3_grad_finish_kernel<float, D, NUFFT_KERNEL_GAUSSIAN>,
                                   t3_grad_finish_kernel<double, D, NUFFT_KERNEL_GAUSSIAN>, a, vec_theta, vec_io);
        default:
            return launch_by_dtype(a.dtype, grid, block, stream, t3_grad_finish_kernel<float, D, NUFFT_KERNEL_BSPLINE>,
                                   t3_grad_finish_kernel<double, D, NUFFT_KERNEL_BSPLINE>, a, vec_theta, vec_io);
    }
}

}  // namespace

hipError_t launch_t3_grad_finish(const T3GradArgs& a, int num_cus, hipStream_t stream) {
    if (a.n <= 0 || a.ncomp <= 0) return hipSuccess;
    int vec_theta = 1, vec_io = aligned16(a.post);
    for (int d = 0; d < a.D; ++d) vec_theta &= aligned16(a.theta[d]);
    for (int c = 0; c < a.ncomp; ++c) {
        vec_io &= aligned16(a.f[c]) ? 1 : 0;
        for (int d = 0; d < a.D; ++d) vec_io &= aligned16(a.grad[c][d]) ? 1 : 0;
    }
    const int W = a.dtype == NUFFT_F32 ? 4 : 2;
    const dim3 grid(grid_for((a.n + W - 1) / W, std::max(1, num_cus / a.ncomp)), a.ncomp);
    switch (a.D) {
        case 1: return launch_grad_finish_d<1>(a, grid, stream, vec_theta, vec_io);
        case 2: return launch_grad_finish_d<2>(a, grid, stream, vec_theta, vec_io);
        default: return launch_grad_finish_d<3>(a, grid, stream, vec_theta, vec_io);
    }
}

}  // namespace nufft
