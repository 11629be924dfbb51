// Kernels of the sample-density compensation iteration (dcf.cpp).
//
// The iteration is w <- w / (C w), C = interpolation after spreading (the plan's own kernels, enqueued by dcf.cpp).  What is left for
// this file are passes over vectors of n reals, with the packs, the loop shape and the fixed-order reduction of the per-workgroup
// partials of stream_kernels.h (here of maxima too: NaN values are caught by the breakdown test, not by δ).
//
// The stopping rule needs δ_k = max |v − 1| of ALL of v before iteration k may divide anything by v, and the breakdown test likewise:
// that is one kernel boundary inside the iteration, so an iteration has two kernels (check: reads v; update: reads v and w, writes w).
// Once the done flag is set the state is frozen: the workgroups leave after reading the flag.  The first workgroup of the update kernel
// writes the flag of the next iteration into the other parity slot (every workgroup of that kernel still reads the current slot).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "dcf.h"
#include "nufft_mi355x.h"
#include "stream_kernels.h"

namespace nufft {
using namespace stream;
namespace {

template <typename T>
__device__ __forceinline__ bool positive_finite(T x) {
    return x > T(0) && x < (T)INFINITY;      // false for NaN
}

// w = 1 (the state u = w / 2^κ of the all-ones start), or the test of the caller's w0, which is only read
template <typename T, bool W0>
__global__ __launch_bounds__(kThreads) void dcf_start_kernel(DcfLaunch a) {
    __shared__ double lds[kWaves];
    constexpr int W = Pack<T>::W;
    T* w = static_cast<T*>(a.w);
    double bad = 0.0;
    Pack<T> ones;
#pragma unroll
    for (int e = 0; e < W; ++e) ones.v[e] = T(1);
    NUFFT_FOR_EACH_PACK(T, a.n, i) {
        const int64_t j = i + step__;
        const bool two = j < npacks__;
        if (W0) {
            Pack<T> w0 = load(w, i), w1 = ones;
            if (two) w1 = load(w, j);
#pragma unroll
            for (int e = 0; e < W; ++e) bad = (positive_finite(w0.v[e]) && positive_finite(w1.v[e])) ? bad : 1.0;
        } else {
            store(w, i, ones);
            if (two) store(w, j, ones);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t e = npacks__ * W; e < a.n; ++e) {
            if (W0) bad = positive_finite(w[e]) ? bad : 1.0;
            else w[e] = T(1);
        }
    bad = block_reduce<Max>(bad, lds);
    if (threadIdx.x == 0) {
        a.s.part[2 * blockIdx.x] = 0.0;
        a.s.part[2 * blockIdx.x + 1] = bad;
    }
}

// One workgroup: the scalars before the first iteration, and NaN into the history.
__global__ __launch_bounds__(kThreads) void dcf_begin_kernel(DcfLaunch a) {
    __shared__ double lds[kWaves];
    const double bad = row_reduce<Max>(a.s.part + 1, a.G, 2, lds);
    for (int k = threadIdx.x; k < a.max_iter; k += kThreads) a.s.history[k] = NAN;
    if (threadIdx.x == 0) {
        const int done = bad != 0.0 ? 1 : 0;
        a.s.flag[0] = done;
        a.s.flag[1] = done;
        a.s.iters[0] = 0;
        a.s.status[0] = done ? NUFFT_DCF_BREAKDOWN : NUFFT_DCF_MAX_ITER;
        a.s.res[0] = NAN;
        a.s.sum[0] = 0.0;
    }
}

// Kernel 1 of an iteration: partials of δ_k = max |v − 1| and of the breakdown test
template <typename T>
__global__ __launch_bounds__(kThreads) void dcf_check_kernel(DcfLaunch a) {
    __shared__ double lds[kWaves];
    constexpr int W = Pack<T>::W;
    if (a.s.flag[a.k & 1]) return;
    const T* v = static_cast<const T*>(a.v);
    const double sc = a.vscale;
    double dmax = 0.0, bad = 0.0;
    auto one = [&](T x) {
        dmax = fmax(dmax, fabs((double)x * sc - 1.0));
        bad = positive_finite(x) ? bad : 1.0;
    };
    NUFFT_FOR_EACH_PACK(T, a.n, i) {
        const int64_t j = i + step__;
        Pack<T> v0 = load(v, i), v1;
#pragma unroll
        for (int e = 0; e < W; ++e) v1.v[e] = v0.v[e];      // no second pack: the first one again changes neither maximum
        if (j < npacks__) v1 = load(v, j);
#pragma unroll
        for (int e = 0; e < W; ++e) { one(v0.v[e]); one(v1.v[e]); }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t e = npacks__ * W; e < a.n; ++e) one(v[e]);
    dmax = block_reduce<Max>(dmax, lds);
    bad = block_reduce<Max>(bad, lds);
    if (threadIdx.x == 0) {
        a.s.part[2 * blockIdx.x] = dmax;
        a.s.part[2 * blockIdx.x + 1] = bad;
    }
}

// Kernel 2: δ_k and the breakdown test from kernel 1's partials, the same bits in every workgroup: they all divide, or none does;
// w /= v;  the first workgroup keeps the scalars
template <typename T>
__global__ __launch_bounds__(kThreads) void dcf_update_kernel(DcfLaunch a) {
    __shared__ double lds[kWaves];
    constexpr int W = Pack<T>::W;
    const int slot = a.k & 1, next = slot ^ 1;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (a.s.flag[slot]) {
        if (first) a.s.flag[next] = 1;
        return;
    }
    const double delta = row_reduce<Max>(a.s.part, a.G, 2, lds);
    const bool bad = row_reduce<Max>(a.s.part + 1, a.G, 2, lds) != 0.0;
    const bool conv = !bad && a.k >= 1 && delta <= a.tol;
    if (first) {
        if (a.report && !bad) {
            a.s.history[a.k] = delta;
            a.s.res[0] = delta;
        }
        a.s.flag[next] = (bad || conv) ? 1 : 0;
        a.s.status[0] = bad ? NUFFT_DCF_BREAKDOWN : (conv ? NUFFT_DCF_CONVERGED : NUFFT_DCF_MAX_ITER);
        if (!bad && !conv) a.s.iters[0] = a.k + 1;
    }
    if (bad || conv) return;
    T* w = static_cast<T*>(a.w);
    const T* v = static_cast<const T*>(a.v);
    NUFFT_FOR_EACH_PACK(T, a.n, i) {
        const int64_t j = i + step__;
        const bool two = j < npacks__;
        Pack<T> w0 = load(w, i), v0 = load(v, i), w1{}, v1{};
        if (two) { w1 = load(w, j); v1 = load(v, j); }
#pragma unroll
        for (int e = 0; e < W; ++e) w0.v[e] = w0.v[e] / v0.v[e];
        store(w, i, w0);
        if (two) {
#pragma unroll
            for (int e = 0; e < W; ++e) w1.v[e] = w1.v[e] / v1.v[e];
            store(w, j, w1);
        }
    }
    if (first)
        for (int64_t e = npacks__ * W; e < a.n; ++e) w[e] = w[e] / v[e];
}

// Finish, kernel 1: partials of Σ w
template <typename T>
__global__ __launch_bounds__(kThreads) void dcf_sum_kernel(DcfLaunch a) {
    __shared__ double lds[kWaves];
    constexpr int W = Pack<T>::W;
    if (a.s.status[0] == NUFFT_DCF_BREAKDOWN) return;
    const T* w = static_cast<const T*>(a.w);
    double s = 0.0;
    NUFFT_FOR_EACH_PACK(T, a.n, i) {
        const int64_t j = i + step__;
        Pack<T> w0 = load(w, i), w1{};
        if (j < npacks__) w1 = load(w, j);
#pragma unroll
        for (int e = 0; e < W; ++e) s += (double)w0.v[e] + (double)w1.v[e];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t e = npacks__ * W; e < a.n; ++e) s += (double)w[e];
    s = block_reduce<Sum>(s, lds);
    if (threadIdx.x == 0) a.s.part[2 * blockIdx.x] = s;
}

// Finish, kernel 2: w /= Σ w, or w *= 2^κ
template <typename T>
__global__ __launch_bounds__(kThreads) void dcf_scale_kernel(DcfLaunch a) {
    __shared__ double lds[kWaves];
    constexpr int W = Pack<T>::W;
    if (a.s.status[0] == NUFFT_DCF_BREAKDOWN) return;
    const bool norm = a.normalize == NUFFT_DCF_NORMALIZE_SUM;
    double total = 1.0;
    if (norm) {
        total = row_reduce<Sum>(a.s.part, a.G, 2, lds);
        if (blockIdx.x == 0 && threadIdx.x == 0) a.s.sum[0] = total;
    }
    const T den = (T)total, mul = (T)a.gamma;
    T* w = static_cast<T*>(a.w);
    auto one = [&](T x) { return norm ? x / den : x * mul; };
    NUFFT_FOR_EACH_PACK(T, a.n, i) {
        const int64_t j = i + step__;
        const bool two = j < npacks__;
        Pack<T> w0 = load(w, i), w1{};
        if (two) w1 = load(w, j);
#pragma unroll
        for (int e = 0; e < W; ++e) w0.v[e] = one(w0.v[e]);
        store(w, i, w0);
        if (two) {
#pragma unroll
            for (int e = 0; e < W; ++e) w1.v[e] = one(w1.v[e]);
            store(w, j, w1);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t e = npacks__ * W; e < a.n; ++e) w[e] = one(w[e]);
}

template <typename KF, typename KD>
hipError_t launch(const DcfLaunch& a, KF kf, KD kd, hipStream_t stream) {
    return launch_by_dtype(a.dtype, dim3(a.G), dim3(kThreads), stream, kf, kd, a);
}

}  // namespace

int dcf_workgroups(int dtype, int64_t n, int num_cus) { return stream_workgroups(n / (dtype == NUFFT_F32 ? 4 : 2), num_cus, kDcfMaxGroups); }

hipError_t launch_dcf_start(const DcfLaunch& a, bool use_w0, hipStream_t stream) {
    if (use_w0) return launch(a, dcf_start_kernel<float, true>, dcf_start_kernel<double, true>, stream);
    return launch(a, dcf_start_kernel<float, false>, dcf_start_kernel<double, false>, stream);
}

hipError_t launch_dcf_begin(const DcfLaunch& a, hipStream_t stream) {
    hipLaunchKernelGGL(dcf_begin_kernel, dim3(1), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_dcf_check(const DcfLaunch& a, hipStream_t stream) {
    return launch(a, dcf_check_kernel<float>, dcf_check_kernel<double>, stream);
}

hipError_t launch_dcf_update(const DcfLaunch& a, hipStream_t stream) {
    return launch(a, dcf_update_kernel<float>, dcf_update_kernel<double>, stream);
}

hipError_t launch_dcf_sum(const DcfLaunch& a, hipStream_t stream) {
    return launch(a, dcf_sum_kernel<float>, dcf_sum_kernel<double>, stream);
}

hipError_t launch_dcf_scale(const DcfLaunch& a, hipStream_t stream) {
    return launch(a, dcf_scale_kernel<float>, dcf_scale_kernel<double>, stream);
}

}  // namespace nufft
