// Instantiation + launcher of the gradient gather (interp_grad_kernels.h) for one (real type, complex?) pair.
// Included by interp_grad_*.hip after defining NUFFT_T, NUFFT_CPLX and NUFFT_GRAD_LAUNCHER (name of the exported launcher).
#include "interp_grad_kernels.h"
#include "kernels.h"

namespace nufft {

using GradKernelPtr = void (*)(GradKArgs<NUFFT_T>);

template <int D, int M, int... W>
static GradKernelPtr grad_pick_w(int wsel, std::integer_sequence<int, W...>) {
    GradKernelPtr k = nullptr;
    ((k = (wsel == W ? interp_grad_kernel<NUFFT_T, NUFFT_CPLX, D, M, W> : k)), ...);
    return k;
}
template <int D, int... MM>
static GradKernelPtr grad_pick_m(int M, int wsel, std::integer_sequence<int, MM...>) {
    GradKernelPtr k = nullptr;
    ((k = (M == MM + 2 ? grad_pick_w<D, MM + 2>(wsel, std::make_integer_sequence<int, 3>{}) : k)), ...);
    return k;
}
static GradKernelPtr grad_kernel(int D, int M, int wsel) {
    constexpr auto ms = std::make_integer_sequence<int, 9>{};      // M = 2..10
    if (D == 1) return grad_pick_m<1>(M, wsel, ms);
    if (D == 2) return grad_pick_m<2>(M, wsel, ms);
    if (D == 3) return grad_pick_m<3>(M, wsel, ms);
    return nullptr;
}

hipError_t NUFFT_GRAD_LAUNCHER(const GradLaunchArgs& a, hipStream_t stream) {
    using T = NUFFT_T;
    const int wsel = grad_window_select(a.kernel, a.evalmode);
    GradKernelPtr k = grad_kernel(a.D, a.M, wsel);
    if (!k) return hipErrorInvalidValue;
    GradKArgs<T> ka{};
    ka.sorted = a.sorted;
    ka.np = a.np;
    ka.coefs = static_cast<const T*>(a.coefs);
    ka.kernel = a.kernel;
    ka.evalmode = a.evalmode;
    ka.prefactor = (T)a.prefactor;
    for (int d = 0; d < 3; ++d) {
        ka.Nover[d] = a.Nover[d];
        ka.p0[d] = (T)a.p0[d];
        ka.p1[d] = (T)a.p1[d];
        ka.dscale[d] = (T)a.dscale[d];
    }
    const int G = next_pow2(2 * a.M);
    const int64_t ppb = kGradThreads / G;
    const int64_t chunks = (a.np + ppb - 1) / ppb;
    const int64_t blocks = (chunks + kGradChunks - 1) / kGradChunks;     // < 2^29 for np < 2^31
    const size_t elem = sizeof(T) * (NUFFT_CPLX ? 2 : 1);
    for (int c0 = 0; c0 < a.C; c0 += kMaxCompPerLaunch) {
        ka.nc = std::min(kMaxCompPerLaunch, a.C - c0);
        for (int c = 0; c < ka.nc; ++c) {
            ka.grid[c] = reinterpret_cast<const T*>(static_cast<const char*>(a.grid) + (size_t)(c0 + c) * a.grid_stride * elem);
            ka.vout[c] = a.values_out ? static_cast<T*>(a.values_out[c0 + c]) : nullptr;
            for (int d = 0; d < a.D; ++d) ka.gout[c][d] = static_cast<T*>(a.grad_out[(size_t)(c0 + c) * a.D + d]);
        }
        hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(kGradThreads), 0, stream, ka);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace nufft
