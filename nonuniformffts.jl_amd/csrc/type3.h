// Launchers of the type-3 streaming kernels (type3_kernels.hip), used by the type-3 plan (type3.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "device_common.h"

namespace nufft {

// Sources: y = x - C; rescaled coordinate y / γ folded into [0, 2π) (plan precision), prephase exp(sign i D·y), count of |y_d| > X_d.
struct T3SourceArgs {
    int dtype, D;
    int64_t n;
    const void* x[3];          // caller's coordinates, T[n]
    void* xr[3];               // rescaled coordinates, T[n] (plan-owned, 16-byte aligned)
    void* phase;               // complex<T>[n]
    unsigned long long* outside;
    double center[3], halfwidth[3], inv_gamma[3], target_center[3];
    double sign;
};

// Targets: t = s - D; θ = sign π t / (σ S) folded into [0, 2π); post factor exp(sign i s·C) Π_d h_d / (ϕ̂_d(γ_d t_d) 2^k_d).
struct T3TargetArgs {
    int dtype, D;
    int64_t n;
    const void* s[3];
    void* theta[3];
    void* post;                // complex<T>[n]
    unsigned long long* outside;
    double center[3], halfwidth[3], theta_scale[3], gamma[3], source_center[3];
    double sign;
    // ϕ̂ of the spreading plan's window on its grid of nf cells (plan_math.cpp: fourier_coefficients_kernel) at real wavenumbers
    int kernel, M;
    double dx[3];              // 2π / nf_d
    double param[3];           // β (Kaiser-Bessel windows), τ (Gaussian), unused (B-spline)
    double h_scaled[3];        // h_d 2^-k_d: the deconvolution's normalisation and the window's power-of-two scale
};

// c'_j = c_j phase_j (premultiply) or f_k *= post_k in place (postmultiply), every component in one launch.
struct T3MultArgs {
    int dtype;
    int64_t n;
    int ncomp;                 // <= kMaxCompPerLaunch
    const void* in[kMaxCompPerLaunch];
    void* out[kMaxCompPerLaunch];
    const void* factor;        // complex<T>[n]
};

// Finish of the type-3 gradient, in place: f[c] holds v_c and grad[c][d] holds ∂v_c/∂θ_d (the inner type-2
// gradient at θ) on entry; on exit f[c] = P v_c and grad[c][d] = ∂f_c/∂s_d = P [sign γ_d h_d ∂v_c/∂θ_d + (sign i C_d − ρ_d) v_c],
// ρ_d = γ_d (d ln ϕ̂_d / dk)(γ_d t_d).  t_d = r / (sign γ_d h_d), r = θ_d if θ_d <= π else θ_d − 2π: the fold is invertible for targets
// inside the box (|sign γ h t| = π |t| / (σ S) <= π / σ <= π); at σ = 1 exactly, |t| = S is ambiguous (t = S reads back as −S).
struct T3GradArgs {
    int dtype, D;
    int64_t n;
    int ncomp;                 // <= kMaxCompPerLaunch
    const void* theta[3];      // T[n]: the type-2 plan's points (set_points3)
    const void* post;          // complex<T>[n]: post factor P (set_points3)
    void* f[kMaxCompPerLaunch];            // complex<T>[n]
    void* grad[kMaxCompPerLaunch][3];      // complex<T>[n]
    double theta_scale[3];     // sign γ_d h_d
    double gamma[3], source_center[3];
    double sign;
    int kernel, M;             // ϕ̂ of the spreading plan's window, as T3TargetArgs
    double dx[3], param[3];
};

hipError_t launch_t3_source_prep(const T3SourceArgs& a, int num_cus, hipStream_t stream);
hipError_t launch_t3_target_prep(const T3TargetArgs& a, int num_cus, hipStream_t stream);
hipError_t launch_t3_multiply(const T3MultArgs& a, int num_cus, hipStream_t stream);
hipError_t launch_t3_grad_finish(const T3GradArgs& a, int num_cus, hipStream_t stream);

}  // namespace nufft
