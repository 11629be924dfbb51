// Launchers of the conjugate-gradient solver's kernels (cg.cpp, cg_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace nufft {

constexpr int kCgBatch = 8;          // components per launch (gridDim.y): the callers' pointers travel as kernel arguments

// Scalars of the solver on the device, all per component (index c < C).  FP64 for both element types.
//   rho, flag are double-buffered by the parity of the iteration that READS them (iteration `it` reads slot it & 1; the first
//   workgroup of its last kernel writes slot (it + 1) & 1), because every workgroup of that kernel still reads the old slot.
struct CgScalars {
    double* rho;        // [2][C]   ‖r‖²
    double* beta0;      // [C]      ‖b‖²
    double* res;        // [C]      sqrt(rho / beta0) after the last iteration that changed the component
    double* rhoz;       // [2][C]   Re<r, z> (preconditioned solves only), double-buffered like rho
    double* history;    // [max_iter + 1][C]
    int32_t* flag;      // [2][C]   done (frozen)
    int32_t* brk;       // [C]      written by the update kernel of this iteration: γ was not positive and finite
    int32_t* iters;     // [C]
    int32_t* status;    // [C]      NUFFT_CG_*
    double* part1;      // [C][G][2]  per-workgroup sums of the dot kernel (Re<p,q>, |p|²) / of the initial residual (|r|², |b|²)
    double* part2;      // [C][G]     per-workgroup sums of |r|² of the update kernel
};

struct CgLaunch {
    int dtype;               // NUFFT_F32 | NUFFT_F64
    int C, c0, nc;           // components in all, first of this launch, number in this launch (<= kCgBatch)
    int G;                   // workgroups per component: the length of the partial-sum rows
    int64_t n;               // complex elements per component
    int64_t stride;          // reals between the components of r, p, q
    void* r;                 // own arrays, component c at + c * stride
    void* p;
    void* q;
    void* z;                 // (preconditioned solves only) z = M⁻¹ r
    void* x[kCgBatch];       // the caller's arrays of components c0 ... c0 + nc − 1
    const void* b[kCgBatch]; // (initial residual only)
    double lambda, rtol;
    int max_iter;
    int it;                  // iteration number, 1-based (parity = it & 1)
    int joint;               // the operator couples its components: they are ONE system — the partial-sum rows
                             // are reduced over all C * G entries from component 0's row (part1 / part2 are contiguous over
                             // components), every component reads the scalars of slot 0 and writes the same values to its own
    CgScalars s;
};

// r = b − (q + λ x) (warm; q = G x) or r = b, x = 0 (cold);  p = r;  partial sums of |r|² and |b|² into part1
hipError_t launch_cg_residual(const CgLaunch& a, bool warm, hipStream_t stream);
// reduces them: rho[1], beta0, res, history[0], flag[1], iters = 0, status; NaN into history[1 ... max_iter]
hipError_t launch_cg_start(const CgLaunch& a, hipStream_t stream);
// the three kernels of an iteration
hipError_t launch_cg_dot(const CgLaunch& a, hipStream_t stream);
hipError_t launch_cg_update(const CgLaunch& a, hipStream_t stream);
hipError_t launch_cg_direction(const CgLaunch& a, hipStream_t stream);

// The preconditioned iteration: the dot kernel, α = ρ_z / γ in the update, the preconditioner's apply, the dot
// kernel again on (r, z) (launch_cg_dot with p = r, q = z: Re<r, z> lands where Re<p, q> did), and the direction kernel
// p = z + (ρ_z'/ρ_z) p, which also takes the stopping decision from the update's ‖r‖².  it = 0: the start (p = z, ρ_z = Re<r, z>).
hipError_t launch_pcg_update(const CgLaunch& a, hipStream_t stream);
hipError_t launch_pcg_direction(const CgLaunch& a, hipStream_t stream);

// workgroups per component for n complex elements of `dtype` on a device with num_cus compute units
int cg_workgroups(int dtype, int64_t n, int num_cus);

}  // namespace nufft
