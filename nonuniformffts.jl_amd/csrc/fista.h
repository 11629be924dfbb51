// Launchers of the FISTA solver's streaming kernels and of the power iteration (fista.cpp, toeplitz.cpp, fista_kernels.hip; DESIGN.md
// section 23).  The wavelet kernels of an iteration are wavelet.h's.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "solver_decide.h"

namespace nufft {

constexpr int kFistaBatch = 8;       // components per launch (gridDim.y): the callers' pointers travel as kernel arguments

struct FistaLaunch {
    int dtype;
    int C, c0, nc;
    int G;                   // workgroups per component of the streaming kernels
    int64_t n;               // complex elements per component
    int64_t stride;          // reals between the components of z, q
    void* z;
    void* q;
    void* x[kFistaBatch];
    const void* b[kFistaBatch];
    double step, lambda, tol;
    int max_iter, it;
    int joint;               // coupled components are ONE system: the sums run over all components' rows (contiguous), and every
                             // component computes — and stores in its own slots — the same change, flag and status
    const double* mom_part;  // [C][G0][2]  ‖x⁺ − x‖², ‖x⁺‖² per workgroup of the level-0 synthesis
    int G0;
    const double* l1_part;   // [C][P]      Σ|stored detail| per workgroup of the analysis levels
    int P;
    ProxScalars s;           // one slot per component; history [max_iter][C][2]: change, ‖D W x‖₁
};

// z = x (warm) or x = z = 0;  scalars reset, NaN into the history
hipError_t launch_fista_start(const FistaLaunch& a, bool warm, hipStream_t stream);
// q <- z − τ (q + μ z − b), in place over q
hipError_t launch_fista_gradient(const FistaLaunch& a, hipStream_t stream);
// the decision of iteration a.it from the partial sums
hipError_t launch_fista_decide(const FistaLaunch& a, hipStream_t stream);
// the same for a solver with the locally low-rank prior (one system): part[G][3] of llr.h's kernel, the outcome stored for all a.C components
hipError_t launch_fista_decide_llr(const FistaLaunch& a, const double* part, int64_t G, hipStream_t stream);
int fista_workgroups(int dtype, int64_t n, int num_cus);

// Power iteration (nufft_toeplitz_max_eigenvalue): v, g are the solver's own arrays (component c at + c * stride reals).
struct PowerLaunch {
    int dtype, C, G, joint;
    int64_t n, stride;
    void* v;
    void* g;
    double* part;            // [C][G][3]   Re<v, g>, <v, v>, <g, g>
    double* rho;             // [C]
};
hipError_t launch_power_dot(const PowerLaunch& a, hipStream_t stream);
// rho = Re<v, g> / <v, v>;  v = g / ‖g‖
hipError_t launch_power_scale(const PowerLaunch& a, hipStream_t stream);

}  // namespace nufft
