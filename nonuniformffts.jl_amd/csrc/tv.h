// Launchers of the total-variation kernels (tv.cpp, tv_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace nufft {

constexpr int kTvBatch = 8;       // components per launch (gridDim.z / tiles of dimension 3): the pointers travel as kernel arguments
constexpr int kTvMarch = 8;       // cells a thread marches along the outermost dimension (D >= 2)

// The tile of a workgroup of 256 threads per (element type, D), in cells.  A lane owns one 16-byte pack along dimension 1 (one
// ComplexF64, two ComplexF32; `wide` = 0: a ComplexF32 row of odd N_1 is not 16-byte aligned, the lane then owns one cell).  D = 1: 256
// packs.  D >= 2: a wave owns 64 packs of a row and marches kTvMarch cells along the outermost dimension; the four waves sit side by
// side along dimension 2 (D = 2: on four consecutive strips of kTvMarch rows).
constexpr int tv_tile(bool f32, bool wide, int D, int d) {
    const int V = f32 && wide ? 2 : 1;
    if (d == 0) return (D == 1 ? 256 : 64) * V;
    if (d == 1) return D == 2 ? 4 * kTvMarch : (D == 3 ? 4 : 1);
    return D == 3 ? kTvMarch : 1;
}

// Scalars of the solver on the device, per component, FP64 (the layout of the FISTA solver's).  tv_decide_kernel is the only writer
// after the start, and it is a launch of its own.
struct TvScalars {
    double* change;     // [C]
    int32_t* flag;      // [C]   done (frozen)
    int32_t* iters;     // [C]
    int32_t* status;    // [C]   NUFFT_TVPD_*
    double* history;    // [max_iter][C][2]   change, Σ_i |(∇x⁺)_i|₂
};

enum TvMode { TV_PRIMAL = 0, TV_ADJOINT = 1, TV_DUAL = 2, TV_GRADIENT = 3, TV_NORM = 4 };

struct TvLaunch {
    int dtype, D, wide;
    int C, c0, nc;
    int N[3];
    int tiles[3];
    int64_t G;                    // workgroups per component = tiles[0] · tiles[1] · tiles[2]
    void* x[kTvBatch];            // primal: x (in place);  adjoint: the output;  dual / gradient / norm: x⁺, only read
    void* q[kTvBatch];            // primal: G x in, x̄ out;  dual: x̄, only read
    const void* b[kTvBatch];
    void* y[kTvBatch][3];         // primal / adjoint: only read;  dual: in place;  gradient: the output
    double tv[kTvBatch];
    double step, sigma, lambda;
    double* part;                 // primal: [C][G][2]  ‖x⁺ − x‖², ‖x⁺‖²;  dual / norm: [C][G]  Σ_i |(∇x⁺)_i|₂
    const int32_t* flag;          // may be null
};

hipError_t launch_tv(const TvLaunch& a, TvMode mode, hipStream_t stream);

struct TvSolve {
    int dtype, C, c0, nc, G;      // G: workgroups per component of the start kernel
    int64_t n, ystride;           // complex cells per component; reals between the components' blocks of y (D arrays each)
    void* x[kTvBatch];
    void* y;
    int max_iter, it, joint;
    double tol;
    const double* part_p;         // [C][P][2]
    const double* part_d;         // [C][P]
    int64_t P;
    TvScalars s;
};

// x = 0 unless warm;  y = 0;  scalars reset, NaN into the history
hipError_t launch_tv_start(const TvSolve& a, bool warm, hipStream_t stream);
// the decision of iteration a.it from the partial sums
hipError_t launch_tv_decide(const TvSolve& a, hipStream_t stream);
// out[c] = Σ_g part[c][g]
hipError_t launch_tv_sum(const double* part, int64_t P, int C, double* out, hipStream_t stream);

}  // namespace nufft
