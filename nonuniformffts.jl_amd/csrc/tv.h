// Launchers of the total-variation kernels (tv.cpp, tv_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "solver_decide.h"

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
    ProxScalars s;                // one slot per component; history [max_iter][C][2]: change, Σ_i |(∇x⁺)_i|₂
};

// x = 0 unless warm;  y = 0;  scalars reset, NaN into the history
hipError_t launch_tv_start(const TvSolve& a, bool warm, hipStream_t stream);
// the decision of iteration a.it from the partial sums
hipError_t launch_tv_decide(const TvSolve& a, hipStream_t stream);
// out[c] = Σ_g part[c][g]
hipError_t launch_tv_sum(const double* part, int64_t P, int C, double* out, hipStream_t stream);

// ---- the difference along the components ("frames"; tvt_kernels.hip) ----
//
// A cell's neighbour in time is the same index of ANOTHER array, so the kernels are flat over the n cells of a frame: a lane owns
// kTvtPacks 16-byte packs (one ComplexF64, two ComplexF32; one ComplexF32 where n is odd), 256 lanes apart.  The pointers travel as
// kernel arguments widened by one frame on each side of the batch: slot j of a table is frame c0 + j − 1, so slot 0 and slot nc + 1
// belong to the neighbouring batch or, on a periodic axis, to the other end.  A null slot is a frame that is zero by definition (z_{−1}
// and z_{K−1} of the adjoint) or absent (the neighbour of the last frame: its difference is zero) on the non-periodic axis.
constexpr int kTvtPacks = 4;

enum TvtMode { TVT_PRIMAL = 0, TVT_ADJOINT = 1, TVT_ADD = 2, TVT_DUAL = 3, TVT_GRADIENT = 4, TVT_NORM = 5 };

struct TvtLaunch {
    int dtype, wide;
    int C, c0, nc;
    int64_t n;                    // complex cells per frame
    int64_t G;                    // workgroups per frame = ceil(packs / (256 · kTvtPacks))
    void* x[kTvBatch + 2];        // primal: x (in place);  adjoint: the output;  dual / gradient / norm: x⁺, only read, also at c + 1
    void* q[kTvBatch + 2];        // primal: G x in, x̄ out;  add: in place;  dual: x̄, only read, also at c + 1
    const void* b[kTvBatch];      // (slot k is frame c0 + k: no neighbour is read)
    void* z[kTvBatch + 2];        // primal / adjoint / add: only read, also at c − 1;  dual: in place;  gradient: the output
    double tv_t, step, sigma, lambda;
    double* part;                 // primal: [C][G][2]  ‖x⁺ − x‖², ‖x⁺‖²;  dual / norm: [C][G]  Σ_i |(∇_t x⁺)_c[i]|
    const int32_t* flag;          // may be null
};

hipError_t launch_tvt(const TvtLaunch& a, TvtMode mode, hipStream_t stream);

// The decision of iteration `it` of a solver with the temporal term: always joint (the frames are one system).  One workgroup per
// component; each forms the same change from all rows, and its own share of the prior, tv_c Σ_i |(∇x⁺_c)_i|₂ + tv_t Σ_i |(∇_t x⁺)_c[i]|.
struct TvtDecide {
    int C, c0, nc, it;
    double tol, tv_t;
    double tv[kTvBatch];          // the spatial weights of the batch
    const double* part_p;         // [C][Pp][2]
    const double* part_s;         // [C][Ps], null when the spatial term is off
    const double* part_t;         // [C][Pt]
    int64_t Pp, Ps, Pt;
    ProxScalars s;
};
hipError_t launch_tvt_decide(const TvtDecide& a, hipStream_t stream);

}  // namespace nufft
