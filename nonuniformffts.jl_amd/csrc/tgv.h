// Launchers of the second-order total-generalized-variation kernels (tgv.cpp, tv.cpp, tgv_kernels.hip).  The
// tiling, the batches and the partial sums are those of tv.h.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "solver_decide.h"
#include "tv.h"

namespace nufft {

// entries of a symmetric D x D tensor, and the array of entry (d, e), d <= e, in row-major upper-triangle order
constexpr int tgv_sym(int D) { return D * (D + 1) / 2; }
constexpr int tgv_pair(int D, int d, int e) { return d * D - d * (d - 1) / 2 + (e - d); }

// TGV_FIELD:        v⁺ = v − τ (−p + Eᴴr);  v <- v⁺;  v̄ <- v⁺ + (v⁺ − v)            reads r at i and i + e
// TGV_SYM_ADJOINT:  v <- Eᴴr
// TGV_P:            p <- P_α1(p + σ (∇x̄ − v̄));  partial of Σ_i |(∇x⁺ − v⁺)_i|₂     reads x̄ (q), x⁺ (x) at i and i + e_d
// TGV_R:            r <- P_α0(r + σ E v̄);  partial of Σ_i |(E v⁺)_i|_F              reads v̄, v⁺ at i and i − e
// TGV_SYM_GRADIENT: r <- E v
// TGV_SYM_NORM:     partial of Σ_i |(E v)_i|_F
enum TgvMode { TGV_FIELD = 0, TGV_SYM_ADJOINT = 1, TGV_P = 2, TGV_R = 3, TGV_SYM_GRADIENT = 4, TGV_SYM_NORM = 5 };

struct TgvLaunch {
    int dtype, D, wide;
    int C, c0, nc;
    int N[3];
    int tiles[3];
    int64_t G;                    // workgroups per component
    const void* x[kTvBatch];      // p-update: x⁺
    const void* q[kTvBatch];      // p-update: x̄
    void* v[kTvBatch][3];         // field: in place;  sym_adjoint: the output;  the others: v⁺ (sym_gradient / sym_norm: v), only read
    void* vb[kTvBatch][3];        // field: the output;  p- and r-update: v̄, only read
    void* p[kTvBatch][3];         // field: only read;  p-update: in place
    void* r[kTvBatch][6];         // field / sym_adjoint: only read;  r-update: in place;  sym_gradient: the output
    double alpha1[kTvBatch], alpha0[kTvBatch];
    double step, sigma;
    double* part;                 // [C][G] of the p-update, the r-update or the norm
    const int32_t* flag;          // may be null
};

hipError_t launch_tgv(const TgvLaunch& a, TgvMode mode, hipStream_t stream);

struct TgvSolve {
    int dtype, C, c0, nc, G;      // G: workgroups per component of the start kernel
    int64_t n, wstride;           // complex cells per component; reals between the components' blocks of w
    void* x[kTvBatch];
    void* w;                      // v, p, r, v̄ of every component: 3 D + S arrays each
    int max_iter, it, joint;
    double tol;
    const double* part_x;         // [C][P][2] of the primal kernel
    const double* part_p;         // [C][P]
    const double* part_r;         // [C][P]
    int64_t P;
    ProxScalars s;                // one slot per component; history [max_iter][C][3]
};

// x = 0 unless warm;  v = v̄ = p = r = 0;  scalars reset, NaN into the history
hipError_t launch_tgv_start(const TgvSolve& a, bool warm, hipStream_t stream);
// the decision of iteration a.it from the partial sums
hipError_t launch_tgv_decide(const TgvSolve& a, hipStream_t stream);

}  // namespace nufft
