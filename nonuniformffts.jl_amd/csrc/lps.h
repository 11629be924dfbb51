// Launchers of the low-rank plus sparse objects (lps.cpp, glr_kernels.hip, tsparse_kernels.hip): the global
// low-rank map (Gram, eigen and apply kernels), the temporal transform with its shrink, and the solver's start, decision and sum kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "hermitian.h"
#include "nufft_mi355x.h"
#include "solver_decide.h"

namespace nufft {

constexpr int kLpsMaxK = 32;             // frames: a one-wave Jacobi team, K x K matrices in LDS, K pointers per array as kernel arguments
constexpr int kLpsThreads = 256;
constexpr int kGlrTileElems = 2048;      // cells x frames of one LDS tile of the Gram and apply kernels
constexpr int kTsTileElems = 1024;       // ... of the temporal kernel, which holds two tiles
constexpr int kGlrGramGroups = 1024;    // workgroups of the Gram kernel: the eigen kernel adds that many sets of partials
constexpr int kLpsStreamGroups = 4096;  // workgroups of the apply and temporal kernels, which leave two or three partial sums each
constexpr int kGlrPairsPerThread = 3;    // ceil(32 * 33 / 2 / 256) Gram entries a thread accumulates

// How the n cells are cut (FlatTiling of hermitian.h): K * TC <= tile_elems, stated as the budget that counts the padding cell of every frame
inline FlatTiling lps_tiling(int K, int64_t n, int tile_elems, int max_groups) { return flat_tiling(K, n, tile_elems + K, kLpsThreads, max_groups); }

// One array of K frames: the pointers travel as kernel arguments, the host writes no device table.
struct LpsFrames {
    void* p[kLpsMaxK];
};

enum { GLR_PLAIN = 0, GLR_SOLVER = 1 };

// GLR_PLAIN:  the matrix is f0 (the input); the apply kernel stores into f1.
// GLR_SOLVER: f0 = zL, f1 = zS, f2 = q, f3 = b in the Gram kernel, which forms g = step (q + lambda (zL + zS) − b), stores it over q and
//             takes zL − g as the matrix; f0 = zL, f1 = L, f2 = q (now g) in the apply kernel, which stores L <- L⁺,
//             zL <- L⁺ + beta (L⁺ − L) and the partials of ‖L⁺ − L‖², ‖L⁺‖².
struct GlrLaunch {
    int dtype, K, mode;
    FlatTiling tl;               // of the launch: the Gram kernel's (the eigen kernel adds tl.G sets) or the apply kernel's
    int64_t n;
    double t;                    // the threshold on the singular values
    double step, lambda, beta;
    double* gram;                // complex double [G][K (K + 1) / 2]
    double* P;                   // complex double [K][K]
    double* nuc;                 // double[1]: Σ_i f_i σ_i
    double* nuc_out;             // (null: none) the caller's copy
    int32_t* sweeps;             // int32[1]
    double* part;                // double[G][2] (GLR_SOLVER), G of the apply kernel's tiling
    const int32_t* flag;         // (null: none) a set flag[0] freezes the system: every workgroup leaves at once
    LpsFrames f0, f1, f2, f3;
};

hipError_t launch_glr_gram(const GlrLaunch& a, hipStream_t stream);
hipError_t launch_glr_eigen(const GlrLaunch& a, hipStream_t stream);
hipError_t launch_glr_apply(const GlrLaunch& a, hipStream_t stream);

enum { TS_FORWARD = 0, TS_INVERSE = 1, TS_SHRINK = 2, TS_SOLVER = 3 };

// TS_FORWARD / TS_INVERSE / TS_SHRINK: f0 the input, f1 the output.
// TS_SOLVER: f0 = zS, f1 = g (in q), f2 = S, f3 = zL, f4 = u: S⁺ = Tᴴ soft_t(T (zS − g)); S <- S⁺, zS <- S⁺ + beta (S⁺ − S), u <- zL + zS and
//            the partials of ‖S⁺ − S‖², ‖S⁺‖², ‖T S⁺‖₁.
struct TsLaunch {
    int dtype, K, mode, transform;
    FlatTiling tl;
    int64_t n;
    double t, beta;
    double tw[2 * kLpsMaxK];     // K^-1/2 exp(−2πi m / K), m < K, FP64: rounded once to the element type by the kernel
    double* part;                // double[G][3]: ‖S⁺ − S‖², ‖S⁺‖² (TS_SOLVER), ‖coefficients‖₁ (TS_SHRINK, TS_SOLVER)
    const int32_t* flag;
    LpsFrames f0, f1, f2, f3, f4;
};

hipError_t launch_tsparse(const TsLaunch& a, hipStream_t stream);
// out[0] = Σ_g part[g * 3 + 2], one workgroup, fixed order
hipError_t launch_tsparse_sum(const double* part, int G, double* out, hipStream_t stream);

struct LpsSolve {
    int dtype, K, G;
    int64_t n;
    int max_iter, it;
    double tol;
    const double* part_l;        // [Gl][2] of the apply kernel
    const double* part_s;        // [Gs][3] of the temporal kernel
    int Gl, Gs;
    const double* nuc;           // the eigen kernel's word
    ProxScalars s;               // one slot: the frames are one system; history [max_iter][3]: change, ‖C(L)‖_*, ‖T S‖₁
    LpsFrames x, L, S, zL, zS;
};

// L = zL = x (warm) or 0, x = 0 unless warm, S = zS = 0; scalars reset, history filled with NaN
hipError_t launch_lps_start(const LpsSolve& a, bool warm, hipStream_t stream);
hipError_t launch_lps_decide(const LpsSolve& a, hipStream_t stream);
// x = L + S
hipError_t launch_lps_sum(const LpsSolve& a, hipStream_t stream);

}  // namespace nufft
