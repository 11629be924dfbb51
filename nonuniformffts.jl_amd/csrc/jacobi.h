// The cyclic complex Jacobi of a Hermitian K x K matrix by a team of lanes of one wave: device code shared by the locally low-rank
// kernel (llr_kernels.hip), the global low-rank eigen kernel (glr_kernels.hip; section 27), the coil-map kernel
// (coilmaps_kernels.hip; section 28) and the eigen kernel of coil compression (coilcomp_kernels.hip; section 29).  All get the same
// rotation order and the same skip constants; tests/llr_reference.py (jacobi_eigh) restates them.  hermitian.h holds what these kernels
// do around the Jacobi.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace nufft {
namespace jacobi_team {

constexpr int kSweepsMax = 24;             // cap of the cyclic sweeps

template <typename T>
struct Cx {
    T re, im;
};
using Cd = Cx<double>;

constexpr double kSkipRel = 0x1p-106;      // a rotation is skipped when |h_pq|² <= 2^-106 h_pp h_qq ...
constexpr double kSkipAbs = 0x1p-60;       // ... or |h_pq| <= 2^-60 trace(H)

__device__ __forceinline__ void team_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (x, y) <- (c x − conj(sp) y, sp x + c y): a pair of one row of A J, J = [[c, sp], [−conj(sp), c]]
__device__ __forceinline__ void rotate_columns(Cd& x, Cd& y, double c, double sr, double si) {
    const Cd nx{c * x.re - (y.re * sr + y.im * si), c * x.im - (y.im * sr - y.re * si)};
    const Cd ny{(x.re * sr - x.im * si) + c * y.re, (x.re * si + x.im * sr) + c * y.im};
    x = nx;
    y = ny;
}

// (x, y) <- (c x − sp y, conj(sp) x + c y): a pair of one column of J^H A
__device__ __forceinline__ void rotate_rows(Cd& x, Cd& y, double c, double sr, double si) {
    const Cd nx{c * x.re - (sr * y.re - si * y.im), c * x.im - (sr * y.im + si * y.re)};
    const Cd ny{(sr * x.re + si * x.im) + c * y.re, (sr * x.im - si * x.re) + c * y.im};
    x = nx;
    y = ny;
}

// Cyclic-by-rows Jacobi on the Hermitian K x K matrix H (row-major, in LDS), V <- V J for every rotation; lane r < TW of the team, TW
// the next power of two >= K.  The rotations run one after the other, lane r updates row r of H J and of V J, then column r of
// J^H (H J); the lanes of a team take every branch together and the LDS serves a wave's accesses in order, so the team needs no
// workgroup barrier.  Stops after the first sweep that rotates nothing, or after kSweepsMax sweeps; returns the sweeps run.
__device__ inline int jacobi(Cd* H, Cd* V, int K, int r) {
    double tr = 0.0;
    for (int i = 0; i < K; ++i) tr += H[i * K + i].re;
    const double floor2 = (kSkipAbs * tr) * (kSkipAbs * tr);
    const bool mine = r < K;
    int sweeps = 0;
    for (int sweep = 0; sweep < kSweepsMax; ++sweep) {
        bool rotated = false;
        ++sweeps;
        for (int p = 0; p < K - 1; ++p)
            for (int q = p + 1; q < K; ++q) {
                team_sync();
                const double app = H[p * K + p].re, aqq = H[q * K + q].re;
                const Cd g = H[p * K + q];
                // |h_pq|² underflows to 0 for |h_pq| below about 1e-162, that is for data below about 1e-81 (both element types:
                // H is FP64): such a matrix is treated as diagonal.  Data above about 1e+150 overflow H.
                const double g2 = g.re * g.re + g.im * g.im;
                if (g2 <= fmax(kSkipRel * fabs(app * aqq), floor2)) continue;
                rotated = true;
                const double ag = sqrt(g2);
                const double tau = (aqq - app) / (2.0 * ag);
                const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                const double c = 1.0 / sqrt(1.0 + tt * tt), s = tt * c;
                const double sr = s * (g.re / ag), si = s * (g.im / ag);
                team_sync();                                       // every lane has read h_pp, h_qq, h_pq
                if (mine) {
                    Cd x = H[r * K + p], y = H[r * K + q];
                    rotate_columns(x, y, c, sr, si);
                    H[r * K + p] = x;
                    H[r * K + q] = y;
                    x = V[r * K + p];
                    y = V[r * K + q];
                    rotate_columns(x, y, c, sr, si);
                    V[r * K + p] = x;
                    V[r * K + q] = y;
                }
                team_sync();
                if (mine) {
                    Cd x = H[p * K + r], y = H[q * K + r];
                    rotate_rows(x, y, c, sr, si);
                    H[p * K + r] = x;
                    H[q * K + r] = y;
                }
                team_sync();
                if (r == 0) {
                    H[p * K + q] = Cd{0.0, 0.0};
                    H[q * K + p] = Cd{0.0, 0.0};
                    H[p * K + p].im = 0.0;
                    H[q * K + q].im = 0.0;
                }
            }
        if (!rotated) break;
    }
    team_sync();
    return sweeps;
}

}  // namespace jacobi_team
}  // namespace nufft
