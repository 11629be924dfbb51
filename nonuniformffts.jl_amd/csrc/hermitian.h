// What stands around the Jacobi of jacobi.h in the four objects that diagonalise a Hermitian K x K matrix on the device: the locally
// low-rank map (llr_kernels.hip), the global low-rank map (glr_kernels.hip; section 27), the coil-map estimate
// (coilmaps_kernels.hip; section 28) and coil compression (coilcomp_kernels.hip; section 29).  The Gram matrix of vectors staged in LDS
// (upper triangle, FP64, one fixed order of every sum), the set-up of the eigen problem, singular-value shrinkage with its projector, the
// epilogue of a solver's proximal step, and the flat tile loop that the Gram, apply and temporal (tsparse_kernels.hip) kernels walk.
// Every function is inlined into its caller: the kernels keep their names, launches and LDS layouts.
#pragma once

#include <algorithm>
#include <cstdint>

#include "jacobi.h"

namespace nufft {

// How n cells of K vectors are cut: tiles of TC cells (a power of two, 32 ... 1024), `tpw` consecutive tiles per workgroup, G <= max_groups
// workgroups.  S: segments of a tile's cells per Gram entry (a power of two).  Host and device use the same numbers.
struct FlatTiling {
    int TC, S, tpw, G;
    int64_t tiles;
};

// `budget`: elements of one tile in LDS with its padding cell per vector; TC doubles while twice the cells still fit, K (2 TC + 1) <= budget.
inline FlatTiling flat_tiling(int K, int64_t n, int budget, int threads, int max_groups) {
    FlatTiling tl{};
    tl.TC = 32;
    while (tl.TC < 1024 && K * (2 * tl.TC + 1) <= budget) tl.TC *= 2;
    const int np = K * (K + 1) / 2;
    tl.S = 1;
    while (tl.S < std::min(tl.TC / 4, 64) && np * tl.S < 2 * threads) tl.S *= 2;
    tl.tiles = (n + tl.TC - 1) / tl.TC;
    tl.tpw = (int)((tl.tiles + max_groups - 1) / max_groups);
    tl.G = (int)((tl.tiles + tl.tpw - 1) / tl.tpw);
    return tl;
}

namespace jacobi_team {

// The lanes of a team: the next power of two >= K
__host__ __device__ inline int team_width(int K) {
    int TW = 1;
    while (TW < K) TW *= 2;
    return TW;
}

// entry pr of the upper triangle, rows first: (0,0) (0,1) ... (0,K-1) (1,1) ...
__device__ __forceinline__ void pair_of(int pr, int K, int& i, int& j) {
    i = 0;
    while (pr >= K - i) {
        pr -= K - i;
        ++i;
    }
    j = i + pr;
}

// Σ_v conj(x[v]) y[v] w[v] over len elements in element order, FP64 (WEIGHTED = false: no w, and no multiply for it)
template <bool WEIGHTED, typename T>
__device__ __forceinline__ Cd gram_segment(const Cx<T>* x, const Cx<T>* y, int len, const double* w = nullptr) {
    double hr = 0.0, hi = 0.0;
    for (int v = 0; v < len; ++v) {
        const double ar = (double)x[v].re, ai = (double)x[v].im;
        const double br = WEIGHTED ? w[v] * (double)y[v].re : (double)y[v].re, bi = WEIGHTED ? w[v] * (double)y[v].im : (double)y[v].im;
        hr += ar * br + ai * bi;
        hi += ar * bi - ai * br;
    }
    return Cd{hr, hi};
}

// part[0] + part[stride] + ... (count terms, in that order)
__device__ __forceinline__ Cd fold(const Cd* part, int count, int64_t stride) {
    double hr = 0.0, hi = 0.0;
#pragma unroll 8
    for (int g = 0; g < count; ++g) {
        const Cd v = part[g * stride];
        hr += v.re;
        hi += v.im;
    }
    return Cd{hr, hi};
}

// Entry (i, j), i <= j, of a Hermitian matrix with its mirror image; the diagonal is real
__device__ __forceinline__ void store_hermitian(Cd* H, int K, int i, int j, Cd h) {
    if (i == j) {
        H[i * K + i] = Cd{h.re, 0.0};
    } else {
        H[i * K + j] = h;
        H[j * K + i] = Cd{h.re, -h.im};
    }
}

__device__ __forceinline__ Cd identity_entry(int i, int j) { return Cd{i == j ? 1.0 : 0.0, 0.0}; }

// f = σ > t ? 1 − t / σ : 0 of the eigenvalue λ = σ² of the Gram matrix; `nuc` gains f σ, the singular value after shrinkage
__device__ __forceinline__ double shrink_factor(double lam, double t, double& nuc) {
    const double sigma = sqrt(fmax(lam, 0.0));
    const double f = sigma > t ? 1.0 - t / sigma : 0.0;
    nuc += f * sigma;
    return f;
}

// Entry (i, j) of P = V diag(f) V^H
__device__ __forceinline__ Cd projector_entry(const Cd* V, const double* f, int K, int i, int j) {
    double pr = 0.0, pi = 0.0;
    for (int k = 0; k < K; ++k) {
        const Cd x = V[i * K + k], y = V[j * K + k];
        pr += f[k] * (x.re * y.re + x.im * y.im);
        pi += f[k] * (x.im * y.re - x.re * y.im);
    }
    return Cd{pr, pi};
}

// The end of an accelerated proximal step at one element: x <- x⁺ = res, z <- x⁺ + β (x⁺ − x); sdd gains |x⁺ − x|², sxx gains |x⁺|².
// Returns what it stored to z.
template <typename T>
__device__ __forceinline__ Cx<T> solver_epilogue(Cx<T>* x, Cx<T>* z, int64_t at, Cx<T> res, T beta, double& sdd, double& sxx) {
    const Cx<T> old = x[at];
    const T dr = res.re - old.re, di = res.im - old.im;
    sdd += (double)dr * (double)dr + (double)di * (double)di;
    sxx += (double)res.re * (double)res.re + (double)res.im * (double)res.im;
    x[at] = res;
    const Cx<T> zn{res.re + beta * dr, res.im + beta * di};
    z[at] = zn;
    return zn;
}

// The tiles of one workgroup of a kernel that is flat over n cells, and the tile in LDS: [vector][cell], the cell fastest, one padding
// cell per vector (TCP = TC + 1 keeps the vectors of one cell on different banks).
struct FlatTiles {
    int TC, TCP, tcs;
    int64_t tile0, tile1;
    template <typename Tiling>
    __device__ __forceinline__ explicit FlatTiles(const Tiling& tl) : TC(tl.TC), TCP(tl.TC + 1), tcs(0) {
        while ((1 << tcs) < TC) ++tcs;
        tile0 = (int64_t)blockIdx.x * tl.tpw;
        tile1 = min(tile0 + tl.tpw, tl.tiles);
    }
    __device__ __forceinline__ int64_t first_cell(int64_t tile) const { return tile << tcs; }
    __device__ __forceinline__ int cells(int64_t tile, int64_t n) const { return (int)min((int64_t)TC, n - first_cell(tile)); }
};

// Runs body(k, v) for every vector k < K and cell v < nc of a tile, a workgroup of THREADS threads, consecutive lanes along the cells
template <int THREADS, typename F>
__device__ __forceinline__ void for_tile(const FlatTiles& ft, int K, int nc, F body) {
    for (int u = threadIdx.x; u < (K << ft.tcs); u += THREADS) {
        const int k = u >> ft.tcs, v = u & (ft.TC - 1);
        if (v >= nc) continue;
        body(k, v);
    }
}

// Stages a whole tile, the cells beyond nc as exact zeros: value(k, at, live) gives element `at` of vector k.  A padding cell loads the
// tile's last cell and replaces what it got (live = false) -- a conditional 16-byte load went through scratch memory.
template <int THREADS, typename T, typename F>
__device__ __forceinline__ void stage_padded(Cx<T>* data, const FlatTiles& ft, int K, int64_t cell0, int nc, F value) {
    for (int u = threadIdx.x; u < (K << ft.tcs); u += THREADS) {
        const int k = u >> ft.tcs, v = u & (ft.TC - 1);
        const Cx<T> got = value(k, cell0 + min(v, nc - 1), v < nc);
        data[k * ft.TCP + v] = Cx<T>{v < nc ? got.re : T(0), v < nc ? got.im : T(0)};
    }
}

}  // namespace jacobi_team
}  // namespace nufft
