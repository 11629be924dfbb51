// Type-2 gradient gather (gfx950, wave64): the values v(x_j) and the D derivatives ∂_d v(x_j) of the type-2 interpolant
//
//   v(x) = h Σ_l g_l φ(x − x_l),   ∂_d v(x) = h Σ_l g_l ∂_d φ(x − x_l)
//
// from the grid g that the backward FFT of a type 2 left in the plan.  The result is the exact derivative
// of what the value gather computes, window by window, in both evaluation modes and for all four kernels.
//
// The kernel walks the sorted point records (PointRec) directly — it needs neither the tile tables of the LDS-tile engine
// nor the task tables of the rings, so it serves every sort (fine bins, two-level slabs, column layers) alike.
//
//   * G = nextpow2(2M) consecutive lanes own one point, lane q the stencil column j1 = q along dimension 1 (rows are
//     contiguous in memory: the G lanes of a group read one contiguous run of the row, periodically wrapped).
//   * Every lane evaluates the value AND the derivative of its own (d, j = q) window once per point; dimensions 2 and 3
//     reach the other lanes of the group by DPP row broadcasts (G = 8, 16) or ds_bpermute (G = 4, 32).
//   * The sums are factored so that the extra work is about one more FMA per grid value, not D more:
//       along dimension 2:  s = Σ g φ₂,  s' = Σ g φ₂'
//       along dimension 3:  A = Σ s φ₃,  B = Σ s' φ₃,  C = Σ s φ₃'
//       across the group :  v = Σ φ₁ A, ∂₁ = Σ φ₁' A, ∂₂ = Σ φ₁ B, ∂₃ = Σ φ₁ C      (group_sum butterflies)
//   * Lane q < D + 1 of the group stores output q (the value, then the D derivatives) with plain vector stores.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_common.h"
#include "nufft_mi355x.h"
#include "tile_kernels.h"     // dev_bessel_i0, dev_bspline_value

namespace nufft {

constexpr int kGradThreads = 256;
constexpr int kGradChunks = 4;           // chunks of PPB points per workgroup (C2 gather: 1 -> 5.53 ms, 4 -> 5.38 ms, 16 -> 6.17 ms)

// window selection, fixed per instantiation: the two default-path forms get kernels of their own
enum GradWindow { kGradBkbDirect = 0, kGradPoly = 1, kGradOther = 2 };

template <typename T>
struct GradKArgs {
    const void* sorted;                  // PointRec<T, D>[np]
    int64_t np;
    int Nover[3];
    const T* coefs;                      // [D][M + 4][2M] (polynomial forms)
    T p0[3], p1[3];                      // per-dimension window parameters, as in TileArgs::beta / bop
    int kernel, evalmode;
    int nc;                              // components of this launch (<= kMaxCompPerLaunch)
    const T* grid[kMaxCompPerLaunch];    // component grids (as arrays of reals)
    T* vout[kMaxCompPerLaunch];          // values (null: not requested)
    T* gout[kMaxCompPerLaunch][3];       // gradient components
    T prefactor;                         // prod(Δx_d)
    T dscale[3];                         // prefactor * dX_d / dx_d (Ñ_d / 2π, times −2π for the NFFT convention)
};

// ---- window derivatives ---------------------------------------------------------------------------------------------

// (t cosh t − sinh t) / t³ for t >= 0: the even Taylor series 1/3 + t²/30 + t⁴/840 + ... (Σ 2n / (2n+1)! t^(2n−2)) below 1,
// where the closed form cancels; one exponential above
template <typename T>
__device__ __forceinline__ T bkb_dratio(T t) {
    if (t < T(1)) {
        const T z = t * t;
        T p = T(20.0 / 51090942171709440000.0);          // n = 10: 20 / 21!
        p = fma(p, z, T(18.0 / 121645100408832000.0));   // 18 / 19!
        p = fma(p, z, T(16.0 / 355687428096000.0));      // 16 / 17!
        p = fma(p, z, T(14.0 / 1307674368000.0));        // 14 / 15!
        p = fma(p, z, T(12.0 / 6227020800.0));           // 12 / 13!
        p = fma(p, z, T(10.0 / 39916800.0));             // 10 / 11!
        p = fma(p, z, T(8.0 / 362880.0));                //  8 / 9!
        p = fma(p, z, T(6.0 / 5040.0));                  //  6 / 7!
        p = fma(p, z, T(4.0 / 120.0));                   //  4 / 5!
        return fma(p, z, T(1.0 / 3.0));                 //  2 / 3!
    }
    const T e = exp_pos(t);
    const T ei = div_pos(T(1), e);
    const T ch = T(0.5) * (e + ei), sh = T(0.5) * (e - ei);
    return div_pos(fma(t, ch, -sh), t * t * t);
}

// I₁(t) / t for t >= 0: power series (1/2) Σ (t²/4)^k / (k! (k+1)!), all terms positive
template <typename T>
__device__ __forceinline__ T dev_bessel_i1_over_x(T x) {
    const T q = T(0.25) * x * x;
    const T eps = sizeof(T) == 8 ? T(1e-17) : T(1e-9);
    T term = T(0.5), sum = T(0.5);
    for (int k = 1; k < 400; ++k) {
        term *= q / (T(k) * T(k + 1));
        sum += term;
        if (term < eps * sum) break;
    }
    return sum;
}

// derivative with respect to X of the order-2M B-spline window value j at x = 1 − X: the order-(2M − 1) splines
// b[i] = N_{2M−1}(x + i) of the same recursion stopped one order earlier give −N'_{2M}(x + j) = b[j − 1] − b[j]
template <typename T, int M>
__device__ __forceinline__ T dev_bspline_deriv(T x, int jsel) {
    constexpr int K = 2 * M - 1;
    T bs[K];
    bs[0] = T(1);
#pragma unroll
    for (int q = 2; q <= K; ++q) {
        const T alpha = T(1) / T(q - 1);
        T ds[K - 1];
        T xx = x;
#pragma unroll
        for (int j = 0; j < q - 1; ++j) { ds[j] = alpha * xx; xx += T(1); }
        bs[q - 1] = (T(1) - ds[q - 2]) * bs[q - 2];
#pragma unroll
        for (int j = q - 2; j >= 1; --j) bs[j] = (T(1) - ds[j - 1]) * bs[j - 1] + ds[j] * bs[j];
        bs[0] = ds[0] * bs[0];
    }
    T lo = T(0), hi = T(0);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        lo = jsel - 1 == j ? bs[j] : lo;
        hi = jsel == j ? bs[j] : hi;
    }
    return lo - hi;
}

// Value and derivative d/dX of window value j (0-based, node c − M + 1 + j) of a point at cell fraction X along dimension d;
// p0 / p1 as TileArgs::beta / bop; cs: the polynomial coefficients of (d, j) with stride 2M.  The value is computed exactly
// as the value gather does (WindowEval::eval_regs).
template <typename T, int M, int WSEL>
__device__ __forceinline__ void window_value_deriv(int kernel, int evalmode, T X, int j, T p0, T p1, const T* cs, T& val, T& der) {
    constexpr int L = 2 * M;
    if constexpr (WSEL == kGradPoly) {
        constexpr int NP = M + 4;
        const T xx = T(2) * X - T(1);
        T p = cs[(NP - 1) * L], dp = T(0);
#pragma unroll
        for (int c = NP - 2; c >= 0; --c) {
            dp = fma(xx, dp, p);
            p = fma(xx, p, cs[c * L]);
        }
        val = p;
        der = T(2) * dp;
        return;
    }
    const T y = (T(M - 1 - j) + X) / T(M);
    if constexpr (WSEL == kGradBkbDirect) {
        const T z = T(1) - y * y;
        const T s = sqrt_unit(z > T(0) ? z : T(0));
        const T t = p0 * s;
        val = sinh_over_x(t) * p1;
        // dφ/dy = −(β/π) β² y (t cosh t − sinh t) / t³, dy/dX = 1/M
        der = -(p1 * p0 * p0 * y) * bkb_dratio(t) / T(M);
        return;
    }
    (void)evalmode;
    if (kernel == NUFFT_KERNEL_KAISER_BESSEL) {          // (Direct; the polynomial form is kGradPoly)
        const T z = T(1) - y * y;
        const T t = p0 * sqrt(z > T(0) ? z : T(0));
        val = dev_bessel_i0<T>(t) * p1;
        der = -(p1 * p0 * p0 * y) * dev_bessel_i1_over_x(t) / T(M);
    } else if (kernel == NUFFT_KERNEL_GAUSSIAN) {
        const T dx = p0, tau = p1;
        const T ys = (T(M - 1 - j) + X) * dx;
        if (evalmode == NUFFT_EVAL_DIRECT) {
            val = exp(-(ys * ys) / tau);
        } else {                                          // fast Gaussian gridding, as WindowEval
            const int m = j - (M - 1);
            const int am = m < 0 ? -m : m;
            const T xm = T(am) * dx;
            const T csm = exp(-(xm * xm) / tau);
            const T Xp = X * dx;
            const T av = exp(-(Xp * Xp) / tau);
            const T bv = exp(T(2) * Xp * dx / tau);
            T bpow = T(1);
            for (int i = 0; i < (am < M - 1 ? am : M - 1); ++i) bpow *= bv;
            const T ac = av * csm;
            val = m == 0 ? av : (m < 0 ? ac / bpow : (m < M ? ac * bpow : ac * bpow * bv));
        }
        der = (T(-2) * ys * dx / tau) * val;
    } else {                                              // B-spline, both modes
        val = dev_bspline_value<T, M>(T(1) - X, j);
        der = dev_bspline_deriv<T, M>(T(1) - X, j);
    }
}

// ---- broadcast inside a group of G lanes ----------------------------------------------------------------------------

// value of lane j (compile-time after unrolling) of this lane's group
template <int G, typename T>
__device__ __forceinline__ T grp_bcast(T x, int j) {
    if constexpr (G == 16) return row_bcast(x, j);
    else if constexpr (G == 8) return half_bcast(x, j);
    else return __shfl(x, j, G);
}

__device__ __forceinline__ int grad_wrap(int i, int n) {
    i %= n;
    return i < 0 ? i + n : i;
}

// ---- the kernel -----------------------------------------------------------------------------------------------------

template <typename T, bool CPLX, int D, int M, int WSEL>
__global__ __launch_bounds__(kGradThreads) void interp_grad_kernel(GradKArgs<T> a) {
    constexpr int L = 2 * M;
    constexpr int G = next_pow2(L);
    constexpr int PPB = kGradThreads / G;            // points per block at once
    constexpr int NP = M + 4;
    constexpr int NQ = CPLX ? 2 : 1;                 // reals per grid element
    using V = typename std::conditional<CPLX, typename std::conditional<sizeof(T) == 8, double2, float2>::type, T>::type;

    const PointRec<T, D>* sorted = static_cast<const PointRec<T, D>*>(a.sorted);
    const int q = threadIdx.x & (G - 1);             // lane in the group = stencil column j1 (lanes >= 2M: weight 0)
    const int j1 = q < L ? q : L - 1;
    const int grp = threadIdx.x / G;
    const int N1 = a.Nover[0], N2 = a.Nover[1], N3 = a.Nover[2];

    // the group loop is uniform over the block (every lane runs every iteration: the broadcasts need the whole wave);
    // groups past the end repeat the last point and store nothing
    // XCD-aware order: each XCD takes one contiguous range of the sorted array (a compact region of the grid that its L2 keeps),
    // each workgroup a run of kGradChunks consecutive chunks of PPB points
    const int64_t nchunk = (a.np + PPB - 1) / PPB;
    const int64_t c0 = (int64_t)xcd_remap((int)blockIdx.x, (int)gridDim.x) * kGradChunks;
    const int64_t c1 = c0 + kGradChunks < nchunk ? c0 + kGradChunks : nchunk;
    for (int64_t ch = c0; ch < c1; ++ch) {
        const int64_t pidx = ch * PPB + grp;
        const bool have = pidx < a.np;
        const PointRec<T, D> rec = sorted[have ? pidx : a.np - 1];

        int cell[3] = {0, 0, 0};
        T wv[3], wd[3];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int c = cell_of(rec.r[d], a.Nover[d]);
            cell[d] = c;
            const T X = rec.r[d] - T(c);
            window_value_deriv<T, M, WSEL>(a.kernel, a.evalmode, X, j1, a.p0[d], a.p1[d],
                                           WSEL == kGradPoly ? a.coefs + (size_t)d * NP * L + j1 : nullptr, wv[d], wd[d]);
        }
        const T w1 = q < L ? wv[0] : T(0);
        const T d1 = q < L ? wd[0] : T(0);

        // stencil rows / planes: wrapped offsets in elements
        const int i1 = grad_wrap(cell[0] - (M - 1) + j1, N1);
        int off2[D >= 2 ? L : 1];
        T w2[D >= 2 ? L : 1], dw2[D >= 2 ? L : 1];
        if constexpr (D >= 2) {
            const int s2 = grad_wrap(cell[1] - (M - 1), N2);
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const int r = s2 + j;
                off2[j] = (r >= N2 ? r - N2 : r) * N1;
                w2[j] = grp_bcast<G>(wv[1], j);
                dw2[j] = grp_bcast<G>(wd[1], j);
            }
        }
        const int s3 = D >= 3 ? grad_wrap(cell[2] - (M - 1), N3) : 0;

        for (int c = 0; c < a.nc; ++c) {
            const V* g = reinterpret_cast<const V*>(a.grid[c]) + i1;
            // per-lane partial sums over dimensions 2 and 3 of the lane's column: A (value), B (∂₂), Cs (∂₃)
            T A[NQ], B[NQ], Cs[NQ];
#pragma unroll
            for (int u = 0; u < NQ; ++u) { A[u] = T(0); B[u] = T(0); Cs[u] = T(0); }
            auto ld = [&](int64_t off, T (&v)[NQ]) {
                const V x = g[off];
                if constexpr (CPLX) { v[0] = x.x; v[1] = x.y; } else { v[0] = x; }
            };
            if constexpr (D == 1) {
                ld(0, A);
            } else {
#pragma unroll
                for (int j3 = 0; j3 < (D >= 3 ? L : 1); ++j3) {
                    int64_t plane = 0;
                    if constexpr (D >= 3) {
                        const int r = s3 + j3;
                        plane = (int64_t)(r >= N3 ? r - N3 : r) * N2 * N1;
                    }
                    T s[NQ], sd[NQ];
#pragma unroll
                    for (int u = 0; u < NQ; ++u) { s[u] = T(0); sd[u] = T(0); }
#pragma unroll
                    for (int j2 = 0; j2 < L; ++j2) {
                        T gv[NQ];
                        ld(plane + off2[j2], gv);
#pragma unroll
                        for (int u = 0; u < NQ; ++u) {
                            s[u] = fma(gv[u], w2[j2], s[u]);
                            sd[u] = fma(gv[u], dw2[j2], sd[u]);
                        }
                    }
                    if constexpr (D == 2) {
#pragma unroll
                        for (int u = 0; u < NQ; ++u) { A[u] = s[u]; B[u] = sd[u]; }
                    } else {
                        const T w3 = grp_bcast<G>(wv[2], j3), dw3 = grp_bcast<G>(wd[2], j3);
#pragma unroll
                        for (int u = 0; u < NQ; ++u) {
                            A[u] = fma(s[u], w3, A[u]);
                            B[u] = fma(sd[u], w3, B[u]);
                            Cs[u] = fma(s[u], dw3, Cs[u]);
                        }
                    }
                }
            }
            // across the group: out[0] = value, out[1 + d] = ∂_d
            T out[D + 1][NQ];
#pragma unroll
            for (int u = 0; u < NQ; ++u) {
                out[0][u] = group_sum<T, G, false>(w1 * A[u]);
                out[1][u] = group_sum<T, G, false>(d1 * A[u]);
                if constexpr (D >= 2) out[2][u] = group_sum<T, G, false>(w1 * B[u]);
                if constexpr (D >= 3) out[3][u] = group_sum<T, G, false>(w1 * Cs[u]);
            }
            if (have && q <= D) {
                T* dst;
                T scale;
                if (q == 0) { dst = a.vout[c]; scale = a.prefactor; }
                else { dst = a.gout[c][q - 1]; scale = a.dscale[q - 1]; }
                T r[NQ];
#pragma unroll
                for (int u = 0; u < NQ; ++u) {
                    T x = out[0][u];
#pragma unroll
                    for (int k = 1; k <= D; ++k) x = q == k ? out[k][u] : x;
                    r[u] = x * scale;
                }
                if (dst) {
                    V* o = reinterpret_cast<V*>(dst) + rec.idx;
                    if constexpr (CPLX) *o = V{r[0], r[1]};
                    else *o = r[0];
                }
            }
        }
    }
}

}  // namespace nufft
