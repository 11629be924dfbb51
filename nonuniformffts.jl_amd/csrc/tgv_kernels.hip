// Kernels of second-order total generalized variation and of its primal-dual solver (tgv.cpp, tv.cpp).
//
//     (E v)_de[i] = ½ ((v_d[i] − v_d[i − e_e]) + (v_e[i] − v_e[i − e_d]))          (Eᴴr)_d[i] = Σ_e (r_de[i] − r_de[i + e_e]),  r_ed = r_de
//
// indices mod N, on the array as stored; a symmetric tensor is S = D (D + 1) / 2 arrays in row-major upper-triangle order (tgv_pair).
// Three stencil kernels beside the TV solver's primal kernel, all bound by memory, on the data path of tv_kernels.hip: a lane owns one
// 16-byte pack along dimension 1, a wave marches kTvMarch cells along the outermost dimension with that dimension's neighbour carried
// in registers, lanes outside the box do nothing.  The "field" kernel reads r at i and i + e and writes v, v̄ at i; the "p" kernel reads
// x̄, x⁺ at i and i + e_d and v̄, v⁺ at i and writes p at i; the "r" kernel reads v̄, v⁺ at i and i − e and writes r at i: no launch reads
// at a neighbour an array it writes.
//
// Sums are FP64, one plain store per workgroup, reduced later in one fixed order.  A component whose done flag is set is frozen: its
// workgroups leave after reading the flag, before the first data load.
#include <hip/hip_runtime.h>

#include <cmath>

#include "nufft_mi355x.h"
#include "stream_kernels.h"
#include "tgv.h"
#include "tv_cells.h"
#include "tv_walk.h"

namespace nufft {
using namespace stream;
using namespace tvcells;
namespace {

template <typename T, int V>
__device__ __forceinline__ Cells<T, V> add(const Cells<T, V>& a, const Cells<T, V>& b) {
    Cells<T, V> r;
#pragma unroll
    for (int w = 0; w < V; ++w) r.v[w] = Cx<T>{a.v[w].re + b.v[w].re, a.v[w].im + b.v[w].im};
    return r;
}

// the cells at i + e_1 / i − e_1 of the pack c that was loaded from a[at]: one cell through the caches, the other from c itself
template <typename T, int V>
__device__ __forceinline__ Cells<T, V> next0(const Cx<T>* a, int64_t at, int64_t right, const Cells<T, V>& c) {
    Cells<T, V> n;
    n.v[V - 1] = a[at + right];
    if (V == 2) n.v[0] = c.v[V - 1];
    return n;
}
template <typename T, int V>
__device__ __forceinline__ Cells<T, V> prev0(const Cx<T>* a, int64_t at, int64_t left, const Cells<T, V>& c) {
    Cells<T, V> n;
    n.v[0] = a[at + left];
    if (V == 2) n.v[V - 1] = c.v[0];
    return n;
}

template <typename T>
__device__ __forceinline__ double abs2(Cx<T> z) {
    return (double)z.re * (double)z.re + (double)z.im * (double)z.im;
}

// v⁺ = v − τ (−p + Eᴴr);  v <- v⁺;  v̄ <- v⁺ + (v⁺ − v)      (TGV_FIELD)
// v <- Eᴴr                                                  (TGV_SYM_ADJOINT)
template <typename T, int D, int V, int MODE>
__global__ __launch_bounds__(kThreads) void tgv_field_kernel(TgvLaunch a) {
    using P = Cells<T, V>;
    constexpr int S = tgv_sym(D), MD = D - 1;
    const Walk w = walk_of<D, V>(a);
    if (a.flag && a.flag[w.c]) return;
    const Cx<T>* r[S];
#pragma unroll
    for (int s = 0; s < S; ++s) r[s] = static_cast<const Cx<T>*>(a.r[w.k][s]);
    Cx<T>* v[D];
    Cx<T>* vb[D];
    const Cx<T>* p[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        v[d] = static_cast<Cx<T>*>(a.v[w.k][d]);
        vb[d] = static_cast<Cx<T>*>(a.vb[w.k][d]);
        p[d] = static_cast<const Cx<T>*>(a.p[w.k][d]);
    }
    const T tau = (T)a.step;
    const int N0 = a.N[0], N1 = a.N[1], N2 = a.N[2];
    const int64_t SM = D == 2 ? (int64_t)N0 : (int64_t)N0 * N1;
    const int NM = D == 2 ? N1 : N2;
    if (!w.inside) return;
    int im = D == 2 ? w.i1 : w.i2;
    int64_t at = w.at;
    // neighbours that do not move with the march: i0 + V (one cell), and for D = 3 row i1 + 1
    const int64_t right = w.i0 + V == N0 ? (int64_t)V - N0 : V;
    const int64_t down = w.i1 + 1 == N1 ? -(int64_t)N0 * (N1 - 1) : (int64_t)N0;
    P cur[D];                                                        // r_{d,MD} at the cell of the march (D >= 2)
    if (D >= 2) {
#pragma unroll
        for (int d = 0; d < D; ++d) cur[d] = load_cells<T, V>(r[tgv_pair(D, d, MD)], at);
    }
    for (int m = 0; m < w.steps; ++m) {
        P rc[S];
#pragma unroll
        for (int d = 0; d < D; ++d)
#pragma unroll
            for (int e = d; e < D; ++e) rc[tgv_pair(D, d, e)] = D >= 2 && e == MD ? cur[d] : load_cells<T, V>(r[tgv_pair(D, d, e)], at);
        const int64_t nx = im + 1 == NM ? at - SM * (NM - 1) : at + SM;
        if (D >= 2) {
#pragma unroll
            for (int d = 0; d < D; ++d) cur[d] = load_cells<T, V>(r[tgv_pair(D, d, MD)], nx);      // the next cell's
        }
#pragma unroll
        for (int d = 0; d < D; ++d) {
            P acc{};
#pragma unroll
            for (int e = 0; e < D; ++e) {
                const int s = tgv_pair(D, d < e ? d : e, d < e ? e : d);
                P nb;
                if (e == 0) nb = next0<T, V>(r[s], at, right, rc[s]);
                else if (e == MD) nb = cur[d];
                else nb = load_cells<T, V>(r[s], at + down);
                const P t = sub(rc[s], nb);
                acc = e == 0 ? t : add(acc, t);
            }
            if (MODE == TGV_SYM_ADJOINT) {
                store_cells<T, V>(v[d], at, acc);
            } else {
                const P vv = load_cells<T, V>(v[d], at), pp = load_cells<T, V>(p[d], at);
                P vn, vbar;
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    vn.v[k].re = vv.v[k].re - tau * (acc.v[k].re - pp.v[k].re);
                    vn.v[k].im = vv.v[k].im - tau * (acc.v[k].im - pp.v[k].im);
                    vbar.v[k] = Cx<T>{vn.v[k].re + (vn.v[k].re - vv.v[k].re), vn.v[k].im + (vn.v[k].im - vv.v[k].im)};
                }
                store_cells<T, V>(v[d], at, vn);
                store_cells<T, V>(vb[d], at, vbar);
            }
        }
        ++im;
        at += SM;
    }
}

// p_d <- P_α1(p_d + σ ((∇x̄)_d − v̄_d)),  P_t(u)_i = u_i · min(1, t / |u_i|₂);  partial of Σ_i |(∇x⁺ − v⁺)_i|₂      (x̄ in q, x⁺ in x)
// (one mode, TGV_P: the parameter is there for NUFFT_TGV_DISPATCH)
template <typename T, int D, int V, int MODE>
__global__ __launch_bounds__(kThreads) void tgv_p_kernel(TgvLaunch a) {
    using P = Cells<T, V>;
    __shared__ double red[kWaves];
    const Walk w = walk_of<D, V>(a);
    if (a.flag && a.flag[w.c]) return;
    const Cx<T>* x = static_cast<const Cx<T>*>(a.x[w.k]);
    const Cx<T>* q = static_cast<const Cx<T>*>(a.q[w.k]);
    const Cx<T>* vp[D];
    const Cx<T>* vb[D];
    Cx<T>* p[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        vp[d] = static_cast<const Cx<T>*>(a.v[w.k][d]);
        vb[d] = static_cast<const Cx<T>*>(a.vb[w.k][d]);
        p[d] = static_cast<Cx<T>*>(a.p[w.k][d]);
    }
    const T sigma = (T)a.sigma, t = (T)a.alpha1[w.k];
    const int N0 = a.N[0], N1 = a.N[1], N2 = a.N[2];
    const int64_t SM = D == 2 ? (int64_t)N0 : (int64_t)N0 * N1;
    const int NM = D == 2 ? N1 : N2;
    double sum = 0.0;
    if (w.inside) {
        int im = D == 2 ? w.i1 : w.i2;
        int64_t at = w.at;
        const int64_t right = w.i0 + V == N0 ? (int64_t)V - N0 : V;
        const int64_t down = w.i1 + 1 == N1 ? -(int64_t)N0 * (N1 - 1) : (int64_t)N0;
        P xc = load_cells<T, V>(x, at), qc = load_cells<T, V>(q, at);
        for (int m = 0; m < w.steps; ++m) {
            P gx[D], gq[D];                                          // (∇x⁺ − v⁺)_d and (∇x̄ − v̄)_d of the lane's cells
            gx[0] = sub(next0<T, V>(x, at, right, xc), xc);
            gq[0] = sub(next0<T, V>(q, at, right, qc), qc);
            if (D == 3) {
                gx[1] = sub(load_cells<T, V>(x, at + down), xc);
                gq[1] = sub(load_cells<T, V>(q, at + down), qc);
            }
            if (D >= 2) {
                const int64_t nx = im + 1 == NM ? at - SM * (NM - 1) : at + SM;
                const P xn = load_cells<T, V>(x, nx), qn = load_cells<T, V>(q, nx);
                gx[D - 1] = sub(xn, xc);
                gq[D - 1] = sub(qn, qc);
                xc = xn;
                qc = qn;
            }
            P u[D];
            T s2[V];
            double f2[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                s2[e] = T(0);
                f2[e] = 0.0;
            }
#pragma unroll
            for (int d = 0; d < D; ++d) {
                gx[d] = sub(gx[d], load_cells<T, V>(vp[d], at));
                gq[d] = sub(gq[d], load_cells<T, V>(vb[d], at));
                u[d] = load_cells<T, V>(p[d], at);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    f2[e] += abs2(gx[d].v[e]);
                    u[d].v[e].re += sigma * gq[d].v[e].re;
                    u[d].v[e].im += sigma * gq[d].v[e].im;
                    s2[e] += u[d].v[e].re * u[d].v[e].re + u[d].v[e].im * u[d].v[e].im;
                }
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                sum += sqrt(f2[e]);
                const T nrm = sqrt(s2[e]);
                s2[e] = nrm > t ? t / nrm : T(1);
            }
#pragma unroll
            for (int d = 0; d < D; ++d) {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    u[d].v[e].re *= s2[e];
                    u[d].v[e].im *= s2[e];
                }
                store_cells<T, V>(p[d], at, u[d]);
            }
            ++im;
            at += SM;
        }
    }
    sum = block_reduce<Sum>(sum, red);
    if (threadIdx.x == 0) a.part[(int64_t)w.c * a.G + w.g] = sum;
}

// E v of the lane's cells: `cur` receives v_d at the cell, `prev` holds v_d at the previous cell of the march (D >= 2)
template <typename T, int D, int V>
__device__ __forceinline__ void sym_gradient_cells(const Cx<T>* const (&v)[D], int64_t at, int64_t left, int64_t up, const Cells<T, V> (&prev)[D],
                                                   Cells<T, V> (&cur)[D], Cells<T, V> (&E)[tgv_sym(D)]) {
    using P = Cells<T, V>;
    constexpr int MD = D - 1;
    P back[D][D];                                                    // back[d][e] = (∂⁻_e v_d) of the cells
#pragma unroll
    for (int d = 0; d < D; ++d) cur[d] = load_cells<T, V>(v[d], at);
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
        for (int e = 0; e < D; ++e) {
            P nb;
            if (e == 0) nb = prev0<T, V>(v[d], at, left, cur[d]);
            else if (e == MD) nb = prev[d];
            else nb = load_cells<T, V>(v[d], at + up);
            back[d][e] = sub(cur[d], nb);
        }
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
        for (int e = d; e < D; ++e) {
            const P s = add(back[d][e], back[e][d]);
            P h;
#pragma unroll
            for (int k = 0; k < V; ++k) h.v[k] = Cx<T>{T(0.5) * s.v[k].re, T(0.5) * s.v[k].im};
            E[tgv_pair(D, d, e)] = h;
        }
}

// r <- P_α0(r + σ E v̄),  P_t(u)_i = u_i · min(1, t / |u_i|_F);  partial of Σ_i |(E v⁺)_i|_F      (TGV_R: v̄ in vb, v⁺ in v)
// r <- E v                                                                                      (TGV_SYM_GRADIENT)
// partial of Σ_i |(E v)_i|_F                                                                    (TGV_SYM_NORM)
template <typename T, int D, int V, int MODE>
__global__ __launch_bounds__(kThreads) void tgv_r_kernel(TgvLaunch a) {
    using P = Cells<T, V>;
    constexpr int S = tgv_sym(D), MD = D - 1;
    constexpr bool BAR = MODE == TGV_R;
    constexpr bool SUM = MODE != TGV_SYM_GRADIENT;
    __shared__ double red[kWaves];
    const Walk w = walk_of<D, V>(a);
    if (a.flag && a.flag[w.c]) return;
    const Cx<T>* vp[D];
    const Cx<T>* vb[D];
    Cx<T>* r[S];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        vp[d] = static_cast<const Cx<T>*>(a.v[w.k][d]);
        vb[d] = BAR ? static_cast<const Cx<T>*>(a.vb[w.k][d]) : vp[d];
    }
#pragma unroll
    for (int s = 0; s < S; ++s) r[s] = static_cast<Cx<T>*>(a.r[w.k][s]);
    const T sigma = (T)a.sigma, t = (T)a.alpha0[w.k];
    const int N0 = a.N[0], N1 = a.N[1], N2 = a.N[2];
    const int64_t SM = D == 2 ? (int64_t)N0 : (int64_t)N0 * N1;
    const int NM = D == 2 ? N1 : N2;
    double sum = 0.0;
    if (w.inside) {
        int im = D == 2 ? w.i1 : w.i2;
        int64_t at = w.at;
        // neighbours that do not move with the march: i0 − 1 (one cell), and for D = 3 row i1 − 1
        const int64_t left = w.i0 == 0 ? (int64_t)N0 - 1 : -1;
        const int64_t up = w.i1 == 0 ? (int64_t)N0 * (N1 - 1) : -(int64_t)N0;
        P pprev[D], bprev[D];                                        // v⁺_d and v̄_d at the previous cell of the march
        if (D >= 2) {
            const int64_t pv = im == 0 ? at + SM * (NM - 1) : at - SM;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                pprev[d] = load_cells<T, V>(vp[d], pv);
                if (BAR) bprev[d] = load_cells<T, V>(vb[d], pv);
            }
        }
        for (int m = 0; m < w.steps; ++m) {
            P cur[D], E[S];
            sym_gradient_cells<T, D, V>(vp, at, left, up, pprev, cur, E);
#pragma unroll
            for (int d = 0; d < D; ++d) pprev[d] = cur[d];
            if (SUM) {
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    double f2 = 0.0;
#pragma unroll
                    for (int d = 0; d < D; ++d)
#pragma unroll
                        for (int e = d; e < D; ++e) f2 += (d == e ? 1.0 : 2.0) * abs2(E[tgv_pair(D, d, e)].v[k]);
                    sum += sqrt(f2);
                }
            }
            if (MODE == TGV_SYM_GRADIENT) {
#pragma unroll
                for (int s = 0; s < S; ++s) store_cells<T, V>(r[s], at, E[s]);
            }
            if (MODE == TGV_R) {
                sym_gradient_cells<T, D, V>(vb, at, left, up, bprev, cur, E);
#pragma unroll
                for (int d = 0; d < D; ++d) bprev[d] = cur[d];
                P u[S];
                T s2[V];
#pragma unroll
                for (int k = 0; k < V; ++k) s2[k] = T(0);
#pragma unroll
                for (int d = 0; d < D; ++d)
#pragma unroll
                    for (int e = d; e < D; ++e) {
                        const int s = tgv_pair(D, d, e);
                        u[s] = load_cells<T, V>(r[s], at);
#pragma unroll
                        for (int k = 0; k < V; ++k) {
                            u[s].v[k].re += sigma * E[s].v[k].re;
                            u[s].v[k].im += sigma * E[s].v[k].im;
                            s2[k] += (d == e ? T(1) : T(2)) * (u[s].v[k].re * u[s].v[k].re + u[s].v[k].im * u[s].v[k].im);
                        }
                    }
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const T nrm = sqrt(s2[k]);
                    s2[k] = nrm > t ? t / nrm : T(1);
                }
#pragma unroll
                for (int s = 0; s < S; ++s) {
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        u[s].v[k].re *= s2[k];
                        u[s].v[k].im *= s2[k];
                    }
                    store_cells<T, V>(r[s], at, u[s]);
                }
            }
            ++im;
            at += SM;
        }
    }
    if (SUM) {
        sum = block_reduce<Sum>(sum, red);
        if (threadIdx.x == 0) a.part[(int64_t)w.c * a.G + w.g] = sum;
    }
}

// x = 0 unless WARM;  v = v̄ = p = r = 0;  the first workgroup of a component resets its scalars and fills its history with NaN
template <typename T, bool WARM>
__global__ __launch_bounds__(kThreads) void tgv_start_kernel(TgvSolve a) {
    constexpr int W = Pack<T>::W;
    const int c = a.c0 + blockIdx.y;
    {
        T* w = static_cast<T*>(a.w) + c * a.wstride;                 // whole packs: the arrays are padded to 256 bytes
        NUFFT_FOR_EACH_PACK(T, a.wstride, i) {
            store(w, i, Pack<T>{});
            if (i + step__ < npacks__) store(w, i + step__, Pack<T>{});
        }
    }
    if (!WARM) {
        T* x = static_cast<T*>(a.x[blockIdx.y]);
        const int64_t nreal = 2 * a.n;
        NUFFT_FOR_EACH_PACK(T, nreal, i) {
            store(x, i, Pack<T>{});
            if (i + step__ < npacks__) store(x, i + step__, Pack<T>{});
        }
        if (blockIdx.x == 0 && threadIdx.x == 0)
            for (int64_t e = npacks__ * W; e < nreal; ++e) x[e] = T(0);
    }
    if (blockIdx.x == 0) reset_outcome<3>(a.s, c, a.C, a.max_iter);
}

// One workgroup per component: change, the two sums of the prior, the history row and the done flag of iteration a.it.  Coupled
// components are one system: the sums run over all components' rows (contiguous), and every component stores the same outcome.
__global__ __launch_bounds__(kThreads) void tgv_decide_kernel(TgvSolve a) {
    __shared__ double lds[kWaves];
    const int c = a.c0 + blockIdx.y;
    if (a.s.flag[c]) return;
    const int sc = a.joint ? 0 : c;
    const int rows = (int)((a.joint ? a.C : 1) * a.P);
    const double* px = a.part_x + (int64_t)sc * a.P * 2;
    const double dd = row_reduce<Sum>(px, rows, 2, lds);
    const double xx = row_reduce<Sum>(px + 1, rows, 2, lds);
    const double s1 = row_reduce<Sum>(a.part_p + (int64_t)sc * a.P, rows, 1, lds);
    const double s0 = row_reduce<Sum>(a.part_r + (int64_t)sc * a.P, rows, 1, lds);
    if (threadIdx.x == 0) {
        const int64_t row = ((int64_t)(a.it - 1) * a.C + c) * 3;
        store_decision(a.s, c, row, dd, xx, a.tol, a.it);
        a.s.history[row + 1] = s1;
        a.s.history[row + 2] = s0;
    }
}

template <typename K>
hipError_t launch(const TgvLaunch& a, K kernel, hipStream_t stream) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)a.tiles[0], (unsigned)a.tiles[1], (unsigned)(a.tiles[2] * a.nc)), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

// the instantiation for (element type, row alignment, D)
#define NUFFT_TGV_DISPATCH(kernel, MODE)                                                        \
    if (a.dtype == NUFFT_F64) {                                                                 \
        if (a.D == 1) return launch(a, kernel<double, 1, 1, MODE>, stream);                     \
        if (a.D == 2) return launch(a, kernel<double, 2, 1, MODE>, stream);                     \
        return launch(a, kernel<double, 3, 1, MODE>, stream);                                   \
    }                                                                                           \
    if (a.wide) {                                                                               \
        if (a.D == 1) return launch(a, kernel<float, 1, 2, MODE>, stream);                      \
        if (a.D == 2) return launch(a, kernel<float, 2, 2, MODE>, stream);                      \
        return launch(a, kernel<float, 3, 2, MODE>, stream);                                    \
    }                                                                                           \
    if (a.D == 1) return launch(a, kernel<float, 1, 1, MODE>, stream);                          \
    if (a.D == 2) return launch(a, kernel<float, 2, 1, MODE>, stream);                          \
    return launch(a, kernel<float, 3, 1, MODE>, stream)

}  // namespace

hipError_t launch_tgv(const TgvLaunch& a, TgvMode mode, hipStream_t stream) {
    switch (mode) {
        case TGV_FIELD: NUFFT_TGV_DISPATCH(tgv_field_kernel, TGV_FIELD);
        case TGV_SYM_ADJOINT: NUFFT_TGV_DISPATCH(tgv_field_kernel, TGV_SYM_ADJOINT);
        case TGV_P: NUFFT_TGV_DISPATCH(tgv_p_kernel, TGV_P);
        case TGV_R: NUFFT_TGV_DISPATCH(tgv_r_kernel, TGV_R);
        case TGV_SYM_GRADIENT: NUFFT_TGV_DISPATCH(tgv_r_kernel, TGV_SYM_GRADIENT);
        default: NUFFT_TGV_DISPATCH(tgv_r_kernel, TGV_SYM_NORM);
    }
}

hipError_t launch_tgv_start(const TgvSolve& a, bool warm, hipStream_t stream) {
    const dim3 gr(a.G, a.nc), bl(kThreads);
    if (warm) return launch_by_dtype(a.dtype, gr, bl, stream, tgv_start_kernel<float, true>, tgv_start_kernel<double, true>, a);
    return launch_by_dtype(a.dtype, gr, bl, stream, tgv_start_kernel<float, false>, tgv_start_kernel<double, false>, a);
}

hipError_t launch_tgv_decide(const TgvSolve& a, hipStream_t stream) {
    hipLaunchKernelGGL(tgv_decide_kernel, dim3(1, a.nc), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace nufft
