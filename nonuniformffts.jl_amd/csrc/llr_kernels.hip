// The locally low-rank proximal map: singular-value soft-thresholding of the B x K Casorati matrix M of every spatial block, through
// the K x K Gram matrix (llr.h, llr.cpp, fista.cpp).
//
//     H = M^H M  (FP64)      H = V Λ V^H  (jacobi.h, FP64)                    σ_i = sqrt(max(λ_i, 0))      f_i = σ_i > t ? 1 − t / σ_i : 0
//     P = V diag(f) V^H      M <- M P                                        nuclear-norm partial += Σ_i f_i σ_i
//
// A workgroup owns nb whole blocks.  Their values are read from global memory once, into LDS ([blk][k][voxel], in the element type), stay
// there through the Gram pass and the multiply by P, and are written once.  H, V and P are FP64 in LDS.  A block is diagonalised by a
// team of TW = team_width(K) lanes of one wave (jacobi.h).  The Gram sum, the Hermitian store, the shrink factors and the projector are
// those of hermitian.h.  Every sum has one fixed order (Gram entries: voxel order inside a segment, then segment order; partial sums:
// stream_kernels.h), and there are no atomics: two runs give the same bits.
//
// LLR_FISTA forms v = z − τ (q + μ z − b) while it loads and x⁺ = result, z = x⁺ + β (x⁺ − x), x = x⁺ while it stores, with the partial
// sums of |x⁺ − x|², |x⁺|² next to the nuclear norm's: with the decision kernel that is a whole iteration outside the apply.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "hermitian.h"
#include "llr.h"
#include "stream_kernels.h"

namespace nufft {
using namespace stream;

static_assert(kLlrThreads == kThreads, "the reductions of stream_kernels.h");
static_assert(kLlrSweepsMax == jacobi_team::kSweepsMax, "nufft_llr_info.jacobi_sweeps_max reports the cap of jacobi.h");

namespace {

using namespace jacobi_team;

template <typename T, int MODE>
__global__ __launch_bounds__(kLlrThreads) void llr_kernel(LlrLaunch a, LlrLayout L) {
    extern __shared__ __align__(16) unsigned char smem[];
    if (a.flag && a.flag[0]) return;
    const int K = a.K, tid = threadIdx.x;
    const int bs0 = a.bshift[0], bs1 = a.bshift[1], bsB = a.bshift[0] + a.bshift[1] + a.bshift[2];
    const int B = 1 << bsB, np = K * (K + 1) / 2, nb = L.nb, S = L.S;
    Cx<T>* data = reinterpret_cast<Cx<T>*>(smem);
    Cd* Hs = reinterpret_cast<Cd*>(smem + L.off_H);
    Cd* Vs = reinterpret_cast<Cd*>(smem + L.off_V);
    Cd* gp = reinterpret_cast<Cd*>(smem + L.off_g);             // shares its space with V: V starts after the Gram entries are summed
    double* fs = reinterpret_cast<double*>(smem + L.off_lam);
    double* red = reinterpret_cast<double*>(smem + L.off_red);
    int* co = reinterpret_cast<int*>(red + kWaves);             // [nb][3]: the first storage index of a block per dimension, not yet wrapped
    const int64_t blk0 = (int64_t)blockIdx.x * nb;
    const int nbl = (int)(a.blocks - blk0 < nb ? a.blocks - blk0 : nb);

    if (tid < nbl) {
        const int64_t id = blk0 + tid;
        const int c0 = (int)(id % a.nblk[0]), c1 = (int)((id / a.nblk[0]) % a.nblk[1]), c2 = (int)(id / ((int64_t)a.nblk[0] * a.nblk[1]));
        co[tid * 3 + 0] = (c0 << bs0) + a.shift[0];
        co[tid * 3 + 1] = (c1 << bs1) + a.shift[1];
        co[tid * 3 + 2] = (c2 << a.bshift[2]) + a.shift[2];
    }
    __syncthreads();

    // a unit of the load and of the store: (k, voxel beyond dimension 1, block, voxel along dimension 1), the last fastest, so that
    // consecutive lanes walk along dimension 1 through the workgroup's blocks
    int nbs = 0;
    while ((1 << nbs) < nb) ++nbs;
    const int units = K << (bsB + nbs);
    auto locate = [&](int u, int& k, int& blk, int& v, int64_t& at) {
        const int v1 = u & ((1 << bs0) - 1);
        blk = (u >> bs0) & (nb - 1);
        const int rest = u >> (bs0 + nbs);
        const int vr = rest & ((1 << (bsB - bs0)) - 1);
        k = rest >> (bsB - bs0);
        v = (vr << bs0) | v1;
        if (blk >= nbl) return false;
        int i0 = co[blk * 3 + 0] + v1, i1 = co[blk * 3 + 1] + (vr & ((1 << bs1) - 1)), i2 = co[blk * 3 + 2] + (vr >> bs1);
        if (i0 >= a.N[0]) i0 -= a.N[0];
        if (i1 >= a.N[1]) i1 -= a.N[1];
        if (i2 >= a.N[2]) i2 -= a.N[2];
        at = i0 + i1 * a.pitch[1] + i2 * a.pitch[2];
        return true;
    };

    const T tau = (T)a.step, mu = (T)a.lambda;
    for (int u = tid; u < units; u += kLlrThreads) {
        int k, blk, v;
        int64_t at;
        if (!locate(u, k, blk, v, at)) continue;
        Cx<T> val;
        if (MODE == LLR_FISTA) {
            const Cx<T> zv = reinterpret_cast<const Cx<T>*>(static_cast<const T*>(a.z) + k * a.stride)[at];
            const Cx<T> qv = reinterpret_cast<const Cx<T>*>(static_cast<const T*>(a.q) + k * a.stride)[at];
            const Cx<T> bv = static_cast<const Cx<T>*>(a.in[k])[at];
            val.re = zv.re - tau * (qv.re + mu * zv.re - bv.re);
            val.im = zv.im - tau * (qv.im + mu * zv.im - bv.im);
        } else {
            val = static_cast<const Cx<T>*>(a.in[k])[at];
        }
        data[((blk * K + k) << bsB) + v] = val;
    }
    __syncthreads();

    // Gram entries (i <= j) of every block, S voxel segments each
    const int seg_len = B / S;
    for (int u = tid; u < nbl * S * np; u += kLlrThreads) {
        const int seg = (u / np) % S, blk = u / (np * S);
        int i, j;
        pair_of(u % np, K, i, j);
        gp[u] = gram_segment<false>(data + ((blk * K + i) << bsB) + seg * seg_len, data + ((blk * K + j) << bsB) + seg * seg_len, seg_len);
    }
    __syncthreads();
    for (int u = tid; u < nbl * np; u += kLlrThreads) {
        const int blk = u / np;
        int i, j;
        pair_of(u % np, K, i, j);
        Cd h{0.0, 0.0};                                         // the segments in order (fold of hermitian.h unrolls for long global sums)
        for (int seg = 0; seg < S; ++seg) {
            const Cd g = gp[(blk * S + seg) * np + (u % np)];
            h.re += g.re;
            h.im += g.im;
        }
        store_hermitian(Hs + blk * K * K, K, i, j, h);
    }
    __syncthreads();
    for (int u = tid; u < nbl * K * K; u += kLlrThreads) {
        const int e = u % (K * K);
        Vs[u] = identity_entry(e / K, e % K);
    }
    __syncthreads();

    if (K > 1) {
        const int team = tid / L.TW, r = tid % L.TW, teams = kLlrThreads / L.TW;
        for (int blk = team; blk < nbl; blk += teams) jacobi(Hs + blk * K * K, Vs + blk * K * K, K, r);
    }
    __syncthreads();

    double nuc = 0.0;
    for (int u = tid; u < nbl * K; u += kLlrThreads) {
        const int blk = u / K, i = u % K;
        fs[u] = shrink_factor(Hs[blk * K * K + i * K + i].re, a.t, nuc);
    }
    __syncthreads();
    for (int u = tid; u < nbl * K * K; u += kLlrThreads) {      // P over H
        const int blk = u / (K * K), e = u % (K * K);
        Hs[u] = projector_entry(Vs + blk * K * K, fs + blk * K, K, e / K, e % K);
    }
    __syncthreads();

    const T beta = (T)a.beta;
    double sdd = 0.0, sxx = 0.0;
    for (int u = tid; u < units; u += kLlrThreads) {
        int j, blk, v;
        int64_t at;
        if (!locate(u, j, blk, v, at)) continue;
        const Cd* P = Hs + blk * K * K;
        const Cx<T>* m = data + ((blk * K) << bsB) + v;
        double rr = 0.0, ri = 0.0;
        for (int i = 0; i < K; ++i) {
            const double mr = (double)m[i << bsB].re, mi = (double)m[i << bsB].im;
            const Cd p = P[i * K + j];
            rr += mr * p.re - mi * p.im;
            ri += mr * p.im + mi * p.re;
        }
        const Cx<T> res{(T)rr, (T)ri};
        Cx<T>* x = static_cast<Cx<T>*>(a.out[j]);
        if (MODE == LLR_FISTA) {
            // solver_epilogue of hermitian.h with both sums of squares as explicit fused multiply-adds: which product the compiler fuses
            // on its own changes with the code around it, and with it the last bit of the ComplexF64 partials
            const Cx<T> old = x[at];
            const T dr = res.re - old.re, di = res.im - old.im;
            sdd += fma((double)dr, (double)dr, (double)di * (double)di);
            sxx += fma((double)res.re, (double)res.re, (double)res.im * (double)res.im);
            x[at] = res;
            reinterpret_cast<Cx<T>*>(static_cast<T*>(a.z) + j * a.stride)[at] = Cx<T>{res.re + beta * dr, res.im + beta * di};
        } else {
            x[at] = res;
        }
    }
    nuc = block_reduce<Sum>(nuc, red);
    if (MODE == LLR_FISTA) {
        sdd = block_reduce<Sum>(sdd, red);
        sxx = block_reduce<Sum>(sxx, red);
    }
    if (tid == 0) {
        double* out = a.part + (int64_t)blockIdx.x * 3;
        out[0] = sdd;
        out[1] = sxx;
        out[2] = nuc;
    }
}

__global__ __launch_bounds__(kThreads) void llr_sum_kernel(const double* part, int64_t G, double* out) {
    __shared__ double lds[kWaves];
    double v = 0.0;
    for (int64_t g = threadIdx.x; g < G; g += kThreads) v += part[g * 3 + 2];
    v = block_reduce<Sum>(v, lds);
    if (threadIdx.x == 0) out[0] = v;
}

template <typename T, int MODE>
hipError_t launch_one(const LlrLaunch& a, const LlrLayout& L, hipStream_t stream) {
    hipLaunchKernelGGL((llr_kernel<T, MODE>), dim3((unsigned)llr_workgroups(a)), dim3(kLlrThreads), L.bytes, stream, a, L);
    return hipGetLastError();
}

}  // namespace

LlrLayout llr_layout(bool f32, int K, int B) {
    LlrLayout L{};
    const int E = B * K, np = K * (K + 1) / 2;
    const size_t eb = f32 ? 8 : 16;
    L.TW = team_width(K);
    int nb = 1;
    while (nb < 256 && 2 * nb * E <= kLlrTileElems) nb *= 2;
    for (;; nb /= 2) {
        int S = 1;
        while (S < std::min(B, kLlrMaxSegments) && nb * np * S < 2 * kLlrThreads) S *= 2;
        L.nb = nb;
        L.S = S;
        L.off_H = up16((size_t)nb * E * eb);
        L.off_V = L.off_g = L.off_H + (size_t)nb * K * K * 16;
        L.off_lam = L.off_V + (size_t)nb * std::max(K * K, S * np) * 16;
        L.off_red = up16(L.off_lam + (size_t)nb * K * 8);
        L.bytes = up16(L.off_red + kWaves * 8 + (size_t)nb * 3 * 4);
        if (nb == 1 || L.bytes <= (64u << 10)) break;
    }
    return L;
}

int64_t llr_workgroups(const LlrLaunch& a) {
    const int B = 1 << (a.bshift[0] + a.bshift[1] + a.bshift[2]);
    const int nb = llr_layout(a.dtype == NUFFT_F32, a.K, B).nb;
    return (a.blocks + nb - 1) / nb;
}

// Workgroups above 64 KiB of dynamic LDS must be allowed per kernel (and device): called when an object is created.
hipError_t llr_allow_lds() {
    return allow_large_lds({reinterpret_cast<const void*>(&llr_kernel<float, LLR_PLAIN>), reinterpret_cast<const void*>(&llr_kernel<float, LLR_FISTA>),
                            reinterpret_cast<const void*>(&llr_kernel<double, LLR_PLAIN>), reinterpret_cast<const void*>(&llr_kernel<double, LLR_FISTA>)});
}

hipError_t launch_llr(const LlrLaunch& a, hipStream_t stream) {
    const bool f32 = a.dtype == NUFFT_F32;
    const LlrLayout L = llr_layout(f32, a.K, 1 << (a.bshift[0] + a.bshift[1] + a.bshift[2]));
    if (a.mode == LLR_FISTA) return f32 ? launch_one<float, LLR_FISTA>(a, L, stream) : launch_one<double, LLR_FISTA>(a, L, stream);
    return f32 ? launch_one<float, LLR_PLAIN>(a, L, stream) : launch_one<double, LLR_PLAIN>(a, L, stream);
}

hipError_t launch_llr_sum(const double* part, int64_t G, double* out, hipStream_t stream) {
    hipLaunchKernelGGL(llr_sum_kernel, dim3(1), dim3(kThreads), 0, stream, part, G, out);
    return hipGetLastError();
}

}  // namespace nufft
