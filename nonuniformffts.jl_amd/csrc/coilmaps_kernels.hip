// Coil sensitivity maps from low-resolution coil images (coilmaps.h, coilmaps.cpp): at every cell the dominant
// eigenvector of the C x C covariance of the coil values over a box around the cell (Walsh, Gmitro & Marcellin 2000).
//
//     R(x)[c, c'] = Σ_{x' ∈ box(x)} a_c(x') conj(a_c'(x'))  (FP64, periodic)      R = V Λ V^H  (jacobi.h)      v = column of the largest λ
//     s = Σ_c conj(p_c) v_c      v <- v conj(s) / |s|  (|s| > 0)      S_c(x) = v_c, rounded once;  0 where λ1 = 0
//
// The main kernel gives a workgroup a tile of output cells.  The coil values of the tile plus a halo of (b_d − 1) / 2 cells per side are
// staged in LDS ([coil][halo cell], in the element type); where not even a small tile fits with its halo, the neighbours are read from
// global memory instead.  A team of TW = 2^ceil(log2 C) lanes of one wave takes one cell at a time: lane r sums the entries
// (r, (r + j) mod C), j = 0 ... C / 2, of R over the box in registers -- k_3 outermost, k_1 innermost, an order that depends on the box
// alone -- and stores them and their mirror images into the team's H; V starts as the identity; jacobi.h diagonalises.  Lane r then
// holds v_r.  The teams of a workgroup never wait for each other inside the loop over the cells: H and V belong to one team, the lanes
// of a team take every branch together and the LDS serves a wave's accesses in order.  A workgroup leaves its largest λ1 and its
// largest sweep count with plain stores; a second kernel reduces them in one workgroup (a maximum does not depend on the order), and
// the crop pass, a streaming kernel, writes zeros where λ1 < crop² max λ1.  No atomics: two runs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "coilmaps.h"
#include "hermitian.h"
#include "stream_kernels.h"

namespace nufft {
using namespace stream;

namespace {

using namespace jacobi_team;

__device__ __forceinline__ int wrap(int v, int N) {
    v %= N;
    return v < 0 ? v + N : v;
}

// CT bounds the coils (C <= CT): lane r keeps CT / 2 + 1 complex sums in registers, indexed by constants only.
template <typename T, int CT>
__global__ __launch_bounds__(kCmMaxThreads) void coilmaps_kernel(CoilmapsLaunch a, CoilmapsLayout L) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int NJ = CT / 2 + 1;
    const int C = a.C, tid = threadIdx.x;
    const int team = tid / L.TW, r = tid % L.TW;
    const bool mine = r < C;
    const Cx<T>* stage = reinterpret_cast<const Cx<T>*>(smem);
    Cd* H = reinterpret_cast<Cd*>(smem + L.off_H) + team * C * C;
    Cd* V = reinterpret_cast<Cd*>(smem + L.off_V) + team * C * C;
    double* red = reinterpret_cast<double*>(smem + L.off_red);
    int* reds = reinterpret_cast<int*>(red + L.teams);

    const int64_t blk = blockIdx.x;
    const int o0 = (int)(blk % L.ntile[0]) * L.tile[0];
    const int o1 = (int)((blk / L.ntile[0]) % L.ntile[1]) * L.tile[1];
    const int o2 = (int)(blk / ((int64_t)L.ntile[0] * L.ntile[1])) * L.tile[2];
    const int h0 = (a.box[0] - 1) / 2, h1 = (a.box[1] - 1) / 2, h2 = (a.box[2] - 1) / 2;
    const int H0 = L.halo[0], H1 = L.halo[1];

    if (L.staged) {
        Cx<T>* st = reinterpret_cast<Cx<T>*>(smem);
        for (int u = tid; u < C * L.hcells; u += L.threads) {
            const int c = u / L.hcells, hc = u % L.hcells;
            const int i0 = wrap(o0 - h0 + hc % H0, a.N[0]);
            const int i1 = wrap(o1 - h1 + (hc / H0) % H1, a.N[1]);
            const int i2 = wrap(o2 - h2 + hc / (H0 * H1), a.N[2]);
            st[c * L.hpitch + hc] = static_cast<const Cx<T>*>(a.in[c])[i0 + i1 * a.pitch[1] + i2 * a.pitch[2]];
        }
        __syncthreads();
    }

    const int nj = C / 2 + 1;
    double top = 0.0;
    int most = 0;
    for (int cell = team; cell < L.tcells; cell += L.teams) {
        const int l0 = cell % L.tile[0], l1 = (cell / L.tile[0]) % L.tile[1], l2 = cell / (L.tile[0] * L.tile[1]);
        const int x0 = o0 + l0, x1 = o1 + l1, x2 = o2 + l2;
        if (x0 >= a.N[0] || x1 >= a.N[1] || x2 >= a.N[2]) continue;         // the last tile of a dimension may reach beyond the array
        const int64_t at = x0 + x1 * a.pitch[1] + x2 * a.pitch[2];

        Cd acc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = Cd{0.0, 0.0};
        if (mine) {
            for (int k2 = 0; k2 < a.box[2]; ++k2)
                for (int k1 = 0; k1 < a.box[1]; ++k1)
                    for (int k0 = 0; k0 < a.box[0]; ++k0) {
                        int64_t nb;
                        if (L.staged) {
                            nb = (l0 + k0) + (l1 + k1) * H0 + (l2 + k2) * H0 * H1;
                        } else {
                            nb = wrap(x0 - h0 + k0, a.N[0]) + wrap(x1 - h1 + k1, a.N[1]) * a.pitch[1] + wrap(x2 - h2 + k2, a.N[2]) * a.pitch[2];
                        }
                        auto value = [&](int c) {
                            return L.staged ? stage[c * L.hpitch + nb] : static_cast<const Cx<T>*>(a.in[c])[nb];
                        };
                        const Cx<T> me = value(r);
                        const double ar = (double)me.re, ai = (double)me.im;
                        acc[0].re += ar * ar + ai * ai;
                        int col = r;
#pragma unroll
                        for (int j = 1; j < NJ; ++j) {
                            if (j < nj) {
                                col = col + 1 == C ? 0 : col + 1;
                                const Cx<T> o = value(col);
                                const double br = (double)o.re, bi = (double)o.im;
                                acc[j].re += ar * br + ai * bi;
                                acc[j].im += ai * br - ar * bi;
                            }
                        }
                    }
            H[r * C + r] = Cd{acc[0].re, 0.0};
            int col = r;
#pragma unroll
            for (int j = 1; j < NJ; ++j) {
                if (j < nj) {
                    col = col + 1 == C ? 0 : col + 1;
                    // an even C reaches the pairs (r, r + C / 2) from both ends: the lower lane's sum is the one that is kept
                    if (!(2 * j == C && r >= j)) {
                        H[r * C + col] = acc[j];
                        H[col * C + r] = Cd{acc[j].re, -acc[j].im};
                    }
                }
            }
            for (int c = 0; c < C; ++c) V[r * C + c] = identity_entry(r, c);
        }
        team_sync();
        int sweeps = 0;
        if (C > 1) sweeps = jacobi(H, V, C, r);

        // the largest and the second largest eigenvalue, the first index on a tie; every lane of the team finds the same
        int i1 = 0;
        double lam1 = H[0].re;
        for (int i = 1; i < C; ++i) {
            const double l = H[i * C + i].re;
            if (l > lam1) {
                lam1 = l;
                i1 = i;
            }
        }
        double lam2 = 0.0;
        bool any = false;
        for (int i = 0; i < C; ++i) {
            if (i == i1) continue;
            const double l = H[i * C + i].re;
            if (!any || l > lam2) lam2 = l;
            any = true;
        }
        // s = Σ_c conj(p_c) v_c and ‖v‖², in coil order.  A column of V has left unit length by a few ε per rotation: it is scaled back
        // (s keeps its direction, which is all that is used of it)
        double sr = 0.0, si = 0.0, nn = 0.0;
        for (int c = 0; c < C; ++c) {
            const Cd v = V[c * C + i1];
            const double pr = a.p[2 * c], pi = a.p[2 * c + 1];
            sr += pr * v.re + pi * v.im;
            si += pr * v.im - pi * v.re;
            nn += v.re * v.re + v.im * v.im;
        }
        if (mine) {
            Cd v = V[r * C + i1];
            const double back = 1.0 / sqrt(nn);
            v = Cd{v.re * back, v.im * back};
            const double as = sqrt(sr * sr + si * si);
            if (as > 0.0) {
                const double ur = sr / as, ui = -si / as;
                v = Cd{v.re * ur - v.im * ui, v.re * ui + v.im * ur};
            }
            if (!(lam1 > 0.0)) v = Cd{0.0, 0.0};
            static_cast<Cx<T>*>(a.out[r])[at] = Cx<T>{(T)v.re, (T)v.im};
        }
        if (r == 0) {
            if (a.lambda1) static_cast<T*>(a.lambda1)[at] = (T)lam1;
            if (a.lambda2) static_cast<T*>(a.lambda2)[at] = (T)lam2;
            top = fmax(top, (double)(T)lam1);                                // of λ1 as the crop pass reads it: rounded to the element type
            most = max(most, sweeps);
        }
        team_sync();                                                         // the next cell overwrites H and V
    }
    if (r == 0) {
        red[team] = top;
        reds[team] = most;
    }
    __syncthreads();
    if (tid == 0) {
        for (int t = 1; t < L.teams; ++t) {
            top = fmax(top, red[t]);
            most = max(most, reds[t]);
        }
        a.part[blk] = top;
        a.sweeps_part[blk] = most;
    }
}

// One workgroup: the maxima of the per-workgroup partials.
__global__ __launch_bounds__(kThreads) void coilmaps_max_kernel(const double* part, const int32_t* sweeps_part, int64_t G, double* words) {
    __shared__ double lds[kWaves];
    double v = 0.0, s = 0.0;
    for (int64_t g = threadIdx.x; g < G; g += kThreads) {
        v = fmax(v, part[g]);
        s = fmax(s, (double)sweeps_part[g]);
    }
    v = block_reduce<Max>(v, lds);
    s = block_reduce<Max>(s, lds);
    if (threadIdx.x == 0) {
        words[0] = v;
        reinterpret_cast<int32_t*>(words)[2] = (int32_t)s;
    }
}

struct CropTable {
    void* out[kCmMaxCoils];
};

// Zeros where λ1 < crop² max λ1: over the n complex elements in 16-byte packs (one ComplexF64, two ComplexF32); the ComplexF32 element
// behind the last pack of an odd n is left to one thread.  Reads λ1, writes only the cells it zeroes.
template <typename T>
__global__ __launch_bounds__(kThreads) void coilmaps_crop_kernel(CropTable tab, int C, const T* lambda1, const double* words, double crop2, int64_t n) {
    constexpr int CW = Pack<T>::W / 2;          // elements per pack
    const double thr = crop2 * words[0];
    Pack<T> zero;
#pragma unroll
    for (int w = 0; w < 2 * CW; ++w) zero.v[w] = T(0);
    NUFFT_FOR_EACH_PACK(T, 2 * n, i) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int64_t q = i + t * step__;
            if (q >= npacks__) break;
            bool cut[CW], all = true, some = false;
#pragma unroll
            for (int w = 0; w < CW; ++w) {
                cut[w] = (double)lambda1[q * CW + w] < thr;
                all = all && cut[w];
                some = some || cut[w];
            }
            if (!some) continue;
            for (int c = 0; c < C; ++c) {
                T* o = static_cast<T*>(tab.out[c]);
                if (all) {
                    store(o, q, zero);
                } else {
#pragma unroll
                    for (int w = 0; w < CW; ++w)
                        if (cut[w]) reinterpret_cast<Cx<T>*>(o)[q * CW + w] = Cx<T>{T(0), T(0)};
                }
            }
        }
    }
    if (CW > 1 && (n & 1) && blockIdx.x == 0 && threadIdx.x == 0 && (double)lambda1[n - 1] < thr)
        for (int c = 0; c < C; ++c) reinterpret_cast<Cx<T>*>(tab.out[c])[n - 1] = Cx<T>{T(0), T(0)};
}

template <typename T, int CT>
hipError_t launch_one(const CoilmapsLaunch& a, const CoilmapsLayout& L, hipStream_t stream) {
    hipLaunchKernelGGL((coilmaps_kernel<T, CT>), dim3((unsigned)L.G), dim3(L.threads), L.bytes, stream, a, L);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_typed(const CoilmapsLaunch& a, const CoilmapsLayout& L, hipStream_t stream) {
    if (a.C <= 4) return launch_one<T, 4>(a, L, stream);
    if (a.C <= 8) return launch_one<T, 8>(a, L, stream);
    if (a.C <= 16) return launch_one<T, 16>(a, L, stream);
    return launch_one<T, 32>(a, L, stream);
}

template <typename T, int CT>
const void* kernel_of() {
    return reinterpret_cast<const void*>(&coilmaps_kernel<T, CT>);
}

}  // namespace

CoilmapsLayout coilmaps_layout(bool f32, int C, int D, const int* box, const int64_t* N) {
    CoilmapsLayout L{};
    const size_t eb = f32 ? 8 : 16;
    const bool wide = C > 16;
    L.TW = team_width(C);
    L.teams = kCmMaxThreads / L.TW;
    while (L.teams > 1 && (size_t)L.teams * C * C * 32 > (size_t)(wide ? kCmMatrixBytesWide : kCmMatrixBytes)) L.teams /= 2;
    while (L.teams * L.TW < 64) L.teams *= 2;                          // whole waves (C = 1 ... : more teams cost C * C * 32 bytes each)
    L.threads = L.teams * L.TW;
    const int first[3] = {D == 1 ? 64 : 16, D == 1 ? 1 : 8, D == 3 ? 4 : 1};
    int b[3];
    for (int d = 0; d < 3; ++d) {
        b[d] = d < D ? box[d] : 1;
        L.tile[d] = d < D ? (int)std::min<int64_t>(first[d], N[d]) : 1;
    }
    const size_t budget = wide ? kCmStageBytesWide : kCmStageBytes;
    auto staged_bytes = [&](const int* t) {
        const size_t hc = (size_t)(t[0] + b[0] - 1) * (t[1] + b[1] - 1) * (t[2] + b[2] - 1);
        return (size_t)C * (hc | 1) * eb;
    };
    int t[3] = {L.tile[0], L.tile[1], L.tile[2]};
    while (staged_bytes(t) > budget && t[0] * t[1] * t[2] > 1) {
        int d = 2;                                                      // halve the longest side, the slowest dimension on a tie
        if (t[1] > t[d]) d = 1;
        if (t[0] > t[d]) d = 0;
        t[d] = (t[d] + 1) / 2;
    }
    // a tile cut down to fewer cells than the workgroup has teams would leave teams idle: then nothing is staged
    L.staged = staged_bytes(t) <= budget && t[0] * t[1] * t[2] >= std::min(L.teams, L.tile[0] * L.tile[1] * L.tile[2]);
    if (L.staged)
        for (int d = 0; d < 3; ++d) L.tile[d] = t[d];
    // a small array in large tiles leaves compute units idle while a team walks through its cells one after the other: smaller tiles
    // (never fewer cells than teams) until there are kCmWantGroups workgroups
    auto groups = [&]() {
        int64_t g = 1;
        for (int d = 0; d < D; ++d) g *= (N[d] + L.tile[d] - 1) / L.tile[d];
        return g;
    };
    while (groups() < kCmWantGroups) {
        int d = 2;
        if (L.tile[1] > L.tile[d]) d = 1;
        if (L.tile[0] > L.tile[d]) d = 0;
        const int half = (L.tile[d] + 1) / 2;
        if (L.tile[d] == 1 || L.tile[0] * L.tile[1] * L.tile[2] / L.tile[d] * half < L.teams) break;
        L.tile[d] = half;
    }
    L.tcells = L.tile[0] * L.tile[1] * L.tile[2];
    L.G = 1;
    for (int d = 0; d < 3; ++d) {
        L.halo[d] = L.tile[d] + b[d] - 1;
        L.ntile[d] = d < D ? (int)((N[d] + L.tile[d] - 1) / L.tile[d]) : 1;
        L.G *= L.ntile[d];
    }
    L.hcells = L.halo[0] * L.halo[1] * L.halo[2];
    L.hpitch = L.hcells | 1;
    L.off_H = L.staged ? up16((size_t)C * L.hpitch * eb) : 0;
    L.off_V = L.off_H + (size_t)L.teams * C * C * 16;
    L.off_red = L.off_V + (size_t)L.teams * C * C * 16;
    L.bytes = up16(L.off_red + (size_t)L.teams * 12);
    return L;
}

hipError_t coilmaps_allow_lds() {
    return allow_large_lds({kernel_of<float, 4>(), kernel_of<float, 8>(), kernel_of<float, 16>(), kernel_of<float, 32>(),
                            kernel_of<double, 4>(), kernel_of<double, 8>(), kernel_of<double, 16>(), kernel_of<double, 32>()});
}

hipError_t launch_coilmaps(const CoilmapsLaunch& a, const CoilmapsLayout& L, hipStream_t stream) {
    return a.dtype == NUFFT_F32 ? launch_typed<float>(a, L, stream) : launch_typed<double>(a, L, stream);
}

hipError_t launch_coilmaps_max(const CoilmapsLaunch& a, int64_t G, hipStream_t stream) {
    hipLaunchKernelGGL(coilmaps_max_kernel, dim3(1), dim3(kThreads), 0, stream, a.part, a.sweeps_part, G, a.words);
    return hipGetLastError();
}

hipError_t launch_coilmaps_crop(const CoilmapsLaunch& a, int num_cus, hipStream_t stream) {
    CropTable tab{};
    for (int c = 0; c < a.C; ++c) tab.out[c] = a.out[c];
    const int64_t np = a.n / (a.dtype == NUFFT_F32 ? 2 : 1);
    return launch_by_dtype(a.dtype, dim3(stream_workgroups(np, num_cus)), dim3(kThreads), stream, coilmaps_crop_kernel<float>, coilmaps_crop_kernel<double>, tab,
                           a.C, a.lambda1, a.words, a.crop2, a.n);
}

}  // namespace nufft
