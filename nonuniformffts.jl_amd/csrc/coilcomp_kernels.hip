// Coil compression and noise pre-whitening (coilcomp.h, coilcomp.cpp): C <= 64 vectors y_c of n complex elements
// become V <= C virtual coils through the principal components of the coil covariance.
//
//     R[c, c'] = Σ_j h_j y_c[j] conj(y_c'[j])  (FP64)      R~ = W R W^H      R~ = U Λ U^H  (jacobi.h, FP64)      A = U^H W
//     out_v[j] = Σ_c A[v, c] in_c[j]           (FP64, rounded once)
//
//   gram      flat over the n samples (FlatTiles and the Gram steps of hermitian.h): a workgroup takes `tpw` consecutive tiles of TC samples
//             x C coils into LDS, every entry i <= j of a tile is summed in sample order over S fixed segments, the segments are added in
//             segment order into the thread that owns the entry, tile after tile; a workgroup leaves C (C + 1) / 2 complex partials
//             with plain stores.  The weight is multiplied into y_i where the product is formed.
//   fold      one workgroup adds the partial sets in workgroup order and adds the sum to R.
//   congruence, eigen, compose   one workgroup each.  H and V of the Jacobi take 2 x 64 KiB of LDS at C = 64, so the two products
//             W R W^H and U^H W pass through global memory in launches of their own; without a noise covariance only eigen runs.
//   apply     a lane owns one 16-byte pack of samples, walks the coils in order and keeps up to 16 complex FP64 accumulators per
//             sample in registers; A[v, c] is the same for the whole wave and is read with scalar loads.
//
// No atomics, every sum in one fixed order: two runs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "coilcomp.h"
#include "hermitian.h"
#include "stream_kernels.h"

namespace nufft {
using namespace stream;

static_assert(kCcThreads == kThreads, "the grid rules of stream_kernels.h");
static_assert(kCcMaxCoils * (kCcMaxCoils + 1) / 2 <= kCcPairsPerThread * kCcThreads, "every Gram entry has an owner");

namespace {

using namespace jacobi_team;

template <typename T>
__global__ __launch_bounds__(kCcThreads) void cc_gram_kernel(CcGramLaunch a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int C = a.C, S = a.tl.S, np = C * (C + 1) / 2, tid = threadIdx.x;
    const FlatTiles ft(a.tl);
    const int TC = ft.TC, TCP = ft.TCP;
    Cx<T>* data = reinterpret_cast<Cx<T>*>(smem);
    double* wl = reinterpret_cast<double*>(smem + a.tl.off_w);
    Cd* gp = reinterpret_cast<Cd*>(smem + a.tl.off_gp);                           // [segment][entry]
    unsigned short* ij = reinterpret_cast<unsigned short*>(smem + a.tl.off_ij);   // [entry]: i << 8 | j
    for (int pr = tid; pr < np; pr += kCcThreads) {
        int i, j;
        pair_of(pr, C, i, j);
        ij[pr] = (unsigned short)(i << 8 | j);
    }
    Cd acc[kCcPairsPerThread];
#pragma unroll
    for (int m = 0; m < kCcPairsPerThread; ++m) acc[m] = Cd{0.0, 0.0};
    const T* h = static_cast<const T*>(a.weights);
    const int seg_len = TC / S;
    for (int64_t tile = ft.tile0; tile < ft.tile1; ++tile) {
        const int64_t s0 = ft.first_cell(tile);
        const int ns = ft.cells(tile, a.n);
        stage_padded<kCcThreads>(data, ft, C, s0, ns, [&](int c, int64_t at, bool) { return static_cast<const Cx<T>*>(a.y.p[c])[at]; });
        for (int v = tid; v < TC; v += kCcThreads) wl[v] = v < ns ? (h ? (double)h[s0 + v] : 1.0) : 0.0;
        __syncthreads();
        for (int u = tid; u < S * np; u += kCcThreads) {
            const int pr = u % np, seg = u / np;
            const int i = ij[pr] >> 8, j = ij[pr] & 255;
            // Σ h y_i conj(y_j): the conjugate is on the other factor than in M^H M
            gp[u] = gram_segment<true>(data + j * TCP + seg * seg_len, data + i * TCP + seg * seg_len, seg_len, wl + seg * seg_len);
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < kCcPairsPerThread; ++m) {
            const int pr = tid + m * kCcThreads;
            if (pr < np)
                for (int seg = 0; seg < S; ++seg) {
                    const Cd g = gp[seg * np + pr];
                    acc[m].re += g.re;
                    acc[m].im += g.im;
                }
        }
        // the next tile's loads overwrite `data` and `wl` only after every thread has passed the barrier above, and its `gp` only after
        // the barrier that follows those loads: no third barrier
    }
    Cd* out = reinterpret_cast<Cd*>(a.part) + (int64_t)blockIdx.x * np;
#pragma unroll
    for (int m = 0; m < kCcPairsPerThread; ++m) {
        const int pr = tid + m * kCcThreads;
        if (pr < np) out[pr] = acc[m];
    }
}

// One workgroup: R += Σ_g part[g], the partial sets in workgroup order; the diagonal stays real and R Hermitian.
__global__ __launch_bounds__(kCcThreads) void cc_fold_kernel(const double* part_, double* R_, int C, int G) {
    const int np = C * (C + 1) / 2;
    const Cd* part = reinterpret_cast<const Cd*>(part_);
    Cd* R = reinterpret_cast<Cd*>(R_);
    for (int pr = threadIdx.x; pr < np; pr += kCcThreads) {
        int i, j;
        pair_of(pr, C, i, j);
        const Cd sum = fold(part + pr, G, np), old = R[i * C + j];
        store_hermitian(R, C, i, j, Cd{sum.re + old.re, sum.im + old.im});
    }
}

// One workgroup: T = W R, then T <- T W^H on the upper triangle, mirrored.  Every sum in index order.
__global__ __launch_bounds__(kCcThreads) void cc_congruence_kernel(CcFinishLaunch a, double* scratch_) {
    const int C = a.C, tid = threadIdx.x;
    const Cd* R = reinterpret_cast<const Cd*>(a.R);
    const Cd* W = reinterpret_cast<const Cd*>(a.W);
    Cd* X = reinterpret_cast<Cd*>(scratch_);       // W R
    Cd* T = reinterpret_cast<Cd*>(a.T);
    for (int e = tid; e < C * C; e += kCcThreads) {
        const int i = e / C, j = e % C;
        double sr = 0.0, si = 0.0;
        for (int k = 0; k < C; ++k) {
            const Cd w = W[i * C + k], r = R[k * C + j];
            sr += w.re * r.re - w.im * r.im;
            si += w.re * r.im + w.im * r.re;
        }
        X[e] = Cd{sr, si};
    }
    __threadfence_block();
    __syncthreads();
    for (int e = tid; e < C * C; e += kCcThreads) {
        const int i = e / C, j = e % C;
        if (i > j) continue;
        double sr = 0.0, si = 0.0;
        for (int k = 0; k < C; ++k) {                                            // X[i, k] conj(W[j, k])
            const Cd x = X[i * C + k], w = W[j * C + k];
            sr += x.re * w.re + x.im * w.im;
            si += x.im * w.re - x.re * w.im;
        }
        if (i == j) {
            T[e] = Cd{sr, 0.0};
        } else {
            T[i * C + j] = Cd{sr, si};
            T[j * C + i] = Cd{sr, -si};
        }
    }
}

// One workgroup.  LDS: H, V (C x C complex double each), lam (C double), order (C int).  Row v of the output is the conjugate of the
// eigenvector of the v-th largest eigenvalue (ties: the lower index first), scaled back to unit length, its entry of largest modulus
// (the lowest index on a tie) real and positive.
__global__ __launch_bounds__(kCcThreads) void cc_eigen_kernel(CcFinishLaunch a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int C = a.C, tid = threadIdx.x;
    Cd* H = reinterpret_cast<Cd*>(smem);
    Cd* V = H + C * C;
    double* lam = reinterpret_cast<double*>(V + C * C);
    int* order = reinterpret_cast<int*>(lam + C);
    const Cd* src = reinterpret_cast<const Cd*>(a.whiten ? a.T : a.R);
    for (int e = tid; e < C * C; e += kCcThreads) {
        H[e] = src[e];
        V[e] = identity_entry(e / C, e % C);
    }
    __syncthreads();
    int sweeps = 0;
    if (C > 1 && tid < team_width(C)) sweeps = jacobi(H, V, C, tid);
    __syncthreads();
    // rank of every eigenvalue: the number of entries that come before it
    if (tid < C) {
        const double l = H[tid * C + tid].re;
        int before = 0;
        bool finite = l - l == 0.0;
        for (int k = 0; k < C; ++k) {
            const double o = H[k * C + k].re;
            if (o > l || (o == l && k < tid)) ++before;
        }
        if (!finite) before = C;                                                // decided below: a status, not an order
        lam[tid] = l;
        if (finite) order[before] = tid;
    }
    __syncthreads();
    if (tid == 0) {
        bool ok = true;
        for (int k = 0; k < C; ++k) ok = ok && lam[k] - lam[k] == 0.0;
        if (!ok)
            for (int k = 0; k < C; ++k) order[k] = k;
        a.words[0] = sweeps;
        a.words[1] = !ok ? 2 : (sweeps >= kSweepsMax ? 1 : 0);
    }
    __syncthreads();
    Cd* out = reinterpret_cast<Cd*>(a.whiten ? a.Uh : a.A);
    if (tid < C) {
        const int col = order[tid];
        a.lambda[tid] = lam[col];
        double nn = 0.0, big = -1.0;
        int at = 0;
        for (int c = 0; c < C; ++c) {
            const Cd v = V[c * C + col];
            const double m = v.re * v.re + v.im * v.im;
            nn += m;
            if (m > big) {
                big = m;
                at = c;
            }
        }
        const double back = 1.0 / sqrt(nn);
        const Cd p = V[at * C + col];
        const double ap = sqrt(p.re * p.re + p.im * p.im);
        double ur = 1.0, ui = 0.0;                                               // conj(p) / |p|
        if (ap > 0.0) {
            ur = p.re / ap;
            ui = -p.im / ap;
        }
        for (int c = 0; c < C; ++c) {
            Cd v = V[c * C + col];
            v = Cd{v.re * back, v.im * back};
            v = Cd{v.re * ur - v.im * ui, v.re * ui + v.im * ur};
            if (c == at) v.im = 0.0;
            out[tid * C + c] = Cd{v.re, -v.im};
        }
    }
}

// One workgroup: A = U^H W, every sum in index order.
__global__ __launch_bounds__(kCcThreads) void cc_compose_kernel(CcFinishLaunch a) {
    const int C = a.C;
    const Cd* Uh = reinterpret_cast<const Cd*>(a.Uh);
    const Cd* W = reinterpret_cast<const Cd*>(a.W);
    Cd* A = reinterpret_cast<Cd*>(a.A);
    for (int e = threadIdx.x; e < C * C; e += kCcThreads) {
        const int i = e / C, j = e % C;
        double sr = 0.0, si = 0.0;
        for (int k = 0; k < C; ++k) {
            const Cd u = Uh[i * C + k], w = W[k * C + j];
            sr += u.re * w.re - u.im * w.im;
            si += u.re * w.im + u.im * w.re;
        }
        A[e] = Cd{sr, si};
    }
}

// NS samples at element j0 of every vector: the coils in order, VC accumulators per sample.
template <typename T, int VC, int NS>
__device__ __forceinline__ void apply_at(const CcApplyLaunch& a, const Cd* __restrict__ A, int64_t j0) {
    struct alignas(NS * sizeof(Cx<T>)) Group {
        Cx<T> s[NS];
    };
    Cd acc[VC][NS];
#pragma unroll
    for (int v = 0; v < VC; ++v)
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[v][s] = Cd{0.0, 0.0};
    const int C = a.C;
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
        const Group x = *reinterpret_cast<const Group*>(static_cast<const Cx<T>*>(a.in.p[c]) + j0);
#pragma unroll
        for (int v = 0; v < VC; ++v) {
            const Cd m = A[v * C + c];                                            // wave-uniform
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const double xr = (double)x.s[s].re, xi = (double)x.s[s].im;
                acc[v][s].re += m.re * xr - m.im * xi;
                acc[v][s].im += m.re * xi + m.im * xr;
            }
        }
    }
#pragma unroll
    for (int v = 0; v < VC; ++v) {
        Group y;
#pragma unroll
        for (int s = 0; s < NS; ++s) y.s[s] = Cx<T>{(T)acc[v][s].re, (T)acc[v][s].im};
        if (v < a.V) *reinterpret_cast<Group*>(static_cast<Cx<T>*>(a.out[v]) + j0) = y;
    }
}

// A launch with V below its instantiation's VC also reads the rows V ... VC - 1 behind its own: A is followed by kCcApplyChunk rows of
// padding for that, and what those rows give is not stored.
template <typename T, int VC>
__global__ __launch_bounds__(kCcThreads) void cc_apply_kernel(CcApplyLaunch a, const double* __restrict__ A_rows) {
    constexpr int NS = 16 / (int)sizeof(Cx<T>);                                    // samples of a 16-byte pack
    const Cd* A = reinterpret_cast<const Cd*>(A_rows);
    const int64_t npacks = a.n / NS, step = (int64_t)gridDim.x * kCcThreads;
    for (int64_t i = (int64_t)blockIdx.x * kCcThreads + threadIdx.x; i < npacks; i += step) apply_at<T, VC, NS>(a, A, i * NS);
    if (NS > 1 && (a.n % NS) && blockIdx.x == 0 && threadIdx.x == 0) apply_at<T, VC, 1>(a, A, a.n - 1);   // the odd ComplexF32 element
}

template <typename T>
hipError_t launch_gram(const CcGramLaunch& a, hipStream_t stream) {
    hipLaunchKernelGGL((cc_gram_kernel<T>), dim3((unsigned)a.tl.G), dim3(kCcThreads), a.tl.bytes, stream, a);
    return hipGetLastError();
}

template <typename T, int VC>
hipError_t launch_apply_vc(const CcApplyLaunch& a, unsigned grid, hipStream_t stream) {
    hipLaunchKernelGGL((cc_apply_kernel<T, VC>), dim3(grid), dim3(kCcThreads), 0, stream, a, a.A);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_apply_t(const CcApplyLaunch& a, unsigned grid, hipStream_t stream) {
    if (a.V <= 1) return launch_apply_vc<T, 1>(a, grid, stream);
    if (a.V <= 2) return launch_apply_vc<T, 2>(a, grid, stream);
    if (a.V <= 4) return launch_apply_vc<T, 4>(a, grid, stream);
    if (a.V <= 8) return launch_apply_vc<T, 8>(a, grid, stream);
    return launch_apply_vc<T, 16>(a, grid, stream);
}

}  // namespace

CcTiling coilcomp_tiling(bool f32, int C, int64_t n) {
    CcTiling tl{};
    const size_t eb = f32 ? 8 : 16;
    const FlatTiling ft = flat_tiling(C, n, kCcTileBytes / (int)eb, kCcThreads, kCcMaxGroups);
    const int np = C * (C + 1) / 2;
    tl.TC = ft.TC;
    tl.S = ft.S;
    tl.tiles = ft.tiles;
    tl.tpw = ft.tpw;
    tl.G = ft.G;
    tl.off_w = up16((size_t)C * (tl.TC + 1) * eb);
    tl.off_gp = tl.off_w + (size_t)tl.TC * 8;
    tl.off_ij = tl.off_gp + (size_t)tl.S * np * 16;
    tl.bytes = up16(tl.off_ij + (size_t)np * 2);
    return tl;
}

size_t coilcomp_eigen_lds(int C) { return (size_t)C * C * 32 + (size_t)C * 8 + up16((size_t)C * 4); }

// Workgroups above 64 KiB of dynamic LDS must be allowed per kernel (and device): called when an object is created.
hipError_t coilcomp_allow_lds() {
    return allow_large_lds({reinterpret_cast<const void*>(&cc_eigen_kernel), reinterpret_cast<const void*>(&cc_gram_kernel<float>),
                            reinterpret_cast<const void*>(&cc_gram_kernel<double>)});
}

hipError_t launch_coilcomp_gram(const CcGramLaunch& a, hipStream_t stream) {
    hipError_t e = a.dtype == NUFFT_F32 ? launch_gram<float>(a, stream) : launch_gram<double>(a, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cc_fold_kernel, dim3(1), dim3(kCcThreads), 0, stream, a.part, a.R, a.C, a.tl.G);
    return hipGetLastError();
}

hipError_t launch_coilcomp_finish(const CcFinishLaunch& a, hipStream_t stream) {
    if (a.whiten) {
        // W R goes through the array A is written to afterwards
        hipLaunchKernelGGL(cc_congruence_kernel, dim3(1), dim3(kCcThreads), 0, stream, a, a.A);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(cc_eigen_kernel, dim3(1), dim3(kCcThreads), coilcomp_eigen_lds(a.C), stream, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (a.whiten) {
        hipLaunchKernelGGL(cc_compose_kernel, dim3(1), dim3(kCcThreads), 0, stream, a);
        return hipGetLastError();
    }
    return hipSuccess;
}

hipError_t launch_coilcomp_apply(const CcApplyLaunch& a, int num_cus, hipStream_t stream) {
    const bool f32 = a.dtype == NUFFT_F32;
    const unsigned grid = grid_for(std::max<int64_t>(1, a.n / (f32 ? 2 : 1)), num_cus);
    return f32 ? launch_apply_t<float>(a, grid, stream) : launch_apply_t<double>(a, grid, stream);
}

}  // namespace nufft
