// Dimension 1 of the Toeplitz normal operator's fused apply for K coupled components (toeplitz.cpp): the
// sibling of toeplitz_lines_kernel (fft_lines.hip) for the K × K block operator of a subspace model,
//   (G_Φ û)_a = Σ_b Toeplitz(T_ab) û_b,      K_ab = backwardDFT_2N(T_ab) / Π 2N_d,      K_ba = conj(K_ab),  K_aa real.
// One wave owns the K lines of a line id, one per component, all in LDS: zero-padded backward FFTs, the block multiply per cell,
// forward FFTs, kept modes stored back.  The padded lines never leave LDS; every multiplier line is read once, in 16-byte loads.
//
// Conjugation bookkeeping.  As in toeplitz_lines_kernel one twiddle table (the forward one) serves both transforms: the kept modes are
// conjugated while they are loaded, so the first forward FFT F leaves  l_b = F conj(x_b) = conj(B x_b)  (B the backward transform).
// There K is real and K ⊙ conj(l) is formed in one step.  Here the multiplier is complex, so the value is un-conjugated FIRST,
//   v_b = conj(l_b) = B x_b,
// and the block row is applied to it as it stands:
//   y_a = K_aa v_a + Σ_{b > a} K_ab v_b + Σ_{b < a} conj(K_ba) v_b         (K_ba, b < a: the stored pair (b, a)),
// no conjugate is left on y_a, and the second forward FFT gives F y_a = (G_Φ û)_a along this dimension.
#include <hip/hip_runtime.h>

#include <atomic>

#include "fft_line.h"
#include "kernels.h"
#include "toeplitz.h"

namespace nufft {
namespace {

struct CoupledLineArgs {
    void* data;             // K arrays complex<T>[nlines][k1], data_stride complex elements apart
    int64_t data_stride;
    const void* kd;         // T[K][nlines * N]: the diagonal blocks
    const void* kc;         // complex<T>[K (K − 1) / 2][nlines * N]: the pairs a < b, row-major
    int64_t nlines;
    int K;
    int k1;
    const int32_t* map;     // [k1]: kept mode -> index of the line
    const void* twiddle;    // complex<T>[N]: exp(-2πi m / N)
};

// Waves per workgroup for K <= KT lines of N elements of `csize` bytes per wave, from {16, 8, 4, 2, 1}: the most that leave room for
// two workgroups per CU while a workgroup still has four waves, else the most that fit at all; 0: not even one wave fits.
constexpr int coupled_waves(size_t csize, int n, int kt) {
    const size_t line = (size_t)(n + (n >> 4) + 1);
    for (int tl = 16; tl >= 4; tl >>= 1)
        if (csize * ((size_t)n + (size_t)tl * kt * line) <= 80 * 1024) return tl;
    for (int tl = 16; tl >= 1; tl >>= 1)
        if (csize * ((size_t)n + (size_t)tl * kt * line) <= kFftLdsLimit) return tl;
    return 0;
}
constexpr int coupled_tier(int K) { return K <= 2 ? 2 : (K <= 4 ? 4 : (K <= 8 ? 8 : 16)); }

// KT: the tier (the compile-time bound of the run-time K: the register arrays of the multiply are sized by it)
template <typename T, int N, int KT, int TL>
__global__ __launch_bounds__(TL * kWave) void toeplitz_lines_coupled_kernel(CoupledLineArgs a) {
    using C = typename Cplx2<T>::type;
    constexpr int LINE = N + (N >> 4) + 1;
    constexpr int PW = 16 / sizeof(T);                        // cells per 16-byte load of a real line (half as many of a complex one)
    constexpr int NQ = N / PW;
    // the diagonal lines of a lane's first cells are fetched before the first transforms where that takes at most 16 registers: they
    // are then in flight under the K backward FFTs (the off-diagonal lines, up to 480 registers' worth, are read where they are used)
    constexpr bool PREFETCH = KT <= 4 && NQ >= kWave;
    struct alignas(16) KPack { T v[PW]; };
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    C* tw = reinterpret_cast<C*>(smem);                       // [N]
    C* lines = tw + N;                                        // [TL][K][LINE]
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid / kWave;
    const int K = a.K;
    const C* twg = static_cast<const C*>(a.twiddle);
    for (int i = tid; i < N; i += TL * kWave) tw[i] = twg[i];
    __syncthreads();
    const int64_t line_id = (int64_t)blockIdx.x * TL + wave;
    if (line_id >= a.nlines) return;
    C* mine = lines + (size_t)wave * K * LINE;
    const int64_t cells = a.nlines * N;
    const T* kd = static_cast<const T*>(a.kd) + line_id * N;
    const T* kc = static_cast<const T*>(a.kc) + 2 * line_id * N;

    C z; z.x = T(0); z.y = T(0);
    for (int e = lane; e < K * LINE; e += kWave) mine[e] = z;
    wave_lds_fence();
    for (int b = 0; b < K; ++b) {
        C* line = mine + b * LINE;
        const C* x = static_cast<const C*>(a.data) + (int64_t)b * a.data_stride + line_id * a.k1;
        if (sizeof(C) == 8 && (a.k1 & 1) == 0) {              // Float32: two kept modes (16 bytes) per lane and step
            const float4* x4 = reinterpret_cast<const float4*>(x);
            for (int k = lane; k < a.k1 / 2; k += kWave) {
                const float4 w = x4[k];
                C u, v;
                u.x = w.x; u.y = -w.y; v.x = w.z; v.y = -w.w;
                line[lpad(a.map[2 * k])] = u;
                line[lpad(a.map[2 * k + 1])] = v;
            }
        } else {
            for (int k = lane; k < a.k1; k += kWave) {
                C u = x[k];
                u.y = -u.y;
                line[lpad(a.map[k])] = u;
            }
        }
    }
    [[maybe_unused]] KPack dpre[PREFETCH ? KT : 1];
    if constexpr (PREFETCH) {
#pragma unroll
        for (int c = 0; c < KT; ++c)
            if (c < K) dpre[c] = *reinterpret_cast<const KPack*>(kd + (int64_t)c * cells + lane * PW);
    }
    wave_lds_fence();
    for (int b = 0; b < K; ++b) fft_line<T, N, -1>(mine + b * LINE, tw, lane);

    for (int q = lane; q < NQ; q += kWave) {
        const int m0 = q * PW;
        C acc[KT][PW];
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            if (c < K) {
                KPack d;
                if constexpr (PREFETCH) {
                    if (q == lane) d = dpre[c];
                    else d = *reinterpret_cast<const KPack*>(kd + (int64_t)c * cells + m0);
                } else {
                    d = *reinterpret_cast<const KPack*>(kd + (int64_t)c * cells + m0);
                }
#pragma unroll
                for (int t = 0; t < PW; ++t) {
                    const C l = mine[c * LINE + lpad(m0 + t)];      // v = conj(l)
                    acc[c][t].x = d.v[t] * l.x;
                    acc[c][t].y = -d.v[t] * l.y;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < KT; ++c) {
#pragma unroll
            for (int b = c + 1; b < KT; ++b) {
                if (b < K) {
                    const T* kp = kc + 2 * ((int64_t)(c * (K - 1) - c * (c - 1) / 2 + (b - c - 1)) * cells + m0);
                    const KPack k0 = *reinterpret_cast<const KPack*>(kp), k1 = *reinterpret_cast<const KPack*>(kp + PW);
#pragma unroll
                    for (int t = 0; t < PW; ++t) {
                        const T kr = 2 * t < PW ? k0.v[(2 * t) % PW] : k1.v[(2 * t) % PW];
                        const T ki = 2 * t < PW ? k0.v[(2 * t + 1) % PW] : k1.v[(2 * t + 1) % PW];
                        const C lc = mine[c * LINE + lpad(m0 + t)], lb = mine[b * LINE + lpad(m0 + t)];
                        // y_c += K_cb v_b,  v_b = conj(l_b) = (lb.x, −lb.y)
                        acc[c][t].x += kr * lb.x + ki * lb.y;
                        acc[c][t].y += ki * lb.x - kr * lb.y;
                        // y_b += conj(K_cb) v_c,  v_c = (lc.x, −lc.y)
                        acc[b][t].x += kr * lc.x - ki * lc.y;
                        acc[b][t].y += -kr * lc.y - ki * lc.x;
                    }
                }
            }
        }
        // (a lane reads and writes its own cells only: no other lane's read can see these stores)
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            if (c < K) {
#pragma unroll
                for (int t = 0; t < PW; ++t) mine[c * LINE + lpad(m0 + t)] = acc[c][t];
            }
        }
    }
    wave_lds_fence();
    for (int b = 0; b < K; ++b) fft_line<T, N, -1>(mine + b * LINE, tw, lane);

    for (int b = 0; b < K; ++b) {
        const C* line = mine + b * LINE;
        C* x = static_cast<C*>(a.data) + (int64_t)b * a.data_stride + line_id * a.k1;
        if (sizeof(C) == 8 && (a.k1 & 1) == 0) {
            float4* x4 = reinterpret_cast<float4*>(x);
            for (int k = lane; k < a.k1 / 2; k += kWave) {
                const C u = line[lpad(a.map[2 * k])], v = line[lpad(a.map[2 * k + 1])];
                x4[k] = make_float4((float)u.x, (float)u.y, (float)v.x, (float)v.y);
            }
        } else {
            for (int k = lane; k < a.k1; k += kWave) x[k] = line[lpad(a.map[k])];
        }
    }
}

template <typename T, int N, int KT>
hipError_t launch_coupled_n_k(const CoupledLineArgs& a, hipStream_t stream) {
    using C = typename Cplx2<T>::type;
    constexpr int TL = coupled_waves(sizeof(C), N, KT);
    if constexpr (TL == 0) {
        return hipErrorInvalidValue;
    } else {
        constexpr int LINE = N + (N >> 4) + 1;
        static_assert(sizeof(C) * ((size_t)N + (size_t)TL * KT * LINE) <= kFftLdsLimit, "line buffers exceed the 160 KiB of LDS");
        const size_t lds = sizeof(C) * ((size_t)N + (size_t)TL * a.K * LINE);
        auto fn = toeplitz_lines_coupled_kernel<T, N, KT, TL>;
        // the attribute is per device: remember which devices of this process have it
        static std::atomic<unsigned long long> prepared{0};
        int dev = 0;
        (void)hipGetDevice(&dev);
        const unsigned long long bit = 1ull << (dev & 63);
        if (!(prepared.load(std::memory_order_relaxed) & bit)) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(sizeof(C) * ((size_t)N + (size_t)TL * KT * LINE)));
            if (e != hipSuccess) return e;
            prepared.fetch_or(bit, std::memory_order_relaxed);
        }
        hipLaunchKernelGGL(fn, dim3((unsigned)((a.nlines + TL - 1) / TL)), dim3(TL * kWave), lds, stream, a);
        return hipGetLastError();
    }
}

template <typename T, int N>
hipError_t launch_coupled_n(const CoupledLineArgs& a, hipStream_t stream) {
    switch (coupled_tier(a.K)) {
        case 2: return launch_coupled_n_k<T, N, 2>(a, stream);
        case 4: return launch_coupled_n_k<T, N, 4>(a, stream);
        case 8: return launch_coupled_n_k<T, N, 8>(a, stream);
        default: return launch_coupled_n_k<T, N, 16>(a, stream);
    }
}

// the line length: the I-th entry of kFftLineSizes (fft_line.h)
template <typename T, int I = 0>
hipError_t launch_coupled_t(int n, const CoupledLineArgs& a, hipStream_t stream) {
    if constexpr (I == kNumFftLineSizes) {
        return hipErrorInvalidValue;
    } else {
        if (n == kFftLineSizes[I]) return launch_coupled_n<T, kFftLineSizes[I]>(a, stream);
        return launch_coupled_t<T, I + 1>(n, a, stream);
    }
}

}  // namespace

bool toeplitz_lines_coupled_supported(int dtype, int64_t n, int K) {
    if (K < 1 || K > kMaxCoupled || !toeplitz_lines_supported(dtype, n)) return false;
    return coupled_waves(dtype == NUFFT_F32 ? 8 : 16, (int)n, coupled_tier(K)) > 0;
}

hipError_t launch_toeplitz_lines_coupled(int dtype, int64_t n, int K, void* data, int64_t data_stride, const void* kd, const void* kc,
                                         int64_t nlines, int k1, const int32_t* map, const void* twiddle, hipStream_t stream) {
    if (nlines <= 0) return hipSuccess;
    if (k1 < 1 || k1 > n || !toeplitz_lines_coupled_supported(dtype, n, K)) return hipErrorInvalidValue;
    CoupledLineArgs a{};
    a.data = data; a.data_stride = data_stride; a.kd = kd; a.kc = kc; a.nlines = nlines; a.K = K; a.k1 = k1; a.map = map; a.twiddle = twiddle;
    return dtype == NUFFT_F32 ? launch_coupled_t<float>((int)n, a, stream) : launch_coupled_t<double>((int)n, a, stream);
}

}  // namespace nufft
