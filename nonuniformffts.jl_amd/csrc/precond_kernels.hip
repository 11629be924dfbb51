// Kernels of the circulant preconditioner of the Toeplitz normal operator (precond.cpp).
//
// Build (once per spectrum): the fold of the operator's generating sequence T on the 2N grid into the first column c of T. Chan's
// optimal circulant (Fejér weights), the real part of its transform with the partial maxima, and the inverse m.  Apply: the streaming
// multiply of the dense path, and precond_lines_kernel, dimension 1 of the fused path.  The streaming kernels follow stream_kernels.h
// (16-byte packs, grid sized to the device, per-workgroup partials reduced later in a fixed order: no atomics).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "fft_line.h"
#include "kernels.h"
#include "precond.h"
#include "stream_kernels.h"

namespace nufft {
namespace {

namespace st = stream;
using st::Pack;

// grid = K + 0 i: one real in, one complex cell out per thread and step (build only)
template <typename T>
__global__ __launch_bounds__(st::kThreads) void pc_embed_kernel(T* grid, const T* K, int64_t cells) {
    typedef T T2 __attribute__((ext_vector_type(2)));
    for (int64_t i = (int64_t)blockIdx.x * st::kThreads + threadIdx.x; i < cells; i += (int64_t)gridDim.x * st::kThreads) {
        T2 v;
        v.x = K[i];
        v.y = T(0);
        reinterpret_cast<T2*>(grid)[i] = v;
    }
}

// One cell of c per thread and step: up to 2^D cells of T, each with the product of its Fejér weights.  A weight of zero (j_d = 0 with
// s_d = 1: the Nyquist plane j_d + N_d = N_d of T) skips the read.
template <typename T>
__global__ __launch_bounds__(st::kThreads) void pc_fold_kernel(PcGrid g, T* c, const T* Tg, int64_t n) {
    typedef T T2 __attribute__((ext_vector_type(2)));
    for (int64_t i = (int64_t)blockIdx.x * st::kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * st::kThreads) {
        int j[3];
        j[0] = (int)(i % g.n[0]);
        const int64_t r = i / g.n[0];
        j[1] = (int)(r % g.n[1]);
        j[2] = (int)(r / g.n[1]);
        double re = 0.0, im = 0.0;
        for (int s = 0; s < (1 << g.D); ++s) {
            double w = 1.0;
            int64_t cell = 0, pitch = 1;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                if (d < g.D) {
                    const int sd = (s >> d) & 1;
                    w *= sd ? (double)j[d] / (double)g.n[d] : (double)(g.n[d] - j[d]) / (double)g.n[d];
                    cell += pitch * (j[d] + sd * g.n[d]);          // (j − s N) mod 2N = j + s N for 0 <= j < N
                    pitch *= 2 * (int64_t)g.n[d];
                }
            }
            if (w != 0.0) {
                const T2 t = reinterpret_cast<const T2*>(Tg)[cell];
                re += w * (double)t.x;
                im += w * (double)t.y;
            }
        }
        T2 v;
        v.x = (T)re;
        v.y = (T)im;
        reinterpret_cast<T2*>(c)[i] = v;
    }
}

// e = Re(c); per workgroup the maxima of e and of −e
template <typename T>
__global__ __launch_bounds__(st::kThreads) void pc_eigen_kernel(T* e, const T* c, int64_t n, double* part) {
    __shared__ double lds[st::kWaves];
    double hi = -INFINITY, lo = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * st::kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * st::kThreads) {
        const T v = c[2 * i];
        e[i] = v;
        hi = fmax(hi, (double)v);
        lo = fmax(lo, -(double)v);
    }
    hi = st::block_reduce<st::Max>(hi, lds);
    lo = st::block_reduce<st::Max>(lo, lds);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = hi;
        part[2 * blockIdx.x + 1] = lo;
    }
}

template <typename T>
__global__ __launch_bounds__(st::kThreads) void pc_invert_kernel(T* m, int64_t n, double mu, double thresh, double count) {
    for (int64_t i = (int64_t)blockIdx.x * st::kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * st::kThreads)
        m[i] = (T)(1.0 / (count * fmax((double)m[i] + mu, thresh)));
}

// out = f ⊙ in over 16-byte packs of complex elements (one ComplexF64 or two ComplexF32); the element behind the last whole pack (an
// odd count of ComplexF32) goes to one thread
template <typename T, bool SCALE>
__global__ __launch_bounds__(st::kThreads) void pc_scale_kernel(T* out, const T* in, const T* f, int64_t n) {
    constexpr int CW = Pack<T>::W / 2;
    const int64_t npacks = n / CW;
    for (int64_t q = (int64_t)blockIdx.x * st::kThreads + threadIdx.x; q < npacks; q += (int64_t)gridDim.x * st::kThreads) {
        Pack<T> pk = st::load(in, q);
        if constexpr (SCALE) {
#pragma unroll
            for (int w = 0; w < CW; ++w) {
                const T s = f[q * CW + w];
                pk.v[2 * w] *= s;
                pk.v[2 * w + 1] *= s;
            }
        }
        st::store(out, q, pk);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = npacks * CW; i < n; ++i) {
            const T s = SCALE ? f[i] : T(1);
            const T re = in[2 * i], im = in[2 * i + 1];
            out[2 * i] = s * re;
            out[2 * i + 1] = s * im;
        }
}

// s = Σ_c |S_c|² in coil order; per workgroup the maximum and the sum of s
constexpr int kPcCoils = 64;
struct PcCoilTable {
    const void* maps[kPcCoils];
};
template <typename T>
__global__ __launch_bounds__(st::kThreads) void pc_coil_power_kernel(T* s, PcCoilTable tab, int ncoils, int accumulate, int last, int64_t n, double* part) {
    __shared__ double lds[st::kWaves];
    typedef T T2 __attribute__((ext_vector_type(2)));
    double hi = 0.0, sum = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * st::kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * st::kThreads) {
        T acc = accumulate ? s[i] : T(0);
        for (int c = 0; c < ncoils; ++c) {
            const T2 v = static_cast<const T2*>(tab.maps[c])[i];
            acc += v.x * v.x + v.y * v.y;
        }
        s[i] = acc;
        hi = fmax(hi, (double)acc);
        sum += (double)acc;
    }
    if (!last) return;
    hi = st::block_reduce<st::Max>(hi, lds);
    sum = st::block_reduce<st::Sum>(sum, lds);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = hi;
        part[2 * blockIdx.x + 1] = sum;
    }
}

template <typename T>
__global__ __launch_bounds__(st::kThreads) void pc_coil_scaling_kernel(T* d, int64_t n, double floor) {
    for (int64_t i = (int64_t)blockIdx.x * st::kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * st::kThreads)
        d[i] = (T)(1.0 / sqrt(fmax((double)d[i], floor)));
}

// ---------------------------------------------------------------------------------------------------
// Dimension 1 of the fused apply, in place: one wave per contiguous line of N cells, which never leaves LDS between the load and the
// store.  The strided passes before this kernel are BACKWARD transforms (their load side carries the scaling d), so the apply is
//     F ( m~ ⊙ B x ),   m~[q] = m[(−q) mod N]   which equals   B ( m ⊙ F x )   (F B = n I and F = B P with P the negation of the index),
// and this kernel runs B, the multiply and F along dimension 1.  One twiddle table (the forward one) serves both, by the conjugation of
// toeplitz_lines_kernel (fft_lines.hip): the line is conjugated while it is loaded, the forward FFT then leaves conj(B x), and the
// multiply writes m~ ⊙ conj(·) = m~ ⊙ B x (m is real).  The negated frequencies are taken where m is read: the wave of line (j_2, j_3)
// reads the line (−j_2, −j_3) of m, and the entry i of that line multiplies the cell (N − i) mod N.
// ---------------------------------------------------------------------------------------------------
struct PrecondLineArgs {
    void* data;             // complex<T>[n3][n2][N]
    const void* m;          // T[n3][n2][N]
    int n2, n3;
    const void* twiddle;    // complex<T>[N]: exp(-2πi k / N)
};

template <typename T, int N, int TL>
__global__ __launch_bounds__(TL * kWave) void precond_lines_kernel(PrecondLineArgs a) {
    using C = typename Cplx2<T>::type;
    constexpr int LINE = N + (N >> 4) + 1;
    constexpr int PW = 16 / sizeof(T);                        // reals of m per 16-byte load
    constexpr int KIT = (N / PW + kWave - 1) / kWave;         // loads of m per lane
    // m is fetched before the first transform where it fits in 16 registers per lane: it is then in flight under the backward FFT
    constexpr bool PREFETCH = KIT * 16 <= 64;
    struct alignas(16) MPack { T v[PW]; };
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    C* tw = reinterpret_cast<C*>(smem);                       // [N]
    C* lines = tw + N;                                        // [TL][LINE]
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid / kWave;
    const C* twg = static_cast<const C*>(a.twiddle);
    for (int i = tid; i < N; i += TL * kWave) tw[i] = twg[i];
    __syncthreads();
    const int64_t nlines = (int64_t)a.n2 * a.n3;
    const int64_t line_id = (int64_t)blockIdx.x * TL + wave;
    if (line_id >= nlines) return;
    C* line = lines + wave * LINE;
    C* x = static_cast<C*>(a.data) + line_id * N;
    const int j3 = (int)(line_id / a.n2), j2 = (int)(line_id - (int64_t)j3 * a.n2);
    const int64_t mline = (int64_t)(j3 == 0 ? 0 : a.n3 - j3) * a.n2 + (j2 == 0 ? 0 : a.n2 - j2);
    const MPack* mg = reinterpret_cast<const MPack*>(static_cast<const T*>(a.m) + mline * N);

    // the line, conjugated, with 16-byte accesses (N is even: a line starts 16-byte aligned)
    if constexpr (sizeof(C) == 8) {
        const float4* x4 = reinterpret_cast<const float4*>(x);
        for (int k = lane; k < N / 2; k += kWave) {
            const float4 w = x4[k];
            C u, v;
            u.x = w.x; u.y = -w.y; v.x = w.z; v.y = -w.w;
            line[lpad(2 * k)] = u;
            line[lpad(2 * k + 1)] = v;
        }
    } else {
        for (int k = lane; k < N; k += kWave) {
            C u = x[k];
            u.y = -u.y;
            line[lpad(k)] = u;
        }
    }
    MPack mp[KIT];
    if constexpr (PREFETCH) {
#pragma unroll
        for (int i = 0; i < KIT; ++i) {
            const int q = lane + i * kWave;
            if (q < N / PW) mp[i] = mg[q];
        }
    }
    wave_lds_fence();
    fft_line<T, N, -1>(line, tw, lane);
#pragma unroll
    for (int i = 0; i < KIT; ++i) {
        const int q = lane + i * kWave;
        if (q < N / PW) {
            if constexpr (!PREFETCH) mp[i] = mg[q];
#pragma unroll
            for (int t = 0; t < PW; ++t) {
                const int src = q * PW + t, cell = src == 0 ? 0 : N - src;
                C v = line[lpad(cell)];
                v.x *= mp[i].v[t];
                v.y *= -mp[i].v[t];
                line[lpad(cell)] = v;
            }
        }
    }
    wave_lds_fence();
    fft_line<T, N, -1>(line, tw, lane);
    if constexpr (sizeof(C) == 8) {
        float4* x4 = reinterpret_cast<float4*>(x);
        for (int k = lane; k < N / 2; k += kWave) {
            const C u = line[lpad(2 * k)], v = line[lpad(2 * k + 1)];
            x4[k] = make_float4(u.x, u.y, v.x, v.y);
        }
    } else {
        for (int k = lane; k < N; k += kWave) x[k] = line[lpad(k)];
    }
}

template <typename T, int N>
hipError_t launch_precond_n(const PrecondLineArgs& a, hipStream_t stream) {
    using C = typename Cplx2<T>::type;
    constexpr int LINE = N + (N >> 4) + 1;
    constexpr int TL = (sizeof(C) * (16 * LINE + N) <= 80 * 1024) ? 16 : 8;      // as toeplitz_lines_kernel: two workgroups per CU
    static_assert(sizeof(C) * (size_t)(TL * LINE + N) <= kFftLdsLimit, "line buffers exceed the 160 KiB of LDS");
    const size_t lds = sizeof(C) * (size_t)(TL * LINE + N);
    auto fn = precond_lines_kernel<T, N, TL>;
    // the attribute is per device: remember which devices of this process have it
    static std::atomic<unsigned long long> prepared{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(prepared.load(std::memory_order_relaxed) & bit)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        prepared.fetch_or(bit, std::memory_order_relaxed);
    }
    const int64_t nlines = (int64_t)a.n2 * a.n3;
    hipLaunchKernelGGL(fn, dim3((unsigned)((nlines + TL - 1) / TL)), dim3(TL * kWave), lds, stream, a);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_precond_t(int n, const PrecondLineArgs& a, hipStream_t stream) {
    switch (n) {
        case 64: return launch_precond_n<T, 64>(a, stream);
        case 80: return launch_precond_n<T, 80>(a, stream);
        case 96: return launch_precond_n<T, 96>(a, stream);
        case 128: return launch_precond_n<T, 128>(a, stream);
        case 160: return launch_precond_n<T, 160>(a, stream);
        case 192: return launch_precond_n<T, 192>(a, stream);
        case 256: return launch_precond_n<T, 256>(a, stream);
        case 320: return launch_precond_n<T, 320>(a, stream);
        case 384: return launch_precond_n<T, 384>(a, stream);
        case 512: return launch_precond_n<T, 512>(a, stream);
        case 640: return launch_precond_n<T, 640>(a, stream);
        case 768: return launch_precond_n<T, 768>(a, stream);
        case 1024: return launch_precond_n<T, 1024>(a, stream);
        default: return hipErrorInvalidValue;
    }
}

constexpr bool precond_cases_cover_sizes() {
    constexpr int cases[] = {64, 80, 96, 128, 160, 192, 256, 320, 384, 512, 640, 768, 1024};
    if ((int)(sizeof(cases) / sizeof(cases[0])) != kNumFftLineSizes) return false;
    for (int i = 0; i < kNumFftLineSizes; ++i)
        if (cases[i] != kFftLineSizes[i]) return false;
    return true;
}
static_assert(precond_cases_cover_sizes(), "launch_precond_t must repeat kFftLineSizes (fft_line.h)");

}  // namespace

hipError_t launch_pc_embed(int dtype, void* grid, const void* K, int64_t cells, int num_cus, hipStream_t stream) {
    return st::launch_by_dtype(dtype, dim3(st::grid_for(cells, num_cus)), dim3(st::kThreads), stream, pc_embed_kernel<float>, pc_embed_kernel<double>, grid,
                               K, cells);
}

hipError_t launch_pc_fold(const PcGrid& g, void* c, const void* T, int num_cus, hipStream_t stream) {
    const int64_t n = (int64_t)g.n[0] * g.n[1] * g.n[2];
    return st::launch_by_dtype(g.dtype, dim3(st::grid_for(n, num_cus)), dim3(st::kThreads), stream, pc_fold_kernel<float>, pc_fold_kernel<double>, g, c, T,
                               n);
}

int pc_workgroups(int64_t n, int num_cus) { return (int)st::grid_for(n, num_cus); }

hipError_t launch_pc_eigen(int dtype, void* e, const void* c, int64_t n, double* part, int G, hipStream_t stream) {
    return st::launch_by_dtype(dtype, dim3(G), dim3(st::kThreads), stream, pc_eigen_kernel<float>, pc_eigen_kernel<double>, e, c, n, part);
}

hipError_t launch_pc_invert(int dtype, void* m, int64_t n, double mu, double thresh, double count, int num_cus, hipStream_t stream) {
    return st::launch_by_dtype(dtype, dim3(st::grid_for(n, num_cus)), dim3(st::kThreads), stream, pc_invert_kernel<float>, pc_invert_kernel<double>, m, n,
                               mu, thresh, count);
}

hipError_t launch_pc_scale(int dtype, void* out, const void* in, const void* f, int64_t n, int num_cus, hipStream_t stream) {
    const int64_t packs = dtype == NUFFT_F32 ? n / 2 : n;
    const dim3 gr(st::grid_for(packs, num_cus)), bl(st::kThreads);
    if (f) return st::launch_by_dtype(dtype, gr, bl, stream, pc_scale_kernel<float, true>, pc_scale_kernel<double, true>, out, in, f, n);
    return st::launch_by_dtype(dtype, gr, bl, stream, pc_scale_kernel<float, false>, pc_scale_kernel<double, false>, out, in, f, n);
}

hipError_t launch_pc_coil_power(int dtype, void* s, const void* const* maps, int ncoils, int64_t n, double* part, int G, hipStream_t stream) {
    for (int c0 = 0; c0 < ncoils; c0 += kPcCoils) {
        PcCoilTable tab{};
        const int nc = std::min(kPcCoils, ncoils - c0);
        for (int c = 0; c < nc; ++c) tab.maps[c] = maps[c0 + c];
        const int accumulate = c0 > 0 ? 1 : 0, last = c0 + nc == ncoils ? 1 : 0;
        hipError_t e = st::launch_by_dtype(dtype, dim3(G), dim3(st::kThreads), stream, pc_coil_power_kernel<float>, pc_coil_power_kernel<double>, s, tab, nc,
                                           accumulate, last, n, part);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_pc_coil_scaling(int dtype, void* d, int64_t n, double floor, int num_cus, hipStream_t stream) {
    return st::launch_by_dtype(dtype, dim3(st::grid_for(n, num_cus)), dim3(st::kThreads), stream, pc_coil_scaling_kernel<float>, pc_coil_scaling_kernel<double>,
                               d, n, floor);
}

bool precond_lines_supported(int dtype, int64_t n) {
    (void)dtype;
    for (int i = 0; i < kNumFftLineSizes; ++i)
        if (kFftLineSizes[i] == n) return true;
    return false;
}

hipError_t launch_precond_lines(int dtype, int64_t n, void* data, const void* m, int n2, int n3, const void* twiddle, hipStream_t stream) {
    if (n2 < 1 || n3 < 1) return hipErrorInvalidValue;
    PrecondLineArgs a{};
    a.data = data; a.m = m; a.n2 = n2; a.n3 = n3; a.twiddle = twiddle;
    return dtype == NUFFT_F32 ? launch_precond_t<float>((int)n, a, stream) : launch_precond_t<double>((int)n, a, stream);
}

}  // namespace nufft
