// Kernels of the block-circulant preconditioner of a coupled Toeplitz normal operator (precond.cpp).
//
// Build: pc_block_invert_kernel turns the K (K + 1) / 2 grids of E (one K × K Hermitian matrix per cell) into B = (E + shift I)⁻¹ / n in
// place.  Apply: pc_block_multiply_kernel, the streaming block multiply of the dense path, and precond_block_lines_kernel, dimension 1
// of the fused path: precond_lines_kernel (precond_kernels.hip) with the K lines of a line id in one wave's LDS and the block row
// of toeplitz_lines_coupled_kernel (toeplitz_coupled.hip) between the transforms.
#include <hip/hip_runtime.h>

#include <atomic>

#include "fft_line.h"
#include "kernels.h"
#include "precond.h"
#include "stream_kernels.h"
#include "toeplitz.h"

namespace nufft {
namespace {

namespace st = stream;
using st::Pack;

// ---------------------------------------------------------------------------------------------------
// The build.  One thread per cell and step; its matrix, the lower triangle in FP64, lives in LDS as [entry][thread] (a thread's entries
// are blockDim.x elements apart: no bank conflicts, no register arrays, nothing spills for any K).  The strict lower triangle holds L
// of A = L L^H and then X = L⁻¹; the diagonal holds 1 / L_jj throughout, which is X_jj.  A⁻¹ = X^H X.
// ---------------------------------------------------------------------------------------------------
template <typename T>
__global__ void pc_block_invert_kernel(T* bd, T* bc, int K, int64_t n, int64_t pitch, double shift, double pivot_floor, double count, double* part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double2* mat = reinterpret_cast<double2*>(smem);
    const int NT = blockDim.x, tid = threadIdx.x;
    auto M = [&](int i, int j) -> double2& { return mat[(size_t)(i * (i + 1) / 2 + j) * NT + tid]; };
    auto pair = [&](int a, int b) { return a * (K - 1) - a * (a - 1) / 2 + (b - a - 1); };      // coupled_offdiag_index (toeplitz.h), a < b
    double floored = 0.0;
    for (int64_t cell = (int64_t)blockIdx.x * NT + tid; cell < n; cell += (int64_t)gridDim.x * NT) {
        for (int i = 0; i < K; ++i) {
            for (int j = 0; j < i; ++j) {      // A_ij = conj(E_ji), the stored pair (j, i)
                const T* e = bc + 2 * ((int64_t)pair(j, i) * pitch + cell);
                M(i, j) = make_double2((double)e[0], -(double)e[1]);
            }
            M(i, i) = make_double2((double)bd[(int64_t)i * pitch + cell] + shift, 0.0);
        }
        bool hit = false;
        for (int j = 0; j < K; ++j) {
            double s = M(j, j).x;
            for (int k = 0; k < j; ++k) {
                const double2 l = M(j, k);
                s -= l.x * l.x + l.y * l.y;
            }
            if (!(s > pivot_floor) || !isfinite(s)) {
                s = pivot_floor;
                hit = true;
            }
            const double rd = 1.0 / sqrt(s);
            M(j, j) = make_double2(rd, 0.0);
            for (int i = j + 1; i < K; ++i) {
                double2 v = M(i, j);
                for (int k = 0; k < j; ++k) {      // v −= L_ik conj(L_jk)
                    const double2 a = M(i, k), b = M(j, k);
                    v.x -= a.x * b.x + a.y * b.y;
                    v.y -= a.y * b.x - a.x * b.y;
                }
                M(i, j) = make_double2(v.x * rd, v.y * rd);
            }
        }
        if (hit) floored += 1.0;
        // X = L⁻¹ column by column: X_ij = −(Σ_{j <= k < i} L_ik X_kj) / L_ii; column j only reads L_ik with k >= j
        for (int j = 0; j < K; ++j) {
            for (int i = j + 1; i < K; ++i) {
                double2 s = make_double2(0.0, 0.0);
                for (int k = j; k < i; ++k) {
                    const double2 l = M(i, k), x = M(k, j);
                    s.x += l.x * x.x - l.y * x.y;
                    s.y += l.x * x.y + l.y * x.x;
                }
                const double rd = M(i, i).x;
                M(i, j) = make_double2(-s.x * rd, -s.y * rd);
            }
        }
        // B_ab = Σ_{k >= b} conj(X_ka) X_kb / count,  a <= b
        for (int a = 0; a < K; ++a) {
            for (int b = a; b < K; ++b) {
                double2 s = make_double2(0.0, 0.0);
                for (int k = b; k < K; ++k) {
                    const double2 u = M(k, a), v = M(k, b);
                    s.x += u.x * v.x + u.y * v.y;
                    s.y += u.x * v.y - u.y * v.x;
                }
                if (a == b) {
                    bd[(int64_t)a * pitch + cell] = (T)(s.x / count);
                } else {
                    T* o = bc + 2 * ((int64_t)pair(a, b) * pitch + cell);
                    o[0] = (T)(s.x / count);
                    o[1] = (T)(s.y / count);
                }
            }
        }
    }
    floored = st::wave_reduce<st::Sum>(floored);
    if ((tid & 63) == 0) part[(int64_t)blockIdx.x * (NT / 64) + (tid >> 6)] = floored;
}

// threads per workgroup of the build: 256 while a workgroup's matrices stay within 40 KiB, else one wave (K = 16: 136 KiB)
int invert_threads(int K) { return K <= 4 ? 256 : 64; }

// ---------------------------------------------------------------------------------------------------
// The dense path's multiply, data[a] = Σ_b B_ab ⊙ data[b] per cell in place: tz_multiply_coupled_kernel (toeplitz_kernels.hip) for a
// cell count that may be odd — the ComplexF32 element behind the last whole pack goes to one thread.  A thread holds the K values of
// its CW cells, so every array and every grid of B is read once.  KT: the compile-time bound of the run-time K.
// ---------------------------------------------------------------------------------------------------
template <typename T, int KT, int CW>
__device__ __forceinline__ void block_cells(T* data, int64_t stride, int K, const T* bd, const T* bc, int64_t pitch, int64_t cell) {
    T v[KT][2 * CW], acc[KT][2 * CW];
#pragma unroll
    for (int a = 0; a < KT; ++a) {
        if (a < K) {
            const T* x = data + a * stride + 2 * cell;
            if constexpr (2 * CW == Pack<T>::W) {
                const Pack<T> pk = *reinterpret_cast<const Pack<T>*>(x);
#pragma unroll
                for (int w = 0; w < 2 * CW; ++w) v[a][w] = pk.v[w];
            } else {
#pragma unroll
                for (int w = 0; w < 2 * CW; ++w) v[a][w] = x[w];
            }
#pragma unroll
            for (int w = 0; w < CW; ++w) {
                const T d = bd[(int64_t)a * pitch + cell + w];
                acc[a][2 * w] = d * v[a][2 * w];
                acc[a][2 * w + 1] = d * v[a][2 * w + 1];
            }
        }
    }
#pragma unroll
    for (int a = 0; a < KT; ++a) {
#pragma unroll
        for (int b = a + 1; b < KT; ++b) {
            if (b < K) {
                const T* k = bc + 2 * ((int64_t)(a * (K - 1) - a * (a - 1) / 2 + (b - a - 1)) * pitch + cell);
                T kv[2 * CW];
                if constexpr (2 * CW == Pack<T>::W) {
                    const Pack<T> pk = *reinterpret_cast<const Pack<T>*>(k);
#pragma unroll
                    for (int w = 0; w < 2 * CW; ++w) kv[w] = pk.v[w];
                } else {
#pragma unroll
                    for (int w = 0; w < 2 * CW; ++w) kv[w] = k[w];
                }
#pragma unroll
                for (int w = 0; w < CW; ++w) {
                    const T kr = kv[2 * w], ki = kv[2 * w + 1];
                    acc[a][2 * w] += kr * v[b][2 * w] - ki * v[b][2 * w + 1];
                    acc[a][2 * w + 1] += kr * v[b][2 * w + 1] + ki * v[b][2 * w];
                    acc[b][2 * w] += kr * v[a][2 * w] + ki * v[a][2 * w + 1];
                    acc[b][2 * w + 1] += kr * v[a][2 * w + 1] - ki * v[a][2 * w];
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < KT; ++a) {
        if (a < K) {
            T* x = data + a * stride + 2 * cell;
            if constexpr (2 * CW == Pack<T>::W) {
                Pack<T> pk;
#pragma unroll
                for (int w = 0; w < 2 * CW; ++w) pk.v[w] = acc[a][w];
                *reinterpret_cast<Pack<T>*>(x) = pk;
            } else {
#pragma unroll
                for (int w = 0; w < 2 * CW; ++w) x[w] = acc[a][w];
            }
        }
    }
}

template <typename T, int KT>
__global__ __launch_bounds__(st::kThreads) void pc_block_multiply_kernel(T* data, int64_t stride, int K, const T* bd, const T* bc, int64_t n, int64_t pitch) {
    constexpr int CW = Pack<T>::W / 2;
    const int64_t npacks = n / CW;
    for (int64_t q = (int64_t)blockIdx.x * st::kThreads + threadIdx.x; q < npacks; q += (int64_t)gridDim.x * st::kThreads)
        block_cells<T, KT, CW>(data, stride, K, bd, bc, pitch, q * CW);
    if constexpr (CW > 1) {
        if (blockIdx.x == 0 && threadIdx.x == 0)
            for (int64_t cell = npacks * CW; cell < n; ++cell) block_cells<T, KT, 1>(data, stride, K, bd, bc, pitch, cell);
    }
}

// ---------------------------------------------------------------------------------------------------
// Dimension 1 of the fused apply.  As precond_lines_kernel the apply is F(B~ ⊙ B x) with B~(q) = B(−q) (F⁻¹ ∘ F = (F ∘ P) ∘ (P ∘ B) / n with P
// the negation of the index, and P moves onto the multiplier; nothing is conjugated by that, so it holds for complex blocks), and the
// negated frequencies are taken where B is read: the wave of line (j_2, j_3) reads the lines (−j_2, −j_3) of B, whose entry i multiplies
// the cell (N − i) mod N.  The conjugation bookkeeping for the single (forward) twiddle table is that of toeplitz_lines_coupled_kernel:
// lines are conjugated while they are loaded, the first forward FFT leaves l_b = conj(B x_b), the block row is applied to v_b = conj(l_b),
//   y_a = B~_aa v_a + Σ_{b > a} B~_ab v_b + Σ_{b < a} conj(B~_ba) v_b,
// and the second forward FFT gives F y_a.  A lane reads and writes its own cells only (i -> (N − i) mod N is a bijection of the line).
// ---------------------------------------------------------------------------------------------------
struct BlockLineArgs {
    void* data;             // K arrays complex<T>[n3][n2][N], data_stride complex elements apart
    int64_t data_stride;
    const void* bd;         // T[K][n3 * n2 * N]
    const void* bc;         // complex<T>[K (K − 1) / 2][n3 * n2 * N]
    int n2, n3, K;
    const void* twiddle;    // complex<T>[N]: exp(-2πi k / N)
};

// Waves per workgroup, as coupled_waves of the operator's kernel: the most of {16, 8, 4} that leave room for two workgroups per CU,
// else the most of {16, ..., 1} that fit at all; 0: not even one wave's KT lines fit.  The tiers 8 and 16 stop at 8 waves: a workgroup of
// 16 waves leaves a lane 128 registers, which the accumulators of the block row of 8 components exceed (ComplexF32, N = 64 spilled).
constexpr int block_waves(size_t csize, int n, int kt) {
    const size_t line = (size_t)(n + (n >> 4) + 1);
    const int most = kt >= 8 ? 8 : 16;
    for (int tl = most; tl >= 4; tl >>= 1)
        if (csize * ((size_t)n + (size_t)tl * kt * line) <= 80 * 1024) return tl;
    for (int tl = most; tl >= 1; tl >>= 1)
        if (csize * ((size_t)n + (size_t)tl * kt * line) <= kFftLdsLimit) return tl;
    return 0;
}
constexpr int block_tier(int K) { return K <= 2 ? 2 : (K <= 4 ? 4 : (K <= 8 ? 8 : 16)); }

template <typename T, int N, int KT, int TL>
__global__ __launch_bounds__(TL * kWave) void precond_block_lines_kernel(BlockLineArgs a) {
    using C = typename Cplx2<T>::type;
    constexpr int LINE = N + (N >> 4) + 1;
    constexpr int PW = 16 / sizeof(T);                        // cells per 16-byte load of a real line (half as many of a complex one)
    constexpr int NQ = N / PW;
    // the diagonal lines of a lane's first cells are in flight under the K backward FFTs where that takes at most 16 registers
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
    const int64_t nlines = (int64_t)a.n2 * a.n3;
    const int64_t line_id = (int64_t)blockIdx.x * TL + wave;
    if (line_id >= nlines) return;
    C* mine = lines + (size_t)wave * K * LINE;
    const int64_t cells = nlines * N;
    const int j3 = (int)(line_id / a.n2), j2 = (int)(line_id - (int64_t)j3 * a.n2);
    const int64_t mline = (int64_t)(j3 == 0 ? 0 : a.n3 - j3) * a.n2 + (j2 == 0 ? 0 : a.n2 - j2);
    const T* bd = static_cast<const T*>(a.bd) + mline * N;
    const T* bc = static_cast<const T*>(a.bc) + 2 * mline * N;

    // the K lines, conjugated, with 16-byte accesses (N is even: a line starts 16-byte aligned)
    for (int b = 0; b < K; ++b) {
        C* line = mine + b * LINE;
        const C* x = static_cast<const C*>(a.data) + (int64_t)b * a.data_stride + line_id * N;
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
    }
    [[maybe_unused]] KPack dpre[PREFETCH ? KT : 1];
    if constexpr (PREFETCH) {
#pragma unroll
        for (int c = 0; c < KT; ++c)
            if (c < K) dpre[c] = *reinterpret_cast<const KPack*>(bd + (int64_t)c * cells + lane * PW);
    }
    wave_lds_fence();
    for (int b = 0; b < K; ++b) fft_line<T, N, -1>(mine + b * LINE, tw, lane);

    for (int q = lane; q < NQ; q += kWave) {
        const int m0 = q * PW;                                // entries m0 ... m0 + PW − 1 of the lines of B: the cells (N − m) mod N
        int cell[PW];
#pragma unroll
        for (int t = 0; t < PW; ++t) cell[t] = lpad(m0 + t == 0 ? 0 : N - (m0 + t));
        C acc[KT][PW];
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            if (c < K) {
                KPack d;
                if constexpr (PREFETCH) {
                    if (q == lane) d = dpre[c];
                    else d = *reinterpret_cast<const KPack*>(bd + (int64_t)c * cells + m0);
                } else {
                    d = *reinterpret_cast<const KPack*>(bd + (int64_t)c * cells + m0);
                }
#pragma unroll
                for (int t = 0; t < PW; ++t) {
                    const C l = mine[c * LINE + cell[t]];           // v = conj(l)
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
                    const T* kp = bc + 2 * ((int64_t)(c * (K - 1) - c * (c - 1) / 2 + (b - c - 1)) * cells + m0);
                    const KPack k0 = *reinterpret_cast<const KPack*>(kp), k1 = *reinterpret_cast<const KPack*>(kp + PW);
#pragma unroll
                    for (int t = 0; t < PW; ++t) {
                        const T kr = 2 * t < PW ? k0.v[(2 * t) % PW] : k1.v[(2 * t) % PW];
                        const T ki = 2 * t < PW ? k0.v[(2 * t + 1) % PW] : k1.v[(2 * t + 1) % PW];
                        const C lc = mine[c * LINE + cell[t]], lb = mine[b * LINE + cell[t]];
                        // y_c += B_cb v_b,  v_b = conj(l_b) = (lb.x, −lb.y)
                        acc[c][t].x += kr * lb.x + ki * lb.y;
                        acc[c][t].y += ki * lb.x - kr * lb.y;
                        // y_b += conj(B_cb) v_c,  v_c = (lc.x, −lc.y)
                        acc[b][t].x += kr * lc.x - ki * lc.y;
                        acc[b][t].y += -kr * lc.y - ki * lc.x;
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            if (c < K) {
#pragma unroll
                for (int t = 0; t < PW; ++t) mine[c * LINE + cell[t]] = acc[c][t];
            }
        }
    }
    wave_lds_fence();
    for (int b = 0; b < K; ++b) fft_line<T, N, -1>(mine + b * LINE, tw, lane);

    for (int b = 0; b < K; ++b) {
        const C* line = mine + b * LINE;
        C* x = static_cast<C*>(a.data) + (int64_t)b * a.data_stride + line_id * N;
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
}

template <typename T, int N, int KT>
hipError_t launch_block_n_k(const BlockLineArgs& a, hipStream_t stream) {
    using C = typename Cplx2<T>::type;
    constexpr int TL = block_waves(sizeof(C), N, KT);
    if constexpr (TL == 0) {
        return hipErrorInvalidValue;
    } else {
        constexpr int LINE = N + (N >> 4) + 1;
        static_assert(sizeof(C) * ((size_t)N + (size_t)TL * KT * LINE) <= kFftLdsLimit, "line buffers exceed the 160 KiB of LDS");
        const size_t lds = sizeof(C) * ((size_t)N + (size_t)TL * a.K * LINE);
        auto fn = precond_block_lines_kernel<T, N, KT, TL>;
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
        const int64_t nlines = (int64_t)a.n2 * a.n3;
        hipLaunchKernelGGL(fn, dim3((unsigned)((nlines + TL - 1) / TL)), dim3(TL * kWave), lds, stream, a);
        return hipGetLastError();
    }
}

template <typename T, int N>
hipError_t launch_block_n(const BlockLineArgs& a, hipStream_t stream) {
    switch (block_tier(a.K)) {
        case 2: return launch_block_n_k<T, N, 2>(a, stream);
        case 4: return launch_block_n_k<T, N, 4>(a, stream);
        case 8: return launch_block_n_k<T, N, 8>(a, stream);
        default: return launch_block_n_k<T, N, 16>(a, stream);
    }
}

// the line length: the I-th entry of kFftLineSizes (fft_line.h)
template <typename T, int I = 0>
hipError_t launch_block_t(int n, const BlockLineArgs& a, hipStream_t stream) {
    if constexpr (I == kNumFftLineSizes) {
        return hipErrorInvalidValue;
    } else {
        if (n == kFftLineSizes[I]) return launch_block_n<T, kFftLineSizes[I]>(a, stream);
        return launch_block_t<T, I + 1>(n, a, stream);
    }
}

}  // namespace

int pc_block_invert_workgroups(int64_t n, int K, int num_cus) {
    const int nt = invert_threads(K);
    const int64_t need = (n + nt - 1) / nt, cap = (int64_t)std::max(num_cus, 1) * (nt == 64 ? 4 : 2);
    return (int)std::max<int64_t>(1, std::min(need, cap)) * (nt / 64);      // one partial per wave
}

hipError_t launch_pc_block_invert(int dtype, void* bd, void* bc, int K, int64_t n, int64_t pitch, double shift, double pivot_floor, double count, double* part,
                                  int G, hipStream_t stream) {
    if (K < 1 || K > kMaxCoupled) return hipErrorInvalidValue;
    const int nt = invert_threads(K);
    const size_t lds = (size_t)(K * (K + 1) / 2) * sizeof(double2) * nt;
    const void* fn = dtype == NUFFT_F32 ? reinterpret_cast<const void*>(pc_block_invert_kernel<float>)
                                        : reinterpret_cast<const void*>(pc_block_invert_kernel<double>);
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);      // (the build is not a hot path)
    if (e != hipSuccess) return e;
    const dim3 gr(G / (nt / 64)), bl(nt);
    if (dtype == NUFFT_F32)
        hipLaunchKernelGGL(pc_block_invert_kernel<float>, gr, bl, lds, stream, static_cast<float*>(bd), static_cast<float*>(bc), K, n, pitch, shift,
                           pivot_floor, count, part);
    else
        hipLaunchKernelGGL(pc_block_invert_kernel<double>, gr, bl, lds, stream, static_cast<double*>(bd), static_cast<double*>(bc), K, n, pitch, shift,
                           pivot_floor, count, part);
    return hipGetLastError();
}

hipError_t launch_pc_block_multiply(int dtype, void* data, int64_t data_stride, int K, const void* bd, const void* bc, int64_t n, int64_t pitch,
                                    int num_cus, hipStream_t stream) {
    if (K < 1 || K > kMaxCoupled) return hipErrorInvalidValue;
    const int64_t packs = dtype == NUFFT_F32 ? n / 2 : n, stride = 2 * data_stride;      // reals between two arrays
    const dim3 gr(st::grid_for(packs, num_cus)), bl(st::kThreads);
    switch (block_tier(K)) {
        case 2: return st::launch_by_dtype(dtype, gr, bl, stream, pc_block_multiply_kernel<float, 2>, pc_block_multiply_kernel<double, 2>, data, stride, K, bd, bc, n, pitch);
        case 4: return st::launch_by_dtype(dtype, gr, bl, stream, pc_block_multiply_kernel<float, 4>, pc_block_multiply_kernel<double, 4>, data, stride, K, bd, bc, n, pitch);
        case 8: return st::launch_by_dtype(dtype, gr, bl, stream, pc_block_multiply_kernel<float, 8>, pc_block_multiply_kernel<double, 8>, data, stride, K, bd, bc, n, pitch);
        default: return st::launch_by_dtype(dtype, gr, bl, stream, pc_block_multiply_kernel<float, 16>, pc_block_multiply_kernel<double, 16>, data, stride, K, bd, bc, n, pitch);
    }
}

bool precond_block_lines_supported(int dtype, int64_t n, int K) {
    if (K < 1 || K > kMaxCoupled || !precond_lines_supported(dtype, n)) return false;
    return block_waves(dtype == NUFFT_F32 ? 8 : 16, (int)n, block_tier(K)) > 0;
}

hipError_t launch_precond_block_lines(int dtype, int64_t n, int K, void* data, int64_t data_stride, const void* bd, const void* bc, int n2, int n3,
                                      const void* twiddle, hipStream_t stream) {
    if (n2 < 1 || n3 < 1 || !precond_block_lines_supported(dtype, n, K)) return hipErrorInvalidValue;
    BlockLineArgs a{};
    a.data = data; a.data_stride = data_stride; a.bd = bd; a.bc = bc; a.n2 = n2; a.n3 = n3; a.K = K; a.twiddle = twiddle;
    return dtype == NUFFT_F32 ? launch_block_t<float>((int)n, a, stream) : launch_block_t<double>((int)n, a, stream);
}

}  // namespace nufft
