// The in-LDS line FFT shared by the pruned passes (fft_lines.hip) and the coupled Toeplitz kernel (toeplitz_coupled.hip): complex
// helpers, the small DFTs, one Stockham stage and fft_line, plus the list of instantiated line lengths and the LDS limit.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.h"

namespace nufft {

template <typename T> struct Cplx2;
template <> struct Cplx2<float>  { using type = float2; };
template <> struct Cplx2<double> { using type = double2; };

template <typename C> __device__ __forceinline__ C cadd(C a, C b) { C r; r.x = a.x + b.x; r.y = a.y + b.y; return r; }
template <typename C> __device__ __forceinline__ C csub(C a, C b) { C r; r.x = a.x - b.x; r.y = a.y - b.y; return r; }
template <typename C> __device__ __forceinline__ C cmul(C a, C b) { C r; r.x = a.x * b.x - a.y * b.y; r.y = a.x * b.y + a.y * b.x; return r; }
// multiply by -i (SIGN = -1, forward) or +i (SIGN = +1, backward)
template <int SIGN, typename C> __device__ __forceinline__ C mul_i(C a) {
    C r;
    if (SIGN < 0) { r.x = a.y; r.y = -a.x; } else { r.x = -a.y; r.y = a.x; }
    return r;
}

template <int SIGN, typename C> __device__ __forceinline__ void dft2(C* u) {
    const C a = u[0], b = u[1];
    u[0] = cadd(a, b);
    u[1] = csub(a, b);
}
template <int SIGN, typename C> __device__ __forceinline__ void dft4(C* u) {
    const C e0 = cadd(u[0], u[2]), e1 = csub(u[0], u[2]);
    const C o0 = cadd(u[1], u[3]), o1 = mul_i<SIGN>(csub(u[1], u[3]));
    u[0] = cadd(e0, o0); u[1] = cadd(e1, o1); u[2] = csub(e0, o0); u[3] = csub(e1, o1);
}
template <int SIGN, typename T, typename C> __device__ __forceinline__ void dft8(C* u) {
    const T h = T(0.70710678118654752440);
    C s[4], d[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { s[t] = cadd(u[t], u[t + 4]); d[t] = csub(u[t], u[t + 4]); }
    // d1 *= w8, d2 *= w8^2 = -+i, d3 *= w8^3   (w8 = exp(SIGN * 2πi / 8))
    { C w; w.x = h; w.y = SIGN * h; d[1] = cmul(d[1], w); }
    d[2] = mul_i<SIGN>(d[2]);
    { C w; w.x = -h; w.y = SIGN * h; d[3] = cmul(d[3], w); }
    dft4<SIGN>(s);
    dft4<SIGN>(d);
#pragma unroll
    for (int t = 0; t < 4; ++t) { u[2 * t] = s[t]; u[2 * t + 1] = d[t]; }
}

// radix 3 and 5 (the oversampled sizes are products of 2, 3 and 5: nextprod((2, 3, 5), ...), src/plan.jl:485-498)
template <int SIGN, typename T, typename C> __device__ __forceinline__ void dft3(C* u) {
    const T s3 = T(0.86602540378443864676);            // sin(2 pi / 3)
    const C t1 = cadd(u[1], u[2]);
    C m1; m1.x = u[0].x - T(0.5) * t1.x; m1.y = u[0].y - T(0.5) * t1.y;
    const C d = csub(u[1], u[2]);
    C m2; m2.x = s3 * d.x; m2.y = s3 * d.y;
    const C im2 = mul_i<SIGN>(m2);                     // SIGN * i * sin(2 pi / 3) * (u1 - u2)
    u[0] = cadd(u[0], t1);
    u[1] = cadd(m1, im2);
    u[2] = csub(m1, im2);
}
template <int SIGN, typename T, typename C> __device__ __forceinline__ void dft5(C* u) {
    const T c1 = T(0.30901699437494742410), c2 = T(-0.80901699437494742410);   // cos(2 pi / 5), cos(4 pi / 5)
    const T s1 = T(0.95105651629515357212), s2 = T(0.58778525229247312917);    // sin(2 pi / 5), sin(4 pi / 5)
    const C a1 = cadd(u[1], u[4]), b1 = csub(u[1], u[4]);
    const C a2 = cadd(u[2], u[3]), b2 = csub(u[2], u[3]);
    C r1, r2, q1, q2;
    r1.x = u[0].x + c1 * a1.x + c2 * a2.x; r1.y = u[0].y + c1 * a1.y + c2 * a2.y;
    r2.x = u[0].x + c2 * a1.x + c1 * a2.x; r2.y = u[0].y + c2 * a1.y + c1 * a2.y;
    q1.x = s1 * b1.x + s2 * b2.x; q1.y = s1 * b1.y + s2 * b2.y;
    q2.x = s2 * b1.x - s1 * b2.x; q2.y = s2 * b1.y - s1 * b2.y;
    const C iq1 = mul_i<SIGN>(q1), iq2 = mul_i<SIGN>(q2);
    C u0; u0.x = u[0].x + a1.x + a2.x; u0.y = u[0].y + a1.y + a2.y;
    u[0] = u0;
    u[1] = cadd(r1, iq1);
    u[4] = csub(r1, iq1);
    u[2] = cadd(r2, iq2);
    u[3] = csub(r2, iq2);
}

__device__ __forceinline__ int lpad(int e) { return e + (e >> 4); }   // one pad element per 16: spreads banks

// One radix-R Stockham stage of a line held in LDS (in place, wave-synchronous).
// TWS: the twiddle table holds the roots of unity of order N * TWS (TWS = 2 for the half-length complex FFT
// inside a real transform, whose table is shared with the real/complex split step).
template <typename T, int N, int R, int P, int SIGN, int TWS = 1>
__device__ __forceinline__ void stage(typename Cplx2<T>::type* line, const typename Cplx2<T>::type* tw, int lane) {
    using C = typename Cplx2<T>::type;
    constexpr int p = P;                              // product of the radices of the earlier stages
    constexpr int NB = N / R;                         // butterflies per line
    constexpr int PER = (NB + kWave - 1) / kWave;     // butterflies per lane
    C u[PER][R];
    int jout[PER];
#pragma unroll
    for (int b = 0; b < PER; ++b) {
        const int i = lane + b * kWave;
        const int k = i % p;
        jout[b] = (i - k) * R + k;
        if (i < NB) {
#pragma unroll
            for (int t = 0; t < R; ++t) u[b][t] = line[lpad(i + t * NB)];
            if (p > 1) {
                const int step = k * (N / (p * R));   // w_{pR}^{k t} = w_N^{k t N / (p R)}; k t N / (p R) < N
#pragma unroll
                for (int t = 1; t < R; ++t) u[b][t] = cmul(u[b][t], tw[(step * t) * TWS]);
            }
            if constexpr (R == 8) dft8<SIGN, T>(u[b]);
            else if constexpr (R == 5) dft5<SIGN, T>(u[b]);
            else if constexpr (R == 4) dft4<SIGN>(u[b]);
            else if constexpr (R == 3) dft3<SIGN, T>(u[b]);
            else dft2<SIGN>(u[b]);
        }
    }
    wave_lds_fence();      // every read of this stage is issued before the first write (same wave, in order)
#pragma unroll
    for (int b = 0; b < PER; ++b) {
        const int i = lane + b * kWave;
        if (i < NB) {
#pragma unroll
            for (int t = 0; t < R; ++t) line[lpad(jout[b] + t * p)] = u[b][t];
        }
    }
    wave_lds_fence();
}

// Stockham stages for N = 2^a 3^b 5^c: radix 8 while possible, then 4 / 2, then 3s and 5s.
template <typename T, int N, int REM, int P, int SIGN, int TWS>
__device__ __forceinline__ void fft_stages(typename Cplx2<T>::type* line, const typename Cplx2<T>::type* tw, int lane) {
    if constexpr (REM > 1) {
        constexpr int R = REM % 8 == 0 ? 8 : (REM % 4 == 0 ? 4 : (REM % 2 == 0 ? 2 : (REM % 3 == 0 ? 3 : 5)));
        static_assert(REM % R == 0, "length must be a product of 2, 3 and 5");
        stage<T, N, R, P, SIGN, TWS>(line, tw, lane);
        fft_stages<T, N, REM / R, P * R, SIGN, TWS>(line, tw, lane);
    }
}

template <typename T, int N, int SIGN, int TWS = 1>
__device__ __forceinline__ void fft_line(typename Cplx2<T>::type* line, const typename Cplx2<T>::type* tw, int lane) {
    fft_stages<T, N, N, 1, SIGN, TWS>(line, tw, lane);
}

// The line lengths fft_lines.hip instantiates (its NUFFT_FFT_SIZES, which a static_assert there holds equal to this list), for
// translation units that dispatch on the length themselves.
constexpr int kFftLineSizes[] = {64, 80, 96, 128, 160, 192, 256, 320, 384, 512, 640, 768, 1024};
constexpr int kNumFftLineSizes = (int)(sizeof(kFftLineSizes) / sizeof(kFftLineSizes[0]));

constexpr size_t kFftLdsLimit = 160 * 1024;      // gfx950: LDS per workgroup

}  // namespace nufft
