// Launchers of the wavelet transform's kernels (wavelet.cpp, wavelet_kernels.hip) and what the FISTA solver
// (fista.cpp) needs from a nufft_wavelet object.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "nufft_mi355x.h"

namespace nufft {

constexpr int kWaveletBatch = 8;       // components per launch (gridDim.y): the callers' pointers travel as kernel arguments
constexpr int kWaveletThreads = 256;

// The tile of a workgroup in coarse positions per dimension, fixed per (element type, D) so that the kernels know every extent at compile
// time: 1-D 256; 2-D 32 x 8; 3-D 16 x 4 x 4 (ComplexF32) or 16 x 4 x 2 (ComplexF64).  With the 4-tap halo both tile buffers stay within
// 64 KiB of LDS, and dimension 1 keeps rows of >= 34 contiguous elements.
constexpr int wavelet_tile(bool f32, int D, int d) {
    return D == 1 ? (d == 0 ? 256 : 1) : D == 2 ? (d == 0 ? 32 : d == 1 ? 8 : 1) : (d == 0 ? 16 : d == 1 ? 4 : (f32 ? 4 : 2));
}

// One level of the transform for up to kWaveletBatch components.  A level works on the sub-box m[d] = N_d / 2^level of every component;
// h[d] = m[d] / 2 (dimensions beyond D: m = h = 1, not transformed).  Every workgroup owns a tile of to[d] = wavelet_tile coarse positions per
// dimension (2 to[d] fine positions), tiles[d] = ceil(h[d] / to[d]) tiles per dimension, linear in blockIdx.x, dimension 1 fastest.
struct WaveletLevel {
    int dtype, D, taps;
    int m[3], h[3], to[3], tiles[3];
    int64_t pitch[3];            // of the full arrays (Mallat layout): elements between neighbours along d = {1, N_1, N_1 N_2}
    int c0, nc;                  // first component of this launch, number in it
    // analysis: src -> detail bands into coef (Mallat positions), the low-pass corner into low
    // synthesis: detail bands from coef and the low-pass corner from low -> dst
    // `fine` is src / dst: either full arrays (level 0: the callers', pitch) or the dense scratch of a level (pitch m)
    const void* fine_in[kWaveletBatch];
    void* fine_out[kWaveletBatch];
    int fine_dense;              // the fine side is a dense scratch array [m3][m2][m1]
    void* coef[kWaveletBatch];   // full arrays (const for synthesis)
    void* low[kWaveletBatch];    // the low-pass corner: dense scratch [h3][h2][h1], or the full array's corner (low_dense = 0)
    int low_dense;
    // analysis only: soft threshold of the detail coefficients on store (shrink != 0), sums of |stored detail| per workgroup
    int shrink;
    double thr[kWaveletBatch];
    double* part;                // [C][P] partial sums; this level's workgroups write [c][part_off + blockIdx.x]  (null: none)
    int P, part_off;
    // synthesis of level 0 inside FISTA (momentum != 0): x⁺ = the result;  z = x⁺ + beta (x⁺ − x);  x = x⁺;  per-workgroup sums of
    // |x⁺ − x|² and |x⁺|² into mom_part[c][blockIdx.x][2]
    int momentum;
    double beta;
    void* x[kWaveletBatch];      // the callers' x, full arrays
    double* mom_part;            // [C][G0][2]
    int G0;
    const int32_t* flag;         // [C] (null: none): a component whose flag is set is frozen, its workgroups leave at once
};

size_t wavelet_lds_bytes(const WaveletLevel& l, bool synthesis);
hipError_t launch_wavelet_analysis(const WaveletLevel& l, hipStream_t stream);
hipError_t launch_wavelet_synthesis(const WaveletLevel& l, hipStream_t stream);
// out[c] = Σ_p part[c][p], one workgroup per component, fixed order
hipError_t launch_wavelet_sum(const double* part, int P, int C, double* out, hipStream_t stream);

// What the solver asks of the object (all enqueue only; `flag` as above, may be null).
struct WaveletFista {
    int momentum = 0;
    double beta = 0.0;
    void* const* x = nullptr;
    double* mom_part = nullptr;
};
int wavelet_forward(::nufft_wavelet* w, void* const* out, const void* const* in, const double* thr_host, const int32_t* flag, hipStream_t stream);
int wavelet_inverse(::nufft_wavelet* w, void* const* out, const void* const* in, const WaveletFista* f, const int32_t* flag, hipStream_t stream);
// partial sums of Σ|shrunk detail| the last wavelet_forward with thresholds left: double[C][P], rows contiguous over components
const double* wavelet_partials(const ::nufft_wavelet* w, int* P);
// workgroups of the level-0 synthesis (the rows of mom_part)
int wavelet_level0_workgroups(const ::nufft_wavelet* w);
// creation from the geometry (what nufft_wavelet_create reads from a plan and nufft_fista_create from an operator)
int wavelet_create_geometry(::nufft_wavelet** out, int dtype, int D, const int64_t* N, int C, int device, const nufft_wavelet_params* params);

}  // namespace nufft
