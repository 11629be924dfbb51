// Launchers of the Toeplitz normal operator's kernels (toeplitz.cpp): the streaming kernels of the dense
// path and of the multiplier's construction (toeplitz_kernels.hip) and the fused dimension-1 pass (fft_lines.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

#include "nufft_mi355x.h"

namespace nufft {

// The coil maps set on an operator (borrowed device pointers, in coil order; empty: none) — for the preconditioner (precond.cpp).
const std::vector<const void*>& toeplitz_coil_maps(const ::nufft_toeplitz* t);

// The embedding grid: n2[d] = 2 N_d cells (dimension 1 fastest), the plan's nk[d] = N_d modes sit at map[d][k'] (= k mod 2 N_d);
// inv[d][j] is the kept index at cell j or -1.  Unused dimensions have n2 = nk = 1 and one-entry maps.
struct TzGrid {
    int dtype, D;
    int n2[3], nk[3];
    const int32_t* map[3];
    const int32_t* inv[3];
};

// grid = zero-padded û: every cell written once (the kept modes gathered through inv, zeros elsewhere)
hipError_t launch_tz_pad(const TzGrid& g, void* grid, const void* u, int num_cus, hipStream_t stream);
// grid *= K (K real, same shape)
hipError_t launch_tz_multiply(const TzGrid& g, void* grid, const void* K, int num_cus, hipStream_t stream);
// out = grid at the kept modes
hipError_t launch_tz_crop(const TzGrid& g, void* out, const void* grid, int num_cus, hipStream_t stream);
// grid = T with the Nyquist planes (index N_d of dimension d) zeroed; T_modes may be grid itself
hipError_t launch_tz_spectrum_load(const TzGrid& g, void* grid, const void* T_modes, int num_cus, hipStream_t stream);
// K = scale * Re(grid)
hipError_t launch_tz_real_part(const TzGrid& g, void* K, const void* grid, double scale, int num_cus, hipStream_t stream);
// values = weights + 0 i (complex<T>[n] from T[n]; weights = null: ones)
hipError_t launch_tz_weights(int dtype, void* values, const void* weights, int64_t n, int num_cus, hipStream_t stream);

// The multi-coil operator.  smap: the coil's sensitivity map, complex<T> laid out like û.
// grid = zero-padded S ⊙ û
hipError_t launch_tz_pad_map(const TzGrid& g, void* grid, const void* u, const void* smap, int num_cus, hipStream_t stream);
// out = conj(S) ⊙ (grid at the kept modes), added to what out holds when `accumulate`
hipError_t launch_tz_crop_map(const TzGrid& g, void* out, const void* grid, const void* smap, bool accumulate, int num_cus, hipStream_t stream);

// Coil expand and combine over n complex elements (host tables of device pointers, passed to the kernel by value kCoilChunk coils at a
// time).  expand: out[c] = S_c ⊙ in.  combine: out = Σ_c conj(S_c) ⊙ in[c] in coil order in registers, started from what out holds
// when `accumulate`; beyond kCoilChunk coils the running sum passes through `out` once per chunk, in the same order.
constexpr int kCoilChunk = 64;
struct CoilTable {
    const void* maps[kCoilChunk];
    void* data[kCoilChunk];
};
hipError_t launch_coil_expand(int dtype, int64_t n, int ncoils, void* const* out, const void* const* maps, const void* in, int num_cus,
                              hipStream_t stream);
hipError_t launch_coil_combine(int dtype, int64_t n, int ncoils, void* out, const void* const* maps, const void* const* in, bool accumulate,
                               int num_cus, hipStream_t stream);

// Dimension 1 of the fused apply, in place: per contiguous line of k1 kept modes, backward FFT of length n (= 2 k1), times the
// line of K, forward FFT, kept modes stored back.  data: complex<T>[nlines][k1]; K: T[nlines][n]; twiddle: exp(-2πi m / n).
bool toeplitz_lines_supported(int dtype, int64_t n);
hipError_t launch_toeplitz_lines(int dtype, int64_t n, void* data, const void* K, int64_t nlines, int k1, const int32_t* map,
                                 const void* twiddle, hipStream_t stream);

// Coupled components.  The K × K block multiplier is stored as K real grids (the diagonal, `kd`:
// T[K][cells]) and K (K − 1) / 2 complex grids (`kc`: complex<T>[pairs a < b, row-major][cells]); K_ba = conj(K_ab).
constexpr int kMaxCoupled = 16;
inline int coupled_offdiag_index(int a, int b, int K) { return a * (K - 1) - a * (a - 1) / 2 + (b - a - 1); }      // a < b
// values[j] = w_j conj(φ_a(j)) φ_b(j)  (complex<T>[n]; weights = null: ones; φ 16-byte aligned)
hipError_t launch_tz_pair_weights(int dtype, void* values, const void* weights, const void* phi_a, const void* phi_b, int64_t n, int num_cus,
                                  hipStream_t stream);
// Kc = scale * grid  (complex, same shape: the multiplier of a pair a < b)
hipError_t launch_tz_complex_part(const TzGrid& g, void* Kc, const void* grid, double scale, int num_cus, hipStream_t stream);
// grids[a] = Σ_b K_ab ⊙ grids[b] per cell, in place; grids: K complex grids `grid_stride` complex elements apart
hipError_t launch_tz_multiply_coupled(const TzGrid& g, void* grids, int64_t grid_stride, int K, const void* kd, const void* kc, int num_cus,
                                      hipStream_t stream);
// Dimension 1 of the fused apply for K coupled components, in place: one wave owns the K lines of a line id (data: K arrays
// complex<T>[nlines][k1], `data_stride` complex elements apart), transforms them backward, applies the block multiplier per cell and
// transforms them forward inside LDS.  _supported: the K lines of length n fit the LDS of one wave.
bool toeplitz_lines_coupled_supported(int dtype, int64_t n, int K);
hipError_t launch_toeplitz_lines_coupled(int dtype, int64_t n, int K, void* data, int64_t data_stride, const void* kd, const void* kc,
                                         int64_t nlines, int k1, const int32_t* map, const void* twiddle, hipStream_t stream);

}  // namespace nufft
