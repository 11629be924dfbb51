// Launchers of the circulant preconditioner's kernels (precond.cpp, precond_kernels.hip), and what the solver
// (cg.cpp) needs to know of a preconditioner object.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "nufft_mi355x.h"

namespace nufft {

// The mode grid: n[d] = N_d cells (dimension 1 fastest), unused dimensions 1.
struct PcGrid {
    int dtype, D;
    int n[3];
};

// grid = K + 0 i on the (2N)^D embedding grid (`cells` elements)
hipError_t launch_pc_embed(int dtype, void* grid, const void* K, int64_t cells, int num_cus, hipStream_t stream);
// c_j = Σ_{s ∈ {0,1}^D} Π_d ω_d(j_d, s_d) T[(j − s ⊙ N) mod 2N],  ω_d(j, 0) = (N_d − j) / N_d,  ω_d(j, 1) = j / N_d  (T: complex<T>[(2N)^D],
// c: complex<T>[N^D]); terms of weight 0 (the Nyquist planes of T) are not read
hipError_t launch_pc_fold(const PcGrid& g, void* c, const void* T, int num_cus, hipStream_t stream);
// e = Re(c) (T[n]); part[g] = (max e, max −e) of workgroup g (double[G][2]).  G = pc_workgroups(...)
int pc_workgroups(int64_t n, int num_cus);
hipError_t launch_pc_eigen(int dtype, void* e, const void* c, int64_t n, double* part, int G, hipStream_t stream);
// m = 1 / (count * max(e + mu, thresh)), in place on e
hipError_t launch_pc_invert(int dtype, void* m, int64_t n, double mu, double thresh, double count, int num_cus, hipStream_t stream);
// out = f ⊙ in (complex<T>[n] times T[n]); f = null: out = in.  out may be in.
hipError_t launch_pc_scale(int dtype, void* out, const void* in, const void* f, int64_t n, int num_cus, hipStream_t stream);
// s = Σ_c |S_c|² in coil order (T[n]); part[g] = (max s, Σ s) of workgroup g (double[G][2])
hipError_t launch_pc_coil_power(int dtype, void* s, const void* const* maps, int ncoils, int64_t n, double* part, int G, hipStream_t stream);
// d = 1 / sqrt(max(s, floor)), in place on s
hipError_t launch_pc_coil_scaling(int dtype, void* d, int64_t n, double floor, int num_cus, hipStream_t stream);

// Dimension 1 of the fused apply, in place: per contiguous line of n cells — backward FFT, times the line of the multiplier at the
// negated frequencies, forward FFT.  data: complex<T>[nlines][n] (line = j_3 * n2 + j_2); m: T[nlines][n]; twiddle: exp(−2πi k / n).
bool precond_lines_supported(int dtype, int64_t n);
hipError_t launch_precond_lines(int dtype, int64_t n, void* data, const void* m, int n2, int n3, const void* twiddle, hipStream_t stream);

// The block preconditioner of a coupled operator (precond_block_kernels.hip).  B is stored like the operator's
// multipliers: `bd` T[K][pitch] (the diagonal blocks, real) and `bc` complex<T>[pairs a < b, row-major][pitch]; B_ba = conj(B_ab).  A grid
// has n cells; pitch >= n keeps every grid 16-byte aligned (the fused path has pitch = n).
constexpr double kPcPivotFraction = 0.25;      // a Cholesky pivot below this fraction of the shift is floored there
// E -> B = (E + shift I)⁻¹ / count per cell, in place on the K (K + 1) / 2 grids: FP64 Cholesky and triangular inverse; part[g] = cells of
// wave g where a pivot was floored at `pivot_floor` (double[G]: whole numbers).  G = pc_block_invert_workgroups(...)
int pc_block_invert_workgroups(int64_t n, int K, int num_cus);
hipError_t launch_pc_block_invert(int dtype, void* bd, void* bc, int K, int64_t n, int64_t pitch, double shift, double pivot_floor, double count,
                                  double* part,
                                  int G, hipStream_t stream);
// data[a] = Σ_b B_ab ⊙ data[b] per cell, in place; data: K arrays complex<T>[n], `data_stride` complex elements apart (dense path)
hipError_t launch_pc_block_multiply(int dtype, void* data, int64_t data_stride, int K, const void* bd, const void* bc, int64_t n, int64_t pitch,
                                    int num_cus, hipStream_t stream);
// Dimension 1 of the fused apply for K coupled components, in place: one wave owns the K lines of a line id (data: K arrays
// complex<T>[nlines][n], `data_stride` complex elements apart) — K backward FFTs, the block of B at the negated frequencies per cell, K
// forward FFTs, all inside LDS.  _supported: the K lines of length n fit the LDS of one wave.
bool precond_block_lines_supported(int dtype, int64_t n, int K);
hipError_t launch_precond_block_lines(int dtype, int64_t n, int K, void* data, int64_t data_stride, const void* bd, const void* bc, int n2, int n3,
                                      const void* twiddle, hipStream_t stream);

// The operator a preconditioner was built for (the solver refuses one built for another).
const ::nufft_toeplitz* precond_operator(const ::nufft_precond* pc);

}  // namespace nufft
