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

// The operator a preconditioner was built for (the solver refuses one built for another).
const ::nufft_toeplitz* precond_operator(const ::nufft_precond* pc);

}  // namespace nufft
