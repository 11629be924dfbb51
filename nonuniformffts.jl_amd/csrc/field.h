// Launchers of the time-segment fit of a field map (field.cpp, field_kernels.hip): the histogram of ω, the
// temporal interpolators φ_l(t_j) and the factors B_l(x) = exp(−i ω(x) τ_l).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "nufft_mi355x.h"

namespace nufft {

constexpr int kFsMaxSegments = 16;         // = kMaxCoupled: what a segmented Toeplitz operator takes
constexpr int kFsMaxBins = 1024;
constexpr int kFsThreads = 256;
constexpr int kFsMaxGroups = 256;          // workgroups of the range kernel = rows of partials the object holds
constexpr int kFsReseed = 32;              // bins between two exact sincos of the recurrence = bins of one staged piece of the table

// The template tier of the interpolator kernel that serves L segments: 1, 2, 4, 8 or 16 accumulators in registers.
inline int fieldseg_tier(int L) {
    int t = 1;
    while (t < L) t *= 2;
    return t;
}
// LDS of one workgroup of the interpolator kernel: a piece of the table (kFsReseed bins × tier complex doubles), the kFsReseed centres
// of the piece and P (tier × tier complex doubles).
inline size_t fieldseg_interp_lds(int L) {
    const size_t t = (size_t)fieldseg_tier(L);
    return (size_t)kFsReseed * t * 16 + (size_t)kFsReseed * 8 + t * t * 16;
}
inline size_t fieldseg_hist_lds(int nbins) { return (size_t)nbins * 4; }

// One row of the range kernel's partials, and the folded result
struct FsRange {
    double lo, hi;                         // over the counted finite values (+inf, −inf when there are none)
    unsigned long long bad, counted;       // counted values that are not finite; counted values
};

struct FsPointers {
    void* p[kFsMaxSegments];
};
struct FsTau {
    double v[kFsMaxSegments];
};

// part[g] = the range of workgroup g's share of ω over the mask (mask = null: every element), then out[0] = their fold in index order
hipError_t launch_fieldseg_range(int dtype, const void* omega, const uint8_t* mask, int64_t n, FsRange* part, FsRange* out, int num_cus,
                                 hipStream_t stream);
// counts[min(nb − 1, (int)((ω − lo) · scale))] += 1 over the mask; counts zeroed by the caller (a memset node)
hipError_t launch_fieldseg_histogram(int dtype, const void* omega, const uint8_t* mask, int64_t n, double lo, double scale, int nb,
                                     uint32_t* counts, int num_cus, hipStream_t stream);
// phi[l][j] = Σ_l' P[l, l'] Σ_b table[b][l'] exp(−i ω_b t_j): table[b][l'] = h_b exp(i ω_b τ_l') (complex double, [nb][tier], zero behind
// L), centres ω_b = centres[b] equally spaced by `delta`, P complex double [L][L] row-major
hipError_t launch_fieldseg_interpolators(int dtype, int L, int nb, const void* times, int64_t np, const double* table, const double* centres,
                                         double delta, const double* P, const FsPointers& phi, hipStream_t stream);
// B[l][x] = exp(−i ω[x] τ_l)
hipError_t launch_fieldseg_factors(int dtype, int L, const void* omega, int64_t n, const FsTau& tau, const FsPointers& B, int num_cus,
                                   hipStream_t stream);

}  // namespace nufft
