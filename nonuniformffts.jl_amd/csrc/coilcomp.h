// Launchers of coil compression and noise pre-whitening (coilcomp.cpp, coilcomp_kernels.hip): the tiling of the
// Gram kernel, shared by host and device, and the launch records.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "nufft_mi355x.h"

namespace nufft {

constexpr int kCcMaxCoils = 64;            // the lanes of a one-wave Jacobi team; all pointers travel in ONE launch
constexpr int kCcThreads = 256;
constexpr int kCcPairsPerThread = 9;       // 64 * 65 / 2 = 2080 upper-triangle entries over 256 threads
constexpr int kCcMaxGroups = 512;          // workgroups of the Gram kernel = partial sets the object holds
constexpr int kCcTileBytes = 32 << 10;     // staged samples of one tile
constexpr int kCcApplyChunk = 16;          // virtual coils per apply launch: complex FP64 accumulators of one lane and sample

// How the Gram kernel walks n samples of C vectors; the same numbers on host and device, and they depend on (element type, C, n) alone.
//   LDS:  data  C * (TC + 1) complex T   [coil][sample], the sample fastest, one padding sample per coil
//         w     TC double                the weights of the tile (ones without a weight vector)
//         gp    S * np complex double    [segment][entry], np = C (C + 1) / 2
//         ij    np uint16                entry -> (i << 8 | j)
struct CcTiling {
    int TC;             // samples per tile (a power of two, 32 ... 1024)
    int S;              // segments of a tile that are summed side by side (a power of two)
    int64_t tiles;      // ceil(n / TC)
    int64_t tpw;        // consecutive tiles of one workgroup
    int G;              // workgroups = ceil(tiles / tpw) <= kCcMaxGroups
    size_t off_w, off_gp, off_ij, bytes;
};
CcTiling coilcomp_tiling(bool f32, int C, int64_t n);
size_t coilcomp_eigen_lds(int C);          // H, V (C x C complex double each), λ (C double), order (C int)

struct CcPointers {
    const void* p[kCcMaxCoils];
};

struct CcGramLaunch {
    int dtype, C;
    int64_t n;
    CcTiling tl;
    CcPointers y;
    const void* weights;       // real T [n] or null
    double* part;              // [G][np] complex double
    double* R;                 // [C][C] complex double, Hermitian
};

struct CcFinishLaunch {
    int C, whiten;
    const double* R;           // the accumulated Gram matrix
    const double* W;           // the whitening matrix (whiten only)
    double* T;                 // W R, then W R W^H (whiten only)
    double* Uh;                // U^H: straight into A without whitening
    double* A;
    double* lambda;            // [C]
    int32_t* words;            // [0] sweeps, [1] status
};

struct CcApplyLaunch {
    int dtype, C, V;           // V virtual coils of this launch (<= kCcApplyChunk), the rows v0 ... v0 + V - 1 of A
    int v0;
    int64_t n;
    CcPointers in;
    void* out[kCcApplyChunk];
    const double* A;           // [rows][C] complex double
};

hipError_t coilcomp_allow_lds();
hipError_t launch_coilcomp_gram(const CcGramLaunch& a, hipStream_t stream);    // the Gram kernel and the fold into R
hipError_t launch_coilcomp_finish(const CcFinishLaunch& a, hipStream_t stream);
hipError_t launch_coilcomp_apply(const CcApplyLaunch& a, int num_cus, hipStream_t stream);

}  // namespace nufft
