// Launchers of the locally low-rank proximal map (llr.cpp, fista.cpp, llr_kernels.hip) and what the FISTA solver
// (fista.cpp) needs from a nufft_llr object.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "nufft_mi355x.h"

namespace nufft {

constexpr int kLlrMaxK = 16;           // components: all pointers travel in ONE launch
constexpr int kLlrThreads = 256;
constexpr int kLlrMaxElems = 8192;     // B * K of one block: 128 KiB of ComplexF64 in LDS
constexpr int kLlrTileElems = 2048;    // a workgroup takes as many whole blocks as fit into this many elements (one block if it is larger)
constexpr int kLlrMaxSegments = 16;    // voxel segments of one Gram entry
constexpr int kLlrSweepsMax = 24;      // cap of the cyclic Jacobi sweeps

// How a workgroup is laid out for (element type, K, B); host and device use the same numbers.
//   LDS:  data   nb * B * K complex T            [blk][k][voxel]
//         H, V   nb * K * K complex double each  (P overwrites H)
//         gpart  nb * S * K (K + 1) / 2 complex double: the Gram entries of S voxel segments, summed in segment order
//         lam    nb * K double, red kWaves double
struct LlrLayout {
    int nb;            // blocks per workgroup (a power of two)
    int S;             // voxel segments per Gram entry (a power of two, <= B)
    int TW;            // lanes of the team that diagonalises one block: the next power of two >= K
    size_t off_H, off_V, off_g, off_lam, off_red, bytes;
};
LlrLayout llr_layout(bool f32, int K, int B);

enum { LLR_PLAIN = 0, LLR_FISTA = 1 };

struct LlrLaunch {
    int dtype, D, K, mode;
    int bshift[3];               // log2 of the block sides (0 beyond D)
    int nblk[3];                 // blocks per dimension
    int N[3];
    int64_t pitch[3];            // elements between neighbours along d = {1, N_1, N_1 N_2}
    int64_t blocks;              // all blocks
    int shift[3];
    double t;                    // the threshold on the singular values
    double* part;                // [G][3]: |x+ - x|^2, |x+|^2 (LLR_FISTA only), sum of the kept singular values
    const void* in[kLlrMaxK];    // LLR_PLAIN: the input;  LLR_FISTA: b
    void* out[kLlrMaxK];         // LLR_PLAIN: the output; LLR_FISTA: x
    // LLR_FISTA: v = z - step (q + lambda z - b) on load;  x+ = result, z = x+ + beta (x+ - x), x = x+ on store
    void* z;
    const void* q;
    int64_t stride;              // reals between the components of z, q
    double step, lambda, beta;
    const int32_t* flag;         // (null: none) a set flag[0] freezes the system: every workgroup leaves at once
};

int64_t llr_workgroups(const LlrLaunch& a);
// allows the kernels more than 64 KiB of dynamic LDS on the current device (once per object, at create time)
hipError_t llr_allow_lds();
hipError_t launch_llr(const LlrLaunch& a, hipStream_t stream);
// out[0] = sum over g of part[g * 3 + 2], one workgroup, fixed order
hipError_t launch_llr_sum(const double* part, int64_t G, double* out, hipStream_t stream);

// What the solver asks of the object.
int llr_create_geometry(::nufft_llr** out, int dtype, int D, const int64_t* N, int C, int device, const nufft_llr_params* params);
// the geometry, partial-sum buffer and pointers left empty: the solver fills mode, t, shift, pointers and the FISTA fields
LlrLaunch llr_launch_template(const ::nufft_llr* l);
int llr_block_side(const ::nufft_llr* l, int d);
int llr_shifts(const ::nufft_llr* l);
uint64_t llr_seed(const ::nufft_llr* l);

}  // namespace nufft
