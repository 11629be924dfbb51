// Launchers of the coil sensitivity map estimate (coilmaps.cpp, coilmaps_kernels.hip): the layout of a workgroup,
// shared by host and device, and the launch record.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "nufft_mi355x.h"

namespace nufft {

constexpr int kCmMaxCoils = 32;            // one Jacobi team is at most 32 lanes of a wave; all pointers travel in ONE launch
constexpr int kCmMaxBox = 9;               // box side
constexpr int kCmMaxThreads = 256;
constexpr int kCmMatrixBytes = 32 << 10;   // H and V of all teams of a workgroup, C <= 16 ...
constexpr int kCmMatrixBytesWide = 64 << 10;   // ... and C > 16 (two teams)
constexpr int kCmStageBytes = 48 << 10;    // staged tile plus halo, C <= 16: two workgroups per compute unit ...
constexpr int kCmStageBytesWide = 90 << 10;    // ... and C > 16: one
constexpr int kCmWantGroups = 1024;        // tiles shrink (down to one cell per team) while there are fewer workgroups than this

// How a workgroup is laid out for (element type, C, D, box, N); host and device use the same numbers.
//   LDS:  stage  C * hpitch complex T   [coil][halo cell], the cell fastest, hpitch odd         (staged only)
//         H, V   teams * C * C complex double each
//         red    teams double (largest λ1 of a team), teams int (its largest sweep count)
// A team of TW lanes takes the cells team, team + teams, ... of the tile, dimension 1 fastest.  Where not even a tile of `teams` cells
// fits with its halo, nothing is staged and the neighbours are read from global memory (through L2).
struct CoilmapsLayout {
    int TW;             // lanes of a team: the next power of two >= C
    int teams;          // teams per workgroup (a power of two); the workgroup has teams * TW threads (at least 64)
    int threads;
    int staged;
    int tile[3];        // output cells per dimension
    int halo[3];        // tile[d] + box[d] - 1
    int tcells, hcells, hpitch;
    int ntile[3];       // tiles per dimension
    int64_t G;          // workgroups
    size_t off_H, off_V, off_red, bytes;
};
CoilmapsLayout coilmaps_layout(bool f32, int C, int D, const int* box, const int64_t* N);

struct CoilmapsLaunch {
    int dtype, D, C;
    int N[3], box[3];
    int64_t pitch[3];                  // elements between neighbours along d = {1, N_1, N_1 N_2}
    int64_t n;
    const void* in[kCmMaxCoils];
    void* out[kCmMaxCoils];
    double p[2 * kCmMaxCoils];         // the phase reference, by value
    void* lambda1;                     // real T [n] or null
    void* lambda2;
    double* part;                      // [G]: the largest λ1 of a workgroup
    int32_t* sweeps_part;              // [G]: its largest sweep count
    double* words;                     // [0]: max λ1; the int32 at byte 8: max sweeps
    double crop2;                      // crop²
};

// allows the main kernel more than 64 KiB of dynamic LDS on the current device (once per object, at create time)
hipError_t coilmaps_allow_lds();
hipError_t launch_coilmaps(const CoilmapsLaunch& a, const CoilmapsLayout& L, hipStream_t stream);
hipError_t launch_coilmaps_max(const CoilmapsLaunch& a, int64_t G, hipStream_t stream);
// out[c][x] = 0 where lambda1[x] < crop2 * words[0]; reads lambda1, writes only the zeroed cells
hipError_t launch_coilmaps_crop(const CoilmapsLaunch& a, int num_cus, hipStream_t stream);

}  // namespace nufft
