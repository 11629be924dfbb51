// Where a thread of the stencil kernels works (tv_kernels.hip, tgv_kernels.hip): the tiling of tv_tile (tv.h) turned into coordinates.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "tv.h"

namespace nufft {

// Cell (i0 ... i0 + V − 1, i1, i2), the first of the `steps` cells the thread visits along the marching dimension (D = 1: one cell,
// D = 2: dimension 2, D = 3: dimension 3), and whether it lies inside the box at all.
struct Walk {
    int k, c;             // component: slot of this launch, index in the solver
    int64_t g;            // workgroup of the component (row of the partial sums)
    int i0, i1, i2;
    int steps;
    bool inside;
    int64_t at;           // i0 + N0 (i1 + N1 i2)
};

// L: a launch struct with c0, tiles[3] and N[3] (TvLaunch, TgvLaunch)
template <int D, int V, typename L>
__device__ __forceinline__ Walk walk_of(const L& a) {
    Walk w;
    w.k = blockIdx.z / a.tiles[2];                      // once per workgroup
    const int t2 = blockIdx.z - w.k * a.tiles[2];
    w.c = a.c0 + w.k;
    w.g = blockIdx.x + (int64_t)a.tiles[0] * (blockIdx.y + (int64_t)a.tiles[1] * t2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    w.i1 = w.i2 = 0;
    w.steps = 1;
    if (D == 1) {
        w.i0 = (blockIdx.x * 256 + threadIdx.x) * V;
        w.inside = w.i0 < a.N[0];
    } else if (D == 2) {
        w.i0 = (blockIdx.x * 64 + lane) * V;
        w.i1 = (blockIdx.y * 4 + wave) * kTvMarch;
        w.inside = w.i0 < a.N[0] && w.i1 < a.N[1];
        w.steps = min(kTvMarch, a.N[1] - w.i1);
    } else {
        w.i0 = (blockIdx.x * 64 + lane) * V;
        w.i1 = blockIdx.y * 4 + wave;
        w.i2 = t2 * kTvMarch;
        w.inside = w.i0 < a.N[0] && w.i1 < a.N[1] && w.i2 < a.N[2];
        w.steps = min(kTvMarch, a.N[2] - w.i2);
    }
    w.at = w.i0 + (int64_t)a.N[0] * (w.i1 + (int64_t)a.N[1] * w.i2);
    return w;
}

}  // namespace nufft
