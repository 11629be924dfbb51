// The 16-byte pack of complex cells a lane of the total-variation kernels owns (tv_kernels.hip, tvt_kernels.hip): one ComplexF64, two
// ComplexF32, or one ComplexF32 where the arrays' rows are not 16-byte aligned.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace nufft {
namespace tvcells {

template <typename T>
struct alignas(2 * sizeof(T)) Cx {
    T re, im;
};

template <typename T, int V>
struct alignas(V * 2 * sizeof(T)) Cells {
    Cx<T> v[V];
};

template <typename T, int V>
__device__ __forceinline__ Cells<T, V> load_cells(const Cx<T>* a, int64_t at) {
    return *reinterpret_cast<const Cells<T, V>*>(a + at);
}
template <typename T, int V>
__device__ __forceinline__ void store_cells(Cx<T>* a, int64_t at, const Cells<T, V>& c) {
    *reinterpret_cast<Cells<T, V>*>(a + at) = c;
}

template <typename T>
__device__ __forceinline__ Cx<T> sub(Cx<T> a, Cx<T> b) {
    return Cx<T>{a.re - b.re, a.im - b.im};
}
template <typename T, int V>
__device__ __forceinline__ Cells<T, V> sub(const Cells<T, V>& a, const Cells<T, V>& b) {
    Cells<T, V> r;
#pragma unroll
    for (int w = 0; w < V; ++w) r.v[w] = sub(a.v[w], b.v[w]);
    return r;
}

}  // namespace tvcells
}  // namespace nufft
