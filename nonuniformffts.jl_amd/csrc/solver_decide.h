// The outcome of the proximal solvers (FISTA, the TV primal-dual solver, L+S) on the device: the scalars' struct, which the host
// lays out (solver_common.h), and the two steps every one of these solvers takes on them: the reset of its start kernel and the last
// step of its decision kernel (fista_kernels.hip, tv_kernels.hip, tvt_kernels.hip, tsparse_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace nufft {

// Scalars of a solver on the device, FP64, `count` slots: one per component, or one for a solver that is always one system.  The
// decision kernel is the only writer after the start, and it is a launch of its own: every other kernel of an iteration only reads
// the flags.
struct ProxScalars {
    double* change;     // [count]   ‖x⁺ − x‖ / ‖x⁺‖ after the last iteration that changed the slot
    int32_t* flag;      // [count]   done (frozen)
    int32_t* iters;     // [count]
    int32_t* status;    // [count]   kProx*: the values of NUFFT_FISTA_*, NUFFT_TVPD_* and NUFFT_LPS_*
    double* history;    // [max_iter][count][COLS]   column 0 the change, the others the solver's own
};

enum { kProxMaxIter = 0, kProxConverged = 1, kProxBreakdown = 2 };

// For all threads of ONE workgroup: NaN into the slot's history, the scalars as before the first iteration.
template <int COLS>
__device__ inline void reset_outcome(ProxScalars s, int slot, int count, int max_iter) {
    for (int it = threadIdx.x; it < max_iter; it += blockDim.x)
#pragma unroll
        for (int k = 0; k < COLS; ++k) s.history[((int64_t)it * count + slot) * COLS + k] = NAN;
    if (threadIdx.x == 0) {
        s.change[slot] = NAN;
        s.flag[slot] = 0;
        s.iters[slot] = 0;
        s.status[slot] = kProxMaxIter;
    }
}

// For one thread: the relative change of iteration `it` from dd = ‖x⁺ − x‖², xx = ‖x⁺‖² (0 when both are 0), stored with column 0 of the
// history row at `hist_index`, the iteration count, the status and the done flag.  A change that is not finite freezes the slot
// (breakdown).  Returns the change; the caller writes its own history columns.
__device__ inline double store_decision(ProxScalars s, int slot, int64_t hist_index, double dd, double xx, double tol, int it) {
    const double change = (dd == 0.0 && xx == 0.0) ? 0.0 : sqrt(dd / xx);
    const bool bad = !isfinite(change);
    const bool done = !bad && change <= tol;
    s.change[slot] = change;
    s.history[hist_index] = change;
    s.iters[slot] = it;
    s.status[slot] = bad ? kProxBreakdown : (done ? kProxConverged : kProxMaxIter);
    s.flag[slot] = bad || done ? 1 : 0;
    return change;
}

}  // namespace nufft
