// Launchers of the kernels of the sample-density compensation iteration (dcf.cpp, dcf_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace nufft {

constexpr int kDcfMaxGroups = 1024;  // rows of the partials: the same for every device, so that a host-only object knows its size

// Scalars of the iteration on the device.  FP64 for both element types.
//   flag is double-buffered by the parity of the iteration that READS it (iteration k reads slot k & 1; the first workgroup of its
//   update kernel writes slot (k + 1) & 1), because every workgroup of that kernel still reads the old slot.
struct DcfScalars {
    double* res;        // [1]  the last δ that was reported (NaN: none yet)
    double* sum;        // [1]  Σ w the finish divided by (0: it did not run)
    double* history;    // [max_iter]
    int32_t* flag;      // [2]  done (frozen)
    int32_t* iters;     // [1]  divisions applied
    int32_t* status;    // [1]  NUFFT_DCF_*
    double* part;       // [kDcfMaxGroups][2]  per-workgroup partials: (max |v − 1|, bad v) of the check kernel, (unused, bad w0) of the
                        //                     start kernel, (Σ w, unused) of the sum kernel
};

struct DcfLaunch {
    int dtype;          // NUFFT_F32 | NUFFT_F64
    int G;              // workgroups of the array kernels = rows of `part` in use
    int64_t n;          // points
    void* w;            // the caller's vector T[n], the state of the iteration
    const void* v;      // own vector T[n]: C w
    double tol;
    double vscale;      // δ is taken of v * vscale (the first iteration of a caller's w0 sees the window's power-of-two scale; 1 otherwise)
    double gamma;       // finish without normalisation: w *= gamma (the same scale)
    int max_iter;
    int k;              // iteration number, 0-based (parity = k & 1)
    int report;         // δ_k goes into the history and the residual (k >= 1, or a caller's w0)
    int normalize;      // NUFFT_DCF_NORMALIZE_*
    DcfScalars s;
};

// w = 1 (no w0) or the test of the caller's w0 for entries that are not positive and finite (w is only read); partials into part
hipError_t launch_dcf_start(const DcfLaunch& a, bool use_w0, hipStream_t stream);
// one workgroup: reduces them; flag[0], iters = 0, status, res = NaN, sum = 0, NaN into the history
hipError_t launch_dcf_begin(const DcfLaunch& a, hipStream_t stream);
// the two kernels of an iteration: partials of max |v − 1| and of the breakdown test;  δ_k, done, status, history from them and w /= v
hipError_t launch_dcf_check(const DcfLaunch& a, hipStream_t stream);
hipError_t launch_dcf_update(const DcfLaunch& a, hipStream_t stream);
// finish: partials of Σ w;  w /= Σ w (or w *= gamma)
hipError_t launch_dcf_sum(const DcfLaunch& a, hipStream_t stream);
hipError_t launch_dcf_scale(const DcfLaunch& a, hipStream_t stream);

// workgroups for n reals of `dtype` on a device with num_cus compute units (<= kDcfMaxGroups)
int dcf_workgroups(int dtype, int64_t n, int num_cus);

}  // namespace nufft
