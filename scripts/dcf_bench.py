"""Density-compensation measurement: N = 256³, m = 4, σ = 2, Direct(), Np = 1e7, 20 iterations.

Times, in one process and alternating rep by rep (hipEvent medians after warm-up), per iteration:
  * baseline: the loop a user writes on the stage-level API of a real plan: fill zeros + spread_from_points, interpolate, the torch
    divide and max                                                           (what users ran before the object existed)
  * DensityCompensation.compute with check_every = 0 and tol = 0, eager     (all iterations enqueued, no host synchronisation)
  * the stages of an iteration alone: zero fill, spread, gather (the check and update kernels' own times come from the kernel trace)
and the peak torch-allocated memory of the baseline loop against the object's own workspace.  Prints one JSON line.
With --trace-only it runs three eager computes and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nufft_pkg import nufft  # noqa: E402


def user_loop(plan, n, T, iters):
    w = torch.ones(n, dtype=T, device="cuda")
    v = torch.empty_like(w)
    delta = None
    for _ in range(iters):
        nufft.spread_from_points(plan, w)           # fill zeros + spread
        nufft.interpolate(plan, v)
        delta = (v - 1).abs().max()
        w = w / v
    return w / w.sum(), delta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e7)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", choices=("f64", "f32"), default="f64")
    ap.add_argument("--points", choices=("uniform", "folded_normal"), default="uniform")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    n, N, iters = int(args.n), (args.size,) * 3, args.iters
    T = torch.float64 if args.dtype == "f64" else torch.float32
    rb = 8 if args.dtype == "f64" else 4
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    if args.points == "uniform":
        xs = tuple(torch.rand(n, generator=g, device=dev, dtype=T) * (2 * math.pi) for _ in N)
    else:
        xs = tuple(torch.remainder(math.pi + torch.randn(n, generator=g, device=dev, dtype=T).abs(), 2 * math.pi) for _ in N)
    plan = nufft.PlanNUFFT(T, N, m=4, sigma=2.0, kernel_evalmode=nufft.Direct(), backend=nufft.ROCBackend(0))
    nufft.set_points(plan, xs)
    dc = nufft.DensityCompensation(plan, maxiter=iters, tol=0.0).set_points(xs)
    out = torch.empty(n, dtype=T, device=dev)
    v = torch.empty(n, dtype=T, device=dev)

    if args.trace_only:
        for _ in range(3):
            dc.compute(out=out)
        torch.cuda.synchronize()
        assert dc.iterations == iters
        return

    def run_baseline():
        user_loop(plan, n, T, iters)

    def run_library():
        dc.compute(out=out)

    def run_zero():
        for _ in range(iters):
            nufft.lib.nufft_fill_zeros(plan._handle, plan._stream())

    def run_spread():
        for _ in range(iters):
            nufft.spread_from_points(plan, out, zero=False)

    def run_gather():
        for _ in range(iters):
            nufft.interpolate(plan, v)

    for _ in range(2):
        run_baseline()
        run_library()
        run_zero()
        run_spread()
        run_gather()
    torch.cuda.synchronize()
    base, _ = user_loop(plan, n, T, iters)
    agree = float(torch.linalg.vector_norm(base - out) / torch.linalg.vector_norm(out))
    del base

    routes = [("user_loop", run_baseline), ("library", run_library), ("zero_fill", run_zero), ("spread", run_spread),
              ("gather", run_gather)]
    acc = {name: [] for name, _ in routes}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.reps):
        for name, fn in routes:
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            acc[name].append(e0.elapsed_time(e1) / iters)
    med = {k: sorted(v)[len(v) // 2] for k, v in acc.items()}
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    at_rest = torch.cuda.memory_allocated()
    run_baseline()
    torch.cuda.synchronize()
    peak_baseline = torch.cuda.max_memory_allocated() - at_rest
    torch.cuda.reset_peak_memory_stats()
    run_library()
    torch.cuda.synchronize()
    peak_library_torch = torch.cuda.max_memory_allocated() - at_rest

    stages = med["zero_fill"] + med["spread"] + med["gather"]
    upd = {k: med[k] - stages for k in ("user_loop", "library")}
    i = dc.info()
    # check: reads v; update: reads v and w, writes w — 4 arrays of Np reals per iteration; total − stages inherits the noise of four medians
    res = {"metric": "dcf_iteration_ms", "value": med["library"], "dtype": args.dtype, "points": args.points, "N": N, "Np": n,
           "iterations": iters, "ms_per_iteration": {k: round(x, 4) for k, x in med.items()},
           "ms_min_max": {k: [round(min(x), 4), round(max(x), 4)] for k, x in acc.items()},
           "library_over_user_loop": round(med["library"] / med["user_loop"], 4),
           "total_minus_stages_ms": {k: round(x, 4) for k, x in upd.items()},
           "kernel_bytes": {"dcf_check_kernel": n * rb, "dcf_update_kernel": 3 * n * rb},
           "peak_mb": {"user_loop_torch": round(peak_baseline / 1e6, 1), "library_torch": round(peak_library_torch / 1e6, 1),
                       "library_workspace": round(i.workspace_bytes / 1e6, 1), "library_plan": round(i.plan_bytes / 1e6, 1)},
           "workgroups": i.workgroups, "user_loop_vs_library_rel_l2": agree}
    for k in acc:
        print(f"  {k:22s} {med[k]:8.4f} ms / iteration   (min {min(acc[k]):.4f}, max {max(acc[k]):.4f})")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
