"""CG solver measurement: N = 256³, fused apply path, 20 iterations, uniform points.

Times, in one process and alternating rep by rep (hipEvent medians after warm-up), per iteration:
  * baseline: the README's PyTorch CG loop around op(p)                 (what users ran before the solver existed)
  * ToeplitzCG.solve with check_every = 0 and rtol = 0, eager          (all iterations enqueued, no host synchronisation)
  * the same solve captured once and replayed as a graph
  * the apply alone                                                     (so that vector work = total − apply)
and the peak torch-allocated memory of the baseline loop against the solver's own workspace.  Prints one JSON line.
With --trace-only it runs three eager solves and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nufft_pkg import nufft  # noqa: E402


def readme_loop(op, b, iters):
    x = torch.zeros_like(b)
    r = b.clone()
    p = r.clone()
    rr = torch.vdot(r.flatten(), r.flatten()).real
    for _ in range(iters):
        Gp = op(p)
        alpha = rr / torch.vdot(p.flatten(), Gp.flatten()).real
        x += alpha * p
        r -= alpha * Gp
        rr_new = torch.vdot(r.flatten(), r.flatten()).real
        p = r + (rr_new / rr) * p
        rr = rr_new
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=2e6, help="number of points the operator is built from")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", choices=("c128", "c64"), default="c128")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    n, N, iters = int(args.n), (args.size,) * 3, args.iters
    Z, T = (torch.complex128, torch.float64) if args.dtype == "c128" else (torch.complex64, torch.float32)
    cb = 16 if args.dtype == "c128" else 8
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    xs = tuple(torch.rand(n, generator=g, device=dev, dtype=T) * (2 * math.pi) for _ in N)
    w = torch.rand(n, generator=g, device=dev, dtype=T) + 0.1
    plan = nufft.PlanNUFFT(Z, N, m=4, sigma=2.0, backend=nufft.ROCBackend(0))
    op = nufft.ToeplitzOperator(plan)
    assert op.path == "fused"
    op.set_points(xs, w)
    plan.close()
    del xs, w
    b = op(torch.randn(tuple(reversed(N)), generator=g, device=dev, dtype=Z))
    sol = nufft.ToeplitzCG(op, maxiter=iters, rtol=0.0, lam=0.0)     # b lies in the range of G: λ = 0 as in the README's loop
    x = torch.empty_like(b)
    q = torch.empty_like(b)

    if args.trace_only:
        for _ in range(3):
            sol.solve(b, out=x)
        torch.cuda.synchronize()
        assert sol.iterations == (iters,), sol.iterations
        return

    def run_baseline():
        readme_loop(op, b, iters)

    def run_solver():
        sol.solve(b, out=x)

    def run_apply():
        for _ in range(iters):
            op.apply(b, out=q)

    for _ in range(2):
        run_baseline()
        run_solver()
        run_apply()
    torch.cuda.synchronize()
    eager = x.clone()
    assert sol.iterations == (iters,), sol.iterations
    base = readme_loop(op, b, iters)
    agree = float(torch.linalg.vector_norm(base - eager) / torch.linalg.vector_norm(eager))
    del base
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        sol.solve(b, out=x)
    x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    graph_same_bits = bool(torch.equal(x, eager))

    routes = [("baseline_loop", run_baseline), ("solver_eager", run_solver), ("solver_graph", graph.replay), ("apply_alone", run_apply)]
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
    # peak memory of the baseline loop (torch's allocator) against the solver's own arrays
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    at_rest = torch.cuda.memory_allocated()
    run_baseline()
    torch.cuda.synchronize()
    peak_baseline = torch.cuda.max_memory_allocated() - at_rest
    torch.cuda.reset_peak_memory_stats()
    run_solver()
    torch.cuda.synchronize()
    peak_solver_torch = torch.cuda.max_memory_allocated() - at_rest

    arr = N[0] * N[1] * N[2] * cb
    vec = {k: med[k] - med["apply_alone"] for k in ("baseline_loop", "solver_eager", "solver_graph")}
    out = {"metric": "cg_iteration_ms", "value": med["solver_eager"], "dtype": args.dtype, "N": N, "iterations": iters,
           "ms_per_iteration": {k: round(v, 4) for k, v in med.items()},
           "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in acc.items()},
           "vector_work_ms": {k: round(v, 4) for k, v in vec.items()},
           "vector_work_ratio_baseline_over_solver": round(vec["baseline_loop"] / vec["solver_eager"], 2),
           "kernel_bytes": {"cg_dot_kernel": 2 * arr, "cg_update_kernel": 6 * arr, "cg_direction_kernel": 3 * arr},
           "vector_gb_per_s_solver": round(11 * arr / (vec["solver_eager"] * 1e-3) / 1e9, 1),
           "peak_mb": {"baseline_torch": round(peak_baseline / 1e6, 1), "solver_torch": round(peak_solver_torch / 1e6, 1),
                       "solver_workspace": round(sol.info().workspace_bytes / 1e6, 1)},
           "workgroups": sol.info().workgroups, "baseline_vs_solver_rel_l2": agree, "graph_same_bits": graph_same_bits}
    for k in acc:
        print(f"  {k:16s} {med[k]:8.4f} ms / iteration   (min {min(acc[k]):.4f}, max {max(acc[k]):.4f})")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
