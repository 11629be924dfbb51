"""TGV² solver measurement: N = 256³, fused apply path, 1e7 uniform points, ComplexF32 and ComplexF64.

Times, in one process per element type and alternating rep by rep (hipEvent medians after warm-up), per iteration:
  * ToeplitzTGV.solve with check_every = 0 and tol = 0, eager           (all iterations enqueued, no host synchronisation)
  * the apply alone                                                     (so that the part outside the apply = total − apply)
  * baseline: the same algorithm written in torch (torch.roll) around op(...)
and checks that the torch loop and the solver agree after the iterations (1e-11 ComplexF64 / 1e-4 ComplexF32 relative, x and v).

The stencil kernels run only inside the solvers, so their own times come from a kernel trace: `--trace-only` runs three eager TGV solves
and three eager TV solves per element type and nothing else (the run to put under `rocprofv3 --kernel-trace --stats`), and
`--kernel-stats FILE... [--fold-only]` folds that run's kernel_stats.csv files into the result as GB/s over the kernels' algorithmic
bytes, in arrays A = n · sizeof(complex T) at D = 3, S = 6: tv_primal (5 + D) A, tv_dual (2 + 2D) A (the yardsticks of the same run),
tgv_field (S + 4D) A, tgv_p (2 + 4D) A, tgv_r (2D + 2S) A; an iteration outside the apply moves (7 + 11D + 3S) A = 58 A
(``ITERATION_ARRAYS``).

Every element type runs in a child process of its own under a time limit; the first one that fails or runs out of time ends the
measurement.  Writes one JSON document (--out) and prints it.
"""
import argparse
import csv
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = {"c128": 1e-11, "c64": 1e-4}
D3, S3 = 3, 6
# algorithmic arrays per launch at D = 3: reads + writes
KERNEL_ARRAYS = {"tv_primal_kernel": 5 + D3, "tv_dual_kernel": 2 + 2 * D3, "tgv_field_kernel": S3 + 4 * D3, "tgv_p_kernel": 2 + 4 * D3,
                 "tgv_r_kernel": 2 * D3 + 2 * S3}
ITERATION_ARRAYS = sum(KERNEL_ARRAYS[k] for k in ("tv_primal_kernel", "tgv_field_kernel", "tgv_p_kernel", "tgv_r_kernel"))      # 58


def torch_loop(torch, op, b, iters, a1, a0, step, sigma):
    """The solver's algorithm in torch: one apply, torch.roll for the differences, elementwise work, no host synchronisation."""
    D = b.dim()
    pairs = [(d, e) for d in range(D) for e in range(d, D)]
    index = {p: s for s, p in enumerate(pairs)}
    ax = lambda d: D - 1 - d      # noqa: E731
    back = lambda f, e: f - torch.roll(f, 1, dims=ax(e))      # noqa: E731
    x = torch.zeros_like(b)
    v = [torch.zeros_like(b) for _ in range(D)]
    p = [torch.zeros_like(b) for _ in range(D)]
    r = [torch.zeros_like(b) for _ in pairs]
    for _ in range(iters):
        div = sum(torch.roll(p[d], 1, dims=ax(d)) - p[d] for d in range(D))
        xp = x - step * (op(x) - b + div)
        xbar = xp + (xp - x)
        vp = [v[d] - step * (sum(r[index[(min(d, e), max(d, e))]] - torch.roll(r[index[(min(d, e), max(d, e))]], -1, dims=ax(e)) for e in range(D)) - p[d])
              for d in range(D)]
        vbar = [vp[d] + (vp[d] - v[d]) for d in range(D)]
        u = [p[d] + sigma * (torch.roll(xbar, -1, dims=ax(d)) - xbar - vbar[d]) for d in range(D)]
        nrm = torch.sqrt(sum(t.real ** 2 + t.imag ** 2 for t in u))
        scale = torch.where(nrm > a1, a1 / nrm, torch.ones_like(nrm))
        p = [t * scale for t in u]
        w = [r[s] + sigma * (0.5 * (back(vbar[d], e) + back(vbar[e], d))) for s, (d, e) in enumerate(pairs)]
        nrm = torch.sqrt(sum((1.0 if d == e else 2.0) * (t.real ** 2 + t.imag ** 2) for t, (d, e) in zip(w, pairs)))
        scale = torch.where(nrm > a0, a0 / nrm, torch.ones_like(nrm))
        r = [t * scale for t in w]
        x, v = xp, vp
    return x, v


def measure(torch, routes, reps, per):
    acc = {name: [] for name, _ in routes}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        for name, fn in routes:
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            acc[name].append(e0.elapsed_time(e1) / per[name])
    return {k: sorted(v)[len(v) // 2] for k, v in acc.items()}, {k: [round(min(v), 4), round(max(v), 4)] for k, v in acc.items()}


def worker(dtype, args):
    import torch
    sys.path.insert(0, ROOT)
    from nufft_pkg import nufft
    n, N, iters = int(args.n), (args.size,) * 3, args.iters
    Z, T = (torch.complex128, torch.float64) if dtype == "c128" else (torch.complex64, torch.float32)
    cb = 16 if dtype == "c128" else 8
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    xs = tuple(torch.rand(n, generator=g, device=dev, dtype=T) * (2 * math.pi) for _ in N)
    w = (torch.rand(n, generator=g, device=dev, dtype=T) + 0.1) / n
    plan = nufft.PlanNUFFT(Z, N, m=4, sigma=2.0, backend=nufft.ROCBackend(0))
    op = nufft.ToeplitzOperator(plan)
    assert op.path == "fused"
    op.set_points(xs, w)
    plan.close()
    del xs, w
    torch.cuda.empty_cache()
    b = op(torch.randn(tuple(reversed(N)), generator=g, device=dev, dtype=Z))
    lmax = max(op.max_eigenvalue())
    step = 1.0 / (1.05 * lmax)
    a1 = 0.1 * float(b.abs().max())
    a0 = 0.5 * a1
    x = torch.empty_like(b)
    q = torch.empty_like(b)
    arr = N[0] * N[1] * N[2] * cb
    sol = nufft.ToeplitzTGV(op, a1, alpha0=a0, step=step, maxiter=iters, tol=0.0)
    if args.trace_only:
        tv = nufft.ToeplitzTV(op, tv=a1, step=step, maxiter=iters, tol=0.0)      # the yardstick kernels, in the same run
        for _ in range(3):
            sol.solve(b, out=x)
            tv.solve(b, out=x)
        torch.cuda.synchronize()
        return {}
    routes = [("solver_eager", lambda: sol.solve(b, out=x)), ("apply_alone", lambda: [op.apply(b, out=q) for _ in range(iters)]),
              ("torch_loop", lambda: torch_loop(torch, op, b, iters, a1, a0, step, sol.sigma))]
    for _, fn in routes:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    assert sol.iterations == (iters,), sol.iterations
    med, minmax = measure(torch, routes, args.reps, {name: iters for name, _ in routes})
    outside = med["solver_eager"] - med["apply_alone"]
    sol.solve(b, out=x)
    field = sol.field()
    base_x, base_v = torch_loop(torch, op, b, iters, a1, a0, step, sol.sigma)
    err = float(torch.linalg.vector_norm(base_x - x) / torch.linalg.vector_norm(x))
    err_v = float(torch.linalg.vector_norm(torch.stack(base_v) - torch.stack(field)) / torch.linalg.vector_norm(torch.stack(field)))
    hist = sol.history()[-1, 0]
    r = {"lambda_max_estimate": lmax, "array_mb": round(arr / 1e6, 1), "alpha1": a1, "alpha0": a0, "step": step, "sigma": sol.sigma,
         "ms_per_iteration": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": minmax,
         "outside_apply_ms": round(outside, 4), "outside_apply_share": round(outside / med["solver_eager"], 3),
         "outside_apply_arrays": ITERATION_ARRAYS, "outside_apply_gb_per_s": round(ITERATION_ARRAYS * arr / (outside * 1e-3) / 1e9, 1),
         "torch_loop_outside_apply_ms": round(med["torch_loop"] - med["apply_alone"], 4),
         "iteration_ratio_torch_over_solver": round(med["torch_loop"] / med["solver_eager"], 2),
         "outside_apply_ratio_torch_over_solver": round((med["torch_loop"] - med["apply_alone"]) / outside, 2),
         "torch_loop_vs_solver_rel_l2": err, "torch_loop_vs_solver_rel_l2_field": err_v, "agreement_bar": BAR[dtype],
         "last_history_row": [float(t) for t in hist], "array_bytes_mb": round(sol.info().array_bytes / 1e6, 1),
         "workspace_mb": round(sol.info().workspace_bytes / 1e6, 1)}
    for k, v in med.items():
        print(f"  {dtype} {k:14s} {v:8.4f} ms", file=sys.stderr)
    assert err <= BAR[dtype] and err_v <= BAR[dtype], \
        f"the torch loop and the solver differ by {err:.3e} (x) / {err_v:.3e} (v) after {iters} iterations (bar {BAR[dtype]:g})"
    sol.close()
    op.close()
    return r


def fold_kernel_stats(results, paths, size):
    """Average time of the stencil kernels from rocprofv3 --kernel-trace --stats CSVs (columns Name, Calls, AverageNs), per element type,
    and the bandwidth they reach over their algorithmic bytes at D = 3.  tv_primal_kernel runs in both solvers: the same instantiation,
    the same bytes."""
    rows = [r for path in paths for r in csv.DictReader(open(path))]
    for dt, elem, cb in (("c64", "If", 8), ("c128", "Id", 16)):
        if dt not in results:
            continue
        arr = size ** 3 * cb
        for kernel, arrays in KERNEL_ARRAYS.items():
            hit = [r for r in rows if kernel in r["Name"] and (elem in r["Name"] or ("float" if dt == "c64" else "double") in r["Name"])]
            if not hit:
                continue
            calls = sum(int(r["Calls"]) for r in hit)
            ns = sum(float(r["AverageNs"]) * int(r["Calls"]) for r in hit) / calls
            results[dt][kernel] = {"calls": calls, "us": round(ns / 1e3, 2), "algorithmic_arrays": arrays,
                                   "gb_per_s": round(arrays * arr / (ns * 1e-9) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e7, help="number of points the operator is built from")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dtypes", default="c64,c128")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds every element type's child process may take")
    ap.add_argument("--trace-only", action="store_true", help="three eager solves of each solver per element type and nothing else")
    ap.add_argument("--kernel-stats", nargs="+", default=None, help="kernel_stats.csv files of a --trace-only run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--fold-only", action="store_true", help="only fold --kernel-stats into the existing --out")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tgv_bench.json"))
    args = ap.parse_args()
    if args.worker:
        print(json.dumps(worker(args.worker, args)))
        return
    if args.fold_only:
        out = json.load(open(args.out))
    else:
        results = {}
        for dt in args.dtypes.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", dt, "--n", str(args.n), "--size", str(args.size), "--iters", str(args.iters),
                   "--reps", str(args.reps)] + (["--trace-only"] if args.trace_only else [])
            done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.step_timeout, check=True)      # a failure or the limit ends the run
            results[dt] = json.loads(done.stdout.decode().strip().splitlines()[-1])
        if args.trace_only:
            return
        out = {"metric": "tgv_iteration_ms", "N": [args.size] * 3, "points": int(args.n), "iterations": args.iters, "results": results}
        out["value"] = results[args.dtypes.split(",")[0]]["ms_per_iteration"]["solver_eager"]
    if args.kernel_stats:
        fold_kernel_stats(out["results"], args.kernel_stats, args.size)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
