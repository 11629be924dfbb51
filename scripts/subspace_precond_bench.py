"""Block-preconditioner measurement: N = 256³, fused paths, clustered points without density weights, the subspace basis of
the tests (exponential decays on 32 time points, the first K left singular vectors with a phase ramp, one time point per sample).

In one process, hipEvent medians after warm-up with the routes alternating rep by rep:
  1. one block M⁻¹ (K components as one vector), against K scalar M⁻¹ applies of the scalar object on an uncoupled operator of the same
     shape (the strided passes are the same work: that is the floor) and against the coupled operator's apply;
  2. one block-PCG iteration against one joint-CG iteration of the same solver with the preconditioner cleared (rtol = 0);
  3. time and iterations to rtol = 1e-6 with λ = 1e-3 max_e: joint CG against block PCG.
Writes one JSON object per (element type, K) into --out (default profiles/subspace_precond_bench.json) and prints it.
With --trace-only it runs three applies of each kind and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`; with
--kernel-stats FILE (the CSV of such a run) the dimension-1 kernels' rates are added from their algorithmic bytes:
  precond_block_lines_kernel      2 K complex lines + K² reals' worth of B per line id
  precond_lines_kernel            2 complex lines + 1 real line
  toeplitz_lines_coupled_kernel   2 K complex lines of N_1 kept modes + K² reals' worth of K_ab on 2 N_1 cells
"""
import argparse
import csv
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nufft_pkg import nufft  # noqa: E402


def clustered(n, D, T, dev, g):
    half = n // 2
    return tuple(torch.remainder(torch.cat([torch.rand(half, generator=g, device=dev, dtype=T) * (2 * math.pi),
                                            0.4 * torch.randn(n - half, generator=g, device=dev, dtype=T)]), 2 * math.pi).contiguous()
                 for _ in range(D))


def subspace_basis(K, n, Z, dev, g, nt=32):
    t = torch.arange(nt, dtype=torch.float64)
    D = torch.exp(-t[:, None] / torch.linspace(3.0, 40.0, 64, dtype=torch.float64)[None, :])
    U = torch.linalg.svd(D, full_matrices=False)[0][:, :K].to(torch.complex128)
    U = U * torch.exp(0.3j * t[:, None] * torch.arange(K, dtype=torch.float64)[None, :])
    tj = torch.randint(0, nt, (n,), generator=g, device=dev)
    return (math.sqrt(nt) * U.to(dev)[tj].T).to(Z).contiguous()


def timed(routes, reps, per):
    acc = {name: [] for name, _ in routes}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        for name, fn in routes:
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            acc[name].append(e0.elapsed_time(e1) / per)
    return {k: sorted(v)[len(v) // 2] for k, v in acc.items()}, {k: [round(min(v), 4), round(max(v), 4)] for k, v in acc.items()}


def kernel_rates(path, N, K, cb):
    """GB/s of the three dimension-1 kernels from a rocprofv3 --kernel-trace --stats CSV (columns Name, Calls, AverageNs, MinNs)."""
    lines = N * N
    byts = {"precond_block_lines_kernel": lines * (2 * K * N * cb + K * K * N * cb // 2),
            "precond_lines_kernel": lines * (2 * N * cb + N * cb // 2),
            "toeplitz_lines_coupled_kernel": 2 * N * 2 * N * (2 * K * N * cb + K * K * 2 * N * cb // 2)}
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for name, b in byts.items():
                if name + "<" in row["Name"] or row["Name"].startswith(name):
                    ns = float(row["MinNs"])                       # the average includes each kernel's first, cold call
                    out[name] = {"us": round(ns / 1e3, 1), "average_us": round(float(row["AverageNs"]) / 1e3, 1), "calls": int(row["Calls"]),
                                 "gb_per_s": round(b / ns, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e7, help="number of points")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", choices=("c128", "c64"), default="c128")
    ap.add_argument("--K", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--maxiter", type=int, default=1000)
    ap.add_argument("--skip-solves", action="store_true", help="parts 1 and 2 only")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subspace_precond_bench.json"))
    args = ap.parse_args()
    n, N, K, iters = int(args.n), (args.size,) * 3, args.K, args.iters
    Z, T = (torch.complex128, torch.float64) if args.dtype == "c128" else (torch.complex64, torch.float32)
    cb = 16 if args.dtype == "c128" else 8
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    pts = clustered(n, 3, T, dev, g)
    w = torch.full((n,), 1.0 / n, device=dev, dtype=T)
    phi = subspace_basis(K, n, Z, dev, g)
    plan = nufft.PlanNUFFT(Z, N, m=4, sigma=2.0, backend=nufft.ROCBackend(0), ntransforms=K)
    op = nufft.ToeplitzOperator(plan)
    assert op.path == "fused"
    op.set_points(pts, w, basis=phi)
    probe = nufft.ToeplitzPreconditioner(op, block=True)
    emax = probe.info().max_e
    probe.close()
    lam = 1e-3 * emax
    pc = nufft.ToeplitzPreconditioner(op, lam=lam, block=True)
    assert pc.path == "fused" and pc.coupled == K
    shape = tuple(reversed(N))
    b = tuple(torch.randn(shape, generator=g, device=dev, dtype=Z) for _ in range(K))
    x, q = tuple(torch.empty_like(v) for v in b), tuple(torch.empty_like(v) for v in b)
    # the floor: the scalar object on an uncoupled operator of the same shape, K components per call
    uop = nufft.ToeplitzOperator(plan)
    uop.set_points(pts, w)
    upc = nufft.ToeplitzPreconditioner(uop, lam=lam)
    assert upc.path == "fused"

    if args.trace_only:
        for _ in range(3):
            pc.apply(b, out=q)
            upc.apply(b, out=q)
            op.apply(b, out=q)
        torch.cuda.synchronize()
        return

    def many(fn):
        def run():
            for _ in range(iters):
                fn()
        return run

    routes = [("block_precond", many(lambda: pc.apply(b, out=q))), ("scalar_precond_K_components", many(lambda: upc.apply(b, out=q))),
              ("coupled_operator_apply", many(lambda: op.apply(b, out=q)))]
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    apply_ms, apply_mm = timed(routes, args.reps, iters)
    upc.close()
    uop.close()

    fixed = nufft.ToeplitzCG(op, maxiter=iters, rtol=0.0, lam=lam, precond=pc)
    fixed.solve(b, out=x)
    fixed.set_preconditioner(None)
    fixed.solve(b, out=x)
    torch.cuda.synchronize()
    acc = {"block_pcg_iteration": [], "joint_cg_iteration": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.reps):
        for name, p in (("block_pcg_iteration", pc), ("joint_cg_iteration", None)):
            fixed.set_preconditioner(p)
            e0.record()
            fixed.solve(b, out=x)
            e1.record()
            torch.cuda.synchronize()
            acc[name].append(e0.elapsed_time(e1) / iters)
    iter_ms = {k: sorted(v)[len(v) // 2] for k, v in acc.items()}
    iter_mm = {k: [round(min(v), 4), round(max(v), 4)] for k, v in acc.items()}
    fixed.close()

    arr = N[0] * N[1] * N[2] * cb
    block_bytes = K * 10 * arr + K * K * arr // 2          # per component five passes read and write N^D complex; B is read once
    i = pc.info()
    out = {"metric": "block_precond_apply_ms", "value": apply_ms["block_precond"], "dtype": args.dtype, "K": K, "N": N, "points": n,
           "lambda_over_max_e": 1e-3, "max_e": emax, "min_e": i.min_e, "floored_cells": pc.floored_cells,
           "apply_ms": {k: round(v, 4) for k, v in apply_ms.items()}, "apply_ms_min_max": apply_mm,
           "block_over_K_scalar": round(apply_ms["block_precond"] / apply_ms["scalar_precond_K_components"], 3),
           "block_over_operator": round(apply_ms["block_precond"] / apply_ms["coupled_operator_apply"], 3),
           "block_algorithmic_bytes": block_bytes, "block_gb_per_s": round(block_bytes / (apply_ms["block_precond"] * 1e-3) / 1e9, 1),
           "iteration_ms": {k: round(v, 4) for k, v in iter_ms.items()}, "iteration_ms_min_max": iter_mm,
           "pcg_over_cg_iteration": round(iter_ms["block_pcg_iteration"] / iter_ms["joint_cg_iteration"], 3),
           "precond_workspace_mb": round(i.workspace_bytes / 1e6, 1)}
    if args.kernel_stats:
        out["dimension_1_kernels"] = kernel_rates(args.kernel_stats, N[0], K, cb)

    if not args.skip_solves:
        def solve(precond):
            sol = nufft.ToeplitzCG(op, maxiter=args.maxiter, rtol=1e-6, lam=lam, precond=precond, check_every=5)
            sol.solve(b, out=x)                            # warm-up
            torch.cuda.synchronize()
            times = []
            for _ in range(3):
                e0.record()
                sol.solve(b, out=x)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            res = {"iterations": sol.iterations[0], "status": sol.status[0], "ms": round(sorted(times)[1], 2),
                   "ms_min_max": [round(min(times), 2), round(max(times), 2)], "residual": sol.residual[0]}
            sol.close()
            return res

        solves = {"joint_cg": solve(None), "block_pcg": solve(pc)}
        out["solves_rtol_1e-6"] = solves
        out["iteration_ratio"] = round(solves["joint_cg"]["iterations"] / max(solves["block_pcg"]["iterations"], 1), 3)
        out["time_ratio"] = round(solves["joint_cg"]["ms"] / solves["block_pcg"]["ms"], 3)
        out["fastest"] = min(solves, key=lambda k: solves[k]["ms"])
    plan.close()

    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    have = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            have = json.load(f)
    have[f"{args.dtype}_K{K}"] = out
    with open(args.out, "w") as f:
        json.dump(have, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
