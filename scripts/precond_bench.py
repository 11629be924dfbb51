"""Preconditioner measurement: N = 256³, fused paths, clustered points without density weights.

In one process, hipEvent medians after warm-up with the routes alternating rep by rep:
  1. one M⁻¹ apply per component on the fused path, against the same operator's apply and against the dense preconditioner path
     (an operator and preconditioner created from a plan with NUFFT_TOEPLITZ_FUSED=0);
  2. one PCG iteration against one plain CG iteration of the same solver with the preconditioner cleared (20 iterations, rtol = 0);
  3. time and iterations to rtol = 1e-6 with λ = 1e-3 max e on the point set (half uniform, half N(0, 0.4²) folded, Np = 1e7,
     w = 1/Np): plain CG, PCG, and plain CG on the operator built with density_weights.
Writes one JSON object per element type into --out (default profiles/precond_bench.json) and prints it.
With --trace-only it runs three applies of M⁻¹ and three PCG iterations and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats`.
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e7, help="number of points")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", choices=("c128", "c64"), default="c128")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--maxiter", type=int, default=600)
    ap.add_argument("--skip-solves", action="store_true", help="parts 1 and 2 only")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precond_bench.json"))
    args = ap.parse_args()
    n, N, iters = int(args.n), (args.size,) * 3, args.iters
    Z, T = (torch.complex128, torch.float64) if args.dtype == "c128" else (torch.complex64, torch.float32)
    cb = 16 if args.dtype == "c128" else 8
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    pts = clustered(n, 3, T, dev, g)
    w = torch.full((n,), 1.0 / n, device=dev, dtype=T)
    plan = nufft.PlanNUFFT(Z, N, m=4, sigma=2.0, backend=nufft.ROCBackend(0))
    op = nufft.ToeplitzOperator(plan)
    assert op.path == "fused"
    op.set_points(pts, w)
    emax = nufft.ToeplitzPreconditioner(op).info().max_e
    lam = 1e-3 * emax
    pc = nufft.ToeplitzPreconditioner(op, lam=lam)
    assert pc.path == "fused"
    shape = tuple(reversed(N))
    b = torch.randn(shape, generator=g, device=dev, dtype=Z)
    x, q = torch.empty_like(b), torch.empty_like(b)
    fixed = nufft.ToeplitzCG(op, maxiter=iters, rtol=0.0, lam=lam, precond=pc)

    if args.trace_only:
        for _ in range(3):
            pc.apply(b, out=q)
        nufft.ToeplitzCG(op, maxiter=3, rtol=0.0, lam=lam, precond=pc).solve(b, out=x)
        torch.cuda.synchronize()
        return

    # 1. the apply of M⁻¹: fused, dense, and the operator's own apply
    dplan = nufft.PlanNUFFT(Z, N, m=4, sigma=2.0, backend=nufft.ROCBackend(0), options={"NUFFT_TOEPLITZ_FUSED": 0})
    dop = nufft.ToeplitzOperator(dplan)
    dop.set_points(pts, w)
    dpc = nufft.ToeplitzPreconditioner(dop, lam=lam)
    assert dpc.path == "dense"
    dplan.close()
    ref = dpc.apply(b)
    paths_agree = float(torch.linalg.vector_norm(pc.apply(b) - ref) / torch.linalg.vector_norm(ref))
    del ref

    def many(fn):
        def run():
            for _ in range(iters):
                fn()
        return run

    routes = [("precond_fused", many(lambda: pc.apply(b, out=q))), ("precond_dense", many(lambda: dpc.apply(b, out=q))),
              ("operator_apply", many(lambda: op.apply(b, out=q)))]
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    apply_ms, apply_mm = timed(routes, args.reps, iters)
    dpc.close()
    dop.close()

    # 2. one iteration with and without the preconditioner, the same solver object
    def run_pcg():
        fixed.solve(b, out=x)

    def run_cg():
        fixed.solve(b, out=x)

    fixed.solve(b, out=x)
    torch.cuda.synchronize()
    assert fixed.iterations == (iters,)
    pcg_ms, pcg_mm = timed([("pcg_iteration", run_pcg)], args.reps, iters)
    fixed.set_preconditioner(None)
    fixed.solve(b, out=x)
    torch.cuda.synchronize()
    cg_ms, cg_mm = timed([("cg_iteration", run_cg)], args.reps, iters)
    # ... and alternating, which is what the medians reported are taken from
    acc = {"pcg_iteration": [], "cg_iteration": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.reps):
        for name, p in (("pcg_iteration", pc), ("cg_iteration", None)):
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
    out = {"metric": "precond_apply_ms", "value": apply_ms["precond_fused"], "dtype": args.dtype, "N": N, "points": n, "lambda_over_max_e": 1e-3,
           "max_e": emax, "min_e": pc.info().min_e,
           "apply_ms": {k: round(v, 4) for k, v in apply_ms.items()}, "apply_ms_min_max": apply_mm,
           "precond_over_operator": round(apply_ms["precond_fused"] / apply_ms["operator_apply"], 3),
           "fused_vs_dense_rel_l2": paths_agree,
           "precond_algorithmic_bytes": 10 * arr + arr // 2,        # five passes read and write N^D complex; m is read once
           "precond_gb_per_s": round((10 * arr + arr // 2) / (apply_ms["precond_fused"] * 1e-3) / 1e9, 1),
           "iteration_ms": {k: round(v, 4) for k, v in iter_ms.items()}, "iteration_ms_min_max": iter_mm,
           "iteration_ms_back_to_back": {"pcg_iteration": round(pcg_ms["pcg_iteration"], 4), "cg_iteration": round(cg_ms["cg_iteration"], 4)},
           "pcg_over_cg_iteration": round(iter_ms["pcg_iteration"] / iter_ms["cg_iteration"], 3),
           "precond_workspace_mb": round(pc.info().workspace_bytes / 1e6, 1)}

    # 3. to rtol = 1e-6: plain CG, PCG, plain CG with density weights
    if not args.skip_solves:
        def solve(operator, precond):
            sol = nufft.ToeplitzCG(operator, maxiter=args.maxiter, rtol=1e-6, lam=lam, precond=precond, check_every=5)
            sol.solve(b, out=x)                            # warm-up
            torch.cuda.synchronize()
            times = []
            for _ in range(3):
                e0.record()
                sol.solve(b, out=x)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            res = {"iterations": sol.iterations[0], "status": sol.status[0], "ms": round(sorted(times)[1], 2), "residual": sol.residual[0]}
            sol.close()
            return res

        solves = {"cg_uniform_weights": solve(op, None), "pcg_uniform_weights": solve(op, pc)}
        wd = nufft.density_weights(plan, pts)
        op.set_points(pts, wd)
        solves["cg_density_weights"] = solve(op, None)
        out["solves_rtol_1e-6"] = solves
        out["fastest"] = min(solves, key=lambda k: solves[k]["ms"])
    plan.close()

    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    have = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            have = json.load(f)
    have[args.dtype] = out
    with open(args.out, "w") as f:
        json.dump(have, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
