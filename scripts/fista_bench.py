"""FISTA solver measurement: N = 256³, fused apply path, 3 wavelet levels, 1e7 uniform points, ComplexF32 and ComplexF64,
"db2" and "haar".

Times, in one process and alternating rep by rep (hipEvent medians after warm-up), per iteration:
  * ToeplitzFISTA.solve with check_every = 0 and tol = 0, eager        (all iterations enqueued, no host synchronisation)
  * the apply alone                                                     (so that the share outside the apply = total − apply)
  * baseline: the same algorithm written in torch around op(...), with a periodic Haar transform built from strided slices — the only
    wavelet a torch user can write without the library's transform
and, per launch, the finest-level analysis and synthesis kernels (a one-level WaveletTransform's forward / inverse: one launch each),
as GB/s over their algorithmic bytes (the array read once and written once).  Writes one JSON document (--out) and prints it.
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nufft_pkg import nufft  # noqa: E402

S = 1.0 / math.sqrt(2.0)


def _corner(shape, level):
    return tuple(slice(0, s >> level) for s in shape)


def haar_forward(x, levels):
    out = x.clone()
    for lev in range(levels):
        sub = out[_corner(x.shape, lev)]
        for ax in range(x.dim()):
            idx = [slice(None)] * x.dim()
            idx[ax] = slice(0, None, 2)
            ev = sub[tuple(idx)]
            idx[ax] = slice(1, None, 2)
            od = sub[tuple(idx)]
            sub = torch.cat([(ev + od) * S, (ev - od) * S], dim=ax)
        out[_corner(x.shape, lev)] = sub
    return out


def haar_inverse(c, levels):
    out = c.clone()
    for lev in reversed(range(levels)):
        sub = out[_corner(c.shape, lev)]
        for ax in range(c.dim()):
            h = sub.shape[ax] // 2
            lo, hi = sub.narrow(ax, 0, h), sub.narrow(ax, h, h)
            sub = torch.stack([(lo + hi) * S, (lo - hi) * S], dim=ax + 1).flatten(ax, ax + 1)
        out[_corner(c.shape, lev)] = sub
    return out


def torch_loop(op, b, iters, levels, l1, step, lam=0.0):
    """The solver's algorithm in torch: one apply, elementwise work, the Haar transform from slices, no host synchronisation."""
    x = torch.zeros_like(b)
    z = torch.zeros_like(b)
    thr = step * l1
    t = 1.0
    change = None
    for _ in range(iters):
        t_next = 0.5 * (1.0 + math.sqrt(1.0 + 4.0 * t * t))
        beta = (t - 1.0) / t_next
        t = t_next
        v = z - step * (op(z) + lam * z - b)
        c = haar_forward(v, levels)
        keep = c[_corner(c.shape, levels)].clone()
        mag = c.abs()
        c = c * torch.where(mag > thr, 1.0 - thr / mag, torch.zeros_like(mag))
        c[_corner(c.shape, levels)] = keep
        xp = haar_inverse(c, levels)
        d = xp - x
        z = xp + beta * d
        change = torch.linalg.vector_norm(d) / torch.linalg.vector_norm(xp)
        x = xp
    return x, change


def measure(routes, reps, per):
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


def run(dtype, args):
    n, N, iters, levels = int(args.n), (args.size,) * 3, args.iters, args.levels
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
    x = torch.empty_like(b)
    q = torch.empty_like(b)
    arr = N[0] * N[1] * N[2] * cb
    results = {}
    for wavelet in ("db2", "haar"):
        one = nufft.WaveletTransform(op, wavelet, 1)
        full = nufft.WaveletTransform(op, wavelet, levels)
        l1 = 0.3 * float(full.forward(b).abs().max())
        sol = nufft.ToeplitzFISTA(op, wavelet=wavelet, levels=levels, l1=l1, step=step, maxiter=iters, tol=0.0)
        c1 = torch.empty_like(b)
        routes = [("solver_eager", lambda: sol.solve(b, out=x)), ("apply_alone", lambda: [op.apply(b, out=q) for _ in range(iters)]),
                  ("finest_analysis", lambda: [one.forward(b, out=c1) for _ in range(iters)]),
                  ("finest_synthesis", lambda: [one.inverse(c1, out=q) for _ in range(iters)]),
                  ("forward_all_levels", lambda: [full.forward(b, out=c1) for _ in range(iters)]),
                  ("inverse_all_levels", lambda: [full.inverse(c1, out=q) for _ in range(iters)])]
        if wavelet == "haar":
            routes.append(("torch_loop", lambda: torch_loop(op, b, iters, levels, l1, step)))
        for _, fn in routes:
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        assert sol.iterations == (iters,), sol.iterations
        med, minmax = measure(routes, args.reps, {name: iters for name, _ in routes})
        outside = med["solver_eager"] - med["apply_alone"]
        r = {"ms_per_iteration": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": minmax,
             "outside_apply_ms": round(outside, 4), "outside_apply_share": round(outside / med["solver_eager"], 3),
             "finest_analysis_gb_per_s": round(2 * arr / (med["finest_analysis"] * 1e-3) / 1e9, 1),
             "finest_synthesis_gb_per_s": round(2 * arr / (med["finest_synthesis"] * 1e-3) / 1e9, 1),
             "l1": l1, "step": step, "workspace_mb": round(sol.info().workspace_bytes / 1e6, 1)}
        if wavelet == "haar":
            sol.solve(b, out=x)
            base, _ = torch_loop(op, b, iters, levels, l1, step)
            r["torch_loop_vs_solver_rel_l2"] = float(torch.linalg.vector_norm(base - x) / torch.linalg.vector_norm(x))
            r["torch_loop_outside_apply_ms"] = round(med["torch_loop"] - med["apply_alone"], 4)
            r["iteration_ratio_torch_over_solver"] = round(med["torch_loop"] / med["solver_eager"], 2)
            r["outside_apply_ratio_torch_over_solver"] = round((med["torch_loop"] - med["apply_alone"]) / outside, 2)
            del base
        results[wavelet] = r
        for k, v in med.items():
            print(f"  {dtype} {wavelet:5s} {k:20s} {v:8.4f} ms")
        sol.close()
        one.close()
        full.close()
    op.close()
    return {"lambda_max_estimate": lmax, "array_mb": round(arr / 1e6, 1), "wavelets": results}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e7, help="number of points the operator is built from")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dtypes", default="c64,c128")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fista_bench.json"))
    args = ap.parse_args()
    out = {"metric": "fista_iteration_ms", "N": [args.size] * 3, "points": int(args.n), "levels": args.levels, "iterations": args.iters,
           "results": {dt: run(dt, args) for dt in args.dtypes.split(",")}}
    out["value"] = out["results"][args.dtypes.split(",")[0]]["wavelets"]["db2"]["ms_per_iteration"]["solver_eager"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
