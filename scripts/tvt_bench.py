"""Dynamic-imaging measurement: a framed operator (one multiplier per frame) and the primal-dual solver with the temporal
term alone, non-periodic.  Cases: `3d` = 256³ × 8 frames, `2d` = 256² × 32 frames; ComplexF32 and ComplexF64.  The frames' spectra are
analytic (T_c[d] = Π a_c^|d|, a_c from 0.15 to 0.45), formed on the device and handed over with set_spectra_frames.

Times, in one process per case and element type and alternating rep by rep (hipEvent medians after warm-up), per iteration:
  * ToeplitzTV.solve with check_every = 0 and tol = 0, eager            (all iterations enqueued, no host synchronisation)
  * the framed apply alone                                              (so that the part outside the apply = total − apply)
  * baseline: the same algorithm written in torch (slices of a stacked tensor) around op(...)
and checks that the torch loop and the solver agree after the iterations (1e-11 ComplexF64 / 1e-4 ComplexF32 relative).

The framed apply against the plain one (K components, one shared multiplier): `--apply-rounds R` runs each in R child processes of its
own, alternating, and records the medians and their ratio.  `--apply-root DIR` takes the plain apply from another checkout of the
project (the commit before the frames, for instance) instead of this one.

The two temporal kernels run only inside the solver, so their own times come from a kernel trace: `--worker DTYPE --case CASE
--trace-only` runs three eager solves and nothing else (the run to put under `rocprofv3 --kernel-trace --stats`), and `--kernel-stats
CASE:DTYPE:FILE` (repeatable, with `--fold-only` on an existing result) folds that run's kernel_stats.csv into the result as time per
iteration and GB/s over the kernels' algorithmic bytes, in arrays A = n · sizeof(complex T) over all K frames: primal 7 K − 2 (x, q, b,
z_c, z_{c−1} in; x, q out; frame 0 has no z_{−1}, frame K − 1 no z_c), dual 6 (K − 1) + 2 (x̄_c, x̄_{c+1}, x⁺_c, x⁺_{c+1}, z_c in; z_c out; the
last frame only passes its z through).

Every measurement runs in a child process of its own under a time limit; the first one that fails or runs out of time ends the run.
Writes one JSON document (--out) and prints it.
"""
import argparse
import csv
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = {"c128": 1e-11, "c64": 1e-4}
CASES = {"3d": ((256, 256, 256), 8), "2d": ((256, 256), 32)}


def frame_a(c, K):
    return 0.15 + 0.3 * c / (K - 1)


def spectrum(torch, N, a, Z, dev):
    """T[d] = Π a^|d_dim| on the 2N mode set of an fftshift = False plan (tensor shape reversed, dimension 1 last)."""
    T = None
    for dim, n in enumerate(N):
        j = torch.arange(2 * n, device=dev, dtype=torch.float64)
        line = a ** torch.where(j < n, j, 2 * n - j)
        shape = [1] * len(N)
        shape[len(N) - 1 - dim] = 2 * n
        T = line.reshape(shape) if T is None else T * line.reshape(shape)
    return T.to(Z).contiguous()


def operator(torch, nufft, case, dtype, framed=True):
    N, K = CASES[case]
    Z = torch.complex128 if dtype == "c128" else torch.complex64
    dev = torch.device("cuda", 0)
    plan = nufft.PlanNUFFT(Z, N, m=4, sigma=2.0, backend=nufft.ROCBackend(0), ntransforms=K)
    op = nufft.ToeplitzOperator(plan)
    plan.close()
    assert op.path == "fused"
    if framed:
        # one spectrum at a time would need its own entry point: K spectra of (2N)^D live next to each other for the build
        op.set_spectra_frames([spectrum(torch, N, frame_a(c, K), Z, dev) for c in range(K)])
    else:
        op.set_spectrum(spectrum(torch, N, frame_a(K - 1, K), Z, dev))
    torch.cuda.empty_cache()
    lmax = ((1 + frame_a(K - 1, K)) / (1 - frame_a(K - 1, K))) ** len(N)      # an upper bound over the frames
    return op, N, K, Z, dev, lmax


def torch_loop(torch, op, b, iters, tv_t, step, sigma):
    """The solver's algorithm in torch on stacked frames [K, ...]: one apply, slices for the differences, elementwise work, no host
    synchronisation.  Non-periodic: z[K − 1] stays zero."""
    K = b.shape[0]
    x, z, q = torch.zeros_like(b), torch.zeros_like(b), torch.empty_like(b)
    change = None
    for _ in range(iters):
        op(tuple(x[c] for c in range(K)), out=tuple(q[c] for c in range(K)))
        div = -z
        div[1:] += z[:-1]
        xp = x - step * (q - b + div)
        d_ = xp - x
        xbar = xp + d_
        v = z.clone()
        v[:-1] += sigma * (xbar[1:] - xbar[:-1])
        nrm = torch.sqrt(v.real ** 2 + v.imag ** 2)
        z = v * torch.where(nrm > tv_t, tv_t / nrm, torch.ones_like(nrm))
        change = torch.linalg.vector_norm(d_) / torch.linalg.vector_norm(xp)
        x = xp
    return x, change


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
    iters = args.iters
    op, N, K, Z, dev, lmax = operator(torch, nufft, args.case, dtype)
    g = torch.Generator(device=dev).manual_seed(0)
    b = torch.randn((K,) + tuple(reversed(N)), generator=g, device=dev, dtype=Z)
    bt = tuple(b[c] for c in range(K))
    step = 1.0 / (1.05 * lmax)
    tv_t = 0.1 * float(b.abs().max())
    x = torch.empty_like(b)
    xt = tuple(x[c] for c in range(K))
    q = torch.empty_like(b)
    qt = tuple(q[c] for c in range(K))
    cb = 16 if dtype == "c128" else 8
    arr = b[0].numel() * cb
    sol = nufft.ToeplitzTV(op, tv_t=tv_t, step=step, maxiter=iters, tol=0.0)
    assert not sol.spatial and sol.info().array_bytes == 2 * K * arr
    if args.trace_only:
        for _ in range(3):
            sol.solve(bt, out=xt)
        torch.cuda.synchronize()
        return {}
    routes = [("solver_eager", lambda: sol.solve(bt, out=xt)), ("apply_alone", lambda: [op.apply(bt, out=qt) for _ in range(iters)]),
              ("torch_loop", lambda: torch_loop(torch, op, b, iters, tv_t, step, sol.sigma))]
    for _, fn in routes:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    assert sol.iterations == (iters,) * K, sol.iterations
    med, minmax = measure(torch, routes, args.reps, {name: iters for name, _ in routes})
    outside = med["solver_eager"] - med["apply_alone"]
    sol.solve(bt, out=xt)
    base, _ = torch_loop(torch, op, b, iters, tv_t, step, sol.sigma)
    err = float(torch.linalg.vector_norm(base - x) / torch.linalg.vector_norm(x))
    arrays = (7 * K - 2) + (6 * (K - 1) + 2)
    r = {"frames": K, "array_mb": round(arr / 1e6, 1), "tv_t": tv_t, "step": step, "sigma": sol.sigma,
         "ms_per_iteration": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": minmax,
         "outside_apply_ms": round(outside, 4), "outside_apply_share": round(outside / med["solver_eager"], 3),
         "outside_apply_gb_per_s": round(arrays * arr / (outside * 1e-3) / 1e9, 1),
         "torch_loop_outside_apply_ms": round(med["torch_loop"] - med["apply_alone"], 4),
         "iteration_ratio_torch_over_solver": round(med["torch_loop"] / med["solver_eager"], 2),
         "outside_apply_ratio_torch_over_solver": round((med["torch_loop"] - med["apply_alone"]) / outside, 2),
         "torch_loop_vs_solver_rel_l2": err, "agreement_bar": BAR[dtype], "workspace_mb": round(sol.info().workspace_bytes / 1e6, 1),
         "operator_workspace_mb": round(op.info().workspace_bytes / 1e6, 1)}
    for k, v in med.items():
        print(f"  {args.case} {dtype} {k:14s} {v:8.4f} ms", file=sys.stderr)
    assert err <= BAR[dtype], f"the torch loop and the solver differ by {err:.3e} after {iters} iterations (bar {BAR[dtype]:g})"
    sol.close()
    op.close()
    return r


def apply_worker(dtype, args):
    """Median time of one apply of the K components: `framed` (this checkout) or `plain` (one shared multiplier; --apply-root)."""
    import torch
    framed = args.apply_worker == "framed"
    sys.path.insert(0, ROOT if framed or not args.apply_root else os.path.abspath(args.apply_root))
    from nufft_pkg import nufft
    op, N, K, Z, dev, _ = operator(torch, nufft, args.case, dtype, framed=framed)
    g = torch.Generator(device=dev).manual_seed(0)
    b = torch.randn((K,) + tuple(reversed(N)), generator=g, device=dev, dtype=Z)
    bt, q = tuple(b[c] for c in range(K)), torch.empty_like(b)
    qt = tuple(q[c] for c in range(K))
    fn = lambda: [op.apply(bt, out=qt) for _ in range(args.iters)]      # noqa: E731
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    med, minmax = measure(torch, [("apply", fn)], args.reps, {"apply": args.iters})
    return {"ms": med["apply"], "min_max": minmax["apply"]}


def fold_kernel_stats(result, path, iters):
    """Time per iteration of the two temporal kernels from a rocprofv3 --kernel-trace --stats CSV (columns Name, Calls, AverageNs) of a
    --trace-only run (three solves), and the rate over their algorithmic bytes."""
    rows = list(csv.DictReader(open(path)))
    K, arr = result["frames"], result["array_mb"] * 1e6
    for kernel, arrays in (("tvt_primal_kernel", 7 * K - 2), ("tvt_dual_kernel", 6 * (K - 1) + 2)):
        hit = [r for r in rows if kernel in r["Name"]]
        if not hit:
            continue
        calls = sum(int(r["Calls"]) for r in hit)
        ns = sum(float(r["AverageNs"]) * int(r["Calls"]) for r in hit) / (3 * iters)
        result[kernel] = {"calls": calls, "launches_per_iteration": calls // (3 * iters), "us_per_iteration": round(ns / 1e3, 2),
                          "algorithmic_arrays": arrays, "gb_per_s": round(arrays * arr / (ns * 1e-9) / 1e9, 1)}


def child(argv, limit):
    done = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, stdout=subprocess.PIPE, timeout=limit, check=True)
    return json.loads(done.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="3d,2d")
    ap.add_argument("--case", default="3d", help=argparse.SUPPRESS)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dtypes", default="c64,c128")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds every child process may take")
    ap.add_argument("--apply-rounds", type=int, default=3, help="child processes per side of the framed / plain apply comparison (0: skip it)")
    ap.add_argument("--apply-root", default=None, help="another checkout of the project whose plain apply is the other side")
    ap.add_argument("--trace-only", action="store_true", help="with --worker: three eager solves and nothing else")
    ap.add_argument("--kernel-stats", action="append", default=[], help="CASE:DTYPE:kernel_stats.csv of a --trace-only run under rocprofv3")
    ap.add_argument("--fold-only", action="store_true", help="only fold --kernel-stats into the existing --out")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--apply-worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tvt_bench.json"))
    args = ap.parse_args()
    if args.worker:
        print(json.dumps(apply_worker(args.worker, args) if args.apply_worker else worker(args.worker, args)))
        return
    if args.fold_only:
        out = json.load(open(args.out))
    else:
        common = ["--iters", str(args.iters), "--reps", str(args.reps)]
        results = {}
        for case in args.cases.split(","):
            results[case] = {}
            for dt in args.dtypes.split(","):
                r = child(["--worker", dt, "--case", case] + common, args.step_timeout)
                sides = {"plain": [], "framed": []}
                for _ in range(args.apply_rounds):
                    for side in ("plain", "framed"):
                        extra = ["--apply-root", args.apply_root] if args.apply_root and side == "plain" else []
                        sides[side].append(child(["--worker", dt, "--case", case, "--apply-worker", side] + common + extra, args.step_timeout)["ms"])
                if args.apply_rounds:
                    med = {k: sorted(v)[len(v) // 2] for k, v in sides.items()}
                    r["apply_ms"] = {"plain_shared_multiplier": [round(v, 4) for v in sides["plain"]], "framed": [round(v, 4) for v in sides["framed"]],
                                     "plain_from": "another checkout" if args.apply_root else "this build",
                                     "ratio_framed_over_plain": round(med["framed"] / med["plain"], 4)}
                results[case][dt] = r
        first = results[args.cases.split(",")[0]][args.dtypes.split(",")[0]]
        out = {"metric": "tvt_iteration_ms", "cases": {c: {"N": list(CASES[c][0]), "frames": CASES[c][1]} for c in results},
               "iterations": args.iters, "results": results, "value": first["ms_per_iteration"]["solver_eager"]}
    for spec in args.kernel_stats:
        case, dt, path = spec.split(":", 2)
        fold_kernel_stats(out["results"][case][dt], path, out["iterations"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
