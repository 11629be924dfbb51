"""Low-rank plus sparse measurement: a framed operator and the L+S solver with the temporal DFT and momentum.  Cases,
operators and the timing loop are those of scripts/tvt_bench.py (`2d` = 256² × 32 frames, `3d` = 256³ × 8 frames; ComplexF32 and
ComplexF64; analytic spectra handed over with set_spectra_frames).

Times, in one process per case and element type and alternating rep by rep (hipEvent medians after warm-up), per iteration:
  * ToeplitzLPS.solve with check_every = 0 and tol = 0, eager          (all iterations enqueued, no host synchronisation)
  * the framed apply alone                                             (so that the part outside the apply = total − apply)
  * baseline: the same algorithm in torch around op(...), with torch.linalg.eigh of the K × K Gram matrix (float64) and torch.fft.fft
    along the frame axis
and asserts that the torch loop and the solver agree after the iterations (1e-11 ComplexF64 / 1e-4 ComplexF32 relative).

The kernels run only inside the solver, so their own times come from a kernel trace: `--worker DTYPE --case CASE --trace-only` runs three
eager solves and nothing else (the run to put under `rocprofv3 --kernel-trace --stats`), and `--kernel-stats CASE:DTYPE:FILE`
(repeatable, with `--fold-only` on an existing result) folds that run's kernel_stats.csv into the result as time per iteration and GB/s
over the kernels' algorithmic bytes, in arrays A = n · sizeof(complex T) of one frame: Gram 5 K (zL, zS, q, b in; g out), apply 5 K
(zL, g, L in; L, zL out), temporal 7 K (zS, g, S, zL in; S, zS, u out).  The eigen kernel (partial sums, Jacobi, P) moves no array: its
time stands alone, and at K = 32 it is the Jacobi's own line.

Every measurement runs in a child process of its own under a time limit; the first one that fails or runs out of time ends the run.
Writes one JSON document (--out) and prints it.
"""
import argparse
import csv
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tvt_bench as TB  # noqa: E402

BAR, CASES = TB.BAR, TB.CASES
KERNELS = (("glr_gram_kernel", 5), ("glr_eigen_kernel", 0), ("glr_apply_kernel", 5), ("tsparse_kernel", 7))


def gram(torch, M):
    """H = M̄ Mᵀ of the K × n matrix M (row c is frame c) in float64.  A K × K result with an inner dimension of millions runs as one
    tile of a matrix product; cutting the cells into 1024 slabs makes it a batched product whose results are added."""
    K, n = M.shape
    if n % 1024 or n < (1 << 20):
        return M.conj() @ M.T
    slabs = M.reshape(K, 1024, n // 1024).permute(1, 0, 2)
    return torch.matmul(slabs.conj(), slabs.transpose(1, 2)).sum(dim=0)


def torch_loop(torch, op, b, iters, nuc, l1, step):
    """The solver's algorithm in torch on stacked frames [K, ...]: one apply, the Gram matrix and its eigendecomposition in float64, an
    FFT along the frames, elementwise work, no host synchronisation."""
    K = b.shape[0]
    rootK = math.sqrt(K)
    L, S = torch.zeros_like(b), torch.zeros_like(b)
    zL, zS, q = L.clone(), S.clone(), torch.empty_like(b)
    tl, ts, t = step * nuc, step * l1, 1.0
    for _ in range(iters):
        t_next = 0.5 * (1.0 + math.sqrt(1.0 + 4.0 * t * t))
        beta, t = (t - 1.0) / t_next, t_next
        u = zL + zS
        op(tuple(u[c] for c in range(K)), out=tuple(q[c] for c in range(K)))
        g = step * (q - b)
        M = (zL - g).reshape(K, -1).to(torch.complex128)            # row c is frame c: C = Mᵀ
        lam, V = torch.linalg.eigh(gram(torch, M))                 # H = Cᴴ C
        sigma = torch.sqrt(torch.clamp(lam, min=0.0))
        f = torch.where(sigma > tl, 1.0 - tl / sigma, torch.zeros_like(sigma))
        P = (V * f) @ V.conj().T
        Lp = (P.T @ M).to(b.dtype).reshape(b.shape)                # (C P)ᵀ
        c = torch.fft.fft(zS - g, dim=0) / rootK
        mag = c.abs()
        c = c * torch.where(mag > ts, 1.0 - ts / mag, torch.zeros_like(mag))
        Sp = torch.fft.ifft(c, dim=0) * rootK
        zL, zS = Lp + beta * (Lp - L), Sp + beta * (Sp - S)
        L, S = Lp, Sp
    return L + S


def worker(dtype, args):
    import torch
    sys.path.insert(0, ROOT)
    from nufft_pkg import nufft
    iters = args.iters
    op, N, K, Z, dev, lmax = TB.operator(torch, nufft, args.case, dtype)
    g = torch.Generator(device=dev).manual_seed(0)
    shape = tuple(reversed(N))
    # two space-time components over noise, so that the Gram matrix is far from diagonal and the Jacobi has work to do
    b = torch.randn((K,) + shape, generator=g, device=dev, dtype=Z)
    for weight in (2.0, 1.0):
        b += weight * torch.randn((K,) + (1,) * len(N), generator=g, device=dev, dtype=Z) * torch.randn((1,) + shape, generator=g, device=dev, dtype=Z)
    bt = tuple(b[c] for c in range(K))
    step = 1.0 / (2.0 * 1.05 * lmax)
    M = b.reshape(K, -1).to(torch.complex128)
    nuc = 0.2 * math.sqrt(float(torch.linalg.eigvalsh(gram(torch, M))[-1]))      # a fifth of σ_max(C(b))
    del M
    l1 = 0.1 * float((torch.fft.fft(b, dim=0) / math.sqrt(K)).abs().max())      # a tenth of max|T b|
    sweeps = None
    if not args.trace_only:                                                      # the trace holds the solver's launches and nothing else
        low = nufft.GlobalLowRank(op)
        low.apply(bt, nuc)
        sweeps = low.last_sweeps()
        low.close()
    torch.cuda.empty_cache()
    x = torch.empty_like(b)
    xt = tuple(x[c] for c in range(K))
    q = torch.empty_like(b)
    qt = tuple(q[c] for c in range(K))
    arr = b[0].numel() * (16 if dtype == "c128" else 8)
    sol = nufft.ToeplitzLPS(op, nuc, l1, transform="dft", momentum=True, step=step, maxiter=iters, tol=0.0)
    assert sol.info().array_bytes == 5 * K * arr
    if args.trace_only:
        for _ in range(3):
            sol.solve(bt, out=xt)
        torch.cuda.synchronize()
        return {}
    routes = [("solver_eager", lambda: sol.solve(bt, out=xt)), ("apply_alone", lambda: [op.apply(bt, out=qt) for _ in range(iters)]),
              ("torch_loop", lambda: torch_loop(torch, op, b, iters, nuc, l1, step))]
    import time
    for name, fn in routes:                                                      # warm-up, with a line per route for the log
        t0 = time.time()
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        print(f"  {args.case} {dtype} warm-up of {name}: {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    assert sol.iterations == (iters,) * K, sol.iterations
    med, minmax = TB.measure(torch, routes, args.reps, {name: iters for name, _ in routes})
    outside = med["solver_eager"] - med["apply_alone"]
    sol.solve(bt, out=xt)
    base = torch_loop(torch, op, b, iters, nuc, l1, step)
    err = float(torch.linalg.vector_norm(base - x) / torch.linalg.vector_norm(x))
    hist = sol.history()
    r = {"frames": K, "array_mb": round(arr / 1e6, 1), "nuc": nuc, "l1": l1, "step": step, "jacobi_sweeps_on_b": sweeps,
         "ms_per_iteration": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": minmax,
         "outside_apply_ms": round(outside, 4), "outside_apply_share": round(outside / med["solver_eager"], 3),
         "outside_apply_gb_per_s": round(17 * K * arr / (outside * 1e-3) / 1e9, 1),
         "torch_loop_outside_apply_ms": round(med["torch_loop"] - med["apply_alone"], 4),
         "iteration_ratio_torch_over_solver": round(med["torch_loop"] / med["solver_eager"], 2),
         "outside_apply_ratio_torch_over_solver": round((med["torch_loop"] - med["apply_alone"]) / outside, 2),
         "torch_loop_vs_solver_rel_l2": err, "agreement_bar": BAR[dtype], "last_history_row": [float(v) for v in hist[-1]],
         "workspace_mb": round(sol.info().workspace_bytes / 1e6, 1), "operator_workspace_mb": round(op.info().workspace_bytes / 1e6, 1)}
    for k, v in med.items():
        print(f"  {args.case} {dtype} {k:14s} {v:8.4f} ms", file=sys.stderr)
    assert err <= BAR[dtype], f"the torch loop and the solver differ by {err:.3e} after {iters} iterations (bar {BAR[dtype]:g})"
    sol.close()
    op.close()
    return r


def fold_kernel_stats(result, path, iters):
    """Time per iteration of the four kernels from a rocprofv3 --kernel-trace --stats CSV (columns Name, Calls, AverageNs) of a
    --trace-only run (three solves), and the rate over their algorithmic bytes."""
    rows = list(csv.DictReader(open(path)))
    K, arr = result["frames"], result["array_mb"] * 1e6
    for kernel, per_frame in KERNELS:
        hit = [r for r in rows if kernel in r["Name"]]
        if not hit:
            continue
        calls = sum(int(r["Calls"]) for r in hit)
        ns = sum(float(r["AverageNs"]) * int(r["Calls"]) for r in hit) / (3 * iters)
        result[kernel] = {"calls": calls, "us_per_iteration": round(ns / 1e3, 2)}
        if per_frame:
            result[kernel].update({"algorithmic_arrays": per_frame * K, "gb_per_s": round(per_frame * K * arr / (ns * 1e-9) / 1e9, 1)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2d,3d")
    ap.add_argument("--case", default="2d", help=argparse.SUPPRESS)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dtypes", default="c64,c128")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds every child process may take")
    ap.add_argument("--trace-only", action="store_true", help="with --worker: three eager solves and nothing else")
    ap.add_argument("--kernel-stats", action="append", default=[], help="CASE:DTYPE:kernel_stats.csv of a --trace-only run under rocprofv3")
    ap.add_argument("--fold-only", action="store_true", help="only fold --kernel-stats into the existing --out")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lps_bench.json"))
    args = ap.parse_args()
    if args.worker:
        print(json.dumps(worker(args.worker, args)))
        return
    if args.fold_only:
        out = json.load(open(args.out))
    else:
        common = ["--iters", str(args.iters), "--reps", str(args.reps)]
        results = {}
        for case in args.cases.split(","):
            results[case] = {}
            for dt in args.dtypes.split(","):
                results[case][dt] = child(["--worker", dt, "--case", case] + common, args.step_timeout)
        first = results[args.cases.split(",")[0]][args.dtypes.split(",")[0]]
        out = {"metric": "lps_iteration_ms", "cases": {c: {"N": list(CASES[c][0]), "frames": CASES[c][1]} for c in results},
               "iterations": args.iters, "results": results, "value": first["ms_per_iteration"]["solver_eager"]}
    for spec in args.kernel_stats:
        case, dt, path = spec.split(":", 2)
        fold_kernel_stats(out["results"][case][dt], path, out["iterations"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def child(argv, limit):
    import subprocess
    done = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, stdout=subprocess.PIPE, timeout=limit, check=True)
    return json.loads(done.stdout.decode().strip().splitlines()[-1])


if __name__ == "__main__":
    main()
