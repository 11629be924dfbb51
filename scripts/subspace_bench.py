"""Coupled-component (subspace) Toeplitz normal operator measurement: N = 256³, ComplexF32 and ComplexF64, K = 2 and 4
components, without coil maps and with 8.

Times, in one process and alternating rep by rep (hipEvent medians after warm-up), per coupled apply and per CG iteration:
  * composed      the only route without the operator: exec_type2 of the K components, the mix Σ_b w conj(φ_a) φ_b v_b at the samples
                  in torch, exec_type1 (Np = 1e7; without maps)
  * plain         K plain fused applies (an uncoupled operator of K components): the floor set by the strided passes, which the
                  coupled apply runs unchanged
  * coupled       the coupled apply, and ToeplitzCG on it (joint scalars) against ToeplitzCG on the uncoupled operator
The spectra are analytic (Poisson kernels; the cross blocks a phase-shifted, damped copy): the cost of an apply does not depend on the
values.  The dimension-1 kernel alone is timed by the profiler: `--trace-only` runs a few applies of each kind and nothing else (the
run to put under `rocprofv3 --kernel-trace --stats`), and `--kernel-stats FILE [--fold-only]` folds that run's kernel_stats.csv into the result
as time and achieved bandwidth over the kernels' algorithmic bytes.  Writes profiles/subspace_bench.json and prints one JSON line per
configuration.
"""
import argparse
import csv
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nufft_pkg import nufft  # noqa: E402
from sense_bench import poisson_spectrum, smooth_maps  # noqa: E402


def line_kernel_bytes(N, K, cb, rb):
    """Algorithmic bytes of the dimension-1 kernels per apply: per line id (K + K (K − 1)) · 2N_1 reals of multiplier and 2 · K · N_1
    complex of data (coupled); 2N_1 reals and 2 N_1 complex per line (plain, K launches)."""
    n1, n2, n3 = N
    lines = 2 * n2 * 2 * n3
    return {"coupled": lines * (K * K * 2 * n1 * rb + 2 * K * n1 * cb), "plain": K * lines * (2 * n1 * rb + 2 * n1 * cb)}


def spectra(N, K, Z, dev):
    """K (K + 1) / 2 spectra in pair order: a Poisson kernel on the diagonal, a damped copy shifted by one mode off it (Hermitian as a
    family by construction of the multipliers: only the pairs a <= b are given)."""
    base = poisson_spectrum(N, 0.15, Z, dev)
    out = []
    for a in range(K):
        for b in range(a, K):
            out.append(base if a == b else (0.3 / (b - a)) * torch.roll(base, shifts=b - a, dims=-1))
    return out


def measure(dtype, size, K, ncoils, reps, cg_iters, npoints, trace_only):
    N = (size,) * 3
    Z = torch.complex128 if dtype == "c128" else torch.complex64
    T = torch.float64 if dtype == "c128" else torch.float32
    rb = 8 if dtype == "c128" else 4
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    us = tuple(torch.randn(tuple(reversed(N)), generator=g, device=dev, dtype=Z) for _ in range(K))
    plan = nufft.PlanNUFFT(Z, N, m=4, sigma=2.0, ntransforms=K, backend=nufft.ROCBackend(0))

    def operator():
        op = nufft.ToeplitzOperator(plan)
        assert op.path == "fused"
        return op

    sp = spectra(N, K, Z, dev)
    coupled, plain = operator().set_spectra(sp), operator().set_spectrum(sp[0])
    del sp
    assert coupled.coupled and not plain.coupled
    if ncoils:
        maps = smooth_maps(ncoils, us[0].shape, Z, dev)
        coupled.set_maps(maps)
        plain.set_maps(maps)
    out_c, out_p = tuple(torch.empty_like(u) for u in us), tuple(torch.empty_like(u) for u in us)
    routes = [("coupled_apply", lambda: coupled.apply(us, out=out_c)), ("plain_apply", lambda: plain.apply(us, out=out_p))]
    if trace_only:
        for _ in range(3):
            for _, fn in routes:
                fn()
        torch.cuda.synchronize()
        return None

    if not ncoils:          # the composed route has no coil maps: compared without them
        pts = tuple((torch.rand(npoints, generator=g, device=dev, dtype=T) * (2 * torch.pi)).contiguous() for _ in N)
        w = torch.rand(npoints, generator=g, device=dev, dtype=T) + 0.1
        phi = torch.randn((K, npoints), generator=g, device=dev, dtype=Z)
        nufft.set_points(plan, pts)
        vs = tuple(torch.empty(npoints, dtype=Z, device=dev) for _ in range(K))
        mixed = tuple(torch.empty(npoints, dtype=Z, device=dev) for _ in range(K))
        out_x = tuple(torch.empty_like(u) for u in us)

        def composed():
            nufft.exec_type2(vs, plan, us)
            y = sum(phi[b] * vs[b] for b in range(K))
            for a in range(K):
                torch.mul(w * phi[a].conj(), y, out=mixed[a])
            nufft.exec_type1(out_x, plan, mixed)

        routes.append(("composed_apply", composed))
    bs = tuple(torch.randn(us[0].shape, generator=g, device=dev, dtype=Z) for _ in range(K))
    x_c, x_p = tuple(torch.empty_like(b) for b in bs), tuple(torch.empty_like(b) for b in bs)
    sol_c = nufft.ToeplitzCG(coupled, maxiter=cg_iters, rtol=0.0, lam=0.0, check_every=0)
    sol_p = nufft.ToeplitzCG(plain, maxiter=cg_iters, rtol=0.0, lam=0.0, check_every=0)
    routes += [("cg_coupled", lambda: sol_c.solve(bs, out=x_c)), ("cg_plain", lambda: sol_p.solve(bs, out=x_p))]
    for _ in range(2):
        for _, fn in routes:
            fn()
    torch.cuda.synchronize()
    acc = {name: [] for name, _ in routes}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        for name, fn in routes:
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            acc[name].append(e0.elapsed_time(e1))
    med = {k: sorted(x)[len(x) // 2] for k, x in acc.items()}
    spread = {k: [min(x), max(x)] for k, x in acc.items()}
    out = {"metric": "subspace_apply_ms", "value": med["coupled_apply"], "dtype": dtype, "N": N, "K": K, "ncoils": ncoils, "cg_iterations": cg_iters,
           "npoints_composed": npoints if not ncoils else None,
           "ms": {k: round(x, 4) for k, x in med.items()}, "ms_min_max": {k: [round(a, 4), round(b, 4)] for k, (a, b) in spread.items()},
           "ms_per_cg_iteration": {"coupled": round(med["cg_coupled"] / cg_iters, 4), "plain": round(med["cg_plain"] / cg_iters, 4)},
           "ratio_coupled_over_plain": round(med["coupled_apply"] / med["plain_apply"], 3),
           "ratio_coupled_over_composed": round(med["coupled_apply"] / med["composed_apply"], 4) if "composed_apply" in med else None,
           "line_kernel_bytes": line_kernel_bytes(N, K, 2 * rb, rb),
           "workspace_mb": {"coupled": round(coupled.info().workspace_bytes / 1e6, 1), "plain": round(plain.info().workspace_bytes / 1e6, 1)}}
    for k in acc:
        print(f"  {dtype} K={K} coils={ncoils} {k:16s} {med[k]:9.3f} ms   (min {spread[k][0]:.3f}, max {spread[k][1]:.3f})", flush=True)
    for s in (sol_c, sol_p):
        s.close()
    for op in (coupled, plain):
        op.close()
    plan.close()
    return out


def fold_kernel_stats(results, path, size):
    """Average time of the two dimension-1 kernels from a kernel_stats.csv, per (element type, K), and the bandwidth they reach over
    their algorithmic bytes."""
    rows = list(csv.DictReader(open(path)))
    for r in results:
        t = "double" if r["dtype"] == "c128" else "float"
        tier = 2 if r["K"] <= 2 else 4 if r["K"] <= 4 else 8 if r["K"] <= 8 else 16
        pat = {"coupled": rf"toeplitz_lines_coupled_kernel<{t}, {2 * size}, {tier},", "plain": rf"toeplitz_lines_kernel<{t}, {2 * size},"}
        found = {}
        for key, p in pat.items():
            for row in rows:
                if re.search(p, row["Name"]):
                    found[key] = float(row["AverageNs"]) * 1e-6
        if len(found) == 2:
            by = r["line_kernel_bytes"]
            r["line_kernel"] = {"coupled_ms": round(found["coupled"], 4), "plain_ms_per_component": round(found["plain"], 4),
                                "coupled_gb_per_s": round(by["coupled"] / (found["coupled"] * 1e-3) / 1e9, 1),
                                "plain_gb_per_s": round(by["plain"] / r["K"] / (found["plain"] * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--components", default="2,4")
    ap.add_argument("--coils", default="0,8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cg-iters", type=int, default=5)
    ap.add_argument("--npoints", type=int, default=10_000_000)
    ap.add_argument("--dtypes", default="c64,c128")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--fold-only", action="store_true", help="with --kernel-stats: add the kernel figures to the results already in --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subspace_bench.json"))
    args = ap.parse_args()
    if args.fold_only:
        results = json.load(open(args.out))["results"]           # fold a profiler run into an earlier measurement
    else:
        if not torch.cuda.is_available():
            sys.exit("subspace_bench.py measures on the GPU: no device found")
        results = []
        for dtype in args.dtypes.split(","):
            for K in (int(k) for k in args.components.split(",")):
                for ncoils in (int(c) for c in args.coils.split(",")):
                    if args.trace_only and ncoils:
                        continue
                    r = measure(dtype, args.size, K, ncoils, args.reps, args.cg_iters, args.npoints, args.trace_only)
                    if r is not None:
                        results.append(r)
                        print(json.dumps(r), flush=True)
                    torch.cuda.empty_cache()
        if args.trace_only:
            return
    if args.kernel_stats:
        fold_kernel_stats(results, args.kernel_stats, args.size)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
