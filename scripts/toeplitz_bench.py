"""Toeplitz normal operator measurement: N = 256³, m = 4, σ = 2, uniform points.

Times, in one process and alternating rep by rep (hipEvent medians after warm-up):
  * apply of the fused path                      (pruned line passes, the 2N grid never exists)
  * apply of the dense path                      (NUFFT_TOEPLITZ_FUSED=0: pad, rocFFT, multiply, rocFFT, crop)
  * the composed pair exec_type2 + exec_type1    (same plan, set_points excluded: the plan's own code paths)
and once each: the build (set_points of the operator: 2N plan, type 1 of the weights, multiplier) and the plan's set_points.
Reports the fused apply against the bytes its passes move by construction, and the agreement of the three routes.
Prints one JSON line.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nufft_pkg import nufft  # noqa: E402


def fused_bytes(N, cb, rb):
    """Bytes per component the five launches of the fused 3-D apply read and write (array sizes)."""
    n1, n2, n3 = N
    u, a, b, k = n1 * n2 * n3 * cb, n1 * n2 * 2 * n3 * cb, n1 * 2 * n2 * 2 * n3 * cb, 8 * n1 * n2 * n3 * rb
    return {"pass1_dim3_bwd": u + a, "pass2_dim2_bwd": a + b, "pass3_dim1": b + k + b, "pass4_dim2_fwd": b + a, "pass5_dim3_fwd": a + u}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e7, help="number of points")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", choices=("c128", "c64"), default="c128")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-dense", action="store_true")
    args = ap.parse_args()
    n, N = int(args.n), (args.size,) * 3
    Z, T = (torch.complex128, torch.float64) if args.dtype == "c128" else (torch.complex64, torch.float32)
    rb = 8 if args.dtype == "c128" else 4
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    xs = tuple(torch.rand(n, generator=g, device=dev, dtype=T) * (2 * math.pi) for _ in N)
    w = torch.rand(n, generator=g, device=dev, dtype=T) + 0.1
    u = torch.randn(tuple(reversed(N)), generator=g, device=dev, dtype=Z)

    plan = nufft.PlanNUFFT(Z, N, m=4, sigma=2.0, backend=nufft.ROCBackend(0))
    t0 = time.perf_counter()
    nufft.set_points(plan, xs)
    torch.cuda.synchronize()
    t_setpoints = (time.perf_counter() - t0) * 1e3
    fused = nufft.ToeplitzOperator(plan)
    assert fused.path == "fused"
    t0 = time.perf_counter()
    fused.set_points(xs, w)
    torch.cuda.synchronize()
    t_build = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    fused.set_points(xs, w)
    torch.cuda.synchronize()
    t_build2 = (time.perf_counter() - t0) * 1e3              # code objects and rocFFT plans warm
    dense = None
    if not args.skip_dense:
        dense_parent = nufft.PlanNUFFT(Z, N, m=4, sigma=2.0, backend=nufft.ROCBackend(0), options={"NUFFT_TOEPLITZ_FUSED": 0})
        dense = nufft.ToeplitzOperator(dense_parent)
        dense_parent.close()
        assert dense.path == "dense"
        dense.set_points(xs, w)

    v = torch.empty(n, dtype=Z, device=dev)
    gf, gd, gc = torch.empty_like(u), torch.empty_like(u), torch.empty_like(u)

    def run_fused():
        fused.apply(u, out=gf)

    def run_dense():
        dense.apply(u, out=gd)

    def run_composed():
        nufft.exec_type2(v, plan, u)
        v.mul_(w)
        nufft.exec_type1(gc, plan, v)

    routes = [("fused_apply", run_fused), ("composed_type2_type1", run_composed)] + ([("dense_apply", run_dense)] if dense else [])
    for _ in range(3):
        for _, fn in routes:
            fn()
    torch.cuda.synchronize()
    acc = {name: [] for name, _ in routes}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.reps):
        for name, fn in routes:
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            acc[name].append(e0.elapsed_time(e1))
    med = {k: sorted(x)[len(x) // 2] for k, x in acc.items()}
    spread = {k: [min(x), max(x)] for k, x in acc.items()}
    rel = lambda a, b: float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))      # noqa: E731
    agree = {"fused_vs_composed": rel(gf, gc)}
    if dense:
        agree["fused_vs_dense"] = rel(gf, gd)
    by = fused_bytes(N, 2 * rb, rb)
    total = sum(by.values())
    out = {"metric": "toeplitz_apply_ms", "value": med["fused_apply"], "dtype": args.dtype, "N": N, "num_points": n,
           "ms": {k: round(x, 4) for k, x in med.items()}, "ms_min_max": {k: [round(a, 4), round(b, 4)] for k, (a, b) in spread.items()},
           "build_ms_first": round(t_build, 1), "build_ms_warm": round(t_build2, 1), "plan_set_points_ms": round(t_setpoints, 1),
           "speedup_vs_composed": round(med["composed_type2_type1"] / med["fused_apply"], 2),
           "fused_bytes_per_component": by, "fused_gb_per_s": round(total / (med["fused_apply"] * 1e-3) / 1e9, 1),
           "workspace_mb": {"fused": round(fused.info().workspace_bytes / 1e6, 1)}, "agreement": agree}
    if dense:
        out["speedup_vs_dense"] = round(med["dense_apply"] / med["fused_apply"], 2)
        out["workspace_mb"]["dense"] = round(dense.info().workspace_bytes / 1e6, 1)
    for k in acc:
        print(f"  {k:24s} {med[k]:8.3f} ms   (min {spread[k][0]:.3f}, max {spread[k][1]:.3f})")
    print(f"  fused apply: {total / 1e9:.2f} GB by construction -> {out['fused_gb_per_s']:.0f} GB/s; build {t_build:.0f} ms first, {t_build2:.0f} ms warm")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
