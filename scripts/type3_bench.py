"""Type-3 measurement: D = 3, ComplexF64, m = 4, σ = 2, Np = Nk = 1e7; sources uniform in a box of half-width π, targets in half-width 64.

Prints nf, the engines the two internal plans chose, hipEvent times of every stage (prep, premultiply, spread, type 2, postmultiply),
NU-points/s and the bandwidth of the four type-3 kernels, then one JSON line.  DESIGN.md section 13 records a run.
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nufft_pkg import nufft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e7, help="sources = targets")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    args = ap.parse_args()
    n, D = int(args.n), 3
    Z, T = (torch.complex128, torch.float64) if args.dtype == "f64" else (torch.complex64, torch.float32)
    rb = 8 if T == torch.float64 else 4
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    xs = tuple(((torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 2 - 1) * math.pi).to(T) for _ in range(D))
    ss = tuple(((torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 2 - 1) * 64.0).to(T) for _ in range(D))
    c = torch.randn(n, generator=g, device=dev, dtype=Z)
    f = torch.empty(n, dtype=Z, device=dev)
    plan = nufft.PlanNUFFT3(Z, D, m=4, sigma=2.0, backend=nufft.ROCBackend(0),
                            source_bounds=[(-math.pi, math.pi)] * D, target_bounds=[(-64.0, 64.0)] * D)
    plan.enable_timing(True)
    for _ in range(2):                                   # warm-up (buffers, rocFFT plans, code objects)
        nufft.set_points3(plan, xs, ss)
        nufft.exec_type3(f, plan, c)
    torch.cuda.synchronize()
    keys = ("prep_sources", "prep_targets", "premultiply", "spread", "type2", "postmultiply")
    acc = {k: [] for k in keys}
    acc["set_points3"], acc["exec_type3"] = [], []
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    for _ in range(args.reps):
        e0.record()
        nufft.set_points3(plan, xs, ss)
        e1.record()
        nufft.exec_type3(f, plan, c)
        e2.record()
        torch.cuda.synchronize()
        t = plan.timer
        for k in keys:
            acc[k].append(t[k])
        acc["set_points3"].append(e0.elapsed_time(e1))
        acc["exec_type3"].append(e1.elapsed_time(e2))
    med = {k: sorted(v)[len(v) // 2] for k, v in acc.items()}
    info = plan.info()
    nf = tuple(int(info.nf[d]) for d in range(D))
    engines = {"spread": plan.spread_engine_used(), "interp": plan.interp_engine_used()}
    # bytes each type-3 kernel moves (reads + writes)
    cb = 2 * rb
    traffic = {
        "prep_sources": n * (D * rb + D * rb + cb),      # coordinates in, rescaled coordinates + phase out
        "prep_targets": n * (D * rb + D * rb + cb),      # coordinates in, θ + post factor out
        "premultiply": n * 3 * cb,                       # values + phase in, prephased values out
        "postmultiply": n * 3 * cb,                      # f + factor in, f out
    }
    gbs = {k: traffic[k] / (med[k] * 1e-3) / 1e9 for k in traffic}
    glue = med["premultiply"] + med["postmultiply"]
    print(f"nf = {nf}, type-2 grid = {tuple(int(info.inner_N_over[d]) for d in range(D))}, engines: {engines}")
    for k in keys + ("set_points3", "exec_type3"):
        extra = f"  {gbs[k]:.0f} GB/s" if k in gbs else ""
        print(f"  {k:14s} {med[k]:8.3f} ms{extra}")
    print(f"  exec glue (pre + post) {glue:.3f} ms = {100 * glue / (med['spread'] + med['type2']):.1f} % of spread + type 2")
    rate = n / (med["exec_type3"] * 1e-3)
    print(f"  exec_type3: {rate:.3e} NU-points/s (sources), set_points3 + exec: {n / ((med['exec_type3'] + med['set_points3']) * 1e-3):.3e}")
    print(json.dumps({"metric": "type3_exec_nu_points_per_s", "value": rate, "nf": nf, "engines": engines,
                      "ms": {k: round(v, 4) for k, v in med.items()}, "gb_per_s": {k: round(v, 1) for k, v in gbs.items()},
                      "dtype": args.dtype, "n": n}))


if __name__ == "__main__":
    main()
