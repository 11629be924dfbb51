"""Type-3 gradient measurement at the type-3 configuration of DESIGN.md §13: D = 3, ComplexF64, m = 4, σ = 2, Np = Nk = 1e7, sources
uniform in a box of half-width π, targets in half-width 64.

Times, in one process and alternating rep by rep:
  * exec_type3                      (values)
  * exec_type3_grad                 (values + 3 derivatives with respect to the targets)
  * the spectral route              (an ntransforms = 4 type 3 of c, −i x_d c; building its inputs excluded)
and the hipEvent stage times of exec_type3_grad; its postmultiply stage is the finish kernel alone, reported with its GB/s over the
algorithmic bytes.  Prints one JSON line.  DESIGN.md section 15 records a run.
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
    args = ap.parse_args()
    n, D = int(args.n), 3
    Z, T, rb = torch.complex128, torch.float64, 8
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    xs = tuple((torch.rand(n, generator=g, device=dev, dtype=T) * 2 - 1) * math.pi for _ in range(D))
    ss = tuple((torch.rand(n, generator=g, device=dev, dtype=T) * 2 - 1) * 64.0 for _ in range(D))
    c = torch.randn(n, generator=g, device=dev, dtype=Z)
    kw = dict(m=4, sigma=2.0, backend=nufft.ROCBackend(0), source_bounds=[(-math.pi, math.pi)] * D, target_bounds=[(-64.0, 64.0)] * D)
    plan = nufft.PlanNUFFT3(Z, D, **kw)
    spec = nufft.PlanNUFFT3(Z, D, ntransforms=D + 1, **kw)
    plan.enable_timing(True)
    nufft.set_points3(plan, xs, ss)
    nufft.set_points3(spec, xs, ss)
    ins = [c] + [(-1j) * x * c for x in xs]                # sign = −1: ∂f/∂s_d = Σ_j c_j (−i x_{j,d}) e^{−i s·x}
    f = torch.empty(n, dtype=Z, device=dev)
    fg = torch.empty(n, dtype=Z, device=dev)
    gp = tuple(torch.empty(n, dtype=Z, device=dev) for _ in range(D))
    outs = [torch.empty(n, dtype=Z, device=dev) for _ in ins]

    def run_value():
        nufft.exec_type3(f, plan, c)

    def run_grad():
        nufft.exec_type3_grad(fg, gp, plan, c)

    def run_spec():
        nufft.exec_type3(outs, spec, ins)

    for _ in range(2):                                   # warm-up (rocFFT plans, code objects)
        run_value(), run_grad(), run_spec()
    torch.cuda.synchronize()
    keys = ("premultiply", "spread", "type2", "postmultiply")
    acc = {k: [] for k in ("exec_type3", "exec_type3_grad", "spectral_route") + tuple("grad_" + k for k in keys) +
           tuple("value_" + k for k in keys)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.reps):
        for name, fn in (("exec_type3", run_value), ("exec_type3_grad", run_grad), ("spectral_route", run_spec)):
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            acc[name].append(e0.elapsed_time(e1))
            if name != "spectral_route":
                t = plan.timer
                pre = "value_" if name == "exec_type3" else "grad_"
                for k in keys:
                    acc[pre + k].append(t[k])
    med = {k: sorted(v)[len(v) // 2] for k, v in acc.items()}
    # agreement at full size: values with exec_type3, gradients with the spectral route
    rel = lambda a, b: float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))   # noqa: E731
    agree = {"values_vs_exec_type3": rel(fg, f), "grad_vs_spectral": max(rel(gp[d], outs[1 + d]) for d in range(D))}
    # the finish kernel: θ (D reals) and the post factor in; v and D derivatives in and out, complex
    finish_bytes = n * (D * rb + 2 * rb + 2 * (1 + D) * 2 * rb)
    finish_gbs = finish_bytes / (med["grad_postmultiply"] * 1e-3) / 1e9
    info = plan.info()
    nf = tuple(int(info.nf[d]) for d in range(D))
    print(f"nf = {nf}, type-2 grid = {tuple(int(info.inner_N_over[d]) for d in range(D))}, "
          f"engines: spread {plan.spread_engine_used()}, interp {plan.interp_engine_used()}")
    for k in acc:
        print(f"  {k:22s} {med[k]:8.3f} ms")
    print(f"  finish kernel: {finish_bytes / n:.0f} B per target, {finish_gbs:.0f} GB/s")
    print(f"  exec_type3_grad / exec_type3 = {med['exec_type3_grad'] / med['exec_type3']:.2f}, "
          f"spectral route / exec_type3_grad = {med['spectral_route'] / med['exec_type3_grad']:.2f}")
    print(f"  agreement: {agree}")
    print(json.dumps({"metric": "type3_grad_ms", "value": med["exec_type3_grad"], "nf": nf, "n": n,
                      "ms": {k: round(v, 4) for k, v in med.items()}, "finish_gb_per_s": round(finish_gbs, 1),
                      "agreement": agree}))


if __name__ == "__main__":
    main()
