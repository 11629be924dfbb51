"""Type-2 gradient measurement at C2: 256³ Float64 (real), Np = 1e7 uniform points, m = 4, σ = 2, Direct().

Times, in one process and alternating rep by rep:
  * exec_type2                      (values)
  * exec_type2_grad                 (values + 3 gradient components)
  * the spectral route              (an ntransforms = 4 type 2 of û, i k_1 û, i k_2 û, i k_3 û; building the spectra excluded)
and the hipEvent time of the gather stage of exec_type2_grad (NUFFT_STAGE_T2_INTERP), with its bytes and FLOPs over that time.
Prints one JSON line.  DESIGN.md section 14 records a run.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nufft_pkg import nufft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e7)
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    n, N, M = int(args.n), args.N, args.m
    dims = (N, N, N)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    xs = tuple(torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 6.283185307179586 for _ in range(3))
    plan = nufft.PlanNUFFT(torch.float64, dims, m=M, sigma=2.0, kernel_evalmode=nufft.Direct(), backend=nufft.ROCBackend(0))
    plan4 = nufft.PlanNUFFT(torch.float64, dims, m=M, sigma=2.0, ntransforms=4, kernel_evalmode=nufft.Direct(),
                            backend=nufft.ROCBackend(0))
    nufft.set_points(plan, xs)
    nufft.set_points(plan4, xs)
    uh = torch.randn(plan.shape, generator=g, device=dev, dtype=torch.complex128)
    k1 = torch.fft.rfftfreq(N, d=1.0 / N, dtype=torch.float64, device=dev)
    k = torch.fft.fftfreq(N, d=1.0 / N, dtype=torch.float64, device=dev)
    spec = (uh, (1j * k1[None, None, :] * uh).contiguous(), (1j * k[None, :, None] * uh).contiguous(), (1j * k[:, None, None] * uh).contiguous())
    v = torch.empty(n, dtype=torch.float64, device=dev)
    gp = tuple(torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
    outs = tuple(torch.empty(n, dtype=torch.float64, device=dev) for _ in range(4))
    plan.enable_timing(True)

    runs = {
        "exec_type2": lambda: nufft.exec_type2(v, plan, uh),
        "exec_type2_grad": lambda: nufft.exec_type2_grad(gp, plan, uh, vp=v),
        "spectral_route": lambda: nufft.exec_type2(outs, plan4, spec),
    }
    for f in runs.values():                              # warm-up (rocFFT plans, code objects)
        f()
        f()
    torch.cuda.synchronize()
    acc = {k_: [] for k_ in runs}
    acc["grad_gather_stage"], acc["interp_stage"] = [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.reps):
        for name, f in runs.items():
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            acc[name].append(e0.elapsed_time(e1))
            if name == "exec_type2":
                acc["interp_stage"].append(plan.timer["t2_interp"])
            elif name == "exec_type2_grad":
                acc["grad_gather_stage"].append(plan.timer["t2_interp"])
    med = {k_: sorted(t)[len(t) // 2] for k_, t in acc.items()}
    L = 2 * M
    # gather: records in, stencil values (L³ reads of 8 bytes: cache traffic, not HBM), 4 outputs; FLOPs: 2 FMA per grid value + the reductions
    rec_bytes = 32
    hbm_bytes = n * (rec_bytes + 4 * 8)
    grid_bytes = 8 * (2 * N) ** 3
    flops = n * (L ** 3 * 4 + L * L * 6 + L * 8)
    gt = med["grad_gather_stage"] * 1e-3
    print(f"C2-like: dims {dims}, Np {n}, m {M}; interp engine for values: {plan.interp_engine_used()}, sort: {plan.sort_method_used()}")
    for k_ in ("exec_type2", "exec_type2_grad", "spectral_route", "interp_stage", "grad_gather_stage"):
        print(f"  {k_:18s} {med[k_]:8.3f} ms")
    print(f"  exec_type2_grad / exec_type2 = {med['exec_type2_grad'] / med['exec_type2']:.2f}, "
          f"spectral route / exec_type2_grad = {med['spectral_route'] / med['exec_type2_grad']:.2f}")
    print(f"  gather: {(hbm_bytes + grid_bytes) / gt / 1e9:.0f} GB/s (records + outputs + one pass over the grid), "
          f"{flops / gt / 1e12:.2f} TFLOP/s, {L ** 3 * n * 8 / gt / 1e12:.1f} TB/s of stencil reads")
    print(json.dumps({"metric": "type2_grad_c2_ms", "ms": {k_: round(t, 4) for k_, t in med.items()},
                      "grad_over_type2": med["exec_type2_grad"] / med["exec_type2"],
                      "spectral_over_grad": med["spectral_route"] / med["exec_type2_grad"], "n": n, "N": N, "m": M}))


if __name__ == "__main__":
    main()
