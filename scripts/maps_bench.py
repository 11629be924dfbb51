"""Coil sensitivity map measurement: CoilMapEstimator.estimate in ComplexF32 and ComplexF64 at

    3d_c8    256³, 8 coils,  box 5      2d_c16   256², 16 coils, box 7      3d_c32_64   64³, 32 coils, box 3

and, only when ``--cases`` names it, ``3d_c32`` (256³, 32 coils, box 3).  That case is not a default: by the cell rate of 3d_c32_64 one
call takes about two minutes, so it runs with one warm-up call and one repetition under a limit of its own (``--big-timeout``).

Times are hipEvent medians after warm-up, the routes alternating rep by rep in one process per case and element type:
  * ``estimate``                  the three launches of one call
  * ``crop_pass``                 ``crop_maps`` alone on the result, threshold at the median λ1 (half the cells are zeroed), rated over
                                  its algorithmic bytes: n reals of λ1 read, C complex elements written per zeroed cell
  * ``torch_route``               the same algorithm in torch (products a_c conj(a_c') in complex128, box sums by ``torch.roll`` one
                                  axis after the other, batched ``torch.linalg.eigh``, the phase rule), where ``--torch-cases`` names the
                                  case (default 2d_c16), on the leading sub-array of side ``--torch-side`` (default 64) next to the
                                  estimate on that same sub-array; the results are compared per cell.  The batched eigh takes about 0.5 ms
                                  per matrix, which rules out the full sizes (30 s per call at 256², two hours at 256³); the C² product
                                  arrays themselves would fit (17 GB at 256³ with 8 coils).

Every measurement runs in a child process of its own under a time limit.  The document (--out) is written after every child, so a
failure or a time limit leaves what was measured before it, and ``not_measured`` names the rest.  Prints the document at the end.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tvt_bench as TB  # noqa: E402

CASES = {"3d_c8": ((256, 256, 256), 8, 5), "2d_c16": ((256, 256), 16, 7), "3d_c32": ((256, 256, 256), 32, 3),
         "3d_c32_64": ((64, 64, 64), 32, 3)}
BAR = {"c128": 1e-9, "c64": 1e-5}


def images(torch, N, C, Z, dev):
    """Smooth coil profiles times a smooth object plus 5 % noise, [C, *reversed(N)]."""
    g = torch.Generator(device=dev).manual_seed(0)
    shape = tuple(reversed(N))
    axes = torch.meshgrid(*[torch.arange(n, device=dev, dtype=torch.float64) / n for n in shape], indexing="ij")
    rho = 1.0 + 0.5 * torch.cos(2 * math.pi * axes[-1]) * torch.exp(2j * math.pi * axes[0])
    a = torch.empty((C,) + shape, dtype=Z, device=dev)
    for c in range(C):
        k = [(c + d) % 3 - 1 for d in range(len(N))]
        prof = math.e ** (1j * c) * (1.0 + 0.4 * torch.exp(2j * math.pi * sum(kk * ax for kk, ax in zip(k, axes))))
        a[c] = (prof * rho).to(Z)
    a += 0.05 * torch.randn(a.shape, generator=g, device=dev, dtype=Z)
    return a


def torch_route(torch, a, box):
    """[C, ...] maps in complex128: the same algorithm with torch's own kernels."""
    C = a.shape[0]
    x = a.to(torch.complex128)
    R = x[:, None] * x[None, :].conj()
    h = (box - 1) // 2
    for ax in range(2, R.dim()):
        R = sum(torch.roll(R, -k, dims=ax) for k in range(-h, h + 1))
    R = R.movedim((0, 1), (-2, -1))
    lam, V = torch.linalg.eigh(R)
    v = V[..., -1]
    s = v[..., 0].conj()
    v = v * (s / s.abs())[..., None]
    return v.movedim(-1, 0), lam[..., -1]


def worker(dtype, args):
    import torch
    sys.path.insert(0, ROOT)
    from nufft_pkg import nufft
    N, C, box = CASES[args.case]
    dev = torch.device("cuda", 0)
    Z = torch.complex128 if dtype == "c128" else torch.complex64
    plan = nufft.PlanNUFFT(Z, N, backend=nufft.ROCBackend(0))
    a = images(torch, N, C, Z, dev)
    at = tuple(a[c] for c in range(C))
    out = tuple(torch.empty_like(v) for v in at)
    est = nufft.CoilMapEstimator(plan, C, box=box)
    est.estimate(at, out=out)
    sweeps = est.last_sweeps()
    lam1 = est.lambda1.double()
    crop = math.sqrt(float(lam1.median() / lam1.max()))
    plan.close()
    routes = [("estimate", lambda: est.estimate(at, out=out)), ("crop_pass", lambda: est.crop_maps(out, crop))]
    with_torch = args.case in args.torch_cases.split(",")
    for name, fn in routes:
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
    med, minmax = TB.measure(torch, routes, args.reps, {name: 1 for name, _ in routes})
    zeroed = int((torch.stack(out).abs().sum(dim=0) == 0).sum())
    n = a[0].numel()
    eb = 16 if dtype == "c128" else 8
    crop_bytes = n * eb // 2 + zeroed * C * eb
    info = est.info()
    r = {"N": list(N), "coils": C, "box": box, "jacobi_sweeps": sweeps, "ms": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": minmax,
         "tile": list(info.tile)[:len(N)], "teams": info.teams, "team_lanes": info.team_lanes, "staged": info.staged, "lds_bytes": info.lds_bytes,
         "workgroups": info.workgroups, "mcells_per_s": round(n / med["estimate"] / 1e3, 2),
         "crop": {"crop": crop, "zeroed_share": round(zeroed / n, 3), "algorithmic_mb": round(crop_bytes / 1e6, 1),
                  "gb_per_s": round(crop_bytes / (med["crop_pass"] * 1e-3) / 1e9, 1)}}
    if with_torch:
        # both routes on the leading sub-array of side --torch-side (periodic on itself), alternating
        side = min(args.torch_side, min(N))
        sub = a[(slice(None),) + (slice(0, side),) * len(N)].contiguous()
        st = tuple(sub[c] for c in range(C))
        so = tuple(torch.empty_like(v) for v in st)
        small = nufft.PlanNUFFT(Z, (side,) * len(N), backend=nufft.ROCBackend(0))
        es = nufft.CoilMapEstimator(small, C, box=box)
        small.close()
        pair = [("estimate_sub", lambda: es.estimate(st, out=so)), ("torch_route_sub", lambda: torch_route(torch, sub, box))]
        for name, fn in pair:
            fn()
            torch.cuda.synchronize()
        m2, mm2 = TB.measure(torch, pair, args.torch_reps, {name: 1 for name, _ in pair})
        es.estimate(st, out=so)
        base, _ = torch_route(torch, sub, box)
        err = float((torch.stack(so).to(torch.complex128) - base).abs().pow(2).sum(dim=0).sqrt().max())
        r["torch"] = {"side": side, "cells": sub[0].numel(), "ms": {k: round(v, 4) for k, v in m2.items()}, "ms_min_max": mm2,
                      "ratio_torch_over_estimate": round(m2["torch_route_sub"] / m2["estimate_sub"], 2),
                      "per_cell_max_difference": err, "agreement_bar": BAR[dtype]}
        es.close()
        assert err <= BAR[dtype], f"the torch route and the estimate differ by {err:.3e} at some cell (bar {BAR[dtype]:g})"
    for k, v in med.items():
        print(f"  {args.case} {dtype} {k:20s} {v:10.4f} ms", file=sys.stderr)
    est.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="3d_c8,2d_c16,3d_c32_64")
    ap.add_argument("--case", default="2d_c16", help=argparse.SUPPRESS)
    ap.add_argument("--torch-cases", default="2d_c16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--torch-side", type=int, default=64)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--dtypes", default="c64,c128")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds every child process may take")
    ap.add_argument("--big-timeout", type=int, default=900, help="seconds a child of the 3d_c32 case may take: its three calls are 64 times the cells of 3d_c32_64 at 1.9 s each, about 6 minutes, "
                    "and the limit leaves that much again")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maps_bench.json"))
    args = ap.parse_args()
    if args.worker:
        print(json.dumps(worker(args.worker, args)))
        return
    cases, dtypes = args.cases.split(","), args.dtypes.split(",")
    todo = [(c, dt) for c in cases for dt in dtypes]
    out = {"metric": "coil_map_estimate_ms", "cases": {c: {"N": list(CASES[c][0]), "coils": CASES[c][1], "box": CASES[c][2]} for c in cases},
           "reps": args.reps, "warmup": args.warmup, "torch_route_cases": args.torch_cases.split(","), "results": {c: {} for c in cases}, "value": None,
           "not_measured": [c for c in CASES if c not in cases]}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for i, (case, dt) in enumerate(todo):
        big = case == "3d_c32"
        argv = ["--worker", dt, "--case", case, "--reps", "1" if big else str(args.reps), "--warmup", "1" if big else str(args.warmup),
                "--torch-cases", args.torch_cases, "--torch-side", str(args.torch_side), "--torch-reps", str(args.torch_reps)]
        try:
            out["results"][case][dt] = child(argv, args.big_timeout if big else args.step_timeout)
        except BaseException:
            out["not_measured"] += [f"{c} {d}" for c, d in todo[i:]]      # this one and everything after it
            write()
            raise
        if out["value"] is None:
            out["value"] = out["results"][case][dt]["ms"]["estimate"]
        write()
    print(json.dumps(out))


def child(argv, limit):
    import subprocess
    done = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, stdout=subprocess.PIPE, timeout=limit, check=True)
    return json.loads(done.stdout.decode().strip().splitlines()[-1])


if __name__ == "__main__":
    main()
