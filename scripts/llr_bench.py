"""Measurement of FISTA with the locally low-rank prior: N = 256³, fused apply path, an operator with K = 2 and 4
transforms built from 1e7 uniform points, blocks of 8³, ComplexF32 and ComplexF64.

Times, in one process and alternating rep by rep (hipEvent medians after warm-up), per iteration:
  * ToeplitzFISTA(prior="llr").solve with check_every = 0 and tol = 0, eager   (all iterations enqueued, no host synchronisation)
  * the apply alone                                                             (outside the apply = total − apply: the fused kernel
                                                                                 and the decision kernel)
  * the standalone map LocallyLowRank.apply                                     (the plain-load variant of the same kernel)
  * baseline: the same algorithm in torch around op(...), torch.linalg.eigh on the Gram matrices of the Casorati blocks
  * the wavelet solver (haar, 3 levels, l1 = 0) of the same operator, and its transform's forward and inverse alone
Rates.  The fused kernel over its algorithmic bytes 6 · K · n · sizeof(complex T) (reads z, q, b, x; writes x, z), from the time outside
the apply: a difference of two medians, which also holds the decision kernel and a tenth of the start kernel.  The plain map over
2 · K · n · sizeof, timed directly.  The existing fista_gradient streaming kernel over its own 4 · K · n · sizeof (reads z, q, b; writes
q), from wavelet solver − apply − forward − inverse: no entry point launches it alone, and that difference also holds the decision
kernel and the momentum step on the last synthesis level's store (2 · K · n · sizeof more than the inverse alone moves), so the rate is
a lower bound.  The torch baseline runs --torch-iters iterations per call (batched eigh of 32768 small matrices takes seconds).
Writes one JSON document (--out) and prints it.
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nufft_pkg import nufft  # noqa: E402


def torch_prox(v, side, thr):
    """Singular-value soft-thresholding of every side³ block of the stacked v [K, n3, n2, n1] through eigh of the Gram matrices."""
    K, n3, n2, n1 = v.shape
    y = v.reshape(K, n3 // side, side, n2 // side, side, n1 // side, side).permute(1, 3, 5, 2, 4, 6, 0).reshape(-1, side ** 3, K)
    lam, V = torch.linalg.eigh(y.mH @ y)
    sig = lam.clamp_min(0).sqrt()
    f = torch.where(sig > thr, 1.0 - thr / sig, torch.zeros_like(sig))
    out = y @ ((V * f[:, None, :].to(V.dtype)) @ V.mH)
    out = out.reshape(n3 // side, n2 // side, n1 // side, side, side, side, K).permute(6, 0, 3, 1, 4, 2, 5)
    return out.reshape(K, n3, n2, n1), (f * sig).sum()


def torch_loop(op, b, iters, side, nuc, step):
    """The solver's algorithm in torch: one apply, elementwise work, eigh of the blocks' Gram matrices, no host synchronisation."""
    x = torch.zeros_like(b)
    z = torch.zeros_like(b)
    t = 1.0
    for _ in range(iters):
        t_next = 0.5 * (1.0 + math.sqrt(1.0 + 4.0 * t * t))
        beta = (t - 1.0) / t_next
        t = t_next
        q = torch.stack(op(tuple(z)))
        xp, _ = torch_prox(z - step * (q - b), side, step * nuc)
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


def run(dtype, K, args):
    n, N, iters, side = int(args.n), (args.size,) * 3, args.iters, args.block
    Z, T = (torch.complex128, torch.float64) if dtype == "c128" else (torch.complex64, torch.float32)
    cb = 16 if dtype == "c128" else 8
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    xs = tuple(torch.rand(n, generator=g, device=dev, dtype=T) * (2 * math.pi) for _ in N)
    w = (torch.rand(n, generator=g, device=dev, dtype=T) + 0.1) / n
    plan = nufft.PlanNUFFT(Z, N, m=4, sigma=2.0, backend=nufft.ROCBackend(0), ntransforms=K)
    op = nufft.ToeplitzOperator(plan)
    assert op.path == "fused"
    op.set_points(xs, w)
    plan.close()
    del xs, w
    torch.cuda.empty_cache()
    shape = tuple(reversed(N))
    u = torch.randn(shape, generator=g, device=dev, dtype=Z)
    truth = tuple((0.3 + 0.7 * (a + 1) / K) * u + 0.05 * torch.randn(shape, generator=g, device=dev, dtype=Z) for a in range(K))
    b = op(truth)
    del truth, u
    lmax = max(op.max_eigenvalue())
    step = 1.0 / (1.05 * lmax)
    llr = nufft.LocallyLowRank(op, side)
    bs = torch.stack(b)
    y = bs.reshape(K, N[2] // side, side, N[1] // side, side, N[0] // side, side).permute(1, 3, 5, 2, 4, 6, 0).reshape(-1, side ** 3, K)
    nuc = 0.2 * float(torch.linalg.eigvalsh(y.mH @ y).clamp_min(0).sqrt().max())
    del y
    sol = nufft.ToeplitzFISTA(op, prior="llr", block=side, nuc=nuc, step=step, maxiter=iters, tol=0.0)
    wav = nufft.ToeplitzFISTA(op, wavelet="haar", levels=3, l1=0.0, step=step, maxiter=iters, tol=0.0)
    wt = nufft.WaveletTransform(op, "haar", 3)
    x = tuple(torch.empty_like(v) for v in b)
    q = tuple(torch.empty_like(v) for v in b)
    c1 = tuple(torch.empty_like(v) for v in b)
    routes = [("solver_eager", lambda: sol.solve(b, out=x)), ("apply_alone", lambda: [op.apply(b, out=q) for _ in range(iters)]),
              ("map_alone", lambda: [llr.apply(b, step * nuc, out=q) for _ in range(iters)]),
              ("wavelet_solver", lambda: wav.solve(b, out=x)),
              ("wavelet_forward", lambda: [wt.forward(b, out=c1) for _ in range(iters)]),
              ("wavelet_inverse", lambda: [wt.inverse(c1, out=q) for _ in range(iters)])]
    per = {name: iters for name, _ in routes}
    if not args.no_torch:
        routes.append(("torch_loop", lambda: torch_loop(op, bs, args.torch_iters, side, nuc, step)))
        per["torch_loop"] = args.torch_iters
    for name, fn in routes:
        for _ in range(1 if name == "torch_loop" else 2):
            fn()
    torch.cuda.synchronize()
    med, minmax = measure(routes, args.reps, per)
    arr = N[0] * N[1] * N[2] * cb
    outside = med["solver_eager"] - med["apply_alone"]
    gradient = med["wavelet_solver"] - med["apply_alone"] - med["wavelet_forward"] - med["wavelet_inverse"]
    info = llr.info()
    r = {"ms_per_iteration": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": minmax,
         "outside_apply_ms": round(outside, 4), "outside_apply_share": round(outside / med["solver_eager"], 3),
         "fused_kernel_bytes": 6 * K * arr,
         "fused_gb_per_s_from_outside_apply": round(6 * K * arr / (outside * 1e-3) / 1e9, 1),
         "map_alone_gb_per_s": round(2 * K * arr / (med["map_alone"] * 1e-3) / 1e9, 1),
         "fista_gradient_ms_from_wavelet_solver": round(gradient, 4),
         "fista_gradient_gb_per_s_lower_bound": round(4 * K * arr / (gradient * 1e-3) / 1e9, 1),
         "waves_per_cu": info.waves_per_cu, "blocks": info.blocks, "nuc": nuc, "step": step,
         "workspace_mb": round(sol.info().workspace_bytes / 1e6, 1)}
    if not args.no_torch:
        short = nufft.ToeplitzFISTA(op, prior="llr", block=side, nuc=nuc, step=step, maxiter=args.torch_iters, tol=0.0)
        short.solve(b, out=x)
        short.close()
        base, _ = torch_loop(op, bs, args.torch_iters, side, nuc, step)
        r["torch_loop_vs_solver_rel_l2"] = float(torch.linalg.vector_norm(base - torch.stack(x)) / torch.linalg.vector_norm(torch.stack(x)))
        r["torch_loop_outside_apply_ms"] = round(med["torch_loop"] - med["apply_alone"], 4)
        r["iteration_ratio_torch_over_solver"] = round(med["torch_loop"] / med["solver_eager"], 2)
        r["outside_apply_ratio_torch_over_solver"] = round((med["torch_loop"] - med["apply_alone"]) / outside, 2)
        del base
    for k, v in med.items():
        print(f"  {dtype} K={K} {k:16s} {v:9.4f} ms")
    for o in (sol, wav, wt, llr, op):
        o.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e7, help="number of points the operator is built from")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-iters", type=int, default=2)
    ap.add_argument("--dtypes", default="c64,c128")
    ap.add_argument("--components", default="2,4")
    ap.add_argument("--no-torch", action="store_true", help="leave the torch baseline out")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "llr_bench.json"))
    args = ap.parse_args()
    out = {"metric": "fista_llr_iteration_ms", "N": [args.size] * 3, "points": int(args.n), "block": [args.block] * 3, "iterations": args.iters,
           "operator": "uncoupled, ntransforms = K, fused apply path", "repetitions": args.reps, "torch_iterations_per_call": args.torch_iters,
           "notes": {"fused_gb_per_s_from_outside_apply": "6 K n sizeof over (solver median - apply median): holds the decision kernel too",
                     "fista_gradient_gb_per_s_lower_bound": "4 K n sizeof over (wavelet solver - apply - forward - inverse): holds the decision "
                                                            "kernel and the momentum step of the last synthesis level too"},
           "results": {dt: {f"K={K}": run(dt, int(K), args) for K in args.components.split(",")} for dt in args.dtypes.split(",")}}
    first = out["results"][args.dtypes.split(",")[0]]
    out["value"] = first[next(iter(first))]["ms_per_iteration"]["solver_eager"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
