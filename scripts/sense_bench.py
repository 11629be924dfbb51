"""Multi-coil (SENSE) Toeplitz normal operator measurement: N = 256³, 8 coils, ComplexF64 and ComplexF32.

Times, in one process and alternating rep by rep (hipEvent medians after warm-up), the three ways to apply
G_S û = Σ_c conj(S_c) ⊙ G (S_c ⊙ û) on the fused path:
  * in-pass     the maps inside the outermost pruned passes                 (NUFFT_TOEPLITZ_MAPS_INPASS=1)
  * streaming   coil expand, the plain in-place apply, combine-accumulate   (NUFFT_TOEPLITZ_MAPS_INPASS=0)
  * torch loop  the coil loop written in torch around the plain apply       (what a user writes without set_maps)
and one CG iteration: ToeplitzCG on the operator with maps against the README's CG loop with the torch coil loop inside.
The operator gets an analytic spectrum (a product of Poisson kernels: positive definite, cond <= ((1 + a) / (1 − a))^6); the cost
of an apply does not depend on the values of K.  Reports the bytes each library route moves by construction and the agreement of
the routes.  Writes profiles/sense_bench.json and prints one JSON line per element type.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nufft_pkg import nufft  # noqa: E402


def route_bytes(N, cb, rb):
    """Bytes per coil, by construction (array sizes): the plain fused apply (scripts/toeplitz_bench.py), what the maps add in the passes
    (two map reads, one read of the running output: none for coil 0), the streaming route's two extra passes and the torch loop's."""
    n1, n2, n3 = N
    u, a, b, k = n1 * n2 * n3 * cb, n1 * n2 * 2 * n3 * cb, n1 * 2 * n2 * 2 * n3 * cb, 8 * n1 * n2 * n3 * rb
    plain = (u + a) + (a + b) + (b + k + b) + (b + a) + (a + u)
    # expand or torch.mul: read û and S, write the temporary (3 arrays); combine or addcmul: read S, the result, the output, write it (4)
    return {"plain_apply": plain, "inpass": plain + 3 * u, "streaming": plain + 7 * u, "torch_loop": plain + 7 * u}


def poisson_spectrum(N, a, Z, dev):
    spec = torch.ones(tuple(2 * n for n in reversed(N)), dtype=torch.float64, device=dev)
    D = len(N)
    for dim, n in enumerate(N):
        k = torch.fft.fftfreq(2 * n, d=1.0 / (2 * n), device=dev, dtype=torch.float64).abs()
        shape = [1] * D
        shape[D - 1 - dim] = 2 * n
        spec = spec * (a ** k).reshape(shape)
    return spec.to(Z)


def smooth_maps(ncoils, shape, Z, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    axes = torch.meshgrid(*[torch.arange(n, device=dev, dtype=torch.float64) / n for n in shape], indexing="ij")
    maps = torch.empty((ncoils,) + tuple(shape), dtype=Z, device=dev)
    for c in range(ncoils):
        f = torch.ones(shape, dtype=torch.complex128, device=dev)
        for _ in range(3):
            k = torch.randint(-1, 2, (len(shape),), generator=g)
            amp = 0.25 * complex(*torch.randn(2, generator=g, dtype=torch.float64).tolist())
            f = f + amp * torch.exp(2j * torch.pi * sum(int(kk) * ax for kk, ax in zip(k, axes)))
        maps[c] = f.to(Z)
    return maps / torch.sqrt((maps.abs() ** 2).sum(dim=0))


def measure(dtype, size, ncoils, reps, cg_iters):
    N = (size,) * 3
    Z = torch.complex128 if dtype == "c128" else torch.complex64
    rb = 8 if dtype == "c128" else 4
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    u = torch.randn(tuple(reversed(N)), generator=g, device=dev, dtype=Z)
    maps = smooth_maps(ncoils, u.shape, Z, dev)
    spec = poisson_spectrum(N, 0.15, Z, dev)

    def operator(inpass):
        plan = nufft.PlanNUFFT(Z, N, m=4, sigma=2.0, backend=nufft.ROCBackend(0), options={"NUFFT_TOEPLITZ_MAPS_INPASS": inpass})
        op = nufft.ToeplitzOperator(plan)
        plan.close()
        assert op.path == "fused"
        return op.set_spectrum(spec)

    inpass, streaming, plain = operator(1).set_maps(maps), operator(0).set_maps(maps), operator(1)
    del spec
    g_in, g_st, g_t, tmp, g1 = (torch.empty_like(u) for _ in range(5))

    def torch_apply(x, out):
        for c in range(ncoils):
            torch.mul(maps[c], x, out=tmp)
            plain.apply(tmp, out=g1)
            if c == 0:
                torch.mul(maps[c].conj(), g1, out=out)
            elif fused_accumulate[0]:
                out.addcmul_(maps[c].conj(), g1)
            else:
                out.add_(maps[c].conj() * g1)
        return out

    fused_accumulate = [True]        # addcmul_ on complex tensors where this torch has it (one pass), else multiply and add
    try:
        torch_apply(u, g_t)
    except RuntimeError:
        fused_accumulate[0] = False

    sol = nufft.ToeplitzCG(inpass, maxiter=cg_iters, rtol=0.0, lam=0.0, check_every=0)
    b = torch.randn(u.shape, generator=g, device=dev, dtype=Z)
    x_lib = torch.empty_like(b)
    Gp = torch.empty_like(b)

    def cg_library():
        sol.solve(b, out=x_lib)

    def cg_torch():          # the README's loop with the coil loop inside
        x = torch.zeros_like(b); r = b.clone(); p = r.clone(); rr = torch.vdot(r.flatten(), r.flatten()).real      # noqa: E702
        for _ in range(cg_iters):
            torch_apply(p, Gp)
            alpha = rr / torch.vdot(p.flatten(), Gp.flatten()).real
            x += alpha * p; r -= alpha * Gp      # noqa: E702
            rr_new = torch.vdot(r.flatten(), r.flatten()).real
            p = r + (rr_new / rr) * p; rr = rr_new      # noqa: E702
        return x

    routes = [("inpass_apply", lambda: inpass.apply(u, out=g_in)), ("streaming_apply", lambda: streaming.apply(u, out=g_st)),
              ("torch_loop_apply", lambda: torch_apply(u, g_t)), ("cg_library", cg_library), ("cg_torch_loop", cg_torch)]
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
    rel = lambda a, b: float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))      # noqa: E731
    x_t = cg_torch()
    torch.cuda.synchronize()
    by = route_bytes(N, 2 * rb, rb)
    # coil 0 reads no running output: one array less than `ncoils` times the per-coil figure
    total = {k: ncoils * v - (u.numel() * 2 * rb if k != "plain_apply" else 0) for k, v in by.items()}
    out = {"metric": "sense_apply_ms", "value": med["inpass_apply"], "dtype": dtype, "N": N, "ncoils": ncoils, "cg_iterations": cg_iters,
           "torch_loop_accumulates_with": "addcmul_" if fused_accumulate[0] else "mul + add_",
           "ms": {k: round(x, 4) for k, x in med.items()}, "ms_min_max": {k: [round(a, 4), round(b, 4)] for k, (a, b) in spread.items()},
           "ms_per_cg_iteration": {"library": round(med["cg_library"] / cg_iters, 4), "torch_loop": round(med["cg_torch_loop"] / cg_iters, 4)},
           "ratio_inpass_over_torch_loop": round(med["inpass_apply"] / med["torch_loop_apply"], 3),
           "ratio_streaming_over_torch_loop": round(med["streaming_apply"] / med["torch_loop_apply"], 3),
           "ratio_inpass_over_streaming": round(med["inpass_apply"] / med["streaming_apply"], 3),
           "ratio_cg_library_over_torch_loop": round(med["cg_library"] / med["cg_torch_loop"], 3),
           "bytes_per_coil": by, "inpass_gb_per_s": round(total["inpass"] / (med["inpass_apply"] * 1e-3) / 1e9, 1),
           "streaming_gb_per_s": round(total["streaming"] / (med["streaming_apply"] * 1e-3) / 1e9, 1),
           "workspace_mb": {"inpass": round(inpass.info().workspace_bytes / 1e6, 1), "streaming": round(streaming.info().workspace_bytes / 1e6, 1)},
           "agreement": {"inpass_vs_torch_loop": rel(g_in, g_t), "streaming_vs_torch_loop": rel(g_st, g_t), "inpass_vs_streaming": rel(g_in, g_st),
                         "cg_library_vs_torch_loop": rel(x_lib, x_t)}}
    for k in acc:
        print(f"  {dtype} {k:20s} {med[k]:9.3f} ms   (min {spread[k][0]:.3f}, max {spread[k][1]:.3f})", flush=True)
    sol.close()
    for op in (inpass, streaming, plain):
        op.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--coils", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cg-iters", type=int, default=5)
    ap.add_argument("--dtypes", default="c128,c64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sense_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sense_bench.py measures on the GPU: no device found")
    results = []
    for dtype in args.dtypes.split(","):
        results.append(measure(dtype, args.size, args.coils, args.reps, args.cg_iters))
        print(json.dumps(results[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
