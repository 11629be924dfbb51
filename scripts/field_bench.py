"""Off-resonance correction measurement: the segmented Toeplitz operator at N = 256² and 256³, L = 4 and 8 segments,
without coil maps and with 8, ComplexF32 and ComplexF64; and the two kernels of the segment fit.

Times, in one process and alternating rep by rep (hipEvent medians after warm-up), per apply and per CG iteration:
  * composed      the only route without the segmented operator: a coupled operator on an L-plan, the products B_b ⊙ u, Σ_a conj(B_a) ⊙ ·
                  and the coil products in torch, the coils looped in Python; its CG is a torch loop around that apply
  * plain         one plain fused apply of a one-component operator (with the same coil maps): L of them per coil plus two streaming
                  passes is the floor of the segmented apply
  * segmented     the segmented apply, and ToeplitzCG on it
The spectra are analytic (Poisson kernels; the cross blocks a phase-shifted, damped copy) and the factors those of a smooth field map:
the cost of an apply does not depend on the values.  A configuration whose two block operators do not fit the free device memory is
recorded as skipped.  `interpolators` (Np = 1e7, L = 8, nbins = 256) is reported with FP64 FMA/s over its algorithmic count
4 · Np · L · nbins, `factors` with bytes/s over n · (real + L complex).  Writes profiles/field_bench.json and prints one JSON line per
configuration.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nufft_pkg import nufft  # noqa: E402
from sense_bench import poisson_spectrum, smooth_maps  # noqa: E402
from subspace_bench import spectra  # noqa: E402


def timed(routes, reps, warm=2):
    for _ in range(warm):
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
    spread = {k: [round(min(x), 4), round(max(x), 4)] for k, x in acc.items()}
    return med, spread


def smooth_omega(shape, T, dev, span=6 * torch.pi):
    axes = [torch.linspace(-1, 1, n, device=dev, dtype=torch.float64) for n in shape]
    grids = torch.meshgrid(*axes, indexing="ij")
    f = sum((0.5 + 0.5 * i) * g for i, g in enumerate(grids)) + 0.1 * torch.sin(3 * grids[-1]) * torch.cos(2 * grids[0])
    f = f - f.min()
    return (f * (span / f.max())).to(T).contiguous()


def block_bytes(N, L, rb):
    cells, half = 1, 1
    for d, n in enumerate(N):
        cells *= 2 * n
        half *= n if d == 0 else 2 * n
    return L * cells * rb + L * (L - 1) // 2 * cells * 2 * rb + L * half * 2 * rb


def measure(dtype, N, L, ncoils, reps, cg_iters):
    Z = torch.complex128 if dtype == "c128" else torch.complex64
    T = torch.float64 if dtype == "c128" else torch.float32
    rb = 8 if dtype == "c128" else 4
    dev = torch.device("cuda", 0)
    shape = tuple(reversed(N))
    cells2 = 1
    for n in N:
        cells2 *= 2 * n
    need = 2 * block_bytes(N, L, rb) + (L * (L + 1) // 2 + 3) * cells2 * 2 * rb
    free = torch.cuda.mem_get_info(dev)[0]
    base = {"metric": "segmented_apply_ms", "dtype": dtype, "N": list(N), "L": L, "ncoils": ncoils, "cg_iterations": cg_iters}
    if need > 0.85 * free:
        return dict(base, value=None, skipped=f"needs about {need / 1e9:.0f} GB for the two block operators and the spectra, {free / 1e9:.0f} GB free")
    g = torch.Generator(device=dev).manual_seed(0)
    u = torch.randn(shape, generator=g, device=dev, dtype=Z)
    plan1 = nufft.PlanNUFFT(Z, N, m=4, sigma=2.0, backend=nufft.ROCBackend(0))
    planL = nufft.PlanNUFFT(Z, N, m=4, sigma=2.0, ntransforms=L, backend=nufft.ROCBackend(0))
    sp = spectra(N, L, Z, dev)
    seg = nufft.ToeplitzOperator(plan1, segments=L).set_spectra(sp)
    cop = nufft.ToeplitzOperator(planL).set_spectra(sp)
    plain = nufft.ToeplitzOperator(plan1).set_spectrum(sp[0])
    del sp
    torch.cuda.empty_cache()
    assert seg.path == cop.path == plain.path == "fused" and cop.coupled and seg.segments == L
    omega = smooth_omega(shape, T, dev)
    fs = nufft.FieldSegments(seg, L).fit(omega, t_range=(0.0, 1.0))
    B = fs.factors(omega)
    seg.set_factors(B)
    maps = None
    if ncoils:
        maps = smooth_maps(ncoils, shape, Z, dev)
        seg.set_maps(maps)
        plain.set_maps(maps)
    ins = tuple(torch.empty_like(u) for _ in range(L))
    gs = tuple(torch.empty_like(u) for _ in range(L))
    out_s, out_p, out_c, tmp = (torch.empty_like(u) for _ in range(4))

    def composed(v=u, out=out_c):
        out.zero_()
        for c in range(max(ncoils, 1)):
            src = v if maps is None else maps[c] * v
            for b in range(L):
                torch.mul(B[b], src, out=ins[b])
            cop.apply(ins if L > 1 else ins[0], out=gs if L > 1 else gs[0])
            tmp.zero_()
            for a in range(L):
                tmp.addcmul_(B[a].conj(), gs[a])
            if maps is None:
                out.add_(tmp)
            else:
                out.addcmul_(maps[c].conj(), tmp)
        return out

    b = torch.randn(shape, generator=g, device=dev, dtype=Z)
    x_s = torch.empty_like(b)
    sol = nufft.ToeplitzCG(seg, maxiter=cg_iters, rtol=0.0, lam=0.0, check_every=0)
    q = torch.empty_like(b)

    def cg_composed():
        x, r = torch.zeros_like(b), b.clone()
        p = r.clone()
        rho = torch.vdot(r.flatten(), r.flatten()).real
        for _ in range(cg_iters):
            composed(p, q)
            alpha = rho / torch.vdot(p.flatten(), q.flatten()).real
            x.add_(alpha * p)
            r.sub_(alpha * q)
            rho_new = torch.vdot(r.flatten(), r.flatten()).real
            p.mul_(rho_new / rho).add_(r)
            rho = rho_new
        return x

    routes = [("segmented_apply", lambda: seg.apply(u, out=out_s)), ("composed_apply", composed), ("plain_apply", lambda: plain.apply(u, out=out_p)),
              ("cg_segmented", lambda: sol.solve(b, out=x_s)), ("cg_composed", cg_composed)]
    med, spread = timed(routes, reps)
    agree = float((out_s - out_c).norm() / out_c.norm())
    out = dict(base, value=round(med["segmented_apply"], 4), ms={k: round(x, 4) for k, x in med.items()}, ms_min_max=spread,
               ms_per_cg_iteration={"segmented": round(med["cg_segmented"] / cg_iters, 4), "composed": round(med["cg_composed"] / cg_iters, 4)},
               ratio_segmented_over_composed=round(med["segmented_apply"] / med["composed_apply"], 4),
               ratio_segmented_over_floor=round(med["segmented_apply"] / (L * med["plain_apply"]), 4),
               segmented_against_composed_rel_l2=agree,
               workspace_mb={"segmented": round(seg.info().workspace_bytes / 1e6, 1), "composed_operator": round(cop.info().workspace_bytes / 1e6, 1)})
    for k in med:
        print(f"  {dtype} N={N} L={L} coils={ncoils} {k:16s} {med[k]:9.3f} ms   (min {spread[k][0]:.3f}, max {spread[k][1]:.3f})", flush=True)
    sol.close()
    fs.close()
    for op in (seg, cop, plain):
        op.close()
    plan1.close()
    planL.close()
    return out


def measure_fit(dtype, npoints, ncells, L, nbins, reps):
    Z = torch.complex128 if dtype == "c128" else torch.complex64
    T = torch.float64 if dtype == "c128" else torch.float32
    rb = 8 if dtype == "c128" else 4
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    omega = (torch.rand(ncells, generator=g, device=dev, dtype=torch.float64) * 6 * torch.pi).to(T)
    times = torch.rand(npoints, generator=g, device=dev, dtype=torch.float64).to(T)
    fs = nufft.FieldSegments(Z, L, nbins=nbins, device=dev).fit(omega, t_range=(0.0, 1.0))
    phi = torch.empty((L, npoints), dtype=Z, device=dev)
    B = tuple(torch.empty(ncells, dtype=Z, device=dev) for _ in range(L))
    med, spread = timed([("interpolators", lambda: fs.interpolators(times, out=phi)), ("factors", lambda: fs.factors(omega, out=B)),
                         ("fit", lambda: fs.fit(omega, t_range=(0.0, 1.0)))], reps)
    fmas = 4.0 * npoints * L * nbins
    nbytes = ncells * (rb + L * 2 * rb)
    out = {"metric": "interpolators_ms", "value": round(med["interpolators"], 4), "dtype": dtype, "npoints": npoints, "ncells": ncells, "L": L, "nbins": nbins,
           "ms": {k: round(x, 4) for k, x in med.items()}, "ms_min_max": spread,
           "interpolators_fp64_tfma_per_s": round(fmas / (med["interpolators"] * 1e-3) / 1e12, 3),
           "factors_gb_per_s": round(nbytes / (med["factors"] * 1e-3) / 1e9, 1)}
    fs.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x256,256x256x256")
    ap.add_argument("--segments", default="4,8")
    ap.add_argument("--coils", default="0,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cg-iters", type=int, default=3)
    ap.add_argument("--npoints", type=int, default=10_000_000)
    ap.add_argument("--dtypes", default="c64,c128")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("field_bench.py measures on the GPU: no device found")
    results = []

    def keep(r):
        results.append(r)
        print(json.dumps(r), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:          # rewritten after every configuration: an interrupted run keeps what it measured
            json.dump({"results": results}, f, indent=1)
            f.write("\n")

    for dtype in args.dtypes.split(","):
        keep(measure_fit(dtype, args.npoints, 256 ** 3, 8, 256, args.reps))
        torch.cuda.empty_cache()
    for dtype in args.dtypes.split(","):
        for shape in args.shapes.split(","):
            N = tuple(int(n) for n in shape.split("x"))
            for L in (int(k) for k in args.segments.split(",")):
                for ncoils in (int(c) for c in args.coils.split(",")):
                    keep(measure(dtype, N, L, ncoils, args.reps, args.cg_iters))
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
