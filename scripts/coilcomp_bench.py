"""Coil compression measurement: CoilCompressor in ComplexF32 and ComplexF64.

  * ``compress``   n = 1e7 samples, (C, V) = (32, 8) and (64, 16): ``accumulate`` (the Gram kernel and its fold), ``finish`` (the
                   one-workgroup eigen launch) and ``apply``, each timed on its own.  The Gram kernel is rated over its algorithmic
                   bytes (C · n elements plus n weights) and its FP64 FMA count (4 per complex product, C (C + 1) / 2 products per
                   sample); apply over (C + V) · n elements, with ``coil_combine`` over the same C · n elements (C inputs, one output;
                   the inputs also serve as its maps, so the distinct bytes are (C + 1) · n elements) measured in the same run as the
                   yardstick.  Next to them
                   the same algorithm in torch: the stacking copy that the tuple-of-vectors layout forces on it, a complex ``matmul``
                   for the Gram matrix, ``torch.linalg.eigh``, a ``matmul`` for the apply.
  * ``jacobi``     the sweeps and the time of ``finish`` at C = 64 (and 32, 16, 8) on a designed spectrum.
  * ``maps``       ``estimate_maps`` at 64³, box 3, on 32 coils against compress 32 → 8 plus the estimate on 8.
  * ``sense``      a SENSE ``ToeplitzOperator.apply`` at 128³ with 32 maps against 8.

Times are hipEvent medians of ``--reps`` after a warm-up, the routes alternating rep by rep in one process per part and element type.
Every part runs in a child process of its own under a time limit.  The document (--out) is written after every child, so a failure or a
time limit leaves what was measured before it, and ``not_measured`` names the rest.  Prints the document at the end.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maps_bench as MB  # noqa: E402
import tvt_bench as TB  # noqa: E402

COMPRESS = {"c32_v8": (32, 8), "c64_v16": (64, 16)}


def vectors(torch, C, n, Z, dev, rho=0.8):
    """C vectors whose covariance has a geometric spectrum: a fixed unitary mix of independent noise of variance rho^k."""
    g = torch.Generator(device=dev).manual_seed(0)
    q, _ = torch.linalg.qr(torch.randn((C, C), generator=g, device=dev, dtype=torch.complex128))
    src = torch.randn((C, n), generator=g, device=dev, dtype=Z) * (rho ** (torch.arange(C, device=dev) / 2)).to(Z)[:, None]
    mixed = q.to(Z) @ src
    del src
    return tuple(mixed[c].clone() for c in range(C))


def compress(dtype, args):
    import torch
    from nufft_pkg import nufft
    C, V = COMPRESS[args.case]
    n = args.n
    dev = torch.device("cuda", 0)
    Z = torch.complex128 if dtype == "c128" else torch.complex64
    eb = 16 if dtype == "c128" else 8
    y = vectors(torch, C, n, Z, dev)
    h = torch.rand(n, device=dev, dtype=torch.float64 if dtype == "c128" else torch.float32)
    out = tuple(torch.empty(n, dtype=Z, device=dev) for _ in range(V))
    comb = torch.empty(n, dtype=Z, device=dev)
    cc = nufft.CoilCompressor(Z, C, device=dev)
    cc.fit(y, weights=h)
    lam, sweeps, status = cc.spectrum()
    A = torch.from_numpy(cc.matrix(V)).to(dev)

    def gram():
        cc.reset()
        cc.accumulate(y, h)

    keep = {}

    def t_stack():
        keep["s"] = torch.stack(y)

    def t_gram():
        s = keep["s"]
        keep["R"] = (s * h) @ s.conj().T

    def t_eigh():
        keep["e"] = torch.linalg.eigh(keep["R"])

    def t_apply():
        keep["o"] = A.to(Z) @ keep["s"]

    routes = [("accumulate", gram), ("finish", cc.finish), ("apply", lambda: cc.apply(y, V, out=out)),
              ("coil_combine", lambda: nufft.coil_combine(y, y, out=comb)),
              ("torch_stack", t_stack), ("torch_gram", t_gram), ("torch_eigh", t_eigh), ("torch_apply", t_apply)]
    for name, fn in routes:
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
    med, minmax = TB.measure(torch, routes, args.reps, {name: 1 for name, _ in routes})
    # the two routes agree: the Gram matrix, and the virtual coils up to the rounding of the element type
    R = torch.from_numpy(cc.gram()).to(dev)
    gram_diff = float((keep["R"].to(torch.complex128) - R).abs().max() / R.abs().max())
    apply_diff = float((torch.stack(out) - keep["o"]).abs().max() / keep["o"].abs().max())
    info = cc.info(n)
    fma = 4 * (C * (C + 1) // 2) * n
    gram_bytes = C * n * eb + n * eb // 2
    apply_bytes = (C + V) * n * eb
    comb_bytes = (C + 1) * n * eb            # the maps alias the inputs: each element comes from memory once
    s = lambda name: med[name] * 1e-3   # noqa: E731
    r = {"coils": C, "virtual": V, "n": n, "jacobi_sweeps": sweeps, "status": status, "energy_kept": round(float(lam[:V].sum() / lam.sum()), 4),
         "ms": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": minmax,
         "tile_samples": info.tile_samples, "segments": info.segments, "tiles_per_workgroup": info.tiles_per_workgroup, "workgroups": info.workgroups,
         "lds_bytes_gram": info.lds_bytes_gram, "lds_bytes_eigen": info.lds_bytes_eigen,
         "gram": {"algorithmic_gb": round(gram_bytes / 1e9, 3), "tb_per_s": round(gram_bytes / s("accumulate") / 1e12, 3),
                  "fp64_gfma": round(fma / 1e9, 2), "tfma_per_s": round(fma / s("accumulate") / 1e12, 3),
                  "lds_complex_reads_g": round(2 * (C * (C + 1) // 2) * n / 1e9, 2)},
         "apply": {"algorithmic_gb": round(apply_bytes / 1e9, 3), "tb_per_s": round(apply_bytes / s("apply") / 1e12, 3)},
         "coil_combine": {"algorithmic_gb": round(comb_bytes / 1e9, 3), "tb_per_s": round(comb_bytes / s("coil_combine") / 1e12, 3)},
         "torch": {"stack_copy_gb": round(C * n * eb / 1e9, 3), "total_ms": round(sum(med[k] for k in med if k.startswith("torch_")), 4),
                   "library_total_ms": round(med["accumulate"] + med["finish"] + med["apply"], 4),
                   "gram_relative_difference": gram_diff, "apply_relative_difference": apply_diff}}
    cc.close()
    return r


def jacobi(dtype, args):
    import torch
    from nufft_pkg import nufft
    dev = torch.device("cuda", 0)
    Z = torch.complex128 if dtype == "c128" else torch.complex64
    r = {}
    for C in (8, 16, 32, 64):
        y = vectors(torch, C, 100000, Z, dev, rho=0.85)
        cc = nufft.CoilCompressor(Z, C, device=dev)
        cc.fit(y)
        routes = [("finish", cc.finish)]
        med, minmax = TB.measure(torch, routes, args.reps, {"finish": 1})
        r[f"c{C}"] = {"ms": round(med["finish"], 4), "ms_min_max": minmax["finish"], "sweeps": cc.last_sweeps()}
        cc.close()
    return r


def maps(dtype, args):
    import torch
    from nufft_pkg import nufft
    N, C, V, box = (64, 64, 64), 32, 8, 3
    dev = torch.device("cuda", 0)
    Z = torch.complex128 if dtype == "c128" else torch.complex64
    plan = nufft.PlanNUFFT(Z, N, backend=nufft.ROCBackend(0))
    a = MB.images(torch, N, C, Z, dev)
    at = tuple(a[c] for c in range(C))
    full, small = nufft.CoilMapEstimator(plan, C, box=box), nufft.CoilMapEstimator(plan, V, box=box)
    plan.close()
    out_full = tuple(torch.empty_like(v) for v in at)
    virt = tuple(torch.empty_like(at[0]) for _ in range(V))
    out_small = tuple(torch.empty_like(v) for v in virt)
    cc = nufft.CoilCompressor(Z, C, device=dev)

    def compressed():
        cc.reset()
        cc.accumulate(at)
        cc.finish()
        cc.apply(at, V, out=virt)
        small.estimate(virt, out=out_small)

    routes = [("estimate_32", lambda: full.estimate(at, out=out_full)), ("compress_and_estimate_8", compressed),
              ("compress_alone", lambda: (cc.reset(), cc.accumulate(at), cc.finish(), cc.apply(at, V, out=virt)))]
    for name, fn in routes:
        fn()
        torch.cuda.synchronize()
    med, minmax = TB.measure(torch, routes, args.reps, {name: 1 for name, _ in routes})
    lam = cc.eigenvalues
    r = {"N": list(N), "coils": C, "virtual": V, "box": box, "ms": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": minmax,
         "energy_kept": round(float(lam[:V].sum() / lam.sum()), 4), "ratio": round(med["estimate_32"] / med["compress_and_estimate_8"], 2)}
    for o in (full, small, cc):
        o.close()
    return r


def sense(dtype, args):
    import torch
    from nufft_pkg import nufft
    import sense_bench as SB
    N = (128, 128, 128)
    dev = torch.device("cuda", 0)
    Z = torch.complex128 if dtype == "c128" else torch.complex64
    g = torch.Generator(device=dev).manual_seed(0)
    u = torch.randn(tuple(reversed(N)), generator=g, device=dev, dtype=Z)
    spec = SB.poisson_spectrum(N, 0.15, Z, dev)
    ops, outs = {}, {}
    for C in (32, 8):
        plan = nufft.PlanNUFFT(Z, N, m=4, sigma=2.0, backend=nufft.ROCBackend(0))
        op = nufft.ToeplitzOperator(plan)
        plan.close()
        ops[C] = op.set_spectrum(spec).set_maps(SB.smooth_maps(C, u.shape, Z, dev))
        outs[C] = torch.empty_like(u)
    routes = [(f"apply_{C}_maps", (lambda C=C: ops[C].apply(u, out=outs[C]))) for C in (32, 8)]
    for name, fn in routes:
        fn()
        torch.cuda.synchronize()
    med, minmax = TB.measure(torch, routes, args.reps, {name: 1 for name, _ in routes})
    return {"N": list(N), "ms": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": minmax,
            "ratio": round(med["apply_32_maps"] / med["apply_8_maps"], 2)}


PARTS = {"compress": compress, "jacobi": jacobi, "maps": maps, "sense": sense}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="compress,jacobi,maps,sense")
    ap.add_argument("--cases", default="c32_v8,c64_v16")
    ap.add_argument("--case", default="c32_v8", help=argparse.SUPPRESS)
    ap.add_argument("--n", type=int, default=10 ** 7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtypes", default="c64,c128")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds every child process may take")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--part", default="compress", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coilcomp_bench.json"))
    args = ap.parse_args()
    if args.worker:
        sys.path.insert(0, ROOT)
        print(json.dumps(PARTS[args.part](args.worker, args)))
        return
    parts, dtypes = args.parts.split(","), args.dtypes.split(",")
    todo = [(p, c, dt) for p in parts for c in (args.cases.split(",") if p == "compress" else [p]) for dt in dtypes]
    out = {"metric": "coil_compression_ms", "n": args.n, "reps": args.reps, "warmup": args.warmup, "results": {}, "value": None, "not_measured": []}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for i, (part, case, dt) in enumerate(todo):
        argv = ["--worker", dt, "--part", part, "--case", case, "--n", str(args.n), "--reps", str(args.reps), "--warmup", str(args.warmup)]
        try:
            out["results"].setdefault(case, {})[dt] = json.loads(run(argv, args.step_timeout))
        except BaseException:
            out["not_measured"] += [f"{c} {d}" for _, c, d in todo[i:]]      # this one and everything after it
            write()
            raise
        if out["value"] is None and part == "compress":
            out["value"] = out["results"][case][dt]["ms"]["accumulate"]
        print(f"  {case} {dt}: {json.dumps(out['results'][case][dt].get('ms', out['results'][case][dt]))}", file=sys.stderr)
        write()
    print(json.dumps(out))


def run(argv, limit):
    import subprocess
    done = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, stdout=subprocess.PIPE, timeout=limit, check=True)
    return done.stdout.decode().strip().splitlines()[-1]


if __name__ == "__main__":
    main()
