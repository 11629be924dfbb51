"""Sample-density compensation on the GPU against the numpy restatement (dcf_reference.py).

The reference runs in the element type of the plan.  Where the un-normalised window overflows Float32 in the reference's formulation
(C 1 is about 1e45 in 3-D at M = 4 and 1e62 in 2-D at M = 8) it runs in Float64 on points located in Float32 exactly as a Float32 plan
locates them (``coord_dtype``), as tests/test_gpu_parity.py does for such plans.

Bars.  Measured on an MI355X over the 21 parity cases below after 10 iterations (rel-L2 of w; largest relative deviation of the history):
Float64 at most 4.9e-15 and 3.7e-13 (the history of the 1-D uniform set with 2e5 points, whose δ is small), Float32 at most 8.4e-6 and
2.4e-5 (DESIGN.md §18 lists them per case).  The bars are 10 × the largest value per element type, below the cap of 100 × the spread /
interpolation parity bar of tests/test_gpu_parity.py (1e-12 and 1e-5 on the grid): 1e-10 and 1e-3.  Every other test of this file uses
the same two bars.
"""
import faulthandler

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import cg_reference as CG  # noqa: E402
import dcf_reference as D  # noqa: E402
import toeplitz_reference as R  # noqa: E402
from oracle import nufft_oracle as O  # noqa: E402

BAR_W = {np.float64: 5e-14, np.float32: 8.4e-5}        # rel-L2 of the weights
BAR_H = {np.float64: 3.7e-12, np.float32: 2.4e-4}        # largest relative deviation of the history
for _T, _cap in ((np.float64, 1e-10), (np.float32, 1e-3)):
    assert BAR_W[_T] <= _cap and BAR_H[_T] <= _cap


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test under its own time limit: a hang ends the process with a traceback instead of holding the GPU."""
    faulthandler.dump_traceback_later(420, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


def points(kind, ndim, Np, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return [rng.random(Np) * 2 * np.pi for _ in range(ndim)]
    if kind == "clustered":                      # half uniform, half N(0, 0.4²)
        h = Np // 2
        return [np.mod(np.concatenate([rng.random(h) * 2 * np.pi, 0.4 * rng.standard_normal(Np - h)]), 2 * np.pi) for _ in range(ndim)]
    assert kind == "radial"                      # spokes through the centre of the cell, uniform in the radius
    r = (rng.random(Np) * 2 - 1) * np.pi
    if ndim == 1:
        return [np.mod(np.pi + r * np.abs(r) / np.pi, 2 * np.pi)]
    nspokes = max(8, int(np.sqrt(Np)))
    dirs = rng.standard_normal((nspokes, ndim))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    spoke = rng.integers(0, nspokes, Np)
    return [np.mod(np.pi + r * dirs[spoke, d], 2 * np.pi) for d in range(ndim)]


_KERNELS = {"bkb": O.KERNEL_BKB, "kb": O.KERNEL_KB, "gauss": O.KERNEL_GAUSSIAN, "bspline": O.KERNEL_BSPLINE}


def _kernel(nufft, name):
    return {"bkb": nufft.BackwardsKaiserBesselKernel, "kb": nufft.KaiserBesselKernel, "gauss": nufft.GaussianKernel,
            "bspline": nufft.BSplineKernel}[name]()


def _real(Z):
    return np.float32 if Z in ("f32", "c64") else np.float64


def _ztype(Z):
    return {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}[Z]


def make(nufft, Z, Ns, M=4, kernel="bkb", fast=False, nfft=False, fftshift=False, **dc_kw):
    """(DensityCompensation, oracle plan, real type) of one configuration."""
    T = _real(Z)
    kw = dict(point_transform="nfft") if nfft else {}
    plan = nufft.PlanNUFFT(_ztype(Z), Ns, m=M, sigma=2.0, kernel=_kernel(nufft, kernel), backend=nufft.ROCBackend(0),
                           kernel_evalmode=nufft.FastApproximation() if fast else nufft.Direct(),
                           fftshift=fftshift and Z in ("c64", "c128"), **kw)
    dc = nufft.DensityCompensation(plan, **dc_kw)
    plan.close()
    # Float32 reference in its own type where its un-normalised window fits; Float64 on Float32 coordinates otherwise
    wide = T == np.float32 and kernel in ("bkb", "kb") and len(Ns) * M >= 12
    oplan = D.make_plan(Ns, dtype=np.float64 if wide else T, M=M, kernel=_KERNELS[kernel],
                        evalmode=O.FAST_APPROXIMATION if fast else O.DIRECT,
                        point_transform=O.POINT_TRANSFORM_NFFT if nfft else O.POINT_TRANSFORM_IDENTITY,
                        coord_dtype=np.float32 if wide else None)
    assert dc.oversampled_dims == oplan.Nover and list(dc.info().beta)[:len(Ns)] == [float(b) for b in oplan.betas]
    return dc, oplan, T


def coords(xs, T, nfft=False):
    """Host coordinates in the plan's precision (NFFT convention: the same physical points in [-1/2, 1/2))."""
    if nfft:
        xs = [np.mod(-x / (2 * np.pi) + 0.5, 1.0) - 0.5 for x in xs]
    return [np.ascontiguousarray(x.astype(T)) for x in xs]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def hist_dev(got, ref):
    """Largest relative deviation of the history; the NaN pattern must agree."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    m = ~np.isnan(ref)
    return float(np.max(np.abs(got[m] / ref[m] - 1))) if m.any() else 0.0


def run(dc, xs_T, **kw):
    dc.set_points(tuple(dev(x) for x in xs_T))
    w = dc.compute(**kw)
    torch.cuda.synchronize()
    return w.cpu().numpy(), dc.iterations, dc.status, dc.residual, dc.history().numpy()


# (Z, N, M, kernel, fast evaluation, NFFT convention, fftshift, point set, Np)
PARITY = [
    ("f64", (256,), 4, "bkb", False, False, False, "uniform", 200000),
    ("c128", (64, 48), 4, "bkb", True, False, True, "clustered", 50000),
    ("f64", (24, 20, 16), 4, "bkb", False, False, False, "radial", 20000),
    ("c128", (16, 16, 16), 8, "bkb", True, False, False, "clustered", 2000),
    ("f64", (64, 48), 4, "bspline", False, False, False, "uniform", 20001),
    ("c128", (48,), 2, "bkb", True, True, True, "clustered", 2000),
    ("f64", (32, 32), 8, "bkb", False, False, False, "radial", 5000),
    ("c128", (64, 48), 4, "kb", False, True, False, "uniform", 20000),
    ("f64", (40, 36), 4, "gauss", True, False, False, "clustered", 30000),
    ("f32", (256,), 4, "kb", False, False, False, "clustered", 20003),
    ("c64", (64, 48), 4, "gauss", False, False, True, "radial", 200000),
    ("f32", (64, 48), 4, "bkb", True, True, False, "clustered", 50000),
    ("c64", (40, 36), 2, "bkb", False, False, False, "uniform", 20000),
    ("f32", (48, 40), 4, "bspline", True, False, False, "radial", 20000),
    ("c64", (128,), 8, "bkb", True, False, False, "uniform", 2001),
    ("f32", (24, 20, 16), 4, "bkb", False, False, False, "uniform", 20000),
    ("c64", (24, 20, 16), 4, "kb", True, False, True, "clustered", 20002),
    ("f32", (16, 16, 16), 8, "bkb", False, False, False, "radial", 2000),
    ("c64", (32, 32), 8, "bkb", False, False, False, "clustered", 5000),
]


@pytest.mark.parametrize("Z,Ns,M,kernel,fast,nfft,fftshift,kind,Np", PARITY)
def test_parity_with_the_reference_after_ten_iterations(nufft, Z, Ns, M, kernel, fast, nfft, fftshift, kind, Np):
    dc, oplan, T = make(nufft, Z, Ns, M, kernel, fast, nfft, fftshift, maxiter=10, tol=0.0)
    xs = coords(points(kind, len(Ns), Np, seed=Np + M), T, nfft)
    ref = D.pipe_menon(oplan, xs, max_iter=10)
    w, its, status, res, hist = run(dc, xs)
    assert w.dtype == T and np.all(np.isfinite(w)) and np.all(w > 0)
    ew, eh = rel(w, ref["w"]), hist_dev(hist, ref["history"])
    print(f"DCF-PARITY {Z} {Ns} M={M} {kernel} fast={fast} nfft={nfft} shift={fftshift} {kind} Np={Np}: w {ew:.3e} history {eh:.3e}")
    assert (its, status) == (10, "max_iter") and ref["iterations"] == 10
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 8 * np.finfo(T).eps
    assert ew <= BAR_W[T] and eh <= BAR_H[T], (ew, eh)
    assert abs(res / ref["residual"] - 1) <= BAR_H[T]
    i = dc.info()
    assert (i.num_points, i.iterations_enqueued) == (Np, 10) and i.capacity >= Np and i.plan_bytes > 0


@pytest.mark.parametrize("Z,Np", [("f64", 300001), ("f32", 600003)])
def test_more_workgroups_than_threads(nufft, Z, Np):
    """150000 packs (293 workgroups) and a tail of one / three reals: more rows of partials than threads in a workgroup, so the fixed-order
    reduction of the next kernel takes its strided part (thread t reduces rows t, t + 256, ...)."""
    Ns = (65536,)
    dc, oplan, T = make(nufft, Z, Ns, maxiter=3, tol=0.0, normalize="sum")
    xs = coords(points("uniform", 1, Np, seed=Np), T)
    ref = D.pipe_menon(oplan, xs, max_iter=3)
    w, its, status, _, hist = run(dc, xs)
    assert dc.info().workgroups > 256, dc.info().workgroups
    ew, eh = rel(w, ref["w"]), hist_dev(hist, ref["history"])
    print(f"DCF {dc.info().workgroups} workgroups {Z} Np={Np}: w {ew:.3e} history {eh:.3e} (bars {BAR_W[T]:g}, {BAR_H[T]:g})")
    assert (its, status) == (3, "max_iter") and ref["iterations"] == 3
    assert ew <= BAR_W[T] and eh <= BAR_H[T], (ew, eh)
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 8 * np.finfo(T).eps


@pytest.mark.parametrize("M", [4, 8])
def test_float32_three_dimensions_do_not_overflow(nufft, M):
    """C 1 is about 1e45 (M = 4) in the reference's formulation: the device runs on w / 2^κ.  Without normalisation the true weights
    (about 1e-45) are below Float32: they underflow to zero or denormals, finite all the same."""
    Ns, Np = (20, 18, 16), 3000
    dc, oplan, T = make(nufft, "f32", Ns, M, maxiter=10)
    xs = coords(points("clustered", 3, Np, seed=M), T)
    ref = D.pipe_menon(oplan, xs, max_iter=10)
    assert ref["w"].dtype == np.float64 and float(np.max(D.apply_C(oplan, np.ones(Np)))) > 1e39     # beyond Float32
    w, its, status, _, hist = run(dc, xs)
    ew, eh = rel(w, ref["w"]), hist_dev(hist, ref["history"])
    print(f"DCF-PARITY f32-3d M={M}: w {ew:.3e} history {eh:.3e} kappa {dc.info().window_scale_log2}")
    assert np.all(np.isfinite(w)) and np.all(w > 0) and (its, status) == (10, "max_iter")
    assert ew <= BAR_W[T] and eh <= BAR_H[T], (ew, eh)
    dc2, _, _ = make(nufft, "f32", Ns, M, maxiter=10, normalize="none")
    raw = run(dc2, xs)[0]
    assert np.all(np.isfinite(raw)) and np.all(raw >= 0)


def _tolerance(history):
    """Geometric mean of the first two consecutive δ (k >= 2) that differ by more than 5 %: (tol, index of the smaller one)."""
    for k in range(2, len(history) - 1):
        if history[k + 1] < 0.95 * history[k]:
            return float(np.sqrt(history[k] * history[k + 1])), k + 1
    raise AssertionError(history)


@pytest.mark.parametrize("Z,Ns,kind,Np", [("f64", (64,), "uniform", 4000), ("c64", (48, 40), "clustered", 12000)])
def test_freeze_rule_and_the_two_modes(nufft, Z, Ns, kind, Np):
    T = _real(Z)
    xs = coords(points(kind, len(Ns), Np, seed=21), T)
    _, oplan, _ = make(nufft, Z, Ns, maxiter=16)
    tol, stop = _tolerance(D.pipe_menon(oplan, xs, max_iter=16)["history"])
    ref = D.pipe_menon(oplan, xs, max_iter=16, tol=tol)
    assert ref["status"] == D.CONVERGED and ref["iterations"] == stop < 15
    out = []
    for every in (0, 3):
        dc, _, _ = make(nufft, Z, Ns, maxiter=16, tol=tol, check_every=every)
        w, its, status, res, hist = run(dc, xs)
        assert (its, status) == (stop, "converged"), (every, its, status)
        assert rel(w, ref["w"]) <= BAR_W[T] and hist_dev(hist, ref["history"]) <= BAR_H[T]
        assert np.all(np.isnan(hist[stop + 1:])) and np.isnan(hist[0]) and hist[stop] <= tol < hist[stop - 1] and res == hist[stop]
        enq = dc.info().iterations_enqueued
        assert enq == 16 if every == 0 else enq == min(16, -(-(stop + 1) // 3) * 3), (every, enq, stop)
        out.append(w)
    assert rel(out[0], out[1]) <= BAR_W[T]


def test_hipgraph_capture(nufft):
    Z, Ns, Np = "f64", (48, 40), 12000
    T = _real(Z)
    xs = coords(points("clustered", 2, Np, seed=3), T)
    dc, _, _ = make(nufft, Z, Ns, maxiter=8)
    eager, its, status, _, hist = run(dc, xs)
    checking, _, _ = make(nufft, Z, Ns, maxiter=8, check_every=2)
    checking.set_points(tuple(dev(x) for x in xs))
    out = torch.zeros(Np, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        dc.compute(out=out)
        with pytest.raises(ValueError):                         # check_every > 0 synchronises: refused while capturing
            checking.compute(out=out)
    for _ in range(2):
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert (dc.iterations, dc.status) == (its, status)
        assert rel(out.cpu().numpy(), eager) <= BAR_W[T] and hist_dev(dc.history().numpy(), hist) <= BAR_H[T]
    del graph


def test_warm_start(nufft):
    """A start equal to the un-normalised result of 6 iterations: δ_0 is the δ that run would have computed next (δ_6 of a longer run),
    and the iterates continue that run.  The same start scaled by 7 gives the same iterates from the first division on (w / (C w) does not
    depend on the scale), so its history continues the longer run from entry 1, while its δ_0 = max |7 C w − 1| measures the scale:
    as the header's algorithm states it, δ is not scale-invariant, and only the unscaled start reproduces the next δ at entry 0."""
    Z, Ns, Np = "f64", (48, 40), 12000
    T = _real(Z)
    xs = coords(points("clustered", 2, Np, seed=5), T)
    long, oplan, _ = make(nufft, Z, Ns, maxiter=10, normalize="none")
    _, _, _, _, hlong = run(long, xs)
    first, _, _ = make(nufft, Z, Ns, maxiter=6, normalize="none")
    w6 = run(first, xs)[0]
    ref6 = D.pipe_menon(oplan, xs, max_iter=6, normalize="none")
    assert rel(w6, ref6["w"]) <= BAR_W[T]                        # true units: the factor 2^κ is back
    warm, _, _ = make(nufft, Z, Ns, maxiter=4, normalize="none")
    w10, its, status, _, h = run(warm, xs, w0=dev(w6))
    assert (its, status) == (4, "max_iter")
    assert np.max(np.abs(h / hlong[6:10] - 1)) <= BAR_H[T], (h, hlong)          # δ_0 = the previous run's next δ, then δ_7 ...
    seven, _, _ = make(nufft, Z, Ns, maxiter=4, normalize="none")
    w10s, _, _, _, hs = run(seven, xs, w0=dev(7.0 * w6))
    v6 = D.apply_C(oplan, ref6["w"])
    assert abs(hs[0] / float(np.max(np.abs(7.0 * v6 - 1))) - 1) <= BAR_H[T]
    assert np.max(np.abs(hs[1:] / hlong[7:10] - 1)) <= BAR_H[T], (hs, hlong)
    assert rel(w10s, w10) <= BAR_W[T] and rel(w10, D.pipe_menon(oplan, xs, max_iter=10, normalize="none")["w"]) <= BAR_W[T]


def test_bad_start_breaks_down_and_leaves_w_alone(nufft):
    Z, Ns, Np = "f32", (48, 40), 5001
    T = _real(Z)
    xs = coords(points("uniform", 2, Np, seed=8), T)
    dc, _, _ = make(nufft, Z, Ns, maxiter=5)
    w0 = np.full(Np, 0.25, dtype=T)
    w0[Np - 1] = 0.0                                             # in the tail behind the last 16-byte pack
    w, its, status, res, hist = run(dc, xs, w0=dev(w0))
    assert (its, status) == (0, "breakdown") and np.array_equal(w, w0) and np.isnan(res) and np.all(np.isnan(hist))
    w0[Np - 1], w0[17] = 0.25, np.nan
    w, its, status, _, _ = run(dc, xs, w0=dev(w0))
    assert (its, status) == (0, "breakdown") and np.array_equal(w, w0, equal_nan=True)
    good = run(dc, xs)                                           # the object is usable afterwards
    assert good[2] == "max_iter" and np.all(good[0] > 0)


def test_point_set_reuse_and_empty_sets(nufft):
    Z, Ns = "f64", (48, 40)
    T = _real(Z)
    dc, oplan, _ = make(nufft, Z, Ns, maxiter=5)
    host_plan = nufft.PlanNUFFT(np.float64, Ns, backend=None)
    host_dc = nufft.DensityCompensation(host_plan, maxiter=5)
    assert dc.info().workspace_bytes == host_dc.info().workspace_bytes      # a host-only object of the same parameters
    host_dc.close()
    host_plan.close()
    buf = torch.zeros(8, dtype=torch.float64, device="cuda")
    assert nufft.lib.nufft_dcf_compute(dc._handle, buf.data_ptr(), 0, None) == nufft._lib.ERR_NO_POINTS      # no points yet
    with pytest.raises(ValueError):
        dc.compute()
    caps = []
    for Np, seed in ((3000, 1), (9000, 2), (1000, 3)):           # more points, then fewer, on the same object
        xs = coords(points("clustered", 2, Np, seed=seed), T)
        w = run(dc, xs)[0]
        assert rel(w, D.pipe_menon(oplan, xs, max_iter=5)["w"]) <= BAR_W[T], Np
        caps.append(dc.info().capacity)
    assert caps == [3000, 9000, 9000]
    dc.set_points((torch.zeros(0, dtype=torch.float64, device="cuda"),) * 2)
    assert dc.compute().numel() == 0                             # a no-op


def test_weights_halve_the_cg_iterations_end_to_end(nufft):
    """density_weights → ToeplitzOperator.set_points(points, w) → ToeplitzCG on a (48, 40) complex plan (the fused Toeplitz path), the
    clustered set with 6000 uniform + 6000 N(0, 0.4²) points.  The numpy reference alone takes 171 iterations with uniform weights and
    41 with the weights of 20 Pipe–Menon iterations (exact Toeplitz apply, rtol 1e-6)."""
    Ns, Np = (48, 40), 12000
    rng = np.random.default_rng(7)
    h = Np // 2
    xs = [np.mod(np.concatenate([rng.random(h) * 2 * np.pi, 0.4 * rng.standard_normal(Np - h)]), 2 * np.pi) for _ in Ns]
    y = rng.standard_normal(Np) + 1j * rng.standard_normal(Np)
    pts = tuple(dev(x) for x in xs)
    plan = nufft.PlanNUFFT(np.complex128, Ns, m=4, sigma=2.0, backend=nufft.ROCBackend(0))
    nufft.set_points(plan, pts)
    w = nufft.density_weights(plan, pts, maxiter=20)
    wref = D.pipe_menon(D.make_plan(Ns), xs, max_iter=20)["w"]
    assert rel(w.cpu().numpy(), wref) <= BAR_W[np.float64]
    counts, refs = [], []
    for wd, wh in ((torch.full_like(w, 1.0 / Np), np.full(Np, 1.0 / Np)), (w, wref)):
        op = nufft.ToeplitzOperator(plan).set_points(pts, wd)
        assert op.path == "fused"
        b = torch.empty(plan.shape, dtype=torch.complex128, device="cuda")
        nufft.exec_type1(b, plan, dev(y) * wd)
        sol = nufft.ToeplitzCG(op, maxiter=400, rtol=1e-6)
        sol.solve(b)
        torch.cuda.synchronize()
        assert sol.status == ("converged",)
        counts.append(sol.iterations[0])
        K = R.multiplier(Ns, R.exact_spectrum(Ns, xs, wh)).real
        got = CG.cg(lambda p: R.apply(Ns, K, p), O.nudft_type1(R.mode_lists(Ns), xs, wh * y), rtol=1e-6, max_iter=400)
        refs.append(got["iterations"])
        sol.close()
        op.close()
    print(f"DCF-CG iterations on the GPU: uniform {counts[0]}, weighted {counts[1]}; reference: {refs[0]}, {refs[1]}")
    assert 2 * refs[1] <= refs[0] and 2 * counts[1] <= counts[0], (counts, refs)
    assert abs(counts[0] - refs[0]) <= 2 and abs(counts[1] - refs[1]) <= 2, (counts, refs)


def test_nfft_plan_sdc(nufft):
    Ns, Np = (48, 40), 6000
    xs = points("clustered", 2, Np, seed=13)
    xn = np.stack([np.mod(-x / (2 * np.pi) + 0.5, 1.0) - 0.5 for x in xs], axis=1)
    p = nufft.NFFTPlan(dev(xn), Ns, m=4, sigma=2.0)
    w = p.sdc(iters=10)
    ref = D.pipe_menon(D.make_plan(Ns, point_transform=O.POINT_TRANSFORM_NFFT), [np.ascontiguousarray(xn[:, d]) for d in range(2)],
                       max_iter=10)["w"]
    assert rel(w.cpu().numpy(), ref) <= BAR_W[np.float64]
