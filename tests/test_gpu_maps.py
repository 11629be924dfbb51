"""The coil sensitivity map estimate on the GPU against numpy (maps_reference.py: ``walsh(eigh=np.linalg.eigh)`` in
float64 on the same images rounded to the element type).  Cases and images: maps_cases.py.

Bars, per case, with ε_T = 2^-52 or 2^-23:
  * every cell: ‖S_gpu(x) − S_ref(x)‖₂ <= bar ε_T, |λ1 − λ1_ref| <= 2 bar ε_T λ1_ref, |λ2 − λ2_ref| <= bar ε_T λ1_ref, with
    bar = max(16, 4 x the largest per-cell difference, in ε, of the reference's Jacobi against ``np.linalg.eigh`` on that case), the
    figure test_maps_host.py prints and checks against maps_cases.SELF_EPS.  The factor 4 covers the kernel's own summation order over
    up to 125 box cells, fused multiply-adds and, for ComplexF32, the single rounding at the store.  The bar comes from the reference,
    never from the kernel.  No cell is left out: the host test asserts a relative gap (λ1 − λ2) / λ1 >= 0.5 and |s| >= 0.05 everywhere.
  * Σ_c |S_c|² = 1 within 8 ε_T; 2 <= sweeps < 24 for C > 1, 0 sweeps for C = 1; the input is only read.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import maps_cases as MC  # noqa: E402
import maps_reference as M  # noqa: E402

TYPES = ["c128", "c64"]
MID = ((32, 40), 4, (5, 5))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(xs):
    return np.stack([v.cpu().numpy() for v in xs])


def _estimator(nufft, Z, Ns, ncoils, box, crop=0.0):
    plan = nufft.PlanNUFFT(MC.dt(Z)[1], Ns, backend=nufft.ROCBackend(0))
    est = nufft.CoilMapEstimator(plan, ncoils, box=box, crop=crop)
    plan.close()
    return est


def _compare(tag, Ns, C_, box, eps, got, l1, l2, want, w1, w2):
    bar = MC.bar(Ns, C_, box)
    ev = MC.per_cell(got, want) / eps
    el = float((np.abs(l1 - w1) / w1).max()) / eps
    e2 = float((np.abs(l2 - w2) / w1).max()) / eps
    print(f"{tag} N={Ns} C={C_} box={box}: maps {ev:.2f} ε (bar {bar:.1f}), λ1 {el:.2f} ε (bar {2 * bar:.1f}), λ2 {e2:.2f} ε of λ1 (bar {bar:.1f})")
    assert ev <= bar and el <= 2 * bar and e2 <= bar


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,ncoils,box", MC.CASES + MC.GLOBAL_CASES)
def test_against_the_reference(Ns, ncoils, box, Z):
    from nufft_pkg import nufft
    _, Zc, _, eps = MC.dt(Z)
    a = MC.images(Ns, ncoils).astype(Zc)
    want, w1, w2, _ = MC.reference(Ns, ncoils, box, Z)
    est = _estimator(nufft, Z, Ns, ncoils, box)
    ad = tuple(_dev(v) for v in a)
    maps = est.estimate(ad)
    sweeps = est.last_sweeps()
    got, l1, l2 = _host(maps), est.lambda1.cpu().numpy().astype(np.float64), est.lambda2.cpu().numpy().astype(np.float64)
    info = est.info()
    print(f"{Z}: {sweeps} sweeps, tile {tuple(info.tile)} ({info.tile_cells} cells), {info.teams} teams of {info.team_lanes}, staged {info.staged}, "
          f"{info.workgroups} workgroups, {info.lds_bytes} B of LDS")
    _compare(Z, Ns, ncoils, box, eps, got, l1, l2, want, w1, w2)
    assert np.array_equal(_host(ad), a)                                             # the input is only read
    norm = (np.abs(got.astype(np.complex128)) ** 2).sum(axis=0)
    print(f"  Σ|S_c|² − 1: {np.abs(norm - 1).max() / eps:.2f} ε (bar 8)")
    assert np.abs(norm - 1).max() <= 8 * eps
    assert (ncoils == 1 and sweeps == 0) or 2 <= sweeps < info.jacobi_sweeps_max == 24
    assert (info.cells, info.ncoils, tuple(info.box)[:len(Ns)]) == (int(np.prod(Ns)), ncoils, box)
    assert info.staged == (0 if (Ns, ncoils, box) in MC.GLOBAL_CASES else 1)         # both routes to the neighbours are covered
    assert all(m.data_ptr() % 16 == 0 for m in maps) and tuple(maps[0].shape) == Ns[::-1]
    if ncoils == 1:
        assert np.array_equal(l2, np.zeros_like(l2))
    if box == (1,) * len(Ns):                                                        # rank 1: λ2 is roundoff of λ1
        assert (l2 <= 16 * eps * l1).all()
    est.close()


@pytest.mark.parametrize("Z", TYPES)
def test_phase_references(Z):
    """A coil index other than 0, a given complex vector and "pca" (maps_cases.PCA_CASE, with p computed by numpy)."""
    from nufft_pkg import nufft
    Ns, ncoils, box = MC.PCA_CASE
    _, Zc, _, eps = MC.dt(Z)
    a = MC.images(Ns, ncoils).astype(Zc)
    ad = tuple(_dev(v) for v in a)
    est = _estimator(nufft, Z, Ns, ncoils, box)
    e2 = np.zeros(ncoils, dtype=np.complex128)
    e2[2] = 1.0
    vec = np.array([0.3 - 0.4j, 0.5, 0.5j, 0.4 - 0.3j])                            # not a unit vector; the reference's |s| >= 0.8 with it
    pca = M.pca_reference(a)
    for name, arg, p in (("coil 2", 2, e2), ("vector", vec, vec), ("vector as tensor", torch.from_numpy(vec), vec), ("pca", "pca", pca)):
        want, w1, w2, info = MC.reference(Ns, ncoils, box, Z, phase=p)
        assert info["min_s"] >= 0.05
        got = _host(est.estimate(ad, phase=arg))
        _compare(f"{Z} phase {name}", Ns, ncoils, box, eps, got, est.lambda1.cpu().numpy().astype(np.float64),
                 est.lambda2.cpu().numpy().astype(np.float64), want, w1, w2)
    got = _host(est.estimate(ad, phase=2))
    assert np.abs(got[2].imag).max() <= eps and got[2].real.min() > 0                # coil 2 is real and positive
    one = _host(nufft.estimate_maps(nufft.PlanNUFFT(Zc, Ns, backend=nufft.ROCBackend(0)), torch.stack(ad), box=box[0], phase=2))
    assert np.array_equal(one, got)                                                  # the one-shot form, a stacked tensor, an integer box
    est.close()


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,ncoils,box", [MID, ((7, 5), 2, (3, 3))])
def test_crop(Ns, ncoils, box, Z):
    """The threshold sits in a gap of 1e-3 between two adjacent eigenvalues of the reference near the median, chosen from the values of
    this element type: the zero pattern is the reference's exactly, zeroed cells are exact zeros and the rest keeps its bits.  (7, 5) has
    an odd number of cells: the ComplexF32 element behind the last 16-byte pack."""
    from nufft_pkg import nufft
    _, Zc, _, eps = MC.dt(Z)
    a = MC.images(Ns, ncoils).astype(Zc)
    _, w1, _, _ = MC.reference(Ns, ncoils, box, Z)
    crop = MC.crop_for(w1)
    want, _, _ = M.walsh(a, box, crop=crop)
    mask = ~np.abs(want).any(axis=0)
    print(f"crop {Z} N={Ns}: crop = {crop:.4f}, masked share {mask.mean():.3f}")
    assert 0.2 <= mask.mean() <= 0.8
    ad = tuple(_dev(v) for v in a)
    plain = _estimator(nufft, Z, Ns, ncoils, box)
    full = _host(plain.estimate(ad))
    plain.close()
    est = _estimator(nufft, Z, Ns, ncoils, box, crop=crop)
    got = _host(est.estimate(ad))
    assert np.array_equal(~np.abs(got).any(axis=0), mask)
    assert not got[:, mask].any() and np.array_equal(got[:, ~mask], full[:, ~mask])
    # the raw call without eigenvalue arrays: the object's own λ1
    out = tuple(torch.full_like(v, 7.0) for v in ad)
    tab = nufft.plan._ptr_table
    nufft.plan._check(nufft.lib.nufft_coilmaps_estimate(est._handle, tab(out), tab(ad), None, None, None, est._stream()))
    assert np.array_equal(_host(out), got)
    assert est.info().workspace_bytes >= a[0].size * (4 if Z == "c64" else 8)
    est.close()
    # the pass on its own, with the level chosen after the estimate: the same bits; level 0 changes nothing; a second level crops more
    plain = _estimator(nufft, Z, Ns, ncoils, box)
    later = plain.estimate(ad)
    assert plain.crop_maps(later, 0.0) is later and np.array_equal(_host(later), full)
    plain.crop_maps(later, crop)
    assert np.array_equal(_host(later), got)
    plain.crop_maps(later, 1.0)                                                      # everything below the maximum itself
    left = np.abs(_host(later)).any(axis=0)
    assert 1 <= left.sum() < (~mask).sum() and np.array_equal(_host(later)[:, left], full[:, left])
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            plain.crop_maps(later, bad)
    with pytest.raises(ValueError, match="no lambda1"):                             # created without crop: no array of its own
        nufft.plan._check(nufft.lib.nufft_coilmaps_apply_crop(plain._handle, tab(later), None, 0.5, plain._stream()))
    with pytest.raises(ValueError, match="overlaps lambda1"):
        nufft.plan._check(nufft.lib.nufft_coilmaps_apply_crop(plain._handle, tab(later), C.c_void_p(later[0].data_ptr()), 0.5, plain._stream()))
    plain.close()


@pytest.mark.parametrize("Z", TYPES)
def test_zero_block(Z):
    from nufft_pkg import nufft
    Ns, ncoils, box = MID
    Zc = MC.dt(Z)[1]
    a = MC.images(Ns, ncoils).astype(Zc)
    a[:, 10:26, 6:20] = 0                                                            # larger than the box of 5 x 5
    est = _estimator(nufft, Z, Ns, ncoils, box)
    got = _host(est.estimate(tuple(_dev(v) for v in a)))
    l1, l2 = est.lambda1.cpu().numpy(), est.lambda2.cpu().numpy()
    inner = (slice(12, 24), slice(8, 18))                                           # cells whose whole box lies in the block
    assert not got[(slice(None),) + inner].any() and not l1[inner].any() and not l2[inner].any()
    assert np.abs(got).sum(axis=0)[0, 0] > 0 and np.isfinite(got).all()
    est.close()


@pytest.mark.parametrize("scale", [2.0 ** 70, 2.0 ** -60])
def test_scaled_single_precision(scale):
    """ComplexF32 images scaled by 2^70 and by 2^-60 keep the bar on the maps: R is FP64.  (λ1 itself, stored in Float32, overflows at
    2^70: it is about 2^140.)"""
    from nufft_pkg import nufft
    Ns, ncoils, box = MID
    eps = MC.dt("c64")[3]
    a = (MC.images(Ns, ncoils).astype(np.complex64) * np.float32(scale)).astype(np.complex64)
    assert np.isfinite(a).all() and (a != 0).all()
    want, w1, _ = M.walsh(a, box)
    est = _estimator(nufft, "c64", Ns, ncoils, box)
    got = _host(est.estimate(tuple(_dev(v) for v in a)))
    ev = MC.per_cell(got, want) / eps
    print(f"c64 scaled by {scale:g}: maps {ev:.2f} ε (bar {MC.bar(Ns, ncoils, box):.1f}), {est.last_sweeps()} sweeps")
    assert ev <= MC.bar(Ns, ncoils, box)
    if scale < 1:
        l1 = est.lambda1.cpu().numpy().astype(np.float64)
        assert (np.abs(l1 - w1) <= 2 * MC.bar(Ns, ncoils, box) * eps * w1).all()
    est.close()


@pytest.mark.parametrize("Z,Ns,ncoils,box", [("c64", (32, 40), 8, (7, 3)), ("c128", (12, 10), 17, (3, 3))])
def test_determinism_and_graph_replay(Z, Ns, ncoils, box):
    """All three kernels (crop > 0): repeated calls, a side stream and two replays of a captured graph give the same bits."""
    from nufft_pkg import nufft
    Zc = MC.dt(Z)[1]
    a = MC.images(Ns, ncoils).astype(Zc)
    crop = MC.crop_for(MC.reference(Ns, ncoils, box, Z)[1])
    est = _estimator(nufft, Z, Ns, ncoils, box, crop=crop)
    ad = tuple(_dev(v) for v in a)
    first = est.estimate(ad, phase=1)
    torch.cuda.synchronize()
    want, want1, want2 = _host(first), est.lambda1.cpu().numpy(), est.lambda2.cpu().numpy()
    assert 0.2 <= (~np.abs(want).any(axis=0)).mean() <= 0.8
    assert np.array_equal(_host(est.estimate(ad, phase=1)), want)
    out = tuple(torch.zeros_like(v) for v in ad)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        est.estimate(ad, phase=1, out=out)
    side.synchronize()
    assert np.array_equal(_host(out), want)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        est.estimate(ad, phase=1, out=out)
    for _ in range(2):
        for o in out + (est.lambda1, est.lambda2):
            o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_host(out), want)
        assert np.array_equal(est.lambda1.cpu().numpy(), want1) and np.array_equal(est.lambda2.cpu().numpy(), want2)
    del graph
    est.close()


def test_into_the_operator():
    """Samples of S_c ρ at about 4000 random points, tapered to low resolution, gridded, estimated: the result matches the reference on the
    same images, goes into the operator without a copy, and the operator solves and preconditions with it."""
    from nufft_pkg import nufft
    Ns, ncoils, box = MID
    eps = MC.dt("c128")[3]
    S, rho = MC.truth(Ns, ncoils)
    rng = np.random.default_rng(5)
    npts = 4000
    pts = tuple(_dev(rng.random(npts) * 2 * np.pi) for _ in Ns)
    coils = nufft.PlanNUFFT(np.complex128, Ns, backend=nufft.ROCBackend(0), ntransforms=ncoils)
    one = nufft.PlanNUFFT(np.complex128, Ns, backend=nufft.ROCBackend(0))
    nufft.set_points(coils, pts)
    y = tuple(torch.empty(npts, dtype=torch.complex128, device="cuda") for _ in range(ncoils))
    nufft.exec_type2(y, coils, tuple(_dev(S[c] * rho) for c in range(ncoils)))
    w = torch.full((npts,), 1.0 / npts, dtype=torch.float64, device="cuda")
    h = nufft.calibration_weights(pts, cutoff=0.5, window="hann")
    a = tuple(torch.empty(coils.shape, dtype=torch.complex128, device="cuda") for _ in range(ncoils))
    nufft.exec_type1(a, coils, tuple(w * h * y_c for y_c in y))
    maps = nufft.estimate_maps(coils, a, box=5, crop=0.0, phase="pca")
    torch.cuda.synchronize()
    ah = _host(a)
    want, w1, w2, info = M.walsh(ah, box, phase_ref=M.pca_reference(ah)) + ({},)
    got = _host(maps)
    ev = MC.per_cell(got, want) / eps
    # the truth, in the same phase convention: S / ‖S‖ with the phase of the estimate's reference
    unit = S / np.sqrt((np.abs(S) ** 2).sum(axis=0))
    s = np.einsum("c...,c...->...", np.conj(unit), want)
    err = np.linalg.norm(unit * (s / np.abs(s)) - want) / np.linalg.norm(unit)
    print(f"into the operator: maps against the reference {ev:.2f} ε (bar {MC.bar(Ns, ncoils, box):.1f}); against the true maps, phase aligned per cell: {err:.3e}")
    assert ev <= MC.bar(Ns, ncoils, box)
    op = nufft.ToeplitzOperator(one).set_points(pts, w).set_maps(maps)
    assert [m.data_ptr() for m in op._maps] == [m.data_ptr() for m in maps] and op.ncoils == ncoils       # no copy
    b = nufft.coil_combine(maps, a)
    x = op.solve(b, maxiter=5, lam=0.1)
    pre = nufft.ToeplitzPreconditioner(op, 0.1)
    torch.cuda.synchronize()
    assert torch.isfinite(torch.view_as_real(x)).all()
    pre.close()
    op.close()
    coils.close()
    one.close()


def test_refusals():
    """Every refusal is an argument check that returns before a launch."""
    from nufft_pkg import nufft
    lib, chk, tab = nufft.lib, nufft.plan._check, nufft.plan._ptr_table
    plan = nufft.PlanNUFFT(np.complex64, (12, 10), backend=nufft.ROCBackend(0))
    real = nufft.PlanNUFFT(np.float64, (12, 10), backend=nufft.ROCBackend(0))
    for make in (lambda: nufft.CoilMapEstimator(plan, 33), lambda: nufft.CoilMapEstimator(plan, 0), lambda: nufft.CoilMapEstimator(plan, 3, box=4),
                 lambda: nufft.CoilMapEstimator(plan, 3, box=(3, 0)), lambda: nufft.CoilMapEstimator(plan, 3, box=(3, 11)),       # box > N
                 lambda: nufft.CoilMapEstimator(plan, 3, box=11), lambda: nufft.CoilMapEstimator(plan, 3, box=(3, 3, 3)),
                 lambda: nufft.CoilMapEstimator(real, 3), lambda: nufft.CoilMapEstimator(plan, 3, crop=-0.1),
                 lambda: nufft.CoilMapEstimator(plan, 3, crop=float("nan")), lambda: nufft.CoilMapEstimator(plan, 3, crop=float("inf")),
                 lambda: nufft.CoilMapEstimator("plan", 3), lambda: nufft.CoilMapEstimator(plan, 3.0)):
        with pytest.raises(ValueError):
            make()
    with pytest.raises(ValueError, match="33 coils"):
        nufft.CoilMapEstimator(plan, 33)
    flat = nufft.PlanNUFFT(np.complex64, (12, 7), backend=nufft.ROCBackend(0))      # box > N on its own: 9 is allowed, N_2 = 7 is smaller
    with pytest.raises(ValueError, match=r"N\[1\] = 7"):
        nufft.CoilMapEstimator(flat, 3, box=(3, 9))
    nufft.CoilMapEstimator(flat, 3, box=(9, 7)).close()
    flat.close()
    wide = nufft.PlanNUFFT(np.complex64, (12, 10), backend=nufft.ROCBackend(0))
    op = nufft.ToeplitzOperator(wide)
    with pytest.raises(ValueError, match="33 coils"):
        nufft.CoilMapEstimator(op, 33)
    nufft.CoilMapEstimator(op, 2).close()
    op.close()
    wide.close()
    real.close()
    K, n = 3, 120
    est = nufft.CoilMapEstimator(plan, K, box=3)
    plan.close()
    x = tuple(torch.ones((10, 12), dtype=torch.complex64, device="cuda") for _ in range(K))
    buf = torch.zeros(4 * n + 8, dtype=torch.complex64, device="cuda")
    view = lambda off: buf[off:off + n].view(10, 12)                                 # noqa: E731
    odd = (view(1),) + tuple(torch.empty_like(v) for v in x[1:])                    # 8 bytes off a 16-byte boundary
    part = (torch.empty_like(x[0]), view(2), view(4))                               # two outputs that overlap each other
    for out in (odd, part):
        with pytest.raises(ValueError):
            est.estimate(x, out=out)
    with pytest.raises(ValueError, match="overlaps an input"):                      # an output that is an input
        est.estimate(x, out=(x[1], torch.empty_like(x[0]), torch.empty_like(x[0])))
    with pytest.raises(ValueError, match="overlaps an input"):                      # ... and through the raw C call, in place
        chk(lib.nufft_coilmaps_estimate(est._handle, tab(x), tab(x), None, None, None, est._stream()))
    fresh = tuple(torch.empty_like(v) for v in x)
    lam = torch.empty(n, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="two outputs overlap"):                    # λ1 and λ2 are outputs too
        chk(lib.nufft_coilmaps_estimate(est._handle, tab(fresh), tab(x), None, C.c_void_p(lam.data_ptr()), C.c_void_p(lam.data_ptr()), est._stream()))
    bad = (C.c_double * (2 * K))(1.0, 0.0, float("nan"), 0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="finite"):
        chk(lib.nufft_coilmaps_estimate(est._handle, tab(fresh), tab(x), bad, None, None, est._stream()))
    assert lib.nufft_coilmaps_estimate(est._handle, None, tab(x), None, None, None, est._stream()) == nufft._lib.ERR_INVALID_ARG
    with pytest.raises(nufft.DimensionMismatch):
        est.estimate(x[:2])
    with pytest.raises(nufft.DimensionMismatch):
        est.estimate(x, phase=[1.0, 0.0])
    with pytest.raises(ValueError):
        est.estimate(tuple(v.to(torch.complex128) for v in x))
    with pytest.raises(ValueError):
        est.estimate(x, phase=3)
    with pytest.raises(ValueError):
        est.estimate(x, phase="svd")
    maps = est.estimate(x)                                                          # all ones: v = (1, 1, 1) / sqrt(3), coil 0 real
    torch.cuda.synchronize()
    assert np.abs(_host(maps) - 1 / np.sqrt(3)).max() <= 1e-6 and est.last_sweeps() >= 2
    est.close()
    est.close()
    with pytest.raises(ValueError, match="closed"):
        est.estimate(x)
    with pytest.raises(ValueError, match="closed"):
        est.info()
