"""Off-resonance correction by time segmentation on the GPU: the segment fit (histogram, interpolators, factors) against
numpy (field_reference.py), the segmented Toeplitz operator against the folded exact product, and the solvers on it.

Every case asserts the path it runs.  Bars (those of test_gpu_subspace.py for the same comparisons):
  * exact spectra, coil maps: rel-L2 <= 1e-12 (ComplexF64) / 1e-5 (ComplexF32), fused against dense likewise;
  * built from points: relative to the composed route (a coupled operator on an L-plan, the products around it in complex128 torch)
    measured in the same test against the same exact product: err <= 3 err_composed (ComplexF64), <= max(5 err_composed, 1e-4) (ComplexF32);
  * CG, fixed iteration count: within 10 × the parity bar at λ = 0.2 λmax; converged: true residual <= 2 rtol, iterations within 10 % + 1;
  * interpolators against numpy evaluated from the object's own read-back P, counts and centres: 10 × the largest measured difference
    relative to max |φ| (ComplexF64 1.571e-13 -> 1.6e-12; ComplexF32 4.744e-8 -> 4.8e-7), below the caps 1e-9 / 1e-5;
  * quality: the error at the occupied bin centres from the GPU's φ <= 1.5 × the reference's own (test_field_host.py prints it);
  * factors: 1e-14 / 1e-6 absolute, one rounding of a unit-modulus value.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import cg_reference as CG  # noqa: E402
import field_cases as FC  # noqa: E402
import field_reference as F  # noqa: E402
import subspace_reference as S  # noqa: E402
import toeplitz_reference as R  # noqa: E402

NP = FC.NP
INTERP_BAR = {"c128": 1.6e-12, "c64": 4.8e-7}
INTERP_CAP = {"c128": 1e-9, "c64": 1e-5}
NBINS_CASES = (1, 31, 33, 256, 1024)


def _dt(Z):
    return (np.float64, np.complex128, 1e-12, 1e-10) if Z == "c128" else (np.float32, np.complex64, 1e-5, 1e-4)


def _tz(Z):
    return torch.complex128 if Z == "c128" else torch.complex64


def _dev(a, Zc=None):
    return torch.from_numpy(np.ascontiguousarray(a if Zc is None else a.astype(Zc))).cuda()


def _plan(nufft, Z, Ns, path, fftshift=False, ntransforms=1, **opts):
    if path == "dense":
        opts["NUFFT_TOEPLITZ_FUSED"] = 0
    return nufft.PlanNUFFT(np.complex128 if Z == "c128" else np.complex64, Ns, backend=nufft.ROCBackend(0), options=opts, fftshift=fftshift,
                           ntransforms=ntransforms)


def _op(nufft, Z, Ns, path, L, fftshift=False, **opts):
    plan = _plan(nufft, Z, Ns, path, fftshift, **opts)
    op = nufft.ToeplitzOperator(plan, segments=L)
    assert op.path == path and op.segments == L and op.ntransforms == 1, (Ns, path, op.path)
    return plan, op


def _apply(op, u, Zc, **kw):
    out = op.apply(_dev(u, Zc), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _field(n, seed):
    rng = np.random.default_rng(seed)
    return 40.0 * rng.random(n) - 15.0 + 3.0 * np.sin(np.arange(n) * 0.37)


# ---- the fit object --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_histogram_and_gram(Z):
    from nufft_pkg import nufft
    T, Zc, _, _ = _dt(Z)
    L = 3
    tau = np.array([0.0, 0.4, 1.0])
    for n in (1, 63, 64, 65, 4099):
        om = _field(n, n).astype(T)
        mask = (np.random.default_rng(n + 1).random(n) < 0.6).astype(np.uint8)
        mask[0] = 1
        for nbins in NBINS_CASES:
            fs = nufft.FieldSegments(_tz(Z), L, nbins=nbins)
            for m in (None, mask, "constant"):
                w = np.full(n, T(1.75)) if isinstance(m, str) else om
                mk = None if isinstance(m, str) else m
                fs.fit(_dev(w), tau=tau, mask=None if mk is None else _dev(mk))
                counts, centres = fs.histogram()
                rc, rcen = F.histogram(w, nbins, mk)
                assert counts.dtype == np.uint32 and np.array_equal(counts, rc), (n, nbins, m)
                assert np.allclose(centres, rcen, rtol=1e-15, atol=1e-15 * np.abs(rcen).max())
                assert fs.info().bins_used == rc.size and np.array_equal(fs.tau, tau)
                G, Gr = fs.gram(), F.gram(rc, rcen, tau)
                assert np.linalg.norm(G - Gr) <= 1e-13 * np.linalg.norm(Gr), (n, nbins, m)
                if n > 1 and not isinstance(m, str):
                    P, Pr = fs.solver_matrix(), F.solver_matrix(G, fs.ridge)
                    cond = np.linalg.cond(F.ridged(G, fs.ridge))
                    assert np.linalg.norm(P - Pr) <= 1e-14 * cond * np.linalg.norm(Pr), (n, nbins, cond)
            fs.close()
    # a bool mask of another shape
    fs = nufft.FieldSegments(_tz(Z), L, nbins=33)
    om2 = _field(35 * 12, 5).astype(T).reshape(12, 35)
    mk2 = om2 > 0
    counts, _ = fs.fit(_dev(om2), tau=tau, mask=torch.from_numpy(mk2).cuda()).histogram()
    assert np.array_equal(counts, F.histogram(om2, 33, mk2)[0])


def _interp_against_own_readback(nufft, Z, L, nbins, Np, seed):
    """What is compared is the kernel's arithmetic, so the system is kept well conditioned: ω spans 2π L, so that the L segment phases of
    the bins go once round the circle (cond of the ridged normal matrix <= 2.2 for every case here), and a one-bin histogram, which is
    one equation for L unknowns, gets a ridge of 1 (cond = L + 1).  P r loses cond · ε in any order of evaluation."""
    T, Zc, _, _ = _dt(Z)
    rng = np.random.default_rng(seed)
    om = (2 * np.pi * L * rng.random(777) - 3.0).astype(T)
    times = np.sort(rng.random(Np) * 1.5 - 0.2).astype(T)
    tau = F.uniform_tau(L, 0.0, 1.0)
    fs = nufft.FieldSegments(_tz(Z), L, nbins=nbins, ridge=1.0 if nbins == 1 else 1e-3).fit(_dev(om), tau=tau)
    phi = fs.interpolators(_dev(times))
    torch.cuda.synchronize()
    assert tuple(phi.shape) == (L, Np) and phi.dtype == _tz(Z) and phi.is_contiguous()
    counts, centres = fs.histogram()
    ref = F.interpolators(fs.solver_matrix(), counts, centres, tau, times)
    fs.close()
    return float(np.max(np.abs(phi.cpu().numpy() - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_interpolators_against_own_readback(Z):
    from nufft_pkg import nufft
    cases = [(L, nbins, Np) for L in (1, 2, 3, 8, 16) for nbins in NBINS_CASES for Np in (1, 63, 64, 65)]
    cases += [(1, 1, 1000), (2, 33, 1000), (3, 256, 1000), (8, 256, 1000), (16, 31, 1000), (16, 1024, 1000), (8, 1024, 1000)]
    worst = 0.0
    for i, (L, nbins, Np) in enumerate(cases):
        err = _interp_against_own_readback(nufft, Z, L, nbins, Np, i)
        worst = max(worst, err)
        assert err <= INTERP_BAR[Z] <= INTERP_CAP[Z], (L, nbins, Np, err)
    print(f"interpolators {Z}: largest difference / max |phi| over {len(cases)} cases {worst:.3e} (bar {INTERP_BAR[Z]:g}, cap {INTERP_CAP[Z]:g})")


@pytest.mark.parametrize("Z", ["c128", "c64"])
@pytest.mark.parametrize("L", FC.QUALITY_SEGMENTS)
def test_quality(Z, L):
    from nufft_pkg import nufft
    T, Zc, _, _ = _dt(Z)
    omega, times = FC.quality_case()
    omega, times = omega.astype(T), times.astype(T)
    fs = nufft.FieldSegments(_tz(Z), L, nbins=FC.NBINS, ridge=FC.RIDGE).fit(_dev(omega), t_range=(0.0, 1.0))
    assert np.array_equal(fs.tau, F.uniform_tau(L, 0.0, 1.0))
    phi = fs.interpolators(_dev(times)).cpu().numpy()
    err, ref = FC.bin_error(phi, omega, fs.tau, times, dtype=T), FC.quality_reference(L, T)
    print(f"quality {Z} L={L}: error from the GPU's interpolators {err:.3e}, the reference's own {ref:.3e}")
    assert err <= 1.5 * ref
    # times= gives the same τ as their range
    fs2 = nufft.FieldSegments(_tz(Z), L).fit(_dev(omega), times=_dev(times))
    assert np.array_equal(fs2.tau, F.uniform_tau(L, float(times.min()), float(times.max())))


@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_factors_repeats_and_graph(Z):
    from nufft_pkg import nufft
    T, Zc, _, _ = _dt(Z)
    L, shape, Np = 5, (13, 21), 1000
    omega = FC.smooth_field(shape, 6 * np.pi).astype(T) - T(4.0)
    times = np.linspace(0, 1, Np).astype(T)
    od, td = _dev(omega), _dev(times)
    fs = nufft.FieldSegments(_tz(Z), L).fit(od, times=td)
    B = fs.factors(od)
    torch.cuda.synchronize()
    assert len(B) == L and all(b.shape == od.shape and b.data_ptr() % 16 == 0 for b in B)
    ref = F.factors(omega, fs.tau)
    err = max(float(np.max(np.abs(b.cpu().numpy() - r))) for b, r in zip(B, ref))
    print(f"factors {Z}: max difference {err:.3e}")
    assert err <= (1e-14 if Z == "c128" else 1e-6)
    phi = fs.interpolators(td)
    B2, phi2 = fs.factors(od), fs.interpolators(td)
    assert all(torch.equal(a, b) for a, b in zip(B, B2)) and torch.equal(phi, phi2)
    Bg, phig = tuple(torch.zeros_like(b) for b in B), torch.zeros_like(phi)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fs.factors(od, out=Bg)
        fs.interpolators(td, out=phig)
        with pytest.raises(ValueError):                  # set-up and read-backs synchronise
            fs.fit(od, t_range=(0.0, 1.0))
        for read in (fs.histogram, fs.gram, fs.solver_matrix, lambda: fs.tau):
            with pytest.raises(ValueError):
                read()
    for _ in range(2):
        phig.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(B, Bg)) and torch.equal(phi, phig)
    del graph
    assert fs.info().bins_used == fs.nbins                # the refused fit left the object as it was


# ---- the segmented operator ------------------------------------------------------------------------------------------------------

# (Z, N, fftshift, paths, L)
EXACT_CASES = [(Z, Ns, sh if Z == "c128" else not sh, paths, L) for Z in ("c128", "c64") for Ns, sh, paths, L in (
    ((48, 40), True, ("fused", "dense"), 3), ((32, 32), False, ("fused",), 8), ((32, 32), True, ("fused",), 16),
    ((32, 32, 32), False, ("fused", "dense"), 2), ((15, 9), True, ("dense",), 5), ((64,), False, ("dense",), 2))]


@pytest.mark.parametrize("Z,Ns,fftshift,paths,L", EXACT_CASES)
def test_exact_spectra(Z, Ns, fftshift, paths, L):
    from nufft_pkg import nufft
    T, Zc, bar, _ = _dt(Z)
    p = FC.problem(Ns, L)
    u, B = p.u.astype(Zc), p.B.astype(Zc)
    ref = F.folded_gram(Ns, p.xs, p.w, p.phi, B, u, fftshift=fftshift)           # of the rounded inputs
    got = {}
    for path in paths:
        plan, op = _op(nufft, Z, Ns, path, L, fftshift)
        spec = _dev(np.stack(p.spectra), Zc)
        op.set_spectra(spec if path == paths[0] else [spec[i] for i in range(spec.shape[0])])
        plan.close()
        assert op.info().has_spectrum == 0                                       # the factors are still missing
        op.set_factors(_dev(B))
        assert op.info().has_spectrum == 1 and not op.coupled and nufft.lib.nufft_toeplitz_num_segments(op._handle) == L
        got[path] = _apply(op, u, Zc)
        err = R.rel(got[path], ref)
        print(f"exact spectra {Z} N={Ns} shift={fftshift} {path} L={L}: rel-L2 {err:.3e} (bar {bar:g})")
        assert err <= bar
        for a, b in ((0, 0), (0, L - 1), (L - 1, L - 1)):
            k, kref = op.multiplier(a, b), p.multipliers[S.pair_index(a, b, L)]
            assert k.is_complex() == (a != b) and R.rel(k.cpu().numpy(), kref.real if a == b else kref) <= bar
        assert np.array_equal(_apply(op, u, Zc), got[path])                      # fixed order, no atomics
        op.close()
    if len(paths) == 2:
        err = R.rel(got["fused"], got["dense"])
        print(f"  fused vs dense: {err:.3e}")
        assert err <= bar


@pytest.mark.parametrize("Z,Ns,path,L,clustered", [(Z, Ns, path, L, cl) for Z in ("c128", "c64")
                                                   for Ns, path, L, cl in (((48, 40), "fused", 3, False), ((48, 40), "dense", 3, True),
                                                                           ((32, 32, 32), "fused", 2, True), ((64,), "dense", 2, False))])
def test_built_from_points(Z, Ns, path, L, clustered):
    from nufft_pkg import nufft
    T, Zc, _, _ = _dt(Z)
    p = FC.problem(Ns, L, clustered)
    xs, w, phi, u, B = [x.astype(T) for x in p.xs], p.w.astype(T), p.phi.astype(Zc), p.u.astype(Zc), p.B.astype(Zc)
    ref = F.folded_gram(Ns, [x.astype(np.float64) for x in xs], w.astype(np.float64), phi, B, u)
    pd, wd, phid, Bd = tuple(_dev(x) for x in xs), _dev(w), _dev(phi), _dev(B)
    # the composed route: a coupled operator on an L-plan, the products in complex128 around it
    cplan = _plan(nufft, Z, Ns, path, ntransforms=L)
    cop = nufft.ToeplitzOperator(cplan).set_points(pd, wd, basis=phid)
    assert cop.coupled and cop.path == path
    B128, u128 = Bd.to(torch.complex128), _dev(u).to(torch.complex128)
    ins = tuple((B128[b] * u128).to(_tz(Z)).contiguous() for b in range(L))
    g = cop.apply(ins if L > 1 else ins[0])
    g = g if L > 1 else (g,)
    comp = sum(B128[a].conj() * g[a].to(torch.complex128) for a in range(L)).cpu().numpy()
    _, op = _op(nufft, Z, Ns, path, L)
    op.set_factors(Bd).set_points(pd, wd, basis=phid)
    assert op.info().has_spectrum == 1
    got = _apply(op, u, Zc)
    err_t, err_c = R.rel(got, ref), R.rel(comp, ref)
    print(f"from points {Z} N={Ns} {path} L={L} clustered={clustered}: segmented {err_t:.3e}, composed {err_c:.3e}, ratio {err_t / err_c:.2f}")
    assert err_t <= 3 * err_c if Z == "c128" else err_t <= max(5 * err_c, 1e-4)


@pytest.mark.parametrize("Z,Ns,path", [(Z, Ns, path) for Z in ("c128", "c64") for Ns, path in (((48, 40), "fused"), ((48, 40), "dense"),
                                                                                              ((32, 32, 32), "fused"))])
def test_with_coil_maps(Z, Ns, path):
    from nufft_pkg import nufft
    T, Zc, bar, _ = _dt(Z)
    L = 3 if len(Ns) == 2 else 2
    p = FC.problem(Ns, L)
    u, B, maps = p.u.astype(Zc), p.B.astype(Zc), p.maps.astype(Zc)
    ref = F.folded_gram(Ns, p.xs, p.w, p.phi, B, u, maps=maps)
    spec, Bd, md, ud = _dev(np.stack(p.spectra), Zc), _dev(B), _dev(maps), _dev(u)
    _, op = _op(nufft, Z, Ns, path, L)
    op.set_spectra(spec)
    base = op.info().workspace_bytes
    op.set_factors(Bd)
    assert op.info().workspace_bytes == base
    plain = op.apply(ud).clone()
    op.set_maps(md)
    scratch = 2 * ((max(int(np.prod(Ns)) * 2 * np.dtype(T).itemsize, 16) + 255) // 256 * 256)
    assert op.ncoils == 3 and op.info().workspace_bytes == base + scratch
    first = op.apply(ud).clone()
    err = R.rel(first.cpu().numpy(), ref)
    print(f"coil maps {Z} N={Ns} {path} L={L}: {err:.3e} (bar {bar:g})")
    assert err <= bar and torch.equal(first, op.apply(ud))
    # factors then maps, maps then factors: the same bits; a clear frees the scratch
    op.clear_factors()
    assert op.info().workspace_bytes == base and op.info().has_spectrum == 0
    with pytest.raises(ValueError):
        op.apply(ud)
    op.set_factors(Bd)
    assert op.info().workspace_bytes == base + scratch and torch.equal(first, op.apply(ud))
    _, op2 = _op(nufft, Z, Ns, path, L, NUFFT_TOEPLITZ_MAPS_INPASS=0)          # the option plays no part here
    op2.set_maps(md).set_factors(Bd).set_spectra(spec)
    assert torch.equal(first, op2.apply(ud))
    op.clear_maps()
    assert op.info().workspace_bytes == base and op.ncoils == 0 and torch.equal(plain, op.apply(ud))
    with pytest.raises(ValueError):
        op.apply(ud, out=ud)


@pytest.mark.parametrize("Z,Ns,path", [("c128", (48, 40), "fused"), ("c64", (48, 40), "dense"), ("c64", (32, 32, 32), "fused")])
def test_one_segment_with_unit_factor_is_the_plain_operator(Z, Ns, path):
    from nufft_pkg import nufft
    T, Zc, bar, _ = _dt(Z)
    p = FC.problem(Ns, 1)
    pd, wd = tuple(_dev(x, T) for x in p.xs), _dev(p.w, T)
    plain = nufft.ToeplitzOperator(_plan(nufft, Z, Ns, path)).set_points(pd, wd)
    _, op = _op(nufft, Z, Ns, path, 1)
    op.set_points(pd, wd, basis=torch.ones(NP, dtype=op.Z, device="cuda")).set_factors(torch.ones((1,) + op.shape, dtype=op.Z, device="cuda"))
    err = R.rel(_apply(op, p.u, Zc), _apply(plain, p.u, Zc))
    print(f"L = 1, unit factor and basis {Z} N={Ns} {path}: {err:.3e} (bar {bar:g})")
    assert err <= bar


# ---- the solvers -----------------------------------------------------------------------------------------------------------------

class System:
    """(48, 40), L = 3, the multipliers of the exact spectra; the float64 folded apply, λmax by power iteration, λ = 0.2 λmax."""

    def __init__(self, with_maps):
        self.Ns, self.L = (48, 40), 3
        self.p = FC.problem(self.Ns, self.L)
        self.maps = self.p.maps if with_maps else None
        rng = np.random.default_rng(5)
        self.b = rng.standard_normal(self.p.shape) + 1j * rng.standard_normal(self.p.shape)
        v = self.b.copy()
        for _ in range(20):
            g = self.apply(v, np.complex128)
            self.lmax = float(np.linalg.norm(g) / np.linalg.norm(v))
            v = g / np.linalg.norm(g)
        self.lam = 0.2 * self.lmax

    def apply(self, v, Zc):
        maps = None if self.maps is None else self.maps.astype(Zc)
        return F.folded_apply(self.Ns, self.p.multipliers, self.p.B.astype(Zc), v, maps)

    def operator(self, nufft, Z, path):
        _, Zc, _, _ = _dt(Z)
        plan, op = _op(nufft, Z, self.Ns, path, self.L)
        op.set_spectra(_dev(np.stack(self.p.spectra), Zc)).set_factors(_dev(self.p.B, Zc))
        if self.maps is not None:
            op.set_maps(_dev(self.maps, Zc))
        plan.close()
        return op


_SYSTEMS = {}


def _system(with_maps):
    if with_maps not in _SYSTEMS:
        _SYSTEMS[with_maps] = System(with_maps)
    return _SYSTEMS[with_maps]


def _solve(sol, b, **kw):
    x = sol.solve(_dev(b), **kw)
    torch.cuda.synchronize()
    return x.cpu().numpy(), sol.iterations, sol.status, sol.history().numpy()


CG_CASES = [(Z, path, m) for Z in ("c128", "c64") for path in ("fused", "dense") for m in (False, True)]


@pytest.mark.parametrize("Z,path,with_maps", CG_CASES)
def test_cg_fixed_iteration_count(Z, path, with_maps):
    from nufft_pkg import nufft
    T, Zc, bar, _ = _dt(Z)
    s = _system(with_maps)
    op = s.operator(nufft, Z, path)
    b = s.b.astype(Zc)
    lmax = op.max_eigenvalue(iters=20, v0=_dev(b))
    assert len(lmax) == 1 and abs(lmax[0] - s.lmax) <= 0.05 * s.lmax
    sol = nufft.ToeplitzCG(op, maxiter=5, rtol=0.0, lam=s.lam)
    x, iters, status, hist = _solve(sol, b)
    assert iters == (5,) and status == ("max_iter",) and hist.shape == (6, 1)
    ref = CG.cg(lambda v: s.apply(v, Zc), b, lam=s.lam, rtol=0.0, max_iter=5, dtype=Zc)
    ex, eh = R.rel(x, ref["x"]), R.rel(hist[:, 0], ref["history"])
    print(f"CG, 5 iterations {Z} {path} maps={with_maps}: x {ex:.3e}, history {eh:.3e} (bar {10 * bar:g})")
    assert ex <= 10 * bar and eh <= 10 * bar
    sol.close()


@pytest.mark.parametrize("Z,path,with_maps", [("c128", "fused", True), ("c64", "fused", False), ("c128", "dense", False), ("c64", "dense", True)])
def test_cg_converged_and_the_two_modes(Z, path, with_maps):
    from nufft_pkg import nufft
    T, Zc, _, rtol = _dt(Z)
    s = _system(with_maps)
    op = s.operator(nufft, Z, path)
    b = s.b.astype(Zc)
    sol = nufft.ToeplitzCG(op, maxiter=100, rtol=rtol, lam=s.lam, check_every=0)
    x, iters, status, hist = _solve(sol, b)
    ref = CG.cg(lambda v: s.apply(v, Zc), b, lam=s.lam, rtol=rtol, max_iter=100, dtype=Zc)
    g = s.apply(x.astype(np.complex128), np.complex128 if Z == "c128" else Zc)
    tr = float(np.linalg.norm(b.astype(np.complex128) - (g + s.lam * x)) / np.linalg.norm(b))
    print(f"CG converged {Z} {path} maps={with_maps}: {iters} iterations (reference {ref['iterations']}), true residual / rtol {tr / rtol:.3f}")
    assert status == ("converged",) and tr <= 2 * rtol and abs(iters[0] - ref["iterations"]) <= 0.1 * ref["iterations"] + 1
    chk = nufft.ToeplitzCG(op, maxiter=100, rtol=rtol, lam=s.lam, check_every=3)
    xc, ic, sc, hc = _solve(chk, b)
    assert (ic, sc) == (iters, status) and np.array_equal(hc, hist, equal_nan=True) and np.array_equal(x, xc)
    one = op.solve(_dev(b), maxiter=100, rtol=rtol, lam=s.lam)
    assert np.array_equal(one.cpu().numpy(), x)
    sol.close()
    chk.close()


@pytest.mark.parametrize("Z,path", [("c128", "fused"), ("c64", "dense")])
def test_other_solvers_repeat_and_cg_replays(Z, path):
    from nufft_pkg import nufft
    T, Zc, _, _ = _dt(Z)
    s = _system(True)
    op = s.operator(nufft, Z, path)
    b, bd = s.b.astype(Zc), _dev(s.b, Zc)
    step = 1.0 / (1.05 * s.lmax)          # the right-hand side has entries of order one: weights of 0.05 leave most coefficients alive
    for sol in (nufft.ToeplitzFISTA(op, wavelet="haar", levels=2, l1=0.05, step=step, maxiter=10, tol=0.0),
                nufft.ToeplitzFISTA(op, prior="llr", block=8, nuc=0.05, step=step, maxiter=10, tol=0.0, seed=1),
                nufft.ToeplitzTV(op, tv=0.05, maxiter=10, tol=0.0)):
        x1 = sol.solve(bd).clone()
        x2 = sol.solve(bd)
        torch.cuda.synchronize()
        assert sol.iterations == (10,) and torch.isfinite(x1.abs()).all() and torch.equal(x1, x2), type(sol).__name__
        sol.close()
    cg = nufft.ToeplitzCG(op, maxiter=10, rtol=0.0, lam=s.lam)
    x, iters, status, hist = _solve(cg, b)
    out = torch.zeros_like(bd)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cg.solve(bd, out=out)
    for _ in range(2):
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert cg.iterations == iters and np.array_equal(cg.history().numpy(), hist) and np.array_equal(out.cpu().numpy(), x)
    del graph
    cg.close()


@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_recovery(Z):
    """Data of the EXACT off-resonance model; CG to rtol 1e-8 at λ = 1e-3 λmax on the segmented operator (L = 8, everything from the
    library: fit, interpolators, factors, the right-hand side by the README's recipe) and on the uncorrected plain operator."""
    from nufft_pkg import nufft
    T, Zc, _, _ = _dt(Z)
    c = FC.recovery_case()
    Ns, L, Np = c["Ns"], c["L"], c["Np"]
    pd, td, od = tuple(_dev(x, T) for x in c["xs"]), _dev(c["times"], T), _dev(c["omega"], T)
    yd = _dev(c["data"], Zc)
    plan = _plan(nufft, Z, Ns, "fused")
    op, fs = nufft.field_corrected_operator(plan, pd, None, od, td, segments=L, nbins=FC.NBINS, ridge=FC.RIDGE)
    assert op.segments == L and op.path == "fused" and op.info().has_spectrum == 1
    phi, B = fs.interpolators(td), fs.factors(od)
    planL = _plan(nufft, Z, Ns, "fused", ntransforms=L)
    nufft.set_points(planL, pd)
    parts = tuple(torch.empty(plan.shape, dtype=plan.Z, device="cuda") for _ in range(L))
    nufft.exec_type1(parts, planL, tuple((phi[l].conj() * yd).contiguous() for l in range(L)))
    rhs = nufft.coil_combine(B, parts)
    x = op.solve(rhs, maxiter=2000, rtol=1e-8, lam=1e-3 * c["lmax_seg"])          # the reference's λ: the same system
    plain = nufft.ToeplitzOperator(plan).set_points(pd)
    nufft.set_points(plan, pd)
    rhs0 = torch.empty(plan.shape, dtype=plan.Z, device="cuda")
    nufft.exec_type1(rhs0, plan, yd)
    x0 = plain.solve(rhs0, maxiter=2000, rtol=1e-8, lam=1e-3 * c["lmax_plain"])
    torch.cuda.synchronize()
    rel = lambda a: float(np.linalg.norm(a.cpu().numpy() - c["u"]) / np.linalg.norm(c["u"]))
    err, err0 = rel(x), rel(x0)
    print(f"recovery {Z}: corrected {err:.3e} (reference {c['err_ref']:.3e}), uncorrected {err0:.3e} (reference {c['err_plain']:.3e})")
    assert abs(err - c["err_ref"]) <= 0.1 * c["err_ref"] and err < 0.5 * err0


# ---- refusals and lifetime -------------------------------------------------------------------------------------------------------

def test_refusals_and_lifetime():
    from nufft_pkg import nufft
    L_, lib = nufft._lib, nufft.lib
    Ns, L = (48, 40), 3
    p = FC.problem(Ns, L)
    pd, wd, phid, Bd, ud = tuple(_dev(x) for x in p.xs), _dev(p.w), _dev(p.phi), _dev(p.B), _dev(p.u)
    spec = _dev(np.stack(p.spectra))
    # an ordinary coupled operator before ...
    cplan = _plan(nufft, "c128", Ns, "fused", ntransforms=L)
    cop = nufft.ToeplitzOperator(cplan).set_spectra(spec)
    cin = tuple(_dev(p.B[l] * p.u) for l in range(L))
    before = [o.clone() for o in cop.apply(cin)]
    # creation
    for bad in (0, 17):
        with pytest.raises(ValueError):
            nufft.ToeplitzOperator(_plan(nufft, "c128", Ns, "fused"), segments=bad)
    with pytest.raises(ValueError, match="ntransforms = 1"):
        nufft.ToeplitzOperator(cplan, segments=L)
    with pytest.raises(ValueError, match="complex plan"):
        nufft.ToeplitzOperator(nufft.PlanNUFFT(np.float64, Ns, backend=nufft.ROCBackend(0)), segments=L)
    with pytest.raises(ValueError, match="NUFFT_TOEPLITZ_FUSED=0"):
        nufft.ToeplitzOperator(_plan(nufft, "c128", (512, 32), "fused"), segments=16)
    plan, op = _op(nufft, "c128", Ns, "fused", L)
    # builds and read-outs a segmented operator has no use for
    with pytest.raises(ValueError, match="segmented"):
        op.set_points(pd, wd)
    with pytest.raises(ValueError, match="segmented"):
        op.set_spectrum(spec[0])
    tab = nufft.plan._ptr_table
    assert lib.nufft_toeplitz_set_spectra_frames(op._handle, tab((spec[0],)), None) == L_.ERR_UNSUPPORTED
    assert lib.nufft_toeplitz_set_points_frames(op._handle, None, (C.c_int64 * 1)(NP), tab(pd), None, None) == L_.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        op.multiplier()
    with pytest.raises(nufft.DimensionMismatch):
        op.set_points(pd, wd, basis=phid[:2])
    with pytest.raises(nufft.DimensionMismatch):
        op.set_spectra(spec[:3])
    # apply needs a build and the factors, in either order
    with pytest.raises(ValueError):
        op.apply(ud)
    op.set_factors(Bd)
    assert op.info().has_spectrum == 0 and lib.nufft_toeplitz_apply(op._handle, tab((torch.empty_like(ud),)), tab((ud,)), None) == L_.ERR_NO_POINTS
    with pytest.raises(ValueError):
        op.multiplier(0, 1)                                                  # no build yet
    op.set_spectra(spec)
    assert op.info().has_spectrum == 1
    want = op.apply(ud).clone()
    with pytest.raises(ValueError):
        op.apply(ud, out=ud)
    assert lib.nufft_toeplitz_apply(op._handle, tab((ud,)), tab((ud,)), None) == L_.ERR_INVALID_ARG
    # factors: count, shape, alignment
    with pytest.raises(nufft.DimensionMismatch):
        op.set_factors(Bd[:2])
    with pytest.raises(nufft.DimensionMismatch):
        op.set_factors(Bd[:, :-1].contiguous())
    with pytest.raises(ValueError):
        op.set_factors(Bd.to(torch.complex64))
    flat = torch.zeros(L * ud.numel() + 1, dtype=torch.complex64, device="cuda")
    odd = tuple(flat[1 + l * ud.numel():1 + (l + 1) * ud.numel()] for l in range(L))          # 8 bytes off a 16-byte boundary
    _, op32 = _op(nufft, "c64", Ns, "fused", L)
    assert odd[0].data_ptr() % 16 == 8 and lib.nufft_toeplitz_set_factors(op32._handle, tab(odd), None) == L_.ERR_INVALID_ARG
    assert torch.equal(op.apply(ud), want)                                   # the refused calls left the factors in force
    # the preconditioner
    with pytest.raises(ValueError, match="segmented"):
        nufft.ToeplitzPreconditioner(op, lam=1.0)
    with pytest.raises(ValueError, match="segmented"):
        nufft.ToeplitzPreconditioner(op, lam=1.0, block=True)
    # workspace: two scratch arrays exactly while maps and factors are both set
    pad = lambda b: (max(b, 16) + 255) // 256 * 256
    base = op.info().workspace_bytes
    op.set_maps(_dev(p.maps))
    assert op.info().workspace_bytes == base + 2 * pad(int(np.prod(Ns)) * 16)
    graph = torch.cuda.CUDAGraph()
    out = torch.empty_like(ud)
    op.apply(ud, out=out)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        op.apply(ud, out=out)
    eager = out.clone()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    del graph
    op.clear_maps()
    assert op.info().workspace_bytes == base and torch.equal(op.apply(ud), want)
    # the fit object
    fs = nufft.FieldSegments(op, L)
    assert fs.Z == op.Z and fs.device == op.device
    om = _dev(FC.smooth_field(Ns[::-1], 3.0))
    with pytest.raises(ValueError):
        fs.interpolators(_dev(np.linspace(0, 1, 10)))                        # no fit yet
    bad = om.clone()
    bad[3, 4] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        fs.fit(bad, t_range=(0, 1))
    fs.fit(bad, t_range=(0, 1), mask=torch.isfinite(bad))                    # ... unless the mask leaves it out
    with pytest.raises(ValueError, match="empty"):
        fs.fit(om, t_range=(0, 1), mask=torch.zeros_like(om, dtype=torch.bool))
    for tau in ([0.0, 0.5, 0.5], [0.0, 1.0, 0.5], [0.0, np.nan, 1.0]):
        with pytest.raises(ValueError):
            fs.fit(om, tau=tau)
    with pytest.raises(ValueError, match="ridge"):
        fs.fit(om, t_range=(0, 1), ridge=-1e-3)
    with pytest.raises(ValueError, match="ridge"):                            # a constant map cannot tell three segments apart
        fs.fit(torch.zeros_like(om), t_range=(0, 1), ridge=0.0)
    with pytest.raises(ValueError):
        fs.fit(om.to(torch.float32), t_range=(0, 1))
    for args in ((torch.complex64, 0), (torch.complex64, 17)):
        with pytest.raises(ValueError):
            nufft.FieldSegments(*args)
    with pytest.raises(ValueError):
        nufft.FieldSegments(torch.complex64, 4, nbins=1025)
    # ... and the ordinary coupled operator after
    after = cop.apply(cin)
    cop2 = nufft.ToeplitzOperator(cplan).set_spectra(spec)
    again = cop2.apply(cin)
    assert all(torch.equal(a, b) and torch.equal(a, c2) for a, b, c2 in zip(before, after, again))
    assert cop.coupled and lib.nufft_toeplitz_num_segments(cop._handle) == 0
