"""Coupled components of the Toeplitz normal operator on the GPU: the K × K block operator of a subspace model,
(G_Φ u)_a = Σ_b A^H diag(w conj(φ_a) φ_b) A u_b, against direct sums on the CPU (subspace_reference.py), and its joint CG.

Every case asserts the apply path it runs.  Bars (those of test_gpu_toeplitz.py / test_gpu_cg.py for the same comparisons):
  * exact spectra: rel-L2 <= 1e-12 (ComplexF64) / 1e-5 (ComplexF32) per component, fused against dense likewise;
  * built from points: relative to the composed route (exec_type2, the mix at the samples in torch, exec_type1) measured in the same
    test against the same exact product: err <= 3 err_composed (ComplexF64), <= max(5 err_composed, 1e-4) (ComplexF32);
  * CG, fixed iteration count: x and history within 10 × the parity bar, on systems with cond(G_Φ + λ) <= 7: λ = 0.2 λmax with λmax
    from a power iteration (from below, within a few per cent: the factor 1.05), so cond <= (1.05 λmax + λ) / λ = 6.25 whatever φ is;
    converged: true residual <= 2 rtol, iterations within 10 % + 1 of the joint numpy CG.
References are computed once per (N, K) and shared.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import subspace_reference as S  # noqa: E402
import toeplitz_reference as R  # noqa: E402

NP = 2000


def _dt(Z):
    return (np.float64, np.complex128, 1e-12, 1e-10) if Z == "c128" else (np.float32, np.complex64, 1e-5, 1e-4)


def _dev(a, Zc=None):
    return torch.from_numpy(np.ascontiguousarray(a if Zc is None else a.astype(Zc))).cuda()


def _op(nufft, Z, Ns, path, K, fftshift=False, **opts):
    if path == "dense":
        opts["NUFFT_TOEPLITZ_FUSED"] = 0
    plan = nufft.PlanNUFFT(np.complex128 if Z == "c128" else np.complex64, Ns, backend=nufft.ROCBackend(0), options=opts, fftshift=fftshift,
                           ntransforms=K)
    op = nufft.ToeplitzOperator(plan)
    assert op.path == path, (Ns, path, op.path)
    return plan, op


def _apply(op, us, Zc, **kw):
    ud = tuple(_dev(u, Zc) for u in us)
    out = op.apply(ud if len(us) > 1 else ud[0], **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in (out if len(us) > 1 else (out,))]


class Problem:
    """Points, weights, basis, inputs; the exact spectra and (per fftshift) the exact product, computed on first use."""

    def __init__(self, Ns, K, seed=0, clustered=False, zero_row=False, coupling="random"):
        rng = np.random.default_rng(seed)
        self.Ns, self.K = Ns, K
        if clustered:
            self.xs = [np.mod(np.pi + 0.3 * rng.standard_normal(NP), 2 * np.pi) for _ in Ns]
        else:
            self.xs = [rng.random(NP) * 2 * np.pi for _ in Ns]
        self.w = rng.random(NP) + 0.1
        if coupling == "fourier":              # a temporal Fourier basis mixed by I + 0.3 shift: every cross block is there
            t = rng.random(NP)
            F = np.exp(2j * np.pi * np.outer(np.arange(K), t)) / np.sqrt(K)
            self.phi = F + 0.3 * np.roll(F, 1, axis=0)
        else:
            self.phi = (rng.standard_normal((K, NP)) + 1j * rng.standard_normal((K, NP))) / np.sqrt(2)
        if zero_row:
            self.phi[K - 1] = 0.0
        self.us = [rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1]) for _ in range(K)]
        self._spectra, self._gram, self._mult = None, {}, None

    @property
    def spectra(self):
        if self._spectra is None:
            self._spectra = S.exact_spectra(self.Ns, self.xs, self.w, self.phi)
        return self._spectra

    @property
    def multipliers(self):
        if self._mult is None:
            self._mult = S.multipliers(self.Ns, self.spectra)
        return self._mult

    def gram(self, fftshift):
        if fftshift not in self._gram:
            self._gram[fftshift] = S.exact_block_gram(self.Ns, self.xs, self.w, self.phi, self.us, fftshift)
        return self._gram[fftshift]


_PROBLEMS = {}


def _problem(Ns, K, **kw):
    key = (Ns, K, tuple(sorted(kw.items())))
    if key not in _PROBLEMS:
        _PROBLEMS[key] = Problem(Ns, K, seed=3 * sum(Ns) + K, **kw)
    return _PROBLEMS[key]


# (Z, N, fftshift, paths, K).  K = 1, 2, 3 (odd, six pairs), 5 (crosses the <= 4 tier); the largest K of every tier of the fused kernel
# (2, 4, 8, 16) and K = 16 on the dense path; 1-D even and odd, unequal table sizes 96 / 80, 3-D cubic and not, a size outside the table
EXACT_CASES = [
    ("c128", (64,), False, ("dense",), 2),
    ("c64", (33,), True, ("dense",), 3),
    ("c128", (48, 40), False, ("fused", "dense"), 3),
    ("c64", (48, 40), True, ("fused", "dense"), 5),
    ("c128", (48, 40), True, ("fused",), 5),
    ("c64", (48, 40), False, ("fused",), 4),
    ("c128", (32, 32), False, ("fused", "dense"), 8),
    ("c64", (32, 32), True, ("fused", "dense"), 16),
    ("c128", (32, 32), True, ("fused",), 16),
    ("c128", (64,), True, ("dense",), 16),
    ("c128", (32, 32, 32), True, ("fused", "dense"), 2),
    ("c64", (32, 32, 32), False, ("fused", "dense"), 2),
    ("c128", (48, 32, 40), False, ("fused", "dense"), 1),
    ("c64", (48, 32, 40), True, ("fused",), 1),
    ("c128", (15, 9), True, ("dense",), 5),
    ("c64", (15, 9), False, ("dense",), 3),
]


@pytest.mark.parametrize("Z,Ns,fftshift,paths,K", EXACT_CASES)
def test_exact_spectra(Z, Ns, fftshift, paths, K):
    from nufft_pkg import nufft
    T, Zc, bar, _ = _dt(Z)
    p = _problem(Ns, K)
    refs = p.gram(fftshift)
    us = [u.astype(Zc) for u in p.us]
    if Z == "c64":
        refs = S.exact_block_gram(Ns, p.xs, p.w, p.phi, [u.astype(np.complex128) for u in us], fftshift)     # of the rounded inputs
    got = {}
    for path in paths:
        plan, op = _op(nufft, Z, Ns, path, K, fftshift)
        assert op.coupled is False
        spec = _dev(np.stack(p.spectra), Zc)
        op.set_spectra(spec if path == paths[0] else [spec[i] for i in range(spec.shape[0])])      # both accepted forms
        plan.close()
        assert op.coupled is True and nufft.lib.nufft_toeplitz_num_coupled(op._handle) == K and op.path == path
        got[path] = _apply(op, us, Zc)
        for a in range(K):
            err = R.rel(got[path][a], refs[a])
            print(f"exact spectra {Z} N={Ns} shift={fftshift} {path} K={K} a={a}: rel-L2 {err:.3e} (bar {bar:g})")
            assert err <= bar
        for a, b in ((0, 0), (0, K - 1), (K - 1, K - 1)):
            k = op.multiplier(a, b)
            assert tuple(k.shape) == tuple(2 * n for n in reversed(Ns)) and k.is_complex() == (a != b)
            kref = p.multipliers[S.pair_index(a, b, K)]
            assert R.rel(k.cpu().numpy(), kref.real if a == b else kref) <= bar
        op.close()
    if len(paths) == 2:
        for a in range(K):
            err = R.rel(got["fused"][a], got["dense"][a])
            print(f"  fused vs dense a={a}: {err:.3e}")
            assert err <= bar


@pytest.mark.parametrize("Z,Ns,path", [("c128", (48, 40), "fused"), ("c64", (48, 40), "fused"), ("c128", (100,), "dense"),
                                       ("c64", (32, 32, 32), "fused")])
def test_one_component_with_unit_basis_is_the_plain_operator(Z, Ns, path):
    from nufft_pkg import nufft
    T, Zc, bar, _ = _dt(Z)
    p = _problem(Ns, 1)
    pd, wd = tuple(_dev(x, T) for x in p.xs), _dev(p.w, T)
    _, plain = _op(nufft, Z, Ns, path, 1)
    _, op = _op(nufft, Z, Ns, path, 1)
    plain.set_points(pd, wd)
    op.set_points(pd, wd, basis=torch.ones(NP, dtype=op.Z, device="cuda"))          # a vector is K = 1
    assert op.coupled and not plain.coupled
    a, b = _apply(op, p.us, Zc)[0], _apply(plain, p.us, Zc)[0]
    err, errk = R.rel(a, b), R.rel(op.multiplier(0, 0).cpu().numpy(), plain.multiplier().cpu().numpy())
    print(f"K = 1, unit basis {Z} N={Ns} {path}: apply {err:.3e}, multiplier {errk:.3e}")
    assert err <= bar and errk <= bar
    with pytest.raises(ValueError):
        op.multiplier()
    with pytest.raises(ValueError):
        plain.multiplier(0, 0)


def _composed(nufft, plan, pd, wd, phid, ud, K):
    """The only route without this operator: exec_type2 of the K components, the mix at the samples in torch, exec_type1."""
    nufft.set_points(plan, pd)
    vs = tuple(torch.empty(NP, dtype=plan.Z, device="cuda") for _ in range(K))
    nufft.exec_type2(vs if K > 1 else vs[0], plan, ud if K > 1 else ud[0])
    y = sum(phid[b] * vs[b] for b in range(K))
    mixed = tuple((wd * phid[a].conj() * y).contiguous() for a in range(K))
    out = tuple(torch.empty_like(u) for u in ud)
    nufft.exec_type1(out if K > 1 else out[0], plan, mixed if K > 1 else mixed[0])
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


# (Z, N, path, K, clustered, zero row)
POINT_CASES = [(Z, Ns, path, K, False, False) for Z in ("c128", "c64")
               for Ns, path, K in (((32, 32, 32), "fused", 2), ((48, 40), "fused", 3), ((100,), "dense", 3))]
POINT_CASES += [("c128", (48, 40), "fused", 2, True, False), ("c128", (48, 40), "fused", 3, False, True), ("c64", (100,), "dense", 2, False, True)]


@pytest.mark.parametrize("Z,Ns,path,K,clustered,zero_row", POINT_CASES)
def test_built_from_points(Z, Ns, path, K, clustered, zero_row):
    from nufft_pkg import nufft
    T, Zc, _, _ = _dt(Z)
    p = _problem(Ns, K, clustered=clustered, zero_row=zero_row)
    xs, w, phi, us = [x.astype(T) for x in p.xs], p.w.astype(T), p.phi.astype(Zc), [u.astype(Zc) for u in p.us]
    refs = S.exact_block_gram(Ns, [x.astype(np.float64) for x in xs], w.astype(np.float64), phi.astype(np.complex128),
                              [u.astype(np.complex128) for u in us])
    plan, op = _op(nufft, Z, Ns, path, K)
    pd, wd, phid, ud = tuple(_dev(x) for x in xs), _dev(w), _dev(phi), tuple(_dev(u) for u in us)
    comp = _composed(nufft, plan, pd, wd, phid, ud, K)
    op.set_points(pd, wd, basis=phid)
    assert op.coupled and op.path == path
    got = _apply(op, us, Zc)
    for a in range(K):
        if zero_row and a == K - 1:
            assert not np.any(got[a])                               # φ_a = 0: an exactly zero block row
            continue
        err_t, err_c = R.rel(got[a], refs[a]), R.rel(comp[a], refs[a])
        print(f"from points {Z} N={Ns} {path} K={K} clustered={clustered} zero_row={zero_row} a={a}: coupled {err_t:.3e}, composed {err_c:.3e}, "
              f"ratio {err_t / err_c:.2f}")
        if Z == "c128":
            assert err_t <= 3 * err_c
        else:
            assert err_t <= max(5 * err_c, 1e-4)


@pytest.mark.parametrize("Ns,path", [((32, 32, 32), "fused"), ((48, 40), "fused"), ((48, 40), "dense"), ((100,), "dense")])
def test_structure(Ns, path):
    from nufft_pkg import nufft
    bar, K = 1e-12, 2 if len(Ns) == 3 else 3
    p = _problem(Ns, K)
    rng = np.random.default_rng(1)
    vs = [rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1]) for _ in range(K)]
    _, op = _op(nufft, "c128", Ns, path, K)
    op.set_points(tuple(_dev(x) for x in p.xs), _dev(p.w), basis=_dev(p.phi))
    Gu, Gv = np.stack(_apply(op, p.us, np.complex128)), np.stack(_apply(op, vs, np.complex128))
    u, v = np.stack(p.us), np.stack(vs)
    lhs, rhs = np.vdot(u, Gv), np.conj(np.vdot(v, Gu))              # <u, G v> = <G u, v>
    assert abs(lhs - rhs) <= bar * np.linalg.norm(u) * np.linalg.norm(Gv)
    assert np.vdot(u, Gu).real >= -bar * np.linalg.norm(u) * np.linalg.norm(Gu)
    for a in range(K):
        for b in range(a, K):
            k, kref = op.multiplier(a, b).cpu().numpy(), p.multipliers[S.pair_index(a, b, K)]
            err = R.rel(k, kref.real if a == b else kref)
            print(f"multiplier({a}, {b}) N={Ns} {path}: {err:.3e} against the exact one")
            assert err <= 1e-5              # built by a type 1 of the default window (test_gpu_toeplitz holds its Gram product to 1e-5)
    with pytest.raises(ValueError):
        op.multiplier(1, 0)


@pytest.mark.parametrize("Z,Ns,path", [("c128", (48, 40), "fused"), ("c64", (32, 32, 32), "fused"), ("c128", (100,), "dense")])
def test_orthogonal_supports_decouple(Z, Ns, path):
    """φ_0 lives on the first half of the samples, φ_1 on the second: zero cross blocks, two independent plain operators."""
    from nufft_pkg import nufft
    T, Zc, bar, _ = _dt(Z)
    p = _problem(Ns, 2)
    half = NP // 2
    phi = np.zeros((2, NP), dtype=Zc)
    phi[0, :half], phi[1, half:] = 1.0, 1.0
    pd, wd = tuple(_dev(x, T) for x in p.xs), _dev(p.w, T)
    _, op = _op(nufft, Z, Ns, path, 2)
    op.set_points(pd, wd, basis=_dev(phi))
    got = _apply(op, p.us, Zc)
    assert not np.any(op.multiplier(0, 1).cpu().numpy())            # w conj(φ_0) φ_1 = 0 exactly
    for a, sl in ((0, slice(0, half)), (1, slice(half, NP))):
        _, plain = _op(nufft, Z, Ns, path, 1)
        plain.set_points(tuple(x[sl].contiguous() for x in pd), wd[sl].contiguous())
        want = _apply(plain, [p.us[a]], Zc)[0]
        err = R.rel(got[a], want)
        print(f"orthogonal supports {Z} N={Ns} {path} a={a}: {err:.3e} (bar {bar:g})")
        assert err <= bar               # the coupled build spreads exact zeros for the other half: the same sums in another order


def _maps(Ns, ncoils, Zc, seed=9):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((ncoils,) + Ns[::-1]) + 1j * rng.standard_normal((ncoils,) + Ns[::-1])
    return (m / np.sqrt((np.abs(m) ** 2).sum(axis=0))).astype(Zc)


@pytest.mark.parametrize("Z,Ns,path", [("c128", (32, 32, 32), "fused"), ("c64", (32, 32, 32), "fused"), ("c128", (48, 40), "dense"),
                                       ("c64", (48, 40), "dense")])
def test_with_coil_maps(Z, Ns, path):
    from nufft_pkg import nufft
    T, Zc, bar, _ = _dt(Z)
    K, ncoils = 2, 3
    p = _problem(Ns, K)
    _, op = _op(nufft, Z, Ns, path, K)
    op.set_spectra(_dev(np.stack(p.spectra), Zc))
    md, ud = _dev(_maps(Ns, ncoils, Zc)), tuple(_dev(u, Zc) for u in p.us)
    want = [torch.zeros_like(u) for u in ud]
    for c in range(ncoils):                                          # the coil loop in torch around the coupled apply without maps
        g = op.apply(tuple((md[c] * u).contiguous() for u in ud))
        for a in range(K):
            want[a] += md[c].conj() * g[a]
    op.set_maps(md)
    assert op.coupled and op.ncoils == ncoils
    first = [o.clone() for o in op.apply(ud)]
    second = op.apply(ud)
    torch.cuda.synchronize()
    for a in range(K):
        err = R.rel(first[a].cpu().numpy(), want[a].cpu().numpy())
        print(f"coil maps {Z} N={Ns} {path} a={a}: {err:.3e} (bar {bar:g})")
        assert err <= bar
        assert torch.equal(first[a], second[a])                     # fixed coil order, no atomics
    for with_maps in (True, False):
        if not with_maps:
            op.clear_maps()
        with pytest.raises(ValueError):
            op.apply(ud, out=ud)
        with pytest.raises(ValueError):
            op.apply(ud, out=(ud[1], torch.empty_like(ud[0])))       # out[0] is in[1]
        out, tab = (ud[1], torch.empty_like(ud[0])), nufft.plan._ptr_table       # and in the library itself
        assert nufft.lib.nufft_toeplitz_apply(op._handle, tab(out), tab(ud), None) == nufft._lib.ERR_INVALID_ARG


@pytest.mark.parametrize("Z,Ns,path,ncoils", [("c128", (32, 32, 32), "fused", 0), ("c64", (48, 40), "fused", 3), ("c128", (48, 40), "dense", 3),
                                              ("c64", (100,), "dense", 0)])
def test_apply_in_a_graph(Z, Ns, path, ncoils):
    from nufft_pkg import nufft
    T, Zc, _, _ = _dt(Z)
    K = 2
    p = _problem(Ns, K)
    _, op = _op(nufft, Z, Ns, path, K)
    op.set_spectra(_dev(np.stack(p.spectra), Zc))
    if ncoils:
        op.set_maps(_dev(_maps(Ns, ncoils, Zc)))
    ud = tuple(_dev(u, Zc) for u in p.us)
    spec, pd, phid = _dev(np.stack(p.spectra), Zc), tuple(_dev(x, T) for x in p.xs), _dev(p.phi, Zc)
    eager = [o.cpu().numpy() for o in op.apply(ud)]
    out = tuple(torch.empty_like(u) for u in ud)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        op.apply(ud, out=out)
        with pytest.raises(ValueError):                             # a coupled build on a capturing stream is refused
            op.set_spectra(spec)
        with pytest.raises(ValueError):
            op.set_points(pd, basis=phid)
    assert op.coupled and op.info().has_spectrum == 1               # ... before it touched the operator
    for _ in range(2):
        for o in out:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a in range(K):
            assert np.array_equal(out[a].cpu().numpy(), eager[a])
    del graph


class System:
    """A coupled system for CG: NP points, a mixed Fourier basis (all cross blocks present), exact spectra; the float64 block apply
    through the reference multipliers, λmax by power iteration, λ = 0.2 λmax (cond <= 6.25, see the module docstring)."""

    def __init__(self, Ns, K, coupling="fourier"):
        self.p = _problem(Ns, K, coupling=coupling)
        self.Ns, self.K, self.shape = Ns, K, Ns[::-1]
        Ks = self.p.multipliers
        self.apply = lambda ps: S.block_apply(Ns, Ks, [np.asarray(q).astype(np.complex128) for q in ps])
        rng = np.random.default_rng(5)
        self.bs = [rng.standard_normal(self.shape) + 1j * rng.standard_normal(self.shape) for _ in range(K)]
        v = [b.copy() for b in self.bs]
        for _ in range(20):
            g = self.apply(v)
            self.lmax = float(np.linalg.norm(np.stack(g)) / np.linalg.norm(np.stack(v)))
            v = [x / np.linalg.norm(np.stack(g)) for x in g]
        self.lam = 0.2 * self.lmax

    def true_residual(self, lam, xs, bs):
        g = self.apply(xs)
        r = np.stack([np.asarray(b).astype(np.complex128) - (ga + lam * np.asarray(x).astype(np.complex128)) for b, ga, x in zip(bs, g, xs)])
        return float(np.linalg.norm(r) / np.linalg.norm(np.stack(bs).astype(np.complex128)))

    def operator(self, nufft, Z, path):
        _, Zc, _, _ = _dt(Z)
        plan, op = _op(nufft, Z, self.Ns, path, self.K)
        op.set_spectra(_dev(np.stack(self.p.spectra), Zc))
        plan.close()
        return op


_SYSTEMS = {}


def _system(Ns, K, coupling="fourier"):
    if (Ns, K, coupling) not in _SYSTEMS:
        _SYSTEMS[(Ns, K, coupling)] = System(Ns, K, coupling)
    return _SYSTEMS[(Ns, K, coupling)]


def _solve(sol, bs, **kw):
    x = sol.solve(tuple(_dev(b) for b in bs), **kw)
    torch.cuda.synchronize()
    return [v.cpu().numpy() for v in x], sol.iterations, sol.status, sol.history().numpy()


CG_CASES = [(Z, Ns, path) for Z in ("c128", "c64") for Ns, path in (((48, 40), "fused"), ((32, 32, 32), "fused"), ((48, 40), "dense"))]


@pytest.mark.parametrize("Z,Ns,path", CG_CASES)
def test_cg_fixed_iteration_count(Z, Ns, path):
    from nufft_pkg import nufft
    T, Zc, bar, _ = _dt(Z)
    s = _system(Ns, 3)
    op = s.operator(nufft, Z, path)
    bs = [b.astype(Zc) for b in s.bs]
    sol = nufft.ToeplitzCG(op, maxiter=5, rtol=0.0, lam=s.lam)
    xs, iters, status, hist = _solve(sol, bs)
    assert iters == (5,) * 3 and status == ("max_iter",) * 3 and hist.shape == (6, 3)
    assert np.array_equal(hist[:, 0], hist[:, 1]) and np.array_equal(hist[:, 0], hist[:, 2])       # one system: one history
    ref = S.joint_cg(s.apply, bs, lam=s.lam, rtol=0.0, max_iter=5, dtype=Zc)
    ex, eh = R.rel(np.stack(xs), ref["x"]), R.rel(hist[:, 0], ref["history"])
    print(f"joint CG, 5 iterations {Z} N={Ns} {path}: x {ex:.3e}, history {eh:.3e} (bar {10 * bar:g})")
    assert ex <= 10 * bar and eh <= 10 * bar
    sol.close()


@pytest.mark.parametrize("Z,Ns,path", CG_CASES)
def test_cg_converged_and_the_two_modes(Z, Ns, path):
    from nufft_pkg import nufft
    T, Zc, _, rtol = _dt(Z)
    s = _system(Ns, 3)
    op = s.operator(nufft, Z, path)
    bs = [b.astype(Zc) for b in s.bs]
    sol = nufft.ToeplitzCG(op, maxiter=100, rtol=rtol, lam=s.lam, check_every=0)
    xs, iters, status, hist = _solve(sol, bs)
    ref = S.joint_cg(s.apply, bs, lam=s.lam, rtol=rtol, max_iter=100, dtype=Zc)
    tr = s.true_residual(s.lam, xs, bs)
    print(f"joint CG converged {Z} N={Ns} {path}: {iters} iterations (reference {ref['iterations']}), true residual / rtol {tr / rtol:.3f}")
    assert status == ("converged",) * 3 and len(set(iters)) == 1 and len(set(sol.residual)) == 1
    assert tr <= 2 * rtol and abs(iters[0] - ref["iterations"]) <= 0.1 * ref["iterations"] + 1
    assert np.array_equal(hist[:, 0], hist[:, 1], equal_nan=True) and np.array_equal(hist[:, 0], hist[:, 2], equal_nan=True)
    chk = nufft.ToeplitzCG(op, maxiter=100, rtol=rtol, lam=s.lam, check_every=3)
    xc, ic, sc, hc = _solve(chk, bs)
    assert (ic, sc) == (iters, status) and np.array_equal(hc, hist, equal_nan=True)
    assert all(np.array_equal(a, b) for a, b in zip(xs, xc))
    # captured, replayed twice: the bits of the eager solve
    bd = tuple(_dev(b) for b in bs)
    out = tuple(torch.zeros_like(b) for b in bd)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sol.solve(bd, out=out)
    for _ in range(2):
        for o in out:
            o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert sol.iterations == iters and np.array_equal(sol.history().numpy(), hist, equal_nan=True)
        assert all(np.array_equal(o.cpu().numpy(), x) for o, x in zip(out, xs))
    del graph
    sol.close()
    chk.close()


@pytest.mark.parametrize("Z,path", [("c128", "fused"), ("c64", "dense")])
def test_cg_more_components_than_one_launch_takes(Z, path):
    """K = 9: the solver's kernels take eight components per launch, so the joint sums span two launches of every kernel."""
    from nufft_pkg import nufft
    T, Zc, bar, _ = _dt(Z)
    s = _system((32, 32), 9)
    op = s.operator(nufft, Z, path)
    bs = [b.astype(Zc) for b in s.bs]
    sol = nufft.ToeplitzCG(op, maxiter=5, rtol=0.0, lam=s.lam)
    xs, iters, status, hist = _solve(sol, bs)
    assert iters == (5,) * 9 and status == ("max_iter",) * 9 and all(np.array_equal(hist[:, 0], hist[:, c]) for c in range(9))
    ref = S.joint_cg(s.apply, bs, lam=s.lam, rtol=0.0, max_iter=5, dtype=Zc)
    ex, eh = R.rel(np.stack(xs), ref["x"]), R.rel(hist[:, 0], ref["history"])
    print(f"joint CG, K = 9, 5 iterations {Z} {path}: x {ex:.3e}, history {eh:.3e} (bar {10 * bar:g})")
    assert ex <= 10 * bar and eh <= 10 * bar
    sol.close()


def test_cg_joint_mode_on_strong_cross_blocks():
    """φ_1 ≈ φ_0: the cross blocks are as large as the diagonal ones.  CG with one α and one ρ per COMPONENT (the uncoupled solver) is
    not CG on this operator; the joint scalars are, and reach rtol."""
    from nufft_pkg import nufft
    Ns, rtol = (48, 40), 1e-10
    p = _problem(Ns, 2)
    phi = np.stack([p.phi[0], 0.9 * p.phi[0] + 0.3 * p.phi[1]])
    spectra = S.exact_spectra(Ns, p.xs, p.w, phi)
    Ks = S.multipliers(Ns, spectra)
    cross = np.linalg.norm(Ks[1]) / np.linalg.norm(Ks[0])
    assert cross > 0.5, cross
    apply = lambda ps: S.block_apply(Ns, Ks, [np.asarray(q).astype(np.complex128) for q in ps])
    v = [u.copy() for u in p.us]
    for _ in range(30):
        g = apply(v)
        lmax = float(np.linalg.norm(np.stack(g)) / np.linalg.norm(np.stack(v)))
        v = [x / np.linalg.norm(np.stack(g)) for x in g]
    lam = 0.05 * lmax
    _, op = _op(nufft, "c128", Ns, "fused", 2)
    op.set_spectra(_dev(np.stack(spectra)))
    sol = nufft.ToeplitzCG(op, maxiter=200, rtol=rtol, lam=lam)
    xs, iters, status, hist = _solve(sol, p.us)
    g = apply(xs)
    r = np.stack([b - (ga + lam * x) for b, ga, x in zip(p.us, g, xs)])
    tr = float(np.linalg.norm(r) / np.linalg.norm(np.stack(p.us)))
    print(f"joint mode, |K_01| / |K_00| = {cross:.2f}: {iters} iterations, true residual / rtol {tr / rtol:.3f}")
    assert status == ("converged", "converged") and iters[0] == iters[1] and tr <= 2 * rtol
    assert np.all(np.diff(hist[: iters[0] + 1, 0]) < 0) or hist[iters[0], 0] <= rtol       # CG on an SPD system: the residual arrives


def test_uncoupled_solver_is_unchanged_around_a_coupled_one():
    from nufft_pkg import nufft
    Ns, K = (48, 40), 2
    p = _problem(Ns, K)
    _, op = _op(nufft, "c64", Ns, "fused", K)
    plain_spec = _dev(R.exact_spectrum(Ns, p.xs, p.w), np.complex64)
    bs = [u.astype(np.complex64) for u in p.us]
    sol = nufft.ToeplitzCG(op, maxiter=8, rtol=0.0, lam=1.0)
    op.set_spectrum(plain_spec)
    before = _solve(sol, bs)
    g_before = _apply(op, bs, np.complex64)
    op.set_spectra(_dev(np.stack(p.spectra), np.complex64))
    coupled = _solve(sol, bs)
    assert op.coupled and np.array_equal(coupled[3][:, 0], coupled[3][:, 1])
    op.set_spectrum(plain_spec)
    assert not op.coupled
    after = _solve(sol, bs)
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and np.array_equal(before[3], after[3])
    assert all(np.array_equal(a, b) for a, b in zip(g_before, _apply(op, bs, np.complex64)))
    assert not np.array_equal(before[3][:, 0], before[3][:, 1])     # independent components: two histories


def test_refusals_and_lifetime():
    from nufft_pkg import nufft
    Ns, K = (48, 40), 2
    p = _problem(Ns, K)
    plan, op = _op(nufft, "c128", Ns, "fused", K)
    pd, wd, phid = tuple(_dev(x) for x in p.xs), _dev(p.w), _dev(p.phi)
    spec = _dev(np.stack(p.spectra))
    # shapes and dtypes of basis / T (the exception types of _check_uniform)
    with pytest.raises(nufft.DimensionMismatch):
        op.set_points(pd, wd, basis=phid[:1])
    with pytest.raises(nufft.DimensionMismatch):
        op.set_points(pd, wd, basis=phid[:, :-1].contiguous())
    with pytest.raises(ValueError):
        op.set_points(pd, wd, basis=phid.to(torch.complex64))
    with pytest.raises(ValueError):
        op.set_points(pd, wd, basis=phid.cpu())
    with pytest.raises(ValueError):
        op.set_points(pd, wd, basis=torch.stack([phid, phid], dim=2)[:, :, 0])      # not contiguous
    with pytest.raises(nufft.DimensionMismatch):
        op.set_spectra(spec[:2])
    with pytest.raises(nufft.DimensionMismatch):
        op.set_spectra(spec[:, :-1].contiguous())
    with pytest.raises(ValueError):
        op.set_spectra(spec.to(torch.complex64))
    assert not op.coupled
    # workspace: the multipliers (K² real grids) and K intermediates, gone after a plain build
    pad = lambda b: (max(b, 16) + 255) // 256 * 256
    cells = int(np.prod([2 * n for n in Ns]))
    base = op.info().workspace_bytes
    op.set_points(pd, wd, basis=phid)
    grown = pad(K * cells * 8) + pad(K * (K - 1) // 2 * cells * 16) + K * pad(Ns[0] * 2 * Ns[1] * 16)
    assert op.info().workspace_bytes == base + grown, (op.info().workspace_bytes - base, grown)
    op.set_spectra(spec)
    assert op.info().workspace_bytes == base + grown                # kept across coupled builds
    op.set_points(pd, wd)
    assert op.info().workspace_bytes == base and not op.coupled
    with pytest.raises(ValueError):
        op.multiplier(0, 1)
    # K lines that do not fit one wave on a fused operator: ComplexF64, 2 N_1 = 1024, K = 16; the message names the way out
    big, bop = _op(nufft, "c128", (512, 32), "fused", 16)
    with pytest.raises(Exception, match="NUFFT_TOEPLITZ_FUSED=0"):
        bop.set_points(tuple(_dev(x) for x in p.xs), basis=torch.ones((16, NP), dtype=torch.complex128, device="cuda"))
    assert not bop.coupled and bop.path == "fused"
    # the streaming route of the maps does not combine with coupling, in either order
    _, sop = _op(nufft, "c128", Ns, "fused", K, NUFFT_TOEPLITZ_MAPS_INPASS=0)
    md = _dev(_maps(Ns, 2, np.complex128))
    sop.set_spectra(spec)
    with pytest.raises(Exception, match="MAPS_INPASS"):
        sop.set_maps(md)
    sop.set_spectrum(spec[0])
    sop.set_maps(md)
    with pytest.raises(Exception, match="MAPS_INPASS"):
        sop.set_spectra(spec)
    with pytest.raises(Exception, match="MAPS_INPASS"):
        sop.set_points(pd, wd, basis=phid)
    assert not sop.coupled
