"""Temporal total variation on the GPU: the difference along the components against numpy, and the primal-dual solver
with the temporal term against the numpy reference (tvt_reference.py) run in the same element type.  Systems, weights and cached
references: tvt_cases.py (framed operators with exact spectra, so the only error in G is the operator's own).

Bars:
  * operator: ``gradient_t`` and ``adjoint_t`` are one subtraction per value and must be bit-equal to numpy in the element type;
    ``norm_t`` <= 64 ε √n relative (an FP64 sum of n terms formed from values of the element type).
  * ten iterations: x and both history columns within 1e-11 (ComplexF64) / 1e-4 (ComplexF32) relative, the project's bars.
  * converged solve (temporal term only, tol = 1e-6, check_every = 8): ComplexF64 stops at the reference's iteration count (68; the
    changes around the crossing are 1.054e-6 / 0.895e-6, 5 % from tol) and reaches the reference's r and temporal gap to three digits,
    with the reference's z as the certificate (the library keeps its own to itself).  ComplexF32 with tol = 1e-4 stops within one
    iteration of its reference (40; 1.078e-4 / 0.911e-4).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import sense_reference as SR  # noqa: E402
import subspace_reference as S  # noqa: E402
import toeplitz_reference as R  # noqa: E402
import tvt_cases as TC  # noqa: E402
import tvt_reference as TT  # noqa: E402

TYPES = ["c128", "c64"]
BAR = {"c128": 1e-11, "c64": 1e-4}
OPERATOR_SHAPES = [(9,), (7, 5), (24, 40), (5, 6, 7)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _solve(sol, b, **kw):
    """solve + outcome as numpy; b: the stacked right-hand sides [K, ...] on the host."""
    bd = tuple(_dev(v) for v in b)
    x = sol.solve(bd, **kw)
    torch.cuda.synchronize()
    return np.stack([v.cpu().numpy() for v in x]), sol.iterations, sol.status, sol.history().numpy()


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("K", [2, 3, 9])
@pytest.mark.parametrize("Ns", OPERATOR_SHAPES)
def test_operator(Ns, K, periodic, Z):
    from nufft_pkg import nufft
    _, Zc, _, eps = TC.dt(Z)
    shape, n = Ns[::-1], int(np.prod(Ns))
    rng = np.random.default_rng(sum(Ns) + K)
    plan = nufft.PlanNUFFT(Zc, Ns, backend=nufft.ROCBackend(0), ntransforms=K)
    tv = nufft.TotalVariation(plan)
    plan.close()
    x = (rng.standard_normal((K,) + shape) + 1j * rng.standard_normal((K,) + shape)).astype(Zc)
    z = (rng.standard_normal((K,) + shape) + 1j * rng.standard_normal((K,) + shape)).astype(Zc)
    xd, zd = tuple(_dev(v) for v in x), tuple(_dev(v) for v in z)
    g = np.stack([v.cpu().numpy() for v in tv.gradient_t(xd, periodic)])
    a = np.stack([v.cpu().numpy() for v in tv.adjoint_t(zd, periodic)])
    nrm = tv.norm_t(xd, periodic).cpu().numpy()
    const = tv.gradient_t(tuple(xd[0].clone() for _ in range(K)), periodic)
    assert np.array_equal(g, TT.gradient_t(x, periodic))                          # one subtraction: the same bits
    assert np.array_equal(a, TT.adjoint_t(z, periodic))
    assert all(not v.cpu().numpy().any() for v in const)                          # constant in time: exact zeros
    if K == 2 and not periodic:
        assert not g[1].any()                                                     # the last frame has no successor
    assert nrm.shape == (K,) and nrm.dtype == np.float64
    want = TT.frame_norms_t(x, periodic)
    live = slice(None) if periodic else slice(0, K - 1)
    worst = float(np.max(np.abs(nrm[live] - want[live]) / want[live]))
    assert periodic or nrm[-1] == 0.0
    # <∇_t x, z> = <x, ∇_tᴴ z> with the device's results, in float64 (z_{K−1} does not take part on the non-periodic axis)
    zz = z.astype(np.complex128)
    if not periodic:
        zz[-1] = 0
    lhs, rhs = np.vdot(g.astype(np.complex128), zz), np.vdot(x.astype(np.complex128), a.astype(np.complex128))
    print(f"temporal operator {Z} N={Ns} K={K} periodic={periodic}: norm {worst / eps:.2f} ε (bar {64 * np.sqrt(n):.0f} ε)")
    assert worst <= 64 * eps * np.sqrt(n)
    assert abs(lhs - rhs) <= 64 * eps * np.sqrt(n * K) * abs(lhs) + 64 * eps * n * K
    with pytest.raises(ValueError):                                               # an output overlapping an input
        nufft.plan._check(nufft.lib.nufft_tv_gradient_t(tv._handle, nufft.plan._ptr_table(xd), nufft.plan._ptr_table(xd), 0, tv._stream()))
    with pytest.raises(nufft.DimensionMismatch):
        tv.gradient_t(xd[:-1], periodic)
    tv.close()


def _compare(tag, Z, x, hist, ref, condition=True):
    """x and both history columns against the reference; the projections' two branches on the reference's tenth iteration."""
    ex, ec, ep = R.rel(x, ref["x"]), R.rel(hist[:, :, 0], ref["history"][:, :, 0]), R.rel(hist[:, :, 1], ref["history"][:, :, 1])
    st = float(ref["clipped_t"][9])
    ss = float(ref["clipped_s"][9]) if ref["spatial"] else None
    print(f"ten iterations {tag} {Z}: x {ex:.3e}, change {ec:.3e}, prior {ep:.3e} (bar {BAR[Z]:g}), clipped: temporal {st:.2f}"
          + (f", spatial {ss:.2f}" if ref["spatial"] else ""))
    assert ex <= BAR[Z] and ec <= BAR[Z] and ep <= BAR[Z]
    assert (hist[:, :, 0] == hist[:, :1, 0]).all()                                # one system: the same change for every frame
    if condition:
        assert 0.2 <= st <= 0.95 and (ss is None or 0.2 <= ss <= 0.95), (st, ss)


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("spatial", [False, True])
@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("Ns,K,path", TC.SOLVER_CASES)
def test_ten_iterations(Ns, K, path, periodic, spatial, Z):
    from nufft_pkg import nufft
    Zc = TC.dt(Z)[1]
    s = TC.frames(Ns, K)
    tv, tv_t = TC.weights(Ns, K, periodic, spatial, s.b)
    op = s.operator(nufft, Z, path)
    sol = nufft.ToeplitzTV(op, tv=tv, tv_t=tv_t, periodic_t=periodic, step=s.step(), maxiter=10, tol=0.0)
    assert sol.spatial == spatial and sol.tv_t == tv_t and sol.sigma == 1.0 / (8 * ((len(Ns) + 1) if spatial else 1) * s.step())
    x, iters, status, hist = _solve(sol, s.b.astype(Zc))
    assert iters == (10,) * K and status == ("max_iter",) * K and hist.shape == (10, K, 2)
    ref = TC.reference(Ns, K, Z, tv, tv_t, periodic, spatial, tol=0.0, max_iter=10)
    _compare(f"N={Ns} K={K} periodic={periodic} spatial={spatial}", Z, x, hist, ref)
    pad = lambda v: (max(v, 16) + 255) // 256 * 256      # noqa: E731
    arrays = (2 + len(Ns)) if spatial else 2
    assert sol.info().array_bytes == arrays * K * pad(int(np.prod(Ns)) * np.dtype(Zc).itemsize)
    sol.close()
    op.close()


class _Coupled:
    """K = 2 coupled components: T_ab = c_ab · T with a real symmetric positive definite c, so the joint operator is c ⊗ G."""
    c = np.array([[1.0, 0.3], [0.3, 0.8]])

    def __init__(self, s):
        self.s, self.lmax = s, float(np.linalg.eigvalsh(self.c)[-1]) * s.lmax

    def apply(self, p):
        g = [self.s.frames[0].apply(p[0]), self.s.frames[0].apply(p[1])]
        return np.stack([self.c[a, 0] * g[0] + self.c[a, 1] * g[1] for a in range(2)])


@pytest.mark.parametrize("Z", TYPES)
def test_ten_iterations_on_every_operator_state(Z):
    """On (32, 40): a Tikhonov term, 2 coil maps on the framed operator, a plain operator (one shared multiplier), a coupled K = 2
    operator, and tv_t = 0."""
    from nufft_pkg import nufft
    Zc = TC.dt(Z)[1]
    Ns, K = (32, 40), 3
    s = TC.frames(Ns, K)
    b = s.b.astype(Zc)
    op = s.operator(nufft, Z, "fused")
    # lam = 0.1 λmax, spatial and temporal, periodic
    tv, tv_t = TC.weights(Ns, K, True, True, s.b)
    lam = 0.1 * s.lmax
    sol = nufft.ToeplitzTV(op, tv=tv, tv_t=tv_t, periodic_t=True, step=s.step(lam), lam=lam, maxiter=10, tol=0.0)
    x, _, _, hist = _solve(sol, b)
    _compare("N=(32, 40) lam=0.1 lmax", Z, x, hist, TC.reference(Ns, K, Z, tv, tv_t, True, True, lam=lam, tol=0.0, max_iter=10))
    sol.close()
    # tv_t = 0 without the spatial term: z stays exactly zero and the iteration is gradient descent.  The library keeps z to itself:
    # it is checked through x, and on the reference
    sol = nufft.ToeplitzTV(op, tv_t=0.0, step=s.step(), maxiter=10, tol=0.0)
    assert not sol.spatial
    x, _, _, hist = _solve(sol, b)
    ref = TC.reference(Ns, K, Z, 0.0, 0.0, False, False, tol=0.0, max_iter=10)
    assert not ref["z"].any() and not hist[:, :, 1].any() and not ref["history"][:, :, 1].any()      # the prior's value is 0 · ‖∇_t x‖₁
    ex, ec = R.rel(x, ref["x"]), R.rel(hist[:, :, 0], ref["history"][:, :, 0])
    print(f"ten iterations N=(32, 40) tv_t=0 {Z}: x {ex:.3e}, change {ec:.3e} (bar {BAR[Z]:g})")
    assert ex <= BAR[Z] and ec <= BAR[Z]
    sol.close()
    # 2 coil maps, the same for every frame: G_c = Σ_j conj(S_j) G0_c S_j
    tv, tv_t = TC.weights(Ns, K, False, False, s.b)
    maps = SR.smooth_maps(2, s.shape[1:], seed=11).astype(Zc)
    m64 = maps.astype(np.complex128)
    apply = lambda v: np.stack([sum(np.conj(m) * f.apply(m * np.asarray(v[c]).astype(np.complex128)) for m in m64)      # noqa: E731
                                for c, f in enumerate(s.frames)])
    step = s.step() / float((np.abs(m64) ** 2).sum(axis=0).max())
    op.set_maps(_dev(maps))
    sol = nufft.ToeplitzTV(op, tv_t=tv_t, step=step, maxiter=10, tol=0.0)
    x, _, _, hist = _solve(sol, b)
    _compare("N=(32, 40) 2 coil maps", Z, x, hist, TT.tvpd_t(apply, b, 0.0, tv_t, step, tol=0.0, max_iter=10, dtype=Zc))
    sol.close()
    op.close()
    # a plain operator: K components, one multiplier
    sh = TC.frames(Ns, K, shared=True)
    op = sh.operator(nufft, Z, "fused", framed=False)
    assert not op.framed
    tv, tv_t = TC.weights(Ns, K, True, True, sh.b)
    sol = nufft.ToeplitzTV(op, tv=tv, tv_t=tv_t, periodic_t=True, step=sh.step(), maxiter=10, tol=0.0)
    x, _, _, hist = _solve(sol, sh.b.astype(Zc))
    _compare("N=(32, 40) shared multiplier", Z, x, hist, TC.reference(Ns, K, Z, tv, tv_t, True, True, shared=True, tol=0.0, max_iter=10))
    sol.close()
    op.close()
    # a coupled K = 2 operator
    s2 = TC.frames(Ns, 2)
    cp = _Coupled(s2)
    plan = nufft.PlanNUFFT(Zc, Ns, backend=nufft.ROCBackend(0), ntransforms=2)
    op = nufft.ToeplitzOperator(plan)
    plan.close()
    pairs = [None] * 3
    for a in range(2):
        for c in range(a, 2):
            pairs[S.pair_index(a, c, 2)] = cp.c[a, c] * s2.spectra[0]
    op.set_spectra(_dev(np.stack(pairs).astype(Zc)))
    assert op.coupled and op.path == "fused"
    tv, tv_t = TC.weights(Ns, 2, False, False, s2.b)
    step = 1.0 / (1.05 * cp.lmax)
    sol = nufft.ToeplitzTV(op, tv_t=tv_t, step=step, maxiter=10, tol=0.0)
    x, _, _, hist = _solve(sol, s2.b.astype(Zc))
    _compare("N=(32, 40) coupled K=2", Z, x, hist, TT.tvpd_t(cp.apply, s2.b.astype(Zc), 0.0, tv_t, step, tol=0.0, max_iter=10, dtype=Zc))
    sol.close()
    op.close()


def test_converged_solve():
    from nufft_pkg import nufft
    Ns, K = (32, 40), 3
    s = TC.frames(Ns, K)
    tv, tv_t = TC.weights(Ns, K, False, False, s.b)
    out = {}
    for Z, tol in (("c128", 1e-6), ("c64", 1e-4)):
        Zc = TC.dt(Z)[1]
        op = s.operator(nufft, Z, "fused")
        sol = nufft.ToeplitzTV(op, tv_t=tv_t, step=s.step(), maxiter=2000, tol=tol, check_every=8)
        x, iters, status, hist = _solve(sol, s.b.astype(Zc))
        ref = TC.reference(Ns, K, Z, 0.0, tv_t, False, False, tol=tol, max_iter=2000)
        print(f"converged {Z} tol={tol:g}: {iters} iterations (reference {ref['iterations']}), change {sol.change[0]:.4e}, "
              f"enqueued {sol.info().iterations_enqueued}")
        assert status == ("converged",) * K and ref["status"] == TT.CONVERGED and len(set(iters)) == 1 and len(set(sol.change)) == 1
        assert sol.change[0] <= tol and hist[iters[0] - 1, 0, 0] == sol.change[0] and hist.shape[0] == iters[0]
        assert sol.info().iterations_enqueued == -(-iters[0] // 8) * 8 < 2000      # stopped at the first look after the system froze
        out[Z] = (x, iters[0], ref)
        sol.close()
        op.close()
    x, it, ref = out["c128"]
    assert it == ref["iterations"]
    h = ref["history"][:, 0, 0]
    assert abs(h[-1] / 1e-6 - 1) > 1e-3 and abs(h[-2] / 1e-6 - 1) > 1e-3           # the crossing is not within 0.1 % of tol
    b64 = s.b.astype(np.complex128)
    own = TT.optimality_t(s.apply, b64, ref["x"], None, ref["z"], tv_t)
    got = TT.optimality_t(s.apply, b64, x, None, ref["z"], tv_t)
    print(f"optimality: r {got[0]:.4e} (reference {own[0]:.4e}), e {got[1]:.3e} ({own[1]:.3e}), g {got[2]:.4e} ({own[2]:.4e})")
    assert abs(got[0] - own[0]) <= 1e-3 * own[0] and abs(got[2] - own[2]) <= 1e-3 * own[2] and got[1] == own[1]
    x32, it32, ref32 = out["c64"]
    assert abs(it32 - ref32["iterations"]) <= 1


@pytest.mark.parametrize("Z,Ns,K,spatial,periodic", [("c64", (32, 40), 3, True, False), ("c128", (5, 6, 7), 9, False, True)])
def test_determinism_modes_graph_and_warm_start(Z, Ns, K, spatial, periodic):
    """On the CPU the reference needs 55 iterations on (32, 40) with both terms and 311 on (5, 6, 7), K = 9, with the periodic temporal
    term for tol = 1e-3; a warm start from the solution restarts the duals at zero and needs 55 and 18."""
    from nufft_pkg import nufft
    Zc = TC.dt(Z)[1]
    s = TC.frames(Ns, K)
    op = s.operator(nufft, Z, TC.PATHS[(Ns, K)])
    b = s.b.astype(Zc)
    tv, tv_t = TC.weights(Ns, K, periodic, spatial, s.b)
    kw = dict(tv=tv, tv_t=tv_t, periodic_t=periodic, step=s.step(), maxiter=400, tol=1e-3)
    a = nufft.ToeplitzTV(op, check_every=0, **kw)
    xa, ia, sa, ha = _solve(a, b)
    print(f"modes {Z} N={Ns} K={K}: iterations {ia}")
    assert a.info().iterations_enqueued == 400 and sa == ("converged",) * K and len(set(ia)) == 1 and ia[0] < 400
    c = nufft.ToeplitzTV(op, check_every=4, **kw)
    xc, ic, sc, hc = _solve(c, b)
    assert c.info().iterations_enqueued == -(-ia[0] // 4) * 4 < 400
    assert ia == ic and sa == sc and _same(ha, hc) and np.array_equal(xa, xc)
    x2, i2, s2, h2 = _solve(a, b)                                                 # two runs
    assert i2 == ia and s2 == sa and _same(h2, ha) and np.array_equal(xa, x2)
    bd = tuple(_dev(v) for v in b)
    out = tuple(torch.zeros_like(v) for v in bd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        a.solve(bd, out=out)
        with pytest.raises(ValueError):                                           # check_every > 0 synchronises: refused while capturing
            c.solve(bd, out=out)
    for _ in range(2):
        for o in out:
            o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert a.iterations == ia and a.status == sa and _same(a.history().numpy(), ha)
        assert np.array_equal(np.stack([o.cpu().numpy() for o in out]), xa)
    del graph
    # a warm start from the solution (out is x0)
    x = tuple(_dev(v) for v in xa)
    again = c.solve(bd, x0=x, out=x)
    torch.cuda.synchronize()
    assert all(u.data_ptr() == v.data_ptr() for u, v in zip(again, x)) and c.status == ("converged",) * K
    print(f"warm start: iterations {c.iterations}")
    assert len(set(c.iterations)) == 1 and c.iterations[0] < 400
    a.close()
    c.close()
    op.close()


def test_arguments_and_the_spatial_switch():
    from nufft_pkg import nufft
    L, lib = nufft._lib, nufft.lib
    Ns, K = (32, 40), 3
    s = TC.frames(Ns, K)
    op = s.operator(nufft, "c128", "fused")
    for kw in ({"tv_t": -1.0}, {"tv_t": float("nan")}, {"tv_t": 0.1, "tv": -1.0}, {"periodic_t": True}, {"spatial": False}):
        with pytest.raises(ValueError):
            nufft.ToeplitzTV(op, **{"step": 1.0, **kw})
    sol = nufft.ToeplitzTV(op, tv_t=0.25, step=s.step(), maxiter=5, tol=0.0)      # no tv: the spatial term is off
    assert not sol.spatial and sol.temporal and sol.tv_t == 0.25 and sol.tv == (0.0,) * K
    pad = lambda v: (max(v, 16) + 255) // 256 * 256      # noqa: E731
    i = sol.info()
    assert i.array_bytes == 2 * K * pad(32 * 40 * 16)                             # q and z: two arrays per frame
    assert i.array_bytes < i.workspace_bytes < i.array_bytes + (64 << 10)         # nothing else of that size: no y
    with pytest.raises(ValueError, match="spatial"):
        sol.set_tv(0.1)
    sol.set_tv(0.0)
    sol.set_tv_t(0.5)
    assert sol.tv_t == 0.5
    with pytest.raises(ValueError):
        sol.set_tv_t(-0.5)
    assert lib.nufft_tvpd_set_tv(sol._handle, (L.C.c_double * K)(0.0, 0.0, 0.1), K) == L.ERR_INVALID_ARG
    sol.close()
    both = nufft.ToeplitzTV(op, tv=0.0, tv_t=0.25, spatial=True, step=s.step(), maxiter=5, tol=0.0)      # tv = 0 with the term kept
    assert both.spatial and both.info().array_bytes == 4 * K * pad(32 * 40 * 16)
    both.set_tv(0.1)
    both.close()
    plain = nufft.ToeplitzTV(op, tv=0.1, step=s.step(), maxiter=5, tol=0.0)      # today's solver: no temporal term to set or get
    assert not plain.temporal and plain.tv_t is None and plain.info().array_bytes == 3 * K * pad(32 * 40 * 16)
    with pytest.raises(ValueError):
        plain.set_tv_t(0.1)
    plain.close()
    op.close()
    # one component has no time axis
    plan = nufft.PlanNUFFT(np.complex128, Ns, backend=nufft.ROCBackend(0))
    one = nufft.ToeplitzOperator(plan)
    tvop = nufft.TotalVariation(plan)
    plan.close()
    one.set_spectrum(_dev(s.spectra[0]))
    with pytest.raises(ValueError, match="ntransforms"):
        nufft.ToeplitzTV(one, tv_t=0.1, step=s.step())
    u = (_dev(s.b[0]),)
    for call in (tvop.gradient_t, tvop.adjoint_t, tvop.norm_t):
        with pytest.raises(ValueError, match="ntransforms"):
            call(u)
    tvop.close()
    one.close()


@pytest.mark.parametrize("Z", TYPES)
def test_breakdown_freezes_the_system(Z):
    """A NaN in one cell of b[1]: the frames are one system, so the reference's rule (tvt_reference.tvpd_t: a change that is not finite is
    BREAKDOWN, and the iteration that found it is the last) holds for every frame.  Then the same solver on finite data: the start kernel's
    reset leaves nothing behind."""
    from nufft_pkg import nufft
    Ns, K = (16, 12), 3
    s = TC.Frames(Ns, K)
    op = s.operator(nufft, Z)
    good = s.b.astype(TC.dt(Z)[1])
    top = float(np.abs(s.b).max())
    kw = dict(tv=0.1 * top, tv_t=0.1 * top, step=s.step(), maxiter=4, tol=0.0)
    bad = good.copy()
    bad[1, 5, 7] = np.nan
    fresh = nufft.ToeplitzTV(op, **kw)
    xg, ig, sg, hg = _solve(fresh, good)
    assert ig == (4,) * 3 and sg == ("max_iter",) * 3 and np.isfinite(hg).all()
    sol = nufft.ToeplitzTV(op, **kw)
    _, ib, sb, hb = _solve(sol, bad)
    print(f"breakdown {Z}: iterations {ib}, status {sb}, history {hb.tolist()}")
    assert sb == ("breakdown",) * 3 and ib == (1,) * 3 and np.isnan(sol.change).all() and np.isnan(hb[0, :, 0]).all()
    full = (C.c_double * (4 * 3 * 2))()
    assert nufft.lib.nufft_tvpd_history(sol._handle, full, len(full), op._stream()) == nufft._lib.OK
    assert np.isnan(np.array(full).reshape(4, -1)[1:]).all()                       # the frozen system writes no later row
    x2, i2, s2, h2 = _solve(sol, good)                                      # a second solve on the solver that broke down
    assert i2 == ig and s2 == sg and _same(h2, hg) and np.array_equal(x2, xg)
    sol.close()
    fresh.close()
    op.close()
