"""Total variation on the GPU: the difference operator against numpy, and the primal-dual solver against the numpy
reference (tv_reference.py) run in the same element type.  Systems, weights and cached references: tv_cases.py.  Operators get the exact
spectrum, so the only error in G is the operator's own.

Bars:
  * operator: ``gradient`` is one subtraction and must be bit-equal to numpy in the element type; ``adjoint`` <= 8 ε relative (D
    subtractions and D − 1 additions of O(1) values); ``norm`` <= 64 ε √n relative (the wavelet tests' bar for an FP64 sum of n terms
    formed from values of the element type).
  * ten iterations: x and both history columns within 1e-11 (ComplexF64) / 1e-4 (ComplexF32) relative, the project's bars.
  * converged solves (tol = 1e-6, check_every = 8): ComplexF64 stops at the reference's iteration count (191 on (48, 40), 184 on
    (64, 80); the changes around the crossing are 1.0115e-6 / 0.987e-6 and 1.0025e-6 / 0.979e-6, at least 0.25 % from tol, and the test
    asserts more than 0.1 %), and r, e, g of the device's x with the reference's dual variable (the library keeps its own to itself;
    any y in the dual ball is a certificate) are within 10 × the reference's own (r 7.5e-6 / 9.4e-6, e 2.2e-16, g 3.8e-7 / 2.2e-7).
    ComplexF32 with tol = 1e-4 stops within one iteration of its reference, and x is within 1e-4, the project's ComplexF32 bar, of the
    ComplexF64 solution for the same tol (the reference's two element types differ by 5.4e-8 / 7.2e-8 there).  The ComplexF64
    solution for tol = 1e-6 is no yardstick for the element type: the reference's own ComplexF32 result is 1.8e-3 from it on both
    systems, all of it the looser stopping tolerance.
  * fftshift = True against False after reordering: the operator's parity bar, 1e-12 / 1e-5.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import sense_reference as SR  # noqa: E402
import subspace_reference as S  # noqa: E402
import toeplitz_reference as R  # noqa: E402
import tv_cases as TC  # noqa: E402
import tv_reference as T  # noqa: E402

TYPES = ["c128", "c64"]
BAR = {"c128": 1e-11, "c64": 1e-4}
OPERATOR_SHAPES = [(9,), (48,), (7, 5), (24, 40), (5, 6, 7), (8, 12, 20), (64, 64, 64)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _solve(sol, bs, **kw):
    """solve + outcome as numpy; bs: list of host arrays (one per component)."""
    bd = tuple(_dev(b) for b in bs)
    x = sol.solve(bd if len(bs) > 1 else bd[0], **kw)
    torch.cuda.synchronize()
    xs = [v.cpu().numpy() for v in (x if len(bs) > 1 else (x,))]
    return xs, sol.iterations, sol.status, sol.history().numpy()


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("Ns", OPERATOR_SHAPES)
def test_operator(Ns, K, Z):
    from nufft_pkg import nufft
    _, Zc, _, eps = TC.dt(Z)
    D, shape, n = len(Ns), Ns[::-1], int(np.prod(Ns))
    rng = np.random.default_rng(sum(Ns) + K)
    plan = nufft.PlanNUFFT(Zc, Ns, backend=nufft.ROCBackend(0), ntransforms=K)
    tv = nufft.TotalVariation(plan)
    plan.close()
    xs = [(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(Zc) for _ in range(K)]
    ys = [(rng.standard_normal((D,) + shape) + 1j * rng.standard_normal((D,) + shape)).astype(Zc) for _ in range(K)]
    xd = tuple(_dev(x) for x in xs)
    yd = tuple(tuple(_dev(y[d]) for d in range(D)) for y in ys)
    g = tv.gradient(xd if K > 1 else xd[0])
    a = tv.adjoint(yd if K > 1 else yd[0])
    nrm = tv.norm(xd if K > 1 else xd[0])
    const = tv.gradient(tuple(torch.full_like(x, 2.5 - 1j) for x in xd) if K > 1 else torch.full_like(xd[0], 2.5 - 1j))
    torch.cuda.synchronize()
    g, a, const = (g, a, const) if K > 1 else ((g,), (a,), (const,))
    nrm = nrm.cpu().numpy()
    assert nrm.shape == (K,) and nrm.dtype == np.float64
    worst_a = worst_n = 0.0
    for c in range(K):
        assert len(g[c]) == D
        want = T.gradient(xs[c])
        for d in range(D):
            assert np.array_equal(g[c][d].cpu().numpy(), want[d]), (c, d)                   # one subtraction: the same bits
            assert not const[c][d].cpu().numpy().any()                                     # a constant has no gradient
        worst_a = max(worst_a, R.rel(a[c].cpu().numpy(), T.adjoint(ys[c].astype(np.complex128))))
        want_n = float(T.cell_norms(want).sum())
        worst_n = max(worst_n, abs(nrm[c] - want_n) / want_n)
        # <∇x, y> = <x, ∇ᴴy> with the device's results, in float64
        lhs = np.vdot(np.stack([u.cpu().numpy() for u in g[c]]).astype(np.complex128), ys[c].astype(np.complex128))
        rhs = np.vdot(xs[c].astype(np.complex128), a[c].cpu().numpy().astype(np.complex128))
        assert abs(lhs - rhs) <= 64 * eps * np.sqrt(n) * abs(lhs) + 64 * eps * n
    print(f"operator {Z} N={Ns} K={K}: adjoint {worst_a / eps:.2f} ε, norm {worst_n / eps:.2f} ε (bar {64 * np.sqrt(n):.0f} ε), tile {tuple(tv.info().tile)}")
    assert worst_a <= 8 * eps and worst_n <= 64 * eps * np.sqrt(n)
    with pytest.raises(ValueError):
        tv.gradient(xd[0][..., :-1].contiguous())
    tv.close()
    with pytest.raises(ValueError, match="closed"):
        tv.norm(xd if K > 1 else xd[0])


class _Coupled:
    """K = 2 coupled components from a system of tv_cases: T_ab = c_ab · T with a real symmetric positive definite c, so the joint
    operator is c ⊗ G, its apply two applies of G, and λmax = λmax(c) · λmax(G)."""
    c = np.array([[1.0, 0.3], [0.3, 0.8]])

    def __init__(self, s):
        self.s, self.lmax = s, float(np.linalg.eigvalsh(self.c)[-1]) * s.lmax

    def apply(self, p):
        g = [self.s.apply(p[0]), self.s.apply(p[1])]
        return np.stack([self.c[a, 0] * g[0] + self.c[a, 1] * g[1] for a in range(2)])

    def operator(self, nufft, Z, path):
        Zc = TC.dt(Z)[1]
        opts = {"NUFFT_TOEPLITZ_FUSED": 0} if path == "dense" else {}
        plan = nufft.PlanNUFFT(Zc, self.s.Ns, backend=nufft.ROCBackend(0), options=opts, ntransforms=2)
        op = nufft.ToeplitzOperator(plan)
        spectra = [None] * 3
        for a in range(2):
            for b in range(a, 2):
                spectra[S.pair_index(a, b, 2)] = self.c[a, b] * self.s.spec
        op.set_spectra(_dev(np.stack(spectra).astype(Zc)))
        plan.close()
        assert op.coupled and op.path == path
        return op


def _compare(tag, Z, xs, hist, ref, clipped=True, stacked=False):
    """x and both history columns against the reference, the projection's two branches on the reference."""
    x = np.stack(xs) if stacked else xs[0]
    ex, ec = R.rel(x, ref["x"]), R.rel(hist[:, 0, 0], ref["history"][:, 0])
    et = R.rel(hist[:, 0, 1], ref["history"][:, 1])
    share = float(ref["clipped"].mean())
    print(f"ten iterations {tag} {Z}: x {ex:.3e}, change {ec:.3e}, tv norm {et:.3e} (bar {BAR[Z]:g}), clipped {share:.2f}")
    assert ex <= BAR[Z] and ec <= BAR[Z] and et <= BAR[Z]
    if clipped:
        assert 0.2 <= share <= 0.95, share


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,path", TC.SOLVER_CASES)
def test_ten_iterations(Ns, path, Z):
    from nufft_pkg import nufft
    _, Zc, _, _ = TC.dt(Z)
    s = TC.system(Ns)
    b = s.bs[0].astype(Zc)
    tv = TC.tv_weight(s.bs[0])
    op = s.operator(nufft, Z, path, 1)
    for weight, lam in ((tv, 0.0), (0.0, 0.0), (tv, 0.1 * s.lmax)):
        sol = nufft.ToeplitzTV(op, tv=weight, step=TC.step(s, lam), lam=lam, maxiter=10, tol=0.0)
        xs, iters, status, hist = _solve(sol, [b])
        assert iters == (10,) and status == ("max_iter",) and hist.shape == (10, 1, 2)
        assert sol.info().iterations_enqueued == 10 and sol.sigma == 1.0 / (8 * len(Ns) * TC.step(s, lam))
        ref = TC.reference(Ns, Z, weight, lam, tol=0.0, max_iter=10)
        _compare(f"N={Ns} {path} tv={weight:.3g} lam={lam:.3g}", Z, xs, hist, ref, clipped=weight > 0)
        if weight == 0.0:
            # y must stay zero.  The library keeps y to itself, so only the reference's y can be looked at; the device's is checked
            # through x, which matches this plain gradient descent within the bar above (tv_dual_kernel with t = 0 scales every
            # v by t / |v| = 0, and |v| = 0 means v = 0)
            assert not ref["y"].any()
        sol.close()
    # 2 coil maps: G = Σ_j conj(S_j) G0 S_j, with the maps as the operator holds them
    maps = SR.smooth_maps(2, s.shape, seed=11).astype(Zc)
    m64 = maps.astype(np.complex128)
    apply = lambda v: sum(np.conj(m) * s.apply(m * np.asarray(v).astype(np.complex128)) for m in m64)      # noqa: E731
    step = TC.step(s) / float((np.abs(m64) ** 2).sum(axis=0).max())
    op.set_maps(_dev(maps))
    sol = nufft.ToeplitzTV(op, tv=tv, step=step, maxiter=10, tol=0.0)
    xs, iters, status, hist = _solve(sol, [b])
    ref = T.tvpd(apply, b, tv, step, tol=0.0, max_iter=10, dtype=Zc)
    _compare(f"N={Ns} {path} 2 coil maps", Z, xs, hist, ref)
    sol.close()
    op.close()
    # uncoupled K = 2 with two different weights: two independent solves
    op = s.operator(nufft, Z, path, 2)
    b2 = (0.5 * s.bs[1]).astype(Zc)
    sol = nufft.ToeplitzTV(op, tv=(tv, 0.4 * tv), step=TC.step(s), maxiter=10, tol=0.0)
    xs, iters, status, hist = _solve(sol, [b, b2])
    assert iters == (10, 10) and sol.tv == (tv, 0.4 * tv)
    _compare(f"N={Ns} {path} K=2, component 1", Z, xs[:1], hist[:, :1], TC.reference(Ns, Z, tv, 0.0, tol=0.0, max_iter=10))
    _compare(f"N={Ns} {path} K=2, component 2", Z, xs[1:], hist[:, 1:], T.tvpd(s.apply, b2, 0.4 * tv, TC.step(s), tol=0.0, max_iter=10, dtype=Zc))
    sol.close()
    op.close()
    # coupled K = 2: one system
    cp = _Coupled(s)
    op = cp.operator(nufft, Z, path)
    step = 1.0 / (1.05 * cp.lmax)
    sol = nufft.ToeplitzTV(op, tv=tv, step=step, maxiter=10, tol=0.0)
    xs, iters, status, hist = _solve(sol, [b, b2])
    ref = T.tvpd(cp.apply, np.stack([b, b2]), tv, step, tol=0.0, max_iter=10, dtype=Zc, component_axis=0)
    assert iters == (10, 10) and status == ("max_iter", "max_iter")
    assert _same(hist[:, 0, :], hist[:, 1, :]) and sol.change[0] == sol.change[1]          # one system: one change, one norm
    _compare(f"N={Ns} {path} coupled K=2", Z, xs, hist, ref, stacked=True)
    sol.close()
    op.close()


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,K", [((15, 9), 9), ((7, 6, 5), 2)])
def test_odd_rows_and_batches(Ns, K, Z):
    """Odd N_1: ComplexF32 rows are not 16-byte aligned, so the solver's kernels run with one cell per lane; nine transforms need two
    launches per kernel (eight components travel as kernel arguments).  Analytic spectra as in fista_cases; every component has its own
    right-hand side and weight 0.1 (1 + c / 10) max|b_c|, and is compared with its own reference run."""
    from nufft_pkg import nufft
    import fista_cases as FC
    _, Zc, _, _ = TC.dt(Z)
    s = FC.Analytic(Ns, seed=sum(Ns), nrhs=K)
    plan = nufft.PlanNUFFT(Zc, Ns, backend=nufft.ROCBackend(0), ntransforms=K)
    op = nufft.ToeplitzOperator(plan)
    op.set_spectrum(_dev(s.spec.astype(Zc)))
    plan.close()
    bs = [v.astype(Zc) for v in s.bs]
    tvs = tuple((1 + c / 10) * TC.tv_weight(b) for c, b in enumerate(bs))
    sol = nufft.ToeplitzTV(op, tv=tvs, step=TC.step(s), maxiter=10, tol=0.0)
    xs, iters, status, hist = _solve(sol, bs)
    assert iters == (10,) * K and status == ("max_iter",) * K
    for c in range(K):
        ref = T.tvpd(s.apply, bs[c], tvs[c], TC.step(s), tol=0.0, max_iter=10, dtype=Zc)
        _compare(f"N={Ns} component {c + 1} of {K}", Z, xs[c:c + 1], hist[:, c:c + 1], ref)
    sol.close()
    op.close()


@pytest.mark.parametrize("Ns,path", TC.SOLVER_CASES[:2])
def test_converged_solve(Ns, path):
    from nufft_pkg import nufft
    s = TC.system(Ns)
    tv = TC.tv_weight(s.bs[0])
    out = {}
    for Z, tol in (("c128", 1e-6), ("c64", 1e-4), ("c128", 1e-4)):
        Zc = TC.dt(Z)[1]
        b = s.bs[0].astype(Zc)
        op = s.operator(nufft, Z, path, 1)
        sol = nufft.ToeplitzTV(op, tv=tv, step=TC.step(s), maxiter=2000, tol=tol, check_every=8)
        xs, iters, status, hist = _solve(sol, [b])
        ref = TC.reference(Ns, Z, tv, 0.0, tol=tol, max_iter=2000)
        print(f"converged {Z} N={Ns} {path} tol={tol:g}: {iters[0]} iterations (reference {ref['iterations']}), change {sol.change[0]:.4e}, "
              f"enqueued {sol.info().iterations_enqueued}")
        assert status == ("converged",) and ref["status"] == T.CONVERGED
        assert sol.change[0] <= tol and hist[iters[0] - 1, 0, 0] == sol.change[0] and hist.shape[0] == iters[0]
        assert sol.info().iterations_enqueued == -(-iters[0] // 8) * 8 < 2000          # stopped at the first look after the component froze
        out[(Z, tol)] = (xs[0], iters[0], ref)
        sol.close()
        op.close()
    x, it, ref = out[("c128", 1e-6)]
    assert it == ref["iterations"]
    h = ref["history"][:, 0]
    assert abs(h[-1] / 1e-6 - 1) > 1e-3 and abs(h[-2] / 1e-6 - 1) > 1e-3                   # the crossing is not within 0.1 % of tol
    own = T.optimality(s.apply, s.bs[0], ref["x"], ref["y"], tv)
    got = T.optimality(s.apply, s.bs[0], x, ref["y"], tv)
    print(f"optimality N={Ns}: r {got[0]:.3e} (reference {own[0]:.3e}), e {got[1]:.3e} ({own[1]:.3e}), g {got[2]:.3e} ({own[2]:.3e})")
    assert all(v <= 10 * w for v, w in zip(got, own))
    x32, it32, ref32 = out[("c64", 1e-4)]
    assert abs(it32 - ref32["iterations"]) <= 1
    e32 = R.rel(x32, out[("c128", 1e-4)][0])
    print(f"ComplexF32 against ComplexF64 at tol 1e-4, N={Ns}: {e32:.3e} (bar {BAR['c64']:g})")
    assert e32 <= BAR["c64"]


@pytest.mark.parametrize("Z,Ns", [("c64", (64, 80)), ("c128", (16, 16, 8)), ("c64", (64, 64, 64))])
def test_determinism_modes_and_graph(Z, Ns):
    from nufft_pkg import nufft
    _, Zc, _, _ = TC.dt(Z)
    s = TC.system(Ns)
    op = s.operator(nufft, Z, TC.PATHS[Ns], 2)
    bs = [s.bs[0].astype(Zc), (0.4 * s.bs[1]).astype(Zc)]
    # on the CPU the reference needs 22 / 18, 182 / 280 and 39 / 33 iterations for the two components of the three cases
    kw = dict(tv=(TC.tv_weight(bs[0]), TC.tv_weight(bs[1])), step=TC.step(s), maxiter=320, tol=1e-3)
    a = nufft.ToeplitzTV(op, check_every=0, **kw)
    xa, ia, sa, ha = _solve(a, bs)
    print(f"modes {Z} N={Ns}: iterations {ia}")
    assert a.info().iterations_enqueued == 320 and sa == ("converged", "converged") and max(ia) < 320
    b = nufft.ToeplitzTV(op, check_every=4, **kw)
    xb, ib, sb, hb = _solve(b, bs)
    assert b.info().iterations_enqueued == -(-max(ia) // 4) * 4 < 320
    assert ia == ib and sa == sb and _same(ha, hb) and all(np.array_equal(u, v) for u, v in zip(xa, xb))
    x2, i2, s2, h2 = _solve(a, bs)                                               # two runs
    assert i2 == ia and s2 == sa and _same(h2, ha) and all(np.array_equal(u, v) for u, v in zip(xa, x2))
    if ia[0] != ia[1]:
        assert np.isnan(ha[min(ia):, int(np.argmin(ia))]).all()                  # a frozen component writes no history
    bd = tuple(_dev(v) for v in bs)
    out = tuple(torch.zeros_like(v) for v in bd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        a.solve(bd, out=out)
        with pytest.raises(ValueError):                                          # check_every > 0 synchronises: refused while capturing
            b.solve(bd, out=out)
    for _ in range(2):
        for o in out:
            o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert a.iterations == ia and a.status == sa and _same(a.history().numpy(), ha)
        assert all(np.array_equal(o.cpu().numpy(), v) for o, v in zip(out, xa))
    del graph


@pytest.mark.parametrize("Z,Ns,scale,tol", [("c64", (64, 80), 0.4, 1e-4), ("c128", (16, 16, 8), 0.5, 1e-3)])
def test_components(Z, Ns, scale, tol):
    """On the CPU the reference needs 50 / 35 iterations on (64, 80) and 182 / 280 on (16, 16, 8).  A warm start from the solution
    restarts y at zero, so the dual variable is built again: on the well-conditioned (64, 80) system that alone takes as long as the
    cold solve (reference: 50 / 35 again); on (16, 16, 8), where x converges slowly, the reference needs 32 / 15."""
    from nufft_pkg import nufft
    _, Zc, _, _ = TC.dt(Z)
    s = TC.system(Ns)
    op = s.operator(nufft, Z, TC.PATHS[Ns], 2)
    b1, b2 = s.bs[0].astype(Zc), (scale * s.bs[1]).astype(Zc)
    zero = np.zeros_like(b1)
    tvs = (TC.tv_weight(b1), TC.tv_weight(b2))
    sol = nufft.ToeplitzTV(op, tv=tvs, step=TC.step(s), maxiter=2000, tol=tol)
    xs, it, st, h = _solve(sol, [b1, b2])
    x1, it1, st1, h1 = _solve(sol, [b1, zero])
    x2, it2, st2, h2 = _solve(sol, [zero, b2])
    print(f"components {Z} N={Ns}: iterations {it}, alone {it1[0]}, {it2[1]}")
    assert st == ("converged", "converged") and abs(it[0] - it[1]) >= 3          # they stop at different iterations
    assert np.array_equal(xs[0], x1[0]) and np.array_equal(xs[1], x2[1])         # the early one is frozen: bit-equal to its own solve
    assert it[0] == it1[0] and it[1] == it2[1]
    assert _same(h[: it[0], 0], h1[: it[0], 0]) and _same(h[: it[1], 1], h2[: it[1], 1])
    assert it1[1] == 1 and st1[1] == "converged" and not x1[1].any() and h1[0, 1, 0] == 0.0      # a zero right-hand side
    assert it2[0] == 1 and st2[0] == "converged" and not x2[0].any()
    # set_tv: without the prior on component 2 its image is rougher; component 1 does not notice
    sol.set_tv((tvs[0], 0.0))
    xh, ith, _, hh = _solve(sol, [b1, b2])
    assert np.array_equal(xh[0], xs[0]) and hh[ith[1] - 1, 1, 1] > h[it[1] - 1, 1, 1]
    sol.set_tv(tvs)
    # a warm start from the solution; out is x0 is allowed
    bd = (_dev(b1), _dev(b2))
    x = tuple(_dev(v) for v in xs)
    again = sol.solve(bd, x0=x, out=x)
    torch.cuda.synchronize()
    assert all(u.data_ptr() == v.data_ptr() for u, v in zip(again, x)) and sol.status == ("converged", "converged")
    print(f"warm start: iterations {sol.iterations}")
    if Ns == (16, 16, 8):
        assert sol.iterations[0] < it[0] and sol.iterations[1] < it[1]
    else:
        assert sol.iterations[0] <= it[0] and sol.iterations[1] <= it[1]
    sol.close()
    op.close()


@pytest.mark.parametrize("Z", TYPES)
def test_fftshift_orders_agree(Z):
    """The operator commutes with cyclic shifts: a plan with fftshift = True solves the same problem in the shifted storage order."""
    from nufft_pkg import nufft
    import test_gpu_cg
    _, Zc, bar, _ = TC.dt(Z)
    Ns = (48, 40)
    s = TC.system(Ns)
    shifted = test_gpu_cg._system(Ns, fftshift=True)
    assert np.array_equal(shifted.spec, s.spec)                                  # the same points and weights
    b = s.bs[0].astype(Zc)
    tv = TC.tv_weight(s.bs[0])
    outs = []
    for sys_, rhs in ((s, b), (shifted, np.fft.fftshift(b))):
        op = sys_.operator(nufft, Z, "dense", 1)
        sol = nufft.ToeplitzTV(op, tv=tv, step=TC.step(s), maxiter=10, tol=0.0)
        xs, _, _, hist = _solve(sol, [np.ascontiguousarray(rhs)])
        outs.append((xs[0], hist))
        sol.close()
        op.close()
    ex, eh = R.rel(np.fft.ifftshift(outs[1][0]), outs[0][0]), R.rel(outs[1][1], outs[0][1])
    print(f"fftshift {Z}: x {ex:.3e}, history {eh:.3e} (bar {bar:g})")
    assert ex <= bar and eh <= bar                                               # the parity bar: 1e-12 / 1e-5


def test_lifetime_and_arguments():
    from nufft_pkg import nufft
    L, lib = nufft._lib, nufft.lib
    Ns = (48, 40)
    s = TC.system(Ns)
    plan = nufft.PlanNUFFT(np.complex128, Ns, backend=nufft.ROCBackend(0), ntransforms=2)
    op = nufft.ToeplitzOperator(plan)
    for kw in ({"maxiter": 0}, {"tol": -1.0}, {"lam": -1e-3}, {"step": 0.0}, {"step": float("nan")}, {"tv": -1.0}, {"tv": (0.1,)},
               {"check_every": -1}, {"sigma": 0.0}, {"sigma": float("inf")}):
        with pytest.raises(ValueError):
            nufft.ToeplitzTV(op, **{"step": 1.0, **kw})
    with pytest.raises(ValueError):
        nufft.ToeplitzTV(op)                                                      # step=None needs the spectrum for the power iteration
    with pytest.raises(ValueError):
        nufft.ToeplitzFISTA(op, prior="tv", step=1.0)
    sol = nufft.ToeplitzTV(op, tv=torch.tensor(0.125), step=0.4 / s.lmax, sigma=0.5, maxiter=5, tol=0.0)      # a 0-d tensor is a scalar
    assert sol.sigma == 0.5 and sol.tv == (0.125, 0.125) and "ToeplitzTV" in repr(sol)
    sol.set_tv(np.float32(0.25))
    assert sol.tv == (0.25, 0.25)
    b = tuple(_dev(v) for v in s.bs[:2])
    with pytest.raises(ValueError):                                               # NUFFT_ERR_NO_POINTS: no spectrum yet
        sol.solve(b)
    op.set_spectrum(_dev(s.spec))
    x = tuple(torch.zeros_like(v) for v in b)
    with pytest.raises(ValueError):
        sol.solve(b, out=b)                                                       # out is b
    with pytest.raises(ValueError):
        sol.solve(b, out=(x[0], x[0]))
    with pytest.raises(nufft.DimensionMismatch):
        sol.solve(b[0])
    with pytest.raises(ValueError):
        sol.solve(tuple(v.to(torch.complex64) for v in b))
    st = op._stream()
    import ctypes as C
    assert lib.nufft_tvpd_get_result(sol._handle, None, None, None, 1, st) == L.ERR_INVALID_ARG      # capacity < ntransforms
    assert lib.nufft_tvpd_history(sol._handle, (C.c_double * 4)(), 4, st) == L.ERR_INVALID_ARG
    assert lib.nufft_tvpd_set_tv(sol._handle, (C.c_double * 2)(0.1, -1.0), 2) == L.ERR_INVALID_ARG
    assert lib.nufft_tvpd_set_tv(sol._handle, (C.c_double * 2)(0.1, 0.1), 1) == L.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert not x[0].any() and not x[1].any()                                      # refused before anything was enqueued
    sol.solve(b, out=x)
    torch.cuda.synchronize()
    i = sol.info()
    pad = lambda v: (max(v, 16) + 255) // 256 * 256      # noqa: E731
    assert sol.iterations == (5, 5) and i.iterations_enqueued == 5 and i.array_bytes == 3 * 2 * pad(48 * 40 * 16) and i.ndim == 2
    assert i.array_bytes < i.workspace_bytes < i.array_bytes + (64 << 10)         # 1 + D arrays per component, nothing else of that size
    tvop = nufft.TotalVariation(op)
    y = tvop.gradient(x)
    with pytest.raises(ValueError):                                               # an output overlapping an input
        lib_rc = lib.nufft_tv_gradient(tvop._handle, nufft.plan._ptr_table([x[0], y[0][1], y[1][0], y[1][1]]), nufft.plan._ptr_table(x), st)
        nufft.plan._check(lib_rc)
    op.close()                                                                    # the library keeps a pointer to the operator
    for call in (lambda: sol.solve(b), sol.info, lambda: sol.iterations, sol.history):
        with pytest.raises(ValueError, match="outlive"):
            call()
    sol.close()
    with pytest.raises(ValueError, match="closed"):
        sol.info()


@pytest.mark.parametrize("Z", TYPES)
def test_breakdown_freezes_one_component(Z):
    """A NaN in one cell of b[1]: the reference's rule (tv_reference.tvpd: a change that is not finite is BREAKDOWN, and the iteration
    that found it is the last) for that component alone; component 0 runs as if b[1] were finite.  Then the same solver on finite data:
    the start kernel's reset leaves nothing behind."""
    from nufft_pkg import nufft
    import fista_cases as FC
    L, lib = nufft._lib, nufft.lib
    _, Zc, _, _ = TC.dt(Z)
    Ns = (16, 12)
    s = FC.Analytic(Ns, seed=4 * sum(Ns))
    plan = nufft.PlanNUFFT(Zc, Ns, backend=nufft.ROCBackend(0), ntransforms=2)
    op = nufft.ToeplitzOperator(plan)
    op.set_spectrum(_dev(s.spec.astype(Zc)))
    plan.close()
    good = [s.bs[0].astype(Zc), (0.4 * s.bs[1]).astype(Zc)]
    bad = [good[0], good[1].copy()]
    bad[1][5, 7] = np.nan
    kw = dict(tv=TC.tv_weight(s.bs[0]), step=TC.step(s), maxiter=4, tol=0.0)
    fresh = nufft.ToeplitzTV(op, **kw)
    xg, ig, sg, hg = _solve(fresh, good)
    assert ig == (4, 4) and sg == ("max_iter", "max_iter") and np.isfinite(hg).all()
    sol = nufft.ToeplitzTV(op, **kw)
    xb, ib, sb, hb = _solve(sol, bad)
    print(f"breakdown {Z}: iterations {ib}, status {sb}, history of component 1 {hb[:, 1, 0]}")
    assert sb[1] == "breakdown" and ib[1] == 1 and np.isnan(hb[0, 1, 0]) and np.isnan(sol.change[1])
    assert sb[0] == sg[0] and ib[0] == ig[0] and _same(hb[:, 0], hg[:, 0])
    assert R.rel(xb[0], xg[0]) <= BAR[Z]
    full = (C.c_double * (4 * 2 * 2))()
    assert lib.nufft_tvpd_history(sol._handle, full, len(full), op._stream()) == L.OK
    assert np.isnan(np.array(full).reshape(4, 2, 2)[1:, 1]).all()                  # the frozen component writes no later row
    x2, i2, s2, h2 = _solve(sol, good)                                             # a second solve on the solver that broke down
    assert i2 == ig and s2 == sg and _same(h2, hg) and all(np.array_equal(u, v) for u, v in zip(x2, xg))
    sol.close()
    fresh.close()
    op.close()
