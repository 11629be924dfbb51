"""TGV² on the GPU: the symmetrised gradient against numpy, and the primal-dual solver against the numpy reference
(tgv_reference.py) run in the same element type.  Systems, weights and cached references: tgv_cases.py.  Operators get the exact
spectrum, so the only error in G is the operator's own.

Bars:
  * operator: ``sym_gradient`` is two subtractions, one addition and one multiply by ½ in a fixed order, with no multiply-add to
    contract, and must be bit-equal to numpy in the element type; ``sym_adjoint`` <= 8 ε relative (D subtractions and D − 1 additions
    of O(1) values, as ∇ᴴ in test_gpu_tv.py); ``sym_norm`` <= 64 ε √n relative (an FP64 sum of n terms formed from values of the
    element type).
  * ten iterations: x, the field v and the three history columns within 1e-11 (ComplexF64) / 1e-4 (ComplexF32) relative, the project's
    bars.  With alpha0 = 0.5 alpha1 both projections run both branches: the reference clips 0.47 / 0.49 / 0.62 / 0.30 of the cells of p
    and 0.39 / 0.39 / 0.30 / 0.21 of those of r on the four systems (asserted in [0.1, 0.95]); with alpha0 = 2 alpha1 the projection of
    r clips nothing in ten iterations (the pass-through branch alone, no share condition).
  * converged solves (alpha0 = 0.5 alpha1, tol = 1e-6, check_every = 8): ComplexF64 stops at the reference's iteration count (289 on
    (48, 40), 371 on (64, 80); the changes around the crossing are 1.0169e-6 / 0.99846e-6 and 1.0107e-6 / 0.99769e-6, at least 0.15 %
    from tol, and the test asserts more than 0.1 %), and the six optimality numbers of the device's x and v with the reference's duals
    are within 10 × the reference's own, measured on the CPU: (48, 40): r_x 5.08e-6, r_v 1.27e-3, e_1 2.2e-16, e_0 2.2e-16, g_1 2.05e-5,
    g_0 9.7e-12; (64, 80): 7.28e-6, 1.84e-3, 2.2e-16, 4.4e-16, 4.41e-6, 1.88e-8 (``REACHED``).  ComplexF32 with tol = 1e-4 stops within
    one iteration of its reference (102 and 116), and x is within 1e-4 of the ComplexF64 result for the same tol (the reference's two
    element types differ by 5.2e-8 / 6.8e-8 there).
  * fftshift = True against False after reordering: the operator's parity bar, 1e-12 / 1e-5.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import fista_cases as FC  # noqa: E402
import sense_reference as SR  # noqa: E402
import subspace_reference as S  # noqa: E402
import tgv_cases as GC  # noqa: E402
import tgv_reference as G  # noqa: E402
import toeplitz_reference as R  # noqa: E402

TYPES = ["c128", "c64"]
BAR = {"c128": 1e-11, "c64": 1e-4}
OPERATOR_SHAPES = [(9,), (48,), (7, 5), (24, 40), (5, 6, 7), (8, 12, 20), (64, 64, 64)]
# the reference's own optimality at tol = 1e-6, alpha0 = 0.5 alpha1, ComplexF64 (measured on the CPU): r_x, r_v, e_1, e_0, g_1, g_0
REACHED = {(48, 40): (5.08e-6, 1.28e-3, 2.22e-16, 2.22e-16, 2.05e-5, 9.71e-12), (64, 80): (7.29e-6, 1.84e-3, 2.22e-16, 4.45e-16, 4.41e-6, 1.88e-8)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _field(sol, K):
    """field() as one host array [K, D, ...]."""
    v = sol.field()
    torch.cuda.synchronize()
    v = v if K > 1 else (v,)
    return np.stack([np.stack([u.cpu().numpy() for u in comp]) for comp in v])


def _solve(sol, bs, **kw):
    """solve + outcome as numpy; bs: list of host arrays (one per component).  Returns xs, v [K, D, ...], iterations, status, history."""
    bd = tuple(_dev(b) for b in bs)
    x = sol.solve(bd if len(bs) > 1 else bd[0], **kw)
    torch.cuda.synchronize()
    xs = [u.cpu().numpy() for u in (x if len(bs) > 1 else (x,))]
    return xs, _field(sol, len(bs)), sol.iterations, sol.status, sol.history().numpy()


def _analytic_operator(nufft, s, Zc, K):
    """An operator with the analytic spectrum of fista_cases.Analytic on whichever path the plan takes."""
    plan = nufft.PlanNUFFT(Zc, s.Ns, backend=nufft.ROCBackend(0), ntransforms=K)
    op = nufft.ToeplitzOperator(plan)
    op.set_spectrum(_dev(s.spec.astype(Zc)))
    plan.close()
    return op


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("Ns", OPERATOR_SHAPES)
def test_operator(Ns, K, Z):
    from nufft_pkg import nufft
    _, Zc, _, eps = GC.dt(Z)
    D, shape, n = len(Ns), Ns[::-1], int(np.prod(Ns))
    Sn = D * (D + 1) // 2
    rng = np.random.default_rng(sum(Ns) + K)
    plan = nufft.PlanNUFFT(Zc, Ns, backend=nufft.ROCBackend(0), ntransforms=K)
    tv = nufft.TotalVariation(plan)
    plan.close()
    draw = lambda *lead: (rng.standard_normal(lead + shape) + 1j * rng.standard_normal(lead + shape)).astype(Zc)      # noqa: E731
    vs, rs = [draw(D) for _ in range(K)], [draw(Sn) for _ in range(K)]
    vd = tuple(tuple(_dev(v[d]) for d in range(D)) for v in vs)
    rd = tuple(tuple(_dev(r[s]) for s in range(Sn)) for r in rs)
    cd = tuple(tuple(torch.full_like(u, 2.5 - 1j * d) for d, u in enumerate(comp)) for comp in vd)
    one = lambda t: t if K > 1 else t[0]      # noqa: E731
    e, a, nrm, const = tv.sym_gradient(one(vd)), tv.sym_adjoint(one(rd)), tv.sym_norm(one(vd)), tv.sym_gradient(one(cd))
    torch.cuda.synchronize()
    e, a, const = (e, a, const) if K > 1 else ((e,), (a,), (const,))
    nrm = nrm.cpu().numpy()
    assert nrm.shape == (K,) and nrm.dtype == np.float64
    worst_a = worst_n = 0.0
    for c in range(K):
        assert len(e[c]) == Sn and len(a[c]) == D
        want = G.sym_gradient(vs[c])
        for s in range(Sn):
            assert np.array_equal(e[c][s].cpu().numpy(), want[s]), (c, s)                   # the same bits
            assert not const[c][s].cpu().numpy().any()                                     # a constant field has no symmetrised gradient
        got_a = np.stack([u.cpu().numpy() for u in a[c]])
        worst_a = max(worst_a, R.rel(got_a, G.sym_adjoint(rs[c].astype(np.complex128), D)))
        want_n = float(G.frobenius_norms(want).sum())
        worst_n = max(worst_n, abs(nrm[c] - want_n) / want_n)
        # <E v, r>_F = <v, Eᴴr> with the device's results, in float64
        lhs = G.sym_inner(np.stack([u.cpu().numpy() for u in e[c]]).astype(np.complex128), rs[c].astype(np.complex128))
        rhs = np.vdot(vs[c].astype(np.complex128), got_a.astype(np.complex128))
        assert abs(lhs - rhs) <= 64 * eps * np.sqrt(n) * abs(lhs) + 64 * eps * n
    print(f"sym operator {Z} N={Ns} K={K}: adjoint {worst_a / eps:.2f} ε, norm {worst_n / eps:.2f} ε (bar {64 * np.sqrt(n):.0f} ε)")
    assert worst_a <= 8 * eps and worst_n <= 64 * eps * np.sqrt(n)
    with pytest.raises(ValueError):
        tv.sym_gradient(tuple(u[..., :-1].contiguous() for u in vd[0]) if K == 1 else tuple(tuple(u[..., :-1].contiguous() for u in comp) for comp in vd))
    with pytest.raises(ValueError):
        tv.sym_adjoint(one(vd) if D > 1 else one(tuple(comp + comp for comp in rd)))      # D arrays where S are expected
    tv.close()
    with pytest.raises(ValueError, match="closed"):
        tv.sym_norm(one(vd))


class _Coupled:
    """K = 2 coupled components from a system of tgv_cases: T_ab = c_ab · T with a real symmetric positive definite c, so the joint
    operator is c ⊗ G, its apply two applies of G, and λmax = λmax(c) · λmax(G).  (The construction of test_gpu_tv.py.)"""
    c = np.array([[1.0, 0.3], [0.3, 0.8]])

    def __init__(self, s):
        self.s, self.lmax = s, float(np.linalg.eigvalsh(self.c)[-1]) * s.lmax

    def apply(self, p):
        g = [self.s.apply(p[0]), self.s.apply(p[1])]
        return np.stack([self.c[a, 0] * g[0] + self.c[a, 1] * g[1] for a in range(2)])

    def operator(self, nufft, Z, path):
        Zc = GC.dt(Z)[1]
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


def _compare(tag, Z, xs, v, hist, ref, shares=False, stacked=False):
    """x, v and the three history columns against the reference; with ``shares`` the two branches of both projections on the reference."""
    x = np.stack(xs) if stacked else xs[0]
    got_v = np.moveaxis(v, 0, 1) if stacked else v[0]                                      # the reference's [D, K, ...]
    ex = R.rel(x, ref["x"])
    ev = R.rel(got_v, ref["v"]) if ref["v"].any() else float(np.abs(got_v).max())
    eh = [R.rel(hist[:, 0, k], ref["history"][:, k]) if ref["history"][:, k].any() else float(np.abs(hist[:, 0, k]).max()) for k in range(3)]
    sp, sr = float(ref["clipped_p"].mean()), float(ref["clipped_r"].mean())
    print(f"ten iterations {tag} {Z}: x {ex:.3e}, v {ev:.3e}, change {eh[0]:.3e}, Σ|∇x − v| {eh[1]:.3e}, Σ|Ev| {eh[2]:.3e} (bar {BAR[Z]:g}), "
          f"clipped p {sp:.2f} r {sr:.2f}")
    assert ex <= BAR[Z] and ev <= BAR[Z] and all(e <= BAR[Z] for e in eh)
    if shares:
        assert 0.1 <= sp <= 0.95 and 0.1 <= sr <= 0.95, (sp, sr)


# (alpha1, alpha0) / (0.1 max|b|) and lam / λmax: both projections clipping, r passing through, no p, no r, Tikhonov
WEIGHT_CASES = [(1.0, 0.5, 0.0), (1.0, 2.0, 0.0), (0.0, 0.5, 0.0), (1.0, 0.0, 0.0), (1.0, 0.5, 0.1)]


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("f1,f0,lam_rel", WEIGHT_CASES)
@pytest.mark.parametrize("Ns,path", GC.SOLVER_CASES)
def test_ten_iterations_weights(Ns, path, f1, f0, lam_rel, Z):
    from nufft_pkg import nufft
    _, Zc, _, _ = GC.dt(Z)
    s = GC.system(Ns)
    b = s.bs[0].astype(Zc)
    a1 = GC.tv_weight(s.bs[0])
    D, w1, w0, lam = len(Ns), f1 * a1, f0 * a1, lam_rel * s.lmax
    op = s.operator(nufft, Z, path, 1)
    sol = nufft.ToeplitzTGV(op, w1, alpha0=w0, step=GC.step(s, lam), lam=lam, maxiter=10, tol=0.0)
    xs, v, iters, status, hist = _solve(sol, [b])
    assert iters == (10,) and status == ("max_iter",) and hist.shape == (10, 1, 3) and v.shape == (1, D) + b.shape
    assert sol.info().iterations_enqueued == 10 and sol.sigma == 1.0 / (16 * D * GC.step(s, lam))
    ref = GC.reference(Ns, Z, w1, w0, lam, tol=0.0, max_iter=10)
    _compare(f"N={Ns} {path} a1={w1:.3g} a0={w0:.3g} lam={lam:.3g}", Z, xs, v, hist, ref, shares=(f1, f0, lam_rel) == WEIGHT_CASES[0])
    if f0 == 2.0:
        assert not ref["clipped_r"].any()                                                  # the pass-through branch alone
    if f1 == 0.0:
        assert not ref["p"].any()                                                          # p stays zero: x runs plain gradient descent
    if f0 == 0.0:
        assert not ref["r"].any()
    sol.close()
    assert nufft.ToeplitzTGV(op, a1, step=GC.step(s)).alpha0 == (2 * a1,)                    # alpha0=None: Knoll's ratio
    op.close()


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("kind", ["maps", "uncoupled", "coupled"])
@pytest.mark.parametrize("Ns,path", GC.SOLVER_CASES)
def test_ten_iterations_operators(Ns, path, kind, Z):
    from nufft_pkg import nufft
    _, Zc, _, _ = GC.dt(Z)
    s = GC.system(Ns)
    b, b2 = s.bs[0].astype(Zc), (0.5 * s.bs[1]).astype(Zc)
    a1 = GC.tv_weight(s.bs[0])
    if kind == "maps":
        # 2 coil maps: G = Σ_j conj(S_j) G0 S_j, with the maps as the operator holds them
        op = s.operator(nufft, Z, path, 1)
        maps = SR.smooth_maps(2, s.shape, seed=11).astype(Zc)
        m64 = maps.astype(np.complex128)
        apply = lambda u: sum(np.conj(m) * s.apply(m * np.asarray(u).astype(np.complex128)) for m in m64)      # noqa: E731
        step = GC.step(s) / float((np.abs(m64) ** 2).sum(axis=0).max())
        op.set_maps(_dev(maps))
        sol = nufft.ToeplitzTGV(op, a1, alpha0=0.5 * a1, step=step, maxiter=10, tol=0.0)
        xs, v, iters, status, hist = _solve(sol, [b])
        _compare(f"N={Ns} {path} 2 coil maps", Z, xs, v, hist, G.tgvpd(apply, b, a1, 0.5 * a1, step, tol=0.0, max_iter=10, dtype=Zc))
    elif kind == "uncoupled":
        # K = 2 with two different weight pairs: two independent solves
        op = s.operator(nufft, Z, path, 2)
        sol = nufft.ToeplitzTGV(op, (a1, 0.4 * a1), alpha0=(0.5 * a1, 0.6 * a1), step=GC.step(s), maxiter=10, tol=0.0)
        xs, v, iters, status, hist = _solve(sol, [b, b2])
        assert iters == (10, 10) and sol.alpha1 == (a1, 0.4 * a1) and sol.alpha0 == (0.5 * a1, 0.6 * a1)
        _compare(f"N={Ns} {path} K=2, component 1", Z, xs[:1], v[:1], hist[:, :1], GC.reference(Ns, Z, a1, 0.5 * a1, 0.0, tol=0.0, max_iter=10))
        _compare(f"N={Ns} {path} K=2, component 2", Z, xs[1:], v[1:], hist[:, 1:],
                 G.tgvpd(s.apply, b2, 0.4 * a1, 0.6 * a1, GC.step(s), tol=0.0, max_iter=10, dtype=Zc))
    else:
        # coupled K = 2: one system
        cp = _Coupled(s)
        op = cp.operator(nufft, Z, path)
        step = 1.0 / (1.05 * cp.lmax)
        sol = nufft.ToeplitzTGV(op, a1, alpha0=0.5 * a1, step=step, maxiter=10, tol=0.0)
        xs, v, iters, status, hist = _solve(sol, [b, b2])
        ref = G.tgvpd(cp.apply, np.stack([b, b2]), a1, 0.5 * a1, step, tol=0.0, max_iter=10, dtype=Zc, component_axis=0)
        assert iters == (10, 10) and status == ("max_iter", "max_iter")
        assert _same(hist[:, 0, :], hist[:, 1, :]) and sol.change[0] == sol.change[1]      # one system: one change, one pair of sums
        _compare(f"N={Ns} {path} coupled K=2", Z, xs, v, hist, ref, stacked=True)
    sol.close()
    op.close()


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,K", [((15, 9), 9), ((7, 6, 5), 2)])
def test_odd_rows_and_batches(Ns, K, Z):
    """Odd N_1: ComplexF32 rows are not 16-byte aligned, so the kernels run with one cell per lane; nine transforms need two launches
    per kernel (eight components travel as kernel arguments).  Analytic spectra as in fista_cases; every component has its own
    right-hand side and weights alpha1 = 0.1 (1 + c / 10) max|b_c|, alpha0 = 0.5 alpha1, and is compared with its own reference run."""
    from nufft_pkg import nufft
    _, Zc, _, _ = GC.dt(Z)
    s = FC.Analytic(Ns, seed=sum(Ns), nrhs=K)
    op = _analytic_operator(nufft, s, Zc, K)
    bs = [u.astype(Zc) for u in s.bs]
    a1 = tuple((1 + c / 10) * GC.tv_weight(b) for c, b in enumerate(bs))
    a0 = tuple(0.5 * w for w in a1)
    sol = nufft.ToeplitzTGV(op, a1, alpha0=a0, step=GC.step(s), maxiter=10, tol=0.0)
    xs, v, iters, status, hist = _solve(sol, bs)
    assert iters == (10,) * K and status == ("max_iter",) * K
    for c in range(K):
        ref = G.tgvpd(s.apply, bs[c], a1[c], a0[c], GC.step(s), tol=0.0, max_iter=10, dtype=Zc)
        _compare(f"N={Ns} component {c + 1} of {K}", Z, xs[c:c + 1], v[c:c + 1], hist[:, c:c + 1], ref)
    sol.close()
    op.close()


@pytest.mark.parametrize("Ns,path", GC.SOLVER_CASES[:2])
def test_converged_solve(Ns, path):
    from nufft_pkg import nufft
    s = GC.system(Ns)
    a1 = GC.tv_weight(s.bs[0])
    a0 = 0.5 * a1
    out = {}
    for Z, tol in (("c128", 1e-6), ("c64", 1e-4), ("c128", 1e-4)):
        Zc = GC.dt(Z)[1]
        b = s.bs[0].astype(Zc)
        op = s.operator(nufft, Z, path, 1)
        sol = nufft.ToeplitzTGV(op, a1, alpha0=a0, step=GC.step(s), maxiter=2000, tol=tol, check_every=8)
        xs, v, iters, status, hist = _solve(sol, [b])
        ref = GC.reference(Ns, Z, a1, a0, 0.0, tol=tol, max_iter=2000)
        print(f"converged {Z} N={Ns} {path} tol={tol:g}: {iters[0]} iterations (reference {ref['iterations']}), change {sol.change[0]:.4e}, "
              f"enqueued {sol.info().iterations_enqueued}")
        assert status == ("converged",) and ref["status"] == G.CONVERGED
        assert sol.change[0] <= tol and hist[iters[0] - 1, 0, 0] == sol.change[0] and hist.shape[0] == iters[0]
        assert sol.info().iterations_enqueued == -(-iters[0] // 8) * 8 < 2000          # stopped at the first look after the component froze
        out[(Z, tol)] = (xs[0], v[0], iters[0], ref)
        sol.close()
        op.close()
    x, v, it, ref = out[("c128", 1e-6)]
    h = ref["history"][:, 0]
    assert abs(h[-1] / 1e-6 - 1) > 1e-3 and abs(h[-2] / 1e-6 - 1) > 1e-3                   # the crossing is not within 0.1 % of tol
    assert it == ref["iterations"]
    own = G.optimality(s.apply, s.bs[0], ref["x"], ref["v"], ref["p"], ref["r"], a1, a0)
    got = G.optimality(s.apply, s.bs[0], x, v, ref["p"], ref["r"], a1, a0)
    names = ("r_x", "r_v", "e_1", "e_0", "g_1", "g_0")
    print(f"optimality N={Ns}: " + ", ".join(f"{n} {g:.3e} (reference {o:.3e})" for n, g, o in zip(names, got, own)))
    assert all(o <= 1.01 * w for o, w in zip(own, REACHED[Ns])), own                       # the recorded numbers are the reference's own
    assert all(g <= 10 * w for g, w in zip(got, REACHED[Ns])), got
    x32, _, it32, ref32 = out[("c64", 1e-4)]
    assert abs(it32 - ref32["iterations"]) <= 1
    e32 = R.rel(x32, out[("c128", 1e-4)][0])
    print(f"ComplexF32 against ComplexF64 at tol 1e-4, N={Ns}: {e32:.3e} (bar {BAR['c64']:g})")
    assert e32 <= BAR["c64"]


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns", [(24, 40), (8, 12, 20)])
def test_determinism_modes_and_graph(Ns, Z):
    """Analytic spectra; on the CPU the reference needs 58 / 52 iterations on (24, 40) and 31 / 46 on (8, 12, 20) for the two components
    at tol = 1e-3 in both element types."""
    from nufft_pkg import nufft
    _, Zc, _, _ = GC.dt(Z)
    s = FC.Analytic(Ns, seed=4 * sum(Ns))
    op = _analytic_operator(nufft, s, Zc, 2)
    bs = [s.bs[0].astype(Zc), (0.4 * s.bs[1]).astype(Zc)]
    a1 = (GC.tv_weight(bs[0]), GC.tv_weight(bs[1]))
    kw = dict(alpha0=tuple(0.5 * w for w in a1), step=GC.step(s), maxiter=160, tol=1e-3)
    a = nufft.ToeplitzTGV(op, a1, check_every=0, **kw)
    xa, va, ia, sa, ha = _solve(a, bs)
    print(f"modes {Z} N={Ns}: iterations {ia}")
    assert a.info().iterations_enqueued == 160 and sa == ("converged", "converged") and max(ia) < 160
    b = nufft.ToeplitzTGV(op, a1, check_every=8, **kw)
    xb, vb, ib, sb, hb = _solve(b, bs)
    assert b.info().iterations_enqueued == -(-max(ia) // 8) * 8 < 160
    assert ia == ib and sa == sb and _same(ha, hb) and np.array_equal(va, vb) and all(np.array_equal(u, w) for u, w in zip(xa, xb))
    x2, v2, i2, s2, h2 = _solve(a, bs)                                           # two runs
    assert i2 == ia and s2 == sa and _same(h2, ha) and np.array_equal(v2, va) and all(np.array_equal(u, w) for u, w in zip(xa, x2))
    if ia[0] != ia[1]:
        assert np.isnan(ha[min(ia):, int(np.argmin(ia))]).all()                  # a frozen component writes no history
    bd = tuple(_dev(u) for u in bs)
    out = tuple(torch.zeros_like(u) for u in bd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        a.solve(bd, out=out)
        field = a.field()                                                        # the copies are captured too
        with pytest.raises(ValueError):                                          # check_every > 0 synchronises: refused while capturing
            b.solve(bd, out=out)
    for _ in range(2):
        for o in out:
            o.fill_(7.0)
        for comp in field:
            for u in comp:
                u.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert a.iterations == ia and a.status == sa and _same(a.history().numpy(), ha)
        assert all(np.array_equal(o.cpu().numpy(), u) for o, u in zip(out, xa))
        assert np.array_equal(np.stack([np.stack([u.cpu().numpy() for u in comp]) for comp in field]), va)
    del graph
    a.close()
    b.close()
    op.close()


@pytest.mark.parametrize("Z", TYPES)
def test_frozen_and_broken_components(Z):
    """Analytic (16, 12), two components, tol = 1e-3: the reference needs 46 / 63 iterations.  A component frozen by its early stop is
    bit-equal to its own solve; a NaN in one cell of b[1] ends that component BREAKDOWN at iteration 1 and leaves component 0 as it was
    (the pattern of test_gpu_tv.py's test_breakdown_freezes_one_component)."""
    from nufft_pkg import nufft
    L, lib = nufft._lib, nufft.lib
    _, Zc, _, _ = GC.dt(Z)
    Ns = (16, 12)
    s = FC.Analytic(Ns, seed=4 * sum(Ns))
    op = _analytic_operator(nufft, s, Zc, 2)
    good = [s.bs[0].astype(Zc), (0.4 * s.bs[1]).astype(Zc)]
    zero = np.zeros_like(good[0])
    a1 = (GC.tv_weight(good[0]), GC.tv_weight(good[1]))
    a0 = tuple(0.5 * w for w in a1)
    sol = nufft.ToeplitzTGV(op, a1, alpha0=a0, step=GC.step(s), maxiter=400, tol=1e-3)
    xs, v, it, st, h = _solve(sol, good)
    x1, v1, it1, st1, h1 = _solve(sol, [good[0], zero])
    x2, v2, it2, st2, h2 = _solve(sol, [zero, good[1]])
    print(f"components {Z}: iterations {it}, alone {it1[0]}, {it2[1]}")
    assert st == ("converged", "converged") and abs(it[0] - it[1]) >= 3          # they stop at different iterations
    assert np.array_equal(xs[0], x1[0]) and np.array_equal(xs[1], x2[1])         # the early one is frozen: bit-equal to its own solve
    assert np.array_equal(v[0], v1[0]) and np.array_equal(v[1], v2[1])
    assert it[0] == it1[0] and it[1] == it2[1]
    assert _same(h[: it[0], 0], h1[: it[0], 0]) and _same(h[: it[1], 1], h2[: it[1], 1])
    assert it1[1] == 1 and st1[1] == "converged" and not x1[1].any() and not v1[1].any() and h1[0, 1, 0] == 0.0      # a zero right-hand side
    sol.close()
    bad = [good[0], good[1].copy()]
    bad[1][5, 7] = np.nan
    kw = dict(alpha0=a0, step=GC.step(s), maxiter=4, tol=0.0)
    fresh = nufft.ToeplitzTGV(op, a1, **kw)
    xg, vg, ig, sg, hg = _solve(fresh, good)
    assert ig == (4, 4) and sg == ("max_iter", "max_iter") and np.isfinite(hg).all()
    sol = nufft.ToeplitzTGV(op, a1, **kw)
    xb, vb, ib, sb, hb = _solve(sol, bad)
    print(f"breakdown {Z}: iterations {ib}, status {sb}, history of component 1 {hb[:, 1, 0]}")
    assert sb[1] == "breakdown" and ib[1] == 1 and np.isnan(hb[0, 1, 0]) and np.isnan(sol.change[1])
    assert sb[0] == sg[0] and ib[0] == ig[0] and _same(hb[:, 0], hg[:, 0])
    assert R.rel(xb[0], xg[0]) <= BAR[Z] and R.rel(vb[0], vg[0]) <= BAR[Z]
    full = (C.c_double * (4 * 2 * 3))()
    assert lib.nufft_tgv_history(sol._handle, full, len(full), op._stream()) == L.OK
    assert np.isnan(np.array(full).reshape(4, 2, 3)[1:, 1]).all()                  # the frozen component writes no later row
    x2, v2, i2, s2, h2 = _solve(sol, good)                                         # a second solve on the solver that broke down
    assert i2 == ig and s2 == sg and _same(h2, hg) and np.array_equal(v2, vg) and all(np.array_equal(u, w) for u, w in zip(x2, xg))
    sol.close()
    fresh.close()
    op.close()


@pytest.mark.parametrize("Z", TYPES)
def test_fftshift_orders_agree(Z):
    """Both operators commute with cyclic shifts: a plan with fftshift = True solves the same problem in the shifted storage order."""
    from nufft_pkg import nufft
    import test_gpu_cg
    _, Zc, bar, _ = GC.dt(Z)
    Ns = (48, 40)
    s = GC.system(Ns)
    shifted = test_gpu_cg._system(Ns, fftshift=True)
    assert np.array_equal(shifted.spec, s.spec)                                  # the same points and weights
    b = s.bs[0].astype(Zc)
    a1 = GC.tv_weight(s.bs[0])
    outs = []
    for sys_, rhs in ((s, b), (shifted, np.fft.fftshift(b))):
        op = sys_.operator(nufft, Z, "dense", 1)
        sol = nufft.ToeplitzTGV(op, a1, alpha0=0.5 * a1, step=GC.step(s), maxiter=10, tol=0.0)
        xs, v, _, _, hist = _solve(sol, [np.ascontiguousarray(rhs)])
        outs.append((xs[0], v[0], hist))
        sol.close()
        op.close()
    ex = R.rel(np.fft.ifftshift(outs[1][0]), outs[0][0])
    ev = R.rel(np.stack([np.fft.ifftshift(u) for u in outs[1][1]]), outs[0][1])
    eh = R.rel(outs[1][2], outs[0][2])
    print(f"fftshift {Z}: x {ex:.3e}, v {ev:.3e}, history {eh:.3e} (bar {bar:g})")
    assert ex <= bar and ev <= bar and eh <= bar                                 # the parity bar: 1e-12 / 1e-5


def test_lifetime_and_arguments():
    from nufft_pkg import nufft
    L, lib = nufft._lib, nufft.lib
    Ns = (48, 40)
    s = GC.system(Ns)
    plan = nufft.PlanNUFFT(np.complex128, Ns, backend=nufft.ROCBackend(0), ntransforms=2)
    op = nufft.ToeplitzOperator(plan)
    for kw in ({"maxiter": 0}, {"tol": -1.0}, {"lam": -1e-3}, {"step": 0.0}, {"step": float("nan")}, {"alpha1": -1.0}, {"alpha1": (0.1,)},
               {"alpha0": -1.0}, {"alpha0": (0.1, 0.2, 0.3)}, {"check_every": -1}, {"sigma": 0.0}, {"sigma": float("inf")}):
        with pytest.raises(ValueError):
            nufft.ToeplitzTGV(op, **{"alpha1": 0.1, "step": 1.0, **kw})
    with pytest.raises(ValueError):
        nufft.ToeplitzTGV(op, 0.1)                                                # step=None needs the spectrum for the power iteration
    sol = nufft.ToeplitzTGV(op, torch.tensor(0.125), step=0.4 / s.lmax, sigma=0.5, maxiter=5, tol=0.0)      # a 0-d tensor is a scalar
    assert sol.sigma == 0.5 and sol.alpha1 == (0.125, 0.125) and sol.alpha0 == (0.25, 0.25) and "ToeplitzTGV" in repr(sol)
    sol.set_weights(np.float32(0.25), (0.5, 0.125))
    assert sol.alpha1 == (0.25, 0.25) and sol.alpha0 == (0.5, 0.125)
    for bad in ((-1.0, None), (0.1, -1.0), (float("nan"), 0.1), ((0.1, 0.1, 0.1), None), (0.1, (0.1,))):
        with pytest.raises(ValueError):
            sol.set_weights(*bad)
    assert sol.alpha1 == (0.25, 0.25) and sol.alpha0 == (0.5, 0.125)              # a refused call changes nothing
    b = tuple(_dev(u) for u in s.bs[:2])
    with pytest.raises(ValueError):                                               # NUFFT_ERR_NO_POINTS: no spectrum yet
        sol.solve(b)
    op.set_spectrum(_dev(s.spec))
    x = tuple(torch.zeros_like(u) for u in b)
    with pytest.raises(ValueError):
        sol.solve(b, out=b)                                                       # out is b
    with pytest.raises(ValueError):
        sol.solve(b, out=(x[0], x[0]))
    with pytest.raises(nufft.DimensionMismatch):
        sol.solve(b[0])
    with pytest.raises(ValueError):
        sol.solve(tuple(u.to(torch.complex64) for u in b))
    st = op._stream()
    assert lib.nufft_tgv_get_result(sol._handle, None, None, None, 1, st) == L.ERR_INVALID_ARG      # capacity < ntransforms
    assert lib.nufft_tgv_history(sol._handle, (C.c_double * 4)(), 4, st) == L.ERR_INVALID_ARG
    assert lib.nufft_tgv_set_weights(sol._handle, (C.c_double * 2)(0.1, 0.1), (C.c_double * 2)(0.1, -1.0), 2) == L.ERR_INVALID_ARG
    assert lib.nufft_tgv_set_weights(sol._handle, (C.c_double * 2)(0.1, 0.1), (C.c_double * 2)(0.1, 0.1), 1) == L.ERR_INVALID_ARG
    assert lib.nufft_tgv_copy_field(sol._handle, None, st) == L.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert not x[0].any() and not x[1].any()                                      # refused before anything was enqueued
    sol.solve(b, out=x)
    again = sol.solve(b, x0=x, out=x)                                             # out is x0 is allowed
    torch.cuda.synchronize()
    assert all(u.data_ptr() == w.data_ptr() for u, w in zip(again, x))
    i = sol.info()
    pad = lambda n: (max(n, 16) + 255) // 256 * 256      # noqa: E731
    assert sol.iterations == (5, 5) and i.iterations_enqueued == 5 and i.ndim == 2
    assert i.array_bytes == (1 + 3 * 2 + 3) * 2 * pad(48 * 40 * 16)               # q, v, v̄, p, r: 1 + 3 D + S arrays per component
    assert i.array_bytes < i.workspace_bytes < i.array_bytes + (64 << 10)         # nothing else of that size
    v = sol.field()
    assert len(v) == 2 and len(v[0]) == 2 and v[0][0].shape == x[0].shape
    tvop = nufft.TotalVariation(op)
    e = tvop.sym_gradient(v)
    with pytest.raises(ValueError):                                               # an output overlapping an input
        nufft.plan._check(lib.nufft_tv_sym_gradient(tvop._handle, nufft.plan._ptr_table([v[0][0], e[0][1], e[0][2], e[1][0], e[1][1], e[1][2]]),
                                                    nufft.plan._ptr_table([u for comp in v for u in comp]), st))
    with pytest.raises(ValueError):
        nufft.plan._check(lib.nufft_tv_sym_adjoint(tvop._handle, nufft.plan._ptr_table([e[0][0], v[0][1], v[1][0], v[1][1]]),
                                                   nufft.plan._ptr_table([u for comp in e for u in comp]), st))
    plan.close()                                                                  # the solver outlives the plan
    sol.solve(b, out=x)
    torch.cuda.synchronize()
    assert sol.iterations == (5, 5)
    op.close()                                                                    # the library keeps a pointer to the operator
    for call in (lambda: sol.solve(b), sol.info, lambda: sol.iterations, sol.history, sol.field):
        with pytest.raises(ValueError, match="outlive"):
            call()
    sol.close()
    with pytest.raises(ValueError, match="closed"):
        sol.info()
