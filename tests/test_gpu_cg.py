"""Conjugate gradients on the Toeplitz normal operator on the GPU, against the numpy reference (cg_reference.py) run in
the same element type and against the exact dense matrix G[k, k'] = T[k − k'] (float64).

Operators get the exact spectrum, so the only error in G is the operator's own (parity bars 1e-12 ComplexF64 / 1e-5 ComplexF32); one
test builds from points.  Bars:
  * fixed iteration count: rel-L2 of x₅ and of the history <= 10 × the parity bar.  Errors of the apply enter each iterate multiplied
    by at most cond(G + λ); every such case asserts cond <= 7 on its own inputs.
  * converged solves: true residual ‖b − (G+λ)x‖/‖b‖ in float64 <= 2 rtol (the recursive residual is <= rtol; the drift between the
    two is of order ε · cond · iterations, far below rtol); iterations within ±1 of the reference (uniform points), ±(10 % + 1)
    (clustered points, cond 1e3, where two summation orders already differ by up to 3).
Point counts: uniform systems take Np >= 20 n points in 2-D (n unknowns) so that cond <= 7; (48,) takes 400 and (15, 9) 2000.  The
32³ operator is built from 2000 points: rank(G) <= 2000 < n, so it runs with λ = 0.2 λmax only (cond <= 7 again); λ = 0 is singular there.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import cg_reference as CG  # noqa: E402
import toeplitz_reference as R  # noqa: E402


def _dt(Z):
    return (np.float64, np.complex128, 1e-12, 1e-10) if Z == "c128" else (np.float32, np.complex64, 1e-5, 1e-4)


def _npoints(Ns):
    n = int(np.prod(Ns))
    return 400 if Ns == (48,) else 2000 if (len(Ns) == 3 or n <= 200) else 20 * n


def _dev(a, Zc=None):
    return torch.from_numpy(np.ascontiguousarray(a if Zc is None else a.astype(Zc))).cuda()


class System:
    """Points, exact spectrum, exact matrix (or the float64 FFT apply at 32³), λmax, right-hand sides, and an operator per request."""

    def __init__(self, Ns, fftshift=False, clustered=False, seed=0, nrhs=2):
        rng = np.random.default_rng(seed)
        self.Ns, self.fftshift, Np = Ns, fftshift, _npoints(Ns)
        if clustered:
            self.xs = [np.mod(np.pi + 0.3 * rng.standard_normal(Np), 2 * np.pi) for _ in Ns]
        else:
            self.xs = [rng.random(Np) * 2 * np.pi for _ in Ns]
        self.w = rng.random(Np) + 0.1
        self.spec = R.exact_spectrum(Ns, self.xs, self.w)
        self.shape = Ns[::-1]
        self.bs = [rng.standard_normal(self.shape) + 1j * rng.standard_normal(self.shape) for _ in range(nrhs)]
        if int(np.prod(Ns)) <= 2048:
            self.A = CG.dense_gram(Ns, self.xs, self.w, fftshift, spectrum=self.spec)
            ev = np.linalg.eigvalsh(self.A)
            self.lmax, self.lmin = float(ev[-1]), float(ev[0])
            self.apply = CG.matrix_apply(self.A, self.shape)
        else:
            self.A = None
            K = R.multiplier(Ns, self.spec).real
            self.apply = lambda p: R.apply(Ns, K, np.asarray(p).astype(np.complex128), fftshift)
            v = self.bs[0]
            for _ in range(30):                                  # power iteration: λmax from below, within a few per cent
                g = self.apply(v)
                self.lmax = float(np.linalg.norm(g) / np.linalg.norm(v))
                v = g / np.linalg.norm(g)
            self.lmin = 0.0

    def easy_rhs(self, k=6):
        """A right-hand side in the span of k eigenvectors of G: CG needs at most k iterations for it (needs the dense matrix)."""
        _, V = np.linalg.eigh(self.A)
        cols = V[:, :: max(1, V.shape[1] // k)][:, :k]
        return (cols @ np.arange(1, cols.shape[1] + 1)).reshape(self.shape)

    def cond(self, lam):
        return (self.lmax * (1.05 if self.A is None else 1.0) + lam) / (self.lmin + lam)

    def true_residual(self, lam, x, b):
        x, b = np.asarray(x).astype(np.complex128), np.asarray(b).astype(np.complex128)
        return float(np.linalg.norm((b - (self.apply(x) + lam * x)).ravel()) / np.linalg.norm(b.ravel()))

    def operator(self, nufft, Z, path, C=1, **kw):
        T, Zc, _, _ = _dt(Z)
        opts = {"NUFFT_TOEPLITZ_FUSED": 0} if path == "dense" else {}
        plan = nufft.PlanNUFFT(Zc, self.Ns, backend=nufft.ROCBackend(0), options=opts, fftshift=self.fftshift, ntransforms=C, **kw)
        op = nufft.ToeplitzOperator(plan)
        assert op.path == path, (self.Ns, path, op.path)
        op.set_spectrum(_dev(self.spec, Zc))
        plan.close()
        return op


_SYSTEMS = {}


def _system(Ns, fftshift=False, clustered=False):
    key = (Ns, fftshift, clustered)
    if key not in _SYSTEMS:
        _SYSTEMS[key] = System(Ns, fftshift, clustered, seed=4 * sum(Ns) + clustered)
    return _SYSTEMS[key]


def _solve(sol, bs, C, **kw):
    """solve + outcome, as numpy; bs: list of C host arrays."""
    bd = tuple(_dev(b) for b in bs)
    x = sol.solve(bd if C > 1 else bd[0], **kw)
    torch.cuda.synchronize()
    xs = [v.cpu().numpy() for v in (x if C > 1 else (x,))]
    return xs, sol.iterations, sol.status, sol.history().numpy()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# (Z, N, fftshift, path, ntransforms): both paths, both element types, fftshift on and off, ntransforms 1 and 2; (15, 9) in ComplexF32
# has an odd number of elements (the kernels' tail behind the last 16-byte pack)
CASES = [
    ("c128", (32, 32), False, "fused", 1), ("c64", (32, 32), True, "fused", 2),
    ("c128", (48, 40), True, "fused", 2), ("c64", (48, 40), False, "fused", 1),
    ("c128", (32, 32, 32), False, "fused", 1), ("c64", (32, 32, 32), True, "fused", 2),
    ("c128", (48,), False, "dense", 1), ("c64", (48,), True, "dense", 2),
    ("c128", (15, 9), True, "dense", 2), ("c64", (15, 9), False, "dense", 1),
]


def _lambdas(s):
    return (0.2 * s.lmax,) if s.A is None else (0.0, 1e-3 * s.lmax)


@pytest.mark.parametrize("Z,Ns,fftshift,path,C", CASES)
def test_fixed_iteration_count(Z, Ns, fftshift, path, C):
    from nufft_pkg import nufft
    T, Zc, bar, _ = _dt(Z)
    s = _system(Ns, fftshift)
    op = s.operator(nufft, Z, path, C)
    bs = [b.astype(Zc) for b in s.bs[:C]]
    for lam in _lambdas(s):
        assert s.cond(lam) <= 7, s.cond(lam)
        sol = nufft.ToeplitzCG(op, maxiter=5, rtol=0.0, lam=lam)
        xs, iters, status, hist = _solve(sol, bs, C)
        assert iters == (5,) * C and status == ("max_iter",) * C and hist.shape == (6, C)
        for c in range(C):
            ref = CG.cg(s.apply, bs[c], lam=lam, rtol=0.0, max_iter=5, dtype=Zc)
            ex, eh = R.rel(xs[c], ref["x"]), R.rel(hist[:, c], ref["history"])
            print(f"fixed 5 iterations {Z} N={Ns} shift={fftshift} {path} lam={lam:.3g} c={c}: x {ex:.3e}, history {eh:.3e} (bar {10 * bar:g})")
            assert ex <= 10 * bar and eh <= 10 * bar
        sol.close()


@pytest.mark.parametrize("Z,Ns,fftshift,path,C", CASES)
def test_converged_solve(Z, Ns, fftshift, path, C):
    from nufft_pkg import nufft
    T, Zc, _, rtol = _dt(Z)
    s = _system(Ns, fftshift)
    op = s.operator(nufft, Z, path, C)
    bs = [b.astype(Zc) for b in s.bs[:C]]
    for lam in _lambdas(s):
        sol = nufft.ToeplitzCG(op, maxiter=100, rtol=rtol, lam=lam)
        xs, iters, status, hist = _solve(sol, bs, C)
        assert status == ("converged",) * C
        for c in range(C):
            ref = CG.cg(s.apply, bs[c], lam=lam, rtol=rtol, max_iter=100, dtype=Zc)
            tr = s.true_residual(lam, xs[c], bs[c])
            print(f"converged {Z} N={Ns} shift={fftshift} {path} lam={lam:.3g} c={c}: {iters[c]} iterations (reference {ref['iterations']}), "
                  f"true residual / rtol {tr / rtol:.3f}, reported {sol.residual[c]:.3e}")
            assert tr <= 2 * rtol
            assert abs(iters[c] - ref["iterations"]) <= 1
            assert sol.residual[c] <= rtol * (1 + 1e-12) and hist[iters[c], c] == sol.residual[c]
        sol.close()


@pytest.mark.parametrize("Z,Ns,path,C,a,cond_bound", [("c128", (512, 512), "fused", 1, 0.2, 5.07), ("c64", (1024, 512), "dense", 2, 0.2, 5.07),
                                                      ("c64", (128, 64, 64), "fused", 2, 0.15, 6.14)])
def test_more_workgroups_than_threads(Z, Ns, path, C, a, cond_bound):
    """More rows of per-workgroup partials than threads in a workgroup (262144 packs per component: 512 workgroups), so the next kernel's
    fixed-order reduction takes its strided part (thread t adds rows t, t + 256, ...), for C = 2 in the [C][G][2] layout beyond one stride.

    The operator gets the analytic spectrum T[d] = Π_dim a^|d_dim|: the coefficients of a product of Poisson kernels, whose symbol
    Π (1 − a²) / (1 − 2a cos θ + a²) lies in [((1 − a) / (1 + a))^D, ((1 + a) / (1 − a))^D], so G is positive definite with
    cond <= 1.5^4 = 5.0625 in 2-D at a = 0.2.  Five iterations against the reference under the bars of test_fixed_iteration_count, and
    two solves of the same inputs equal bit for bit.  (1024, 512) runs the dense path: the fused passes stop at lines of 2N = 1024
    cells, and no fused 2-D ComplexF32 system has more than 256 workgroups.  (128, 64, 64) is the fused ComplexF32 system of the same
    size; a = 0.15 keeps its cond <= (1.15 / 0.85)^6 = 6.133 under the file's limit of 7 (0.2 would give 11.4 in 3-D)."""
    from nufft_pkg import nufft
    T, Zc, bar, _ = _dt(Z)
    D = len(Ns)
    cond = ((1 + a) / (1 - a)) ** (2 * D)
    assert cond <= cond_bound <= 7, cond
    spec = np.ones([2 * n for n in reversed(Ns)])
    for dim, n in enumerate(Ns):                                               # dimension dim is axis D − 1 − dim
        shape = [1] * D
        shape[D - 1 - dim] = 2 * n
        spec = spec * (a ** np.abs(np.asarray(R.modes(2 * n)).astype(np.float64))).reshape(shape)
    spec = spec.astype(np.complex128)
    plan = nufft.PlanNUFFT(Zc, Ns, backend=nufft.ROCBackend(0), ntransforms=C)
    op = nufft.ToeplitzOperator(plan)
    assert op.path == path, (Ns, path, op.path)
    op.set_spectrum(_dev(spec, Zc))
    plan.close()
    K = R.multiplier(Ns, spec).real
    apply = lambda p: R.apply(Ns, K, np.asarray(p).astype(np.complex128))     # noqa: E731
    rng = np.random.default_rng(4 * sum(Ns))
    bs = [(rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1])).astype(Zc) for _ in range(C)]
    sol = nufft.ToeplitzCG(op, maxiter=5, rtol=0.0, lam=0.0)
    assert sol.info().workgroups > 256, sol.info().workgroups
    xs, iters, status, hist = _solve(sol, bs, C)
    assert iters == (5,) * C and status == ("max_iter",) * C and hist.shape == (6, C)
    for c in range(C):
        ref = CG.cg(apply, bs[c], lam=0.0, rtol=0.0, max_iter=5, dtype=Zc)
        ex, eh = R.rel(xs[c], ref["x"]), R.rel(hist[:, c], ref["history"])
        print(f"{sol.info().workgroups} workgroups {Z} N={Ns} {path} c={c}: x {ex:.3e}, history {eh:.3e} (bar {10 * bar:g})")
        assert ex <= 10 * bar and eh <= 10 * bar
    xs2, iters2, status2, hist2 = _solve(sol, bs, C)
    assert iters2 == iters and status2 == status and _same(hist, hist2) and all(_same(u, v) for u, v in zip(xs, xs2))
    sol.close()
    op.close()


@pytest.mark.parametrize("Z,Ns", [("c128", (48,)), ("c64", (48,)), ("c128", (15, 9)), ("c64", (15, 9))])
def test_converged_solve_clustered_points(Z, Ns):
    from nufft_pkg import nufft
    T, Zc, _, rtol = _dt(Z)
    s = _system(Ns, False, clustered=True)
    lam = 1e-3 * s.lmax
    op = s.operator(nufft, Z, "dense")
    b = s.bs[0].astype(Zc)
    sol = nufft.ToeplitzCG(op, maxiter=100, rtol=rtol, lam=lam)
    xs, iters, status, _ = _solve(sol, [b], 1)
    ref = CG.cg(s.apply, b, lam=lam, rtol=rtol, max_iter=100, dtype=Zc)
    tr = s.true_residual(lam, xs[0], b)
    print(f"clustered {Z} N={Ns} cond {s.cond(lam):.3g}: {iters[0]} iterations (reference {ref['iterations']}), true residual / rtol {tr / rtol:.3f}")
    assert status == ("converged",) and tr <= 2 * rtol
    assert abs(iters[0] - ref["iterations"]) <= 0.1 * ref["iterations"] + 1


@pytest.mark.parametrize("Z,Ns,path,C", [("c128", (32, 32), "fused", 2), ("c64", (32, 32, 32), "fused", 1), ("c64", (15, 9), "dense", 2)])
def test_freeze_and_the_two_modes(Z, Ns, path, C):
    from nufft_pkg import nufft
    T, Zc, _, rtol = _dt(Z)
    s = _system(Ns)
    lam = _lambdas(s)[-1]
    op = s.operator(nufft, Z, path, C)
    bs = [b.astype(Zc) for b in s.bs[:C]]
    if C == 2:
        bs[1] = s.easy_rhs(3).astype(Zc)                                      # three eigenvectors: done after three iterations, then frozen
    a = nufft.ToeplitzCG(op, maxiter=100, rtol=rtol, lam=lam, check_every=0)
    xa, ia, sa, ha = _solve(a, bs, C)
    assert a.info().iterations_enqueued == 100
    b = nufft.ToeplitzCG(op, maxiter=100, rtol=rtol, lam=lam, check_every=3)
    xb, ib, sb, hb = _solve(b, bs, C)
    assert b.info().iterations_enqueued == -(-max(ia) // 3) * 3 < 100          # stopped at the first look after the last component froze
    assert ia == ib and sa == sb and _same(ha, hb) and all(np.array_equal(u, v) for u, v in zip(xa, xb))
    c = nufft.ToeplitzCG(op, maxiter=max(ia) + 1, rtol=rtol, lam=lam, check_every=0)
    xc, ic, _, hc = _solve(c, bs, C)
    assert ic == ia and _same(hc, ha) and all(np.array_equal(u, v) for u, v in zip(xa, xc))
    assert np.isnan(ha[min(ia) + 1:, int(np.argmin(ia))]).all()               # a frozen component writes no history
    if C == 2:
        assert ia[1] <= ia[0] - 3, ia


def test_components_are_independent():
    from nufft_pkg import nufft
    Z, Ns = "c128", (48, 40)
    T, Zc, _, rtol = _dt(Z)
    s = _system(Ns, True)
    op = s.operator(nufft, Z, "fused", 2)
    b1 = s.bs[0].astype(Zc)
    b2 = (1e3 * s.easy_rhs()).astype(Zc)   # another scale, and in the span of six eigenvectors: converges many iterations earlier
    zero = np.zeros_like(b1)
    sol = nufft.ToeplitzCG(op, maxiter=100, rtol=rtol)
    xs, it, st, h = _solve(sol, [b1, b2], 2)
    x1, it1, _, h1 = _solve(sol, [b1, zero], 2)
    x2, it2, _, h2 = _solve(sol, [zero, b2], 2)
    assert st == ("converged", "converged")
    assert np.array_equal(xs[0], x1[0]) and np.array_equal(xs[1], x2[1])
    assert it[0] == it1[0] and it[1] == it2[1] and it1[1] == 0 and it2[0] == 0
    assert _same(h[: it[0] + 1, 0], h1[:, 0]) and _same(h[: it[1] + 1, 1], h2[:, 1])
    assert not x1[1].any() and not x2[0].any()
    # a looser tolerance on a second solver: the same component stops several iterations earlier, and its iterates are a prefix
    loose = nufft.ToeplitzCG(op, maxiter=100, rtol=1e-6)
    _, itl, _, hl = _solve(loose, [b1, b2], 2)
    assert itl[0] <= it[0] - 3 and _same(hl[: itl[0] + 1, 0], h[: itl[0] + 1, 0])
    print(f"independent components: iterations {it}, alone {it1[0]}, {it2[1]}; rtol 1e-6: {itl}")
    assert it[1] <= it[0] - 3


def test_warm_start():
    from nufft_pkg import nufft
    # ComplexF64 only for the zero-iteration statement: the true residual of the converged x is the recursive one (<= 0.95 rtol in the
    # reference's probe) plus a drift of ε · cond · iterations = 1e-16 · 7 · 30 = 2e-14, far below the 5e-12 that is left; in ComplexF32
    # the drift (6e-8 · 7 · 13 = 5e-6) is of the order of what is left of rtol = 1e-4, so nothing can be asserted there.
    Z, Ns = "c128", (32, 32)
    T, Zc, _, rtol = _dt(Z)
    s = _system(Ns)
    op = s.operator(nufft, Z, "fused")
    b = s.bs[0].astype(Zc)
    sol = nufft.ToeplitzCG(op, maxiter=100, rtol=rtol)
    bd = _dev(b)
    x = sol.solve(bd)
    torch.cuda.synchronize()
    first, keep = sol.iterations[0], x.clone()
    again = sol.solve(bd, x0=x, out=x)
    torch.cuda.synchronize()
    assert again.data_ptr() == x.data_ptr() and sol.iterations == (0,) and sol.status == ("converged",)
    assert torch.equal(x, keep) and sol.history().shape == (1, 1)
    for Z2 in ("c128", "c64"):
        T2, Zc2, _, rtol2 = _dt(Z2)
        op2 = op if Z2 == Z else s.operator(nufft, Z2, "fused")
        # a random start of the solution's own size (the norm of the reference's cold solve).  The residual recursion starts from
        # r0 = b − (G + λ) x0, whose rounding error is ε ‖G‖ ‖x0‖: with ‖x0‖ = 1e4 ‖x‖ (unit normal entries here) that alone is
        # 6e-8 · 1e4 = 6 rtol of ‖b‖ in ComplexF32, in the numpy reference as well, and the drift argument behind the 2 rtol bar
        # (ε · cond · iterations relative to ‖b‖) does not cover such a start
        rng = np.random.default_rng(3)
        x0 = rng.standard_normal(s.shape) + 1j * rng.standard_normal(s.shape)
        xc = CG.cg(s.apply, b.astype(Zc2), lam=1e-3 * s.lmax, rtol=rtol2, max_iter=100, dtype=Zc2)["x"]
        x0 = (x0 * (np.linalg.norm(xc) / np.linalg.norm(x0))).astype(Zc2)
        sol2 = nufft.ToeplitzCG(op2, maxiter=100, rtol=rtol2, lam=1e-3 * s.lmax)
        x0d = _dev(x0)
        y = sol2.solve(_dev(b.astype(Zc2)), x0=x0d)
        torch.cuda.synchronize()
        assert y.data_ptr() != x0d.data_ptr() and np.array_equal(x0d.cpu().numpy(), x0)         # x0 is only read when out is not x0
        ref = CG.cg(s.apply, b.astype(Zc2), x0=x0, lam=1e-3 * s.lmax, rtol=rtol2, max_iter=100, dtype=Zc2)
        tr = s.true_residual(1e-3 * s.lmax, y.cpu().numpy(), b.astype(Zc2))
        print(f"warm start {Z2}: first solve {first} iterations; from a random x0 {sol2.iterations[0]} (reference {ref['iterations']}), true residual / rtol {tr / rtol2:.3f}")
        assert sol2.status == ("converged",) and tr <= 2 * rtol2 and abs(sol2.iterations[0] - ref["iterations"]) <= 1
        cold = sol2.solve(_dev(b.astype(Zc2)))
        torch.cuda.synchronize()
        assert R.rel(y.cpu().numpy(), cold.cpu().numpy()) <= 4 * rtol2 * s.cond(1e-3 * s.lmax)  # each within cond · 2 rtol of the one solution


@pytest.mark.parametrize("Z,Ns,path,C", [("c128", (32, 32, 32), "fused", 1), ("c64", (48, 40), "fused", 2), ("c128", (48,), "dense", 1)])
def test_graph_and_stream(Z, Ns, path, C):
    from nufft_pkg import nufft
    T, Zc, _, rtol = _dt(Z)
    s = _system(Ns)
    lam = _lambdas(s)[-1]
    op = s.operator(nufft, Z, path, C)
    bs = [b.astype(Zc) for b in s.bs[:C]]
    sol = nufft.ToeplitzCG(op, maxiter=40, rtol=rtol, lam=lam)
    x1, it1, st1, h1 = _solve(sol, bs, C)
    x2, it2, st2, h2 = _solve(sol, bs, C)
    assert it1 == it2 and st1 == st2 and _same(h1, h2) and all(np.array_equal(u, v) for u, v in zip(x1, x2))      # determinism
    bd = tuple(_dev(b) for b in bs)
    out = tuple(torch.zeros_like(b) for b in bd)
    checking = nufft.ToeplitzCG(op, maxiter=40, rtol=rtol, lam=lam, check_every=2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        sol.solve(bd if C > 1 else bd[0], out=out if C > 1 else out[0])
        with pytest.raises(ValueError):                         # check_every > 0 synchronises: refused while capturing
            checking.solve(bd if C > 1 else bd[0], out=out if C > 1 else out[0])
    for _ in range(2):
        for o in out:
            o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert sol.iterations == it1 and sol.status == st1 and _same(sol.history().numpy(), h1)
        assert all(np.array_equal(o.cpu().numpy(), v) for o, v in zip(out, x1))
    del graph


def test_zero_right_hand_side_and_singular_system():
    from nufft_pkg import nufft
    s = _system((15, 9))
    op = s.operator(nufft, "c128", "dense", 2)
    sol = nufft.ToeplitzCG(op, maxiter=10, rtol=0.0)
    zero = np.zeros(s.shape, dtype=np.complex128)
    xs, it, st, h = _solve(sol, [zero, s.bs[0]], 2)
    assert it[0] == 0 and st[0] == "converged" and not xs[0].any() and h[0, 0] == 0.0 and sol.residual[0] == 0.0
    assert it[1] == 10 and np.isnan(h[1:, 0]).all()
    for Z in ("c128", "c64"):
        T, Zc, _, rtol = _dt(Z)
        sing = _system((48,), False, clustered=True)
        assert sing.lmax / max(sing.lmin, 1e-300) > 1e12                      # numerically singular
        ops = sing.operator(nufft, Z, "dense")
        sol = nufft.ToeplitzCG(ops, maxiter=300, rtol=rtol, lam=0.0)
        xs, it, st, h = _solve(sol, [sing.bs[0].astype(Zc)], 1)
        print(f"singular system {Z}: status {st[0]} after {it[0]} iterations, last residual {sol.residual[0]:.3e}, max |x| {np.abs(xs[0]).max():.3e}")
        assert st[0] in ("breakdown", "max_iter") and np.isfinite(xs[0]).all() and np.isfinite(h[: it[0] + 1]).all()


def test_refusals():
    from nufft_pkg import nufft
    L, lib = nufft._lib, nufft.lib
    s = _system((32, 32))
    plan = nufft.PlanNUFFT(np.complex128, s.Ns, backend=nufft.ROCBackend(0), ntransforms=2)
    op = nufft.ToeplitzOperator(plan)
    for kw in ({"maxiter": 0}, {"rtol": -1.0}, {"lam": -1e-3}, {"rtol": float("nan")}, {"lam": float("inf")}, {"check_every": -1}):
        with pytest.raises(ValueError):
            nufft.ToeplitzCG(op, **kw)
    h = C.c_void_p()
    prm = L.NufftCgParams(struct_size=8, max_iter=5)                          # a layout older than any published one
    assert lib.nufft_cg_create(C.byref(h), op._handle, C.byref(prm)) == L.ERR_INVALID_ARG and not h.value
    sol = nufft.ToeplitzCG(op, maxiter=5)
    b = tuple(_dev(v) for v in s.bs[:2])
    with pytest.raises(ValueError):                                           # NUFFT_ERR_NO_POINTS: no spectrum yet
        sol.solve(b)
    op.set_spectrum(_dev(s.spec))
    x = tuple(torch.zeros_like(v) for v in b)
    st = op._stream()
    tab = lambda *t: (C.c_void_p * 2)(*[v if isinstance(v, int) else v.data_ptr() for v in t])      # noqa: E731
    assert lib.nufft_cg_solve(sol._handle, None, tab(*b), 0, st) == L.ERR_INVALID_ARG               # null table
    assert lib.nufft_cg_solve(sol._handle, tab(*x), None, 0, st) == L.ERR_INVALID_ARG
    assert lib.nufft_cg_solve(sol._handle, tab(x[0], 0), tab(*b), 0, st) == L.ERR_INVALID_ARG       # null vector
    assert lib.nufft_cg_solve(sol._handle, tab(b[0], x[1]), tab(*b), 0, st) == L.ERR_INVALID_ARG    # x[0] is b[0]
    assert lib.nufft_cg_solve(sol._handle, tab(b[1], x[1]), tab(*b), 0, st) == L.ERR_INVALID_ARG    # x[0] is b[1]
    assert lib.nufft_cg_solve(sol._handle, tab(x[0], x[0]), tab(*b), 0, st) == L.ERR_INVALID_ARG    # the two x are one array
    assert lib.nufft_cg_solve(sol._handle, tab(x[0].data_ptr() + 8, x[1]), tab(*b), 0, st) == L.ERR_INVALID_ARG   # not 16-byte aligned
    torch.cuda.synchronize()
    assert not x[0].any() and not x[1].any()                                  # refused before anything was enqueued
    with pytest.raises(ValueError):
        sol.solve(b, out=b)
    with pytest.raises(nufft.DimensionMismatch):
        sol.solve(b[0])
    with pytest.raises(ValueError):
        sol.solve(tuple(v.to(torch.complex64) for v in b))
    assert lib.nufft_cg_get_result(sol._handle, None, None, None, 1, st) == L.ERR_INVALID_ARG       # capacity < ntransforms
    assert lib.nufft_cg_history(sol._handle, (C.c_double * 4)(), 4, st) == L.ERR_INVALID_ARG
    sol.solve(b, out=x)                                                       # and the solver still works
    torch.cuda.synchronize()
    assert sol.iterations == (5, 5)
    op.set_spectrum(_dev(2 * s.spec))                                         # a new G between two solves: x halves
    y = sol.solve(b)
    torch.cuda.synchronize()
    assert R.rel(2 * y[0].cpu().numpy(), x[0].cpu().numpy()) <= 1e-12
    op.close()                                                                # the library keeps a pointer to the operator: the Python
    for call in (lambda: sol.solve(b), sol.info, lambda: sol.iterations, sol.history):      # layer refuses to follow it once it is gone
        with pytest.raises(ValueError, match="outlive"):
            call()
    sol.close()
    with pytest.raises(ValueError, match="closed"):
        sol.info()


def test_workspace_and_memory_return():
    from nufft_pkg import nufft
    Ns, Cn, maxiter = (32, 32, 32), 2, 50
    s = _system(Ns)
    op = s.operator(nufft, "c128", "fused", Cn)
    pad = lambda v: (max(v, 16) + 255) // 256 * 256      # noqa: E731
    torch.cuda.synchronize()
    nufft.ToeplitzCG(op, maxiter=maxiter).close()        # code objects loaded, the allocator warm
    free0 = torch.cuda.mem_get_info()[0]
    sol = nufft.ToeplitzCG(op, maxiter=maxiter)
    i = sol.info()
    n = int(np.prod(Ns))
    assert i.array_bytes == 3 * Cn * pad(n * 16)
    small = pad(Cn * i.workgroups * 3 * 8) + pad(Cn * (4 * 8 + 5 * 4)) + pad((maxiter + 1) * Cn * 8)
    assert i.workspace_bytes == i.array_bytes + small and small < 64 * 1024
    assert i.ntransforms == Cn and i.max_iter == maxiter and i.iterations_enqueued == -1 and i.workgroups >= 1
    b = tuple(_dev(v) for v in s.bs[:2])
    x = tuple(torch.empty_like(v) for v in b)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    sol.solve(b, out=x)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == held                                # solve allocates nothing through torch either
    sol.close()
    sol.close()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20)
    y = op.solve(b, maxiter=maxiter, rtol=1e-8, lam=0.2 * s.lmax)               # the one-shot convenience
    assert s.true_residual(0.2 * s.lmax, y[1].cpu().numpy(), s.bs[1]) <= 2e-8


def test_built_from_points():
    from nufft_pkg import nufft
    Z, Ns = "c128", (32, 32)
    T, Zc, _, rtol = _dt(Z)
    s = _system(Ns)
    plan = nufft.PlanNUFFT(Zc, Ns, m=8, backend=nufft.ROCBackend(0))
    op = nufft.ToeplitzOperator(plan)
    assert op.path == "fused"
    op.set_points(tuple(_dev(x) for x in s.xs), _dev(s.w))
    b = s.bs[0]
    u = s.bs[1]
    err = R.rel(op(_dev(u)).cpu().numpy(), R.exact_gram(Ns, s.xs, s.w, u))
    sol = nufft.ToeplitzCG(op, maxiter=100, rtol=rtol)
    xs, it, st, _ = _solve(sol, [b], 1)
    tr = s.true_residual(0.0, xs[0], b)
    print(f"built from points (m = 8): apply error {err:.3e}, {it[0]} iterations, true residual {tr:.3e} (bar {2 * rtol + 10 * err:.3e})")
    assert st == ("converged",) and tr <= 2 * rtol + 10 * err
