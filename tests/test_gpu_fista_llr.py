"""FISTA with the locally low-rank prior on the GPU against the numpy reference (llr_reference.fista_llr) run in the same
element type.  Systems: the coupled operators of test_gpu_subspace.py with exact spectra ((48, 40) on the fused path, (16, 16, 8) on the
dense one) and the uncoupled analytic system (64, 80) of fista_cases.py with three transforms.  Right-hand sides b = G x_true with
x_true locally low-rank plus noise (llr_cases.py); nuc = 0.2 × the largest block singular value of b; τ = 1 / (1.05² λmax) for the
coupled systems (λmax there is a power-iteration estimate from below), fista_cases.step otherwise.

Bars:
  * fixed 10 iterations, tol = 0, without and with shifts: rel-L2 of x and of both history columns <= 10 × the operator's parity bar
    (1e-12 / 1e-5): every step is non-expansive.  The ComplexF32 reference differs from its float64 run by 0.9e-7 ... 1.7e-7 in x on
    these systems; every case asserts that it stays below a third of the bar, and that the reference zeroes between 0.2 and 0.95 of the
    singular values in its tenth iteration (0.50 / 0.28 / 0.36 / 0.51 on the four coupled cases, 0.67 on the uncoupled one; these
    depend on the seeded inputs of llr_cases.py).  With nuc = 0 the result is also compared with plain accelerated gradient,
    fista_reference.fista with l1 = 0, within the same bar.
  * converged solves (tol = 1e-6, check_every = 4, maxiter = 2000): the float64 fixed-point residual
    ‖x − prox(x − τ ((G + μ) x − b))‖ / ‖x‖ of the GPU result <= 3 × the reference's own residual of the same case, taken from the
    reference at test time (1.0e-7 ... 1.9e-7); iterations <= 1.1 × the reference's + 2 (the reference: 321 / 325 at (48, 40) K = 2,
    640 / 673 at K = 4, 368 / 387 at (16, 16, 8) K = 3, ComplexF64 / ComplexF32; the GPU takes the same counts except 674 for 673).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import fista_cases as FC  # noqa: E402
import fista_reference as F  # noqa: E402
import llr_cases as LC  # noqa: E402
import llr_reference as L  # noqa: E402
import sense_reference as SR  # noqa: E402

TYPES = ["c128", "c64"]
PATH = {(48, 40): "fused", (16, 16, 8): "dense"}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _solve(sol, bs, **kw):
    x = sol.solve(tuple(_dev(b) for b in bs), **kw)
    torch.cuda.synchronize()
    return np.stack([v.cpu().numpy() for v in x]), sol.iterations, sol.status, sol.history().numpy()


class Case:
    """A coupled system with its right-hand side, weight and step; float64 throughout."""

    def __init__(self, Ns, K, block):
        import test_gpu_subspace as TS
        self.Ns, self.K, self.block = Ns, K, block
        self.sub = TS._system(Ns, K)
        self.apply = lambda p: np.stack(self.sub.apply([p[a] for a in range(K)]))
        self.b = self.apply(LC.low_rank_input(Ns, K))
        self.nuc = 0.2 * float(L.block_singular_values(self.b, block).max())
        self.step = 1.0 / (1.05 * 1.05 * self.sub.lmax)

    def operator(self, nufft, Z):
        op = self.sub.operator(nufft, Z, PATH[self.Ns])
        assert op.coupled
        return op


_CASES, _REFS = {}, {}


def _case(Ns, K, block):
    if (Ns, K, block) not in _CASES:
        _CASES[(Ns, K, block)] = Case(Ns, K, block)
    return _CASES[(Ns, K, block)]


def _reference(c, Z, high=False, nuc=None, **kw):
    key = (c.Ns, c.K, c.block, Z, high, nuc, tuple(sorted(kw.items())))
    if key not in _REFS:
        Zc = LC.CTYPE[Z]
        _REFS[key] = L.fista_llr(c.apply, c.b.astype(Zc), c.block, c.nuc if nuc is None else nuc, c.step,
                                 dtype=np.complex128 if high else Zc, **kw)
    return _REFS[key]


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,K,block", LC.SOLVER_CASES)
def test_fixed_iteration_count(Ns, K, block, Z):
    from nufft_pkg import nufft
    bar = FC.dt(Z)[2]
    c = _case(Ns, K, block)
    op = c.operator(nufft, Z)
    bs = list(c.b.astype(LC.CTYPE[Z]))
    for shifts, nuc in ((False, c.nuc), (True, c.nuc), (False, 0.0)):
        kw = dict(tol=0.0, max_iter=10, shifts=shifts, seed=11)
        sol = nufft.ToeplitzFISTA(op, prior="llr", block=block, nuc=nuc, shifts=shifts, seed=11, step=c.step, maxiter=10, tol=0.0)
        x, iters, status, hist = _solve(sol, bs)
        assert iters == (10,) * K and status == ("max_iter",) * K and hist.shape == (10, K, 2) and sol.info().iterations_enqueued == 10
        ref, high = _reference(c, Z, nuc=nuc, **kw), _reference(c, Z, high=True, nuc=nuc, **kw)
        own = max(LC.rel(ref["x"], high["x"]), LC.rel(ref["history"][:, 0], high["history"][:, 0]))
        ex, ec = LC.rel(x, ref["x"]), LC.rel(hist[:, 0, 0], ref["history"][:, 0])
        en = LC.rel(hist[:, 0, 1], ref["history"][:, 1])
        print(f"fixed 10 iterations {Z} N={Ns} K={K} block={block} shifts={shifts} nuc={nuc:.3g}: x {ex:.3e}, change {ec:.3e}, nuclear norm {en:.3e} "
              f"(bar {10 * bar:g}; reference vs float64 {own:.1e}), zero share {ref['zero_fraction']:.2f}")
        assert own <= 10 * bar / 3, own
        assert ex <= 10 * bar and ec <= 10 * bar and en <= 10 * bar
        if nuc > 0:
            assert 0.2 <= ref["zero_fraction"] <= 0.95, ref["zero_fraction"]
        else:                                                                   # nuc = 0: plain accelerated gradient, here from the
            assert ref["zero_fraction"] == 0.0                                  # wavelet reference with l1 = 0 (no SVD, no blocks)
            plain = F.fista(c.apply, np.stack(bs), "haar", 1, 0.0, c.step, tol=0.0, max_iter=10, dtype=LC.CTYPE[Z], component_axis=0)
            ep = LC.rel(x, plain["x"])
            print(f"    against plain accelerated gradient: x {ep:.3e}")
            assert ep <= 10 * bar and LC.rel(hist[:, 0, 0], plain["history"][:, 0]) <= 10 * bar
        for a in range(1, K):                                                   # one system
            assert _same(hist[:, a], hist[:, 0])
        sol.close()
    op.close()


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,K,block", LC.SOLVER_CASES[:3])
def test_converged_solve(Ns, K, block, Z):
    from nufft_pkg import nufft
    c = _case(Ns, K, block)
    op = c.operator(nufft, Z)
    bs = list(c.b.astype(LC.CTYPE[Z]))
    sol = nufft.ToeplitzFISTA(op, prior="llr", block=block, nuc=c.nuc, step=c.step, maxiter=2000, tol=1e-6, check_every=4)
    x, iters, status, hist = _solve(sol, bs)
    ref = _reference(c, Z, tol=1e-6, max_iter=2000)
    b64 = np.stack(bs).astype(np.complex128)
    res = L.fixed_point_residual(c.apply, b64, x, block, c.nuc, c.step)
    res_ref = L.fixed_point_residual(c.apply, b64, ref["x"], block, c.nuc, c.step)
    print(f"converged {Z} N={Ns} K={K} block={block}: {iters[0]} iterations (reference {ref['iterations']}), fixed-point residual {res:.3e} "
          f"(reference {res_ref:.3e}), change {sol.change[0]:.3e}, enqueued {sol.info().iterations_enqueued}")
    assert status == ("converged",) * K and ref["status"] == L.CONVERGED
    assert len(set(iters)) == 1 and len(set(sol.change)) == 1
    assert res <= 3 * res_ref
    assert iters[0] <= 1.1 * ref["iterations"] + 2
    assert sol.change[0] <= 1e-6 and hist[iters[0] - 1, 0, 0] == sol.change[0] and hist.shape[0] == iters[0]
    assert sol.info().iterations_enqueued == -(-iters[0] // 4) * 4 < 2000
    want_nuc = L.prox(x, block, 0.0)[1]
    assert abs(hist[iters[0] - 1, 0, 1] - want_nuc) <= 1e-4 * want_nuc
    sol.close()
    op.close()


def _uncoupled(nufft, Z):
    Ns, K, block = (64, 80), 3, (16, 4)
    s = FC.system(Ns)
    op = s.operator(nufft, Z, FC.PATHS[Ns], K)
    assert not op.coupled
    apply = lambda p: np.stack([s.apply(p[a]) for a in range(K)])      # noqa: E731
    b = apply(LC.low_rank_input(Ns, K))
    return s, op, apply, b, block, 0.2 * float(L.block_singular_values(b, block).max()), FC.step(s)


@pytest.mark.parametrize("Z", TYPES)
def test_one_system_on_an_uncoupled_operator(Z):
    from nufft_pkg import nufft
    bar, Zc = FC.dt(Z)[2], LC.CTYPE[Z]
    s, op, apply, b, block, nuc, step = _uncoupled(nufft, Z)
    bs = [(v * w).astype(Zc) for v, w in zip(b, (1.0, 0.3, 0.05))]            # per-component solvers would stop at different iterations
    sol = nufft.ToeplitzFISTA(op, prior="llr", block=block, nuc=nuc, step=step, maxiter=10, tol=0.0)
    x, iters, status, hist = _solve(sol, bs)
    ref = L.fista_llr(apply, np.stack(bs), block, nuc, step, tol=0.0, max_iter=10, dtype=Zc)
    ex, eh = LC.rel(x, ref["x"]), LC.rel(hist[:, 0, :], ref["history"])
    print(f"uncoupled K=3 {Z}: x {ex:.3e}, history {eh:.3e} (bar {10 * bar:g}), zero share {ref['zero_fraction']:.2f}")
    assert ex <= 10 * bar and eh <= 10 * bar and 0.2 <= ref["zero_fraction"] <= 0.95
    assert _same(hist[:, 1], hist[:, 0]) and _same(hist[:, 2], hist[:, 0]) and len(set(sol.change)) == 1
    loose = nufft.ToeplitzFISTA(op, prior="llr", block=block, nuc=nuc, step=step, maxiter=400, tol=1e-3, check_every=5)
    x, iters, status, hist = _solve(loose, bs)
    assert status == ("converged",) * 3 and len(set(iters)) == 1 and iters[0] < 400 and len(set(loose.change)) == 1
    assert _same(hist[:, 1], hist[:, 0]) and _same(hist[:, 2], hist[:, 0])
    zero = [np.zeros_like(v) for v in bs]                                       # a zero right-hand side
    x, iters, status, hist = _solve(loose, zero)
    assert iters == (1, 1, 1) and status == ("converged",) * 3 and not x.any() and hist[0, 0, 0] == 0.0 and hist[0, 0, 1] == 0.0


@pytest.mark.parametrize("Z", TYPES)
def test_zero_right_hand_side_coupled(Z):
    from nufft_pkg import nufft
    c = _case(*LC.SOLVER_CASES[0])
    op = c.operator(nufft, Z)
    sol = nufft.ToeplitzFISTA(op, prior="llr", block=c.block, nuc=c.nuc, step=c.step, maxiter=50, tol=1e-6)
    x, iters, status, hist = _solve(sol, [np.zeros(c.b.shape[1:], dtype=LC.CTYPE[Z])] * c.K)
    assert iters == (1,) * c.K and status == ("converged",) * c.K and not x.any() and sol.change == (0.0,) * c.K


@pytest.mark.parametrize("shifts", [False, True])
@pytest.mark.parametrize("Z,case", [("c64", 1), ("c128", 2)])
def test_determinism_modes_and_graph(Z, case, shifts):
    from nufft_pkg import nufft
    c = _case(*LC.SOLVER_CASES[case])
    op = c.operator(nufft, Z)
    bs = list(c.b.astype(LC.CTYPE[Z]))
    kw = dict(prior="llr", block=c.block, nuc=c.nuc, shifts=shifts, seed=3, step=c.step, maxiter=120, tol=0.0 if shifts else 2e-3)
    a = nufft.ToeplitzFISTA(op, check_every=0, **kw)
    xa, ia, sa, ha = _solve(a, bs)
    assert a.info().iterations_enqueued == 120
    b = nufft.ToeplitzFISTA(op, check_every=3, **kw)
    xb, ib, sb, hb = _solve(b, bs)
    if shifts:
        assert sa == ("max_iter",) * c.K and ia == (120,) * c.K
    else:
        assert sa == ("converged",) * c.K and ia[0] < 120 and b.info().iterations_enqueued == -(-ia[0] // 3) * 3 < 120
    assert ia == ib and sa == sb and _same(ha, hb) and np.array_equal(xa, xb)
    x2, i2, s2, h2 = _solve(a, bs)                                               # two runs
    assert i2 == ia and s2 == sa and _same(h2, ha) and np.array_equal(xa, x2)
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
        assert np.array_equal(np.stack([o.cpu().numpy() for o in out]), xa)
    del graph


@pytest.mark.parametrize("Z", TYPES)
def test_with_coil_maps(Z):
    from nufft_pkg import nufft
    import test_gpu_cg
    bar, Zc = FC.dt(Z)[2], LC.CTYPE[Z]
    Ns, K, block = (48, 40), 2, (4, 4)
    s = test_gpu_cg._system(Ns)
    maps = SR.smooth_maps(2, s.shape, seed=11).astype(Zc)
    A = SR.dense_sense_gram(s.A, maps.astype(np.complex128))                    # the maps as the operator holds them
    lmax = float(np.linalg.eigvalsh(A)[-1])
    apply = lambda p: np.stack([(A @ np.asarray(v).astype(np.complex128).ravel()).reshape(s.shape) for v in p])      # noqa: E731
    op = s.operator(nufft, Z, "dense", K)
    op.set_maps(_dev(maps))
    b = apply(LC.low_rank_input(Ns, K)).astype(Zc)
    nuc, step = 0.2 * float(L.block_singular_values(b, block).max()), 1.0 / (1.05 * lmax)
    sol = nufft.ToeplitzFISTA(op, prior="llr", block=block, nuc=nuc, step=step, maxiter=10, tol=0.0)
    x, iters, status, hist = _solve(sol, list(b))
    ref = L.fista_llr(apply, b, block, nuc, step, tol=0.0, max_iter=10, dtype=Zc)
    ex, eh = LC.rel(x, ref["x"]), LC.rel(hist[:, 0, :], ref["history"])
    print(f"2 coil maps {Z}: x {ex:.3e}, history {eh:.3e} (bar {10 * bar:g}), zero share {ref['zero_fraction']:.2f}")
    assert iters == (10, 10) and ex <= 10 * bar and eh <= 10 * bar and 0.2 <= ref["zero_fraction"] <= 0.95


def test_arguments_and_lifetime():
    from nufft_pkg import nufft
    L_, lib = nufft._lib, nufft.lib
    Ns, K = (48, 40), 2
    s = FC.system(Ns)
    plan = nufft.PlanNUFFT(np.complex128, Ns, backend=nufft.ROCBackend(0), ntransforms=K)
    op = nufft.ToeplitzOperator(plan)
    for kw in ({"wavelet": "db2"}, {"levels": 3}, {"l1": 0.1}, {"block": 3}, {"block": (4, 16)}, {"nuc": -1.0}, {"nuc": float("nan")},
               {"seed": -1}, {"maxiter": 0}, {"tol": -1.0}, {"step": 0.0}, {"check_every": -1}):
        with pytest.raises(ValueError):
            nufft.ToeplitzFISTA(op, **{"prior": "llr", "step": 1.0, **kw})
    for kw in ({"block": 4}, {"nuc": 0.1}, {"shifts": True}, {"seed": 1}, {"shifts": False}):
        with pytest.raises(ValueError):
            nufft.ToeplitzFISTA(op, step=1.0, **kw)
    with pytest.raises(ValueError):
        nufft.ToeplitzFISTA(op, prior="tv", step=1.0)
    with pytest.raises(ValueError):
        nufft.ToeplitzFISTA(op, prior="llr")                                      # step=None needs the spectrum
    wav = nufft.ToeplitzFISTA(op, step=0.5)                                       # no prior arguments: the wavelet solver, as before
    wi = wav.info()
    pad = lambda v: (max(v, 16) + 255) // 256 * 256      # noqa: E731
    assert wav.prior == "wavelet" and (wav.wavelet, wav.levels, wav.l1) == ("db2", 3, (0.0, 0.0))
    assert (wi.wavelet, wi.levels, wi.max_iter, wi.check_every, wi.tol, wi.array_bytes) == (L_.WAVELET_DB2, 3, 100, 0, 1e-4, 3 * K * pad(48 * 40 * 16))
    sol = nufft.ToeplitzFISTA(op, prior="llr", block=(4, 8), nuc=0.1, step=0.4 / s.lmax, maxiter=5, tol=0.0)
    assert "locally low-rank" in repr(sol) and sol.block == (4, 8)
    with pytest.raises(ValueError):
        wav.set_nuc(0.1)
    with pytest.raises(ValueError):
        sol.set_l1(0.1)
    assert lib.nufft_fista_set_nuc(wav._handle, 0.1) == L_.ERR_INVALID_ARG
    assert lib.nufft_fista_set_l1(sol._handle, (nufft._lib.C.c_double * 2)(0.1, 0.1), 2) == L_.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        sol.set_nuc(-1.0)
    sol.set_nuc(0.2)
    wav.set_l1(0.3)
    i = sol.info()
    assert i.array_bytes == 2 * K * pad(48 * 40 * 16) and (i.wavelet, i.levels) == (0, 0)
    assert i.array_bytes < i.workspace_bytes < i.array_bytes + (64 << 10)
    b = tuple(_dev(v) for v in s.bs[:2])
    with pytest.raises(ValueError):                                               # no spectrum yet
        sol.solve(b)
    op.set_spectrum(_dev(s.spec))
    x = tuple(torch.zeros_like(v) for v in b)
    with pytest.raises(ValueError):
        sol.solve(b, out=b)
    with pytest.raises(nufft.DimensionMismatch):
        sol.solve(b[0])
    sol.solve(b, out=x)
    torch.cuda.synchronize()
    assert sol.iterations == (5, 5) and sol.info().iterations_enqueued == 5
    op.set_spectrum(_dev(2 * s.spec))                                             # a new G between two solves is allowed
    sol.solve(b, out=x)
    torch.cuda.synchronize()
    assert sol.iterations == (5, 5)
    auto = nufft.ToeplitzFISTA(op, prior="llr", block=4, nuc=0.1, maxiter=5)      # step=None: from the power iteration
    assert 0.8 / (2 * s.lmax) <= auto.step <= 1.0 / (1.05 * 0.9 * 2 * s.lmax)
    op.close()                                                                    # the library keeps a pointer to the operator
    for call in (lambda: sol.solve(b), sol.info, lambda: sol.iterations, sol.history):
        with pytest.raises(ValueError, match="outlive"):
            call()
    sol.close()
    with pytest.raises(ValueError, match="closed"):
        sol.info()


@pytest.mark.parametrize("Z", TYPES)
def test_breakdown_freezes_the_system(Z):
    """A NaN in one cell of b[1]: the frames are one system, so the reference's rule (llr_reference.fista_llr: a change that is not finite is
    BREAKDOWN, and the iteration that found it is the last) holds for every frame.  Then the same solver on finite data: the start kernel's
    reset leaves nothing behind."""
    from nufft_pkg import nufft
    Ns, K, block = (16, 12), 3, (4, 4)
    s = FC.Analytic(Ns, seed=4 * sum(Ns))
    Zc = LC.CTYPE[Z]
    plan = nufft.PlanNUFFT(Zc, Ns, backend=nufft.ROCBackend(0), ntransforms=K)
    op = nufft.ToeplitzOperator(plan)
    op.set_spectrum(_dev(s.spec.astype(Zc)))
    plan.close()
    good = np.stack([s.apply(v) for v in LC.low_rank_input(Ns, K)]).astype(Zc)
    kw = dict(prior="llr", block=block, nuc=0.2 * float(L.block_singular_values(good, block).max()), step=FC.step(s), maxiter=4, tol=0.0)
    bad = good.copy()
    bad[1, 5, 7] = np.nan
    fresh = nufft.ToeplitzFISTA(op, **kw)
    xg, ig, sg, hg = _solve(fresh, good)
    assert ig == (4,) * 3 and sg == ("max_iter",) * 3 and np.isfinite(hg).all()
    sol = nufft.ToeplitzFISTA(op, **kw)
    _, ib, sb, hb = _solve(sol, bad)
    print(f"breakdown {Z}: iterations {ib}, status {sb}, history {hb.tolist()}")
    assert sb == ("breakdown",) * 3 and ib == (1,) * 3 and np.isnan(sol.change).all() and np.isnan(hb[0, :, 0]).all()
    full = (C.c_double * (4 * 3 * 2))()
    assert nufft.lib.nufft_fista_history(sol._handle, full, len(full), op._stream()) == nufft._lib.OK
    assert np.isnan(np.array(full).reshape(4, -1)[1:]).all()                       # the frozen system writes no later row
    x2, i2, s2, h2 = _solve(sol, good)                                      # a second solve on the solver that broke down
    assert i2 == ig and s2 == sg and _same(h2, hg) and np.array_equal(x2, xg)
    sol.close()
    fresh.close()
    op.close()
