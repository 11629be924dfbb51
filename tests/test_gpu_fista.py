"""FISTA with an l1-wavelet prior on the GPU, against the numpy reference (fista_reference.py) run in the same element
type.  Systems, l1 weights and cached references: fista_cases.py.  Operators get the exact spectrum, so the only error in G is the
operator's own (parity bars 1e-12 ComplexF64 / 1e-5 ComplexF32).

Bars:
  * fixed 10 iterations: rel-L2 of x and of both history columns <= 10 × the parity bar (every step of the iteration is non-expansive
    for τ <= 1 / λmax).  On the CPU the ComplexF32 reference differs from its float64 run by 2e-7 ... 1.2e-6 in x on these cases, far
    below a third of the bar (3.3e-5), so no case needs its own bar; every case asserts that.
  * converged solves (tol = 1e-6, check_every = 4): the float64 KKT residual of the GPU result relative to l1 <= 1e-3 (ComplexF32) and
    <= 1e-5 (ComplexF64).  The reference itself meets these on (48, 40) (4.2e-6 / 6.1e-6 in ComplexF64, <= 2.6e-5 in ComplexF32) and
    (64, 80) (4.3e-6 / 4.9e-6, <= 9.2e-5).  On (16, 16, 8), whose G has rank <= 2000 < 2048, the ComplexF64 reference stops at 3.52e-5
    (haar) and 1.13e-4 (db2): the bar there is 3 × those, 1.06e-4 and 3.4e-4 (ComplexF32: 1.7e-4 and 1.1e-4, inside 1e-3).
    Iterations <= 1.1 × the reference's + 2.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import fista_cases as FC  # noqa: E402
import fista_reference as F  # noqa: E402
import sense_reference as SR  # noqa: E402
import toeplitz_reference as R  # noqa: E402
import wavelet_reference as W  # noqa: E402

WAVELETS = ["haar", "db2"]
TYPES = ["c128", "c64"]
KKT_BAR = {"c128": 1e-5, "c64": 1e-3}
KKT_BAR_SINGULAR = {("c128", "haar"): 3 * 3.52e-5, ("c128", "db2"): 3 * 1.13e-4}        # (16, 16, 8): 3 × the reference's own residual


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


def _kkt(s, b, x, wavelet, levels, l1, Z, lam=0.0):
    c = W.forward(np.asarray(x).astype(np.complex128), wavelet, levels)
    return F.kkt_residual(s.apply, b, x, wavelet, levels, l1, lam=lam, zero_tol=(1e-12 if Z == "c128" else 1e-5) * np.abs(c).max())


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("wavelet", WAVELETS)
@pytest.mark.parametrize("Ns,levels,path", FC.SOLVER_CASES)
def test_fixed_iteration_count(Ns, levels, path, wavelet, Z):
    from nufft_pkg import nufft
    _, Zc, bar, _ = FC.dt(Z)
    s = FC.system(Ns)
    op = s.operator(nufft, Z, path, 1)
    b = s.bs[0].astype(Zc)
    l1 = FC.l1_weight(Ns, wavelet, s.bs[0])
    for weight, lam in ((l1, 0.0), (0.0, 0.0), (l1, 0.1 * s.lmax)):
        sol = nufft.ToeplitzFISTA(op, wavelet=wavelet, levels=levels, l1=weight, step=FC.step(s, lam), lam=lam, maxiter=10, tol=0.0)
        xs, iters, status, hist = _solve(sol, [b])
        assert iters == (10,) and status == ("max_iter",) and hist.shape == (10, 1, 2)
        assert sol.info().iterations_enqueued == 10
        ref = FC.reference(Ns, Z, wavelet, weight, lam, tol=0.0, max_iter=10)
        high = FC.reference(Ns, Z, wavelet, weight, lam, high=True, tol=0.0, max_iter=10)
        own = max(R.rel(ref["x"], high["x"]), R.rel(ref["history"][:, 0], high["history"][:, 0]))
        assert own <= 10 * bar / 3, own                                        # the reference in this element type is itself well inside the bar
        ex, ec = R.rel(xs[0], ref["x"]), R.rel(hist[:, 0, 0], ref["history"][:, 0])
        el = R.rel(hist[:, 0, 1], ref["history"][:, 1])
        print(f"fixed 10 iterations {wavelet} {Z} N={Ns} {path} l1={weight:.3g} lam={lam:.3g}: x {ex:.3e}, change {ec:.3e}, l1 norm {el:.3e} "
              f"(bar {10 * bar:g}; reference vs float64 {own:.1e}), zero details {ref['zero_fraction']:.2f}")
        assert ex <= 10 * bar and ec <= 10 * bar and el <= 10 * bar
        if weight > 0 and lam == 0.0:
            assert 0.2 <= ref["zero_fraction"] <= 0.95, ref["zero_fraction"]    # the threshold is active
        if weight == 0.0:
            assert ref["zero_fraction"] < 0.01                                  # plain accelerated gradient
        sol.close()
    op.close()


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("wavelet", WAVELETS)
@pytest.mark.parametrize("Ns,levels,path", FC.SOLVER_CASES[:3])
def test_converged_solve(Ns, levels, path, wavelet, Z):
    from nufft_pkg import nufft
    _, Zc, _, _ = FC.dt(Z)
    s = FC.system(Ns)
    op = s.operator(nufft, Z, path, 1)
    b = s.bs[0].astype(Zc)
    l1 = FC.l1_weight(Ns, wavelet, s.bs[0])
    sol = nufft.ToeplitzFISTA(op, wavelet=wavelet, levels=levels, l1=l1, step=FC.step(s), maxiter=2000, tol=1e-6, check_every=4)
    xs, iters, status, hist = _solve(sol, [b])
    ref = FC.reference(Ns, Z, wavelet, l1, 0.0, tol=1e-6, max_iter=2000)
    res = _kkt(s, b, xs[0], wavelet, levels, l1, Z)
    bar = KKT_BAR_SINGULAR.get((Z, wavelet), KKT_BAR[Z]) if Ns == (16, 16, 8) else KKT_BAR[Z]
    print(f"converged {wavelet} {Z} N={Ns} {path}: {iters[0]} iterations (reference {ref['iterations']}), KKT residual / l1 {res:.3e} (bar {bar:g}), "
          f"change {sol.change[0]:.3e}, enqueued {sol.info().iterations_enqueued}")
    assert status == ("converged",) and ref["status"] == F.CONVERGED
    assert res <= bar
    assert iters[0] <= 1.1 * ref["iterations"] + 2
    assert sol.change[0] <= 1e-6 and hist[iters[0] - 1, 0, 0] == sol.change[0] and hist.shape[0] == iters[0]
    assert sol.info().iterations_enqueued == -(-iters[0] // 4) * 4 < 2000       # stopped at the first look after the component froze
    c = W.forward(xs[0].astype(np.complex128), wavelet, levels)
    assert abs(hist[iters[0] - 1, 0, 1] - np.abs(c[W.detail_mask(c.shape, levels)]).sum()) <= 1e-4 * hist[iters[0] - 1, 0, 1]
    sol.close()
    op.close()


@pytest.mark.parametrize("Z,Ns,wavelet", [("c64", (64, 80), "db2"), ("c128", (16, 16, 8), "haar"), ("c64", (64, 64, 64), "db2")])
def test_determinism_modes_and_graph(Z, Ns, wavelet):
    from nufft_pkg import nufft
    _, Zc, _, _ = FC.dt(Z)
    s = FC.system(Ns)
    levels, C_ = FC.LEVELS[Ns], 2
    op = s.operator(nufft, Z, FC.PATHS[Ns], C_)
    bs = [s.bs[0].astype(Zc), (0.4 * s.bs[1]).astype(Zc)]
    l1 = FC.l1_weight(Ns, wavelet, s.bs[0])
    kw = dict(wavelet=wavelet, levels=levels, l1=l1, step=FC.step(s), maxiter=240, tol=1e-4)
    a = nufft.ToeplitzFISTA(op, check_every=0, **kw)
    xa, ia, sa, ha = _solve(a, bs)
    assert a.info().iterations_enqueued == 240 and sa == ("converged", "converged") and max(ia) < 240
    b = nufft.ToeplitzFISTA(op, check_every=3, **kw)
    xb, ib, sb, hb = _solve(b, bs)
    assert b.info().iterations_enqueued == -(-max(ia) // 3) * 3 < 240
    assert ia == ib and sa == sb and _same(ha, hb) and all(np.array_equal(u, v) for u, v in zip(xa, xb))
    x2, i2, s2, h2 = _solve(a, bs)                                               # two runs
    assert i2 == ia and s2 == sa and _same(h2, ha) and all(np.array_equal(u, v) for u, v in zip(xa, x2))
    assert np.isnan(ha[min(ia):, int(np.argmin(ia))]).all()                      # a frozen component writes no history
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


@pytest.mark.parametrize("Z,Ns,scale", [("c64", (64, 80), 0.4), ("c128", (16, 16, 8), 0.5)])
def test_components(Z, Ns, scale):
    from nufft_pkg import nufft
    _, Zc, _, _ = FC.dt(Z)
    s = FC.system(Ns)
    levels, wavelet = FC.LEVELS[Ns], "db2"
    op = s.operator(nufft, Z, FC.PATHS[Ns], 2)
    b1, b2 = s.bs[0].astype(Zc), (scale * s.bs[1]).astype(Zc)
    zero = np.zeros_like(b1)
    l1 = FC.l1_weight(Ns, wavelet, s.bs[0])
    sol = nufft.ToeplitzFISTA(op, wavelet=wavelet, levels=levels, l1=l1, step=FC.step(s), maxiter=2000, tol=1e-6)
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
    # per-component weights: a huge weight on component 1 leaves only its approximation band
    heavy = nufft.ToeplitzFISTA(op, wavelet=wavelet, levels=levels, l1=(l1, 1e6 * l1), step=FC.step(s), maxiter=20, tol=0.0)
    xh, _, _, hh = _solve(heavy, [b1, b2])
    assert hh[-1, 1, 1] == 0.0 and hh[-1, 0, 1] > 0.0
    assert not W.forward(xh[1].astype(np.complex128), wavelet, levels)[W.detail_mask(b1.shape, levels)].round(4).any()
    # a warm start with out is x0: five iterations, then the rest in place
    short = nufft.ToeplitzFISTA(op, wavelet=wavelet, levels=levels, l1=l1, step=FC.step(s), maxiter=5, tol=1e-6)
    bd = (_dev(b1), _dev(b2))
    x = short.solve(bd)
    again = sol.solve(bd, x0=x, out=x)
    torch.cuda.synchronize()
    assert all(u.data_ptr() == v.data_ptr() for u, v in zip(again, x)) and sol.status == ("converged", "converged")
    if s.A is None:                                                              # positive definite: one minimiser, both solves are near it
        assert R.rel(x[0].cpu().numpy(), xs[0]) <= 1e-2 and R.rel(x[1].cpu().numpy(), xs[1]) <= 1e-2


_SENSE = {}


def _sense_system():
    import test_gpu_cg
    if not _SENSE:
        s = test_gpu_cg._system((48, 40))
        maps = SR.smooth_maps(2, s.shape, seed=11)
        A = SR.dense_sense_gram(s.A, maps)
        _SENSE.update(s=s, maps=maps, A=A, lmax=float(np.linalg.eigvalsh(A)[-1]))
    return _SENSE


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("wavelet", WAVELETS)
def test_with_coil_maps(wavelet, Z):
    from nufft_pkg import nufft
    _, Zc, bar, _ = FC.dt(Z)
    sen = _sense_system()
    s, A = sen["s"], sen["A"]
    maps = sen["maps"].astype(Zc)
    A_used = SR.dense_sense_gram(s.A, maps.astype(np.complex128)) if Z == "c64" else A      # the maps as the operator holds them
    apply = lambda v: (A_used @ np.asarray(v).astype(np.complex128).ravel()).reshape(s.shape)      # noqa: E731
    op = s.operator(nufft, Z, "dense", 1)
    op.set_maps(_dev(maps))
    b = s.bs[0].astype(Zc)
    l1 = 0.3 * float(np.abs(W.forward(b.astype(np.complex128), wavelet, 3)).max())
    step = 1.0 / (1.05 * sen["lmax"])
    sol = nufft.ToeplitzFISTA(op, wavelet=wavelet, levels=3, l1=l1, step=step, maxiter=10, tol=0.0)
    xs, iters, status, hist = _solve(sol, [b])
    ref = F.fista(apply, b, wavelet, 3, l1, step, tol=0.0, max_iter=10, dtype=Zc)
    ex, eh = R.rel(xs[0], ref["x"]), R.rel(hist[:, 0, :], ref["history"])
    print(f"2 coil maps {wavelet} {Z}: x {ex:.3e}, history {eh:.3e} (bar {10 * bar:g}), zero details {ref['zero_fraction']:.2f}")
    assert iters == (10,) and ex <= 10 * bar and eh <= 10 * bar and 0.2 <= ref["zero_fraction"] <= 0.95


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("wavelet", WAVELETS)
def test_coupled_components(wavelet, Z):
    from nufft_pkg import nufft
    import test_gpu_subspace as TS
    _, Zc, bar, _ = FC.dt(Z)
    Ns, K = (48, 40), 2
    sub = TS._system(Ns, K)
    op = sub.operator(nufft, Z, "fused")
    assert op.coupled
    bs = [v.astype(Zc) for v in sub.bs]
    stacked = lambda p: np.stack(sub.apply([p[a] for a in range(K)]))      # noqa: E731
    l1 = 0.3 * float(np.abs(W.forward(bs[0].astype(np.complex128), wavelet, 3)).max())
    step = 1.0 / (1.05 * 1.05 * sub.lmax)                                 # λmax there is a power-iteration estimate from below
    sol = nufft.ToeplitzFISTA(op, wavelet=wavelet, levels=3, l1=l1, step=step, maxiter=10, tol=0.0)
    xs, iters, status, hist = _solve(sol, bs)
    ref = F.fista(stacked, np.stack(bs), wavelet, 3, l1, step, tol=0.0, max_iter=10, dtype=Zc, component_axis=0)
    ex = R.rel(np.stack(xs), ref["x"])
    eh = R.rel(hist[:, 0, :], ref["history"])
    print(f"coupled K=2 {wavelet} {Z}: x {ex:.3e}, history {eh:.3e} (bar {10 * bar:g}), zero details {ref['zero_fraction']:.2f}")
    assert iters == (10, 10) and status == ("max_iter", "max_iter")
    assert _same(hist[:, 0, :], hist[:, 1, :]) and sol.change[0] == sol.change[1]      # one system: one change, one ‖D W x‖₁
    assert ex <= 10 * bar and eh <= 10 * bar and 0.2 <= ref["zero_fraction"] <= 0.95
    auto = nufft.ToeplitzFISTA(op, wavelet=wavelet, levels=3, l1=l1, maxiter=10)      # step=None: from the power iteration
    assert 0.8 / sub.lmax <= auto.step <= 1.0 / (1.05 * 0.95 * sub.lmax)


def test_lifetime_and_arguments():
    from nufft_pkg import nufft
    L, lib = nufft._lib, nufft.lib
    Ns = (48, 40)
    s = FC.system(Ns)
    plan = nufft.PlanNUFFT(np.complex128, Ns, backend=nufft.ROCBackend(0), ntransforms=2)
    op = nufft.ToeplitzOperator(plan)
    for kw in ({"maxiter": 0}, {"tol": -1.0}, {"lam": -1e-3}, {"step": 0.0}, {"step": float("nan")}, {"l1": -1.0}, {"l1": (0.1,)},
               {"check_every": -1}, {"levels": 4}, {"wavelet": "sym4"}):
        with pytest.raises(ValueError):
            nufft.ToeplitzFISTA(op, **{"step": 1.0, **kw})
    with pytest.raises(ValueError):
        nufft.ToeplitzFISTA(op)                                                   # step=None needs the spectrum for the power iteration
    sol = nufft.ToeplitzFISTA(op, l1=0.1, step=0.4 / s.lmax, maxiter=5, tol=0.0)
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
    with pytest.raises(nufft.DimensionMismatch):
        sol.solve(tuple(v[:, :-8].contiguous() for v in b))
    with pytest.raises(ValueError):
        sol.solve(tuple(v.to(torch.complex64) for v in b))
    st = op._stream()
    assert lib.nufft_fista_get_result(sol._handle, None, None, None, 1, st) == L.ERR_INVALID_ARG      # capacity < ntransforms
    assert lib.nufft_fista_history(sol._handle, (C.c_double * 4)(), 4, st) == L.ERR_INVALID_ARG
    assert lib.nufft_fista_set_l1(sol._handle, (C.c_double * 2)(0.1, -1.0), 2) == L.ERR_INVALID_ARG
    assert lib.nufft_fista_set_l1(sol._handle, (C.c_double * 2)(0.1, 0.1), 1) == L.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert not x[0].any() and not x[1].any()                                      # refused before anything was enqueued
    sol.solve(b, out=x)
    torch.cuda.synchronize()
    i = sol.info()
    pad = lambda v: (max(v, 16) + 255) // 256 * 256      # noqa: E731
    assert sol.iterations == (5, 5) and i.iterations_enqueued == 5 and i.array_bytes == 3 * 2 * pad(48 * 40 * 16)
    assert i.array_bytes < i.workspace_bytes < i.array_bytes * 1.5 + (64 << 10)   # three arrays per component plus the ping-pong scratch
    op.set_spectrum(_dev(2 * s.spec))                                             # a new G between two solves is allowed
    sol.solve(b, out=x)
    torch.cuda.synchronize()
    assert sol.iterations == (5, 5)
    op.close()                                                                    # the library keeps a pointer to the operator
    for call in (lambda: sol.solve(b), sol.info, lambda: sol.iterations, sol.history):
        with pytest.raises(ValueError, match="outlive"):
            call()
    sol.close()
    with pytest.raises(ValueError, match="closed"):
        sol.info()


@pytest.mark.parametrize("Z", TYPES)
def test_breakdown_freezes_one_component(Z):
    """A NaN in one cell of b[1]: the reference's rule (fista_reference.fista: a change that is not finite is BREAKDOWN, and the iteration
    that found it is the last) for that component alone; component 0 runs as if b[1] were finite.  Then the same solver on finite data:
    the start kernel's reset leaves nothing behind."""
    from nufft_pkg import nufft
    L, lib = nufft._lib, nufft.lib
    _, Zc, bar, _ = FC.dt(Z)
    Ns = (16, 12)
    s = FC.Analytic(Ns, seed=4 * sum(Ns))
    plan = nufft.PlanNUFFT(Zc, Ns, backend=nufft.ROCBackend(0), ntransforms=2)
    op = nufft.ToeplitzOperator(plan)
    op.set_spectrum(_dev(s.spec.astype(Zc)))
    plan.close()
    good = [s.bs[0].astype(Zc), (0.4 * s.bs[1]).astype(Zc)]
    bad = [good[0], good[1].copy()]
    bad[1][5, 7] = np.nan
    l1 = 0.3 * float(np.abs(W.forward(s.bs[0], "haar", 2)).max())
    kw = dict(wavelet="haar", levels=2, l1=l1, step=FC.step(s), maxiter=4, tol=0.0)
    fresh = nufft.ToeplitzFISTA(op, **kw)
    xg, ig, sg, hg = _solve(fresh, good)
    assert ig == (4, 4) and sg == ("max_iter", "max_iter") and np.isfinite(hg).all()
    sol = nufft.ToeplitzFISTA(op, **kw)
    xb, ib, sb, hb = _solve(sol, bad)
    print(f"breakdown {Z}: iterations {ib}, status {sb}, history of component 1 {hb[:, 1, 0]}")
    assert sb[1] == "breakdown" and ib[1] == 1 and np.isnan(hb[0, 1, 0]) and np.isnan(sol.change[1])
    assert sb[0] == sg[0] and ib[0] == ig[0] and _same(hb[:, 0], hg[:, 0])
    assert R.rel(xb[0], xg[0]) <= 10 * bar
    full = (C.c_double * (4 * 2 * 2))()
    assert lib.nufft_fista_history(sol._handle, full, len(full), op._stream()) == L.OK
    assert np.isnan(np.array(full).reshape(4, 2, 2)[1:, 1]).all()                  # the frozen component writes no later row
    x2, i2, s2, h2 = _solve(sol, good)                                             # a second solve on the solver that broke down
    assert i2 == ig and s2 == sg and _same(h2, hg) and all(np.array_equal(u, v) for u, v in zip(x2, xg))
    sol.close()
    fresh.close()
    op.close()
