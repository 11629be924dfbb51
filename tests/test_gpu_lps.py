"""The low-rank plus sparse solver on the GPU against the numpy reference (lps_reference.lps) run in the same element
type.  Systems, weights and cached references: lps_cases.py (framed operators with exact spectra, so the only error in G is the
operator's own).

Bars:
  * ten iterations (tol = 0): x, L, S and the three history columns within 10 × the operator's parity bar (1e-11 / 1e-4) relative L2:
    every step is non-expansive.  The ComplexF32 reference must stay within a third of that of its float64 run, and the reference's
    tenth iteration must zero some but not all singular values and between 0.2 and 0.95 of the temporal coefficients.
  * converged solve on (32, 40) K = 3 (tol = 1e-6, check_every = 8): iterations <= 1.1 × the reference's + 2 (the float64 reference takes
    363 with momentum and 488 without), the float64 fixed-point residual of the GPU's (L, S) <= 3 × the reference's own, taken from the
    reference at test time.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import lps_cases as LC  # noqa: E402
import lps_reference as P  # noqa: E402
import sense_reference as SR  # noqa: E402

TYPES = ["c128", "c64"]
BAR = {"c128": 1e-11, "c64": 1e-4}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(xs):
    return np.stack([v.cpu().numpy() for v in xs])


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _solve(sol, b, **kw):
    """solve + outcome as numpy; b: the stacked right-hand sides [K, ...] on the host."""
    bd = tuple(_dev(v) for v in b)
    x = sol.solve(bd, **kw)
    torch.cuda.synchronize()
    return {"x": _host(x), "L": _host(sol.low_rank), "S": _host(sol.sparse), "iterations": sol.iterations, "status": sol.status,
            "history": sol.history().numpy()}


def _compare(tag, Z, got, ref, high, K, condition=True):
    bar = BAR[Z]
    errs = {k: LC.rel(got[k], ref[k]) for k in ("x", "L", "S")}
    for j, name in enumerate(("change", "nuclear norm", "l1")):
        errs[name] = LC.rel(got["history"][:, j], ref["history"][:, j])
    own = max(LC.rel(ref[k], high[k]) for k in ("x", "L", "S", "history"))
    print(f"ten iterations {tag} {Z}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) +
          f" (bar {bar:g}; reference vs float64 {own:.1e}), zeroed {ref['zeroed_sv']}/{K}, zero share {ref['zero_share']:.2f}")
    assert got["iterations"] == (10,) * K and got["status"] == ("max_iter",) * K and got["history"].shape == (10, 3)
    assert own <= bar / 3, own
    assert all(v <= bar for v in errs.values()), errs
    if condition:
        assert 0 < ref["zeroed_sv"] < K and 0.2 <= ref["zero_share"] <= 0.95, (ref["zeroed_sv"], ref["zero_share"])


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("transform", P.TRANSFORMS)
@pytest.mark.parametrize("momentum", [True, False])
@pytest.mark.parametrize("Ns,K,path", LC.SOLVER_CASES)
def test_ten_iterations(Ns, K, path, momentum, transform, Z):
    from nufft_pkg import nufft
    Zc = LC.dt(Z)[1]
    c = LC.case(Ns, K)
    nuc, l1 = c.weights(transform)
    op = c.s.operator(nufft, Z, path)
    sol = nufft.ToeplitzLPS(op, nuc, l1, transform=transform, momentum=momentum, step=c.step(), maxiter=10, tol=0.0)
    got = _solve(sol, c.b.astype(Zc))
    kw = dict(tol=0.0, max_iter=10)
    _compare(f"N={Ns} K={K} {transform} momentum={momentum}", Z, got, LC.reference(c, Z, nuc, l1, transform, momentum, **kw),
             LC.reference(c, Z, nuc, l1, transform, momentum, high=True, **kw), K)
    i = sol.info()
    pad = lambda v: (max(v, 16) + 255) // 256 * 256      # noqa: E731
    assert i.array_bytes == 5 * K * pad(int(np.prod(Ns)) * np.dtype(Zc).itemsize) and i.iterations_enqueued == 10
    assert i.array_bytes < i.workspace_bytes < i.array_bytes + (1 << 20) + 16 * 512 * K * (K + 1) // 2
    sol.close()
    op.close()


@pytest.mark.parametrize("Z", TYPES)
def test_ten_iterations_on_every_operator_state(Z):
    """On (32, 40) K = 3: a Tikhonov term, 2 coil maps on the framed operator, a plain operator (one shared multiplier), nuc = 0, and an
    l1 so large that S stays exactly zero."""
    from nufft_pkg import nufft
    Zc = LC.dt(Z)[1]
    Ns, K = (32, 40), 3
    c = LC.case(Ns, K)
    b = c.b.astype(Zc)
    nuc, l1 = c.weights("dft")
    kw = dict(tol=0.0, max_iter=10)
    op = c.s.operator(nufft, Z, "fused")
    # lam = 0.1 λmax
    lam = 0.1 * c.lmax
    sol = nufft.ToeplitzLPS(op, nuc, l1, step=c.step(lam), lam=lam, maxiter=10, tol=0.0)
    _compare("lam=0.1 lmax", Z, _solve(sol, b), LC.reference(c, Z, nuc, l1, "dft", True, lam=lam, **kw),
             LC.reference(c, Z, nuc, l1, "dft", True, lam=lam, high=True, **kw), K)
    # nuc = 0: no singular value is touched
    sol.set_weights(0.0, l1)
    got = _solve(sol, b)
    ref = LC.reference(c, Z, 0.0, l1, "dft", True, lam=lam, **kw)
    _compare("nuc=0", Z, got, ref, LC.reference(c, Z, 0.0, l1, "dft", True, lam=lam, high=True, **kw), K, condition=False)
    assert ref["zeroed_sv"] == 0
    sol.close()
    # l1 far above max|T b|: every coefficient is below the threshold, S is exactly zero and x is L bit for bit
    big = 10.0 * float(np.abs(P.tdft(c.b)).max())
    sol = nufft.ToeplitzLPS(op, nuc, big, momentum=False, step=c.step(), maxiter=10, tol=0.0)
    got = _solve(sol, b)
    ref = LC.reference(c, Z, nuc, big, "dft", False, **kw)
    _compare("l1 large", Z, got, ref, LC.reference(c, Z, nuc, big, "dft", False, high=True, **kw), K, condition=False)
    assert ref["zero_share"] == 1.0 and not ref["S"].any()
    assert not got["S"].any() and np.array_equal(got["x"], got["L"]) and not got["history"][:, 2].any()
    sol.close()
    # 2 coil maps, the same for every frame: G_c = Σ_j conj(S_j) G0_c S_j
    maps = SR.smooth_maps(2, c.s.shape[1:], seed=11).astype(Zc)
    m64 = maps.astype(np.complex128)
    apply = lambda v: np.stack([sum(np.conj(m) * f.apply(m * np.asarray(v[k]).astype(np.complex128)) for m in m64)      # noqa: E731
                                for k, f in enumerate(c.s.frames)])
    step = c.step() / float((np.abs(m64) ** 2).sum(axis=0).max())
    op.set_maps(_dev(maps))
    sol = nufft.ToeplitzLPS(op, nuc, l1, step=step, maxiter=10, tol=0.0)
    mk = dict(apply=apply, key="maps", step=step, **kw)
    _compare("2 coil maps", Z, _solve(sol, b), LC.reference(c, Z, nuc, l1, "dft", True, **mk), LC.reference(c, Z, nuc, l1, "dft", True, high=True, **mk), K)
    sol.close()
    op.close()
    # a plain operator: K components, one multiplier
    sh = LC.case(Ns, K, shared=True)
    op = sh.s.operator(nufft, Z, "fused", framed=False)
    assert not op.framed
    nuc, l1 = sh.weights("dft")
    sol = nufft.ToeplitzLPS(op, nuc, l1, step=sh.step(), maxiter=10, tol=0.0)
    _compare("shared multiplier", Z, _solve(sol, sh.b.astype(Zc)), LC.reference(sh, Z, nuc, l1, "dft", True, key="shared", **kw),
             LC.reference(sh, Z, nuc, l1, "dft", True, key="shared", high=True, **kw), K)
    sol.close()
    op.close()


@pytest.mark.parametrize("Z,momentum", [("c128", True), ("c128", False), ("c64", True)])
def test_converged_solve(Z, momentum):
    from nufft_pkg import nufft
    Zc = LC.dt(Z)[1]
    Ns, K = (32, 40), 3
    c = LC.case(Ns, K)
    nuc, l1 = c.weights("dft")
    op = c.s.operator(nufft, Z, "fused")
    sol = nufft.ToeplitzLPS(op, nuc, l1, momentum=momentum, step=c.step(), maxiter=3000, tol=1e-6, check_every=8)
    got = _solve(sol, c.b.astype(Zc))
    ref = LC.reference(c, Z, nuc, l1, "dft", momentum, tol=1e-6, max_iter=3000)
    b64 = c.b.astype(Zc).astype(np.complex128)
    res = P.fixed_point_residual(c.apply, b64, got["L"], got["S"], nuc, l1, c.step())
    res_ref = P.fixed_point_residual(c.apply, b64, ref["L"], ref["S"], nuc, l1, c.step())
    iters = got["iterations"]
    print(f"converged {Z} momentum={momentum}: {iters[0]} iterations (reference {ref['iterations']}), fixed-point residual {res:.3e} "
          f"(reference {res_ref:.3e}), change {sol.change[0]:.3e}, enqueued {sol.info().iterations_enqueued}")
    assert got["status"] == ("converged",) * K and ref["status"] == P.CONVERGED
    assert len(set(iters)) == 1 and len(set(sol.change)) == 1
    assert res <= 3 * res_ref
    assert iters[0] <= 1.1 * ref["iterations"] + 2
    hist = got["history"]
    assert sol.change[0] <= 1e-6 and hist[iters[0] - 1, 0] == sol.change[0] and hist.shape == (iters[0], 3)
    assert sol.info().iterations_enqueued == -(-iters[0] // 8) * 8 < 3000
    want_nuc, want_l1 = P.singular_values(got["L"]).sum(), np.abs(P.tdft(got["S"])).sum()
    assert abs(hist[-1, 1] - want_nuc) <= 1e-4 * want_nuc and abs(hist[-1, 2] - want_l1) <= 1e-4 * want_l1
    sol.close()
    op.close()


@pytest.mark.parametrize("Z,Ns,K", [("c64", (32, 40), 3), ("c128", (12, 10), 17)])
def test_determinism_modes_graph_and_warm_start(Z, Ns, K):
    from nufft_pkg import nufft
    Zc = LC.dt(Z)[1]
    c = LC.case(Ns, K)
    op = c.s.operator(nufft, Z, LC.PATHS[(Ns, K)])
    b = c.b.astype(Zc)
    nuc, l1 = c.weights("dft")
    kw = dict(step=c.step(), maxiter=400, tol=1e-3)
    a = nufft.ToeplitzLPS(op, nuc, l1, check_every=0, **kw)
    ra = _solve(a, b)
    ia = ra["iterations"]
    print(f"modes {Z} N={Ns} K={K}: iterations {ia}")
    assert a.info().iterations_enqueued == 400 and ra["status"] == ("converged",) * K and len(set(ia)) == 1 and ia[0] < 400
    d = nufft.ToeplitzLPS(op, nuc, l1, check_every=4, **kw)
    rd = _solve(d, b)
    assert d.info().iterations_enqueued == -(-ia[0] // 4) * 4 < 400
    r2 = _solve(a, b)                                                             # two runs
    for other in (rd, r2):
        assert other["iterations"] == ia and other["status"] == ra["status"] and _same(other["history"], ra["history"])
        assert all(np.array_equal(other[k], ra[k]) for k in ("x", "L", "S"))
    bd = tuple(_dev(v) for v in b)
    out = tuple(torch.zeros_like(v) for v in bd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        a.solve(bd, out=out)
        with pytest.raises(ValueError):                                           # check_every > 0 synchronises: refused while capturing
            d.solve(bd, out=out)
    for _ in range(2):
        for o in out:
            o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert a.iterations == ia and a.status == ra["status"] and _same(a.history().numpy(), ra["history"])
        assert np.array_equal(_host(out), ra["x"]) and np.array_equal(_host(a.low_rank), ra["L"]) and np.array_equal(_host(a.sparse), ra["S"])
    del graph
    # x = L + S, one rounding
    eps = LC.dt(Z)[3]
    assert np.abs(ra["x"] - (ra["L"] + ra["S"])).max() <= eps * np.abs(ra["x"]).max()
    # a warm start from the solution (out is x0): L starts at x, S at zero
    x = tuple(_dev(v) for v in ra["x"])
    again = d.solve(bd, x0=x, out=x)
    torch.cuda.synchronize()
    assert all(u.data_ptr() == v.data_ptr() for u, v in zip(again, x)) and d.status == ("converged",) * K
    print(f"warm start: iterations {d.iterations}")
    assert len(set(d.iterations)) == 1 and d.iterations[0] < 400
    # other weights take effect, and the first ones give the first answer again
    d.set_weights(2.0 * nuc, 0.5 * l1)
    other = _solve(d, b)
    assert other["status"] == ("converged",) * K and not np.array_equal(other["x"], ra["x"])
    assert other["history"][-1, 1] < ra["history"][-1, 1]                          # a heavier nuclear-norm weight: a smaller nuclear norm
    d.set_weights(nuc, l1)
    back = _solve(d, b)
    assert np.array_equal(back["x"], ra["x"]) and _same(back["history"], ra["history"])
    a.close()
    d.close()
    op.close()


def test_arguments_and_lifetime():
    from nufft_pkg import nufft
    Ns, K = (32, 40), 3
    c = LC.case(Ns, K)
    plan = nufft.PlanNUFFT(np.complex128, Ns, backend=nufft.ROCBackend(0), ntransforms=K)
    op = nufft.ToeplitzOperator(plan)
    plan.close()
    for kw in ({"nuc": -1.0}, {"l1": float("nan")}, {"transform": "difference"}, {"maxiter": 0}, {"tol": -1.0}, {"step": 0.0}, {"check_every": -1},
               {"lam": -1.0}):
        with pytest.raises(ValueError):
            nufft.ToeplitzLPS(op, **{"nuc": 0.1, "l1": 0.1, "step": 1.0, **kw})
    with pytest.raises(ValueError):
        nufft.ToeplitzLPS(op, 0.1, 0.1)                                             # step=None needs the spectrum
    sol = nufft.ToeplitzLPS(op, 0.1, 0.1, step=c.step(), maxiter=5, tol=0.0)
    b = tuple(_dev(v) for v in c.b)
    with pytest.raises(ValueError):                                               # no spectrum yet
        sol.solve(b)
    with pytest.raises(ValueError):
        sol.low_rank
    op.set_spectra_frames([_dev(s) for s in c.s.spectra])
    with pytest.raises(ValueError):
        sol.solve(b, out=b)
    with pytest.raises(nufft.DimensionMismatch):
        sol.solve(b[0])
    with pytest.raises(ValueError):
        sol.set_weights(-1.0, 0.1)
    sol.solve(b)
    torch.cuda.synchronize()
    assert sol.iterations == (5,) * K and sol.info().iterations_enqueued == 5 and "ToeplitzLPS" in repr(sol)
    lib, E, tab = nufft.lib, nufft._lib.ERR_INVALID_ARG, nufft.plan._ptr_table
    parts = tuple(torch.empty_like(v) for v in b)
    flat = torch.empty(2 * b[0].numel(), dtype=b[0].dtype, device="cuda")
    n = b[0].numel()
    assert lib.nufft_lps_get_parts(sol._handle, tab(parts), tab(parts), op._stream()) == E          # L and S into the same arrays
    assert lib.nufft_lps_get_parts(sol._handle, tab((flat[:n], flat[n // 2:n // 2 + n], parts[2])), None, op._stream()) == E
    assert lib.nufft_lps_get_parts(sol._handle, tab(parts), None, op._stream()) == 0 and lib.nufft_lps_get_parts(sol._handle, None, None, op._stream()) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(parts, sol.low_rank))
    auto = nufft.ToeplitzLPS(op, 0.1, 0.1, maxiter=5)                               # step=None: from the power iteration, with the 2
    assert 0.8 / (2 * c.lmax) <= auto.step <= 1.0 / (2 * 1.05 * 0.9 * c.lmax)
    auto.close()
    op.close()                                                                    # the library keeps a pointer to the operator
    for call in (lambda: sol.solve(b), sol.info, lambda: sol.iterations, sol.history):
        with pytest.raises(ValueError, match="outlive"):
            call()
    sol.close()
    with pytest.raises(ValueError, match="closed"):
        sol.info()


@pytest.mark.parametrize("Z", TYPES)
def test_breakdown_freezes_the_system(Z):
    """A NaN in one cell of b[1]: the frames are one system, so the reference's rule (lps_reference.lps: a change that is not finite is
    BREAKDOWN, and the iteration that found it is the last) holds for every frame.  Then the same solver on finite data: the start kernel's
    reset leaves nothing behind."""
    from nufft_pkg import nufft
    Ns, K = (16, 12), 3
    c = LC.Case(Ns, K)
    op = c.s.operator(nufft, Z)
    good = c.b.astype(LC.dt(Z)[1])
    nuc, l1 = c.weights("dft")
    make = lambda: nufft.ToeplitzLPS(op, nuc, l1, step=c.step(), maxiter=4, tol=0.0)      # noqa: E731
    run = lambda sol, b: (lambda g: (g, g["iterations"], g["status"], g["history"]))(_solve(sol, b))      # noqa: E731
    bad = good.copy()
    bad[1, 5, 7] = np.nan
    fresh = make()
    gg, ig, sg, hg = run(fresh, good)
    assert ig == (4,) * 3 and sg == ("max_iter",) * 3 and np.isfinite(hg).all()
    sol = make()
    _, ib, sb, hb = run(sol, bad)
    print(f"breakdown {Z}: iterations {ib}, status {sb}, history {hb.tolist()}")
    assert sb == ("breakdown",) * 3 and ib == (1,) * 3 and np.isnan(sol.change).all() and np.isnan(hb[0, 0]).all()
    full = (C.c_double * (4 * 3))()
    assert nufft.lib.nufft_lps_history(sol._handle, full, len(full), op._stream()) == nufft._lib.OK
    assert np.isnan(np.array(full).reshape(4, -1)[1:]).all()                       # the frozen system writes no later row
    g2, i2, s2, h2 = run(sol, good)                                                # a second solve on the solver that broke down
    assert i2 == ig and s2 == sg and _same(h2, hg) and all(np.array_equal(g2[k], gg[k]) for k in ("x", "L", "S"))
    sol.close()
    fresh.close()
    op.close()
