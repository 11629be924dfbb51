"""Coil sensitivity maps in the Toeplitz normal operator on the GPU: G_S û = Σ_c conj(S_c) ⊙ G (S_c ⊙ û) against the
exact product from direct sums on the CPU (sense_reference.py), its CG, and the coil expand / combine passes.

Every case asserts the apply path it runs; fused cases run both routes (`NUFFT_TOEPLITZ_MAPS_INPASS` 1: the maps inside the outermost
pruned passes; 0: expand, plain apply, combine).  Bars:
  * exact spectrum: the project's parity bars, rel-L2 <= 1e-12 (ComplexF64) / 1e-5 (ComplexF32), as in test_gpu_toeplitz.py;
  * built from points: relative to the composed route measured in the same test (the bars of test_gpu_toeplitz.test_built_from_points);
  * CG: the bars of test_gpu_cg.py.  With normalised maps the eigenvalues of G_S lie within those of G (test_sense_host.py), so the
    argument behind them (errors of the apply enter multiplied by cond <= 7) carries over; every case asserts cond on its own matrix;
  * coil expand / combine, with u = 2^-24 or 2^-53 the unit roundoff: each part of a complex product s·a is two rounded products and
    one rounded sum (with or without fused multiply-add), an error of at most 2u (|s_r a_r| + |s_i a_i|) <= 2u |s||a| to first order;
    adding n such terms in order adds n − 1 roundings of partial sums, each at most u Σ_c |s_c||a_c|.  Per part that is
    (n + 1) u Σ_c |s_c||a_c|, for the complex element √2 times as much; asserted in the 2-norm over the array with 1 % on top for the
    second-order terms.  Expand is the case n = 1.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import cg_reference as CG  # noqa: E402
import sense_reference as S  # noqa: E402
import toeplitz_reference as R  # noqa: E402

NP = 2000


def _dt(Z):
    return (np.float64, np.complex128, 1e-12, 1e-10) if Z == "c128" else (np.float32, np.complex64, 1e-5, 1e-4)


def _dev(a, Zc=None):
    return torch.from_numpy(np.ascontiguousarray(a if Zc is None else a.astype(Zc))).cuda()


def _routes(path):
    """(path, NUFFT_TOEPLITZ_MAPS_INPASS) pairs: the fused path has two routes, the dense path one."""
    return (("fused", 1), ("fused", 0)) if path == "fused" else (("dense", 1),)


def _op(nufft, Z, Ns, path, inpass=1, **kw):
    opts = {"NUFFT_TOEPLITZ_MAPS_INPASS": inpass}
    if path == "dense":
        opts["NUFFT_TOEPLITZ_FUSED"] = 0
    plan = nufft.PlanNUFFT(np.complex128 if Z == "c128" else np.complex64, Ns, backend=nufft.ROCBackend(0), options=opts, **kw)
    op = nufft.ToeplitzOperator(plan)
    assert op.path == path, (Ns, path, op.path)
    return plan, op


def _problem(Ns, T, C=1, seed=0, ncoils=2):
    rng = np.random.default_rng(seed)
    xs = [(rng.random(NP) * 2 * np.pi).astype(T) for _ in Ns]
    w = (rng.random(NP) + 0.1).astype(T)
    us = [rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1]) for _ in range(C)]
    return xs, w, us, S.smooth_maps(ncoils, Ns[::-1], seed=seed + 100)


# (Z, N, fftshift, paths, ncoils, ntransforms, maps handed over as one stacked tensor)
EXACT_CASES = [
    ("c128", (40, 48), True, ("fused", "dense"), 3, 1, False),   # 40 columns: not a multiple of the 16 lines per workgroup
    ("c64", (32, 32), False, ("fused", "dense"), 2, 2, True),
    ("c128", (48, 40), False, ("fused",), 1, 1, False),          # one coil: never accumulates
    ("c128", (48, 32, 40), False, ("fused", "dense"), 3, 1, True),
    ("c64", (48, 32, 40), True, ("fused",), 2, 1, False),
    ("c128", (64,), False, ("dense",), 3, 1, False),
    ("c64", (15, 9), False, ("dense",), 3, 1, True),             # stacked, odd element count: misaligned slices, realigned in Python
    ("c128", (9, 7, 5), False, ("dense",), 2, 1, False),
]


@pytest.mark.parametrize("Z,Ns,fftshift,paths,ncoils,C,stacked", EXACT_CASES)
def test_exact_spectrum(Z, Ns, fftshift, paths, ncoils, C, stacked):
    from nufft_pkg import nufft
    T, Zc, bar, _ = _dt(Z)
    xs, w, us, maps = _problem(Ns, T, C, seed=len(Ns) + C, ncoils=ncoils)
    x64, w64 = [x.astype(np.float64) for x in xs], w.astype(np.float64)
    us, maps = [u.astype(Zc) for u in us], maps.astype(Zc)
    if ncoils > 1:
        assert not maps[-1].ravel()[0]                           # the exactly zero region of the last coil
    spec = R.exact_spectrum(Ns, x64, w64)
    m128 = maps.astype(np.complex128)
    refs = [S.exact_sense_gram(Ns, x64, w64, m128, u.astype(np.complex128), fftshift) for u in us]
    got = {}
    for path in paths:
        for route in _routes(path):
            plan, op = _op(nufft, Z, Ns, path, route[1], fftshift=fftshift, ntransforms=C)
            md = _dev(maps) if stacked else tuple(_dev(m) for m in maps)
            assert op.set_maps(md) is op and op.ncoils == ncoils and f"{ncoils} coil maps" in repr(op)   # maps before the spectrum
            if stacked and Z == "c64" and int(np.prod(Ns)) % 2:
                assert any(m.data_ptr() % 16 for m in md) and all(m.data_ptr() % 16 == 0 for m in op._maps)
            op.set_spectrum(_dev(spec, Zc))
            plan.close()
            ud = tuple(_dev(u) for u in us)
            out = op.apply(ud if C > 1 else ud[0])
            torch.cuda.synchronize()
            got[route] = [o.cpu().numpy() for o in (out if C > 1 else (out,))]
            for c in range(C):
                err = R.rel(got[route][c], refs[c])
                print(f"exact spectrum {Z} N={Ns} shift={fftshift} {ncoils} coils {route} c={c}: rel-L2 {err:.3e} (bar {bar:g})")
                assert err <= bar
                assert np.array_equal(ud[c].cpu().numpy(), us[c])                  # the input is only read
            op.close()
    keys = list(got)
    for other in keys[1:]:
        for c in range(C):
            err = R.rel(got[other][c], got[keys[0]][c])
            print(f"  {other} vs {keys[0]} c={c}: {err:.3e}")
            assert err <= bar


@pytest.mark.parametrize("Z,Ns,path", [("c128", (48, 40), "fused"), ("c64", (32, 32, 32), "fused"), ("c64", (15, 9), "dense")])
def test_all_ones_maps_and_clear(Z, Ns, path):
    from nufft_pkg import nufft
    T, Zc, bar, _ = _dt(Z)
    _, _, us, _ = _problem(Ns, T, 1, seed=3)
    u = us[0].astype(Zc)
    # an analytic spectrum, T[d] = Π 0.2^|d_dim| (test_gpu_cg.test_more_workgroups): two operators hold the same K bit for bit, which
    # two builds from points do not (spreading accumulates with atomics)
    D = len(Ns)
    spec = np.ones([2 * n for n in reversed(Ns)])
    for dim, n in enumerate(Ns):
        shape = [1] * D
        shape[D - 1 - dim] = 2 * n
        spec = spec * (0.2 ** np.abs(np.asarray(R.modes(2 * n)).astype(np.float64))).reshape(shape)
    sd = _dev(spec.astype(np.complex128), Zc)
    _, never = _op(nufft, Z, Ns, path)
    never.set_spectrum(sd)
    plain = never(_dev(u)).cpu().numpy()
    ones = torch.ones((2,) + Ns[::-1], dtype=torch.complex128 if Z == "c128" else torch.complex64, device="cuda")
    for route in _routes(path):
        _, op = _op(nufft, Z, Ns, path, route[1])
        op.set_spectrum(sd).set_maps(ones)
        twice = op(_dev(u)).cpu().numpy()
        err = R.rel(twice, 2 * plain)
        print(f"all-ones maps {Z} N={Ns} {route}: rel-L2 against 2 x plain {err:.3e} (bar {bar:g})")
        assert err <= bar
        assert op.clear_maps() is op and op.ncoils == 0
        op.clear_maps()                                                          # idempotent
        ud = _dev(u)
        assert np.array_equal(op(ud).cpu().numpy(), plain)
        res = op.apply(ud, out=ud)                                               # in place is allowed again
        assert res.data_ptr() == ud.data_ptr() and np.array_equal(ud.cpu().numpy(), plain)


@pytest.mark.parametrize("Z", ["c128", "c64"])
@pytest.mark.parametrize("Ns", [(48, 40), (32, 32, 32)])
def test_built_from_points(Z, Ns):
    from nufft_pkg import nufft
    T, Zc, _, _ = _dt(Z)
    xs, w, us, maps = _problem(Ns, T, 1, seed=11, ncoils=2)
    u, maps = us[0].astype(Zc), maps.astype(Zc)
    ref = S.exact_sense_gram(Ns, [x.astype(np.float64) for x in xs], w.astype(np.float64), maps.astype(np.complex128), u.astype(np.complex128))
    plan, op = _op(nufft, Z, Ns, "fused", m=4)
    pd, wd, ud, md = tuple(_dev(x) for x in xs), _dev(w), _dev(u), _dev(maps)
    # the composed route Σ_c conj(S_c) · exec_type1(w · exec_type2(S_c · u)) on the plan's own code paths
    nufft.set_points(plan, pd)
    v = torch.empty(NP, dtype=plan.Z, device="cuda")
    g1 = torch.empty_like(ud)
    gc = torch.zeros_like(ud)
    for c in range(2):
        nufft.exec_type2(v, plan, md[c] * ud)
        v *= wd
        nufft.exec_type1(g1, plan, v)
        gc += md[c].conj() * g1
    torch.cuda.synchronize()
    err_c = R.rel(gc.cpu().numpy(), ref)
    gt = op.set_maps(md).set_points(pd, wd)(ud)
    torch.cuda.synchronize()
    err_t = R.rel(gt.cpu().numpy(), ref)
    print(f"from points {Z} N={Ns} m=4, 2 coils: toeplitz {err_t:.3e}, composed {err_c:.3e}, ratio {err_t / err_c:.2f}")
    if Z == "c128":
        assert err_t <= 3 * err_c
    else:
        assert err_t <= max(5 * err_c, 1e-4)


@pytest.mark.parametrize("Z,Ns,path", [("c128", (32, 32, 32), "fused"), ("c64", (40, 48), "fused"), ("c128", (48,), "dense")])
def test_determinism_stream_and_graph(Z, Ns, path):
    from nufft_pkg import nufft
    T, Zc, _, _ = _dt(Z)
    xs, w, us, maps = _problem(Ns, T, 1, seed=4, ncoils=3)
    pd, wd, md = tuple(_dev(x) for x in xs), _dev(w), _dev(maps.astype(Zc))
    for route in _routes(path):
        _, op = _op(nufft, Z, Ns, path, route[1])
        op.set_points(pd, wd).set_maps(md)
        ud = _dev(us[0].astype(Zc))
        eager = op(ud).cpu().numpy()
        assert np.array_equal(op(ud).cpu().numpy(), eager)                       # two applies
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            side = op(ud)
        s.synchronize()
        assert np.array_equal(side.cpu().numpy(), eager)
        out = torch.empty_like(ud)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                            # one stream, as in test_gpu_toeplitz.test_stream_and_graph
            op.apply(ud, out=out)
        for _ in range(2):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), eager)
        del graph
        op.close()


class System:
    """The recipe of test_gpu_cg.py (uniform points, Np >= 20 n in 2-D, exact spectrum, exact dense matrix) with normalised maps."""

    def __init__(self, Ns, ncoils, seed):
        rng = np.random.default_rng(seed)
        n = int(np.prod(Ns))
        Np = 400 if Ns == (48,) else 2000 if n <= 200 else 20 * n
        self.Ns, self.shape = Ns, Ns[::-1]
        self.xs = [rng.random(Np) * 2 * np.pi for _ in Ns]
        self.w = rng.random(Np) + 0.1
        self.spec = R.exact_spectrum(Ns, self.xs, self.w)
        self.maps = S.normalise(S.smooth_maps(ncoils, self.shape, seed=seed + 1))
        self.b = rng.standard_normal(self.shape) + 1j * rng.standard_normal(self.shape)

    def matrix(self, Zc):
        """G_S with the maps as the device holds them (rounded to the element type), and its extreme eigenvalues."""
        A = S.dense_sense_gram(CG.dense_gram(self.Ns, self.xs, self.w, spectrum=self.spec), self.maps.astype(Zc).astype(np.complex128))
        ev = np.linalg.eigvalsh(A)
        return A, float(ev[0]), float(ev[-1])


_SYSTEMS = {}

# (Z, N, path, ncoils)
CG_CASES = [("c128", (32, 32), "fused", 2), ("c64", (48, 40), "fused", 3), ("c64", (15, 9), "dense", 3), ("c128", (48,), "dense", 2)]


def _system(Ns, ncoils):
    if (Ns, ncoils) not in _SYSTEMS:
        _SYSTEMS[(Ns, ncoils)] = System(Ns, ncoils, seed=4 * sum(Ns))
    return _SYSTEMS[(Ns, ncoils)]


def _cg_op(nufft, s, Z, path, inpass=1):
    Zc = _dt(Z)[1]
    plan, op = _op(nufft, Z, s.Ns, path, inpass)
    op.set_spectrum(_dev(s.spec, Zc)).set_maps(_dev(s.maps, Zc))
    plan.close()
    return op


def _solve(sol, b, **kw):
    x = sol.solve(_dev(b), **kw)
    torch.cuda.synchronize()
    return x.cpu().numpy(), sol.iterations[0], sol.status[0], sol.history().numpy()[:, 0]


@pytest.mark.parametrize("Z,Ns,path,ncoils", CG_CASES)
def test_cg_with_maps(Z, Ns, path, ncoils):
    from nufft_pkg import nufft
    T, Zc, bar, rtol = _dt(Z)
    s = _system(Ns, ncoils)
    A, lmin, lmax = s.matrix(Zc)
    apply = CG.matrix_apply(A, s.shape)
    b = s.b.astype(Zc)
    for route in _routes(path):
        op = _cg_op(nufft, s, Z, path, route[1])
        for lam in (0.0, 1e-3 * lmax):
            cond = (lmax + lam) / (lmin + lam)
            assert cond <= 7, cond
            sol = nufft.ToeplitzCG(op, maxiter=5, rtol=0.0, lam=lam)
            x, it, st, hist = _solve(sol, b)
            ref = CG.cg(apply, b, lam=lam, rtol=0.0, max_iter=5, dtype=Zc)
            ex, eh = R.rel(x, ref["x"]), R.rel(hist, ref["history"])
            print(f"CG 5 iterations {Z} N={Ns} {route} {ncoils} coils lam={lam:.3g} cond={cond:.2f}: x {ex:.3e}, history {eh:.3e} (bar {10 * bar:g})")
            assert it == 5 and st == "max_iter" and hist.shape == (6,)
            assert ex <= 10 * bar and eh <= 10 * bar
            sol.close()
            sol = nufft.ToeplitzCG(op, maxiter=100, rtol=rtol, lam=lam)
            x, it, st, hist = _solve(sol, b)
            ref = CG.cg(apply, b, lam=lam, rtol=rtol, max_iter=100, dtype=Zc)
            tr = CG.true_residual(A, lam, x, b)
            print(f"CG converged {Z} N={Ns} {route} lam={lam:.3g}: {it} iterations (reference {ref['iterations']}), true residual / rtol {tr / rtol:.3f}")
            assert st == "converged" and tr <= 2 * rtol and abs(it - ref["iterations"]) <= 1
            sol.close()
        op.close()


@pytest.mark.parametrize("Z,Ns,path,ncoils", CG_CASES)
def test_cg_modes_and_capture(Z, Ns, path, ncoils):
    from nufft_pkg import nufft
    T, Zc, _, rtol = _dt(Z)
    s = _system(Ns, ncoils)
    op = _cg_op(nufft, s, Z, path)
    b = s.b.astype(Zc)
    a = nufft.ToeplitzCG(op, maxiter=60, rtol=rtol, check_every=0)
    xa, ia, sa, ha = _solve(a, b)
    c = nufft.ToeplitzCG(op, maxiter=60, rtol=rtol, check_every=3)
    xc, ic, sc, hc = _solve(c, b)
    assert sa == "converged" and (ia, sa) == (ic, sc) and np.array_equal(ha, hc, equal_nan=True) and np.array_equal(xa, xc)
    bd, out = _dev(b), torch.zeros(s.shape, dtype=torch.complex128 if Z == "c128" else torch.complex64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a.solve(bd, out=out)
    for _ in range(2):
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert a.iterations[0] == ia and np.array_equal(a.history().numpy()[:, 0], ha, equal_nan=True)
        assert np.array_equal(out.cpu().numpy(), xa)
    del graph


@pytest.mark.parametrize("Z,shape,ncoils", [("c64", (9, 15), 1), ("c64", (9, 15), 3), ("c128", (32, 32, 32), 3), ("c64", (0,), 2)])
def test_coil_expand_and_combine(Z, shape, ncoils):
    from nufft_pkg import nufft
    T, Zc, _, _ = _dt(Z)
    eps = float(np.finfo(T).eps) / 2
    rng = np.random.default_rng(5)
    maps = S.smooth_maps(ncoils, shape, seed=6, zero_region=ncoils > 1).astype(Zc) if 0 not in shape else np.zeros((ncoils,) + shape, Zc)
    x = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(Zc)
    a = (rng.standard_normal((ncoils,) + shape) + 1j * rng.standard_normal((ncoils,) + shape)).astype(Zc)
    md, xd, ad = _dev(maps), _dev(x), _dev(a)
    e1 = nufft.coil_expand(md, xd)
    e2 = nufft.coil_expand(tuple(md[c] for c in range(ncoils)), xd, out=torch.empty_like(e1))
    c1 = nufft.coil_combine(md, ad)
    c2 = nufft.coil_combine(md, tuple(ad[c] for c in range(ncoils)), out=torch.empty_like(c1))
    torch.cuda.synchronize()
    assert tuple(e1.shape) == (ncoils,) + shape and tuple(c1.shape) == shape and e1.dtype == c1.dtype == xd.dtype
    assert torch.equal(e1, e2) and torch.equal(c1, c2)                            # two runs, same bits
    if 0 in shape:
        return
    m128, x128, a128 = maps.astype(np.complex128), x.astype(np.complex128), a.astype(np.complex128)
    err_e = np.linalg.norm((e1.cpu().numpy() - m128 * x128).ravel())
    bound_e = 1.01 * np.sqrt(2) * 2 * eps * np.linalg.norm((np.abs(m128) * np.abs(x128)).ravel())
    err_c = np.linalg.norm((c1.cpu().numpy() - np.sum(np.conj(m128) * a128, axis=0)).ravel())
    bound_c = 1.01 * np.sqrt(2) * (ncoils + 1) * eps * np.linalg.norm(np.sum(np.abs(m128) * np.abs(a128), axis=0).ravel())
    print(f"coil passes {Z} {shape} {ncoils} coils: expand {err_e:.3e} (bound {bound_e:.3e}), combine {err_c:.3e} (bound {bound_c:.3e})")
    assert err_e <= bound_e and err_c <= bound_c
    assert np.array_equal(md.cpu().numpy(), maps) and np.array_equal(xd.cpu().numpy(), x) and np.array_equal(ad.cpu().numpy(), a)


def test_refusals():
    from nufft_pkg import nufft
    L, lib = nufft._lib, nufft.lib
    Ns = (48, 40)
    xs, w, us, maps = _problem(Ns, np.float64, 1, seed=2, ncoils=2)
    _, op = _op(nufft, "c128", Ns, "fused")
    op.set_points(tuple(_dev(x) for x in xs), _dev(w))
    md, ud = _dev(maps), _dev(us[0])
    op.set_maps(md)
    good = op(ud).cpu().numpy()

    def still_works():
        assert op.ncoils == 2 and np.array_equal(op(ud).cpu().numpy(), good)

    for bad, exc in ((md.to(torch.complex64), ValueError), (md[:, :, :-1].contiguous(), nufft.DimensionMismatch),
                     (md[:, :-1].contiguous(), nufft.DimensionMismatch), (md.cpu(), ValueError), (md.transpose(1, 2), ValueError),
                     (torch.empty((2, 48, 40), dtype=md.dtype, device="cuda").transpose(1, 2), ValueError),
                     ((md[0], md[1].cpu()), ValueError), ((md[0], md[1].t().contiguous().t()), ValueError), ((), ValueError), ([], ValueError)):
        with pytest.raises(exc):
            op.set_maps(bad)
        still_works()
    with pytest.raises(ValueError):                                               # coil 0's store would destroy the input of coil 1
        op.apply(ud, out=ud)
    assert np.array_equal(ud.cpu().numpy(), us[0])
    still_works()
    # the C entry points directly
    st = op._stream()
    tab = lambda *p: (C.c_void_p * len(p))(*p)      # noqa: E731
    out = torch.zeros_like(ud)
    assert lib.nufft_toeplitz_apply(op._handle, tab(ud.data_ptr()), tab(ud.data_ptr()), st) == L.ERR_INVALID_ARG
    assert lib.nufft_toeplitz_set_maps(op._handle, 2, tab(md[0].data_ptr(), md[1].data_ptr() + 8), st) == L.ERR_INVALID_ARG
    assert lib.nufft_toeplitz_set_maps(op._handle, 2, tab(md[0].data_ptr(), 0), st) == L.ERR_INVALID_ARG
    assert lib.nufft_toeplitz_set_maps(op._handle, 0, tab(md[0].data_ptr()), st) == L.ERR_INVALID_ARG
    assert lib.nufft_toeplitz_set_maps(op._handle, 2, None, st) == L.ERR_INVALID_ARG
    assert lib.nufft_coil_combine(L.F64, ud.numel(), 2, out.data_ptr() + 8, tab(md[0].data_ptr(), md[1].data_ptr()),
                                  tab(md[0].data_ptr(), md[1].data_ptr()), 0, st) == L.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert not out.any()
    still_works()
    op.close()
    assert op.ncoils == 0
    with pytest.raises(ValueError):
        op.set_maps(md)
    with pytest.raises(ValueError):
        op.apply(ud)
    with pytest.raises(ValueError):
        op.clear_maps()


def test_workspace_bytes():
    from nufft_pkg import nufft
    pad = lambda v: (max(v, 16) + 255) // 256 * 256      # noqa: E731
    for Z, Ns, path in (("c128", (32, 32, 32), "fused"), ("c64", (48, 40), "fused"), ("c128", (15, 9), "dense")):
        Zc = _dt(Z)[1]
        maps = _dev(S.smooth_maps(2, Ns[::-1]).astype(Zc))
        for route in _routes(path):
            _, op = _op(nufft, Z, Ns, path, route[1])
            before = op.info().workspace_bytes
            op.set_maps(maps)
            grown = op.info().workspace_bytes - before
            assert grown == (pad(int(np.prod(Ns)) * np.dtype(Zc).itemsize) if route == ("fused", 0) else 0), (route, grown)
            op.set_maps(maps)                                                     # redone: the scratch array is kept, not doubled
            assert op.info().workspace_bytes == before + grown
            op.clear_maps()
            assert op.info().workspace_bytes == before
            op.close()
