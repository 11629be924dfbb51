"""Toeplitz normal operator on the GPU, against the exact Gram product nudft_type1(w · nudft_type2(û)) from direct sums on the CPU.

Every case asserts the apply path it runs (fused or dense): none may silently fall to the other.  Bars:
  * exact spectrum: the project's GPU-vs-exact parity bars, rel-L2 <= 1e-12 (ComplexF64) / 1e-5 (ComplexF32);
  * built from points: relative to the composed route exec_type1(w · exec_type2(û)) measured in the same test against the same
    exact product: err_toeplitz <= 3 err_composed (ComplexF64), <= max(5 err_composed, 1e-4) (ComplexF32).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import toeplitz_reference as R  # noqa: E402
from oracle import nufft_oracle as O  # noqa: E402

NP = 2000


def _dt(Z):
    return (np.float64, np.complex128, 1e-12) if Z == "c128" else (np.float32, np.complex64, 1e-5)


def _problem(Ns, T, C=1, seed=0, clustered=False):
    rng = np.random.default_rng(seed)
    xs = [(rng.random(NP) * 2 * np.pi).astype(T) for _ in Ns]
    if clustered:
        xs = [np.mod(np.pi + 0.3 * rng.standard_normal(NP), 2 * np.pi).astype(T) for _ in Ns]
    w = (rng.random(NP) + 0.1).astype(T)
    us = [rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1]) for _ in range(C)]
    return xs, w, us


def _plan(nufft, Z, Ns, path, **kw):
    opts = {"NUFFT_TOEPLITZ_FUSED": 0} if path == "dense" else {}
    return nufft.PlanNUFFT(np.complex128 if Z == "c128" else np.complex64, Ns, backend=nufft.ROCBackend(0), options=opts, **kw)


def _op(nufft, Z, Ns, path, **kw):
    plan = _plan(nufft, Z, Ns, path, **kw)
    op = nufft.ToeplitzOperator(plan)
    assert op.path == path, (Ns, path, op.path)
    return plan, op


def _dev(a, Zc=None):
    t = torch.from_numpy(np.ascontiguousarray(a if Zc is None else a.astype(Zc)))
    return t.cuda()


# (Z, N, fftshift, paths, ntransforms)
EXACT_CASES = [
    ("c128", (64,), False, ("dense",), 1),                      # 1-D is always dense
    ("c128", (100,), True, ("dense",), 1),
    ("c64", (64,), True, ("dense",), 1),
    ("c128", (33,), False, ("dense",), 1),                      # odd
    ("c128", (48, 40), False, ("fused", "dense"), 1),
    ("c128", (48, 40), True, ("fused", "dense"), 2),
    ("c64", (48, 40), False, ("fused", "dense"), 1),
    ("c64", (32, 32), True, ("fused", "dense"), 2),
    ("c128", (15, 9), True, ("dense",), 1),                     # odd, outside the table
    ("c128", (32, 32, 32), False, ("fused", "dense"), 1),
    ("c128", (32, 32, 32), True, ("fused", "dense"), 1),
    ("c64", (32, 32, 32), False, ("fused", "dense"), 2),
    ("c128", (48, 32, 40), False, ("fused", "dense"), 1),       # non-cubic fused size
    ("c64", (48, 32, 40), True, ("fused",), 1),
    ("c128", (33, 32, 32), False, ("dense",), 1),               # one size outside the table: the whole apply is dense
    ("c128", (9, 7, 5), True, ("dense",), 1),
]


@pytest.mark.parametrize("Z,Ns,fftshift,paths,C", EXACT_CASES)
def test_exact_spectrum(Z, Ns, fftshift, paths, C):
    from nufft_pkg import nufft
    T, Zc, bar = _dt(Z)
    xs, w, us = _problem(Ns, T, C, seed=len(Ns) + C)
    x64 = [x.astype(np.float64) for x in xs]
    w64 = w.astype(np.float64)
    us = [u.astype(Zc) for u in us]
    spec = R.exact_spectrum(Ns, x64, w64)
    refs = [R.exact_gram(Ns, x64, w64, u.astype(np.complex128), fftshift) for u in us]
    got = {}
    for path in paths:
        plan, op = _op(nufft, Z, Ns, path, fftshift=fftshift, ntransforms=C)
        op.set_spectrum(_dev(spec, Zc))
        plan.close()                                            # the operator keeps no pointer to the plan
        ud = tuple(_dev(u) for u in us)
        out = op.apply(ud if C > 1 else ud[0])
        out = out if C > 1 else (out,)
        torch.cuda.synchronize()
        got[path] = [o.cpu().numpy() for o in out]
        for c in range(C):
            err = R.rel(got[path][c], refs[c])
            print(f"exact spectrum {Z} N={Ns} shift={fftshift} {path} c={c}: rel-L2 {err:.3e} (bar {bar:g})")
            assert err <= bar
        # in place: out is in
        res = op.apply(ud if C > 1 else ud[0], out=ud if C > 1 else ud[0])
        torch.cuda.synchronize()
        res = res if C > 1 else (res,)
        for c in range(C):
            assert res[c].data_ptr() == ud[c].data_ptr()
            assert np.array_equal(res[c].cpu().numpy(), got[path][c])
        k = op.multiplier()
        assert k.dtype == (torch.float64 if Z == "c128" else torch.float32) and not k.is_complex()
        assert tuple(k.shape) == tuple(2 * n for n in reversed(Ns))
        kref = R.multiplier(Ns, spec).real
        assert R.rel(k.cpu().numpy(), kref) <= bar
    if len(paths) == 2:
        for c in range(C):
            err = R.rel(got["fused"][c], got["dense"][c])
            print(f"  fused vs dense c={c}: {err:.3e}")
            assert err <= bar


_KERNELS = {"bkb": "BackwardsKaiserBesselKernel", "kb": "KaiserBesselKernel", "gauss": "GaussianKernel", "bspline": "BSplineKernel"}

# (Z, N, kernel, m, point convention, path, clustered points)
POINT_CASES = [(Z, Ns, kern, m, conv, path, False)
               for Z in ("c128", "c64")
               for Ns, path in (((32, 32, 32), "fused"), ((48, 40), "fused"), ((100,), "dense"))
               for kern, m in (("bkb", 4), ("kb", 4), ("gauss", 4), ("bspline", 4), ("bkb", 8))
               for conv in (None, "nfft")
               if not (conv == "nfft" and (kern not in ("bkb",) or len(Ns) == 1))]
POINT_CASES += [("c128", (32, 32, 32), "bkb", 4, None, "fused", True), ("c128", (48, 40), "bkb", 8, None, "dense", True),
                ("c64", (32, 32, 32), "bkb", 4, None, "dense", False)]


@pytest.mark.parametrize("Z,Ns,kern,m,conv,path,clustered", POINT_CASES)
def test_built_from_points(Z, Ns, kern, m, conv, path, clustered):
    from nufft_pkg import nufft
    T, Zc, _ = _dt(Z)
    xs, w, us = _problem(Ns, T, 1, seed=7 + m, clustered=clustered)
    if clustered:
        w = (w * np.where(np.arange(NP) % 50 == 0, 40.0, 1.0)).astype(T)       # uneven weights on top
    u = us[0].astype(Zc)
    if conv == "nfft":
        pts = [(x / (2 * np.pi) - 0.5).astype(T) for x in xs]                 # [-1/2, 1/2)
        x64 = [O.nfft_point_convention(p.astype(np.float64)) for p in pts]
    else:
        pts = xs
        x64 = [x.astype(np.float64) for x in xs]
    ref = R.exact_gram(Ns, x64, w.astype(np.float64), u.astype(np.complex128))
    plan, op = _op(nufft, Z, Ns, path, m=m, kernel=getattr(nufft, _KERNELS[kern])(), point_transform=conv)
    pd = tuple(_dev(p) for p in pts)
    wd, ud = _dev(w), _dev(u)
    # the composed route on the plan's own (unchanged) code paths
    nufft.set_points(plan, pd)
    v = torch.empty(NP, dtype=plan.Z, device="cuda")
    nufft.exec_type2(v, plan, ud)
    v *= wd
    gc = torch.empty_like(ud)
    nufft.exec_type1(gc, plan, v)
    torch.cuda.synchronize()
    err_c = R.rel(gc.cpu().numpy(), ref)
    op.set_points(pd, wd)
    gt = op(ud)
    torch.cuda.synchronize()
    err_t = R.rel(gt.cpu().numpy(), ref)
    print(f"from points {Z} N={Ns} {kern} m={m} conv={conv} {path} clustered={clustered}: toeplitz {err_t:.3e}, composed {err_c:.3e}, "
          f"ratio {err_t / err_c:.2f}")
    if Z == "c128":
        assert err_t <= 3 * err_c
    else:
        assert err_t <= max(5 * err_c, 1e-4)


def test_build_overrides_change_the_accuracy():
    from nufft_pkg import nufft
    Ns = (48, 40)
    xs, w, us = _problem(Ns, np.float64, 1, seed=5)
    ref = R.exact_gram(Ns, xs, w, us[0])
    plan, op = _op(nufft, "c128", Ns, "fused", m=4)
    pd, wd, ud = tuple(_dev(x) for x in xs), _dev(w), _dev(us[0])
    e4 = R.rel(op.set_points(pd, wd)(ud).cpu().numpy(), ref)
    e8 = R.rel(op.set_points(pd, wd, m=8)(ud).cpu().numpy(), ref)
    e1 = R.rel(op.set_points(pd, None)(ud).cpu().numpy(), R.exact_gram(Ns, xs, np.ones(NP), us[0]))      # weights = None: ones
    print(f"build m=4: {e4:.3e}, m=8: {e8:.3e}, unit weights: {e1:.3e}")
    assert e8 < 1e-2 * e4 and e4 < 1e-5 and e1 < 1e-5


@pytest.mark.parametrize("Ns,path", [((32, 32, 32), "fused"), ((48, 40), "fused"), ((48, 40), "dense"), ((100,), "dense")])
def test_properties(Ns, path):
    from nufft_pkg import nufft
    xs, w, us = _problem(Ns, np.float64, 2, seed=11)
    plan, op = _op(nufft, "c128", Ns, path)
    op.set_points(tuple(_dev(x) for x in xs), _dev(w))          # w >= 0
    a, b = us
    Ga, Gb = op(_dev(a)).cpu().numpy(), op(_dev(b)).cpu().numpy()
    ip = np.vdot(a, Ga)                                         # <a, G a>
    assert ip.real >= 0
    assert abs(ip.imag) <= 1e-12 * np.linalg.norm(a) * np.linalg.norm(Ga)
    lhs, rhs = np.vdot(a, Gb), np.conj(np.vdot(b, Ga))          # <a, G b> = conj <b, G a>
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(a) * np.linalg.norm(Gb)
    k = op.multiplier()
    assert k.dtype == torch.float64 and tuple(k.shape) == tuple(2 * n for n in reversed(Ns))


def test_second_point_set_replaces_the_operator_and_memory_returns():
    from nufft_pkg import nufft
    Ns = (32, 32, 32)
    plan, op = _op(nufft, "c128", Ns, "fused")
    x1, w1, us = _problem(Ns, np.float64, 1, seed=1)
    x2, w2, _ = _problem(Ns, np.float64, 1, seed=2)
    ud = _dev(us[0])
    with pytest.raises(ValueError):                             # NUFFT_ERR_NO_POINTS before any spectrum
        op(ud)
    before = op.info().workspace_bytes
    p1, p2, wd1, wd2 = tuple(_dev(x) for x in x1), tuple(_dev(x) for x in x2), _dev(w1), _dev(w2)
    g1 = op.set_points(p1, wd1)(ud).cpu().numpy()
    assert op.info().workspace_bytes == before                  # the internal 2N plan and the temporaries are gone
    # device memory around the second build (the first one also loads code objects and rocFFT kernels, which stay)
    gd = torch.empty_like(ud)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    op.set_points(p2, wd2)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20)    # the 2N plan (a 128^3 ComplexF64 grid alone is 33 MB) has been freed
    assert op.info().workspace_bytes == before
    g2 = op.apply(ud, out=gd).cpu().numpy()
    e1 = R.rel(g1, R.exact_gram(Ns, x1, w1, us[0]))
    e2 = R.rel(g2, R.exact_gram(Ns, x2, w2, us[0]))
    assert e1 < 1e-5 and e2 < 1e-5 and R.rel(g2, g1) > 1e-2
    plan.close()                                                # the parent plan may be destroyed before apply
    g2b = op(ud).cpu().numpy()
    assert np.array_equal(g2b, g2)


@pytest.mark.parametrize("Z,Ns,path", [("c128", (32, 32, 32), "fused"), ("c64", (48, 40), "fused"), ("c128", (48, 40), "dense"),
                                       ("c128", (100,), "dense")])
def test_stream_and_graph(Z, Ns, path):
    from nufft_pkg import nufft
    T, Zc, _ = _dt(Z)
    xs, w, _ = _problem(Ns, T, 1, seed=4)
    plan, op = _op(nufft, Z, Ns, path)
    pd, wd = tuple(_dev(x) for x in xs), _dev(w)
    op.set_points(pd, wd)
    rng = np.random.default_rng(9)
    new = lambda: (rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1])).astype(Zc)      # noqa: E731
    u0 = new()
    ud = _dev(u0)
    eager = op(ud).cpu().numpy()
    # a non-default stream
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = op(ud)
    s.synchronize()
    assert np.array_equal(side.cpu().numpy(), eager)
    # apply alone in a hipGraph, replayed with changed input
    out = torch.empty_like(ud)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        op.apply(ud, out=out)
        with pytest.raises(ValueError):                         # set_points on a capturing stream is refused
            op.set_points(pd, wd)
    assert op.info().has_spectrum == 1                          # ... before it touched the operator
    for _ in range(3):
        u = new()
        ud.copy_(torch.from_numpy(u))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        ref = op(ud).cpu().numpy()
        assert np.array_equal(got, ref)
    del graph


def test_nfft_plan_toeplitz_constructor():
    from nufft_pkg import nufft
    Ns = (32, 40)
    rng = np.random.default_rng(2)
    x = rng.random((NP, 2)) - 0.5
    w = rng.random(NP) + 0.1
    u = rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1])
    p = nufft.plan_nfft(_dev(x), Ns, m=6)
    op = p.toeplitz(_dev(w))
    assert op.path == "fused"
    g = op(_dev(u))
    v = p.mul(_dev(u)) * _dev(w)
    gc = p.adjoint_mul(v)
    torch.cuda.synchronize()
    assert R.rel(g.cpu().numpy(), gc.cpu().numpy()) < 1e-7
