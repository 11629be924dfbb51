"""Type-3 transforms (nonuniform to nonuniform) on the GPU against direct sums in numpy complex128.

The accuracy bar is calibrated, not guessed: a case passes when its rel-L2 error is at most 5x the rel-L2 error of a type-1 plan of the
same (M, σ, kernel, precision) against its own direct sums (ComplexF32: at least 1e-4).  Float32 cases sum the same Float32-rounded
inputs the plan receives.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RATIO = 5.0


def _nufft():
    from nufft_pkg import nufft
    return nufft


def _rel(a, b):
    b = np.asarray(b)
    return float(np.linalg.norm(np.asarray(a) - b) / max(np.linalg.norm(b), 1e-300))


def _direct3(x, s, c, sign):
    """f_k = Σ_j c_j exp(sign i s_k·x_j); x (Np, D), s (Nk, D) in float64."""
    if x.shape[0] == 0:
        return np.zeros(s.shape[0], dtype=np.complex128)
    return np.exp(sign * 1j * (s.astype(np.float64) @ x.astype(np.float64).T)) @ c.astype(np.complex128)


def _kernel(name):
    nufft = _nufft()
    return {"bkb": nufft.BackwardsKaiserBesselKernel, "kb": nufft.KaiserBesselKernel,
            "gauss": nufft.GaussianKernel, "bspline": nufft.BSplineKernel}[name]()


def _real(Z):
    return np.float32 if np.dtype(Z) == np.complex64 else np.float64


def _torch_dtype(Z):
    return torch.complex64 if np.dtype(Z) == np.complex64 else torch.complex128


@functools.lru_cache(maxsize=None)
def _type1_error(Z, M, sigma, kernel):
    """rel-L2 of a 2-D type-1 plan (32 x 32 modes, 2000 points) with these parameters against its direct sums."""
    nufft = _nufft()
    T = _real(Z)
    rng = np.random.default_rng(123)
    N, Np = 32, 2000
    x = (rng.random((Np, 2)) * 2 * np.pi).astype(T)
    c = (rng.standard_normal(Np) + 1j * rng.standard_normal(Np)).astype(Z)
    plan = nufft.PlanNUFFT(_torch_dtype(Z), (N, N), m=M, sigma=sigma, kernel=_kernel(kernel), backend=nufft.ROCBackend(0))
    nufft.set_points(plan, tuple(torch.from_numpy(np.ascontiguousarray(x[:, d])).cuda() for d in range(2)))
    u = torch.empty(plan.shape, dtype=_torch_dtype(Z), device="cuda")
    nufft.exec_type1(u, plan, torch.from_numpy(c).cuda())
    k = np.fft.fftfreq(N) * N
    k1, k2 = np.meshgrid(k, k, indexing="xy")          # array [i2, i1]: k1 along the last axis
    modes = np.stack([k1.ravel(), k2.ravel()], axis=1)
    ref = _direct3(x, modes, c, -1).reshape(N, N)
    return _rel(u.cpu().numpy(), ref)


def _bar(Z, M, sigma, kernel):
    e = RATIO * _type1_error(Z, M, sigma, kernel)
    return max(e, 1e-4) if np.dtype(Z) == np.complex64 else e


def _run(Z, x, s, c, *, M=4, sigma=2.0, kernel="bkb", sign=-1, ntransforms=1, bounds=None):
    """Plan from the point sets' bounding boxes (or `bounds`), one set_points3 + exec_type3; returns (f, plan)."""
    nufft = _nufft()
    xd = tuple(torch.from_numpy(np.ascontiguousarray(x[:, d])).cuda() for d in range(x.shape[1]))
    sd = tuple(torch.from_numpy(np.ascontiguousarray(s[:, d])).cuda() for d in range(s.shape[1]))
    kw = dict(m=M, sigma=sigma, kernel=_kernel(kernel), sign=sign, ntransforms=ntransforms, backend=nufft.ROCBackend(0))
    if bounds is None:
        plan = nufft.PlanNUFFT3.from_points(_torch_dtype(Z), xd, sd, **kw)
    else:
        plan = nufft.PlanNUFFT3(_torch_dtype(Z), x.shape[1], source_bounds=bounds[0], target_bounds=bounds[1], **kw)
    nufft.set_points3(plan, xd, sd)
    cs = c if isinstance(c, (list, tuple)) else [c]
    fs = [torch.empty(s.shape[0], dtype=_torch_dtype(Z), device="cuda") for _ in cs]
    nufft.exec_type3(fs if ntransforms > 1 else fs[0], plan, [torch.from_numpy(ci).cuda() for ci in cs] if ntransforms > 1
                     else torch.from_numpy(cs[0]).cuda())
    out = [f.cpu().numpy() for f in fs]
    return (out if ntransforms > 1 else out[0]), plan


def _random_case(rng, D, Z, Np=2000, Nk=2000, xc=None, sc=None):
    T = _real(Z)
    xc = rng.uniform(-5, 5, D) if xc is None else np.asarray(xc, dtype=np.float64)
    sc = rng.uniform(-20, 20, D) if sc is None else np.asarray(sc, dtype=np.float64)
    X = rng.uniform(1.0, 4.0, D)
    S = rng.uniform(5.0, 40.0 if D < 3 else 12.0, D)
    x = (xc + X * rng.uniform(-1, 1, (Np, D))).astype(T)
    s = (sc + S * rng.uniform(-1, 1, (Nk, D))).astype(T)
    c = (rng.standard_normal(Np) + 1j * rng.standard_normal(Np)).astype(Z)
    return x, s, c


CASES = [(D, Z, "bkb") for D in (1, 2, 3) for Z in (np.complex128, np.complex64)] + \
        [(2, Z, k) for Z in (np.complex128, np.complex64) for k in ("kb", "gauss", "bspline")]


@pytest.mark.parametrize("D,Z,kernel", CASES)
def test_random_boxes_against_direct_sums(D, Z, kernel):
    rng = np.random.default_rng(10 * D + len(kernel))
    x, s, c = _random_case(rng, D, Z)
    f, plan = _run(Z, x, s, c, kernel=kernel)
    err = _rel(f, _direct3(x, s, c, -1))
    bar = _bar(Z, 4, 2.0, kernel)
    print(f"type 3 D={D} {np.dtype(Z)} {kernel}: rel-L2 {err:.3e}, type-1 {_type1_error(Z, 4, 2.0, kernel):.3e}, "
          f"ratio {err / _type1_error(Z, 4, 2.0, kernel):.2f}, nf {plan.nf}")
    assert plan.points_outside() == (0, 0)
    assert err <= bar, (err, bar)


def test_large_centres_float32():
    """|C| ≈ 200, |D| ≈ 500: s·C ≈ 1e5 rad.  Phases formed in Float32 would miss the bar by orders of magnitude."""
    Z = np.complex64
    rng = np.random.default_rng(7)
    x, s, c = _random_case(rng, 2, Z, xc=[200.0, -190.0], sc=[500.0, -480.0])
    f, _ = _run(Z, x, s, c)
    err = _rel(f, _direct3(x, s, c, -1))
    print(f"type 3 large centres ComplexF32: rel-L2 {err:.3e}")
    assert err <= _bar(Z, 4, 2.0, "bkb"), err


def test_convergence_in_m():
    rng = np.random.default_rng(11)
    x, s, c = _random_case(rng, 2, np.complex128)
    ref = _direct3(x, s, c, -1)
    e4 = _rel(_run(np.complex128, x, s, c, M=4)[0], ref)
    e8 = _rel(_run(np.complex128, x, s, c, M=8)[0], ref)
    print(f"type 3 convergence: M=4 {e4:.3e}, M=8 {e8:.3e}")
    assert e8 * 1e3 <= e4, (e4, e8)


@pytest.mark.parametrize("D", [2, 3])
def test_integer_targets_reduce_to_type1(D):
    nufft = _nufft()
    N = 16 if D == 3 else 24
    rng = np.random.default_rng(D)
    Np = 2000
    x = rng.random((Np, D)) * 2 * np.pi
    c = rng.standard_normal(Np) + 1j * rng.standard_normal(Np)
    k = np.fft.fftfreq(N) * N
    grids = np.meshgrid(*([k] * D), indexing="ij")          # [i1, i2, (i3)]
    modes = np.stack([g.ravel() for g in grids], axis=1).astype(np.float64)
    f, _ = _run(np.complex128, x, modes, c)
    plan = nufft.PlanNUFFT(torch.complex128, (N,) * D, m=4, sigma=2.0, backend=nufft.ROCBackend(0))
    nufft.set_points(plan, tuple(torch.from_numpy(np.ascontiguousarray(x[:, d])).cuda() for d in range(D)))
    u = torch.empty(plan.shape, dtype=torch.complex128, device="cuda")
    nufft.exec_type1(u, plan, torch.from_numpy(c).cuda())
    u1 = u.cpu().numpy().transpose(tuple(reversed(range(D)))).ravel()      # torch [iD..i1] -> [i1..iD], same order as `modes`
    bar = 2 * _bar(np.complex128, 4, 2.0, "bkb")
    assert _rel(f, u1) <= bar
    assert _rel(f, _direct3(x, modes, c, -1)) <= _bar(np.complex128, 4, 2.0, "bkb")


def test_integer_sources_with_plus_sign_reduce_to_type2():
    nufft = _nufft()
    N, D, Nk = 24, 2, 2000
    rng = np.random.default_rng(5)
    k = np.fft.fftfreq(N) * N
    grids = np.meshgrid(k, k, indexing="ij")
    srcs = np.stack([g.ravel() for g in grids], axis=1)          # [i1, i2] order
    uhat = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))       # [i1, i2]
    s = rng.random((Nk, D)) * 2 * np.pi
    f, _ = _run(np.complex128, srcs, s, uhat.ravel().copy(), sign=+1)
    plan = nufft.PlanNUFFT(torch.complex128, (N, N), m=4, sigma=2.0, backend=nufft.ROCBackend(0))
    nufft.set_points(plan, tuple(torch.from_numpy(np.ascontiguousarray(s[:, d])).cuda() for d in range(D)))
    v = torch.empty(Nk, dtype=torch.complex128, device="cuda")
    nufft.exec_type2(v, plan, torch.from_numpy(np.ascontiguousarray(uhat.T)).cuda())      # torch shape (N2, N1)
    assert _rel(f, v.cpu().numpy()) <= 2 * _bar(np.complex128, 4, 2.0, "bkb")


def test_sign_symmetry():
    rng = np.random.default_rng(9)
    x, s, c = _random_case(rng, 2, np.complex128)
    bounds = ([(float(x[:, d].min()) - 1e-9, float(x[:, d].max()) + 1e-9) for d in range(2)],
              [(float(s[:, d].min()) - 1e-9, float(s[:, d].max()) + 1e-9) for d in range(2)])
    fp, _ = _run(np.complex128, x, s, c, sign=+1, bounds=bounds)
    fm, _ = _run(np.complex128, x, s, np.conj(c), sign=-1, bounds=bounds)
    assert _rel(fp, np.conj(fm)) <= _bar(np.complex128, 4, 2.0, "bkb")
    assert _rel(fp, _direct3(x, s, c, +1)) <= _bar(np.complex128, 4, 2.0, "bkb")


def test_ntransforms_three():
    rng = np.random.default_rng(4)
    x, s, _ = _random_case(rng, 3, np.complex128)
    cs = [(rng.standard_normal(x.shape[0]) + 1j * rng.standard_normal(x.shape[0])) for _ in range(3)]
    fs, _ = _run(np.complex128, x, s, cs, ntransforms=3)
    for ci, fi in zip(cs, fs):
        single, _ = _run(np.complex128, x, s, ci)
        assert _rel(fi, single) <= 1e-12
        assert _rel(fi, _direct3(x, s, ci, -1)) <= _bar(np.complex128, 4, 2.0, "bkb")


@pytest.mark.parametrize("Z", [np.complex128, np.complex64])
def test_degenerate_point_sets(Z):
    nufft = _nufft()
    T = _real(Z)
    rng = np.random.default_rng(2)
    # a set of identical sources or targets is ONE sample of the pointwise error, which scatters by a factor of a few about the
    # rel-L2 of a spread-out set: these cases get twice the calibrated bar
    bar = 2 * _bar(Z, 4, 2.0, "bkb")
    # all sources at one point
    x = np.full((500, 2), [1.5, -2.0]).astype(T)
    s = rng.uniform(-10, 10, (700, 2)).astype(T)
    c = (rng.standard_normal(500) + 1j * rng.standard_normal(500)).astype(Z)
    f, plan = _run(Z, x, s, c)
    assert np.all(np.isfinite(f)) and _rel(f, _direct3(x, s, c, -1)) <= bar
    assert all(g > 0 and np.isfinite(g) for g in plan.info().gamma[:2])
    # all targets at one point
    x = rng.uniform(-3, 3, (600, 2)).astype(T)
    s = np.full((300, 2), [4.0, 7.0]).astype(T)
    c = (rng.standard_normal(600) + 1j * rng.standard_normal(600)).astype(Z)
    f, _ = _run(Z, x, s, c)
    assert np.all(np.isfinite(f)) and _rel(f, _direct3(x, s, c, -1)) <= bar
    # a single source and a single target
    x = np.array([[0.3, -0.7]], dtype=T)
    s = np.array([[12.0, 5.0]], dtype=T)
    c = np.array([1.0 - 2.0j], dtype=Z)
    f, _ = _run(Z, x, s, c)
    assert _rel(f, _direct3(x, s, c, -1)) <= bar
    # Np = 0: zeros; Nk = 0: a no-op
    plan = nufft.PlanNUFFT3(_torch_dtype(Z), 2, backend=nufft.ROCBackend(0), source_bounds=[(-1, 1)] * 2, target_bounds=[(-5, 5)] * 2)
    empty = tuple(torch.empty(0, dtype=torch.float32 if T == np.float32 else torch.float64, device="cuda") for _ in range(2))
    sd = tuple(torch.from_numpy(rng.uniform(-5, 5, 50).astype(T)).cuda() for _ in range(2))
    nufft.set_points3(plan, empty, sd)
    f = torch.full((50,), 7.0, dtype=_torch_dtype(Z), device="cuda")
    nufft.exec_type3(f, plan, torch.empty(0, dtype=_torch_dtype(Z), device="cuda"))
    assert torch.count_nonzero(f).item() == 0
    xd = tuple(torch.from_numpy(rng.uniform(-1, 1, 40).astype(T)).cuda() for _ in range(2))
    nufft.set_points3(plan, xd, empty)
    out = torch.empty(0, dtype=_torch_dtype(Z), device="cuda")
    nufft.exec_type3(out, plan, torch.ones(40, dtype=_torch_dtype(Z), device="cuda"))
    torch.cuda.synchronize()
    assert plan.num_sources == 40 and plan.num_targets == 0


def test_points_outside_are_counted():
    nufft = _nufft()
    rng = np.random.default_rng(3)
    D, Np, Nk = 3, 3001, 2503
    x = rng.uniform(-1, 1, (Np, D))
    s = rng.uniform(-8, 8, (Nk, D))
    out_x = rng.choice(Np, 37, replace=False)
    out_s = rng.choice(Nk, 11, replace=False)
    x[out_x, rng.integers(0, D, 37)] = 1.5
    s[out_s, rng.integers(0, D, 11)] = -9.0
    plan = nufft.PlanNUFFT3(torch.complex128, D, backend=nufft.ROCBackend(0), source_bounds=[(-1, 1)] * D, target_bounds=[(-8, 8)] * D)
    nufft.set_points3(plan, torch.from_numpy(x).cuda(), torch.from_numpy(s).cuda())     # (Np, D) tensors
    assert plan.points_outside() == (37, 11)


def test_plan_reuse_across_point_sets():
    nufft = _nufft()
    rng = np.random.default_rng(8)
    bounds = ([(-3, 3), (-2, 4)], [(-10, 10), (0, 30)])
    plan = nufft.PlanNUFFT3(torch.complex128, 2, backend=nufft.ROCBackend(0), source_bounds=bounds[0], target_bounds=bounds[1])
    for Np, Nk in [(1000, 800), (3000, 2500), (200, 3000), (2500, 100), (1, 1)]:
        x = np.stack([rng.uniform(-3, 3, Np), rng.uniform(-2, 4, Np)], axis=1)
        s = np.stack([rng.uniform(-10, 10, Nk), rng.uniform(0, 30, Nk)], axis=1)
        c = rng.standard_normal(Np) + 1j * rng.standard_normal(Np)
        nufft.set_points3(plan, torch.from_numpy(x).cuda(), torch.from_numpy(s).cuda())
        f = torch.empty(Nk, dtype=torch.complex128, device="cuda")
        nufft.exec_type3(f, plan, torch.from_numpy(c).cuda())
        fresh, _ = _run(np.complex128, x, s, c, bounds=bounds)
        assert _rel(f.cpu().numpy(), fresh) <= 1e-13


def test_graph_capture_matches_eager():
    nufft = _nufft()
    rng = np.random.default_rng(6)
    D, Np, Nk = 3, 2000, 1500
    bounds = ([(-2, 2)] * D, [(-12, 12)] * D)
    plan = nufft.PlanNUFFT3(torch.complex128, D, backend=nufft.ROCBackend(0), source_bounds=bounds[0], target_bounds=bounds[1])

    def inputs():
        return rng.uniform(-2, 2, (Np, D)), rng.uniform(-12, 12, (Nk, D)), rng.standard_normal(Np) + 1j * rng.standard_normal(Np)

    x, s, c = inputs()
    xd = tuple(torch.from_numpy(np.ascontiguousarray(x[:, d])).cuda() for d in range(D))
    sd = tuple(torch.from_numpy(np.ascontiguousarray(s[:, d])).cuda() for d in range(D))
    cd = torch.from_numpy(c).cuda()
    fd = torch.empty(Nk, dtype=torch.complex128, device="cuda")

    def step():
        nufft.set_points3(plan, xd, sd)
        nufft.exec_type3(fd, plan, cd)

    step()                  # sizes every buffer (allocation is not capturable)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(2):
        x, s, c = inputs()
        for d in range(D):
            xd[d].copy_(torch.from_numpy(x[:, d]))
            sd[d].copy_(torch.from_numpy(s[:, d]))
        cd.copy_(torch.from_numpy(c))
        fd.zero_()
        graph.replay()
        torch.cuda.synchronize()
        eager, _ = _run(np.complex128, x, s, c, bounds=bounds)
        assert _rel(fd.cpu().numpy(), eager) <= 1e-13
        assert _rel(fd.cpu().numpy(), _direct3(x, s, c, -1)) <= _bar(np.complex128, 4, 2.0, "bkb")
