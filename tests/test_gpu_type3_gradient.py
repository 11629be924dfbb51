"""Type-3 gradients with respect to the targets (nufft_exec_type3_grad) and autograd through type 3, on the GPU.

1. against exact derivative sums Σ_j c_j (σ i x_{j,d}) e^{σ i s_k·x_j}: the gradient error is a bounded multiple of the same plan's
   value error (the §14 rule; the measured ratios go into DESIGN.md §15), and the values equal exec_type3's;
2. the finish kernel against its float64 restatement (tests/type3_grad_reference.py) from the inner type-2 gradient;
3. sign, large centres, several transforms, box faces, empty sets, refusals, streams and hipGraph capture;
4. the spectral route (ntransforms = D + 1) at 2e5 points, the adjoint identity and torch.autograd.gradcheck.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import type3_grad_reference as R  # noqa: E402

RATIO = 100.0
_KERNEL_CLASS = {"bkb": "BackwardsKaiserBesselKernel", "kb": "KaiserBesselKernel", "gauss": "GaussianKernel",
                 "bspline": "BSplineKernel"}


def _nufft():
    from nufft_pkg import nufft
    return nufft


def _rel(a, b):
    b = np.asarray(b)
    return float(np.linalg.norm(np.asarray(a) - b) / max(np.linalg.norm(b), 1e-300))


def _real(Z):
    return np.float32 if np.dtype(Z) == np.complex64 else np.float64


def _tz(Z):
    return torch.complex64 if np.dtype(Z) == np.complex64 else torch.complex128


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cols(a):
    return tuple(_dev(a[:, d]) for d in range(a.shape[1]))


def _case(rng, D, Z, Np=2000, Nk=2000, xc=None, sc=None):
    """Points in random boxes with non-zero centres; returns (x, s, c, bounds) with x, s rounded to the plan's precision."""
    T = _real(Z)
    xc = rng.uniform(-5, 5, D) if xc is None else np.asarray(xc, dtype=np.float64)
    sc = rng.uniform(-20, 20, D) if sc is None else np.asarray(sc, dtype=np.float64)
    X = rng.uniform(1.0, 4.0, D)
    S = rng.uniform(5.0, 40.0 if D < 3 else 12.0, D)
    x = (xc + X * rng.uniform(-1, 1, (Np, D))).astype(T)
    s = (sc + S * rng.uniform(-1, 1, (Nk, D))).astype(T)
    c = (rng.standard_normal(Np) + 1j * rng.standard_normal(Np)).astype(Z)
    bounds = ([(xc[d] - X[d], xc[d] + X[d]) for d in range(D)], [(sc[d] - S[d], sc[d] + S[d]) for d in range(D)])
    return x, s, c, bounds


def _plan(Z, D, bounds, *, M=4, sigma=2.0, kernel="bkb", mode="direct", sign=-1, ntransforms=1):
    nufft = _nufft()
    ev = nufft.Direct() if mode == "direct" else nufft.FastApproximation()
    return nufft.PlanNUFFT3(_tz(Z), D, m=M, sigma=sigma, kernel=getattr(nufft, _KERNEL_CLASS[kernel])(), kernel_evalmode=ev,
                            sign=sign, ntransforms=ntransforms, backend=nufft.ROCBackend(0),
                            source_bounds=bounds[0], target_bounds=bounds[1])


def _grad_run(plan, x, s, c):
    """set_points3 + exec_type3_grad (one transform): (f, (Nk, D) gradients) as numpy."""
    nufft = _nufft()
    nufft.set_points3(plan, _cols(x), _cols(s))
    Nk, D = s.shape
    f = torch.empty(Nk, dtype=plan.Z, device="cuda")
    g = tuple(torch.empty(Nk, dtype=plan.Z, device="cuda") for _ in range(D))
    out = nufft.exec_type3_grad(f, g, plan, _dev(c))
    assert out[0] is f and tuple(out[1]) == g
    return f.cpu().numpy(), np.stack([gd.cpu().numpy() for gd in g], axis=1)


def _value_run(plan, c):
    nufft = _nufft()
    f = torch.empty(plan._targets[0].numel(), dtype=plan.Z, device="cuda")
    nufft.exec_type3(f, plan, _dev(c))
    return f.cpu().numpy()


def _bar(Z, value_err):
    e = RATIO * value_err
    return max(e, 1e-3) if np.dtype(Z) == np.complex64 else e


CASES = [(D, Z, k, m) for D in (1, 2, 3) for Z in (np.complex128, np.complex64) for k in R.KERNELS
         for m in ("direct", "fast")]


@pytest.mark.parametrize("D,Z,kernel,mode", CASES)
def test_random_boxes_against_exact_derivative_sums(D, Z, kernel, mode):
    rng = np.random.default_rng(100 + 7 * D + (3 if Z == np.complex64 else 0) + R.KERNELS.index(kernel) * 11 + (mode == "fast"))
    x, s, c, bounds = _case(rng, D, Z)
    plan = _plan(Z, D, bounds, kernel=kernel, mode=mode)
    f, g = _grad_run(plan, x, s, c)
    ef = _rel(f, R.direct3(x, s, c, -1))
    eg = _rel(g, R.direct3_grad(x, s, c, -1))
    print(f"D={D} {np.dtype(Z).name} {kernel} {mode}: value {ef:.3e}, gradient {eg:.3e}, ratio {eg / ef:.2f}")
    assert eg <= _bar(Z, ef), (ef, eg)
    # the values are exec_type3's
    fv = _value_run(plan, c)
    assert _rel(f, fv) <= (1e-12 if Z == np.complex128 else 1e-5)


@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("D", [1, 3])
def test_finish_kernel_matches_float64_restatement(kernel, D):
    """f = P v and ∂f/∂s from the inner type-2 gradient at θ (read from the spreading plan's grid), the numpy post factor and ρ."""
    nufft = _nufft()
    rng = np.random.default_rng(40 + D + 3 * R.KERNELS.index(kernel))
    x, s, c, bounds = _case(rng, D, np.complex128)
    sign = 1 if kernel == "kb" else -1
    plan = _plan(np.complex128, D, bounds, kernel=kernel, sign=sign)
    f, g = _grad_run(plan, x, s, c)
    Nk = s.shape[0]
    # the inner type-2 gradient, again, from the spread grid the last exec left
    sp, t2 = plan._internal(0), plan._internal(1)
    us = C.c_void_p()
    assert nufft.lib.nufft_grid_ptr(sp, 0, 0, C.byref(us), None) == 0
    v = torch.empty(Nk, dtype=torch.complex128, device="cuda")
    dv = tuple(torch.empty(Nk, dtype=torch.complex128, device="cuda") for _ in range(D))
    vt = (C.c_void_p * 1)(v.data_ptr())
    gt = (C.c_void_p * D)(*[t.data_ptr() for t in dv])
    ut = (C.c_void_p * 1)(us.value)
    assert nufft.lib.nufft_exec_type2_grad(t2, vt, gt, ut, plan._stream()) == 0
    torch.cuda.synchronize()
    info, spi = plan.info(), plan.internal_info(0)
    h = [info.h[d] for d in range(D)]
    gamma = [info.gamma[d] for d in range(D)]
    beta = [spi.beta[d] for d in range(D)]
    param = [2.0 * (beta[d] * h[d]) ** 2 for d in range(D)] if kernel == "gauss" else beta
    src_c = [0.5 * (lo + hi) for lo, hi in bounds[0]]
    tgt_c = [0.5 * (lo + hi) for lo, hi in bounds[1]]
    P, rho = R.post_factor(kernel, plan._M, sign, s, src_c, tgt_c, gamma, h, param, [spi.window_scale_log2[d] for d in range(D)])
    theta_scale = [sign * gamma[d] * h[d] for d in range(D)]
    fr, gr = R.finish(P, rho, v.cpu().numpy(), [t.cpu().numpy() for t in dv], sign, src_c, theta_scale)
    assert _rel(f, fr) <= 1e-12
    assert _rel(g, np.stack(gr, axis=1)) <= 1e-12


def test_sign_plus_one():
    rng = np.random.default_rng(7)
    x, s, c, bounds = _case(rng, 2, np.complex128)
    plan = _plan(np.complex128, 2, bounds, sign=1)
    f, g = _grad_run(plan, x, s, c)
    ef = _rel(f, R.direct3(x, s, c, 1))
    eg = _rel(g, R.direct3_grad(x, s, c, 1))
    assert eg <= _bar(np.complex128, ef), (ef, eg)


def test_large_centres_float32():
    # |C| ≈ 200, |D| ≈ 500: the sign i C_d term dominates the derivative; phases and ρ are formed in FP64
    rng = np.random.default_rng(8)
    x, s, c, bounds = _case(rng, 2, np.complex64, xc=[200.0, -150.0], sc=[-500.0, 420.0])
    plan = _plan(np.complex64, 2, bounds)
    f, g = _grad_run(plan, x, s, c)
    ef = _rel(f, R.direct3(x, s, c, -1))
    eg = _rel(g, R.direct3_grad(x, s, c, -1))
    print(f"large centres ComplexF32: value {ef:.3e}, gradient {eg:.3e}")
    assert eg <= _bar(np.complex64, ef), (ef, eg)


def test_ntransforms_three():
    nufft = _nufft()
    rng = np.random.default_rng(9)
    x, s, c0, bounds = _case(rng, 3, np.complex128, Np=1500, Nk=1200)
    cs = [c0] + [(rng.standard_normal(1500) + 1j * rng.standard_normal(1500)) for _ in range(2)]
    plan = _plan(np.complex128, 3, bounds, ntransforms=3)
    nufft.set_points3(plan, _cols(x), _cols(s))
    fs = [torch.empty(1200, dtype=torch.complex128, device="cuda") for _ in cs]
    gs = tuple(tuple(torch.empty(1200, dtype=torch.complex128, device="cuda") for _ in range(3)) for _ in cs)
    nufft.exec_type3_grad(fs, gs, plan, [_dev(ci) for ci in cs])
    for i, ci in enumerate(cs):
        ef = _rel(fs[i].cpu().numpy(), R.direct3(x, s, ci, -1))
        eg = _rel(np.stack([t.cpu().numpy() for t in gs[i]], axis=1), R.direct3_grad(x, s, ci, -1))
        assert eg <= _bar(np.complex128, ef), (i, ef, eg)


@pytest.mark.parametrize("Z", [np.complex128, np.complex64])
def test_targets_on_box_faces_and_centre(Z):
    rng = np.random.default_rng(10)
    D = 2
    T = _real(Z)
    xc, X, sc, S = np.array([1.5, -2.0]), np.array([3.0, 2.0]), np.array([-7.0, 12.0]), np.array([20.0, 9.0])
    bounds = ([(xc[d] - X[d], xc[d] + X[d]) for d in range(D)], [(sc[d] - S[d], sc[d] + S[d]) for d in range(D)])
    x = (xc + X * rng.uniform(-1, 1, (1000, D))).astype(T)
    corners = np.array([[a, b] for a in (-1, 0, 1) for b in (-1, 0, 1)], dtype=np.float64)
    s = np.concatenate([sc + S * corners, sc + S * rng.uniform(-1, 1, (200, D))]).astype(T)
    c = (rng.standard_normal(1000) + 1j * rng.standard_normal(1000)).astype(Z)
    plan = _plan(Z, D, bounds)
    f, g = _grad_run(plan, x, s, c)
    ef = _rel(f, R.direct3(x, s, c, -1))
    ref = R.direct3_grad(x, s, c, -1)
    eg = _rel(g, ref)
    assert eg <= _bar(Z, ef), (ef, eg)
    # the nine faces / corners / centre alone, against the whole set's scale
    face = np.linalg.norm(g[:9] - ref[:9]) / np.linalg.norm(ref)
    assert face <= _bar(Z, ef)


def test_empty_point_sets():
    nufft = _nufft()
    D = 2
    bounds = ([(-1, 1)] * D, [(-5, 5)] * D)
    plan = _plan(np.complex128, D, bounds)
    z0 = torch.empty(0, dtype=torch.float64, device="cuda")
    s = tuple(torch.linspace(-5, 5, 37, dtype=torch.float64, device="cuda") for _ in range(D))
    nufft.set_points3(plan, (z0, z0), s)
    f = torch.full((37,), 3.0 + 1j, dtype=torch.complex128, device="cuda")
    g = tuple(torch.full((37,), 3.0 + 1j, dtype=torch.complex128, device="cuda") for _ in range(D))
    nufft.exec_type3_grad(f, g, plan, torch.empty(0, dtype=torch.complex128, device="cuda"))
    assert torch.count_nonzero(f).item() == 0 and all(torch.count_nonzero(t).item() == 0 for t in g)
    # no targets: a no-op
    x = tuple(torch.zeros(11, dtype=torch.float64, device="cuda") for _ in range(D))
    nufft.set_points3(plan, x, (z0, z0))
    e = torch.empty(0, dtype=torch.complex128, device="cuda")
    nufft.exec_type3_grad(e, (e, e), plan, torch.ones(11, dtype=torch.complex128, device="cuda"))
    torch.cuda.synchronize()


def test_refusals_come_before_any_stage():
    nufft = _nufft()
    L = nufft._lib
    lib = nufft.lib
    D, n = 2, 64
    bounds = ([(-1, 1)] * D, [(-5, 5)] * D)
    plan = _plan(np.complex128, D, bounds)
    f = torch.zeros(n, dtype=torch.complex128, device="cuda")
    c = torch.ones(n, dtype=torch.complex128, device="cuda")
    gs = [torch.zeros(n, dtype=torch.complex128, device="cuda") for _ in range(D)]
    ft = (C.c_void_p * 1)(f.data_ptr())
    ct = (C.c_void_p * 1)(c.data_ptr())
    assert lib.nufft_exec_type3_grad(plan._handle, ft, (C.c_void_p * D)(*[t.data_ptr() for t in gs]), ct, plan._stream()) == L.ERR_NO_POINTS
    x = tuple(torch.rand(n, dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(D))
    s = tuple(torch.rand(n, dtype=torch.float64, device="cuda") * 10 - 5 for _ in range(D))
    nufft.set_points3(plan, x, s)
    plan.enable_timing(True)
    torch.cuda.synchronize()
    assert lib.nufft_exec_type3_grad(plan._handle, ft, None, ct, plan._stream()) == L.ERR_INVALID_ARG
    assert lib.nufft_exec_type3_grad(plan._handle, ft, (C.c_void_p * D)(gs[0].data_ptr(), None), ct, plan._stream()) == L.ERR_INVALID_ARG
    assert lib.nufft_exec_type3_grad(plan._handle, None, (C.c_void_p * D)(*[t.data_ptr() for t in gs]), ct, plan._stream()) == L.ERR_INVALID_ARG
    assert lib.nufft_exec_type3_grad(plan._handle, ft, (C.c_void_p * D)(*[t.data_ptr() for t in gs]), None, plan._stream()) == L.ERR_INVALID_ARG
    t = plan.timer
    assert not any(k in t for k in ("premultiply", "spread", "type2", "postmultiply")), t
    # wrong containers are refused in Python
    with pytest.raises(nufft.DimensionMismatch):
        nufft.exec_type3_grad(f, (gs[0],), plan, c)
    with pytest.raises(ValueError):
        nufft.exec_type3_grad(f, (gs[0], gs[1].real.contiguous()), plan, c)
    nufft.exec_type3_grad(f, tuple(gs), plan, c)
    t = plan.timer
    assert all(k in t for k in ("premultiply", "spread", "type2", "postmultiply")), t


def test_non_default_stream():
    rng = np.random.default_rng(12)
    x, s, c, bounds = _case(rng, 3, np.complex128, Np=1000, Nk=900)
    plan = _plan(np.complex128, 3, bounds)
    f0, g0 = _grad_run(plan, x, s, c)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        f1, g1 = _grad_run(plan, x, s, c)
    st.synchronize()
    assert _rel(f1, f0) <= 1e-14 and _rel(g1, g0) <= 1e-14


def test_graph_capture_matches_eager():
    nufft = _nufft()
    rng = np.random.default_rng(13)
    D, Np, Nk = 3, 2000, 1500
    bounds = ([(-2, 2)] * D, [(-12, 12)] * D)
    plan = _plan(np.complex128, D, bounds)

    def inputs():
        return rng.uniform(-2, 2, (Np, D)), rng.uniform(-12, 12, (Nk, D)), rng.standard_normal(Np) + 1j * rng.standard_normal(Np)

    x, s, c = inputs()
    xd, sd, cd = _cols(x), _cols(s), _dev(c)
    fd = torch.empty(Nk, dtype=torch.complex128, device="cuda")
    gd = tuple(torch.empty(Nk, dtype=torch.complex128, device="cuda") for _ in range(D))

    def step():
        nufft.set_points3(plan, xd, sd)
        nufft.exec_type3_grad(fd, gd, plan, cd)

    step()                  # sizes every buffer (allocation is not capturable)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    x, s, c = inputs()
    for d in range(D):
        xd[d].copy_(torch.from_numpy(x[:, d]))
        sd[d].copy_(torch.from_numpy(s[:, d]))
    cd.copy_(torch.from_numpy(c))
    fd.zero_()
    graph.replay()
    torch.cuda.synchronize()
    eager_f, eager_g = _grad_run(_plan(np.complex128, D, bounds), x, s, c)
    assert _rel(fd.cpu().numpy(), eager_f) <= 1e-13
    assert _rel(np.stack([t.cpu().numpy() for t in gd], axis=1), eager_g) <= 1e-13


def test_agrees_with_spectral_route():
    """exec_type3_grad against an ntransforms = D + 1 type 3 of (c, σ i x_d c), Np = Nk = 2e5, D = 3: the difference is within the
    sum of the two routes' errors (each measured against exact sums at 200 targets)."""
    nufft = _nufft()
    rng = np.random.default_rng(14)
    D, n = 3, 200_000
    x, s, c, bounds = _case(rng, D, np.complex128, Np=n, Nk=n)
    plan = _plan(np.complex128, D, bounds)
    f, g = _grad_run(plan, x, s, c)
    spec = _plan(np.complex128, D, bounds, ntransforms=D + 1)
    nufft.set_points3(spec, _cols(x), _cols(s))
    ins = [c] + [(-1j) * x[:, d] * c for d in range(D)]
    outs = [torch.empty(n, dtype=torch.complex128, device="cuda") for _ in ins]
    nufft.exec_type3(outs, spec, [_dev(v) for v in ins])
    gs = np.stack([o.cpu().numpy() for o in outs[1:]], axis=1)
    sub = rng.choice(n, 200, replace=False)
    ref = R.direct3_grad(x, s[sub], c, -1)
    e_grad = _rel(g[sub], ref)
    e_spec = _rel(gs[sub], ref)
    diff = _rel(g, gs)
    print(f"spectral route: gradient {e_grad:.3e}, spectral {e_spec:.3e}, difference {diff:.3e}")
    assert diff <= 2.0 * (e_grad + e_spec)
    assert _rel(f, outs[0].cpu().numpy()) <= 1e-12


@pytest.mark.parametrize("D", [1, 2, 3])
def test_adjoint_identity(D):
    """⟨A c, g⟩ = ⟨c, A^H g⟩ with A^H the adjoint() plan (sources s, targets x)."""
    nufft = _nufft()
    rng = np.random.default_rng(15 + D)
    x, s, c, bounds = _case(rng, D, np.complex128, Np=1500, Nk=1300)
    gv = rng.standard_normal(1300) + 1j * rng.standard_normal(1300)
    plan = _plan(np.complex128, D, bounds, M=8)
    adj = plan.adjoint()
    assert adj.nf == plan.nf
    nufft.set_points3(plan, _cols(x), _cols(s))
    nufft.set_points3(adj, _cols(s), _cols(x))
    Ac = _value_run(plan, c)
    AHg = _value_run(adj, gv)
    lhs, rhs = np.vdot(gv, Ac), np.vdot(AHg, c)
    scale = np.linalg.norm(Ac) * np.linalg.norm(gv)
    assert abs(lhs - rhs) <= 1e-11 * scale, (lhs, rhs)
    assert _rel(AHg, R.direct3(s, x, gv, +1)) <= 1e-11


@pytest.mark.parametrize("D", [1, 2, 3])
def test_autograd_gradcheck(D):
    nufft = _nufft()
    rng = np.random.default_rng(20 + D)
    n = 20
    xc, sc = rng.uniform(-2, 2, D), rng.uniform(-6, 6, D)
    bounds = ([(xc[d] - 2.0, xc[d] + 2.0) for d in range(D)], [(sc[d] - 6.0, sc[d] + 6.0) for d in range(D)])
    plan = _plan(np.complex128, D, bounds, M=8)
    xs = tuple(torch.from_numpy(xc[d] + 1.6 * rng.uniform(-1, 1, n)).cuda().requires_grad_(True) for d in range(D))
    ss = tuple(torch.from_numpy(sc[d] + 5.0 * rng.uniform(-1, 1, n)).cuda().requires_grad_(True) for d in range(D))
    c = torch.from_numpy(rng.standard_normal(n) + 1j * rng.standard_normal(n)).cuda().requires_grad_(True)
    kw = dict(eps=1e-6, atol=1e-6, rtol=1e-4)

    def f_all(v, *p):
        return nufft.autograd.type3(plan, p[:D], p[D:], v)

    assert torch.autograd.gradcheck(f_all, (c, *xs, *ss), **kw)
    xd, sd, cd = tuple(t.detach() for t in xs), tuple(t.detach() for t in ss), c.detach()
    assert torch.autograd.gradcheck(lambda v: nufft.autograd.type3(plan, xd, sd, v), (c,), **kw)
    assert torch.autograd.gradcheck(lambda *p: nufft.autograd.type3(plan, p, sd, cd), xs, **kw)
    assert torch.autograd.gradcheck(lambda *p: nufft.autograd.type3(plan, xd, p, cd), ss, **kw)
    assert plan._adjoint_plan is not None and plan._adjoint_plan.info().sign == 1


def test_autograd_refuses_several_transforms():
    nufft = _nufft()
    plan = _plan(np.complex128, 1, ([(-1, 1)], [(-5, 5)]), ntransforms=2)
    x = (torch.zeros(3, dtype=torch.float64, device="cuda"),)
    with pytest.raises(ValueError):
        nufft.autograd.type3(plan, x, x, torch.zeros(3, dtype=torch.complex128, device="cuda"))
