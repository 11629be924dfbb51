"""Total variation without a GPU: the numpy reference (tv_reference.py) reaches the minimiser (optimality conditions in float64), its
freeze, prefix and zero right-hand-side rules, the adjoint identity, and the C ABI of the difference operator and of the primal-dual
solver (header, ctypes mirror, symbols, struct sizes, the refusals that need no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import toeplitz_reference as R
import tv_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("nufft_tv_create", "nufft_tv_create_for_operator", "nufft_tv_destroy", "nufft_tv_get_info", "nufft_tv_gradient",
                "nufft_tv_adjoint", "nufft_tv_norm", "nufft_sizeof_tv_info", "nufft_tvpd_create", "nufft_tvpd_destroy", "nufft_tvpd_set_tv",
                "nufft_tvpd_solve", "nufft_tvpd_get_info", "nufft_tvpd_get_result", "nufft_tvpd_history", "nufft_sizeof_tvpd_params",
                "nufft_sizeof_tvpd_info")

# what the float64 reference reaches on the (32, 24) system with tol = 1e-8 (measured on the CPU), per lam / λmax: (r, e, g)
REACHED = {0.0: (6.13e-8, 2.22e-16, 1.68e-9), 0.05: (7.25e-8, 2.22e-16, 2.02e-9)}


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


@pytest.fixture(scope="module")
def system():
    """(32, 24) unknowns, 4 n uniform points, the exact spectrum through toeplitz_reference: the system of test_fista_host.py."""
    Ns = (32, 24)
    rng = np.random.default_rng(7)
    Np = 4 * int(np.prod(Ns))
    xs = [rng.random(Np) * 2 * np.pi for _ in Ns]
    w = (rng.random(Np) + 0.1) / Np
    K = R.multiplier(Ns, R.exact_spectrum(Ns, xs, w)).real
    apply = lambda p: R.apply(Ns, K, np.asarray(p).astype(np.complex128))      # noqa: E731
    b = rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1])
    v = b.copy()
    for _ in range(60):
        g = apply(v)
        lmax = float(np.linalg.norm(g) / np.linalg.norm(v))
        v = g / np.linalg.norm(g)
    return Ns, apply, b, lmax


@pytest.mark.parametrize("lam_rel", [0.0, 0.05])
def test_reference_reaches_the_minimiser(system, lam_rel):
    """Measured on the CPU in float64 with tol = 1e-8: lam = 0: 269 iterations, clipped share 0.98 at the end, r = 6.13e-8,
    e = 2.22e-16, g = 1.68e-9; lam = 0.05 λmax: 369 iterations, 0.98, r = 7.25e-8, e = 2.22e-16, g = 2.02e-9.  The bars are 10 × those
    (e is one rounding of the projection: 10 × 2.22e-16)."""
    Ns, apply, b, lmax = system
    lam = lam_rel * lmax
    tv = 0.1 * np.abs(b).max()
    got = T.tvpd(apply, b, tv, 1.0 / (1.05 * lmax + lam), lam=lam, tol=1e-8, max_iter=20000)
    assert got["status"] == T.CONVERGED and got["change"] <= 1e-8
    assert 0.2 <= got["clipped"][:10].mean() <= 0.95, got["clipped"][:10]                   # both branches of the projection run
    r, e, g = T.optimality(apply, b, got["x"], got["y"], tv, lam=lam)
    print(f"lam = {lam_rel} lmax: {got['iterations']} iterations, clipped {got['clipped'][-1]:.2f}, r {r:.2e}, e {e:.2e}, g {g:.2e}")
    br, be, bg = REACHED[lam_rel]
    assert r <= 10 * br and e <= 10 * be and g <= 10 * bg
    hist = got["history"]
    assert hist.shape == (got["iterations"], 2) and hist[-1, 0] == got["change"]
    assert abs(hist[-1, 1] - T.norm(got["x"])) <= 1e-12 * hist[-1, 1]


def test_reference_rules(system):
    Ns, apply, b, lmax = system
    step = 1.0 / (1.05 * lmax)
    tv = 0.1 * np.abs(b).max()
    zero = T.tvpd(apply, np.zeros_like(b), tv, step, tol=1e-6, max_iter=10)
    assert zero["iterations"] == 1 and zero["status"] == T.CONVERGED and not zero["x"].any() and zero["change"] == 0.0
    a = T.tvpd(apply, b, tv, step, tol=1e-4, max_iter=2000)
    short = T.tvpd(apply, b, tv, step, tol=1e-4, max_iter=a["iterations"] - 2)
    assert a["status"] == T.CONVERGED and short["status"] == T.MAX_ITER and short["iterations"] == a["iterations"] - 2
    assert np.array_equal(short["history"], a["history"][:-2])                               # a shorter run is a prefix
    plain = T.tvpd(apply, b, 0.0, step, tol=1e-10, max_iter=20000)                           # tv = 0: gradient descent on G x = b
    assert not plain["y"].any()                                                              # every dual vector is projected onto {0}
    assert np.linalg.norm(apply(plain["x"]) - b) <= 1e-5 * np.linalg.norm(b)
    low = T.tvpd(apply, b, tv, step, tol=1e-4, max_iter=2000, dtype=np.complex64)
    assert low["x"].dtype == np.complex64 and low["y"].dtype == np.complex64 and R.rel(low["x"], a["x"]) <= 1e-3
    nan = T.tvpd(lambda p: np.full_like(p, np.nan), b, tv, step, tol=1e-4, max_iter=5)
    assert nan["status"] == T.BREAKDOWN and nan["iterations"] == 1
    two = np.stack([b, 0.5 * b[::-1]])                                                       # a joint system: one change over both
    joint = T.tvpd(lambda p: np.stack([apply(p[0]), apply(p[1])]), two, (tv, 0.0), step, tol=0.0, max_iter=5, component_axis=0)
    assert joint["x"].shape == two.shape and joint["y"].shape == (2,) + two.shape and not joint["y"][:, 1].any()
    alone = T.tvpd(apply, b, tv, step, tol=0.0, max_iter=5)
    assert np.array_equal(joint["x"][0], alone["x"])


@pytest.mark.parametrize("shape", [(9,), (7, 5), (5, 6, 7)])
def test_adjoint_identity(shape):
    rng = np.random.default_rng(len(shape))
    x = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    y = rng.standard_normal((len(shape),) + shape) + 1j * rng.standard_normal((len(shape),) + shape)
    lhs, rhs = np.vdot(T.gradient(x), y), np.vdot(x, T.adjoint(y))
    assert abs(lhs - rhs) <= 1e-13 * abs(lhs)
    assert not T.gradient(np.full(shape, 2.5 - 1j)).any()
    assert T.gradient(x).shape == (len(shape),) + shape
    assert np.array_equal(T.gradient(x)[0], np.roll(x, -1, axis=-1) - x)                    # dimension 1 is the last axis


def test_header_ctypes_and_library_agree(nufft):
    header = open(os.path.join(ROOT, "include", "nufft_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(nufft.LIB_PATH)
    for name in ENTRY_POINTS:
        proto = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert proto, name
        nargs = 0 if proto.group(2).strip() == "void" else proto.group(2).count(",") + 1
        res, args = nufft._lib.SYMBOLS[name]
        assert len(args) == nargs, name
        assert res is (C.c_int64 if proto.group(1) == "int64_t" else C.c_int), name
        assert hasattr(raw, name), name
    L = nufft._lib
    assert nufft.lib.nufft_sizeof_tv_info() == C.sizeof(L.NufftTvInfo) == 72
    assert nufft.lib.nufft_sizeof_tvpd_params() == C.sizeof(L.NufftTvpdParams) == 56
    assert nufft.lib.nufft_sizeof_tvpd_info() == C.sizeof(L.NufftTvpdInfo) == 80
    assert nufft.lib.nufft_sizeof_fista_params() == 56 and nufft.lib.nufft_sizeof_fista_info() == 72      # the FISTA structs did not move
    for name, value in (("NUFFT_TVPD_MAX_ITER", L.TVPD_MAX_ITER), ("NUFFT_TVPD_CONVERGED", L.TVPD_CONVERGED),
                        ("NUFFT_TVPD_BREAKDOWN", L.TVPD_BREAKDOWN)):
        assert re.search(name + r"\s*=\s*" + str(value) + r"\b", header), name
    assert nufft.lib.nufft_version() == 104      # added without an ABI bump: detected by symbol
    assert callable(nufft.ToeplitzTV) and callable(nufft.TotalVariation)


def _params(nufft, **kw):
    p = nufft._lib.NufftTvpdParams()
    p.struct_size = C.sizeof(nufft._lib.NufftTvpdParams)
    p.max_iter, p.check_every = 10, 0
    p.tol, p.step, p.sigma, p.tv, p.lambda_ = 1e-4, 1.0, 0.0, 0.1, 0.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_refusals_without_a_device(nufft):
    L, lib = nufft._lib, nufft.lib
    plan = nufft.PlanNUFFT(torch.complex128, (24, 40), backend=None)
    op = nufft.ToeplitzOperator(plan)
    h = C.c_void_p()
    assert lib.nufft_tvpd_create(C.byref(h), op._handle, C.byref(_params(nufft))) == L.ERR_NO_DEVICE and not h.value
    assert "host-only" in lib.nufft_last_error_message().decode()
    for kw in ({"max_iter": 0}, {"max_iter": (1 << 24) + 1}, {"check_every": -1}, {"tol": -1.0}, {"tol": float("nan")}, {"step": 0.0},
               {"step": -1.0}, {"step": float("nan")}, {"step": float("inf")}, {"sigma": -1.0}, {"sigma": float("inf")}, {"tv": -1.0},
               {"tv": float("nan")}, {"lambda_": -1.0}, {"lambda_": float("inf")}, {"struct_size": 8}):
        assert lib.nufft_tvpd_create(C.byref(h), op._handle, C.byref(_params(nufft, **kw))) == L.ERR_INVALID_ARG, kw      # before NO_DEVICE
        assert not h.value
    assert lib.nufft_tvpd_create(C.byref(h), None, C.byref(_params(nufft))) == L.ERR_INVALID_ARG
    assert lib.nufft_tvpd_create(C.byref(h), op._handle, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tvpd_create(None, op._handle, C.byref(_params(nufft))) == L.ERR_INVALID_ARG
    assert lib.nufft_tvpd_solve(None, None, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tvpd_set_tv(None, None, 0) == L.ERR_INVALID_ARG
    assert lib.nufft_tvpd_get_info(None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tvpd_get_result(None, None, None, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tvpd_history(None, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tvpd_destroy(None) == 0
    # the difference operator alone
    assert lib.nufft_tv_create(C.byref(h), plan._handle) == L.ERR_NO_DEVICE and not h.value
    assert lib.nufft_tv_create_for_operator(C.byref(h), op._handle) == L.ERR_NO_DEVICE and not h.value
    assert lib.nufft_tv_create(C.byref(h), None) == L.ERR_INVALID_ARG
    assert lib.nufft_tv_create(None, plan._handle) == L.ERR_INVALID_ARG
    assert lib.nufft_tv_create_for_operator(C.byref(h), None) == L.ERR_INVALID_ARG
    real = nufft.PlanNUFFT(torch.float64, (24, 40), backend=None)
    assert lib.nufft_tv_create(C.byref(h), real._handle) == L.ERR_UNSUPPORTED and not h.value      # a real-data plan, before NO_DEVICE
    assert lib.nufft_tv_gradient(None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tv_adjoint(None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tv_norm(None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tv_get_info(None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tv_destroy(None) == 0
    with pytest.raises(ValueError):
        nufft.ToeplitzTV(op, step=1.0)
    with pytest.raises(ValueError):
        nufft.ToeplitzTV(op)                          # step=None needs the device already
    with pytest.raises(ValueError):
        nufft.ToeplitzTV(object())
    with pytest.raises(ValueError):
        nufft.ToeplitzTV(op, step=1.0, maxiter=2.5)
    with pytest.raises(ValueError):
        nufft.ToeplitzTV(op, step=1.0, check_every=True)
    with pytest.raises(ValueError):
        nufft.ToeplitzTV(op, step=1.0, sigma=0.0)
    with pytest.raises(ValueError):
        nufft.ToeplitzTV(op, step=1.0, tv=-1.0)
    with pytest.raises(ValueError):
        nufft.ToeplitzTV(op, step=1.0, tv=(0.1, 0.2))
    for scalar in (np.float32(0.1), np.float64(0.1), torch.tensor(0.1), 1):      # numbers of any kind are one weight for all components
        with pytest.raises(ValueError, match="host-only"):
            nufft.ToeplitzTV(op, step=1.0, tv=scalar)
    with pytest.raises(ValueError, match="host-only"):
        nufft.ToeplitzTV(op, step=1.0, tv=np.array([0.1]))
    with pytest.raises(ValueError):
        nufft.ToeplitzTV(op, step=1.0, tv=np.array([0.1, 0.2]))
    with pytest.raises(ValueError):
        nufft.TotalVariation(op)
    with pytest.raises(ValueError):
        nufft.TotalVariation(object())
    with pytest.raises(ValueError):
        nufft.ToeplitzFISTA(op, prior="tv", step=1.0)     # total variation is a solver of its own, not a FISTA prior
