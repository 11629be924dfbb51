"""FISTA with an l1-wavelet prior without a GPU: the numpy reference (fista_reference.py) reaches the minimiser (KKT conditions in
float64), its freeze and zero right-hand-side rules, and the C ABI of the solver and of the power iteration (header, ctypes mirror,
symbols, struct sizes, the refusals that need no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import cg_reference as CG
import fista_reference as F
import toeplitz_reference as R
import wavelet_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("nufft_fista_create", "nufft_fista_destroy", "nufft_fista_set_l1", "nufft_fista_solve", "nufft_fista_get_info",
                "nufft_fista_get_result", "nufft_fista_history", "nufft_sizeof_fista_params", "nufft_sizeof_fista_info",
                "nufft_toeplitz_max_eigenvalue")


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


@pytest.fixture(scope="module")
def system():
    """(32, 24) unknowns, 4 n uniform points, the exact spectrum through toeplitz_reference."""
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


@pytest.mark.parametrize("wavelet", ["haar", "db2"])
@pytest.mark.parametrize("lam_rel", [0.0, 0.05])
def test_reference_reaches_the_minimiser(system, wavelet, lam_rel):
    Ns, apply, b, lmax = system
    lam = lam_rel * lmax
    l1 = 0.4 * np.abs(W.forward(b, wavelet, 3)).max()
    got = F.fista(apply, b, wavelet, 3, l1, 1.0 / (1.05 * lmax + lam), lam=lam, tol=1e-10, max_iter=20000)
    assert got["status"] == F.CONVERGED and got["change"] <= 1e-10
    assert 0.2 <= got["zero_fraction"] <= 0.95, got["zero_fraction"]                         # the prior is active, and not everything is zero
    res = F.kkt_residual(apply, b, got["x"], wavelet, 3, l1, lam=lam, zero_tol=1e-12 * np.abs(got["x"]).max())
    print(f"{wavelet} lam = {lam_rel} lmax: {got['iterations']} iterations, zero details {got['zero_fraction']:.2f}, KKT residual / l1 {res:.2e}")
    assert res <= 1e-6
    hist = got["history"]
    assert hist.shape == (got["iterations"], 2) and hist[-1, 0] == got["change"]
    c = W.forward(got["x"], wavelet, 3)
    assert abs(hist[-1, 1] - np.abs(c[W.detail_mask(c.shape, 3)]).sum()) <= 1e-9 * hist[-1, 1]


def test_reference_rules(system):
    Ns, apply, b, lmax = system
    step = 1.0 / (1.05 * lmax)
    l1 = 0.4 * np.abs(W.forward(b, "db2", 3)).max()
    zero = F.fista(apply, np.zeros_like(b), "db2", 3, l1, step, tol=1e-6, max_iter=10)
    assert zero["iterations"] == 1 and zero["status"] == F.CONVERGED and not zero["x"].any() and zero["change"] == 0.0
    a = F.fista(apply, b, "db2", 3, l1, step, tol=1e-4, max_iter=500)
    short = F.fista(apply, b, "db2", 3, l1, step, tol=1e-4, max_iter=a["iterations"] - 2)
    assert a["status"] == F.CONVERGED and short["status"] == F.MAX_ITER and short["iterations"] == a["iterations"] - 2
    assert np.array_equal(short["history"], a["history"][:-2])
    warm = F.fista(apply, b, "db2", 3, l1, step, tol=1e-4, max_iter=500, x0=a["x"])
    assert warm["status"] == F.CONVERGED and warm["iterations"] <= a["iterations"]
    plain = F.fista(apply, b, "db2", 3, 0.0, step, tol=1e-9, max_iter=5000)                      # l1 = 0: accelerated gradient on G x = b
    assert plain["zero_fraction"] < 0.01 and np.linalg.norm(apply(plain["x"]) - b) <= 1e-5 * np.linalg.norm(b)
    low = F.fista(apply, b, "db2", 3, l1, step, tol=1e-4, max_iter=500, dtype=np.complex64)
    assert low["x"].dtype == np.complex64 and R.rel(low["x"], a["x"]) <= 1e-3
    nan = F.fista(lambda p: np.full_like(p, np.nan), b, "haar", 3, l1, step, tol=1e-4, max_iter=5)
    assert nan["status"] == F.BREAKDOWN and nan["iterations"] == 1


def test_power_iteration_bounds_the_step(system):
    """What ToeplitzFISTA does for step=None: 30 applies from a random start give a Rayleigh quotient within a few per cent below λmax,
    so 1.05 times it is a safe Lipschitz bound on well-sampled systems."""
    Ns = (16, 12)
    rng = np.random.default_rng(3)
    xs = [rng.random(2000) * 2 * np.pi for _ in Ns]
    A = CG.dense_gram(Ns, xs, rng.random(2000) + 0.1)
    lmax = float(np.linalg.eigvalsh(A)[-1])
    v = rng.standard_normal(A.shape[0]) + 1j * rng.standard_normal(A.shape[0])
    for _ in range(30):
        g = A @ v
        rho = float(np.real(np.vdot(v, g)) / np.real(np.vdot(v, v)))
        v = g / np.linalg.norm(g)
    assert 0.95 * lmax <= rho <= lmax * (1 + 1e-12)


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
    assert nufft.lib.nufft_sizeof_fista_params() == C.sizeof(L.NufftFistaParams) == 56
    assert nufft.lib.nufft_sizeof_fista_info() == C.sizeof(L.NufftFistaInfo) == 72
    for name, value in (("NUFFT_FISTA_MAX_ITER", L.FISTA_MAX_ITER), ("NUFFT_FISTA_CONVERGED", L.FISTA_CONVERGED),
                        ("NUFFT_FISTA_BREAKDOWN", L.FISTA_BREAKDOWN)):
        assert re.search(name + r"\s*=\s*" + str(value) + r"\b", header), name
    assert nufft.lib.nufft_version() == 104      # added without an ABI bump: detected by symbol
    assert callable(nufft.ToeplitzFISTA) and hasattr(nufft.ToeplitzOperator, "max_eigenvalue")


def _params(nufft, **kw):
    p = nufft._lib.NufftFistaParams()
    p.struct_size = C.sizeof(nufft._lib.NufftFistaParams)
    p.max_iter, p.check_every, p.wavelet, p.levels = 10, 0, nufft._lib.WAVELET_DB2, 3
    p.tol, p.step, p.l1, p.lambda_ = 1e-4, 1.0, 0.1, 0.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_refusals_without_a_device(nufft):
    L, lib = nufft._lib, nufft.lib
    op = nufft.ToeplitzOperator(nufft.PlanNUFFT(torch.complex128, (24, 40), backend=None))
    h = C.c_void_p()
    assert lib.nufft_fista_create(C.byref(h), op._handle, C.byref(_params(nufft))) == L.ERR_NO_DEVICE and not h.value
    assert "host-only" in lib.nufft_last_error_message().decode()
    for kw in ({"max_iter": 0}, {"check_every": -1}, {"tol": -1.0}, {"step": 0.0}, {"step": float("nan")}, {"l1": -1.0},
               {"lambda_": float("inf")}, {"struct_size": 8}, {"levels": 4}, {"levels": 0}, {"wavelet": 7}):
        assert lib.nufft_fista_create(C.byref(h), op._handle, C.byref(_params(nufft, **kw))) == L.ERR_INVALID_ARG, kw
        assert not h.value
    assert lib.nufft_fista_create(C.byref(h), None, C.byref(_params(nufft))) == L.ERR_INVALID_ARG
    assert lib.nufft_fista_create(C.byref(h), op._handle, None) == L.ERR_INVALID_ARG
    assert lib.nufft_fista_create(None, op._handle, C.byref(_params(nufft))) == L.ERR_INVALID_ARG
    assert lib.nufft_fista_solve(None, None, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_fista_set_l1(None, None, 0) == L.ERR_INVALID_ARG
    assert lib.nufft_fista_get_info(None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_fista_get_result(None, None, None, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_fista_history(None, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_fista_destroy(None) == 0
    out = (C.c_double * 1)()
    assert lib.nufft_toeplitz_max_eigenvalue(None, None, 30, out, None) == L.ERR_INVALID_ARG
    tab = (C.c_void_p * 1)(16)
    assert lib.nufft_toeplitz_max_eigenvalue(op._handle, tab, 30, out, None) == L.ERR_NO_DEVICE
    assert lib.nufft_toeplitz_max_eigenvalue(op._handle, tab, 0, out, None) == L.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        nufft.ToeplitzFISTA(op, step=1.0)
    with pytest.raises(ValueError):
        nufft.ToeplitzFISTA(op)                       # step=None needs the device already
    with pytest.raises(ValueError):
        op.max_eigenvalue()
    with pytest.raises(ValueError):
        nufft.ToeplitzFISTA(object())
    with pytest.raises(ValueError):
        nufft.ToeplitzFISTA(op, step=1.0, maxiter=2.5)
    with pytest.raises(ValueError):
        nufft.ToeplitzFISTA(op, step=1.0, wavelet="sym4")
