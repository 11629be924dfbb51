"""The circulant preconditioner and preconditioned CG without a GPU: the fold formula against the dense matrix, positivity,
the numpy PCG against numpy.linalg.solve and against plain CG, the iteration counts on clustered point sets, and the C ABI (header,
ctypes mirror, symbols, struct sizes, refusals that need no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import cg_reference as CG
import precond_reference as P
import toeplitz_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("nufft_precond_create", "nufft_precond_destroy", "nufft_precond_update", "nufft_precond_set_scaling", "nufft_precond_apply",
                "nufft_precond_get_info", "nufft_precond_multiplier_ptr", "nufft_precond_scaling_ptr", "nufft_sizeof_precond_params",
                "nufft_sizeof_precond_info", "nufft_cg_set_preconditioner")
SHAPES = [(8,), (9,), (8, 6), (7, 10), (6, 5, 4)]


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


def _points(Ns, Np, seed, weights="random"):
    rng = np.random.default_rng(seed)
    xs = [rng.random(Np) * 2 * np.pi for _ in Ns]
    w = rng.random(Np) + 0.1 if weights == "random" else np.full(Np, 1.0 / Np)
    return xs, w


def _dft_matrix(Ns):
    """The unnormalised DFT over the array indices, on arrays flattened like shape N[::-1]."""
    F = np.ones((1, 1), dtype=np.complex128)
    for n in reversed(Ns):                      # the first axis is the slowest: Kronecker factors in axis order
        j = np.arange(n)
        F = np.kron(F, np.exp(-2j * np.pi * np.outer(j, j) / n))
    return F


@pytest.mark.parametrize("Ns", SHAPES)
@pytest.mark.parametrize("fftshift", [False, True])
def test_fold_formula_matches_the_dense_matrix(Ns, fftshift):
    xs, w = _points(Ns, 60, seed=1)
    T = R.exact_spectrum(Ns, xs, w)
    G = CG.dense_gram(Ns, xs, w, fftshift)
    F = _dft_matrix(Ns)
    n = G.shape[0]
    exact = np.diag(F @ G @ F.conj().T) / n
    e = P.chan_eigenvalues(Ns, T).ravel()
    scale = np.abs(exact.real).max()
    assert np.abs(e.real - exact.real).max() <= 1e-12 * scale
    assert np.abs(e.imag).max() <= 1e-12 * scale
    assert e.real.min() >= -1e-12 * scale            # positive weights: G is positive semi-definite, and so is its circulant
    # from the multiplier instead of the spectrum: what the library does (the Nyquist planes, zeroed in K, carry weight 0)
    K = R.multiplier(Ns, T)
    assert np.abs(K.imag).max() <= 1e-12 * np.abs(K.real).max()
    e2 = P.chan_eigenvalues(Ns, P.generating_sequence(Ns, K.real)).ravel()
    assert np.abs(e2 - e).max() <= 1e-12 * scale


def test_separable_spectrum_is_the_direct_sum():
    for Ns in [(8, 6), (6, 5, 4)]:
        xs, w = _points(Ns, 50, seed=2)
        assert R.rel(P.exact_spectrum_separable(Ns, xs, w), R.exact_spectrum(Ns, xs, w)) <= 1e-13


@pytest.mark.parametrize("Ns", [(8, 6), (6, 5, 4)])
@pytest.mark.parametrize("scaled", [False, True])
def test_inverse_is_hermitian_positive_definite(Ns, scaled):
    rng = np.random.default_rng(3)
    xs = [np.mod(0.3 * rng.standard_normal(40), 2 * np.pi) for _ in Ns]          # clustered: small eigenvalues, the floor is in force
    w = np.full(40, 1.0 / 40)
    e = P.chan_eigenvalues(Ns, R.exact_spectrum(Ns, xs, w))
    m = P.multiplier(e, mu=0.0, floor=1e-6)
    assert (m > 0).all() and m.max() <= (1 + 1e-12) / (m.size * 1e-6 * e.real.max())
    d = rng.random(Ns[::-1]) + 0.5 if scaled else None
    M = P.dense_inverse(m, d)
    assert np.abs(M - M.conj().T).max() <= 1e-12 * np.abs(M).max()
    assert np.linalg.eigvalsh(0.5 * (M + M.conj().T)).min() > 0


def _dense_system(Ns, seed=0):
    rng = np.random.default_rng(seed)
    xs, w = _points(Ns, 2000, seed)
    A = CG.dense_gram(Ns, xs, w)
    b = rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1])
    e = P.chan_eigenvalues(Ns, R.exact_spectrum(Ns, xs, w))
    return A, b, e


@pytest.mark.parametrize("Ns", [(16, 12), (8, 6, 5)])
@pytest.mark.parametrize("lam_rel", [0.0, 1e-3])
def test_pcg_solves_the_system(Ns, lam_rel):
    A, b, e = _dense_system(Ns)
    lam = lam_rel * float(np.linalg.eigvalsh(A)[-1])
    m = P.multiplier(e, mu=lam)
    ap = CG.matrix_apply(A, b.shape)
    exact = np.linalg.solve(A + lam * np.eye(A.shape[0]), b.ravel()).reshape(b.shape)
    got = P.pcg(ap, lambda r: P.apply(m, None, r), b, lam=lam, rtol=1e-10, max_iter=100)
    assert got["status"] == CG.CONVERGED and 2 < got["iterations"] < 60
    assert CG.true_residual(A, lam, got["x"], b) <= 2e-10
    assert R.rel(got["x"], exact) <= 2e-10 * np.linalg.cond(A + lam * np.eye(A.shape[0]))
    assert len(got["history"]) == got["iterations"] + 1 and got["history"][-1] <= 1e-10 < got["history"][-2]
    low = P.pcg(ap, lambda r: P.apply(m, None, r), b, lam=lam, rtol=1e-4, max_iter=100, dtype=np.complex64)
    assert low["x"].dtype == np.complex64 and low["status"] == CG.CONVERGED
    assert CG.true_residual(A, lam, low["x"], b.astype(np.complex64)) <= 2e-4


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_identity_preconditioner_is_plain_cg(dtype):
    A, b, _ = _dense_system((16, 12))
    ap = CG.matrix_apply(A, b.shape)
    lam = 1e-3 * float(np.linalg.eigvalsh(A)[-1])
    a = CG.cg(ap, b, lam=lam, rtol=1e-8, max_iter=100, dtype=dtype)
    c = P.pcg(ap, lambda r: r, b, lam=lam, rtol=1e-8, max_iter=100, dtype=dtype)
    eps = np.finfo(np.float32 if dtype == np.complex64 else np.float64).eps
    assert a["iterations"] == c["iterations"] and a["status"] == c["status"]
    assert R.rel(c["x"], a["x"]) <= 100 * eps
    assert np.allclose(c["history"], a["history"], rtol=1e3 * eps, atol=0)
    rng = np.random.default_rng(7)
    x0 = rng.standard_normal(b.shape) + 1j * rng.standard_normal(b.shape)
    a = CG.cg(ap, b, x0=x0, lam=lam, rtol=1e-8, max_iter=100, dtype=dtype)
    c = P.pcg(ap, lambda r: r, b, x0=x0, lam=lam, rtol=1e-8, max_iter=100, dtype=dtype)
    assert a["iterations"] == c["iterations"] and R.rel(c["x"], a["x"]) <= 100 * eps
    zero = P.pcg(ap, lambda r: r, np.zeros_like(b), rtol=1e-6, max_iter=10, dtype=dtype)
    assert zero["iterations"] == 0 and zero["status"] == CG.CONVERGED and not zero["x"].any()


def clustered_points(Ns, Np, seed):
    """Half of the points uniform, half N(0, 0.4²) (0.5² in 3-D) folded into [0, 2π)."""
    rng = np.random.default_rng(seed)
    sd = 0.5 if len(Ns) == 3 else 0.4
    return [np.mod(np.concatenate([rng.random(Np // 2) * 2 * np.pi, sd * rng.standard_normal(Np - Np // 2)]), 2 * np.pi) for _ in Ns]


@pytest.mark.parametrize("Ns,Np,seed", [((48, 40), 12000, 11), ((64, 80), 40000, 12), ((16, 12, 10), 20000, 13)])
@pytest.mark.parametrize("lam_rel", [0.0, 1e-3])
def test_preconditioning_halves_the_iterations(Ns, Np, seed, lam_rel):
    """A condition, not a measurement: on clustered point sets without density weights PCG needs at most half the iterations of CG."""
    xs = clustered_points(Ns, Np, seed)
    w = np.full(Np, 1.0 / Np)
    T = P.exact_spectrum_separable(Ns, xs, w)
    K = R.multiplier(Ns, T).real
    e = P.chan_eigenvalues(Ns, T).real
    lam = lam_rel * float(e.max())
    m = P.multiplier(e, mu=lam)
    rng = np.random.default_rng(seed + 100)
    b = rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1])
    ap = lambda p: R.apply(Ns, K, p)
    plain = CG.cg(ap, b, lam=lam, rtol=1e-6, max_iter=600)
    pre = P.pcg(ap, lambda r: P.apply(m, None, r), b, lam=lam, rtol=1e-6, max_iter=600)
    print(f"N = {Ns}, lam = {lam_rel:g} max e: CG {plain['iterations']} iterations, PCG {pre['iterations']}")
    assert plain["status"] == CG.CONVERGED and pre["status"] == CG.CONVERGED
    assert 2 * pre["iterations"] <= plain["iterations"]
    r = b - (ap(pre["x"]) + lam * pre["x"])
    assert np.linalg.norm(r) <= 2e-6 * np.linalg.norm(b)


def test_header_ctypes_and_library_agree(nufft):
    header = open(os.path.join(ROOT, "include", "nufft_mi355x.h")).read()
    assert "---- Preconditioner" in header
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
    assert nufft.lib.nufft_sizeof_precond_params() == C.sizeof(L.NufftPrecondParams) == 24
    assert nufft.lib.nufft_sizeof_precond_info() == C.sizeof(L.NufftPrecondInfo) == 112
    for name, value in (("NUFFT_PRECOND_PATH_DENSE", L.PRECOND_PATH_DENSE), ("NUFFT_PRECOND_PATH_FUSED", L.PRECOND_PATH_FUSED),
                        ("NUFFT_PRECOND_SCALING_NONE", L.PRECOND_SCALING_NONE), ("NUFFT_PRECOND_SCALING_MAPS", L.PRECOND_SCALING_MAPS),
                        ("NUFFT_PRECOND_SCALING_CALLER", L.PRECOND_SCALING_CALLER)):
        assert re.search(name + r"\s*=\s*" + str(value) + r"\b", header), name
    assert nufft.lib.nufft_version() == 104      # added without an ABI bump: detected by symbol
    assert callable(nufft.ToeplitzPreconditioner) and "ToeplitzPreconditioner" in nufft.__all__
    assert nufft.lib.nufft_sizeof_cg_params() == 32      # the solver's parameters did not grow


def _params(nufft, lam=0.0, floor=1e-6):
    p = nufft._lib.NufftPrecondParams()
    p.struct_size = C.sizeof(nufft._lib.NufftPrecondParams)
    p.lambda_, p.floor = lam, floor
    return p


def test_refusals_without_a_device(nufft):
    L, lib = nufft._lib, nufft.lib
    op = nufft.ToeplitzOperator(nufft.PlanNUFFT(torch.complex128, (32, 32), backend=None))
    h = C.c_void_p()
    assert lib.nufft_precond_create(C.byref(h), None, C.byref(_params(nufft))) == L.ERR_INVALID_ARG
    assert lib.nufft_precond_create(C.byref(h), op._handle, None) == L.ERR_INVALID_ARG
    assert lib.nufft_precond_create(None, op._handle, C.byref(_params(nufft))) == L.ERR_INVALID_ARG
    assert lib.nufft_precond_create(C.byref(h), op._handle, C.byref(_params(nufft, lam=-1.0))) == L.ERR_INVALID_ARG
    assert "lambda" in lib.nufft_last_error_message().decode()
    for floor in (0.0, -1e-6, float("nan"), float("inf")):
        assert lib.nufft_precond_create(C.byref(h), op._handle, C.byref(_params(nufft, floor=floor))) == L.ERR_INVALID_ARG
        assert "floor" in lib.nufft_last_error_message().decode()
    small = _params(nufft)
    small.struct_size = 8
    assert lib.nufft_precond_create(C.byref(h), op._handle, C.byref(small)) == L.ERR_INVALID_ARG
    assert lib.nufft_precond_create(C.byref(h), op._handle, C.byref(_params(nufft))) == L.ERR_NO_DEVICE
    assert not h.value and "host-only" in lib.nufft_last_error_message().decode()
    assert lib.nufft_precond_update(None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_precond_set_scaling(None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_precond_apply(None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_precond_get_info(None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_precond_multiplier_ptr(None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_precond_scaling_ptr(None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_cg_set_preconditioner(None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_precond_destroy(None) == 0
    with pytest.raises(ValueError):
        nufft.ToeplitzPreconditioner(op)
    with pytest.raises(ValueError):
        nufft.ToeplitzPreconditioner(op, lam=-1.0)
    with pytest.raises(ValueError):
        nufft.ToeplitzPreconditioner(op, floor=0.0)
    with pytest.raises(ValueError):
        nufft.ToeplitzPreconditioner(object())
