"""Conjugate gradients on the Toeplitz normal operator without a GPU: the numpy reference against numpy.linalg.solve, the freeze rule,
b = 0, breakdown on a singular system, the dense Gram matrix against direct sums, and the C ABI (header, ctypes mirror, symbols,
struct sizes, refusals that need no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import cg_reference as CG
import toeplitz_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("nufft_cg_create", "nufft_cg_destroy", "nufft_cg_solve", "nufft_cg_get_info", "nufft_cg_get_result", "nufft_cg_history",
                "nufft_sizeof_cg_params", "nufft_sizeof_cg_info")


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


def _system(Ns, Np=2000, seed=0, clustered=False, fftshift=False):
    rng = np.random.default_rng(seed)
    if clustered:
        xs = [np.mod(np.pi + 0.3 * rng.standard_normal(Np), 2 * np.pi) for _ in Ns]
    else:
        xs = [rng.random(Np) * 2 * np.pi for _ in Ns]
    w = rng.random(Np) + 0.1
    A = CG.dense_gram(Ns, xs, w, fftshift)
    b = rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1])
    return xs, w, A, b


@pytest.mark.parametrize("Ns", [(8,), (9,), (8, 6), (7, 10), (6, 5, 4)])
@pytest.mark.parametrize("fftshift", [False, True])
def test_dense_gram_matches_direct_sums(Ns, fftshift):
    xs, w, A, u = _system(Ns, Np=60, fftshift=fftshift)
    assert R.rel((A @ u.ravel()).reshape(u.shape), R.exact_gram(Ns, xs, w, u, fftshift)) <= 1e-12
    assert np.allclose(A, A.conj().T, rtol=0, atol=1e-12 * np.abs(A).max())          # Hermitian for real weights


@pytest.mark.parametrize("Ns", [(16, 12), (8, 6, 5), (48,)])
@pytest.mark.parametrize("lam_rel", [0.0, 1e-3])
def test_reference_solves_the_system(Ns, lam_rel):
    xs, w, A, b = _system(Ns, Np=400 if Ns == (48,) else 2000)
    lam = lam_rel * float(np.linalg.eigvalsh(A)[-1])
    exact = np.linalg.solve(A + lam * np.eye(A.shape[0]), b.ravel()).reshape(b.shape)
    got = CG.cg(CG.matrix_apply(A, b.shape), b, lam=lam, rtol=1e-10, max_iter=100)
    assert got["status"] == CG.CONVERGED and 5 < got["iterations"] < 60
    assert CG.true_residual(A, lam, got["x"], b) <= 2e-10
    cond = np.linalg.cond(A + lam * np.eye(A.shape[0]))
    assert R.rel(got["x"], exact) <= 2e-10 * cond
    assert len(got["history"]) == got["iterations"] + 1 and got["history"][-1] <= 1e-10 < got["history"][-2]
    low = CG.cg(CG.matrix_apply(A, b.shape), b, lam=lam, rtol=1e-4, max_iter=100, dtype=np.complex64)
    assert low["x"].dtype == np.complex64 and low["status"] == CG.CONVERGED
    assert CG.true_residual(A, lam, low["x"], b.astype(np.complex64)) <= 2e-4


def test_freeze_rule_and_warm_start():
    Ns = (16, 12)
    xs, w, A, b = _system(Ns)
    ap = CG.matrix_apply(A, b.shape)
    a = CG.cg(ap, b, rtol=1e-8, max_iter=100)
    c = CG.cg(ap, b, rtol=1e-8, max_iter=a["iterations"] + 1)        # one spare iteration changes nothing: the component is done
    assert np.array_equal(a["x"], c["x"]) and a["iterations"] == c["iterations"]
    short = CG.cg(ap, b, rtol=1e-8, max_iter=a["iterations"] - 2)
    assert short["status"] == CG.MAX_ITER and short["iterations"] == a["iterations"] - 2
    assert np.array_equal(short["history"], a["history"][:-2])
    fixed = CG.cg(ap, b, rtol=0.0, max_iter=5)                        # rtol = 0: runs max_iter iterations
    assert fixed["iterations"] == 5 and fixed["status"] == CG.MAX_ITER
    tight = CG.cg(ap, b, rtol=1e-12, max_iter=100)
    warm = CG.cg(ap, b, x0=tight["x"], rtol=1e-8, max_iter=100)       # already below rtol: nothing runs
    assert warm["iterations"] == 0 and np.array_equal(warm["x"], tight["x"]) and warm["status"] == CG.CONVERGED
    rng = np.random.default_rng(5)
    x0 = rng.standard_normal(b.shape) + 1j * rng.standard_normal(b.shape)
    other = CG.cg(ap, b, x0=x0, rtol=1e-10, max_iter=100)
    assert other["status"] == CG.CONVERGED and CG.true_residual(A, 0.0, other["x"], b) <= 2e-10


def test_zero_right_hand_side():
    xs, w, A, b = _system((8, 6))
    got = CG.cg(CG.matrix_apply(A, b.shape), np.zeros_like(b), rtol=1e-6, max_iter=10)
    assert got["iterations"] == 0 and got["status"] == CG.CONVERGED and not got["x"].any() and got["history"].tolist() == [0.0]


def test_breakdown_and_singular_systems():
    b = np.array([1.0, 2.0, 0.5], dtype=np.complex128)
    zero = CG.cg(lambda p: np.zeros_like(p), b, rtol=1e-6, max_iter=10)            # γ = 0: no division
    assert zero["status"] == CG.BREAKDOWN and zero["iterations"] == 0 and not zero["x"].any()
    neg = CG.cg(lambda p: -p, b, rtol=1e-6, max_iter=10)                           # γ < 0
    assert neg["status"] == CG.BREAKDOWN and np.isfinite(neg["x"]).all()
    xs, w, A, rhs = _system((16, 12), clustered=True)                              # numerically singular: never reaches rtol
    assert np.linalg.cond(A) > 1e12
    sing = CG.cg(CG.matrix_apply(A, rhs.shape), rhs, rtol=1e-10, max_iter=300)
    assert sing["status"] in (CG.BREAKDOWN, CG.MAX_ITER) and np.isfinite(sing["x"]).all()
    lam = 1e-3 * float(np.linalg.eigvalsh(A)[-1])
    reg = CG.cg(CG.matrix_apply(A, rhs.shape), rhs, lam=lam, rtol=1e-10, max_iter=300)
    assert reg["status"] == CG.CONVERGED and CG.true_residual(A, lam, reg["x"], rhs) <= 2e-10


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
    assert nufft.lib.nufft_sizeof_cg_params() == C.sizeof(L.NufftCgParams) == 32
    assert nufft.lib.nufft_sizeof_cg_info() == C.sizeof(L.NufftCgInfo) == 64
    for name, value in (("NUFFT_CG_MAX_ITER", L.CG_MAX_ITER), ("NUFFT_CG_CONVERGED", L.CG_CONVERGED), ("NUFFT_CG_BREAKDOWN", L.CG_BREAKDOWN)):
        assert re.search(name + r"\s*=\s*" + str(value) + r"\b", header), name
    assert nufft.lib.nufft_version() == 104      # added without an ABI bump: detected by symbol
    assert callable(nufft.ToeplitzCG) and hasattr(nufft.ToeplitzOperator, "solve")


def _params(nufft, **kw):
    p = nufft._lib.NufftCgParams()
    p.struct_size = C.sizeof(nufft._lib.NufftCgParams)
    p.max_iter, p.check_every, p.rtol, p.lambda_ = 10, 0, 1e-6, 0.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_host_only_operator_is_refused(nufft):
    L, lib = nufft._lib, nufft.lib
    op = nufft.ToeplitzOperator(nufft.PlanNUFFT(torch.complex128, (32, 32), backend=None))
    h = C.c_void_p()
    assert lib.nufft_cg_create(C.byref(h), op._handle, C.byref(_params(nufft))) == L.ERR_NO_DEVICE
    assert not h.value
    assert "host-only" in lib.nufft_last_error_message().decode()
    assert lib.nufft_cg_create(C.byref(h), None, C.byref(_params(nufft))) == L.ERR_INVALID_ARG
    assert lib.nufft_cg_create(C.byref(h), op._handle, None) == L.ERR_INVALID_ARG
    assert lib.nufft_cg_create(None, op._handle, C.byref(_params(nufft))) == L.ERR_INVALID_ARG
    assert lib.nufft_cg_solve(None, None, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_cg_get_info(None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_cg_get_result(None, None, None, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_cg_history(None, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_cg_destroy(None) == 0
    with pytest.raises(ValueError):
        nufft.ToeplitzCG(op)
    with pytest.raises(ValueError):
        op.solve(torch.zeros(op.shape, dtype=torch.complex128))
    with pytest.raises(ValueError):
        nufft.ToeplitzCG(object())
    with pytest.raises(ValueError):
        nufft.ToeplitzCG(op, maxiter=2.5)
