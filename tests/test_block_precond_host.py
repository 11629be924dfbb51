"""The block-circulant preconditioner of a coupled operator without a GPU: the block fold formula against the dense block
matrix, positivity with the shift in force, the reductions to the scalar reference, the numpy block PCG against numpy.linalg.solve and
against joint CG on clustered point sets, and the C ABI (header, ctypes mirror, symbols, refusals that need no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import block_precond_reference as BP
import cg_reference as CG
import precond_reference as P
import subspace_reference as SR
import toeplitz_reference as R
from test_precond_host import _dft_matrix, _points, clustered_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("nufft_precond_create_block", "nufft_precond_num_coupled", "nufft_precond_block_ptr", "nufft_precond_floored_cells")


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


def _random_basis(K, Np, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((K, Np)) + 1j * rng.standard_normal((K, Np))


def _stack_apply(Ns, Ks):
    return lambda p: np.stack(SR.block_apply(Ns, Ks, [p[a] for a in range(p.shape[0])]))


# ---- H1 ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Ns", [(8,), (8, 6), (6, 5, 4)])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("fftshift", [False, True])
def test_block_fold_formula_matches_the_dense_block_matrix(Ns, K, fftshift):
    xs, w = _points(Ns, 60, seed=1)
    phi = _random_basis(K, 60, seed=2)
    spectra = SR.exact_spectra(Ns, xs, w, phi)
    G = SR.dense_block_gram(Ns, spectra, K, fftshift)
    n = int(np.prod(Ns))
    F = _dft_matrix(Ns)
    E = BP.block_eigenvalues(Ns, spectra, K).reshape(K, K, n)
    exact = np.zeros((K, K, n), dtype=np.complex128)
    for a in range(K):
        for b in range(K):
            exact[a, b] = np.diag(F @ G[a * n:(a + 1) * n, b * n:(b + 1) * n] @ F.conj().T) / n
    scale = np.abs(exact).max()
    assert np.abs(E - exact).max() <= 1e-12 * scale
    cells = np.moveaxis(E, -1, 0)
    assert np.abs(cells - np.conj(np.swapaxes(cells, 1, 2))).max() <= 1e-12 * scale
    assert np.linalg.eigvalsh(cells).min() >= -1e-12 * scale          # positive weights: G_Φ is positive semi-definite, and so is every E(q)
    # from the multipliers instead of the spectra: what the library does (the Nyquist planes, zeroed in K_ab, carry weight 0)
    Ks = SR.multipliers(Ns, spectra)
    E2 = BP.block_eigenvalues(Ns, [P.generating_sequence(Ns, Kab) for Kab in Ks], K).reshape(K, K, n)
    assert np.abs(E2 - E).max() <= 1e-12 * scale


# ---- H2 ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Ns,K", [((8, 6), 2), ((6, 5, 4), 3)])
@pytest.mark.parametrize("scaled", [False, True])
def test_block_inverse_is_hermitian_positive_definite(Ns, K, scaled):
    rng = np.random.default_rng(3)
    xs = [np.mod(0.3 * rng.standard_normal(40), 2 * np.pi) for _ in Ns]          # clustered: small eigenvalues, the shift (μ = 0) is in force
    w = np.full(40, 1.0 / 40)
    E = BP.block_eigenvalues(Ns, SR.exact_spectra(Ns, xs, w, BP.subspace_basis(K, 40, 3)), K)
    lam_min = np.linalg.eigvalsh(np.moveaxis(E.reshape(K, K, -1), -1, 0)).min()
    floor = 1e-2
    shift = BP.shift_of(E, 0.0, floor)
    assert lam_min < 0.1 * shift         # the shift decides the small eigenvalues of B's inverse
    B, floored = BP.block_inverse(E, 0.0, floor)
    assert floored == 0
    d = rng.random(Ns[::-1]) + 0.5 if scaled else None
    M = BP.dense_block_inverse(B, d)
    assert np.abs(M - M.conj().T).max() <= 1e-12 * np.abs(M).max()
    assert np.linalg.eigvalsh(0.5 * (M + M.conj().T)).min() > 0


def test_pivot_floor_engages_on_an_indefinite_cell():
    E = np.zeros((2, 2, 3), dtype=np.complex128)
    E[0, 0], E[1, 1] = 1.0, 1.0
    E[0, 1, 1], E[1, 0, 1] = 2.0, 2.0                                   # cell 1: eigenvalues 3 and −1, which no round-off produces
    B, floored = BP.block_inverse(E, 0.0, 1e-6)
    assert floored == 1 and np.isfinite(B).all()
    assert np.allclose(B[:, :, 0], np.eye(2) / (3 * (1 + 1e-6)))


# ---- H3, H4 -----------------------------------------------------------------------------------------------------------------------

def test_one_component_is_the_scalar_reference():
    Ns = (16, 12)
    xs, w = _points(Ns, 2000, seed=4)
    T = R.exact_spectrum(Ns, xs, w)
    e = P.chan_eigenvalues(Ns, T).real
    E = BP.block_eigenvalues(Ns, [T], 1)
    for mu, floor in ((1e-3 * e.max(), 1e-6), (0.0, 1e-6)):
        B, _ = BP.block_inverse(E, mu, floor)
        m = P.multiplier(e, mu, floor)
        # the scalar object clamps, the block object shifts: they agree where the clamp is idle, once the shift is μ itself
        idle = e + mu >= floor * (e + mu).max()
        shift = BP.shift_of(E, mu, floor)
        assert idle.any()
        assert np.abs(B[0, 0].real * (e + shift) / (e + mu) - m)[idle].max() <= 1e-12 * m.max()
        if mu > 0:
            assert shift == mu and idle.all() and np.abs(B[0, 0].imag).max() == 0
            r = np.random.default_rng(5).standard_normal((1,) + Ns[::-1]) + 0j
            assert R.rel(BP.block_apply(B, None, r)[0], P.apply(m, None, r[0])) <= 1e-13


def test_uncoupled_spectra_give_scalar_inverses():
    Ns, K = (8, 6), 3
    Ts = []
    for a, b in SR.pairs(K):
        xs, w = _points(Ns, 300, seed=10 + a)
        Ts.append(R.exact_spectrum(Ns, xs, w) if a == b else np.zeros([2 * n for n in reversed(Ns)], dtype=np.complex128))
    E = BP.block_eigenvalues(Ns, Ts, K)
    mu = 1e-2 * max(E[a, a].real.max() for a in range(K))
    B, floored = BP.block_inverse(E, mu, 1e-6)
    assert floored == 0
    for a in range(K):
        for b in range(K):
            if a == b:
                m = P.multiplier(E[a, a].real, mu, 1e-6)
                assert np.abs(B[a, a] - m).max() <= 1e-13 * m.max()
            else:
                assert not B[a, b].any()


# ---- H5 ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Ns,K", [((16, 12), 2), ((8, 6, 5), 3)])
@pytest.mark.parametrize("lam_rel", [0.0, 1e-3])
def test_block_pcg_solves_the_system(Ns, K, lam_rel):
    seed = 0
    xs, w = _points(Ns, 2000, seed)
    phi = BP.subspace_basis(K, 2000, seed)
    spectra = BP.separable_spectra(Ns, xs, w, phi)
    A = SR.dense_block_gram(Ns, spectra, K)
    lam = lam_rel * float(np.linalg.eigvalsh(A)[-1])
    shape = (K,) + Ns[::-1]
    rng = np.random.default_rng(seed + 7)
    b = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    B, floored = BP.block_inverse(BP.block_eigenvalues(Ns, spectra, K), lam)
    assert floored == 0
    ap = CG.matrix_apply(A, shape)
    exact = np.linalg.solve(A + lam * np.eye(A.shape[0]), b.ravel()).reshape(shape)
    got = P.pcg(ap, lambda r: BP.block_apply(B, None, r), b, lam=lam, rtol=1e-10, max_iter=300)
    assert got["status"] == CG.CONVERGED and got["iterations"] > 2
    assert CG.true_residual(A, lam, got["x"], b) <= 2e-10
    assert R.rel(got["x"], exact) <= 2e-10 * np.linalg.cond(A + lam * np.eye(A.shape[0]))


# ---- H6 ---------------------------------------------------------------------------------------------------------------------------

_CLUSTERED = [((48, 40), 12000, 11, 2, 0.0), ((48, 40), 12000, 11, 2, 1e-3), ((64, 80), 40000, 12, 2, 0.0), ((64, 80), 40000, 12, 2, 1e-3),
              ((16, 12, 10), 20000, 13, 2, 0.0), ((16, 12, 10), 20000, 13, 2, 1e-3), ((16, 12, 10), 20000, 13, 4, 0.0),
              ((16, 12, 10), 20000, 13, 4, 1e-3), ((48, 40), 12000, 11, 3, 1e-3)]
_SPECTRA = {}


def _clustered_spectra(Ns, Np, seed, K):
    key = (Ns, Np, seed, K)
    if key not in _SPECTRA:
        xs = clustered_points(Ns, Np, seed)
        _SPECTRA[key] = BP.separable_spectra(Ns, xs, np.full(Np, 1.0 / Np), BP.subspace_basis(K, Np, seed))
    return _SPECTRA[key]


@pytest.mark.parametrize("Ns,Np,seed,K,lam_rel", _CLUSTERED)
def test_block_preconditioning_halves_the_iterations(Ns, Np, seed, K, lam_rel):
    """A condition, not a measurement: on clustered point sets without density weights, with the subspace basis of the tests, block PCG
    needs at most half the iterations of joint CG.  ((48, 40), K = 3 at λ = 0 is not a case: plain CG does not converge in 2000 iterations.)"""
    spectra = _clustered_spectra(Ns, Np, seed, K)
    Ks = SR.multipliers(Ns, spectra)
    E = BP.block_eigenvalues(Ns, spectra, K)
    lam = lam_rel * float(np.linalg.eigvalsh(np.moveaxis(E.reshape(K, K, -1), -1, 0)).max())
    B, floored = BP.block_inverse(E, lam)
    shape = (K,) + Ns[::-1]
    rng = np.random.default_rng(seed + 100)
    b = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    ap = _stack_apply(Ns, Ks)
    plain = CG.cg(ap, b, lam=lam, rtol=1e-6, max_iter=2000)
    pre = P.pcg(ap, lambda r: BP.block_apply(B, None, r), b, lam=lam, rtol=1e-6, max_iter=2000)
    print(f"N = {Ns}, K = {K}, lam = {lam_rel:g} max E: joint CG {plain['iterations']} iterations, block PCG {pre['iterations']} ({floored} floored cells)")
    assert plain["status"] == CG.CONVERGED and pre["status"] == CG.CONVERGED
    assert 2 * pre["iterations"] <= plain["iterations"]
    r = b - (ap(pre["x"]) + lam * pre["x"])
    assert np.linalg.norm(r) <= 2e-6 * np.linalg.norm(b)


# ---- H7 ---------------------------------------------------------------------------------------------------------------------------

def test_header_ctypes_and_library_agree(nufft):
    header = open(os.path.join(ROOT, "include", "nufft_mi355x.h")).read()
    assert "floor is a SHIFT" in header and "bound λ_max(E) from below" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(nufft.LIB_PATH)
    ctype = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name in NEW_ENTRY_POINTS:
        proto = re.search(r"\b(int64_t|int32_t|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert proto, name
        res, args = nufft._lib.SYMBOLS[name]
        assert len(args) == proto.group(2).count(",") + 1, name
        assert res is ctype[proto.group(1)], name
        assert hasattr(raw, name), name
    L = nufft._lib
    assert nufft.lib.nufft_sizeof_precond_params() == C.sizeof(L.NufftPrecondParams) == 24
    assert nufft.lib.nufft_sizeof_precond_info() == C.sizeof(L.NufftPrecondInfo) == 112
    assert nufft.lib.nufft_version() == 104      # added without an ABI bump: detected by symbol


def test_refusals_without_a_device(nufft):
    L, lib = nufft._lib, nufft.lib
    op = nufft.ToeplitzOperator(nufft.PlanNUFFT(torch.complex128, (32, 32), backend=None, ntransforms=2))
    prm = L.NufftPrecondParams()
    prm.struct_size = C.sizeof(L.NufftPrecondParams)
    prm.lambda_, prm.floor = 0.0, 1e-6
    h, ptr, nbytes = C.c_void_p(), C.c_void_p(), C.c_int64()
    assert lib.nufft_precond_create_block(C.byref(h), None, C.byref(prm)) == L.ERR_INVALID_ARG
    assert lib.nufft_precond_create_block(C.byref(h), op._handle, None) == L.ERR_INVALID_ARG
    assert lib.nufft_precond_create_block(None, op._handle, C.byref(prm)) == L.ERR_INVALID_ARG
    bad = L.NufftPrecondParams()
    bad.struct_size = C.sizeof(L.NufftPrecondParams)
    bad.lambda_, bad.floor = -1.0, 1e-6
    assert lib.nufft_precond_create_block(C.byref(h), op._handle, C.byref(bad)) == L.ERR_INVALID_ARG
    assert "lambda" in lib.nufft_last_error_message().decode()
    bad.lambda_, bad.floor = 0.0, 0.0
    assert lib.nufft_precond_create_block(C.byref(h), op._handle, C.byref(bad)) == L.ERR_INVALID_ARG
    assert "floor" in lib.nufft_last_error_message().decode()
    assert lib.nufft_precond_create_block(C.byref(h), op._handle, C.byref(prm)) == L.ERR_NO_DEVICE
    assert not h.value and "host-only" in lib.nufft_last_error_message().decode()
    assert lib.nufft_precond_block_ptr(None, 0, 0, C.byref(ptr), C.byref(nbytes)) == L.ERR_INVALID_ARG
    assert lib.nufft_precond_block_ptr(None, 1, 0, C.byref(ptr), C.byref(nbytes)) == L.ERR_INVALID_ARG
    assert lib.nufft_precond_num_coupled(None) == 0
    assert lib.nufft_precond_floored_cells(None) == -1
    with pytest.raises(ValueError):
        nufft.ToeplitzPreconditioner(op, block=True)
