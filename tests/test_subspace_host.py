"""Coupled components of the Toeplitz normal operator without a GPU: the numpy reference against the brute-force
matrix E^H W E, the structure of the multipliers, the pair order, and the refusals of a host-only object."""
import ctypes as C

import numpy as np
import pytest
import torch

import subspace_reference as S
import toeplitz_reference as R

ENTRY_POINTS = ("nufft_toeplitz_set_points_coupled", "nufft_toeplitz_set_spectra_coupled", "nufft_toeplitz_num_coupled",
                "nufft_toeplitz_multiplier_pair_ptr")


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


def _tiny(seed=0, Ns=(6, 5), Np=40, K=3):
    rng = np.random.default_rng(seed)
    xs = [rng.random(Np) * 2 * np.pi for _ in Ns]
    w = rng.random(Np) + 0.1
    phi = rng.standard_normal((K, Np)) + 1j * rng.standard_normal((K, Np))
    us = [rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1]) for _ in range(K)]
    return Ns, xs, w, phi, us


@pytest.mark.parametrize("fftshift", [False, True])
def test_reference_against_the_brute_force_matrix(fftshift):
    Ns, xs, w, phi, us = _tiny()
    K, n = phi.shape[0], int(np.prod(Ns))
    A = S.brute_force_gram(Ns, xs, w, phi, fftshift)
    assert np.allclose(A, A.conj().T, rtol=0, atol=1e-12 * np.abs(A).max())
    want = A @ np.concatenate([u.ravel() for u in us])
    direct = S.exact_block_gram(Ns, xs, w, phi, us, fftshift)
    spectra = S.exact_spectra(Ns, xs, w, phi)
    via_fft = S.block_apply(Ns, S.multipliers(Ns, spectra), us, fftshift)
    dense = S.dense_block_gram(Ns, spectra, K, fftshift)
    for a in range(K):
        assert R.rel(direct[a].ravel(), want[a * n:(a + 1) * n]) <= 1e-13
        assert R.rel(via_fft[a].ravel(), want[a * n:(a + 1) * n]) <= 1e-13
    assert R.rel(dense, A) <= 1e-13
    # the joint CG of the reference solves the block system
    bs = [d for d in direct]
    sol = S.joint_cg(S.matrix_block_apply(A, K, Ns[::-1]), bs, lam=0.1 * np.linalg.eigvalsh(A)[-1], rtol=1e-10, max_iter=200)
    assert sol["status"] == "converged" and sol["x"].shape == (K,) + Ns[::-1]


def test_multipliers_are_hermitian_in_the_pair():
    Ns, xs, w, phi, _ = _tiny(seed=1)
    K = phi.shape[0]
    Ks = S.multipliers(Ns, S.exact_spectra(Ns, xs, w, phi))
    for a in range(K):
        kaa = Ks[S.pair_index(a, a, K)]
        assert np.abs(kaa.imag).max() <= 1e-14 * np.abs(kaa).max()
        for b in range(a + 1, K):
            kba = R.multiplier(Ns, R.exact_spectrum(Ns, xs, S.pair_weights(w, phi, b, a)))       # built on its own, not by conjugation
            assert R.rel(kba, np.conj(Ks[S.pair_index(a, b, K)])) <= 1e-13
            assert np.abs(Ks[S.pair_index(a, b, K)].imag).max() > 1e-3 * np.abs(kaa).max()        # and it is truly complex


def test_pair_index_is_row_major(nufft):
    for K in (1, 2, 3, 5, 16):
        order = S.pairs(K)
        assert len(order) == K * (K + 1) // 2
        for p, (a, b) in enumerate(order):
            assert S.pair_index(a, b, K) == p == nufft.ToeplitzOperator.pair_index(a, b, K) == a * K - a * (a - 1) // 2 + (b - a)
    with pytest.raises(ValueError):
        nufft.ToeplitzOperator.pair_index(1, 0, 2)


def test_symbols_are_bound(nufft):
    raw = C.CDLL(nufft.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in nufft._lib.SYMBOLS and hasattr(raw, name), name
    assert nufft.lib.nufft_version() == 104                      # added without an ABI bump: detected by symbol
    assert nufft.lib.nufft_sizeof_toeplitz_info() == C.sizeof(nufft._lib.NufftToeplitzInfo)


def test_host_only_object_refuses_coupled_builds(nufft):
    L, lib = nufft._lib, nufft.lib
    op = nufft.ToeplitzOperator(nufft.PlanNUFFT(torch.complex128, (32, 32), ntransforms=2, backend=None))
    h = op._handle
    tab2, tab3 = (C.c_void_p * 2)(4096, 8192), (C.c_void_p * 3)(4096, 8192, 12288)
    assert lib.nufft_toeplitz_num_coupled(h) == 0 and lib.nufft_toeplitz_num_coupled(None) == 0 and op.coupled is False
    assert lib.nufft_toeplitz_set_spectra_coupled(h, tab3, None) == L.ERR_NO_DEVICE
    assert lib.nufft_toeplitz_set_points_coupled(h, None, 4, tab2, None, tab2, None) == L.ERR_NO_DEVICE
    assert lib.nufft_toeplitz_set_spectra_coupled(h, None, None) == L.ERR_INVALID_ARG                    # null tables
    assert lib.nufft_toeplitz_set_points_coupled(h, None, 4, tab2, None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_toeplitz_set_spectra_coupled(None, tab3, None) == L.ERR_INVALID_ARG
    assert lib.nufft_toeplitz_set_points_coupled(None, None, 4, tab2, None, tab2, None) == L.ERR_INVALID_ARG
    ptr, nb = C.c_void_p(), C.c_int64()
    assert lib.nufft_toeplitz_multiplier_pair_ptr(h, 0, 1, C.byref(ptr), C.byref(nb)) == L.ERR_NO_DEVICE
    assert lib.nufft_toeplitz_multiplier_pair_ptr(h, 0, 1, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_toeplitz_num_coupled(h) == 0
    # the component count is checked before a device is asked for: K != ntransforms
    pts = (torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64))
    with pytest.raises(nufft.DimensionMismatch):
        op.set_points(pts, basis=torch.ones((3, 8), dtype=torch.complex128))
    with pytest.raises(nufft.DimensionMismatch):
        op.set_points(pts, basis=torch.ones(8, dtype=torch.complex128))          # a vector only where ntransforms == 1
    with pytest.raises(nufft.DimensionMismatch):
        op.set_spectra(torch.ones((2, 64, 64), dtype=torch.complex128))          # 3 pairs for 2 components
    with pytest.raises(nufft.DimensionMismatch):
        op.set_spectra([torch.ones((64, 64), dtype=torch.complex128)] * 4)
    with pytest.raises(ValueError):
        op.set_points(pts, basis=torch.ones((2, 8), dtype=torch.complex128))     # right count: now the missing device is the complaint
    with pytest.raises(ValueError):
        op.set_spectra(torch.ones((3, 64, 64), dtype=torch.complex128))
