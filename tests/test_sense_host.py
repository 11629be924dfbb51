"""Coil sensitivity maps in the Toeplitz normal operator without a GPU: the ABI (symbols, ctypes mirror), the
refusals of a host-only object, and the numpy reference with the spectral bound that lets the CG bars carry over."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import cg_reference as CG
import sense_reference as S
import toeplitz_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("nufft_toeplitz_set_maps", "nufft_toeplitz_clear_maps", "nufft_toeplitz_num_coils", "nufft_coil_expand",
                "nufft_coil_combine")


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


def test_symbols_are_exported_and_mirrored(nufft):
    header = open(os.path.join(ROOT, "include", "nufft_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(nufft.LIB_PATH)
    for name in ENTRY_POINTS:
        proto = re.search(r"\b(int32_t|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert proto, name
        res, args = nufft._lib.SYMBOLS[name]
        assert len(args) == proto.group(2).count(",") + 1, name
        assert res is (C.c_int32 if proto.group(1) == "int32_t" else C.c_int), name
        assert hasattr(raw, name), name
    assert nufft.lib.nufft_version() == 104                      # added without an ABI bump: detected by symbol
    assert nufft.lib.nufft_sizeof_toeplitz_info() == C.sizeof(nufft._lib.NufftToeplitzInfo)
    assert callable(nufft.coil_expand) and callable(nufft.coil_combine)
    assert all(hasattr(nufft.ToeplitzOperator, a) for a in ("set_maps", "clear_maps", "ncoils"))


def test_host_only_object_refuses_maps(nufft):
    L, lib = nufft._lib, nufft.lib
    op = nufft.ToeplitzOperator(nufft.PlanNUFFT(torch.complex128, (32, 32), backend=None))
    h = op._handle
    tab = (C.c_void_p * 2)(4096, 8192)
    assert lib.nufft_toeplitz_num_coils(h) == 0 and op.ncoils == 0
    assert lib.nufft_toeplitz_set_maps(h, 2, tab, None) == L.ERR_NO_DEVICE
    assert lib.nufft_toeplitz_set_maps(h, 2, None, None) == L.ERR_INVALID_ARG          # null table
    assert lib.nufft_toeplitz_set_maps(h, 0, tab, None) == L.ERR_INVALID_ARG           # range
    assert lib.nufft_toeplitz_set_maps(h, -1, tab, None) == L.ERR_INVALID_ARG
    assert lib.nufft_toeplitz_set_maps(h, 1025, tab, None) == L.ERR_INVALID_ARG
    assert lib.nufft_toeplitz_set_maps(None, 2, tab, None) == L.ERR_INVALID_ARG
    assert lib.nufft_toeplitz_num_coils(h) == 0
    assert lib.nufft_toeplitz_clear_maps(h) == L.OK and lib.nufft_toeplitz_clear_maps(h) == L.OK
    assert lib.nufft_toeplitz_clear_maps(None) == L.ERR_INVALID_ARG and lib.nufft_toeplitz_num_coils(None) == 0
    with pytest.raises(ValueError):
        op.set_maps(torch.ones((2, 32, 32), dtype=torch.complex128))
    assert op.clear_maps() is op and "coil" not in repr(op)
    # the stateless coil passes: argument checks come before anything touches a device
    assert lib.nufft_coil_expand(L.F64, 4, 2, tab, tab, 4096, -1, None) == L.ERR_NO_DEVICE
    assert lib.nufft_coil_combine(L.F64, 4, 2, 4096, tab, tab, -1, None) == L.ERR_NO_DEVICE
    assert lib.nufft_coil_expand(L.F64, -1, 2, tab, tab, 4096, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_coil_expand(L.F64, 4, 0, tab, tab, 4096, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_coil_expand(L.F64, 4, 2, None, tab, 4096, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_coil_expand(7, 4, 2, tab, tab, 4096, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_coil_combine(L.F32, 4, 2, 4096 + 8, tab, tab, 0, None) == L.ERR_INVALID_ARG     # not 16-byte aligned
    assert lib.nufft_coil_combine(L.F32, 4, 2, 4096, tab, (C.c_void_p * 2)(4096, 0), 0, None) == L.ERR_INVALID_ARG


def test_development_switch_is_accepted(nufft):
    for v in (0, 1):
        op = nufft.ToeplitzOperator(nufft.PlanNUFFT(torch.complex64, (32, 48), backend=None, options={"NUFFT_TOEPLITZ_MAPS_INPASS": v}))
        assert op.path == "fused" and op.ncoils == 0


def _problem(Ns, ncoils, Np=60, seed=0):
    rng = np.random.default_rng(seed)
    xs = [rng.random(Np) * 2 * np.pi for _ in Ns]
    w = rng.random(Np) + 0.1
    u = rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1])
    return xs, w, u, S.smooth_maps(ncoils, Ns[::-1], seed=seed + 1)


@pytest.mark.parametrize("Ns", [(8,), (8, 6), (6, 5, 4)])
@pytest.mark.parametrize("fftshift", [False, True])
def test_reference_forms_agree(Ns, fftshift):
    xs, w, u, maps = _problem(Ns, 3)
    assert not maps[2].ravel()[0] and np.all(np.abs(maps[0]) > 0.1)               # one coil with an exactly zero region
    ref = S.exact_sense_gram(Ns, xs, w, maps, u, fftshift)
    K = R.multiplier(Ns, R.exact_spectrum(Ns, xs, w)).real
    got = sum(np.conj(m) * R.apply(Ns, K, m * u, fftshift) for m in maps)
    assert R.rel(got, ref) <= 1e-12
    assert R.rel(S.toeplitz_sense_gram(Ns, K, maps, u, fftshift), ref) <= 1e-12
    GS = S.dense_sense_gram(CG.dense_gram(Ns, xs, w, fftshift), maps)
    assert R.rel((GS @ u.ravel()).reshape(u.shape), ref) <= 1e-12


@pytest.mark.parametrize("Ns,Np", [((8,), 60), ((8, 6), 400), ((6, 5, 4), 800)])
def test_dense_matrix_is_hermitian_and_its_spectrum_is_enclosed(Ns, Np):
    """x^H G_S x = Σ_c (S_c x)^H G (S_c x) and Σ_c ‖S_c x‖² = ‖x‖² for normalised maps: the Rayleigh quotients of G_S are convex
    combinations of those of G, so its eigenvalues lie in [λmin(G), λmax(G)] and cond(G_S + λ) <= cond(G + λ)."""
    xs, w, _, maps = _problem(Ns, 3, Np=Np, seed=3)
    maps = S.normalise(maps)
    assert np.allclose(np.sum(np.abs(maps) ** 2, axis=0), 1.0, rtol=0, atol=1e-14)
    G = CG.dense_gram(Ns, xs, w)
    GS = S.dense_sense_gram(G, maps)
    assert np.linalg.norm(GS - GS.conj().T) <= 1e-13 * np.linalg.norm(GS)
    ev, evs = np.linalg.eigvalsh(G), np.linalg.eigvalsh((GS + GS.conj().T) / 2)
    tol = 1e-12 * ev[-1]
    assert ev[0] - tol <= evs[0] and evs[-1] <= ev[-1] + tol, (ev[0], evs[0], evs[-1], ev[-1])
