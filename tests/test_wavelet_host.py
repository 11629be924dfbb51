"""The wavelet transform without a GPU: the numpy reference (wavelet_reference.py) against the properties of an orthogonal periodic
transform, and the C ABI (header, ctypes mirror, symbols, struct sizes, the refusals that need no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import wavelet_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("nufft_wavelet_create", "nufft_wavelet_create_for_operator", "nufft_wavelet_destroy", "nufft_wavelet_get_info",
                "nufft_wavelet_forward", "nufft_wavelet_inverse", "nufft_wavelet_shrink", "nufft_sizeof_wavelet_params",
                "nufft_sizeof_wavelet_info")

# (Ns, levels): D = 1 ... 3, slowest dimension last as everywhere in the tests
SHAPES = [((16,), 3), ((48,), 3), ((24, 40), 3), ((16, 16, 8), 2), ((8, 12, 20), 2)]


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


def _random(Ns, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1])


@pytest.mark.parametrize("wavelet", ["haar", "db2"])
@pytest.mark.parametrize("Ns,levels", SHAPES)
def test_reference_is_orthogonal(Ns, levels, wavelet):
    a = _random(Ns)
    c = W.forward(a, wavelet, levels)
    assert c.shape == a.shape and c.dtype == np.complex128
    assert np.linalg.norm(W.inverse(c, wavelet, levels) - a) <= 1e-13 * np.linalg.norm(a)
    assert abs(np.linalg.norm(c) - np.linalg.norm(a)) <= 1e-13 * np.linalg.norm(a)                # Parseval
    h, g = W.filters(wavelet)
    assert abs(h.sum() - np.sqrt(2)) <= 1e-15 and abs(g.sum()) <= 1e-15 and abs(h @ h - 1) <= 1e-15


@pytest.mark.parametrize("wavelet", ["haar", "db2"])
@pytest.mark.parametrize("Ns,levels", SHAPES)
def test_reference_on_a_constant_image(Ns, levels, wavelet):
    D = len(Ns)
    c = W.forward(np.full(Ns[::-1], 2.5 - 1.0j), wavelet, levels)
    mask = W.detail_mask(c.shape, levels)
    assert np.abs(c[mask]).max() <= 1e-13
    assert np.abs(c[~mask] - (2.5 - 1.0j) * 2.0 ** (D * levels / 2)).max() <= 1e-13 * 2.0 ** (D * levels / 2)


@pytest.mark.parametrize("Ns,levels", SHAPES)
def test_db2_annihilates_a_linear_ramp_away_from_the_wrap(Ns, levels):
    """Two vanishing moments: the first-level details of a ramp along one axis vanish except where the filter straddles the periodic
    boundary (the last coarse position of that axis)."""
    for axis in range(len(Ns)):
        shape = Ns[::-1]
        ramp = np.arange(shape[axis], dtype=np.float64).reshape([-1 if a == axis else 1 for a in range(len(shape))])
        a = np.broadcast_to(ramp, shape).astype(np.complex128)
        c = W.forward(a, "db2", 1)
        hi = np.take(c, np.arange(shape[axis] // 2, shape[axis] - 1), axis=axis)                  # all but the wrapping position
        assert np.abs(hi).max() <= 1e-13 * shape[axis]
        wrapping = np.take(c, [shape[axis] - 1], axis=axis)
        assert np.abs(wrapping).max() > 0.1


@pytest.mark.parametrize("wavelet", ["haar", "db2"])
@pytest.mark.parametrize("Ns,levels", SHAPES)
def test_reference_shift_equivariance(Ns, levels, wavelet):
    """A cyclic shift by 2^L along an axis shifts every band of level l by 2^(L − l) along it; so the proximal map commutes with the shift."""
    a = _random(Ns, seed=1)
    t = 0.3
    prox = lambda v: W.inverse(W.shrink(v, wavelet, levels, t)[0], wavelet, levels)      # noqa: E731
    for axis in range(len(Ns)):
        s = 2 ** levels
        assert np.linalg.norm(prox(np.roll(a, s, axis=axis)) - np.roll(prox(a), s, axis=axis)) <= 1e-13 * np.linalg.norm(a)
        c, cs = W.forward(a, wavelet, levels), W.forward(np.roll(a, s, axis=axis), wavelet, levels)
        n = a.shape[axis] >> levels
        corner = tuple(slice(0, d >> levels) for d in a.shape)
        assert np.linalg.norm(cs[corner] - np.roll(c[corner], 1, axis=axis)) <= 1e-13 * np.linalg.norm(a) and n >= 1
    odd = prox(np.roll(a, 1, axis=0))                                                           # not a multiple of 2^L: another pairing
    assert np.linalg.norm(odd - np.roll(prox(a), 1, axis=0)) > 1e-3 * np.linalg.norm(a)


def test_reference_shrink():
    a = _random((24, 40), seed=2)
    c = W.forward(a, "db2", 3)
    mask = W.detail_mask(c.shape, 3)
    s, l1 = W.shrink(a, "db2", 3, 0.5)
    assert np.array_equal(s[~mask], c[~mask])                                                   # the approximation is never thresholded
    assert np.allclose(np.abs(s[mask]), np.maximum(np.abs(c[mask]) - 0.5, 0.0), rtol=0, atol=1e-13)
    assert abs(l1 - np.abs(s[mask]).sum()) <= 1e-12 * l1
    assert np.array_equal(W.shrink(a, "db2", 3, 0.0)[0], c)
    assert not W.shrink(a, "db2", 3, 2 * np.abs(c).max())[0][mask].any()
    low = W.forward(a.astype(np.complex64), "db2", 3)
    assert low.dtype == np.complex64 and np.linalg.norm(low - c) <= 1e-5 * np.linalg.norm(c)


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
    assert nufft.lib.nufft_sizeof_wavelet_params() == C.sizeof(L.NufftWaveletParams) == 16
    assert nufft.lib.nufft_sizeof_wavelet_info() == C.sizeof(L.NufftWaveletInfo) == 72
    for name, value in (("NUFFT_WAVELET_HAAR", L.WAVELET_HAAR), ("NUFFT_WAVELET_DB2", L.WAVELET_DB2)):
        assert re.search(name + r"\s*=\s*" + str(value) + r"\b", header), name
    assert nufft.lib.nufft_version() == 104      # added without an ABI bump: detected by symbol
    assert callable(nufft.WaveletTransform) and all(hasattr(nufft.WaveletTransform, m) for m in ("forward", "inverse", "shrink"))


def _create(nufft, handle, wavelet, levels, struct_size=None, for_operator=False):
    L = nufft._lib
    prm = L.NufftWaveletParams()
    prm.struct_size = C.sizeof(L.NufftWaveletParams) if struct_size is None else struct_size
    prm.wavelet, prm.levels = wavelet, levels
    h = C.c_void_p()
    fn = nufft.lib.nufft_wavelet_create_for_operator if for_operator else nufft.lib.nufft_wavelet_create
    rc = fn(C.byref(h), handle, C.byref(prm))
    assert not h.value
    return rc, nufft.lib.nufft_last_error_message().decode()


def test_refusals_without_a_device(nufft):
    L, lib = nufft._lib, nufft.lib
    plan = nufft.PlanNUFFT(torch.complex128, (24, 40), backend=None)
    op = nufft.ToeplitzOperator(plan)
    for handle, for_op in ((plan._handle, False), (op._handle, True)):
        rc, msg = _create(nufft, handle, L.WAVELET_DB2, 3, for_operator=for_op)                # every rule passes: only the device is missing
        assert rc == L.ERR_NO_DEVICE and "host-only" in msg
        assert _create(nufft, handle, L.WAVELET_HAAR, 4, for_operator=for_op)[0] == L.ERR_INVALID_ARG      # 24 is no multiple of 16
        assert _create(nufft, handle, 2, 3, for_operator=for_op)[0] == L.ERR_INVALID_ARG                   # unknown wavelet
        assert _create(nufft, handle, L.WAVELET_HAAR, 0, for_operator=for_op)[0] == L.ERR_INVALID_ARG
        assert _create(nufft, handle, L.WAVELET_HAAR, 3, struct_size=8, for_operator=for_op)[0] == L.ERR_INVALID_ARG
    small = nufft.PlanNUFFT(torch.complex64, (8, 16), backend=None)
    rc, msg = _create(nufft, small._handle, L.WAVELET_DB2, 3)                                  # 8 / 2^3 = 1 < 2: the deepest input is shorter than the filter
    assert rc == L.ERR_INVALID_ARG and "at least 2" in msg
    assert _create(nufft, small._handle, L.WAVELET_HAAR, 3)[0] == L.ERR_NO_DEVICE              # Haar needs no such room
    assert _create(nufft, small._handle, L.WAVELET_DB2, 2)[0] == L.ERR_NO_DEVICE
    real = nufft.PlanNUFFT(torch.float64, (24, 40), backend=None)
    rc, msg = _create(nufft, real._handle, L.WAVELET_HAAR, 3)
    assert rc == L.ERR_UNSUPPORTED and "complex plan" in msg
    h = C.c_void_p()
    prm = L.NufftWaveletParams(struct_size=16, wavelet=0, levels=1)
    assert lib.nufft_wavelet_create(C.byref(h), None, C.byref(prm)) == L.ERR_INVALID_ARG
    assert lib.nufft_wavelet_create(C.byref(h), plan._handle, None) == L.ERR_INVALID_ARG
    assert lib.nufft_wavelet_create(None, plan._handle, C.byref(prm)) == L.ERR_INVALID_ARG
    assert lib.nufft_wavelet_forward(None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_wavelet_inverse(None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_wavelet_shrink(None, None, None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_wavelet_get_info(None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_wavelet_destroy(None) == 0
    for bad in (lambda: nufft.WaveletTransform(plan, "db2", 3), lambda: nufft.WaveletTransform(op, "haar", 3),
                lambda: nufft.WaveletTransform(real, "haar", 3), lambda: nufft.WaveletTransform(plan, "db4", 3),
                lambda: nufft.WaveletTransform(plan, "haar", 2.0), lambda: nufft.WaveletTransform(object())):
        with pytest.raises(ValueError):
            bad()
