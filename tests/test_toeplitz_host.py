"""Toeplitz normal operator without a GPU: the numpy reference against the exact Gram product, the real-plan failure that
justifies the refusal, the ABI (header, ctypes mirror, symbols) and host-only objects (path choice, sizes, refusals)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import toeplitz_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(8,), (9,), (8, 6), (7, 10), (6, 5, 4)]
ENTRY_POINTS = ("nufft_toeplitz_create", "nufft_toeplitz_destroy", "nufft_toeplitz_get_info", "nufft_toeplitz_set_spectrum",
                "nufft_toeplitz_set_points", "nufft_toeplitz_apply", "nufft_toeplitz_multiplier_ptr", "nufft_sizeof_toeplitz_info")


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


def _problem(Ns, Np=60, seed=0):
    rng = np.random.default_rng(seed)
    xs = [rng.random(Np) * 2 * np.pi for _ in Ns]
    w = rng.random(Np) + 0.1
    u = rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1])
    return xs, w, u


@pytest.mark.parametrize("Ns", SIZES)
@pytest.mark.parametrize("fftshift", [False, True])
def test_reference_matches_exact_gram(Ns, fftshift):
    xs, w, u = _problem(Ns)
    got, K = R.toeplitz_gram(Ns, xs, w, u, fftshift)
    ref = R.exact_gram(Ns, xs, w, u, fftshift)
    assert R.rel(got, ref) <= 1e-12
    assert np.max(np.abs(K.imag)) <= 1e-12 * np.max(np.abs(K.real))      # real weights, Nyquist planes zeroed: K is real


def test_nyquist_planes_are_never_used():
    # garbage in the Nyquist planes of T changes nothing once they are zeroed: differences of the plan's modes stay within ±(N − 1)
    Ns = (8, 6)
    xs, w, u = _problem(Ns)
    T = R.exact_spectrum(Ns, xs, w)
    T2 = T.copy()
    T2[Ns[1], :] = 1e3
    T2[:, Ns[0]] = -7e2j
    assert np.array_equal(R.multiplier(Ns, T), R.multiplier(Ns, T2))


def test_real_plan_construction_fails_for_even_sizes():
    rng = np.random.default_rng(3)
    errs = {}
    for N in (8, 9):
        x = rng.random(60) * 2 * np.pi
        w = rng.random(60) + 0.1
        u = rng.standard_normal(N // 2 + 1) + 1j * rng.standard_normal(N // 2 + 1)
        u[0] = u[0].real                        # a c2r transform ignores the imaginary part of k = 0
        errs[N] = R.rel(R.real_plan_toeplitz_1d(N, x, w, u), R.real_plan_gram_1d(N, x, w, u))
    assert errs[8] > 1e-2, errs                 # the mode +N/2 of the Hermitian extension aliases in the 2N embedding
    assert errs[9] <= 1e-12, errs               # odd sizes have no such mode


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
    assert nufft.lib.nufft_sizeof_toeplitz_info() == C.sizeof(nufft._lib.NufftToeplitzInfo)
    assert nufft.lib.nufft_version() == 104      # added without an ABI bump: detected by symbol
    assert callable(nufft.ToeplitzOperator) and hasattr(nufft.NFFTPlan, "toeplitz")


def _host_op(nufft, Ns, Z=torch.complex128, **kw):
    return nufft.ToeplitzOperator(nufft.PlanNUFFT(Z, Ns, backend=None, **kw))


def _pad(b):
    return (max(b, 16) + 255) // 256 * 256


@pytest.mark.parametrize("Ns,path", [((32, 48), "fused"), ((64, 64, 64), "fused"), ((256, 256, 256), "fused"),
                                     ((100,), "dense"), ((30, 30), "dense"), ((33, 32, 32), "dense"), ((64,), "dense")])
@pytest.mark.parametrize("Z", [torch.complex128, torch.complex64])
def test_host_only_path_and_sizes(nufft, Ns, path, Z):
    op = _host_op(nufft, Ns, Z, ntransforms=2, fftshift=True)
    i = op.info()
    assert op.path == path
    assert i.ndim == len(Ns) and i.ntransforms == 2 and i.fftshift == 1 and i.device == -1 and i.has_spectrum == 0
    assert i.dtype == (nufft._lib.F64 if Z == torch.complex128 else nufft._lib.F32)
    N = list(Ns) + [1] * (3 - len(Ns))
    N2 = [2 * n for n in Ns] + [1] * (3 - len(Ns))
    assert [i.N[d] for d in range(3)] == N and [i.N2[d] for d in range(3)] == N2
    assert op.padded_shape == tuple(2 * n for n in reversed(Ns))
    rb = 8 if Z == torch.complex128 else 4
    cells = N2[0] * N2[1] * N2[2]
    assert i.multiplier_bytes == cells * rb
    # predicted workspace: K, then the two intermediates (fused; the first only in 3-D) or the 2N work grid (dense), then the tables
    big = _pad(cells * rb)
    if path == "fused":
        big += _pad(N[0] * N2[1] * N2[2] * 2 * rb) + (_pad(N[0] * N[1] * N2[2] * 2 * rb) if len(Ns) == 3 else 0)
    else:
        big += _pad(cells * 2 * rb)
    tables = i.workspace_bytes - big
    assert 0 < tables <= 64 * 1024 + 6 * 256 + 7 * sum(N2) * 2 * rb
    if path == "fused":
        assert i.workspace_bytes < _pad(cells * 2 * rb) + _pad(cells * rb)      # less than K plus the grid it never builds


def test_development_switch_forces_the_dense_path(nufft):
    assert _host_op(nufft, (32, 48), options={"NUFFT_TOEPLITZ_FUSED": 0}).path == "dense"
    assert _host_op(nufft, (32, 48), options={"NUFFT_TOEPLITZ_FUSED": 1}).path == "fused"


def test_real_plan_is_refused_with_the_reason(nufft):
    L = nufft._lib
    p = nufft.PlanNUFFT(torch.float64, (16, 16), backend=None)
    h = C.c_void_p()
    assert nufft.lib.nufft_toeplitz_create(C.byref(h), p._handle) == L.ERR_UNSUPPORTED
    assert not h.value
    msg = nufft.lib.nufft_last_error_message().decode()
    assert "complex plan" in msg and "Hermitian" in msg
    with pytest.raises(ValueError):
        nufft.ToeplitzOperator(p)
    assert nufft.lib.nufft_toeplitz_create(C.byref(h), None) == L.ERR_INVALID_ARG
    assert nufft.lib.nufft_toeplitz_create(None, p._handle) == L.ERR_INVALID_ARG


def test_device_entry_points_refuse_host_only_objects(nufft):
    L, lib = nufft._lib, nufft.lib
    op = _host_op(nufft, (32, 32))
    h = op._handle
    # the device check comes first: null tables do not change the answer
    assert lib.nufft_toeplitz_apply(h, None, None, None) == L.ERR_NO_DEVICE
    assert lib.nufft_toeplitz_set_spectrum(h, None, None) == L.ERR_NO_DEVICE
    assert lib.nufft_toeplitz_set_points(h, None, 0, None, None, None) == L.ERR_NO_DEVICE
    assert lib.nufft_toeplitz_multiplier_ptr(h, C.byref(C.c_void_p()), None) == L.ERR_NO_DEVICE
    assert lib.nufft_toeplitz_apply(None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_toeplitz_get_info(h, None) == L.ERR_INVALID_ARG
    u = torch.zeros(op.shape, dtype=torch.complex128)
    with pytest.raises(ValueError):
        op.apply(u)
    with pytest.raises(ValueError):
        op.set_points((torch.zeros(3, dtype=torch.float64),) * 2)
    with pytest.raises(ValueError):
        op.multiplier()


def test_info_writes_only_the_callers_struct_size(nufft):
    op = _host_op(nufft, (32, 48))
    i = nufft._lib.NufftToeplitzInfo()
    i.struct_size = nufft._lib.NufftToeplitzInfo.N.offset       # a caller that knows the header only up to `N`
    i.workspace_bytes = -5
    assert nufft.lib.nufft_toeplitz_get_info(op._handle, C.byref(i)) == 0
    assert i.path == nufft._lib.TOEPLITZ_PATH_FUSED and i.workspace_bytes == -5 and i.N[0] == 0


def test_the_plan_may_go_first(nufft):
    p = nufft.PlanNUFFT(torch.complex64, (40, 32), backend=None)
    op = nufft.ToeplitzOperator(p)
    p.close()
    assert op.path == "fused" and op.info().N[0] == 40
    op.close()
    op.close()
