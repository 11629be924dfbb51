"""Type-3 plans without a GPU: the fine-grid rule, the refusals of nufft_plan3_create and the ctypes mirrors of its structs."""
import ctypes as C
import math

import pytest
import torch


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


def _smooth235(n):
    for p in (2, 3, 5):
        while n % p == 0:
            n //= p
    return n == 1


def _rule(sigma, M, X, S):
    """Restatement of the parameter rule: (nf, γ, h, X, S) for one dimension."""
    if X == 0 and S == 0:
        X = S = 1.0
    elif X == 0:
        X = 1.0 / S
    elif S == 0:
        S = 1.0 / X
    bound = 2 * sigma * X * S / math.pi + 2 * M + 2
    nf = 4
    while nf < bound or not _smooth235(nf):
        nf += 4
    return nf, nf / (2 * sigma * S), 2 * math.pi / nf, X, S


BOXES = [
    # (sigma, M, source half-widths, target half-widths)
    (2.0, 4, (math.pi,), (64.0,)),
    (2.0, 4, (math.pi, math.pi, math.pi), (64.0, 64.0, 64.0)),
    (1.5, 6, (3.0, 0.5), (100.0, 7.0)),
    (1.25, 2, (10.0,), (1000.0,)),
    (2.0, 10, (0.01, 1.0, 50.0), (0.01, 3.0, 2.0)),
    (2.0, 8, (0.0, 2.0), (5.0, 0.0)),
    (1.75, 5, (0.0,), (0.0,)),
]


def _plan(nufft, ndim, X, S, Z=torch.complex128, **kw):
    return nufft.PlanNUFFT3(Z, ndim, backend=None, source_bounds=[(1.0 - x, 1.0 + x) for x in X],
                            target_bounds=[(-3.0 - s, -3.0 + s) for s in S], **kw)


@pytest.mark.parametrize("sigma,M,X,S", BOXES)
def test_fine_grid_rule(nufft, sigma, M, X, S):
    D = len(X)
    info = _plan(nufft, D, X, S, m=M, sigma=sigma).info()
    for d in range(D):
        nf, gamma, h, Xd, Sd = _rule(sigma, M, X[d], S[d])
        assert info.nf[d] == nf
        assert info.gamma[d] == pytest.approx(gamma, rel=1e-12)
        assert info.h[d] == pytest.approx(h, rel=1e-14)
        assert nf % 4 == 0 and _smooth235(nf)
        # the spread of the rescaled sources never wraps: X/γ + M h <= π
        assert Xd / info.gamma[d] + M * info.h[d] <= math.pi
        assert math.isfinite(info.gamma[d]) and info.gamma[d] > 0
        assert info.source_halfwidth[d] == pytest.approx(Xd) and info.target_halfwidth[d] == pytest.approx(Sd)
        inner = int(math.floor(sigma * nf))
        while not _smooth235(inner):
            inner += 1
        assert info.inner_N_over[d] == inner
    assert info.ndim == D and info.half_support == M and info.sign == -1 and info.device == -1
    assert info.num_sources == -1 and info.num_targets == -1


def test_zero_width_boxes_give_finite_gamma(nufft):
    for X, S in [((0.0,), (0.0,)), ((0.0,), (3.0,)), ((2.0,), (0.0,))]:
        info = _plan(nufft, 1, X, S).info()
        assert math.isfinite(info.gamma[0]) and info.gamma[0] > 0
        assert info.source_halfwidth[0] * info.target_halfwidth[0] == pytest.approx(1.0 if 0.0 in (X[0], S[0]) else X[0] * S[0])


def test_window_shape_is_optimal_for_requested_sigma(nufft):
    # BackwardsKaiserBessel: β = π a γ with a = M (2 - 1/σ) (the plan's rule for σ itself, not for any σ implied by the grid)
    for sigma, M in [(2.0, 4), (1.5, 6)]:
        a = M * (2 - 1 / sigma)
        beta = math.pi * a * max(0.995, math.sqrt(1 - 0.3 / (a * a)))
        assert _plan(nufft, 2, (1.0, 1.0), (9.0, 9.0), m=M, sigma=sigma).info().beta[0] == pytest.approx(beta, rel=1e-14)


def _raw_create(nufft, **over):
    L = nufft._lib
    prm = L.NufftParams()
    prm.struct_size = C.sizeof(L.NufftParams)
    prm.dtype, prm.is_complex, prm.ndim, prm.device = L.F64, 1, 2, -1
    t3 = L.NufftType3Params()
    t3.struct_size = C.sizeof(L.NufftType3Params)
    for d in range(2):
        t3.source_halfwidth[d], t3.target_halfwidth[d] = 1.0, 10.0
    for k, v in over.items():
        obj, field = (t3, k[3:]) if k.startswith("t3_") else (prm, k)
        if isinstance(v, tuple):
            getattr(obj, field)[v[0]] = v[1]
        else:
            setattr(obj, field, v)
    h = C.c_void_p()
    rc = nufft.lib.nufft_plan3_create(C.byref(h), C.byref(prm), C.byref(t3))
    if rc == 0:
        nufft.lib.nufft_plan3_destroy(h)
    return rc


def test_refusals(nufft):
    L = nufft._lib
    assert _raw_create(nufft) == L.OK
    assert _raw_create(nufft, is_complex=0) == L.ERR_INVALID_ARG
    assert _raw_create(nufft, N=(0, 16)) == L.ERR_INVALID_ARG
    assert _raw_create(nufft, N_over=(1, 32)) == L.ERR_INVALID_ARG
    assert _raw_create(nufft, fftshift=1) == L.ERR_INVALID_ARG
    assert _raw_create(nufft, point_transform=1) == L.ERR_INVALID_ARG
    assert _raw_create(nufft, t3_source_halfwidth=(0, -1.0)) == L.ERR_INVALID_ARG
    assert _raw_create(nufft, t3_target_halfwidth=(1, float("inf"))) == L.ERR_INVALID_ARG
    assert _raw_create(nufft, t3_source_center=(0, float("nan"))) == L.ERR_INVALID_ARG
    assert _raw_create(nufft, t3_sign=2) == L.ERR_INVALID_ARG
    assert _raw_create(nufft, ndim=4) == L.ERR_UNSUPPORTED
    assert _raw_create(nufft, dtype=7) == L.ERR_INVALID_ARG
    # an nf beyond 2^30 cells per axis is refused, and the message names nf
    assert _raw_create(nufft, t3_source_halfwidth=(0, 1e6), t3_target_halfwidth=(0, 1e6)) == L.ERR_UNSUPPORTED
    assert "nf" in nufft.lib.nufft_last_error_message().decode()
    with pytest.raises(ValueError):
        nufft.PlanNUFFT3(torch.float64, 1, backend=None)


def test_host_only_plan_has_no_device_path(nufft):
    p = _plan(nufft, 1, (1.0,), (5.0,))
    with pytest.raises(ValueError):
        nufft.set_points3(p, (torch.zeros(3, dtype=torch.float64),), (torch.zeros(3, dtype=torch.float64),))
    L = nufft._lib
    assert nufft.lib.nufft_set_points3(p._handle, 0, None, 0, None, None) == L.ERR_NO_DEVICE
    assert nufft.lib.nufft_exec_type3(p._handle, None, None, None) == L.ERR_NO_DEVICE


def test_struct_mirrors_and_abi_version(nufft):
    L = nufft._lib
    assert nufft.lib.nufft_sizeof_type3_params() == C.sizeof(L.NufftType3Params)
    assert nufft.lib.nufft_sizeof_info3() == C.sizeof(L.NufftInfo3)
    assert nufft.lib.nufft_version() == 104


def test_from_points_pads_the_bounding_box(nufft):
    xs = (torch.tensor([0.0, 1.0, 3.0], dtype=torch.float64),)
    ss = (torch.tensor([-5.0, 7.0], dtype=torch.float64),)
    p = nufft.PlanNUFFT3.from_points(torch.complex128, xs, ss, backend=None)
    i = p.info()
    assert i.source_halfwidth[0] > 1.5 and i.source_halfwidth[0] == pytest.approx(1.5, rel=1e-14)
    assert i.target_halfwidth[0] > 6.0 and i.target_halfwidth[0] == pytest.approx(6.0, rel=1e-14)
