"""Type-3 gradients without a GPU: the window's logarithmic derivative against central differences of ϕ̂, the refusals of
nufft_exec_type3_grad and the adjoint plan's parameters."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import type3_grad_reference as R


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


_KERNEL_CLASS = {"bkb": "BackwardsKaiserBesselKernel", "kb": "KaiserBesselKernel", "gauss": "GaussianKernel",
                 "bspline": "BSplineKernel"}


def _window(nufft, kernel, M, sigma, nf=64):
    """(dx, param) of a spreading window of this kind on a grid of nf cells: β from a host-only plan's rule, τ = 2 (β dx)²."""
    p = nufft.PlanNUFFT3(torch.complex128, 1, m=M, sigma=sigma, kernel=getattr(nufft, _KERNEL_CLASS[kernel])(), backend=None)
    beta = p.info().beta[0]
    dx = 2 * math.pi / nf
    return dx, (2.0 * (beta * dx) ** 2 if kernel == "gauss" else beta)


def _central(kernel, M, dx, param, k, eps):
    lo, hi = R.phihat(kernel, M, dx, param, k - eps), R.phihat(kernel, M, dx, param, k + eps)
    return (np.log(np.abs(hi)) - np.log(np.abs(lo))) / (2 * eps)


@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("M", [2, 4, 7, 10])
@pytest.mark.parametrize("sigma", [1.25, 2.0])
def test_dlogphihat_matches_central_differences(nufft, kernel, M, sigma):
    dx, param = _window(nufft, kernel, M, sigma)
    kmax = math.pi / (sigma * dx)                       # the band of in-box targets: |γ t| h <= π / σ
    k = np.concatenate([np.linspace(-kmax, kmax, 41), [1e-7, -3e-6, 0.5, 1e-3 / dx]])
    eps = 1e-5 * max(kmax, 1.0)
    got = R.dlogphihat(kernel, M, dx, param, k)
    ref = _central(kernel, M, dx, param, k, eps)
    scale = np.max(np.abs(ref)) + 1e-300
    assert np.all(np.isfinite(got))
    assert np.max(np.abs(got - ref)) <= 1e-6 * scale, (kernel, M, sigma)


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_dlogphihat_series_branches_at_zero(nufft, kernel):
    # k → 0: the series branches meet the closed forms and vanish linearly (ln ϕ̂ is even in k)
    dx, param = _window(nufft, kernel, 4, 2.0)
    k = np.array([0.0, 1e-12, 1e-9, 1e-6])
    got = R.dlogphihat(kernel, 4, dx, param, k)
    assert got[0] == 0.0
    slope = got[1:] / k[1:]
    assert np.allclose(slope, slope[-1], rtol=1e-6)
    assert np.allclose(R.dlogphihat(kernel, 4, dx, param, -k[1:]), -got[1:], rtol=1e-14)


@pytest.mark.parametrize("kernel", ["bkb", "kb"])
def test_dlogphihat_just_past_the_kaiser_bessel_band(nufft, kernel):
    # targets slightly outside the box: z = β² − (w k)² < 0; finite, and still the derivative of the ϕ̂ branch taken there
    M = 4
    dx, beta = _window(nufft, kernel, M, 2.0)
    kband = beta / (M * dx)
    k = kband * np.array([1.0 + 1e-9, 1.001, 1.01, 1.05])
    got = R.dlogphihat(kernel, M, dx, beta, k)
    assert np.all(np.isfinite(got))
    ref = _central(kernel, M, dx, beta, k[1:], 1e-6 * kband)
    assert np.allclose(got[1:], ref, rtol=1e-5)


def test_type3_grad_symbol_exported(nufft):
    raw = C.CDLL(nufft.LIB_PATH)
    assert hasattr(raw, "nufft_exec_type3_grad")
    assert "nufft_exec_type3_grad" in nufft._lib.SYMBOLS
    assert callable(nufft.exec_type3_grad) and callable(nufft.autograd.type3)


def test_exec_type3_grad_refusals_without_device(nufft):
    lib = nufft.lib
    p = nufft.PlanNUFFT3(torch.complex128, 2, backend=None)
    # the device check comes first: null tables do not change the answer
    assert lib.nufft_exec_type3_grad(p._handle, None, None, None, None) == nufft._lib.ERR_NO_DEVICE
    assert lib.nufft_exec_type3_grad(None, None, None, None, None) == nufft._lib.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        nufft.exec_type3_grad(torch.zeros(1, dtype=torch.complex128), (torch.zeros(1, dtype=torch.complex128),) * 2, p,
                              torch.zeros(1, dtype=torch.complex128))


@pytest.mark.parametrize("Z", [torch.complex128, torch.complex64])
@pytest.mark.parametrize("kernel", list(_KERNEL_CLASS))
def test_adjoint_plan_parameters(nufft, Z, kernel):
    sb = [(-2.0, 5.0), (1.0, 1.5), (-40.0, -30.0)]
    tb = [(10.0, 90.0), (-7.0, 3.0), (0.0, 0.0)]
    p = nufft.PlanNUFFT3(Z, 3, m=5, sigma=1.75, kernel=getattr(nufft, _KERNEL_CLASS[kernel])(), sign=+1, ntransforms=2,
                         backend=None, source_bounds=sb, target_bounds=tb)
    a = p.adjoint()
    i, j = p.info(), a.info()
    assert a.sign == -1 and j.sign == -1 and i.sign == 1
    assert a.Z == p.Z and a.ndim == 3 and a.ntransforms == 2 and a.device is None
    assert type(a.kernel) is type(p.kernel) and type(a.kernel_evalmode) is type(p.kernel_evalmode)
    assert j.half_support == i.half_support and j.sigma == i.sigma and j.kernel == i.kernel and j.evalmode == i.evalmode
    assert a.nf == p.nf
    for d in range(3):
        assert j.inner_N_over[d] == i.inner_N_over[d]
        assert j.beta[d] == i.beta[d]
        assert j.source_halfwidth[d] == i.target_halfwidth[d] and j.target_halfwidth[d] == i.source_halfwidth[d]
        assert j.gamma[d] == pytest.approx(j.nf[d] / (2 * j.sigma * j.target_halfwidth[d]), rel=1e-14)
    assert a._source_bounds == tb and a._target_bounds == sb
    assert a.adjoint().info().sign == 1 and a.adjoint().nf == p.nf


def test_adjoint_of_default_boxes(nufft):
    p = nufft.PlanNUFFT3(torch.complex128, 1, backend=None)
    a = p.adjoint()
    assert a.nf == p.nf and a.info().sign == 1
    assert a.info().source_halfwidth[0] == pytest.approx(1.0) and a.info().target_halfwidth[0] == pytest.approx(math.pi)


def test_autograd_type3_refuses_several_transforms(nufft):
    p = nufft.PlanNUFFT3(torch.complex128, 1, ntransforms=2, backend=None)
    x = torch.zeros(3, dtype=torch.float64)
    with pytest.raises(ValueError):
        nufft.autograd.type3(p, (x,), (x,), torch.zeros(3, dtype=torch.complex128))
