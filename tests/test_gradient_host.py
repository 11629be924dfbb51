"""Type-2 gradients without a GPU: the numpy window derivatives of tests/grad_reference.py against central differences of the
oracle's windows, the new C entry points and their refusals on host-only plans, and the numpy gather against exact sums."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_reference as GR  # noqa: E402
from oracle import nufft_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


KERNELS = [O.KERNEL_BKB, O.KERNEL_KB, O.KERNEL_GAUSSIAN, O.KERNEL_BSPLINE]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("evalmode", [O.DIRECT, O.FAST_APPROXIMATION])
@pytest.mark.parametrize("M", [2, 4, 7, 10])
def test_window_derivatives_match_central_differences(kernel, evalmode, M):
    plan = O.OraclePlan((48,), is_real=False, M=M, sigma=2.0, evalmode=evalmode, kernel=kernel)
    N = plan.Nover[0]
    rng = np.random.default_rng(M + 10 * kernel + 100 * evalmode)
    cells = rng.integers(0, N, 64)
    X = rng.uniform(0.05, 0.95, 64)                     # away from the cell edges: the stencil does not move
    x = (cells + X) * (O.TWO_PI / N)
    _, vals, ders = GR.window_derivatives(plan, 0, x)
    h = 1e-5 * (O.TWO_PI / N)
    _, vp = O.evaluate_window(plan, 0, x + h)
    _, vm = O.evaluate_window(plan, 0, x - h)
    fd = (vp - vm) / (2 * h) * (O.TWO_PI / N)          # d/dX = d/dx * 2π / Ñ
    scale = np.abs(vals).max()
    assert np.abs(ders - fd).max() <= 2e-7 * scale * M, (np.abs(ders - fd).max(), scale)


def test_bkb_ratio_series_meets_closed_form():
    t = np.array([0.999999, 1.0, 1.000001])
    r = GR._bkb_dratio(t)
    assert np.allclose(r[0], r[1], rtol=1e-5) and np.allclose(r[1], r[2], rtol=1e-5)
    assert abs(GR._bkb_dratio(np.array([0.0]))[0] - 1.0 / 3.0) < 1e-16


@pytest.mark.parametrize("is_real", [True, False])
@pytest.mark.parametrize("D", [1, 2])
def test_numpy_gather_against_exact_gradient(is_real, D):
    """The restated gather, on the oracle's own type-2 grid, converges to Σ i k û e^{ikx}: the reference every GPU test
    compares with is itself right."""
    Ns = (32,) if D == 1 else (16, 12)
    plan = O.OraclePlan(Ns, is_real=is_real, M=6, sigma=2.0, evalmode=O.DIRECT)
    rng = np.random.default_rng(3)
    xs = [rng.random(200) * O.TWO_PI for _ in range(D)]
    O.set_points(plan, xs)
    shape = tuple(reversed(plan.size))
    uh = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    v, grids = O.exec_type2(plan, uh, return_grid=True)
    (vg, gg), = GR.interpolate_grad(plan, grids)
    assert O.l2_error(vg, v) < 1e-13
    ev, eg = GR.exact_type2_grad(plan, xs, uh)
    assert O.l2_error(vg, ev) < 1e-9
    for d in range(D):
        assert O.l2_error(gg[d], eg[d]) < 1e-7


def test_gradient_symbols_exported(nufft):
    raw = C.CDLL(nufft.LIB_PATH)
    for name in ("nufft_interpolate_grad", "nufft_exec_type2_grad"):
        assert hasattr(raw, name)
        assert name in nufft._lib.SYMBOLS
    assert callable(nufft.exec_type2_grad) and callable(nufft.interpolate_grad)
    assert callable(nufft.autograd.type1) and callable(nufft.autograd.type2)


def test_gradient_entry_points_refuse_host_only_plans(nufft):
    lib = nufft.lib
    h = C.c_void_p()
    N = (C.c_int64 * 3)(32, 32, 32)
    assert lib.nufft_plan_create(C.byref(h), 1, 0, 3, N, 4, 2.0, 0, 0, 1, 0, 0, -1) == 0
    # the device check comes first: null tables do not change the answer
    assert lib.nufft_interpolate_grad(h, None, None, None) == nufft._lib.ERR_NO_DEVICE
    assert lib.nufft_exec_type2_grad(h, None, None, None, None) == nufft._lib.ERR_NO_DEVICE
    assert lib.nufft_plan_destroy(h) == 0
    assert lib.nufft_interpolate_grad(None, None, None, None) == nufft._lib.ERR_INVALID_ARG
    assert lib.nufft_exec_type2_grad(None, None, None, None, None) == nufft._lib.ERR_INVALID_ARG


def test_python_gradient_calls_refuse_host_only_plans(nufft):
    import torch
    p = nufft.PlanNUFFT(np.complex128, (16, 16), backend=None)
    with pytest.raises(ValueError):
        nufft.exec_type2_grad((torch.zeros(1), torch.zeros(1)), p, torch.zeros(16, 16, dtype=torch.complex128))
    with pytest.raises(ValueError):
        nufft.autograd.type2(nufft.PlanNUFFT(np.float64, (16,), backend=None), (torch.zeros(1),), torch.zeros(9))


def test_version_unchanged(nufft):
    assert nufft.lib.nufft_version() == 104
