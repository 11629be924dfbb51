"""Sample-density compensation without a GPU: the numpy restatement (dcf_reference.py: scale invariance, normalisation, positivity,
periodicity, its effect on CG, its convergence history) and the C ABI (header, ctypes mirror, symbols, struct sizes, a host-only object,
refusals that need no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import cg_reference as CG
import dcf_reference as D
import toeplitz_reference as R
from oracle import nufft_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("nufft_dcf_create", "nufft_dcf_destroy", "nufft_dcf_set_points", "nufft_dcf_compute", "nufft_dcf_get_info",
                "nufft_dcf_get_result", "nufft_dcf_history", "nufft_sizeof_dcf_params", "nufft_sizeof_dcf_info")


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


def clustered(ndim, Np, seed):
    """Half uniform, half N(0, 0.4²) per coordinate, folded to [0, 2π)."""
    rng = np.random.default_rng(seed)
    h = Np // 2
    xs = [np.mod(np.concatenate([rng.random(h) * 2 * np.pi, 0.4 * rng.standard_normal(Np - h)]), 2 * np.pi) for _ in range(ndim)]
    return xs, rng


def jittered_1d(Np=400, seed=11):
    return [np.sort(np.random.default_rng(seed).random(Np) * 2 * np.pi)]


def cg_count(Ns, xs, w, y, rtol=1e-6, max_iter=600):
    """Iterations CG takes on A^H W A x = A^H W y with the exact Toeplitz apply."""
    K = R.multiplier(Ns, R.exact_spectrum(Ns, xs, w)).real
    b = O.nudft_type1(R.mode_lists(Ns), xs, w * y)
    got = CG.cg(lambda p: R.apply(Ns, K, p), b, rtol=rtol, max_iter=max_iter)
    assert got["status"] == CG.CONVERGED
    return got["iterations"]


def test_first_iterate_does_not_depend_on_the_scale_of_the_start():
    xs, _ = clustered(2, 1500, 3)
    Np = len(xs[0])
    a = D.pipe_menon(D.make_plan((24, 20)), xs, max_iter=1, normalize="none")
    b = D.pipe_menon(D.make_plan((24, 20)), xs, max_iter=1, w0=np.full(Np, 1e-20), normalize="none")
    assert a["iterations"] == b["iterations"] == 1
    assert np.max(np.abs(a["w"] / b["w"] - 1)) <= 1e-13           # a few roundings of the products with 1e-20
    assert np.isnan(a["history"][0]) and b["history"][0] > 1.0    # δ_0 is reported for a caller's start only


@pytest.mark.parametrize("Ns,dtype", [((64,), np.float64), ((24, 20), np.float64), ((12, 10, 8), np.float64), ((24, 20), np.float32)])
def test_weights_are_positive_and_sum_to_one(Ns, dtype):
    xs, _ = clustered(len(Ns), 1200, 5)
    xs = [x.astype(dtype) for x in xs]
    got = D.pipe_menon(D.make_plan(Ns, dtype=dtype), xs, max_iter=8)
    w = got["w"]
    assert w.dtype == dtype and got["status"] == D.MAX_ITER and got["iterations"] == 8
    assert np.all(w > 0) and np.all(np.isfinite(w))
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 4 * np.finfo(dtype).eps
    raw = D.pipe_menon(D.make_plan(Ns, dtype=dtype), xs, max_iter=8, normalize="none")["w"]
    assert np.max(np.abs(raw / raw.astype(np.float64).sum() / w - 1)) <= 4 * np.finfo(dtype).eps


def test_weights_are_periodic_and_follow_the_point_convention():
    xs, _ = clustered(2, 1500, 9)
    base = D.pipe_menon(D.make_plan((24, 20)), xs, max_iter=6)["w"]
    shifted = D.pipe_menon(D.make_plan((24, 20)), [xs[0] + 2 * np.pi, xs[1] - 2 * np.pi], max_iter=6)["w"]
    assert np.max(np.abs(shifted / base - 1)) <= 1e-9            # the fold of x ± 2π moves a point by a few ulp of 2π
    # the same physical points in the NFFT convention: x_nfft in [-1/2, 1/2) with x = -2π x_nfft (mod 2π)
    xn = [np.mod(-x / (2 * np.pi) + 0.5, 1.0) - 0.5 for x in xs]
    nfft = D.pipe_menon(D.make_plan((24, 20), point_transform=O.POINT_TRANSFORM_NFFT), xn, max_iter=6)["w"]
    assert np.max(np.abs(nfft / base - 1)) <= 1e-9


def test_breakdown_leaves_the_start_alone():
    xs, _ = clustered(1, 300, 2)
    w0 = np.full(300, 0.5)
    w0[17] = 0.0
    got = D.pipe_menon(D.make_plan((32,)), xs, max_iter=5, w0=w0)
    assert got["status"] == D.BREAKDOWN and got["iterations"] == 0 and np.array_equal(got["w"], w0)
    bad = [xs[0].copy()]
    bad[0][5] = np.nan
    with np.errstate(invalid="ignore"):
        got = D.pipe_menon(D.make_plan((32,)), bad, max_iter=5)
    assert got["status"] == D.BREAKDOWN and got["iterations"] == 0
    empty = D.pipe_menon(D.make_plan((32,)), [np.zeros(0)], max_iter=5)
    assert empty["w"].size == 0 and empty["iterations"] == 0


def test_tolerance_stops_before_the_division():
    x = jittered_1d()
    full = D.pipe_menon(D.make_plan((64,)), x, max_iter=12, normalize="none")
    h = full["history"]
    tol = float(np.sqrt(h[6] * h[7]))
    assert h[7] < tol < h[6]
    got = D.pipe_menon(D.make_plan((64,)), x, max_iter=12, tol=tol, normalize="none")
    assert got["status"] == D.CONVERGED and got["iterations"] == 7 and got["residual"] == h[7]
    assert np.all(np.isnan(got["history"][8:])) and np.array_equal(got["history"][1:8], h[1:8])
    short = D.pipe_menon(D.make_plan((64,)), x, max_iter=7, normalize="none")
    assert np.array_equal(short["w"], got["w"])                   # w^7: the iterate δ_7 was measured on


def test_weights_halve_the_cg_iterations_on_a_clustered_set():
    # 32 × 32 modes, 3000 uniform + 3000 N(0, 0.4²) points (seed 7), m = 4, σ = 2, BKB, 30 iterations of the weights; CG with the exact
    # Toeplitz apply at rtol 1e-6.  Measured with this seed: 186 iterations with uniform weights 1/Np, 52 with the Pipe–Menon weights.
    Ns = (32, 32)
    xs, rng = clustered(2, 6000, 7)
    Np = len(xs[0])
    w = D.pipe_menon(D.make_plan(Ns, M=4, sigma=2.0, kernel=O.KERNEL_BKB), xs, max_iter=30)["w"]
    y = rng.standard_normal(Np) + 1j * rng.standard_normal(Np)
    uniform, weighted = cg_count(Ns, xs, np.full(Np, 1.0 / Np), y), cg_count(Ns, xs, w, y)
    print(f"CG iterations: uniform weights {uniform}, Pipe-Menon weights {weighted}")
    assert 2 * weighted <= uniform, (uniform, weighted)


def test_convergence_history_of_the_reference():
    # δ_k after 5, 10, 20 and 30 iterations, measured with these seeds:
    #   2-D clustered set (32 × 32, 6000 points, seed 7):  0.1040 / 0.0861 / 0.0787 / 0.0728
    #   1-D jittered set (N = 64, 400 sorted uniform points, seed 11):  0.0645 / 0.0286 / 0.0094 / 0.0075
    # Convergence in the maximum norm is slow: that is the method, and why the default is a fixed iteration count.
    two = D.pipe_menon(D.make_plan((32, 32)), clustered(2, 6000, 7)[0], max_iter=31)["history"]
    one = D.pipe_menon(D.make_plan((64,)), jittered_1d(), max_iter=31)["history"]
    for name, h, recorded in (("2-D", two, (0.1040, 0.0861, 0.0787, 0.0728)), ("1-D", one, (0.0645, 0.0286, 0.0094, 0.0075))):
        got = [float(h[k]) for k in (5, 10, 20, 30)]
        print(name, "delta after 5, 10, 20, 30 iterations:", got)
        assert np.isnan(h[0]) and np.all(np.isfinite(h[1:]))
        assert h[30] < h[5]
        assert np.allclose(got, recorded, rtol=0, atol=6e-5)      # the recorded digits


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
    assert nufft.lib.nufft_sizeof_dcf_params() == C.sizeof(L.NufftDcfParams) == 24
    assert nufft.lib.nufft_sizeof_dcf_info() == C.sizeof(L.NufftDcfInfo) == 128
    for name, value in (("NUFFT_DCF_MAX_ITER", L.DCF_MAX_ITER), ("NUFFT_DCF_CONVERGED", L.DCF_CONVERGED),
                        ("NUFFT_DCF_BREAKDOWN", L.DCF_BREAKDOWN), ("NUFFT_DCF_NORMALIZE_SUM", L.DCF_NORMALIZE["sum"]),
                        ("NUFFT_DCF_NORMALIZE_NONE", L.DCF_NORMALIZE["none"])):
        assert re.search(name + r"\s*=\s*" + str(value) + r"\b", header), name
    assert (L.DCF_MAX_ITER, L.DCF_CONVERGED, L.DCF_BREAKDOWN) == (D.MAX_ITER, D.CONVERGED, D.BREAKDOWN)
    assert nufft.lib.nufft_version() == 104      # added without an ABI bump: detected by symbol
    assert callable(nufft.DensityCompensation) and callable(nufft.density_weights) and hasattr(nufft.NFFTPlan, "sdc")
    assert {"DensityCompensation", "density_weights"} <= set(nufft.__all__)


def _params(nufft, **kw):
    p = nufft._lib.NufftDcfParams()
    p.struct_size = C.sizeof(nufft._lib.NufftDcfParams)
    p.max_iter, p.check_every, p.normalize, p.tol = 10, 0, 0, 0.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("Z,Ns,M,sigma", [(torch.float64, (32, 32), 4, 2.0), (torch.complex64, (30,), 4, 1.25),
                                          (torch.complex128, (35, 64, 40), 6, 1.5)])
def test_host_only_object_answers_get_info(nufft, Z, Ns, M, sigma):
    plan = nufft.PlanNUFFT(Z, Ns, m=M, sigma=sigma, backend=None)
    dc = nufft.DensityCompensation(plan, maxiter=12, tol=1e-3, normalize="none")
    plan_beta = list(plan.info().beta)
    plan.close()                                                  # no pointer to the parent is kept
    i = dc.info()
    real = np.float32 if Z in (torch.float32, torch.complex64) else np.float64
    o = D.make_plan(Ns, dtype=real, M=M, sigma=sigma)
    assert (i.ndim, i.dtype, i.device) == (len(Ns), 0 if real == np.float32 else 1, -1)
    assert (i.max_iter, i.check_every, i.normalize, i.tol) == (12, 0, 1, 1e-3)
    assert dc.oversampled_dims == o.Nover                         # the REAL plan's grid: even along dimension 1
    assert (i.capacity, i.num_points, i.iterations_enqueued, i.plan_bytes, i.workgroups) == (0, -1, -1, 0, 0)
    assert i.workspace_bytes == 16384 + 256 + 256                 # partials, scalars, history (12 doubles, padded); no v yet
    # the parent's shape parameter (BKB) on the real plan's grid: windows scaled by 2^k_d, k_d = -round(log2(sinh(β_d) / π)); C carries both
    assert i.window_scale_log2 == -2 * sum(int(np.rint(np.log2(np.sinh(i.beta[d]) / np.pi))) for d in range(len(Ns)))
    assert list(i.beta) == list(plan_beta)
    for what in (lambda: dc.set_points(torch.zeros(4)), dc.compute, lambda: dc.iterations, dc.history):
        with pytest.raises(ValueError):
            what()
    dc.close()
    with pytest.raises(ValueError):
        dc.info()


def test_complex_parent_with_an_odd_grid_reports_the_grid_used(nufft):
    plan = nufft.PlanNUFFT(torch.complex128, (33,), m=4, sigma=1.25, backend=None)
    dc = nufft.DensityCompensation(plan)
    assert plan.oversampled_dims == (45,) and dc.oversampled_dims == (48,)
    assert dc.info().beta[0] == plan.info().beta[0]               # the parent's window shape, on the finer grid


def test_refusals_that_need_no_device(nufft):
    L, lib = nufft._lib, nufft.lib
    plan = nufft.PlanNUFFT(torch.complex128, (32, 32), backend=None)
    h = C.c_void_p()
    for kw in (dict(max_iter=0), dict(max_iter=-3), dict(max_iter=(1 << 24) + 1), dict(check_every=-1), dict(tol=-1e-3),
               dict(tol=float("nan")), dict(tol=float("inf")), dict(normalize=2), dict(struct_size=16)):
        assert lib.nufft_dcf_create(C.byref(h), plan._handle, C.byref(_params(nufft, **kw))) == L.ERR_INVALID_ARG, kw
        assert not h.value
    assert lib.nufft_dcf_create(C.byref(h), None, C.byref(_params(nufft))) == L.ERR_INVALID_ARG
    assert lib.nufft_dcf_create(C.byref(h), plan._handle, None) == L.ERR_INVALID_ARG
    assert lib.nufft_dcf_create(None, plan._handle, C.byref(_params(nufft))) == L.ERR_INVALID_ARG
    assert lib.nufft_dcf_create(C.byref(h), plan._handle, C.byref(_params(nufft))) == 0 and h.value
    buf = (C.c_double * 10)()
    table = (C.c_void_p * 2)()
    assert lib.nufft_dcf_set_points(h, 4, table, None) == L.ERR_NO_DEVICE
    assert "host-only" in lib.nufft_last_error_message().decode()
    assert lib.nufft_dcf_compute(h, C.cast(buf, C.c_void_p), 0, None) == L.ERR_NO_DEVICE
    assert lib.nufft_dcf_get_result(h, None, None, None, None) == L.ERR_NO_DEVICE
    assert lib.nufft_dcf_history(h, buf, 10, None) == L.ERR_NO_DEVICE
    assert lib.nufft_dcf_get_info(h, None) == L.ERR_INVALID_ARG
    assert lib.nufft_dcf_destroy(h) == 0
    assert lib.nufft_dcf_set_points(None, 0, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_dcf_compute(None, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_dcf_get_info(None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_dcf_get_result(None, None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_dcf_history(None, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_dcf_destroy(None) == 0
    for bad in (dict(maxiter=2.5), dict(check_every=True), dict(normalize="mean"), dict(tol=-1.0)):
        with pytest.raises(ValueError):
            nufft.DensityCompensation(plan, **bad)
    with pytest.raises(ValueError):
        nufft.DensityCompensation(object())
    with pytest.raises(ValueError):
        nufft.density_weights(plan, torch.zeros(8, 2, dtype=torch.float64))
