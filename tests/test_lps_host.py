"""Low-rank plus sparse reconstruction without a GPU: the numpy reference (lps_reference.py) -- the Gram route against
the SVD, the temporal transform, the descent of the objective, the fixed point -- and the C ABI of the three objects (header, ctypes
mirror, symbols, struct sizes, the refusals that need no device, in the documented order)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lps_cases as LC
import lps_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
ENTRY_POINTS = ("nufft_glr_create", "nufft_glr_create_for_operator", "nufft_glr_destroy", "nufft_glr_get_info", "nufft_glr_apply",
                "nufft_glr_last_sweeps", "nufft_sizeof_glr_info",
                "nufft_tsparse_create", "nufft_tsparse_create_for_operator", "nufft_tsparse_destroy", "nufft_tsparse_get_info",
                "nufft_tsparse_forward", "nufft_tsparse_inverse", "nufft_tsparse_shrink", "nufft_sizeof_tsparse_info",
                "nufft_lps_create", "nufft_lps_destroy", "nufft_lps_set_weights", "nufft_lps_solve", "nufft_lps_get_parts", "nufft_lps_get_info",
                "nufft_lps_get_result", "nufft_lps_history", "nufft_sizeof_lps_params", "nufft_sizeof_lps_info")


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


@pytest.mark.parametrize("Ns,K", LC.HOST_CASES)
def test_gram_route_against_the_svd(Ns, K):
    """256 ε: four times the bar of the locally low-rank map, because the Gram sums run over n cells instead of at most 4096."""
    x = LC.case(Ns, K).b
    sv = P.singular_values(x)
    t = float(np.median(sv))
    want, nuc, zeroed = P.svt(x, t)
    got, nuc_g, sweeps = P.svt_gram(x, t)
    err = LC.rel(got, want)
    print(f"N={Ns} K={K}: svt_gram vs svt {err / EPS:.1f} ε, nuclear norm {abs(nuc_g - nuc) / nuc / EPS:.1f} ε, {sweeps} sweeps, {zeroed}/{K} zeroed")
    assert err <= 256 * EPS and abs(nuc_g - nuc) <= 256 * EPS * nuc and 2 <= sweeps < 24 and 0 < zeroed < K
    assert LC.rel(P.svt_gram(x, 0.0)[0], x) <= 256 * EPS
    assert not P.svt_gram(x, 1.01 * sv[0])[0].any() and not P.svt_gram(np.zeros_like(x), t)[0].any()


@pytest.mark.parametrize("K", [1, 2, 3, 9, 17, 32])
def test_temporal_transform_is_unitary_and_inverts(K):
    rng = np.random.default_rng(K)
    x = rng.standard_normal((K, 7, 5)) + 1j * rng.standard_normal((K, 7, 5))
    for tr in P.TRANSFORMS:
        c = P.tdft(x, tr)
        assert abs(np.linalg.norm(c) - np.linalg.norm(x)) <= 8 * EPS * np.linalg.norm(x)
        assert LC.rel(P.tdft(c, tr, inverse=True), x) <= 8 * EPS
    w = np.exp(-2j * np.pi * np.outer(np.arange(K), np.arange(K)) / K) / np.sqrt(K)      # the definition, as a matrix
    assert LC.rel(P.tdft(x, "dft"), np.einsum("kc,c...->k...", w, x)) <= 4 * K * EPS
    out, l1, share = P.tshrink(P.tdft(x, "dft"), 0.5)
    assert abs(l1 - np.abs(out).sum()) <= 1e-12 * l1 and share == np.mean(out == 0) and 0 < share < 1
    assert np.abs(np.abs(out[out != 0]) - (np.abs(P.tdft(x, "dft"))[out != 0] - 0.5)).max() <= 8 * EPS


@pytest.mark.parametrize("transform", P.TRANSFORMS)
def test_objective_never_increases_without_momentum(transform):
    """Every one of 50 iterations: the reference is run to 1, 2, ... 50 iterations (a shorter run is a prefix of a longer one)."""
    c = LC.case((7, 5), 3)
    nuc, l1 = c.weights(transform)
    values = [P.objective(c.apply, c.b, 0 * c.b, 0 * c.b, nuc, l1, transform)]
    for it in range(1, 51):
        r = P.lps(c.apply, c.b, nuc, l1, c.step(), transform=transform, momentum=False, tol=0.0, max_iter=it)
        values.append(P.objective(c.apply, c.b, r["L"], r["S"], nuc, l1, transform))
    assert all(b <= a + 1e-12 * abs(a) for a, b in zip(values, values[1:])) and values[-1] < values[0]


def test_converged_reference_is_a_fixed_point():
    """(32, 40) K = 3, tol 1e-6: 363 iterations with momentum, 488 without (measured on the CPU); the residual of one more step < 1e-5."""
    c = LC.case((32, 40), 3)
    nuc, l1 = c.weights("dft")
    for momentum in (True, False):
        r = P.lps(c.apply, c.b, nuc, l1, c.step(), momentum=momentum, tol=1e-6, max_iter=5000)
        res = P.fixed_point_residual(c.apply, c.b, r["L"], r["S"], nuc, l1, c.step())
        tenth = P.lps(c.apply, c.b, nuc, l1, c.step(), momentum=momentum, tol=0.0, max_iter=10)
        print(f"momentum {momentum}: {r['iterations']} iterations, residual {res:.2e}, tenth iteration: {tenth['zeroed_sv']}/3 zeroed, share {tenth['zero_share']:.2f}")
        assert r["status"] == P.CONVERGED and res < 1e-5
        assert 0 < tenth["zeroed_sv"] < 3 and 0.2 <= tenth["zero_share"] <= 0.95
        assert np.array_equal(r["x"], r["L"] + r["S"]) and r["history"].shape == (r["iterations"], 3)
        assert abs(r["history"][-1, 1] - P.singular_values(r["L"]).sum()) <= 1e-10 * r["history"][-1, 1]
        assert abs(r["history"][-1, 2] - np.abs(P.tdft(r["S"])).sum()) <= 1e-10 * r["history"][-1, 2]


@pytest.mark.parametrize("Ns,K,path", LC.SOLVER_CASES)
def test_weights_exercise_both_branches(Ns, K, path):
    c = LC.case(Ns, K)
    for transform in P.TRANSFORMS:
        nuc, l1 = c.weights(transform)
        for momentum in (True, False):
            r = LC.reference(c, "c128", nuc, l1, transform, momentum, tol=0.0, max_iter=10)
            assert 0 < r["zeroed_sv"] < K and 0.2 <= r["zero_share"] <= 0.95, (transform, momentum, r["zeroed_sv"], r["zero_share"])


def test_header_ctypes_and_library_agree(nufft):
    header = open(os.path.join(ROOT, "include", "nufft_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(nufft.LIB_PATH)
    for name in ENTRY_POINTS:
        proto = re.search(r"\b(int64_t|int32_t|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert proto, name
        nargs = 0 if proto.group(2).strip() == "void" else proto.group(2).count(",") + 1
        res, args = nufft._lib.SYMBOLS[name]
        assert len(args) == nargs, name
        assert res is {"int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int}[proto.group(1)], name
        assert hasattr(raw, name), name
    L = nufft._lib
    for cname, mirror, size in (("nufft_glr_info", L.NufftGlrInfo, 80), ("nufft_tsparse_info", L.NufftTsparseInfo, 80),
                                ("nufft_lps_params", L.NufftLpsParams, 64), ("nufft_lps_info", L.NufftLpsInfo, 88)):
        assert getattr(nufft.lib, "nufft_sizeof_" + cname[6:])() == C.sizeof(mirror) == size, cname
        fields = re.search(r"typedef struct " + cname + r" \{(.*?)\}", header, flags=re.S).group(1)
        names = [re.sub(r"\[\d+\]", "", n.strip()) for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f[0].rstrip("_") for f in mirror._fields_], cname
    assert (L.TSPARSE_IDENTITY, L.TSPARSE_DFT) == (0, 1) and nufft.lib.nufft_version() == 104
    for name in ("GlobalLowRank", "TemporalSparsity", "ToeplitzLPS"):
        assert name in nufft.__all__ and hasattr(nufft, name)


def _params(nufft, **kw):
    p = nufft._lib.NufftLpsParams()
    p.struct_size = C.sizeof(nufft._lib.NufftLpsParams)
    p.max_iter, p.check_every, p.transform, p.momentum, p.tol, p.step, p.lambda_, p.nuc, p.l1 = 10, 0, 1, 1, 1e-4, 0.5, 0.0, 0.1, 0.1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_refusals_without_a_device(nufft):
    """Null arguments, then the arguments, then a real plan / more than 32 frames (UNSUPPORTED), and the missing device last."""
    L, lib = nufft._lib, nufft.lib
    plans = {K: nufft.PlanNUFFT(np.complex128, (12, 10), backend=None, ntransforms=K) for K in (3, 33)}
    real = nufft.PlanNUFFT(np.float64, (12, 10), backend=None, ntransforms=3)
    ops = {K: nufft.ToeplitzOperator(p) for K, p in plans.items()}
    h = C.c_void_p()
    # the global low-rank map
    assert lib.nufft_glr_create(None, plans[3]._handle) == L.ERR_INVALID_ARG and lib.nufft_glr_create(C.byref(h), None) == L.ERR_INVALID_ARG
    assert lib.nufft_glr_create(C.byref(h), real._handle) == L.ERR_UNSUPPORTED and b"complex plan" in lib.nufft_last_error_message()
    assert lib.nufft_glr_create(C.byref(h), plans[33]._handle) == L.ERR_UNSUPPORTED and b"33 transforms" in lib.nufft_last_error_message()
    assert lib.nufft_glr_create_for_operator(C.byref(h), ops[33]._handle) == L.ERR_UNSUPPORTED
    assert lib.nufft_glr_create(C.byref(h), plans[3]._handle) == L.ERR_NO_DEVICE and not h.value
    assert lib.nufft_glr_create_for_operator(C.byref(h), ops[3]._handle) == L.ERR_NO_DEVICE and not h.value
    assert lib.nufft_glr_create_for_operator(C.byref(h), None) == L.ERR_INVALID_ARG
    assert lib.nufft_glr_apply(None, None, None, 0.0, None, None) == L.ERR_INVALID_ARG and lib.nufft_glr_get_info(None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_glr_last_sweeps(None, None, None) == L.ERR_INVALID_ARG and lib.nufft_glr_destroy(None) == L.OK
    # the temporal transform: the transform is an argument and is checked before the plan is looked at
    assert lib.nufft_tsparse_create(C.byref(h), None, 1) == L.ERR_INVALID_ARG
    for bad in (-1, 2):
        assert lib.nufft_tsparse_create(C.byref(h), real._handle, bad) == L.ERR_INVALID_ARG
        assert lib.nufft_tsparse_create_for_operator(C.byref(h), ops[33]._handle, bad) == L.ERR_INVALID_ARG
    for tr in (0, 1):
        assert lib.nufft_tsparse_create(C.byref(h), real._handle, tr) == L.ERR_UNSUPPORTED
        assert lib.nufft_tsparse_create(C.byref(h), plans[33]._handle, tr) == L.ERR_UNSUPPORTED
        assert lib.nufft_tsparse_create(C.byref(h), plans[3]._handle, tr) == L.ERR_NO_DEVICE and not h.value
        assert lib.nufft_tsparse_create_for_operator(C.byref(h), ops[3]._handle, tr) == L.ERR_NO_DEVICE and not h.value
    for fn in (lib.nufft_tsparse_forward, lib.nufft_tsparse_inverse):
        assert fn(None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tsparse_shrink(None, None, None, 0.0, None, None) == L.ERR_INVALID_ARG and lib.nufft_tsparse_destroy(None) == L.OK
    # the solver
    create = lib.nufft_lps_create
    assert create(C.byref(h), ops[3]._handle, None) == L.ERR_INVALID_ARG and create(C.byref(h), None, C.byref(_params(nufft))) == L.ERR_INVALID_ARG
    for kw in ({"max_iter": 0}, {"max_iter": (1 << 24) + 1}, {"check_every": -1}, {"transform": 2}, {"momentum": 2}, {"tol": -1.0},
               {"lambda_": -1.0}, {"nuc": -1.0}, {"nuc": float("nan")}, {"l1": -1.0}, {"l1": float("inf")}, {"step": 0.0}, {"step": float("nan")},
               {"struct_size": 8}):
        assert create(C.byref(h), ops[3]._handle, C.byref(_params(nufft, **kw))) == L.ERR_INVALID_ARG, kw
        assert create(C.byref(h), ops[33]._handle, C.byref(_params(nufft, **kw))) == L.ERR_INVALID_ARG, kw      # before the frame limit
    assert create(C.byref(h), ops[33]._handle, C.byref(_params(nufft))) == L.ERR_UNSUPPORTED
    assert create(C.byref(h), ops[3]._handle, C.byref(_params(nufft))) == L.ERR_NO_DEVICE and not h.value
    assert lib.nufft_lps_set_weights(None, 0.1, 0.1) == L.ERR_INVALID_ARG and lib.nufft_lps_solve(None, None, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_lps_get_parts(None, None, None, None) == L.ERR_INVALID_ARG and lib.nufft_lps_get_info(None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_lps_get_result(None, None, None, None, 0, None) == L.ERR_INVALID_ARG and lib.nufft_lps_history(None, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_lps_destroy(None) == L.OK
    # the Python layer refuses the same way
    for make in (lambda: nufft.GlobalLowRank(plans[3]), lambda: nufft.TemporalSparsity(ops[3]), lambda: nufft.ToeplitzLPS(ops[3], 0.1, 0.1, step=0.5),
                 lambda: nufft.TemporalSparsity(plans[3], "difference"), lambda: nufft.ToeplitzLPS(ops[3], 0.1, 0.1, transform="tv", step=0.5),
                 lambda: nufft.GlobalLowRank(real)):
        with pytest.raises(ValueError):
            make()
    for o in list(ops.values()) + list(plans.values()) + [real]:
        o.close()
