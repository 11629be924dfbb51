"""TGV² without a GPU: the numpy reference (tgv_reference.py) — adjoint identities of the symmetrised gradient, the bound on ‖K‖², the
optimality conditions at the minimiser in float64, the reduction to total variation, its freeze, prefix and zero right-hand-side rules —
and the C ABI of the solver and of the operator (header, ctypes mirror, symbols, struct sizes, the refusals that need no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import tgv_reference as G
import toeplitz_reference as R
import tv_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("nufft_tv_sym_gradient", "nufft_tv_sym_adjoint", "nufft_tv_sym_norm", "nufft_tgv_create", "nufft_tgv_destroy",
                "nufft_tgv_set_weights", "nufft_tgv_solve", "nufft_tgv_get_info", "nufft_tgv_get_result", "nufft_tgv_history",
                "nufft_tgv_copy_field", "nufft_sizeof_tgv_params", "nufft_sizeof_tgv_info")

# what the float64 reference reaches on the (32, 24) system with tol = 1e-8, alpha0 = 0.5 alpha1 (measured on the CPU), per lam / λmax:
# (r_x, r_v, e_1, e_0, g_1, g_0)
REACHED = {0.0: (1.09e-7, 2.12e-5, 2.22e-16, 2.22e-16, 8.23e-8, 1.11e-11), 0.05: (8.43e-8, 1.58e-5, 2.22e-16, 2.22e-16, 9.68e-8, 1.71e-11)}
# ‖x_TGV − x_TV‖ / ‖x_TV‖ on the same system with alpha0 = 2 alpha1, both references at tol = 1e-8 (measured on the CPU)
TV_DISTANCE = 5.25e-3
SHAPES = [(9,), (7, 5), (5, 6, 7)]


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


@pytest.fixture(scope="module")
def system():
    """(32, 24) unknowns, 4 n uniform points, the exact spectrum through toeplitz_reference: the system of test_tv_host.py."""
    Ns = (32, 24)
    rng = np.random.default_rng(7)
    Np = 4 * int(np.prod(Ns))
    xs = [rng.random(Np) * 2 * np.pi for _ in Ns]
    w = (rng.random(Np) + 0.1) / Np
    K = R.multiplier(Ns, R.exact_spectrum(Ns, xs, w)).real
    apply = lambda p: R.apply(Ns, K, np.asarray(p).astype(np.complex128))      # noqa: E731
    b = rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1])
    v = b.copy()
    for _ in range(60):
        g = apply(v)
        lmax = float(np.linalg.norm(g) / np.linalg.norm(v))
        v = g / np.linalg.norm(g)
    return Ns, apply, b, lmax


def _fields(shape, seed):
    D, S = len(shape), len(shape) * (len(shape) + 1) // 2
    rng = np.random.default_rng(seed)
    draw = lambda *lead: rng.standard_normal(lead + shape) + 1j * rng.standard_normal(lead + shape)      # noqa: E731
    return draw(), draw(D), draw(D), draw(S)


@pytest.mark.parametrize("shape", SHAPES)
def test_adjoint_identities(shape):
    D = len(shape)
    _, v, _, r = _fields(shape, D)
    ev = G.sym_gradient(v)
    lhs, rhs = G.sym_inner(ev, r), np.vdot(v, G.sym_adjoint(r, D))
    assert abs(lhs - rhs) <= 1e-13 * abs(lhs)
    assert ev.shape == (D * (D + 1) // 2,) + shape and G.sym_adjoint(r, D).shape == (D,) + shape
    const = np.stack([np.full(shape, 2.5 - 1j * d) for d in range(D)])
    assert not G.sym_gradient(const).any()                                                 # E of a constant field is exactly zero
    for s, (d, e) in enumerate(G.pairs(D)):
        if d == e:                                                                         # the diagonal is ∂⁻_d v_d bit for bit
            assert np.array_equal(ev[s], v[d] - np.roll(v[d], 1, axis=-1 - d)), d
    assert G.pairs(3) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    assert np.allclose(G.frobenius_norms(r) ** 2, sum(w * np.abs(u) ** 2 for w, u in zip(G.sym_weights(D), r)))
    v32 = v.astype(np.complex64)
    assert G.sym_gradient(v32).dtype == np.complex64 and G.sym_adjoint(r.astype(np.complex64), D).dtype == np.complex64


@pytest.mark.parametrize("shape", SHAPES)
def test_operator_norm_bound(shape):
    """Power iteration on KᴴK, K(x, v) = (∇x − v, E v), Kᴴ(p, r) = (∇ᴴp, −p + Eᴴr): measured 6.41 / 10.68 / 15.26 against 8 D."""
    D = len(shape)
    x, v, _, _ = _fields(shape, D)
    lam = 0.0
    for _ in range(300):
        p, r = T.gradient(x) - v, G.sym_gradient(v)
        x2, v2 = T.adjoint(p), G.sym_adjoint(r, D) - p
        n = np.sqrt(np.vdot(x2, x2).real + np.vdot(v2, v2).real)
        lam = n / np.sqrt(np.vdot(x, x).real + np.vdot(v, v).real)
        x, v = x2 / n, v2 / n
    print(f"‖K‖² on {shape}: {lam:.3f} (bound {8 * D})")
    assert 2 * D < lam <= 8 * D


@pytest.mark.parametrize("lam_rel", [0.0, 0.05])
def test_reference_reaches_the_minimiser(system, lam_rel):
    """Measured on the CPU in float64 with tol = 1e-8, alpha1 = 0.1 max|b|, alpha0 = 0.5 alpha1: lam = 0: 985 iterations, r_x 1.09e-7,
    r_v 2.12e-5, e_1 = e_0 = 2.22e-16, g_1 8.23e-8, g_0 1.11e-11; lam = 0.05 λmax: 767 iterations, 8.43e-8, 1.58e-5, 2.22e-16, 2.22e-16,
    9.68e-8, 1.71e-11.  The bars are 10 × those.  Both prior terms are active at the minimiser (390 and 2413 at lam = 0)."""
    Ns, apply, b, lmax = system
    lam = lam_rel * lmax
    a1 = 0.1 * np.abs(b).max()
    a0 = 0.5 * a1
    got = G.tgvpd(apply, b, a1, a0, 1.0 / (1.05 * lmax + lam), lam=lam, tol=1e-8, max_iter=20000)
    assert got["status"] == G.CONVERGED and got["change"] <= 1e-8
    assert 0.1 <= got["clipped_p"][:10].mean() <= 0.95 and 0.1 <= got["clipped_r"][:10].mean() <= 0.95      # both branches of both projections
    o = G.optimality(apply, b, got["x"], got["v"], got["p"], got["r"], a1, a0, lam=lam)
    print(f"lam = {lam_rel} lmax: {got['iterations']} iterations, " + ", ".join(f"{n} {v:.2e}" for n, v in zip(("r_x", "r_v", "e_1", "e_0", "g_1", "g_0"), o)))
    assert all(v <= 10 * bar for v, bar in zip(o, REACHED[lam_rel])), o
    hist = got["history"]
    assert hist.shape == (got["iterations"], 3) and hist[-1, 0] == got["change"]
    assert hist[-1, 1] > 1.0 and hist[-1, 2] > 1.0                                           # both terms of the prior are active
    assert abs(hist[-1, 1] - T.cell_norms(T.gradient(got["x"]) - got["v"]).sum()) <= 1e-12 * hist[-1, 1]
    assert abs(hist[-1, 2] - G.frobenius_norms(G.sym_gradient(got["v"])).sum()) <= 1e-12 * hist[-1, 2]


def test_reduces_to_total_variation(system):
    """alpha0 = 2 alpha1: the minimiser has E v -> 0 (alpha0 Σ|Ev|_F = 8.7e-4 against alpha1 Σ|∇x − v|₂ = 750 at tol 1e-8), and x is the
    TV solution: measured 5.24e-3 from tv_reference.tvpd's x for tv = alpha1 at the same tol (1416 and 269 iterations); the bar is
    10 × that.  g_0 is not asserted: its denominator vanishes."""
    Ns, apply, b, lmax = system
    a1 = 0.1 * np.abs(b).max()
    step = 1.0 / (1.05 * lmax)
    got = G.tgvpd(apply, b, a1, 2 * a1, step, tol=1e-8, max_iter=20000)
    tv = T.tvpd(apply, b, a1, step, tol=1e-8, max_iter=20000)
    assert got["status"] == G.CONVERGED and tv["status"] == T.CONVERGED
    dist = R.rel(got["x"], tv["x"])
    print(f"TGV against TV: {dist:.3e}; alpha0 Σ|Ev|_F = {2 * a1 * got['history'][-1, 2]:.2e}, alpha1 Σ|∇x − v|₂ = {a1 * got['history'][-1, 1]:.1f}")
    assert dist <= 10 * TV_DISTANCE
    assert 2 * a1 * got["history"][-1, 2] <= 1e-4 * a1 * got["history"][-1, 1]


def test_reference_rules(system):
    Ns, apply, b, lmax = system
    step = 1.0 / (1.05 * lmax)
    a1 = 0.1 * np.abs(b).max()
    a0 = 0.5 * a1
    zero = G.tgvpd(apply, np.zeros_like(b), a1, a0, step, tol=1e-6, max_iter=10)
    assert zero["iterations"] == 1 and zero["status"] == G.CONVERGED and not zero["x"].any() and zero["change"] == 0.0
    a = G.tgvpd(apply, b, a1, a0, step, tol=1e-4, max_iter=2000)
    short = G.tgvpd(apply, b, a1, a0, step, tol=1e-4, max_iter=a["iterations"] - 2)
    assert a["status"] == G.CONVERGED and short["status"] == G.MAX_ITER and short["iterations"] == a["iterations"] - 2
    assert np.array_equal(short["history"], a["history"][:-2])                               # a shorter run is a prefix
    plain = G.tgvpd(apply, b, 0.0, a0, step, tol=0.0, max_iter=50)                           # alpha1 = 0: gradient descent on G x = b
    descent = T.tvpd(apply, b, 0.0, step, tol=0.0, max_iter=50)
    assert not plain["p"].any() and np.array_equal(plain["x"], descent["x"])
    free = G.tgvpd(apply, b, a1, 0.0, step, tol=0.0, max_iter=50)                            # alpha0 = 0: r is projected onto {0}
    assert not free["r"].any() and free["p"].any() and free["v"].any()
    low = G.tgvpd(apply, b, a1, a0, step, tol=1e-4, max_iter=2000, dtype=np.complex64)
    assert all(low[k].dtype == np.complex64 for k in "xvpr") and R.rel(low["x"], a["x"]) <= 1e-3
    nan = G.tgvpd(lambda p: np.full_like(p, np.nan), b, a1, a0, step, tol=1e-4, max_iter=5)
    assert nan["status"] == G.BREAKDOWN and nan["iterations"] == 1
    two = np.stack([b, 0.5 * b[::-1]])                                                       # a joint system: one change over both
    joint = G.tgvpd(lambda p: np.stack([apply(p[0]), apply(p[1])]), two, (a1, 0.0), (a0, a0), step, tol=0.0, max_iter=5, component_axis=0)
    assert joint["x"].shape == two.shape and joint["v"].shape == (2,) + two.shape and joint["r"].shape == (3,) + two.shape
    assert not joint["p"][:, 1].any()
    alone = G.tgvpd(apply, b, a1, a0, step, tol=0.0, max_iter=5)
    assert np.array_equal(joint["x"][0], alone["x"]) and np.array_equal(joint["v"][:, 0], alone["v"])


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
    assert nufft.lib.nufft_sizeof_tgv_params() == C.sizeof(L.NufftTgvParams) == 64
    assert nufft.lib.nufft_sizeof_tgv_info() == C.sizeof(L.NufftTgvInfo) == 80
    assert nufft.lib.nufft_sizeof_tvpd_params() == 56 and nufft.lib.nufft_sizeof_tvpd_info() == 80 and nufft.lib.nufft_sizeof_tv_info() == 72
    for name, value in (("NUFFT_TGV_MAX_ITER", L.TGV_MAX_ITER), ("NUFFT_TGV_CONVERGED", L.TGV_CONVERGED), ("NUFFT_TGV_BREAKDOWN", L.TGV_BREAKDOWN)):
        assert re.search(name + r"\s*=\s*" + str(value) + r"\b", header), name
    assert nufft.lib.nufft_version() == 104      # added without an ABI bump: detected by symbol
    assert callable(nufft.ToeplitzTGV) and "ToeplitzTGV" in nufft.__all__
    assert all(hasattr(nufft.TotalVariation, m) for m in ("sym_gradient", "sym_adjoint", "sym_norm"))


def _params(nufft, **kw):
    p = nufft._lib.NufftTgvParams()
    p.struct_size = C.sizeof(nufft._lib.NufftTgvParams)
    p.max_iter, p.check_every = 10, 0
    p.tol, p.step, p.sigma, p.lambda_, p.alpha1, p.alpha0 = 1e-4, 1.0, 0.0, 0.0, 0.1, 0.2
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_refusals_without_a_device(nufft):
    L, lib = nufft._lib, nufft.lib
    plan = nufft.PlanNUFFT(torch.complex128, (24, 40), backend=None)
    op = nufft.ToeplitzOperator(plan)
    h = C.c_void_p()
    assert lib.nufft_tgv_create(C.byref(h), op._handle, C.byref(_params(nufft))) == L.ERR_NO_DEVICE and not h.value
    assert "host-only" in lib.nufft_last_error_message().decode()
    for kw in ({"max_iter": 0}, {"max_iter": (1 << 24) + 1}, {"check_every": -1}, {"tol": -1.0}, {"tol": float("nan")}, {"step": 0.0},
               {"step": -1.0}, {"step": float("nan")}, {"step": float("inf")}, {"sigma": -1.0}, {"sigma": float("inf")}, {"alpha1": -1.0},
               {"alpha1": float("nan")}, {"alpha0": -1.0}, {"alpha0": float("inf")}, {"lambda_": -1.0}, {"lambda_": float("inf")},
               {"struct_size": 8}):
        assert lib.nufft_tgv_create(C.byref(h), op._handle, C.byref(_params(nufft, **kw))) == L.ERR_INVALID_ARG, kw      # before NO_DEVICE
        assert not h.value
    assert lib.nufft_tgv_create(C.byref(h), None, C.byref(_params(nufft))) == L.ERR_INVALID_ARG
    assert lib.nufft_tgv_create(C.byref(h), op._handle, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tgv_create(None, op._handle, C.byref(_params(nufft))) == L.ERR_INVALID_ARG
    assert lib.nufft_tgv_solve(None, None, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tgv_set_weights(None, None, None, 0) == L.ERR_INVALID_ARG
    assert lib.nufft_tgv_get_info(None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tgv_get_result(None, None, None, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tgv_history(None, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tgv_copy_field(None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tgv_destroy(None) == 0
    # the operator alone
    assert lib.nufft_tv_sym_gradient(None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tv_sym_adjoint(None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_tv_sym_norm(None, None, None, None) == L.ERR_INVALID_ARG
    with pytest.raises(ValueError, match="host-only"):
        nufft.ToeplitzTGV(op, 0.1, step=1.0)
    with pytest.raises(ValueError):
        nufft.ToeplitzTGV(op, 0.1)                        # step=None needs the device already
    with pytest.raises(ValueError):
        nufft.ToeplitzTGV(object(), 0.1)
    with pytest.raises(ValueError):
        nufft.ToeplitzTGV(op, 0.1, step=1.0, maxiter=2.5)
    with pytest.raises(ValueError):
        nufft.ToeplitzTGV(op, 0.1, step=1.0, check_every=True)
    with pytest.raises(ValueError):
        nufft.ToeplitzTGV(op, 0.1, step=1.0, sigma=0.0)
    with pytest.raises(ValueError):
        nufft.ToeplitzTGV(op, -1.0, step=1.0)
    with pytest.raises(ValueError):
        nufft.ToeplitzTGV(op, 0.1, alpha0=-1.0, step=1.0)
    with pytest.raises(ValueError):
        nufft.ToeplitzTGV(op, (0.1, 0.2), step=1.0)
    with pytest.raises(ValueError):
        nufft.ToeplitzTGV(op, 0.1, alpha0=(0.1, 0.2), step=1.0)
    for scalar in (np.float32(0.1), np.float64(0.1), torch.tensor(0.1), 1):      # numbers of any kind are one weight for all components
        with pytest.raises(ValueError, match="host-only"):
            nufft.ToeplitzTGV(op, scalar, alpha0=scalar, step=1.0)
