"""Plans with more transforms than one launch takes (ntransforms = 9, 16, 17 against kMaxCompPerLaunch = 8, csrc/device_common.h)
in every transform engine, against the CPU oracle per component.

Every host loop `for (c0 = 0; c0 < C; c0 += 8)` of the transforms runs here with c0 > 0: fill_tile_args, the LDS-tile spread and
interpolation, the interpolation ring, the patch engine with its per-component sorted value copies, the spreading ring with its halo
side buffer (tile_launch.hip), run_deconv (deconv.hip), the gradient gather (interp_grad_inst.h) and the pre- / postphase and gradient
finish of type 3 (type3.cpp); and the stages that index all C components in one launch (FFT passes, halo add, rocFFT batch, grid copy)
with C > 8.  The cases and the reasoning behind them: tests/many_transforms_cases.py; their eligibility is checked without a GPU by
tests/test_many_transforms_host.py.

Bounds are the project's parity bounds: rel-L2 < 1e-7 (Float64 plans) / 1e-5 (Float32 plans) for transforms (`_rtol`, the reference's
own, test/pseudo_gpu.jl:159-171), 1e-12 / 1e-5 for grids, 1e-12 / 2e-5 for gradients (tests/test_gpu_parity.py, test_gpu_gradient.py),
the calibrated `_bar` of tests/test_gpu_type3.py and test_gpu_type3_gradient.py for type 3.  Before any comparison the reference
components are asserted pairwise distinguishable (rel > 0.5): a mix-up between components cannot pass.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import many_transforms_cases as MT  # noqa: E402
import test_gpu_gradient as TG  # noqa: E402
import test_gpu_type3 as T3  # noqa: E402
import test_gpu_type3_gradient as T3G  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from oracle import nufft_oracle as O  # noqa: E402
from test_gpu_parity import _f32_overflows, _oracle_inputs, _rel, _rtol, plan_real_dtype  # noqa: E402


def _nufft():
    from nufft_pkg import nufft
    return nufft


def _set_switches(monkeypatch, options):
    """The case's NUFFT_* switches and no others (the plan reads them from the environment at creation)."""
    harness = _nufft().plan._HARNESS_ENV
    for var in list(os.environ):
        if var.startswith("NUFFT_") and var not in harness:
            monkeypatch.delenv(var)
    for k, v in options.items():
        monkeypatch.setenv(k, v)


def _oracle_plan(case):
    """The oracle plan of a case, by the precision rules of tests/test_gpu_parity.py::_make_case (Float32 plans whose un-normalised
    window overflows Float32: the Float64 oracle that locates the points in Float32); the dense cases (3e5 points) go to the C oracle,
    which is Float64, as in test_dense_window_engine_every_instantiation."""
    name, Z, dims, M, sigma, evalmode, C, Np, spread_method, options, expected = case
    T = plan_real_dtype(Z)
    wide = _f32_overflows(Z, dims, M)
    return O.OraclePlan(dims, is_real=np.dtype(Z).kind == "f", dtype=np.float64 if wide else T, coord_dtype=T if wide else None,
                        M=M, sigma=sigma, evalmode=evalmode, ntransforms=C)


_REFERENCES = {}


def _reference(case):
    """(xs, vs, ws, ref1, ref2) of a case: inputs, type 1 of vs and type 2 of ws by the oracle.  Computed once per key and never
    modified (cases that differ only in switches share it, and so do the tests of this file)."""
    k = MT.key(case)
    if k not in _REFERENCES:
        name = case[0]
        oplan = _oracle_plan(case)
        xs, vs = MT.points(case), MT.values(case)
        ws = MT.spectra(case, tuple(reversed(oplan.size)))
        O.set_points(oplan, xs)
        if name.startswith("dense-"):
            assert CO.available(), "the C oracle (oracle/libnufft_oracle.so) is built by build()"
            ref1 = [r.copy() for r in CO.exec_type1(oplan, vs)]
            ref2 = CO.exec_type2(oplan, ws)
        else:
            ref1 = O.exec_type1(oplan, _oracle_inputs(oplan, vs))
            ref2 = O.exec_type2(oplan, _oracle_inputs(oplan, ws))
        MT.assert_distinguishable(ref1, (name, "type 1"))
        MT.assert_distinguishable(ref2, (name, "type 2"))
        for a in ref1 + ref2 + xs + vs + ws:
            a.setflags(write=False)
        _REFERENCES[k] = (xs, vs, ws, ref1, ref2)
    return _REFERENCES[k]


def _gpu_plan(case, monkeypatch):
    """The plan of a case under its switches; `expected` asserted against plan.info()."""
    nufft = _nufft()
    name, Z, dims, M, sigma, evalmode, C, Np, spread_method, options, expected = case
    _set_switches(monkeypatch, options)
    mode = nufft.Direct() if evalmode == O.DIRECT else nufft.FastApproximation()
    plan = nufft.PlanNUFFT(Z, dims, m=M, sigma=sigma, ntransforms=C, kernel_evalmode=mode, spread_method=spread_method,
                           backend=nufft.ROCBackend(0))
    info = plan.info()
    assert info.ntransforms == C
    for k in MT.INFO_KEYS:
        if k in expected:
            assert getattr(info, k) == expected[k], (name, k, getattr(info, k))
    return nufft, plan


def _to_dev(arrs, dev):
    return tuple(torch.from_numpy(np.array(a)).to(dev) for a in arrs)       # (np.array: a writable copy of the shared inputs)


@pytest.mark.parametrize("case", MT.CASES, ids=MT.IDS)
def test_type1_type2_match_oracle(case, monkeypatch):
    name, Z, dims, M, sigma, evalmode, C, Np, spread_method, options, expected = case
    nufft, plan = _gpu_plan(case, monkeypatch)
    xs, vs, ws, ref1, ref2 = _reference(case)
    dev = plan.device
    nufft.set_points(plan, _to_dev(xs, dev))
    spread_used, interp_used = plan.spread_engine_used(), plan.interp_engine_used()
    info = plan.info()
    print(f"\n{name}: spread_method {info.spread_method} ring_halo {info.ring_halo} patch_planar {info.patch_planar} "
          f"patch_f32acc {info.patch_f32acc}; set_points chose {spread_used} / {interp_used}")
    if "spread_engine_used" in expected:
        assert spread_used == expected["spread_engine_used"], name
    if "interp_engine_used" in expected:
        assert interp_used == expected["interp_engine_used"], name
    tol = _rtol(Z)

    us = tuple(torch.full(plan.shape, float("nan"), dtype=plan.eltype, device=dev) for _ in range(C))
    nufft.exec_type1(us, plan, _to_dev(vs, dev))
    err1 = [_rel(us[c].cpu().numpy(), ref1[c]) for c in range(C)]
    print(f"{name}: type 1 rel-L2 per component " + " ".join(f"{e:.1e}" for e in err1))
    for c in range(C):
        assert err1[c] < tol, (name, "type 1", c, err1[c])

    out = tuple(torch.full((Np,), float("nan"), dtype=plan.Z, device=dev) for _ in range(C))
    nufft.exec_type2(out, plan, _to_dev(ws, dev))
    err2 = [_rel(out[c].cpu().numpy(), ref2[c]) for c in range(C)]
    print(f"{name}: type 2 rel-L2 per component " + " ".join(f"{e:.1e}" for e in err2))
    for c in range(C):
        assert err2[c] < tol, (name, "type 2", c, err2[c])
    # the device-side decisions did not change under the transforms
    assert plan.spread_engine_used() == spread_used and plan.interp_engine_used() == interp_used


@pytest.mark.parametrize("name", ["ring-halo-f64-fuse1", "ring-halo-c128-fuse1"])
def test_stage_level_and_grid_access(name, monkeypatch):
    """spread_from_points, then the complete grid of components 0, 7, 8 and C - 1 (nufft_copy_grid, the halo add over all C components)
    against the oracle's spread field; then interpolate from those grids (as _ring_halo_variant_case and
    test_oversampled_grid_after_exec_type1_on_halo_plans of tests/test_gpu_parity.py do for C <= 2)."""
    case = MT.case(name)
    _, Z, dims, M, sigma, evalmode, C, Np, spread_method, options, expected = case
    nufft, plan = _gpu_plan(case, monkeypatch)
    info = plan.info()
    assert info.ring_halo == 1
    is_real = np.dtype(Z).kind == "f"
    wide = np.float64 if is_real else np.complex128
    xs, vs = MT.points(case), MT.values(case)
    dev = plan.device
    nufft.set_points(plan, _to_dev(xs, dev))
    assert plan.spread_engine_used() == "marching_ring"
    o64 = O.OraclePlan(dims, is_real=is_real, dtype=np.float64, M=M, sigma=sigma, evalmode=evalmode, ntransforms=C)
    O.set_points(o64, [x.astype(np.float64) for x in xs])
    refg = O.spread(o64, [v.astype(wide) for v in vs])
    MT.assert_distinguishable(refg, (name, "grids"))
    nufft.spread_from_points(plan, _to_dev(vs, dev))
    scale = 2.0 ** sum(info.window_scale_log2[d] for d in range(3))
    for c in sorted({0, 7, 8, C - 1}):
        grid = nufft.oversampled_grid(plan, c).cpu().numpy().astype(wide) / scale
        err = _rel(grid, refg[c])
        print(f"\n{name}: grid of component {c} rel-L2 {err:.1e}")
        assert err < 1e-12, (name, "grid", c, err)
    out = tuple(torch.full((Np,), float("nan"), dtype=plan.Z, device=dev) for _ in range(C))
    nufft.interpolate(plan, out)
    refv = O.interpolate(o64, refg)
    MT.assert_distinguishable(refv, (name, "interpolated"))
    for c in range(C):
        err = _rel(out[c].cpu().numpy().astype(wide) / scale ** 2, refv[c])
        assert err < 1e-12, (name, "interpolate", c, err)


@pytest.mark.parametrize("name", ["tiles-f64", "interp-ring-f64"])
def test_callbacks(name, monkeypatch):
    """PointWeights and ModeFactors (the callbacks of test/callbacks.jl:17-25, as tests/test_gpu_parity.py::test_callbacks_match_oracle)
    on all nine components: the general variant of the tile kernels, the ring that applies the weights itself, and the deconvolution
    with mode factors, each in chunks of eight."""
    case = MT.case(name)
    _, Z, dims, M, sigma, evalmode, C, Np, spread_method, options, expected = case
    nufft, plan = _gpu_plan(case, monkeypatch)
    T = plan_real_dtype(Z)
    xs, vs = MT.points(case), MT.values(case)
    oplan = _oracle_plan(case)
    rng = np.random.default_rng(MT.seed_of(case) + 77)
    weights = rng.random(Np).astype(T)
    ks = [(np.fft.rfftfreq(N, 1 / N) if d == 0 else np.fft.fftfreq(N, 1 / N)) for d, N in enumerate(dims)]
    k2 = sum(np.reshape(k ** 2, [-1 if e == d else 1 for e in range(len(dims))][::-1]) for d, k in enumerate(ks))
    factors = np.where(k2 == 0, 0.0, 1.0 / np.where(k2 == 0, 1.0, k2)).astype(T)     # reversed axes = torch layout
    ocb = O.NUFFTCallbacks(nonuniform=lambda v, n: tuple(type(x)(x * weights[n]) for x in v),
                           uniform=lambda w, idx: tuple(type(x)(x * factors[tuple(reversed(idx))]) for x in w))
    dev = plan.device
    nufft.set_points(plan, _to_dev(xs, dev))
    O.set_points(oplan, xs)
    if "interp_engine_used" in expected:
        assert plan.interp_engine_used() == expected["interp_engine_used"]
    cb = nufft.NUFFTCallbacks(nonuniform=nufft.PointWeights(torch.from_numpy(weights).to(dev)),
                              uniform=nufft.ModeFactors(torch.from_numpy(np.ascontiguousarray(factors)).to(dev)))
    tol = _rtol(Z)
    us = tuple(torch.full(plan.shape, float("nan"), dtype=plan.eltype, device=dev) for _ in range(C))
    nufft.exec_type1(us, plan, _to_dev(vs, dev), callbacks=cb)
    ref1 = O.exec_type1(oplan, _oracle_inputs(oplan, vs), callbacks=ocb)
    MT.assert_distinguishable(ref1, (name, "type 1"))
    for c in range(C):
        assert _rel(us[c].cpu().numpy(), ref1[c]) < tol, (name, "type 1", c)
    ws = MT.spectra(case, plan.shape)
    out = tuple(torch.full((Np,), float("nan"), dtype=plan.Z, device=dev) for _ in range(C))
    nufft.exec_type2(out, plan, _to_dev(ws, dev), callbacks=cb)
    ref2 = O.exec_type2(oplan, _oracle_inputs(oplan, ws), callbacks=ocb)
    MT.assert_distinguishable(ref2, (name, "type 2"))
    for c in range(C):
        assert _rel(out[c].cpu().numpy(), ref2[c]) < tol, (name, "type 2", c)


@pytest.mark.parametrize("Z,dims", [(np.float64, (48, 40, 56)), (np.complex64, (64, 48))])
def test_type2_gradient(Z, dims):
    """exec_type2_grad with nine components against the oracle's type-2 grid gathered with the numpy window derivatives of
    tests/grad_reference.py (test_gpu_gradient.py::_oracle_grad): values and all D gradient components of every transform."""
    C, M, Np = 9, 4, 3000
    nufft, plan, oplan, T = TG._plans(Z, dims, M, C=C)
    D = len(dims)
    seed = 4100 + 7 * sum(dims)
    rng = np.random.default_rng(seed)
    xs = [((rng.random(Np) * 3 - 1) * O.TWO_PI).astype(T) for _ in range(D)]
    uhs = [TG._spectra(plan, 1, np.random.default_rng(seed + 1000 * c))[0] for c in range(C)]
    v, g, _ = TG._run_grad(nufft, plan, xs, uhs)
    ref = TG._oracle_grad(oplan, xs, uhs)
    MT.assert_distinguishable([r[0] for r in ref], "values")
    for d in range(D):
        MT.assert_distinguishable([r[1][d] for r in ref], ("gradient", d))
    f64 = T == np.float64
    for c in range(C):
        rv, rg = ref[c]
        ev = _rel(v[c], rv)
        eg = [_rel(g[c][d], rg[d]) for d in range(D)]
        print(f"\ncomponent {c}: values {ev:.1e}, gradient " + " ".join(f"{e:.1e}" for e in eg))
        assert ev < (1e-12 if f64 else 1e-5), (c, ev)
        for d in range(D):
            assert eg[d] < (1e-12 if f64 else 2e-5), (c, d, eg[d])


def test_type3_and_its_gradient():
    """Type 3 with ntransforms = 9 (prephase, postphase and gradient finish of type3.cpp in two chunks) against direct sums in
    complex128, as test_ntransforms_three of tests/test_gpu_type3.py and of tests/test_gpu_type3_gradient.py with their own bars."""
    nufft = _nufft()
    C, Z = 9, np.complex128
    rng = np.random.default_rng(9009)
    x, s, _, bounds = T3G._case(rng, 3, Z, Np=1500, Nk=1200)
    cs = []
    for c in range(C):
        r = np.random.default_rng(9009 + 1000 * c)
        cs.append(r.standard_normal(1500) + 1j * r.standard_normal(1500))
    E = np.exp(-1j * (s.astype(np.float64) @ x.astype(np.float64).T))                         # (Nk, Np)
    ref = [E @ c for c in cs]
    refg = [np.stack([E @ (c * (-1j) * x[:, d]) for d in range(3)], axis=1) for c in cs]      # (Nk, 3) per component
    MT.assert_distinguishable(ref, "type 3")
    MT.assert_distinguishable(refg, "type 3 gradient")
    # values: exec_type3 on a plan from the point sets' bounding boxes
    fs, _ = T3._run(Z, x, s, cs, ntransforms=C)
    bar = T3._bar(Z, 4, 2.0, "bkb")
    for c in range(C):
        single, _ = T3._run(Z, x, s, cs[c])
        assert _rel(fs[c], single) <= 1e-12, c
        assert _rel(fs[c], ref[c]) <= bar, (c, _rel(fs[c], ref[c]), bar)
    # values and gradients at the targets: exec_type3_grad
    plan = T3G._plan(Z, 3, bounds, ntransforms=C)
    nufft.set_points3(plan, T3G._cols(x), T3G._cols(s))
    fd = [torch.full((1200,), float("nan"), dtype=torch.complex128, device="cuda") for _ in cs]
    gd = tuple(tuple(torch.full((1200,), float("nan"), dtype=torch.complex128, device="cuda") for _ in range(3)) for _ in cs)
    nufft.exec_type3_grad(fd, gd, plan, [T3G._dev(c) for c in cs])
    for c in range(C):
        ef = _rel(fd[c].cpu().numpy(), ref[c])
        eg = _rel(np.stack([t.cpu().numpy() for t in gd[c]], axis=1), refg[c])
        assert ef <= bar, (c, ef, bar)
        assert eg <= T3G._bar(Z, ef), (c, ef, eg)


def test_graph_replay(monkeypatch):
    """exec_type1 followed by exec_type2 on the Float64 tile plan with nine components, captured once on a side stream (as
    tests/test_gpu_graph.py) and replayed twice into outputs filled with a sentinel: every replay meets the oracle bound for all
    nine components."""
    case = MT.case("tiles-f64")
    _, Z, dims, M, sigma, evalmode, C, Np, spread_method, options, expected = case
    nufft, plan = _gpu_plan(case, monkeypatch)
    xs, vs, ws, ref1, ref2 = _reference(case)
    dev = plan.device
    nufft.set_points(plan, _to_dev(xs, dev))
    vd, wd = _to_dev(vs, dev), _to_dev(ws, dev)
    us = tuple(torch.empty(plan.shape, dtype=plan.eltype, device=dev) for _ in range(C))
    out = tuple(torch.empty(Np, dtype=plan.Z, device=dev) for _ in range(C))

    def step():
        nufft.exec_type1(us, plan, vd)
        nufft.exec_type2(out, plan, wd)

    step()                                   # everything the plan allocates lazily exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    tol = _rtol(Z)
    for replay in range(2):
        for t in us + out:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for c in range(C):
            assert _rel(us[c].cpu().numpy(), ref1[c]) < tol, (replay, "type 1", c)
            assert _rel(out[c].cpu().numpy(), ref2[c]) < tol, (replay, "type 2", c)
