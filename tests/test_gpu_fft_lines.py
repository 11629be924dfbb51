"""Every line length of the library's own FFT passes (csrc/fft_lines.hip, NUFFT_FFT_SIZES) in every kernel kind, Float32 and Float64,
against references.  The case tables live in tests/fft_lines_cases.py (checked on the CPU by tests/test_fft_lines_host.py).

  * plan paths: each case creates its plan twice, with defaults (the library's own passes) and with NUFFT_PRUNED_FFT=0 (rocFFT), asserts
    from workspace_breakdown() which path each runs, and compares type 1 and type 2 of both with the oracle: (a) both meet the project's
    bars (rel-L2 1e-7 / 1e-5), (b) the own passes' rel-L2 and rel-max error are at most RATIO_BAR times those of the rocFFT path measured
    in the same test (what tests/test_gpu_toeplitz.py grants the same kind of comparison);
  * the MULT variants (mode factors) with a point-weight callback on top, against the oracle's NUFFTCallbacks;
  * the Toeplitz operator's fused apply against the exact Gram product, the dense path and each other;
  * the halo-adding forward dimension-1 pass behind the spreading window's halo variant.

Lengths without a halo case: none.  At the shapes of fft_lines_cases.halo_shape (half-support 4) plan.info() reports the halo variant for
all thirteen lengths and all four element types (asserted on the CPU by tests/test_fft_lines_host.py).
"""
import ctypes as Ct
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import fft_lines_cases as FC  # noqa: E402
import toeplitz_reference as R  # noqa: E402
from oracle import nufft_oracle as O  # noqa: E402

RATIO_BAR = 3.0


def _nufft():
    from nufft_pkg import nufft
    return nufft


def _real_type(Z):
    return np.float32 if np.dtype(Z) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64


def _bar(Z):
    return 1e-5 if _real_type(Z) == np.float32 else 1e-7


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def _relmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _draw(Z, dims, C, Np, seed):
    """Points (outside the unit cell too) and values, drawn as tests/test_gpu_parity.py `_make_case` draws them."""
    Z = np.dtype(Z)
    T = _real_type(Z)
    rng = np.random.default_rng(seed)
    xs = [((rng.random(Np) * 3 - 1) * O.TWO_PI).astype(T) for _ in dims]
    if Z.kind == "f":
        vs = [rng.standard_normal(Np).astype(Z) for _ in range(C)]
    else:
        vs = [(rng.standard_normal(Np) + 1j * rng.standard_normal(Np)).astype(Z) for _ in range(C)]
    return xs, vs


def _oracle_plan(Z, dims, C, fftshift=False):
    """Float64 oracle; for Float32 plans it locates the points in Float32 as the plan does (coord_dtype)."""
    T = _real_type(Z)
    return O.OraclePlan(dims, is_real=np.dtype(Z).kind == "f", dtype=np.float64, coord_dtype=T if T == np.float32 else None,
                        M=FC.HALF_SUPPORT, sigma=FC.SIGMA, evalmode=O.DIRECT, ntransforms=C, fftshift=fftshift)


def _wide(arrs):
    return [a.astype(np.complex128 if np.iscomplexobj(a) else np.float64) for a in arrs]


def _plan_pair(case, monkeypatch):
    """The plan with defaults and the same plan with NUFFT_PRUNED_FFT=0; which path each runs is read from the workspace breakdown:
    3-D plans of the own passes hold the intermediate `tmp2`; complex plans hold a compact spectrum `uhat` only there (the general path
    transforms in place); 2-D real plans hold the twiddle tables of their strided pass (two tables of n complex numbers among `tables`)
    only there and, where dimension 1 is the library's own too, a compact `uhat` (N1/2 + 1 modes per line, rows padded) instead of
    rocFFT's half spectrum of the oversampled line."""
    nufft = _nufft()
    kw = dict(m=FC.HALF_SUPPORT, sigma=FC.SIGMA, ntransforms=case.C, kernel_evalmode=nufft.Direct(), fftshift=case.fftshift,
              backend=nufft.ROCBackend(0))
    monkeypatch.delenv("NUFFT_PRUNED_FFT", raising=False)
    own = nufft.PlanNUFFT(np.dtype(case.Z), case.dims, **kw)
    monkeypatch.setenv("NUFFT_PRUNED_FFT", "0")
    general = nufft.PlanNUFFT(np.dtype(case.Z), case.dims, **kw)
    monkeypatch.delenv("NUFFT_PRUNED_FFT", raising=False)
    assert own.oversampled_dims == tuple(case.over) and general.oversampled_dims == tuple(case.over)
    assert "NUFFT_PRUNED_FFT=0" in general.options and "NUFFT_PRUNED_FFT" not in own.options
    po, pg = own.workspace_breakdown(), general.workspace_breakdown()
    is_real = np.dtype(case.Z).kind == "f"
    if len(case.dims) == 3:
        assert "tmp2" in po and "tmp2" not in pg, (po, pg)
    if not is_real:
        assert "uhat" in po and "uhat" not in pg, (po, pg)
    else:
        tsize = np.dtype(_real_type(case.Z)).itemsize
        nlast = case.over[-1]
        assert po["tables"] >= pg["tables"] + 2 * (2 * nlast * tsize), (po, pg)
        if case.kind == "real_dim1":
            assert po["uhat"] < pg["uhat"], (po, pg)
        else:
            assert po["uhat"] == pg["uhat"], (po, pg)      # dimension 1 (80) stays with rocFFT on both plans
    return nufft, own, general


def _type2_inputs(plan, C):
    """As `_check_type1_type2` of tests/test_gpu_parity.py: a random spectrum in the plan's complex type."""
    rng = np.random.default_rng(7)
    ctype = np.complex64 if plan.T == torch.float32 else np.complex128
    return [(rng.standard_normal(plan.shape) + 1j * rng.standard_normal(plan.shape)).astype(ctype) for _ in range(C)]


def _run(nufft, plan, xs, vs, ws, callbacks=None):
    dev, C = plan.device, len(vs)
    tup = (lambda t: t if C > 1 else t[0])
    nufft.set_points(plan, tuple(torch.from_numpy(x).to(dev) for x in xs))
    us = tuple(torch.empty(plan.shape, dtype=plan.eltype, device=dev) for _ in range(C))
    nufft.exec_type1(tup(us), plan, tup(tuple(torch.from_numpy(v).to(dev) for v in vs)), callbacks=callbacks)
    out = tuple(torch.empty(len(xs[0]), dtype=plan.Z, device=dev) for _ in range(C))
    nufft.exec_type2(tup(out), plan, tup(tuple(torch.from_numpy(w).to(dev) for w in ws)), callbacks=callbacks)
    torch.cuda.synchronize()
    return [u.cpu().numpy() for u in us], [o.cpu().numpy() for o in out]


PLAN_CASES = FC.plan_cases()


@pytest.mark.parametrize("case", PLAN_CASES, ids=FC.case_id)
def test_plan_paths_every_length(case, monkeypatch):
    """Own passes and rocFFT on the same plan parameters, type 1 and type 2, both against the oracle (see the module docstring)."""
    nufft, own, general = _plan_pair(case, monkeypatch)
    C, i = case.C, FC.SIZES.index(case.n)
    xs, vs = _draw(case.Z, case.dims, C, FC.NP_PLAN, seed=1000 + i)
    ws = _type2_inputs(own, C)
    oplan = _oracle_plan(case.Z, case.dims, C, case.fftshift)
    O.set_points(oplan, xs)
    ref1 = O.exec_type1(oplan, _wide(vs))
    ref2 = O.exec_type2(oplan, _wide(ws))
    got_own = _run(nufft, own, xs, vs, ws)
    got_gen = _run(nufft, general, xs, vs, ws)
    bar = _bar(case.Z)
    failures = []
    for t, ref in ((0, ref1), (1, ref2)):
        for c in range(C):
            eo = (_rel(got_own[t][c], ref[c]), _relmax(got_own[t][c], ref[c]))
            eg = (_rel(got_gen[t][c], ref[c]), _relmax(got_gen[t][c], ref[c]))
            print(f"FFTLINES plan {FC.case_id(case)} type{t + 1} c={c}: own l2 {eo[0]:.3e} max {eo[1]:.3e}; rocfft l2 {eg[0]:.3e} max {eg[1]:.3e}; "
                  f"ratio l2 {eo[0] / eg[0]:.2f} max {eo[1] / eg[1]:.2f}")
            if not (eo[0] < bar and eg[0] < bar):
                failures.append(("bar", t + 1, c, eo, eg))
            if not (eo[0] <= RATIO_BAR * eg[0] and eo[1] <= RATIO_BAR * eg[1]):
                failures.append(("ratio", t + 1, c, eo, eg))
    own.close()
    general.close()
    assert not failures, failures


MULT_CASES = FC.mult_cases()


@pytest.mark.parametrize("case", MULT_CASES, ids=FC.case_id)
def test_mode_factor_variants_every_length(case, monkeypatch):
    """fft_lines_kernel<..., MULT = true>, forward and backward: the callbacks of tests/test_gpu_parity.py `test_callbacks_match_oracle`
    (mode factors 1/k², 0 at k = 0; per-point weights) on the 2-D strided arrangement, against the oracle's NUFFTCallbacks."""
    nufft, own, general = _plan_pair(case, monkeypatch)
    general.close()
    T = _real_type(case.Z)
    i = FC.SIZES.index(case.n)
    Ns, Np = case.dims, FC.NP_PLAN
    xs, vs = _draw(case.Z, Ns, 1, Np, seed=2000 + i)
    ws = _type2_inputs(own, 1)
    rng = np.random.default_rng(42)
    weights = rng.random(Np).astype(T)
    ks = [(np.fft.rfftfreq(N, 1 / N) if d == 0 else np.fft.fftfreq(N, 1 / N)) for d, N in enumerate(Ns)]
    k2 = sum(np.reshape(k ** 2, [-1 if e == d else 1 for e in range(len(Ns))][::-1]) for d, k in enumerate(ks))
    factors = np.where(k2 == 0, 0.0, 1.0 / np.where(k2 == 0, 1.0, k2)).astype(T)          # reversed axes = torch layout
    dev = own.device
    cb = nufft.NUFFTCallbacks(nonuniform=nufft.PointWeights(torch.from_numpy(weights).to(dev)),
                              uniform=nufft.ModeFactors(torch.from_numpy(np.ascontiguousarray(factors)).to(dev)))
    w64, f64 = weights.astype(np.float64), factors.astype(np.float64)
    ocb = O.NUFFTCallbacks(nonuniform=lambda v, n: tuple(type(x)(x * w64[n]) for x in v),
                           uniform=lambda w, idx: tuple(type(x)(x * f64[tuple(reversed(idx))]) for x in w))
    oplan = _oracle_plan(case.Z, Ns, 1)
    O.set_points(oplan, xs)
    ref1 = O.exec_type1(oplan, _wide(vs), callbacks=ocb)
    ref2 = O.exec_type2(oplan, _wide(ws), callbacks=ocb)
    got1, got2 = _run(nufft, own, xs, vs, ws, callbacks=cb)
    e1, e2 = _rel(got1[0], ref1[0]), _rel(got2[0], ref2[0])
    print(f"FFTLINES mult {FC.case_id(case)}: type1 l2 {e1:.3e} max {_relmax(got1[0], ref1[0]):.3e}; type2 l2 {e2:.3e} max {_relmax(got2[0], ref2[0]):.3e}")
    own.close()
    assert e1 < _bar(case.Z) and e2 < _bar(case.Z), (e1, e2)


TOEPLITZ_CASES = FC.toeplitz_cases()


@functools.lru_cache(maxsize=2)
def _toeplitz_reference(dims, fftshift, seed):
    """Exact spectrum and exact Gram product of one shape, shared by its ComplexF64 and ComplexF32 case: points, weights and the input are
    drawn in single precision, so both element types hold exactly these numbers."""
    rng = np.random.default_rng(seed)
    Np = FC.NP_TOEPLITZ
    xs = [(rng.random(Np) * 2 * np.pi).astype(np.float32).astype(np.float64) for _ in dims]
    w = (rng.random(Np) + 0.1).astype(np.float32).astype(np.float64)
    u = (rng.standard_normal(dims[::-1]) + 1j * rng.standard_normal(dims[::-1])).astype(np.complex64).astype(np.complex128)
    spec = np.ascontiguousarray(R.exact_spectrum(dims, xs, w))          # (einsum may return a transposed view)
    ref = np.ascontiguousarray(R.exact_gram(dims, xs, w, u, fftshift))
    kref = np.ascontiguousarray(R.multiplier(dims, spec).real)
    for a in (spec, ref, kref, u):
        a.setflags(write=False)
    return spec, ref, kref, u


@pytest.mark.parametrize("case", TOEPLITZ_CASES, ids=FC.case_id)
def test_toeplitz_fused_apply_every_length(case):
    """The fused apply (strided passes of fft_lines_kernel, toeplitz_lines_kernel along dimension 1) at every 2 N of the table, against the
    exact Gram product from direct sums, the dense path (rocFFT on the 2N grid) against the same, and the two against each other."""
    nufft = _nufft()
    Zc, bar = (np.complex128, 1e-12) if case.Z == "c128" else (np.complex64, 1e-5)
    spec, ref, kref, u = _toeplitz_reference(tuple(case.dims), case.fftshift, 3000 + FC.SIZES.index(case.n))
    got = {}
    for path in ("fused", "dense"):
        plan = nufft.PlanNUFFT(Zc, case.dims, backend=nufft.ROCBackend(0), fftshift=case.fftshift,
                               options={"NUFFT_TOEPLITZ_FUSED": 0} if path == "dense" else {})
        op = nufft.ToeplitzOperator(plan)
        assert op.path == path, (case, path, op.path)
        op.set_spectrum(torch.from_numpy(np.ascontiguousarray(spec.astype(Zc))).cuda())
        plan.close()
        out = op.apply(torch.from_numpy(np.ascontiguousarray(u.astype(Zc))).cuda())
        torch.cuda.synchronize()
        got[path] = out.cpu().numpy()
        k = op.multiplier().cpu().numpy()
        op.close()
        ek = R.rel(k, kref)
        assert k.shape == tuple(2 * n for n in reversed(case.dims)) and ek <= bar, (path, ek)
    ef, ed, efd = R.rel(got["fused"], ref), R.rel(got["dense"], ref), R.rel(got["fused"], got["dense"])
    print(f"FFTLINES toeplitz {FC.case_id(case)}: fused l2 {ef:.3e} max {_relmax(got['fused'], ref):.3e}; dense l2 {ed:.3e}; fused vs dense {efd:.3e}; "
          f"ratio {ef / ed:.2f}")
    assert ef <= bar and ed <= bar and efd <= bar, (ef, ed, efd)


HALO_CASES = FC.halo_cases()


@pytest.mark.parametrize("case", HALO_CASES, ids=FC.case_id)
def test_halo_adding_dimension1_pass_every_length(case, monkeypatch):
    """real_lines_kernel<..., HALO> / cplx_lines_kernel<..., HALO>: the forward dimension-1 pass that adds the side buffer of the spreading
    window's halo variant to the lines it loads, as tests/test_gpu_parity.py checks it at one length: the variant is on, the fused consumer
    ran (nufft_grid_ptr refuses while the grid is incomplete), type 1 meets the oracle's bar and the grid completed on demand is the
    oracle's spread field."""
    nufft = _nufft()
    monkeypatch.setenv("NUFFT_SMARCH_HALO", "2")
    monkeypatch.delenv("NUFFT_SMARCH_HALO_FUSE", raising=False)
    Z = np.dtype(case.Z)
    is_real = Z.kind == "f"
    T = _real_type(Z)
    plan = nufft.PlanNUFFT(Z, case.dims, m=FC.HALF_SUPPORT, sigma=FC.SIGMA, kernel_evalmode=nufft.Direct(), spread_method="marching_ring",
                           backend=nufft.ROCBackend(0))
    info = plan.info()
    assert plan.oversampled_dims == tuple(case.over)
    assert info.spread_method == 3 and info.ring_halo == 1, list(info.ring_column)
    assert "tmp2" in plan.workspace_breakdown()                      # the library's own passes: the fused consumer exists
    xs, vs = _draw(Z, case.dims, 1, FC.NP_HALO, seed=4000 + FC.SIZES.index(case.n))
    dev = plan.device
    nufft.set_points(plan, tuple(torch.from_numpy(x).to(dev) for x in xs))
    assert plan.spread_engine_used() == "marching_ring"
    u = torch.empty(plan.shape, dtype=plan.eltype, device=dev)
    nufft.exec_type1(u, plan, torch.from_numpy(vs[0]).to(dev))
    ptr, nbytes = Ct.c_void_p(), Ct.c_int64()
    assert nufft.lib.nufft_grid_ptr(plan._handle, 0, 0, Ct.byref(ptr), Ct.byref(nbytes)) == nufft._lib.ERR_INVALID_ARG      # pending
    oplan = _oracle_plan(Z, case.dims, 1)
    O.set_points(oplan, xs)
    e1 = _rel(u.cpu().numpy(), O.exec_type1(oplan, _wide(vs)[0]))
    # the grid, completed on demand, against the spread field of the same oracle plan: Float32 plans locate their points in Float32, and
    # so does this reference (coord_dtype) — against points located in Float64 the difference grows with the line length (measured
    # 4.6e-6 at 128 cells to 5.1e-5 at 2048: the Float32 rounding of a coordinate, in cells), which says nothing about the pass
    wide = np.float64 if is_real else np.complex128
    refg = O.spread(oplan, [vs[0].astype(wide)])[0]
    scale = 2.0 ** sum(info.window_scale_log2[d] for d in range(3))
    grid = nufft.oversampled_grid(plan, 0).cpu().numpy().astype(wide) / scale
    assert nufft.lib.nufft_grid_ptr(plan._handle, 0, 0, Ct.byref(ptr), Ct.byref(nbytes)) == 0
    eg = _rel(grid, refg)
    print(f"FFTLINES halo {FC.case_id(case)}: type1 l2 {e1:.3e}; grid l2 {eg:.3e}")
    plan.close()
    assert e1 < _bar(Z), e1
    assert eg < (1e-12 if T == np.float64 else 1e-5), eg
