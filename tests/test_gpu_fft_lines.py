"""Every line length of the library's own FFT passes (csrc/fft_lines.hip, NUFFT_FFT_SIZES) in every kernel kind, Float32 and Float64,
against references.  The case tables live in tests/fft_lines_cases.py (checked on the CPU by tests/test_fft_lines_host.py).

  * plan paths: each case creates its plan twice, with defaults (the library's own passes) and with NUFFT_PRUNED_FFT=0 (rocFFT), asserts
    from workspace_breakdown() which path each runs, and compares type 1 and type 2 of both with the oracle: (a) both meet the project's
    bars (rel-L2 1e-7 / 1e-5), (b) the own passes' rel-L2 and rel-max error are at most RATIO_BAR times those of the rocFFT path measured
    in the same test (what tests/test_gpu_toeplitz.py grants the same kind of comparison);
  * the MULT variants (mode factors) with a point-weight callback on top, against the oracle's NUFFTCallbacks;
  * the Toeplitz operator's fused apply against the exact Gram product, the dense path and each other;
  * the halo-adding forward dimension-1 pass behind the spreading window's halo variant;
  * the coupled dimension-1 kernel (csrc/toeplitz_coupled.hip) in every launchable (element type, length, tier) against the exact block
    product, the dense path and each other, and the edge of what it refuses;
  * the coil-map (CMAP) variants of the strided passes at every length, against the exact SENSE product and the two routes without them.

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
import sense_reference as SR  # noqa: E402
import subspace_reference as S  # noqa: E402
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


COUPLED_CASES = FC.coupled_cases()


class _CoupledProblem:
    """Points, weights, basis and the K inputs of one (dims, K), drawn in single precision and widened, so that both element types hold
    exactly these numbers; the exact spectra of all pairs (direct sums), the three multipliers the tests read back and, per fftshift, the
    exact block product."""

    def __init__(self, dims, K, seed):
        rng = np.random.default_rng(seed)
        Np = FC.NP_TOEPLITZ
        cplx = lambda *shape: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64).astype(np.complex128)
        self.dims, self.K = dims, K
        self.xs = [(rng.random(Np) * 2 * np.pi).astype(np.float32).astype(np.float64) for _ in dims]
        self.w = (rng.random(Np) + 0.1).astype(np.float32).astype(np.float64)
        self.phi = cplx(K, Np) / np.sqrt(2)
        self.us = [cplx(*dims[::-1]) for _ in range(K)]
        self.spectra = np.ascontiguousarray(np.stack(S.exact_spectra(dims, self.xs, self.w, self.phi)))     # (einsum may return transposed views)
        self.mults = {(a, b): R.multiplier(dims, self.spectra[S.pair_index(a, b, K)]) for a, b in ((0, 0), (0, K - 1), (K - 1, K - 1))}
        for a in [self.phi, self.spectra, *self.us, *self.mults.values()]:
            a.setflags(write=False)
        self._gram = {}

    def gram(self, fftshift):
        if fftshift not in self._gram:
            self._gram[fftshift] = [np.ascontiguousarray(g) for g in S.exact_block_gram(self.dims, self.xs, self.w, self.phi, self.us, fftshift)]
            for g in self._gram[fftshift]:
                g.setflags(write=False)
        return self._gram[fftshift]


@functools.lru_cache(maxsize=2)
def _coupled_problem(dims, K):
    return _CoupledProblem(dims, K, seed=5000 + 17 * sum(dims) + K)


def _coupled_run(nufft, Zc, dims, K, fftshift, path, p, bar):
    """One coupled operator from the exact spectra on `path`: the K outputs of the apply; the three multipliers are checked here."""
    plan = nufft.PlanNUFFT(Zc, dims, backend=nufft.ROCBackend(0), fftshift=fftshift, ntransforms=K,
                           options={"NUFFT_TOEPLITZ_FUSED": 0} if path == "dense" else {})
    op = nufft.ToeplitzOperator(plan)
    assert op.path == path, (dims, K, path, op.path)
    op.set_spectra(torch.from_numpy(p.spectra.astype(Zc)).cuda())
    plan.close()
    assert op.coupled and nufft.lib.nufft_toeplitz_num_coupled(op._handle) == K and op.path == path
    out = op.apply(tuple(torch.from_numpy(u.astype(Zc)).cuda() for u in p.us))
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in out]
    for (a, b), kref in p.mults.items():
        k = op.multiplier(a, b)
        assert tuple(k.shape) == tuple(2 * n for n in reversed(dims)) and k.is_complex() == (a != b)
        ek = R.rel(k.cpu().numpy(), kref.real if a == b else kref)
        assert ek <= bar, (path, a, b, ek)
    op.close()
    return got


@pytest.mark.parametrize("case", COUPLED_CASES, ids=FC.case_id)
def test_toeplitz_coupled_lines_every_length_and_tier(case):
    """toeplitz_lines_coupled_kernel<T, N, KT, TL> (csrc/toeplitz_coupled.hip) in every launchable (element type, length, tier), with K
    walking through the tiers: the fused apply of K coupled components from exact spectra against the exact block product from direct
    sums, the dense path against the same, and the two against each other, per component.  Bars: those of
    tests/test_gpu_subspace.py `test_exact_spectra` (1e-12 / 1e-5) for every case: ComplexF32 at 2 N_1 >= 512 with K >= 9 measured
    2.8e-7 … 3.0e-7 fused and 2.9e-7 … 3.2e-7 dense, so no case needs a bar derived from the dense path."""
    nufft = _nufft()
    Zc, bar = (np.complex128, 1e-12) if case.Z == "c128" else (np.complex64, 1e-5)
    dims, K = tuple(case.dims), case.K
    p = _coupled_problem(dims, K)
    refs = p.gram(case.fftshift)
    got = {path: _coupled_run(nufft, Zc, dims, K, case.fftshift, path, p, bar) for path in ("fused", "dense")}
    ef = [R.rel(got["fused"][a], refs[a]) for a in range(K)]
    ed = [R.rel(got["dense"][a], refs[a]) for a in range(K)]
    efd = [R.rel(got["fused"][a], got["dense"][a]) for a in range(K)]
    mf = max(_relmax(got["fused"][a], refs[a]) for a in range(K))
    md = max(_relmax(got["dense"][a], refs[a]) for a in range(K))
    tier = FC.coupled_tier(K)
    print(f"FFTLINES coupled {FC.case_id(case)} KT={tier} TL={FC.coupled_waves(FC.CSIZE[case.Z], case.n, tier)}: fused l2 {max(ef):.3e} max {mf:.3e}; "
          f"dense l2 {max(ed):.3e} max {md:.3e}; fused vs dense {max(efd):.3e}; ratio {max(ef) / max(ed):.2f}")
    assert max(ef) <= bar and max(ed) <= bar and max(efd) <= bar, (ef, ed, efd)


def test_toeplitz_coupled_fit_boundary():
    """The edge of toeplitz_lines_coupled_supported: ComplexF64, tier 16 (K = 9 like K = 16), from 2 N_1 = 640 on.  The fused operator
    refuses the coupled build (NUFFT_ERR_UNSUPPORTED, the message names the way out) and is left without one; the dense operator of the
    same shape builds and meets the bar.  (The neighbours that fit, tier 16 at 512 and K = 8 at 640, 768 and 1024, run in the matrix.)"""
    nufft = _nufft()
    tab = nufft.plan._ptr_table
    for Z, n, K in FC.coupled_refused():
        assert Z == "c128"
        dims, npairs = (n // 2, 32), K * (K + 1) // 2
        plan = nufft.PlanNUFFT(np.complex128, dims, backend=nufft.ROCBackend(0), ntransforms=K)
        op = nufft.ToeplitzOperator(plan)
        plan.close()
        assert op.path == "fused"
        zeros = torch.zeros((npairs, 64, n), dtype=torch.complex128, device="cuda")
        code = nufft.lib.nufft_toeplitz_set_spectra_coupled(op._handle, tab(tuple(zeros[i] for i in range(npairs))), None)
        assert code == nufft._lib.ERR_UNSUPPORTED, (n, K, code)
        with pytest.raises(ValueError, match="NUFFT_TOEPLITZ_FUSED=0"):
            op.set_spectra(zeros)
        assert not op.coupled and nufft.lib.nufft_toeplitz_num_coupled(op._handle) == 0 and op.path == "fused" and op.info().has_spectrum == 0
        op.close()
        del zeros
        p = _coupled_problem(dims, K)
        refs = p.gram(False)
        got = _coupled_run(nufft, np.complex128, dims, K, False, "dense", p, 1e-12)
        ed = max(R.rel(got[a], refs[a]) for a in range(K))
        print(f"FFTLINES coupled boundary c128 n={n} K={K}: refused on the fused path; dense l2 {ed:.3e}")
        assert ed <= 1e-12, (n, K, ed)


MAPS_CASES = FC.maps_cases()
NCOILS = 3


@functools.lru_cache(maxsize=2)
def _maps_reference(dims, fftshift, seed):
    """Exact spectrum, three coil maps and the exact SENSE Gram product of one shape, shared by its ComplexF64 and ComplexF32 case: the
    draws and the maps are rounded to single precision before the reference is formed, so both element types hold exactly these numbers."""
    rng = np.random.default_rng(seed)
    Np = FC.NP_TOEPLITZ
    xs = [(rng.random(Np) * 2 * np.pi).astype(np.float32).astype(np.float64) for _ in dims]
    w = (rng.random(Np) + 0.1).astype(np.float32).astype(np.float64)
    u = (rng.standard_normal(dims[::-1]) + 1j * rng.standard_normal(dims[::-1])).astype(np.complex64).astype(np.complex128)
    maps = SR.smooth_maps(NCOILS, dims[::-1], seed=seed + 100).astype(np.complex64).astype(np.complex128)
    spec = np.ascontiguousarray(R.exact_spectrum(dims, xs, w))
    ref = np.ascontiguousarray(SR.exact_sense_gram(dims, xs, w, maps, u, fftshift))
    for a in (spec, ref, u, maps):
        a.setflags(write=False)
    return spec, ref, u, maps


@pytest.mark.parametrize("case", MAPS_CASES, ids=FC.case_id)
def test_toeplitz_coil_maps_in_pass_every_length(case):
    """fft_lines_kernel<..., CMAP = true> at every length: the outermost strided passes of the fused apply with three coil maps inside
    (backward times S; forward times conj(S), coil 0 storing, coils 1 and 2 accumulating) against the exact SENSE product from direct
    sums; the route without them (expand, plain apply, combine) and the dense path against the same, and the three against each other."""
    nufft = _nufft()
    Zc, bar = (np.complex128, 1e-12) if case.Z == "c128" else (np.complex64, 1e-5)
    dims = tuple(case.dims)
    spec, ref, u, maps = _maps_reference(dims, case.fftshift, 6000 + FC.SIZES.index(case.n))
    assert not maps[-1].ravel()[0] and np.all(maps[0])               # the exactly zero region of the last coil
    uz = np.ascontiguousarray(u.astype(Zc))
    got = {}
    for route, opts in (("inpass", {"NUFFT_TOEPLITZ_MAPS_INPASS": 1}), ("expand", {"NUFFT_TOEPLITZ_MAPS_INPASS": 0}),
                        ("dense", {"NUFFT_TOEPLITZ_MAPS_INPASS": 1, "NUFFT_TOEPLITZ_FUSED": 0})):
        plan = nufft.PlanNUFFT(Zc, dims, backend=nufft.ROCBackend(0), fftshift=case.fftshift, options=opts)
        op = nufft.ToeplitzOperator(plan)
        assert op.path == ("dense" if route == "dense" else "fused"), (case, route, op.path)
        op.set_maps(torch.from_numpy(np.ascontiguousarray(maps.astype(Zc))).cuda())
        op.set_spectrum(torch.from_numpy(np.ascontiguousarray(spec.astype(Zc))).cuda())
        plan.close()
        assert op.ncoils == NCOILS
        ud = torch.from_numpy(uz).cuda()
        out = op.apply(ud)
        torch.cuda.synchronize()
        got[route] = out.cpu().numpy()
        assert np.array_equal(ud.cpu().numpy(), uz), route           # the input is only read
        op.close()
    err = {route: R.rel(g, ref) for route, g in got.items()}
    cross = {"inpass vs expand": R.rel(got["inpass"], got["expand"]), "inpass vs dense": R.rel(got["inpass"], got["dense"]),
             "expand vs dense": R.rel(got["expand"], got["dense"])}
    print(f"FFTLINES maps {FC.case_id(case)}: inpass l2 {err['inpass']:.3e} max {_relmax(got['inpass'], ref):.3e}; expand l2 {err['expand']:.3e}; "
          f"dense l2 {err['dense']:.3e}; " + "; ".join(f"{k} {v:.3e}" for k, v in cross.items()) + f"; ratio {err['inpass'] / err['dense']:.2f}")
    assert all(e <= bar for e in err.values()) and all(e <= bar for e in cross.values()), (err, cross)


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
