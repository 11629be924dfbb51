"""The circulant preconditioner and preconditioned CG on the GPU, against the numpy reference (precond_reference.py) run
in the same element type.

Operators get an exact spectrum (point sets by the separable direct sum, or the analytic Poisson-kernel spectrum Π a^|d| whose symbol is
known), so the only error is the library's own; the 64³ operator is built from 8 n uniform points with m = 8 and the numpy side takes K from
``op.multiplier()``.  Bars:
  * m and M⁻¹ r: parity bars 1e-12 (ComplexF64) / 1e-5 (ComplexF32) of the maximum / in rel-L2.  m = 1 / (n (e + μ)) multiplies the
    relative error of e by max(e + μ) / (e + μ) where e is small, so these cases use systems whose e + μ spans less than a factor 30
    (uniform points with Np >= 8 n, or the Poisson spectrum with a <= 0.2); the floor is tested on its own.
  * fixed iteration count: rel-L2 of x₅ and of the history <= 10 × the parity bar, on systems with cond(G + λ) <= 7 as in test_gpu_cg.py.
  * converged solves: true residual in float64 <= 2 rtol; iterations within ±(10 % + 1) of the reference's (clustered points).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import cg_reference as CG  # noqa: E402
import precond_reference as P  # noqa: E402
import sense_reference as S  # noqa: E402
import toeplitz_reference as R  # noqa: E402
from fft_lines_cases import SIZES as LINE_SIZES  # noqa: E402


def _dt(Z):
    return (np.float64, np.complex128, 1e-12, 1e-10) if Z == "c128" else (np.float32, np.complex64, 1e-5, 1e-4)


def _dev(a, Zc=None):
    return torch.from_numpy(np.ascontiguousarray(a if Zc is None else a.astype(Zc))).cuda()


def _rand(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def poisson_spectrum(Ns, a=0.2):
    """T[d] = Π a^|d_dim| on the 2N grid: positive definite, cond <= ((1 + a) / (1 − a))^(2 D)."""
    D = len(Ns)
    spec = np.ones([2 * n for n in reversed(Ns)])
    for dim, n in enumerate(Ns):
        shape = [1] * D
        shape[D - 1 - dim] = 2 * n
        spec = spec * (a ** np.abs(np.asarray(R.modes(2 * n)).astype(np.float64))).reshape(shape)
    return spec.astype(np.complex128)


class System:
    """A spectrum, the float64 operator and circulant from it, and right-hand sides.  kind: "uniform" (random weights, Np = 8 n points:
    well conditioned), "clustered" (half uniform, half N(0, 0.4²) folded, w = 1/Np), "singular" (every point N(π, 0.3²): the numerically
    singular system of test_gpu_cg.py), "poisson" (analytic)."""

    def __init__(self, Ns, fftshift=False, kind="uniform", seed=0):
        rng = np.random.default_rng(seed)
        self.Ns, self.fftshift, self.shape = Ns, fftshift, Ns[::-1]
        n = int(np.prod(Ns))
        if kind == "poisson":
            self.spec = poisson_spectrum(Ns)
        else:
            if kind == "singular":
                Np = 400
                xs = [np.mod(np.pi + 0.3 * rng.standard_normal(Np), 2 * np.pi) for _ in Ns]
                w = rng.random(Np) + 0.1
            elif kind == "clustered":
                Np = 40000
                sd = 0.5 if len(Ns) == 3 else 0.4
                xs = [np.mod(np.concatenate([rng.random(Np // 2) * 2 * np.pi, sd * rng.standard_normal(Np - Np // 2)]), 2 * np.pi) for _ in Ns]
                w = np.full(Np, 1.0 / Np)
            else:
                Np = 400 if Ns == (48,) else max(2000, 8 * n)
                xs = [rng.random(Np) * 2 * np.pi for _ in Ns]
                w = (rng.random(Np) + 0.1) / Np
            self.spec = P.exact_spectrum_separable(Ns, xs, w)
        self.bs = [_rand(self.shape, seed + 1 + k) for k in range(2)]
        self.set_multiplier(R.multiplier(Ns, self.spec).real)

    def set_multiplier(self, K):
        Ns, fftshift = self.Ns, self.fftshift
        self.K = np.asarray(K, dtype=np.float64)
        self.e = P.chan_eigenvalues(Ns, P.generating_sequence(Ns, self.K)).real
        self.apply = lambda p: R.apply(Ns, self.K, np.asarray(p).astype(np.complex128), fftshift)

    def m(self, lam=0.0, floor=1e-6):
        return P.multiplier(self.e, mu=lam, floor=floor)

    def true_residual(self, lam, x, b, apply=None):
        x, b = np.asarray(x).astype(np.complex128), np.asarray(b).astype(np.complex128)
        return float(np.linalg.norm((b - ((apply or self.apply)(x) + lam * x)).ravel()) / np.linalg.norm(b.ravel()))

    def operator(self, nufft, Z, C=1, dense=False):
        _, Zc, _, _ = _dt(Z)
        plan = nufft.PlanNUFFT(Zc, self.Ns, backend=nufft.ROCBackend(0), options={"NUFFT_TOEPLITZ_FUSED": 0} if dense else {},
                               fftshift=self.fftshift, ntransforms=C)
        op = nufft.ToeplitzOperator(plan)
        op.set_spectrum(_dev(self.spec, Zc))
        plan.close()
        return op


_SYSTEMS = {}


def _system(Ns, fftshift=False, kind="uniform"):
    key = (Ns, fftshift, kind)
    if key not in _SYSTEMS:
        _SYSTEMS[key] = System(Ns, fftshift, kind, seed=7 * sum(Ns) + len(kind))
    return _SYSTEMS[key]


def _expected_path(Ns):
    return "fused" if len(Ns) >= 2 and all(n in LINE_SIZES for n in Ns) else "dense"


def _solve(sol, bs, C, **kw):
    bd = tuple(_dev(b) for b in bs)
    x = sol.solve(bd if C > 1 else bd[0], **kw)
    torch.cuda.synchronize()
    xs = [v.cpu().numpy() for v in (x if C > 1 else (x,))]
    return xs, sol.iterations, sol.status, sol.history().numpy()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- the multiplier ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Ns", [(48,), (15, 9), (48, 40), (64, 80)])
@pytest.mark.parametrize("Z", ["c128", "c64"])
@pytest.mark.parametrize("fftshift", [False, True])
def test_multiplier_matches_the_fold_formula(Ns, Z, fftshift):
    from nufft_pkg import nufft
    _, Zc, bar, _ = _dt(Z)
    s = _system(Ns, fftshift)
    assert s.e.max() / s.e.min() <= 30, s.e.max() / s.e.min()
    op = s.operator(nufft, Z)
    for lam_rel in (0.0, 0.1):
        lam = lam_rel * float(s.e.max())
        pc = nufft.ToeplitzPreconditioner(op, lam=lam)
        i = pc.info()
        assert pc.path == _expected_path(Ns) and i.mu == lam and i.scaling == 0 and pc.scaling() is None
        assert abs(i.max_e - s.e.max()) <= 10 * bar * s.e.max() and abs(i.min_e - s.e.min()) <= 10 * bar * s.e.max()
        got, ref = pc.multiplier().cpu().numpy().astype(np.float64), s.m(lam)
        err = np.abs(got - ref).max() / ref.max()
        print(f"m {Z} N={Ns} shift={fftshift} lam={lam_rel:g} max e ({pc.path}): {err:.3e} of max (bar {bar:g})")
        assert got.shape == s.shape and err <= bar
        pc.close()
    op.close()


def _points_operator_64(nufft, Z, C=1):
    """64³ from 8 n uniform points (cond about 4) with m = 8; K for numpy from the operator itself."""
    T, Zc, _, _ = _dt(Z)
    Ns = (64, 64, 64)
    rng = np.random.default_rng(64)
    Np = 8 * 64 ** 3
    xs = [rng.random(Np) * 2 * np.pi for _ in Ns]
    plan = nufft.PlanNUFFT(Zc, Ns, backend=nufft.ROCBackend(0), ntransforms=C, m=8 if Z == "c128" else 4)
    op = nufft.ToeplitzOperator(plan)
    op.set_points(tuple(_dev(x.astype(T)) for x in xs), _dev(np.full(Np, 1.0 / Np, dtype=T)))
    plan.close()
    s = System.__new__(System)
    s.Ns, s.fftshift, s.shape = Ns, False, Ns[::-1]
    s.bs = [_rand(s.shape, 640 + k) for k in range(2)]
    s.set_multiplier(op.multiplier().cpu().numpy())
    return s, op


@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_multiplier_64_cubed_from_points(Z):
    from nufft_pkg import nufft
    _, Zc, bar, _ = _dt(Z)
    s, op = _points_operator_64(nufft, Z)
    lam = 0.1 * float(s.e.max())
    assert s.e.max() / s.e.min() <= 30
    pc = nufft.ToeplitzPreconditioner(op, lam=lam)
    assert pc.path == "fused" and op.path == "fused"
    got, ref = pc.multiplier().cpu().numpy().astype(np.float64), s.m(lam)
    err = np.abs(got - ref).max() / ref.max()
    print(f"m {Z} 64^3 from points: {err:.3e} of max (bar {bar:g}); e in [{pc.info().min_e:.3e}, {pc.info().max_e:.3e}]")
    assert err <= bar
    r = _rand(s.shape, 5).astype(Zc)
    out = pc.apply(_dev(r)).cpu().numpy()
    ea = R.rel(out, P.apply(ref, None, r))
    print(f"apply {Z} 64^3: {ea:.3e} (bar {bar:g})")
    assert ea <= bar
    pc.close()
    op.close()


def test_floor_is_in_force():
    from nufft_pkg import nufft
    s = _system((48,), False, "singular")
    floor = 0.05
    assert s.e.min() < 0.1 * floor * s.e.max()
    op = s.operator(nufft, "c128")
    pc = nufft.ToeplitzPreconditioner(op, lam=0.0, floor=floor)
    assert pc.floor == floor and pc.info().floor == floor
    m = pc.multiplier().cpu().numpy()
    n = m.size
    assert np.isclose(m.max(), 1.0 / (n * floor * s.e.max()), rtol=1e-9) and (m > 0).all()
    assert np.abs(m - s.m(0.0, floor)).max() <= 1e-10 * m.max()
    pc.close()
    op.close()


@pytest.mark.parametrize("Z,Ns", [("c128", (64, 80)), ("c64", (15, 9))])
def test_update_follows_the_operator(Z, Ns):
    from nufft_pkg import nufft
    _, Zc, bar, _ = _dt(Z)
    s = _system(Ns, False, "poisson")
    op = s.operator(nufft, Z)
    pc = nufft.ToeplitzPreconditioner(op, lam=0.05)
    before = pc.multiplier().cpu().numpy().astype(np.float64)
    assert np.abs(before - s.m(0.05)).max() <= bar * before.max()
    spec2 = poisson_spectrum(Ns, a=0.1)
    op.set_spectrum(_dev(spec2, Zc))
    assert np.array_equal(pc.multiplier().cpu().numpy(), before.astype(_dt(Z)[0]))          # nothing changes until update()
    pc.update()
    e2 = P.chan_eigenvalues(Ns, P.generating_sequence(Ns, R.multiplier(Ns, spec2).real)).real
    after = pc.multiplier().cpu().numpy().astype(np.float64)
    ref = P.multiplier(e2, mu=0.05)
    assert np.abs(after - ref).max() <= bar * ref.max() and np.abs(after - before).max() > 100 * bar * ref.max()
    assert abs(pc.info().max_e - e2.max()) <= 10 * bar * e2.max()
    pc.close()
    op.close()


# ---- the apply --------------------------------------------------------------------------------------------------------------------

def _check_apply(nufft, s, Z, C=1, d=None, lam_rel=0.1, dense=False, inplace=False):
    _, Zc, bar, _ = _dt(Z)
    T = np.float32 if Z == "c64" else np.float64
    op = s.operator(nufft, Z, C, dense=dense)
    lam = lam_rel * float(s.e.max())
    pc = nufft.ToeplitzPreconditioner(op, lam=lam)
    assert pc.path == ("dense" if dense else _expected_path(s.Ns)), (s.Ns, pc.path)
    if d is not None:
        pc.set_scaling(_dev(d.astype(T)))
        assert pc.info().scaling == 2 and np.array_equal(pc.scaling().cpu().numpy(), d.astype(T))
    rs = [_rand(s.shape, 31 + c).astype(Zc) for c in range(C)]
    rd = tuple(_dev(r) for r in rs)
    out = pc.apply(rd if C > 1 else rd[0], out=(rd if C > 1 else rd[0]) if inplace else None)
    torch.cuda.synchronize()
    outs = [o.cpu().numpy() for o in (out if C > 1 else (out,))]
    if inplace:
        assert all(o.data_ptr() == r.data_ptr() for o, r in zip(out if C > 1 else (out,), rd))
    else:
        assert all(np.array_equal(r.cpu().numpy(), h) for r, h in zip(rd, rs))          # the input is only read
    m = s.m(lam)
    errs = [R.rel(o, P.apply(m, None if d is None else d.astype(T).astype(np.float64), r)) for o, r in zip(outs, rs)]
    print(f"apply {Z} N={s.Ns} C={C} {pc.path}{' scaled' if d is not None else ''}{' in place' if inplace else ''}: {max(errs):.3e} (bar {bar:g})")
    assert max(errs) <= bar
    pc.close()
    op.close()
    return outs


@pytest.mark.parametrize("N1", LINE_SIZES)
@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_apply_every_line_length(N1, Z):
    from nufft_pkg import nufft
    assert len(LINE_SIZES) == 13
    s = _system((N1, 64), False, "poisson")
    assert _expected_path(s.Ns) == "fused"
    _check_apply(nufft, s, Z)


@pytest.mark.parametrize("Ns", [(64, 80, 96), (96, 64, 64)])
@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_apply_three_dimensions(Ns, Z):
    from nufft_pkg import nufft
    s = _system(Ns, True, "poisson")
    d = np.random.default_rng(9).random(s.shape) + 0.5
    _check_apply(nufft, s, Z)
    _check_apply(nufft, s, Z, C=2, d=d, inplace=True)


@pytest.mark.parametrize("Ns", [(48, 40), (15, 9), (48,)])
@pytest.mark.parametrize("Z", ["c128", "c64"])              # (15, 9) in ComplexF32: an odd element count, the tail behind the last pack
def test_apply_dense_path(Ns, Z):
    from nufft_pkg import nufft
    s = _system(Ns, False, "poisson")
    d = np.random.default_rng(10).random(s.shape) + 0.5
    _check_apply(nufft, s, Z)
    _check_apply(nufft, s, Z, C=2, d=d)
    _check_apply(nufft, s, Z, d=d, inplace=True)


@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_apply_paths_agree_and_variants(Z):
    from nufft_pkg import nufft
    _, _, bar, _ = _dt(Z)
    s = _system((64, 80), False, "poisson")
    d = np.random.default_rng(11).random(s.shape) + 0.5
    fused = _check_apply(nufft, s, Z, C=2, d=d)
    dense = _check_apply(nufft, s, Z, C=2, d=d, dense=True)
    assert max(R.rel(a, b) for a, b in zip(fused, dense)) <= 2 * bar
    _check_apply(nufft, s, Z, inplace=True)
    _check_apply(nufft, s, Z, C=2, inplace=True)
    _check_apply(nufft, _system((64, 80), True, "poisson"), Z, d=d)


@pytest.mark.parametrize("Z,Ns", [("c128", (64, 80)), ("c64", (64, 80)), ("c128", (15, 9)), ("c64", (64, 64, 64))])
def test_inverse_is_hermitian_and_positive(Z, Ns):
    from nufft_pkg import nufft
    _, Zc, bar, _ = _dt(Z)
    s = _system(Ns, False, "poisson")
    op = s.operator(nufft, Z)
    pc = nufft.ToeplitzPreconditioner(op).set_scaling(_dev((np.random.default_rng(12).random(s.shape) + 0.5).astype(_dt(Z)[0])))
    a, b = _rand(s.shape, 1).astype(Zc), _rand(s.shape, 2).astype(Zc)
    Ma, Mb = (pc.apply(_dev(v)).cpu().numpy().astype(np.complex128) for v in (a, b))
    a, b = a.astype(np.complex128), b.astype(np.complex128)
    lhs, rhs = np.vdot(a, Mb), np.conj(np.vdot(b, Ma))
    scale = np.linalg.norm(a) * np.linalg.norm(Mb)
    print(f"Hermitian {Z} N={Ns}: |<a, Mb> - conj<b, Ma>| / (|a| |Mb|) = {abs(lhs - rhs) / scale:.3e}")
    assert abs(lhs - rhs) <= 10 * bar * scale
    assert np.vdot(a, Ma).real > 0 and np.vdot(b, Mb).real > 0
    assert abs(np.vdot(a, Ma).imag) <= 10 * bar * np.linalg.norm(a) * np.linalg.norm(Ma)


# ---- preconditioned CG ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Z,Ns,C", [("c128", (64, 80), 1), ("c64", (64, 80), 2), ("c128", (48, 40), 2), ("c64", (48, 40), 1)])
def test_pcg_fixed_iteration_count(Z, Ns, C):
    from nufft_pkg import nufft
    _, Zc, bar, _ = _dt(Z)
    s = _system(Ns, C == 2)
    op = s.operator(nufft, Z, C)
    assert op.path == "fused"
    bs = [b.astype(Zc) for b in s.bs[:C]]
    for lam_rel in (0.0, 1e-3):
        lam = lam_rel * float(s.e.max())
        pc = nufft.ToeplitzPreconditioner(op, lam=lam)
        assert pc.path == _expected_path(Ns)
        sol = nufft.ToeplitzCG(op, maxiter=5, rtol=0.0, lam=lam, precond=pc)
        xs, iters, status, hist = _solve(sol, bs, C)
        assert iters == (5,) * C and status == ("max_iter",) * C and hist.shape == (6, C)
        m = s.m(lam)
        for c in range(C):
            ref = P.pcg(s.apply, lambda r: P.apply(m, None, r), bs[c], lam=lam, rtol=0.0, max_iter=5, dtype=Zc)
            ex, eh = R.rel(xs[c], ref["x"]), R.rel(hist[:, c], ref["history"])
            print(f"PCG 5 iterations {Z} N={Ns} pc {pc.path} lam={lam_rel:g} c={c}: x {ex:.3e}, history {eh:.3e} (bar {10 * bar:g})")
            assert ex <= 10 * bar and eh <= 10 * bar
        sol.close()
        pc.close()
    op.close()


@pytest.mark.parametrize("Z,C", [("c128", 1), ("c64", 2)])
def test_pcg_fixed_iteration_count_64_cubed(Z, C):
    from nufft_pkg import nufft
    _, Zc, bar, _ = _dt(Z)
    s, op = _points_operator_64(nufft, Z, C)
    lam = 1e-3 * float(s.e.max())
    pc = nufft.ToeplitzPreconditioner(op, lam=lam)
    assert pc.path == "fused"
    bs = [b.astype(Zc) for b in s.bs[:C]]
    sol = nufft.ToeplitzCG(op, maxiter=5, rtol=0.0, lam=lam, precond=pc)
    xs, iters, status, hist = _solve(sol, bs, C)
    assert iters == (5,) * C and status == ("max_iter",) * C
    m = s.m(lam)
    for c in range(C):
        ref = P.pcg(s.apply, lambda r: P.apply(m, None, r), bs[c], lam=lam, rtol=0.0, max_iter=5, dtype=Zc)
        ex, eh = R.rel(xs[c], ref["x"]), R.rel(hist[:, c], ref["history"])
        print(f"PCG 5 iterations {Z} 64^3 c={c}: x {ex:.3e}, history {eh:.3e} (bar {10 * bar:g})")
        assert ex <= 10 * bar and eh <= 10 * bar
    sol.close()
    pc.close()
    op.close()


@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_pcg_converged_on_clustered_points(Z):
    from nufft_pkg import nufft
    _, Zc, _, rtol = _dt(Z)
    s = _system((64, 80), False, "clustered")
    lam = 1e-3 * float(s.e.max())
    op = s.operator(nufft, Z)
    pc = nufft.ToeplitzPreconditioner(op, lam=lam)
    b = s.bs[0].astype(Zc)
    sol = nufft.ToeplitzCG(op, maxiter=600, rtol=rtol, lam=lam, precond=pc, check_every=10)
    xs, iters, status, hist = _solve(sol, [b], 1)
    m = s.m(lam)
    ref = P.pcg(s.apply, lambda r: P.apply(m, None, r), b, lam=lam, rtol=rtol, max_iter=600, dtype=Zc)
    tr = s.true_residual(lam, xs[0], b)
    assert status == ("converged",) and tr <= 2 * rtol
    assert abs(iters[0] - ref["iterations"]) <= 0.1 * ref["iterations"] + 1
    assert sol.residual[0] <= rtol * (1 + 1e-12) and hist[iters[0], 0] == sol.residual[0]
    sol.set_preconditioner(None)                                            # the same solver object, plain CG
    xp, itp, stp, _ = _solve(sol, [b], 1)
    print(f"clustered (64, 80) {Z}: PCG {iters[0]} iterations (reference {ref['iterations']}), true residual / rtol {tr / rtol:.3f}; plain CG {itp[0]}")
    assert stp == ("converged",) and itp[0] >= 2 * iters[0]
    assert s.true_residual(lam, xp[0], b) <= 2 * rtol
    sol.close()
    pc.close()
    op.close()


@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_pcg_with_coil_maps(Z):
    from nufft_pkg import nufft
    T, Zc, bar, rtol = _dt(Z)
    s = _system((64, 80), False, "clustered")
    maps = S.smooth_maps(4, s.shape, seed=3, zero_region=False).astype(Zc)
    lam = 1e-3 * float(s.e.max())
    op = s.operator(nufft, Z)
    op.set_maps(_dev(maps))
    pc = nufft.ToeplitzPreconditioner(op, lam=lam)
    maps64 = maps.astype(np.complex128)
    d_ref, mu_ref = P.coil_scaling(maps64, lam)
    i = pc.info()
    assert i.scaling == 1 and abs(i.mu - mu_ref) <= 10 * bar * mu_ref
    d = pc.scaling().cpu().numpy().astype(np.float64)
    assert np.abs(d - d_ref).max() <= bar * d_ref.max()
    m = s.m(mu_ref)
    r = _rand(s.shape, 77).astype(Zc)
    assert R.rel(pc.apply(_dev(r)).cpu().numpy(), P.apply(m, d_ref, r)) <= bar
    GS = lambda p: S.toeplitz_sense_gram(s.Ns, s.K, maps64, np.asarray(p).astype(np.complex128))
    b = s.bs[0].astype(Zc)
    sol = nufft.ToeplitzCG(op, maxiter=600, rtol=rtol, lam=lam, precond=pc, check_every=10)
    xs, iters, status, _ = _solve(sol, [b], 1)
    ref = P.pcg(GS, lambda v: P.apply(m, d_ref, v), b, lam=lam, rtol=rtol, max_iter=600, dtype=Zc)
    tr = s.true_residual(lam, xs[0], b, apply=GS)
    sol.set_preconditioner(None)
    _, itp, stp, _ = _solve(sol, [b], 1)
    print(f"4 coils (64, 80) {Z}: PCG {iters[0]} iterations (reference {ref['iterations']}), true residual / rtol {tr / rtol:.3f}; plain CG {itp[0]}")
    assert status == ("converged",) and tr <= 2 * rtol
    assert abs(iters[0] - ref["iterations"]) <= 0.1 * ref["iterations"] + 1
    assert stp == ("converged",) and itp[0] > iters[0]
    # the maps go: update() returns to no scaling and μ = λ
    op.clear_maps()
    pc.update()
    assert pc.info().scaling == 0 and pc.info().mu == lam and pc.scaling() is None
    sol.close()
    pc.close()
    op.close()


@pytest.mark.parametrize("Z,Ns,C", [("c128", (64, 80), 2), ("c64", (64, 64, 64), 1), ("c64", (15, 9), 2)])
def test_pcg_reproducible_graph_and_modes(Z, Ns, C):
    from nufft_pkg import nufft
    _, Zc, _, rtol = _dt(Z)
    s = _system(Ns, False, "poisson")
    lam = 1e-3 * float(s.e.max())
    op = s.operator(nufft, Z, C)
    pc = nufft.ToeplitzPreconditioner(op, lam=lam)
    bs = [b.astype(Zc) for b in s.bs[:C]]
    if C == 2:
        delta = np.zeros(s.shape)                      # another scale and an easy right-hand side: one Fourier mode over the array indices,
        delta[(1,) * len(Ns)] = 3e3                    # nearly an eigenvector of this rapidly decaying Toeplitz matrix
        bs[1] = np.fft.ifftn(delta).astype(Zc)
    sol = nufft.ToeplitzCG(op, maxiter=30, rtol=rtol, lam=lam, precond=pc)
    x1, it1, st1, h1 = _solve(sol, bs, C)
    x2, it2, st2, h2 = _solve(sol, bs, C)
    assert st1 == ("converged",) * C and max(it1) < 30
    assert it1 == it2 and st1 == st2 and _same(h1, h2) and all(np.array_equal(u, v) for u, v in zip(x1, x2))
    assert sol.info().iterations_enqueued == 30
    checking = nufft.ToeplitzCG(op, maxiter=30, rtol=rtol, lam=lam, precond=pc, check_every=3)
    x3, it3, st3, h3 = _solve(checking, bs, C)
    assert checking.info().iterations_enqueued == -(-max(it1) // 3) * 3 < 30
    assert it3 == it1 and st3 == st1 and _same(h3, h1) and all(np.array_equal(u, v) for u, v in zip(x1, x3))
    if C == 2:      # the component that finished first is frozen: its bits are those of a solver that stops right there
        first = int(np.argmin(it1))
        short = nufft.ToeplitzCG(op, maxiter=min(it1), rtol=rtol, lam=lam, precond=pc)
        xs_, its_, _, hs_ = _solve(short, bs, C)
        assert its_[first] == it1[first] and np.array_equal(xs_[first], x1[first])
        assert np.isnan(h1[min(it1) + 1:, first]).all()
        short.close()
    bd = tuple(_dev(b) for b in bs)
    out = tuple(torch.zeros_like(b) for b in bd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        sol.solve(bd if C > 1 else bd[0], out=out if C > 1 else out[0])
        with pytest.raises(ValueError):
            checking.solve(bd if C > 1 else bd[0], out=out if C > 1 else out[0])
    for _ in range(2):
        for o in out:
            o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert sol.iterations == it1 and sol.status == st1 and _same(sol.history().numpy(), h1)
        assert all(np.array_equal(o.cpu().numpy(), v) for o, v in zip(out, x1))
    del graph
    checking.close()
    sol.close()
    pc.close()
    op.close()


def test_pcg_warm_start_zero_rhs_and_breakdown():
    from nufft_pkg import nufft
    Z = "c128"
    _, Zc, _, rtol = _dt(Z)
    s = _system((64, 80), False, "poisson")
    op = s.operator(nufft, Z, 2)
    pc = nufft.ToeplitzPreconditioner(op)
    sol = nufft.ToeplitzCG(op, maxiter=50, rtol=rtol, precond=pc)
    bd = tuple(_dev(b.astype(Zc)) for b in s.bs)
    x = sol.solve(bd)
    torch.cuda.synchronize()
    assert sol.status == ("converged",) * 2 and min(sol.iterations) > 0
    keep = tuple(v.clone() for v in x)
    again = sol.solve(bd, x0=x, out=x)                    # already below rtol (drift ε · cond · iterations = 1e-16 · 5 · 20): nothing runs
    torch.cuda.synchronize()
    assert sol.iterations == (0, 0) and sol.status == ("converged",) * 2 and sol.history().shape == (1, 2)
    assert all(torch.equal(u, v) for u, v in zip(again, keep))
    rng_x0 = _rand(s.shape, 99).astype(Zc)
    warm = sol.solve(bd, x0=(_dev(rng_x0), _dev(rng_x0)))
    torch.cuda.synchronize()
    assert sol.status == ("converged",) * 2
    assert max(s.true_residual(0.0, w.cpu().numpy(), b) for w, b in zip(warm, s.bs)) <= 2 * rtol
    zero = torch.zeros_like(bd[0])
    xz = sol.solve((zero, bd[1]))
    torch.cuda.synchronize()
    h = sol.history().numpy()
    assert sol.iterations[0] == 0 and sol.status[0] == "converged" and not xz[0].any() and h[0, 0] == 0.0 and sol.residual[0] == 0.0
    assert torch.equal(xz[1], keep[1])                    # the other component does not notice
    sol.close()
    pc.close()
    op.close()
    # the singular clustered system with λ = 0: the floor keeps m finite, the solve ends with finite x whatever its status
    for Z in ("c128", "c64"):
        _, Zc, _, rtol = _dt(Z)
        sing = _system((48,), False, "singular")
        ops = sing.operator(nufft, Z)
        pcs = nufft.ToeplitzPreconditioner(ops, lam=0.0)
        sols = nufft.ToeplitzCG(ops, maxiter=300, rtol=rtol, lam=0.0, precond=pcs)
        xs, it, st, h = _solve(sols, [sing.bs[0].astype(Zc)], 1)
        print(f"singular system {Z}: status {st[0]} after {it[0]} iterations, last residual {sols.residual[0]:.3e}, max |x| {np.abs(xs[0]).max():.3e}")
        assert st[0] in ("breakdown", "max_iter", "converged") and np.isfinite(xs[0]).all() and np.isfinite(h[: it[0] + 1]).all()
        # a preconditioner that is not positive (a negative scaling cannot make it so, but NaN in d does): breakdown, finite x
        bad = np.ones(sing.shape, dtype=_dt(Z)[0])
        bad[3] = np.nan
        pcs.set_scaling(_dev(bad))
        xs, it, st, _ = _solve(sols, [sing.bs[0].astype(Zc)], 1)
        assert st == ("breakdown",) and it == (0,) and np.isfinite(xs[0]).all() and not xs[0].any()
        sols.close()
        pcs.close()
        ops.close()


def test_refusals():
    from nufft_pkg import nufft
    s = _system((64, 80), False, "poisson")
    op = s.operator(nufft, "c128")
    other = s.operator(nufft, "c128")
    two = s.operator(nufft, "c128", 2)
    f32 = s.operator(nufft, "c64")
    pc = nufft.ToeplitzPreconditioner(op)
    for wrong in (other, two, f32):                                          # another operator, ntransforms, element type
        with pytest.raises(ValueError, match="another operator"):
            nufft.ToeplitzCG(wrong, precond=pc)
    sol = nufft.ToeplitzCG(other)
    with pytest.raises(ValueError, match="another operator"):
        sol.set_preconditioner(pc)
    with pytest.raises(ValueError):
        sol.set_preconditioner(object())
    with pytest.raises(ValueError, match="another operator"):
        other.solve(_dev(s.bs[0]), precond=pc)
    with pytest.raises(nufft.DimensionMismatch):
        pc.set_scaling(torch.ones((80, 80), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        pc.set_scaling(torch.ones(s.shape, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        pc.set_scaling(torch.ones(s.shape, dtype=torch.float64))
    with pytest.raises(nufft.DimensionMismatch):
        pc.apply(torch.zeros((8, 8), dtype=torch.complex128, device="cuda"))
    # no spectrum yet
    plan = nufft.PlanNUFFT(np.complex128, (64, 80), backend=nufft.ROCBackend(0))
    empty = nufft.ToeplitzOperator(plan)
    with pytest.raises(ValueError, match="set_spectrum"):
        nufft.ToeplitzPreconditioner(empty)
    # a coupled operator
    K = 2
    spectra = torch.stack([_dev(s.spec)] * (K * (K + 1) // 2))
    two.set_spectra(spectra)
    with pytest.raises(ValueError, match="coupled"):
        nufft.ToeplitzPreconditioner(two)
    # closed objects
    good = nufft.ToeplitzCG(op, precond=pc)
    pc.close()
    with pytest.raises(ValueError, match="closed"):
        pc.apply(_dev(s.bs[0]))
    with pytest.raises(ValueError, match="closed"):
        pc.multiplier()
    with pytest.raises(ValueError, match="closed"):
        good.solve(_dev(s.bs[0]))
    with pytest.raises(ValueError, match="closed"):
        nufft.ToeplitzCG(op, precond=pc)
    good.set_preconditioner(None)
    good.solve(_dev(s.bs[0]))
    torch.cuda.synchronize()
    for o in (good, sol, op, other, two, f32, empty):
        o.close()
    plan.close()


@pytest.mark.parametrize("Z,Ns", [("c128", (64, 80)), ("c64", (48, 40))])
def test_no_change_without_a_preconditioner(Z, Ns):
    from nufft_pkg import nufft
    _, Zc, _, rtol = _dt(Z)
    s = _system(Ns, False, "poisson")
    op = s.operator(nufft, Z)
    b = [s.bs[0].astype(Zc)]
    a = nufft.ToeplitzCG(op, maxiter=40, rtol=rtol)
    c = nufft.ToeplitzCG(op, maxiter=40, rtol=rtol, precond=None)
    xa, ia, sa, ha = _solve(a, b, 1)
    xc, ic, sc, hc = _solve(c, b, 1)
    assert ia == ic and sa == sc and _same(ha, hc) and np.array_equal(xa[0], xc[0])
    assert a.info().array_bytes == c.info().array_bytes
    pc = nufft.ToeplitzPreconditioner(op)
    c.set_preconditioner(pc)
    assert c.info().array_bytes == a.info().array_bytes * 4 // 3            # one more array per component
    _solve(c, b, 1)
    c.set_preconditioner(None)                                              # cleared: the plain solver's bits again
    xd, id_, sd, hd = _solve(c, b, 1)
    assert id_ == ia and sd == sa and _same(hd, ha) and np.array_equal(xd[0], xa[0])
    for o in (a, c, pc, op):
        o.close()
