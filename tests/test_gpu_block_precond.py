"""The block-circulant preconditioner of a coupled operator and block PCG on the GPU, against the numpy reference
(block_precond_reference.py) run in the same element type.

Spectra: direct sums over point sets with the subspace basis of the tests (``BP.subspace_basis``) through ``op.set_spectra``; for large or
many-pair cases the analytic modulated-Poisson family (``BP.modulated_poisson_spectra``: positive definite by construction and asymmetric
in q, so a wrong index negation or a missing conjugate shows); for 64³ points on the device with the numpy side reading
``op.multiplier(a, b)``.  Bars are those of test_gpu_precond.py:
  * B and M⁻¹ r: 1e-12 (ComplexF64) / 1e-5 (ComplexF32), B element by element relative to max |B|, M⁻¹ r in rel-L2.  B(q) multiplies the relative
    error of E(q) by its spread (λ_max + shift) / (λ_min + shift), so every parity test asserts from the reference that the spread over all
    cells is <= 30, with λ = 0.1 λ_max(E) to get there; the shift is tested on its own with the bar scaled by 1 / floor.
  * five iterations of PCG: x and the history within 10 × that.
  * converged solves: true residual in float64 <= 2 rtol, iterations within ±(10 % + 1) of the reference's.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import block_precond_reference as BP  # noqa: E402
import cg_reference as CG  # noqa: E402
import precond_reference as P  # noqa: E402
import sense_reference as S  # noqa: E402
import subspace_reference as SR  # noqa: E402
import toeplitz_reference as R  # noqa: E402
from fft_lines_cases import SIZES as LINE_SIZES  # noqa: E402


def _dt(Z):
    return (np.float64, np.complex128, 1e-12, 1e-10) if Z == "c128" else (np.float32, np.complex64, 1e-5, 1e-4)


def _dev(a, Zc=None):
    return torch.from_numpy(np.ascontiguousarray(a if Zc is None else a.astype(Zc))).cuda()


def _rand(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


class System:
    """The spectra of the pairs a <= b, the float64 operator and block circulant from them, and a right-hand side.  kind: "uniform" (random
    weights, Np = 8 n points), "clustered" (half uniform, half N(0, 0.4²) folded, w = 1/Np), "singular" (every point N(π, 0.3²)) — all three with
    the subspace basis — and "analytic" (the modulated-Poisson family)."""

    def __init__(self, Ns, K, fftshift=False, kind="uniform", seed=0, basis_seed=None):
        rng = np.random.default_rng(seed)
        self.Ns, self.K, self.fftshift, self.shape = Ns, K, fftshift, (K,) + Ns[::-1]
        n = int(np.prod(Ns))
        self.xs = self.w = self.phi = None
        if kind == "analytic":
            self.spectra = BP.modulated_poisson_spectra(Ns, K, seed)
        else:
            if kind == "singular":
                Np = 400
                self.xs = [np.mod(np.pi + 0.3 * rng.standard_normal(Np), 2 * np.pi) for _ in Ns]
                self.w = rng.random(Np) + 0.1
            elif kind == "clustered":
                Np = 40000
                self.xs = [np.mod(np.concatenate([rng.random(Np // 2) * 2 * np.pi, 0.4 * rng.standard_normal(Np - Np // 2)]), 2 * np.pi) for _ in Ns]
                self.w = np.full(Np, 1.0 / Np)
            else:
                Np = max(2000, 8 * n)
                self.xs = [rng.random(Np) * 2 * np.pi for _ in Ns]
                self.w = (rng.random(Np) + 0.1) / Np
            self.phi = BP.subspace_basis(K, Np, seed if basis_seed is None else basis_seed)
            self.spectra = BP.separable_spectra(Ns, self.xs, self.w, self.phi)
        self.b = _rand(self.shape, seed + 1)
        self.set_multipliers(SR.multipliers(Ns, self.spectra), self.spectra)

    def set_multipliers(self, Ks, spectra=None):
        Ns, K = self.Ns, self.K
        self.Ks = Ks
        self.E = BP.block_eigenvalues(Ns, spectra if spectra is not None else [P.generating_sequence(Ns, k) for k in Ks], K)
        self.lam_max = float(np.linalg.eigvalsh(np.moveaxis(self.E.reshape(K, K, -1), -1, 0)).max())
        self.max_e = max(float(self.E[a, a].real.max()) for a in range(K))
        self.min_e = min(float(self.E[a, a].real.min()) for a in range(K))
        self.apply = lambda p: np.stack(SR.block_apply(Ns, self.Ks, [np.asarray(p[a]).astype(np.complex128) for a in range(K)], self.fftshift))
        self._B = {}

    def B(self, mu, floor=1e-6):
        if (mu, floor) not in self._B:
            self._B[(mu, floor)] = BP.block_inverse(self.E, mu, floor)
        return self._B[(mu, floor)]

    def true_residual(self, lam, x, b, apply=None):
        x, b = np.asarray(x).astype(np.complex128), np.asarray(b).astype(np.complex128)
        return float(np.linalg.norm((b - ((apply or self.apply)(x) + lam * x)).ravel()) / np.linalg.norm(b.ravel()))

    def operator(self, nufft, Z, dense=False):
        _, Zc, _, _ = _dt(Z)
        plan = nufft.PlanNUFFT(Zc, self.Ns, backend=nufft.ROCBackend(0), options={"NUFFT_TOEPLITZ_FUSED": 0} if dense else {},
                               fftshift=self.fftshift, ntransforms=self.K)
        op = nufft.ToeplitzOperator(plan)
        op.set_spectra(_dev(np.stack(self.spectra), Zc))
        plan.close()
        assert op.coupled
        return op


_SYSTEMS = {}


def _system(Ns, K, fftshift=False, kind="uniform"):
    key = (Ns, K, fftshift, kind)
    if key not in _SYSTEMS:
        _SYSTEMS[key] = System(Ns, K, fftshift, kind, seed=7 * sum(Ns) + K + len(kind))
    return _SYSTEMS[key]


def _points_system_64(nufft):
    """64³, K = 2, ComplexF32, from 8 n uniform points on the device with the subspace basis; the K_ab for numpy from the operator itself.  Built
    once and kept for the module (the reference is the expensive part, and it belongs to this operator's multipliers)."""
    if "64" not in _SYSTEMS:
        Ns, K = (64, 64, 64), 2
        rng = np.random.default_rng(64)
        Np = 8 * 64 ** 3
        xs = [rng.random(Np) * 2 * np.pi for _ in Ns]
        phi = BP.subspace_basis(K, Np, 64)
        plan = nufft.PlanNUFFT(np.complex64, Ns, backend=nufft.ROCBackend(0), ntransforms=K, m=4)
        op = nufft.ToeplitzOperator(plan)
        op.set_points(tuple(_dev(x.astype(np.float32)) for x in xs), _dev(np.full(Np, 1.0 / Np, dtype=np.float32)), basis=_dev(phi, np.complex64))
        plan.close()
        s = System.__new__(System)
        s.Ns, s.K, s.fftshift, s.shape = Ns, K, False, (K,) + Ns[::-1]
        s.b = _rand(s.shape, 640)
        s.set_multipliers([op.multiplier(a, b).cpu().numpy().astype(np.complex128) for a, b in SR.pairs(K)])
        _SYSTEMS["64"] = (s, op)
    return _SYSTEMS["64"]


def _expected_path(Ns, K, Z):
    if not (len(Ns) >= 2 and all(n in LINE_SIZES for n in Ns)):
        return "dense"
    tier = 2 if K <= 2 else 4 if K <= 4 else 8 if K <= 8 else 16
    line = Ns[0] + Ns[0] // 16 + 1
    return "fused" if (8 if Z == "c64" else 16) * (Ns[0] + tier * line) <= 160 * 1024 else "dense"


def _block_of(pc, K):
    """The (K, K) + shape array of B from the object's views."""
    first = pc.block(0, 0).cpu().numpy()
    B = np.zeros((K, K) + first.shape, dtype=np.complex128)
    for a, b in SR.pairs(K):
        v = pc.block(a, b).cpu().numpy()
        assert v.shape == first.shape and np.iscomplexobj(v) == (a != b)
        B[a, b] = v
        if a != b:
            B[b, a] = np.conj(v)
    return B


def _check_B(pc, s, mu, bar, floor=1e-6):
    ref, floored = s.B(mu, floor)
    got = _block_of(pc, s.K)
    scale = np.abs(ref).max()
    worst = max(np.abs(got[a, b] - ref[a, b]).max() for a, b in SR.pairs(s.K)) / scale
    return worst, R.rel(got, ref), floored


def _solve(sol, b, Zc):
    bd = tuple(_dev(v, Zc) for v in b)
    x = sol.solve(bd)
    torch.cuda.synchronize()
    return np.stack([v.cpu().numpy() for v in x]), sol.iterations, sol.status, sol.history().numpy()


# ---- G1: B ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Ns,K,fftshift", [((15, 9), 2, False), ((48, 40), 3, False), ((64, 80), 2, False), ((64, 80), 2, True)])
@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_blocks_match_the_reference(Ns, K, fftshift, Z):
    from nufft_pkg import nufft
    _, Zc, bar, _ = _dt(Z)
    s = _system(Ns, K, fftshift)
    lam = 0.1 * s.lam_max
    spread = BP.spread(s.E, lam, 1e-6)
    assert spread <= 30, spread
    op = s.operator(nufft, Z)
    pc = nufft.ToeplitzPreconditioner(op, lam=lam, block=True)
    i = pc.info()
    assert pc.path == _expected_path(Ns, K, Z) == ("fused" if Ns == (64, 80) else "dense")
    assert pc.coupled == K and i.mu == lam and i.scaling == 0 and pc.scaling() is None
    assert i.multiplier_bytes == K * K * int(np.prod(Ns)) * (4 if Z == "c64" else 8)
    assert abs(i.max_e - s.max_e) <= 10 * bar * s.max_e and abs(i.min_e - s.min_e) <= 10 * bar * s.max_e
    worst, l2, floored = _check_B(pc, s, lam, bar)
    print(f"B {Z} N={Ns} K={K} shift={fftshift} ({pc.path}): max {worst:.3e} of max |B|, rel-L2 {l2:.3e} (bar {bar:g}); spread {spread:.1f}")
    assert worst <= bar and l2 <= bar
    assert pc.floored_cells == 0 == floored
    pc.close()
    op.close()


# ---- G2, G3: the apply ------------------------------------------------------------------------------------------------------------

def _check_apply(nufft, s, Z, dense=False, d=None, inplace=False, path=None):
    T, Zc, bar, _ = _dt(Z)
    lam = 0.1 * s.lam_max
    spread = BP.spread(s.E, lam, 1e-6)
    assert spread <= 30, spread
    op = s.operator(nufft, Z, dense=dense)
    pc = nufft.ToeplitzPreconditioner(op, lam=lam, block=True)
    assert pc.path == (path or ("dense" if dense else _expected_path(s.Ns, s.K, Z))), (s.Ns, s.K, pc.path)
    if d is not None:
        pc.set_scaling(_dev(d.astype(T)))
        assert pc.info().scaling == 2
    rs = np.stack([_rand(s.shape[1:], 31 + c) for c in range(s.K)]).astype(Zc)
    rd = tuple(_dev(r) for r in rs)
    out = pc.apply(rd, out=rd if inplace else None)
    torch.cuda.synchronize()
    if inplace:
        assert all(o.data_ptr() == r.data_ptr() for o, r in zip(out, rd))
    else:
        assert all(np.array_equal(r.cpu().numpy(), h) for r, h in zip(rd, rs))          # the inputs are only read
    got = np.stack([o.cpu().numpy() for o in out])
    ref = BP.block_apply(s.B(lam)[0], None if d is None else d.astype(T).astype(np.float64), rs)
    err = max(R.rel(got[a], ref[a]) for a in range(s.K))
    print(f"apply {Z} N={s.Ns} K={s.K} {pc.path}{' scaled' if d is not None else ''}{' in place' if inplace else ''}: {err:.3e} (bar {bar:g})")
    assert err <= bar and pc.floored_cells == 0
    pc.close()
    op.close()
    return got


@pytest.mark.parametrize("N1", LINE_SIZES)
@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_apply_every_line_length(N1, Z):
    from nufft_pkg import nufft
    assert len(LINE_SIZES) == 13
    _check_apply(nufft, _system((N1, 64), 2, False, "analytic"), Z, path="fused")


@pytest.mark.parametrize("K", [3, 5, 9])                      # the tiers 4, 8, 16 of the fused kernel (K = 2 above)
@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_apply_every_tier(K, Z):
    from nufft_pkg import nufft
    _check_apply(nufft, _system((64, 64), K, True, "analytic"), Z, path="fused")


@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_apply_three_dimensions_scaled_in_place(Z):
    from nufft_pkg import nufft
    s = _system((64, 80, 96), 2, True, "analytic")
    d = np.random.default_rng(9).random(s.shape[1:]) + 0.5
    _check_apply(nufft, s, Z, path="fused")
    _check_apply(nufft, s, Z, d=d, inplace=True, path="fused")


@pytest.mark.parametrize("Z,Ns,K", [("c64", (15, 9), 2), ("c128", (15, 9), 2), ("c128", (48, 40), 3), ("c64", (48, 40), 3), ("c128", (48,), 2),
                                    ("c64", (48,), 2)])      # (15, 9) in ComplexF32: an odd cell count, the tail behind the last pack
def test_apply_dense_path(Z, Ns, K):
    from nufft_pkg import nufft
    s = _system(Ns, K, False, "analytic")
    d = np.random.default_rng(10).random(s.shape[1:]) + 0.5
    _check_apply(nufft, s, Z, path="dense")
    _check_apply(nufft, s, Z, d=d, inplace=True, path="dense")


@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_apply_paths_agree(Z):
    from nufft_pkg import nufft
    _, _, bar, _ = _dt(Z)
    s = _system((64, 80), 2, False, "analytic")
    d = np.random.default_rng(11).random(s.shape[1:]) + 0.5
    fused = _check_apply(nufft, s, Z, d=d, path="fused")
    dense = _check_apply(nufft, s, Z, d=d, dense=True, path="dense")
    assert max(R.rel(a, b) for a, b in zip(fused, dense)) <= 2 * bar


def test_lines_that_do_not_fit_take_the_dense_path():
    from nufft_pkg import nufft
    s = _system((1024, 64), 9, False, "analytic")            # 9 lines (tier 16) of 1024 ComplexF64 cells: beyond one wave's LDS
    assert _expected_path(s.Ns, 9, "c128") == "dense" and _expected_path(s.Ns, 2, "c128") == "fused"
    _check_apply(nufft, s, "c128", path="dense")


# ---- G4: Hermitian and positive ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["(64, 80) K=3 c128", "(64, 80) K=3 c64", "64^3 K=2 c64"])
def test_inverse_is_hermitian_and_positive(case):
    from nufft_pkg import nufft
    Z = case.split()[-1]
    T, Zc, bar, _ = _dt(Z)
    if case.startswith("64^3"):
        s, op = _points_system_64(nufft)
    else:
        s = _system((64, 80), 3, False, "analytic")
        op = s.operator(nufft, Z)
    pc = nufft.ToeplitzPreconditioner(op, block=True).set_scaling(_dev((np.random.default_rng(12).random(s.shape[1:]) + 0.5).astype(T)))
    assert pc.path == "fused"
    a, b = _rand(s.shape, 1).astype(Zc), _rand(s.shape, 2).astype(Zc)
    Ma, Mb = (np.stack([o.cpu().numpy() for o in pc.apply(tuple(_dev(c) for c in v))]).astype(np.complex128) for v in (a, b))
    a, b = a.astype(np.complex128), b.astype(np.complex128)
    lhs, rhs = np.vdot(a, Mb), np.conj(np.vdot(b, Ma))
    scale = np.linalg.norm(a) * np.linalg.norm(Mb)
    print(f"Hermitian {case}: |<a, Mb> - conj<b, Ma>| / (|a| |Mb|) = {abs(lhs - rhs) / scale:.3e}")
    assert abs(lhs - rhs) <= 10 * bar * scale
    assert np.vdot(a, Ma).real > 0 and np.vdot(b, Mb).real > 0
    assert abs(np.vdot(a, Ma).imag) <= 10 * bar * np.linalg.norm(a) * np.linalg.norm(Ma)
    pc.close()
    if not case.startswith("64^3"):
        op.close()


# ---- G5: the shift ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Z", ["c128", "c64"])
@pytest.mark.parametrize("floor", [1e-2, 1e-4])
def test_shift_is_in_force(Z, floor):
    from nufft_pkg import nufft
    _, Zc, bar, _ = _dt(Z)
    s = _system((48, 40), 2, False, "singular")
    lam_min = float(np.linalg.eigvalsh(np.moveaxis(s.E.reshape(2, 2, -1), -1, 0)).min())
    shift = BP.shift_of(s.E, 0.0, floor)
    assert lam_min < 0.1 * shift and shift == floor * s.max_e
    op = s.operator(nufft, Z)
    pc = nufft.ToeplitzPreconditioner(op, lam=0.0, floor=floor, block=True)
    assert pc.floor == floor and pc.info().floor == floor and pc.info().mu == 0.0
    worst, l2, floored = _check_B(pc, s, 0.0, bar, floor)
    print(f"shift {Z} floor={floor:g}: B max {worst:.3e} of max |B|, rel-L2 {l2:.3e} (bar {bar / floor:g}); floored cells {pc.floored_cells} (reference {floored})")
    assert worst <= bar / floor and l2 <= bar / floor
    B = _block_of(pc, 2)
    n = int(np.prod(s.Ns))
    assert np.abs(B).max() <= (1 + 1e-3) / (n * shift * (1 if pc.floored_cells == 0 else BP.PIVOT_FRACTION))
    out = pc.apply(tuple(_dev(v, Zc) for v in s.b))
    torch.cuda.synchronize()
    assert all(torch.isfinite(torch.view_as_real(o)).all() for o in out)
    pc.close()
    op.close()


# ---- G6: five iterations ----------------------------------------------------------------------------------------------------------

def _five_iterations(nufft, s, op, Z, path):
    _, Zc, bar, _ = _dt(Z)
    lam = 0.1 * s.lam_max
    assert BP.spread(s.E, lam, 1e-6) <= 30
    pc = nufft.ToeplitzPreconditioner(op, lam=lam, block=True)
    assert pc.path == path
    b = s.b.astype(Zc)
    sol = nufft.ToeplitzCG(op, maxiter=5, rtol=0.0, lam=lam, precond=pc)
    x, iters, status, hist = _solve(sol, b, Zc)
    assert iters == (5,) * s.K and status == ("max_iter",) * s.K and hist.shape == (6, s.K)
    assert all(np.array_equal(hist[:, 0], hist[:, c]) for c in range(s.K))                    # one system: one history
    B = s.B(lam)[0]
    ref = P.pcg(s.apply, lambda r: BP.block_apply(B, None, r), b, lam=lam, rtol=0.0, max_iter=5, dtype=Zc)
    ex, eh = R.rel(x, ref["x"]), R.rel(hist[:, 0], ref["history"])
    print(f"block PCG 5 iterations {Z} N={s.Ns} K={s.K} pc {pc.path}: x {ex:.3e}, history {eh:.3e} (bar {10 * bar:g})")
    assert ex <= 10 * bar and eh <= 10 * bar
    sol.close()
    pc.close()


@pytest.mark.parametrize("Z,Ns,K,path", [("c128", (64, 80), 2, "fused"), ("c64", (64, 80), 2, "fused"), ("c128", (48, 40), 3, "dense"),
                                         ("c64", (48, 40), 3, "dense")])
def test_pcg_fixed_iteration_count(Z, Ns, K, path):
    from nufft_pkg import nufft
    s = _system(Ns, K)
    op = s.operator(nufft, Z)
    _five_iterations(nufft, s, op, Z, path)
    op.close()


def test_pcg_fixed_iteration_count_64_cubed():
    from nufft_pkg import nufft
    s, op = _points_system_64(nufft)
    _five_iterations(nufft, s, op, "c64", "fused")


# ---- G7: converged ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_pcg_converged_on_clustered_points(Z):
    from nufft_pkg import nufft
    _, Zc, _, rtol = _dt(Z)
    s = _system((64, 80), 2, False, "clustered")
    lam = 1e-3 * s.lam_max
    op = s.operator(nufft, Z)
    pc = nufft.ToeplitzPreconditioner(op, lam=lam, block=True)
    b = s.b.astype(Zc)
    sol = nufft.ToeplitzCG(op, maxiter=2000, rtol=rtol, lam=lam, precond=pc, check_every=10)
    x, iters, status, hist = _solve(sol, b, Zc)
    B = s.B(lam)[0]
    ref = P.pcg(s.apply, lambda r: BP.block_apply(B, None, r), b, lam=lam, rtol=rtol, max_iter=2000, dtype=Zc)
    tr = s.true_residual(lam, x, b)
    assert status == ("converged",) * 2 and iters[0] == iters[1] and tr <= 2 * rtol
    assert abs(iters[0] - ref["iterations"]) <= 0.1 * ref["iterations"] + 1
    assert sol.residual[0] <= rtol * (1 + 1e-12) and hist[iters[0], 0] == sol.residual[0]
    sol.set_preconditioner(None)                                            # the same solver object, plain joint CG
    xp, itp, stp, _ = _solve(sol, b, Zc)
    print(f"clustered (64, 80) K=2 {Z}: block PCG {iters[0]} iterations (reference {ref['iterations']}), true residual / rtol {tr / rtol:.3f}; joint CG {itp[0]}")
    assert stp == ("converged",) * 2 and itp[0] >= 2 * iters[0]
    assert s.true_residual(lam, xp, b) <= 2 * rtol
    sol.close()
    pc.close()
    op.close()


# ---- G8: coil maps ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Z", ["c128", "c64"])
def test_pcg_with_coil_maps(Z):
    from nufft_pkg import nufft
    T, Zc, bar, rtol = _dt(Z)
    s = _system((64, 80), 2, False, "clustered")
    maps = S.smooth_maps(3, s.shape[1:], seed=3, zero_region=False).astype(Zc)
    lam = 1e-3 * s.lam_max
    op = s.operator(nufft, Z)
    op.set_maps(_dev(maps))
    pc = nufft.ToeplitzPreconditioner(op, lam=lam, block=True)
    maps64 = maps.astype(np.complex128)
    d_ref, mu_ref = P.coil_scaling(maps64, lam)
    i = pc.info()
    assert i.scaling == 1 and abs(i.mu - mu_ref) <= 10 * bar * mu_ref
    d = pc.scaling().cpu().numpy().astype(np.float64)
    assert np.abs(d - d_ref).max() <= bar * d_ref.max()
    GS = lambda p: sum(np.conj(m)[None] * s.apply(m[None] * np.asarray(p).astype(np.complex128)) for m in maps64)
    b = s.b.astype(Zc)
    sol = nufft.ToeplitzCG(op, maxiter=2000, rtol=rtol, lam=lam, precond=pc, check_every=10)
    x, iters, status, _ = _solve(sol, b, Zc)
    tr = s.true_residual(lam, x, b, apply=GS)
    print(f"3 coils (64, 80) K=2 {Z}: block PCG {iters[0]} iterations, true residual / rtol {tr / rtol:.3f}, mu {i.mu:.4e} (reference {mu_ref:.4e})")
    assert status == ("converged",) * 2 and tr <= 2 * rtol
    op.clear_maps()                                                         # the maps go: update() returns to no scaling and μ = λ
    pc.update()
    assert pc.info().scaling == 0 and pc.info().mu == lam and pc.scaling() is None
    sol.close()
    pc.close()
    op.close()


# ---- G9: reproducibility and modes ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Z,Ns", [("c128", (64, 80)), ("c64", (15, 9))])
def test_pcg_reproducible_graph_and_modes(Z, Ns):
    from nufft_pkg import nufft
    _, Zc, _, rtol = _dt(Z)
    K = 2
    s = _system(Ns, K, False, "analytic")
    lam = 0.1 * s.lam_max
    op = s.operator(nufft, Z)
    pc = nufft.ToeplitzPreconditioner(op, lam=lam, block=True)
    b = s.b.astype(Zc)
    sol = nufft.ToeplitzCG(op, maxiter=40, rtol=rtol, lam=lam, precond=pc)
    x1, it1, st1, h1 = _solve(sol, b, Zc)
    x2, it2, st2, h2 = _solve(sol, b, Zc)
    assert st1 == ("converged",) * K and 0 < it1[0] < 40 and s.true_residual(lam, x1, b) <= 2 * rtol
    assert it1 == it2 and st1 == st2 and _same(h1, h2) and np.array_equal(x1, x2)
    assert sol.info().iterations_enqueued == 40
    checking = nufft.ToeplitzCG(op, maxiter=40, rtol=rtol, lam=lam, precond=pc, check_every=7)
    x3, it3, st3, h3 = _solve(checking, b, Zc)
    assert checking.info().iterations_enqueued == min(40, -(-it1[0] // 7) * 7)
    assert it3 == it1 and st3 == st1 and _same(h3, h1) and np.array_equal(x1, x3)
    bd = tuple(_dev(v) for v in b)
    out = tuple(torch.zeros_like(v) for v in bd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        sol.solve(bd, out=out)
        with pytest.raises(ValueError):
            checking.solve(bd, out=out)
    for _ in range(2):
        for o in out:
            o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert sol.iterations == it1 and sol.status == st1 and _same(sol.history().numpy(), h1)
        assert np.array_equal(np.stack([o.cpu().numpy() for o in out]), x1)
    del graph
    # warm start from the solution: nothing runs; from a random guess: converges; b = 0: x = 0 at once
    xd = tuple(_dev(v) for v in x1)
    again = sol.solve(bd, x0=xd)
    torch.cuda.synchronize()
    assert sol.status == ("converged",) * K and sol.iterations[0] <= 1
    warm = sol.solve(bd, x0=tuple(_dev(v, Zc) for v in _rand(s.shape, 99)))
    torch.cuda.synchronize()
    assert sol.status == ("converged",) * K
    assert s.true_residual(lam, np.stack([w.cpu().numpy() for w in warm]), b) <= 2 * rtol
    xz = sol.solve(tuple(torch.zeros_like(v) for v in bd))
    torch.cuda.synchronize()
    assert sol.iterations == (0,) * K and sol.status == ("converged",) * K and not any(v.any() for v in xz) and sol.residual[0] == 0.0
    del again
    checking.close()
    sol.close()
    pc.close()
    op.close()


def test_update_follows_another_basis():
    from nufft_pkg import nufft
    Z, Ns, K = "c128", (64, 80), 2
    T, Zc, bar, _ = _dt(Z)
    rng = np.random.default_rng(5)
    Np = 8 * 64 * 80
    xs = [rng.random(Np) * 2 * np.pi for _ in Ns]
    w = (rng.random(Np) + 0.1) / Np
    plan = nufft.PlanNUFFT(Zc, Ns, backend=nufft.ROCBackend(0), ntransforms=K, m=8)
    op = nufft.ToeplitzOperator(plan)
    pd, wd = tuple(_dev(x) for x in xs), _dev(w)
    s = System.__new__(System)
    s.Ns, s.K, s.fftshift, s.shape = Ns, K, False, (K,) + Ns[::-1]
    pc, before, lam = None, None, None
    for seed in (1, 2):
        op.set_points(pd, wd, basis=_dev(BP.subspace_basis(K, Np, seed) * (1.0 if seed == 1 else 1.5)))
        s.set_multipliers([op.multiplier(a, b).cpu().numpy().astype(np.complex128) for a, b in SR.pairs(K)])
        if pc is None:
            lam = 0.1 * s.lam_max
            pc = nufft.ToeplitzPreconditioner(op, lam=lam, block=True)
        else:
            assert np.array_equal(_block_of(pc, K), before)                 # nothing changes until update()
            pc.update()
        assert BP.spread(s.E, lam, 1e-6) <= 30
        worst, l2, _ = _check_B(pc, s, lam, bar)
        print(f"update, basis {seed}: B max {worst:.3e} of max |B| (bar {bar:g})")
        assert worst <= bar and l2 <= bar and abs(pc.info().max_e - s.max_e) <= 10 * bar * s.max_e
        if before is not None:
            assert np.abs(_block_of(pc, K) - before).max() > 100 * bar * np.abs(before).max()
        before = _block_of(pc, K)
    # a plain set_points: the operator no longer couples its components
    op.set_points(pd, wd)
    with pytest.raises(ValueError, match="coupled"):
        pc.update()
    plan.close()
    pc.close()
    op.close()


# ---- G10: refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals():
    from nufft_pkg import nufft
    s = _system((64, 80), 2, False, "analytic")
    op = s.operator(nufft, "c128")
    other = s.operator(nufft, "c128")
    plan = nufft.PlanNUFFT(np.complex128, (64, 80), backend=nufft.ROCBackend(0), ntransforms=2)
    plain = nufft.ToeplitzOperator(plan)
    plain.set_spectrum(_dev(s.spectra[0]))
    with pytest.raises(ValueError, match="nufft_precond_create"):           # block=True on an uncoupled operator
        nufft.ToeplitzPreconditioner(plain, block=True)
    with pytest.raises(ValueError, match="coupled"):                        # block=False on a coupled one
        nufft.ToeplitzPreconditioner(op)
    with pytest.raises(ValueError, match="block=True"):
        nufft.ToeplitzPreconditioner(op, block=False)
    pc = nufft.ToeplitzPreconditioner(op, block=True)
    scalar = nufft.ToeplitzPreconditioner(plain)
    bd = tuple(_dev(v) for v in s.b)
    # a scalar object handed to a coupled solver: it was created while the operator was uncoupled
    sol = nufft.ToeplitzCG(plain, precond=scalar)
    plain.set_spectra(_dev(np.stack(s.spectra)))
    with pytest.raises(ValueError, match="block"):
        sol.solve(bd)
    with pytest.raises(ValueError, match="coupled"):
        scalar.update()
    sol.close()
    # a block object handed to another operator's solver
    with pytest.raises(ValueError, match="another operator"):
        nufft.ToeplitzCG(other, precond=pc)
    with pytest.raises(ValueError, match="another operator"):
        other.solve(bd, precond=pc)
    # a block object whose operator is no longer coupled
    sol = nufft.ToeplitzCG(op, precond=pc)
    op.set_spectrum(_dev(s.spectra[0]))
    with pytest.raises(ValueError):
        pc.update()
    with pytest.raises(ValueError, match="no longer couples"):
        sol.solve(bd)
    op.set_spectra(_dev(np.stack(s.spectra)))
    pc.update()
    sol.solve(bd)
    torch.cuda.synchronize()
    # views
    with pytest.raises(ValueError, match="block_ptr"):
        pc.multiplier()
    with pytest.raises(ValueError):
        pc.block(1, 0)
    with pytest.raises(ValueError):
        pc.block(0, 2)
    with pytest.raises(ValueError):
        scalar.block(0, 0)
    assert scalar.coupled == 0 and scalar.floored_cells == 0
    # a build on a capturing stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        with pytest.raises(ValueError, match="capturing"):
            pc.update()
        pc.apply(bd)
    del graph
    # closed objects
    pc.close()
    for call in (lambda: pc.apply(bd), lambda: pc.block(0, 0), lambda: pc.coupled, lambda: pc.floored_cells, lambda: sol.solve(bd)):
        with pytest.raises(ValueError, match="closed"):
            call()
    for o in (sol, scalar, op, other, plain):
        o.close()
    plan.close()


# ---- G11: nothing else moved ------------------------------------------------------------------------------------------------------

def test_other_solvers_keep_their_bits():
    from nufft_pkg import nufft
    Z = "c64"
    _, Zc, _, rtol = _dt(Z)
    s = _system((64, 80), 2, False, "analytic")
    lam = 0.1 * s.lam_max
    b = s.b.astype(Zc)
    # uncoupled PCG (the scalar object on independent components) and plain joint CG, before any block object exists in the process ...
    plan = nufft.PlanNUFFT(Zc, s.Ns, backend=nufft.ROCBackend(0), ntransforms=2)
    plain = nufft.ToeplitzOperator(plan)
    plain.set_spectrum(_dev(s.spectra[0], Zc))
    plan.close()
    spc = nufft.ToeplitzPreconditioner(plain, lam=lam)
    upcg = nufft.ToeplitzCG(plain, maxiter=30, rtol=rtol, lam=lam, precond=spc)
    op = s.operator(nufft, Z)
    joint = nufft.ToeplitzCG(op, maxiter=30, rtol=rtol, lam=lam)
    first = (_solve(upcg, b, Zc), _solve(joint, b, Zc))
    # ... and after a block solve
    pc = nufft.ToeplitzPreconditioner(op, lam=lam, block=True)
    blk = nufft.ToeplitzCG(op, maxiter=30, rtol=rtol, lam=lam, precond=pc)
    xb, itb, stb, _ = _solve(blk, b, Zc)
    assert stb == ("converged",) * 2
    joint.set_preconditioner(pc)
    _solve(joint, b, Zc)
    joint.set_preconditioner(None)
    second = (_solve(upcg, b, Zc), _solve(joint, b, Zc))
    for (x1, i1, s1, h1), (x2, i2, s2, h2) in zip(first, second):
        assert i1 == i2 and s1 == s2 and _same(h1, h2) and np.array_equal(x1, x2)
    assert first[0][2] == ("converged",) * 2 and first[1][2] == ("converged",) * 2
    for o in (blk, joint, upcg, pc, spc, op, plain):
        o.close()
