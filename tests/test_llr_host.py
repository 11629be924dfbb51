"""The numpy reference of the locally low-rank proximal map (llr_reference.py): the properties of a proximal map on
the SVD route, the kernel's Jacobi eigensolver against ``np.linalg.eigh``, and the kernel's Gram route against the SVD route.

Bars.  ``P = V diag(f) V^H`` from ``jacobi_eigh`` against the one from ``eigh``: Frobenius distance <= 64 ε₆₄ (|P_ij| <= 1).  The
threshold there is half the largest singular value: f(λ) = 1 − t / sqrt(λ) has slope <= 1 / (2 t²) above the threshold, so an error
δ ‖H‖ of either eigensolver moves P by about δ ‖H‖ / (2 t²) = 2 δ, and both stay well inside the bar; a threshold far below σ_max would
measure the conditioning of the map, not the solver.  Gram route against SVD route: rel-L2 <= 64 ε of the storage type, the bar of
the GPU test (measured here: 5e-16 ... 1.3e-15 in complex128, 2.6e-8 with complex64 storage).
"""
import numpy as np
import pytest

import llr_cases as LC
import llr_reference as L

E64 = 2.0 ** -52


@pytest.mark.parametrize("Ns,K,block", LC.SOLVER_CASES)
def test_prox_properties(Ns, K, block):
    x, y = LC.low_rank_input(Ns, K, 0), LC.low_rank_input(Ns, K, 1)
    t = LC.median_threshold(x, block)
    shift = tuple(b // 2 for b in block)
    for s in (None, shift):
        px, nuc, zero = L.prox(x, block, t, s)
        py, _, _ = L.prox(y, block, t, s)
        d, e = px - py, x - y
        assert np.vdot(d, d).real <= np.vdot(d, e).real * (1 + 1e-12)              # firmly non-expansive
        assert 0.2 <= zero <= 0.95
        assert abs(nuc - L.block_singular_values(px, block, s).sum()) <= 1e-12 * nuc
        ident, n0, z0 = L.prox(x, block, 0.0, s)
        assert LC.rel(ident, x) <= 1e-13 and z0 == 0.0
        big, nb, zb = L.prox(x, block, 1.001 * L.block_singular_values(x, block, s).max(), s)
        assert not big.any() and nb == 0.0 and zb == 1.0
        scaled, ns, _ = L.prox(3.5 * x, block, 3.5 * t, s)
        assert LC.rel(scaled, 3.5 * px) <= 1e-13 and abs(ns - 3.5 * nuc) <= 1e-12 * ns
    moved = L.prox(x, block, t, shift)[0]
    assert LC.rel(moved, px) <= 1e-13 and LC.rel(moved, L.prox(x, block, t)[0]) > 1e-3   # the shift matters


def test_shift_sequence():
    block = (4, 8, 2)
    seq = [L.shift_sequence(5, block, it) for it in range(1, 40)]
    assert all(0 <= s < b for sh in seq for s, b in zip(sh, block)) and len(set(seq)) > 10
    assert seq[6] == L.shift_sequence(5, block, 7) and L.shift_sequence(6, block, 7) != seq[6]
    state = (5 * L.LCG_A + L.LCG_C) & L.MASK
    assert seq[0][0] == (state >> 33) % 4


def _unitary(rng, K):
    q, _ = np.linalg.qr(rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K)))
    return q


def _gram_matrices(K, rng):
    out = {}
    m = rng.standard_normal((64, K)) + 1j * rng.standard_normal((64, K))
    out["random"] = m.conj().T @ m
    v = rng.standard_normal(K) + 1j * rng.standard_normal(K)
    out["rank-1"] = np.outer(v.conj(), v)
    m = rng.standard_normal((4, K)) + 1j * rng.standard_normal((4, K))
    out["rank <= 4 (2 x 2 blocks)"] = m.conj().T @ m
    out["zero"] = np.zeros((K, K), dtype=np.complex128)
    q = _unitary(rng, K)
    lam = np.linspace(1.0, 2.0, K)
    lam[: (K + 1) // 2] = 2.0
    out["repeated"] = (q * lam[None, :]) @ q.conj().T
    out["condition 1e12"] = (q * np.logspace(0, -12, K)[None, :]) @ q.conj().T if K > 1 else np.array([[1e-12 + 0j]])
    return out


def test_jacobi_against_eigh():
    rng = np.random.default_rng(24)
    most = 0
    for K in (1, 2, 3, 8, 16):
        for name, H in _gram_matrices(K, rng).items():
            H = 0.5 * (H + H.conj().T)
            lam_e, V_e = np.linalg.eigh(H)
            lam, V, sweeps = L.jacobi_eigh(H)
            most = max(most, sweeps)
            t = 0.5 * np.sqrt(max(lam_e.max(), 0.0))
            P, nuc = L.shrink_matrix(lam, V, t)
            P_e, nuc_e = L.shrink_matrix(lam_e, V_e, t)
            err = np.linalg.norm(P - P_e)
            scale = max(abs(lam_e).max(), 1e-300)
            print(f"K={K:2d} {name:26s}: {sweeps} sweeps, |P - P_eigh| = {err / E64:.1f} ε, eigenvalues {np.abs(np.sort(lam) - lam_e).max() / scale / E64:.1f} ε")
            assert np.isfinite(P).all() and err <= 64 * E64
            assert np.abs(np.sort(lam) - lam_e).max() <= 64 * E64 * scale
            assert abs(nuc - nuc_e) <= 64 * E64 * max(nuc_e, np.sqrt(scale))
            assert np.linalg.norm(V.conj().T @ V - np.eye(K)) <= 64 * E64
            assert sweeps < L.SWEEPS_MAX
            if name == "zero":
                assert sweeps == (1 if K > 1 else 0) and not P.any()
    print(f"largest sweep count {most} (cap {L.SWEEPS_MAX})")
    assert most <= 12


@pytest.mark.parametrize("Z", ["c128", "c64"])
@pytest.mark.parametrize("Ns,K,block", LC.SOLVER_CASES)
def test_gram_route_against_svd_route(Ns, K, block, Z):
    x = LC.low_rank_input(Ns, K).astype(LC.CTYPE[Z])
    t = LC.median_threshold(x, block)
    shift = tuple(b - 1 for b in block)
    for s in (None, shift):
        want, nuc, zero = L.prox(x, block, t, s)
        got, nuc_g, sweeps = L.prox_gram(x, block, t, s)
        err = LC.rel(got.astype(LC.CTYPE[Z]), want)
        print(f"Gram route {Z} N={Ns} K={K} block={block} shift={s}: rel-L2 {err:.2e} = {err / LC.EPS[Z]:.2f} ε, zero share {zero:.2f}, {sweeps} sweeps")
        assert 0.2 <= zero <= 0.95 and err <= 64 * LC.EPS[Z] and sweeps < L.SWEEPS_MAX
        assert abs(nuc_g - nuc) <= 64 * E64 * np.sqrt(x.size) * nuc
