"""numpy restatement of the block-circulant preconditioner of a coupled Toeplitz normal operator, on top of
precond_reference.py (the scalar circulant), subspace_reference.py (the coupled operator) and cg_reference.py.

A vector of the block system is a stack of K arrays, shape ``(K,) + N[::-1]``; ``E`` and ``B`` are full ``(K, K) + N[::-1]`` arrays (the library
stores the pairs a <= b only; the rest is the conjugate).  ``F`` is ``numpy.fft.fftn`` over the array indices of a component.
"""
import numpy as np

import precond_reference as P
import subspace_reference as SR
import toeplitz_reference as R

PIVOT_FRACTION = 0.25      # of the shift: the library's kPcPivotFraction


def block_eigenvalues(Ns, spectra, K):
    """``E[a, b] = DFT_N(fold(T_ab))`` from the spectra of the pairs a <= b (2N grid, FFT order, the library's pair order): the fold of
    ``precond_reference.chan_eigenvalues`` is linear and holds for a complex, non-symmetric generating sequence.  The diagonal keeps its real
    part (its imaginary part is round-off) and ``E[b, a] = conj(E[a, b])`` cell by cell."""
    E = np.zeros((K, K) + tuple(reversed(Ns)), dtype=np.complex128)
    for (a, b), T in zip(SR.pairs(K), spectra):
        e = P.chan_eigenvalues(Ns, T)
        if a == b:
            E[a, a] = e.real
        else:
            E[a, b] = e
            E[b, a] = np.conj(e)
    return E


def shift_of(E, mu, floor):
    """``shift = max(μ, floor · s)``, ``s = max_{q,a} E_aa(q) + μ``."""
    K = E.shape[0]
    s = max(float(E[a, a].real.max()) for a in range(K)) + mu
    return max(mu, floor * s)


def block_inverse(E, mu=0.0, floor=1e-6):
    """``B(q) = (E(q) + shift I)⁻¹ / n`` for every cell as the library forms it: Cholesky ``A = L L^H`` with every pivot that is not finite
    or not above ``PIVOT_FRACTION · shift`` floored there, ``X = L⁻¹``, ``A⁻¹ = X^H X``.  Returns ``(B, floored_cells)``."""
    K = E.shape[0]
    n = int(np.prod(E.shape[2:]))
    shift = shift_of(E, mu, floor)
    pf = PIVOT_FRACTION * shift
    L = np.zeros_like(E)
    hit = np.zeros(E.shape[2:], dtype=bool)
    for j in range(K):
        s = E[j, j].real + shift - sum(np.abs(L[j, k]) ** 2 for k in range(j))
        bad = ~(s > pf) | ~np.isfinite(s)
        hit |= bad
        s = np.where(bad, pf, s)
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, K):
            L[i, j] = (E[i, j] - sum(L[i, k] * np.conj(L[j, k]) for k in range(j))) / L[j, j]
    X = np.zeros_like(E)
    for j in range(K):
        X[j, j] = 1.0 / L[j, j]
        for i in range(j + 1, K):
            X[i, j] = -sum(L[i, k] * X[k, j] for k in range(j, i)) / L[i, i]
    B = np.zeros_like(E)
    for a in range(K):
        for b in range(K):
            B[a, b] = sum(np.conj(X[k, a]) * X[k, b] for k in range(max(a, b), K)) / n
    return B, int(hit.sum())


def block_apply(B, d, rs):
    """``(M⁻¹ r)_a = d ⊙ F⁻¹(Σ_b B_ab ⊙ F(d ⊙ r_b))`` with the unnormalised transforms (1/n is in B); ``d = None``: no scaling.  ``rs``: a stack
    (or list) of K arrays; returns the stack."""
    rs = np.asarray(rs).astype(np.complex128)
    K, axes = rs.shape[0], tuple(range(1, rs.ndim))
    v = rs if d is None else d * rs
    V = np.fft.fftn(v, axes=axes)
    Y = np.stack([sum(B[a, b] * V[b] for b in range(K)) for a in range(K)])
    out = np.fft.ifftn(Y, axes=axes) * rs[0].size
    return out if d is None else d * out


def dense_block_inverse(B, d=None):
    """The (K n) × (K n) matrix of ``block_apply`` (a stack flattened component after component)."""
    K, shape = B.shape[0], B.shape[2:]
    n = int(np.prod(shape))
    eye = np.eye(K * n, dtype=np.complex128)
    return np.stack([block_apply(B, d, eye[:, k].reshape((K,) + shape)).ravel() for k in range(K * n)], axis=1)


def spread(E, mu, floor):
    """``(λ_max + shift) / (λ_min + shift)`` of E(q) over all cells: what multiplies the relative error of E in B."""
    lam = np.linalg.eigvalsh(np.moveaxis(E.reshape(E.shape[:2] + (-1,)), -1, 0))
    shift = shift_of(E, mu, floor)
    return float((lam.max() + shift) / (lam.min() + shift))


def subspace_basis(K, Np, seed, nt=32):
    """The basis of the tests: ``t = 0 … nt − 1``, ``D[:, i] = exp(−t / T2_i)`` for 64 values of T2 linearly spaced in [3, 40], U = the first K
    left singular vectors of D with ``U[t, a] *= exp(0.3 i t a)``, ``t_j`` uniform integers from ``default_rng(seed + 1)``,
    ``φ = √nt · U[t_j].T`` (shape (K, Np))."""
    t = np.arange(nt, dtype=np.float64)
    D = np.exp(-t[:, None] / np.linspace(3.0, 40.0, 64)[None, :])
    U = np.linalg.svd(D, full_matrices=False)[0][:, :K].astype(np.complex128)
    U = U * np.exp(0.3j * t[:, None] * np.arange(K)[None, :])
    tj = np.random.default_rng(seed + 1).integers(0, nt, Np)
    return np.sqrt(nt) * U[tj].T


def separable_spectra(Ns, xs, w, phi):
    """``subspace_reference.exact_spectra`` through ``precond_reference.exact_spectrum_separable``: the same direct sums, fast enough for
    tens of thousands of points."""
    phi = np.atleast_2d(phi)
    return [P.exact_spectrum_separable(Ns, xs, SR.pair_weights(w, phi, a, b)) for a, b in SR.pairs(phi.shape[0])]


def modulated_poisson_spectra(Ns, K, seed, terms=3, gamma=0.5):
    """An analytic Hermitian positive definite family, asymmetric in q:

        T_ab[d] = δ_ab Π_dim 0.2^|d| + Σ_p γ conj(c_pa) c_pb Π_dim a_p^|d| exp(i θ_p · d),   c_p random complex, a_p in [0.1, 0.3], θ_p in [0, 2π)^D.

    Every term is (a positive semi-definite K × K matrix) ⊗ (a Toeplitz matrix whose symbol, a shifted Poisson kernel, is positive)."""
    rng = np.random.default_rng(seed)
    D = len(Ns)
    shape = [2 * n for n in reversed(Ns)]
    ds = []
    for dim, n in enumerate(Ns):
        s = [1] * D
        s[D - 1 - dim] = 2 * n
        ds.append(np.asarray(R.modes(2 * n)).astype(np.float64).reshape(s))

    def kernel(a, theta):
        out = np.ones(shape, dtype=np.complex128)
        for dim in range(D):
            out = out * (a ** np.abs(ds[dim])) * np.exp(1j * theta[dim] * ds[dim])
        return out

    base = kernel(0.2, np.zeros(D))
    c = (rng.standard_normal((terms, K)) + 1j * rng.standard_normal((terms, K))) / np.sqrt(2)
    kern = [kernel(0.1 + 0.2 * rng.random(), rng.random(D) * 2 * np.pi) for _ in range(terms)]
    out = []
    for a, b in SR.pairs(K):
        T = base.copy() if a == b else np.zeros(shape, dtype=np.complex128)
        for p in range(terms):
            T = T + gamma * np.conj(c[p, a]) * c[p, b] * kern[p]
        out.append(T)
    return out
