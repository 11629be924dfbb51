"""numpy reference of coil compression and noise pre-whitening, complex128 throughout.  No GPU import.

    R = Y diag(h) Yᴴ        Ψ = L Lᴴ, W = L⁻¹        R̃ = W R Wᴴ = U Λ Uᴴ        A = Uᴴ W        out = A[:V] Y

with the library's rules: eigenvalues sorted descending (ties: the lower original index first), every eigenvector scaled back to unit
length, its entry of largest modulus (lowest index on a tie) real and positive.
"""
import numpy as np

EPS = 2.0 ** -52


def gram(y, h=None):
    """``y``: [C, n]; ``h``: n non-negative weights or None.  R[c, c'] = Σ_j h_j y_c[j] conj(y_c'[j])."""
    y = np.asarray(y).astype(np.complex128)
    yw = y if h is None else y * np.asarray(h, dtype=np.float64)[None, :]
    R = yw @ y.conj().T
    return (R + R.conj().T) / 2


def whitening_matrix(psi):
    """W = L⁻¹ of Ψ = L Lᴴ (lower triangular)."""
    L = np.linalg.cholesky(np.asarray(psi, dtype=np.complex128))
    return np.linalg.solve(L, np.eye(L.shape[0], dtype=np.complex128))


def whiten(R, W, left_first=True):
    """W R Wᴴ, Hermitian to the bit; the two orders of the products differ by roundoff (the device forms W R first)."""
    T = (W @ R) @ W.conj().T if left_first else W @ (R @ W.conj().T)
    T = (T + T.conj().T) / 2
    T[np.diag_indices_from(T)] = T.diagonal().real
    return T


def fix_vectors(lam, V):
    """The sort, unit-length and phase rules on the columns of V.  Returns (λ descending, U)."""
    lam = np.asarray(lam, dtype=np.float64)
    order = sorted(range(len(lam)), key=lambda k: (-lam[k], k))
    U = np.array(V, dtype=np.complex128)[:, order]
    for v in range(U.shape[1]):
        u = U[:, v]
        m = u.real * u.real + u.imag * u.imag
        u = u / np.sqrt(m.sum())
        k = int(np.argmax(m))                                    # the first index on a tie
        u = u * (np.conj(u[k]) / abs(u[k]))
        u[k] = u[k].real
        U[:, v] = u
    return lam[order], U


def compression_matrix(R, psi=None, eigh=np.linalg.eigh, info=None):
    """(A = Uᴴ W with all C rows, λ descending).  ``eigh``: ``np.linalg.eigh`` or ``llr_reference.jacobi_eigh`` (its sweep count goes
    to ``info["sweeps"]``).  Without Ψ nothing is multiplied: A = Uᴴ to the bit."""
    R = np.asarray(R, dtype=np.complex128)
    W = None if psi is None else whitening_matrix(psi)
    out = eigh(R if W is None else whiten(R, W))
    if info is not None and len(out) > 2:
        info["sweeps"] = out[2]
    lam, U = fix_vectors(out[0], out[1])
    Uh = U.conj().T
    return (Uh if W is None else Uh @ W), lam


def apply(A, x, V=None):
    """out_v = Σ_c A[v, c] x_c for v < V; ``x``: [C, n]."""
    A = np.asarray(A, dtype=np.complex128)
    return A[:V] @ np.asarray(x).astype(np.complex128)


def row_difference(got, want):
    """Per row: min over φ of ‖got − e^{iφ} want‖₂ / ‖want‖₂."""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    s = np.einsum("vc,vc->v", np.conj(want), got)
    ph = np.where(np.abs(s) > 0, s / np.where(np.abs(s) > 0, np.abs(s), 1.0), 1.0)
    return np.linalg.norm(got - ph[:, None] * want, axis=1) / np.linalg.norm(want, axis=1)
