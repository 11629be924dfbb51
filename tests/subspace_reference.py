"""numpy restatement of the coupled (subspace) Toeplitz normal operator from direct sums, in the style of
toeplitz_reference.py, and the joint conjugate gradients on it.

    y_j = Σ_a φ_a(j) (A u_a)_j,        (G_Φ u)_a = Σ_b A^H diag(w conj(φ_a) φ_b) A u_b = Σ_b Toeplitz(T_ab) u_b

``phi`` has shape (K, Np); lists over pairs follow the library's order, row-major over a <= b.  Arrays follow the oracle's layout
(shape ``N[::-1]``, dimension 1 fastest); a list of K such arrays is one vector of the block system.
"""
import numpy as np

import cg_reference as CG
import toeplitz_reference as R
from oracle import nufft_oracle as O


def pair_index(a, b, K):
    """idx(a, b) = a K − a (a − 1) / 2 + (b − a), a <= b."""
    assert 0 <= a <= b < K
    return a * K - a * (a - 1) // 2 + (b - a)


def pairs(K):
    """The pairs a <= b in the library's order."""
    return [(a, b) for a in range(K) for b in range(a, K)]


def pair_weights(w, phi, a, b):
    return np.asarray(w) * np.conj(phi[a]) * phi[b]


def exact_spectra(Ns, xs, w, phi):
    """T_ab = Σ_j w_j conj(φ_a(j)) φ_b(j) exp(−i d·x_j) on the mode set of a 2N plan, one per pair a <= b."""
    phi = np.atleast_2d(phi)
    return [R.exact_spectrum(Ns, xs, pair_weights(w, phi, a, b)) for a, b in pairs(phi.shape[0])]


def exact_block_gram(Ns, xs, w, phi, us, fftshift=False):
    """(G_Φ u)_a = nudft_type1(w conj(φ_a) Σ_b φ_b nudft_type2(u_b)) = Σ_b nudft_type1(w conj(φ_a) φ_b nudft_type2(u_b))."""
    phi = np.atleast_2d(phi)
    ks = R.mode_lists(Ns, fftshift)
    y = sum(phi[b] * O.nudft_type2(ks, xs, us[b]) for b in range(phi.shape[0]))
    return [O.nudft_type1(ks, xs, np.asarray(w) * np.conj(phi[a]) * y) for a in range(phi.shape[0])]


def multipliers(Ns, spectra):
    """K_ab = backwardDFT_2N(T_ab with its Nyquist planes zeroed) / Π 2N_d per pair a <= b (complex; real for a = b)."""
    return [R.multiplier(Ns, T) for T in spectra]


def block(Ks, a, b, K):
    """K_ab for any a, b from the stored pairs: the conjugate of the stored pair for a > b."""
    return Ks[pair_index(a, b, K)] if a <= b else np.conj(Ks[pair_index(b, a, K)])


def block_apply(Ns, Ks, us, fftshift=False):
    """Σ_b crop(forwardDFT(K_ab ⊙ backwardDFT(pad(u_b)))): the steps of toeplitz_reference.apply with the K backward transforms shared
    by the block rows (they hold for a complex multiplier as they stand)."""
    K = len(us)
    idx = np.ix_(*[np.mod(np.asarray(R.modes(n, fftshift)).astype(np.int64), 2 * n) for n in reversed(Ns)])
    back = []
    for u in us:
        g = np.zeros([2 * n for n in reversed(Ns)], dtype=np.complex128)
        g[idx] = u
        back.append(np.fft.ifftn(g) * g.size)
    return [np.fft.fftn(sum(block(Ks, a, b, K) * back[b] for b in range(K)))[idx] for a in range(K)]


def dense_block_gram(Ns, spectra, K, fftshift=False):
    """The (K n) × (K n) matrix of G_Φ from the spectra: block (a, b) is T_ab[k − k'], block (b, a) its conjugate transpose."""
    n = int(np.prod(Ns))
    A = np.zeros((K * n, K * n), dtype=np.complex128)
    for (a, b), T in zip(pairs(K), spectra):
        blk = CG.dense_gram(Ns, None, None, fftshift, spectrum=T)
        A[a * n:(a + 1) * n, b * n:(b + 1) * n] = blk
        if a != b:
            A[b * n:(b + 1) * n, a * n:(a + 1) * n] = blk.conj().T
    return A


def brute_force_gram(Ns, xs, w, phi, fftshift=False):
    """E^H W E with E[j, (a, k)] = φ_a(j) exp(+i k·x_j): nothing but the definition of the forward model."""
    phi = np.atleast_2d(phi)
    ks = R.mode_lists(Ns, fftshift)
    grids = np.meshgrid(*[ks[d] for d in reversed(range(len(Ns)))], indexing="ij")      # axis i is dimension D − 1 − i
    phase = sum(np.outer(np.asarray(xs[d], dtype=np.float64), grids[len(Ns) - 1 - d].ravel()) for d in range(len(Ns)))
    F = np.exp(1j * phase)                                                              # (Np, n)
    E = np.concatenate([phi[a][:, None] * F for a in range(phi.shape[0])], axis=1)
    return E.conj().T @ (np.asarray(w)[:, None] * E)


def joint_cg(apply, bs, x0=None, lam=0.0, rtol=1e-6, max_iter=50, dtype=np.complex128):
    """Conjugate gradients on the K components as ONE system: cg_reference.cg on the stacked arrays, whose sums then run over all
    components (one α, one β, one stopping test).  ``apply(list of K arrays)`` returns the list G_Φ p."""
    stacked = lambda p: np.stack(apply([p[a] for a in range(p.shape[0])]))
    return CG.cg(stacked, np.stack(bs), None if x0 is None else np.stack(x0), lam=lam, rtol=rtol, max_iter=max_iter, dtype=dtype)


def matrix_block_apply(A, K, shape):
    """apply(list) for joint_cg from the dense block matrix, in float64."""
    def f(ps):
        v = A @ np.concatenate([np.asarray(p).astype(np.complex128).ravel() for p in ps])
        return [v[a * (v.size // K):(a + 1) * (v.size // K)].reshape(shape) for a in range(K)]
    return f
