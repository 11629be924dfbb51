"""numpy restatement of the multi-coil (SENSE) normal operator

    G_S û = Σ_c conj(S_c) ⊙ G (S_c ⊙ û),        G = A^H W A  (toeplitz_reference.py),

with the exact Gram product from the oracle's direct sums, its dense matrix, and the test maps.

Arrays follow the oracle's layout: reversed axes, dimension 1 fastest (shape ``N[::-1]``); maps have shape ``(ncoils, *N[::-1])``.
"""
import numpy as np

import cg_reference as CG
import toeplitz_reference as R


def exact_sense_gram(Ns, xs, w, maps, u, fftshift=False):
    """Σ_c conj(S_c) · exact_gram(S_c · u): the answer every route is compared with."""
    out = np.zeros(np.shape(u), dtype=np.complex128)
    for S in maps:
        out += np.conj(S) * R.exact_gram(Ns, xs, w, S * u, fftshift)
    return out


def toeplitz_sense_gram(Ns, K, maps, u, fftshift=False):
    """The same through the FFT form of G: Σ_c conj(S_c) · R.apply(K, S_c · u)."""
    out = np.zeros(np.shape(u), dtype=np.complex128)
    for S in maps:
        out += np.conj(S) * R.apply(Ns, K, S * u, fftshift)
    return out


def dense_sense_gram(G, maps):
    """The matrix of G_S from the dense matrix of G (cg_reference.dense_gram): Σ_c diag(conj s_c) G diag(s_c), for n <= 2048 unknowns."""
    n = G.shape[0]
    assert n <= 2048, n
    out = np.zeros_like(G, dtype=np.complex128)
    for S in maps:
        s = np.asarray(S, dtype=np.complex128).ravel()
        out += np.conj(s)[:, None] * G * s[None, :]
    return out


def normalise(maps):
    """maps / sqrt(Σ_c |S_c|²): afterwards Σ_c |S_c|² = 1 at every cell (cells where every coil is zero are left as they are)."""
    maps = np.asarray(maps)
    rss = np.sqrt(np.sum(np.abs(maps) ** 2, axis=0))
    return maps / np.where(rss > 0, rss, 1.0)


def smooth_maps(ncoils, shape, seed=0, zero_region=True):
    """Smooth random complex fields of magnitude about 1: 1 + a few low-order Fourier modes per coil with random complex amplitudes.
    With ``zero_region`` the last coil is exactly zero on a corner block of the array (a coil that does not see part of the object)."""
    rng = np.random.default_rng(seed)
    axes = np.meshgrid(*[np.arange(n) / n for n in shape], indexing="ij")
    maps = np.empty((ncoils,) + tuple(shape), dtype=np.complex128)
    for c in range(ncoils):
        f = np.full(shape, np.exp(2j * np.pi * rng.random()), dtype=np.complex128)
        for _ in range(3):
            k = rng.integers(-1, 2, size=len(shape))
            phase = sum(kk * ax for kk, ax in zip(k, axes))
            f = f + 0.25 * (rng.standard_normal() + 1j * rng.standard_normal()) * np.exp(2j * np.pi * phase)
        maps[c] = f
    if zero_region:
        maps[(ncoils - 1,) + tuple(slice(0, max(1, n // 3)) for n in shape)] = 0.0
    return maps


__all__ = ["exact_sense_gram", "toeplitz_sense_gram", "dense_sense_gram", "normalise", "smooth_maps", "CG", "R"]
