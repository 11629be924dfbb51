"""numpy reference of off-resonance correction by time segmentation, complex128 / float64 throughout.  No GPU import.

    exp(−i ω t) ≈ Σ_l φ_l(t) exp(−i ω τ_l),     B_l = exp(−i ω τ_l)
    G_ω u = Σ_c conj(S_c) Σ_a conj(B_a) Σ_b Toeplitz(T_ab) (B_b S_c u),     T_ab from w conj(φ_a) φ_b

The fit is the histogram least-squares fit of Sutton, Noll & Fessler (IEEE TMI 2003) with the library's bin rule.  Arrays follow the
oracle's layout (shape ``N[::-1]``, dimension 1 fastest); ω lives on the plan's uniform side, like û.
"""
import numpy as np

import subspace_reference as S
import toeplitz_reference as R


def histogram(omega, nbins, mask=None):
    """(counts uint32, centres float64): bin = min(nbins − 1, (int)((ω − ωmin) · scale)), scale = nbins / (ωmax − ωmin), in float64; one
    bin at the value for a constant ω."""
    w = np.asarray(omega).astype(np.float64).ravel()
    if mask is not None:
        w = w[np.asarray(mask).ravel() != 0]
    lo, hi = w.min(), w.max()
    if hi == lo:
        return np.array([w.size], dtype=np.uint32), np.array([lo])
    scale = nbins / (hi - lo)
    bins = np.minimum(nbins - 1, ((w - lo) * scale).astype(np.int64))
    counts = np.bincount(bins, minlength=nbins).astype(np.uint32)
    centres = lo + (np.arange(nbins) + 0.5) * ((hi - lo) / nbins)
    return counts, centres


def gram(counts, centres, tau):
    """Gm[l, l'] = Σ_b h_b exp(−i ω_b (τ_l' − τ_l))."""
    tau = np.asarray(tau, dtype=np.float64)
    dt = tau[None, :] - tau[:, None]
    return np.einsum("b,blm->lm", counts.astype(np.float64), np.exp(-1j * centres[:, None, None] * dt[None]))


def ridged(G, ridge):
    L = G.shape[0]
    return G + ridge * (np.trace(G).real / L) * np.eye(L)


def solver_matrix(G, ridge):
    return np.linalg.inv(ridged(G, ridge))


def rhs(counts, centres, tau, times):
    """r[l, j] = Σ_b h_b exp(−i ω_b (t_j − τ_l)) by direct sums."""
    tau, t = np.asarray(tau, dtype=np.float64), np.asarray(times).astype(np.float64)
    out = np.empty((tau.size, t.size), dtype=np.complex128)
    h = counts.astype(np.float64)
    for l in range(tau.size):
        out[l] = np.exp(-1j * np.outer(t - tau[l], centres)) @ h
    return out


def interpolators(P, counts, centres, tau, times):
    """φ[l, j] = (P r(t_j))_l."""
    return P @ rhs(counts, centres, tau, times)


def fit(omega, tau, times, nbins=256, ridge=1e-8, mask=None):
    counts, centres = histogram(omega, nbins, mask)
    G = gram(counts, centres, tau)
    return interpolators(solver_matrix(G, ridge), counts, centres, tau, times)


def factors(omega, tau):
    w = np.asarray(omega).astype(np.float64)
    return np.stack([np.exp(-1j * w * t) for t in tau])


def uniform_tau(L, lo, hi):
    return np.array([0.5 * (lo + hi)]) if L == 1 else np.linspace(lo, hi, L)


def interpolation_error(phi, values, tau, times):
    """max over the values ω and the times of |exp(−i ω t) − Σ_l φ_l(t) exp(−i ω τ_l)|."""
    v, t = np.asarray(values, dtype=np.float64), np.asarray(times).astype(np.float64)
    exact = np.exp(-1j * np.outer(v, t))
    approx = np.exp(-1j * np.outer(v, np.asarray(tau))) @ np.asarray(phi).astype(np.complex128)
    return float(np.max(np.abs(exact - approx)))


def folded_gram(Ns, xs, w, phi, B, u, maps=None, fftshift=False):
    """The folded exact product by direct sums (subspace_reference.exact_block_gram): inputs B_b S_c u, outputs folded by conj(B_a), conj(S_c)."""
    B = [np.asarray(b).astype(np.complex128) for b in B]
    out = np.zeros(np.asarray(u).shape, dtype=np.complex128)
    for Sc in ([None] if maps is None else list(maps)):
        v = np.asarray(u).astype(np.complex128) if Sc is None else np.asarray(Sc).astype(np.complex128) * u
        g = S.exact_block_gram(Ns, xs, w, phi, [b * v for b in B], fftshift)
        f = sum(np.conj(b) * ga for b, ga in zip(B, g))
        out += f if Sc is None else np.conj(Sc) * f
    return out


def folded_apply(Ns, Ks, B, u, maps=None, fftshift=False):
    """The same operator through the block multipliers (subspace_reference.block_apply): fast enough for a CG reference."""
    B = [np.asarray(b).astype(np.complex128) for b in B]
    out = np.zeros(np.asarray(u).shape, dtype=np.complex128)
    for Sc in ([None] if maps is None else list(maps)):
        v = np.asarray(u).astype(np.complex128) if Sc is None else np.asarray(Sc).astype(np.complex128) * u
        g = S.block_apply(Ns, Ks, [b * v for b in B], fftshift)
        f = sum(np.conj(b) * ga for b, ga in zip(B, g))
        out += f if Sc is None else np.conj(Sc) * f
    return out


def fourier_matrix(Ns, xs, fftshift=False):
    """F[j, k] = exp(+i k·x_j), the columns flattened like an array of shape N[::-1]: the plan's type 2 as a matrix."""
    ks = R.mode_lists(Ns, fftshift)
    grids = np.meshgrid(*[ks[d] for d in reversed(range(len(Ns)))], indexing="ij")
    phase = sum(np.outer(np.asarray(xs[d], dtype=np.float64), grids[len(Ns) - 1 - d].ravel()) for d in range(len(Ns)))
    return np.exp(1j * phase)


def segmented_matrix(F, phi, B):
    """A_seg = Σ_l diag(φ_l) F diag(B_l)."""
    return sum(np.asarray(phi[l])[:, None] * F * np.asarray(B[l]).ravel()[None, :] for l in range(len(B)))


def exact_matrix(F, omega, times):
    """The exact off-resonance model: E[j, k] = exp(−i ω_k t_j) F[j, k]."""
    return F * np.exp(-1j * np.outer(np.asarray(times).astype(np.float64), np.asarray(omega).astype(np.float64).ravel()))
