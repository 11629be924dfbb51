"""Field maps, cases and cached numpy references shared by the tests of off-resonance correction.  No GPU import."""
import functools

import numpy as np

import field_reference as F
import subspace_reference as S

NP = 2000
QUALITY_SEGMENTS = (2, 4, 8)
NBINS, RIDGE = 256, 1e-8


def smooth_field(shape, span):
    """A smooth 2-D field map with max − min = span exactly: a tilt with one slow wave.  Its histogram is close to flat (244 of 256
    bins occupied on 32 × 32, none with more than 10 counts), so the fit, which weights the bins by their counts, controls the error at
    every occupied bin and the maximum over them follows the weighted error."""
    ny, nx = shape
    y, x = np.meshgrid(np.linspace(-1, 1, ny), np.linspace(-1, 1, nx), indexing="ij")
    f = x + 0.5 * y + 0.1 * np.sin(3.0 * x) * np.cos(2.0 * y)
    f = f - f.min()
    return f * (span / f.max())


@functools.lru_cache(maxsize=None)
def quality_case():
    """(ω, the 200 times): (ωmax − ωmin)(t_max − t_min) = 6π with t in [0, 1]."""
    return smooth_field((32, 32), 6 * np.pi), np.linspace(0.0, 1.0, 200)


def bin_error(phi, omega, tau, times, nbins=NBINS, dtype=np.float64):
    """The quality figure: the interpolation error at the centres of the occupied bins of ω (rounded to `dtype` first, as the device sees it)."""
    counts, centres = F.histogram(np.asarray(omega).astype(dtype), nbins)
    return F.interpolation_error(phi, centres[counts > 0], tau, times)


@functools.lru_cache(maxsize=None)
def quality_reference(L, dtype=np.float64):
    """The reference's own error for L segments on the quality case (inputs rounded to `dtype`)."""
    omega, times = quality_case()
    omega, times = omega.astype(dtype), times.astype(dtype)
    tau = F.uniform_tau(L, 0.0, 1.0)
    phi = F.fit(omega, tau, times, NBINS, RIDGE)
    return bin_error(phi, omega, tau, times, dtype=dtype)


class Problem:
    """A segmented operator's inputs: points, weights, L interpolator rows, L random complex factors (not unit modulus: a conj slip
    shows), one image; exact spectra, multipliers and folded products computed on first use."""

    def __init__(self, Ns, L, seed, clustered=False):
        rng = np.random.default_rng(seed)
        self.Ns, self.L, self.shape = Ns, L, Ns[::-1]
        if clustered:
            self.xs = [np.mod(np.pi + 0.3 * rng.standard_normal(NP), 2 * np.pi) for _ in Ns]
        else:
            self.xs = [rng.random(NP) * 2 * np.pi for _ in Ns]
        self.w = rng.random(NP) + 0.1
        self.phi = (rng.standard_normal((L, NP)) + 1j * rng.standard_normal((L, NP))) / np.sqrt(2 * L)
        self.B = (rng.standard_normal((L,) + self.shape) + 1j * rng.standard_normal((L,) + self.shape)) * 0.6 + 0.5
        self.u = rng.standard_normal(self.shape) + 1j * rng.standard_normal(self.shape)
        m = rng.standard_normal((3,) + self.shape) + 1j * rng.standard_normal((3,) + self.shape)
        self.maps = m / np.sqrt((np.abs(m) ** 2).sum(axis=0))
        self._spectra, self._mult = None, None

    @property
    def spectra(self):
        if self._spectra is None:
            self._spectra = S.exact_spectra(self.Ns, self.xs, self.w, self.phi)
        return self._spectra

    @property
    def multipliers(self):
        if self._mult is None:
            self._mult = S.multipliers(self.Ns, self.spectra)
        return self._mult


_PROBLEMS = {}


def problem(Ns, L, clustered=False):
    key = (Ns, L, clustered)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = Problem(Ns, L, seed=7 * sum(Ns) + L, clustered=clustered)
    return _PROBLEMS[key]


@functools.lru_cache(maxsize=None)
def recovery_case():
    """32 × 32, 3000 samples on a spiral that winds out of the centre of k-space while t runs over [0, 1], a smooth ω of range 6π and a
    piecewise smooth image.  Returns a dict with the exact model's data and the numpy reconstructions (direct solves of the regularised
    normal equations, λ = 1e-3 λmax): `err_ref` with L = 8 segments, `err_plain` without correction."""
    Ns, Np, L = (32, 32), 3000, 8
    t = (np.arange(Np) + 0.5) / Np
    r, ang = 1.25 * np.pi * np.sqrt(t), 2 * np.pi * 20 * np.sqrt(t)
    xs = [np.mod(r * np.cos(ang), 2 * np.pi), np.mod(r * np.sin(ang), 2 * np.pi)]
    omega = smooth_field((32, 32), 6 * np.pi)
    y, x = np.meshgrid(np.linspace(-1, 1, 32), np.linspace(-1, 1, 32), indexing="ij")
    u = (np.exp(-3 * (x * x + y * y)) + 0.7 * ((x - 0.2) ** 2 + (y + 0.1) ** 2 < 0.2) * np.exp(1j * (0.5 * x - 0.3 * y))).astype(np.complex128)
    Fm = F.fourier_matrix(Ns, xs)
    data = F.exact_matrix(Fm, omega, t) @ u.ravel()
    tau = F.uniform_tau(L, 0.0, 1.0)
    phi = F.fit(omega, tau, t, NBINS, RIDGE)
    B = F.factors(omega, tau)
    A = F.segmented_matrix(Fm, phi, B)

    def solve(M):
        G = M.conj().T @ M
        lmax = float(np.linalg.eigvalsh(G)[-1])
        xhat = np.linalg.solve(G + 1e-3 * lmax * np.eye(G.shape[0]), M.conj().T @ data)
        return xhat.reshape(u.shape), lmax

    x_seg, lmax_seg = solve(A)
    x_plain, lmax_plain = solve(Fm)
    rel = lambda a: float(np.linalg.norm(a - u) / np.linalg.norm(u))
    return dict(Ns=Ns, Np=Np, L=L, xs=xs, times=t, omega=omega, u=u, data=data, tau=tau, err_ref=rel(x_seg), err_plain=rel(x_plain),
                lmax_seg=lmax_seg, lmax_plain=lmax_plain)
