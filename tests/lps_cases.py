"""Systems, weights and cached numpy references shared by the tests of the low-rank plus sparse solver.  No GPU import.

Systems of K <= 16 frames are those of tvt_cases.py (``frames(Ns, K)``: analytic spectra, ``a = 0.15 + 0.05 c`` for frame c, handed to
the operator with ``set_spectra_frames``).  For K > 16 the frames here use ``a = 0.15 + 0.05 (c mod 9)``: the analytic spectrum divides
by zero at a = 1.

The truth is rank 2 with a dominant first component, plus a term whose temporal DFT has 15 % non-zero coefficients, plus 5 % noise; the
right-hand side is b = G x.  The weights are ``nuc = f_L σ_max(C(b))`` and ``l1 = f_S max|T b|``.  The pairs (f_L, f_S) are fixed in
FRACTIONS so that in the reference's tenth iteration (float64, step = 1 / (2 · 1.05 λmax), momentum on and off) the number of zeroed
singular values lies strictly between 0 and K and the share of zeroed temporal coefficients in [0.2, 0.95]; the tests assert both.
"""
import numpy as np

import fista_cases as FC
import lps_reference as P
import tvt_cases as TC

dt = FC.dt


class WideFrames(TC.Frames):
    """More than 16 frames: the multipliers repeat with period 9."""

    def __init__(self, Ns, K):
        self.Ns, self.K, self.shape = Ns, K, (K,) + Ns[::-1]
        self.frames = [FC.Analytic(Ns, a=0.15 + 0.05 * (c % 9), seed=100 * sum(Ns) + c, nrhs=1) for c in range(K)]
        self.b = np.stack([f.bs[0] for f in self.frames])
        self.lmax = max(f.lmax for f in self.frames)
        self.spectra = [f.spec for f in self.frames]


_FRAMES = {}


def frames(Ns, K, shared=False):
    if K <= 16:
        return TC.frames(Ns, K, shared)
    assert not shared
    if (Ns, K) not in _FRAMES:
        _FRAMES[(Ns, K)] = WideFrames(Ns, K)
    return _FRAMES[(Ns, K)]


def truth(Ns, K):
    """[K, ...] in float64: rank 2 (second component at 0.3), a temporally sparse term at 0.5 and 5 % noise, relative to unit rms."""
    rng = np.random.default_rng(7 * sum(Ns) + K)
    shape, n = (K,) + Ns[::-1], int(np.prod(Ns))
    cplx = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2.0)      # noqa: E731
    low = np.outer(cplx(K), cplx(n)) + 0.3 * np.outer(cplx(K), cplx(n))
    coef = cplx(K, n) * (rng.random((K, n)) < 0.15)
    sparse = 0.5 * P.tdft(coef, "dft", inverse=True) / np.sqrt(0.15)
    return (low + sparse + 0.05 * cplx(K, n)).reshape(shape)


# (Ns, K, path the operator must take or None): the solver's systems, and those of the operator tests
SOLVER_CASES = [((9,), 9, None), ((7, 5), 3, None), ((32, 40), 3, "fused"), ((5, 6, 7), 9, None), ((32, 32, 32), 2, "fused"), ((12, 10), 17, None)]
PATHS = {(Ns, K): path for Ns, K, path in SOLVER_CASES}
MAP_CASES = [((9,), 9), ((7, 5), 3), ((32, 40), 3), ((32, 40), 8), ((5, 6, 7), 9), ((12, 10), 17), ((12, 10), 32), ((32, 32, 32), 2), ((7, 5), 1)]
HOST_CASES = MAP_CASES[:-1] + [((16, 16, 8), 5)]

# (f_L, f_S) per (Ns, K), the same for both transforms.  Tenth iteration of the float64 reference, momentum on | off: zeroed singular values, zeroed
# coefficient share -- in the comments.
DEFAULT_FRACTIONS = (0.1, 0.1)
FRACTIONS = {                          # "dft" on | off;  "identity" on | off                     with (0.1, 0.1)
    ((9,), 9): (0.1, 0.2),              # 5/9 0.88 | 5/9 0.78;  5/9 0.73 | 5/9 0.48                identity: 6/9 0.16 | 5/9 0.10
    ((7, 5), 3): (0.2, 0.1),            # 1/3 0.49 | 1/3 0.36;  2/3 0.25 | 1/3 0.21                0/3 zeroed singular values
    ((32, 40), 3): (0.2, 0.1),          # 2/3 0.52 | 2/3 0.40;  2/3 0.47 | 2/3 0.32                0/3 zeroed singular values
    ((5, 6, 7), 9): (0.1, 0.2),         # 3/9 0.54 | 3/9 0.49;  3/9 0.56 | 3/9 0.50                3/9 0.20 | 3/9 0.17
    ((32, 32, 32), 2): (0.5, 0.1),      # 1/2 0.47 | 1/2 0.47;  1/2 0.40 | 1/2 0.40                0/2 zeroed singular values
    # ((12, 10), 17): the default       # 10/17 0.45 | 10/17 0.37;  10/17 0.33 | 9/17 0.26
}
# svt_gram against svt at the median singular value on HOST_CASES (float64): 2.3 ... 50.8 ε relative L2 in 2 ... 10 sweeps (the worst is
# (12, 10) K = 32, then 27.8 ε at K = 17 and 24.9 ε at (5, 6, 7) K = 9; the figures depend on the seeds above); the tests' bar is 256 ε.


class Case:
    def __init__(self, Ns, K, shared=False):
        self.Ns, self.K, self.s = Ns, K, frames(Ns, K, shared)
        self.apply, self.lmax = self.s.apply, self.s.lmax
        self.b = self.apply(truth(Ns, K))
        self.smax = float(P.singular_values(self.b)[0])

    def step(self, lam=0.0):
        return 1.0 / (2.0 * (1.05 * self.lmax + lam))

    def weights(self, transform):
        f_L, f_S = FRACTIONS.get((self.Ns, self.K), DEFAULT_FRACTIONS)
        return f_L * self.smax, f_S * float(np.abs(P.tdft(self.b, transform)).max())


_CASES, _REFERENCES = {}, {}


def case(Ns, K, shared=False):
    if (Ns, K, shared) not in _CASES:
        _CASES[(Ns, K, shared)] = Case(Ns, K, shared)
    return _CASES[(Ns, K, shared)]


def reference(c, Z, nuc, l1, transform, momentum, lam=0.0, high=False, apply=None, key=None, **kw):
    """lps_reference.lps on the case with the right-hand side rounded to the element type of Z, run in that element type (or, with
    ``high``, in float64 on the same rounded input), cached and never modified.  ``apply`` / ``key``: another operator on the same
    right-hand side, cached under ``key``."""
    k = (c.Ns, c.K, Z, float(nuc), float(l1), transform, bool(momentum), float(lam), high, key, tuple(sorted(kw.items())))
    if k not in _REFERENCES:
        Zc = dt(Z)[1]
        step = kw.pop("step", c.step(lam))
        _REFERENCES[k] = P.lps(apply or c.apply, c.b.astype(Zc), nuc, l1, step, transform=transform, momentum=momentum, lam=lam,
                               dtype=np.complex128 if high else Zc, **kw)
    return _REFERENCES[k]


def rel(a, b):
    a, b = np.asarray(a).astype(np.complex128), np.asarray(b).astype(np.complex128)
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / nb) if nb > 0 else float(np.linalg.norm(a - b))
