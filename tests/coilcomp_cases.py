"""Data, cases and cached numpy references shared by the tests of coil compression.  No GPU import.

Data of a case ``(C, n)`` have a designed spectrum:  Y = Q diag(ρ^{k/2}) Xᵀ  with Q a random unitary C × C matrix and X an n × r matrix
with orthonormal columns (both from a QR of complex standard normals of ``default_rng(C · 100003 + n)``, r = min(C, n)), so that
R = Y Yᴴ = Q diag(ρ^k) Qᴴ: neighbouring eigenvalues are a factor 1/ρ apart, and the eigenvectors that are compared are well defined.
A whitened case multiplies Y by the Cholesky factor of its Ψ, so that the WHITENED Gram matrix has the designed spectrum.
"""
import numpy as np

import coilcomp_reference as CR
from fista_cases import dt  # noqa: F401
from llr_reference import jacobi_eigh

# (C, n) -> ρ: see the table of DESIGN.md §29
RHO = {(1, 9): 0.5, (2, 1): 0.5, (2, 9): 0.5, (3, 35): 0.5, (8, 210): 0.6, (17, 9): 0.7, (17, 210): 0.7, (32, 1000): 0.8,
       (33, 1000): 0.8, (64, 1000): 0.85, (32, 40000): 0.8}
CASES = [(1, 9), (2, 1), (2, 9), (3, 35), (8, 210), (17, 9), (17, 210), (32, 1000), (33, 1000), (64, 1000)]
BIG = (32, 40000)                     # more than one tile per workgroup; the GPU test picks the exact length from the layout
NOISE_CASES = [(8, 210), (33, 1000)]  # with a correlated-noise Ψ of condition number 50
PSI_COND = 50.0
MIN_RATIO = 1.15                      # between neighbouring eigenvalues among the rows compared

# The largest row difference up to a phase (relative to the row's length) and the largest eigenvalue difference over λ_max of
# compression_matrix(eigh=jacobi_eigh) against compression_matrix(eigh=np.linalg.eigh) on the reference's own Gram matrix, in units of
# ε = 2^-52, rounded up: printed and checked by test_coilcomp_host.py::test_reference_against_itself.  For the whitened cases the figure
# also covers the two orders of the products in W R Wᴴ, (W R) Wᴴ against W (R Wᴴ), under LAPACK.  The bars of the GPU tests are
# max(16, 4 x the first figure) ε on the rows and max(64, 4 x the second) ε λ_max on the eigenvalues.
SELF_EPS = {
    (1, 9, False): (0.0, 0.0), (2, 1, False): (0.5, 1.5), (2, 9, False): (2.0, 2.0), (3, 35, False): (4.5, 2.5), (8, 210, False): (6.5, 1.5),
    (17, 9, False): (3.0, 9.0), (17, 210, False): (18.0, 15.0), (32, 1000, False): (26.0, 15.0), (33, 1000, False): (49.5, 20.5),
    (64, 1000, False): (66.0, 62.5), (8, 210, True): (7.5, 2.0), (33, 1000, True): (50.5, 23.5),
}
# ‖A Aᴴ − I‖_max (‖A Ψ Aᴴ − I‖_max for a whitened case) of the reference with jacobi_eigh, in ε, rounded up
SELF_ORTHO = {
    (1, 9, False): 0.0, (2, 1, False): 1.5, (2, 9, False): 1.5, (3, 35, False): 1.0, (8, 210, False): 2.5, (17, 9, False): 7.0,
    (17, 210, False): 4.0, (32, 1000, False): 5.0, (33, 1000, False): 6.0, (64, 1000, False): 8.0, (8, 210, True): 3.5, (33, 1000, True): 6.5,
}


def rows_compared(C, n):
    """The first min(⌈C/2⌉, 16) virtual coils; a rank-deficient case (n < C) compares the first row only."""
    return 1 if n < C else min((C + 1) // 2, 16)


_DATA, _PSI, _REFERENCES = {}, {}, {}


def psi(C):
    """A correlated-noise covariance of condition number PSI_COND: P diag(geometric 1 ... 1/50) Pᴴ, P random unitary."""
    if C not in _PSI:
        rng = np.random.default_rng(7000 + C)
        P, _ = np.linalg.qr(rng.standard_normal((C, C)) + 1j * rng.standard_normal((C, C)))
        d = PSI_COND ** (-np.arange(C) / max(C - 1, 1))
        m = (P * d[None, :]) @ P.conj().T
        m = (m + m.conj().T) / 2
        m.setflags(write=False)
        _PSI[C] = m
    return _PSI[C]


def data(C, n, rho=None, noise=False):
    """[C, n] complex128, never modified."""
    rho = RHO[(C, n)] if rho is None else rho
    key = (C, n, rho, noise)
    if key not in _DATA:
        rng = np.random.default_rng(C * 100003 + n)
        r = min(C, n)
        Q, _ = np.linalg.qr(rng.standard_normal((C, C)) + 1j * rng.standard_normal((C, C)))
        X, _ = np.linalg.qr(rng.standard_normal((n, r)) + 1j * rng.standard_normal((n, r)))
        y = (Q[:, :r] * (rho ** (np.arange(r) / 2.0))[None, :]) @ X.T
        if noise:
            y = np.linalg.cholesky(psi(C)) @ y
        y = np.ascontiguousarray(y)
        y.setflags(write=False)
        _DATA[key] = y
    return _DATA[key]


def weights(n, seed=0):
    """Non-negative weights in [0, 1] of which about a quarter are exact zeros."""
    rng = np.random.default_rng(9000 + seed + n)
    h = rng.random(n)
    h[rng.random(n) < 0.25] = 0.0
    return h


def reference(C, n, Z="c128", noise=False, jacobi=False):
    """(A, λ, R, info) of the data rounded to the element type of Z; cached and never modified."""
    key = (C, n, Z, noise, jacobi)
    if key not in _REFERENCES:
        R = CR.gram(data(C, n, noise=noise).astype(dt(Z)[1]))
        info = {}
        A, lam = CR.compression_matrix(R, psi(C) if noise else None, eigh=jacobi_eigh if jacobi else np.linalg.eigh, info=info)
        for v in (A, lam, R):
            v.setflags(write=False)
        _REFERENCES[key] = (A, lam, R, info)
    return _REFERENCES[key]


def separation(lam, rows, rank):
    """The smallest ratio between neighbouring eigenvalues among the first ``rows`` and the one behind them, within the rank."""
    lam = np.asarray(lam)
    upto = min(rows + 1, rank)
    return float(np.min(lam[:upto - 1] / lam[1:upto])) if upto > 1 else np.inf


def bars(C, n, noise=False):
    """(rows, eigenvalues, orthogonality) bars in ε."""
    rows, eig = SELF_EPS[(C, n, noise)]
    return max(16.0, 4.0 * rows), max(64.0, 4.0 * eig), max(64.0, 4.0 * SELF_ORTHO[(C, n, noise)])
