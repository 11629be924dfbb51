"""Inputs, thresholds and cases shared by tests/test_llr_host.py, tests/test_gpu_llr.py and tests/test_gpu_fista_llr.py.  No GPU import.

Inputs are locally low-rank plus noise, ``x_a = α_a u + 0.05 · noise_a`` with u and the noise of unit variance and 0.3 <= |α_a| <= 1:
every block's Casorati matrix then has one large singular value and the others small, so a threshold can zero a controlled share of
them (white noise has no such gap).  The Gram route squares the condition number: its error on the small singular directions is about
(σ_max / σ_small)² ε = (‖α‖ / 0.05)² ε, between 100 ε and 3000 ε here for K = 1 ... 16, on directions that carry 1e-2 ... 1e-3 of the
output's norm.  Larger |α| would measure that conditioning and not the kernel.
"""
import numpy as np

import llr_reference as L

EPS = {"c128": 2.0 ** -52, "c64": 2.0 ** -23}
CTYPE = {"c128": np.complex128, "c64": np.complex64}

# (Ns, K, block): the standalone map's cases.  Blocks that share a wave (B = 4, 8), blocks of one or several per workgroup, a block
# that spans a workgroup with K = 16 (8³: B · K = 8192, the limit), odd K, K > 8, K = 1, and B < K (rank-deficient Gram matrices)
PROX_CASES = [
    ((48, 40), 2, (4, 4)),
    ((48, 40), 4, (8, 8)),
    ((64, 80), 3, (16, 4)),
    ((16, 16, 8), 3, (4, 4, 4)),
    ((16, 16, 8), 2, (2, 2, 2)),
    ((64, 64, 64), 16, (8, 8, 8)),
    ((64, 64, 64), 12, (2, 2, 1)),
    ((48, 40), 1, (4, 4)),
    ((48, 40), 8, (2, 2)),
]

# the solver's coupled systems: (Ns, K, block)
SOLVER_CASES = [((48, 40), 2, (4, 4)), ((48, 40), 4, (8, 8)), ((16, 16, 8), 3, (4, 4, 4)), ((16, 16, 8), 2, (2, 2, 2))]


def low_rank_input(Ns, K, seed=0):
    """[K, *Ns[::-1]] complex128."""
    rng = np.random.default_rng(1000 * seed + 7 * sum(Ns) + K)
    shape = Ns[::-1]
    u = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)
    alpha = rng.uniform(0.3, 1.0, K) * np.exp(2j * np.pi * rng.random(K))
    noise = (rng.standard_normal((K,) + shape) + 1j * rng.standard_normal((K,) + shape)) / np.sqrt(2)
    return alpha.reshape((K,) + (1,) * len(Ns)) * u[None] + 0.05 * noise


def median_threshold(x, block, shift=None):
    """The median of all block singular values: the reference zeroes about half of them."""
    return float(np.median(L.block_singular_values(x, block, shift)))


def rel(a, b):
    a, b = np.asarray(a).astype(np.complex128), np.asarray(b).astype(np.complex128)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
