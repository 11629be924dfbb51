"""Coil images, cases and cached numpy references shared by the tests of the coil map estimate.  No GPU import.

Images of a case ``(Ns, C, box)``, stacked ``[C, *Ns[::-1]]``:  a_c = S_c ρ + 0.05 (complex standard normal), with
S = sense_reference.smooth_maps(C, shape, seed=0, zero_region=False), ρ = 1 + 0.5 cos(2π x_1 / N_1) exp(2πi x_D / N_D) on 0-based cell
indices, and the noise (re + i im) / sqrt(2) of ``default_rng(0)``, real parts drawn first.
"""
import numpy as np

import maps_reference as M
import sense_reference as SR
from fista_cases import dt  # noqa: F401

# (Ns, C, box): see the table of DESIGN.md §28
CASES = [
    ((9,), 3, (3,)),                     # D = 1
    ((7, 5), 2, (3, 3)),                 # the halo wraps in every tile
    ((7, 5), 3, (7, 5)),                 # box = whole array: every cell has the same R
    ((32, 40), 4, (5, 5)),
    ((32, 40), 8, (7, 3)),               # anisotropic box
    ((32, 40), 1, (3, 3)),               # one coil: the maps are phases only
    ((32, 40), 4, (1, 1)),               # box 1: R has rank 1, λ2 = 0
    ((5, 6, 7), 8, (3, 3, 3)),           # D = 3, no side a multiple of a tile
    ((12, 10), 16, (5, 5)),
    ((12, 10), 17, (3, 3)),              # wide team
    ((12, 10), 32, (3, 3)),              # wide team
    ((32, 32, 32), 2, (3, 3, 3)),        # many workgroups
    ((16, 16, 16), 4, (5, 5, 5)),
    ((20, 12, 9), 3, (9, 1, 3)),         # the largest side, a side of 1, and b_3 = 9 = N_3
]
# beyond the issue's table: a tile with its halo does not fit into LDS, the kernel reads the neighbours from global memory
GLOBAL_CASES = [((9, 9, 9), 16, (9, 9, 9))]
PCA_CASE = ((32, 40), 4, (5, 5))         # the reference's |s| with the PCA vector is >= 0.05 at every cell (asserted by the host test)

# The largest per-cell ‖v − v'‖₂ and relative λ1 difference of walsh(eigh=jacobi_eigh) against walsh(eigh=np.linalg.eigh), in units of
# ε = 2^-52, over EVERY cell of the case, rounded up: printed and checked by test_maps_host.py::test_reference_against_itself.  The bar of
# the GPU tests is max(16, 4 x the first figure).
SELF_EPS = {
    ((9,), 3, (3,)): (2.5, 5.5), ((7, 5), 2, (3, 3)): (2.0, 2.0), ((7, 5), 3, (7, 5)): (3.5, 2.5), ((32, 40), 4, (5, 5)): (5.0, 12.5),
    ((32, 40), 8, (7, 3)): (5.0, 17.0), ((32, 40), 1, (3, 3)): (0.0, 0.0), ((32, 40), 4, (1, 1)): (4.0, 6.0), ((5, 6, 7), 8, (3, 3, 3)): (6.0, 16.0),
    ((12, 10), 16, (5, 5)): (6.0, 27.5), ((12, 10), 17, (3, 3)): (7.0, 24.0), ((12, 10), 32, (3, 3)): (7.5, 34.5),
    ((32, 32, 32), 2, (3, 3, 3)): (3.5, 4.5), ((16, 16, 16), 4, (5, 5, 5)): (5.0, 12.0), ((20, 12, 9), 3, (9, 1, 3)): (4.0, 7.0),
    ((9, 9, 9), 16, (9, 9, 9)): (4.0, 10.5),
}


def truth(Ns, C):
    """(S [C, ...], ρ [...])"""
    shape = Ns[::-1]
    S = SR.smooth_maps(C, shape, seed=0, zero_region=False)
    idx = np.indices(shape)
    x1, xD = idx[-1], idx[0]
    rho = 1.0 + 0.5 * np.cos(2.0 * np.pi * x1 / Ns[0]) * np.exp(2j * np.pi * xD / Ns[-1])
    return S, rho


_IMAGES, _REFERENCES = {}, {}


def images(Ns, C):
    if (Ns, C) not in _IMAGES:
        S, rho = truth(Ns, C)
        rng = np.random.default_rng(0)
        noise = (rng.standard_normal(S.shape) + 1j * rng.standard_normal(S.shape)) / np.sqrt(2.0)
        a = S * rho + 0.05 * noise
        a.setflags(write=False)
        _IMAGES[(Ns, C)] = a
    return _IMAGES[(Ns, C)]


def reference(Ns, C, box, Z="c128", phase=None):
    """walsh(eigh=np.linalg.eigh) on the images rounded to the element type of Z, in float64; cached and never modified.  Returns
    (maps, λ1, λ2, info)."""
    key = (Ns, C, box, Z, None if phase is None else tuple(np.asarray(phase).tolist()))
    if key not in _REFERENCES:
        info = {}
        out = M.walsh(images(Ns, C).astype(dt(Z)[1]), box, phase_ref=phase, info=info)
        for v in out:
            v.setflags(write=False)
        _REFERENCES[key] = out + (info,)
    return _REFERENCES[key]


def bar(Ns, C, box):
    return max(16.0, 4.0 * SELF_EPS[(Ns, C, box)][0])


def crop_for(lam1):
    """crop with crop² max λ1 at the geometric mean of two adjacent sorted λ1 values near the median whose ratio is >= 1 + 1e-3."""
    s = np.sort(np.asarray(lam1, dtype=np.float64).ravel())
    mid = len(s) // 2
    for off in sorted(range(-mid, len(s) - mid - 1), key=abs):
        lo, hi = s[mid + off], s[mid + off + 1]
        if lo > 0 and hi / lo >= 1.0 + 1e-3:
            return float(np.sqrt(np.sqrt(lo * hi) / s[-1]))
    raise AssertionError("no gap of 1e-3 between adjacent eigenvalues")


def per_cell(got, want):
    """The largest ‖got(x) − want(x)‖₂ over the cells."""
    d = np.asarray(got).astype(np.complex128) - np.asarray(want).astype(np.complex128)
    return float(np.sqrt((np.abs(d) ** 2).sum(axis=0)).max())
