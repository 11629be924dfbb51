"""Systems, weights and cached numpy references shared by the total-variation tests.  No GPU import.

The systems are those of fista_cases.py (``system(Ns)``, ``step``, the paths of ``SOLVER_CASES``): point sets whose dense matrix exists
and analytic spectra, both given to the operator as an exact spectrum.  The weight is tv = 0.1 · max|b|; on the CPU that clips 0.63 –
0.82 of the dual vectors, averaged over the first ten iterations (the tests assert [0.2, 0.95] on the reference).
"""
import numpy as np

import fista_cases as FC
import tv_reference as T

dt, system, step = FC.dt, FC.system, FC.step
SOLVER_CASES = [(Ns, path) for Ns, _, path in FC.SOLVER_CASES]
PATHS = FC.PATHS
TV_FRACTION = 0.1


def tv_weight(b):
    return TV_FRACTION * float(np.abs(np.asarray(b)).max())


_REFERENCES = {}


def reference(Ns, Z, tv, lam, rhs=0, high=False, **kw):
    """tv_reference.tvpd on system(Ns) with the right-hand side rounded to the element type of Z, run in that element type (or, with
    ``high``, in float64 on the same rounded input), cached and never modified."""
    key = (Ns, Z, float(tv), float(lam), rhs, high, tuple(sorted(kw.items())))
    if key not in _REFERENCES:
        s = system(Ns)
        Zc = dt(Z)[1]
        b = s.bs[rhs].astype(Zc)
        _REFERENCES[key] = T.tvpd(s.apply, b, tv, step(s, lam), lam=lam, dtype=np.complex128 if high else Zc, **kw)
    return _REFERENCES[key]
