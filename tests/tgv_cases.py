"""Systems, weights and cached numpy references shared by the TGV² tests.  No GPU import.

The systems are those of tv_cases.py / fista_cases.py.  The weights are alpha1 = 0.1 · max|b| (tv_cases.tv_weight) and alpha0 a multiple
of it; with alpha0 = 0.5 alpha1 both projections clip a share of the cells in the first ten iterations (the tests assert [0.1, 0.95] on
the reference), with alpha0 = 2 alpha1 the projection of r clips none.
"""
import numpy as np

import tgv_reference as G
import tv_cases as TC

dt, system, step, tv_weight = TC.dt, TC.system, TC.step, TC.tv_weight
SOLVER_CASES, PATHS = TC.SOLVER_CASES, TC.PATHS

_REFERENCES = {}


def reference(Ns, Z, alpha1, alpha0, lam, rhs=0, **kw):
    """tgv_reference.tgvpd on system(Ns) with the right-hand side rounded to the element type of Z, run in that element type, cached and
    never modified."""
    key = (Ns, Z, float(alpha1), float(alpha0), float(lam), rhs, tuple(sorted(kw.items())))
    if key not in _REFERENCES:
        s = system(Ns)
        Zc = dt(Z)[1]
        _REFERENCES[key] = G.tgvpd(s.apply, s.bs[rhs].astype(Zc), alpha1, alpha0, step(s, lam), lam=lam, dtype=Zc, **kw)
    return _REFERENCES[key]
