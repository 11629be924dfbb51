"""Systems, weights and cached numpy references shared by the tests of the framed operator and of temporal total variation.  No GPU
import.

A system of K frames on the box Ns is K analytic spectra of fista_cases.py, ``Analytic(Ns, a = 0.15 + 0.05 c)`` for frame c: a different
multiplier per frame, handed to the operator with ``set_spectra_frames``, so the only error in G is the library's.

The weights are fractions of max|b|, fixed here on the CPU so that in the reference's tenth iteration the share of live dual cells the
projection shortens lies in [0.2, 0.95] for the temporal duals and, where the spatial term is on, for the spatial ones (the tests assert
it).  0.1 / 0.1 does that for most cases; the exceptions are listed in FRACTIONS with the shares measured for them.
"""
import numpy as np

import fista_cases as FC
import tvt_reference as TT

dt = FC.dt


class Frames:
    def __init__(self, Ns, K, a=None):
        self.Ns, self.K, self.shape = Ns, K, (K,) + Ns[::-1]
        a = [0.15 + 0.05 * c for c in range(K)] if a is None else [a] * K
        self.frames = [FC.Analytic(Ns, a=a[c], seed=100 * sum(Ns) + c, nrhs=1) for c in range(K)]
        self.b = np.stack([f.bs[0] for f in self.frames])
        self.lmax = max(f.lmax for f in self.frames)                              # an upper bound
        self.spectra = [f.spec for f in self.frames]

    def apply(self, x):
        return np.stack([f.apply(x[c]) for c, f in enumerate(self.frames)])

    def step(self, lam=0.0):
        return 1.0 / (1.05 * self.lmax + lam)

    def operator(self, nufft, Z, path=None, framed=True, **kw):
        """The operator of the K frames on cuda:0 (``framed=False``: K plain components with frame 0's multiplier)."""
        import torch
        Zc = dt(Z)[1]
        opts = {"NUFFT_TOEPLITZ_FUSED": 0} if path == "dense" else {}
        plan = nufft.PlanNUFFT(Zc, self.Ns, backend=nufft.ROCBackend(0), options=opts, ntransforms=self.K, **kw)
        op = nufft.ToeplitzOperator(plan)
        plan.close()
        assert path is None or op.path == path, (self.Ns, path, op.path)
        spec = [torch.from_numpy(np.ascontiguousarray(s.astype(Zc))).cuda() for s in self.spectra]
        if framed:
            op.set_spectra_frames(spec)
        else:
            op.set_spectrum(spec[0])
        return op


_FRAMES = {}


def frames(Ns, K, shared=False):
    """``shared``: every frame has the multiplier of a = 0.2 (a plain operator's system)."""
    key = (Ns, K, shared)
    if key not in _FRAMES:
        _FRAMES[key] = Frames(Ns, K, a=0.2 if shared else None)
    return _FRAMES[key]


# (Ns, K, path the operator must take or None)
SOLVER_CASES = [((9,), 9, None), ((7, 5), 3, None), ((32, 40), 3, "fused"), ((5, 6, 7), 9, None), ((32, 32, 32), 2, "fused")]
PATHS = {(Ns, K): path for Ns, K, path in SOLVER_CASES}

# (tv fraction, tv_t fraction) of max|b| per (Ns, K, spatial), the same for both periodic settings; elsewhere (0.1, 0.1).  The shares of
# the tenth iteration measured on the CPU in float64 are in the comments (temporal; spatial), with those of (0.1, 0.1) where it fails.
DEFAULT_FRACTIONS = (0.1, 0.1)
FRACTIONS = {                                    # (Ns, K, spatial): non-periodic | periodic
    ((9,), 9, False): (0.0, 0.2),                # 0.76 | 0.72                       (0.1: 0.94 | 0.94)
    ((9,), 9, True): (0.15, 0.15),               # 0.74; 0.68 | 0.65; 0.63          (0.1, 0.1: 0.96; 0.86 | 0.93; 0.85)
    ((7, 5), 3, False): (0.0, 0.2),              # 0.73 | 0.61                       (0.1: 0.91 | 0.90)
    ((7, 5), 3, True): (0.2, 0.1),               # 0.71; 0.68 | 0.62; 0.56          (0.1, 0.1: 0.83; 0.99 | 0.76; 0.98)
    ((32, 40), 3, False): (0.0, 0.1),            # 0.86 | 0.78
    ((32, 40), 3, True): (0.12, 0.1),            # 0.48; 0.71 | 0.36; 0.60          (0.1, 0.1: 0.56; 0.86 | 0.45; 0.80)
    ((5, 6, 7), 9, False): (0.0, 0.2),           # 0.73 | 0.73                       (0.1: 0.93 | 0.93)
    ((5, 6, 7), 9, True): (0.15, 0.1),           # 0.60; 0.86 | 0.55; 0.81          (0.1, 0.1: 0.83; 1.00 | 0.81; 1.00)
    ((32, 32, 32), 2, False): (0.0, 0.1),        # 0.80 | 0.38
    ((32, 32, 32), 2, True): (0.12, 0.03),       # 0.72; 0.47 | 0.56; 0.36          (0.1, 0.1: 0.20; 0.66 | 0.04; 0.50)
}


def weights(Ns, K, periodic, spatial, b):
    f_s, f_t = FRACTIONS.get((Ns, K, bool(spatial)), DEFAULT_FRACTIONS)
    top = float(np.abs(np.asarray(b)).max())
    return (f_s * top if spatial else 0.0), f_t * top


_REFERENCES = {}


def reference(Ns, K, Z, tv, tv_t, periodic, spatial, lam=0.0, shared=False, high=False, apply=None, key=None, **kw):
    """tvt_reference.tvpd_t on frames(Ns, K) with the right-hand side rounded to the element type of Z, run in that element type (or, with
    ``high``, in float64 on the same rounded input), cached and never modified.  ``apply`` / ``key``: another operator on the same
    right-hand side (coil maps, a coupled system), cached under ``key``."""
    k = (Ns, K, Z, float(np.max(tv)), float(tv_t), bool(periodic), bool(spatial), float(lam), shared, high, key, tuple(sorted(kw.items())))
    if k not in _REFERENCES:
        s = frames(Ns, K, shared)
        Zc = dt(Z)[1]
        step = kw.pop("step", s.step(lam))
        _REFERENCES[k] = TT.tvpd_t(apply or s.apply, s.b.astype(Zc), tv, tv_t, step, periodic=periodic, spatial=spatial, lam=lam,
                                   dtype=np.complex128 if high else Zc, **kw)
    return _REFERENCES[k]
