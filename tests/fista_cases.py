"""Systems, bars and cached numpy references shared by tests/test_gpu_wavelet.py and tests/test_gpu_fista.py.  No GPU import.

Two kinds of system, both given to the operator as an exact spectrum (``set_spectrum``), so the only error in G is the operator's own:
  * point sets whose dense matrix exists (n <= 2048): the ``System`` of test_gpu_cg.py, shared with it through its cache;
  * the analytic spectrum T[d] = Π_dim a^|d_dim| (coefficients of a product of Poisson kernels, as in test_gpu_cg.py's
    test_more_workgroups): G is the Kronecker product of the D matrices a^|k − k'|, applied here axis by axis in float64, and its
    eigenvalues lie in [((1 − a) / (1 + a))^D, ((1 + a) / (1 − a))^D].
"""
import numpy as np

import fista_reference as F
import toeplitz_reference as R
import wavelet_reference as W

EPS = {"c128": 2.0 ** -52, "c64": 2.0 ** -23}


def dt(Z):
    """(real type, complex type, parity bar of the operator, ε)."""
    return (np.float64, np.complex128, 1e-12, EPS[Z]) if Z == "c128" else (np.float32, np.complex64, 1e-5, EPS[Z])


class Analytic:
    def __init__(self, Ns, a=0.2, seed=0, nrhs=2):
        rng = np.random.default_rng(seed)
        self.Ns, self.fftshift, self.a, self.shape, D = Ns, False, a, Ns[::-1], len(Ns)
        spec = np.ones([2 * n for n in reversed(Ns)])
        self.mats = []
        for dim, n in enumerate(Ns):                                               # dimension dim is axis D − 1 − dim
            shape = [1] * D
            shape[D - 1 - dim] = 2 * n
            spec = spec * (a ** np.abs(np.asarray(R.modes(2 * n)).astype(np.float64))).reshape(shape)
            k = np.asarray(R.modes(n)).astype(np.float64)
            self.mats.append(a ** np.abs(k[:, None] - k[None, :]))
        self.spec = spec.astype(np.complex128)
        self.lmax = ((1 + a) / (1 - a)) ** D                                       # an upper bound
        self.A = None
        self.bs = [rng.standard_normal(self.shape) + 1j * rng.standard_normal(self.shape) for _ in range(nrhs)]

    def apply(self, u):
        u = np.asarray(u).astype(np.complex128)
        D = len(self.Ns)
        for dim, M in enumerate(self.mats):
            u = np.moveaxis(np.tensordot(M, u, axes=([1], [D - 1 - dim])), 0, D - 1 - dim)
        return u

    def operator(self, nufft, Z, path, C=1, **kw):
        import torch
        _, Zc, _, _ = dt(Z)
        opts = {"NUFFT_TOEPLITZ_FUSED": 0} if path == "dense" else {}
        plan = nufft.PlanNUFFT(Zc, self.Ns, backend=nufft.ROCBackend(0), options=opts, ntransforms=C, **kw)
        op = nufft.ToeplitzOperator(plan)
        assert op.path == path, (self.Ns, path, op.path)
        op.set_spectrum(torch.from_numpy(np.ascontiguousarray(self.spec.astype(Zc))).cuda())
        plan.close()
        return op


# (Ns, levels, path): the solver's cases.  Dense: point sets with the exact matrix; fused: the analytic spectrum.
SOLVER_CASES = [((48, 40), 3, "dense"), ((64, 80), 3, "fused"), ((16, 16, 8), 2, "dense"), ((64, 64, 64), 3, "fused")]
LEVELS = {Ns: lev for Ns, lev, _ in SOLVER_CASES}
PATHS = {Ns: path for Ns, _, path in SOLVER_CASES}

# l1 as a fraction of max|W b| per case and wavelet, chosen on the CPU so that in the reference's tenth iteration the share of zero
# detail coefficients lies in [0.2, 0.95] (the tests assert it)
L1_FRACTION = {
    ((48, 40), "haar"): 0.3, ((48, 40), "db2"): 0.3,
    ((64, 80), "haar"): 0.3, ((64, 80), "db2"): 0.3,
    ((16, 16, 8), "haar"): 0.3, ((16, 16, 8), "db2"): 0.3,
    ((64, 64, 64), "haar"): 0.3, ((64, 64, 64), "db2"): 0.3,
}

_SYSTEMS = {}


def system(Ns):
    if Ns not in _SYSTEMS:
        if PATHS.get(Ns, "dense") == "fused":
            _SYSTEMS[Ns] = Analytic(Ns, seed=4 * sum(Ns))
        else:
            import test_gpu_cg                                                     # its System and its cache of systems
            _SYSTEMS[Ns] = test_gpu_cg._system(Ns)
    return _SYSTEMS[Ns]


def l1_weight(Ns, wavelet, b):
    return L1_FRACTION[(Ns, wavelet)] * float(np.abs(W.forward(np.asarray(b).astype(np.complex128), wavelet, LEVELS[Ns])).max())


def step(s, lam=0.0):
    """τ = 1 / (1.05 λmax + λ): λmax exact for the dense systems, the analytic upper bound otherwise."""
    return 1.0 / (1.05 * s.lmax + lam)


_REFERENCES = {}


def reference(Ns, Z, wavelet, l1, lam, rhs=0, high=False, **kw):
    """fista_reference.fista on system(Ns) with the right-hand side rounded to the element type of Z, run in that element type (or, with
    ``high``, in float64 on the same rounded input), cached."""
    key = (Ns, Z, wavelet, float(l1), float(lam), rhs, high, tuple(sorted(kw.items())))
    if key not in _REFERENCES:
        s = system(Ns)
        Zc = dt(Z)[1]
        b = s.bs[rhs].astype(Zc)
        _REFERENCES[key] = F.fista(s.apply, b, wavelet, LEVELS[Ns], l1, step(s, lam), lam=lam, dtype=np.complex128 if high else Zc, **kw)
    return _REFERENCES[key]
