"""Second-order total generalized variation (TGV²) on a :class:`ToeplitzOperator`: the primal-dual solver above the C ABI's
``nufft_tgv_*`` entry points.  The operator alone is ``TotalVariation.sym_gradient / sym_adjoint / sym_norm`` (tv.py).

    min over x, v   ½⟨x, (G + lam I) x⟩ − Re⟨b, x⟩ + Σ_c α1_c Σ_i |(∇x_c − v_c)_i|₂ + α0_c Σ_i |(E v_c)_i|_F

``∇`` is the periodic forward difference of :class:`TotalVariation`, ``E`` the symmetrised gradient from periodic backward differences.
Total variation turns smooth ramps into stairs; here the vector field ``v`` takes up the slope, and only its own roughness is charged.
The whole loop runs in the library: per iteration one apply of the operator, four stencil kernels and one decision kernel, every scalar
on the device.  Plumbing only: argument checks, pointers, and reading the outcome back.

    sol = ToeplitzTGV(op, alpha1=1e-3, maxiter=200, tol=1e-4)        # alpha0 = 2 alpha1
    x = sol.solve(b)
    sol.iterations, sol.status, sol.change, sol.history(), sol.field()
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import lib
from ._solver import _ToeplitzSolver, _change, _doc
from .plan import DimensionMismatch, _check, _ptr_table
from .toeplitz import ToeplitzOperator
from .tv import _weights


class ToeplitzTGV(_ToeplitzSolver):
    """``ToeplitzTGV(op, alpha1, alpha0=None, step=None, sigma=None, lam=0.0, maxiter=100, tol=1e-4, check_every=0)``.

    ``alpha1``, ``alpha0``: scalars or one weight per component; ``alpha0=None`` is ``2 · alpha1`` (Knoll et al. 2011).  ``alpha1 = 0``
    leaves x on plain gradient descent, ``alpha0 = 0`` lets ``v`` follow ``∇x`` for free.  ``lam``: the Tikhonov weight.  ``step``: the
    primal step ``τ``; None computes ``1 / (1.05 · max(op.max_eigenvalue()) + lam)`` once, here.  ``sigma``: the dual step ``σ``; None is
    ``1 / (16 D τ)``, which keeps ``1/τ − σ‖K‖² >= L/2`` for ``τ <= 1/L`` (``‖K‖² <= 8 D``).  ``check_every``, frozen components, coupled
    operators and the life of ``op`` are as for :class:`ToeplitzTV`.  ``v`` and both dual variables restart at zero in every ``solve``."""

    _prefix, _info, _status_names = "tgv", _lib.NufftTgvInfo, _lib.TGV_STATUS_NAMES
    _columns = staticmethod(lambda n: (n, 3))

    def __init__(self, op: ToeplitzOperator, alpha1, alpha0=None, step=None, sigma=None, lam: float = 0.0, maxiter: int = 100,
                 tol: float = 1e-4, check_every: int = 0):
        if not isinstance(op, ToeplitzOperator):
            raise ValueError("ToeplitzTGV takes a ToeplitzOperator")
        self._check_ints(maxiter=maxiter, check_every=check_every)
        op._require_open()
        a1, a0 = self._pairs(alpha1, alpha0, op.ntransforms)
        if sigma is not None and not float(sigma) > 0.0:
            raise ValueError("sigma must be positive (None: 1 / (16 D step))")
        if step is None:
            step = self._default_step(op, lam)
        prm = _lib.NufftTgvParams()
        prm.struct_size = C.sizeof(_lib.NufftTgvParams)
        prm.max_iter, prm.check_every = maxiter, check_every
        prm.tol, prm.step, prm.sigma, prm.lambda_ = float(tol), float(step), 0.0 if sigma is None else float(sigma), float(lam)
        prm.alpha1, prm.alpha0 = a1[0], a0[0]
        self._handle = C.c_void_p()
        _check(lib.nufft_tgv_create(C.byref(self._handle), op._handle, C.byref(prm)))
        self.op = op
        self.step, self.lam = float(step), float(lam)
        self.maxiter, self.tol, self.check_every = maxiter, float(tol), check_every
        try:
            self._set(a1, a0)
            self.sigma = self.info().sigma
        except Exception:
            self.close()
            raise

    @staticmethod
    def _pairs(alpha1, alpha0, n):
        a1 = _weights(alpha1, n)
        a0 = [2.0 * v for v in a1] if alpha0 is None else _weights(alpha0, n)
        if len(a1) != n or len(a0) != n:
            raise DimensionMismatch(f"wrong amount of weights (expected {n})")
        return a1, a0

    def _set(self, a1, a0):
        n = len(a1)
        _check(lib.nufft_tgv_set_weights(self._handle, (C.c_double * n)(*a1), (C.c_double * n)(*a0), n))
        self.alpha1, self.alpha0 = tuple(a1), tuple(a0)

    def set_weights(self, alpha1, alpha0=None):
        """One pair of weights per component (or scalars; ``alpha0=None``: ``2 · alpha1``) for the following solves."""
        self._require_open()
        self._set(*self._pairs(alpha1, alpha0, self.op.ntransforms))

    def field(self):
        """``v`` of the last solve: per component a tuple of D tensors, dimension 1 first (one component: that tuple itself).  Copies on
        the current stream without synchronising."""
        self._require_open()
        op = self.op
        v = tuple(tuple(torch.empty(op.shape, dtype=op.Z, device=op.device) for _ in range(op.ndim)) for _ in range(op.ntransforms))
        _check(lib.nufft_tgv_copy_field(self._handle, _ptr_table([u for comp in v for u in comp]), op._stream()))
        return v[0] if op.ntransforms == 1 else v

    change = _change
    history = _doc(_ToeplitzSolver.history,
                   """``[max(iterations), ntransforms, 3]`` (host, float64): relative change, ``Σ_i |(∇x − v)_i|₂`` and ``Σ_i |(E v)_i|_F`` after
        every iteration; NaN where an iteration did not change the component.""")

    def __repr__(self):
        i = self.info()
        return (f"ToeplitzTGV on a {self.op.ndim}-dimensional {self.op.Z} operator, alpha1 = {self.alpha1}, alpha0 = {self.alpha0}, "
                f"step = {self.step:g}, sigma = {self.sigma:g}, lam = {self.lam:g}, maxiter = {self.maxiter}, tol = {self.tol:g}, "
                f"check_every = {self.check_every}, {i.workspace_bytes / 1e6:.1f} MB")
