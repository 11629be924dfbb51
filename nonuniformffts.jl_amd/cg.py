"""Conjugate gradients on ``(G + λ I) x = b`` with ``G`` a :class:`ToeplitzOperator`, above the C ABI's ``nufft_cg_*`` entry points.

With ``b = exec_type1(w ⊙ y)`` this is the weighted, Tikhonov-regularised least-squares inverse of ``exec_type2``.  The whole loop runs
in the library: per iteration one apply of the operator and three HIP kernels, every scalar on the device.  Plumbing
only: argument checks, pointers, and reading the outcome back.

    sol = ToeplitzCG(op, maxiter=50, rtol=1e-6, lam=0.0)
    x = sol.solve(b)
    sol.iterations, sol.status, sol.residual, sol.history()

``precond=ToeplitzPreconditioner(op, lam=...)`` makes it preconditioned CG: the same stopping rule on ``‖r‖ / ‖b‖``, one
apply of ``M⁻¹`` more per iteration and one more array per component.  A coupled operator takes the block preconditioner
``ToeplitzPreconditioner(op, lam=..., block=True)`` and is refused with the scalar one.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import lib
from ._solver import _ToeplitzSolver, _doc
from .plan import _check
from .toeplitz import ToeplitzOperator


class ToeplitzCG(_ToeplitzSolver):
    """``ToeplitzCG(op, maxiter=50, rtol=1e-6, lam=0.0, check_every=0)``: allocates three arrays per component next to the operator.

    ``check_every=0`` enqueues all ``maxiter`` iterations without synchronising (components that reached ``rtol`` are frozen on the
    device; legal inside ``torch.cuda.graph``); ``check_every=k`` lets the host look at the done flags every ``k`` iterations and stop
    early.  Both return the same bits.  The solver keeps ``op`` alive; ``op.set_points`` / ``set_spectrum`` between two solves is
    allowed and changes ``G``.  On a coupled operator (``op.set_points(..., basis=)`` / ``op.set_spectra``) the components are ONE system:
    one α, one β and one stopping test from sums over all components; ``iterations``, ``status``, ``residual`` and ``history()`` then
    report the same values for every component.

    ``precond``: a :class:`ToeplitzPreconditioner` built for ``op`` (kept alive by the solver) or None; ``set_preconditioner`` changes it
    between two solves.  Without one the solver enqueues exactly what it always did."""

    _prefix, _info, _status_names = "cg", _lib.NufftCgInfo, _lib.CG_STATUS_NAMES
    _start_row, _columns = 1, staticmethod(lambda n: (n,))

    def __init__(self, op: ToeplitzOperator, maxiter: int = 50, rtol: float = 1e-6, lam: float = 0.0, check_every: int = 0, precond=None):
        if not isinstance(op, ToeplitzOperator):
            raise ValueError("ToeplitzCG takes a ToeplitzOperator")
        self._check_ints(maxiter=maxiter, check_every=check_every)
        prm = _lib.NufftCgParams()
        prm.struct_size = C.sizeof(_lib.NufftCgParams)
        prm.max_iter, prm.check_every = maxiter, check_every
        prm.rtol, prm.lambda_ = float(rtol), float(lam)
        self._handle = C.c_void_p()
        _check(lib.nufft_cg_create(C.byref(self._handle), op._handle, C.byref(prm)))
        self.op = op
        self.maxiter, self.rtol, self.lam, self.check_every = maxiter, float(rtol), float(lam), check_every
        self.precond = None
        if precond is not None:
            try:
                self.set_preconditioner(precond)
            except Exception:
                self.close()
                raise

    def set_preconditioner(self, precond) -> "ToeplitzCG":
        """``precond``: a :class:`ToeplitzPreconditioner` created for this solver's operator, or None for plain CG."""
        from .precond import ToeplitzPreconditioner
        self._require_open(check_precond=False)
        if precond is None:
            _check(lib.nufft_cg_set_preconditioner(self._handle, None))
            self.precond = None
            return self
        if not isinstance(precond, ToeplitzPreconditioner):
            raise ValueError("precond must be a ToeplitzPreconditioner or None")
        precond._require_open()
        _check(lib.nufft_cg_set_preconditioner(self._handle, precond._handle))
        self.precond = precond
        return self

    def _require_open(self, check_precond=True):
        super()._require_open()
        if check_precond and self.precond is not None and not self.precond._handle.value:
            raise ValueError("the ToeplitzPreconditioner of this solver has been closed: clear it with set_preconditioner(None) first")

    solve = _doc(_ToeplitzSolver.solve,
                 """``b``: a tensor of ``plan.shape`` or a tuple of ntransforms such tensors (only read).  ``x0``: starting guess (None = zero);
        ``out``: where the solution goes (may be ``x0``: it is then refined in place; None = new tensors).  Returns ``out``.""")
    status = _doc(_ToeplitzSolver.status, """Per component: ``"converged"``, ``"max_iter"`` or ``"breakdown"``.""")

    @property
    def residual(self):
        """Per component: the recursive relative residual ``‖r‖ / ‖b‖`` the stopping rule saw last."""
        return tuple(self._result()[2])

    history = _doc(_ToeplitzSolver.history,
                   """``[max(iterations) + 1, ntransforms]`` (host, float64): relative residual after every iteration, row 0 the start; NaN
        where an iteration did not change the component.""")

    def __repr__(self):
        i = self.info()
        return (f"ToeplitzCG on a {self.op.ndim}-dimensional {self.op.Z} operator, maxiter = {self.maxiter}, rtol = {self.rtol:g}, "
                f"lam = {self.lam:g}, check_every = {self.check_every}, {'preconditioned, ' if self.precond is not None else ''}"
                f"{i.workspace_bytes / 1e6:.1f} MB")
