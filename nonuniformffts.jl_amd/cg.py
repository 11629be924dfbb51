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
from .plan import _check, _ptr_table
from .toeplitz import ToeplitzOperator


class ToeplitzCG:
    """``ToeplitzCG(op, maxiter=50, rtol=1e-6, lam=0.0, check_every=0)``: allocates three arrays per component next to the operator.

    ``check_every=0`` enqueues all ``maxiter`` iterations without synchronising (components that reached ``rtol`` are frozen on the
    device; legal inside ``torch.cuda.graph``); ``check_every=k`` lets the host look at the done flags every ``k`` iterations and stop
    early.  Both return the same bits.  The solver keeps ``op`` alive; ``op.set_points`` / ``set_spectrum`` between two solves is
    allowed and changes ``G``.  On a coupled operator (``op.set_points(..., basis=)`` / ``op.set_spectra``) the components are ONE system:
    one α, one β and one stopping test from sums over all components; ``iterations``, ``status``, ``residual`` and ``history()`` then
    report the same values for every component.

    ``precond``: a :class:`ToeplitzPreconditioner` built for ``op`` (kept alive by the solver) or None; ``set_preconditioner`` changes it
    between two solves.  Without one the solver enqueues exactly what it always did."""

    def __init__(self, op: ToeplitzOperator, maxiter: int = 50, rtol: float = 1e-6, lam: float = 0.0, check_every: int = 0, precond=None):
        if not isinstance(op, ToeplitzOperator):
            raise ValueError("ToeplitzCG takes a ToeplitzOperator")
        for name, v in (("maxiter", maxiter), ("check_every", check_every)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name} must be an integer")
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

    def close(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            lib.nufft_cg_destroy(h)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _require_open(self, check_precond=True):
        """The library keeps a pointer to the operator: refuse to follow it once either object has been closed."""
        if not self._handle.value:
            raise ValueError("this ToeplitzCG has been closed")
        if not self.op._handle.value:
            raise ValueError("the ToeplitzOperator of this solver has been closed: the operator must outlive the solver")
        if check_precond and self.precond is not None and not self.precond._handle.value:
            raise ValueError("the ToeplitzPreconditioner of this solver has been closed: clear it with set_preconditioner(None) first")

    def info(self) -> _lib.NufftCgInfo:
        self._require_open()
        out = _lib.NufftCgInfo()
        out.struct_size = C.sizeof(_lib.NufftCgInfo)
        _check(lib.nufft_cg_get_info(self._handle, C.byref(out)))
        return out

    def solve(self, b, x0=None, out=None):
        """``b``: a tensor of ``plan.shape`` or a tuple of ntransforms such tensors (only read).  ``x0``: starting guess (None = zero);
        ``out``: where the solution goes (may be ``x0``: it is then refined in place; None = new tensors).  Returns ``out``."""
        self._require_open()
        op = self.op
        op._require_gpu()
        single = isinstance(b, torch.Tensor)
        b_t = (b,) if single else tuple(b)
        op._check_uniform(b_t, "right-hand side")
        if out is None:
            out_t = tuple(torch.empty_like(v) for v in b_t)
            out = out_t[0] if single else out_t
        else:
            out_t = (out,) if isinstance(out, torch.Tensor) else tuple(out)
            op._check_uniform(out_t, "output")
        if x0 is not None:
            x0_t = (x0,) if isinstance(x0, torch.Tensor) else tuple(x0)
            op._check_uniform(x0_t, "starting guess")
            for o, g in zip(out_t, x0_t):
                if o.data_ptr() != g.data_ptr():
                    o.copy_(g)
        _check(lib.nufft_cg_solve(self._handle, _ptr_table(out_t), _ptr_table(b_t), 0 if x0 is None else 1, op._stream()))
        return out

    def _result(self):
        self._require_open()
        n = self.op.ntransforms
        it, st, res = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_double * n)()
        _check(lib.nufft_cg_get_result(self._handle, it, st, res, n, self.op._stream()))
        return list(it), list(st), list(res)

    @property
    def iterations(self):
        """Per component: iterations that changed it (synchronises the current stream)."""
        return tuple(self._result()[0])

    @property
    def status(self):
        """Per component: ``"converged"``, ``"max_iter"`` or ``"breakdown"``."""
        return tuple(_lib.CG_STATUS_NAMES[s] for s in self._result()[1])

    @property
    def residual(self):
        """Per component: the recursive relative residual ``‖r‖ / ‖b‖`` the stopping rule saw last."""
        return tuple(self._result()[2])

    def history(self) -> torch.Tensor:
        """``[max(iterations) + 1, ntransforms]`` (host, float64): relative residual after every iteration, row 0 the start; NaN
        where an iteration did not change the component."""
        self._require_open()
        n = self.op.ntransforms
        buf = (C.c_double * ((self.maxiter + 1) * n))()
        _check(lib.nufft_cg_history(self._handle, buf, len(buf), self.op._stream()))
        rows = max(self.iterations) + 1
        return torch.tensor(list(buf), dtype=torch.float64).reshape(self.maxiter + 1, n)[:rows].clone()

    def __repr__(self):
        i = self.info()
        return (f"ToeplitzCG on a {self.op.ndim}-dimensional {self.op.Z} operator, maxiter = {self.maxiter}, rtol = {self.rtol:g}, "
                f"lam = {self.lam:g}, check_every = {self.check_every}, {'preconditioned, ' if self.precond is not None else ''}"
                f"{i.workspace_bytes / 1e6:.1f} MB")
