"""What the solver classes on a :class:`ToeplitzOperator` share (:class:`ToeplitzCG`, :class:`ToeplitzFISTA`, :class:`ToeplitzTV`,
:class:`ToeplitzLPS`) on top of the handle of ``_handle.py``: ``solve`` and reading the outcome back.  The C ABI's solvers are shaped alike
(``nufft_<prefix>_destroy / _get_info / _solve / _get_result / _history``), so a class states its prefix and the shape of its history."""
from __future__ import annotations

import ctypes as C
import functools
import math

import torch

from ._handle import _HandleObject
from .plan import _check, _ptr_table


def _doc(member, doc):
    """``member`` (a method or a property of the base class) under a class's own docstring."""
    if isinstance(member, property):
        return property(member.fget, doc=doc)

    @functools.wraps(member)
    def method(self, *args, **kwargs):
        return member(self, *args, **kwargs)
    method.__doc__ = doc
    return method


class _ToeplitzSolver(_HandleObject):
    _status_names = None      # of _lib
    _start_row = 0            # 1: row 0 of the history is the start
    _columns = None           # n -> the shape of one history row

    @staticmethod
    def _check_ints(**values):
        for name, v in values.items():
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name} must be an integer")

    @staticmethod
    def _default_step(op, lam, factor=1.0):
        """``1 / (factor · (1.05 · max(op.max_eigenvalue()) + lam))``: the operator needs its spectrum already."""
        op._require_gpu()
        return 1.0 / (factor * (1.05 * max(op.max_eigenvalue()) + float(lam)))

    def _require_open(self):
        """The library keeps a pointer to the operator: refuse to follow it once either object has been closed."""
        super()._require_open()
        if not self.op._handle.value:
            raise ValueError("the ToeplitzOperator of this solver has been closed: the operator must outlive the solver")

    def solve(self, b, x0=None, out=None):
        """``b``: a tensor of ``plan.shape`` or a tuple of ntransforms such tensors (only read).  ``x0``: starting guess (None = zero);
        ``out``: where the solution goes (may be ``x0``; None = new tensors; never ``b``).  Returns ``out``."""
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
        _check(self._entry("solve")(self._handle, _ptr_table(out_t), _ptr_table(b_t), 0 if x0 is None else 1, op._stream()))
        self._solved(b_t)
        return out

    def _solved(self, b_t):
        """After a solve of the right-hand sides ``b_t`` was enqueued."""

    def _result(self):
        self._require_open()
        n = self.op.ntransforms
        it, st, ch = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_double * n)()
        _check(self._entry("get_result")(self._handle, it, st, ch, n, self.op._stream()))
        return list(it), list(st), list(ch)

    @property
    def iterations(self):
        """Per component: iterations that changed it (synchronises the current stream)."""
        return tuple(self._result()[0])

    @property
    def status(self):
        """Per component: ``"converged"``, ``"max_iter"`` or ``"breakdown"`` (a relative change that is not finite)."""
        return tuple(self._status_names[s] for s in self._result()[1])

    def history(self) -> torch.Tensor:
        """(host, float64) one row per iteration that ran; the class states the columns."""
        self._require_open()
        row = self._columns(self.op.ntransforms)
        all_rows = self.maxiter + self._start_row
        buf = (C.c_double * (all_rows * math.prod(row)))()
        _check(self._entry("history")(self._handle, buf, len(buf), self.op._stream()))
        rows = max(self.iterations) + self._start_row
        return torch.tensor(list(buf), dtype=torch.float64).reshape(all_rows, *row)[:rows].clone()


def _get_change(self):
    return tuple(self._result()[2])


# ``change`` of the solvers that stop on the relative change (ToeplitzCG reports a residual there)
_change = property(_get_change, doc="""Per component: ``‖x⁺ − x‖ / ‖x⁺‖`` of the last iteration that changed it.""")
