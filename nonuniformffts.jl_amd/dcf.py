"""Sample-density compensation weights (Pipe & Menon), above the C ABI's ``nufft_dcf_*`` entry points.

The weights ``w_j`` that :class:`ToeplitzOperator` and ``PointWeights`` take: with them ``exec_type1(w ⊙ y)`` approximates the inverse of
``exec_type2`` and CG on ``A^H W A`` needs fewer iterations on clustered, radial or spiral point sets.  The iteration
``w ← w / (C w)``, ``C`` = interpolation after spreading on the fine grid of a real-data plan with the parent's window, runs in the
library with every scalar on the device (NFFT.jl: ``sdc``).  Plumbing only: argument checks, pointers, and reading the
outcome back.

    w = density_weights(plan, points)                     # Σ w = 1
    dc = DensityCompensation(plan, maxiter=20).set_points(points)
    w = dc.compute()
    dc.iterations, dc.status, dc.residual, dc.history()

The weights are not bit-reproducible between runs: spreading accumulates with atomics.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._handle import _HandleObject
from ._lib import lib
from .plan import _check, _ptr_table, DimensionMismatch, PlanNUFFT


class DensityCompensation(_HandleObject):
    """``DensityCompensation(plan, maxiter=20, tol=0.0, check_every=0, normalize="sum")``: owns a real-data plan with the geometry and
    window of ``plan`` (which is not kept and may be closed afterwards), kept across point sets.

    ``tol=0`` runs ``maxiter`` iterations; ``tol>0`` stops once ``max |C w − 1| <= tol`` (convergence in the maximum norm is slow: a
    fixed count is the default).  ``check_every=0`` enqueues everything without synchronising (a finished state is frozen on the device;
    legal inside ``torch.cuda.graph``); ``check_every=k`` lets the host look at the done flag every ``k`` iterations and stop early.
    ``normalize="sum"`` returns ``Σ w = 1``, ``"none"`` the raw fixed-point iterate."""

    _prefix, _info = "dcf", _lib.NufftDcfInfo

    def __init__(self, plan: PlanNUFFT, maxiter: int = 20, tol: float = 0.0, check_every: int = 0, normalize: str = "sum"):
        if not isinstance(plan, PlanNUFFT):
            raise ValueError("DensityCompensation takes a PlanNUFFT")
        for name, v in (("maxiter", maxiter), ("check_every", check_every)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name} must be an integer")
        if normalize not in _lib.DCF_NORMALIZE:
            raise ValueError('normalize must be "sum" or "none"')
        prm = _lib.NufftDcfParams()
        prm.struct_size = C.sizeof(_lib.NufftDcfParams)
        prm.max_iter, prm.check_every, prm.normalize = maxiter, check_every, _lib.DCF_NORMALIZE[normalize]
        prm.tol = float(tol)
        self._handle = C.c_void_p()
        _check(lib.nufft_dcf_create(C.byref(self._handle), plan._handle, C.byref(prm)))
        self.T = plan.T
        self.device = plan.device
        self.ndim = plan.ndim
        self.maxiter, self.tol, self.check_every, self.normalize = maxiter, float(tol), check_every, normalize
        self.num_points = None

    def _require_gpu(self):
        self._require_open()
        if self.device is None:
            raise ValueError("host-only density compensation (plan with backend=None) has no device path")

    @property
    def oversampled_dims(self):
        """Fine grid of the internal real plan; differs from a complex parent's in dimension 1 where that one is odd."""
        i = self.info()
        return tuple(int(i.N_over[d]) for d in range(self.ndim))

    def set_points(self, points) -> "DensityCompensation":
        """``points``: what ``set_points`` of the plan accepts: a tuple of D vectors, or an ``(Np, D)`` tensor."""
        self._require_gpu()
        if isinstance(points, torch.Tensor):
            if points.dim() == 1:
                points = (points,)
            elif points.dim() == 2:
                points = tuple(points[:, d].contiguous() for d in range(points.shape[1]))
            else:
                raise ValueError("unexpected point container")
        points = tuple(points)
        if len(points) != self.ndim:
            raise DimensionMismatch(f"expected {self.ndim}-dimensional points")
        for x in points:
            if not isinstance(x, torch.Tensor) or x.device != self.device:
                raise ValueError(f"unexpected point container: expected torch tensors on {self.device}")
            if x.dtype != self.T:
                raise ValueError(f"input points must have the same accuracy as the created plan (got {x.dtype})")
            if x.dim() != 1 or not x.is_contiguous():
                raise ValueError("unexpected point container: expected contiguous vectors")
        n = points[0].numel()
        if any(x.numel() != n for x in points):
            raise DimensionMismatch("input points must have the same length along all dimensions")
        _check(lib.nufft_dcf_set_points(self._handle, n, _ptr_table(points), self._stream()))
        self.num_points = n
        return self

    def compute(self, w0: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The weights of the current point set, a real vector of ``Np`` entries.  ``w0``: positive start (None = ones); ``out``: where
        they go (may be ``w0``; None = a new tensor).  Returns ``out``."""
        self._require_gpu()
        if self.num_points is None:
            raise ValueError("set_points must be called before compute")
        n = self.num_points

        def vector(t, what):
            if not isinstance(t, torch.Tensor) or t.device != self.device:
                raise ValueError(f"{what} must be a torch tensor on {self.device}")
            if t.dtype != self.T:
                raise ValueError(f"{what} must be real with the plan's accuracy ({self.T})")
            if t.dim() != 1 or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous vector")
            if t.numel() != n:
                raise DimensionMismatch(f"wrong length of {what} (expected {n}, got {t.numel()})")

        if out is None:
            out = torch.empty(n, dtype=self.T, device=self.device)
        else:
            vector(out, "out")
        if w0 is not None:
            vector(w0, "w0")
            if out.data_ptr() != w0.data_ptr():
                out.copy_(w0)
        _check(lib.nufft_dcf_compute(self._handle, C.c_void_p(out.data_ptr()), 0 if w0 is None else 1, self._stream()))
        return out

    def _result(self):
        self._require_gpu()
        it, st, res = C.c_int32(), C.c_int32(), C.c_double()
        _check(lib.nufft_dcf_get_result(self._handle, C.byref(it), C.byref(st), C.byref(res), self._stream()))
        return it.value, st.value, res.value

    @property
    def iterations(self) -> int:
        """Divisions ``w ← w / (C w)`` applied by the last compute (synchronises the current stream)."""
        return self._result()[0]

    @property
    def status(self) -> str:
        """``"converged"``, ``"max_iter"`` or ``"breakdown"``."""
        return _lib.DCF_STATUS_NAMES[self._result()[1]]

    @property
    def residual(self) -> float:
        """The last ``δ = max |C w − 1|`` the iteration reported (NaN: none); it belongs to the iterate BEFORE the last division."""
        return self._result()[2]

    def history(self) -> torch.Tensor:
        """``[maxiter]`` (host, float64): ``δ_k`` of every iteration; NaN where none was reported (``δ_0`` of the all-ones start,
        iterations after the stop)."""
        self._require_gpu()
        buf = (C.c_double * self.maxiter)()
        _check(lib.nufft_dcf_history(self._handle, buf, len(buf), self._stream()))
        return torch.tensor(list(buf), dtype=torch.float64)

    def __repr__(self):
        i = self.info()
        return (f"DensityCompensation on a {self.ndim}-dimensional {self.T} grid {self.oversampled_dims}, maxiter = {self.maxiter}, "
                f"tol = {self.tol:g}, check_every = {self.check_every}, normalize = {self.normalize}, "
                f"{(i.workspace_bytes + i.plan_bytes) / 1e6:.1f} MB")


def density_weights(plan: PlanNUFFT, points, **kw) -> torch.Tensor:
    """One-shot ``DensityCompensation(plan, **kw).set_points(points).compute()``; the object's plan and arrays are freed before returning."""
    dc = DensityCompensation(plan, **kw)
    try:
        w = dc.set_points(points).compute()
        torch.cuda.current_stream(dc.device).synchronize()       # the object's arrays go away below
    finally:
        dc.close()
    return w
