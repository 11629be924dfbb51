"""FISTA with an l1-wavelet or a locally low-rank prior on a :class:`ToeplitzOperator`, above the C ABI's ``nufft_fista_*`` entry
points.

    min_x  ½⟨x, (G + lam I) x⟩ − Re⟨b, x⟩ + Σ_c l1_c ‖D W x_c‖₁

``W`` an orthogonal periodic wavelet transform, ``D`` the projection on its detail bands.  The whole loop runs in the library: per
iteration one apply of the operator, one streaming kernel, one kernel per wavelet level each way and one decision kernel, every scalar
on the device.  Plumbing only: argument checks, pointers, and reading the outcome back.

    sol = ToeplitzFISTA(op, wavelet="db2", levels=3, l1=1e-3, maxiter=100, tol=1e-4)
    x = sol.solve(b)
    sol.iterations, sol.status, sol.change, sol.history()

With ``prior="llr"`` the last term is ``nuc · Σ_blocks ‖M_block(x)‖_*``, the nuclear norms of the ``B × K`` Casorati matrices of small
spatial blocks over the K components (:class:`LocallyLowRank`): one kernel forms the gradient step, the proximal map and the momentum
step, and the components are one system.

    sol = ToeplitzFISTA(op, prior="llr", block=8, nuc=1e-2, maxiter=100, tol=1e-4)
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import lib
from ._solver import _ToeplitzSolver, _change, _doc
from .plan import DimensionMismatch, _check
from .toeplitz import ToeplitzOperator
from .llr import _llr_params
from .wavelet import _wavelet_id


class ToeplitzFISTA(_ToeplitzSolver):
    """``ToeplitzFISTA(op, wavelet="db2", levels=3, l1=0.0, step=None, lam=0.0, maxiter=100, tol=1e-4, check_every=0)``.

    ``l1``: a scalar or one weight per component.  ``lam``: the Tikhonov weight (named as in :class:`ToeplitzCG`).  ``step``: the step
    ``τ``; None computes ``1 / (1.05 · max(op.max_eigenvalue()) + lam)`` once, here (the operator then needs its spectrum already).
    ``check_every=0`` enqueues all ``maxiter`` iterations without synchronising (components whose relative change reached ``tol`` are
    frozen on the device; legal inside ``torch.cuda.graph``); ``check_every=k`` lets the host stop early.  Both return the same bits.
    The solver keeps ``op`` alive; ``op.set_points`` / ``set_spectrum`` between two solves is allowed.  On a coupled operator the
    components are one system: one change and one stopping test, reported identically for every component.

    ``ToeplitzFISTA(op, prior="llr", block=8 | (b1, …, bD), nuc=0.0, shifts=False, seed=0, step=None, lam=0.0, maxiter=100, tol=1e-4,
    check_every=0)``: the locally low-rank prior of :class:`LocallyLowRank` with weight ``nuc`` instead.  The prior couples the
    components, so they are one system on every operator, and ``history()[:, :, 1]`` is the sum of the blocks' nuclear norms.  With
    ``shifts=True`` every iteration uses another cyclic shift of the blocks (a function of the iteration number and ``seed`` only);
    the objective then changes every iteration and the relative change does not fall to a small ``tol``: use ``tol=0`` and a fixed
    ``maxiter``.  ``wavelet``, ``levels`` and ``l1`` belong to ``prior="wavelet"`` (the default), ``block``, ``nuc``, ``shifts`` and
    ``seed`` to ``prior="llr"``; passing the other prior's arguments raises ``ValueError``."""

    _prefix, _info, _status_names = "fista", _lib.NufftFistaInfo, _lib.FISTA_STATUS_NAMES
    _columns = staticmethod(lambda n: (n, 2))

    def __init__(self, op: ToeplitzOperator, wavelet=None, levels=None, l1=None, step=None, lam: float = 0.0,
                 maxiter: int = 100, tol: float = 1e-4, check_every: int = 0, prior: str = "wavelet", block=None, nuc=None, shifts=None,
                 seed=None):
        if not isinstance(op, ToeplitzOperator):
            raise ValueError("ToeplitzFISTA takes a ToeplitzOperator")
        if prior not in ("wavelet", "llr"):
            raise ValueError(f'prior must be "wavelet" or "llr" (got {prior!r})')
        theirs = {"wavelet": wavelet, "levels": levels, "l1": l1} if prior == "llr" else {"block": block, "nuc": nuc, "shifts": shifts, "seed": seed}
        given = [k for k, v in theirs.items() if v is not None]
        if given:
            raise ValueError(f'{", ".join(given)} cannot be passed with prior="{prior}"')
        self.prior = prior
        if prior == "llr":
            self._init_llr(op, 8 if block is None else block, 0.0 if nuc is None else nuc, bool(shifts), 0 if seed is None else seed, step, lam,
                           maxiter, tol, check_every)
            return
        wavelet, levels, l1 = "db2" if wavelet is None else wavelet, 3 if levels is None else levels, 0.0 if l1 is None else l1
        self._check_ints(maxiter=maxiter, check_every=check_every, levels=levels)
        l1s = [float(l1)] * op.ntransforms if isinstance(l1, (int, float)) else [float(v) for v in l1]
        if len(l1s) != op.ntransforms:
            raise DimensionMismatch(f"wrong amount of l1 weights (expected {op.ntransforms})")
        wid = _wavelet_id(wavelet)
        if step is None:
            step = self._default_step(op, lam)
        prm = _lib.NufftFistaParams()
        prm.struct_size = C.sizeof(_lib.NufftFistaParams)
        prm.max_iter, prm.check_every, prm.wavelet, prm.levels = maxiter, check_every, wid, levels
        prm.tol, prm.step, prm.l1, prm.lambda_ = float(tol), float(step), l1s[0], float(lam)
        self._handle = C.c_void_p()
        _check(lib.nufft_fista_create(C.byref(self._handle), op._handle, C.byref(prm)))
        self.op = op
        self.wavelet, self.levels, self.l1, self.step, self.lam = wavelet, levels, tuple(l1s), float(step), float(lam)
        self.maxiter, self.tol, self.check_every = maxiter, float(tol), check_every
        try:
            _check(lib.nufft_fista_set_l1(self._handle, (C.c_double * len(l1s))(*l1s), len(l1s)))
        except Exception:
            self.close()
            raise

    def _init_llr(self, op, block, nuc, shifts, seed, step, lam, maxiter, tol, check_every):
        self._check_ints(maxiter=maxiter, check_every=check_every)
        op._require_open()
        lp = _llr_params(op.ndim, block, shifts, seed)
        if step is None:
            step = self._default_step(op, lam)
        prm = _lib.NufftFistaParams()
        prm.struct_size = C.sizeof(_lib.NufftFistaParams)
        prm.max_iter, prm.check_every = maxiter, check_every
        prm.tol, prm.step, prm.lambda_ = float(tol), float(step), float(lam)
        self._handle = C.c_void_p()
        _check(lib.nufft_fista_create_llr(C.byref(self._handle), op._handle, C.byref(prm), C.byref(lp), float(nuc)))
        self.op = op
        self.block, self.nuc, self.shifts, self.seed = tuple(lp.block[d] for d in range(op.ndim)), float(nuc), bool(shifts), seed
        self.step, self.lam, self.maxiter, self.tol, self.check_every = float(step), float(lam), maxiter, float(tol), check_every

    def set_nuc(self, nuc):
        """The weight of the locally low-rank prior for the following solves."""
        self._require_open()
        _check(lib.nufft_fista_set_nuc(self._handle, float(nuc)))
        self.nuc = float(nuc)

    def set_l1(self, l1):
        """One weight per component (or a scalar) of the wavelet prior for the following solves."""
        self._require_open()
        n = self.op.ntransforms
        l1s = [float(l1)] * n if isinstance(l1, (int, float)) else [float(v) for v in l1]
        _check(lib.nufft_fista_set_l1(self._handle, (C.c_double * len(l1s))(*l1s), len(l1s)))
        self.l1 = tuple(l1s)

    change = _change
    history = _doc(_ToeplitzSolver.history,
                   """``[max(iterations), ntransforms, 2]`` (host, float64): relative change and ``‖D W x‖₁`` (``prior="llr"``: the sum of the
        blocks' nuclear norms) after every iteration; NaN where an iteration did not change the component.""")

    def __repr__(self):
        i = self.info()
        what = f"locally low-rank blocks {self.block}" if self.prior == "llr" else f"{self.wavelet!r} x {self.levels} levels"
        return (f"ToeplitzFISTA on a {self.op.ndim}-dimensional {self.op.Z} operator, {what}, "
                f"step = {self.step:g}, lam = {self.lam:g}, maxiter = {self.maxiter}, tol = {self.tol:g}, check_every = {self.check_every}, "
                f"{i.workspace_bytes / 1e6:.1f} MB")
