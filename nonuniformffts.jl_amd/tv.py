"""Total variation on a :class:`ToeplitzOperator`: the periodic difference operator and the primal-dual solver, above the C ABI's
``nufft_tv_*`` and ``nufft_tvpd_*`` entry points.

    min_x  ½⟨x, (G + lam I) x⟩ − Re⟨b, x⟩ + Σ_c tv_c Σ_i |(∇x_c)_i|₂

``(∇x)_d[i] = x[i + e_d] − x[i]`` with indices mod ``N_d`` on the array as stored, ``|(∇x)_i|₂`` one norm over the D complex differences of
a cell (isotropic TV of a complex image).  The whole loop runs in the library: per iteration one apply of the operator, two stencil
kernels and one decision kernel, every scalar on the device.  Plumbing only: argument checks, pointers, and reading the outcome back.

    sol = ToeplitzTV(op, tv=1e-3, maxiter=200, tol=1e-4)
    x = sol.solve(b)
    sol.iterations, sol.status, sol.change, sol.history()

    T = TotalVariation(op_or_plan)
    y = T.gradient(x)                # a tuple of D tensors, dimension 1 first
    x = T.adjoint(y)                 # ∇ᴴ y
    T.norm(x)                        # Σ_i |(∇x)_i|₂ per component (float64, on the device)

Dynamic imaging: the components are frames, and ``tv_t`` adds ``tv_t ‖∇_t x‖₁``, the difference along the components,
``(∇_t x)_c = x_{c+1} − x_c`` (the last one zero, or ``x_0 − x_{K−1}`` with ``periodic_t=True``); the frames are then one system.

    op.set_points_frames(points_per_frame, weights_per_frame)
    sol = ToeplitzTV(op, tv_t=1e-3, maxiter=200)           # temporal term only: two arrays per frame
    sol = ToeplitzTV(op, tv=1e-4, tv_t=1e-3)               # spatial and temporal
    T.gradient_t(x), T.adjoint_t(z), T.norm_t(x)           # tuples of ntransforms tensors
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._handle import _HandleObject
from ._lib import lib
from ._solver import _ToeplitzSolver, _change, _doc
from .plan import DimensionMismatch, PlanNUFFT, _check, _ptr_table
from .toeplitz import ToeplitzOperator


def _weights(tv, n):
    """One weight per component from a scalar (a Python or numpy number, a 0-d tensor) or from a sequence."""
    if isinstance(tv, (list, tuple)) or getattr(tv, "ndim", 0) > 0:
        return [float(v) for v in tv]
    return [float(tv)] * n


class TotalVariation(_HandleObject):
    """``TotalVariation(op_or_plan)``: element type, shape, ntransforms and device are those of a complex ``PlanNUFFT`` or of a
    ``ToeplitzOperator`` (neither is kept).  Dimension 1 is the fastest one, the LAST axis of the tensors.  The operator is periodic
    in the storage index and commutes with every cyclic shift: ``fftshift=True`` and ``False`` plans give the same prior after
    reordering, whatever the sizes."""

    _prefix, _info = "tv", _lib.NufftTvInfo

    def __init__(self, op_or_plan):
        if not isinstance(op_or_plan, (PlanNUFFT, ToeplitzOperator)):
            raise ValueError("TotalVariation takes a PlanNUFFT or a ToeplitzOperator")
        src = op_or_plan
        if isinstance(src, ToeplitzOperator):
            src._require_open()
            create, self.Z = lib.nufft_tv_create_for_operator, src.Z
        else:
            create, self.Z = lib.nufft_tv_create, src.eltype
        self._handle = C.c_void_p()
        _check(create(C.byref(self._handle), src._handle))
        self.device, self.shape, self.ndim, self.ntransforms = src.device, src.shape, src.ndim, src.ntransforms

    def _check_arrays(self, us, what, count):
        if len(us) != count:
            raise DimensionMismatch(f"wrong amount of {what} arrays (expected {count})")
        super()._check_arrays(us, what, count)

    def _components(self, x):
        """A tensor (one component) or a tuple of ntransforms tensors -> (single, tuple)."""
        single = isinstance(x, torch.Tensor)
        x_t = (x,) if single else tuple(x)
        self._check_arrays(x_t, "input", self.ntransforms)
        return single, x_t

    def gradient(self, x):
        """``∇x``: a tuple of D tensors, dimension 1 first (for a tuple of components: a tuple of such tuples)."""
        self._require_open()
        single, x_t = self._components(x)
        y = tuple(tuple(torch.empty_like(v) for _ in range(self.ndim)) for v in x_t)
        _check(lib.nufft_tv_gradient(self._handle, _ptr_table([u for comp in y for u in comp]), _ptr_table(x_t), self._stream()))
        return y[0] if single else y

    def adjoint(self, y):
        """``∇ᴴy`` for ``y`` as ``gradient`` returns it."""
        self._require_open()
        single = len(y) > 0 and isinstance(y[0], torch.Tensor)
        y_t = (tuple(y),) if single else tuple(tuple(comp) for comp in y)
        if len(y_t) != self.ntransforms or (single and self.ntransforms != 1):
            raise DimensionMismatch(f"wrong amount of components (expected {self.ntransforms})")
        flat = [u for comp in y_t for u in comp]
        for comp in y_t:
            self._check_arrays(comp, "input", self.ndim)
        out = tuple(torch.empty_like(comp[0]) for comp in y_t)
        _check(lib.nufft_tv_adjoint(self._handle, _ptr_table(out), _ptr_table(flat), self._stream()))
        return out[0] if single else out

    def norm(self, x) -> torch.Tensor:
        """``Σ_i |(∇x)_i|₂`` per component: a float64 device tensor of ntransforms values."""
        self._require_open()
        _, x_t = self._components(x)
        sums = torch.empty(self.ntransforms, dtype=torch.float64, device=self.device)
        _check(lib.nufft_tv_norm(self._handle, _ptr_table(x_t), C.c_void_p(sums.data_ptr()), self._stream()))
        return sums

    def _fields(self, y, count):
        """A tuple of ``count`` tensors (one component) or a tuple of ntransforms such tuples -> (single, tuple of tuples)."""
        single = len(y) > 0 and isinstance(y[0], torch.Tensor)
        y_t = (tuple(y),) if single else tuple(tuple(comp) for comp in y)
        if len(y_t) != self.ntransforms or (single and self.ntransforms != 1):
            raise DimensionMismatch(f"wrong amount of components (expected {self.ntransforms})")
        for comp in y_t:
            self._check_arrays(comp, "input", count)
        return single, y_t

    def _sym(self, entry, src, count_in, count_out):
        self._require_open()
        single, src_t = self._fields(src, count_in)
        out = tuple(tuple(torch.empty_like(comp[0]) for _ in range(count_out)) for comp in src_t)
        _check(entry(self._handle, _ptr_table([u for comp in out for u in comp]), _ptr_table([u for comp in src_t for u in comp]), self._stream()))
        return out[0] if single else out

    def sym_gradient(self, v):
        """``E v`` for a vector field ``v`` as ``gradient`` returns it: ``(E v)_de = ½(∂⁻_e v_d + ∂⁻_d v_e)`` from periodic
        backward differences, a tuple of ``D (D + 1) / 2`` tensors in row-major upper-triangle order, (1,1), (1,2), (1,3), (2,2), ..."""
        return self._sym(lib.nufft_tv_sym_gradient, v, self.ndim, self.ndim * (self.ndim + 1) // 2)

    def sym_adjoint(self, r):
        """``Eᴴ r`` for ``r`` as ``sym_gradient`` returns it (off-diagonal entries count twice in the inner product): D tensors."""
        return self._sym(lib.nufft_tv_sym_adjoint, r, self.ndim * (self.ndim + 1) // 2, self.ndim)

    def sym_norm(self, v) -> torch.Tensor:
        """``Σ_i |(E v)_i|_F`` per component, ``|W|_F² = Σ_d |W_dd|² + 2 Σ_{d<e} |W_de|²``: a float64 device tensor of ntransforms values."""
        self._require_open()
        _, v_t = self._fields(v, self.ndim)
        sums = torch.empty(self.ntransforms, dtype=torch.float64, device=self.device)
        _check(lib.nufft_tv_sym_norm(self._handle, _ptr_table([u for comp in v_t for u in comp]), C.c_void_p(sums.data_ptr()), self._stream()))
        return sums

    def _frames(self, x, periodic):
        if self.ntransforms < 2:
            raise ValueError("the difference along the components needs ntransforms >= 2")
        if not isinstance(periodic, (bool, int)):
            raise ValueError("periodic must be a bool")
        x_t = tuple(x)
        self._check_arrays(x_t, "input", self.ntransforms)
        return x_t

    def gradient_t(self, x, periodic: bool = False):
        """``∇_t x``: a tuple of ntransforms tensors, ``x[c + 1] − x[c]``; the last one is zero, or ``x[0] − x[K − 1]`` if ``periodic``."""
        self._require_open()
        x_t = self._frames(x, periodic)
        z = tuple(torch.empty_like(v) for v in x_t)
        _check(lib.nufft_tv_gradient_t(self._handle, _ptr_table(z), _ptr_table(x_t), int(bool(periodic)), self._stream()))
        return z

    def adjoint_t(self, z, periodic: bool = False):
        """``∇_tᴴ z``: ``z[c − 1] − z[c]`` with ``z[−1] = z[K − 1]`` if ``periodic``, else both taken as zero."""
        self._require_open()
        z_t = self._frames(z, periodic)
        out = tuple(torch.empty_like(v) for v in z_t)
        _check(lib.nufft_tv_adjoint_t(self._handle, _ptr_table(out), _ptr_table(z_t), int(bool(periodic)), self._stream()))
        return out

    def norm_t(self, x, periodic: bool = False) -> torch.Tensor:
        """``Σ_i |(∇_t x)_c[i]|`` per component: a float64 device tensor of ntransforms values (their sum is ``‖∇_t x‖₁``)."""
        self._require_open()
        x_t = self._frames(x, periodic)
        sums = torch.empty(self.ntransforms, dtype=torch.float64, device=self.device)
        _check(lib.nufft_tv_norm_t(self._handle, _ptr_table(x_t), int(bool(periodic)), C.c_void_p(sums.data_ptr()), self._stream()))
        return sums

    def __repr__(self):
        i = self.info()
        return (f"TotalVariation on {self.ndim}-dimensional {self.Z} arrays of shape {self.shape}, tile {tuple(i.tile[d] for d in range(self.ndim))}, "
                f"{i.workspace_bytes / 1e3:.1f} kB")


class ToeplitzTV(_ToeplitzSolver):
    """``ToeplitzTV(op, tv=0.0, step=None, sigma=None, lam=0.0, maxiter=100, tol=1e-4, check_every=0, tv_t=None, periodic_t=False,
    spatial=None)``.

    ``tv``: a scalar or one weight per component.  ``lam``: the Tikhonov weight (named as in :class:`ToeplitzCG`).  ``step``: the
    primal step ``τ``; None computes ``1 / (1.05 · max(op.max_eigenvalue()) + lam)`` once, here (the operator then needs its spectrum
    already).  ``sigma``: the dual step ``σ``; None is ``1 / (8 D τ)``, which keeps ``1/τ − σ‖∇‖² >= L/2`` for ``τ <= 1/L``.
    ``check_every=0`` enqueues all ``maxiter`` iterations without synchronising (components whose relative change reached ``tol`` are
    frozen on the device; legal inside ``torch.cuda.graph``); ``check_every=k`` lets the host stop early.  Both return the same bits.
    The solver keeps ``op`` alive; ``op.set_points`` / ``set_spectrum`` between two solves is allowed.  On a coupled operator the
    components are one system: one change and one stopping test, reported identically for every component.  The dual variable restarts
    at zero in every ``solve``.

    ``tv_t`` (None: no temporal term, the solver above): the weight of ``‖∇_t x‖₁`` along the components, which needs
    ``ntransforms >= 2`` and makes the frames one system on every operator (one change, one stopping test); history column 2 is then
    each frame's share of the prior's value.  ``periodic_t``: the last frame is followed by the first (cine).  ``spatial``: keep the
    spatial term (None: iff any ``tv > 0``), decided here and never switched; without it the solver holds two arrays per frame instead
    of ``2 + D`` and ``set_tv`` with a non-zero weight is refused.  ``sigma=None`` is then ``1 / (8 n_d τ)`` with ``n_d = D + 1``
    (spatial term on) or ``1``."""

    _prefix, _info, _status_names = "tvpd", _lib.NufftTvpdInfo, _lib.TVPD_STATUS_NAMES
    _columns = staticmethod(lambda n: (n, 2))

    def __init__(self, op: ToeplitzOperator, tv=0.0, step=None, sigma=None, lam: float = 0.0, maxiter: int = 100, tol: float = 1e-4,
                 check_every: int = 0, tv_t=None, periodic_t: bool = False, spatial=None):
        if not isinstance(op, ToeplitzOperator):
            raise ValueError("ToeplitzTV takes a ToeplitzOperator")
        self._check_ints(maxiter=maxiter, check_every=check_every)
        op._require_open()
        tvs = _weights(tv, op.ntransforms)
        if len(tvs) != op.ntransforms:
            raise DimensionMismatch(f"wrong amount of tv weights (expected {op.ntransforms})")
        if sigma is not None and not float(sigma) > 0.0:
            raise ValueError("sigma must be positive (None: 1 / (8 D step))")
        if step is None:
            step = self._default_step(op, lam)
        prm = _lib.NufftTvpdParams()
        prm.struct_size = C.sizeof(_lib.NufftTvpdParams)
        prm.max_iter, prm.check_every = maxiter, check_every
        prm.tol, prm.step, prm.sigma, prm.tv, prm.lambda_ = float(tol), float(step), 0.0 if sigma is None else float(sigma), tvs[0], float(lam)
        self._handle = C.c_void_p()
        self.temporal = tv_t is not None
        if self.temporal:
            if spatial is None:
                spatial = any(v > 0.0 for v in tvs)
            tprm = _lib.NufftTvtParams()
            tprm.struct_size = C.sizeof(_lib.NufftTvtParams)
            tprm.periodic, tprm.spatial, tprm.tv_t = int(bool(periodic_t)), int(bool(spatial)), float(tv_t)
            _check(lib.nufft_tvpd_create_temporal(C.byref(self._handle), op._handle, C.byref(prm), C.byref(tprm)))
        else:
            if spatial is not None or periodic_t:
                raise ValueError("spatial and periodic_t belong to the temporal term: give tv_t")
            _check(lib.nufft_tvpd_create(C.byref(self._handle), op._handle, C.byref(prm)))
        self.periodic_t, self.spatial = bool(periodic_t), True if not self.temporal else bool(spatial)
        self.op = op
        self.tv, self.step, self.lam = tuple(tvs), float(step), float(lam)
        self.maxiter, self.tol, self.check_every = maxiter, float(tol), check_every
        try:
            _check(lib.nufft_tvpd_set_tv(self._handle, (C.c_double * len(tvs))(*tvs), len(tvs)))
            self.sigma = self.info().sigma
        except Exception:
            self.close()
            raise

    def set_tv(self, tv):
        """One weight per component (or a scalar) for the following solves."""
        self._require_open()
        n = self.op.ntransforms
        tvs = _weights(tv, n)
        _check(lib.nufft_tvpd_set_tv(self._handle, (C.c_double * len(tvs))(*tvs), len(tvs)))
        self.tv = tuple(tvs)

    @property
    def tv_t(self):
        """The temporal weight in use (None on a solver without the temporal term)."""
        if not self.temporal:
            return None
        self._require_open()
        out = _lib.NufftTvtParams()
        out.struct_size = C.sizeof(_lib.NufftTvtParams)
        _check(lib.nufft_tvpd_get_temporal(self._handle, C.byref(out)))
        return out.tv_t

    def set_tv_t(self, tv_t):
        """The temporal weight of the following solves."""
        self._require_open()
        _check(lib.nufft_tvpd_set_tv_t(self._handle, float(tv_t)))

    change = _change
    history = _doc(_ToeplitzSolver.history,
                   """``[max(iterations), ntransforms, 2]`` (host, float64): relative change and ``Σ_i |(∇x)_i|₂`` after every iteration; NaN where
        an iteration did not change the component.""")

    def __repr__(self):
        i = self.info()
        return (f"ToeplitzTV on a {self.op.ndim}-dimensional {self.op.Z} operator, tv = {self.tv}, step = {self.step:g}, sigma = {self.sigma:g}, "
                f"lam = {self.lam:g}, maxiter = {self.maxiter}, tol = {self.tol:g}, check_every = {self.check_every}, "
                f"{i.workspace_bytes / 1e6:.1f} MB")
