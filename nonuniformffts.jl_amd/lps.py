"""Low-rank plus sparse (L+S) reconstruction of a series of frames on a :class:`ToeplitzOperator`, above the C ABI's ``nufft_glr_*``,
``nufft_tsparse_*`` and ``nufft_lps_*`` entry points.

    min over (L, S)   ½⟨L + S, (G + lam I)(L + S)⟩ − Re⟨b, L + S⟩ + nuc ‖C(L)‖_* + l1 ‖T S‖₁

The K = ntransforms components are frames.  ``C(L)`` is the n × K space-time matrix whose column c is frame c; ``T`` is a unitary
transform along the frames, applied per cell: ``"dft"`` (length-K DFT scaled by 1/√K) or ``"identity"``.  The whole loop runs in the
library: per iteration one apply of the operator, four kernels and one decision kernel, every scalar on the device.  Plumbing only.

    op.set_points_frames(points_per_frame, weights_per_frame)
    sol = ToeplitzLPS(op, nuc=…, l1=…, transform="dft", maxiter=200, tol=1e-4)
    x = sol.solve(b)                 # a tuple of K tensors, x = L + S
    sol.low_rank, sol.sparse         # tuples of K tensors (copies)
    sol.iterations, sol.status, sol.change, sol.history()

    G = GlobalLowRank(op_or_plan);   y, nuc = G.apply(x, t)          # singular-value soft-thresholding of C(x)
    T = TemporalSparsity(op_or_plan, "dft");  T.forward(x), T.inverse(c), T.shrink(x, t)
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._handle import _HandleObject
from ._lib import lib
from ._solver import _ToeplitzSolver, _change, _doc
from .plan import PlanNUFFT, _check, _ptr_table
from .toeplitz import ToeplitzOperator


def _transform_id(transform) -> int:
    if transform not in _lib.TSPARSE_IDS:
        raise ValueError(f"transform must be one of {sorted(_lib.TSPARSE_IDS)} (got {transform!r})")
    return _lib.TSPARSE_IDS[transform]


class _FrameObject(_HandleObject):
    """What the two operator objects share: the source's geometry and the argument checks."""

    def _adopt(self, src):
        self.device, self.shape, self.ndim, self.ntransforms = src.device, src.shape, src.ndim, src.ntransforms

    def _in_out(self, x, out):
        """(inputs, outputs, what to return) for a tensor or a tuple of ntransforms tensors; ``out`` may be ``x``."""
        single = isinstance(x, torch.Tensor)
        x_t = (x,) if single else tuple(x)
        self._check_arrays(x_t, "input")
        if out is None:
            out_t = tuple(torch.empty_like(v) for v in x_t)
            out = out_t[0] if single else out_t
        else:
            out_t = (out,) if isinstance(out, torch.Tensor) else tuple(out)
            self._check_arrays(out_t, "output")
        return x_t, out_t, out


class GlobalLowRank(_FrameObject):
    """``GlobalLowRank(op_or_plan)``: element type, shape, ntransforms (1 … 32) and device are those of a complex ``PlanNUFFT`` or of a
    ``ToeplitzOperator`` (neither is kept).  ``apply`` shrinks the singular values of the n × K matrix whose columns are the K arrays,
    through its K × K Gram matrix in FP64: a direction with ``σ_i ≪ σ_max`` is resolved to about ``(σ_max/σ_i)² ε``."""

    _prefix, _info = "glr", _lib.NufftGlrInfo

    def __init__(self, op_or_plan):
        if not isinstance(op_or_plan, (PlanNUFFT, ToeplitzOperator)):
            raise ValueError("GlobalLowRank takes a PlanNUFFT or a ToeplitzOperator")
        src = op_or_plan
        if isinstance(src, ToeplitzOperator):
            src._require_open()
            create, self.Z = lib.nufft_glr_create_for_operator, src.Z
        else:
            create, self.Z = lib.nufft_glr_create, src.eltype
        self._handle = C.c_void_p()
        _check(create(C.byref(self._handle), src._handle))
        self._adopt(src)

    def apply(self, x, t, out=None):
        """``out = prox_{t ‖C(·)‖_*}(x)``; ``out`` may be ``x`` itself.  Returns ``(out, nuc)`` with ``nuc`` a float64 device tensor of
        one element, the nuclear norm of the result."""
        self._require_open()
        x_t, out_t, out = self._in_out(x, out)
        nuc = torch.empty(1, dtype=torch.float64, device=self.device)
        _check(lib.nufft_glr_apply(self._handle, _ptr_table(out_t), _ptr_table(x_t), float(t), C.c_void_p(nuc.data_ptr()), self._stream()))
        return out, nuc

    def last_sweeps(self) -> int:
        """Jacobi sweeps of the last ``apply`` (synchronises the current stream)."""
        self._require_open()
        n = C.c_int32()
        _check(lib.nufft_glr_last_sweeps(self._handle, C.byref(n), self._stream()))
        return n.value

    def __repr__(self):
        i = self.info()
        return (f"GlobalLowRank on {self.ndim}-dimensional {self.Z} arrays of shape {self.shape} x {self.ntransforms} frames, "
                f"tiles of {i.tile_cells} cells, {i.workgroups} workgroups")


class TemporalSparsity(_FrameObject):
    """``TemporalSparsity(op_or_plan, transform="dft" | "identity")``: the unitary transform along the ntransforms (1 … 32) frames,
    per cell.  ``forward`` / ``inverse`` apply ``T`` / ``Tᴴ``; ``shrink(x, t)`` returns the coefficients after the complex soft
    threshold, so that ``inverse`` of them is ``prox_{t ‖T·‖₁}(x)``."""

    _prefix, _info = "tsparse", _lib.NufftTsparseInfo

    def __init__(self, op_or_plan, transform="dft"):
        if not isinstance(op_or_plan, (PlanNUFFT, ToeplitzOperator)):
            raise ValueError("TemporalSparsity takes a PlanNUFFT or a ToeplitzOperator")
        tid = _transform_id(transform)
        src = op_or_plan
        if isinstance(src, ToeplitzOperator):
            src._require_open()
            create, self.Z = lib.nufft_tsparse_create_for_operator, src.Z
        else:
            create, self.Z = lib.nufft_tsparse_create, src.eltype
        self._handle = C.c_void_p()
        _check(create(C.byref(self._handle), src._handle, tid))
        self._adopt(src)
        self.transform = transform

    def forward(self, x, out=None):
        self._require_open()
        x_t, out_t, out = self._in_out(x, out)
        _check(lib.nufft_tsparse_forward(self._handle, _ptr_table(out_t), _ptr_table(x_t), self._stream()))
        return out

    def inverse(self, c, out=None):
        self._require_open()
        c_t, out_t, out = self._in_out(c, out)
        _check(lib.nufft_tsparse_inverse(self._handle, _ptr_table(out_t), _ptr_table(c_t), self._stream()))
        return out

    def shrink(self, x, t, out=None):
        """Returns ``(coefficients, l1)``: ``soft_t(T x)`` and its 1-norm (a float64 device tensor of one element)."""
        self._require_open()
        x_t, out_t, out = self._in_out(x, out)
        l1 = torch.empty(1, dtype=torch.float64, device=self.device)
        _check(lib.nufft_tsparse_shrink(self._handle, _ptr_table(out_t), _ptr_table(x_t), float(t), C.c_void_p(l1.data_ptr()), self._stream()))
        return out, l1

    def __repr__(self):
        return f"TemporalSparsity({self.transform!r}) on {self.ndim}-dimensional {self.Z} arrays of shape {self.shape} x {self.ntransforms} frames"


class ToeplitzLPS(_ToeplitzSolver):
    """``ToeplitzLPS(op, nuc, l1, transform="dft", momentum=True, step=None, lam=0.0, maxiter=100, tol=1e-4, check_every=0)``.

    ``nuc``, ``l1``: the weights of ``‖C(L)‖_*`` and ``‖T S‖₁``.  ``momentum=False`` is the scheme of Otazo, Candès & Sodickson.
    ``step``: None computes ``1 / (2 · (1.05 · max(op.max_eigenvalue()) + lam))`` once, here (the operator then needs its spectrum
    already); the 2 is there because the smooth term, as a function of the pair ``(L, S)``, has the Hessian ``[[A, A], [A, A]]`` with
    largest eigenvalue ``2 λ_max(A)``.  ``check_every`` as for :class:`ToeplitzFISTA`.  The frames are one system: one change, one
    status, reported identically for every component.  The solver keeps ``op`` alive; a new build of it between two solves is allowed."""

    _prefix, _info, _status_names = "lps", _lib.NufftLpsInfo, _lib.LPS_STATUS_NAMES
    _columns = staticmethod(lambda n: (3,))

    def __init__(self, op: ToeplitzOperator, nuc, l1, transform="dft", momentum: bool = True, step=None, lam: float = 0.0,
                 maxiter: int = 100, tol: float = 1e-4, check_every: int = 0):
        if not isinstance(op, ToeplitzOperator):
            raise ValueError("ToeplitzLPS takes a ToeplitzOperator")
        self._check_ints(maxiter=maxiter, check_every=check_every)
        tid = _transform_id(transform)
        op._require_open()
        if step is None:
            step = self._default_step(op, lam, factor=2.0)
        prm = _lib.NufftLpsParams()
        prm.struct_size = C.sizeof(_lib.NufftLpsParams)
        prm.max_iter, prm.check_every, prm.transform, prm.momentum = maxiter, check_every, tid, int(bool(momentum))
        prm.tol, prm.step, prm.lambda_, prm.nuc, prm.l1 = float(tol), float(step), float(lam), float(nuc), float(l1)
        self._handle = C.c_void_p()
        _check(lib.nufft_lps_create(C.byref(self._handle), op._handle, C.byref(prm)))
        self.op = op
        self.nuc, self.l1, self.transform, self.momentum = float(nuc), float(l1), transform, bool(momentum)
        self.step, self.lam, self.maxiter, self.tol, self.check_every = float(step), float(lam), maxiter, float(tol), check_every

    def set_weights(self, nuc, l1):
        """The two weights of the following solves."""
        self._require_open()
        _check(lib.nufft_lps_set_weights(self._handle, float(nuc), float(l1)))
        self.nuc, self.l1 = float(nuc), float(l1)

    solve = _doc(_ToeplitzSolver.solve,
                 """``b``: a tensor of ``plan.shape`` or a tuple of ntransforms such tensors (only read).  ``x0``: starting guess for ``L``
        (None = zero; ``S`` always starts at zero); ``out``: where ``x = L + S`` goes (may be ``x0``; None = new tensors; never ``b``).
        Returns ``out``.""")

    def _solved(self, b_t):
        self._like = b_t

    def _parts(self, which):
        self._require_open()
        like = getattr(self, "_like", None)
        if like is None:
            raise ValueError("no solve yet")
        out = tuple(torch.empty_like(v) for v in like)
        tab = _ptr_table(out)
        _check(lib.nufft_lps_get_parts(self._handle, tab if which == 0 else None, tab if which == 1 else None, self.op._stream()))
        return out

    @property
    def low_rank(self):
        """``L`` of the last solve: a tuple of ntransforms new tensors."""
        return self._parts(0)

    @property
    def sparse(self):
        """``S`` of the last solve: a tuple of ntransforms new tensors."""
        return self._parts(1)

    iterations = _doc(_ToeplitzSolver.iterations, """Per component (all equal): iterations that changed the system (synchronises the current stream).""")
    status = _doc(_ToeplitzSolver.status, """Per component (all equal): ``"converged"``, ``"max_iter"`` or ``"breakdown"``.""")
    change = _doc(_change, """Per component (all equal): ``sqrt((‖L⁺−L‖² + ‖S⁺−S‖²) / (‖L⁺‖² + ‖S⁺‖²))`` of the last iteration that ran.""")
    history = _doc(_ToeplitzSolver.history, """``[iterations, 3]`` (host, float64): the change, ``‖C(L)‖_*`` and ``‖T S‖₁`` after every iteration.""")

    def __repr__(self):
        i = self.info()
        return (f"ToeplitzLPS on a {self.op.ndim}-dimensional {self.op.Z} operator x {self.op.ntransforms} frames, nuc = {self.nuc:g}, l1 = {self.l1:g}, "
                f"transform = {self.transform!r}, momentum = {self.momentum}, step = {self.step:g}, lam = {self.lam:g}, maxiter = {self.maxiter}, "
                f"tol = {self.tol:g}, check_every = {self.check_every}, {i.workspace_bytes / 1e6:.1f} MB")
