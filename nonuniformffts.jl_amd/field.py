"""Time segmentation of a field map for off-resonance correction, above the C ABI's ``nufft_fieldseg_*`` entry points.

    fs = FieldSegments(torch.complex64, segments=8, device=dev).fit(omega, times=t)     # or FieldSegments(plan_or_op, 8)
    phi = fs.interpolators(t)                   # (L, Np): φ_l(t_j)
    B = fs.factors(omega)                       # L tensors shaped like omega: exp(−i ω τ_l)
    op = ToeplitzOperator(plan, segments=8).set_points(points, weights, basis=phi).set_factors(B)
    op, fs = field_corrected_operator(plan, points, weights, omega, t, segments=8, maps=S)

The method is the histogram least-squares fit of Sutton, Noll & Fessler (IEEE TMI 2003): ``exp(−i ω t) ≈ Σ_l φ_l(t) exp(−i ω τ_l)`` with
the ``φ_l(t)`` that minimise the error over the histogram of ω.  The histogram is exact (integer counts); the normal matrix, its
Cholesky factor and every sum are FP64 for both element types.  Plumbing only: the work is the library's.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._handle import _HandleObject
from ._lib import lib
from .plan import DimensionMismatch, PlanNUFFT, _check, _ptr_table
from .toeplitz import ToeplitzOperator

_COMPLEX = {torch.complex64: torch.float32, torch.complex128: torch.float64}


def _dptr(m):
    return m.ctypes.data_as(C.POINTER(C.c_double))


class FieldSegments(_HandleObject):
    """``FieldSegments(Z, segments, nbins=256, ridge=1e-8, device=None)`` with ``Z`` ``torch.complex64`` or ``torch.complex128`` (the
    current device when ``device`` is None), or ``FieldSegments(plan_or_op, segments, ...)``: element type and device of a complex
    ``PlanNUFFT`` or of a ``ToeplitzOperator`` (neither is kept).  ``1 <= segments <= 16``, ``1 <= nbins <= 1024``.  ``ridge`` is the
    relative Tikhonov term of the fit, ``(Gm + ridge · tr(Gm) / L · I)``.  The object needs no shape: ω is read as a flat vector."""

    _prefix = "fieldseg"
    _info = _lib.NufftFieldsegInfo

    def __init__(self, Z_or_plan, segments: int, nbins: int = 256, ridge: float = 1e-8, device=None):
        for name, v in (("segments", segments), ("nbins", nbins)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name} must be an integer (got {v!r})")
        src = Z_or_plan
        if isinstance(src, (PlanNUFFT, ToeplitzOperator)):
            if device is not None:
                raise ValueError("device comes from the plan or operator")
            if isinstance(src, ToeplitzOperator):
                src._require_open()
                Z = src.Z
            else:
                if not src.is_complex:
                    raise ValueError("unsupported: the segment fit needs a complex plan (interpolators and factors are complex)")
                Z = src.eltype
            device = src.device
            index = -1 if device is None else int(device.index or 0)
        else:
            if src not in _COMPLEX:
                raise ValueError(f"FieldSegments takes torch.complex64, torch.complex128, a PlanNUFFT or a ToeplitzOperator (got {src!r})")
            Z = src
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            if device.type != "cuda":
                raise ValueError(f"the segment fit runs on the GPU (got device {device})")
            index = torch.cuda.current_device() if device.index is None else int(device.index)
            device = torch.device("cuda", index)
        self._handle = C.c_void_p()
        _check(lib.nufft_fieldseg_create(C.byref(self._handle), _lib.F32 if Z == torch.complex64 else _lib.F64, segments, nbins, index))
        self.Z, self.T, self.device = Z, _COMPLEX[Z], device
        self.segments, self.nbins, self.ridge = segments, nbins, float(ridge)

    def _real_vector(self, x, what):
        if not isinstance(x, torch.Tensor) or x.device != self.device:
            raise ValueError(f"{what} must be a torch tensor on {self.device}")
        if x.dtype != self.T:
            raise ValueError(f"{what} must have element type {self.T} (got {x.dtype})")
        if not x.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
        if x.numel() < 1:
            raise DimensionMismatch(f"{what} is empty")
        return x.reshape(-1)

    @staticmethod
    def uniform_tau(segments: int, t_lo: float, t_hi: float) -> np.ndarray:
        """``segments`` values uniform over ``[t_lo, t_hi]``, both ends included; the midpoint for one segment."""
        if segments == 1:
            return np.array([0.5 * (t_lo + t_hi)], dtype=np.float64)
        return np.linspace(float(t_lo), float(t_hi), segments, dtype=np.float64)

    def fit(self, omega, times=None, t_range=None, mask=None, tau=None, ridge=None):
        """Histogram of ``omega`` (a real tensor of any shape; ``mask``: a bool / uint8 tensor of as many elements, nonzero = counted) and
        the solver matrix for the segment times ``tau``: given, or uniform over ``t_range = (t_lo, t_hi)``, or over the minimum and
        maximum of ``times`` (one host synchronisation more).  Synchronises; not inside a graph capture.  Returns self."""
        self._require_open()
        w = self._real_vector(omega, "the field map")
        m = None
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.device != self.device or mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f"the mask must be a bool or uint8 torch tensor on {self.device}")
            if mask.numel() != w.numel():
                raise DimensionMismatch(f"a mask of {mask.numel()} elements for a field map of {w.numel()}")
            m = mask.reshape(-1).contiguous().view(torch.uint8) if mask.dtype == torch.bool else mask.reshape(-1).contiguous()
        if tau is None:
            if t_range is None:
                if times is None:
                    raise ValueError("fit needs tau, t_range or times")
                t = self._real_vector(times, "the times")
                t_range = (float(t.min()), float(t.max()))
            tau = self.uniform_tau(self.segments, float(t_range[0]), float(t_range[1]))
        tau = np.ascontiguousarray(tau, dtype=np.float64).reshape(-1)
        if tau.shape[0] != self.segments:
            raise DimensionMismatch(f"{tau.shape[0]} segment times for {self.segments} segments")
        r = self.ridge if ridge is None else float(ridge)
        _check(lib.nufft_fieldseg_fit(self._handle, C.c_void_p(w.data_ptr()), C.c_void_p(m.data_ptr() if m is not None else None), w.numel(),
                                      _dptr(tau), r, self._stream()))
        return self

    # ---- the two kernels of the reconstruction: neither synchronises ---------------------------------------------------------------
    def interpolators(self, times, out=None):
        """``φ_l(t_j)`` as a contiguous ``(segments, Np)`` complex tensor (``out``: such a tensor), which
        ``ToeplitzOperator.set_points(..., basis=)`` takes.  A row that is not 16-byte aligned (ComplexF32, odd Np) is written through an
        aligned temporary: inside a ``torch.cuda.graph`` capture pass ``out`` with an even Np."""
        self._require_open()
        t = self._real_vector(times, "the times")
        n, L = t.numel(), self.segments
        if out is None:
            out = torch.empty((L, n), dtype=self.Z, device=self.device)
        elif not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != self.Z or tuple(out.shape) != (L, n) or not out.is_contiguous():
            raise DimensionMismatch(f"out must be a contiguous {self.Z} tensor of shape ({L}, {n}) on {self.device}")
        rows = tuple(out[l] for l in range(L))
        work = tuple(r if r.data_ptr() % 16 == 0 else torch.empty_like(r) for r in rows)     # ComplexF32 rows of odd length
        _check(lib.nufft_fieldseg_interpolators(self._handle, C.c_void_p(t.data_ptr()), n, _ptr_table(work), self._stream()))
        for r, w in zip(rows, work):
            if r is not w:
                r.copy_(w)
        return out

    def factors(self, omega, out=None):
        """``B_l = exp(−i ω τ_l)`` with the τ of the last fit: a tuple of ``segments`` separate tensors shaped like ``omega`` (``out``: such
        a tuple), which ``ToeplitzOperator.set_factors`` takes without a copy."""
        self._require_open()
        w = self._real_vector(omega, "the field map")
        if out is None:
            out = tuple(torch.empty(omega.shape, dtype=self.Z, device=self.device) for _ in range(self.segments))
        else:
            out = tuple(out)
            if len(out) != self.segments:
                raise DimensionMismatch(f"wrong amount of factors (expected a tuple of {self.segments})")
            for b in out:
                if not isinstance(b, torch.Tensor) or b.device != self.device or b.dtype != self.Z or b.shape != omega.shape or not b.is_contiguous():
                    raise ValueError(f"every factor must be a contiguous {self.Z} tensor shaped like the field map on {self.device}")
        _check(lib.nufft_fieldseg_factors(self._handle, C.c_void_p(w.data_ptr()), w.numel(), _ptr_table(out), self._stream()))
        return out

    # ---- host reads: each synchronises the current stream --------------------------------------------------------------------------
    def histogram(self):
        """(counts as uint32, centres as float64) of the bins in use: ``nbins``, or one bin for a constant field map."""
        self._require_open()
        nb = max(1, int(self.info().bins_used))
        counts, centres = np.zeros(nb, dtype=np.uint32), np.zeros(nb, dtype=np.float64)
        _check(lib.nufft_fieldseg_get_histogram(self._handle, counts.ctypes.data_as(C.POINTER(C.c_uint32)), _dptr(centres), self._stream()))
        return counts, centres

    @property
    def centres(self) -> np.ndarray:
        return self.histogram()[1]

    def gram(self) -> np.ndarray:
        """``Gm[l, l'] = Σ_b h_b exp(−i ω_b (τ_l' − τ_l))`` as complex128 (without the ridge)."""
        self._require_open()
        m = np.empty((self.segments, self.segments), dtype=np.complex128)
        _check(lib.nufft_fieldseg_get_gram(self._handle, _dptr(m), self._stream()))
        return m

    def solver_matrix(self) -> np.ndarray:
        """``P = (Gm + ridge · tr(Gm) / L · I)⁻¹`` as complex128."""
        self._require_open()
        m = np.empty((self.segments, self.segments), dtype=np.complex128)
        _check(lib.nufft_fieldseg_get_solver_matrix(self._handle, _dptr(m), self._stream()))
        return m

    @property
    def tau(self) -> np.ndarray:
        self._require_open()
        m = np.empty(self.segments, dtype=np.float64)
        _check(lib.nufft_fieldseg_get_tau(self._handle, _dptr(m), self._stream()))
        return m

    def __repr__(self):
        i = self.info()
        return (f"FieldSegments of {self.segments} segments, {self.nbins} bins, {self.Z} on {self.device}: "
                f"{'fitted on ' + str(i.bins_used) + ' bins' if i.bins_used else 'not fitted'}")


def field_corrected_operator(plan, points, weights, omega, times, segments: int, maps=None, nbins: int = 256, ridge: float = 1e-8,
                             t_range=None, mask=None, **build):
    """The segmented operator of ``plan`` (complex, ``ntransforms == 1``) for the field map ``omega`` (a real tensor of ``plan.shape``) and
    the sample times ``times`` (a real vector, one per point): fit, interpolators, factors, ``set_points(points, weights, basis=phi)``,
    ``set_factors`` and, with ``maps``, ``set_maps``.  ``build``: the window overrides of ``set_points``.  Returns ``(op, fs)``: the
    operator keeps the factors alive, ``fs`` is the fitted ``FieldSegments`` (its ``interpolators(times)`` and ``factors(omega)`` are what
    the right-hand side needs)."""
    op = ToeplitzOperator(plan, segments=segments)
    try:
        if tuple(omega.shape) != tuple(op.shape):
            raise DimensionMismatch(f"wrong dimensions of the field map (expected tensor shape {op.shape}, got {tuple(omega.shape)})")
        fs = FieldSegments(op, segments, nbins=nbins, ridge=ridge)
        fs.fit(omega, times=times, t_range=t_range, mask=mask)
        phi = fs.interpolators(times)
        op.set_points(points, weights, basis=phi, **build)
        op.set_factors(fs.factors(omega))
        if maps is not None:
            op.set_maps(maps)
    except Exception:
        op.close()
        raise
    return op, fs
