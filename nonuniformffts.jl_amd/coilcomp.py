"""Coil compression and noise pre-whitening, above the C ABI's ``nufft_coilcomp_*`` entry points.

    cc = CoilCompressor(torch.complex64, ncoils=32, device=dev)     # or CoilCompressor(plan_or_op, ncoils)
    cc.fit(y, weights=h, noise=noise_scan)      # y: a tuple of C vectors, or a list of such tuples (frames) with a matching list of weights
    V = cc.choose(energy=0.98)                  # the smallest V with Σ_{v<V} λ_v >= energy · Σ λ
    yv = cc.apply(y, V)                         # V vectors; the same call compresses coil images or maps of any shape
    cc.eigenvalues, cc.matrix(V), cc.gram(), cc.last_sweeps()
    yv = compress_coils(y, nvirtual=8, weights=h)

The method is the principal-component compression of Huang et al. (MRI 2008) and Buehrer et al. (MRM 2007): the eigenvectors of the
``C × C`` coil covariance, the largest eigenvalues first; with a noise covariance the whitening ``Ψ = L Lᴴ``, ``W = L⁻¹`` is folded into
the same matrix ``A = Uᴴ W``.  Sums and the eigen-decomposition are FP64 for both element types.  Plumbing only: the work is the library's.
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


def _host_matrix(a, rows, cols, what):
    m = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.complex128)
    if m.shape != (rows, cols):
        raise DimensionMismatch(f"{what} must be a {rows} x {cols} matrix (got shape {m.shape})")
    return m


def _dptr(m):
    return m.ctypes.data_as(C.POINTER(C.c_double))


class CoilCompressor(_HandleObject):
    """``CoilCompressor(Z, ncoils, device=None)`` with ``Z`` ``torch.complex64`` or ``torch.complex128`` (the current device when
    ``device`` is None), or ``CoilCompressor(plan_or_op, ncoils)``: element type and device of a complex ``PlanNUFFT`` or of a
    ``ToeplitzOperator`` (neither is kept).  ``1 <= ncoils <= 64``.  The object needs no shape: every call takes tensors of any shape,
    which are read as flat vectors."""

    _prefix = "coilcomp"

    def __init__(self, Z_or_plan, ncoils: int, device=None):
        if isinstance(ncoils, bool) or not isinstance(ncoils, int):
            raise ValueError(f"ncoils must be an integer (got {ncoils!r})")
        src = Z_or_plan
        if isinstance(src, (PlanNUFFT, ToeplitzOperator)):
            if device is not None:
                raise ValueError("device comes from the plan or operator")
            if isinstance(src, ToeplitzOperator):
                src._require_open()
                Z = src.Z
            else:
                if not src.is_complex:
                    raise ValueError("unsupported: coil compression needs a complex plan (the coil data are complex vectors)")
                Z = src.eltype
            device = src.device
            index = -1 if device is None else int(device.index or 0)
        else:
            if src not in _COMPLEX:
                raise ValueError(f"CoilCompressor takes torch.complex64, torch.complex128, a PlanNUFFT or a ToeplitzOperator (got {src!r})")
            Z = src
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            if device.type != "cuda":
                raise ValueError(f"coil compression runs on the GPU (got device {device})")
            index = torch.cuda.current_device() if device.index is None else int(device.index)
            device = torch.device("cuda", index)
        self._handle = C.c_void_p()
        _check(lib.nufft_coilcomp_create(C.byref(self._handle), _lib.F32 if Z == torch.complex64 else _lib.F64, ncoils, index))
        self.Z, self.T, self.device, self.ncoils = Z, _COMPLEX[Z], device, ncoils

    def info(self, n: int = 1) -> _lib.NufftCoilcompInfo:
        """Static facts, and the tiling of an ``accumulate`` of vectors of ``n`` elements."""
        self._require_open()
        out = _lib.NufftCoilcompInfo()
        out.struct_size = C.sizeof(_lib.NufftCoilcompInfo)
        _check(lib.nufft_coilcomp_get_info(self._handle, int(n), C.byref(out)))
        return out

    def _vectors(self, us, count, what):
        """Flat views of ``count`` tensors of one length; a copy only of those that are not 16-byte aligned."""
        us = tuple(us[c] for c in range(us.shape[0])) if isinstance(us, torch.Tensor) else tuple(us)
        if len(us) != count:
            raise DimensionMismatch(f"wrong amount of {what} vectors (expected a tuple of {count})")
        flat = []
        for u in us:
            if not isinstance(u, torch.Tensor) or u.device != self.device:
                raise ValueError(f"{what} vectors must be torch tensors on {self.device}")
            if u.dtype != self.Z:
                raise ValueError(f"{what} vectors must have element type {self.Z} (got {u.dtype})")
            if not u.is_contiguous():
                raise ValueError(f"{what} vectors must be contiguous")
            if u.numel() != us[0].numel():
                raise DimensionMismatch(f"{what} vectors of unequal length ({u.numel()} and {us[0].numel()})")
            flat.append(u.reshape(-1))
        if flat[0].numel() < 1:
            raise DimensionMismatch(f"empty {what} vectors")
        return us, flat

    # ---- the stages, none of which synchronises --------------------------------------------------------------------------------
    def reset(self):
        self._require_open()
        _check(lib.nufft_coilcomp_reset(self._handle, self._stream()))

    def accumulate(self, y, weights=None):
        """Adds the weighted Gram matrix of the ``ncoils`` vectors ``y`` to ``R``.  ``weights``: a real tensor of as many elements,
        non-negative (not checked on the device: a negative weight is subtracted, a non-finite one spoils ``R``)."""
        self._require_open()
        _, flat = self._vectors(y, self.ncoils, "data")
        flat = [v if v.data_ptr() % 16 == 0 else v.clone() for v in flat]
        n, w = flat[0].numel(), None
        if weights is not None:
            if not isinstance(weights, torch.Tensor) or weights.device != self.device or weights.is_complex():
                raise ValueError(f"weights must be a real torch tensor on {self.device}")
            if weights.numel() != n:
                raise DimensionMismatch(f"{weights.numel()} weights for vectors of {n} elements")
            w = weights.reshape(-1).to(self.T).contiguous()
        _check(lib.nufft_coilcomp_accumulate(self._handle, _ptr_table(flat), C.c_void_p(w.data_ptr() if w is not None else None), n, self._stream()))

    def finish(self):
        self._require_open()
        _check(lib.nufft_coilcomp_finish(self._handle, self._stream()))

    def set_noise_covariance(self, psi):
        """``psi``: a ``C × C`` Hermitian positive definite matrix (numpy or torch), or None for no whitening.  Factored on the host in
        FP64; synchronises.  Takes effect at the next ``finish``."""
        self._require_open()
        if psi is None:
            _check(lib.nufft_coilcomp_set_noise_covariance(self._handle, None, self._stream()))
            return
        m = _host_matrix(psi, self.ncoils, self.ncoils, "the noise covariance")
        _check(lib.nufft_coilcomp_set_noise_covariance(self._handle, _dptr(m), self._stream()))

    def set_matrix(self, A):
        """Installs a caller's ``rows × C`` matrix (``1 <= rows <= C``) as the one ``apply`` uses; synchronises."""
        self._require_open()
        a = np.asarray(A.detach().cpu().numpy() if isinstance(A, torch.Tensor) else A)
        if a.ndim != 2:
            raise DimensionMismatch(f"the matrix must have two dimensions (got shape {a.shape})")
        m = _host_matrix(a, a.shape[0], self.ncoils, "the matrix")
        _check(lib.nufft_coilcomp_set_matrix(self._handle, _dptr(m), m.shape[0], self._stream()))

    def fit(self, y, weights=None, noise=None):
        """``reset``, one ``accumulate`` per set, ``finish``.  ``y``: a tuple of C vectors, or a list of such tuples (the frames of a
        series, several scans) with ``weights`` None, one tensor for all (equal lengths) or a matching list.  ``noise``: a ``C × C``
        covariance Ψ, or a tuple of C noise vectors (Ψ = their Gram matrix / n, formed by this object: one host synchronisation);
        None keeps what ``set_noise_covariance`` set.  Returns self."""
        self._require_open()
        sets = list(y) if isinstance(y, list) and y and not isinstance(y[0], torch.Tensor) else [y]
        ws = list(weights) if isinstance(weights, (list, tuple)) else [weights] * len(sets)
        if len(ws) != len(sets):
            raise DimensionMismatch(f"{len(ws)} weight vectors for {len(sets)} sets")
        if noise is not None:
            if isinstance(noise, (tuple, list)):
                _, flat = self._vectors(noise, self.ncoils, "noise")
                self.reset()
                self.accumulate(noise)
                noise = self.gram() / flat[0].numel()
            self.set_noise_covariance(noise)
        self.reset()
        for s, w in zip(sets, ws):
            self.accumulate(s, w)
        self.finish()
        return self

    def apply(self, x, nvirtual: int, out=None):
        """``out_v = Σ_c A[v, c] x_c`` for ``v < nvirtual``: a tuple of ``nvirtual`` tensors of the inputs' shape.  ``out``: a tuple of
        ``nvirtual`` tensors, none of them overlapping another or an input.  Allocates the outputs when ``out`` is None, and a copy of
        every input that is not 16-byte aligned; inside a ``torch.cuda.graph`` capture pass ``out`` and aligned inputs."""
        self._require_open()
        if isinstance(nvirtual, bool) or not isinstance(nvirtual, int):
            raise ValueError(f"nvirtual must be an integer (got {nvirtual!r})")
        xs, flat = self._vectors(x, self.ncoils, "input")
        flat = [v if v.data_ptr() % 16 == 0 else v.clone() for v in flat]
        if not 1 <= nvirtual <= self.ncoils:
            raise ValueError(f"nvirtual = {nvirtual} must be 1 ... {self.ncoils}")
        if out is None:
            out = tuple(torch.empty(xs[0].shape, dtype=self.Z, device=self.device) for _ in range(nvirtual))
            oflat = [o.reshape(-1) for o in out]
        else:
            out, oflat = self._vectors(out, nvirtual, "output")
            if oflat[0].numel() != flat[0].numel():
                raise DimensionMismatch(f"outputs of {oflat[0].numel()} elements for inputs of {flat[0].numel()}")
        _check(lib.nufft_coilcomp_apply(self._handle, _ptr_table(oflat), nvirtual, _ptr_table(flat), flat[0].numel(), self._stream()))
        return out

    # ---- host reads: each synchronises the current stream -----------------------------------------------------------------------
    def gram(self) -> np.ndarray:
        self._require_open()
        m = np.empty((self.ncoils, self.ncoils), dtype=np.complex128)
        _check(lib.nufft_coilcomp_get_gram(self._handle, _dptr(m), self._stream()))
        return m

    def matrix(self, nvirtual=None) -> np.ndarray:
        """The first ``nvirtual`` rows of ``A`` (all C by default) as complex128."""
        self._require_open()
        m = np.empty((self.ncoils, self.ncoils), dtype=np.complex128)
        _check(lib.nufft_coilcomp_get_matrix(self._handle, _dptr(m), self._stream()))
        return m if nvirtual is None else m[:int(nvirtual)].copy()

    def spectrum(self):
        """(λ as C doubles, the Jacobi's sweep count, the status word) of the last ``finish``."""
        self._require_open()
        lam = np.empty(self.ncoils, dtype=np.float64)
        sweeps, status = C.c_int32(), C.c_int32()
        _check(lib.nufft_coilcomp_get_spectrum(self._handle, _dptr(lam), C.byref(sweeps), C.byref(status), self._stream()))
        return lam, sweeps.value, status.value

    @property
    def eigenvalues(self) -> np.ndarray:
        return self.spectrum()[0]

    def last_sweeps(self) -> int:
        return self.spectrum()[1]

    def choose(self, energy: float = 0.98) -> int:
        """The smallest V with ``Σ_{v<V} λ_v >= energy · Σ λ`` (one host synchronisation); refuses a zero trace."""
        if not 0.0 < energy <= 1.0:
            raise ValueError(f"energy = {energy} must be in (0, 1]")
        lam = np.maximum(self.eigenvalues, 0.0)
        total = float(lam.sum())
        if not total > 0.0 or not np.isfinite(total):
            raise ValueError("the eigenvalues sum to zero (or are not finite): nothing to choose from")
        return min(self.ncoils, int(np.searchsorted(np.cumsum(lam), energy * total, side="left")) + 1)

    def __repr__(self):
        i = self.info()
        return (f"CoilCompressor of {self.ncoils} coils of {self.Z} on {self.device}: matrix of {i.matrix_rows} rows, "
                f"{'whitened' if i.has_noise else 'not whitened'}")


def compress_coils(y, nvirtual: int, weights=None, noise=None):
    """One shot: fit on ``y`` (a tuple of C vectors on one device) and return its ``nvirtual`` virtual coils."""
    y = tuple(y[c] for c in range(y.shape[0])) if isinstance(y, torch.Tensor) else tuple(y)
    if not y or not isinstance(y[0], torch.Tensor):
        raise ValueError("compress_coils takes a tuple of torch tensors")
    cc = CoilCompressor(y[0].dtype, len(y), device=y[0].device)
    try:
        return cc.fit(y, weights=weights, noise=noise).apply(y, nvirtual)
    finally:
        cc.close()
