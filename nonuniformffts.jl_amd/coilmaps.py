"""Coil sensitivity maps from low-resolution coil images, above the C ABI's ``nufft_coilmaps_*`` entry points.

    est = CoilMapEstimator(plan_or_op, ncoils, box=5, crop=0.0)
    maps = est.estimate(images, phase=0)        # a tuple of ncoils tensors
    est.crop_maps(maps, 0.1)                    # the crop pass alone, with another level, in place
    est.lambda1, est.lambda2                    # the two largest eigenvalues per cell of the last call
    maps = estimate_maps(plan_or_op, images, box=5, crop=0.05, phase="pca")
    h = calibration_weights(points, cutoff=0.15, window="hann")

The estimate is Walsh, Gmitro & Marcellin's (MRM 2000): at every cell the dominant eigenvector of the ``C × C`` covariance of the coil
values over a box around the cell, normalised to unit length, with the phase fixed by a reference vector.  The box is periodic on the
array as stored, the covariance and the eigen-decomposition are FP64 for both element types.  Plumbing only: the work is the library's.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from ._handle import _HandleObject
from ._lib import lib
from .plan import DimensionMismatch, PlanNUFFT, _check, _ptr_table
from .toeplitz import ToeplitzOperator

_WINDOWS = ("hann", "box")


def _params(ndim: int, box, crop) -> _lib.NufftCoilmapsParams:
    try:
        sides = [box] * ndim if isinstance(box, int) and not isinstance(box, bool) else list(box)
    except TypeError:
        sides = []
    if len(sides) != ndim or any(isinstance(b, bool) or not isinstance(b, int) for b in sides):
        raise ValueError(f"box must be an integer or {ndim} integers (got {box!r})")
    prm = _lib.NufftCoilmapsParams()
    prm.struct_size = C.sizeof(_lib.NufftCoilmapsParams)
    for d in range(3):
        prm.box[d] = sides[d] if d < ndim else 1
    prm.crop = float(crop)
    return prm


class CoilMapEstimator(_HandleObject):
    """``CoilMapEstimator(plan_or_op, ncoils, box=5 | (b1, …, bD), crop=0.0)``: element type, shape and device are those of a complex
    ``PlanNUFFT`` or of a ``ToeplitzOperator`` (neither is kept; their ntransforms plays no part).  ``1 <= ncoils <= 32``; box sides are
    odd, ``1 <= b_d <= min(9, N_d)``.  With ``crop > 0`` the maps are set to exact zeros where ``λ1 < crop² · max λ1``."""

    _prefix, _info = "coilmaps", _lib.NufftCoilmapsInfo

    def __init__(self, plan_or_op, ncoils: int, box=5, crop: float = 0.0):
        if not isinstance(plan_or_op, (PlanNUFFT, ToeplitzOperator)):
            raise ValueError("CoilMapEstimator takes a PlanNUFFT or a ToeplitzOperator")
        if isinstance(ncoils, bool) or not isinstance(ncoils, int):
            raise ValueError(f"ncoils must be an integer (got {ncoils!r})")
        src = plan_or_op
        prm = _params(src.ndim, box, crop)
        self._handle = C.c_void_p()
        if isinstance(src, ToeplitzOperator):
            src._require_open()
            self.Z = src.Z
            _check(lib.nufft_coilmaps_create_for_operator(C.byref(self._handle), src._handle, ncoils, C.byref(prm)))
        else:
            if not src.is_complex:
                raise ValueError("unsupported: the coil map estimate needs a complex plan (the coil images are complex arrays)")
            self.Z = src.eltype
            dims = (C.c_int64 * 3)(*(list(src.shape[::-1]) + [1] * (3 - src.ndim)))
            device = -1 if src.device is None else int(src.device.index or 0)
            dtype = _lib.F32 if self.Z == torch.complex64 else _lib.F64
            _check(lib.nufft_coilmaps_create(C.byref(self._handle), dtype, src.ndim, dims, ncoils, device, C.byref(prm)))
        self.T = torch.float32 if self.Z == torch.complex64 else torch.float64
        self.device, self.shape, self.ndim, self.ncoils = src.device, src.shape, src.ndim, ncoils
        self.box, self.crop = tuple(prm.box[d] for d in range(self.ndim)), float(crop)
        # allocated here, so that estimate() itself allocates nothing but (without ``out``) the maps
        self.lambda1 = torch.empty(self.shape, dtype=self.T, device=self.device)
        self.lambda2 = torch.empty(self.shape, dtype=self.T, device=self.device)

    def _phase(self, phase, images):
        """The reference vector as ncoils (re, im) pairs of doubles, or None for the library's default e_0."""
        if isinstance(phase, str):
            if phase != "pca":
                raise ValueError(f"phase must be a coil index, {self.ncoils} complex numbers or \"pca\" (got {phase!r})")
            # the dominant eigenvector of the global Gram matrix G[c, c'] = Σ_x a_c conj(a_c'): one host synchronisation
            a = torch.stack([u.reshape(-1) for u in images]).to(torch.complex128)
            lam, vec = torch.linalg.eigh((a @ a.conj().T).cpu())
            p = vec[:, -1]
            k = int(torch.argmax(p.abs()))                   # an eigenvector has no phase of its own: its largest entry is made real
            p = p * (p[k].conj() / p[k].abs())
        elif isinstance(phase, int) and not isinstance(phase, bool):
            if not 0 <= phase < self.ncoils:
                raise ValueError(f"phase = {phase} is no coil index (0 ... {self.ncoils - 1})")
            if phase == 0:
                return None
            p = torch.zeros(self.ncoils, dtype=torch.complex128)
            p[phase] = 1.0
        else:
            p = torch.as_tensor(phase).detach().cpu().to(torch.complex128).reshape(-1)
            if p.numel() != self.ncoils:
                raise DimensionMismatch(f"the phase reference has {p.numel()} entries (expected {self.ncoils})")
        flat = torch.view_as_real(p.contiguous()).reshape(-1).tolist()
        return (C.c_double * (2 * self.ncoils))(*flat)

    def estimate(self, images, phase=0, out=None):
        """``images``: a tuple of ncoils tensors of the plan's shape, or a contiguous ``(ncoils, *shape)`` tensor.  ``phase``: a coil
        index (that coil becomes real and non-negative), ncoils complex numbers, or ``"pca"`` (the dominant eigenvector of the global
        Gram matrix of the images, computed with torch: one host synchronisation).  ``out``: a tuple of ncoils tensors, none of them
        overlapping another or an input.  Returns the maps as a tuple of ncoils tensors, each its own 16-byte aligned allocation;
        ``lambda1`` and ``lambda2`` (allocated with the object) hold the two largest eigenvalues per cell afterwards.  Apart from
        ``"pca"`` nothing synchronises.  What this layer allocates per call: the maps when ``out`` is None, and a copy of every input
        that is not 16-byte aligned (every second slice of a stacked ComplexF32 tensor with an odd cell count).  Inside a
        ``torch.cuda.graph`` capture pass ``out`` and aligned inputs, so that the graph holds the library's launches only."""
        self._require_open()
        if isinstance(images, torch.Tensor):
            if images.dim() != self.ndim + 1:
                raise DimensionMismatch(f"wrong dimensions of the coil images (expected tensor shape ({self.ncoils}, {', '.join(map(str, self.shape))}), "
                                        f"got {tuple(images.shape)})")
            if not images.is_contiguous():
                raise ValueError("coil images must be contiguous")
            images = tuple(images[c] for c in range(images.shape[0]))
        else:
            images = tuple(images)
        self._check_arrays(images, "coil image", self.ncoils)
        images = tuple(a if a.data_ptr() % 16 == 0 else a.clone() for a in images)
        if out is None:
            out = tuple(torch.empty(self.shape, dtype=self.Z, device=self.device) for _ in range(self.ncoils))
        else:
            out = tuple(out)
            self._check_arrays(out, "output", self.ncoils)
        p = self._phase(phase, images)
        _check(lib.nufft_coilmaps_estimate(self._handle, _ptr_table(out), _ptr_table(images), p, C.c_void_p(self.lambda1.data_ptr()),
                                           C.c_void_p(self.lambda2.data_ptr()), self._stream()))
        return out

    def crop_maps(self, maps, crop: float):
        """The crop pass alone, in place, with another level: zeros where ``lambda1 < crop² · max λ1`` of the last ``estimate`` of this
        object (``maps``: its result).  Returns ``maps``.  Does not synchronise."""
        self._require_open()
        maps = tuple(maps)
        self._check_arrays(maps, "map", self.ncoils)
        _check(lib.nufft_coilmaps_apply_crop(self._handle, _ptr_table(maps), C.c_void_p(self.lambda1.data_ptr()), float(crop), self._stream()))
        return maps

    def last_sweeps(self) -> int:
        """The largest Jacobi sweep count over the cells of the last ``estimate`` (synchronises the current stream)."""
        self._require_open()
        n = C.c_int32()
        _check(lib.nufft_coilmaps_last_sweeps(self._handle, C.byref(n), self._stream()))
        return n.value

    def __repr__(self):
        i = self.info()
        return (f"CoilMapEstimator box {self.box} on {self.ndim}-dimensional {self.Z} arrays of shape {self.shape} x {self.ncoils} coils, "
                f"tiles of {i.tile_cells} cells ({'staged in LDS' if i.staged else 'neighbours from global memory'}), {i.workgroups} workgroups")


def estimate_maps(plan_or_op, images, box=5, crop: float = 0.0, phase=0):
    """One shot: ``CoilMapEstimator(plan_or_op, len(images), box, crop).estimate(images, phase)``."""
    ncoils = int(images.shape[0]) if isinstance(images, torch.Tensor) else len(images)
    est = CoilMapEstimator(plan_or_op, ncoils, box=box, crop=crop)
    try:
        return est.estimate(images, phase=phase)
    finally:
        est.close()


def calibration_weights(points, cutoff: float = 0.15, window: str = "hann"):
    """Per-sample taper that keeps the centre of k-space, for the low-resolution coil images the estimate starts from.  ``points``: what
    ``set_points`` takes (a tuple of D vectors, one vector, or an ``(Np, D)`` tensor), in radians.  The points are folded to
    ``[−π, π)``; ``r = ‖x‖₂ / π``; ``"hann"``: ``½ (1 + cos(π r / cutoff))`` for ``r < cutoff``, else 0; ``"box"``: 1 for
    ``r <= cutoff``, else 0.  Plain torch; returns a real tensor of Np weights on the points' device."""
    if window not in _WINDOWS:
        raise ValueError(f"window must be one of {_WINDOWS} (got {window!r})")
    if not (cutoff > 0.0 and math.isfinite(cutoff)):
        raise ValueError("cutoff must be positive and finite")
    if isinstance(points, torch.Tensor):
        if points.dim() not in (1, 2):
            raise DimensionMismatch("points must be a vector or an (Np, D) tensor")
        comps = (points,) if points.dim() == 1 else tuple(points[:, d] for d in range(points.shape[1]))
    else:
        comps = tuple(points)
    if not 1 <= len(comps) <= 3:
        raise DimensionMismatch("1, 2 or 3 point components")
    r2 = None
    for x in comps:
        f = torch.remainder(x + math.pi, 2.0 * math.pi) - math.pi
        r2 = f * f if r2 is None else r2 + f * f
    r = torch.sqrt(r2) / math.pi
    if window == "box":
        return (r <= cutoff).to(r.dtype)
    return torch.where(r < cutoff, 0.5 * (1.0 + torch.cos(math.pi * r / cutoff)), torch.zeros_like(r))
