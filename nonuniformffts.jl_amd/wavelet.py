"""Periodic orthogonal wavelet transform with its proximal map, above the C ABI's ``nufft_wavelet_*`` entry points.

    W = WaveletTransform(op_or_plan, wavelet="db2", levels=3)
    c = W.forward(x)                 # Mallat layout, the shape of x
    x = W.inverse(c)
    c, l1 = W.shrink(x, t)           # forward with the detail coefficients soft-thresholded on store, and Σ|detail| per component

``W.inverse(W.shrink(x, t)[0])`` is the proximal map of ``t ‖D W x‖₁``; with ``op.solve(..., lam=ρ, x0=x)`` as the x-update it
composes ADMM.  Plumbing only: every array operation runs in the library.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._handle import _HandleObject
from ._lib import lib
from .plan import DimensionMismatch, PlanNUFFT, _check, _ptr_table
from .toeplitz import ToeplitzOperator


def _wavelet_id(wavelet) -> int:
    if wavelet not in _lib.WAVELET_IDS:
        raise ValueError(f'wavelet must be one of {sorted(_lib.WAVELET_IDS)} (got {wavelet!r})')
    return _lib.WAVELET_IDS[wavelet]


class WaveletTransform(_HandleObject):
    """``WaveletTransform(op_or_plan, wavelet="haar" | "db2", levels=L)``: element type, shape, ntransforms and device are those of a
    complex ``PlanNUFFT`` or of a ``ToeplitzOperator`` (neither is kept).  Every ``N_d`` must be a multiple of ``2^L``, and for
    ``"db2"`` ``N_d / 2^L >= 2``.  The transform acts on the array as stored, periodic in the storage index; it commutes with cyclic
    shifts by multiples of ``2^L``, so ``fftshift=True`` and ``False`` plans give the same prox whenever ``2^(L+1)`` divides every
    ``N_d``."""

    _prefix, _info = "wavelet", _lib.NufftWaveletInfo

    def __init__(self, op_or_plan, wavelet: str = "haar", levels: int = 1):
        if not isinstance(op_or_plan, (PlanNUFFT, ToeplitzOperator)):
            raise ValueError("WaveletTransform takes a PlanNUFFT or a ToeplitzOperator")
        if isinstance(levels, bool) or not isinstance(levels, int):
            raise ValueError("levels must be an integer")
        prm = _lib.NufftWaveletParams()
        prm.struct_size = C.sizeof(_lib.NufftWaveletParams)
        prm.wavelet, prm.levels = _wavelet_id(wavelet), levels
        src = op_or_plan
        if isinstance(src, ToeplitzOperator):
            src._require_open()
            create, self.Z = lib.nufft_wavelet_create_for_operator, src.Z
        else:
            create, self.Z = lib.nufft_wavelet_create, src.eltype
        self._handle = C.c_void_p()
        _check(create(C.byref(self._handle), src._handle, C.byref(prm)))
        self.device, self.shape, self.ndim, self.ntransforms = src.device, src.shape, src.ndim, src.ntransforms
        self.wavelet, self.levels = wavelet, levels

    def _io(self, x, out):
        self._require_open()
        single = isinstance(x, torch.Tensor)
        x_t = (x,) if single else tuple(x)
        self._check_arrays(x_t, "input")
        if out is None:
            out_t = tuple(torch.empty_like(v) for v in x_t)
            out = out_t[0] if single else out_t
        else:
            out_t = (out,) if isinstance(out, torch.Tensor) else tuple(out)
            self._check_arrays(out_t, "output")
            if any(o.data_ptr() == v.data_ptr() for o in out_t for v in x_t):
                raise ValueError("the output must not be the input: a level reads its sub-box while other tiles store into it")
        return x_t, out_t, out

    def forward(self, x, out=None):
        """``out = W x`` for every component (a tensor of the plan's shape or a tuple of ntransforms such tensors).  Returns ``out``."""
        x_t, out_t, out = self._io(x, out)
        _check(lib.nufft_wavelet_forward(self._handle, _ptr_table(out_t), _ptr_table(x_t), self._stream()))
        return out

    def inverse(self, c, out=None):
        """``out = Wᴴ c``.  Returns ``out``."""
        c_t, out_t, out = self._io(c, out)
        _check(lib.nufft_wavelet_inverse(self._handle, _ptr_table(out_t), _ptr_table(c_t), self._stream()))
        return out

    def shrink(self, x, t, out=None):
        """``forward`` whose detail coefficients are soft-thresholded where they are stored: ``c · max(1 − t/|c|, 0)``; the coarsest
        approximation band is never thresholded.  ``t``: a scalar or one value per component.  Returns ``(out, l1)`` with ``l1`` a
        float64 device tensor of ``Σ|shrunk detail|`` per component."""
        x_t, out_t, out = self._io(x, out)
        ts = [float(t)] * self.ntransforms if isinstance(t, (int, float)) else [float(v) for v in t]
        if len(ts) != self.ntransforms:
            raise DimensionMismatch(f"wrong amount of thresholds (expected {self.ntransforms})")
        l1 = torch.empty(self.ntransforms, dtype=torch.float64, device=self.device)
        _check(lib.nufft_wavelet_shrink(self._handle, _ptr_table(out_t), _ptr_table(x_t), (C.c_double * len(ts))(*ts),
                                        C.c_void_p(l1.data_ptr()), self._stream()))
        return out, l1

    def __repr__(self):
        i = self.info()
        return (f"WaveletTransform {self.wavelet!r}, {self.levels} levels, on {self.ndim}-dimensional {self.Z} arrays of shape {self.shape}, "
                f"{i.workspace_bytes / 1e6:.1f} MB")
