"""What the objects that own one handle of the C ABI share: the life of the handle, the current stream, ``info`` and the check of the
arrays they are given.  The C ABI's objects are shaped alike (``nufft_<prefix>_destroy / _get_info``), so a class states its prefix and
its info struct.  (``PlanNUFFT``, ``PlanNUFFT3`` and ``ToeplitzOperator`` live differently and keep their own.)"""
from __future__ import annotations

import ctypes as C

import torch

from ._lib import lib
from .plan import DimensionMismatch, _check


class _HandleObject:
    _prefix = None            # "llr": the entry points are lib.nufft_llr_*
    _info = None              # the info struct of _lib

    def _entry(self, name):
        return getattr(lib, f"nufft_{self._prefix}_{name}")

    def close(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            self._entry("destroy")(h)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _require_open(self):
        if not self._handle.value:
            raise ValueError(f"this {type(self).__name__} has been closed")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def info(self):
        self._require_open()
        out = self._info()
        out.struct_size = C.sizeof(self._info)
        _check(self._entry("get_info")(self._handle, C.byref(out)))
        return out

    def _check_arrays(self, us, what, count=None):
        """``count`` (None: ntransforms) contiguous tensors of the object's shape, element type and device."""
        count = self.ntransforms if count is None else count
        if len(us) != count:
            raise DimensionMismatch(f"wrong amount of {what} arrays (expected a tuple of {count} arrays)")
        for u in us:
            if not isinstance(u, torch.Tensor) or u.device != self.device:
                raise ValueError(f"{what} must be torch tensors on {self.device}")
            if u.dtype != self.Z:
                raise ValueError(f"{what} must have element type {self.Z} (got {u.dtype})")
            if tuple(u.shape) != self.shape:
                raise DimensionMismatch(f"wrong dimensions of {what} array (expected tensor shape {self.shape}, got {tuple(u.shape)})")
            if not u.is_contiguous():
                raise ValueError(f"{what} must be contiguous")
