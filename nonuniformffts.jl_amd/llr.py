"""Locally low-rank proximal map, above the C ABI's ``nufft_llr_*`` entry points.

    L = LocallyLowRank(op_or_plan, block=8)
    y, nuc = L.apply(x, t)           # singular-value soft-thresholding of every block's Casorati matrix, and the LLR norm of y

The K = ntransforms arrays are cut into spatial blocks; each block's ``B × K`` matrix has its singular values shrunk by ``t``.  The
kernel diagonalises the ``K × K`` Gram matrix in FP64 on the chip and reads and writes every array once.  Plumbing only.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._handle import _HandleObject
from ._lib import lib
from .plan import DimensionMismatch, PlanNUFFT, _check, _ptr_table
from .toeplitz import ToeplitzOperator


def _llr_params(ndim: int, block, shifts, seed) -> _lib.NufftLlrParams:
    try:
        sides = [block] * ndim if isinstance(block, int) and not isinstance(block, bool) else list(block)
    except TypeError:
        sides = []
    if len(sides) != ndim or any(isinstance(b, bool) or not isinstance(b, int) for b in sides):
        raise ValueError(f"block must be an integer or {ndim} integers (got {block!r})")
    if not isinstance(shifts, (bool, int)) or shifts not in (0, 1, False, True):
        raise ValueError("shifts must be True or False")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be an integer in [0, 2^64)")
    prm = _lib.NufftLlrParams()
    prm.struct_size = C.sizeof(_lib.NufftLlrParams)
    for d in range(3):
        prm.block[d] = sides[d] if d < ndim else 1
    prm.shifts, prm.seed = int(bool(shifts)), seed
    return prm


class LocallyLowRank(_HandleObject):
    """``LocallyLowRank(op_or_plan, block=8 | (b1, …, bD), shifts=False, seed=0)``: element type, shape, ntransforms and device are
    those of a complex ``PlanNUFFT`` or of a ``ToeplitzOperator`` (neither is kept).  Block sides are powers of two, 1 … 16, each
    dividing its ``N_d``, with ``Π b_d · ntransforms <= 8192``.  ``shifts`` and ``seed`` only matter to :class:`ToeplitzFISTA`, which
    draws a new cyclic shift every iteration; ``apply`` takes its shift as an argument.  The map acts on the arrays as stored, periodic
    in the storage index."""

    _prefix, _info = "llr", _lib.NufftLlrInfo

    def __init__(self, op_or_plan, block=8, shifts: bool = False, seed: int = 0):
        if not isinstance(op_or_plan, (PlanNUFFT, ToeplitzOperator)):
            raise ValueError("LocallyLowRank takes a PlanNUFFT or a ToeplitzOperator")
        src = op_or_plan
        prm = _llr_params(src.ndim, block, shifts, seed)
        if isinstance(src, ToeplitzOperator):
            src._require_open()
            create, self.Z = lib.nufft_llr_create_for_operator, src.Z
        else:
            create, self.Z = lib.nufft_llr_create, src.eltype
        self._handle = C.c_void_p()
        _check(create(C.byref(self._handle), src._handle, C.byref(prm)))
        self.device, self.shape, self.ndim, self.ntransforms = src.device, src.shape, src.ndim, src.ntransforms
        self.block, self.shifts, self.seed = tuple(prm.block[d] for d in range(self.ndim)), bool(shifts), seed

    def apply(self, x, t, out=None, shift=None):
        """``out = prox_{t ‖·‖_LLR}(x)``: a tensor of the plan's shape or a tuple of ntransforms such tensors.  ``out`` may be ``x``
        itself (in place).  ``shift``: one cyclic shift per dimension, ``0 <= shift[d] < block[d]`` (None = zero).  Returns
        ``(out, nuc)`` with ``nuc`` a float64 device tensor of one element: the sum over all blocks of the kept singular values."""
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
        sh = None
        if shift is not None:
            vals = [int(v) for v in shift]
            if len(vals) != self.ndim:
                raise DimensionMismatch(f"wrong amount of shifts (expected {self.ndim})")
            sh = (C.c_int32 * self.ndim)(*vals)
        nuc = torch.empty(1, dtype=torch.float64, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _check(lib.nufft_llr_apply(self._handle, _ptr_table(out_t), _ptr_table(x_t), float(t), sh, C.c_void_p(nuc.data_ptr()), stream))
        return out, nuc

    def __repr__(self):
        i = self.info()
        return (f"LocallyLowRank blocks {self.block} on {self.ndim}-dimensional {self.Z} arrays of shape {self.shape} x {self.ntransforms} components, "
                f"{i.blocks} blocks, {i.waves_per_cu} waves per CU")
