"""T. Chan's optimal circulant preconditioner of a :class:`ToeplitzOperator`, above the C ABI's ``nufft_precond_*`` entry points.

``G`` is multi-level Toeplitz, so the circulant ``C`` closest to it in the Frobenius norm has its eigenvalues ``e`` in the DFT basis of size
N (not 2N), and they follow from the operator's own multiplier — the points are not needed again.  The object applies

    M⁻¹ r = d ⊙ F⁻¹( m ⊙ F( d ⊙ r ) ),      m = 1 / max(e + μ, floor · max(e + μ))

(DESIGN.md §21).  On a coupled operator (``op.set_points(..., basis=)`` / ``op.set_spectra``) ``block=True`` builds the block-circulant
preconditioner of the K × K block system: per mode ``q`` the Hermitian matrix ``E(q)`` of the blocks' optimal circulants, and

    (M⁻¹ r)_a = d ⊙ F⁻¹( Σ_b B_ab ⊙ F( d ⊙ r_b ) ),      B(q) = (E(q) + shift I)⁻¹ / n,   shift = max(μ, floor · (max_{q,a} E_aa(q) + μ)).

Plumbing only: every array operation runs in the library.

    pc = ToeplitzPreconditioner(op, lam=lam)
    x = op.solve(b, lam=lam, rtol=1e-6, maxiter=200, precond=pc)
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._handle import _HandleObject
from ._lib import lib
from .plan import _check, _ptr_table, DimensionMismatch
from .toeplitz import ToeplitzOperator

_PATHS = {_lib.PRECOND_PATH_DENSE: "dense", _lib.PRECOND_PATH_FUSED: "fused"}


class ToeplitzPreconditioner(_HandleObject):
    """``ToeplitzPreconditioner(op, lam=0.0, floor=1e-6)``: built from the multiplier ``op`` holds now (``op.set_points`` /
    ``set_spectrum`` first); ``update()`` rebuilds it after the operator's spectrum or coil maps changed.  ``lam`` is the λ of the system
    ``(G + λ I)`` it preconditions.  With coil maps set on ``op`` the scaling ``d = (Σ_c |S_c|²)^(-1/2)`` is computed and owned here and
    ``μ = λ / mean(Σ_c |S_c|²)``; ``set_scaling(d)`` passes another ``d``.  A coupled operator (``basis=``) takes ``block=True`` — the
    components are then ONE vector: ``apply`` takes and returns a tuple of K arrays, ``block(a, b)`` returns ``B_ab``, ``floor`` is a shift
    of every cell's eigenvalues instead of a clamp, and ``floored_cells`` counts the cells whose Cholesky pivot had to be floored (round-off
    in ``E``; 0 on any reasonable system) — and is refused with ``block=False``, as an uncoupled one is with ``block=True``.

    ``path`` is ``"fused"`` (2-D and 3-D shapes whose every ``N_d`` is one of the library's line lengths 64 … 1024) or ``"dense"``
    (rocFFT); it does not depend on the operator's own path — a 48 × 40 operator is fused while its preconditioner is dense.  Building
    allocates temporaries and synchronises (not inside ``torch.cuda.graph``); ``apply`` allocates nothing and is capturable.  The object
    keeps ``op`` alive."""

    _prefix, _info = "precond", _lib.NufftPrecondInfo

    def __init__(self, op: ToeplitzOperator, lam: float = 0.0, floor: float = 1e-6, block: bool = False):
        if not isinstance(op, ToeplitzOperator):
            raise ValueError("ToeplitzPreconditioner takes a ToeplitzOperator")
        op._require_open()
        prm = _lib.NufftPrecondParams()
        prm.struct_size = C.sizeof(_lib.NufftPrecondParams)
        prm.lambda_, prm.floor = float(lam), float(floor)
        self._handle = C.c_void_p()
        self._d = None
        if op.device is not None:
            torch.cuda.current_stream(op.device).synchronize()      # the build runs on the default stream
        create = lib.nufft_precond_create_block if block else lib.nufft_precond_create
        _check(create(C.byref(self._handle), op._handle, C.byref(prm)))
        self.op = op
        self.lam, self.floor = float(lam), float(floor)

    def close(self):
        super().close()
        self._d = None

    def _require_open(self):
        super()._require_open()
        if not self.op._handle.value:
            raise ValueError("the ToeplitzOperator of this preconditioner has been closed: the operator must outlive it")

    @property
    def path(self) -> str:
        return _PATHS[self.info().path]

    @property
    def coupled(self) -> int:
        """K for a block preconditioner (``block=True``), else 0."""
        self._require_open()
        return int(lib.nufft_precond_num_coupled(self._handle))

    @property
    def floored_cells(self) -> int:
        """Cells of the last build whose Cholesky pivot was floored (a block preconditioner; 0 otherwise)."""
        self._require_open()
        return int(lib.nufft_precond_floored_cells(self._handle))

    def update(self) -> "ToeplitzPreconditioner":
        """Rebuilds ``m`` — a block preconditioner: ``B`` — (and the scaling from coil maps) from what the operator holds now."""
        self._require_open()
        _check(lib.nufft_precond_update(self._handle, self.op._stream()))
        if self.info().scaling != _lib.PRECOND_SCALING_CALLER:
            self._d = None
        return self

    def set_scaling(self, d: Optional[torch.Tensor]) -> "ToeplitzPreconditioner":
        """``d``: a real positive tensor of ``plan.shape`` with the operator's accuracy (borrowed: this object keeps a reference and its
        values must not change while it is set); ``None``: no scaling."""
        self._require_open()
        op = self.op
        if d is None:
            _check(lib.nufft_precond_set_scaling(self._handle, None))
            self._d = None
            return self
        if not isinstance(d, torch.Tensor) or d.device != op.device:
            raise ValueError(f"the scaling must be a torch tensor on {op.device}")
        if d.dtype != op.T:
            raise ValueError(f"the scaling must be real with the operator's accuracy ({op.T}; got {d.dtype})")
        if tuple(d.shape) != tuple(op.shape):
            raise DimensionMismatch(f"wrong dimensions of the scaling (expected tensor shape {tuple(op.shape)}, got {tuple(d.shape)})")
        if not d.is_contiguous():
            raise ValueError("the scaling must be contiguous")
        if d.data_ptr() % 16:
            d = d.clone()
        _check(lib.nufft_precond_set_scaling(self._handle, C.c_void_p(d.data_ptr())))
        self._d = d
        return self

    def apply(self, r, out=None):
        """``out = M⁻¹ r`` for every component; ``r``: a tensor of ``plan.shape`` or a tuple of ntransforms such tensors; ``out`` may
        be ``r``.  A block preconditioner takes the tuple of its K components as one vector.  Returns ``out``."""
        self._require_open()
        op = self.op
        single = isinstance(r, torch.Tensor)
        r_t = (r,) if single else tuple(r)
        op._check_uniform(r_t, "input")
        if out is None:
            out_t = tuple(torch.empty_like(v) for v in r_t)
            out = out_t[0] if single else out_t
        else:
            out_t = (out,) if isinstance(out, torch.Tensor) else tuple(out)
            op._check_uniform(out_t, "output")
        _check(lib.nufft_precond_apply(self._handle, _ptr_table(out_t), _ptr_table(r_t), op._stream()))
        return out

    __call__ = apply

    def _view(self, ptr, nbytes, real=True):
        shape = tuple(self.op.shape)
        typestr = ("<f4" if self.op.T == torch.float32 else "<f8") if real else ("<c8" if self.op.T == torch.float32 else "<c16")

        class _View:       # the array-interface protocol: torch wraps the pointer without copying
            __cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr.value), False), "version": 2, "strides": None}

        t = torch.as_tensor(_View(), device=self.op.device)
        assert t.numel() * t.element_size() == nbytes.value
        return t

    def multiplier(self) -> torch.Tensor:
        """``m`` (shape ``plan.shape``, real, ``1 / Π N_d`` folded in): a view of the device array, rewritten by ``update()``."""
        self._require_open()
        ptr, nbytes = C.c_void_p(), C.c_int64()
        _check(lib.nufft_precond_multiplier_ptr(self._handle, C.byref(ptr), C.byref(nbytes)))
        return self._view(ptr, nbytes)

    def block(self, a: int, b: int) -> torch.Tensor:
        """``B_ab`` of a block preconditioner (shape ``plan.shape``, ``1 / Π N_d`` folded in): a real view for ``a == b``, a complex view
        for ``a < b`` (``B_ba = conj(B_ab)``: ``a > b`` raises), rewritten by ``update()``."""
        self._require_open()
        ptr, nbytes = C.c_void_p(), C.c_int64()
        _check(lib.nufft_precond_block_ptr(self._handle, int(a), int(b), C.byref(ptr), C.byref(nbytes)))
        return self._view(ptr, nbytes, real=a == b)

    def scaling(self) -> Optional[torch.Tensor]:
        """The scaling ``d`` in force (a view; ``None``: no scaling)."""
        self._require_open()
        ptr, nbytes = C.c_void_p(), C.c_int64()
        _check(lib.nufft_precond_scaling_ptr(self._handle, C.byref(ptr), C.byref(nbytes)))
        return self._view(ptr, nbytes) if ptr.value else None

    def __repr__(self):
        i = self.info()
        return (f"{'Block ' if self.coupled else ''}ToeplitzPreconditioner of a {self.op.ndim}-dimensional {self.op.Z} operator, {self.path} path, lam = {self.lam:g}, "
                f"mu = {i.mu:g}, floor = {self.floor:g}, e in [{i.min_e:g}, {i.max_e:g}], {i.workspace_bytes / 1e6:.1f} MB")
