"""Type-3 (nonuniform-to-nonuniform) transforms above the C ABI's type-3 entry points (include/nufft_mi355x.h).

    f_k = Σ_j c_j exp(sign i s_k · x_j),   x_j ∈ R^D (sources),  s_k ∈ R^D (targets),  sign = -1 by default

``PlanNUFFT3`` owns the plan; ``set_points3(p, xs, ss)`` sets sources and targets, ``exec_type3(f, p, c)`` computes ``f`` from ``c``.
NonuniformFFTs.jl has no type 3: this is a capability of the engine, not a mirror of a reference function.  The declared boxes
(``source_bounds`` / ``target_bounds``, or ``PlanNUFFT3.from_points``) set the fine grid; results for points outside them are undefined,
``points_outside()`` counts such points.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional, Sequence, Tuple, Union

import torch

from . import _lib
from ._lib import lib
from .plan import (_HARNESS_ENV, _KERNEL_IDS, _REAL, _check, _ptr_table, _to_torch_dtype, Direct, DimensionMismatch,
                   FastApproximation, GaussianKernel, HalfSupport, ROCBackend, default_kernel, default_kernel_evalmode)

_ENGINES_SPREAD = {1: "lds_tiles", 2: "mfma_patches", 3: "marching_ring", 4: "marching_ring_dense"}
_ENGINES_INTERP = {1: "lds_tiles", 2: "marching_ring"}


def _bounds(b, ndim, what):
    """((lo, hi) per dimension) -> (centres, half-widths)."""
    b = list(b)
    if ndim == 1 and len(b) == 2 and not isinstance(b[0], (tuple, list)):
        b = [tuple(b)]
    if len(b) != ndim:
        raise DimensionMismatch(f"{what} must hold one (min, max) pair per dimension ({ndim})")
    cs, ws = [], []
    for lo, hi in b:
        lo, hi = float(lo), float(hi)
        if not (math.isfinite(lo) and math.isfinite(hi)) or hi < lo:
            raise ValueError(f"{what}: expected finite (min, max) with min <= max, got ({lo}, {hi})")
        cs.append(0.5 * (lo + hi))
        ws.append(0.5 * (hi - lo))
    return cs, ws


class PlanNUFFT3:
    """``PlanNUFFT3(Z, ndim; m, σ, kernel, kernel_evalmode, ntransforms, sign, backend, source_bounds, target_bounds)``.

    ``Z`` must be complex (ComplexF32 or ComplexF64).  ``source_bounds`` / ``target_bounds``: one ``(min, max)`` pair per dimension;
    ``None`` means the box [-π, π] for the sources and [-1, 1] for the targets (narrow boxes make small grids: give the real ones).
    ``backend=None`` gives a host-only plan (parameter rule and ``info()`` only).
    """

    def __init__(self, Z=torch.complex128, ndim: int = 1, *, m: Union[int, HalfSupport] = 4, sigma: float = 2.0,
                 σ: Optional[float] = None, kernel=None, kernel_evalmode=None, ntransforms: int = 1, sign: int = -1,
                 backend=ROCBackend(0), source_bounds=None, target_bounds=None, options: Optional[dict] = None):
        self.Z = _to_torch_dtype(Z)
        if not self.Z.is_complex:
            raise ValueError("type-3 plans take complex data (ComplexF32 or ComplexF64)")
        self.T = _REAL[self.Z]
        if σ is not None:
            sigma = σ
        M = m.M if isinstance(m, HalfSupport) else int(m)
        kernel = default_kernel(backend) if kernel is None else kernel
        if isinstance(kernel, type):
            kernel = kernel()
        if type(kernel) not in _KERNEL_IDS:
            raise ValueError("kernel must be BackwardsKaiserBesselKernel, KaiserBesselKernel, GaussianKernel or BSplineKernel")
        kernel_evalmode = default_kernel_evalmode(backend) if kernel_evalmode is None else kernel_evalmode
        if isinstance(kernel_evalmode, type):
            kernel_evalmode = kernel_evalmode()
        if not isinstance(kernel_evalmode, (Direct, FastApproximation)):
            raise ValueError("kernel_evalmode must be Direct() or FastApproximation()")
        self.kernel = kernel
        self.kernel_evalmode = kernel_evalmode
        self.backend = backend
        self.sign = int(sign)
        self._M, self._sigma = M, float(sigma)
        self._adjoint_plan = None
        self._ndim = int(ndim)
        self._ntransforms = int(ntransforms)
        self._sources = self._targets = None
        self._handle = C.c_void_p()

        prm = _lib.NufftParams()
        prm.struct_size = C.sizeof(_lib.NufftParams)
        prm.dtype = _lib.F32 if self.T == torch.float32 else _lib.F64
        prm.is_complex = 1
        prm.ndim = self._ndim
        prm.half_support = M
        prm.sigma = float(sigma)
        prm.kernel = _KERNEL_IDS[type(kernel)]
        kparam = getattr(kernel, "beta", None) if not isinstance(kernel, GaussianKernel) else kernel.ell
        prm.kernel_param = 0.0 if kparam is None else float(kparam)
        prm.evalmode = _lib.EVAL_DIRECT if isinstance(kernel_evalmode, Direct) else _lib.EVAL_FAST_APPROXIMATION
        prm.ntransforms = self._ntransforms
        if backend is None:
            prm.device = -1
            self.device = None
        else:
            dev = backend.device if isinstance(backend, ROCBackend) else torch.device(backend).index or 0
            if not torch.cuda.is_available():
                raise RuntimeError("no HIP device available: GPU plans need an MI355X (there is no CPU fallback)")
            torch.cuda.init()
            prm.device = int(dev)
            self.device = torch.device("cuda", int(dev))
        opts = {k: v for k, v in os.environ.items() if k.startswith("NUFFT_") and k not in _HARNESS_ENV and v != ""}
        opts.update({str(k): str(v) for k, v in (options or {}).items()})
        self._options = opts
        self._options_text = ";".join(f"{k}={v}" for k, v in sorted(opts.items())).encode()
        prm.options = self._options_text if opts else None

        t3 = _lib.NufftType3Params()
        t3.struct_size = C.sizeof(_lib.NufftType3Params)
        t3.sign = self.sign
        self._source_bounds = source_bounds if source_bounds is not None else [(-math.pi, math.pi)] * self._ndim
        self._target_bounds = target_bounds if target_bounds is not None else [(-1.0, 1.0)] * self._ndim
        if 1 <= self._ndim <= 3:
            sc, sw = _bounds(self._source_bounds, self._ndim, "source_bounds")
            tc, tw = _bounds(self._target_bounds, self._ndim, "target_bounds")
            for d in range(self._ndim):
                t3.source_center[d], t3.source_halfwidth[d] = sc[d], sw[d]
                t3.target_center[d], t3.target_halfwidth[d] = tc[d], tw[d]
        _check(lib.nufft_plan3_create(C.byref(self._handle), C.byref(prm), C.byref(t3)))
        self._info = self.info()

    @classmethod
    def from_points(cls, Z, xs, ss, **kwargs) -> "PlanNUFFT3":
        """A plan whose boxes are the bounding boxes of the point sets ``xs`` (sources) and ``ss`` (targets), padded by a few ulps so
        that the extreme points lie inside.  Accepts what ``set_points3`` accepts; the points are not set."""
        xs, ss = _as_vectors(xs), _as_vectors(ss)
        if len(xs) != len(ss):
            raise DimensionMismatch("sources and targets must have the same dimension")

        def box(vs):
            out = []
            for v in vs:
                if v.numel() == 0:
                    out.append((0.0, 0.0))
                    continue
                lo, hi = float(v.min()), float(v.max())
                pad = 4.0 * max(abs(lo), abs(hi)) * float(torch.finfo(v.dtype).eps) if v.dtype.is_floating_point else 0.0
                out.append((lo - pad, hi + pad))
            return out

        return cls(Z, len(xs), source_bounds=box(xs), target_bounds=box(ss), **kwargs)

    def adjoint(self) -> "PlanNUFFT3":
        """A new plan of the adjoint transform ``u(x) = Σ_k G_k exp(−sign i s_k · x)``: the same element type, dimension, M, σ,
        kernel, evaluation mode, ntransforms, backend and options, with ``sign = −sign`` and the source and target boxes swapped
        (its sources are this plan's targets).  Its fine grid ``nf`` equals this plan's (the rule depends on the product of the
        half-widths).  Its type 3 applied to ``G`` is the gradient of ``Re Σ_k conj(G_k) f_k`` with respect to the values, and its
        ``exec_type3_grad`` the one with respect to the sources.  The new plan owns its own grids."""
        return PlanNUFFT3(self.Z, self._ndim, m=self._M, sigma=self._sigma, kernel=self.kernel, kernel_evalmode=self.kernel_evalmode,
                          ntransforms=self._ntransforms, sign=-self.sign, backend=self.backend,
                          source_bounds=self._target_bounds, target_bounds=self._source_bounds, options=self._options)

    def close(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            lib.nufft_plan3_destroy(h)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> _lib.NufftInfo3:
        out = _lib.NufftInfo3()
        _check(lib.nufft_plan3_info(self._handle, C.byref(out)))
        return out

    @property
    def ndim(self) -> int:
        return self._ndim

    @property
    def ntransforms(self) -> int:
        return self._ntransforms

    @property
    def eltype(self) -> torch.dtype:
        return self.Z

    @property
    def nf(self) -> Tuple[int, ...]:
        """Fine grid (cells per dimension) of the spreading stage."""
        i = self.info()
        return tuple(int(i.nf[d]) for d in range(self._ndim))

    @property
    def num_sources(self) -> int:
        return int(self.info().num_sources)

    @property
    def num_targets(self) -> int:
        return int(self.info().num_targets)

    def points_outside(self) -> Tuple[int, int]:
        """(sources, targets) of the last set_points3 outside the declared boxes (synchronises)."""
        self._require_gpu()
        a, b = C.c_int64(), C.c_int64()
        _check(lib.nufft_type3_points_outside(self._handle, C.byref(a), C.byref(b), self._stream()))
        return int(a.value), int(b.value)

    def _internal(self, which: int):
        h = C.c_void_p()
        _check(lib.nufft_plan3_internal(self._handle, which, C.byref(h)))
        return h

    def spread_engine_used(self) -> str:
        """Engine that spread the current sources (the internal spreading plan's per-point-set choice; synchronises)."""
        self._require_gpu()
        out = C.c_int()
        _check(lib.nufft_spread_engine_used(self._internal(0), C.byref(out), self._stream()))
        return _ENGINES_SPREAD[out.value]

    def interp_engine_used(self) -> str:
        """Engine that interpolates at the current targets (the internal type-2 plan's choice; synchronises)."""
        self._require_gpu()
        out = C.c_int()
        _check(lib.nufft_interp_engine_used(self._internal(1), C.byref(out), self._stream()))
        return _ENGINES_INTERP[out.value]

    def internal_info(self, which: int) -> _lib.NufftInfo:
        """nufft_info of the internal spreading plan (0) or type-2 plan (1)."""
        out = _lib.NufftInfo()
        _check(lib.nufft_plan_info(self._internal(which), C.byref(out)))
        return out

    def enable_timing(self, on: bool = True):
        _check(lib.nufft_set_timing3(self._handle, int(on)))

    @property
    def timer(self) -> dict:
        """Milliseconds of the latest run of each type-3 stage (synchronises on the events)."""
        buf = (C.c_float * _lib.NUM_STAGES3)()
        _check(lib.nufft_get_stage_times3(self._handle, buf))
        return {name: float(buf[i]) for i, name in enumerate(_lib.STAGE_NAMES3) if buf[i] >= 0}

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _require_gpu(self):
        if self.device is None:
            raise ValueError("host-only plan (backend=None) has no device path")

    def __repr__(self):
        i = self.info()
        D = self._ndim
        return (f"{D}-dimensional PlanNUFFT3 with input type {self.Z}: sign {i.sign:+d}, M = {i.half_support}, σ = {i.sigma}, "
                f"{type(self.kernel).__name__}, fine grid {self.nf}, type-2 grid {tuple(int(i.inner_N_over[d]) for d in range(D))}, "
                f"{self._ntransforms} transform(s)")


def _as_vectors(xp) -> Tuple[torch.Tensor, ...]:
    if isinstance(xp, torch.Tensor):
        if xp.dim() == 1:
            return (xp,)
        if xp.dim() == 2:
            return tuple(xp[:, d].contiguous() for d in range(xp.shape[1]))
        raise ValueError("unexpected point container")
    return tuple(xp)


def _check_points(p: PlanNUFFT3, xp, what: str) -> Tuple[torch.Tensor, ...]:
    if isinstance(xp, torch.Tensor) and xp.dim() == 2 and xp.shape[1] != p.ndim:
        raise DimensionMismatch(f"expected {what} as an (Np, {p.ndim}) tensor")
    xp = _as_vectors(xp)
    if len(xp) != p.ndim:
        raise DimensionMismatch(f"expected {p.ndim}-dimensional {what}")
    for x in xp:
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"unexpected {what} container: expected torch tensors")
        if x.dtype != p.T:
            raise ValueError(f"{what} must have the same accuracy as the created plan (got {x.dtype} for a {p.Z} plan)")
        if x.device != p.device:
            raise ValueError(f"unexpected {what} container: expected tensors on {p.device}, got {x.device}")
        if x.dim() != 1 or not x.is_contiguous():
            raise ValueError(f"unexpected {what} container: expected contiguous vectors")
    n = xp[0].numel()
    if any(x.numel() != n for x in xp):
        raise DimensionMismatch(f"{what} must have the same length along all dimensions")
    return xp


def set_points3(p: PlanNUFFT3, xs, ss) -> PlanNUFFT3:
    """Sources ``xs`` and targets ``ss``: tuples of D device vectors, or ``(Np, D)`` tensors (copied), of the plan's real type."""
    p._require_gpu()
    xs = _check_points(p, xs, "sources")
    ss = _check_points(p, ss, "targets")
    _check(lib.nufft_set_points3(p._handle, xs[0].numel(), _ptr_table(xs), ss[0].numel(), _ptr_table(ss), p._stream()))
    p._sources, p._targets = xs, ss
    return p


def _check_vectors(p: PlanNUFFT3, vs, n: int, what: str):
    if len(vs) != p.ntransforms:
        raise DimensionMismatch(f"wrong amount of {what} vectors (expected {p.ntransforms})")
    for v in vs:
        if not isinstance(v, torch.Tensor) or v.device != p.device:
            raise ValueError(f"{what} must be torch tensors on {p.device}")
        if v.dtype != p.Z:
            raise ValueError(f"{what} must have element type {p.Z} (got {v.dtype})")
        if v.dim() != 1 or not v.is_contiguous():
            raise ValueError(f"{what} must be contiguous vectors")
        if v.numel() != n:
            raise DimensionMismatch(f"wrong length of {what} vector (expected {n}, got {v.numel()})")


def exec_type3(f, p: PlanNUFFT3, c):
    """f_k = Σ_j c_j exp(sign i s_k · x_j) for every component.  ``f``: complex vector(s) of num_targets, ``c``: of num_sources.
    Returns ``f``."""
    p._require_gpu()
    if p._sources is None:
        raise ValueError("set_points3 must be called before exec_type3")
    f_t = (f,) if isinstance(f, torch.Tensor) else tuple(f)
    c_t = (c,) if isinstance(c, torch.Tensor) else tuple(c)
    _check_vectors(p, f_t, p._targets[0].numel(), "output")
    _check_vectors(p, c_t, p._sources[0].numel(), "input")
    _check(lib.nufft_exec_type3(p._handle, _ptr_table(f_t), _ptr_table(c_t), p._stream()))
    return f


def _grad_table(p: PlanNUFFT3, gp, n: int):
    """``gp``: a tuple of D vectors (ntransforms = 1) or a tuple of ntransforms such tuples -> (nested tuple, flat table)."""
    if p.ntransforms == 1 and len(gp) == p.ndim and all(isinstance(g, torch.Tensor) for g in gp):
        gp = (tuple(gp),)
    gp = tuple(tuple(g) for g in gp)
    if len(gp) != p.ntransforms:
        raise DimensionMismatch(f"wrong amount of gradient tuples (expected {p.ntransforms} tuples of {p.ndim} vectors)")
    for g in gp:
        if len(g) != p.ndim:
            raise DimensionMismatch(f"wrong amount of gradient vectors (expected {p.ndim} per component)")
    for d in range(p.ndim):
        _check_vectors(p, tuple(g[d] for g in gp), n, "gradient output")
    return _ptr_table(tuple(v for g in gp for v in g))


def exec_type3_grad(f, gp, p: PlanNUFFT3, c):
    """exec_type3 with the derivatives with respect to the targets: ``gp[c][d] = ∂f_c/∂s_d`` at every target (same sizes and
    element type as ``f``), from one premultiply and spread, the inner type-2 gradient and one finishing kernel.
    ``gp``: a tuple of D vectors, or a tuple of ntransforms such tuples.  Derivatives with respect to the sources come from the
    ``adjoint()`` plan.  Returns ``(f, gp)``."""
    p._require_gpu()
    if p._sources is None:
        raise ValueError("set_points3 must be called before exec_type3_grad")
    f_t = (f,) if isinstance(f, torch.Tensor) else tuple(f)
    c_t = (c,) if isinstance(c, torch.Tensor) else tuple(c)
    nk = p._targets[0].numel()
    _check_vectors(p, f_t, nk, "output")
    _check_vectors(p, c_t, p._sources[0].numel(), "input")
    gtbl = _grad_table(p, gp, nk)
    _check(lib.nufft_exec_type3_grad(p._handle, _ptr_table(f_t), gtbl, _ptr_table(c_t), p._stream()))
    return f, gp
