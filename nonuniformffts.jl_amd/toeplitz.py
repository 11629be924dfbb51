"""Toeplitz normal operator ``G = A^H W A`` of a complex plan, above the C ABI's ``nufft_toeplitz_*`` entry points.

    G û = exec_type1( w ⊙ exec_type2(û) ),   w_j real weights at the points

is what CG / LSQR on the normal equations applies once per iteration.  ``G[k, k'] = T[k − k']`` with ``T_d = Σ_j w_j exp(−i d·x_j)``,
so after one build per point set it is applied with FFTs of size 2N alone, at a cost that does not depend on the number of points
(NFFT.jl: ``calculateToeplitzKernel`` / ``convolveToeplitzKernel!``).  Plumbing only: every array operation runs in the library.

    op = ToeplitzOperator(plan).set_points(points, weights)
    g = op(u)                      # = exec_type1(w * exec_type2(u)) up to the accuracy of one NUFFT

With coil sensitivity maps (``op.set_maps(maps)``, parallel MRI) the same ``apply`` computes ``Σ_c conj(S_c) ⊙ G (S_c ⊙ û)``;
``coil_expand`` / ``coil_combine`` are the coil passes of the forward model and of the right-hand side.

Coupled components (subspace models, ``y_j = Σ_a φ_a(j) (A û_a)_j``): ``op.set_points(points, weights, basis=phi)`` with ``phi`` of shape
``(ntransforms, Np)`` makes ``apply`` the block operator ``(G_Φ u)_a = Σ_b A^H diag(w conj(φ_a) φ_b) A u_b`` and ``solve`` / ``ToeplitzCG``
one joint system; a plain ``set_points`` / ``set_spectrum`` returns to independent components.

Off-resonance correction: ``ToeplitzOperator(plan, segments=L)`` is ONE component outside and L time segments inside,
``G_ω u = Σ_a conj(B_a) ⊙ Σ_b A^H diag(w conj(φ_a) φ_b) A (B_b ⊙ u)``: ``set_points(points, weights, basis=phi)`` with ``phi`` of shape
``(L, Np)`` and ``set_factors(B)``; ``field.py`` computes ``phi`` and ``B`` from a field map.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import lib
from .plan import (_KERNEL_IDS, _check, _ptr_table, Direct, DimensionMismatch, FastApproximation, GaussianKernel, HalfSupport,
                   PlanNUFFT)

_PATHS = {_lib.TOEPLITZ_PATH_DENSE: "dense", _lib.TOEPLITZ_PATH_FUSED: "fused"}


class ToeplitzOperator:
    """``ToeplitzOperator(plan)``: tied to the geometry of a complex ``PlanNUFFT`` (element type, dims, ntransforms, fftshift, point
    convention, window parameters, device); the plan itself is not kept and may be closed afterwards.  Real-data plans are refused:
    their type 2 extends the half spectrum Hermitian-ly, which for even N adds the mode +N/2, and the 2N embedding aliases."""

    def __init__(self, plan: PlanNUFFT, segments: Optional[int] = None):
        if not isinstance(plan, PlanNUFFT):
            raise ValueError("ToeplitzOperator takes a PlanNUFFT")
        if segments is not None and (isinstance(segments, bool) or not isinstance(segments, int)):
            raise ValueError(f"segments must be an integer (got {segments!r})")
        self._handle = C.c_void_p()
        self._factors = ()
        if segments is None:
            _check(lib.nufft_toeplitz_create(C.byref(self._handle), plan._handle))
        else:
            _check(lib.nufft_toeplitz_create_segmented(C.byref(self._handle), plan._handle, segments))
        #: time segments of a segmented operator (``segments=L``: one component outside, L coupled segments inside), else 0
        self.segments = 0 if segments is None else segments
        self.Z, self.T = plan.eltype, plan.T
        self.device = plan.device
        self.shape = plan.shape
        self.ndim = plan.ndim
        self.ntransforms = plan.ntransforms
        self._kernel, self._evalmode = plan.kernel, plan.kernel_evalmode
        self._maps = ()

    def close(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            lib.nufft_toeplitz_destroy(h)
            self._handle = C.c_void_p()
        self._maps = ()
        self._factors = ()

    def _require_open(self):
        if not self._handle.value:
            raise ValueError("the ToeplitzOperator is closed")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> _lib.NufftToeplitzInfo:
        out = _lib.NufftToeplitzInfo()
        out.struct_size = C.sizeof(_lib.NufftToeplitzInfo)
        _check(lib.nufft_toeplitz_get_info(self._handle, C.byref(out)))
        return out

    @property
    def path(self) -> str:
        """``"fused"`` (pruned line passes, the 2N grid never exists) or ``"dense"`` (rocFFT on the 2N grid)."""
        return _PATHS[self.info().path]

    @property
    def padded_shape(self):
        """Tensor shape of the multiplier: 2N per dimension, reversed like ``plan.shape``."""
        i = self.info()
        return tuple(int(i.N2[d]) for d in reversed(range(self.ndim)))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _require_gpu(self):
        if self.device is None:
            raise ValueError("host-only Toeplitz operator (plan with backend=None) has no device path")

    def set_spectrum(self, T: torch.Tensor) -> "ToeplitzOperator":
        """``T``: the type 1 of the weights on the mode set of a plan with 2N modes per dimension and ``fftshift=False`` (a complex
        tensor of shape ``padded_shape``).  Only read."""
        self._require_gpu()
        if not isinstance(T, torch.Tensor) or T.device != self.device:
            raise ValueError(f"the spectrum must be a torch tensor on {self.device}")
        if T.dtype != self.Z:
            raise ValueError(f"the spectrum must have element type {self.Z} (got {T.dtype})")
        if tuple(T.shape) != self.padded_shape:
            raise DimensionMismatch(f"wrong dimensions of the spectrum (expected tensor shape {self.padded_shape}, got {tuple(T.shape)})")
        if not T.is_contiguous():
            raise ValueError("the spectrum must be contiguous")
        _check(lib.nufft_toeplitz_set_spectrum(self._handle, C.c_void_p(T.data_ptr()), self._stream()))
        return self

    @staticmethod
    def pair_index(a: int, b: int, K: int) -> int:
        """Position of the pair ``a <= b`` in the row-major order over ``a <= b`` that ``set_spectra`` uses."""
        if not 0 <= a <= b < K:
            raise ValueError(f"the pair must satisfy 0 <= a <= b < {K}")
        return a * K - a * (a - 1) // 2 + (b - a)

    @property
    def _inner(self) -> int:
        """Size of the coupled block: the segments of a segmented operator, ``ntransforms`` of any other."""
        return self.segments or self.ntransforms

    @property
    def coupled(self) -> bool:
        """True while a coupled build (``set_points(..., basis=)`` / ``set_spectra``) is in force."""
        return bool(self._handle.value) and lib.nufft_toeplitz_num_coupled(self._handle) > 0

    def _checked_tuple(self, x, shape, what, expected, count=None, counted=None, *, stacked_count=False, empty=None):
        """A contiguous stacked tensor ``(count, *shape)`` or a sequence of ``shape`` tensors -> the tuple of its arrays, checked like
        ``_check_uniform`` checks.  ``what`` names the arrays in the messages and ``expected`` is the stacked shape they quote.
        ``count``: how many there must be, ``counted`` in words (default: the number); None: at least one, else ``ValueError(empty)``.
        ``stacked_count``: a stacked tensor of another count has the wrong dimensions, not the wrong amount."""
        if isinstance(x, torch.Tensor):
            if x.dim() != self.ndim + 1 or (stacked_count and x.shape[0] != count):
                raise DimensionMismatch(f"wrong dimensions of the {what.removeprefix('the ')} (expected tensor shape {expected}, "
                                        f"got {tuple(x.shape)})")
            if not x.is_contiguous():
                raise ValueError(f"{what} must be contiguous")
            x = tuple(x[i] for i in range(x.shape[0]))
        else:
            x = tuple(x)
        if count is None and not x:
            raise ValueError(empty)
        if count is not None and len(x) != count:
            raise DimensionMismatch(f"wrong amount of {what.removeprefix('the ')} (expected {counted or count}, got {len(x)})")
        self._require_gpu()
        self._require_open()
        _check_coil_arrays(x, self.device, self.Z, shape, what)
        return x

    def set_spectra(self, T) -> "ToeplitzOperator":
        """The coupled counterpart of ``set_spectrum``: ``T`` of shape ``(K (K + 1) / 2, *padded_shape)`` or a sequence of that many
        ``padded_shape`` tensors, ``T[pair_index(a, b, K)] = T_ab`` on the mode set of a 2N plan, ``K = ntransforms`` (``K = segments`` on
        a segmented operator).  Only read."""
        K = self._inner
        npairs = K * (K + 1) // 2
        T = self._checked_tuple(T, self.padded_shape, "the spectra", f"({npairs}, ...) for {K} components", npairs, f"{npairs} for {K} components",
                                stacked_count=True)
        _check(lib.nufft_toeplitz_set_spectra_coupled(self._handle, _ptr_table(T), self._stream()))
        return self

    def _basis_rows(self, basis):
        """``basis`` as a ``(K, Np)`` tensor: a vector counts as one row where ``K == 1``."""
        K = self._inner
        if not isinstance(basis, torch.Tensor):
            raise ValueError("basis must be a torch tensor of shape (ntransforms, Np)")
        if basis.dim() == 1 and K == 1:
            basis = basis[None]
        if basis.dim() != 2 or basis.shape[0] != K:
            raise DimensionMismatch(f"wrong dimensions of the basis (expected {K} rows of Np values, got tensor shape {tuple(basis.shape)})")
        return basis

    def _check_basis(self, basis, n):
        """``basis`` (from ``_basis_rows``) as a tuple of K aligned ``(Np,)`` tensors (the exception types of ``_check_uniform``)."""
        K = self._inner
        if basis.device != self.device:
            raise ValueError(f"basis must be a torch tensor on {self.device}")
        if basis.dtype != self.Z:
            raise ValueError(f"basis must have element type {self.Z} (got {basis.dtype})")
        if basis.shape[1] != n:
            raise DimensionMismatch(f"wrong length of the basis (expected {n} points, got {basis.shape[1]})")
        if not basis.is_contiguous():
            raise ValueError("basis must be contiguous")
        return _aligned(tuple(basis[a] for a in range(K)))

    def _check_points(self, points):
        """One point set as ``set_points`` of the plan takes it -> (tuple of ndim contiguous vectors, their length)."""
        if isinstance(points, torch.Tensor):
            if points.dim() == 1:
                points = (points,)
            elif points.dim() == 2:
                points = tuple(points[:, d].contiguous() for d in range(points.shape[1]))
            else:
                raise ValueError("unexpected point container")
        points = tuple(points)
        if len(points) != self.ndim:
            raise DimensionMismatch(f"expected {self.ndim}-dimensional points")
        for x in points:
            if not isinstance(x, torch.Tensor) or x.device != self.device:
                raise ValueError(f"unexpected point container: expected torch tensors on {self.device}")
            if x.dtype != self.T:
                raise ValueError(f"input points must have the same accuracy as the created plan (got {x.dtype})")
            if x.dim() != 1 or not x.is_contiguous():
                raise ValueError("unexpected point container: expected contiguous vectors")
        n = points[0].numel()
        if any(x.numel() != n for x in points):
            raise DimensionMismatch("input points must have the same length along all dimensions")
        return points, n

    def _check_weights(self, weights, n):
        """Real weights of ``n`` points -> their device pointer (None: ones)."""
        if weights is None:
            return None
        if not isinstance(weights, torch.Tensor) or weights.device != self.device:
            raise ValueError(f"weights must be a torch tensor on {self.device}")
        if weights.dtype != self.T:
            raise ValueError(f"weights must be real with the plan's accuracy ({self.T}); complex weights are not supported")
        if weights.dim() != 1 or not weights.is_contiguous():
            raise ValueError("weights must be a contiguous vector")
        if weights.numel() != n:
            raise DimensionMismatch(f"wrong length of the weights (expected {n}, got {weights.numel()})")
        return C.c_void_p(weights.data_ptr())

    def _build_params(self, m, sigma, kernel, kernel_evalmode):
        """The window of a build that overrides the parent plan's: a ``byref`` for the C ABI, or None."""
        if all(v is None for v in (m, sigma, kernel, kernel_evalmode)):
            return None
        kernel = self._kernel if kernel is None else (kernel() if isinstance(kernel, type) else kernel)
        mode = self._evalmode if kernel_evalmode is None else (kernel_evalmode() if isinstance(kernel_evalmode, type) else kernel_evalmode)
        if type(kernel) not in _KERNEL_IDS:
            raise ValueError("kernel must be BackwardsKaiserBesselKernel, KaiserBesselKernel, GaussianKernel or BSplineKernel")
        if not isinstance(mode, (Direct, FastApproximation)):
            raise ValueError("kernel_evalmode must be Direct() or FastApproximation()")
        prm = _lib.NufftParams()
        prm.struct_size = C.sizeof(_lib.NufftParams)
        prm.half_support = 0 if m is None else (m.M if isinstance(m, HalfSupport) else int(m))
        prm.sigma = 0.0 if sigma is None else float(sigma)
        prm.kernel = _KERNEL_IDS[type(kernel)]
        kparam = getattr(kernel, "beta", None) if not isinstance(kernel, GaussianKernel) else kernel.ell
        prm.kernel_param = 0.0 if kparam is None else float(kparam)
        prm.evalmode = _lib.EVAL_DIRECT if isinstance(mode, Direct) else _lib.EVAL_FAST_APPROXIMATION
        return C.byref(prm)

    def set_points(self, points, weights: Optional[torch.Tensor] = None, *, basis: Optional[torch.Tensor] = None, m=None,
                   sigma: Optional[float] = None, σ: Optional[float] = None, kernel=None, kernel_evalmode=None) -> "ToeplitzOperator":
        """Builds the multiplier from ``points`` (what ``set_points`` of the plan accepts) and real ``weights`` (None = ones) with an
        internal plan of 2N modes that is destroyed before the call returns (it is large while it lives: 17 GB at 256³, σ = 2,
        ComplexF64).  ``m`` / ``sigma`` / ``kernel`` / ``kernel_evalmode`` override the parent plan's window for this build.

        ``basis``: a contiguous complex tensor ``(ntransforms, Np)`` of the plan's element type (a ``(Np,)`` vector when
        ``ntransforms == 1``): the components are then coupled, ``(G u)_a = Σ_b A^H diag(w conj(φ_a) φ_b) A u_b``.  On a segmented
        operator ``basis`` is required and has ``segments`` rows: the temporal interpolators ``φ_l(t_j)``."""
        if basis is not None:
            basis = self._basis_rows(basis)        # the component count needs no device
        self._require_gpu()
        points, n = self._check_points(points)
        wptr = self._check_weights(weights, n)
        build = self._build_params(m, σ if σ is not None else sigma, kernel, kernel_evalmode)
        if basis is not None:
            rows = self._check_basis(basis, n)
            _check(lib.nufft_toeplitz_set_points_coupled(self._handle, build, n, _ptr_table(points), wptr, _ptr_table(rows), self._stream()))
            return self
        _check(lib.nufft_toeplitz_set_points(self._handle, build, n, _ptr_table(points), wptr, self._stream()))
        return self

    @property
    def framed(self) -> bool:
        """True while a framed build (``set_points_frames`` / ``set_spectra_frames``) is in force: one multiplier per component."""
        return bool(self._handle.value) and lib.nufft_toeplitz_num_frames(self._handle) > 0

    def set_points_frames(self, points, weights=None, *, m=None, sigma: Optional[float] = None, σ: Optional[float] = None, kernel=None,
                          kernel_evalmode=None) -> "ToeplitzOperator":
        """Dynamic imaging: ``points`` is a sequence of ``ntransforms`` point sets, each as ``set_points`` takes one (a frame may have no
        points: its multiplier is zero); ``weights``: None, or a sequence with None (= ones) or a real vector per frame.  From here on
        ``apply`` computes ``out[c] = G_c u[c]`` with frame c's own multiplier; the solvers treat the frames as independent
        components.  One internal 2N plan serves every frame and is destroyed before the call returns."""
        self._require_gpu()
        self._require_open()
        K = self.ntransforms
        points = tuple(points)
        if len(points) != K:
            raise DimensionMismatch(f"wrong amount of point sets (expected {K} frames, got {len(points)})")
        weights = (None,) * K if weights is None else tuple(weights)
        if len(weights) != K:
            raise DimensionMismatch(f"wrong amount of weight vectors (expected {K} frames, got {len(weights)})")
        sets, counts, wptrs = [], [], []
        for pts, w in zip(points, weights):
            pts, n = self._check_points(pts)
            sets.extend(pts)
            counts.append(n)
            wptrs.append(self._check_weights(w, n))
        build = self._build_params(m, σ if σ is not None else sigma, kernel, kernel_evalmode)
        wtab = None if all(w is None for w in wptrs) else (C.c_void_p * K)(*wptrs)
        _check(lib.nufft_toeplitz_set_points_frames(self._handle, build, (C.c_int64 * K)(*counts), _ptr_table(sets), wtab, self._stream()))
        return self

    def set_spectra_frames(self, T) -> "ToeplitzOperator":
        """The framed counterpart of ``set_spectrum``: ``T`` of shape ``(ntransforms, *padded_shape)`` or a sequence of that many
        ``padded_shape`` tensors, ``T[c]`` the spectrum of frame c.  Only read."""
        K = self.ntransforms
        T = self._checked_tuple(T, self.padded_shape, "the spectra", f"({K}, ...)", K, f"{K} frames", stacked_count=True)
        _check(lib.nufft_toeplitz_set_spectra_frames(self._handle, _ptr_table(T), self._stream()))
        return self

    def set_maps(self, maps) -> "ToeplitzOperator":
        """Coil sensitivity maps ``S_c``: a contiguous complex tensor of shape ``(ncoils, *plan.shape)`` or a sequence of ``plan.shape``
        tensors.  From here on ``apply`` computes ``Σ_c conj(S_c) ⊙ G (S_c ⊙ u)`` for every component.  The library borrows the device
        arrays: this object keeps references to them, and their values must not change while they are set.  Slices of a stacked tensor
        that are not 16-byte aligned (an odd element count in ComplexF32) are copied to their own allocations."""
        self._require_gpu()
        self._require_open()
        maps = _aligned(self._checked_tuple(maps, self.shape, "coil maps", f"(ncoils, {', '.join(map(str, self.shape))})",
                                            empty="at least one coil map is needed"))
        _check(lib.nufft_toeplitz_set_maps(self._handle, len(maps), _ptr_table(maps), self._stream()))
        self._maps = maps
        return self

    def set_factors(self, B) -> "ToeplitzOperator":
        """The factors ``B_l`` of a segmented operator (``B_l = exp(−i ω τ_l)`` for a field map ω; any values are taken): a contiguous
        complex tensor of shape ``(segments, *plan.shape)`` or a sequence of ``plan.shape`` tensors.  Borrowed like coil maps: this
        object keeps references, and the values must not change while they are set.  Independent of the builds and of ``set_maps``."""
        self._require_gpu()
        self._require_open()
        if not self.segments:
            raise ValueError("set_factors needs a segmented operator: ToeplitzOperator(plan, segments=L)")
        B = _aligned(self._checked_tuple(B, self.shape, "the factors", f"({self.segments}, {', '.join(map(str, self.shape))})", self.segments))
        _check(lib.nufft_toeplitz_set_factors(self._handle, _ptr_table(B), self._stream()))
        self._factors = B
        return self

    def clear_factors(self) -> "ToeplitzOperator":
        """Forgets the factors (``apply`` is refused until the next ``set_factors``)."""
        self._require_open()
        _check(lib.nufft_toeplitz_clear_factors(self._handle))
        self._factors = ()
        return self

    def clear_maps(self) -> "ToeplitzOperator":
        """Back to the plain operator ``G``."""
        self._require_open()
        _check(lib.nufft_toeplitz_clear_maps(self._handle))
        self._maps = ()
        return self

    @property
    def ncoils(self) -> int:
        """Number of coil maps set (0: the plain operator)."""
        return int(lib.nufft_toeplitz_num_coils(self._handle)) if self._handle.value else 0

    def _check_uniform(self, us: Sequence[torch.Tensor], what: str):
        if len(us) != self.ntransforms:
            raise DimensionMismatch(f"wrong amount of {what} arrays (expected a tuple of {self.ntransforms} arrays)")
        for u in us:
            if not isinstance(u, torch.Tensor) or u.device != self.device:
                raise ValueError(f"{what} must be torch tensors on {self.device}")
            if u.dtype != self.Z:
                raise ValueError(f"{what} must have element type {self.Z} (got {u.dtype})")
            if tuple(u.shape) != self.shape:
                raise DimensionMismatch(f"wrong dimensions of {what} array (expected tensor shape {self.shape}, got {tuple(u.shape)})")
            if not u.is_contiguous():
                raise ValueError(f"{what} must be contiguous")

    def apply(self, u, out=None):
        """``out = G u`` for every component; ``u``: a tensor of ``plan.shape`` or a tuple of ntransforms such tensors; ``out`` may be
        ``u`` unless coil maps are set (coil 0's store would destroy the input of coil 1).  Returns ``out``."""
        self._require_gpu()
        self._require_open()
        single = isinstance(u, torch.Tensor)
        u_t = (u,) if single else tuple(u)
        self._check_uniform(u_t, "input")
        if out is None:
            out_t = tuple(torch.empty_like(v) for v in u_t)
            out = out_t[0] if single else out_t
        else:
            out_t = (out,) if isinstance(out, torch.Tensor) else tuple(out)
            self._check_uniform(out_t, "output")
            refusal = ("with coil maps set the output must not be the input" if self._maps else
                       "on coupled components the output must not be the input: every output depends on every input" if self.coupled else
                       "on a segmented operator the output must not be the input: every segment reads the input" if self.segments else None)
            if refusal and any(o is v or o.data_ptr() == v.data_ptr() for o in out_t for v in u_t):
                raise ValueError(refusal)
        _check(lib.nufft_toeplitz_apply(self._handle, _ptr_table(out_t), _ptr_table(u_t), self._stream()))
        return out

    __call__ = apply

    def solve(self, b, x0=None, out=None, **kw):
        """One-shot ``ToeplitzCG(self, **kw).solve(b, x0, out)``: conjugate gradients on ``(G + lam I) x = b`` (cg.py); the solver's
        arrays are freed before returning.  Returns ``out``."""
        from .cg import ToeplitzCG
        sol = ToeplitzCG(self, **kw)
        try:
            out = sol.solve(b, x0=x0, out=out)
            torch.cuda.current_stream(self.device).synchronize()       # the solver's arrays go away below
        finally:
            sol.close()
        return out

    def max_eigenvalue(self, iters: int = 30, v0=None):
        """The Rayleigh quotient ``<v, G v> / <v, v>`` (float64) after ``iters`` applies of a power iteration on what ``apply`` computes
        now (plain, with coil maps, coupled): a lower bound of ``λmax``, one value per component as a tuple (coupled components are one
        vector: the same value for each).  ``v0``: start vectors like the input of ``apply`` (None: a seeded ``torch.randn``).
        Synchronises the current stream; not inside a graph capture."""
        self._require_gpu()
        self._require_open()
        if isinstance(iters, bool) or not isinstance(iters, int):
            raise ValueError("iters must be an integer")
        if v0 is None:
            gen = torch.Generator(device=self.device).manual_seed(0)
            v_t = tuple(torch.randn(self.shape, dtype=self.Z, device=self.device, generator=gen) for _ in range(self.ntransforms))
        else:
            v_t = (v0,) if isinstance(v0, torch.Tensor) else tuple(v0)
            self._check_uniform(v_t, "start vector")
        out = (C.c_double * self.ntransforms)()
        _check(lib.nufft_toeplitz_max_eigenvalue(self._handle, _ptr_table(v_t), iters, out, self._stream()))
        return tuple(out)

    def multiplier(self, a: Optional[int] = None, b: Optional[int] = None, *, frame: Optional[int] = None) -> torch.Tensor:
        """The real multiplier ``K`` (shape ``padded_shape``): a view of the device array the operator holds — valid while the
        operator lives, rewritten by the next ``set_points`` / ``set_spectrum``; ``.clone()`` it to keep it.

        On a coupled operator ``multiplier(a, b)`` is the block ``K_ab``: a real view for ``a == b``, a complex view for ``a < b``
        (``K_ba = conj(K_ab)``: ``a > b`` raises), freed by the next uncoupled build.  On a framed operator ``multiplier(frame=c)``
        is the real multiplier of frame c, freed by the next plain or coupled build.  A segmented operator has the block of its segments:
        ``multiplier(a, b)`` with ``a <= b < segments``."""
        self._require_gpu()
        self._require_open()
        ptr, nbytes = C.c_void_p(), C.c_int64()
        if (a is None) != (b is None):
            raise ValueError("multiplier() takes no component or the pair (a, b)")
        if frame is not None and a is not None:
            raise ValueError("multiplier() takes the pair (a, b) of a coupled operator or the frame of a framed one, not both")
        if (frame is not None) != self.framed:
            raise ValueError("a framed operator has one multiplier per frame: ask for multiplier(frame=c)" if self.framed
                             else "multiplier(frame=c) needs a framed build (set_points_frames or set_spectra_frames)")
        if a is None and self.coupled:
            raise ValueError("a coupled operator has a block of multipliers: ask for multiplier(a, b) with a <= b")
        if a is not None:
            if not self.coupled and not self.segments:
                raise ValueError("multiplier(a, b) needs a coupled build (set_points(..., basis=) or set_spectra)")
            if not 0 <= a < self._inner or not 0 <= b < self._inner:
                raise ValueError(f"components must lie in 0 ... {self._inner - 1}")
            if a > b:
                raise ValueError("only the pairs a <= b are stored: multiplier(b, a) is the conjugate of multiplier(a, b)")
            _check(lib.nufft_toeplitz_multiplier_pair_ptr(self._handle, a, b, C.byref(ptr), C.byref(nbytes)))
        elif frame is not None:
            if isinstance(frame, bool) or not isinstance(frame, int) or not 0 <= frame < self.ntransforms:
                raise ValueError(f"frame must lie in 0 ... {self.ntransforms - 1}")
            _check(lib.nufft_toeplitz_multiplier_frame_ptr(self._handle, frame, C.byref(ptr), C.byref(nbytes)))
        else:
            _check(lib.nufft_toeplitz_multiplier_ptr(self._handle, C.byref(ptr), C.byref(nbytes)))
        shape = self.padded_shape
        real = a is None or a == b
        typestr = ("<f4" if self.T == torch.float32 else "<f8") if real else ("<c8" if self.T == torch.float32 else "<c16")

        class _View:       # the array-interface protocol: torch wraps the pointer without copying
            __cuda_array_interface__ = {"shape": shape, "typestr": typestr,
                                        "data": (int(ptr.value), False), "version": 2, "strides": None}

        k = torch.as_tensor(_View(), device=self.device)
        assert k.numel() * k.element_size() == nbytes.value
        return k

    def __repr__(self):
        i = self.info()
        return (f"ToeplitzOperator of a {self.ndim}-dimensional {self.Z} plan, N = {tuple(int(i.N[d]) for d in range(self.ndim))}, "
                f"{self.path} path, {f'{self.segments} time segments, ' if self.segments else ''}{'coupled components, ' if self.coupled else ''}{'one multiplier per frame, ' if self.framed else ''}{f'{self.ncoils} coil maps, ' if self.ncoils else ''}{i.workspace_bytes / 1e6:.1f} MB")


def _check_coil_arrays(arrays, device, Z, shape, what):
    """The checks of ``_check_uniform`` (same exception types) for a sequence of coil arrays."""
    for a in arrays:
        if not isinstance(a, torch.Tensor) or a.device != device:
            raise ValueError(f"{what} must be torch tensors on {device}")
        if a.dtype != Z:
            raise ValueError(f"{what} must have element type {Z} (got {a.dtype})")
        if tuple(a.shape) != tuple(shape):
            raise DimensionMismatch(f"wrong dimensions of {what} (expected tensor shape {tuple(shape)}, got {tuple(a.shape)})")
        if not a.is_contiguous():
            raise ValueError(f"{what} must be contiguous")


def _aligned(arrays):
    """The arrays themselves where they are 16-byte aligned, own copies where not (slices of a stacked tensor with an odd element
    count in ComplexF32)."""
    return tuple(a if a.data_ptr() % 16 == 0 else a.clone() for a in arrays)


def _coil_list(maps, what="coil maps"):
    if isinstance(maps, torch.Tensor):
        if maps.dim() < 1 or not maps.is_contiguous():
            raise ValueError(f"{what} must be a contiguous stacked tensor or a sequence of tensors")
        return tuple(maps[c] for c in range(maps.shape[0]))
    return tuple(maps)


def _coil_setup(maps, x):
    if not isinstance(x, torch.Tensor) or not x.is_cuda or not x.is_complex():
        raise ValueError("expected a complex torch tensor on a GPU")
    if x.dtype not in (torch.complex64, torch.complex128):
        raise ValueError(f"unsupported element type {x.dtype}")
    maps = _coil_list(maps)
    if len(maps) < 1:
        raise ValueError("at least one coil map is needed")
    _check_coil_arrays(maps, x.device, x.dtype, x.shape, "coil maps")
    return maps, (_lib.F32 if x.dtype == torch.complex64 else _lib.F64), C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)


def coil_expand(maps, x, out=None):
    """``out[c] = S_c ⊙ x``: ``maps`` a stacked tensor ``(ncoils, *x.shape)`` or a sequence of tensors shaped like ``x``; ``out`` likewise
    (None: a new stacked tensor, returned)."""
    if not isinstance(x, torch.Tensor) or not x.is_contiguous():
        raise ValueError("the input must be a contiguous torch tensor")
    maps, dtype, stream = _coil_setup(maps, x)
    if out is None:
        out = torch.empty((len(maps),) + tuple(x.shape), dtype=x.dtype, device=x.device)
    outs = _coil_list(out, "outputs")
    if len(outs) != len(maps):
        raise DimensionMismatch(f"wrong amount of output arrays (expected {len(maps)})")
    _check_coil_arrays(outs, x.device, x.dtype, x.shape, "outputs")
    work = _aligned(outs)          # a misaligned slice is written through an aligned copy
    maps_a, xin = _aligned(maps), _aligned((x,))[0]
    _check(lib.nufft_coil_expand(dtype, x.numel(), len(maps), _ptr_table(work), _ptr_table(maps_a), C.c_void_p(xin.data_ptr()), x.device.index or 0,
                                 stream))
    for o, w in zip(outs, work):
        if o is not w:
            o.copy_(w)
    return out


def coil_combine(maps, a, out=None):
    """``out = Σ_c conj(S_c) ⊙ a[c]``, summed in coil order; ``maps`` and ``a``: stacked tensors or sequences of equally shaped tensors."""
    arrs = _coil_list(a, "inputs")
    if len(arrs) < 1:
        raise ValueError("at least one coil is needed")
    maps, dtype, stream = _coil_setup(maps, arrs[0])
    if len(arrs) != len(maps):
        raise DimensionMismatch(f"wrong amount of input arrays (expected {len(maps)})")
    x = arrs[0]
    _check_coil_arrays(arrs, x.device, x.dtype, x.shape, "inputs")
    if out is None:
        out = torch.empty_like(x)
    _check_coil_arrays((out,), x.device, x.dtype, x.shape, "the output")
    work = _aligned((out,))[0]
    maps_a, arrs_a = _aligned(maps), _aligned(arrs)      # held until the call is enqueued: a freed copy's memory would be handed out again
    _check(lib.nufft_coil_combine(dtype, x.numel(), len(maps), C.c_void_p(work.data_ptr()), _ptr_table(maps_a), _ptr_table(arrs_a),
                                  x.device.index or 0, stream))
    if work is not out:
        out.copy_(work)
    return out
