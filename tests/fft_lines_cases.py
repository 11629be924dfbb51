"""Case tables of the line-length matrix of the library's own FFT passes (csrc/fft_lines.hip): one table per kernel kind, every
length of NUFFT_FFT_SIZES in each.  No GPU import: tests/test_fft_lines_host.py checks the tables on the CPU (the list of lengths
against the macro, every case's dims against the oversampled sizes it is meant to reach, the halo list against what host-only
plans accept), tests/test_gpu_fft_lines.py runs them.

Rule (sigma = 2, checked for every length by the host test): on a complex or non-first axis N = n/2 and N = n/2 - 1 both give
the oversampled size n (n/2 - 1 is odd for every length: the odd kept count); on the real first axis N = M and N = M - 1 both give 2 M.

Partial workgroups: the strided passes meet them in their column groups (21 kept columns against groups of 16, 8 or 4).  The
contiguous-line kernels (real, complex, Toeplitz) cannot meet one through a plan: they run only where every other oversampled size
is in the table, all multiples of 16, so their line count is a multiple of every lines-per-workgroup value (16, 8, 4).

The coupled dimension-1 kernel (csrc/toeplitz_coupled.hip) and the coil-map variants of the strided pass have tables of their own
(`coupled_cases`, `coupled_refused`, `maps_cases`).  What an operator cannot reach in the coupled kernel: the kept count of its
dimension 1 is always n / 2, which is even, so the scalar (odd `k1`) load/store branch of its ComplexF32 instantiations is dead
there; and the line count is the product of the other padded sizes, all from the table and so multiples of 16 (in these tables 64
and 4096 line ids, multiples of 64), a multiple of every waves-per-workgroup value (16 … 1), so `line_id >= nlines` never fires.
"""
from collections import namedtuple

import numpy as np

# the lengths NUFFT_FFT_SIZES instantiates (radix sequences: 320 = 8 * 8 * 5, 640 = 8 * 8 * 2 * 5, 768 = 8 * 8 * 4 * 3)
SIZES = (64, 80, 96, 128, 160, 192, 256, 320, 384, 512, 640, 768, 1024)

HALF_SUPPORT, SIGMA = 4, 2.0
NP_PLAN, NP_TOEPLITZ, NP_HALO = 500, 200, 2000

# kind: which kernel runs at length n — Z: element type of the plan — dims: (N1, N2[, N3]) — over: the oversampled sizes the dims
# are meant to give — C: ntransforms
PlanCase = namedtuple("PlanCase", "kind Z n dims over fftshift C")

REAL_TYPES = (np.float32, np.float64)
COMPLEX_OF = {np.float32: np.complex64, np.float64: np.complex128}

# groups of the plan-path matrix; ntransforms = 2 on every third length of each group, staggered so that over the groups every
# length meets it
GROUPS = ("strided_2d", "strided_3d_dim2", "strided_3d_dim3", "real_dim1", "cplx_dim1", "cplx_strided")


def _ntransforms(group, i):
    return 2 if (i + GROUPS.index(group)) % 3 == 0 else 1


def plan_cases():
    """Section 2 of the matrix: every length in every kernel kind of the plan paths, Float32 and Float64."""
    out = []
    for T in REAL_TYPES:
        Zc = COMPLEX_OF[T]
        for i, n in enumerate(SIZES):
            h = n // 2
            # strided pass of a 2-D real plan: 21 kept columns = one full column group and one partial one; dimension 1 (80) by rocFFT
            for N2 in (h, h - 1):
                out.append(PlanCase("strided_2d", T, n, (40, N2), (80, n), False, _ntransforms("strided_2d", i)))
            # 3-D real plans: the row-structured pass along dimension 2 and the pass along dimension 3 at length n; the odd kept count
            # and fftshift alternate over the lengths, differently for the two kinds
            out.append(PlanCase("strided_3d_dim2", T, n, (40, h - (i % 2), 32), (80, n, 64), i % 2 == 0, _ntransforms("strided_3d_dim2", i)))
            out.append(PlanCase("strided_3d_dim3", T, n, (40, 32, h - ((i + 1) % 2)), (80, 64, n), (i // 2) % 2 == 0,
                                _ntransforms("strided_3d_dim3", i)))
            # dimension 1 of real plans: real_lines_kernel at M = n
            for N1 in (n, n - 1):
                out.append(PlanCase("real_dim1", T, n, (N1, 32), (2 * n, 64), False, _ntransforms("real_dim1", i)))
            # dimension 1 of complex plans: cplx_lines_kernel at n; and the strided pass with the compact complex spectrum
            for N1 in (h, h - 1):
                out.append(PlanCase("cplx_dim1", Zc, n, (N1, 32), (n, 64), False, _ntransforms("cplx_dim1", i)))
            out.append(PlanCase("cplx_strided", Zc, n, (32, h), (64, n), i % 2 == 1, _ntransforms("cplx_strided", i)))
    return out


def mult_cases():
    """Section 3: the MULT variants of the strided pass (mode factors), 2-D real plans as in `strided_2d`."""
    return [PlanCase("mult", T, n, (40, n // 2 - (i % 2)), (80, n), False, 1) for T in REAL_TYPES for i, n in enumerate(SIZES)]


ToeplitzCase = namedtuple("ToeplitzCase", "kind Z n dims fftshift")


def toeplitz_cases():
    """Section 4: the fused apply at every 2 N of the table: toeplitz_lines_kernel at n, the strided pass at n in 2-D, the pass along
    dimension 2 (nc = 2 N3 launches) and along dimension 3 in 3-D.  Each shape for both element types, one after the other (they
    share the exact reference)."""
    out = []
    for i, n in enumerate(SIZES):
        h = n // 2
        for kind, dims, shift in (("lines", (h, 32), i % 2 == 0), ("strided_2d", (32, h), i % 2 == 1),
                                  ("strided_3d_dim2", (32, h, 32), i % 2 == 0), ("strided_3d_dim3", (32, 32, h), i % 2 == 1)):
            for Z in ("c128", "c64"):
                out.append(ToeplitzCase(kind, Z, n, dims, shift))
    return out


# Section 6: toeplitz_lines_coupled_kernel<T, N, KT, TL> (csrc/toeplitz_coupled.hip), dimension 1 of the fused apply for K coupled
# components.  Three rules of that file decide which instantiation runs and how; they are restated here so that the tables can be
# checked for what they reach (tests/test_fft_lines_host.py pins the restatement against a literal table).
LDS_LIMIT = 160 * 1024            # kFftLdsLimit (csrc/fft_line.h): LDS per workgroup
CSIZE = {"c128": 16, "c64": 8}    # bytes of one complex element
TIERS = (2, 4, 8, 16)
TIER_KS = {2: (2,), 4: (3, 4), 8: (5, 6, 7, 8), 16: (9, 12, 16)}


def coupled_waves(csize, n, kt):
    """Waves per workgroup (the template parameter TL) — `coupled_waves` of csrc/toeplitz_coupled.hip (lines 37-46): the most of
    16, 8, 4 that leave room for two workgroups per CU, else the most of 16 … 1 that fit at all; 0: not even one wave fits."""
    line = n + (n >> 4) + 1
    for tl in (16, 8, 4):
        if csize * (n + tl * kt * line) <= 80 * 1024:
            return tl
    for tl in (16, 8, 4, 2, 1):
        if csize * (n + tl * kt * line) <= LDS_LIMIT:
            return tl
    return 0


def coupled_tier(K):
    """The compile-time bound KT of the run-time K — `coupled_tier` of csrc/toeplitz_coupled.hip (line 47)."""
    return 2 if K <= 2 else (4 if K <= 4 else (8 if K <= 8 else 16))


def coupled_prefetch(csize, n, kt):
    """Whether the instantiation holds the diagonal lines of a lane's first pack in registers across the backward FFTs — `PREFETCH` of
    csrc/toeplitz_coupled.hip (lines 54-58): KT <= 4 && N / PW >= 64 with PW = 16 / sizeof(T) cells per 16-byte load."""
    pw = 16 // (csize // 2)
    return kt <= 4 and n // pw >= 64


CoupledCase = namedtuple("CoupledCase", "kind Z n dims K fftshift")


def coupled_cases():
    """One case per launchable (element type, length, tier): dims (n / 2, 32) give the dimension-1 line length n, the other padded size 64
    and 64 line ids.  K walks through the tier over the lengths, fftshift alternates, oppositely for the two types.  Then four 3-D
    shapes with 4096 line ids (many workgroups).  The two types of a (length, tier) follow each other: they share the reference."""
    out = []
    for i, n in enumerate(SIZES):
        for tier in TIERS:
            ks = TIER_KS[tier]
            for Z in ("c128", "c64"):
                if coupled_waves(CSIZE[Z], n, tier) > 0:
                    out.append(CoupledCase("coupled_lines", Z, n, (n // 2, 32), ks[i % len(ks)], (i % 2 == 0) == (Z == "c128")))
    out.append(CoupledCase("coupled_lines", "c128", 128, (64, 32, 32), 3, False))      # prefetch on
    out.append(CoupledCase("coupled_lines", "c64", 256, (128, 32, 32), 2, True))       # prefetch on
    out.append(CoupledCase("coupled_lines", "c64", 64, (32, 32, 32), 7, False))
    out.append(CoupledCase("coupled_lines", "c128", 80, (40, 32, 32), 9, True))
    return out


def coupled_refused():
    """(Z, n, K) the fused path must refuse (coupled_waves = 0): ComplexF64, tier 16, from 640 cells on — the smallest K of the tier at
    each length and the largest at the first."""
    return [("c128", 640, 9), ("c128", 640, 16), ("c128", 768, 9), ("c128", 1024, 9)]


def maps_cases():
    """Section 7: fft_lines_kernel<..., CMAP = true>, the coil maps inside the outermost strided passes of the fused apply (backward:
    times S on load; forward: times conj(S) on store, coil 0 storing, coils 1 and 2 accumulating), three coils each.
    maps_2d, dims (40, n / 2): the strided pass at n carries the map over 40 kept columns (a partial column group against groups of 16, full
    ones against 8 and 4), dimension 1 runs at 80.  maps_3d, dims (32, 32, n / 2): the pass along dimension 3 at n carries the map, the
    pass along dimension 2 runs without it.  Each shape for both element types, one after the other (they share the reference)."""
    out = []
    for i, n in enumerate(SIZES):
        for kind, dims, shift in (("maps_2d", (40, n // 2), i % 2 == 0), ("maps_3d", (32, 32, n // 2), i % 2 == 1)):
            for Z in ("c128", "c64"):
                out.append(ToeplitzCase(kind, Z, n, dims, shift))
    return out


HaloCase = namedtuple("HaloCase", "Z n dims over")

# Section 5: the halo-adding forward dimension-1 pass behind the spreading window's halo variant (spread_method = "marching_ring",
# NUFFT_SMARCH_HALO = 2), 3-D plans (N1, 32, 32): real plans N1 = M (real_lines_kernel at M, oversampled 2 M x 64 x 64), complex plans
# N1 = n / 2 (cplx_lines_kernel at n).  The window's column must divide the axes: at M = 4 the chooser finds one for all thirteen
# lengths (16, 20, 24 or 32 cells along dimension 1), so no length is left out — tests/test_fft_lines_host.py asserts that from
# host-only plans; a length the plan refuses would have to leave this list with the plan's reason next to it
HALO_TYPES = (np.float32, np.float64, np.complex64, np.complex128)
HALO_LENGTHS = SIZES


def halo_shape(Z, n):
    """(dims, oversampled sizes) of the halo case of element type Z at line length n (real: M = n)."""
    if np.dtype(Z).kind == "f":
        return (n, 32, 32), (2 * n, 64, 64)
    return (n // 2, 32, 32), (n, 64, 64)


def halo_cases():
    return [HaloCase(Z, n, *halo_shape(Z, n)) for Z in HALO_TYPES for n in HALO_LENGTHS]


def case_id(c):
    Z = c.Z if isinstance(c.Z, str) else np.dtype(c.Z).name
    extra = f"-K{c.K}" if hasattr(c, "K") else ""
    if getattr(c, "fftshift", False):
        extra += "-shift"
    if getattr(c, "C", 1) > 1:
        extra += f"-C{c.C}"
    kind = getattr(c, "kind", "halo")
    return f"{kind}-{Z}-n{c.n}-{'x'.join(str(d) for d in c.dims)}{extra}"
