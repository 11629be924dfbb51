"""Case tables of the line-length matrix of the library's own FFT passes (csrc/fft_lines.hip): one table per kernel kind, every
length of NUFFT_FFT_SIZES in each.  No GPU import: tests/test_fft_lines_host.py checks the tables on the CPU (the list of lengths
against the macro, every case's dims against the oversampled sizes it is meant to reach, the halo list against what host-only
plans accept), tests/test_gpu_fft_lines.py runs them.

Rule (sigma = 2, checked for every length by the host test): on a complex or non-first axis N = n/2 and N = n/2 - 1 both give
the oversampled size n (n/2 - 1 is odd for every length: the odd kept count); on the real first axis N = M and N = M - 1 both give 2 M.

Partial workgroups: the strided passes meet them in their column groups (21 kept columns against groups of 16, 8 or 4).  The
contiguous-line kernels (real, complex, Toeplitz) cannot meet one through a plan: they run only where every other oversampled size
is in the table, all multiples of 16, so their line count is a multiple of every lines-per-workgroup value (16, 8, 4).
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
    extra = ""
    if getattr(c, "fftshift", False):
        extra += "-shift"
    if getattr(c, "C", 1) > 1:
        extra += f"-C{c.C}"
    kind = getattr(c, "kind", "halo")
    return f"{kind}-{Z}-n{c.n}-{'x'.join(str(d) for d in c.dims)}{extra}"
