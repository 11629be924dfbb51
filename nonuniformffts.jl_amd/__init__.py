"""nonuniformffts.jl_amd — MI355X-native backend for the GPU hot path of NonuniformFFTs.jl.

Python host mirror of the reference interface (``PlanNUFFT``, ``set_points!``, ``exec_type1!``,
``exec_type2!``) above the C ABI of ``libnufft_mi355x.so`` (include/nufft_mi355x.h).  Importing
this package loads the HIP library and raises if it has not been built: there is no fallback.

The directory name contains a dot, so load it with ``nufft_pkg.py`` at the repo root
(``from nufft_pkg import nufft``) or ``importlib``.
"""
from ._lib import LIB_PATH, lib  # noqa: F401  (fails loudly if the extension is missing)
from .plan import (  # noqa: F401
    BackwardsKaiserBesselKernel, BSplineKernel, DimensionMismatch, Direct, FastApproximation, GaussianKernel,
    HalfSupport, KaiserBesselKernel, ModeFactors, NUFFTCallbacks, PlanNUFFT, PointWeights, ROCBackend, default_kernel,
    default_kernel_evalmode, exec_type1, exec_type1_, exec_type2, exec_type2_, exec_type2_grad, interpolate, interpolate_grad,
    oversampled_grid,
    set_points, set_points_, sort_result, spread_from_points, transform_point_convention,
)
from .nfft_interface import NFFTPlan, plan_nfft  # noqa: F401
from .type3 import PlanNUFFT3, exec_type3, exec_type3_grad, set_points3  # noqa: F401
from .toeplitz import ToeplitzOperator, coil_combine, coil_expand  # noqa: F401
from .cg import ToeplitzCG  # noqa: F401
from .precond import ToeplitzPreconditioner  # noqa: F401
from .wavelet import WaveletTransform  # noqa: F401
from .llr import LocallyLowRank  # noqa: F401
from .fista import ToeplitzFISTA  # noqa: F401
from .tv import ToeplitzTV, TotalVariation  # noqa: F401
from .tgv import ToeplitzTGV  # noqa: F401
from .lps import GlobalLowRank, TemporalSparsity, ToeplitzLPS  # noqa: F401
from .dcf import DensityCompensation, density_weights  # noqa: F401
from .coilmaps import CoilMapEstimator, calibration_weights, estimate_maps  # noqa: F401
from .coilcomp import CoilCompressor, compress_coils  # noqa: F401
from .field import FieldSegments, field_corrected_operator  # noqa: F401
from . import autograd  # noqa: F401

__all__ = [
    "PlanNUFFT", "NUFFTCallbacks", "PointWeights", "ModeFactors", "HalfSupport", "Direct", "FastApproximation",
    "BackwardsKaiserBesselKernel", "KaiserBesselKernel", "GaussianKernel", "BSplineKernel", "ROCBackend", "DimensionMismatch",
    "set_points", "exec_type1", "exec_type2", "set_points_", "exec_type1_", "exec_type2_",
    "NFFTPlan", "plan_nfft",
    "PlanNUFFT3", "set_points3", "exec_type3", "exec_type3_grad",
    "exec_type2_grad", "interpolate_grad", "autograd",
    "ToeplitzOperator", "ToeplitzCG", "ToeplitzPreconditioner", "coil_expand", "coil_combine",
    "WaveletTransform", "LocallyLowRank", "ToeplitzFISTA", "TotalVariation", "ToeplitzTV", "ToeplitzTGV",
    "GlobalLowRank", "TemporalSparsity", "ToeplitzLPS",
    "DensityCompensation", "density_weights",
    "CoilMapEstimator", "estimate_maps", "calibration_weights",
    "CoilCompressor", "compress_coils",
    "FieldSegments", "field_corrected_operator",
]
