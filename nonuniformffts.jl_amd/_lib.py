"""ctypes binding of libnufft_mi355x.so (the C ABI declared in include/nufft_mi355x.h).

The library is the product: there is no CPU or PyTorch fallback.  If it is missing or cannot be
loaded, importing this module raises immediately.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NUFFT_LIB_PATH") or os.path.join(_HERE, "libnufft_mi355x.so")   # override: ablation builds

# error codes (include/nufft_mi355x.h)
OK = 0
ERR_INVALID_ARG = 1
ERR_SIZE_TOO_SMALL = 2
ERR_DIM_MISMATCH = 3
ERR_LDS_TOO_SMALL = 4
ERR_UNSUPPORTED = 5
ERR_NO_POINTS = 6
ERR_ALLOC = 7
ERR_HIP = 8
ERR_ROCFFT = 9
ERR_NO_DEVICE = 10

F32, F64 = 0, 1
EVAL_DIRECT, EVAL_FAST_APPROXIMATION = 0, 1
NUM_STAGES = 8
STAGE_NAMES = ("set_points", "t1_zero", "t1_spread", "t1_fft", "t1_deconv", "t2_deconv_pad", "t2_fft", "t2_interp")


class NufftParams(C.Structure):
    _fields_ = [
        ("dtype", C.c_int32), ("is_complex", C.c_int32), ("ndim", C.c_int32),
        ("N", C.c_int64 * 3),
        ("half_support", C.c_int32),
        ("sigma", C.c_double),
        ("kernel", C.c_int32), ("evalmode", C.c_int32), ("ntransforms", C.c_int32),
        ("fftshift", C.c_int32), ("point_transform", C.c_int32), ("gpu_method", C.c_int32),
        ("device", C.c_int32),
        ("tile_dims", C.c_int32 * 3),
        ("lds_budget_bytes", C.c_int32), ("spread_threads", C.c_int32), ("interp_threads", C.c_int32),
        ("interp_tile_dims", C.c_int32 * 3), ("bin_log2", C.c_int32),
        ("spread_method", C.c_int32),
        ("kernel_param", C.c_double),
        ("struct_size", C.c_int32), ("reserved", C.c_int32),
        ("kernel_param_dim", C.c_double * 3),
        ("N_over", C.c_int64 * 3),
        ("options", C.c_char_p),
    ]


class NufftCallbacks(C.Structure):
    _fields_ = [("point_weights", C.c_void_p), ("mode_factors", C.c_void_p)]


class NufftInfo(C.Structure):
    _fields_ = [
        ("dtype", C.c_int32), ("is_complex", C.c_int32), ("ndim", C.c_int32), ("half_support", C.c_int32),
        ("ntransforms", C.c_int32), ("evalmode", C.c_int32), ("fftshift", C.c_int32), ("device", C.c_int32),
        ("N", C.c_int64 * 3), ("N_over", C.c_int64 * 3), ("N_out", C.c_int64 * 3),
        ("sigma", C.c_double), ("beta", C.c_double * 3),
        ("bin_dims", C.c_int32 * 3), ("nbins", C.c_int32 * 3),
        ("spread_tile", C.c_int32 * 3), ("spread_ntiles", C.c_int32 * 3),
        ("interp_tile", C.c_int32 * 3), ("interp_ntiles", C.c_int32 * 3),
        ("spread_threads", C.c_int32), ("interp_threads", C.c_int32),
        ("lds_bytes_spread", C.c_int64), ("lds_bytes_interp", C.c_int64),
        ("workspace_bytes", C.c_int64), ("num_points", C.c_int64),
        ("npoly", C.c_int32), ("window_scale_log2", C.c_int32 * 3), ("kernel", C.c_int32),
        ("spread_max_items", C.c_int32), ("interp_max_items", C.c_int32), ("spread_method", C.c_int32),
        ("patch_dims", C.c_int32 * 2), ("patch_f32acc", C.c_int32), ("patch_planar", C.c_int32),
        ("ring_column", C.c_int32 * 2), ("ring_segments", C.c_int32), ("ring_halo", C.c_int32),
        ("sort_column", C.c_int32 * 2),
    ]


class NufftType3Params(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("sign", C.c_int32),
        ("source_center", C.c_double * 3), ("source_halfwidth", C.c_double * 3),
        ("target_center", C.c_double * 3), ("target_halfwidth", C.c_double * 3),
    ]


class NufftInfo3(C.Structure):
    _fields_ = [
        ("ndim", C.c_int32), ("ntransforms", C.c_int32), ("dtype", C.c_int32), ("half_support", C.c_int32),
        ("sign", C.c_int32), ("kernel", C.c_int32), ("evalmode", C.c_int32), ("device", C.c_int32),
        ("nf", C.c_int64 * 3), ("gamma", C.c_double * 3), ("h", C.c_double * 3),
        ("source_halfwidth", C.c_double * 3), ("target_halfwidth", C.c_double * 3),
        ("inner_N_over", C.c_int64 * 3), ("sigma", C.c_double), ("beta", C.c_double * 3),
        ("spread_method", C.c_int32), ("reserved", C.c_int32),
        ("num_sources", C.c_int64), ("num_targets", C.c_int64), ("workspace_bytes", C.c_int64),
    ]


class NufftToeplitzInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("ndim", C.c_int32), ("dtype", C.c_int32), ("ntransforms", C.c_int32),
        ("fftshift", C.c_int32), ("device", C.c_int32), ("path", C.c_int32), ("has_spectrum", C.c_int32),
        ("N", C.c_int64 * 3), ("N2", C.c_int64 * 3),
        ("multiplier_bytes", C.c_int64), ("workspace_bytes", C.c_int64),
    ]


TOEPLITZ_PATH_DENSE, TOEPLITZ_PATH_FUSED = 0, 1


class NufftCgParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("max_iter", C.c_int32), ("check_every", C.c_int32), ("reserved", C.c_int32),
        ("rtol", C.c_double), ("lambda_", C.c_double),
    ]


class NufftCgInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("ntransforms", C.c_int32), ("dtype", C.c_int32), ("max_iter", C.c_int32),
        ("check_every", C.c_int32), ("workgroups", C.c_int32), ("iterations_enqueued", C.c_int32), ("reserved", C.c_int32),
        ("rtol", C.c_double), ("lambda_", C.c_double), ("array_bytes", C.c_int64), ("workspace_bytes", C.c_int64),
    ]


CG_MAX_ITER, CG_CONVERGED, CG_BREAKDOWN = 0, 1, 2
CG_STATUS_NAMES = {CG_MAX_ITER: "max_iter", CG_CONVERGED: "converged", CG_BREAKDOWN: "breakdown"}


class NufftPrecondParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("reserved", C.c_int32), ("lambda_", C.c_double), ("floor", C.c_double),
    ]


class NufftPrecondInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("ndim", C.c_int32), ("dtype", C.c_int32), ("ntransforms", C.c_int32), ("device", C.c_int32),
        ("path", C.c_int32), ("scaling", C.c_int32), ("reserved", C.c_int32),
        ("N", C.c_int64 * 3), ("lambda_", C.c_double), ("mu", C.c_double), ("floor", C.c_double),
        ("max_e", C.c_double), ("min_e", C.c_double), ("multiplier_bytes", C.c_int64), ("workspace_bytes", C.c_int64),
    ]


PRECOND_PATH_DENSE, PRECOND_PATH_FUSED = 0, 1
PRECOND_SCALING_NONE, PRECOND_SCALING_MAPS, PRECOND_SCALING_CALLER = 0, 1, 2


class NufftWaveletParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("wavelet", C.c_int32), ("levels", C.c_int32), ("reserved", C.c_int32)]


class NufftWaveletInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("ndim", C.c_int32), ("dtype", C.c_int32), ("ntransforms", C.c_int32), ("device", C.c_int32),
        ("wavelet", C.c_int32), ("taps", C.c_int32), ("levels", C.c_int32),
        ("N", C.c_int64 * 3), ("scratch_bytes", C.c_int64), ("workspace_bytes", C.c_int64),
    ]


WAVELET_HAAR, WAVELET_DB2 = 0, 1
WAVELET_IDS = {"haar": WAVELET_HAAR, "db2": WAVELET_DB2}


class NufftFistaParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("max_iter", C.c_int32), ("check_every", C.c_int32), ("wavelet", C.c_int32),
        ("levels", C.c_int32), ("reserved", C.c_int32),
        ("tol", C.c_double), ("step", C.c_double), ("l1", C.c_double), ("lambda_", C.c_double),
    ]


class NufftFistaInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("ntransforms", C.c_int32), ("dtype", C.c_int32), ("max_iter", C.c_int32),
        ("check_every", C.c_int32), ("wavelet", C.c_int32), ("levels", C.c_int32), ("iterations_enqueued", C.c_int32),
        ("tol", C.c_double), ("step", C.c_double), ("lambda_", C.c_double), ("array_bytes", C.c_int64), ("workspace_bytes", C.c_int64),
    ]


class NufftLlrParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("block", C.c_int32 * 3), ("shifts", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64)]


class NufftLlrInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("ndim", C.c_int32), ("dtype", C.c_int32), ("ntransforms", C.c_int32), ("device", C.c_int32),
        ("block", C.c_int32 * 3), ("shifts", C.c_int32),
        ("N", C.c_int64 * 3), ("blocks", C.c_int64), ("workspace_bytes", C.c_int64),
        ("jacobi_sweeps_max", C.c_int32), ("waves_per_cu", C.c_int32),
    ]


FISTA_MAX_ITER, FISTA_CONVERGED, FISTA_BREAKDOWN = 0, 1, 2
FISTA_STATUS_NAMES = {FISTA_MAX_ITER: "max_iter", FISTA_CONVERGED: "converged", FISTA_BREAKDOWN: "breakdown"}


class NufftTvInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("ndim", C.c_int32), ("dtype", C.c_int32), ("ntransforms", C.c_int32), ("device", C.c_int32),
        ("tile", C.c_int32 * 3),
        ("N", C.c_int64 * 3), ("workgroups", C.c_int64), ("workspace_bytes", C.c_int64),
    ]


class NufftTvpdParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("max_iter", C.c_int32), ("check_every", C.c_int32), ("reserved", C.c_int32),
        ("tol", C.c_double), ("step", C.c_double), ("sigma", C.c_double), ("tv", C.c_double), ("lambda_", C.c_double),
    ]


class NufftTvpdInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("ntransforms", C.c_int32), ("dtype", C.c_int32), ("ndim", C.c_int32), ("max_iter", C.c_int32),
        ("check_every", C.c_int32), ("iterations_enqueued", C.c_int32), ("reserved", C.c_int32),
        ("tol", C.c_double), ("step", C.c_double), ("sigma", C.c_double), ("lambda_", C.c_double),
        ("array_bytes", C.c_int64), ("workspace_bytes", C.c_int64),
    ]


class NufftTvtParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("periodic", C.c_int32), ("spatial", C.c_int32), ("reserved", C.c_int32), ("tv_t", C.c_double)]


TVPD_MAX_ITER, TVPD_CONVERGED, TVPD_BREAKDOWN = 0, 1, 2
TVPD_STATUS_NAMES = {TVPD_MAX_ITER: "max_iter", TVPD_CONVERGED: "converged", TVPD_BREAKDOWN: "breakdown"}


class NufftTgvParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("max_iter", C.c_int32), ("check_every", C.c_int32), ("reserved", C.c_int32),
        ("tol", C.c_double), ("step", C.c_double), ("sigma", C.c_double), ("lambda_", C.c_double), ("alpha1", C.c_double),
        ("alpha0", C.c_double),
    ]


class NufftTgvInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("ntransforms", C.c_int32), ("dtype", C.c_int32), ("ndim", C.c_int32), ("max_iter", C.c_int32),
        ("check_every", C.c_int32), ("iterations_enqueued", C.c_int32), ("reserved", C.c_int32),
        ("tol", C.c_double), ("step", C.c_double), ("sigma", C.c_double), ("lambda_", C.c_double),
        ("array_bytes", C.c_int64), ("workspace_bytes", C.c_int64),
    ]


TGV_MAX_ITER, TGV_CONVERGED, TGV_BREAKDOWN = 0, 1, 2
TGV_STATUS_NAMES = {TGV_MAX_ITER: "max_iter", TGV_CONVERGED: "converged", TGV_BREAKDOWN: "breakdown"}


class NufftGlrInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("ndim", C.c_int32), ("dtype", C.c_int32), ("ntransforms", C.c_int32), ("device", C.c_int32),
        ("tile_cells", C.c_int32), ("jacobi_sweeps_max", C.c_int32), ("reserved", C.c_int32),
        ("N", C.c_int64 * 3), ("cells", C.c_int64), ("workgroups", C.c_int64), ("workspace_bytes", C.c_int64),
    ]


class NufftTsparseInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("ndim", C.c_int32), ("dtype", C.c_int32), ("ntransforms", C.c_int32), ("device", C.c_int32),
        ("transform", C.c_int32), ("tile_cells", C.c_int32), ("reserved", C.c_int32),
        ("N", C.c_int64 * 3), ("cells", C.c_int64), ("workgroups", C.c_int64), ("workspace_bytes", C.c_int64),
    ]


TSPARSE_IDENTITY, TSPARSE_DFT = 0, 1
TSPARSE_IDS = {"identity": TSPARSE_IDENTITY, "dft": TSPARSE_DFT}


class NufftLpsParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("max_iter", C.c_int32), ("check_every", C.c_int32), ("transform", C.c_int32),
        ("momentum", C.c_int32), ("reserved", C.c_int32),
        ("tol", C.c_double), ("step", C.c_double), ("lambda_", C.c_double), ("nuc", C.c_double), ("l1", C.c_double),
    ]


class NufftLpsInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("ntransforms", C.c_int32), ("dtype", C.c_int32), ("max_iter", C.c_int32),
        ("check_every", C.c_int32), ("transform", C.c_int32), ("momentum", C.c_int32), ("iterations_enqueued", C.c_int32),
        ("tol", C.c_double), ("step", C.c_double), ("lambda_", C.c_double), ("nuc", C.c_double), ("l1", C.c_double),
        ("array_bytes", C.c_int64), ("workspace_bytes", C.c_int64),
    ]


LPS_MAX_ITER, LPS_CONVERGED, LPS_BREAKDOWN = 0, 1, 2
LPS_STATUS_NAMES = {LPS_MAX_ITER: "max_iter", LPS_CONVERGED: "converged", LPS_BREAKDOWN: "breakdown"}


class NufftCoilmapsParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("box", C.c_int32 * 3), ("crop", C.c_double), ("reserved", C.c_int64 * 2)]


class NufftCoilmapsInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("ndim", C.c_int32), ("dtype", C.c_int32), ("ncoils", C.c_int32), ("device", C.c_int32),
        ("box", C.c_int32 * 3), ("tile", C.c_int32 * 3), ("tile_cells", C.c_int32), ("team_lanes", C.c_int32), ("teams", C.c_int32),
        ("staged", C.c_int32), ("lds_bytes", C.c_int32), ("jacobi_sweeps_max", C.c_int32), ("reserved", C.c_int32),
        ("crop", C.c_double), ("N", C.c_int64 * 3), ("cells", C.c_int64), ("workgroups", C.c_int64), ("workspace_bytes", C.c_int64),
    ]


class NufftCoilcompInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("dtype", C.c_int32), ("ncoils", C.c_int32), ("device", C.c_int32), ("threads", C.c_int32),
        ("tile_samples", C.c_int32), ("segments", C.c_int32), ("pairs", C.c_int32), ("pairs_per_thread", C.c_int32),
        ("max_workgroups", C.c_int32), ("apply_chunk", C.c_int32), ("jacobi_team_lanes", C.c_int32), ("jacobi_sweeps_max", C.c_int32),
        ("lds_bytes_gram", C.c_int32), ("lds_bytes_eigen", C.c_int32), ("matrix_rows", C.c_int32), ("has_noise", C.c_int32),
        ("reserved", C.c_int32),
        ("n", C.c_int64), ("tiles", C.c_int64), ("tiles_per_workgroup", C.c_int64), ("workgroups", C.c_int64), ("workspace_bytes", C.c_int64),
    ]


COILCOMP_OK, COILCOMP_SWEEPS, COILCOMP_NONFINITE = 0, 1, 2


class NufftDcfParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("max_iter", C.c_int32), ("check_every", C.c_int32), ("normalize", C.c_int32),
        ("tol", C.c_double),
    ]


class NufftDcfInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("ndim", C.c_int32), ("dtype", C.c_int32), ("device", C.c_int32), ("max_iter", C.c_int32),
        ("check_every", C.c_int32), ("normalize", C.c_int32), ("workgroups", C.c_int32), ("iterations_enqueued", C.c_int32),
        ("window_scale_log2", C.c_int32),
        ("N_over", C.c_int64 * 3), ("tol", C.c_double), ("beta", C.c_double * 3),
        ("capacity", C.c_int64), ("num_points", C.c_int64), ("workspace_bytes", C.c_int64), ("plan_bytes", C.c_int64),
    ]


DCF_MAX_ITER, DCF_CONVERGED, DCF_BREAKDOWN = 0, 1, 2
DCF_STATUS_NAMES = {DCF_MAX_ITER: "max_iter", DCF_CONVERGED: "converged", DCF_BREAKDOWN: "breakdown"}
DCF_NORMALIZE = {"sum": 0, "none": 1}

class NufftFieldsegInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("dtype", C.c_int32), ("nsegments", C.c_int32), ("nbins", C.c_int32), ("device", C.c_int32),
        ("threads", C.c_int32), ("segment_tier", C.c_int32), ("reseed_bins", C.c_int32), ("max_workgroups", C.c_int32),
        ("lds_bytes_interpolators", C.c_int32), ("lds_bytes_histogram", C.c_int32), ("bins_used", C.c_int32),
        ("workspace_bytes", C.c_int64),
    ]


NUM_STAGES3 = 6
STAGE_NAMES3 = ("prep_sources", "prep_targets", "premultiply", "spread", "type2", "postmultiply")


#: every symbol include/nufft_mi355x.h declares, with (restype, argtypes)
_P = C.c_void_p
_PP = C.POINTER(C.c_void_p)
SYMBOLS = {
    "nufft_plan_create_ex": (C.c_int, [C.POINTER(_P), C.POINTER(NufftParams)]),
    "nufft_plan_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int,
                                    C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "nufft_plan_destroy": (C.c_int, [_P]),
    "nufft_plan_info": (C.c_int, [_P, C.POINTER(NufftInfo)]),
    "nufft_plan_get_phi_hat": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.c_int64]),
    "nufft_plan_get_poly_coefs": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.c_int64]),
    "nufft_plan_get_index_map": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64), C.c_int64]),
    "nufft_set_points": (C.c_int, [_P, C.c_int64, _PP, _P]),
    "nufft_exec_type1": (C.c_int, [_P, _PP, _PP, _P]),
    "nufft_exec_type2": (C.c_int, [_P, _PP, _PP, _P]),
    "nufft_exec_type1_cb": (C.c_int, [_P, _PP, _PP, _P, _P]),
    "nufft_exec_type2_cb": (C.c_int, [_P, _PP, _PP, _P, _P]),
    "nufft_set_callbacks": (C.c_int, [_P, _P]),
    "nufft_fill_zeros": (C.c_int, [_P, _P]),
    "nufft_spread": (C.c_int, [_P, _PP, _P]),
    "nufft_spread_deferred": (C.c_int, [_P, _PP, _P]),
    "nufft_fft_forward": (C.c_int, [_P, _P]),
    "nufft_deconvolve_truncate": (C.c_int, [_P, _PP, _P]),
    "nufft_deconvolve_pad": (C.c_int, [_P, _PP, _P]),
    "nufft_fft_backward": (C.c_int, [_P, _P]),
    "nufft_interpolate": (C.c_int, [_P, _PP, _P]),
    "nufft_interpolate_grad": (C.c_int, [_P, _PP, _PP, _P]),
    "nufft_exec_type2_grad": (C.c_int, [_P, _PP, _PP, _PP, _P]),
    "nufft_complete_grid": (C.c_int, [_P, _P]),
    "nufft_grid_ptr": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "nufft_copy_grid": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int64, _P]),
    "nufft_get_sort_result": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_uint32), C.c_int64, _P]),
    "nufft_sort_columns_used": (C.c_int, [_P, C.POINTER(C.c_int), _P]),
    "nufft_steady_path_used": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "nufft_steady_path_observe": (C.c_int, [C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32]),
    "nufft_set_timing": (C.c_int, [_P, C.c_int]),
    "nufft_get_stage_times": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "nufft_spread_engine_used": (C.c_int, [_P, C.POINTER(C.c_int), _P]),
    "nufft_interp_engine_used": (C.c_int, [_P, C.POINTER(C.c_int), _P]),
    "nufft_plan_options": (C.c_char_p, [_P]),
    "nufft_workspace_breakdown": (C.c_int, [_P, C.c_char_p, C.c_int64]),
    "nufft_plan3_create": (C.c_int, [C.POINTER(_P), C.POINTER(NufftParams), C.POINTER(NufftType3Params)]),
    "nufft_plan3_destroy": (C.c_int, [_P]),
    "nufft_plan3_info": (C.c_int, [_P, C.POINTER(NufftInfo3)]),
    "nufft_set_points3": (C.c_int, [_P, C.c_int64, _PP, C.c_int64, _PP, _P]),
    "nufft_exec_type3": (C.c_int, [_P, _PP, _PP, _P]),
    "nufft_exec_type3_grad": (C.c_int, [_P, _PP, _PP, _PP, _P]),
    "nufft_type3_points_outside": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    "nufft_plan3_internal": (C.c_int, [_P, C.c_int, C.POINTER(_P)]),
    "nufft_set_timing3": (C.c_int, [_P, C.c_int]),
    "nufft_get_stage_times3": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "nufft_sizeof_type3_params": (C.c_int64, []),
    "nufft_sizeof_info3": (C.c_int64, []),
    "nufft_toeplitz_create": (C.c_int, [C.POINTER(_P), _P]),
    "nufft_toeplitz_destroy": (C.c_int, [_P]),
    "nufft_toeplitz_get_info": (C.c_int, [_P, C.POINTER(NufftToeplitzInfo)]),
    "nufft_toeplitz_set_spectrum": (C.c_int, [_P, _P, _P]),
    "nufft_toeplitz_set_points": (C.c_int, [_P, C.POINTER(NufftParams), C.c_int64, _PP, _P, _P]),
    "nufft_toeplitz_apply": (C.c_int, [_P, _PP, _PP, _P]),
    "nufft_toeplitz_multiplier_ptr": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "nufft_sizeof_toeplitz_info": (C.c_int64, []),
    "nufft_toeplitz_set_maps": (C.c_int, [_P, C.c_int32, _PP, _P]),
    "nufft_toeplitz_clear_maps": (C.c_int, [_P]),
    "nufft_toeplitz_num_coils": (C.c_int32, [_P]),
    "nufft_toeplitz_set_points_coupled": (C.c_int, [_P, C.POINTER(NufftParams), C.c_int64, _PP, _P, _PP, _P]),
    "nufft_toeplitz_set_spectra_coupled": (C.c_int, [_P, _PP, _P]),
    "nufft_toeplitz_num_coupled": (C.c_int32, [_P]),
    "nufft_toeplitz_multiplier_pair_ptr": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "nufft_coil_expand": (C.c_int, [C.c_int, C.c_int64, C.c_int32, _PP, _PP, _P, C.c_int, _P]),
    "nufft_coil_combine": (C.c_int, [C.c_int, C.c_int64, C.c_int32, _P, _PP, _PP, C.c_int, _P]),
    "nufft_cg_create": (C.c_int, [C.POINTER(_P), _P, C.POINTER(NufftCgParams)]),
    "nufft_cg_destroy": (C.c_int, [_P]),
    "nufft_cg_solve": (C.c_int, [_P, _PP, _PP, C.c_int, _P]),
    "nufft_cg_get_info": (C.c_int, [_P, C.POINTER(NufftCgInfo)]),
    "nufft_cg_get_result": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int64, _P]),
    "nufft_cg_history": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int64, _P]),
    "nufft_sizeof_cg_params": (C.c_int64, []),
    "nufft_sizeof_cg_info": (C.c_int64, []),
    "nufft_precond_create": (C.c_int, [C.POINTER(_P), _P, C.POINTER(NufftPrecondParams)]),
    "nufft_precond_destroy": (C.c_int, [_P]),
    "nufft_precond_update": (C.c_int, [_P, _P]),
    "nufft_precond_set_scaling": (C.c_int, [_P, _P]),
    "nufft_precond_apply": (C.c_int, [_P, _PP, _PP, _P]),
    "nufft_precond_get_info": (C.c_int, [_P, C.POINTER(NufftPrecondInfo)]),
    "nufft_precond_multiplier_ptr": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "nufft_precond_scaling_ptr": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "nufft_sizeof_precond_params": (C.c_int64, []),
    "nufft_sizeof_precond_info": (C.c_int64, []),
    "nufft_precond_create_block": (C.c_int, [C.POINTER(_P), _P, C.POINTER(NufftPrecondParams)]),
    "nufft_precond_num_coupled": (C.c_int32, [_P]),
    "nufft_precond_block_ptr": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "nufft_precond_floored_cells": (C.c_int64, [_P]),
    "nufft_cg_set_preconditioner": (C.c_int, [_P, _P]),
    "nufft_dcf_create": (C.c_int, [C.POINTER(_P), _P, C.POINTER(NufftDcfParams)]),
    "nufft_dcf_destroy": (C.c_int, [_P]),
    "nufft_dcf_set_points": (C.c_int, [_P, C.c_int64, _PP, _P]),
    "nufft_dcf_compute": (C.c_int, [_P, _P, C.c_int, _P]),
    "nufft_dcf_get_info": (C.c_int, [_P, C.POINTER(NufftDcfInfo)]),
    "nufft_dcf_get_result": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), _P]),
    "nufft_dcf_history": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int64, _P]),
    "nufft_sizeof_dcf_params": (C.c_int64, []),
    "nufft_sizeof_dcf_info": (C.c_int64, []),
    "nufft_wavelet_create": (C.c_int, [C.POINTER(_P), _P, C.POINTER(NufftWaveletParams)]),
    "nufft_wavelet_create_for_operator": (C.c_int, [C.POINTER(_P), _P, C.POINTER(NufftWaveletParams)]),
    "nufft_wavelet_destroy": (C.c_int, [_P]),
    "nufft_wavelet_get_info": (C.c_int, [_P, C.POINTER(NufftWaveletInfo)]),
    "nufft_wavelet_forward": (C.c_int, [_P, _PP, _PP, _P]),
    "nufft_wavelet_inverse": (C.c_int, [_P, _PP, _PP, _P]),
    "nufft_wavelet_shrink": (C.c_int, [_P, _PP, _PP, C.POINTER(C.c_double), _P, _P]),
    "nufft_sizeof_wavelet_params": (C.c_int64, []),
    "nufft_sizeof_wavelet_info": (C.c_int64, []),
    "nufft_toeplitz_max_eigenvalue": (C.c_int, [_P, _PP, C.c_int32, C.POINTER(C.c_double), _P]),
    "nufft_fista_create": (C.c_int, [C.POINTER(_P), _P, C.POINTER(NufftFistaParams)]),
    "nufft_fista_destroy": (C.c_int, [_P]),
    "nufft_fista_set_l1": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int64]),
    "nufft_fista_solve": (C.c_int, [_P, _PP, _PP, C.c_int, _P]),
    "nufft_fista_get_info": (C.c_int, [_P, C.POINTER(NufftFistaInfo)]),
    "nufft_fista_get_result": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int64, _P]),
    "nufft_fista_history": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int64, _P]),
    "nufft_sizeof_fista_params": (C.c_int64, []),
    "nufft_sizeof_fista_info": (C.c_int64, []),
    "nufft_llr_create": (C.c_int, [C.POINTER(_P), _P, C.POINTER(NufftLlrParams)]),
    "nufft_llr_create_for_operator": (C.c_int, [C.POINTER(_P), _P, C.POINTER(NufftLlrParams)]),
    "nufft_llr_destroy": (C.c_int, [_P]),
    "nufft_llr_get_info": (C.c_int, [_P, C.POINTER(NufftLlrInfo)]),
    "nufft_llr_apply": (C.c_int, [_P, _PP, _PP, C.c_double, C.POINTER(C.c_int32), _P, _P]),
    "nufft_sizeof_llr_params": (C.c_int64, []),
    "nufft_sizeof_llr_info": (C.c_int64, []),
    "nufft_fista_create_llr": (C.c_int, [C.POINTER(_P), _P, C.POINTER(NufftFistaParams), C.POINTER(NufftLlrParams), C.c_double]),
    "nufft_fista_set_nuc": (C.c_int, [_P, C.c_double]),
    "nufft_tv_create": (C.c_int, [C.POINTER(_P), _P]),
    "nufft_tv_create_for_operator": (C.c_int, [C.POINTER(_P), _P]),
    "nufft_tv_destroy": (C.c_int, [_P]),
    "nufft_tv_get_info": (C.c_int, [_P, C.POINTER(NufftTvInfo)]),
    "nufft_tv_gradient": (C.c_int, [_P, _PP, _PP, _P]),
    "nufft_tv_adjoint": (C.c_int, [_P, _PP, _PP, _P]),
    "nufft_tv_norm": (C.c_int, [_P, _PP, _P, _P]),
    "nufft_sizeof_tv_info": (C.c_int64, []),
    "nufft_tvpd_create": (C.c_int, [C.POINTER(_P), _P, C.POINTER(NufftTvpdParams)]),
    "nufft_tvpd_destroy": (C.c_int, [_P]),
    "nufft_tvpd_set_tv": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int64]),
    "nufft_tvpd_solve": (C.c_int, [_P, _PP, _PP, C.c_int, _P]),
    "nufft_tvpd_get_info": (C.c_int, [_P, C.POINTER(NufftTvpdInfo)]),
    "nufft_tvpd_get_result": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int64, _P]),
    "nufft_tvpd_history": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int64, _P]),
    "nufft_sizeof_tvpd_params": (C.c_int64, []),
    "nufft_sizeof_tvpd_info": (C.c_int64, []),
    "nufft_toeplitz_set_points_frames": (C.c_int, [_P, C.POINTER(NufftParams), C.POINTER(C.c_int64), _PP, _PP, _P]),
    "nufft_toeplitz_set_spectra_frames": (C.c_int, [_P, _PP, _P]),
    "nufft_toeplitz_num_frames": (C.c_int32, [_P]),
    "nufft_toeplitz_multiplier_frame_ptr": (C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "nufft_tv_gradient_t": (C.c_int, [_P, _PP, _PP, C.c_int, _P]),
    "nufft_tv_adjoint_t": (C.c_int, [_P, _PP, _PP, C.c_int, _P]),
    "nufft_tv_norm_t": (C.c_int, [_P, _PP, C.c_int, _P, _P]),
    "nufft_tvpd_create_temporal": (C.c_int, [C.POINTER(_P), _P, C.POINTER(NufftTvpdParams), C.POINTER(NufftTvtParams)]),
    "nufft_tvpd_set_tv_t": (C.c_int, [_P, C.c_double]),
    "nufft_tvpd_get_temporal": (C.c_int, [_P, C.POINTER(NufftTvtParams)]),
    "nufft_sizeof_tvt_params": (C.c_int64, []),
    "nufft_glr_create": (C.c_int, [C.POINTER(_P), _P]),
    "nufft_glr_create_for_operator": (C.c_int, [C.POINTER(_P), _P]),
    "nufft_glr_destroy": (C.c_int, [_P]),
    "nufft_glr_get_info": (C.c_int, [_P, C.POINTER(NufftGlrInfo)]),
    "nufft_glr_apply": (C.c_int, [_P, _PP, _PP, C.c_double, _P, _P]),
    "nufft_glr_last_sweeps": (C.c_int, [_P, C.POINTER(C.c_int32), _P]),
    "nufft_sizeof_glr_info": (C.c_int64, []),
    "nufft_tsparse_create": (C.c_int, [C.POINTER(_P), _P, C.c_int32]),
    "nufft_tsparse_create_for_operator": (C.c_int, [C.POINTER(_P), _P, C.c_int32]),
    "nufft_tsparse_destroy": (C.c_int, [_P]),
    "nufft_tsparse_get_info": (C.c_int, [_P, C.POINTER(NufftTsparseInfo)]),
    "nufft_tsparse_forward": (C.c_int, [_P, _PP, _PP, _P]),
    "nufft_tsparse_inverse": (C.c_int, [_P, _PP, _PP, _P]),
    "nufft_tsparse_shrink": (C.c_int, [_P, _PP, _PP, C.c_double, _P, _P]),
    "nufft_sizeof_tsparse_info": (C.c_int64, []),
    "nufft_lps_create": (C.c_int, [C.POINTER(_P), _P, C.POINTER(NufftLpsParams)]),
    "nufft_lps_destroy": (C.c_int, [_P]),
    "nufft_lps_set_weights": (C.c_int, [_P, C.c_double, C.c_double]),
    "nufft_lps_solve": (C.c_int, [_P, _PP, _PP, C.c_int, _P]),
    "nufft_lps_get_parts": (C.c_int, [_P, _PP, _PP, _P]),
    "nufft_lps_get_info": (C.c_int, [_P, C.POINTER(NufftLpsInfo)]),
    "nufft_lps_get_result": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int64, _P]),
    "nufft_lps_history": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int64, _P]),
    "nufft_sizeof_lps_params": (C.c_int64, []),
    "nufft_sizeof_lps_info": (C.c_int64, []),
    "nufft_coilmaps_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int32, C.c_int, C.POINTER(NufftCoilmapsParams)]),
    "nufft_coilmaps_create_for_operator": (C.c_int, [C.POINTER(_P), _P, C.c_int32, C.POINTER(NufftCoilmapsParams)]),
    "nufft_coilmaps_destroy": (C.c_int, [_P]),
    "nufft_coilmaps_get_info": (C.c_int, [_P, C.POINTER(NufftCoilmapsInfo)]),
    "nufft_coilmaps_estimate": (C.c_int, [_P, _PP, _PP, C.POINTER(C.c_double), _P, _P, _P]),
    "nufft_coilmaps_layout": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int32, C.POINTER(NufftCoilmapsParams), C.POINTER(NufftCoilmapsInfo)]),
    "nufft_coilmaps_apply_crop": (C.c_int, [_P, _PP, _P, C.c_double, _P]),
    "nufft_coilmaps_last_sweeps": (C.c_int, [_P, C.POINTER(C.c_int32), _P]),
    "nufft_sizeof_coilmaps_params": (C.c_int64, []),
    "nufft_sizeof_coilmaps_info": (C.c_int64, []),
    "nufft_coilcomp_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int32, C.c_int]),
    "nufft_coilcomp_destroy": (C.c_int, [_P]),
    "nufft_coilcomp_layout": (C.c_int, [C.c_int, C.c_int32, C.c_int64, C.POINTER(NufftCoilcompInfo)]),
    "nufft_coilcomp_get_info": (C.c_int, [_P, C.c_int64, C.POINTER(NufftCoilcompInfo)]),
    "nufft_coilcomp_whitening_matrix": (C.c_int, [C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "nufft_coilcomp_set_noise_covariance": (C.c_int, [_P, C.POINTER(C.c_double), _P]),
    "nufft_coilcomp_reset": (C.c_int, [_P, _P]),
    "nufft_coilcomp_accumulate": (C.c_int, [_P, _PP, _P, C.c_int64, _P]),
    "nufft_coilcomp_finish": (C.c_int, [_P, _P]),
    "nufft_coilcomp_set_matrix": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int32, _P]),
    "nufft_coilcomp_apply": (C.c_int, [_P, _PP, C.c_int32, _PP, C.c_int64, _P]),
    "nufft_coilcomp_get_gram": (C.c_int, [_P, C.POINTER(C.c_double), _P]),
    "nufft_coilcomp_get_matrix": (C.c_int, [_P, C.POINTER(C.c_double), _P]),
    "nufft_coilcomp_get_spectrum": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P]),
    "nufft_sizeof_coilcomp_info": (C.c_int64, []),
    "nufft_toeplitz_create_segmented": (C.c_int, [C.POINTER(_P), _P, C.c_int32]),
    "nufft_toeplitz_num_segments": (C.c_int32, [_P]),
    "nufft_toeplitz_set_factors": (C.c_int, [_P, _PP, _P]),
    "nufft_toeplitz_clear_factors": (C.c_int, [_P]),
    "nufft_fieldseg_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int32, C.c_int32, C.c_int]),
    "nufft_fieldseg_destroy": (C.c_int, [_P]),
    "nufft_fieldseg_layout": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.POINTER(NufftFieldsegInfo)]),
    "nufft_fieldseg_get_info": (C.c_int, [_P, C.POINTER(NufftFieldsegInfo)]),
    "nufft_fieldseg_fit": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_double), C.c_double, _P]),
    "nufft_fieldseg_interpolators": (C.c_int, [_P, _P, C.c_int64, _PP, _P]),
    "nufft_fieldseg_factors": (C.c_int, [_P, _P, C.c_int64, _PP, _P]),
    "nufft_fieldseg_get_histogram": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_double), _P]),
    "nufft_fieldseg_get_gram": (C.c_int, [_P, C.POINTER(C.c_double), _P]),
    "nufft_fieldseg_get_solver_matrix": (C.c_int, [_P, C.POINTER(C.c_double), _P]),
    "nufft_fieldseg_get_tau": (C.c_int, [_P, C.POINTER(C.c_double), _P]),
    "nufft_sizeof_fieldseg_info": (C.c_int64, []),
    "nufft_tv_sym_gradient": (C.c_int, [_P, _PP, _PP, _P]),
    "nufft_tv_sym_adjoint": (C.c_int, [_P, _PP, _PP, _P]),
    "nufft_tv_sym_norm": (C.c_int, [_P, _PP, _P, _P]),
    "nufft_tgv_create": (C.c_int, [C.POINTER(_P), _P, C.POINTER(NufftTgvParams)]),
    "nufft_tgv_destroy": (C.c_int, [_P]),
    "nufft_tgv_set_weights": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64]),
    "nufft_tgv_solve": (C.c_int, [_P, _PP, _PP, C.c_int, _P]),
    "nufft_tgv_get_info": (C.c_int, [_P, C.POINTER(NufftTgvInfo)]),
    "nufft_tgv_get_result": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int64, _P]),
    "nufft_tgv_history": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int64, _P]),
    "nufft_tgv_copy_field": (C.c_int, [_P, _PP, _P]),
    "nufft_sizeof_tgv_params": (C.c_int64, []),
    "nufft_sizeof_tgv_info": (C.c_int64, []),
    "nufft_sizeof_params": (C.c_int64, []),
    "nufft_sizeof_info": (C.c_int64, []),
    "nufft_strerror": (C.c_char_p, [C.c_int]),
    "nufft_last_error_message": (C.c_char_p, []),
    "nufft_version": (C.c_int, []),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (or `make -C nonuniformffts.jl_amd/csrc`). "
            "There is no CPU fallback.")
    try:
        # torch ships its own ROCm runtime with the same sonames; importing it first makes this
        # library bind to the runtime that owns the caller's tensors.
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is only needed for device memory
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)   # AttributeError if the header and the library disagree
        fn.restype = res
        fn.argtypes = args
    # the two structs are mirrored by hand above: refuse a library whose layout differs
    for name, mirror in (("nufft_sizeof_params", NufftParams), ("nufft_sizeof_info", NufftInfo),
                         ("nufft_sizeof_type3_params", NufftType3Params), ("nufft_sizeof_info3", NufftInfo3),
                         ("nufft_sizeof_toeplitz_info", NufftToeplitzInfo), ("nufft_sizeof_cg_params", NufftCgParams),
                         ("nufft_sizeof_cg_info", NufftCgInfo), ("nufft_sizeof_precond_params", NufftPrecondParams),
                         ("nufft_sizeof_precond_info", NufftPrecondInfo), ("nufft_sizeof_dcf_params", NufftDcfParams),
                         ("nufft_sizeof_dcf_info", NufftDcfInfo), ("nufft_sizeof_wavelet_params", NufftWaveletParams),
                         ("nufft_sizeof_wavelet_info", NufftWaveletInfo), ("nufft_sizeof_fista_params", NufftFistaParams),
                         ("nufft_sizeof_fista_info", NufftFistaInfo), ("nufft_sizeof_llr_params", NufftLlrParams),
                         ("nufft_sizeof_llr_info", NufftLlrInfo), ("nufft_sizeof_tv_info", NufftTvInfo),
                         ("nufft_sizeof_tvpd_params", NufftTvpdParams), ("nufft_sizeof_tvpd_info", NufftTvpdInfo),
                         ("nufft_sizeof_tvt_params", NufftTvtParams), ("nufft_sizeof_glr_info", NufftGlrInfo),
                         ("nufft_sizeof_tsparse_info", NufftTsparseInfo), ("nufft_sizeof_lps_params", NufftLpsParams),
                         ("nufft_sizeof_lps_info", NufftLpsInfo), ("nufft_sizeof_coilmaps_params", NufftCoilmapsParams),
                         ("nufft_sizeof_coilmaps_info", NufftCoilmapsInfo), ("nufft_sizeof_coilcomp_info", NufftCoilcompInfo),
                         ("nufft_sizeof_fieldseg_info", NufftFieldsegInfo), ("nufft_sizeof_tgv_params", NufftTgvParams),
                         ("nufft_sizeof_tgv_info", NufftTgvInfo)):
        if getattr(lib, name)() != C.sizeof(mirror):
            raise ImportError(f"{LIB_PATH}: {name}() = {getattr(lib, name)()} but the ctypes mirror has {C.sizeof(mirror)} bytes "
                              "(include/nufft_mi355x.h and _lib.py disagree)")
    return lib


lib = _load()


def error_message(code: int) -> str:
    base = lib.nufft_strerror(code).decode()
    detail = lib.nufft_last_error_message().decode()
    return f"{base}: {detail}" if detail else base
