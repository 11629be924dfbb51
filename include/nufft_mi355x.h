/*
 * nufft_mi355x.h — C ABI of the MI355X-native NUFFT engine (libnufft_mi355x.so).
 *
 * Drop-in boundary for the GPU hot path of jipolanco/NonuniformFFTs.jl
 * (PlanNUFFT -> set_points! -> exec_type1! / exec_type2!).  The reference has no FFI: its
 * backend "plugin API" is multiple dispatch on a KernelAbstractions backend plus the hooks of
 * ext/NonuniformFFTsAMDGPUExt.jl.  Each entry point below names the reference generic
 * function (file:line relative to the reference checkout) that a Julia `ccall` shim would
 * route to it; INTEGRATION.md shows that shim.
 *
 * Conventions (identical to the reference):
 *   - all data pointers are DEVICE pointers owned by the caller (ROCArray / torch tensor);
 *   - arrays are column-major ("dimension 1 fastest"), coordinates are structure-of-arrays;
 *   - no entry point synchronises the device: all work is enqueued on the `stream` argument
 *     (a hipStream_t passed as void*; NULL = the default stream);
 *   - errors are return codes, never exceptions; nothing is launched when a check fails;
 *   - the plan owns its scratch (oversampled grids, bin-sort buffers, rocFFT plans);
 *   - one plan must not be used concurrently from several threads (same as the reference).
 *
 * No torch / Julia / C++ types appear in any signature.
 */
#ifndef NUFFT_MI355X_H
#define NUFFT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NUFFT_MI355X_VERSION 104 /* 0.1.4: nufft_params.struct_size (was reserved[0]) and .options (appended); the library no longer reads NUFFT_*
                                    environment variables; nufft_plan_options, nufft_workspace_breakdown added;
                                    0.1.3: nufft_params grew (kernel_param_dim, N_over; nufft_info: sort_column: what a binding that already holds the reference's
                                    per-dimension kernel data forwards verbatim), NUFFT_METHOD_GLOBAL_MEMORY accepted, nufft_copy_grid
                                    takes a non-const plan since 102;
                                    0.1.2: nufft_spread_deferred added, nufft_info.reserved_info became ring_halo (same layout) since 101;
                                    0.1.1: nufft_info grew (patch_dims .. ring_segments) since 100 — a caller built against an older
                                    header must compare nufft_sizeof_info() / nufft_version() with its own before nufft_plan_info() */

/* ---- return codes ------------------------------------------------------------------- */
enum {
    NUFFT_OK = 0,
    NUFFT_ERR_INVALID_ARG   = 1, /* Julia ArgumentError (bad enum/eltype/null pointer)            */
    NUFFT_ERR_SIZE_TOO_SMALL = 2, /* ArgumentError "data size is too small" src/plan.jl:545-556    */
    NUFFT_ERR_DIM_MISMATCH  = 3, /* DimensionMismatch src/NonuniformFFTs.jl:92-114                */
    NUFFT_ERR_LDS_TOO_SMALL = 4, /* ArgumentError of block_dims_gpu_shmem src/gpu_common.jl:55-65 */
    NUFFT_ERR_UNSUPPORTED   = 5, /* feature outside the built menu (kernel, M, gpu_method, ...)   */
    NUFFT_ERR_NO_POINTS     = 6, /* exec_* before set_points                                      */
    NUFFT_ERR_ALLOC         = 7, /* hipMalloc failed                                              */
    NUFFT_ERR_HIP           = 8, /* any other HIP runtime error                                   */
    NUFFT_ERR_ROCFFT        = 9, /* rocFFT plan creation / execution failed                       */
    NUFFT_ERR_NO_DEVICE     = 10 /* device entry point called on a host-only (device = -1) plan   */
};

/* ---- enums --------------------------------------------------------------------------- */
enum { NUFFT_F32 = 0, NUFFT_F64 = 1 };                         /* real(Z) of the plan            */
enum {                                                          /* the four kernels of src/Kernels */
    NUFFT_KERNEL_BACKWARDS_KAISER_BESSEL = 0,  /* default_kernel(::ROCBackend), kaiser_bessel_backwards.jl */
    NUFFT_KERNEL_KAISER_BESSEL           = 1,  /* KaiserBesselKernel, kaiser_bessel.jl                     */
    NUFFT_KERNEL_GAUSSIAN                = 2,  /* GaussianKernel, gaussian.jl                              */
    NUFFT_KERNEL_BSPLINE                 = 3   /* BSplineKernel, bspline.jl                                */
};
enum { NUFFT_EVAL_DIRECT = 0, NUFFT_EVAL_FAST_APPROXIMATION = 1 }; /* Kernels.EvaluationMode     */
enum {                                                          /* gpu_method (src/blocking/gpu.jl:26): scheduling-only in the   */
    NUFFT_METHOD_SHARED_MEMORY = 0,                             /* reference (same sums, src/spreading/gpu.jl:168-214); every    */
    NUFFT_METHOD_GLOBAL_MEMORY = 1                              /* plan here runs the LDS engines, both values are accepted      */
};
enum {
    NUFFT_POINT_TRANSFORM_IDENTITY = 0, /* point_transform = identity (src/plan.jl:476)                    */
    NUFFT_POINT_TRANSFORM_NFFT     = 1  /* _transform_point_convention, src/abstractNFFTs.jl:147-155:
                                           x in [-1/2, 1/2), opposite sign of the exponent (plan_nfft)     */
};

/* Stage identifiers (nufft_get_stage_times), in the order of the reference's TimerOutputs
 * labels: src/blocking/gpu.jl:93-139, src/NonuniformFFTs.jl:157-186,246-283. */
enum {
    NUFFT_STAGE_SET_POINTS = 0, /* "Set points": bin-sort of the points                           */
    NUFFT_STAGE_T1_ZERO    = 1, /* "(0) Fill with zeros"                                          */
    NUFFT_STAGE_T1_SPREAD  = 2, /* "(1) Spreading"                                                */
    NUFFT_STAGE_T1_FFT     = 3, /* "(2) Forward FFT"                                              */
    NUFFT_STAGE_T1_DECONV  = 4, /* "(3) Deconvolution"                                            */
    NUFFT_STAGE_T2_DECONV  = 5, /* "(0)+(1) zero-pad + deconvolution" (fused)                     */
    NUFFT_STAGE_T2_FFT     = 6, /* "(2) Backward FFT"                                             */
    NUFFT_STAGE_T2_INTERP  = 7, /* "(3) Interpolation"                                            */
    NUFFT_NUM_STAGES       = 8
};

typedef struct nufft_plan nufft_plan; /* opaque */

/* Plan parameters: the keyword arguments of PlanNUFFT (src/plan.jl:467-482,568-599) that can
 * cross a C ABI, plus the MI355X tile knobs that replace `block_size` / `gpu_batch_size`.
 * Zero-initialise, then set what you need (0 means "reference default" for every field). */
typedef struct nufft_params {
    int32_t dtype;           /* NUFFT_F32 | NUFFT_F64  = real(Z)                                  */
    int32_t is_complex;      /* Z <: Complex (non-uniform values are complex)                     */
    int32_t ndim;            /* 1..3                                                               */
    int64_t N[3];            /* uniform grid size Ns (dimension 1 first)                           */
    int32_t half_support;    /* m = HalfSupport(M); 0 -> 4 (src/plan.jl:583)                       */
    double  sigma;           /* oversampling factor; 0 -> 2.0 (src/plan.jl:573)                    */
    int32_t kernel;          /* NUFFT_KERNEL_*                                                     */
    int32_t evalmode;        /* NUFFT_EVAL_*; the ROC default is Direct (ext/..AMDGPUExt.jl:56)    */
    int32_t ntransforms;     /* ntransforms = Val(C); 0 -> 1                                       */
    int32_t fftshift;        /* fftshift = true/false (src/plan.jl:472)                            */
    int32_t point_transform; /* NUFFT_POINT_TRANSFORM_*                                            */
    int32_t gpu_method;      /* NUFFT_METHOD_*                                                     */
    int32_t device;          /* HIP device ordinal; -1 = host-only plan (parameter math only)      */
    /* --- MI355X tuning knobs (0 = automatic) --- */
    int32_t tile_dims[3];    /* spreading tile (cells; replaces block_dims_gpu_shmem's cube)       */
    int32_t lds_budget_bytes;/* LDS bytes the tile search may use (<= 163840 on gfx950)            */
    int32_t spread_threads;  /* workgroup size of the spreading kernel (multiple of 64)            */
    int32_t interp_threads;  /* workgroup size of the interpolation kernel                         */
    int32_t interp_tile_dims[3]; /* interpolation tile interior (cells)                            */
    int32_t bin_log2;        /* log2 of the bin edge of the point sort (default 2: 4^D cells)      */
    int32_t spread_method;   /* NUFFT_SPREAD_* (0 = automatic: MFMA patches where they apply)       */
    double  kernel_param;    /* KaiserBesselKernel(β) / BackwardsKaiserBesselKernel(β) / GaussianKernel(ℓ):
                                explicit shape parameter; 0 -> the optimal one for (M, σ)              */
    int32_t struct_size;     /* sizeof(nufft_params) of the CALLER's header (ABI >= 104; the slot was reserved[0]): the library reads only
                                that many bytes and treats the rest as zero.  0 = the layout of ABI <= 102, which ends here: every field
                                below is then ignored — a caller that fills them must set struct_size                              */
    int32_t reserved;
    double  kernel_param_dim[3]; /* per-dimension shape parameter, as the reference's kernel data holds it (the field β of
                                    BackwardsKaiserBesselKernelData / KaiserBesselKernelData, kaiser_bessel_backwards.jl:84,
                                    kaiser_bessel.jl:112; σ / Δx of GaussianKernelData, gaussian.jl:67,76-78): an entry > 0 overrides
                                    kernel_param and the optimal value for that dimension, so a binding forwards p.kernels[d] verbatim */
    int64_t N_over[3];       /* oversampled grid size Ñ_d (gridsize(p.kernels[d]), src/Kernels/Kernels.jl:87): an entry > 0 replaces the
                                size rule of src/plan.jl:485-498 for that dimension (it must be even in dimension 1 of a real plan
                                and >= N_d); sigma is then only reported */
    const char* options;     /* development switches of this plan, "NUFFT_NAME=value;NUFFT_OTHER=value" (DESIGN.md section 4.3 lists them;
                                A/B experiments and tests of rarely taken paths — the defaults are the measured optimum), or NULL.
                                The library reads no environment variable: what changes a plan is in this struct.  Copied at
                                plan creation; nufft_plan_options() returns the canonical form the plan holds                  */
} nufft_params;

/* What show(::PlanNUFFT) prints (src/plan.jl:362-392) plus sizes a caller needs. */
/* Spreading engines (nufft_info.spread_method; nufft_params.spread_method selects, 0 = automatic):
 *   LDS tiles    — output-driven LDS tile with native ds_add_f64 (every D, M, kernel, grid size)
 *   MFMA patches — register-resident patches accumulated by the matrix pipe (3-D grids of 4-cell bins):
 *                  v_mfma_f64_4x4x4_4b with Float64 accumulators, or — ComplexF32 plans whose dimension 3 is a
 *                  multiple of 8 cells — v_mfma_f32_16x16x4 with Float32 accumulators (nufft_info.patch_f32acc)
 *   marching ring — a workgroup owns a column of the grid and marches along dimension 3 with a ring of 2M - 1 + 4 planes in
 *                  LDS (ds_add_f64 as for the tiles, 1.4 - 1.5 point visits per point instead of 2.1, finished planes leave with
 *                  coalesced stores while the ring moves on): 3-D grids of 4-cell bins; the automatic choice for real data, M <= 4
 *   marching ring, dense — the same window for dense point sets (mean load of the 4^3-cell bins above a threshold per M, decided per point
 *                  set by nufft_set_points): the points of a bin are accumulated in registers by v_mfma_f64_16x16x4 and flushed to the
 *                  window once per bin.  Reported by nufft_spread_engine_used only (never a plan parameter). */
enum { NUFFT_SPREAD_AUTO = 0, NUFFT_SPREAD_LDS_TILES = 1, NUFFT_SPREAD_MFMA_PATCHES = 2, NUFFT_SPREAD_MARCHING_RING = 3,
       NUFFT_SPREAD_MARCHING_RING_DENSE = 4 };

typedef struct nufft_info {
    int32_t dtype, is_complex, ndim, half_support, ntransforms, evalmode, fftshift, device;
    int64_t N[3];            /* Ns                                                                 */
    int64_t N_over[3];       /* oversampled grid dims  (src/plan.jl:485-498)                       */
    int64_t N_out[3];        /* size(p): dims of the uniform arrays (src/plan.jl:426)              */
    double  sigma;           /* actual sigma = max(N_over / N) (src/plan.jl:500)                   */
    double  beta[3];         /* kernel shape parameter per dimension (β; ℓ/Δx for the Gaussian; 0: B-spline) */
    int32_t bin_dims[3];     /* cells per sort bin                                                 */
    int32_t nbins[3];        /* bins per dimension                                                 */
    int32_t spread_tile[3];  /* spreading tile: interior cells held in LDS (no halo)               */
    int32_t spread_ntiles[3];
    int32_t interp_tile[3];  /* interpolation tile interior; LDS holds interior + 2M - 1           */
    int32_t interp_ntiles[3];
    int32_t spread_threads, interp_threads;
    int64_t lds_bytes_spread, lds_bytes_interp;
    int64_t workspace_bytes; /* device bytes owned by the plan right now                           */
    int64_t num_points;      /* Np of the last set_points                                          */
    int32_t npoly;           /* M + 4 polynomial coefficients per sub-interval                     */
    int32_t window_scale_log2[3]; /* device windows and phi_hat are scaled by 2^k_d (exact) */
    int32_t kernel;          /* NUFFT_KERNEL_*                                                     */
    int32_t spread_max_items, interp_max_items; /* capacity of the per-tile work-item tables (runs of sorted points) */
    int32_t spread_method;   /* NUFFT_SPREAD_LDS_TILES, _MFMA_PATCHES or _MARCHING_RING (what nufft_spread launches)  */
    int32_t patch_dims[2];   /* MFMA patches: cube columns (of 4 x 4 cells) a wave owns along dimensions 1, 2; 0 otherwise */
    int32_t patch_f32acc;    /* MFMA patches: 1 = ComplexF32 on v_mfma_f32_16x16x4 with Float32 accumulators (the reference's
                                accumulation type, src/spreading/gpu.jl:271-283), 0 = v_mfma_f64_4x4x4 with Float64 ones  */
    int32_t patch_planar;    /* MFMA patches: real plans with ntransforms = 2 / 3 spread that many components together (shared window
                                evaluation and operands — the reference's TODO at src/spreading/gpu.jl:293); 0 = one at a time    */
    int32_t ring_column[2];  /* marching ring: cells of a workgroup's column along dimensions 1, 2; 0 otherwise         */
    int32_t ring_segments;   /* marching ring: segments a column is cut into along dimension 3 for uniform point sets  */
    int32_t ring_halo;       /* marching ring: 1 = halo variant (every point spread once by its own column; the stencil reach
                                travels through a side buffer that the first FFT pass adds), 0 = clipped columns          */
    int32_t sort_column[2];  /* plans whose spreading window (halo variant) and interpolation ring own the same columns: bins of a column
                                along dimensions 1, 2 — set_points then groups the points by (column, layer of bins) only, unless a
                                ring hands the point set to the tile kernels (nufft_sort_columns_used); 0: always the fine bins   */
} nufft_info;

/* ---- plan lifetime -------------------------------------------------------------------- */

/* PlanNUFFT(Z, Ns; m, σ, kernel, ntransforms, backend = ROCBackend(), kernel_evalmode, fftshift,
 * gpu_method = :shared_memory) -> _PlanNUFFT, src/plan.jl:467-541; BlockDataGPU src/blocking/gpu.jl:41-69;
 * init_plan_data (grids + FFT plans) src/plan.jl:37-60. */
int nufft_plan_create_ex(nufft_plan** out, const nufft_params* params);

/* Flat-argument form of the same constructor (what SURVEY.md §8(b) lists). */
int nufft_plan_create(nufft_plan** out, int dtype, int is_complex, int ndim, const int64_t* N,
                      int half_support, double sigma, int kernel, int evalmode, int ntransforms,
                      int fftshift, int point_transform, int device);

/* Julia finalizer of the plan. */
int nufft_plan_destroy(nufft_plan* plan);

/* size(p), ndims(p), ntransforms(p), show(p): src/plan.jl:360-435. */
int nufft_plan_info(const nufft_plan* plan, nufft_info* out);

/* Plan-time host arrays, for inspection and tests:
 *   phi_hat : Kernels.fourier_coefficients(g), src/Kernels/Kernels.jl:84 (length N_out[dim])
 *   poly    : piecewise-polynomial coefficients cs[k][j], k < npoly, j < 2M
 *             (src/Kernels/piecewise_polynomial.jl:50-74), row-major [npoly][2M]
 *   index_map : non_oversampled_indices!, src/NonuniformFFTs.jl:318-348, 0-based */
int nufft_plan_get_phi_hat(const nufft_plan* plan, int dim, double* out, int64_t capacity);
int nufft_plan_get_poly_coefs(const nufft_plan* plan, int dim, double* out, int64_t capacity);
int nufft_plan_get_index_map(const nufft_plan* plan, int dim, int64_t* out, int64_t capacity);

/* ---- the hot path --------------------------------------------------------------------- */

/* set_points!(p, (xs, ys, zs)) -> set_points_impl!(::GPU, ...), src/set_points.jl:33-52,
 * src/blocking/gpu.jl:73-142.  coords[d] = device vector of Np reals of the plan's precision.
 * The coordinates are folded to [0, 2π) and bin-sorted by LDS tile into plan-owned storage; the
 * caller's arrays are only read (and, unlike the reference, need not stay alive afterwards). */
int nufft_set_points(nufft_plan* plan, int64_t num_points, const void* const* coords, void* stream);

/* exec_type1!(ûs_k, p, vp), src/NonuniformFFTs.jl:148-195.
 * values_in[c]: device vector Z[Np]; uhat_out[c]: device array complex(T)[N_out...]. */
int nufft_exec_type1(nufft_plan* plan, void* const* uhat_out, const void* const* values_in, void* stream);

/* exec_type2!(vp, p, ûs_k), src/NonuniformFFTs.jl:237-291. */
int nufft_exec_type2(nufft_plan* plan, void* const* values_out, const void* const* uhat_in, void* stream);

/* exec_type1!(ûs, p, vp; callbacks) / exec_type2!(vp, p, ûs; callbacks), src/NonuniformFFTs.jl:148-195,237-291,
 * for the two documented uses of NUFFTCallbacks (src/plan.jl:105-143, test/callbacks.jl:17-25) — arbitrary
 * closures cannot cross a C ABI:
 *   point_weights  T[Np]  (device, real, in the caller's point order): callbacks.nonuniform = (v, n) -> v * w[n],
 *                  applied to the values read by type 1 / written by type 2 (src/spreading/gpu.jl:289,
 *                  src/interpolation/gpu.jl:254);
 *   mode_factors   T[N_out...] (device, real, same layout as one uniform array, shared by all components):
 *                  callbacks.uniform = (w, idx) -> w * f[idx], applied to the modes written by type 1 / read by
 *                  type 2 (src/NonuniformFFTs.jl:395-399,461-464).
 * Either pointer may be NULL (identity).  Both are fused into existing kernels: no extra pass over the data. */
typedef struct nufft_callbacks {
    const void* point_weights;
    const void* mode_factors;
} nufft_callbacks;
int nufft_exec_type1_cb(nufft_plan* plan, void* const* uhat_out, const void* const* values_in,
                        const nufft_callbacks* callbacks, void* stream);
int nufft_exec_type2_cb(nufft_plan* plan, void* const* values_out, const void* const* uhat_in,
                        const nufft_callbacks* callbacks, void* stream);

/* ---- stage-level entry points (the backend-dispatched generic functions) -- */

/* The callback menu (above) for the stage-level entry points below: `callbacks.nonuniform` is read by nufft_spread[_deferred] and
 * nufft_interpolate, `callbacks.uniform` by nufft_deconvolve_truncate and nufft_deconvolve_pad — the arguments the reference passes
 * to spread_from_points! / interpolate! / copy_deconvolve_to_*! (src/NonuniformFFTs.jl:170,183,270,280).  In force until the next call;
 * NULL (or two NULL pointers) = none.  The pointers are read while a stage enqueues its kernels, not later. */
int nufft_set_callbacks(nufft_plan* plan, const nufft_callbacks* callbacks);

/* fill_with_zeros_kernel!(us), src/NonuniformFFTs.jl:116-122,161-167. */
int nufft_fill_zeros(nufft_plan* plan, void* stream);
/* spread_from_points!(::GPU, ...), src/spreading/gpu.jl:134-214 (adds onto the plan's grids). */
int nufft_spread(nufft_plan* plan, const void* const* values_in, void* stream);
/* The same stage as exec_type1 enqueues it: on plans whose spreading engine is the marching ring's halo variant (nufft_info.ring_halo)
 * the stencil reach beyond each workgroup's column is left in a side buffer.  nufft_fft_forward consumes it on the fly (its
 * dimension-1 pass adds the buffer to the lines it loads — the spectrum is that of the complete grid, `us` itself stays without
 * the reach); nufft_complete_grid, nufft_copy_grid(which = 0) and nufft_interpolate add it to `us` (once), before or after that FFT.
 * The pending state ends with the next nufft_set_points, nufft_spread[_deferred], nufft_fill_zeros or nufft_fft_backward.
 * nufft_spread completes the grid itself with one more pass.  Identical to nufft_spread on every other plan.
 * The state is host-side: a deferred spread and its consumer must be enqueued on the same stream, and captured in the same hipGraph
 * (tests/test_gpu_graph.py), since a replayed spread does not set it again.
 * (No reference counterpart: src/NonuniformFFTs.jl:169-177 calls spread_from_points! and _type1_fft! back to back.) */
int nufft_spread_deferred(nufft_plan* plan, const void* const* values_in, void* stream);
/* _type1_fft!, src/NonuniformFFTs.jl:197-211. */
int nufft_fft_forward(nufft_plan* plan, void* stream);
/* copy_deconvolve_to_non_oversampled!(::GPU, ...), src/NonuniformFFTs.jl:387-414. */
int nufft_deconvolve_truncate(nufft_plan* plan, void* const* uhat_out, void* stream);
/* fill_with_zeros + copy_deconvolve_to_oversampled!(::GPU, ...), src/NonuniformFFTs.jl:260-272,453-480. */
int nufft_deconvolve_pad(nufft_plan* plan, const void* const* uhat_in, void* stream);
/* _type2_fft! / _fft_c2r!, src/NonuniformFFTs.jl:293-314. */
int nufft_fft_backward(nufft_plan* plan, void* stream);
/* interpolate!(::GPU, ...), src/interpolation/gpu.jl:40-118. */
int nufft_interpolate(nufft_plan* plan, void* const* values_out, void* stream);

/* ---- gradients of type 2 (no reference counterpart) ----------------
 * The type-2 interpolant v_c(x) = prod(Δx_d) Σ_l g_l φ(x − x_l) and its derivatives ∂_d v_c(x_j) at the plan's points, from the grids
 * the last backward FFT left: the exact derivative of what nufft_interpolate returns (window derivatives, same grid).
 *   values_out: C device vectors Z[Np], or NULL (gradients only);  grad_out[c * D + d]: C * D device vectors Z[Np] (caller order).
 * The outputs have type Z: the gradient of a real plan is real.  Derivatives are taken with respect to the coordinates the caller
 * passed to nufft_set_points: plans with NUFFT_POINT_TRANSFORM_NFFT (internal point = −2π x, folded) include the factor −2π;
 * fftshift changes nothing.  A mode-factor callback in force applies as in type 2 (it lives in nufft_deconvolve_pad); a point-weight
 * callback in force is refused with NUFFT_ERR_UNSUPPORTED.  A host-only plan gives NUFFT_ERR_NO_DEVICE (checked first), a plan
 * without points NUFFT_ERR_NO_POINTS, a null table or vector NUFFT_ERR_INVALID_ARG; Np = 0 is a no-op.  Like nufft_interpolate the
 * stage completes a deferred spread first, allocates nothing and does not synchronise (hipGraph-capture safe); it is timed into
 * NUFFT_STAGE_T2_INTERP and adds no plan memory.  Added after ABI 104 without changing NUFFT_MI355X_VERSION: a caller detects
 * these two symbols by lookup. */
int nufft_interpolate_grad(nufft_plan* plan, void* const* values_out, void* const* grad_out, void* stream);
/* nufft_deconvolve_pad -> nufft_fft_backward -> nufft_interpolate_grad. */
int nufft_exec_type2_grad(nufft_plan* plan, void* const* values_out, void* const* grad_out, const void* const* uhat_in, void* stream);

/* Adds the side buffer of a deferred spread to `us` if that has not happened yet (no-op otherwise): after it, `us` holds the full
 * spread field as after the reference's spread_from_points! (src/NonuniformFFTs.jl:169-172), also behind nufft_exec_type1. */
int nufft_complete_grid(nufft_plan* plan, void* stream);

/* Device pointer of plan-owned oversampled arrays (p.data.us / p.data.ûs, src/plan.jl:3-29):
 * which = 0 -> us[c] (real T[N_over] or complex), which = 1 -> ûs[c] (real plans only).
 * which = 0 is refused (NUFFT_ERR_INVALID_ARG) while a deferred spread is pending: call nufft_complete_grid first. */
int nufft_grid_ptr(const nufft_plan* plan, int which, int component, void** out_ptr, int64_t* out_bytes);

/* Device-to-device copy of one plan-owned oversampled array (same `which` as nufft_grid_ptr) into
 * a caller buffer of at least `capacity_bytes`; enqueued on `stream`. */
int nufft_copy_grid(nufft_plan* plan, int which, int component, void* dst, int64_t capacity_bytes, void* stream);

/* Sorted-point inspection: copies the bin-sort permutation (sorted position -> original index,
 * 0-based; BlockDataGPU.pointperm, src/blocking/gpu.jl:15) and the per-tile offsets
 * (cumulative_npoints_per_block, :13) to HOST buffers.  Synchronises `stream`. */
int nufft_get_sort_result(nufft_plan* plan, int32_t* perm_host, int64_t perm_capacity,
                          uint32_t* tile_offsets_host, int64_t offsets_capacity, void* stream);

/* Which sort the last nufft_set_points used: 1 = by column layers (nufft_info.sort_column; the offsets returned by
 * nufft_get_sort_result then hold a column layer's points in its first bin and nothing in its other bins), 0 = by fine bins
 * (histogram with global atomics), 2 = by fine bins in two levels (slabs of bin rows with LDS histograms, then every slab in LDS:
 * the same array and offsets as 0 up to the order inside a bin; 3-D plans without sort_column, point sets whose fullest slab fits
 * a workgroup's LDS).  Reads device flags back (synchronises `stream`).  Inspection only. */
int nufft_sort_columns_used(nufft_plan* plan, int* used_out, void* stream);

/* Whether the last nufft_set_points took the steady path (1) or the full one (0).  Plans with nufft_info.sort_column decide on the device, per
 * point set, whether the two rings or the tile kernels serve it, so the full path enqueues both alternatives and one of them returns on a
 * device flag.  The decisions come back to the host through mapped memory, without a synchronisation; once the newest record the host has
 * seen reports three point sets in a row that both rings served from their equal-length task tables, set_points enqueues the rings' path
 * alone — no stand-by of the fine sort, no tile tables, no task-table kernels — and spreading / interpolation launch no tile kernel for that
 * set.  The rings are then FORCED for it (either engine computes the same transform for any point set; nufft_spread_engine_used,
 * nufft_interp_engine_used and nufft_sort_columns_used report the rings and the column-layer sort, which is what ran); what they would have
 * decided still comes back, and the first set they would not have served from those tables sends the next call seen to report it back to
 * the full path.  Never taken while `stream` is capturing, nor on a plan that has had any call captured into a hipGraph; option
 * NUFFT_STEADY_PATH=0 (nufft_params.options) turns it off.  A host flag: no device read, no synchronisation.  Inspection only. */
int nufft_steady_path_used(const nufft_plan* plan, int* used_out);

/* The host bookkeeping behind it, as a function (no plan, no device): state[0] = sequence number of the newest feedback record seen,
 * state[1] = 1 while that record reports the streak; (seq, streak) = a record as the host reads it.  A record whose sequence number is
 * not new is ignored.  Updates `state`: state[1] = 1 means that a set_points seeing it is eligible for the steady path. */
int nufft_steady_path_observe(uint32_t* state, uint32_t seq, uint32_t streak);

/* ---- timing (TimerOutputs analogue, src/plan.jl:397-417) -------------------------------- */

/* enable != 0: bracket every stage with hipEvents on the caller's stream. */
int nufft_set_timing(nufft_plan* plan, int enable);
/* Milliseconds of the most recent run of every stage (NUFFT_NUM_STAGES floats; -1 = never run).
 * Synchronises on the recorded events. */
int nufft_get_stage_times(nufft_plan* plan, float* ms_out);

/* Which engine served the point set of the last nufft_set_points: NUFFT_SPREAD_LDS_TILES, _MFMA_PATCHES or _MARCHING_RING.
 * On plans whose nufft_info.spread_method is MFMA patches or the marching ring, set_points decides per point set on the
 * device (a point set that concentrates in a few patches / columns goes to the LDS tiles, whose heavy tiles are shared by
 * several workgroups);
 * this reads the decision back (4 bytes, synchronises `stream`).  Inspection only: nothing on the hot path needs it. */
int nufft_spread_engine_used(nufft_plan* plan, int* engine_out, void* stream);
/* The same for the interpolation stage of nufft_exec_type2: NUFFT_INTERP_LDS_TILES (padded boxes, heavy tiles shared by
 * several workgroups: interp_tile_kernel) or NUFFT_INTERP_MARCHING_RING (3-D plans with the default window evaluation,
 * point sets whose heaviest ring task and total work stay within the ring's measured advantage over the tile kernel:
 * interp_march_kernel).  Replaces nothing in the reference — its
 * interpolate! (src/interpolation/gpu.jl:3-89) has one shared-memory kernel; inspection only. */
enum { NUFFT_INTERP_LDS_TILES = 1, NUFFT_INTERP_MARCHING_RING = 2 };
int nufft_interp_engine_used(nufft_plan* plan, int* engine_out, void* stream);

/* ---- type 3 (nonuniform to nonuniform) ------------------------------------------------ */
/* f_k = Σ_j c_j exp(sign i s_k · x_j) for sources x_j ∈ R^D and targets s_k ∈ R^D (no reference counterpart: NonuniformFFTs.jl has
 * type 1 and 2 only).  The scheme of Barnett, Magland & af Klinteberg (SISC 2019, section 3.3): the sources, rescaled and prephased,
 * are spread onto a grid of nf cells per axis by an internal plan of this library, a type-2 transform of an internal complex plan
 * (N = nf, same σ, M, kernel) reads that grid as its spectrum at the rescaled targets, and a per-target factor corrects the window and
 * the phase of the centres.  Added after ABI 104 without changing NUFFT_MI355X_VERSION: a caller detects these
 * entry points by symbol (dlsym nufft_plan3_create) and compares nufft_sizeof_type3_params() / nufft_sizeof_info3() with its own.
 *
 * The declared boxes: sources in source_center ± source_halfwidth, targets in target_center ± target_halfwidth (per dimension; only the
 * first ndim entries are read).  They set the fine grid; results for points outside them are UNDEFINED (the spread of such a source can
 * wrap around the grid; such a target can fall beyond the window's band) and nufft_type3_points_outside counts them. */
typedef struct nufft_type3_params {
    int32_t struct_size;     /* sizeof(nufft_type3_params) of the caller's header (as nufft_params.struct_size); 0 = this layout   */
    int32_t sign;            /* -1 (0 -> -1, the sign of the reference's type 1) or +1                                             */
    double  source_center[3], source_halfwidth[3];
    double  target_center[3], target_halfwidth[3];
} nufft_type3_params;

typedef struct nufft_plan3 nufft_plan3; /* opaque */

typedef struct nufft_info3 {
    int32_t ndim, ntransforms, dtype, half_support, sign, kernel, evalmode, device;
    int64_t nf[3];           /* fine grid: smallest multiple of 4 that is 2,3,5-smooth and >= 2σ X S / π + 2M + 2 (X, S the half-widths) */
    double  gamma[3];        /* γ = nf / (2σ S): sources are spread at (x - C) / γ                                                     */
    double  h[3];            /* 2π / nf                                                                                                */
    double  source_halfwidth[3], target_halfwidth[3];  /* X, S the rule used (a zero half-width replaced: X = 1/S, S = 1/X, or 1 and 1) */
    int64_t inner_N_over[3]; /* oversampled grid of the internal type-2 plan (nextprod235(σ nf))                                        */
    double  sigma;           /* requested σ                                                                                           */
    double  beta[3];         /* window shape parameter of both internal plans (optimal for the requested σ and M)                     */
    int32_t spread_method;   /* nufft_info.spread_method of the internal spreading plan                                               */
    int32_t reserved;
    int64_t num_sources, num_targets;   /* of the last nufft_set_points3 (-1: none yet)                                                */
    int64_t workspace_bytes; /* device bytes owned right now: both internal plans plus the type-3 buffers                              */
} nufft_info3;

/* From `params`: dtype, is_complex (must be 1), ndim 1..3, half_support, sigma, kernel, kernel_param, evalmode, ntransforms, device,
 * options; N, N_over, fftshift and point_transform must be zero (NUFFT_ERR_INVALID_ARG).  A negative or non-finite half-width is
 * NUFFT_ERR_INVALID_ARG; an nf beyond 2^30 or a pair of grids beyond the device's memory NUFFT_ERR_UNSUPPORTED.  device = -1: a host-only
 * plan (parameter rule and info only). */
int nufft_plan3_create(nufft_plan3** out, const nufft_params* params, const nufft_type3_params* t3);
int nufft_plan3_destroy(nufft_plan3* plan);
int nufft_plan3_info(const nufft_plan3* plan, nufft_info3* out);
/* x[d]: device vectors of num_sources reals, s[d]: of num_targets reals (plan precision).  Rescales and prephases the sources, computes
 * the targets' coordinates and correction factors (in Float64 from the caller's values, stored in the plan's precision), counts points
 * outside the boxes, and sets the points of both internal plans.  Buffers grow when a size exceeds what the plan holds (never on a
 * capturing stream: pre-size the plan with the largest point sets before capturing into a hipGraph); the caller's arrays are only read. */
int nufft_set_points3(nufft_plan3* plan, int64_t num_sources, const void* const* x, int64_t num_targets, const void* const* s,
                      void* stream);
/* f_out[c]: device vector complex(T)[num_targets]; c_in[c]: device vector complex(T)[num_sources], c < ntransforms. */
int nufft_exec_type3(nufft_plan3* plan, void* const* f_out, const void* const* c_in, void* stream);
/* ---- gradient of type 3 with respect to the targets ----
 * f_out[c]: complex(T)[num_targets], required (the derivative needs the values);
 * grad_out[c * D + d]: complex(T)[num_targets] = ∂f_c/∂s_d with respect to the caller's target coordinates.
 * Premultiply and spread as nufft_exec_type3, the inner plan's nufft_exec_type2_grad straight into f_out / grad_out, then one kernel in
 * place: ∂f/∂s_d = P(s) [sign γ_d h_d ∂v/∂θ_d + (sign i C_d − ρ_d(t_d)) v(θ)], P the per-target factor, ρ_d = γ_d (d ln ϕ̂_d/dk)(γ_d t_d).
 * t = s − D is recovered from the stored θ (no new per-target table): exact for targets inside the box, except that at σ = 1 a target at
 * exactly |t_d| = S_d is ambiguous (t = +S reads back as −S).  Refusals as nufft_exec_type3, all before anything is enqueued: a host-only
 * plan NUFFT_ERR_NO_DEVICE, no points NUFFT_ERR_NO_POINTS, a null table or vector NUFFT_ERR_INVALID_ARG.  num_targets = 0 is a no-op;
 * num_sources = 0 writes zeros to the values and the gradients.  Allocates nothing, does not synchronise (hipGraph-capture safe); timed
 * into NUFFT3_STAGE_TYPE2 (the inner gradient) and NUFFT3_STAGE_POSTMULTIPLY (the finish).  Added after ABI 104 without changing
 * NUFFT_MI355X_VERSION: detect it by symbol.
 * Gradients with respect to the sources need no entry point of their own.  For L = Re Σ_k conj(G_k) f_k, let u(x) = Σ_k G_k
 * exp(−sign i s_k·x): then ∂L/∂c_j (conjugate-Wirtinger) = u(x_j) and ∂L/∂x_{j,d} = Re(c_j conj(∂_d u(x_j))).  u is the type 3 of the
 * adjoint plan — sign −sign, the two boxes swapped, sources s_k with values G_k, targets x_j — and one nufft_exec_type3_grad on that plan
 * returns u and ∂_d u together. */
int nufft_exec_type3_grad(nufft_plan3* plan, void* const* f_out, void* const* grad_out, const void* const* c_in, void* stream);
/* Sources / targets of the last nufft_set_points3 outside the declared boxes (|x_d - C_d| > X_d in some dimension, with the caller's
 * half-widths).  Synchronises `stream`. */
int nufft_type3_points_outside(nufft_plan3* plan, int64_t* sources_out, int64_t* targets_out, void* stream);
/* The internal plans, for inspection (nufft_plan_info, nufft_spread_engine_used, nufft_interp_engine_used, nufft_set_timing /
 * nufft_get_stage_times): which = 0 the spreading plan (N_over = nf), 1 the type-2 plan (N = nf).  Owned by the type-3 plan: do not
 * destroy them or set their points. */
int nufft_plan3_internal(const nufft_plan3* plan, int which, nufft_plan** out);
/* enable != 0: bracket the four type-3 kernels and the two internal stages with hipEvents; nufft_get_stage_times3 returns
 * NUFFT3_NUM_STAGES milliseconds of their latest runs (-1 = never run) and synchronises on the events. */
enum {
    NUFFT3_STAGE_PREP_SOURCES = 0, NUFFT3_STAGE_PREP_TARGETS = 1, NUFFT3_STAGE_PREMULTIPLY = 2, NUFFT3_STAGE_SPREAD = 3,
    NUFFT3_STAGE_TYPE2 = 4, NUFFT3_STAGE_POSTMULTIPLY = 5, NUFFT3_NUM_STAGES = 6
};
int nufft_set_timing3(nufft_plan3* plan, int enable);
int nufft_get_stage_times3(nufft_plan3* plan, float* ms_out);
int64_t nufft_sizeof_type3_params(void);
int64_t nufft_sizeof_info3(void);

/* ---- Toeplitz normal operator ----------------------------------- */
/* G û = exec_type1(w ⊙ exec_type2(û)) for real weights w_j at the points — the Gram operator A^H W A that CG / LSQR on the normal
 * equations applies once per iteration — without touching the points: G[k, k'] = T[k − k'] with T_d = Σ_j w_j exp(−i d·x_j), so G is
 * applied by FFTs of size 2 N_d at a cost that does not depend on the number of points (NFFT.jl: calculateToeplitzKernel /
 * convolveToeplitzKernel!).  The object holds the real multiplier K = backwardDFT_{2N}(T) / Π 2N_d (T with its Nyquist planes zeroed:
 * differences of the plan's modes never reach them) and applies  û -> crop(forwardDFT(K ⊙ backwardDFT(pad(û)))).
 *
 * Complex plans only (is_complex = 1): the type 2 of a real-data plan extends its half spectrum Hermitian-ly, which for even N_d adds
 * the mode +N_d/2 next to −N_d/2; mode differences then reach ±N_d, the 2N embedding aliases and the identity fails (rel-L2 0.04 – 0.25
 * measured on small grids; exact only when every N_d is odd).  A real plan is refused with NUFFT_ERR_UNSUPPORTED.  The weights are real
 * (K would not be real otherwise).
 *
 * Two apply paths, chosen at creation (nufft_toeplitz_info.path, from nufft_toeplitz_get_info):
 *   fused — D = 2, 3 and every 2 N_d among the line lengths of the pruned FFT passes (N_d ∈ {32, 40, 48, 64, 80, 96, 128, 160, 192, 256,
 *           320, 384, 512}): pruned strided passes along dimensions 3 and 2 straight from / into the caller's arrays and one kernel along
 *           dimension 1 that transforms, multiplies by K and transforms back inside LDS (2 D − 1 launches per component); the (2N)^D
 *           complex grid never exists.  Workspace: K and two intermediates, complex[N_1, N_2, 2N_3] and complex[N_1, 2N_2, 2N_3].
 *   dense — everything else: pad kernel, rocFFT backward of size 2N, multiply kernel, rocFFT forward, crop kernel, on a (2N)^D complex
 *           work grid.  The option NUFFT_TOEPLITZ_FUSED=0 in the plan's options string forces this path.
 * Added after ABI 104 without changing NUFFT_MI355X_VERSION: detect by symbol (dlsym nufft_toeplitz_create) and compare
 * nufft_sizeof_toeplitz_info() with your own. */
typedef struct nufft_toeplitz nufft_toeplitz; /* opaque */

enum { NUFFT_TOEPLITZ_PATH_DENSE = 0, NUFFT_TOEPLITZ_PATH_FUSED = 1 };

typedef struct nufft_toeplitz_info {
    int32_t struct_size;     /* sizeof(nufft_toeplitz_info) of the CALLER's header, set before the call: the library writes only that many
                                bytes (0 = this layout)                                                                            */
    int32_t ndim, dtype, ntransforms, fftshift, device;
    int32_t path;            /* NUFFT_TOEPLITZ_PATH_*                                                                              */
    int32_t has_spectrum;    /* 1 once nufft_toeplitz_set_spectrum / _set_points has completed                                     */
    int64_t N[3];            /* the plan's modes per dimension                                                                     */
    int64_t N2[3];           /* the embedding grid, 2 N_d (1 beyond ndim)                                                          */
    int64_t multiplier_bytes;/* bytes of K: real(T)[2N_1, 2N_2, 2N_3]                                                              */
    int64_t workspace_bytes; /* device bytes owned right now (a host-only object: what a device object of these parameters holds at
                                rest): K, the intermediates or the work grid, tables, rocFFT work; while nufft_toeplitz_set_points
                                runs, plus the internal 2N plan                                                                   */
} nufft_toeplitz_info;

/* Geometry (dtype, ndim, N, ntransforms, fftshift, index maps, window parameters, device, options) is copied from `plan`; no pointer to it
 * is kept, so the plan may be destroyed first.  Allocates K and the intermediates (fused) or the work grid (dense).  A host-only plan
 * (device = -1) gives a host-only object that answers nufft_toeplitz_get_info only. */
int nufft_toeplitz_create(nufft_toeplitz** out, const nufft_plan* plan);
int nufft_toeplitz_destroy(nufft_toeplitz* tz);
int nufft_toeplitz_get_info(const nufft_toeplitz* tz, nufft_toeplitz_info* out);
/* T_modes: device array complex(T)[2N_1, 2N_2, 2N_3] in FFT order — what nufft_exec_type1 of a plan with 2 N_d modes, the same Z and
 * fftshift = 0 returns for the weights.  Zeroes the Nyquist planes, transforms (rocFFT, once per point set), keeps the scaled real part
 * as K.  The fused path needs a temporary (2N)^D complex grid for this, allocated and freed inside the call: the call synchronises the
 * stream and is refused on a capturing stream (NUFFT_ERR_INVALID_ARG). */
int nufft_toeplitz_set_spectrum(nufft_toeplitz* tz, const void* T_modes, void* stream);
/* The convenience path: builds an internal plan with 2 N_d modes (window parameters of the parent plan unless `build_params` — may be
 * NULL — gives half_support / sigma / kernel / kernel_param / evalmode; always ntransforms = 1, fftshift = 0), sets its points,
 * runs nufft_exec_type1 of the weights (real(T)[num_points] on the device; NULL = ones), then nufft_toeplitz_set_spectrum, then
 * DESTROYS the internal plan.  That plan is large while it lives: at N = 256³, σ = 2 its oversampled grid is 1024³ complex, 17 GB in
 * ComplexF64 (reported in workspace_bytes during the call).  Never on a capturing stream. */
int nufft_toeplitz_set_points(nufft_toeplitz* tz, const nufft_params* build_params, int64_t num_points, const void* const* coords,
                              const void* weights, void* stream);
/* out[c] = G in[c], c < ntransforms: device arrays complex(T)[N_out...] in the plan's mode order (fftshift plans work unchanged);
 * out[c] may equal in[c] (not while coil maps are set, see below).  Allocates nothing, does not synchronise, is hipGraph-capture safe.  Refusals, all before anything is
 * enqueued: a host-only object NUFFT_ERR_NO_DEVICE, no spectrum yet NUFFT_ERR_NO_POINTS, a null table or vector NUFFT_ERR_INVALID_ARG. */
int nufft_toeplitz_apply(nufft_toeplitz* tz, void* const* out, const void* const* in, void* stream);
/* Device pointer and bytes of K (inspection and tests). */
int nufft_toeplitz_multiplier_ptr(const nufft_toeplitz* tz, void** out_ptr, int64_t* out_bytes);
int64_t nufft_sizeof_toeplitz_info(void);

/* ---- Coil sensitivity maps in the Toeplitz normal operator: SENSE --- */
/* A multi-coil acquisition solves with  G_S û = Σ_c conj(S_c) ⊙ G (S_c ⊙ û),  c < ncoils,  S_c complex maps on the uniform side.
 * Added after the Toeplitz section under the same rule: detect by symbol (dlsym nufft_toeplitz_set_maps); NUFFT_MI355X_VERSION and
 * nufft_toeplitz_info are unchanged.
 *
 * maps[c]: device arrays complex(T)[N...] laid out like the arrays of nufft_toeplitz_apply, 16-byte aligned.  The operator BORROWS
 * them: the host table is copied, the device data is not (32 coils at 256³ are 8.6 GB).  They must stay valid, and hold their values,
 * until the next nufft_toeplitz_set_maps, nufft_toeplitz_clear_maps or nufft_toeplitz_destroy.  The same maps serve every component
 * of an ntransforms operator.  Independent of nufft_toeplitz_set_spectrum / _set_points: any order, either redone without the other.
 * Refusals: a null table or ncoils outside 1 ... 1024 NUFFT_ERR_INVALID_ARG; then a host-only object NUFFT_ERR_NO_DEVICE; then a null
 * or not 16-byte aligned entry NUFFT_ERR_INVALID_ARG.
 *
 * With maps set nufft_toeplitz_apply computes G_S per component: the coils run in index order on the caller's stream, coil 0 writes
 * out[c], coils >= 1 read it and add — no atomics, so two runs and a graph replay give the same bits; it still allocates nothing
 * and does not synchronise.  out[c] == in[c'] for any c, c' is then refused (NUFFT_ERR_INVALID_ARG): coil 0's store would destroy
 * the input of coil 1.  Without maps nothing changes, in place included.
 *
 * Routes: on the fused path S_c multiplies where the first pruned pass loads the caller's array and conj(S_c) where the last one
 * stores into it (no extra pass); on the dense path the pad and crop kernels do the same.  The option
 * NUFFT_TOEPLITZ_MAPS_INPASS=0 of the plan's options string (read at nufft_toeplitz_create) makes the fused path run
 * nufft_coil_expand into one N^D scratch array, the plain in-place apply on it, and a combine that adds into out[c]; the scratch
 * array is allocated by nufft_toeplitz_set_maps (never on a capturing stream in this mode), counted in workspace_bytes and freed by
 * nufft_toeplitz_clear_maps.  `stream` is otherwise unused: the call enqueues nothing. */
int nufft_toeplitz_set_maps(nufft_toeplitz* tz, int32_t ncoils, const void* const* maps, void* stream);
/* Back to the plain operator G; idempotent. */
int nufft_toeplitz_clear_maps(nufft_toeplitz* tz);
/* 0 without maps. */
int32_t nufft_toeplitz_num_coils(const nufft_toeplitz* tz);
/* The forward model's and the right-hand side's coil passes, on `n` complex(T) elements (dtype: NUFFT_F32 / NUFFT_F64 = the real type;
 * n >= 0, an odd count of ComplexF32 elements included); every pointer 16-byte aligned; ncoils in 1 ... 1024; tables on the host.
 *   expand:   out[c] = S_c ⊙ in
 *   combine:  out = Σ_c conj(S_c) ⊙ in[c], summed in coil order in registers: one pass reads every array once and no partial result
 *             goes through memory (up to 64 coils; beyond, the running sum passes through `out` once per 64 coils, same order).
 * Both allocate nothing and do not synchronise. */
int nufft_coil_expand(int dtype, int64_t n, int32_t ncoils, void* const* out, const void* const* maps, const void* in, int device, void* stream);
int nufft_coil_combine(int dtype, int64_t n, int32_t ncoils, void* out, const void* const* maps, const void* const* in, int device, void* stream);

/* ---- Coupled components in the Toeplitz normal operator: subspace models --- */
/* A subspace / low-rank model mixes the K = ntransforms components at the samples,  y_j = Σ_a φ_a(j) (A û_a)_j,  φ ∈ C^{K × Np}  (a
 * temporal basis, or the temporal interpolators of time-segmented off-resonance correction).  Its normal operator is a K × K block
 * operator whose blocks are Toeplitz:
 *     (G_Φ û)_a = Σ_b A^H diag(w ⊙ conj(φ_a) ⊙ φ_b) A û_b = Σ_b Toeplitz(T_ab) û_b,     T_ab = Σ_j w_j conj(φ_a(j)) φ_b(j) exp(−i d·x_j).
 * With the Nyquist planes of every T_ab zeroed, K_ab = backwardDFT_{2N}(T_ab) / Π 2N_d satisfies K_ba = conj(K_ab) and K_aa is real:
 * the object holds K real grids (the diagonal) and K (K − 1) / 2 complex grids (the pairs a < b), each real(T) / complex(T)[2N_1, 2N_2,
 * 2N_3], and applies K_ab for a < b and its conjugate for a > b.  Pair order everywhere is row-major over a <= b:
 * idx(a, b) = a K − a (a − 1) / 2 + (b − a).  1 <= K <= 16 (more: NUFFT_ERR_UNSUPPORTED).
 * Added after the SENSE section under the same rule: detect by symbol (dlsym nufft_toeplitz_set_points_coupled);
 * NUFFT_MI355X_VERSION and nufft_toeplitz_info are unchanged.
 *
 * The first coupled build allocates the multipliers (K² real grids' worth) and K intermediates — fused: complex[N_1, 2N_2, 2N_3] each,
 * dense: complex[(2N)^D] each — all counted in workspace_bytes; they are kept across coupled builds and freed by the next
 * nufft_toeplitz_set_points / _set_spectrum, which return the operator to independent components, bit for bit, or by
 * nufft_toeplitz_destroy.  No coupled build runs on a capturing stream (NUFFT_ERR_INVALID_ARG).
 *
 * While a coupled build is in force nufft_toeplitz_apply computes out[a] = Σ_b Toeplitz(T_ab) in[b]: per component the strided passes
 * of the fused path (or pad + rocFFT of the dense path) into its own intermediate, ONE kernel that applies the K × K block to every
 * cell (fused: inside the dimension-1 kernel, where a wave holds the K lines of a line id in LDS between their backward and forward
 * transforms; dense: a streaming kernel over the K grids), and the passes back.  Every output depends on every input: out[a] == in[b]
 * for any a, b is refused (NUFFT_ERR_INVALID_ARG), with or without coil maps.  With coil maps G_{S,Φ} û = Σ_c conj(S_c) ⊙ G_Φ (S_c ⊙ û),
 * the same maps for every component, coils in index order, coil 0 stores and coils >= 1 add — no atomics: two runs and a graph replay
 * give the same bits.  The apply still allocates nothing and does not synchronise.
 *
 * Fused path: the K lines of 2 N_1 cells (plus 1/16 padding) and the twiddle table must fit the 160 KiB of LDS of one wave's workgroup —
 * K <= 8 at 2 N_1 <= 512 always does; otherwise the coupled build returns NUFFT_ERR_UNSUPPORTED and names the option
 * NUFFT_TOEPLITZ_FUSED=0 (the path is decided at creation and never switched silently).  On the route NUFFT_TOEPLITZ_MAPS_INPASS=0
 * nufft_toeplitz_set_maps on a coupled operator, and a coupled build while maps are set, return NUFFT_ERR_UNSUPPORTED.
 *
 * nufft_cg_solve on an operator with a coupled build in force treats the K components as ONE system: Re<p, q>, |p|², |r|² and |b|² are
 * summed over all components (the per-workgroup partial sums are contiguous over components and reduced in one fixed order, so runs
 * and graph replays still agree bit for bit), with one α, one β, one done flag and one breakdown test; nufft_cg_get_result and
 * nufft_cg_history report the same iterations, status and residual for every component.  Uncoupled operators keep their
 * per-component scalars.
 *
 * Refusals of the two builds, in order: a null object or table NUFFT_ERR_INVALID_ARG; a host-only object NUFFT_ERR_NO_DEVICE; a null
 * (or, basis: not 16-byte aligned) entry NUFFT_ERR_INVALID_ARG; the limits above NUFFT_ERR_UNSUPPORTED; a capturing stream. */
/* basis: host table of K device pointers complex(T)[num_points], 16-byte aligned, only read during the call.  The internal 2N plan is
 * created once, its points are set once, and it runs one type 1 per pair a <= b of the weights w_j conj(φ_a(j)) φ_b(j); each result
 * becomes a multiplier (real part for a = b, complex for a < b) before the next pair runs.  Peak memory: the internal plan, one (2N)^D
 * complex grid and rocFFT's work buffer on top of what the operator holds.  Other arguments as nufft_toeplitz_set_points. */
int nufft_toeplitz_set_points_coupled(nufft_toeplitz* tz, const nufft_params* build_params, int64_t num_points, const void* const* coords,
                                      const void* weights, const void* const* basis, void* stream);
/* T_pairs: host table of K (K + 1) / 2 device pointers, T_ab on the 2N mode set as for nufft_toeplitz_set_spectrum, in pair order.  Any
 * Hermitian family (T_ba(d) = conj(T_ab(−d))) is admitted, not only the rank-one form that _set_points_coupled builds. */
int nufft_toeplitz_set_spectra_coupled(nufft_toeplitz* tz, const void* const* T_pairs, void* stream);
/* K while a coupled build is in force, else 0. */
int32_t nufft_toeplitz_num_coupled(const nufft_toeplitz* tz);
/* Device pointer and bytes of K_ab, 0 <= a <= b < K (inspection and tests): real(T) for a = b, complex(T) for a < b. */
int nufft_toeplitz_multiplier_pair_ptr(const nufft_toeplitz* tz, int32_t a, int32_t b, void** out_ptr, int64_t* out_bytes);

/* ---- Conjugate gradients on the Toeplitz normal operator --------- */
/* Solves (G + λ I) x_c = b_c for every component c < ntransforms independently (G is block-diagonal over components: each has its
 * own scalars), G = what a nufft_toeplitz object applies, λ >= 0 real.  With b = nufft_exec_type1(w ⊙ y) this is the weighted,
 * Tikhonov-regularised least-squares inverse of nufft_exec_type2.  Everything runs on the device; no scalar visits the host.
 *
 *     r = b − (G + λ) x0  (no x0: x = 0, r = b, no apply)     p = r     ρ = ‖r‖²     β0 = ‖b‖²
 *     for it = 1 ... max_iter:
 *         done ← done or (ρ <= rtol² β0)                                  per component, sticky
 *         q = G p                                                         nufft_toeplitz_apply
 *         γ = Re<p, q> + λ ‖p‖²                                           cg_dot_kernel
 *         α = ρ / γ;  x += α p;  r −= α (q + λ p);  ρ' = ‖r‖²             cg_update_kernel
 *         p = r + (ρ'/ρ) p;  ρ = ρ'                                       cg_direction_kernel
 *         history[it][c] = sqrt(ρ / β0)
 *
 * A component that is done is FROZEN: the three kernels leave its x, r, p, scalars and iteration count bit-for-bit untouched.  b = 0
 * gives x = 0 and done at once.  A γ that is not positive and finite (G is only positive semi-definite) sets done with the status
 * NUFFT_CG_BREAKDOWN instead of dividing.  Sums and scalars are FP64 also for ComplexF32 operators; the arrays keep the operator's
 * precision.  Sums are formed in one fixed order without atomics: two runs, and a replayed hipGraph, give the same bits.
 *
 * check_every = 0: all max_iter iterations are enqueued without synchronising or allocating (hipGraph-capture safe; frozen components
 *                  cost their share of the apply only).
 * check_every = k > 0: after every k iterations the host reads the done flags (one small copy and a stream synchronise) and stops
 *                  enqueuing once every component is done.  Refused on a capturing stream.  Because frozen components do not change,
 *                  both modes return bit-identical x, iteration counts and history.
 *
 * Added after ABI 104 without changing NUFFT_MI355X_VERSION: detect by symbol (dlsym nufft_cg_create) and compare
 * nufft_sizeof_cg_params() / nufft_sizeof_cg_info() with your own. */
typedef struct nufft_cg nufft_cg; /* opaque */

enum { NUFFT_CG_MAX_ITER = 0,   /* max_iter iterations ran without reaching rtol */
       NUFFT_CG_CONVERGED = 1,  /* ‖r‖ <= rtol ‖b‖ (recursive residual)         */
       NUFFT_CG_BREAKDOWN = 2   /* γ <= 0 or not finite: stopped before dividing */ };

typedef struct nufft_cg_params {
    int32_t struct_size;     /* sizeof(nufft_cg_params) of the caller's header (0 = this layout)                                   */
    int32_t max_iter;        /* 1 ... 2^24                                                                                         */
    int32_t check_every;     /* 0, or the number of iterations between two looks at the done flags                                 */
    int32_t reserved;        /* 0                                                                                                  */
    double rtol;             /* >= 0, finite; 0 = run max_iter iterations unless ρ reaches 0 exactly                               */
    double lambda;           /* >= 0, finite                                                                                       */
} nufft_cg_params;

typedef struct nufft_cg_info {
    int32_t struct_size;     /* sizeof(nufft_cg_info) of the caller's header, set before the call (0 = this layout)                */
    int32_t ntransforms, dtype, max_iter, check_every;
    int32_t workgroups;      /* per component and kernel = length of a row of partial sums                                         */
    int32_t iterations_enqueued; /* by the last nufft_cg_solve (check_every > 0 stops early); -1 before the first                  */
    int32_t reserved;
    double rtol, lambda;
    int64_t array_bytes;     /* r, p, q: 3 arrays per component                                                                    */
    int64_t workspace_bytes; /* device bytes owned: array_bytes + partial sums + scalars + history                                 */
} nufft_cg_info;

/* Allocates r, p, q (3 arrays per component), the partial sums, scalars and history on the operator's device, and a few pinned host
 * words.  The solver keeps the POINTER `tz`: the operator must outlive it; nufft_toeplitz_set_points / _set_spectrum on it between two
 * solves is allowed and simply changes G.  Refusals: a host-only operator NUFFT_ERR_NO_DEVICE; null arguments, max_iter < 1 or
 * > 2^24, check_every < 0, rtol < 0, lambda < 0 or non-finite values NUFFT_ERR_INVALID_ARG. */
int nufft_cg_create(nufft_cg** out, nufft_toeplitz* tz, const nufft_cg_params* params);
int nufft_cg_destroy(nufft_cg* cg);
/* x_inout[c], b[c]: device arrays complex(T)[N...] like those of nufft_toeplitz_apply, 16-byte aligned; b is only read.  use_x0 = 0:
 * x is overwritten (start from zero); use_x0 != 0: x holds the starting guess (one extra apply).  Allocates nothing.  Refusals, all
 * before anything is enqueued: operator without spectrum NUFFT_ERR_NO_POINTS; a null table or vector, a pointer that is not 16-byte
 * aligned, x[c] overlapping any b[c'], two x overlapping, check_every > 0 on a capturing stream NUFFT_ERR_INVALID_ARG. */
int nufft_cg_solve(nufft_cg* cg, void* const* x_inout, const void* const* b, int use_x0, void* stream);
/* Static facts and sizes; does not synchronise. */
int nufft_cg_get_info(const nufft_cg* cg, nufft_cg_info* out);
/* Per-component outcome of the last solve: iterations that changed the component, NUFFT_CG_* status, sqrt(ρ / β0) (∞ if b = 0 but
 * r != 0).  Each output may be NULL; `capacity` entries each, at least ntransforms.  Synchronises `stream` (never a capturing one). */
int nufft_cg_get_result(nufft_cg* cg, int32_t* iterations, int32_t* status, double* residual, int64_t capacity, void* stream);
/* host_out[(max_iter + 1) * ntransforms], row it = sqrt(ρ / β0) of every component after iteration it (row 0: the start); NaN where
 * the component was not changed by that iteration (frozen, or beyond the last iteration run).  Synchronises `stream`. */
int nufft_cg_history(nufft_cg* cg, double* host_out, int64_t capacity, void* stream);
int64_t nufft_sizeof_cg_params(void);
int64_t nufft_sizeof_cg_info(void);

/* ---- Preconditioner: T. Chan's optimal circulant for the Toeplitz normal operator ---- */
/* G is multi-level Toeplitz over the array indices of a component (for fftshift = 0 after a cyclic rotation of rows and columns,
 * which leaves a circulant unchanged: the same object serves both layouts).  C = argmin over circulants of ‖C − G‖_F has the
 * eigenvalues e = Re diag(F G F^H) / n, F the unnormalised N-point DFT over the array indices, n = Π N_d; they follow from the
 * operator's multiplier alone (Fejér-weighted fold of its generating sequence and one N-point transform).  The object applies
 *
 *     M⁻¹ r = d ⊙ F⁻¹( m ⊙ F( d ⊙ r ) ),      m_q = 1 / max(e_q + μ, floor · max_q(e_q + μ))
 *
 * to every component: Hermitian and positive definite.  d is an optional real positive array shaped like a component (none: the two
 * multiplies are skipped).  If the operator has coil maps set when the preconditioner is created or updated, d = (Σ_c |S_c|²)^(−1/2)
 * (the sum floored at 1e-3 of its maximum) is computed into an array the object owns and μ = λ / mean(Σ_c |S_c|²); otherwise μ = λ.
 * nufft_precond_set_scaling replaces d by a caller's array (borrowed; NULL: none) and leaves μ as it is.
 *
 * Two paths, chosen at creation from the shape alone and independent of the operator's own path: FUSED (2-D and 3-D, every N_d one
 * of the line lengths 64 ... 1024 of the library's own FFT passes, unless the plan carries NUFFT_TOEPLITZ_FUSED=0): strided line
 * passes and one in-LDS kernel along dimension 1; DENSE: rocFFT forward, one multiply, rocFFT backward on one scratch array.
 *
 * Added after ABI 104 without changing NUFFT_MI355X_VERSION: detect by symbol (dlsym nufft_precond_create) and compare
 * nufft_sizeof_precond_params() / nufft_sizeof_precond_info() with your own. */
typedef struct nufft_precond nufft_precond; /* opaque */

enum { NUFFT_PRECOND_PATH_DENSE = 0, NUFFT_PRECOND_PATH_FUSED = 1 };
enum { NUFFT_PRECOND_SCALING_NONE = 0, NUFFT_PRECOND_SCALING_MAPS = 1, NUFFT_PRECOND_SCALING_CALLER = 2 };

typedef struct nufft_precond_params {
    int32_t struct_size;     /* sizeof(nufft_precond_params) of the caller's header (0 = this layout)                              */
    int32_t reserved;        /* 0                                                                                                  */
    double lambda;           /* the λ of the system (G + λ I) that is preconditioned: >= 0, finite                                 */
    double floor;            /* > 0, finite; 0 is NOT a default here: pass 1e-6                                                    */
} nufft_precond_params;

typedef struct nufft_precond_info {
    int32_t struct_size;     /* sizeof(nufft_precond_info) of the caller's header, set before the call (0 = this layout)           */
    int32_t ndim, dtype, ntransforms, device;
    int32_t path;            /* NUFFT_PRECOND_PATH_*                                                                               */
    int32_t scaling;         /* NUFFT_PRECOND_SCALING_*                                                                            */
    int32_t reserved;
    int64_t N[3];
    double lambda, mu, floor;
    double max_e, min_e;     /* of the eigenvalues e of the last build (before μ and the floor); block object: of the E_aa(q)      */
    int64_t multiplier_bytes;/* m: one real per mode                                                                               */
    int64_t workspace_bytes; /* device bytes owned at rest                                                                         */
} nufft_precond_info;

/* Builds m from the operator's current multiplier on the default stream: allocates temporaries (a complex (2N)^D grid and rocFFT's work
 * buffers), synchronises and frees them before returning — like nufft_toeplitz_set_spectrum the build is not capturable
 * (nufft_precond_update, which takes a stream, refuses a capturing one).  The object keeps the POINTER `tz`: the operator must outlive it.  Refusals, in order: null arguments, lambda < 0, floor <= 0
 * or non-finite values NUFFT_ERR_INVALID_ARG; a host-only operator NUFFT_ERR_NO_DEVICE; no spectrum yet NUFFT_ERR_NO_POINTS; a coupled
 * build in force NUFFT_ERR_UNSUPPORTED (this entry point builds the scalar object: nufft_precond_create_block builds the block one); an
 * operator whose e + μ is nowhere positive NUFFT_ERR_INVALID_ARG. */
int nufft_precond_create(nufft_precond** out, nufft_toeplitz* tz, const nufft_precond_params* params);
int nufft_precond_destroy(nufft_precond* pc);
/* Rebuilds m (and the scaling from coil maps) after the operator's spectrum or maps changed; same rules as the build in _create.  A scalar
 * object whose operator has become coupled, and a block object whose operator is no longer coupled with the same K, are refused
 * (NUFFT_ERR_UNSUPPORTED). */
int nufft_precond_update(nufft_precond* pc, void* stream);
/* d: real(T)[N...] on the device, 16-byte aligned, positive, borrowed until replaced; NULL: no scaling. */
int nufft_precond_set_scaling(nufft_precond* pc, const void* d);
/* out[c] = M⁻¹ in[c] for every component; complex(T)[N...], 16-byte aligned; out[c] may be in[c].  Allocates nothing, does not
 * synchronise, hipGraph-capture safe. */
int nufft_precond_apply(nufft_precond* pc, void* const* out, const void* const* in, void* stream);
int nufft_precond_get_info(const nufft_precond* pc, nufft_precond_info* out);
/* Device pointers (inspection and tests): m, real(T)[N...] with 1 / Π N_d folded in (a block object has no m: NUFFT_ERR_UNSUPPORTED, see
 * nufft_precond_block_ptr); the scaling d in force (NULL: none). */
int nufft_precond_multiplier_ptr(const nufft_precond* pc, void** out_ptr, int64_t* out_bytes);
int nufft_precond_scaling_ptr(const nufft_precond* pc, void** out_ptr, int64_t* out_bytes);
int64_t nufft_sizeof_precond_params(void);
int64_t nufft_sizeof_precond_info(void);

/* Block-circulant preconditioner of a COUPLED operator (nufft_toeplitz_set_points_coupled / _set_spectra_coupled).
 * G_Φ has the blocks Toeplitz(T_ab); the block circulant closest to it in the Frobenius norm replaces every block by its own optimal
 * circulant, so E_ab = DFT_N(fold(T_ab)) per stored pair a <= b, with T_ab = forwardDFT_2N(K_ab) from the operator's own multiplier
 * grids (no pass over the points): complex for a < b, E_aa real, E_ba = conj(E_ab) cell by cell.  For every mode q, E(q) is a K × K
 * Hermitian positive semi-definite matrix.  The object applies, the K components being ONE vector,
 *
 *     (M⁻¹ r)_a = d ⊙ F⁻¹( Σ_b B_ab ⊙ F(d ⊙ r_b) ),      B(q) = (E(q) + shift · I)⁻¹ / n,
 *     shift = max(μ, floor · s),      s = max_{q,a} E_aa(q) + μ,
 *
 * with μ and d exactly as in the scalar object.  The floor is a SHIFT here, not a clamp: a clamp needs the eigen-decomposition of every
 * cell, whereas the shift moves every eigenvalue of E(q) + μ I up by at most floor · s (by nothing while μ >= floor · s) and keeps B(q)
 * Hermitian positive definite.  B(q) is formed per cell by a Cholesky factorisation and a triangular inverse in FP64 whatever the
 * element type, and stored in T.  A pivot that is not finite or not above shift / 4 — in exact arithmetic every pivot is >= shift, so
 * only round-off in E does that — is floored at shift / 4; nufft_precond_floored_cells counts the cells where that happened in the
 * last build.  B is stored like the operator's multipliers: K real grids (the diagonal) and K (K − 1) / 2 complex grids (the pairs
 * a < b, row-major), N^D cells each, 1 / n folded in.
 *
 * nufft_precond_apply, _update, _set_scaling, _get_info, _scaling_ptr and _destroy take a block object.  Every out[a] depends on every
 * in[b]; out[a] == in[a] is still allowed: all K inputs pass into K scratch arrays the object owns before any output is written.
 * Capture-safe, allocates nothing, no atomics: two runs and a graph replay give the same bits.  The fused path needs, on top of the
 * scalar object's conditions, the K lines of N_1 cells of one wave to fit LDS (K tiered 2, 4, 8, 16 as in the operator); where they
 * do not, the object takes the dense path silently.  In nufft_precond_info of a block object multiplier_bytes is the total over all
 * blocks, and max_e / min_e are the extreme DIAGONAL entries E_aa(q): they bound λ_max(E) from below and λ_min(E) from above.
 *
 * nufft_cg_solve accepts a block object on a coupled operator (one ρ_z, one γ, one done flag: the joint mode of the plain solver) and
 * refuses a scalar object there, and a block object whose operator no longer couples the same K (NUFFT_ERR_UNSUPPORTED).
 *
 * Added without changing NUFFT_MI355X_VERSION, nufft_precond_params or nufft_precond_info: detect by symbol (dlsym
 * nufft_precond_create_block). */
/* As nufft_precond_create, same parameters, validations in the same order; requires a coupled build in force (else
 * NUFFT_ERR_UNSUPPORTED, naming nufft_precond_create). */
int nufft_precond_create_block(nufft_precond** out, nufft_toeplitz* tz, const nufft_precond_params* params);
/* K for a block object, else 0. */
int32_t nufft_precond_num_coupled(const nufft_precond* pc);
/* Device pointer and bytes of B_ab, 0 <= a <= b < K (inspection and tests): real(T) for a = b, complex(T) for a < b; a > b
 * NUFFT_ERR_INVALID_ARG (B_ba = conj(B_ab)); a scalar object NUFFT_ERR_UNSUPPORTED. */
int nufft_precond_block_ptr(const nufft_precond* pc, int32_t a, int32_t b, void** out_ptr, int64_t* out_bytes);
/* Cells of the last build where a Cholesky pivot was floored (0 for a scalar object, -1 for NULL). */
int64_t nufft_precond_floored_cells(const nufft_precond* pc);

/* Preconditioned CG: with a preconditioner set, nufft_cg_solve runs
 *
 *     r = b − (G + λ) x0     z = M⁻¹ r     p = z     ρ_z = Re<r, z>     ρ = ‖r‖²     β0 = ‖b‖²
 *     for it = 1 ... max_iter:
 *         q = G p                                                         nufft_toeplitz_apply
 *         γ = Re<p, q> + λ ‖p‖²                                           cg_dot_kernel
 *         α = ρ_z / γ;  x += α p;  r −= α (q + λ p);  ρ' = ‖r‖²           pcg_update_kernel
 *         z = M⁻¹ r                                                       nufft_precond_apply
 *         ρ_z' = Re<r, z>                                                 cg_dot_kernel on (r, z)
 *         done from ρ';  p = z + (ρ_z'/ρ_z) p;  ρ_z = ρ_z';  ρ = ρ'       pcg_direction_kernel
 *
 * with the stopping test, residual and history of the plain solver (‖r‖ / ‖b‖), its freeze rule, fixed-order sums and capture rules;
 * NUFFT_CG_BREAKDOWN also when ρ_z is not positive and finite while the component is not done.  One more array per component (z),
 * allocated by this call (not on a capturing stream).  pc = NULL returns to the plain solver, which enqueues exactly what it did
 * before this entry point existed.  The preconditioner must have been created for the solver's operator (else
 * NUFFT_ERR_INVALID_ARG) and must outlive the solver or be cleared first. */
int nufft_cg_set_preconditioner(nufft_cg* cg, nufft_precond* pc);

/* ---- Sample-density compensation weights ------------------------ */
/* The weights w_j of nufft_exec_type1_cb / nufft_toeplitz_set_points for a point set, by the fixed-point iteration of Pipe & Menon
 * (MRM 41, 1999; NFFT.jl: sdc).  C is interpolation after spreading on the fine grid of a REAL-data plan with the parent plan's window:
 * (C w)_j = nufft_interpolate of the grid that nufft_fill_zeros + nufft_spread of w leaves — no FFT, no deconvolution.  All four windows
 * are non-negative, so C w > 0 for w > 0.
 *
 *     w = s 1 (or the caller's positive w0)
 *     for k = 0 ... max_iter − 1:
 *         v = C w                                                 nufft_fill_zeros, nufft_spread_deferred, nufft_interpolate
 *         δ_k = max_j |v_j − 1|;  bad = some v_j not positive and finite      dcf_check_kernel
 *         done ← done or bad or (k >= 1 and δ_k <= tol)           sticky      dcf_update_kernel
 *         w ← w / v                                               not applied once done
 *     finish: w ← w / Σ_j w_j  (NUFFT_DCF_NORMALIZE_SUM)  or unchanged (NUFFT_DCF_NORMALIZE_NONE)
 *
 * w / (C w) does not depend on the scale of w, so the first iterate is the same for every s, and δ_0 of the all-ones start only measures
 * the normalisation of the window: it is neither reported nor tested.  With a caller's w0 δ_0 is reported (never tested: k >= 1).
 * The window is not normalised (C 1 is about 1e30 in 2-D and 1e45 in 3-D at M = 4), which Float32 cannot hold.  The library's windows
 * carry an exact factor 2^k_d (nufft_info.window_scale_log2), so its C is 2^κ times the mathematical one, κ = 2 Σ_d k_d
 * (nufft_dcf_info.window_scale_log2), with values of order one.  The iteration runs on u = w / 2^κ, for which C w is what the device
 * computes from u: s = 2^κ, no intermediate leaves the range of Float32 in any dimension, and the normalised result does not contain
 * 2^κ at all.  NUFFT_DCF_NORMALIZE_NONE multiplies by 2^κ at the end, which in Float32 underflows where the true weights do (3-D);
 * a caller's w0 is read in true units, and its C w0 overflows Float32 where the true value does (status NUFFT_DCF_BREAKDOWN).
 * Σ w = 1 makes the diagonal of G = A^H W A one (G[k, k] = T_0 = Σ_j w_j): the scaling under which nufft_exec_type1 of w ⊙ y
 * approximates the inverse of nufft_exec_type2.
 *
 * A v_j that is not positive and finite (possible only with NaN coordinates, or a w0 whose C w0 leaves the range), or a w0 entry that
 * is not positive and finite, sets NUFFT_DCF_BREAKDOWN before anything is divided and leaves w as it was: the caller's w0, or the
 * iterate of the last completed iteration in the units of u, without the finish.
 * δ and Σ w are FP64 for both element types, formed without atomics in one fixed order; the weights are NOT bit-reproducible between
 * runs all the same, because spreading accumulates with LDS and global atomics in an order that varies.
 *
 * check_every = 0: all max_iter iterations are enqueued without synchronising or allocating (hipGraph-capture safe); a finished
 *                  state freezes w on the device, the remaining spreads and gathers run as scratch work.
 * check_every = k > 0: after every k iterations the host reads the done flag and stops enqueuing.  Refused on a capturing stream.
 *
 * The object owns an internal real-data plan (dtype, ndim, N, σ, half support, kernel, the parent's shape parameter per dimension,
 * evaluation mode, point convention, options, device of the parent; ntransforms = 1; fftshift does not matter) that is kept across
 * point sets; no pointer to the parent is kept.  Its fine grid can differ from a complex parent's in dimension 1, where a real plan
 * needs an even size: nufft_dcf_info.N_over is the grid actually used.
 * Added after ABI 104 without changing NUFFT_MI355X_VERSION: detect by symbol (dlsym nufft_dcf_create) and compare
 * nufft_sizeof_dcf_params() / nufft_sizeof_dcf_info() with your own. */
typedef struct nufft_dcf nufft_dcf; /* opaque */

enum { NUFFT_DCF_MAX_ITER = 0,   /* max_iter iterations ran                                     */
       NUFFT_DCF_CONVERGED = 1,  /* δ_k <= tol at some k >= 1                                   */
       NUFFT_DCF_BREAKDOWN = 2   /* a v_j or w0_j not positive and finite: nothing was divided  */ };
enum { NUFFT_DCF_NORMALIZE_SUM = 0, NUFFT_DCF_NORMALIZE_NONE = 1 };

typedef struct nufft_dcf_params {
    int32_t struct_size;     /* sizeof(nufft_dcf_params) of the caller's header (0 = this layout)                                  */
    int32_t max_iter;        /* 1 ... 2^24                                                                                         */
    int32_t check_every;     /* 0, or the number of iterations between two looks at the done flag                                  */
    int32_t normalize;       /* NUFFT_DCF_NORMALIZE_*                                                                              */
    double tol;              /* >= 0, finite; 0 = run max_iter iterations                                                          */
} nufft_dcf_params;

typedef struct nufft_dcf_info {
    int32_t struct_size;     /* sizeof(nufft_dcf_info) of the caller's header, set before the call (0 = this layout)               */
    int32_t ndim, dtype, device, max_iter, check_every, normalize;
    int32_t workgroups;      /* of the array kernels for the current point set (0: none yet)                                       */
    int32_t iterations_enqueued; /* by the last nufft_dcf_compute (check_every > 0 stops early); -1 before the first              */
    int32_t window_scale_log2;   /* κ: the device's C is 2^κ times the mathematical one                                            */
    int64_t N_over[3];       /* fine grid of the internal real plan (1 beyond ndim)                                                */
    double tol;
    double beta[3];          /* window shape parameter per dimension (the parent's)                                                */
    int64_t capacity;        /* points the vector v holds; grows with nufft_dcf_set_points, never shrinks                          */
    int64_t num_points;      /* of the last nufft_dcf_set_points (-1: none yet)                                                    */
    int64_t workspace_bytes; /* device bytes the object owns next to its plan (a host-only object: what a device object of these
                                parameters and this capacity holds): v, partials, scalars, history                                 */
    int64_t plan_bytes;      /* nufft_info.workspace_bytes of the internal plan right now (0 for a host-only object)               */
} nufft_dcf_info;

/* Builds the internal plan and allocates partials, scalars, history and a few pinned host words.  A host-only plan (device = -1) gives
 * a host-only object that answers nufft_dcf_get_info only.  Refusals: null arguments, max_iter < 1 or > 2^24, check_every < 0, tol < 0
 * or not finite, an unknown normalize NUFFT_ERR_INVALID_ARG; whatever nufft_plan_create_ex refuses for the internal plan. */
int nufft_dcf_create(nufft_dcf** out, const nufft_plan* plan, const nufft_dcf_params* params);
int nufft_dcf_destroy(nufft_dcf* dcf);
/* As nufft_set_points on the internal plan.  Grows v when num_points exceeds the capacity (never on a capturing stream). */
int nufft_dcf_set_points(nufft_dcf* dcf, int64_t num_points, const void* const* coords, void* stream);
/* w_inout: device vector T[num_points] (real, the plan's precision, 16-byte aligned) in the caller's point order.  use_w0 = 0: it is
 * overwritten; use_w0 != 0: it holds the start.  Allocates nothing.  num_points = 0 is a no-op.  Refusals, all before anything is
 * enqueued: a host-only object NUFFT_ERR_NO_DEVICE, no points yet NUFFT_ERR_NO_POINTS, a null or misaligned pointer, check_every > 0
 * on a capturing stream NUFFT_ERR_INVALID_ARG. */
int nufft_dcf_compute(nufft_dcf* dcf, void* w_inout, int use_w0, void* stream);
/* Static facts and sizes; does not synchronise. */
int nufft_dcf_get_info(const nufft_dcf* dcf, nufft_dcf_info* out);
/* Outcome of the last compute: divisions applied, NUFFT_DCF_* status, the last reported δ (NaN: none).  Each output may be NULL.
 * Synchronises `stream` (never a capturing one). */
int nufft_dcf_get_result(nufft_dcf* dcf, int32_t* iterations, int32_t* status, double* residual, void* stream);
/* host_out[max_iter]: entry k = δ_k (entry 0 only with a caller's w0); NaN where iteration k reported nothing (δ_0 of the all-ones
 * start, frozen, or beyond the last iteration run).  Synchronises `stream`. */
int nufft_dcf_history(nufft_dcf* dcf, double* host_out, int64_t capacity, void* stream);
int64_t nufft_sizeof_dcf_params(void);
int64_t nufft_sizeof_dcf_info(void);

/* ---- Wavelet transform with its proximal map -------------------- */
/* Orthogonal periodic wavelets of 2 taps (Haar) and 4 taps (Daubechies, two vanishing moments) on arrays laid out like those of
 * nufft_toeplitz_apply: complex(T)[N...], T the plan's precision, ntransforms components, D = 1, 2, 3.  One analysis stage along an axis
 * of length n is
 *
 *     lo[i] = Σ_k h[k] a[(2i + k) mod n]      hi[i] = Σ_k g[k] a[(2i + k) mod n]      g[k] = (−1)^k h[L − 1 − k],  i < n / 2
 *
 * (filter coefficients: FP64 constants cast to T), applied separably; every level recurses on the low-pass corner, and the output is
 * the Mallat layout in one array of the input's shape: along every axis the approximation of the deepest level sits at [0, N_d / 2^L),
 * the details of level l at [N_d / 2^l, N_d / 2^(l − 1)).  The transform is orthogonal: the inverse is its transpose.  It acts on the
 * array AS STORED, periodic in the storage index.  A periodic transform of L levels commutes with cyclic shifts by multiples of 2^L, so
 * fftshift = 1 and fftshift = 0 plans (whose storage orders differ by a shift of N_d / 2) give the same proximal map whenever 2^(L + 1)
 * divides every N_d; otherwise the two orders differ only in which pixels are paired.
 *
 * One launch per level handles all D dimensions of a tile in LDS (a level reads its sub-box once and writes it once); the levels pass
 * their low-pass corner through two scratch arrays the object owns (n / 2^D and n / 4^D elements per component), never in place.
 * forward, inverse and shrink allocate nothing, do not synchronise and are hipGraph-capture safe; no atomics: two runs give the same
 * bits.  The object keeps scratch and partial sums: one call at a time per object.
 *
 * Added after ABI 104 without changing NUFFT_MI355X_VERSION: detect by symbol (dlsym nufft_wavelet_create) and compare
 * nufft_sizeof_wavelet_params() / nufft_sizeof_wavelet_info() with your own. */
typedef struct nufft_wavelet nufft_wavelet; /* opaque */

enum { NUFFT_WAVELET_HAAR = 0, NUFFT_WAVELET_DB2 = 1 };

typedef struct nufft_wavelet_params {
    int32_t struct_size;     /* sizeof(nufft_wavelet_params) of the caller's header (0 = this layout)                              */
    int32_t wavelet;         /* NUFFT_WAVELET_*                                                                                    */
    int32_t levels;          /* L >= 1                                                                                             */
    int32_t reserved;        /* 0                                                                                                  */
} nufft_wavelet_params;

typedef struct nufft_wavelet_info {
    int32_t struct_size;     /* sizeof(nufft_wavelet_info) of the caller's header, set before the call (0 = this layout)           */
    int32_t ndim, dtype, ntransforms, device;
    int32_t wavelet;         /* NUFFT_WAVELET_*                                                                                    */
    int32_t taps;            /* 2 or 4                                                                                             */
    int32_t levels;
    int64_t N[3];            /* 1 beyond ndim                                                                                      */
    int64_t scratch_bytes;   /* the two low-pass scratch arrays of all components                                                  */
    int64_t workspace_bytes; /* device bytes owned: scratch_bytes + partial sums                                                   */
} nufft_wavelet_info;

/* Takes element type, shape, ntransforms and device from the plan; the plan is not kept.  Refusals, in order: null arguments, a
 * struct_size smaller than the published layout NUFFT_ERR_INVALID_ARG; a real-data plan NUFFT_ERR_UNSUPPORTED (as
 * nufft_toeplitz_create); an unknown wavelet, levels < 1, an N_d that is no multiple of 2^levels, DB2 with N_d / 2^levels < 2 (every
 * level's input must be at least one filter long) NUFFT_ERR_INVALID_ARG; a host-only plan NUFFT_ERR_NO_DEVICE. */
int nufft_wavelet_create(nufft_wavelet** out, const nufft_plan* plan, const nufft_wavelet_params* params);
/* The same from a Toeplitz operator (the operator is not kept). */
int nufft_wavelet_create_for_operator(nufft_wavelet** out, const nufft_toeplitz* tz, const nufft_wavelet_params* params);
int nufft_wavelet_destroy(nufft_wavelet* w);
/* Static facts and sizes; does not synchronise. */
int nufft_wavelet_get_info(const nufft_wavelet* w, nufft_wavelet_info* out);
/* out[c] = W in[c] (Mallat layout) for every component; host tables of ntransforms device pointers, 16-byte aligned.  in is only read.
 * Refusals, before anything is enqueued: a null table or vector, a pointer that is not 16-byte aligned, out[c] overlapping any in[c']
 * (a level reads its sub-box while other tiles store into it) or another out[c'] NUFFT_ERR_INVALID_ARG. */
int nufft_wavelet_forward(nufft_wavelet* w, void* const* out, const void* const* in, void* stream);
/* out[c] = W^H in[c]; same rules. */
int nufft_wavelet_inverse(nufft_wavelet* w, void* const* out, const void* const* in, void* stream);
/* The forward transform whose detail coefficients are soft-thresholded where they are stored: c <- c · max(1 − t[c'] / |c|, 0) with the
 * threshold t[c'] of the coefficient's component (HOST array of ntransforms values, finite and >= 0, read during the call); the
 * approximation band of the deepest level is never thresholded, and t = 0 stores exactly what nufft_wavelet_forward stores.
 * l1_out_device (device, double[ntransforms], may be NULL): Σ |stored detail coefficient| per component, FP64, summed in one fixed
 * order.  With inverse this is the proximal map of t ‖D W x‖₁: x <- W^H shrink(W x, t); ADMM's x-update is nufft_cg_solve with
 * lambda = ρ and a starting guess. */
int nufft_wavelet_shrink(nufft_wavelet* w, void* const* out, const void* const* in, const double* t, double* l1_out_device, void* stream);
int64_t nufft_sizeof_wavelet_params(void);
int64_t nufft_sizeof_wavelet_info(void);

/* ---- Largest eigenvalue of the Toeplitz normal operator ---------- */
/* Power iteration on whatever nufft_toeplitz_apply currently computes (plain, with coil maps, coupled):
 *
 *     v = v0;  repeat iters times:  g = G v;  ρ = Re<v, g> / <v, v>;  v = g / ‖g‖
 *
 * out_host[c], c < ntransforms: the FP64 Rayleigh quotient ρ of the LAST apply — a lower bound of λ_max(G).  Uncoupled components give
 * one value each; coupled components are one vector (sums over all components) and every entry receives the same value.  <v, v> = 0
 * gives 0.  v0: host table of ntransforms device pointers, complex(T)[N...], 16-byte aligned, only read.  Sums are FP64 in one fixed
 * order.  Allocates two arrays per component for the duration of the call, synchronises `stream` and frees them: refused on a
 * capturing stream.  Refusals: null arguments, iters < 1, a null or misaligned vector, a capturing stream NUFFT_ERR_INVALID_ARG; a
 * host-only operator NUFFT_ERR_NO_DEVICE; no spectrum yet NUFFT_ERR_NO_POINTS.  Added without changing NUFFT_MI355X_VERSION. */
int nufft_toeplitz_max_eigenvalue(nufft_toeplitz* tz, const void* const* v0, int32_t iters, double* out_host, void* stream);

/* ---- FISTA with an l1-wavelet prior on the Toeplitz normal operator ---- */
/* Minimises, for every component c (coupled components: jointly, the quadratic term coupling them),
 *
 *     ½ <x, (G + μ I) x> − Re<b, x> + Σ_c l1_c ‖D W x_c‖₁
 *
 * G what the nufft_toeplitz object applies, W the wavelet transform above, D the projection on its detail bands, by the accelerated
 * proximal-gradient iteration of Beck & Teboulle (2009) with the fixed step τ.  Start: t_1 = 1, z = x = x0 (or 0).
 *
 *     for it = 1 ... max_iter:
 *         q = G z                                                          nufft_toeplitz_apply
 *         v = z − τ (q + μ z − b)                                          fista_gradient_kernel, in place over q
 *         c = shrink(W v, τ l1)                                            one launch per level, threshold and ‖·‖₁ partials on store
 *         x⁺ = W^H c;  z = x⁺ + ((t_it − 1) / t_it+1) (x⁺ − x);  x = x⁺    one launch per level, the step on the last level's store
 *         change = ‖x⁺ − x‖ / ‖x⁺‖ (0 when both are 0)                     fista_decide_kernel
 *         done ← change <= tol, or change not finite (NUFFT_FISTA_BREAKDOWN)
 *
 * t_it+1 = (1 + sqrt(1 + 4 t_it²)) / 2 depends on the iteration number only: the host passes the factor as a kernel argument.  The
 * iteration converges for τ <= 1 / (λ_max(G) + μ) (nufft_toeplitz_max_eigenvalue).  A component that is done is FROZEN: no kernel writes
 * its x, z or scalars again.  Uncoupled operators stop per component; a coupled operator is one system with one change and one flag,
 * reported identically for every component.  Sums and scalars are FP64, formed without atomics in one fixed order: two runs, and a
 * replayed hipGraph, give the same bits.
 *
 * check_every = 0: all max_iter iterations are enqueued without synchronising or allocating (hipGraph-capture safe).
 * check_every = k > 0: after every k iterations the host reads the done flags and stops enqueuing once every component is done.
 *                  Refused on a capturing stream.  Both modes return bit-identical x, iteration counts and history.
 *
 * Added after ABI 104 without changing NUFFT_MI355X_VERSION: detect by symbol (dlsym nufft_fista_create) and compare
 * nufft_sizeof_fista_params() / nufft_sizeof_fista_info() with your own. */
typedef struct nufft_fista nufft_fista; /* opaque */

enum { NUFFT_FISTA_MAX_ITER = 0,   /* max_iter iterations ran without reaching tol */
       NUFFT_FISTA_CONVERGED = 1,  /* change <= tol                                */
       NUFFT_FISTA_BREAKDOWN = 2   /* change not finite: the component was frozen  */ };

typedef struct nufft_fista_params {
    int32_t struct_size;     /* sizeof(nufft_fista_params) of the caller's header (0 = this layout)                                */
    int32_t max_iter;        /* 1 ... 2^24                                                                                         */
    int32_t check_every;     /* 0, or the number of iterations between two looks at the done flags                                 */
    int32_t wavelet;         /* NUFFT_WAVELET_*                                                                                    */
    int32_t levels;          /* of the wavelet transform                                                                           */
    int32_t reserved;        /* 0                                                                                                  */
    double tol;              /* >= 0, finite; 0 = run max_iter iterations unless x stops changing exactly                          */
    double step;             /* τ > 0, finite                                                                                      */
    double l1;               /* >= 0, finite: the weight of every component until nufft_fista_set_l1                               */
    double lambda;           /* the Tikhonov μ: >= 0, finite                                                                       */
} nufft_fista_params;

typedef struct nufft_fista_info {
    int32_t struct_size;     /* sizeof(nufft_fista_info) of the caller's header, set before the call (0 = this layout)             */
    int32_t ntransforms, dtype, max_iter, check_every, wavelet, levels;
    int32_t iterations_enqueued; /* by the last nufft_fista_solve (check_every > 0 stops early); -1 before the first               */
    double tol, step, lambda;
    int64_t array_bytes;     /* z, q / v, c: 3 arrays per component                                                                */
    int64_t workspace_bytes; /* device bytes owned: array_bytes + the wavelet object's scratch and partials + partial sums + scalars
                                + history                                                                                          */
} nufft_fista_info;

/* Allocates z, q, c (3 arrays per component), a wavelet object for the operator's shape, partial sums, scalars and history on the
 * operator's device.  The solver keeps the POINTER `tz`: the operator must outlive it; nufft_toeplitz_set_points / _set_spectrum on it
 * between two solves is allowed.  Refusals: null arguments, max_iter < 1 or > 2^24, check_every < 0, tol < 0, l1 < 0, lambda < 0,
 * step <= 0 or non-finite values, and whatever nufft_wavelet_create refuses for the shape NUFFT_ERR_INVALID_ARG; a host-only operator
 * NUFFT_ERR_NO_DEVICE (after the argument checks). */
int nufft_fista_create(nufft_fista** out, nufft_toeplitz* tz, const nufft_fista_params* params);
int nufft_fista_destroy(nufft_fista* f);
/* One weight per component (host array, count = ntransforms, each finite and >= 0) for the following solves. */
int nufft_fista_set_l1(nufft_fista* f, const double* l1, int64_t count);
/* x_inout[c], b[c] as in nufft_cg_solve, with the same refusals.  use_x0 = 0: start from zero. */
int nufft_fista_solve(nufft_fista* f, void* const* x_inout, const void* const* b, int use_x0, void* stream);
/* Static facts and sizes; does not synchronise. */
int nufft_fista_get_info(const nufft_fista* f, nufft_fista_info* out);
/* Per-component outcome of the last solve: iterations that changed the component, NUFFT_FISTA_* status, the last change.  Each output
 * may be NULL; `capacity` entries each, at least ntransforms.  Synchronises `stream` (never a capturing one). */
int nufft_fista_get_result(nufft_fista* f, int32_t* iterations, int32_t* status, double* change, int64_t capacity, void* stream);
/* host_out[max_iter][ntransforms][2]: row it − 1 holds the change and ‖D W x‖₁ of every component after iteration it (a coupled operator:
 * the joint values); NaN where the iteration did not change the component.  Synchronises `stream`. */
int nufft_fista_history(nufft_fista* f, double* host_out, int64_t capacity, void* stream);
int64_t nufft_sizeof_fista_params(void);
int64_t nufft_sizeof_fista_info(void);

/* ---- Locally low-rank proximal map ------------------------------- */
/* The K = ntransforms arrays x_a (complex(T)[N...], as those of nufft_toeplitz_apply) are cut into spatial blocks of b_1 x ... x b_D
 * cells; storage index i_d belongs to block floor(((i_d − s_d) mod N_d) / b_d), s the cyclic shift, 0 <= s_d < b_d.  Like the wavelet
 * transform the map acts on the arrays AS STORED and is periodic in the storage index.  Every block gives a B x K Casorati matrix M
 * (B = Π b_d, column a = the block's cells of x_a), and the map is singular-value soft-thresholding of every M,
 *
 *     prox_{t ‖·‖_*}(M) = U max(Σ − t, 0) V^H,
 *
 * computed without an SVD of M:  H = M^H M (K x K, accumulated in FP64 for both element types, one fixed order);  H = V Λ V^H by cyclic
 * complex Jacobi in FP64 (row-cyclic rotation order; a rotation is skipped when |h_pq|² <= 2^-106 h_pp h_qq or |h_pq| <= 2^-60 trace H;
 * the sweeps stop after the first one that rotates nothing, at most jacobi_sweeps_max);  σ_i = sqrt(max(λ_i, 0)),
 * f_i = σ_i > t ? 1 − t / σ_i : 0;  M <- M V diag(f) V^H.  Nothing is divided where σ_i <= t: a zero block stays zero.  K = 1 is block-wise
 * group shrinkage.  One kernel reads every array once and writes it once; a block's values stay in LDS in between.  No atomics: two
 * runs and a replayed hipGraph give the same bits.
 *
 * Block sides are powers of two, 1 ... 16, each dividing its N_d, with B · K <= 8192.
 *
 * Added after ABI 104 without changing NUFFT_MI355X_VERSION: detect by symbol (dlsym nufft_llr_create) and compare
 * nufft_sizeof_llr_params() / nufft_sizeof_llr_info() with your own. */
typedef struct nufft_llr nufft_llr; /* opaque */

typedef struct nufft_llr_params {
    int32_t struct_size;     /* sizeof(nufft_llr_params) of the caller's header (0 = this layout)                                  */
    int32_t block[3];        /* block sides: powers of two, 1 ... 16, b_d | N_d; 1 beyond ndim                                     */
    int32_t shifts;          /* 0 / 1: nufft_fista_create_llr draws a new cyclic shift every iteration (ignored by nufft_llr_apply) */
    int32_t reserved;        /* 0                                                                                                  */
    uint64_t seed;           /* of the shift sequence                                                                              */
} nufft_llr_params;

typedef struct nufft_llr_info {
    int32_t struct_size;     /* sizeof(nufft_llr_info) of the caller's header, set before the call (0 = this layout)               */
    int32_t ndim, dtype, ntransforms, device;
    int32_t block[3];
    int32_t shifts;
    int64_t N[3];            /* 1 beyond ndim                                                                                      */
    int64_t blocks;          /* Π N_d / b_d                                                                                        */
    int64_t workspace_bytes; /* device bytes owned: the partial sums                                                               */
    int32_t jacobi_sweeps_max;
    int32_t waves_per_cu;    /* the LDS bound: resident waves per compute unit that the kernel's LDS use admits for this (element
                                type, K, B).  nufft_llr_apply's variant reaches it; the solver's fused variant needs more registers
                                and is limited to 20 waves per compute unit where this reads more            */
} nufft_llr_info;

/* Takes element type, shape, ntransforms and device from the plan; the plan is not kept.  Refusals, in order: null arguments, a
 * struct_size smaller than the published layout NUFFT_ERR_INVALID_ARG; a real-data plan NUFFT_ERR_UNSUPPORTED; a block side that is no
 * power of two in 1 ... 16 (or not 1 beyond ndim), shifts not 0 / 1, a b_d that does not divide N_d NUFFT_ERR_INVALID_ARG; more than 16
 * transforms or B · K > 8192 NUFFT_ERR_UNSUPPORTED; a host-only plan NUFFT_ERR_NO_DEVICE. */
int nufft_llr_create(nufft_llr** out, const nufft_plan* plan, const nufft_llr_params* params);
/* The same from a Toeplitz operator (the operator is not kept). */
int nufft_llr_create_for_operator(nufft_llr** out, const nufft_toeplitz* tz, const nufft_llr_params* params);
int nufft_llr_destroy(nufft_llr* l);
/* Static facts and sizes; does not synchronise. */
int nufft_llr_get_info(const nufft_llr* l, nufft_llr_info* out);
/* out = prox_{t ‖·‖_LLR}(in) with the given shift (host array of ndim values, 0 <= shift[d] < b_d; NULL = zero shift).  Host tables of
 * ntransforms device pointers, 16-byte aligned.  out[c] may be exactly in[c] (a block is owned by one workgroup, which stores after it
 * has loaded); any other overlap between an output and an input or another output is refused.  nuc_out_device (device, double[1], may be
 * NULL): Σ over all blocks of the kept singular values max(σ_i − t, 0), the LLR norm of the output, FP64, summed in one fixed order.
 * Allocates nothing, does not synchronise, hipGraph-capture safe; the object keeps the partial sums: one call at a time per object.
 * Refusals, before anything is enqueued: a null table or vector, a pointer that is not 16-byte aligned, a partial overlap, t < 0 or not
 * finite, a shift outside [0, b_d) NUFFT_ERR_INVALID_ARG. */
int nufft_llr_apply(nufft_llr* l, void* const* out, const void* const* in, double t, const int32_t* shift, double* nuc_out_device, void* stream);
int64_t nufft_sizeof_llr_params(void);
int64_t nufft_sizeof_llr_info(void);

/* ---- FISTA with a locally low-rank prior ------------------------- */
/* Minimises  ½ <x, (G + μ I) x> − Re<b, x> + nuc · Σ_blocks ‖M_block(x)‖_*  with the iteration of nufft_fista_create, the proximal map
 * being the one above with t = τ · nuc.  The prior couples the components: they are ONE system with one change, one flag and one status,
 * reported identically for every component, whether the operator is coupled or not.  One iteration is
 *
 *     q = G z                                                                          nufft_toeplitz_apply
 *     v = z − τ (q + μ z − b) on load;  x⁺ = prox(v);  z = x⁺ + β (x⁺ − x), x = x⁺ on store    one kernel
 *     change, done flag, history                                                       the decision kernel
 *
 * The solver owns two arrays per component (z, q; nufft_fista_info.array_bytes says so; wavelet and levels read 0).  Reads max_iter,
 * check_every, tol, step and lambda from `params`; wavelet, levels and l1 must be 0 (NUFFT_ERR_INVALID_ARG otherwise); nuc >= 0, finite.
 * History column 2 holds Σ_blocks ‖M_block(x⁺)‖_* after the iteration.  nufft_fista_set_l1 on such a solver and nufft_fista_set_nuc on a
 * wavelet solver return NUFFT_ERR_INVALID_ARG.  Everything else (solve, result, history, capture with check_every = 0, set_points /
 * set_spectrum between two solves, bit-identical modes) is as for nufft_fista_create.
 *
 * llr->shifts = 1: iteration it uses the cyclic shift s(it), which depends on it and llr->seed only:  state_0 = seed;  for it = 1, 2, ...
 * and d = 1 ... ndim:  state <- state · 6364136223846793005 + 1442695040888963407 (mod 2^64),  s_d = (state >> 33) mod b_d.  The host passes
 * the shift as kernel arguments.  With shifts the objective changes every iteration and the relative change does not fall to a small
 * tol (it stalls around 1e-2 ... 7e-2 on small systems): shifts are for tol = 0 and a fixed max_iter. */
int nufft_fista_create_llr(nufft_fista** out, nufft_toeplitz* tz, const nufft_fista_params* params, const nufft_llr_params* llr, double nuc);
/* The weight of the LLR prior for the following solves (>= 0, finite). */
int nufft_fista_set_nuc(nufft_fista* f, double nuc);

/* ---- Total variation: the periodic difference operator ----------- */
/* On arrays laid out like those of nufft_toeplitz_apply (complex(T)[N...], ntransforms components, D = 1, 2, 3), AS STORED and periodic
 * in the storage index:
 *
 *     (∇x)_d[i] = x[i + e_d] − x[i]                  d = 1 ... D, indices mod N_d          (D arrays per component)
 *     (∇ᴴy)[i]  = Σ_d (y_d[i − e_d] − y_d[i])        summed in the order d = 1 ... D
 *     ‖∇x‖₂,₁   = Σ_i |(∇x)_i|₂,   |(∇x)_i|₂ = sqrt(Σ_d |(∇x)_d[i]|²)                      isotropic: one norm over the D complex differences
 *
 * The operator commutes with every cyclic shift, so fftshift = 1 and fftshift = 0 plans give the same prior after reordering, with no
 * divisibility condition.  A table of "D arrays per component" holds ntransforms · D pointers, y_d of component c at [c · D + (d − 1)].
 * The calls allocate nothing, do not synchronise and are hipGraph-capture safe; no atomics: two runs give the same bits.  The object
 * keeps partial sums: one call at a time per object.
 *
 * Added after ABI 104 without changing NUFFT_MI355X_VERSION: detect by symbol (dlsym nufft_tv_create) and compare
 * nufft_sizeof_tv_info() with your own. */
typedef struct nufft_tv nufft_tv; /* opaque */

typedef struct nufft_tv_info {
    int32_t struct_size;     /* sizeof(nufft_tv_info) of the caller's header, set before the call (0 = this layout)                */
    int32_t ndim, dtype, ntransforms, device;
    int32_t tile[3];         /* cells of a workgroup's tile per dimension (1 beyond ndim)                                          */
    int64_t N[3];            /* 1 beyond ndim                                                                                      */
    int64_t workgroups;      /* per component and launch                                                                           */
    int64_t workspace_bytes; /* device bytes owned: the partial sums                                                               */
} nufft_tv_info;

/* Takes element type, shape, ntransforms and device from the plan; the plan is not kept.  Refusals, in order: null arguments
 * NUFFT_ERR_INVALID_ARG; a real-data plan NUFFT_ERR_UNSUPPORTED (as nufft_toeplitz_create); N_1 > 2^30, or more than 2^20 (ndim = 2) /
 * 2^17 (ndim = 3) cells along dimension 2, or more than 2^18 along dimension 3, or more than 2^31 - 1 workgroups over all components
 * (tiles of nufft_tv_info.tile cells, times ntransforms) NUFFT_ERR_UNSUPPORTED; a host-only plan NUFFT_ERR_NO_DEVICE. */
int nufft_tv_create(nufft_tv** out, const nufft_plan* plan);
/* The same from a Toeplitz operator (the operator is not kept). */
int nufft_tv_create_for_operator(nufft_tv** out, const nufft_toeplitz* tz);
int nufft_tv_destroy(nufft_tv* tv);
/* Static facts and sizes; does not synchronise. */
int nufft_tv_get_info(const nufft_tv* tv, nufft_tv_info* out);
/* y_out[c · D + d − 1] = (∇x[c])_d: one subtraction per value, so the result is the correctly rounded difference.  Host tables of device
 * pointers (ntransforms · D and ntransforms), 16-byte aligned; x is only read.  Refusals, before anything is enqueued: a null table or
 * vector, a pointer that is not 16-byte aligned, an output overlapping an input (a cell's neighbours are read while other workgroups
 * store) or another output NUFFT_ERR_INVALID_ARG. */
int nufft_tv_gradient(nufft_tv* tv, void* const* y_out, const void* const* x, void* stream);
/* x_out[c] = ∇ᴴ (y[c · D], ..., y[c · D + D − 1]); same rules. */
int nufft_tv_adjoint(nufft_tv* tv, void* const* x_out, const void* const* y, void* stream);
/* sums_out_device (device, double[ntransforms]): ‖∇x[c]‖₂,₁ per component.  The differences are formed in T, their squares, the square
 * root and the sum in FP64, in one fixed order. */
int nufft_tv_norm(nufft_tv* tv, const void* const* x, double* sums_out_device, void* stream);
int64_t nufft_sizeof_tv_info(void);

/* ---- Primal-dual solver with a total-variation prior ------------- */
/* Minimises, for every component c (coupled components: jointly, the quadratic term coupling them),
 *
 *     ½ <x, (G + μ I) x> − Re<b, x> + tv_c · Σ_i |(∇x)_i|₂
 *
 * G what the nufft_toeplitz object applies, ∇ the periodic forward difference above.  The proximal map of ‖∇x‖₂,₁ has no closed form, so
 * the iteration is the primal-dual one of Condat (2013) and Vũ (2013) (Chambolle & Pock 2011 with the smooth term taken by its
 * gradient), with fixed steps τ and σ and one dual array y_d per dimension:
 *
 *     start:  x = x0 (or 0),  y_d = 0
 *     for it = 1 ... max_iter:
 *         q  = G x                                        nufft_toeplitz_apply
 *         x⁺ = x − τ (q + μ x − b + ∇ᴴ y)                 tv_primal_kernel: stores x <- x⁺ and q <- x̄ = x⁺ + (x⁺ − x),
 *                                                         partials of ‖x⁺ − x‖², ‖x⁺‖²
 *         y  <- P_tv(y + σ ∇x̄)                            tv_dual_kernel, in place: P_t(v)_i = v_i · min(1, t / |v_i|₂);
 *                                                         partial of Σ_i |(∇x⁺)_i|₂
 *         change = ‖x⁺ − x‖ / ‖x⁺‖ (0 when both are 0);  history row (change, Σ_i |(∇x⁺)_i|₂)          tv_decide_kernel
 *         done <- change <= tol, or change not finite (NUFFT_TVPD_BREAKDOWN)
 *
 * The iteration converges for 1 / τ − σ ‖∇‖² >= L / 2, L = λ_max(G) + μ.  With ‖∇‖² <= 4 D, τ <= 1 / L (nufft_toeplitz_max_eigenvalue) and
 * the default σ = 1 / (8 D τ) the left side is 1 / (2 τ) >= L / 2.  Any finite σ > 0 is accepted: the condition is the caller's to keep.
 * tv_c = 0 leaves y exactly zero: the iteration is then plain gradient descent on (G + μ) x = b.  y restarts at 0 in every solve.
 *
 * The primal kernel reads y at neighbours and writes only x[i] and q[i]; the dual kernel reads x̄ and x⁺ at neighbours and writes only
 * y_d[i]: no launch reads at a neighbour an array it writes.  The solver owns 1 + D arrays per component (q and y_1 ... y_D).  A
 * component that is done is FROZEN: no kernel writes its x, y or scalars again, and its x is bit-equal to that of a solve of this
 * component alone.  Uncoupled operators stop per component; a coupled operator is one system with one change and one flag, reported
 * identically for every component.  Sums and scalars are FP64, formed without atomics in one fixed order: two runs, and a replayed
 * hipGraph, give the same bits.
 *
 * check_every = 0: all max_iter iterations are enqueued without synchronising or allocating (hipGraph-capture safe).
 * check_every = k > 0: after every k iterations the host reads the done flags and stops enqueuing once every component is done.
 *                  Refused on a capturing stream.  Both modes return bit-identical x, iteration counts and history.
 *
 * Added after ABI 104 without changing NUFFT_MI355X_VERSION: detect by symbol (dlsym nufft_tvpd_create) and compare
 * nufft_sizeof_tvpd_params() / nufft_sizeof_tvpd_info() with your own. */
typedef struct nufft_tvpd nufft_tvpd; /* opaque */

enum { NUFFT_TVPD_MAX_ITER = 0,   /* max_iter iterations ran without reaching tol */
       NUFFT_TVPD_CONVERGED = 1,  /* change <= tol                                */
       NUFFT_TVPD_BREAKDOWN = 2   /* change not finite: the component was frozen  */ };

typedef struct nufft_tvpd_params {
    int32_t struct_size;     /* sizeof(nufft_tvpd_params) of the caller's header (0 = this layout)                                 */
    int32_t max_iter;        /* 1 ... 2^24                                                                                         */
    int32_t check_every;     /* 0, or the number of iterations between two looks at the done flags                                 */
    int32_t reserved;        /* 0                                                                                                  */
    double tol;              /* >= 0, finite; 0 = run max_iter iterations unless x stops changing exactly                          */
    double step;             /* τ > 0, finite                                                                                      */
    double sigma;            /* σ > 0, finite; 0 = 1 / (8 ndim τ)                                                                  */
    double tv;               /* >= 0, finite: the weight of every component until nufft_tvpd_set_tv                                */
    double lambda;           /* the Tikhonov μ: >= 0, finite                                                                       */
} nufft_tvpd_params;

typedef struct nufft_tvpd_info {
    int32_t struct_size;     /* sizeof(nufft_tvpd_info) of the caller's header, set before the call (0 = this layout)              */
    int32_t ntransforms, dtype, ndim, max_iter, check_every;
    int32_t iterations_enqueued; /* by the last nufft_tvpd_solve (check_every > 0 stops early); -1 before the first                */
    int32_t reserved;
    double tol, step, sigma, lambda;   /* sigma: the value in use                                                                  */
    int64_t array_bytes;     /* q, y_1 ... y_ndim: 1 + ndim arrays per component (nufft_tvpd_create_temporal: + z, − y if spatial = 0) */
    int64_t workspace_bytes; /* device bytes owned: array_bytes + partial sums + scalars + history                                 */
} nufft_tvpd_info;

/* Allocates q and y (1 + ndim arrays per component), partial sums, scalars and history on the operator's device.  The solver keeps the
 * POINTER `tz`: the operator must outlive it; nufft_toeplitz_set_points / _set_spectrum on it between two solves is allowed.  Refusals:
 * null arguments, max_iter < 1 or > 2^24, check_every < 0, tol < 0, tv < 0, lambda < 0, sigma < 0, step <= 0 or non-finite values
 * NUFFT_ERR_INVALID_ARG; whatever nufft_tv_create refuses for the shape; a host-only operator NUFFT_ERR_NO_DEVICE (after the argument
 * checks). */
int nufft_tvpd_create(nufft_tvpd** out, nufft_toeplitz* tz, const nufft_tvpd_params* params);
int nufft_tvpd_destroy(nufft_tvpd* s);
/* One weight per component (host array, count = ntransforms, each finite and >= 0) for the following solves. */
int nufft_tvpd_set_tv(nufft_tvpd* s, const double* weights, int64_t count);
/* x_inout[c], b[c] as in nufft_cg_solve, with the same refusals (x overlapping b among them).  use_x0 = 0: start from zero. */
int nufft_tvpd_solve(nufft_tvpd* s, void* const* x_inout, const void* const* b, int use_x0, void* stream);
/* Static facts and sizes; does not synchronise. */
int nufft_tvpd_get_info(const nufft_tvpd* s, nufft_tvpd_info* out);
/* Per-component outcome of the last solve: iterations that changed the component, NUFFT_TVPD_* status, the last change.  Each output
 * may be NULL; `capacity` entries each, at least ntransforms.  Synchronises `stream` (never a capturing one). */
int nufft_tvpd_get_result(nufft_tvpd* s, int32_t* iterations, int32_t* status, double* change, int64_t capacity, void* stream);
/* host_out[max_iter][ntransforms][2]: row it − 1 holds the change and Σ_i |(∇x)_i|₂ of every component after iteration it (a coupled
 * operator: the joint values); NaN where the iteration did not change the component.  Synchronises `stream`. */
int nufft_tvpd_history(nufft_tvpd* s, double* host_out, int64_t capacity, void* stream);
int64_t nufft_sizeof_tvpd_params(void);
int64_t nufft_sizeof_tvpd_info(void);

/* ---- Dynamic imaging: one Toeplitz multiplier per component ("frames") ----
 * A FRAMED operator holds K = ntransforms real multipliers, one per component: out[c] = Toeplitz(T_c) in[c].  Every component runs
 * exactly the launches of the plain apply with its own multiplier pointer, on the fused and on the dense path, so the result of frame c
 * is bit-equal to that of a plain operator built from T_c; out[c] == in[c] stays allowed without coil maps, and with coil maps the same
 * maps serve every frame.  nufft_toeplitz_num_coupled stays 0: the solvers (CG, FISTA, TV, nufft_toeplitz_max_eigenvalue) treat the
 * frames as independent components.  There is no limit of 16 on K.
 *
 * Storage: K real grids of (2N)^D (each padded to 256 bytes), allocated by the first framed build, counted in workspace_bytes, kept
 * across framed builds and freed by the next nufft_toeplitz_set_points / _set_spectrum, by a coupled build or by
 * nufft_toeplitz_destroy; the operator is then bit for bit the plain (or coupled) operator again.  A framed build drops a coupled one
 * and a coupled build drops a framed one.  nufft_precond_create, nufft_precond_create_block and nufft_precond_update on a framed
 * operator return NUFFT_ERR_UNSUPPORTED (per-frame circulants are not built).
 *
 * Refusals of the two builds, in order: a null object or table NUFFT_ERR_INVALID_ARG; a host-only object NUFFT_ERR_NO_DEVICE; null
 * entries (a spectrum; the coordinates of a frame with points) or a negative num_points[c] NUFFT_ERR_INVALID_ARG; a capturing stream
 * NUFFT_ERR_INVALID_ARG.
 *
 * Added after the total-variation section under the same rule: detect by symbol (dlsym nufft_toeplitz_set_points_frames);
 * NUFFT_MI355X_VERSION and nufft_toeplitz_info are unchanged. */
/* K = ntransforms frames.  num_points[c] >= 0 (0: that frame's multiplier is zero); coords: K·D device vectors, frame c's
 * dimension d at [c·D + d]; weights: NULL, or K entries each NULL (= ones) or real(T)[num_points[c]].  The internal 2N plan is created
 * once, takes every frame's points in turn and is destroyed before the call returns: peak memory as nufft_toeplitz_set_points plus the
 * K real grids. */
int nufft_toeplitz_set_points_frames(nufft_toeplitz* tz, const nufft_params* build_params, const int64_t* num_points,
                                     const void* const* coords, const void* const* weights, void* stream);
/* T[c]: as nufft_toeplitz_set_spectrum, one per frame. */
int nufft_toeplitz_set_spectra_frames(nufft_toeplitz* tz, const void* const* T, void* stream);
/* K while a framed build is in force, else 0. */
int32_t nufft_toeplitz_num_frames(const nufft_toeplitz* tz);
/* The real multiplier of frame c (device, T[2N_1, 2N_2, 2N_3]); NUFFT_ERR_INVALID_ARG without a framed build or for c outside 0 ... K − 1. */
int nufft_toeplitz_multiplier_frame_ptr(const nufft_toeplitz* tz, int32_t c, void** out_ptr, int64_t* out_bytes);

/* ---- Total variation along the components (temporal TV) ----------- */
/* Frames are the components c = 0 ... K − 1, K = ntransforms >= 2, the arrays those of nufft_toeplitz_apply:
 *
 *     (∇_t x)_c[i]  = x_{c+1}[i] − x_c[i]          c < K − 1;     c = K − 1:  x_0[i] − x_{K−1}[i] if periodic, else 0
 *     (∇_tᴴ z)_c[i] = z_{c−1}[i] − z_c[i]          with z_{−1} = z_{K−1} if periodic, else z_{−1} = z_{K−1} = 0
 *     ‖∇_t x‖₁      = Σ_c Σ_i |(∇_t x)_c[i]|       complex modulus
 *
 * The operator alone, on a nufft_tv object: host tables of ntransforms device pointers in and out, 16-byte aligned, no output
 * overlapping an input or another output, `periodic` 0 or 1 (NUFFT_ERR_INVALID_ARG otherwise, and for ntransforms < 2).  One subtraction
 * per value; no atomics; the calls do not synchronise.  nufft_tv_norm_t allocates the object's partial sums in its first call (never on
 * a capturing stream); sums_out_device[c] = Σ_i |(∇_t x)_c[i]|, differences in T, modulus and sum in FP64 in one fixed order. */
int nufft_tv_gradient_t(nufft_tv* tv, void* const* z_out, const void* const* x, int periodic, void* stream);
int nufft_tv_adjoint_t(nufft_tv* tv, void* const* x_out, const void* const* z, int periodic, void* stream);
int nufft_tv_norm_t(nufft_tv* tv, const void* const* x, int periodic, double* sums_out_device, void* stream);

/* The primal-dual solver with a spatial and a temporal term (the usual form of golden-angle radial reconstruction),
 *
 *     ½ <x, (G + μ I) x> − Re<b, x> + Σ_c tv_c Σ_i |(∇x_c)_i|₂ + tv_t ‖∇_t x‖₁
 *
 * on whatever nufft_toeplitz_apply computes (plain, framed, with maps, coupled).  Condat–Vũ as above with one more dual array z_c per
 * component:
 *
 *     q  = G x
 *     x⁺ = x − τ (q + μ x − b + ∇ᴴy + ∇_tᴴz)         x <- x⁺,  q <- x̄ = x⁺ + (x⁺ − x);  partials of ‖x⁺ − x‖², ‖x⁺‖²
 *     y  <- P_{tv_c}(y + σ ∇x̄)                        only when the spatial term is on
 *     z  <- P_{tv_t}(z + σ ∇_t x̄)                     per cell: v · min(1, tv_t / |v|)
 *     decide: always JOINT — one change, one flag, one stopping test, reported identically for every component
 *
 * History column 2 of component c is its share of the prior at x⁺: tv_c Σ_i |(∇x⁺_c)_i|₂ + tv_t Σ_i |(∇_t x⁺)_c[i]| (the first term
 * absent when the spatial term is off); the rows sum to the prior.  Default σ = 1 / (8 n_d τ), n_d = ndim + 1 with the spatial term and
 * 1 without: ‖[∇; ∇_t]‖² <= 4 ndim + 4 and ‖∇_t‖² <= 4 keep 1 / τ − σ ‖·‖² >= 1 / (2 τ) >= L / 2.
 *
 * `spatial` is decided at creation and never switched.  spatial = 0: the solver neither allocates nor touches y — it holds 2 arrays per
 * component (q, z) instead of 2 + ndim, nufft_tvpd_params.tv is ignored and nufft_tvpd_set_tv with a non-zero weight is refused
 * (NUFFT_ERR_INVALID_ARG).  nufft_tvpd_info.array_bytes reports what is held.  solve, get_result, history, get_info and destroy are the
 * calls above; two runs, check_every = 0 and > 0, and a replayed hipGraph give the same bits.
 *
 * Refusals of nufft_tvpd_create_temporal: null arguments, ntransforms < 2, tv_t negative or not finite, spatial or periodic outside
 * {0, 1} NUFFT_ERR_INVALID_ARG; otherwise whatever nufft_tvpd_create refuses, in its order.
 *
 * Added under the same rule: detect by symbol (dlsym nufft_tvpd_create_temporal) and compare nufft_sizeof_tvt_params() with your own;
 * nufft_tvpd_params and nufft_tvpd_info keep their sizes. */
typedef struct nufft_tvt_params {
    int32_t struct_size;     /* sizeof(nufft_tvt_params) of the caller's header (0 = this layout)                                  */
    int32_t periodic;        /* 0: the last frame has no successor (time is not a circle); 1: it is followed by frame 0 (cine)     */
    int32_t spatial;         /* 1: the spatial term of nufft_tvpd_create is kept; 0: temporal term only                            */
    int32_t reserved;        /* 0                                                                                                  */
    double tv_t;             /* >= 0, finite: the weight of ‖∇_t x‖₁                                                               */
} nufft_tvt_params;
int nufft_tvpd_create_temporal(nufft_tvpd** out, nufft_toeplitz* tz, const nufft_tvpd_params* params, const nufft_tvt_params* temporal);
/* The temporal weight of the following solves (finite, >= 0); NUFFT_ERR_INVALID_ARG on a solver made by nufft_tvpd_create. */
int nufft_tvpd_set_tv_t(nufft_tvpd* s, double tv_t);
/* periodic, spatial and tv_t in use; NUFFT_ERR_INVALID_ARG on a solver made by nufft_tvpd_create. */
int nufft_tvpd_get_temporal(const nufft_tvpd* s, nufft_tvt_params* out);
int64_t nufft_sizeof_tvt_params(void);

/* ---- Low-rank plus sparse reconstruction of a series of frames (L+S) ----
 * The K = ntransforms components are frames x_c = L_c + S_c (Otazo, Candès & Sodickson, MRM 2015).  Three objects, each added after
 * ABI 104 without changing NUFFT_MI355X_VERSION: detect by symbol (dlsym nufft_glr_create, nufft_tsparse_create, nufft_lps_create) and
 * compare the nufft_sizeof_* functions below with your own.  1 <= K <= 32 for all three (more: NUFFT_ERR_UNSUPPORTED; the Jacobi team is
 * one wave of at most 32 lanes, and the K x K matrices live in LDS).
 *
 * GLOBAL LOW RANK (nufft_glr_*).  C(x) is the n x K space-time (Casorati) matrix whose column c is frame c, n = Π N_d.  The map is
 * singular-value soft-thresholding of that ONE matrix, by the route of the locally low-rank map above and with its constants:
 *
 *     H = C^H C  (K x K, FP64 for both element types)      H = V Λ V^H  (the same cyclic Jacobi, one team of 2^ceil(log2 K) lanes)
 *     σ_i = sqrt(max(λ_i, 0))     f_i = σ_i > t ? 1 − t / σ_i : 0     P = V diag(f) V^H     C <- C P     nuc = Σ_i f_i σ_i
 *
 * in three launches: the Gram kernel (flat over the cells, one set of K (K + 1) / 2 FP64 partials per workgroup, every entry summed in
 * cell order over fixed segments, the segments in segment order, the workgroup's tiles in tile order), the eigen kernel (one workgroup:
 * adds the partial sets in workgroup order, diagonalises, writes P, nuc and the sweep count to device memory) and the apply kernel
 * (Σ_i C_vi P_ij in FP64, one store).  No atomics: two runs and a replayed hipGraph give the same bits.  The Gram route resolves a
 * direction with σ_i << σ_max only to about (σ_max / σ_i)² ε of FP64 relative to σ_i, as the locally low-rank map does. */
typedef struct nufft_glr nufft_glr; /* opaque */

typedef struct nufft_glr_info {
    int32_t struct_size;     /* sizeof(nufft_glr_info) of the caller's header, set before the call (0 = this layout)               */
    int32_t ndim, dtype, ntransforms, device;
    int32_t tile_cells;      /* cells of one LDS tile (times ntransforms frames)                                                   */
    int32_t jacobi_sweeps_max;
    int32_t reserved;
    int64_t N[3];            /* 1 beyond ndim                                                                                      */
    int64_t cells;           /* n = Π N_d                                                                                          */
    int64_t workgroups;      /* of the Gram and apply kernels = sets of partial sums                                               */
    int64_t workspace_bytes; /* device bytes owned: Gram partials, P, the nuclear norm and the sweep count                         */
} nufft_glr_info;

/* Takes element type, shape, ntransforms and device from the plan; the plan is not kept.  Refusals, in order: null arguments
 * NUFFT_ERR_INVALID_ARG; a real-data plan NUFFT_ERR_UNSUPPORTED; more than 32 transforms NUFFT_ERR_UNSUPPORTED; a host-only plan
 * NUFFT_ERR_NO_DEVICE. */
int nufft_glr_create(nufft_glr** out, const nufft_plan* plan);
/* The same from a Toeplitz operator (the operator is not kept). */
int nufft_glr_create_for_operator(nufft_glr** out, const nufft_toeplitz* tz);
int nufft_glr_destroy(nufft_glr* g);
/* Static facts and sizes; does not synchronise. */
int nufft_glr_get_info(const nufft_glr* g, nufft_glr_info* out);
/* out = prox_{t ‖C(·)‖_*}(in).  Host tables of ntransforms device pointers, 16-byte aligned.  out[c] may be exactly in[c] (a tile is
 * owned by one workgroup, which stores after it has loaded); any other overlap is refused.  nuc_out_device (device, double[1], may be
 * NULL): ‖C(out)‖_* = Σ_i max(σ_i − t, 0).  Allocates nothing, does not synchronise, hipGraph-capture safe; one call at a time per
 * object.  Refusals, before anything is enqueued: a null table or vector, a pointer that is not 16-byte aligned, a partial overlap,
 * t < 0 or not finite NUFFT_ERR_INVALID_ARG. */
int nufft_glr_apply(nufft_glr* g, void* const* out, const void* const* in, double t, double* nuc_out_device, void* stream);
/* The Jacobi sweeps of the last apply (the last one rotates nothing; 0 for K = 1).  Synchronises `stream` (never a capturing one). */
int nufft_glr_last_sweeps(nufft_glr* g, int32_t* sweeps_out, void* stream);
int64_t nufft_sizeof_glr_info(void);

/* TEMPORAL SPARSITY (nufft_tsparse_*).  A unitary transform T along the frames, per cell:
 *
 *     NUFFT_TSPARSE_DFT:       (T x)_k[i] = K^-1/2 Σ_c x_c[i] exp(−2πi k c / K)      (Tᴴ y)_c[i] = K^-1/2 Σ_k y_k[i] exp(+2πi k c / K)
 *     NUFFT_TSPARSE_IDENTITY:  T = I
 *
 * The DFT is the direct sum of K terms for any K in 1 ... 32, accumulated in the element type, with a table of K twiddles (K^-1/2 folded
 * in) computed in FP64 on the host, rounded once to the element type and indexed (k · c) mod K.  A workgroup stages a tile [frame][cell]
 * in LDS.  The shrink is the complex soft threshold c · max(1 − t / |c|, 0), applied where the coefficient is produced; nothing is
 * divided where |c| <= t.  A temporal difference is not offered (it is not unitary: nufft_tvpd_create_temporal covers it). */
typedef struct nufft_tsparse nufft_tsparse; /* opaque */

enum { NUFFT_TSPARSE_IDENTITY = 0, NUFFT_TSPARSE_DFT = 1 };

typedef struct nufft_tsparse_info {
    int32_t struct_size;     /* sizeof(nufft_tsparse_info) of the caller's header, set before the call (0 = this layout)           */
    int32_t ndim, dtype, ntransforms, device;
    int32_t transform;       /* NUFFT_TSPARSE_*                                                                                    */
    int32_t tile_cells;      /* cells of one LDS tile (times ntransforms frames)                                                   */
    int32_t reserved;
    int64_t N[3];            /* 1 beyond ndim                                                                                      */
    int64_t cells;           /* n = Π N_d                                                                                          */
    int64_t workgroups;      /* per launch = rows of partial sums                                                                  */
    int64_t workspace_bytes; /* device bytes owned: the partial sums                                                               */
} nufft_tsparse_info;

/* Refusals, in order: null arguments, an unknown transform NUFFT_ERR_INVALID_ARG; a real-data plan NUFFT_ERR_UNSUPPORTED; more than 32
 * transforms NUFFT_ERR_UNSUPPORTED; a host-only plan NUFFT_ERR_NO_DEVICE. */
int nufft_tsparse_create(nufft_tsparse** out, const nufft_plan* plan, int32_t transform);
int nufft_tsparse_create_for_operator(nufft_tsparse** out, const nufft_toeplitz* tz, int32_t transform);
int nufft_tsparse_destroy(nufft_tsparse* ts);
int nufft_tsparse_get_info(const nufft_tsparse* ts, nufft_tsparse_info* out);
/* out = T in and out = Tᴴ in.  Tables and overlap rules as for nufft_glr_apply (out[c] may be exactly in[c]).  No allocation, no
 * synchronisation, hipGraph-capture safe. */
int nufft_tsparse_forward(nufft_tsparse* ts, void* const* out, const void* const* in, void* stream);
int nufft_tsparse_inverse(nufft_tsparse* ts, void* const* out, const void* const* in, void* stream);
/* coeff_out = soft_t(T in): the coefficients after thresholding, so that nufft_tsparse_inverse of them is prox_{t ‖T·‖₁}(in).
 * l1_out_device (device, double[1], may be NULL): ‖coeff_out‖₁, FP64, one fixed order.  t >= 0 and finite. */
int nufft_tsparse_shrink(nufft_tsparse* ts, void* const* coeff_out, const void* const* in, double t, double* l1_out_device, void* stream);
int64_t nufft_sizeof_tsparse_info(void);

/* THE SOLVER (nufft_lps_*).  Minimises over the pair (L, S)
 *
 *     ½ <L + S, (G + μ I)(L + S)> − Re<b, L + S> + nuc · ‖C(L)‖_* + l1 · ‖T S‖₁
 *
 * G what the nufft_toeplitz object applies (framed, plain, with coil maps, coupled).  Proximal gradient on the pair, with FISTA momentum
 * (β of iteration `it` as in nufft_fista_create; momentum = 0: β = 0, the scheme of Otazo et al.):
 *
 *     start:  L = x0 (or 0),  S = 0,  zL = L,  zS = 0,  u = zL + zS
 *     for it = 1 ... max_iter:
 *         q  = G u                                                  nufft_toeplitz_apply
 *         g  = τ (q + μ u − b);  H = C(zL − g)^H C(zL − g)           Gram kernel: stores g over q
 *         P, ‖C(L⁺)‖_*                                              eigen kernel, t = τ · nuc
 *         L⁺ = (zL − g) P;  zL = L⁺ + β (L⁺ − L);  L = L⁺             apply kernel: partials of ‖L⁺ − L‖², ‖L⁺‖²
 *         S⁺ = Tᴴ soft_{τ·l1}(T (zS − g));  zS likewise;  S = S⁺;  u = zL + zS      temporal kernel: partials of ‖S⁺ − S‖², ‖S⁺‖², ‖T S⁺‖₁
 *         change = sqrt((‖L⁺ − L‖² + ‖S⁺ − S‖²) / (‖L⁺‖² + ‖S⁺‖²)) (0 when both are 0);  history row (change, ‖C(L⁺)‖_*, ‖T S⁺‖₁)
 *         done <- change <= tol, or change not finite (NUFFT_LPS_BREAKDOWN)
 *     x = L + S
 *
 * The smooth term ½ <L + S, (G + μ)(L + S)> has, as a function of the PAIR, the Hessian [[A, A], [A, A]] (A = G + μ I), whose largest
 * eigenvalue is 2 λ_max(A): τ <= 1 / (2 (λ_max(G) + μ)).  The frames are ONE system: one change, one flag, one status, reported
 * identically for every component.  u lives in the caller's x between the iterations.  The solver owns five arrays per frame (L, S,
 * zL, zS, q).  Sums and scalars are FP64, formed without atomics in one fixed order; a done system is frozen (every kernel reads the
 * flag before its first load); check_every as for nufft_fista_create: 0 enqueues everything without synchronising or allocating
 * (hipGraph-capture safe), k > 0 stops early and is refused on a capturing stream; both give the same bits. */
typedef struct nufft_lps nufft_lps; /* opaque */

enum { NUFFT_LPS_MAX_ITER = 0,   /* max_iter iterations ran without reaching tol */
       NUFFT_LPS_CONVERGED = 1,  /* change <= tol                                */
       NUFFT_LPS_BREAKDOWN = 2   /* change not finite: the system was frozen     */ };

typedef struct nufft_lps_params {
    int32_t struct_size;     /* sizeof(nufft_lps_params) of the caller's header (0 = this layout)                                  */
    int32_t max_iter;        /* 1 ... 2^24                                                                                         */
    int32_t check_every;     /* 0, or the number of iterations between two looks at the done flag                                  */
    int32_t transform;       /* NUFFT_TSPARSE_*                                                                                    */
    int32_t momentum;        /* 1: FISTA's β;  0: β = 0                                                                            */
    int32_t reserved;        /* 0                                                                                                  */
    double tol;              /* >= 0, finite                                                                                       */
    double step;             /* τ > 0, finite: 1 / (2 (λ_max + lambda)), nufft_toeplitz_max_eigenvalue                             */
    double lambda;           /* the Tikhonov μ: >= 0, finite                                                                       */
    double nuc;              /* >= 0, finite                                                                                       */
    double l1;               /* >= 0, finite                                                                                       */
} nufft_lps_params;

typedef struct nufft_lps_info {
    int32_t struct_size;     /* sizeof(nufft_lps_info) of the caller's header, set before the call (0 = this layout)               */
    int32_t ntransforms, dtype, max_iter, check_every, transform, momentum;
    int32_t iterations_enqueued; /* by the last nufft_lps_solve (check_every > 0 stops early); -1 before the first                 */
    double tol, step, lambda, nuc, l1;
    int64_t array_bytes;     /* L, S, zL, zS, q: five arrays per frame                                                             */
    int64_t workspace_bytes; /* device bytes owned: array_bytes + partial sums + scalars + history + the two prior objects'        */
} nufft_lps_info;

/* The solver keeps the POINTER `tz`: the operator must outlive it; a new build of the operator between two solves is allowed.
 * Refusals: null arguments, max_iter < 1 or > 2^24, check_every < 0, an unknown transform, momentum outside {0, 1}, tol < 0, lambda < 0,
 * nuc < 0, l1 < 0, step <= 0 or non-finite values NUFFT_ERR_INVALID_ARG; more than 32 transforms NUFFT_ERR_UNSUPPORTED; a host-only
 * operator NUFFT_ERR_NO_DEVICE (after the argument checks). */
int nufft_lps_create(nufft_lps** out, nufft_toeplitz* tz, const nufft_lps_params* params);
int nufft_lps_destroy(nufft_lps* s);
/* The two weights of the following solves (each finite and >= 0). */
int nufft_lps_set_weights(nufft_lps* s, double nuc, double l1);
/* x_inout[c], b[c] as in nufft_fista_solve, with the same refusals.  use_x0 = 0: start from zero.  On return (in stream order)
 * x = L + S. */
int nufft_lps_solve(nufft_lps* s, void* const* x_inout, const void* const* b, int use_x0, void* stream);
/* Copies the two parts of the last solve into the caller's arrays (tables of ntransforms device pointers; either table may be NULL).
 * Enqueues device-to-device copies; does not synchronise.  Refusals: a null entry, two destinations (of either table) that overlap, a
 * destination that overlaps the solver's own arrays NUFFT_ERR_INVALID_ARG. */
int nufft_lps_get_parts(nufft_lps* s, void* const* L_out, void* const* S_out, void* stream);
int nufft_lps_get_info(const nufft_lps* s, nufft_lps_info* out);
/* The outcome of the last solve, the same for every component: iterations that changed the system, NUFFT_LPS_* status, the last
 * change.  Each output may be NULL; `capacity` entries each, at least ntransforms.  Synchronises `stream` (never a capturing one). */
int nufft_lps_get_result(nufft_lps* s, int32_t* iterations, int32_t* status, double* change, int64_t capacity, void* stream);
/* host_out[max_iter][3]: row it − 1 holds the change, ‖C(L⁺)‖_* and ‖T S⁺‖₁ after iteration it; NaN where the iteration did not run.
 * Synchronises `stream`. */
int nufft_lps_history(nufft_lps* s, double* host_out, int64_t capacity, void* stream);
int64_t nufft_sizeof_lps_params(void);
int64_t nufft_sizeof_lps_info(void);

/* ---- Coil sensitivity maps from coil images ----
 * The adaptive estimate of Walsh, Gmitro & Marcellin (MRM 2000): at every cell the dominant eigenvector of the covariance of the coil
 * values over a box around the cell.  Added after ABI 104 without changing NUFFT_MI355X_VERSION: detect by symbol (dlsym
 * nufft_coilmaps_create) and compare nufft_sizeof_coilmaps_params() / nufft_sizeof_coilmaps_info() with your own.
 *
 * Input: C = ncoils complex arrays a_c of the given shape (the low-resolution coil images), 1 <= C <= 32.  Box sides b_d odd,
 * 1 <= b_d <= min(9, N_d).  For every cell x:
 *
 *     R(x)[c, c'] = Σ_{x' ∈ box(x)} a_c(x') conj(a_c'(x'))     the box centred at x and periodic on the array as stored; FP64 for both
 *                                                              element types; summed with k_3 outermost and k_1 innermost
 *     R = V Λ V^H                                              the cyclic Jacobi of the locally low-rank map, with its constants
 *     λ1 = the largest final diagonal entry (the first index on a tie), λ2 = the second largest (0 for C = 1), v = the column of λ1,
 *                                                              scaled back to unit length (the rotations cost it a few ε)
 *     s = Σ_c conj(p_c) v_c;   v <- v conj(s) / |s| if |s| > 0     p = phase_ref (default e_0: coil 0 becomes real and non-negative)
 *     S_c(x) = v_c, rounded once to the element type;  S(x) = 0 exactly where λ1(x) = 0
 *     crop > 0:  S(x) = 0 exactly where λ1(x) < crop² max_x λ1(x)     (formed on the device; both sides are λ1 as stored, that is
 *                                                              rounded to the real element type)
 *
 * so Σ_c |S_c|² = 1 at every cell that is not zeroed.  No atomics, every sum in one fixed order: two runs and a replayed hipGraph give
 * the same bits. */
typedef struct nufft_coilmaps nufft_coilmaps; /* opaque */

typedef struct nufft_coilmaps_params {
    int32_t struct_size;     /* sizeof(nufft_coilmaps_params) of the caller's header (0 = this layout)                             */
    int32_t box[3];          /* box sides, odd; 1 (or 0) beyond ndim                                                               */
    double crop;             /* >= 0, finite; 0: nothing is cropped                                                                */
    int64_t reserved[2];     /* 0                                                                                                  */
} nufft_coilmaps_params;

typedef struct nufft_coilmaps_info {
    int32_t struct_size;     /* sizeof(nufft_coilmaps_info) of the caller's header, set before the call (0 = this layout)          */
    int32_t ndim, dtype, ncoils, device;
    int32_t box[3];
    int32_t tile[3];         /* output cells of one workgroup per dimension                                                        */
    int32_t tile_cells;
    int32_t team_lanes;      /* lanes that diagonalise one cell: the next power of two >= ncoils                                   */
    int32_t teams;           /* teams per workgroup                                                                                */
    int32_t staged;          /* 1: tile plus halo are staged in LDS;  0: the neighbours are read from global memory                */
    int32_t lds_bytes;       /* of one workgroup                                                                                   */
    int32_t jacobi_sweeps_max;
    int32_t reserved;
    double crop;
    int64_t N[3];            /* 1 beyond ndim                                                                                      */
    int64_t cells;           /* n = Π N_d                                                                                          */
    int64_t workgroups;      /* of the main kernel = max partials                                                                  */
    int64_t workspace_bytes; /* device bytes owned: the partials, two words and, with crop > 0, n reals for λ1                     */
} nufft_coilmaps_info;

/* dtype: NUFFT_F32 / NUFFT_F64, the real type of the complex arrays (the arrays are always complex: a binding that starts from a plan
 * refuses a real-data plan itself).  N: ndim sizes, N[0] the fastest.  Refusals, in order: a null argument, a struct_size below the
 * published layout, an unknown dtype, ndim outside 1 ... 3, N_d < 1, ncoils < 1, an even or non-positive box side, a negative or
 * non-finite crop NUFFT_ERR_INVALID_ARG; ncoils > 32, b_d > 9 or b_d > N_d NUFFT_ERR_UNSUPPORTED; device < 0 NUFFT_ERR_NO_DEVICE. */
int nufft_coilmaps_create(nufft_coilmaps** out, int dtype, int ndim, const int64_t* N, int32_t ncoils, int device, const nufft_coilmaps_params* params);
/* Element type, shape and device of a Toeplitz operator (the operator is not kept; its ntransforms plays no part). */
int nufft_coilmaps_create_for_operator(nufft_coilmaps** out, const nufft_toeplitz* tz, int32_t ncoils, const nufft_coilmaps_params* params);
int nufft_coilmaps_destroy(nufft_coilmaps* h);
/* What nufft_coilmaps_create would lay out for these arguments, without a device: the same checks in the same order (the device
 * aside), the same tile, teams and LDS bytes; device = -1 and workspace_bytes = what the object would allocate. */
int nufft_coilmaps_layout(int dtype, int ndim, const int64_t* N, int32_t ncoils, const nufft_coilmaps_params* params, nufft_coilmaps_info* out);
/* Static facts and sizes; does not synchronise. */
int nufft_coilmaps_get_info(const nufft_coilmaps* h, nufft_coilmaps_info* out);
/* maps_out, images_in: host tables of ncoils device pointers, 16-byte aligned.  phase_ref: ncoils complex doubles (re, im) on the HOST,
 * or NULL for e_0; it travels by value in the kernel arguments.  lambda1, lambda2: device arrays of n reals of the element type, or
 * NULL.  λ is about box cells x |a|²: in Float32 it overflows to infinity for |a| above about 1e18 and underflows to 0 for |a| below
 * about 1e-23; the maps do not (R is FP64), but the crop compares the stored values: with an infinite maximum every finite cell is
 * cropped, and a cell whose stored λ1 is 0 is cropped whenever the threshold is positive.  Scale such images first.  With crop > 0 and
 * lambda1 = NULL the object uses an array of its own, allocated at create time.  Allocates nothing, does not
 * synchronise, hipGraph-capture safe; one call at a time per object.  Refusals, before anything is enqueued: a null object or table, a
 * non-finite phase_ref, a null or not 16-byte aligned entry, two outputs (maps and eigenvalue arrays) that overlap, an output that
 * overlaps any input NUFFT_ERR_INVALID_ARG. */
int nufft_coilmaps_estimate(nufft_coilmaps* h, void* const* maps_out, const void* const* images_in, const double* phase_ref, void* lambda1, void* lambda2,
                            void* stream);
/* The crop pass on its own, with another level: maps_inout[c][x] = 0 where lambda1[x] < crop² max λ1, the maximum being that of the LAST
 * nufft_coilmaps_estimate of this object (on the device; nothing is read back).  lambda1: what that call wrote, or NULL for the object's
 * own array (an object created with crop > 0).  Reads lambda1, writes only the cells it zeroes; crop = 0 does nothing.  Capturable.
 * Refusals: a null object or table, a negative or non-finite crop, no lambda1 at all, a null or misaligned entry, maps that overlap each
 * other or lambda1 NUFFT_ERR_INVALID_ARG. */
int nufft_coilmaps_apply_crop(nufft_coilmaps* h, void* const* maps_inout, const void* lambda1, double crop, void* stream);
/* The largest Jacobi sweep count over the cells of the last estimate (the last sweep rotates nothing; 0 for ncoils = 1).
 * Synchronises `stream` (never a capturing one). */
int nufft_coilmaps_last_sweeps(nufft_coilmaps* h, int32_t* sweeps_out, void* stream);
int64_t nufft_sizeof_coilmaps_params(void);
int64_t nufft_sizeof_coilmaps_info(void);

/* ---- Coil compression and noise pre-whitening ----
 * The principal components of the coil covariance (Huang et al., MRI 2008; Buehrer et al., MRM 2007): C = ncoils physical coils become
 * V <= C virtual coils, the first stage of a parallel-imaging reconstruction.  Added after ABI 104 without changing
 * NUFFT_MI355X_VERSION: detect by symbol (dlsym nufft_coilcomp_create) and compare nufft_sizeof_coilcomp_info() with your own.
 *
 * The object knows the element type (complex of NUFFT_F32 / NUFFT_F64), 1 <= C <= 64 and the device.  It needs no plan: every call takes
 * tables of C device vectors of n >= 1 complex elements, each vector 16-byte aligned, and n may differ from call to call (sample
 * vectors, coil images and maps all pass through the same entries).
 *
 *     R[c, c'] = Σ_j h_j y_c[j] conj(y_c'[j])        h: optional real weights (NULL = ones).  Every product and sum is FP64 for both
 *                                                    element types, in one fixed order: within a tile of samples, then the tiles of a
 *                                                    workgroup, then the workgroups; no atomics.  Accumulated over every
 *                                                    nufft_coilcomp_accumulate since the last reset, each call added to R in stream order
 *                                                    (two sets accumulated one after the other give the same bits in every run, not
 *                                                    necessarily those of the concatenated vector)
 *     Ψ = L L^H,  W = L^-1                           on the host, FP64 (nufft_coilcomp_set_noise_covariance; W = I without)
 *     R~ = W R W^H                                   skipped bit-exactly when no noise covariance is set
 *     R~ = U Λ U^H                                   the cyclic Jacobi of the low-rank maps, with its constants; eigenvalues sorted
 *                                                    descending (ties: the lower original index first); every eigenvector scaled back
 *                                                    to unit length, its entry of largest modulus (lowest index on a tie) real and
 *                                                    positive
 *     A = U^H W                                      all C rows; row v is virtual coil v.  A zero Gram matrix gives A = W, λ = 0
 *     out_v[j] = Σ_c A[v, c] in_c[j]                 FP64 in coil order, rounded once to the element type
 *
 * R, A (complex double, row-major), λ (double[C]), the sweep count and a status word stay on the device.  reset, accumulate, finish and
 * apply allocate nothing, never synchronise and are hipGraph-capture safe; two runs and a replayed graph give the same bits.  One call at
 * a time per object. */
typedef struct nufft_coilcomp nufft_coilcomp; /* opaque */

#define NUFFT_COILCOMP_OK 0          /* status of the last finish                                                                   */
#define NUFFT_COILCOMP_SWEEPS 1      /* the Jacobi ran into its sweep cap                                                           */
#define NUFFT_COILCOMP_NONFINITE 2   /* an eigenvalue is not finite (the data were not): A holds U^H W in the Jacobi's own order    */

typedef struct nufft_coilcomp_info {
    int32_t struct_size;     /* sizeof(nufft_coilcomp_info) of the caller's header, set before the call (0 = this layout)          */
    int32_t dtype, ncoils, device;
    int32_t threads;         /* of a workgroup of the Gram kernel                                                                  */
    int32_t tile_samples;    /* samples of one tile in LDS                                                                         */
    int32_t segments;        /* parts of a tile that are summed side by side                                                       */
    int32_t pairs;           /* C (C + 1) / 2 entries of the upper triangle                                                        */
    int32_t pairs_per_thread; /* entries one thread owns, at most 9                                                                */
    int32_t max_workgroups;  /* cap of the Gram kernel's grid = partial sets the object holds                                      */
    int32_t apply_chunk;     /* virtual coils per apply launch; the inputs are read once per chunk                                 */
    int32_t jacobi_team_lanes;
    int32_t jacobi_sweeps_max;
    int32_t lds_bytes_gram, lds_bytes_eigen;   /* of one workgroup                                                                 */
    int32_t matrix_rows;     /* rows of the matrix apply uses: 0 before the first finish / set_matrix                              */
    int32_t has_noise;
    int32_t reserved;
    int64_t n;               /* the vector length these numbers are for                                                            */
    int64_t tiles;           /* ceil(n / tile_samples)                                                                             */
    int64_t tiles_per_workgroup;
    int64_t workgroups;      /* of the Gram kernel for this n                                                                      */
    int64_t workspace_bytes; /* device bytes owned: max_workgroups sets of partials, R, W, W R W^H, U^H and A with 16 spare rows  */
} nufft_coilcomp_info;

/* dtype: the real type of the complex vectors.  Refusals, in order: a null argument, an unknown dtype, ncoils < 1
 * NUFFT_ERR_INVALID_ARG; ncoils > 64 NUFFT_ERR_UNSUPPORTED; device < 0 NUFFT_ERR_NO_DEVICE. */
int nufft_coilcomp_create(nufft_coilcomp** out, int dtype, int32_t ncoils, int device);
int nufft_coilcomp_destroy(nufft_coilcomp* h);
/* What an object of these arguments would do with vectors of n elements, without a device: the same checks in the same order (n < 1
 * NUFFT_ERR_INVALID_ARG before the limit on ncoils), the same tiling and LDS bytes; device = -1. */
int nufft_coilcomp_layout(int dtype, int32_t ncoils, int64_t n, nufft_coilcomp_info* out);
/* Static facts, and the tiling of an accumulate of n elements; does not synchronise. */
int nufft_coilcomp_get_info(const nufft_coilcomp* h, int64_t n, nufft_coilcomp_info* out);
/* w_out = L^-1 of psi = L L^H, both ncoils x ncoils complex doubles (re, im), row-major, on the HOST; no device is touched.  Refusals,
 * in order: a null argument, ncoils < 1 NUFFT_ERR_INVALID_ARG; ncoils > 64 NUFFT_ERR_UNSUPPORTED; an entry that is not finite, a
 * matrix that is not Hermitian to 1e-12 max |psi|, a pivot that is not positive NUFFT_ERR_INVALID_ARG. */
int nufft_coilcomp_whitening_matrix(int32_t ncoils, const double* psi, double* w_out);
/* psi as above, or NULL to return to W = I.  Factors on the host (the refusals of nufft_coilcomp_whitening_matrix, before the device
 * is touched) and uploads W: set-up, synchronises `stream` (never a capturing one).  Takes effect at the next finish. */
int nufft_coilcomp_set_noise_covariance(nufft_coilcomp* h, const double* psi, void* stream);
/* R = 0 (a memset node). */
int nufft_coilcomp_reset(nufft_coilcomp* h, void* stream);
/* R += the weighted Gram matrix of y[0 .. ncoils): a host table of device pointers.  weights: n reals of the element type on the
 * device, or NULL.  The weights are NOT checked on the device: a negative weight is subtracted, a non-finite one spoils R.  A weight
 * of exactly zero contributes exactly nothing.  Refusals: a null object or table, n < 1, a null or not 16-byte aligned vector,
 * misaligned weights NUFFT_ERR_INVALID_ARG. */
int nufft_coilcomp_accumulate(nufft_coilcomp* h, const void* const* y, const void* weights, int64_t n, void* stream);
/* Whitening (when set), eigen-decomposition, A = U^H W: one launch of one workgroup without a noise covariance, three with. */
int nufft_coilcomp_finish(nufft_coilcomp* h, void* stream);
/* Installs rows x ncoils complex doubles from the HOST as the matrix of apply (for example one fitted on another scan), 1 <= rows <=
 * ncoils; λ, the sweep count and the status keep what the last finish left.  Synchronises `stream` (never a capturing one).
 * Refusals: a null argument, rows out of range, an entry that is not finite NUFFT_ERR_INVALID_ARG. */
int nufft_coilcomp_set_matrix(nufft_coilcomp* h, const double* A_host, int32_t rows, void* stream);
/* out[0 .. nvirtual), in[0 .. ncoils): host tables of device pointers to vectors of n elements, 1 <= nvirtual <= the rows of the
 * matrix.  The inputs are only read, once per 16 virtual coils.  Refusals, before anything is enqueued: a null object or table, no
 * finish or set_matrix yet, nvirtual out of range, n < 1, a null or not 16-byte aligned vector, an output that overlaps an input or
 * another output NUFFT_ERR_INVALID_ARG. */
int nufft_coilcomp_apply(nufft_coilcomp* h, void* const* out, int32_t nvirtual, const void* const* in, int64_t n, void* stream);
/* Copies to the host: R and A as ncoils x ncoils complex doubles (rows of A behind those of a set_matrix are zero); λ as ncoils doubles
 * with the sweep count and the NUFFT_COILCOMP_* status of the last finish (each output may be NULL).  They synchronise `stream` (never
 * a capturing one); get_matrix is refused before the first finish / set_matrix. */
int nufft_coilcomp_get_gram(nufft_coilcomp* h, double* host_out, void* stream);
int nufft_coilcomp_get_matrix(nufft_coilcomp* h, double* host_out, void* stream);
int nufft_coilcomp_get_spectrum(nufft_coilcomp* h, double* lambda_out, int32_t* sweeps_out, int32_t* status_out, void* stream);
int64_t nufft_sizeof_coilcomp_info(void);

/* ---- Off-resonance correction by time segmentation: the segmented Toeplitz operator ----
 * With a field map ω(x) the signal model is y_j = Σ_x exp(−i ω(x) t_j) a_j(x) S_c(x) u(x), a_j(x) the plan's type-2 kernel.  Time
 * segmentation writes exp(−i ω t) ≈ Σ_l φ_l(t) exp(−i ω τ_l), l = 0 ... L − 1, so with the factors B_l(x) = exp(−i ω(x) τ_l)
 *
 *     y ≈ Σ_l φ_l ⊙ A (B_l ⊙ S_c ⊙ u)
 *     G_ω u = Σ_c conj(S_c) ⊙ Σ_a conj(B_a) ⊙ Σ_b Toeplitz(T_ab) (B_b ⊙ S_c ⊙ u),     T_ab from  w conj(φ_a) φ_b
 *
 * The inner L × L block is the block multiplier of a coupled operator; outside, the operator has ONE component.  A SEGMENTED operator
 * is that: nufft_toeplitz_info.ntransforms is 1 for life, so the solvers (CG, FISTA, TV, nufft_toeplitz_max_eigenvalue), the wavelet
 * transform, the total variation and everything else created for it see one image; nufft_toeplitz_num_coupled and
 * nufft_toeplitz_num_frames return 0 and nufft_toeplitz_num_segments returns L.
 *
 * Builds: nufft_toeplitz_set_points_coupled (basis = the L rows φ_l) and nufft_toeplitz_set_spectra_coupled (the L (L + 1) / 2 pair
 * spectra) with K = L, and nufft_toeplitz_multiplier_pair_ptr, work as on a coupled operator.  nufft_toeplitz_set_points,
 * _set_spectrum, _set_points_frames, _set_spectra_frames and nufft_toeplitz_multiplier_ptr return NUFFT_ERR_UNSUPPORTED.
 *
 * Factors: L complex arrays shaped like û, 16-byte aligned, BORROWED like coil maps (they must stay alive and unchanged while set);
 * any values, not only unit-modulus exponentials.  Builds, factors and coil maps are independent and may come in any order.
 * has_spectrum is 1 only while a build and the factors are both in force; nufft_toeplitz_apply before that returns
 * NUFFT_ERR_NO_POINTS.
 *
 * nufft_toeplitz_apply, all with the kernels of the coupled apply, on the fused and on the dense path:
 *   without coil maps   for b = 0 ... L − 1 the backward half of û into intermediate b with B_b where the coil's map would multiply;
 *                       the block multiply; for a = 0 ... L − 1 the forward half into out with conj(B_a), a = 0 storing, a > 0 adding.
 *   with coil maps      per coil c in index order: v = S_c ⊙ û; the sequence above from v into w; out (+)= conj(S_c) ⊙ w.  v and w are
 *                       two N^D scratch arrays, allocated when maps and factors are both set (never on a capturing stream), counted in
 *                       workspace_bytes and freed when either is cleared.  NUFFT_TOEPLITZ_MAPS_INPASS plays no part.
 * out == in is refused (NUFFT_ERR_INVALID_ARG).  The order is fixed and there are no atomics: two runs and a replayed graph give the
 * same bits; the apply allocates nothing and never synchronises.  Storage: that of a coupled operator of L components.
 * nufft_precond_create, _create_block and _update on a segmented operator return NUFFT_ERR_UNSUPPORTED.
 *
 * Added after ABI 104 without changing NUFFT_MI355X_VERSION or nufft_toeplitz_info: detect by symbol (dlsym
 * nufft_toeplitz_create_segmented). */
/* As nufft_toeplitz_create, with its refusals first; then: a plan with ntransforms != 1, nsegments < 1 NUFFT_ERR_INVALID_ARG;
 * nsegments > 16 NUFFT_ERR_UNSUPPORTED; on the fused path, L lines of 2 N_1 cells that do not fit the coupled dimension-1 kernel
 * NUFFT_ERR_UNSUPPORTED (the message names the plan option NUFFT_TOEPLITZ_FUSED=0). */
int nufft_toeplitz_create_segmented(nufft_toeplitz** out, const nufft_plan* plan, int32_t nsegments);
/* L of a segmented operator, 0 of any other. */
int32_t nufft_toeplitz_num_segments(const nufft_toeplitz* tz);
/* B[0 .. L): host table of device pointers.  Refusals: a null object or table, an operator that is not segmented
 * NUFFT_ERR_INVALID_ARG; a host-only object NUFFT_ERR_NO_DEVICE; a null or not 16-byte aligned factor NUFFT_ERR_INVALID_ARG; with coil
 * maps set and the scratch arrays not yet held, a capturing stream NUFFT_ERR_INVALID_ARG. */
int nufft_toeplitz_set_factors(nufft_toeplitz* tz, const void* const* B, void* stream);
/* Forgets the factors (has_spectrum returns to 0) and frees the two scratch arrays. */
int nufft_toeplitz_clear_factors(nufft_toeplitz* tz);

/* ---- The segment fit of a field map ----
 * The histogram least-squares fit of Sutton, Noll & Fessler (IEEE TMI 2003): the interpolators φ_l(t) minimise
 * Σ_b h_b |exp(−i ω_b t) − Σ_l φ_l(t) exp(−i ω_b τ_l)|² over the histogram (h_b, ω_b) of the field map.  Like coil compression the
 * object needs no plan: it knows the element type, 1 <= L <= 16, 1 <= nbins <= 1024 and the device.
 *
 *     range       FP64 minimum and maximum of ω over the mask, and the count of values that are not finite
 *     histogram   bin = min(nbins − 1, (int)((ω − ωmin) · scale)) in FP64, scale = nbins / (ωmax − ωmin) from the host; uint32 counts by
 *                 integer atomics: exact and the same in every run.  ωmax == ωmin: one bin, at that value
 *     centres     ω_b = ωmin + (b + 1/2) (ωmax − ωmin) / nbins
 *     Gm[l, l']   = Σ_b h_b exp(−i ω_b (τ_l' − τ_l))                               host, FP64
 *     P           = (Gm + ridge · (tr Gm / L) · I)^-1 by Cholesky                   host, FP64
 *     φ(t_j)      = P r,  r_l = Σ_b h_b exp(−i ω_b (t_j − τ_l))                     device, FP64, rounded once to the element type
 *     B_l(x)      = exp(−i ω(x) τ_l)                                               device, FP64, rounded once
 *
 * interpolators and factors allocate nothing, never synchronise and are hipGraph-capture safe; two runs give the same bits.  fit and
 * the read-backs synchronise `stream` and are refused on a capturing one.  One call at a time per object.  Added after ABI 104 without
 * changing NUFFT_MI355X_VERSION: detect by symbol (dlsym nufft_fieldseg_create) and compare nufft_sizeof_fieldseg_info() with your own. */
typedef struct nufft_fieldseg nufft_fieldseg; /* opaque */

typedef struct nufft_fieldseg_info {
    int32_t struct_size;     /* sizeof(nufft_fieldseg_info) of the caller's header, set before the call (0 = this layout)           */
    int32_t dtype, nsegments, nbins, device;
    int32_t threads;         /* of a workgroup of every kernel; the interpolator kernel runs one sample per thread                 */
    int32_t segment_tier;    /* accumulators of the interpolator kernel's instantiation: 1, 2, 4, 8 or 16                          */
    int32_t reseed_bins;     /* bins between two exact sincos of the recurrence = bins of one staged piece of the table            */
    int32_t max_workgroups;  /* of the range kernel = rows of partials the object holds                                            */
    int32_t lds_bytes_interpolators, lds_bytes_histogram;   /* of one workgroup                                                   */
    int32_t bins_used;       /* 0 before the first fit, 1 for a constant field map, else nbins                                     */
    int64_t workspace_bytes; /* device bytes owned: partials, counts, centres, the table h_b exp(i ω_b τ_l), Gm and P             */
} nufft_fieldseg_info;

/* dtype: the real type of ω, of the times and of the complex outputs.  Refusals, in order: a null argument, an unknown dtype,
 * nsegments < 1, nbins outside 1 ... 1024 NUFFT_ERR_INVALID_ARG; nsegments > 16 NUFFT_ERR_UNSUPPORTED; device < 0 NUFFT_ERR_NO_DEVICE. */
int nufft_fieldseg_create(nufft_fieldseg** out, int dtype, int32_t nsegments, int32_t nbins, int device);
int nufft_fieldseg_destroy(nufft_fieldseg* h);
/* What an object of these arguments would launch, without a device: the same checks in the same order; device = -1. */
int nufft_fieldseg_layout(int dtype, int32_t nsegments, int32_t nbins, nufft_fieldseg_info* out);
/* Does not synchronise. */
int nufft_fieldseg_get_info(const nufft_fieldseg* h, nufft_fieldseg_info* out);
/* omega: real(T)[n] on the device; mask: NULL or uint8[n] on the device, nonzero = counted; tau: nsegments doubles on the HOST,
 * strictly increasing; ridge >= 0.  Refusals, in order: a null object, omega or tau, n < 1, misaligned omega, tau not finite or not
 * strictly increasing, ridge negative or not finite, a capturing stream, an empty mask, a counted value that is not finite, a range
 * whose scale is not finite, a pivot of the Cholesky factor that is not positive (the message names ridge): all
 * NUFFT_ERR_INVALID_ARG.  After a refused fit the object is unfitted. */
int nufft_fieldseg_fit(nufft_fieldseg* h, const void* omega, const uint8_t* mask, int64_t n, const double* tau, double ridge, void* stream);
/* times: real(T)[num_points] on the device; phi_rows[0 .. nsegments): host table of device pointers to complex(T)[num_points], 16-byte
 * aligned: row l receives φ_l(t_j).  Refusals: a null argument, no fit yet, num_points < 1, misaligned times, a null or misaligned row
 * NUFFT_ERR_INVALID_ARG. */
int nufft_fieldseg_interpolators(nufft_fieldseg* h, const void* times, int64_t num_points, void* const* phi_rows, void* stream);
/* B[0 .. nsegments): host table of device pointers to complex(T)[n], 16-byte aligned: B[l][x] = exp(−i omega[x] τ_l) with the τ of the
 * last fit; nufft_toeplitz_set_factors takes the same table.  Refusals as above. */
int nufft_fieldseg_factors(nufft_fieldseg* h, const void* omega, int64_t n, void* const* B, void* stream);
/* Copies to the host (each output may be NULL): bins_used counts and centres; Gm and P as nsegments x nsegments complex doubles
 * (re, im), row-major; tau as nsegments doubles.  Refused before the first fit and on a capturing stream. */
int nufft_fieldseg_get_histogram(nufft_fieldseg* h, uint32_t* counts_out, double* centres_out, void* stream);
int nufft_fieldseg_get_gram(nufft_fieldseg* h, double* host_out, void* stream);
int nufft_fieldseg_get_solver_matrix(nufft_fieldseg* h, double* host_out, void* stream);
int nufft_fieldseg_get_tau(nufft_fieldseg* h, double* host_out, void* stream);
int64_t nufft_sizeof_fieldseg_info(void);

/* ---- Second-order total generalized variation, TGV² -------------- */
/* Total variation turns smooth ramps into stairs; TGV² (Bredies, Kunisch & Pock 2010; Knoll, Bredies, Pock & Stollberger 2011 for
 * undersampled radial MRI) lets a vector field v take up the slope.  Per component (coupled components: jointly), with x an image and
 * v = (v_1 ... v_D) a complex vector field of the same shape,
 *
 *     minimise over x, v:   ½ <x, (G + μ I) x> − Re<b, x> + α1 Σ_i |(∇x − v)_i|₂ + α0 Σ_i |(E v)_i|_F
 *
 * ∇ is the periodic forward difference of the total-variation section.  E is the symmetrised gradient built from periodic BACKWARD
 * differences (∂⁻_e u)[i] = u[i] − u[i − e_e] on the array as stored:
 *
 *     (E v)_de[i]  = ½ ((∂⁻_e v_d)[i] + (∂⁻_d v_e)[i])         two subtractions, one addition, one multiply by ½, in this order:
 *                                                              the diagonal entry is ∂⁻_d v_d exactly
 *     |W|_F        = sqrt(Σ_d |W_dd|² + 2 Σ_{d<e} |W_de|²)     the inner product on such tensors carries the same weights 1 / 2
 *     (Eᴴ r)_d[i]  = Σ_e (r_de[i] − r_de[i + e_e])             r_ed = r_de, summed in the order e = 1 ... D
 *
 * A symmetric tensor is S = D (D + 1) / 2 arrays in row-major upper-triangle order, (1,1), (1,2), (1,3), (2,2), (2,3), (3,3) for D = 3
 * (the order of the coupled operator's pair index); a table of them holds ntransforms · S pointers, component c's entry s at
 * [c · S + s]; a table of fields holds ntransforms · D pointers as in nufft_tv_gradient.  Both operators commute with every cyclic
 * shift.
 *
 * The operator alone, on a nufft_tv object; rules and refusals as nufft_tv_gradient / _adjoint / _norm (null or misaligned pointers, an
 * output overlapping an input or another output NUFFT_ERR_INVALID_ARG); no atomics, no synchronisation, hipGraph-capture safe.
 * nufft_tv_sym_norm: sums_out_device[c] = Σ_i |(E v[c])_i|_F, the entries formed in T, squares, root and sum in FP64 in one fixed
 * order. */
int nufft_tv_sym_gradient(nufft_tv* tv, void* const* r_out, const void* const* v, void* stream);
int nufft_tv_sym_adjoint(nufft_tv* tv, void* const* v_out, const void* const* r, void* stream);
int nufft_tv_sym_norm(nufft_tv* tv, const void* const* v, double* sums_out_device, void* stream);

/* The solver: Condat–Vũ on K(x, v) = (∇x − v, E v), Kᴴ(p, r) = (∇ᴴp, −p + Eᴴr), fixed steps τ and σ, duals p (D arrays) and r (S arrays):
 *
 *     start:  x = x0 (or 0),  v = 0,  p = 0,  r = 0
 *     for it = 1 ... max_iter:
 *         q  = G x                                        nufft_toeplitz_apply
 *         x⁺ = x − τ (q + μ x − b + ∇ᴴ p)                 x̄ = x⁺ + (x⁺ − x)          the primal kernel of the TV solver, p for y
 *         v⁺ = v − τ (−p + Eᴴ r)                          v̄ = v⁺ + (v⁺ − v)
 *         p  <- P_α1(p + σ (∇x̄ − v̄))                      P_t(u)_i = u_i · min(1, t / |u_i|₂) over the D entries of a cell
 *         r  <- P_α0(r + σ E v̄)                           the same with |·|_F over the S entries of a cell
 *         change = ‖x⁺ − x‖ / ‖x⁺‖ (0 when both are 0);  history row (change, Σ_i |(∇x⁺ − v⁺)_i|₂, Σ_i |(E v⁺)_i|_F)
 *         done <- change <= tol, or change not finite (NUFFT_TGV_BREAKDOWN)
 *
 * ‖K‖² <= 8 D (‖∇x − v‖² + ‖Ev‖² <= 2 ‖∇x‖² + (2 + 4 D) ‖v‖², ‖∇‖², ‖E‖² <= 4 D), so with τ <= 1 / L and the default σ = 1 / (16 D τ)
 * 1 / τ − σ ‖K‖² >= 1 / (2 τ) >= L / 2, the convergence condition.  Any finite σ > 0 is accepted.  α1 = 0 leaves p exactly zero (x then
 * runs plain gradient descent), α0 = 0 leaves r exactly zero.  The stopping rule is on x alone.  v, p and r restart at 0 in every solve.
 *
 * No launch reads at a neighbour an array it writes.  The solver owns 1 + 3 D + S arrays per component (q, v, v̄, p, r).  Frozen
 * components, coupled operators (one system: one change, one flag), FP64 sums without atomics in one fixed order, check_every and
 * hipGraph capture are as in the TV solver above: two runs, both modes and a replayed graph give the same bits.
 *
 * Added after ABI 104 without changing NUFFT_MI355X_VERSION: detect by symbol (dlsym nufft_tgv_create) and compare
 * nufft_sizeof_tgv_params() / nufft_sizeof_tgv_info() with your own. */
typedef struct nufft_tgv nufft_tgv; /* opaque */

enum { NUFFT_TGV_MAX_ITER = 0,   /* max_iter iterations ran without reaching tol */
       NUFFT_TGV_CONVERGED = 1,  /* change <= tol                                */
       NUFFT_TGV_BREAKDOWN = 2   /* change not finite: the component was frozen  */ };

typedef struct nufft_tgv_params {
    int32_t struct_size;     /* sizeof(nufft_tgv_params) of the caller's header (0 = this layout)                                  */
    int32_t max_iter;        /* 1 ... 2^24                                                                                         */
    int32_t check_every;     /* 0, or the number of iterations between two looks at the done flags                                 */
    int32_t reserved;        /* 0                                                                                                  */
    double tol;              /* >= 0, finite                                                                                       */
    double step;             /* τ > 0, finite                                                                                      */
    double sigma;            /* σ > 0, finite; 0 = 1 / (16 ndim τ)                                                                 */
    double lambda;           /* the Tikhonov μ: >= 0, finite                                                                       */
    double alpha1, alpha0;   /* >= 0, finite: the weights of every component until nufft_tgv_set_weights                           */
} nufft_tgv_params;

typedef struct nufft_tgv_info {
    int32_t struct_size;     /* sizeof(nufft_tgv_info) of the caller's header, set before the call (0 = this layout)               */
    int32_t ntransforms, dtype, ndim, max_iter, check_every;
    int32_t iterations_enqueued; /* by the last nufft_tgv_solve (check_every > 0 stops early); -1 before the first                 */
    int32_t reserved;
    double tol, step, sigma, lambda;   /* sigma: the value in use                                                                  */
    int64_t array_bytes;     /* q, v, v̄, p, r: 1 + 3 ndim + ndim (ndim + 1) / 2 arrays per component                               */
    int64_t workspace_bytes; /* device bytes owned: array_bytes + partial sums + scalars + history                                 */
} nufft_tgv_info;

/* The solver keeps the POINTER `tz`, as nufft_tvpd_create.  Refusals, in the order and with the codes of nufft_tvpd_create: null
 * arguments, max_iter < 1 or > 2^24, check_every < 0, tol, alpha1, alpha0, lambda or sigma negative or not finite, step <= 0 or not
 * finite NUFFT_ERR_INVALID_ARG; whatever nufft_tv_create refuses for the shape; a host-only operator NUFFT_ERR_NO_DEVICE (after the
 * argument checks). */
int nufft_tgv_create(nufft_tgv** out, nufft_toeplitz* tz, const nufft_tgv_params* params);
int nufft_tgv_destroy(nufft_tgv* s);
/* One pair of weights per component (host arrays, count = ntransforms, each finite and >= 0) for the following solves. */
int nufft_tgv_set_weights(nufft_tgv* s, const double* alpha1, const double* alpha0, int64_t count);
/* As nufft_tvpd_solve, with the same refusals. */
int nufft_tgv_solve(nufft_tgv* s, void* const* x_inout, const void* const* b, int use_x0, void* stream);
int nufft_tgv_get_info(const nufft_tgv* s, nufft_tgv_info* out);
/* As nufft_tvpd_get_result (status: NUFFT_TGV_*). */
int nufft_tgv_get_result(nufft_tgv* s, int32_t* iterations, int32_t* status, double* change, int64_t capacity, void* stream);
/* host_out[max_iter][ntransforms][3]: change, Σ_i |(∇x − v)_i|₂ and Σ_i |(E v)_i|_F after every iteration; NaN where the iteration did
 * not change the component.  Synchronises `stream`. */
int nufft_tgv_history(nufft_tgv* s, double* host_out, int64_t capacity, void* stream);
/* v of the last solve into ntransforms · D caller arrays (16-byte aligned, v_d of component c at [c · D + d − 1]): device-to-device
 * copies on `stream`; does not synchronise; hipGraph-capture safe. */
int nufft_tgv_copy_field(nufft_tgv* s, void* const* v_out, void* stream);
int64_t nufft_sizeof_tgv_params(void);
int64_t nufft_sizeof_tgv_info(void);

/* ---- misc----------------------------------------------------------------------------- */
/* sizeof(nufft_params) / sizeof(nufft_info) of the library build: a binding that mirrors the structs by hand
 * (ctypes, Julia) compares them with its own layout before the first call. */
/* Plan-owned device memory right now, buffer by buffer: "name=bytes;name=bytes;..." (NUL-terminated) into `out`; the values sum to
 * nufft_info.workspace_bytes.  Names: us, uhat, tmp2 (oversampled grids / spectra / intermediate of the pruned FFT passes), sorted
 * (bin-sorted point records), sort_scratch, sort_slice_table, bin_counts, bin_offsets, vsorted (values in sorted order: MFMA-patch
 * plans), ring_side_buffer (halo variant of the spreading window), rocfft_work, tables (everything small).  The reference's plan holds
 * us + ûs (src/plan.jl:37-60) and blockidx + pointperm + offsets (src/blocking/gpu.jl:41-69) and aliases the caller's points. */
int nufft_workspace_breakdown(const nufft_plan* plan, char* out, int64_t capacity);
/* The development switches the plan was created with (nufft_params.options), canonical form "NAME=value;..." sorted by name; "" if none.
 * The pointer stays valid until the plan is destroyed. */
const char* nufft_plan_options(const nufft_plan* plan);
int64_t nufft_sizeof_params(void);
int64_t nufft_sizeof_info(void);
const char* nufft_strerror(int code);
/* Last error message of the calling thread (more detail than nufft_strerror). */
const char* nufft_last_error_message(void);
int nufft_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NUFFT_MI355X_H */
