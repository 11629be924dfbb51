// T. Chan's optimal circulant preconditioner of a Toeplitz normal operator (include/nufft_mi355x.h, Preconditioner section; DESIGN.md
// section 21).
//
// Build: the operator's real multiplier K on the 2N grid is transformed forward (rocFFT), which returns its generating sequence T;
// pc_fold_kernel folds T with Fejér weights into the first column c of the circulant on the N grid; one more forward transform of size N
// gives the eigenvalues e = Re DFT_N(c); pc_invert_kernel leaves m = 1 / (n max(e + μ, floor max(e + μ))).
//
// Apply, per component: M⁻¹ r = d ⊙ F⁻¹(m ⊙ F(d ⊙ r)).  The fused path runs it as F(m~ ⊙ B(·)) with m~ the index-negated m (the same
// operator): backward strided passes of fft_lines.hip along dimensions 3 and 2 (unpruned: all N modes kept, identity map, unit
// factors; d rides on the first load), precond_lines_kernel along dimension 1, forward strided passes along 2 and 3 (d on the last
// store).  The dense path runs rocFFT on one scratch array.
//
// Block object (nufft_precond_create_block): the same build per stored pair of a coupled operator's multipliers
// gives the K (K + 1) / 2 grids E_ab, pc_block_invert_kernel turns them into B = (E + shift I)⁻¹ / n in place, and the apply runs the
// passes above per component around ONE kernel that applies the K × K block of every cell (precond_block_kernels.hip).
#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "kernels.h"
#include "precond.h"
#include "solver_common.h"
#include "toeplitz.h"

using namespace nufft;

struct nufft_precond {
    nufft_toeplitz* tz = nullptr;
    int dtype = NUFFT_F64, D = 1, C = 1, device = -1, num_cus = 256;
    int64_t N[3] = {1, 1, 1};
    int64_t n = 1;                         // modes per component
    int path = NUFFT_PRECOND_PATH_DENSE;
    double lambda = 0.0, mu = 0.0, floor = 1e-6, max_e = 0.0, min_e = 0.0;
    void* d_m = nullptr;                   // T[N_1, N_2, N_3] (scalar object)
    void* d_scratch = nullptr;             // complex<T>[N_1, N_2, N_3]: shared by all components; block object: K of them, sstride apart
    // block object
    int K = 0;                             // coupled components (0: the scalar object)
    int64_t pitch = 0;                     // cells between two grids of B: n rounded up to whole 16-byte packs of reals
    int64_t sstride = 0;                   // complex elements between two scratch arrays
    void* d_bd = nullptr;                  // T[K][pitch]: B_aa
    void* d_bc = nullptr;                  // complex<T>[K (K − 1) / 2][pitch]: B_ab, a < b, row-major
    double* d_cnt = nullptr;               // double[Gc]: partial counts of floored cells
    int Gc = 1;
    int64_t floored = 0;
    void* d_own_d = nullptr;               // T[N...]: the scaling from coil maps
    const void* d_scaling = nullptr;       // in force: d_own_d, a caller's array, or null
    int scaling = NUFFT_PRECOND_SCALING_NONE;
    double* d_part = nullptr;              // double[G][2]: partial maxima / sums of the build
    int G = 1;
    // fused
    void* d_tw_fw[3] = {nullptr, nullptr, nullptr};    // complex<T>[N_d]: exp(-2πi k / N_d)
    void* d_tw_bw[3] = {nullptr, nullptr, nullptr};    // (dimensions 2, 3)
    void* d_ones = nullptr;                            // T[max N_d] = 1
    int32_t* d_iota = nullptr;                         // int32[max N_d]: the identity map of an unpruned pass
    // rocFFT: size N, in place
    rocfft_plan_t* fft_fw = nullptr;
    rocfft_plan_t* fft_bw = nullptr;                   // dense only
    rocfft_execution_info_t* fft_info = nullptr;
    void* d_fft_work = nullptr;                        // dense: kept; fused: lives inside the build
    size_t fft_work_bytes = 0;
    int64_t own_bytes = 0;
};

namespace {

int alloc(nufft_precond* p, void** ptr, size_t bytes) { return alloc_buffer(p->own_bytes, "preconditioner", ptr, bytes); }

void release(nufft_precond* p) {
    if (!p) return;
    if (p->device >= 0) {
        DeviceGuard g(p->device);
        for (int d = 0; d < 3; ++d) {
            if (p->d_tw_fw[d]) (void)hipFree(p->d_tw_fw[d]);
            if (p->d_tw_bw[d]) (void)hipFree(p->d_tw_bw[d]);
        }
        for (void* q : {p->d_m, p->d_scratch, p->d_own_d, static_cast<void*>(p->d_part), p->d_ones, static_cast<void*>(p->d_iota), p->d_fft_work, p->d_bd,
                        p->d_bc, static_cast<void*>(p->d_cnt)})
            if (q) (void)hipFree(q);
        if (p->fft_fw) (void)rocfft_plan_destroy(p->fft_fw);
        if (p->fft_bw) (void)rocfft_plan_destroy(p->fft_bw);
        if (p->fft_info) (void)rocfft_execution_info_destroy(p->fft_info);
    }
    delete p;
}

int upload_reals(nufft_precond* p, void** dst, const std::vector<double>& src) {
    const size_t rb = real_bytes(p->dtype);
    int rc = alloc(p, dst, src.size() * rb);
    if (rc) return rc;
    if (p->dtype == NUFFT_F32) {
        std::vector<float> tmp(src.begin(), src.end());
        NUFFT_HIP(hipMemcpy(*dst, tmp.data(), tmp.size() * rb, hipMemcpyHostToDevice));
    } else {
        NUFFT_HIP(hipMemcpy(*dst, src.data(), src.size() * rb, hipMemcpyHostToDevice));
    }
    return NUFFT_OK;
}

int build_device(nufft_precond* p) {
    const size_t rb = real_bytes(p->dtype), cb = 2 * rb;
    const bool fused = p->path == NUFFT_PRECOND_PATH_FUSED;
    int rc;
    p->G = pc_workgroups(p->n, p->num_cus);
    if (p->K > 0) {
        const size_t K = (size_t)p->K;
        p->pitch = (p->n + 3) / 4 * 4;
        p->sstride = (p->n + 1) / 2 * 2;
        p->Gc = pc_block_invert_workgroups(p->n, p->K, p->num_cus);
        if ((rc = alloc(p, &p->d_bd, K * (size_t)p->pitch * rb)) || (rc = alloc(p, &p->d_scratch, K * (size_t)p->sstride * cb)) ||
            (rc = alloc(p, reinterpret_cast<void**>(&p->d_cnt), (size_t)p->Gc * sizeof(double))))
            return rc;
        if (K > 1 && (rc = alloc(p, &p->d_bc, K * (K - 1) / 2 * (size_t)p->pitch * cb))) return rc;
    } else if ((rc = alloc(p, &p->d_m, (size_t)p->n * rb)) || (rc = alloc(p, &p->d_scratch, (size_t)p->n * cb))) {
        return rc;
    }
    if ((rc = alloc(p, reinterpret_cast<void**>(&p->d_part), (size_t)std::max(p->K, 1) * p->G * 2 * sizeof(double)))) return rc;
    if (fused) {
        int64_t nmax = 1;
        for (int d = 0; d < p->D; ++d) {
            const int64_t n = p->N[d];
            nmax = std::max(nmax, n);
            std::vector<double> twf(2 * (size_t)n), twb(2 * (size_t)n);
            for (int64_t k = 0; k < n; ++k) {
                const double ang = 2.0 * M_PI * (double)k / (double)n;
                twf[2 * k] = std::cos(ang); twf[2 * k + 1] = -std::sin(ang);
                twb[2 * k] = std::cos(ang); twb[2 * k + 1] = std::sin(ang);
            }
            if ((rc = upload_reals(p, &p->d_tw_fw[d], twf))) return rc;
            if (d > 0 && (rc = upload_reals(p, &p->d_tw_bw[d], twb))) return rc;
        }
        if ((rc = upload_reals(p, &p->d_ones, std::vector<double>((size_t)nmax, 1.0)))) return rc;
        std::vector<int32_t> iota((size_t)nmax);
        for (int64_t k = 0; k < nmax; ++k) iota[(size_t)k] = (int32_t)k;
        if ((rc = alloc(p, reinterpret_cast<void**>(&p->d_iota), iota.size() * sizeof(int32_t)))) return rc;
        NUFFT_HIP(hipMemcpy(p->d_iota, iota.data(), iota.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    size_t lengths[3] = {1, 1, 1};
    for (int d = 0; d < p->D; ++d) lengths[d] = (size_t)p->N[d];
    const rocfft_precision prec = p->dtype == NUFFT_F32 ? rocfft_precision_single : rocfft_precision_double;
    NUFFT_ROCFFT(rocfft_execution_info_create(&p->fft_info));
    NUFFT_ROCFFT(rocfft_plan_create(&p->fft_fw, rocfft_placement_inplace, rocfft_transform_type_complex_forward, prec, (size_t)p->D, lengths, 1, nullptr));
    NUFFT_ROCFFT(rocfft_plan_get_work_buffer_size(p->fft_fw, &p->fft_work_bytes));
    if (!fused) {
        size_t wb = 0;
        NUFFT_ROCFFT(rocfft_plan_create(&p->fft_bw, rocfft_placement_inplace, rocfft_transform_type_complex_inverse, prec, (size_t)p->D, lengths, 1, nullptr));
        NUFFT_ROCFFT(rocfft_plan_get_work_buffer_size(p->fft_bw, &wb));
        p->fft_work_bytes = std::max(p->fft_work_bytes, wb);
        if (p->fft_work_bytes > 0) {
            if ((rc = alloc(p, &p->d_fft_work, p->fft_work_bytes))) return rc;
            NUFFT_ROCFFT(rocfft_execution_info_set_work_buffer(p->fft_info, p->d_fft_work, p->fft_work_bytes));
        }
    }
    return NUFFT_OK;
}

// The temporaries of a build: the (2N)^D complex grid with its transform, and (fused path) the work buffer of the size-N transform.
struct BuildScratch {
    nufft_precond* p;
    void* grid = nullptr;
    size_t grid_bytes = 0;
    rocfft_plan_t* plan2 = nullptr;
    rocfft_execution_info_t* info2 = nullptr;
    void* work2 = nullptr;
    size_t work2_bytes = 0;
    void* work = nullptr;
    explicit BuildScratch(nufft_precond* pc) : p(pc) {}
    ~BuildScratch() {
        if (plan2) (void)rocfft_plan_destroy(plan2);
        if (info2) (void)rocfft_execution_info_destroy(info2);
        free_buffer(p->own_bytes, grid, grid_bytes);
        free_buffer(p->own_bytes, work2, work2_bytes);
        if (work) {
            free_buffer(p->own_bytes, work, p->fft_work_bytes);
            (void)rocfft_execution_info_set_work_buffer(p->fft_info, nullptr, 0);
        }
    }
};

// The scalar object serves independent components, the block object the K coupled components it was created for.
int check_coupling(const nufft_precond* p) {
    if (nufft_toeplitz_num_frames(p->tz) > 0)
        return fail(NUFFT_ERR_UNSUPPORTED, "the operator is framed (nufft_toeplitz_set_points_frames / _set_spectra_frames: one multiplier per component): "
                                           "a preconditioner of per-frame circulants is not built");
    if (nufft_toeplitz_num_segments(p->tz) > 0)
        return fail(NUFFT_ERR_UNSUPPORTED, "the operator is segmented (nufft_toeplitz_create_segmented: field-map factors around a block of segments): "
                                           "a preconditioner of the folded operator is not built");
    const int K = nufft_toeplitz_num_coupled(p->tz);
    if (p->K == 0 && K > 0)
        return fail(NUFFT_ERR_UNSUPPORTED, "the operator couples its components: nufft_precond_create builds the preconditioner of independent components; a "
                                           "coupled operator takes the block preconditioner of nufft_precond_create_block (Python: block=True)");
    if (p->K > 0 && K != p->K)
        return fail(NUFFT_ERR_UNSUPPORTED, K > 0 ? "the block preconditioner was created for another number of coupled components: create a new one"
                                                 : "nufft_precond_create_block needs a coupled build in force (nufft_toeplitz_set_points_coupled / "
                                                   "_set_spectra_coupled); independent components take nufft_precond_create");
    return NUFFT_OK;
}

// d = (Σ_c |S_c|²)^(−1/2) from the operator's maps, and the mean of the sum (for μ)
int scaling_from_maps(nufft_precond* p, const std::vector<const void*>& maps, double& mean, hipStream_t stream) {
    int rc;
    if (!p->d_own_d && (rc = alloc(p, &p->d_own_d, (size_t)p->n * real_bytes(p->dtype)))) return rc;
    NUFFT_HIP(launch_pc_coil_power(p->dtype, p->d_own_d, maps.data(), (int)maps.size(), p->n, p->d_part, p->G, stream));
    std::vector<double> part((size_t)p->G * 2);
    NUFFT_HIP(hipMemcpyAsync(part.data(), p->d_part, part.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    NUFFT_HIP(hipStreamSynchronize(stream));
    double hi = 0.0, sum = 0.0;
    for (int g = 0; g < p->G; ++g) {
        hi = std::max(hi, part[2 * (size_t)g]);
        sum += part[2 * (size_t)g + 1];
    }
    if (!(hi > 0.0) || !std::isfinite(hi) || !std::isfinite(sum))
        return fail(NUFFT_ERR_INVALID_ARG, "the coil maps of the operator are zero or not finite: no scaling can be formed from them");
    mean = sum / (double)p->n;
    NUFFT_HIP(launch_pc_coil_scaling(p->dtype, p->d_own_d, p->n, 1e-3 * hi, p->num_cus, stream));
    return NUFFT_OK;
}

int build(nufft_precond* p, hipStream_t stream) {
    nufft_toeplitz_info ti;
    std::memset(&ti, 0, sizeof(ti));
    ti.struct_size = (int32_t)sizeof(ti);
    int rc = nufft_toeplitz_get_info(p->tz, &ti);
    if (rc) return rc;
    if (!ti.has_spectrum)
        return fail(NUFFT_ERR_NO_POINTS, "nufft_toeplitz_set_spectrum or nufft_toeplitz_set_points must be called before the preconditioner is built");
    if ((rc = check_coupling(p))) return rc;
    if (capturing(stream))
        return fail(NUFFT_ERR_INVALID_ARG, "the build of a preconditioner allocates and synchronises: not on a capturing stream");
    const size_t cb = 2 * real_bytes(p->dtype);
    const int64_t cells2 = ti.N2[0] * ti.N2[1] * ti.N2[2];
    BuildScratch s(p);
    s.grid_bytes = (size_t)cells2 * cb;
    if ((rc = alloc(p, &s.grid, s.grid_bytes))) return rc;
    size_t lengths2[3] = {1, 1, 1};
    for (int d = 0; d < p->D; ++d) lengths2[d] = (size_t)ti.N2[d];
    const rocfft_precision prec = p->dtype == NUFFT_F32 ? rocfft_precision_single : rocfft_precision_double;
    NUFFT_ROCFFT(rocfft_plan_create(&s.plan2, rocfft_placement_inplace, rocfft_transform_type_complex_forward, prec, (size_t)p->D, lengths2, 1, nullptr));
    NUFFT_ROCFFT(rocfft_execution_info_create(&s.info2));
    NUFFT_ROCFFT(rocfft_plan_get_work_buffer_size(s.plan2, &s.work2_bytes));
    if (s.work2_bytes > 0) {
        if ((rc = alloc(p, &s.work2, s.work2_bytes))) return rc;
        NUFFT_ROCFFT(rocfft_execution_info_set_work_buffer(s.info2, s.work2, s.work2_bytes));
    }
    NUFFT_ROCFFT(rocfft_execution_info_set_stream(s.info2, stream));
    if (p->path == NUFFT_PRECOND_PATH_FUSED && p->fft_work_bytes > 0) {
        if ((rc = alloc(p, &s.work, p->fft_work_bytes))) return rc;
        NUFFT_ROCFFT(rocfft_execution_info_set_work_buffer(p->fft_info, s.work, p->fft_work_bytes));
    }
    NUFFT_ROCFFT(rocfft_execution_info_set_stream(p->fft_info, stream));

    // the scaling and μ
    const std::vector<const void*>& maps = toeplitz_coil_maps(p->tz);
    double mu = p->lambda;
    if (!maps.empty()) {
        double mean = 1.0;
        if ((rc = scaling_from_maps(p, maps, mean, stream))) return rc;
        mu = p->lambda / mean;
        p->d_scaling = p->d_own_d;
        p->scaling = NUFFT_PRECOND_SCALING_MAPS;
    } else if (p->scaling == NUFFT_PRECOND_SCALING_MAPS) {
        p->d_scaling = nullptr;
        p->scaling = NUFFT_PRECOND_SCALING_NONE;
    }

    // per multiplier grid: T = forwardDFT_2N(K);  c = fold(T);  E = DFT_N(c), left in d_scratch.  The scalar object has one real grid; the
    // block object one per stored pair a <= b (complex for a < b), through the one (2N)^D temporary.  The diagonal keeps Re E.
    PcGrid g{};
    g.dtype = p->dtype;
    g.D = p->D;
    for (int d = 0; d < 3; ++d) g.n[d] = (int)p->N[d];
    const size_t rb = real_bytes(p->dtype);
    const int rows = std::max(p->K, 1);
    for (int a = 0; a < rows; ++a)
        for (int b = a; b < rows; ++b) {
            void* K = nullptr;
            if ((rc = p->K > 0 ? nufft_toeplitz_multiplier_pair_ptr(p->tz, a, b, &K, nullptr) : nufft_toeplitz_multiplier_ptr(p->tz, &K, nullptr))) return rc;
            if (a == b) NUFFT_HIP(launch_pc_embed(p->dtype, s.grid, K, cells2, p->num_cus, stream));
            else NUFFT_HIP(hipMemcpyAsync(s.grid, K, s.grid_bytes, hipMemcpyDeviceToDevice, stream));
            void* io2[1] = {s.grid};
            NUFFT_ROCFFT(rocfft_execute(s.plan2, io2, nullptr, s.info2));
            NUFFT_HIP(launch_pc_fold(g, p->d_scratch, s.grid, p->num_cus, stream));
            void* io[1] = {p->d_scratch};
            NUFFT_ROCFFT(rocfft_execute(p->fft_fw, io, nullptr, p->fft_info));
            if (a == b) {
                void* e = p->K > 0 ? static_cast<char*>(p->d_bd) + (size_t)a * p->pitch * rb : p->d_m;
                NUFFT_HIP(launch_pc_eigen(p->dtype, e, p->d_scratch, p->n, p->d_part + (size_t)a * p->G * 2, p->G, stream));
            } else {
                void* e = static_cast<char*>(p->d_bc) + (size_t)coupled_offdiag_index(a, b, p->K) * p->pitch * cb;
                NUFFT_HIP(hipMemcpyAsync(e, p->d_scratch, (size_t)p->n * cb, hipMemcpyDeviceToDevice, stream));
            }
        }
    std::vector<double> part((size_t)rows * p->G * 2);
    NUFFT_HIP(hipMemcpyAsync(part.data(), p->d_part, part.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    NUFFT_HIP(hipStreamSynchronize(stream));
    double hi = -INFINITY, lo = -INFINITY;
    for (size_t w = 0; w < (size_t)rows * p->G; ++w) {
        hi = std::max(hi, part[2 * w]);
        lo = std::max(lo, part[2 * w + 1]);
    }
    p->max_e = hi;
    p->min_e = -lo;
    p->mu = mu;
    if (!std::isfinite(hi) || !(hi + mu > 0.0))
        return fail(NUFFT_ERR_INVALID_ARG, "the eigenvalues of the circulant plus mu are nowhere positive (a zero operator with lambda = 0?): nothing to invert");
    if (p->K > 0) {
        // the floor as a shift: every eigenvalue of E(q) + shift I is at least shift, so is every Cholesky pivot in exact arithmetic
        const double shift = std::max(mu, p->floor * (hi + mu));
        NUFFT_HIP(launch_pc_block_invert(p->dtype, p->d_bd, p->d_bc, p->K, p->n, p->pitch, shift, kPcPivotFraction * shift, (double)p->n, p->d_cnt,
                                         p->Gc, stream));
        std::vector<double> cnt((size_t)p->Gc);
        NUFFT_HIP(hipMemcpyAsync(cnt.data(), p->d_cnt, cnt.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        NUFFT_HIP(hipStreamSynchronize(stream));      // the temporaries are freed on return
        double total = 0.0;
        for (double c : cnt) total += c;
        p->floored = (int64_t)total;
        return NUFFT_OK;
    }
    NUFFT_HIP(launch_pc_invert(p->dtype, p->d_m, p->n, mu, p->floor * (hi + mu), (double)p->n, p->num_cus, stream));
    NUFFT_HIP(hipStreamSynchronize(stream));      // the temporaries are freed on return
    return NUFFT_OK;
}

// One unpruned strided pass along dimension `dim` (1 or 2, zero-based) of a component: all N_dim modes are kept (identity map, unit
// factor tables), so the backward instantiation reads d on its load side and the forward one on its store side.
int strided_pass(const nufft_precond* p, int dim, bool forward, const void* in, void* out, const void* mult, hipStream_t stream) {
    FftLinePass q{};
    q.in = in;
    q.out = out;
    q.map = p->d_iota;
    q.nk = (int)p->N[dim];
    q.twiddle = forward ? p->d_tw_fw[dim] : p->d_tw_bw[dim];
    q.fa = p->d_ones; q.ka = 1;
    q.fk = p->d_ones;
    q.scale = 1.0;
    q.mult = mult;
    const int64_t N1 = p->N[0];
    if (dim == 2) {
        q.a_total = q.a_out = N1 * p->N[1];
        q.in_stride_j = q.out_stride_j = N1 * p->N[1];
        q.in_stride_c = q.out_stride_c = 0;
        q.nc = 1;
    } else {
        q.a_total = q.a_out = N1;
        q.in_stride_j = q.out_stride_j = N1;
        q.in_stride_c = q.out_stride_c = N1 * p->N[1];
        q.nc = (int)p->N[2];
    }
    NUFFT_HIP(launch_fft_lines(p->dtype, p->N[dim], forward, q, stream));
    return NUFFT_OK;
}

int apply_fused(nufft_precond* p, void* out, const void* in, hipStream_t stream) {
    int rc;
    void* s = p->d_scratch;
    if (p->D == 3) {
        if ((rc = strided_pass(p, 2, false, in, s, p->d_scaling, stream)) || (rc = strided_pass(p, 1, false, s, s, nullptr, stream))) return rc;
    } else if ((rc = strided_pass(p, 1, false, in, s, p->d_scaling, stream))) {
        return rc;
    }
    NUFFT_HIP(launch_precond_lines(p->dtype, p->N[0], s, p->d_m, (int)p->N[1], (int)p->N[2], p->d_tw_fw[0], stream));
    if (p->D == 3) {
        if ((rc = strided_pass(p, 1, true, s, s, nullptr, stream))) return rc;
        return strided_pass(p, 2, true, s, out, p->d_scaling, stream);
    }
    return strided_pass(p, 1, true, s, out, p->d_scaling, stream);
}

int apply_dense(nufft_precond* p, void* out, const void* in, hipStream_t stream) {
    void* io[1] = {p->d_scratch};
    NUFFT_HIP(launch_pc_scale(p->dtype, p->d_scratch, in, p->d_scaling, p->n, p->num_cus, stream));
    NUFFT_ROCFFT(rocfft_execute(p->fft_fw, io, nullptr, p->fft_info));
    NUFFT_HIP(launch_pc_scale(p->dtype, p->d_scratch, p->d_scratch, p->d_m, p->n, p->num_cus, stream));
    NUFFT_ROCFFT(rocfft_execute(p->fft_bw, io, nullptr, p->fft_info));
    NUFFT_HIP(launch_pc_scale(p->dtype, out, p->d_scratch, p->d_scaling, p->n, p->num_cus, stream));
    return NUFFT_OK;
}

// The block object: every input passes into its own scratch array before the one kernel that mixes them, and only then is any output
// written — out[a] may be in[a].
int apply_block(nufft_precond* p, void* const* out, const void* const* in, hipStream_t stream) {
    int rc;
    const size_t sb = (size_t)p->sstride * 2 * real_bytes(p->dtype);
    auto scratch = [&](int a) { return static_cast<void*>(static_cast<char*>(p->d_scratch) + (size_t)a * sb); };
    if (p->path == NUFFT_PRECOND_PATH_DENSE) {
        for (int b = 0; b < p->K; ++b) {
            void* io[1] = {scratch(b)};
            NUFFT_HIP(launch_pc_scale(p->dtype, io[0], in[b], p->d_scaling, p->n, p->num_cus, stream));
            NUFFT_ROCFFT(rocfft_execute(p->fft_fw, io, nullptr, p->fft_info));
        }
        NUFFT_HIP(launch_pc_block_multiply(p->dtype, p->d_scratch, p->sstride, p->K, p->d_bd, p->d_bc, p->n, p->pitch, p->num_cus, stream));
        for (int a = 0; a < p->K; ++a) {
            void* io[1] = {scratch(a)};
            NUFFT_ROCFFT(rocfft_execute(p->fft_bw, io, nullptr, p->fft_info));
            NUFFT_HIP(launch_pc_scale(p->dtype, out[a], io[0], p->d_scaling, p->n, p->num_cus, stream));
        }
        return NUFFT_OK;
    }
    for (int b = 0; b < p->K; ++b) {
        void* s = scratch(b);
        if (p->D == 3) {
            if ((rc = strided_pass(p, 2, false, in[b], s, p->d_scaling, stream)) || (rc = strided_pass(p, 1, false, s, s, nullptr, stream))) return rc;
        } else if ((rc = strided_pass(p, 1, false, in[b], s, p->d_scaling, stream))) {
            return rc;
        }
    }
    NUFFT_HIP(launch_precond_block_lines(p->dtype, p->N[0], p->K, p->d_scratch, p->sstride, p->d_bd, p->d_bc, (int)p->N[1], (int)p->N[2], p->d_tw_fw[0],
                                         stream));
    for (int a = 0; a < p->K; ++a) {
        void* s = scratch(a);
        if (p->D == 3) {
            if ((rc = strided_pass(p, 1, true, s, s, nullptr, stream)) || (rc = strided_pass(p, 2, true, s, out[a], p->d_scaling, stream))) return rc;
        } else if ((rc = strided_pass(p, 1, true, s, out[a], p->d_scaling, stream))) {
            return rc;
        }
    }
    return NUFFT_OK;
}

int create(nufft_precond** out, nufft_toeplitz* tz, const nufft_precond_params* params, bool block) {
    if (!out || !tz || !params) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    nufft_precond_params prm;
    int rc = read_params(prm, params, "nufft_precond_params");
    if (rc) return rc;
    if (!std::isfinite(prm.lambda) || prm.lambda < 0) return fail(NUFFT_ERR_INVALID_ARG, "lambda must be finite and not negative");
    if (!std::isfinite(prm.floor) || !(prm.floor > 0)) return fail(NUFFT_ERR_INVALID_ARG, "floor must be finite and positive");
    nufft_toeplitz_info ti;
    std::memset(&ti, 0, sizeof(ti));
    ti.struct_size = (int32_t)sizeof(ti);
    if ((rc = nufft_toeplitz_get_info(tz, &ti))) return rc;
    if (ti.device < 0) return fail(NUFFT_ERR_NO_DEVICE, "host-only Toeplitz object (device = -1): the preconditioner runs on the device");
    if (nufft_toeplitz_num_frames(tz) > 0)
        return fail(NUFFT_ERR_UNSUPPORTED, "the operator is framed (nufft_toeplitz_set_points_frames / _set_spectra_frames: one multiplier per component): "
                                           "a preconditioner of per-frame circulants is not built");
    if (nufft_toeplitz_num_segments(tz) > 0)
        return fail(NUFFT_ERR_UNSUPPORTED, "the operator is segmented (nufft_toeplitz_create_segmented: field-map factors around a block of segments): "
                                           "a preconditioner of the folded operator is not built");

    nufft_precond* p = new (std::nothrow) nufft_precond();
    if (!p) return fail(NUFFT_ERR_ALLOC, "out of host memory");
    p->tz = tz;
    p->dtype = ti.dtype;
    p->D = ti.ndim;
    p->C = ti.ntransforms;
    p->device = ti.device;
    p->lambda = prm.lambda;
    p->floor = prm.floor;
    if (block) {      // the arrays are sized by K: the refusals of the build that depend on the operator's state come first, in its order
        p->K = ti.ntransforms;
        if (!ti.has_spectrum) rc = fail(NUFFT_ERR_NO_POINTS, "nufft_toeplitz_set_spectrum or nufft_toeplitz_set_points must be called before the preconditioner is built");
        else rc = check_coupling(p);
        if (rc) {
            delete p;
            return rc;
        }
    }
    // the operator's dense path on a shape its fused path supports is the plan's option NUFFT_TOEPLITZ_FUSED=0, which this object honours
    bool op_fusable = ti.ndim >= 2;
    bool fused = ti.ndim >= 2;
    for (int d = 0; d < 3; ++d) {
        p->N[d] = ti.N[d];
        if (d >= ti.ndim) continue;
        op_fusable = op_fusable && fft_lines_supported(ti.dtype, ti.N2[d]) && toeplitz_lines_supported(ti.dtype, ti.N2[d]);
        fused = fused && fft_lines_supported(ti.dtype, ti.N[d]) && precond_lines_supported(ti.dtype, ti.N[d]);
    }
    if (op_fusable && ti.path == NUFFT_TOEPLITZ_PATH_DENSE) fused = false;
    // the K lines of one wave must fit LDS; where they do not, the dense path serves (the operator refuses such a build instead)
    if (block && !precond_block_lines_supported(ti.dtype, ti.N[0], p->K)) fused = false;
    p->n = p->N[0] * p->N[1] * p->N[2];
    p->path = fused ? NUFFT_PRECOND_PATH_FUSED : NUFFT_PRECOND_PATH_DENSE;

    DeviceGuard guard(p->device);
    p->num_cus = device_cus(p->device);
    if ((rc = build_device(p)) || (rc = build(p, nullptr))) {
        const std::string keep = nufft_last_error_message();
        release(p);
        return fail(rc, keep);
    }
    *out = p;
    return NUFFT_OK;
}

}  // namespace

const nufft_toeplitz* nufft::precond_operator(const nufft_precond* pc) { return pc ? pc->tz : nullptr; }

extern "C" {

int64_t nufft_sizeof_precond_params(void) { return (int64_t)sizeof(nufft_precond_params); }
int64_t nufft_sizeof_precond_info(void) { return (int64_t)sizeof(nufft_precond_info); }

int nufft_precond_create(nufft_precond** out, nufft_toeplitz* tz, const nufft_precond_params* params) { return create(out, tz, params, false); }

int nufft_precond_create_block(nufft_precond** out, nufft_toeplitz* tz, const nufft_precond_params* params) { return create(out, tz, params, true); }

int nufft_precond_destroy(nufft_precond* pc) {
    release(pc);
    return NUFFT_OK;
}

int nufft_precond_update(nufft_precond* pc, void* stream) {
    if (!pc) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    DeviceGuard guard(pc->device);
    return build(pc, static_cast<hipStream_t>(stream));
}

int nufft_precond_set_scaling(nufft_precond* pc, const void* d) {
    if (!pc) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(d) & 15) return fail(NUFFT_ERR_INVALID_ARG, "the scaling must be 16-byte aligned");
    pc->d_scaling = d;
    pc->scaling = d ? NUFFT_PRECOND_SCALING_CALLER : NUFFT_PRECOND_SCALING_NONE;
    return NUFFT_OK;
}

int nufft_precond_apply(nufft_precond* pc, void* const* out, const void* const* in, void* stream_) {
    if (!pc) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (!out || !in) return fail(NUFFT_ERR_INVALID_ARG, "null table");
    for (int c = 0; c < pc->C; ++c) {
        if (!out[c] || !in[c]) return fail(NUFFT_ERR_INVALID_ARG, "null data vector");
        if ((reinterpret_cast<uintptr_t>(out[c]) | reinterpret_cast<uintptr_t>(in[c])) & 15)
            return fail(NUFFT_ERR_INVALID_ARG, "the arrays of nufft_precond_apply must be 16-byte aligned");
    }
    DeviceGuard guard(pc->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (pc->path == NUFFT_PRECOND_PATH_DENSE) NUFFT_ROCFFT(rocfft_execution_info_set_stream(pc->fft_info, stream));
    if (pc->K > 0) return apply_block(pc, out, in, stream);
    for (int c = 0; c < pc->C; ++c) {
        const int rc = pc->path == NUFFT_PRECOND_PATH_FUSED ? apply_fused(pc, out[c], in[c], stream) : apply_dense(pc, out[c], in[c], stream);
        if (rc) return rc;
    }
    return NUFFT_OK;
}

int nufft_precond_get_info(const nufft_precond* pc, nufft_precond_info* o) {
    if (!pc || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    nufft_precond_info i;
    std::memset(&i, 0, sizeof(i));
    i.ndim = pc->D;
    i.dtype = pc->dtype;
    i.ntransforms = pc->C;
    i.device = pc->device;
    i.path = pc->path;
    i.scaling = pc->scaling;
    for (int d = 0; d < 3; ++d) i.N[d] = pc->N[d];
    i.lambda = pc->lambda;
    i.mu = pc->mu;
    i.floor = pc->floor;
    i.max_e = pc->max_e;
    i.min_e = pc->min_e;
    i.multiplier_bytes = (pc->K > 0 ? (int64_t)pc->K * pc->K : 1) * pc->n * (int64_t)real_bytes(pc->dtype);
    i.workspace_bytes = pc->own_bytes;
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_precond_multiplier_ptr(const nufft_precond* pc, void** out_ptr, int64_t* out_bytes) {
    if (!pc || !out_ptr) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (pc->K > 0) return fail(NUFFT_ERR_UNSUPPORTED, "a block preconditioner has no single multiplier: ask nufft_precond_block_ptr for B_ab");
    *out_ptr = pc->d_m;
    if (out_bytes) *out_bytes = pc->n * (int64_t)real_bytes(pc->dtype);
    return NUFFT_OK;
}

int nufft_precond_scaling_ptr(const nufft_precond* pc, void** out_ptr, int64_t* out_bytes) {
    if (!pc || !out_ptr) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out_ptr = const_cast<void*>(pc->d_scaling);
    if (out_bytes) *out_bytes = pc->d_scaling ? pc->n * (int64_t)real_bytes(pc->dtype) : 0;
    return NUFFT_OK;
}

int32_t nufft_precond_num_coupled(const nufft_precond* pc) { return pc ? (int32_t)pc->K : 0; }

int64_t nufft_precond_floored_cells(const nufft_precond* pc) { return pc ? pc->floored : -1; }

int nufft_precond_block_ptr(const nufft_precond* pc, int32_t a, int32_t b, void** out_ptr, int64_t* out_bytes) {
    if (!pc || !out_ptr) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (pc->K == 0) return fail(NUFFT_ERR_UNSUPPORTED, "nufft_precond_block_ptr: not a block preconditioner (nufft_precond_multiplier_ptr returns m)");
    if (a < 0 || b < a || b >= pc->K) return fail(NUFFT_ERR_INVALID_ARG, "nufft_precond_block_ptr: the pair must satisfy 0 <= a <= b < K (B_ba = conj(B_ab))");
    const int64_t rb = (int64_t)real_bytes(pc->dtype);
    if (a == b) {
        *out_ptr = static_cast<char*>(pc->d_bd) + a * pc->pitch * rb;
        if (out_bytes) *out_bytes = pc->n * rb;
    } else {
        *out_ptr = static_cast<char*>(pc->d_bc) + coupled_offdiag_index(a, b, pc->K) * pc->pitch * 2 * rb;
        if (out_bytes) *out_bytes = pc->n * 2 * rb;
    }
    return NUFFT_OK;
}

}  // extern "C"
