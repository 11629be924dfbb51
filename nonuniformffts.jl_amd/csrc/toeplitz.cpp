// Toeplitz normal operator G = A^H W A of a complex plan (include/nufft_mi355x.h, Toeplitz section).
//
// G[k, k'] = T[k − k'] with T_d = Σ_j w_j exp(−i d·x_j): a multi-level Toeplitz matrix, embedded in a circulant of size 2 N_d per
// dimension.  With K = backwardDFT_{2N}(T) / Π 2N_d (real for real weights, once the never-used Nyquist planes of T are zeroed),
//   G û = crop(forwardDFT_{2N}(K ⊙ backwardDFT_{2N}(pad(û)))).
// The fused path runs pad + backward transform and forward transform + crop as the pruned line passes of fft_lines.hip (kept modes
// in, full line out and back) with the multiply inside the dimension-1 kernel; the dense path runs rocFFT on a (2N)^D grid.
//
// With coil sensitivity maps S_c set the same apply computes G_S û = Σ_c conj(S_c) ⊙ G (S_c ⊙ û), coil after
// coil in stream order: S_c multiplies where the first pass loads the caller's array, conj(S_c) where the last pass stores into it,
// and coils >= 1 add to what coil 0 stored.
//
// With a coupled build the C components are one block operator, out[a] = Σ_b Toeplitz(T_ab) in[b]: the halves of
// the apply before and after the multiply run per component into C intermediates, and one kernel applies the C × C block of
// multipliers (C real grids K_aa, C (C − 1) / 2 complex grids K_ab, a < b; K_ba = conj(K_ab)) to every cell in between.
//
// A segmented operator (off-resonance correction by time segmentation) has one component outside and L coupled
// segments inside: G_ω û = Σ_a conj(B_a) ⊙ Σ_b Toeplitz(T_ab) (B_b ⊙ û).  It is the coupled apply with in[b] = û for every b, the factor
// B_b where the coil's map multiplies, and every forward half accumulating into the one output; coil maps go around it through two
// scratch arrays.
#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "host_common.h"
#include "kernels.h"
#include "toeplitz.h"

using namespace nufft;

namespace {
// The build in force: none, one shared multiplier (d_K), the C × C block of a coupled build, or one multiplier per frame.
enum Mode { MODE_NONE, MODE_PLAIN, MODE_COUPLED, MODE_FRAMED };
}  // namespace

struct nufft_toeplitz {
    int dtype = NUFFT_F64, D = 1, C = 1, device = -1, num_cus = 256;
    bool fftshift = false;
    int64_t N[3] = {1, 1, 1}, N2[3] = {1, 1, 1};
    int path = NUFFT_TOEPLITZ_PATH_DENSE;
    // the parent plan's window parameters (the internal 2N plan of set_points takes them)
    int M = 4, kernel = 0, evalmode = 0, point_transform = 0;
    double sigma_req = 2.0;
    std::string options;
    std::vector<int32_t> map[3], inv[3];
    // device
    int32_t* d_map[3] = {nullptr, nullptr, nullptr};
    int32_t* d_inv[3] = {nullptr, nullptr, nullptr};
    void* d_tw_fw[3] = {nullptr, nullptr, nullptr};    // complex<T>[2N_d]: exp(-2πi m / 2N_d)
    void* d_tw_bw[3] = {nullptr, nullptr, nullptr};    // (dimensions 2, 3 of the fused path)
    void* d_ones = nullptr;                            // T[max N_d] = 1: the unit factor tables of the strided passes
    void* d_K = nullptr;                               // T[2N_1, 2N_2, 2N_3]
    void* d_tmpA = nullptr;                            // fused, 3-D: complex<T>[N_1, N_2, 2N_3]
    void* d_tmpB = nullptr;                            // fused: complex<T>[N_1, 2N_2, 2N_3]
    void* d_work = nullptr;                            // dense: complex<T>[2N_1, 2N_2, 2N_3]
    rocfft_plan_t* fft_bw = nullptr;                   // in-place c2c of the embedding grid (multiplier; dense apply)
    rocfft_plan_t* fft_fw = nullptr;                   // dense apply
    rocfft_execution_info_t* fft_info = nullptr;
    void* d_fft_work = nullptr;                        // dense: kept; fused: lives inside set_spectrum
    size_t fft_work_bytes = 0;
    int64_t own_bytes = 0, build_bytes = 0;
    Mode mode = MODE_NONE;                             // set by a build that succeeded (begin_build resets it)
    // coil sensitivity maps: borrowed device pointers, the host table is the operator's
    std::vector<const void*> coil_maps;
    bool maps_inpass = true;                           // fused: the maps ride in the outermost passes (false: expand / apply / combine)
    void* d_coil = nullptr;                            // fused, streaming route: complex<T>[N_1, N_2, N_3], held while maps are set
    // coupled components: the C × C block multiplier and one intermediate per component, held from the first
    // coupled build to the next uncoupled one
    void* d_kd = nullptr;                              // T[C][2N_1, 2N_2, 2N_3]: the diagonal blocks K_aa
    void* d_kc = nullptr;                              // complex<T>[C (C − 1) / 2][2N_1, 2N_2, 2N_3]: K_ab, a < b, row-major
    void* d_grids = nullptr;                           // fused: C arrays like d_tmpB; dense: C arrays like d_work
    // frames: one real multiplier per component, held from the first framed build to the next plain or
    // coupled one
    void* d_kf = nullptr;                              // C arrays like d_K, frame_stride bytes apart
    // time segments: fixed at creation; C = 1 outside, `seg` coupled segments inside
    int seg = 0;                                       // L of nufft_toeplitz_create_segmented, 0 on an ordinary operator
    std::vector<const void*> factors;                  // B_l: borrowed device pointers, the host table is the operator's
    void* d_sv = nullptr;                              // complex<T>[N_1, N_2, N_3] each: S_c ⊙ û and the folded product of one coil,
    void* d_sw = nullptr;                              // held while coil maps and factors are both set
};

namespace {

int64_t grid_cells(const nufft_toeplitz* t) { return t->N2[0] * t->N2[1] * t->N2[2]; }
int64_t num_modes(const nufft_toeplitz* t) { return t->N[0] * t->N[1] * t->N[2]; }
// The size of the coupled block: the segments of a segmented operator, the components of any other.
int inner(const nufft_toeplitz* t) { return t->seg > 0 ? t->seg : t->C; }

// Bytes of every buffer the object holds at rest, in allocation order (a host-only object reports their sum; rocFFT's own work
// buffer, known only on a device, comes on top for the dense path).
struct Sizes {
    size_t K, tmpA, tmpB, work, maps, twiddles, ones;
    size_t total() const { return K + tmpA + tmpB + work + maps + twiddles + ones; }
};
Sizes sizes_of(const nufft_toeplitz* t) {
    const size_t rb = real_bytes(t->dtype), cb = 2 * rb;
    const bool fused = t->path == NUFFT_TOEPLITZ_PATH_FUSED;
    Sizes s{};
    s.K = padded((size_t)grid_cells(t) * rb);
    s.tmpA = fused && t->D == 3 ? padded((size_t)(t->N[0] * t->N[1] * t->N2[2]) * cb) : 0;
    s.tmpB = fused ? padded((size_t)(t->N[0] * t->N2[1] * t->N2[2]) * cb) : 0;
    s.work = fused ? 0 : padded((size_t)grid_cells(t) * cb);
    int64_t nmax = 1;
    for (int d = 0; d < 3; ++d) {
        s.maps += padded((size_t)t->N[d] * 4) + padded((size_t)t->N2[d] * 4);
        if (fused && d < t->D) s.twiddles += padded((size_t)t->N2[d] * cb) * (d == 0 ? 1 : 2);
        nmax = std::max(nmax, t->N[d]);
    }
    s.ones = fused ? padded((size_t)nmax * rb) : 0;
    return s;
}

int alloc(nufft_toeplitz* t, void** ptr, size_t bytes) { return alloc_buffer(t->own_bytes, "Toeplitz", ptr, bytes); }

// The buffers of a coupled build: C real and C (C − 1) / 2 complex multiplier grids, and C intermediates (each padded on its own:
// the components of d_grids are grid_stride complex elements apart).
size_t coupled_kd_bytes(const nufft_toeplitz* t) { return (size_t)inner(t) * (size_t)grid_cells(t) * real_bytes(t->dtype); }
size_t coupled_kc_bytes(const nufft_toeplitz* t) { return (size_t)(inner(t) * (inner(t) - 1) / 2) * (size_t)grid_cells(t) * 2 * real_bytes(t->dtype); }
size_t coupled_grid_stride(const nufft_toeplitz* t) {
    const size_t cb = 2 * real_bytes(t->dtype);
    const size_t n = t->path == NUFFT_TOEPLITZ_PATH_FUSED ? (size_t)(t->N[0] * t->N2[1] * t->N2[2]) : (size_t)grid_cells(t);
    return padded(n * cb) / cb;
}
size_t coupled_grids_bytes(const nufft_toeplitz* t) { return (size_t)inner(t) * coupled_grid_stride(t) * 2 * real_bytes(t->dtype); }

// The multipliers of a framed build: C real grids, each padded on its own (the alignment of d_K for every frame).
size_t frame_stride(const nufft_toeplitz* t) { return padded((size_t)grid_cells(t) * real_bytes(t->dtype)); }
size_t frames_bytes(const nufft_toeplitz* t) { return (size_t)t->C * frame_stride(t); }

// What every build starts with: no build is in force, the storage of the other modes goes (hipFree waits for the applies in flight)
// and this mode's is taken unless an earlier build of the mode left it.  `acquire` = false: the build is refused after this and takes
// nothing new.
int begin_build(nufft_toeplitz* t, Mode mode, bool acquire = true) {
    t->mode = MODE_NONE;
    if (mode != MODE_COUPLED) {
        free_buffer(t->own_bytes, t->d_kd, coupled_kd_bytes(t));
        free_buffer(t->own_bytes, t->d_kc, coupled_kc_bytes(t));
        free_buffer(t->own_bytes, t->d_grids, coupled_grids_bytes(t));
    }
    if (mode != MODE_FRAMED) free_buffer(t->own_bytes, t->d_kf, frames_bytes(t));
    if (!acquire) return NUFFT_OK;
    int rc;
    if (mode == MODE_COUPLED) {
        if (!t->d_kd && (rc = alloc(t, &t->d_kd, coupled_kd_bytes(t)))) return rc;
        if (!t->d_kc && inner(t) > 1 && (rc = alloc(t, &t->d_kc, coupled_kc_bytes(t)))) return rc;
        if (!t->d_grids && (rc = alloc(t, &t->d_grids, coupled_grids_bytes(t)))) return rc;
    }
    if (mode == MODE_FRAMED && !t->d_kf && (rc = alloc(t, &t->d_kf, frames_bytes(t)))) return rc;
    return NUFFT_OK;
}

// Where the multipliers of a mode live, in build order: the one of a plain build, one per frame, the pairs a <= b of a coupled build
// row-major.  Real grids but for the pairs a < b, which are complex.
struct Multiplier {
    void* ptr;
    bool complex;
};
int num_multipliers(const nufft_toeplitz* t, Mode mode) {
    return mode == MODE_COUPLED ? inner(t) * (inner(t) + 1) / 2 : mode == MODE_FRAMED ? t->C : 1;
}
Multiplier pair_multiplier(const nufft_toeplitz* t, int a, int b) {        // a <= b
    const size_t real_grid = (size_t)grid_cells(t) * real_bytes(t->dtype);
    if (a == b) return {static_cast<char*>(t->d_kd) + (size_t)a * real_grid, false};
    return {static_cast<char*>(t->d_kc) + (size_t)nufft::coupled_offdiag_index(a, b, inner(t)) * 2 * real_grid, true};
}
Multiplier multiplier_at(const nufft_toeplitz* t, Mode mode, int i) {
    if (mode == MODE_PLAIN) return {t->d_K, false};
    if (mode == MODE_FRAMED) return {static_cast<char*>(t->d_kf) + (size_t)i * frame_stride(t), false};
    int a = 0;
    for (const int K = inner(t); i >= K - a; ++a) i -= K - a;        // row a holds the K − a pairs (a, a + i)
    return pair_multiplier(t, a, a + i);
}
int64_t multiplier_bytes(const nufft_toeplitz* t, const Multiplier& m) { return grid_cells(t) * (int64_t)real_bytes(t->dtype) * (m.complex ? 2 : 1); }

template <typename T>
int upload_real(nufft_toeplitz* t, void** dst, const std::vector<double>& src) {
    std::vector<T> tmp(src.begin(), src.end());
    int rc = alloc(t, dst, tmp.size() * sizeof(T));
    if (rc) return rc;
    NUFFT_HIP(hipMemcpy(*dst, tmp.data(), tmp.size() * sizeof(T), hipMemcpyHostToDevice));
    return NUFFT_OK;
}
int upload(nufft_toeplitz* t, void** dst, const std::vector<double>& src) {
    return t->dtype == NUFFT_F32 ? upload_real<float>(t, dst, src) : upload_real<double>(t, dst, src);
}
int upload_i32(nufft_toeplitz* t, int32_t** dst, const std::vector<int32_t>& src) {
    int rc = alloc(t, reinterpret_cast<void**>(dst), src.size() * sizeof(int32_t));
    if (rc) return rc;
    NUFFT_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return NUFFT_OK;
}

void release(nufft_toeplitz* t) {
    if (!t) return;
    if (t->device >= 0) {
        DeviceGuard g(t->device);
        for (int d = 0; d < 3; ++d) {
            if (t->d_map[d]) (void)hipFree(t->d_map[d]);
            if (t->d_inv[d]) (void)hipFree(t->d_inv[d]);
            if (t->d_tw_fw[d]) (void)hipFree(t->d_tw_fw[d]);
            if (t->d_tw_bw[d]) (void)hipFree(t->d_tw_bw[d]);
        }
        for (void* p : {t->d_ones, t->d_K, t->d_tmpA, t->d_tmpB, t->d_work, t->d_fft_work, t->d_coil, t->d_kd, t->d_kc, t->d_grids, t->d_kf, t->d_sv, t->d_sw})
            if (p) (void)hipFree(p);
        if (t->fft_bw) (void)rocfft_plan_destroy(t->fft_bw);
        if (t->fft_fw) (void)rocfft_plan_destroy(t->fft_fw);
        if (t->fft_info) (void)rocfft_execution_info_destroy(t->fft_info);
    }
    delete t;
}

nufft::TzGrid grid_of(const nufft_toeplitz* t) {
    nufft::TzGrid g{};
    g.dtype = t->dtype;
    g.D = t->D;
    for (int d = 0; d < 3; ++d) {
        g.n2[d] = (int)t->N2[d];
        g.nk[d] = (int)t->N[d];
        g.map[d] = t->d_map[d];
        g.inv[d] = t->d_inv[d];
    }
    return g;
}

int build_device(nufft_toeplitz* t) {
    DeviceGuard guard(t->device);
    const size_t rb = real_bytes(t->dtype), cb = 2 * rb;
    const bool fused = t->path == NUFFT_TOEPLITZ_PATH_FUSED;
    int rc;
    if ((rc = alloc(t, &t->d_K, (size_t)grid_cells(t) * rb))) return rc;
    if (fused) {
        if (t->D == 3 && (rc = alloc(t, &t->d_tmpA, (size_t)(t->N[0] * t->N[1] * t->N2[2]) * cb))) return rc;
        if ((rc = alloc(t, &t->d_tmpB, (size_t)(t->N[0] * t->N2[1] * t->N2[2]) * cb))) return rc;
    } else {
        if ((rc = alloc(t, &t->d_work, (size_t)grid_cells(t) * cb))) return rc;
    }
    int64_t nmax = 1;
    for (int d = 0; d < 3; ++d) {
        if ((rc = upload_i32(t, &t->d_map[d], t->map[d])) || (rc = upload_i32(t, &t->d_inv[d], t->inv[d]))) return rc;
        nmax = std::max(nmax, t->N[d]);
        if (!fused || d >= t->D) continue;
        const int64_t n = t->N2[d];
        std::vector<double> twf(2 * (size_t)n), twb(2 * (size_t)n);
        for (int64_t m = 0; m < n; ++m) {
            const double ang = 2.0 * M_PI * (double)m / (double)n;
            twf[2 * m] = std::cos(ang); twf[2 * m + 1] = -std::sin(ang);
            twb[2 * m] = std::cos(ang); twb[2 * m + 1] = std::sin(ang);
        }
        if ((rc = upload(t, &t->d_tw_fw[d], twf))) return rc;
        if (d > 0 && (rc = upload(t, &t->d_tw_bw[d], twb))) return rc;
    }
    if (fused && (rc = upload(t, &t->d_ones, std::vector<double>((size_t)nmax, 1.0)))) return rc;

    size_t lengths[3] = {1, 1, 1};
    for (int d = 0; d < t->D; ++d) lengths[d] = (size_t)t->N2[d];
    const rocfft_precision prec = t->dtype == NUFFT_F32 ? rocfft_precision_single : rocfft_precision_double;
    NUFFT_ROCFFT(rocfft_execution_info_create(&t->fft_info));
    NUFFT_ROCFFT(rocfft_plan_create(&t->fft_bw, rocfft_placement_inplace, rocfft_transform_type_complex_inverse, prec, (size_t)t->D, lengths, 1, nullptr));
    NUFFT_ROCFFT(rocfft_plan_get_work_buffer_size(t->fft_bw, &t->fft_work_bytes));
    if (!fused) {
        size_t wf = 0;
        NUFFT_ROCFFT(rocfft_plan_create(&t->fft_fw, rocfft_placement_inplace, rocfft_transform_type_complex_forward, prec, (size_t)t->D, lengths, 1, nullptr));
        NUFFT_ROCFFT(rocfft_plan_get_work_buffer_size(t->fft_fw, &wf));
        t->fft_work_bytes = std::max(t->fft_work_bytes, wf);
        if (t->fft_work_bytes > 0) {
            if ((rc = alloc(t, &t->d_fft_work, t->fft_work_bytes))) return rc;
            NUFFT_ROCFFT(rocfft_execution_info_set_work_buffer(t->fft_info, t->d_fft_work, t->fft_work_bytes));
        }
    }
    return NUFFT_OK;
}

// K from the spectrum held in `grid` (complex<T>[2N...], overwritten): Nyquist planes zeroed, backward transform, scaled real part.
// `src` may be `grid` itself.  `K`: where the multiplier goes; a complex one (K_ab, a < b) keeps the scaled complex value.
int multiplier_from(nufft_toeplitz* t, Multiplier K, void* grid, const void* src, hipStream_t stream) {
    const nufft::TzGrid g = grid_of(t);
    NUFFT_HIP(nufft::launch_tz_spectrum_load(g, grid, src, t->num_cus, stream));
    NUFFT_ROCFFT(rocfft_execution_info_set_stream(t->fft_info, stream));
    void* io[1] = {grid};
    NUFFT_ROCFFT(rocfft_execute(t->fft_bw, io, nullptr, t->fft_info));
    const double scale = 1.0 / (double)grid_cells(t);
    if (K.complex) NUFFT_HIP(nufft::launch_tz_complex_part(g, K.ptr, grid, scale, t->num_cus, stream));
    else NUFFT_HIP(nufft::launch_tz_real_part(g, K.ptr, grid, scale, t->num_cus, stream));
    return NUFFT_OK;
}

// The fused path's temporaries of set_spectrum / set_points: the (2N)^D complex grid and rocFFT's work buffer.
struct Scratch {
    nufft_toeplitz* t;
    void* grid = nullptr;
    void* fft_work = nullptr;
    explicit Scratch(nufft_toeplitz* tz) : t(tz) {}
    int acquire_grid() {
        if (t->path != NUFFT_TOEPLITZ_PATH_FUSED) { grid = t->d_work; return NUFFT_OK; }
        return alloc(t, &grid, (size_t)grid_cells(t) * 2 * real_bytes(t->dtype));
    }
    int acquire_fft_work() {
        if (t->path != NUFFT_TOEPLITZ_PATH_FUSED || t->fft_work_bytes == 0) return NUFFT_OK;
        int rc = alloc(t, &fft_work, t->fft_work_bytes);
        if (rc) return rc;
        if (rocfft_execution_info_set_work_buffer(t->fft_info, fft_work, t->fft_work_bytes) != rocfft_status_success)
            return fail(NUFFT_ERR_ROCFFT, "rocfft_execution_info_set_work_buffer failed");
        return NUFFT_OK;
    }
    ~Scratch() {
        if (t->path != NUFFT_TOEPLITZ_PATH_FUSED) return;
        free_buffer(t->own_bytes, grid, (size_t)grid_cells(t) * 2 * real_bytes(t->dtype));
        free_buffer(t->own_bytes, fft_work, t->fft_work_bytes);
    }
};

// One pruned strided pass of the fused apply along dimension `dim` (1 or 2, zero-based): backward = kept modes in, full line out.
// `smap` (the outermost pass only: its pruned side is the caller's array): the coil's map, see FftLinePass::cmap.
int strided_pass(const nufft_toeplitz* t, int dim, bool forward, const void* in, void* out, hipStream_t stream, const void* smap = nullptr,
                 bool accumulate = false) {
    // pruned side: N_dim kept modes; full side: 2 N_dim.  Columns: dimension 1 (and 2 for the pass along dimension 3) of the KEPT
    // modes; the outer index of the pass along dimension 2 of a 3-D grid is the full dimension 3.
    nufft::FftLinePass q{};
    q.in = in;
    q.out = out;
    q.map = t->d_map[dim];
    q.nk = (int)t->N[dim];
    q.twiddle = forward ? t->d_tw_fw[dim] : t->d_tw_bw[dim];
    q.fa = t->d_ones; q.ka = 1;
    q.fk = t->d_ones;
    q.scale = 1.0;
    q.mult = nullptr;
    q.cmap = smap;
    q.accumulate = accumulate;
    const int64_t N1 = t->N[0];
    if (dim == 2) {
        q.a_total = q.a_out = N1 * t->N[1];
        q.in_stride_j = q.out_stride_j = N1 * t->N[1];
        q.in_stride_c = q.out_stride_c = 0;
        q.nc = 1;
    } else {
        q.a_total = q.a_out = N1;
        q.in_stride_j = q.out_stride_j = N1;
        q.nc = (int)t->N2[2];
        const int64_t pruned_c = N1 * t->N[1], full_c = N1 * t->N2[1];
        q.in_stride_c = forward ? full_c : pruned_c;
        q.out_stride_c = forward ? pruned_c : full_c;
    }
    NUFFT_HIP(nufft::launch_fft_lines(t->dtype, t->N2[dim], forward, q, stream));
    return NUFFT_OK;
}

// smap != null: out (+)= conj(S) ⊙ G (S ⊙ in), the map inside the two passes that touch the caller's arrays
// the strided passes before (in -> tmpB) and after (tmpB -> out) the dimension-1 kernel; tmpB: complex<T>[N_1, 2N_2, 2N_3]
int fused_backward(nufft_toeplitz* t, void* tmpB, const void* in, hipStream_t stream, const void* smap) {
    int rc;
    const void* src = in;
    if (t->D == 3) {
        if ((rc = strided_pass(t, 2, false, in, t->d_tmpA, stream, smap))) return rc;
        src = t->d_tmpA;
    }
    return strided_pass(t, 1, false, src, tmpB, stream, t->D == 3 ? nullptr : smap);
}
int fused_forward(nufft_toeplitz* t, void* out, const void* tmpB, hipStream_t stream, const void* smap, bool accumulate) {
    int rc;
    if (t->D == 3) {
        if ((rc = strided_pass(t, 1, true, tmpB, t->d_tmpA, stream))) return rc;
        return strided_pass(t, 2, true, t->d_tmpA, out, stream, smap, accumulate);
    }
    return strided_pass(t, 1, true, tmpB, out, stream, smap, accumulate);
}

// `K`: the multiplier of this component (d_K, or its frame's)
int apply_fused(nufft_toeplitz* t, const void* K, void* out, const void* in, hipStream_t stream, const void* smap = nullptr, bool accumulate = false) {
    if (int rc = fused_backward(t, t->d_tmpB, in, stream, smap)) return rc;
    NUFFT_HIP(nufft::launch_toeplitz_lines(t->dtype, t->N2[0], t->d_tmpB, K, t->N2[1] * t->N2[2], (int)t->N[0], t->d_map[0],
                                        t->d_tw_fw[0], stream));
    return fused_forward(t, out, t->d_tmpB, stream, smap, accumulate);
}

// The halves of an apply before and after the multiply, on either path.  `grid`: like d_tmpB (fused) or d_work (dense).
// backward: grid = backward transform of pad(map ⊙ src); forward: dst (+)= conj(map) ⊙ crop(forward transform of grid).  map = null:
// no product, and the forward half stores.
int backward_half(nufft_toeplitz* t, void* grid, const void* src, const void* map, hipStream_t stream) {
    if (t->path == NUFFT_TOEPLITZ_PATH_FUSED) return fused_backward(t, grid, src, stream, map);
    const nufft::TzGrid g = grid_of(t);
    void* io[1] = {grid};
    if (map) NUFFT_HIP(nufft::launch_tz_pad_map(g, grid, src, map, t->num_cus, stream));
    else NUFFT_HIP(nufft::launch_tz_pad(g, grid, src, t->num_cus, stream));
    NUFFT_ROCFFT(rocfft_execute(t->fft_bw, io, nullptr, t->fft_info));
    return NUFFT_OK;
}
int forward_half(nufft_toeplitz* t, void* dst, void* grid, const void* map, bool accumulate, hipStream_t stream) {
    if (t->path == NUFFT_TOEPLITZ_PATH_FUSED) return fused_forward(t, dst, grid, stream, map, accumulate);
    const nufft::TzGrid g = grid_of(t);
    void* io[1] = {grid};
    NUFFT_ROCFFT(rocfft_execute(t->fft_fw, io, nullptr, t->fft_info));
    if (map) NUFFT_HIP(nufft::launch_tz_crop_map(g, dst, grid, map, accumulate, t->num_cus, stream));
    else NUFFT_HIP(nufft::launch_tz_crop(g, dst, grid, t->num_cus, stream));
    return NUFFT_OK;
}

int apply_dense(nufft_toeplitz* t, const void* K, void* out, const void* in, hipStream_t stream, const void* smap = nullptr, bool accumulate = false) {
    if (int rc = backward_half(t, t->d_work, in, smap, stream)) return rc;
    NUFFT_HIP(nufft::launch_tz_multiply(grid_of(t), t->d_work, K, t->num_cus, stream));
    return forward_half(t, out, t->d_work, smap, accumulate, stream);
}

// One coil of G_S: out (+)= conj(S) ⊙ G (S ⊙ in), or the plain apply (smap = null).  The streaming route of the fused path expands
// into d_coil, runs the plain apply in place on it and combines into out.
int apply_coil(nufft_toeplitz* t, const void* K, void* out, const void* in, const void* smap, bool accumulate, hipStream_t stream) {
    if (t->path == NUFFT_TOEPLITZ_PATH_DENSE) return apply_dense(t, K, out, in, stream, smap, accumulate);
    if (t->maps_inpass || !smap) return apply_fused(t, K, out, in, stream, smap, accumulate);
    void* outs[1] = {t->d_coil};
    const void* maps[1] = {smap};
    const void* ins[1] = {t->d_coil};
    NUFFT_HIP(nufft::launch_coil_expand(t->dtype, num_modes(t), 1, outs, maps, in, t->num_cus, stream));
    if (int rc = apply_fused(t, K, t->d_coil, t->d_coil, stream)) return rc;
    NUFFT_HIP(nufft::launch_coil_combine(t->dtype, num_modes(t), 1, out, maps, ins, accumulate, t->num_cus, stream));
    return NUFFT_OK;
}

// One coil (or the plain operator, smap = null) of the coupled apply: out[a] (+)= conj(S) ⊙ Σ_b Toeplitz(T_ab) (S ⊙ in[b]).  All K
// backward halves first, each into its own intermediate, then the block multiply across them, then the K forward halves.
// `fold` (a segmented operator: its K factors): out[0] = Σ_a conj(B_a) ⊙ Σ_b Toeplitz(T_ab) (B_b ⊙ in[0]), segment 0 storing and the
// others adding in index order.
int apply_coupled(nufft_toeplitz* t, void* const* out, const void* const* in, const void* smap, bool accumulate, hipStream_t stream,
                  const void* const* fold = nullptr) {
    const size_t stride = coupled_grid_stride(t), cb = 2 * real_bytes(t->dtype);
    auto grid_at = [&](int c) { return static_cast<void*>(static_cast<char*>(t->d_grids) + (size_t)c * stride * cb); };
    const int K = inner(t);
    int rc;
    for (int b = 0; b < K; ++b)
        if ((rc = backward_half(t, grid_at(b), fold ? in[0] : in[b], fold ? fold[b] : smap, stream))) return rc;
    if (t->path == NUFFT_TOEPLITZ_PATH_FUSED)
        NUFFT_HIP(nufft::launch_toeplitz_lines_coupled(t->dtype, t->N2[0], K, t->d_grids, (int64_t)stride, t->d_kd, t->d_kc, t->N2[1] * t->N2[2],
                                                    (int)t->N[0], t->d_map[0], t->d_tw_fw[0], stream));
    else
        NUFFT_HIP(nufft::launch_tz_multiply_coupled(grid_of(t), t->d_grids, (int64_t)stride, K, t->d_kd, t->d_kc, t->num_cus, stream));
    for (int a = 0; a < K; ++a)
        if ((rc = forward_half(t, fold ? out[0] : out[a], grid_at(a), fold ? fold[a] : smap, fold ? a > 0 : accumulate, stream))) return rc;
    return NUFFT_OK;
}

// The segmented operator.  Without coil maps one folded pass from `in` into `out`; with them, per coil in index order, v = S_c ⊙ in,
// the folded pass from v into w, out (+)= conj(S_c) ⊙ w.
int apply_segmented(nufft_toeplitz* t, void* out, const void* in, hipStream_t stream) {
    const void* const* B = t->factors.data();
    const int ncoils = (int)t->coil_maps.size();
    if (ncoils == 0) {
        void* outs[1] = {out};
        const void* ins[1] = {in};
        return apply_coupled(t, outs, ins, nullptr, false, stream, B);
    }
    for (int c = 0; c < ncoils; ++c) {
        void* v[1] = {t->d_sv};
        void* w[1] = {t->d_sw};
        const void* vin[1] = {t->d_sv};
        const void* win[1] = {t->d_sw};
        const void* map[1] = {t->coil_maps[(size_t)c]};
        NUFFT_HIP(nufft::launch_coil_expand(t->dtype, num_modes(t), 1, v, map, in, t->num_cus, stream));
        if (int rc = apply_coupled(t, w, vin, nullptr, false, stream, B)) return rc;
        NUFFT_HIP(nufft::launch_coil_combine(t->dtype, num_modes(t), 1, out, map, win, c > 0, t->num_cus, stream));
    }
    return NUFFT_OK;
}

// What every coupled build checks before it touches the device, in the order of the header.
int coupled_refusals(const nufft_toeplitz* t, const char* fn) {
    const int K = inner(t);
    if (K > nufft::kMaxCoupled)
        return fail(NUFFT_ERR_UNSUPPORTED, std::string(fn) + ": at most " + std::to_string(nufft::kMaxCoupled) + " coupled components (ntransforms)");
    if (t->path == NUFFT_TOEPLITZ_PATH_FUSED && !nufft::toeplitz_lines_coupled_supported(t->dtype, t->N2[0], K))
        return fail(NUFFT_ERR_UNSUPPORTED, std::string(fn) + ": the " + std::to_string(K) + " lines of 2 N_1 = " + std::to_string(t->N2[0]) +
                                               " cells of a line id do not fit the LDS of one wave of the fused dimension-1 kernel; create the "
                                               "operator from a plan with the option NUFFT_TOEPLITZ_FUSED=0 (the dense path)");
    if (!t->seg && t->path == NUFFT_TOEPLITZ_PATH_FUSED && !t->maps_inpass && !t->coil_maps.empty())
        return fail(NUFFT_ERR_UNSUPPORTED, std::string(fn) + ": coil maps on the route NUFFT_TOEPLITZ_MAPS_INPASS=0 do not combine with coupled components");
    return NUFFT_OK;
}

// What a segmented operator has no use for: one shared multiplier or one per frame.
int segmented_refusal(const nufft_toeplitz* t, const char* fn) {
    if (!t->seg) return NUFFT_OK;
    return fail(NUFFT_ERR_UNSUPPORTED, std::string(fn) + ": the operator is segmented (nufft_toeplitz_create_segmented): its multiplier is the block of "
                                           "its segments, built by nufft_toeplitz_set_points_coupled / _set_spectra_coupled");
}

int host_only_refusal(const nufft_toeplitz* t) {
    return t->device < 0 ? fail(NUFFT_ERR_NO_DEVICE, "host-only Toeplitz object (device = -1)") : NUFFT_OK;
}

// `why`: what `fn` does that a capture cannot record.
int capture_refusal(hipStream_t stream, const char* fn, const char* why) {
    return capturing(stream) ? fail(NUFFT_ERR_INVALID_ARG, std::string(fn) + " " + why + ": not on a capturing stream") : NUFFT_OK;
}

// One point set as the point builds take it: `coords` has a vector per dimension unless there are no points.
int points_refusal(const nufft_toeplitz* t, int64_t np, const void* const* coords) {
    if (np < 0) return fail(NUFFT_ERR_INVALID_ARG, "negative number of points");
    if (!coords) return fail(NUFFT_ERR_INVALID_ARG, "null coordinate table");
    for (int d = 0; d < t->D; ++d)
        if (np > 0 && !coords[d]) return fail(NUFFT_ERR_INVALID_ARG, "null coordinate vector");
    return NUFFT_OK;
}

// A build and, on a segmented operator, the factors: what nufft_toeplitz_apply needs.
bool ready(const nufft_toeplitz* t) { return t->mode != MODE_NONE && (!t->seg || !t->factors.empty()); }

// The internal 2N plan's parameters: the parent plan's window unless `build` overrides it (nufft_toeplitz_set_points).
int build_plan_params(const nufft_toeplitz* t, const nufft_params* build, nufft_params& prm) {
    std::memset(&prm, 0, sizeof(prm));
    prm.struct_size = (int32_t)sizeof(prm);
    prm.dtype = t->dtype;
    prm.is_complex = 1;
    prm.ndim = t->D;
    for (int d = 0; d < t->D; ++d) prm.N[d] = t->N2[d];
    prm.half_support = t->M;
    prm.sigma = t->sigma_req;
    prm.kernel = t->kernel;
    prm.evalmode = t->evalmode;
    prm.ntransforms = 1;
    prm.fftshift = 0;
    prm.point_transform = t->point_transform;
    prm.device = t->device;
    prm.options = t->options.empty() ? nullptr : t->options.c_str();
    if (build) {        // the caller's window for the build: half_support and sigma where set, kernel / kernel_param / evalmode verbatim
        nufft_params b;
        std::memset(&b, 0, sizeof(b));
        const size_t known = build->struct_size > 0 ? (size_t)build->struct_size : offsetof(nufft_params, kernel_param_dim);
        if (known < offsetof(nufft_params, kernel_param_dim)) return fail(NUFFT_ERR_INVALID_ARG, "nufft_params.struct_size is smaller than any published layout");
        std::memcpy(&b, build, std::min(known, sizeof(b)));
        if (b.half_support > 0) prm.half_support = b.half_support;
        if (b.sigma > 0) prm.sigma = b.sigma;
        prm.kernel = b.kernel;
        prm.kernel_param = b.kernel_param;
        prm.evalmode = b.evalmode;
    }
    return NUFFT_OK;
}

size_t coil_scratch_bytes(const nufft_toeplitz* t) { return (size_t)num_modes(t) * 2 * real_bytes(t->dtype); }

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The two scratch arrays of a segmented operator with coil maps: held exactly while maps and factors are both set.
int acquire_segment_scratch(nufft_toeplitz* t, const char* fn, void* stream_) {
    if (!t->seg || t->coil_maps.empty() || t->factors.empty() || t->d_sv) return NUFFT_OK;
    DeviceGuard guard(t->device);
    int rc;
    if ((rc = capture_refusal(static_cast<hipStream_t>(stream_), fn, "allocates the two scratch arrays of a segmented operator with coil maps"))) return rc;
    if ((rc = alloc(t, &t->d_sv, coil_scratch_bytes(t))) || (rc = alloc(t, &t->d_sw, coil_scratch_bytes(t)))) {
        free_buffer(t->own_bytes, t->d_sv, coil_scratch_bytes(t));
        return rc;
    }
    return NUFFT_OK;
}
void drop_segment_scratch(nufft_toeplitz* t) {
    if (!t->d_sv && !t->d_sw) return;
    DeviceGuard guard(t->device);
    free_buffer(t->own_bytes, t->d_sv, coil_scratch_bytes(t));      // hipFree waits for the applies in flight
    free_buffer(t->own_bytes, t->d_sw, coil_scratch_bytes(t));
}

// A build from spectra: T[i] is the spectrum of the mode's i-th multiplier (multiplier_at).
int build_from_spectra(nufft_toeplitz* t, Mode mode, const void* const* T, hipStream_t stream) {
    int rc;
    if ((rc = begin_build(t, mode))) return rc;
    Scratch s(t);
    if ((rc = s.acquire_grid()) || (rc = s.acquire_fft_work())) return rc;
    for (int i = 0; i < num_multipliers(t, mode); ++i)
        if ((rc = multiplier_from(t, multiplier_at(t, mode, i), s.grid, T[i], stream))) return rc;
    NUFFT_HIP(hipStreamSynchronize(stream));      // the temporaries are freed on return
    t->mode = mode;
    return NUFFT_OK;
}

// What a build from points spreads for the mode's i-th multiplier.
struct PointItem {
    const void* const* coords;      // the point set to bind first, or null: the one the item before left bound
    int64_t np;
    const void* weights;            // null: ones
    bool pair;                      // values = w conj(φ_a) φ_b (launch_tz_pair_weights); false: values = w (launch_tz_weights)
    const void *phi_a, *phi_b;
};

// The prefix of a failed build from points, [mode][the failure lies in the plan, its points or the type 1].
const char* const kBuildPrefix[][2] = {
    {"", ""},
    {"Toeplitz build (type 1 of the weights on the 2N grid): ", "Toeplitz build (type 1 of the weights on the 2N grid): "},
    {"coupled Toeplitz build: ", "coupled Toeplitz build (type 1 of a pair's weights on the 2N grid): "},
    {"framed Toeplitz build: ", "framed Toeplitz build (type 1 of a frame's weights on the 2N grid): "}};

// A build from points with an internal 2N plan that lives inside this call: per multiplier the type 1 of `values` (of at most `most`
// points) onto the scratch grid, then multiplier_from in place.
int build_from_points(nufft_toeplitz* t, Mode mode, const nufft_params* build, const PointItem* items, int64_t most, hipStream_t stream) {
    nufft_params prm;
    const int refused = build_plan_params(t, build, prm);      // reads `t` only; refused parameters end the build in force all the same
    int rc;
    if ((rc = begin_build(t, mode, !refused))) return rc;
    if (refused) return refused;
    // The one place the modes differ.  A plain build has a single multiplier, so it transforms it after the 2N plan is destroyed and
    // takes rocFFT's work buffer only then: the two never coexist.  The others transform every multiplier while the plan exists, so
    // the work buffer lives next to it from the start.
    const bool late = mode == MODE_PLAIN;
    Scratch s(t);
    if ((rc = s.acquire_grid()) || (!late && (rc = s.acquire_fft_work()))) return rc;
    void* values = nullptr;
    const size_t vbytes = (size_t)most * 2 * real_bytes(t->dtype);
    if ((rc = alloc(t, &values, vbytes))) return rc;
    nufft_plan* bp = nullptr;
    rc = nufft_plan_create_ex(&bp, &prm);
    bool in_type1 = true;
    for (int i = 0; i < num_multipliers(t, mode) && rc == NUFFT_OK; ++i) {
        const PointItem& it = items[i];
        in_type1 = true;
        if (it.coords) {
            t->build_bytes = bp->workspace_bytes;
            rc = nufft_set_points(bp, it.np, it.coords, stream);
            t->build_bytes = bp->workspace_bytes;
            // a coupled build binds its one point set ahead of its pairs: a failure there keeps the type-1 prefix, where a framed
            // build, which binds a set per frame, has always reported the short one
            if (rc && mode == MODE_COUPLED) break;
        }
        if (rc == NUFFT_OK) {
            hipError_t e = it.pair ? nufft::launch_tz_pair_weights(t->dtype, values, it.weights, it.phi_a, it.phi_b, it.np, t->num_cus, stream)
                                   : nufft::launch_tz_weights(t->dtype, values, it.weights, it.np, t->num_cus, stream);
            if (e != hipSuccess) rc = fail(NUFFT_ERR_HIP, std::string(it.pair ? "launch_tz_pair_weights: " : "launch_tz_weights: ") + hipGetErrorString(e));
        }
        if (rc == NUFFT_OK) {
            void* outs[1] = {s.grid};
            const void* ins[1] = {values};
            rc = nufft_exec_type1(bp, outs, ins, stream);
        }
        in_type1 = false;
        if (rc == NUFFT_OK && !late) rc = multiplier_from(t, multiplier_at(t, mode, i), s.grid, s.grid, stream);
    }
    if (rc == NUFFT_OK && hipStreamSynchronize(stream) != hipSuccess) rc = fail(NUFFT_ERR_HIP, "hipStreamSynchronize failed");
    const std::string keep = rc ? nufft_last_error_message() : "";
    if (bp) nufft_plan_destroy(bp);
    t->build_bytes = 0;
    free_buffer(t->own_bytes, values, vbytes);
    if (rc) return fail(rc, kBuildPrefix[mode][in_type1] + keep);
    if (late) {
        if ((rc = s.acquire_fft_work())) return rc;
        if ((rc = multiplier_from(t, multiplier_at(t, mode, 0), s.grid, s.grid, stream))) return rc;
        NUFFT_HIP(hipStreamSynchronize(stream));
    }
    t->mode = mode;
    return NUFFT_OK;
}

int create(nufft_toeplitz** out, const nufft_plan* plan, int nsegments);

}  // namespace

const std::vector<const void*>& nufft::toeplitz_coil_maps(const nufft_toeplitz* t) { return t->coil_maps; }

extern "C" {

int64_t nufft_sizeof_toeplitz_info(void) { return (int64_t)sizeof(nufft_toeplitz_info); }

int nufft_toeplitz_create(nufft_toeplitz** out, const nufft_plan* plan) { return create(out, plan, 0); }

int nufft_toeplitz_create_segmented(nufft_toeplitz** out, const nufft_plan* plan, int32_t nsegments) {
    if (!out || !plan) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (nsegments < 1) return fail(NUFFT_ERR_INVALID_ARG, "nufft_toeplitz_create_segmented: nsegments = " + std::to_string(nsegments) + " must be at least 1");
    if (nsegments > nufft::kMaxCoupled)
        return fail(NUFFT_ERR_UNSUPPORTED, "nufft_toeplitz_create_segmented: at most " + std::to_string(nufft::kMaxCoupled) + " segments");
    return create(out, plan, nsegments);
}

}  // extern "C"

namespace {
// nsegments = 0: an ordinary operator
int create(nufft_toeplitz** out, const nufft_plan* plan, int nsegments) {
    if (!out || !plan) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!plan->is_complex)
        return fail(NUFFT_ERR_UNSUPPORTED,
                    "the Toeplitz normal operator needs a complex plan: the type 2 of a real-data plan extends its half spectrum "
                    "Hermitian-ly, which for even N adds the mode +N/2 next to -N/2; mode differences then reach +-N and the 2N "
                    "embedding aliases");
    for (int d = 0; d < plan->D; ++d)
        if (plan->N[d] > ((int64_t)1 << 29)) return fail(NUFFT_ERR_UNSUPPORTED, "2 N exceeds 2^30 cells per axis");
    if (nsegments > 0 && plan->C != 1)
        return fail(NUFFT_ERR_INVALID_ARG, "nufft_toeplitz_create_segmented: a segmented operator has one component outside: the plan must have "
                                           "ntransforms = 1 (got " + std::to_string(plan->C) + ")");
    nufft_toeplitz* t = new (std::nothrow) nufft_toeplitz();
    if (!t) return fail(NUFFT_ERR_ALLOC, "out of host memory");
    t->dtype = plan->dtype;
    t->D = plan->D;
    t->C = plan->C;
    t->seg = nsegments;
    t->device = plan->device;
    t->num_cus = plan->num_cus;
    t->fftshift = plan->fftshift;
    t->M = plan->M;
    t->kernel = plan->kernel;
    t->evalmode = plan->evalmode;
    t->point_transform = plan->point_transform;
    t->sigma_req = plan->sigma_req;
    t->options = plan->opts.str();
    bool fused = plan->D >= 2 && plan->opts.option_int("NUFFT_TOEPLITZ_FUSED", 1) != 0;
    t->maps_inpass = plan->opts.option_int("NUFFT_TOEPLITZ_MAPS_INPASS", 1) != 0;
    for (int d = 0; d < 3; ++d) {
        const bool in = d < plan->D;
        t->N[d] = in ? plan->N[d] : 1;
        t->N2[d] = in ? 2 * plan->N[d] : 1;
        if (in) {
            // mode k of the plan's mode order -> cell k mod 2N of the embedding grid (the same rule that places the kept modes in
            // the oversampled spectrum)
            std::vector<double> ks;
            std::vector<int64_t> m64;
            nufft::wavenumbers(t->N[d], false, ks);
            nufft::non_oversampled_indices(ks, t->N2[d], t->fftshift, m64);
            t->map[d].assign(m64.begin(), m64.end());
            fused = fused && nufft::fft_lines_supported(t->dtype, t->N2[d]) && nufft::toeplitz_lines_supported(t->dtype, t->N2[d]);
        } else {
            t->map[d].assign(1, 0);
        }
        t->inv[d].assign((size_t)t->N2[d], -1);
        for (size_t k = 0; k < t->map[d].size(); ++k) t->inv[d][(size_t)t->map[d][k]] = (int32_t)k;
    }
    t->path = fused ? NUFFT_TOEPLITZ_PATH_FUSED : NUFFT_TOEPLITZ_PATH_DENSE;
    if (t->seg > 0) {
        if (int rc = coupled_refusals(t, "nufft_toeplitz_create_segmented")) {
            const std::string keep = nufft_last_error_message();
            release(t);
            return fail(rc, keep);
        }
    }
    if (t->device >= 0) {
        const int rc = build_device(t);
        if (rc) {
            const std::string keep = nufft_last_error_message();
            release(t);
            return fail(rc, keep);
        }
    }
    *out = t;
    return NUFFT_OK;
}
}  // namespace

extern "C" {

int nufft_toeplitz_destroy(nufft_toeplitz* t) {
    release(t);
    return NUFFT_OK;
}

int nufft_toeplitz_get_info(const nufft_toeplitz* t, nufft_toeplitz_info* o) {
    if (!t || !o) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    nufft_toeplitz_info i;
    std::memset(&i, 0, sizeof(i));
    i.ndim = t->D;
    i.dtype = t->dtype;
    i.ntransforms = t->C;
    i.fftshift = t->fftshift;
    i.device = t->device;
    i.path = t->path;
    i.has_spectrum = ready(t);
    for (int d = 0; d < 3; ++d) { i.N[d] = t->N[d]; i.N2[d] = t->N2[d]; }
    i.multiplier_bytes = grid_cells(t) * (int64_t)real_bytes(t->dtype);
    i.workspace_bytes = t->device >= 0 ? t->own_bytes + t->build_bytes : (int64_t)sizes_of(t).total();
    write_info(o, i);
    return NUFFT_OK;
}

int nufft_toeplitz_multiplier_ptr(const nufft_toeplitz* t, void** out_ptr, int64_t* out_bytes) {
    if (!t || !out_ptr) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (int rc = segmented_refusal(t, "nufft_toeplitz_multiplier_ptr")) return rc;
    if (int rc = host_only_refusal(t)) return rc;
    *out_ptr = t->d_K;
    if (out_bytes) *out_bytes = grid_cells(t) * (int64_t)real_bytes(t->dtype);
    return NUFFT_OK;
}

// The six builds: the checks of each in the order of the header, then build_from_spectra or build_from_points.

int nufft_toeplitz_set_spectrum(nufft_toeplitz* t, const void* T_modes, void* stream_) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = segmented_refusal(t, "nufft_toeplitz_set_spectrum")) || (rc = host_only_refusal(t))) return rc;
    if (!T_modes) return fail(NUFFT_ERR_INVALID_ARG, "null spectrum");
    DeviceGuard guard(t->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = capture_refusal(stream, "nufft_toeplitz_set_spectrum", "allocates and synchronises"))) return rc;
    return build_from_spectra(t, MODE_PLAIN, &T_modes, stream);
}

int nufft_toeplitz_set_points(nufft_toeplitz* t, const nufft_params* build, int64_t np, const void* const* coords, const void* weights,
                              void* stream_) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = segmented_refusal(t, "nufft_toeplitz_set_points")) || (rc = host_only_refusal(t)) || (rc = points_refusal(t, np, coords))) return rc;
    DeviceGuard guard(t->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = capture_refusal(stream, "nufft_toeplitz_set_points", "builds and destroys a plan"))) return rc;
    const PointItem item{coords, np, weights, false, nullptr, nullptr};
    return build_from_points(t, MODE_PLAIN, build, &item, std::max<int64_t>(np, 1), stream);
}

int nufft_toeplitz_set_spectra_coupled(nufft_toeplitz* t, const void* const* T_pairs, void* stream_) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (!T_pairs) return fail(NUFFT_ERR_INVALID_ARG, "null table of spectra");
    int rc;
    if ((rc = host_only_refusal(t))) return rc;
    for (int p = 0; p < num_multipliers(t, MODE_COUPLED); ++p)
        if (!T_pairs[p]) return fail(NUFFT_ERR_INVALID_ARG, "null spectrum");
    if ((rc = coupled_refusals(t, "nufft_toeplitz_set_spectra_coupled"))) return rc;
    DeviceGuard guard(t->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = capture_refusal(stream, "nufft_toeplitz_set_spectra_coupled", "allocates and synchronises"))) return rc;
    return build_from_spectra(t, MODE_COUPLED, T_pairs, stream);
}

int nufft_toeplitz_set_points_coupled(nufft_toeplitz* t, const nufft_params* build, int64_t np, const void* const* coords, const void* weights,
                                      const void* const* basis, void* stream_) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (!basis) return fail(NUFFT_ERR_INVALID_ARG, "null table of basis functions");
    int rc;
    if ((rc = host_only_refusal(t)) || (rc = points_refusal(t, np, coords))) return rc;
    const int K = inner(t);
    for (int c = 0; c < K; ++c)
        if (np > 0 && (!basis[c] || !aligned16(basis[c]))) return fail(NUFFT_ERR_INVALID_ARG, "null or not 16-byte aligned basis function");
    if ((rc = coupled_refusals(t, "nufft_toeplitz_set_points_coupled"))) return rc;
    DeviceGuard guard(t->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = capture_refusal(stream, "nufft_toeplitz_set_points_coupled", "builds and destroys a plan"))) return rc;
    std::vector<PointItem> items;
    for (int a = 0; a < K; ++a)
        for (int b = a; b < K; ++b) items.push_back({items.empty() ? coords : nullptr, np, weights, true, basis[a], basis[b]});      // one point set for all pairs
    return build_from_points(t, MODE_COUPLED, build, items.data(), std::max<int64_t>(np, 1), stream);
}

int nufft_toeplitz_set_spectra_frames(nufft_toeplitz* t, const void* const* T, void* stream_) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = segmented_refusal(t, "nufft_toeplitz_set_spectra_frames"))) return rc;
    if (!T) return fail(NUFFT_ERR_INVALID_ARG, "null table of spectra");
    if ((rc = host_only_refusal(t))) return rc;
    for (int c = 0; c < t->C; ++c)
        if (!T[c]) return fail(NUFFT_ERR_INVALID_ARG, "null spectrum");
    DeviceGuard guard(t->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = capture_refusal(stream, "nufft_toeplitz_set_spectra_frames", "allocates and synchronises"))) return rc;
    return build_from_spectra(t, MODE_FRAMED, T, stream);
}

int nufft_toeplitz_set_points_frames(nufft_toeplitz* t, const nufft_params* build, const int64_t* np, const void* const* coords,
                                     const void* const* weights, void* stream_) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = segmented_refusal(t, "nufft_toeplitz_set_points_frames"))) return rc;
    if (!np || !coords) return fail(NUFFT_ERR_INVALID_ARG, "null table of point counts or coordinates");
    if ((rc = host_only_refusal(t))) return rc;
    int64_t most = 1;
    std::vector<PointItem> items;
    for (int c = 0; c < t->C; ++c) {
        if ((rc = points_refusal(t, np[c], coords + (size_t)c * t->D))) return rc;
        most = std::max(most, np[c]);
        items.push_back({coords + (size_t)c * t->D, np[c], weights ? weights[c] : nullptr, false, nullptr, nullptr});
    }
    DeviceGuard guard(t->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if ((rc = capture_refusal(stream, "nufft_toeplitz_set_points_frames", "builds and destroys a plan"))) return rc;
    return build_from_points(t, MODE_FRAMED, build, items.data(), most, stream);
}

int32_t nufft_toeplitz_num_frames(const nufft_toeplitz* t) { return t && t->mode == MODE_FRAMED ? (int32_t)t->C : 0; }

int nufft_toeplitz_multiplier_frame_ptr(const nufft_toeplitz* t, int32_t c, void** out_ptr, int64_t* out_bytes) {
    if (!t || !out_ptr) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (int rc = host_only_refusal(t)) return rc;
    if (t->mode != MODE_FRAMED) return fail(NUFFT_ERR_INVALID_ARG, "nufft_toeplitz_multiplier_frame_ptr: no framed build is in force");
    if (c < 0 || c >= t->C) return fail(NUFFT_ERR_INVALID_ARG, "nufft_toeplitz_multiplier_frame_ptr: the frame must satisfy 0 <= c < ntransforms");
    const Multiplier m = multiplier_at(t, MODE_FRAMED, c);
    *out_ptr = m.ptr;
    if (out_bytes) *out_bytes = multiplier_bytes(t, m);
    return NUFFT_OK;
}

int32_t nufft_toeplitz_num_coupled(const nufft_toeplitz* t) { return t && t->mode == MODE_COUPLED && !t->seg ? (int32_t)t->C : 0; }

int32_t nufft_toeplitz_num_segments(const nufft_toeplitz* t) { return t ? (int32_t)t->seg : 0; }

int nufft_toeplitz_multiplier_pair_ptr(const nufft_toeplitz* t, int32_t a, int32_t b, void** out_ptr, int64_t* out_bytes) {
    if (!t || !out_ptr) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (int rc = host_only_refusal(t)) return rc;
    if (t->mode != MODE_COUPLED) return fail(NUFFT_ERR_INVALID_ARG, "nufft_toeplitz_multiplier_pair_ptr: no coupled build is in force");
    if (a < 0 || b < a || b >= inner(t))
        return fail(NUFFT_ERR_INVALID_ARG, "nufft_toeplitz_multiplier_pair_ptr: the pair must satisfy 0 <= a <= b < ntransforms (segmented: nsegments)");
    const Multiplier m = pair_multiplier(t, a, b);
    *out_ptr = m.ptr;
    if (out_bytes) *out_bytes = multiplier_bytes(t, m);
    return NUFFT_OK;
}

int nufft_toeplitz_apply(nufft_toeplitz* t, void* const* out, const void* const* in, void* stream_) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (int rc = host_only_refusal(t)) return rc;
    if (t->seg && !ready(t))
        return fail(NUFFT_ERR_NO_POINTS, "a coupled build (nufft_toeplitz_set_points_coupled / _set_spectra_coupled) and nufft_toeplitz_set_factors must "
                                         "both be in force before nufft_toeplitz_apply on a segmented operator");
    if (t->mode == MODE_NONE) return fail(NUFFT_ERR_NO_POINTS, "nufft_toeplitz_set_spectrum or nufft_toeplitz_set_points must be called before nufft_toeplitz_apply");
    if (!out || !in) return fail(NUFFT_ERR_INVALID_ARG, "null table");
    for (int c = 0; c < t->C; ++c)
        if (!out[c] || !in[c]) return fail(NUFFT_ERR_INVALID_ARG, "null data vector");
    DeviceGuard guard(t->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (t->path == NUFFT_TOEPLITZ_PATH_DENSE) NUFFT_ROCFFT(rocfft_execution_info_set_stream(t->fft_info, stream));
    const int ncoils = (int)t->coil_maps.size();
    if (t->seg) {
        if (out[0] == in[0]) return fail(NUFFT_ERR_INVALID_ARG, "nufft_toeplitz_apply on a segmented operator: the output array is also the input array");
        return apply_segmented(t, out[0], in[0], stream);
    }
    const bool coupled = t->mode == MODE_COUPLED;
    if (ncoils > 0 || coupled) {       // coil 0 stores into out[c] what coil 1 still has to read from in[c']; coupled: every output needs every input
        for (int c = 0; c < t->C; ++c)
            for (int c2 = 0; c2 < t->C; ++c2)
                if (out[c] == in[c2])
                    return fail(NUFFT_ERR_INVALID_ARG, ncoils > 0 ? "nufft_toeplitz_apply with coil maps set: an output array is also an input array"
                                                                  : "nufft_toeplitz_apply on coupled components: an output array is also an input array");
    }
    // The passes over the coil maps: without maps one pass with a null map that stores, with maps one per coil, accumulating from the
    // second coil on.
    const int passes = std::max(ncoils, 1);
    auto map_of = [&](int s) -> const void* { return ncoils ? t->coil_maps[(size_t)s] : nullptr; };
    int rc = NUFFT_OK;
    if (coupled) {
        for (int s = 0; s < passes && !rc; ++s) rc = apply_coupled(t, out, in, map_of(s), s > 0, stream);
        return rc;
    }
    for (int c = 0; c < t->C && !rc; ++c) {
        const void* K = multiplier_at(t, t->mode, c).ptr;      // the frame's, or d_K for every component
        for (int s = 0; s < passes && !rc; ++s) rc = apply_coil(t, K, out[c], in[c], map_of(s), s > 0, stream);
    }
    return rc;
}

int nufft_toeplitz_set_maps(nufft_toeplitz* t, int32_t ncoils, const void* const* maps, void* stream_) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (!maps) return fail(NUFFT_ERR_INVALID_ARG, "null table of coil maps");
    if (ncoils < 1 || ncoils > 1024) return fail(NUFFT_ERR_INVALID_ARG, "the number of coils must lie in 1 ... 1024");
    int rc;
    if ((rc = host_only_refusal(t))) return rc;
    for (int32_t c = 0; c < ncoils; ++c) {
        if (!maps[c]) return fail(NUFFT_ERR_INVALID_ARG, "null coil map");
        if (!aligned16(maps[c])) return fail(NUFFT_ERR_INVALID_ARG, "coil maps must be 16-byte aligned");
    }
    if (t->mode == MODE_COUPLED && !t->seg && t->path == NUFFT_TOEPLITZ_PATH_FUSED && !t->maps_inpass)
        return fail(NUFFT_ERR_UNSUPPORTED, "nufft_toeplitz_set_maps: coil maps on the route NUFFT_TOEPLITZ_MAPS_INPASS=0 do not combine with coupled components");
    if (!t->seg && t->path == NUFFT_TOEPLITZ_PATH_FUSED && !t->maps_inpass && !t->d_coil) {
        DeviceGuard guard(t->device);
        if ((rc = capture_refusal(static_cast<hipStream_t>(stream_), "nufft_toeplitz_set_maps", "allocates on the streaming route"))) return rc;
        if ((rc = alloc(t, &t->d_coil, coil_scratch_bytes(t)))) return rc;
    }
    const std::vector<const void*> before = t->coil_maps;
    t->coil_maps.assign(maps, maps + ncoils);
    if ((rc = acquire_segment_scratch(t, "nufft_toeplitz_set_maps", stream_))) {
        t->coil_maps = before;
        return rc;
    }
    return NUFFT_OK;
}

int nufft_toeplitz_clear_maps(nufft_toeplitz* t) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    t->coil_maps.clear();
    drop_segment_scratch(t);
    if (t->d_coil) {
        DeviceGuard guard(t->device);
        free_buffer(t->own_bytes, t->d_coil, coil_scratch_bytes(t));      // hipFree waits for the applies in flight
    }
    return NUFFT_OK;
}

int32_t nufft_toeplitz_num_coils(const nufft_toeplitz* t) { return t ? (int32_t)t->coil_maps.size() : 0; }

int nufft_toeplitz_set_factors(nufft_toeplitz* t, const void* const* B, void* stream_) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    if (!t->seg) return fail(NUFFT_ERR_INVALID_ARG, "nufft_toeplitz_set_factors: the operator is not segmented (nufft_toeplitz_create_segmented)");
    if (!B) return fail(NUFFT_ERR_INVALID_ARG, "null table of factors");
    if (int rc = host_only_refusal(t)) return rc;
    for (int l = 0; l < t->seg; ++l) {
        if (!B[l]) return fail(NUFFT_ERR_INVALID_ARG, "null factor");
        if (!aligned16(B[l])) return fail(NUFFT_ERR_INVALID_ARG, "the factors must be 16-byte aligned");
    }
    const std::vector<const void*> before = t->factors;
    t->factors.assign(B, B + t->seg);
    if (int rc = acquire_segment_scratch(t, "nufft_toeplitz_set_factors", stream_)) {
        t->factors = before;
        return rc;
    }
    return NUFFT_OK;
}

int nufft_toeplitz_clear_factors(nufft_toeplitz* t) {
    if (!t) return fail(NUFFT_ERR_INVALID_ARG, "null argument");
    t->factors.clear();
    drop_segment_scratch(t);
    return NUFFT_OK;
}

namespace {
int coil_args(int dtype, int64_t n, int32_t ncoils, const void* const* a, const void* const* b, const void* single) {
    if (dtype != NUFFT_F32 && dtype != NUFFT_F64) return fail(NUFFT_ERR_INVALID_ARG, "dtype must be NUFFT_F32 or NUFFT_F64");
    if (n < 0) return fail(NUFFT_ERR_INVALID_ARG, "negative number of elements");
    if (ncoils < 1 || ncoils > 1024) return fail(NUFFT_ERR_INVALID_ARG, "the number of coils must lie in 1 ... 1024");
    if (!a || !b) return fail(NUFFT_ERR_INVALID_ARG, "null table");
    if (n == 0) return NUFFT_OK;
    if (!single || !aligned16(single)) return fail(NUFFT_ERR_INVALID_ARG, "null or not 16-byte aligned array");
    for (int32_t c = 0; c < ncoils; ++c)
        if (!a[c] || !b[c] || !aligned16(a[c]) || !aligned16(b[c])) return fail(NUFFT_ERR_INVALID_ARG, "null or not 16-byte aligned coil array");
    return NUFFT_OK;
}

int device_cus(int device, int* num_cus) {
    NUFFT_HIP(hipDeviceGetAttribute(num_cus, hipDeviceAttributeMultiprocessorCount, device));
    return NUFFT_OK;
}
}  // namespace

int nufft_coil_expand(int dtype, int64_t n, int32_t ncoils, void* const* out, const void* const* maps, const void* in, int device, void* stream) {
    if (device < 0) return fail(NUFFT_ERR_NO_DEVICE, "nufft_coil_expand needs a device");
    if (int rc = coil_args(dtype, n, ncoils, out, maps, in)) return rc;
    if (n == 0) return NUFFT_OK;
    DeviceGuard guard(device);
    int cus = 256;
    if (int rc = device_cus(device, &cus)) return rc;
    NUFFT_HIP(nufft::launch_coil_expand(dtype, n, ncoils, out, maps, in, cus, static_cast<hipStream_t>(stream)));
    return NUFFT_OK;
}

int nufft_coil_combine(int dtype, int64_t n, int32_t ncoils, void* out, const void* const* maps, const void* const* in, int device, void* stream) {
    if (device < 0) return fail(NUFFT_ERR_NO_DEVICE, "nufft_coil_combine needs a device");
    if (int rc = coil_args(dtype, n, ncoils, maps, in, out)) return rc;
    if (n == 0) return NUFFT_OK;
    DeviceGuard guard(device);
    int cus = 256;
    if (int rc = device_cus(device, &cus)) return rc;
    NUFFT_HIP(nufft::launch_coil_combine(dtype, n, ncoils, out, maps, in, false, cus, static_cast<hipStream_t>(stream)));
    return NUFFT_OK;
}

}  // extern "C"
