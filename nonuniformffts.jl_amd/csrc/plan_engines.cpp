// Which engines serve a plan, and the per-point-set policy of set_points: host arithmetic only — no HIP call, nothing written into the
// plan.  Plan creation (plan.cpp) runs the creation stage for 256 CUs, build_device the device stage for the CU count of its device;
// a host-only plan reports the device stage's sort column for 256 CUs.  Every measured threshold lives here, next to its measurements.
#include <algorithm>
#include <cmath>

#include "host_common.h"
#include "kernels.h"

namespace nufft {

static TileShape make_shape(const TileShapeHost& h) {
    TileShape t{};
    for (int d = 0; d < 3; ++d) { t.n[d] = h.n[d]; t.nt[d] = h.nt[d]; }
    t.row_stride = h.row_stride;
    t.plane_stride = h.plane_stride;
    t.elems = (int)h.elems;
    t.ntiles = (int)h.ntiles;
    t.max_items = h.max_items;
    return t;
}

Geom make_geom(const nufft_plan* p) {
    Geom g{};
    for (int d = 0; d < 3; ++d) {
        g.Nover[d] = (int)p->Nover[d];
        g.blog[d] = p->tile.blog[d];
        g.nb[d] = p->tile.nb[d];
    }
    g.nbins = (int)p->tile.nbins;
    g.sp = make_shape(p->tile.sp);
    g.ip = make_shape(p->tile.ip);
    return g;
}

// Default of the spreading ring's halo variant for this plan (0: clipped columns, 2: halo variant); see DESIGN.md section 4.9.
// Measured (256^3 -> 512^3, Np = 1e7; spread + FFT stages, ms; scripts/r4_halo_matrix.sh): Float64 m = 2 ... 7: 2.08 / 2.57 / 3.03 / 5.72 /
// 11.4 / 20.7 with clipped columns, 1.88 / 2.22 / 2.62 / 4.68 / 8.35 / 14.8 with the halo variant; Float32 alike (m = 8: 17.3 -> 13.1).
// Only where the plan's own dimension-1 pass adds the side buffer (real plans on the pruned FFT path); smarch_plan falls back to the
// clipped columns where the variant cannot run (axes the column does not divide, LDS).
// Complex data (interleaved components double the window): it pays where a 32 x 16 column or larger still fits — ComplexF64 m = 2 (3.29 -> 2.84 ms),
// ComplexF32 m = 2, 3 (2.55 -> 1.97, 4.03 -> 3.51); with 16 x 16 columns the reach is 1.2 x the grid (ComplexF64 m = 3: 4.70 -> 5.08 ms).
static int smarch_halo_default(const nufft_plan& p, int parts) {      // (device stage: ... and only on the plan's own pruned FFT path)
    if (p.D != 3) return 0;
    if (!p.is_complex || parts == 2) return 2;      // (complex data part by part through the real kernel: as real data)
    return p.M <= (p.dtype == NUFFT_F32 ? 3 : 2) ? 2 : 0;
}

// Largest half-support for which the automatic choice takes the marching window (measured spread + FFT stages):
// real data 6 (Float32 with the halo variant: 7); complex data part by part through the real kernel: 6 — measured round 5, 256^3 -> 512^3,
// Np = 1e7, spread + FFT stages in ms, window against patches: ComplexF64 m = 4 5.46 / 6.31 (interleaved window), m = 5 9.87 / 14.30, m = 6 14.47 / 24.88,
// m = 7 24.10 / 24.29; ComplexF32 m = 4 4.65 / 5.61, m = 5 8.78 / 9.94, m = 6 13.08 / 15.08, m = 7 20.67 / 14.94; the interleaved complex
// instantiations (NUFFT_SMARCH_SPLIT=0): ComplexF64 4, ComplexF32 3
static int ring_max_half_support(const nufft_plan& p, const SMarchPlan& sm) {
    if (!p.is_complex) return (p.dtype == NUFFT_F32 && sm.halo == 2) ? 7 : 6;
    if (sm.parts == 2 && sm.halo == 2) return 6;
    return p.dtype == NUFFT_F64 ? 4 : 3;
}

// The retry sequence of the ring's launch model: the wanted variant, then the clipped columns where the halo variant cannot run
SMarchPlan ring_ladder(const nufft_plan& p, int num_cus, int want_halo, int parts) {
    const bool other = needs_other_eval(p.kernel, p.evalmode);
    SMarchPlan sm = smarch_plan(p.opts, p.dtype, p.is_complex, p.D, p.M, make_geom(&p), other, num_cus, p.C, want_halo, parts);
    if (!sm.eligible && want_halo) sm = smarch_plan(p.opts, p.dtype, p.is_complex, p.D, p.M, make_geom(&p), other, num_cus, p.C, 0, parts);
    return sm;
}

// automatic choice, from the measurements in DESIGN.md section 4.4: the patches win where the stencil carries
// more matrix work per point visit (complex data, M >= 5: 1.15x ... 2x), the LDS tiles for real data at M <= 4
// — and for real plans with ntransforms = 2 / 3, whose components the patches spread together (shared windows and operands:
// C4 9.1 -> 7.5 ms, two components 6.1 -> 5.2 ms)
// third engine, the z-marching LDS window (smarch_kernels.h): the per-point arithmetic of the LDS tiles with 1.5 instead of
// 2.1 visits per point and no per-plane control.  Automatic choice from the measured spread stage of the three engines
// (256^3 -> 512^3, Np = 1e7): real data up to M = 6 (M = 4: 2.44 ms against 3.07 tiles / 4.05 patches;
// M = 6: 10.8 / 15.5 / 13.2; M = 7: 20.1 against 13.4 patches), ntransforms components one after the other (C = 3: 7.3 ms
// against 7.5 with the planar patches); ComplexF64 up to M = 4 (5.06 against 5.36 patches), ComplexF32 up to M = 3 (M = 4:
// 4.71 against 4.10 patches).
// (with the halo variant the window also beats the patches for Float32 at M = 7: 10.8 against 12.8 ms spread + FFT)
// `sm`: the ring's plan for the CU count at hand.  Both stages run this rule.  The device stage used to leave the NUFFT_PREFER_PATCHES read out
// of its copy, which made no difference: it runs only where the creation stage chose the ring, and with that switch set an automatic
// request never chooses the ring there.
int auto_spread_method(const nufft_plan& p, const SMarchPlan& sm) {
    const int req = p.spread_method_req;
    const bool force_patches = p.opts.option_int("NUFFT_PREFER_PATCHES", 0) != 0;      // (the switch: test runs)
    const bool prefer_ring = p.opts.option_int("NUFFT_PREFER_RING", 1) != 0 && p.M <= ring_max_half_support(p, sm) && !force_patches;
    if (sm.eligible && (req == NUFFT_SPREAD_MARCHING_RING || (req == NUFFT_SPREAD_AUTO && prefer_ring))) return NUFFT_SPREAD_MARCHING_RING;
    const bool prefer_patches = p.is_complex || p.M >= 5 || p.patch.planar != 0 || force_patches;
    return (p.patch.eligible && (req == NUFFT_SPREAD_MFMA_PATCHES || (req == NUFFT_SPREAD_AUTO && prefer_patches))) ? NUFFT_SPREAD_MFMA_PATCHES
                                                                                                                         : NUFFT_SPREAD_LDS_TILES;
}

// Creation stage: 256 CUs assumed here, the device stage redoes the decomposition for the device.
// halo variant of the ring (every point spread once, the stencil reach through a side buffer that the first FFT pass adds):
// real data on grids whose axes the column divides; NUFFT_SMARCH_HALO=0 / 2 forces the choice (A/B runs, tests)
// complex data part by part through the REAL window kernel (smarch_kernels.h: 8 x 8 faces, 32 x 32 columns, halo variant — ComplexF64
// m = 4: 5.06 -> 3.9 ms); NUFFT_SMARCH_SPLIT=0: the interleaved complex instantiations (A/B runs, tests)
SMarchPlan creation_stage_ring(const nufft_plan& p, int* parts_out) {
    SMarchPlan sm{};
    for (int parts = (p.is_complex && p.opts.option_int("NUFFT_SMARCH_SPLIT", 1) != 0) ? 2 : 1; parts >= 1; --parts) {
        *parts_out = parts;      // (2 without a real-kernel decomposition: the complex instantiations as before)
        sm = ring_ladder(p, 256, p.opts.option_int("NUFFT_SMARCH_HALO", smarch_halo_default(p, parts)) == 2 ? 2 : 0, parts);
        if (sm.eligible) break;
    }
    return sm;
}

// pruned FFT path: D >= 2, every higher dimension (and dimension 1 of complex plans) of an instantiated length; a real
// plan whose dimension-1 pass is the library's own keeps the COMPACT spectrum only
FftPath fft_path(const nufft_plan& p) {
    FftPath f{};
    f.pruned = p.D >= 2 && p.opts.option_int("NUFFT_PRUNED_FFT", 1) != 0;
    for (int d = p.is_complex ? 0 : 1; d < p.D && f.pruned; ++d) f.pruned = fft_lines_supported(p.dtype, p.Nover[d]);
    f.compact_dim1 = f.pruned && (p.is_complex || (real_lines_supported(p.dtype, p.Nover[0]) && p.opts.option_int("NUFFT_COMPACT_DIM1", 1) != 0));
    return f;
}

// interpolation ring: which form (complex data part by part through the real kernels?) and whether it exists for this plan
InterpRing choose_interp_ring(const nufft_plan& p) {
    InterpRing r{};
    r.mode = p.opts.option_int("NUFFT_INTERP_MARCH", 1);
    // ComplexF64 part by part through the REAL ring kernels (march_setup.inc, MarchGeom::parts = 2): the complex instantiation reads 128-bit pairs
    // from LDS at a quarter of the rate (scripts/microbench7.hip) and owns a narrower column — two passes of the real kernel are faster from
    // m = 4 on (interpolation stage 256^3 -> 512^3, Np = 1e7: 2.76 against 2 x 1.2 ms; m = 8: 20.4 against 2 x 5.8), and the plan can then share
    // its columns with the spreading window (column-layer sort).  ComplexF32 keeps its paired-lane kernel (1.25 ms against 2 x 1.08).
    // NUFFT_INTERP_SPLIT=0: the complex instantiations (A/B runs, tests)
    const bool other = needs_other_eval(p.kernel, p.evalmode), poly = p.evalmode != NUFFT_EVAL_DIRECT;
    for (r.parts = (p.is_complex && p.dtype == NUFFT_F64 && p.opts.option_int("NUFFT_INTERP_SPLIT", 1) != 0) ? 2 : 1; r.parts >= 1; --r.parts) {
        r.available = r.mode != 0 && interp_march_available(p.dtype, r.parts == 2 ? 0 : (int)p.is_complex, p.D, p.M, poly, make_geom(&p), other);
        if (r.available || r.parts == 1) break;
    }
    return r;
}

// Column-layer sort: ONE column for both rings — the spreading window's (chosen for this grid by its launch model, smarch_plan); the
// interpolation ring takes it wherever its kernels can hold it (a column <= their compile-time one: march_setup.inc).  Round 6; before,
// only plans whose two rings happened to pick the same column qualified (Float64 / ComplexF64 m = 4).  `sm`: the window's final plan
// (halo variant), `interp_parts`: the interpolation ring's form.
bool shared_ring_column(const nufft_plan& p, const SMarchPlan& sm, int interp_parts, ColumnTasks* shared) {
    if (!sm.eligible || sm.halo != 2 || p.D != 3) return false;
    const int nkeys = sm.ct.ncolx * sm.ct.ncoly * p.tile.nb[2];
    const int mcplx = interp_parts == 2 ? 0 : (int)p.is_complex;
    const bool poly = p.evalmode != NUFFT_EVAL_DIRECT;
    if (p.Nover[0] % sm.n1 != 0 || p.Nover[1] % sm.n2 != 0 || nkeys > kCoarseMaxKeys) return false;
    // Measured (256^3 -> 512^3, Np = 1e7, set_points + spread / set_points + interpolation against the plan without it, ms; scripts/r6_e.sh,
    // profiles/round6_*): Float64 m = 2 / 3 / 4 -0.18 / -0.18 / -0.12 and -0.14 / -0.20 / -0.21, ComplexF64 m = 4 -0.12 / -0.29, Float32 m = 3 / 4
    // -0.06 / -0.03 and -0.07 / -0.04, ComplexF32 m = 3 / 4 -0.15 / -0.04 and -0.02 / -0.02 (polynomial window: +0.02) — and Float32 m = 2
    // -0.11 but +0.12 (Direct) / +0.22 (polynomial) on the type-2 side: its ring gathers through the LDS strips (no register window at 4-lane
    // rows) from a 64 x 64 column of its own, which the 32 x 32 window column cannot replace.  That one keeps its own column
    // (NUFFT_COARSE_SORT=2: shared all the same — the test of its staged instantiation).
    if (p.dtype == NUFFT_F32 && !p.is_complex && p.M == 2 && p.opts.option_int("NUFFT_COARSE_SORT", 1) != 2) return false;
    if (!interp_march_staged_available(p.dtype, mcplx, p.M, poly, sm.n1, sm.n2)) return false;
    const ColumnTasks ct = march_column_tasks(p.dtype, mcplx, p.M, poly, make_geom(&p), sm.n1, sm.n2);
    if (ct.ntasks <= 0 || ct.ncolx != sm.ct.ncolx || ct.ncoly != sm.ct.ncoly || (size_t)ct.ncolx * ct.ncoly >= 65536 || p.tile.nb[2] > 2048) return false;
    *shared = ct;
    return true;
}

// Device stage: every engine decision of a plan on a device of `num_cus` compute units.  `halo_allowed` = false: the side buffer of the
// ring's halo variant could not be allocated.  Needs what the creation stage left in the plan (tiles, patch plan, p.smarch, p.smarch_parts).
EngineDecision decide_engines(const nufft_plan& p, int num_cus, bool halo_allowed) {
    EngineDecision e{};
    const bool other = needs_other_eval(p.kernel, p.evalmode), poly = p.evalmode != NUFFT_EVAL_DIRECT;
    // second interpolation engine (z-marching ring, march_kernels.h): 3-D plans with the default window evaluation.  Which of
    // the two kernels gathers a point set is decided on the device at set_points (heaviest ring task and total work against the
    // ring's fitted advantage over the tile kernel: balance.hip, d_march_choice[2]); the mode is latched here —
    // NUFFT_INTERP_MARCH = 0: never the ring (A/B runs), 2: always (tests of its instantiations on small grids)
    e.interp = choose_interp_ring(p);
    if (e.interp.available) {
        e.march_ct = march_column_tasks(p.dtype, e.interp.parts == 2 ? 0 : (int)p.is_complex, p.M, poly, make_geom(&p));
        if ((size_t)e.march_ct.ncolx * e.march_ct.ncoly >= 65536 || p.tile.nb[2] > 2048) e.interp.available = false;      // (beyond the task kernels' table formats)
    }
    e.spread_method = p.spread_method;
    e.smarch = p.smarch;
    if (p.spread_method == NUFFT_SPREAD_MARCHING_RING) {
        int want_halo = halo_allowed ? p.smarch.halo : 0;
        if (want_halo == 2 && !(p.pruned_fft && p.compact_dim1) && p.opts.option_int("NUFFT_SMARCH_HALO", 0) != 2) want_halo = 0;   // no fused consumer: not worth it
        e.smarch = ring_ladder(p, num_cus, want_halo, p.smarch_parts);
        // the creation stage chose the engine for 256 CUs and the halo variant it hoped for: redo the automatic choice for what this device got
        // (Float32 m = 7 belongs to the ring only with the halo variant: 20.1 ms clipped against 13.4 ms with the patches)
        const bool keep = e.smarch.eligible && (p.spread_method_req == NUFFT_SPREAD_MARCHING_RING || p.M <= ring_max_half_support(p, e.smarch));
        if (!keep) {
            e.ring_lost = p.spread_method_req == NUFFT_SPREAD_MARCHING_RING;
            e.smarch.eligible = false;
            e.spread_method = auto_spread_method(p, e.smarch);
        }
    }
    const bool ring = e.spread_method == NUFFT_SPREAD_MARCHING_RING;
    // Column-layer sort (binsort.hip, CoarseSort): where the spreading window (halo variant: a column visits its own points only) and
    // the interpolation ring own the same columns, set_points only groups the points by (column, layer of bins) — few enough keys for
    // LDS histograms, no global atomics — and the interpolation ring's staged variant orders a layer's points by bin on their way
    // into LDS.  Per point set: only while both rings serve it (device flags); NUFFT_COARSE_SORT=0 keeps the fine sort (A/B runs).
    ColumnTasks shared{};
    e.shared_column = ring && e.smarch.halo == 2 && e.interp.available && p.D == 3 && p.opts.option_int("NUFFT_COARSE_SORT", 1) != 0 &&
                      shared_ring_column(p, e.smarch, e.interp.parts, &shared);
    if (e.shared_column) e.march_ct = shared;
    // Dense-set engine of the spreading window (dmarch_kernels.h): the points of a bin accumulated in registers by the FP64 matrix pipe, one flush
    // per bin.  Taken per point set from the mean bin load (set_points: dense_now); it needs the fine-bin order, so on plans of the
    // column-layer sort a dense point set takes the slab sort below.  NUFFT_DENSE=0: never; NUFFT_DENSE_MIN: the threshold (points per bin).
    e.dense_available = ring && p.opts.option_int("NUFFT_DENSE", 1) != 0 && !other && spread_dense_available(p.dtype, p.is_complex, p.M, poly, e.smarch);
    // Break-even against the stream of atomics, mean points per bin — measured (profiles/round6_dense_engine.md; 256^3 Float64, spread stage, ms, dense /
    // atomic): m = 4 Direct() 3.69 / 2.97 at 19 per bin, 9.38 / 9.21 at 60; polynomial window 2.76 / 2.72 at 19, 6.66 / 8.40 at 60, and on the
    // reference's folded N(0, 1) sets 4.52 / 5.57 at a mean of 19; m = 5 Direct() 6.38 / 4.13 at 4.8, 12.99 / 14.18 at 19, polynomial 5.05 / 3.91 and
    // 8.79 / 13.27; m = 6 Direct() 7.70 / 6.48 and 15.80 / 22.61, polynomial 7.95 / 7.49 and 15.14 / 23.63; m = 2, 3 lose at 19 per bin (1.15 - 1.4 x).
    // The FP64 matrix instructions run on the SIMD's FP64 vector ALUs (vector 37 % + matrix 25 % + LDS 32 % of the kernel's cycles ADD UP,
    // counters in the same file): the engine only trades LDS-atomic time for vector time, which pays where a point costs 20 - 36 atomics
    // (m = 5, 6) or the window evaluation is cheap (polynomial) and the bins are full.
    static const int dense_min_direct[7] = {0, 0, 1 << 30, 1 << 30, 96, 16, 12};
    static const int dense_min_poly[7] = {0, 0, 1 << 30, 1 << 30, 24, 10, 6};
    e.dense_min = p.opts.option_int("NUFFT_DENSE_MIN", p.M <= 6 ? (poly ? dense_min_poly : dense_min_direct)[p.M] : 1 << 30);
    // every other 3-D plan: two-level slab sort (column_tasks.h) — the sorted array and offsets of the fine sort, without global atomics
    e.slab = p.D == 3 && p.opts.option_int("NUFFT_SLAB_SORT", 1) != 0 && p.tile.nb[0] <= kSlabMaxBins && p.tile.nb[2] <= kCoarseMaxKeys;
    if (e.slab) {
        e.slab_min_points = p.opts.option_int("NUFFT_SLAB_MIN_POINTS", 16384);
        e.slab_fill = std::min(95, std::max(5, p.opts.option_int("NUFFT_SLAB_FILL", 85)));
        // [slices][keys] table of level 1: at most one slice per CU; the keys are (rows of bins / slab height) x layers — never more than
        // nb[1] x nb[2], whatever height set_points picks (a 16^3 plan used to pay the 37.7 MB of the largest grid: ADVICE round 5)
        e.slab_max_keys = (int)std::min<int64_t>(kCoarseMaxKeys, (int64_t)p.tile.nb[1] * p.tile.nb[2]);
    }
    e.adaptive = e.shared_column && e.slab && p.opts.option_int("NUFFT_SORT_ADAPTIVE", 1) != 0;
    return e;
}

// ------------------------------------------------------------------------------------------
// per-point-set policy (nufft_set_points)
// ------------------------------------------------------------------------------------------
// steady path (nufft_internal.h: steady_now).  A record is counted when its sequence number is new to the host — not only the record of the latest
// call, as the exact two-misses logic of the slab sort wants it: the host may run many calls ahead of the device, and the streak it reads is the
// device's own count, so ANY record tells how the sets up to it went.  A record that reports a miss carries a streak of 0.
void steady_observe(SteadyState& s, uint32_t seq, uint32_t streak) {
    if (seq == s.seq_seen) return;
    s.seq_seen = seq;
    s.ok = streak >= (uint32_t)kSteadyStreak;
}
bool steady_eligible(const SteadyState& s, bool enabled, bool coarse, bool dense, int64_t np, bool barred) {
    return enabled && coarse && !dense && np > 0 && s.ok && !barred;
}

// bytes of the scratch of the sort a point set takes: {bin, rank} of the fine sort (8 bytes per point; also what a clustered set of a
// column-layer plan falls back to, decided on the device), or the level-1 records of the slab sort in the same allocation
// (plans of the column-layer sort use neither unless a point set is clustered — the fine sort, 8 bytes — or dense — the slab sort, a record)
int64_t sort_scratch_bytes(const nufft_plan& p, int64_t np, bool slab_sort) {
    return np * (slab_sort ? std::max<int64_t>(8, (int64_t)point_record_bytes(p.dtype, p.D)) : 8);
}

// slab height for this point set (0: the fine sort): the tallest slab (longest runs in level 1: C3 `set_points` 5.2 ms with 32 768 slabs, 4.4 ms with 16 384)
// whose average load is at most 85 % of what a level-2 workgroup can hold (fuller slabs take its two-pass form), while there are
// slabs enough to fill the chip
int slab_height(const nufft_plan& p, int64_t np) {
    if (!p.slab.enabled || np < std::max<int64_t>(p.slab_min_points, 1)) return 0;
    const int capmax = slab_sort_capacity(p.dtype, kLdsLimit - 256);
    int best = 0;
    for (int sby = 1; sby <= p.tile.nb[1] && (int64_t)sby * p.tile.nb[0] <= kSlabMaxBins; sby *= 2) {
        const int64_t nkeys = (int64_t)p.tile.nb[2] * ((p.tile.nb[1] + sby - 1) / sby);
        if (nkeys > p.slab_max_keys) continue;
        if (np / nkeys > (int64_t)capmax * p.slab_fill / 100) break;
        if (best > 0 && nkeys < 2048) break;
        best = sby;
    }
    return best;
}

// the patches' measured advantage over the LDS tiles on uniform points grows with the matrix work per point visit
// (ComplexF64 m = 4 1.17, m = 7 3.7; Float64 m = 6 1.5-1.7, m = 9 3.7; ComplexF32 on the FP32
// matrix pipe m = 8 3.4-4): 1.15 x g^(m - 4) with g = 1.2 (real) / 1.45 (complex), x 1.3 with Float32 accumulators,
// x 0.85 because the estimate counts a task's own column only and no scheduling tail.  An explicit request always
// takes the patches.
double patch_advantage(const nufft_plan& p) {
    if (p.spread_method_req == NUFFT_SPREAD_MFMA_PATCHES) return 0.0;
    return 0.85 * 1.15 * std::pow(p.is_complex ? 1.45 : 1.2, (double)std::max(p.M - 4, 0)) * (p.patch.f32acc ? 1.3 : 1.0);
}

// the spreading ring serves a point set while the heaviest task stays
// within its measured advantage over the LDS tiles on uniform points (x 0.85 for what the estimate leaves out); an
// explicit request always takes the ring
// (halo variant: 1.87 instead of 2.44 ms at C2, + 0.15 ms in the FFT pass: 3.67 / 2.62 = 1.4 against the tiles, stage + FFT; the
// reference's benchmark distribution — folded N(0, 1), sigma = 1.5, Np = 1.68e7 — sits at the threshold: tiles 6.78 + 0.32 ms
// below 1.19, window 6.18 + 0.38 ms from 1.3 on, hence 0.93 instead of 0.85 here)
double smarch_advantage(const nufft_plan& p) {
    if (p.spread_method_req == NUFFT_SPREAD_MARCHING_RING) return 0.0;
    const double adv_env = p.opts.option_double("NUFFT_SMARCH_ADVANTAGE", 0.0);
    return adv_env > 0.0 ? adv_env /* (experiments) */ : (p.smarch.halo == 2 ? 0.93 * 1.4 : 0.85 * 1.3);
}

// What the interpolation ring saves
// over interp_tile_kernel is grid traffic (halo 1.5x instead of 2.6x at m = 4, 3.75x instead of 12.5x at m = 8), which
// it also takes off the critical path; its gather itself is ~9 % slower per point (ring index arithmetic, two barriers
// per bin layer).  So its advantage falls with the point density rho = points per oversampled cell,
//   advantage = (rho + c_t) / (1.09 rho + c_r),  c_t = 0.038 (m/4)^1.85,  c_r = 0.0086 (m/4)^1.2
// fitted to: C2 (m = 4, rho = 0.075) 1.26, Float64 m = 6 1.55, C3 (m = 8, rho = 0.093) 1.9, and Float64 m = 4 at
// rho = 0.3 (1.68e7 points on 384^3) 1.0 — above that density the tile kernel is the faster one even for uniform points.
// (NUFFT_INTERP_MARCH=2: always the ring — tests of its instantiations on small grids)
double march_advantage(const nufft_plan& p, int64_t np) {
    if (p.interp_march_mode == 2) return 0.0;      // (<= 0: always the ring)
    const double rho = (double)np / (double)std::max<int64_t>(p.grid_elems, 1), mr = (double)p.M / 4.0;
    return (rho + 0.038 * std::pow(mr, 1.85)) / (1.09 * rho + 0.0086 * std::pow(mr, 1.2));
}

// Point sets far from uniform (tasks of equal point count): the same trade at the density the points themselves see,
// rho_eff = sum n^2 / (sum n x cells) over the column layers (balance.hip).  Uniform sets break even at
// rho* = (c_t - c_r) / 0.09 (0.33 at m = 4); cut tasks amortise the window loads better — measured at m = 4, Np = 1e7 ... 1.7e7:
// rho_eff = 0.42 (folded N(0, 1) on 512^3, Gaussian cluster of 1 rad) ring 1.87 / 1.88 ms against 2.10 / 2.09 tiles;
// 1.66 (folded N(0, 1), 1.68e7 points on 384^3) 3.42 against 2.58; 3.3 (cluster of 0.5 rad) 2.01 against 1.43 — so the ring
// keeps such sets up to 2.5 rho*.
double march_rho_bound(const nufft_plan& p) {
    const double mr = (double)p.M / 4.0;
    const double rho_star = (0.038 * std::pow(mr, 1.85) - 0.0086 * std::pow(mr, 1.2)) / 0.09;
    return 2.5 * rho_star;
}

}  // namespace nufft
