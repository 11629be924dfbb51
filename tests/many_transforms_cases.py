"""Cases shared by tests/test_gpu_many_transforms.py and tests/test_many_transforms_host.py: plans with more transforms
(`ntransforms = C`) than one kernel launch takes.  No GPU import.

A launch handles at most kMaxCompPerLaunch = 8 components (csrc/device_common.h); a plan with more is served by host loops
`for (c0 = 0; c0 < C; c0 += 8)` that derive every per-component pointer from `c0 + c` again: grids, value vectors, the sorted value
copies of the patch engine, the halo side buffer of the spreading ring, the deconvolution, the gradient gather, the pre- / postphase
of type 3.  C = 9 is one full chunk plus one component, C = 16 two full chunks, C = 17 two full chunks plus one.  A wrong offset in
a chunk loop stays inside the plan's allocations (nothing faults): components 9 and up would read or write the data of components 1
to 8, so every component gets values of its own (`default_rng(seed + 1000 c)`) and the tests assert that the reference components
are pairwise distinguishable before they compare.

Each case is `(name, Z, dims, M, sigma, evalmode, C, Np, spread_method, options, expected)`:
`options` are the NUFFT_* switches that force the engine the name says (applied with monkeypatch.setenv, as tests/test_gpu_parity.py
does), `expected` what `plan.info()` must report for the case to exercise that engine (plus, under the keys `spread_engine_used` /
`interp_engine_used`, what the device-side decision of set_points must be; those two are read on the GPU only).  The grids are those
of the per-engine tests of tests/test_gpu_parity.py, already the smallest on which the named engine exists.  Cases that share a
`key` (the same table row run under several switches) share inputs, evaluation mode and therefore one oracle reference; the
evaluation mode alternates from row to row.

Out of scope: the column-layer sort with the staged interpolation ring.  Its smallest eligible grid is 512 x 512 x 64 oversampled,
nine components of which cost the oracle more than this suite's budget per test; its launch sits inside the same chunk loop as the
plain ring's (tile_launch.hip, launch_t), which is covered here.  Planar patches (C = 2, 3) are covered by
tests/test_gpu_parity.py::test_planar_patch_every_instantiation, the solver layers beyond eight components by tests/test_gpu_cg.py,
test_gpu_tvt.py, test_gpu_frames.py and test_gpu_glr.py.
"""
import numpy as np

DIRECT, FAST = 0, 1          # oracle.nufft_oracle.DIRECT / FAST_APPROXIMATION
TWO_PI = 2.0 * np.pi
SEED = 9000

LDS_TILES, MFMA_PATCHES, MARCHING_RING = 1, 2, 3          # info().spread_method (include/nufft_mi355x.h NUFFT_SPREAD_*)
ENGINE_NAMES = {"lds_tiles", "mfma_patches", "marching_ring"}

f32, f64, c64, c128 = np.float32, np.float64, np.complex64, np.complex128

_TILES = dict(NUFFT_INTERP_MARCH="0")
_TILES_EXP = dict(spread_method=LDS_TILES, spread_engine_used="lds_tiles", interp_engine_used="lds_tiles")
_PATCH_EXP = dict(spread_method=MFMA_PATCHES, patch_planar=0, spread_engine_used="mfma_patches")
_CLIPPED_EXP = dict(spread_method=MARCHING_RING, ring_halo=0, spread_engine_used="marching_ring")
_HALO_EXP = dict(spread_method=MARCHING_RING, ring_halo=1, spread_engine_used="marching_ring")
_DENSE_EXP = dict(spread_method=MARCHING_RING, ring_halo=1, spread_engine_used="marching_ring_dense")
_IRING_EXP = dict(interp_engine_used="marching_ring")
_DENSE_NP = 20 * (96 // 4) * (96 // 4) * (112 // 4)       # 20 points per 4^3-cell bin of the 96 x 96 x 112 grid

CASES = [
    # name, Z, dims, M, sigma, evalmode, C, Np, spread_method, options, expected
    ("tiles-f64", f64, (48, 40, 56), 4, 2.0, DIRECT, 9, 3000, "lds_tiles", _TILES, _TILES_EXP),
    ("tiles-c64", c64, (48, 40, 56), 4, 2.0, FAST, 9, 3000, "lds_tiles", _TILES, _TILES_EXP),
    # 48 x 40 x 60 oversampled: rocFFT with batch = C and the kernels of deconv.hip
    ("tiles-general-fft-c128", c128, (24, 20, 30), 6, 2.0, DIRECT, 17, 3000, "lds_tiles", _TILES, _TILES_EXP),
    ("tiles-small-f32", f32, (12, 16, 10), 3, 2.0, FAST, 16, 3000, "lds_tiles", _TILES, _TILES_EXP),      # a grid smaller than one tile
    # nine components are not planar: the per-component sorted value copies (vsorted)
    ("patches-f64", f64, (48, 48, 48), 4, 2.0, DIRECT, 9, 4000, "mfma_patches", {}, _PATCH_EXP),
    ("patches-c128", c128, (48, 48, 48), 4, 2.0, FAST, 9, 4000, "mfma_patches", {}, _PATCH_EXP),
    ("patches-f32acc-c64", c64, (48, 48, 48), 4, 2.0, DIRECT, 9, 4000, "mfma_patches", {}, dict(_PATCH_EXP, patch_f32acc=1)),
    ("ring-clipped-f32", f32, (48, 40, 56), 4, 2.0, FAST, 9, 4000, "marching_ring", dict(NUFFT_SMARCH_HALO="0"), _CLIPPED_EXP),
    ("ring-clipped-c128-split1", c128, (48, 40, 56), 4, 2.0, DIRECT, 9, 4000, "marching_ring",
     dict(NUFFT_SMARCH_HALO="0", NUFFT_SMARCH_SPLIT="1"), _CLIPPED_EXP),
    ("ring-clipped-c128-split0", c128, (48, 40, 56), 4, 2.0, DIRECT, 9, 4000, "marching_ring",
     dict(NUFFT_SMARCH_HALO="0", NUFFT_SMARCH_SPLIT="0"), _CLIPPED_EXP),
    ("ring-halo-f64-fuse1", f64, (64, 48, 64), 4, 2.0, FAST, 9, 5000, "marching_ring",
     dict(NUFFT_SMARCH_HALO="2", NUFFT_SMARCH_HALO_FUSE="1"), _HALO_EXP),
    ("ring-halo-f64-fuse0", f64, (64, 48, 64), 4, 2.0, FAST, 9, 5000, "marching_ring",
     dict(NUFFT_SMARCH_HALO="2", NUFFT_SMARCH_HALO_FUSE="0"), _HALO_EXP),
    # complex data part by part through the real kernel: planar side buffers, two rows per component
    ("ring-halo-c128-fuse1", c128, (64, 48, 64), 4, 2.0, DIRECT, 9, 5000, "marching_ring",
     dict(NUFFT_SMARCH_HALO="2", NUFFT_SMARCH_SPLIT="1", NUFFT_SMARCH_HALO_FUSE="1"), _HALO_EXP),
    ("ring-halo-c128-fuse0", c128, (64, 48, 64), 4, 2.0, DIRECT, 9, 5000, "marching_ring",
     dict(NUFFT_SMARCH_HALO="2", NUFFT_SMARCH_SPLIT="1", NUFFT_SMARCH_HALO_FUSE="0"), _HALO_EXP),
    ("dense-f64", f64, (48, 48, 56), 5, 2.0, FAST, 9, _DENSE_NP, "marching_ring",
     dict(NUFFT_SMARCH_HALO="2", NUFFT_DENSE_MIN="0"), _DENSE_EXP),
    ("dense-c128", c128, (48, 48, 56), 5, 2.0, DIRECT, 9, _DENSE_NP, "marching_ring",
     dict(NUFFT_SMARCH_HALO="2", NUFFT_DENSE_MIN="0"), _DENSE_EXP),
    ("interp-ring-f64", f64, (48, 40, 56), 4, 2.0, FAST, 9, 4000, "auto", dict(NUFFT_INTERP_MARCH="2"), _IRING_EXP),
    ("interp-ring-c64", c64, (48, 40, 56), 4, 2.0, DIRECT, 9, 4000, "auto", dict(NUFFT_INTERP_MARCH="2"), _IRING_EXP),
    ("interp-ring-c128", c128, (48, 40, 56), 4, 2.0, FAST, 9, 4000, "auto", dict(NUFFT_INTERP_MARCH="2"), _IRING_EXP),
    ("interp-ring-c128-split0", c128, (48, 40, 56), 4, 2.0, FAST, 9, 4000, "auto",
     dict(NUFFT_INTERP_MARCH="2", NUFFT_INTERP_SPLIT="0"), _IRING_EXP),
    ("automatic-f64", f64, (64, 64, 64), 4, 2.0, DIRECT, 9, 5000, "auto", {}, {}),          # nothing forced: the engines are printed
    ("real-odd-n1-f64", f64, (31, 31, 31), 4, 2.0, FAST, 9, 3000, "auto", {}, {}),
    ("2d-f64", f64, (64, 64), 4, 2.0, DIRECT, 9, 3000, "auto", {}, {}),
    ("2d-c128", c128, (37, 41), 5, 1.25, FAST, 16, 3000, "auto", {}, {}),
    ("1d-f64", f64, (256,), 4, 2.0, DIRECT, 17, 3000, "auto", {}, {}),
    ("1d-c64", c64, (100,), 3, 2.0, FAST, 9, 3000, "auto", {}, {}),
]

IDS = [c[0] for c in CASES]

# keys of `expected` that plan.info() answers (the others are device-side decisions, read back on the GPU)
INFO_KEYS = ("spread_method", "ring_halo", "patch_f32acc", "patch_planar")


def case(name):
    return CASES[IDS.index(name)]


def key(c):
    """What the inputs and the oracle's reference of a case depend on: cases with equal keys share one reference."""
    name, Z, dims, M, sigma, evalmode, C, Np, spread_method, options, expected = c
    return (np.dtype(Z).name, dims, M, sigma, evalmode, C, Np)


def real_dtype(Z):
    return np.dtype(np.float32) if np.dtype(Z) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.dtype(np.float64)


def seed_of(c):
    """One seed per key (stable across runs and processes)."""
    name, Z, dims, M, sigma, evalmode, C, Np, spread_method, options, expected = c
    return SEED + 7 * sum(dims) + 31 * M + 101 * C + np.dtype(Z).itemsize


def points(c):
    """D coordinate vectors in the plan's precision, outside the unit cell too (as tests/test_gpu_parity.py::_make_case)."""
    name, Z, dims, M, sigma, evalmode, C, Np, spread_method, options, expected = c
    rng = np.random.default_rng(seed_of(c))
    return [((rng.random(Np) * 3 - 1) * TWO_PI).astype(real_dtype(Z)) for _ in dims]


def values(c):
    """C value vectors of type Z: component k from its own generator."""
    name, Z, dims, M, sigma, evalmode, C, Np, spread_method, options, expected = c
    out = []
    for k in range(C):
        rng = np.random.default_rng(seed_of(c) + 1000 * k)
        v = rng.standard_normal(Np)
        if np.dtype(Z).kind == "c":
            v = v + 1j * rng.standard_normal(Np)
        out.append(v.astype(Z))
    return out


def spectra(c, shape):
    """C uniform arrays (tensor shape `shape` = reversed size(plan)) in the plan's complex type: component k from its own generator."""
    name, Z, dims, M, sigma, evalmode, C, Np, spread_method, options, expected = c
    ctype = np.complex64 if real_dtype(Z) == np.float32 else np.complex128
    out = []
    for k in range(C):
        rng = np.random.default_rng(seed_of(c) + 1000 * k + 500)
        out.append((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(ctype))
    return out


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def assert_distinguishable(refs, what=""):
    """rel(ref[a], ref[b]) > 0.5 for all a != b (independent random components: about sqrt(2)): without it a mix-up between
    components could pass a comparison with the reference."""
    for a in range(len(refs)):
        for b in range(len(refs)):
            if a != b:
                assert rel(refs[a], refs[b]) > 0.5, (what, a, b)
