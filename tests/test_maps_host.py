"""The coil sensitivity map estimate without a GPU: the numpy reference (maps_reference.py) against itself -- the kernel's
Jacobi against ``np.linalg.eigh`` on every cell of every case --, exact properties of the estimate, the crop mask, the calibration taper
and the C ABI (header, ctypes mirror, symbols, struct sizes, the refusals that need no device, in the documented order)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import maps_cases as MC
import maps_reference as M
from llr_reference import jacobi_eigh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
ENTRY_POINTS = ("nufft_coilmaps_create", "nufft_coilmaps_create_for_operator", "nufft_coilmaps_destroy", "nufft_coilmaps_get_info",
                "nufft_coilmaps_estimate", "nufft_coilmaps_last_sweeps", "nufft_coilmaps_layout", "nufft_coilmaps_apply_crop",
                "nufft_sizeof_coilmaps_params", "nufft_sizeof_coilmaps_info")


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


@pytest.mark.parametrize("Ns,ncoils,box", MC.CASES + MC.GLOBAL_CASES)
def test_reference_against_itself(Ns, ncoils, box):
    """Every cell of the case.  The conditions that let every cell be compared (relative gap >= 0.5, |s| >= 0.05) are asserted here; the
    printed maxima are what maps_cases.SELF_EPS records and the GPU bars are derived from.  Measured: at most 7.1 ε on the maps and
    34.3 ε on λ1 ((12, 10), C = 32), at most 11 sweeps; smallest gap 0.773 ((7, 5), C = 2), smallest |s| 0.063 ((12, 10), C = 32)."""
    a = MC.images(Ns, ncoils)
    want, w1, w2, info = MC.reference(Ns, ncoils, box)
    mine = {}
    got, l1, l2 = M.walsh(a, box, eigh=jacobi_eigh, info=mine)
    ev, el = MC.per_cell(got, want) / EPS, float((np.abs(l1 - w1) / w1).max()) / EPS
    print(f"N={Ns} C={ncoils} box={box}: maps {ev:.1f} ε, λ1 {el:.1f} ε, {mine['sweeps']} sweeps, smallest gap {info['min_gap']:.3f}, smallest |s| {info['min_s']:.3f}")
    assert info["min_gap"] >= 0.5 and info["min_s"] >= 0.05
    assert ev <= 64 and el <= 128 and mine["sweeps"] < 24
    assert ev <= MC.SELF_EPS[(Ns, ncoils, box)][0] and el <= MC.SELF_EPS[(Ns, ncoils, box)][1]
    assert (np.abs(l2 - w2) <= 128 * EPS * w1).all()
    assert (ncoils == 1 and mine["sweeps"] == 0) or mine["sweeps"] >= 2


def test_pca_case_keeps_the_phase_condition():
    Ns, ncoils, box = MC.PCA_CASE
    for Z in ("c128", "c64"):
        p = M.pca_reference(MC.images(Ns, ncoils).astype(MC.dt(Z)[1]))
        assert abs(np.linalg.norm(p) - 1) <= 8 * EPS and abs(p[np.argmax(np.abs(p))].imag) <= EPS
        assert MC.reference(Ns, ncoils, box, Z, phase=p)[3]["min_s"] >= 0.05


def test_exact_properties():
    Ns, ncoils, box = (32, 40), 4, (5, 5)
    shape = Ns[::-1]
    _, rho = MC.truth(Ns, ncoils)
    s = np.array([0.8 + 0.1j, -0.3 + 0.5j, 0.2 - 0.6j, 0.4j])
    # maps constant in space, no noise: v = s / ‖s‖ up to the phase rule, at every cell
    v, l1, l2 = M.walsh(s.reshape(-1, 1, 1) * rho, box)
    unit = s / np.linalg.norm(s) * (np.conj(s[0]) / abs(s[0]))
    assert MC.per_cell(v, np.broadcast_to(unit.reshape(-1, 1, 1), v.shape)) <= 16 * EPS
    assert (l2 <= 16 * EPS * l1).all()
    a = MC.images(Ns, ncoils)
    # box 1: v = a / ‖a‖ with coil 0 real, λ2 = 0
    v, l1, l2 = M.walsh(a, (1, 1))
    unit = a / np.sqrt((np.abs(a) ** 2).sum(axis=0)) * (np.conj(a[0]) / np.abs(a[0]))
    assert MC.per_cell(v, unit) <= 16 * EPS and (l2 <= 16 * EPS * l1).all()
    # unit norm, coil 0 real and non-negative
    v, l1, l2 = MC.reference(Ns, ncoils, box)[:3]
    assert np.abs((np.abs(v) ** 2).sum(axis=0) - 1).max() <= 8 * EPS
    assert np.abs(v[0].imag).max() <= EPS and v[0].real.min() > 0
    # a positive scale leaves the maps alone; a cyclic shift shifts them
    assert MC.per_cell(M.walsh(3.7 * a, box)[0], v) <= 16 * EPS
    rolled = M.walsh(np.roll(a, (3, -5), axis=(1, 2)), box)[0]
    assert MC.per_cell(rolled, np.roll(v, (3, -5), axis=(1, 2))) <= 16 * EPS
    # a zero block larger than the box gives exact zeros there, for both solvers
    z = a.copy()
    z[:, 10:26, 6:20] = 0
    inner = (slice(None), slice(12, 24), slice(8, 18))
    small = (slice(None), slice(8, 28), slice(4, 22))
    for eigh in (np.linalg.eigh, jacobi_eigh):
        crop_z = z[small]
        v, l1, l2 = M.walsh(crop_z, box, eigh=eigh)
        assert not v[:, 4:16, 4:14].any() and not l1[4:16, 4:14].any() and not l2[4:16, 4:14].any() and v[:, 0, 0].any()
    assert not z[inner].any() and shape == (40, 32)


@pytest.mark.parametrize("Ns,ncoils,box", [((32, 40), 4, (5, 5)), ((7, 5), 2, (3, 3)), ((32, 40), 8, (7, 3)), ((12, 10), 17, (3, 3))])
def test_crop_mask_is_the_same_for_both_solvers(Ns, ncoils, box):
    for Z in ("c128", "c64"):
        a = MC.images(Ns, ncoils).astype(MC.dt(Z)[1])
        crop = MC.crop_for(MC.reference(Ns, ncoils, box, Z)[1])
        masks = [~np.abs(M.walsh(a, box, crop=crop, eigh=eigh)[0]).any(axis=0) for eigh in (np.linalg.eigh, jacobi_eigh)]
        print(f"N={Ns} C={ncoils} {Z}: crop {crop:.4f}, masked share {masks[0].mean():.3f}")
        assert 0.2 <= masks[0].mean() <= 0.8 and np.array_equal(masks[0], masks[1])


@pytest.mark.parametrize("D", [1, 2, 3])
def test_calibration_weights(nufft, D):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(D)
    x = rng.random((D, 500)) * 4 * np.pi - 2 * np.pi                   # beyond one period on both sides: the fold matters
    x[:, 0] = 0.0
    folded = np.mod(x + np.pi, 2 * np.pi) - np.pi
    r = np.sqrt((folded ** 2).sum(axis=0)) / np.pi
    cutoff = 0.4
    want = {"hann": np.where(r < cutoff, 0.5 * (1 + np.cos(np.pi * r / cutoff)), 0.0), "box": (r <= cutoff).astype(np.float64)}
    pts = tuple(torch.from_numpy(x[d]) for d in range(D))
    for window in ("hann", "box"):
        for form in (pts, torch.from_numpy(np.ascontiguousarray(x.T))) + ((pts[0],) if D == 1 else ()):
            h = nufft.calibration_weights(form, cutoff=cutoff, window=window).numpy()
            assert h.shape == (500,) and np.abs(h - want[window]).max() <= 8 * EPS and h[0] == 1.0
        assert 0.02 < (want[window] > 0).mean() < 0.98
    with pytest.raises(ValueError):
        nufft.calibration_weights(pts, window="hamming")
    with pytest.raises(ValueError):
        nufft.calibration_weights(pts, cutoff=0.0)


def test_walsh_estimate_against_the_true_maps():
    """A property of the method, printed and not asserted: 2.7e-2 relative L2 on (32, 40), C = 4, box 5 (the noise here
    has unit variance per complex sample, 0.05 / sqrt(2) per part)."""
    Ns, ncoils, box = (32, 40), 4, (5, 5)
    S, _ = MC.truth(Ns, ncoils)
    v = MC.reference(Ns, ncoils, box)[0]
    unit = S / np.sqrt((np.abs(S) ** 2).sum(axis=0))
    s = np.einsum("c...,c...->...", np.conj(unit), v)
    err = np.linalg.norm(unit * (s / np.abs(s)) - v) / np.linalg.norm(unit)
    print(f"Walsh estimate against the true maps (unit norm, phase aligned per cell): relative L2 {err:.3e}")
    assert np.isfinite(err)


def test_header_ctypes_and_library_agree(nufft):
    header = open(os.path.join(ROOT, "include", "nufft_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(nufft.LIB_PATH)
    for name in ENTRY_POINTS:
        proto = re.search(r"\b(int64_t|int32_t|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert proto, name
        nargs = 0 if proto.group(2).strip() == "void" else proto.group(2).count(",") + 1
        res, args = nufft._lib.SYMBOLS[name]
        assert len(args) == nargs, name
        assert res is {"int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int}[proto.group(1)], name
        assert hasattr(raw, name), name
    L = nufft._lib
    for cname, mirror, size in (("nufft_coilmaps_params", L.NufftCoilmapsParams, 40), ("nufft_coilmaps_info", L.NufftCoilmapsInfo, 128)):
        assert getattr(nufft.lib, "nufft_sizeof_" + cname[6:])() == C.sizeof(mirror) == size, cname
        fields = re.search(r"typedef struct " + cname + r" \{(.*?)\}", header, flags=re.S).group(1)
        names = [re.sub(r"\[\d+\]", "", n.strip()) for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f[0].rstrip("_") for f in mirror._fields_], cname
    assert nufft.lib.nufft_version() == 104
    for name in ("CoilMapEstimator", "estimate_maps", "calibration_weights"):
        assert name in nufft.__all__ and hasattr(nufft, name)


def _params(nufft, box=(3, 3, 1), crop=0.0, **kw):
    p = nufft._lib.NufftCoilmapsParams()
    p.struct_size = C.sizeof(nufft._lib.NufftCoilmapsParams)
    for d in range(3):
        p.box[d] = box[d]
    p.crop = crop
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_every_layout_fits(nufft):
    """nufft_coilmaps_layout is the function the kernel launches with.  Over both element types, every C, D = 1, 2, 3, box sides 1, 3, 5,
    9 and array sides 1, 3, 5, 9, 10, 33, 256: the workgroup is whole waves of at most 256 threads, a team has at least C lanes, the tiles
    cover the array, a staged tile is no smaller than the teams (or is the whole array), and LDS holds what DESIGN.md §28 lists -- the
    staged halo tile, H and V of every team, the partial maxima -- within the 160 KiB of a compute unit."""
    L, lib = nufft._lib, nufft.lib
    info = L.NufftCoilmapsInfo()
    sides, boxes = (1, 3, 5, 9, 10, 33, 256), (1, 3, 5, 9)
    seen = staged = 0
    for D in (1, 2, 3):
        shapes = [(a,) + (b if D > 1 else 1,) + (c if D > 2 else 1,) for a in sides for b in (sides if D > 1 else (1,)) for c in (sides if D > 2 else (1,))]
        if D == 3:
            shapes = shapes[::5]                                     # every fifth of the 343 shapes: every side in every position
        for N in shapes:
            for box in [(a, b, c) for a in boxes for b in (boxes if D > 1 else (1,)) for c in (boxes if D > 2 else (1,))]:
                if any(b > n for b, n in zip(box, N)):
                    continue
                prm = _params(nufft, box=box)
                for dtype, eb in ((L.F32, 8), (L.F64, 16)):
                    for ncoils in (range(1, 33) if D < 3 else (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32)):
                        info.struct_size = C.sizeof(info)
                        assert lib.nufft_coilmaps_layout(dtype, D, (C.c_int64 * 3)(*N), ncoils, C.byref(prm), C.byref(info)) == L.OK
                        threads, tile = info.teams * info.team_lanes, tuple(info.tile)
                        assert threads % 64 == 0 and 64 <= threads <= 256 and ncoils <= info.team_lanes < 2 * max(ncoils, 1) + 1
                        assert info.tile_cells == tile[0] * tile[1] * tile[2] >= 1 and all(1 <= t <= max(n, 1) for t, n in zip(tile, N))
                        groups = 1
                        for t, n in zip(tile, N):
                            groups *= -(-n // t)
                        assert info.workgroups == groups and info.cells == N[0] * N[1] * N[2] and info.device == -1
                        halo = 1
                        for t, b in zip(tile, box):
                            halo *= t + b - 1
                        need = info.teams * ncoils * ncoils * 32 + info.teams * 12 + (ncoils * halo * eb if info.staged else 0)
                        assert need <= info.lds_bytes <= 160 << 10, (dtype, ncoils, N, box, need, info.lds_bytes)
                        assert info.workspace_bytes >= 12 * groups + 16
                        seen += 1
                        staged += info.staged
    print(f"{seen} layouts, {staged} staged")
    assert seen > 20000 and 0 < staged < seen


def test_refusals_without_a_device(nufft):
    """Null arguments and the arguments (INVALID_ARG), then the limits (UNSUPPORTED), and the missing device last."""
    L, lib = nufft._lib, nufft.lib
    h = C.c_void_p()
    N = (C.c_int64 * 3)(12, 10, 1)
    create = lambda C_=3, prm=None, dtype=L.F64, D=2, n=N: lib.nufft_coilmaps_create(C.byref(h), dtype, D, n, C_, -1, C.byref(prm or _params(nufft)))   # noqa: E731
    assert lib.nufft_coilmaps_create(None, L.F64, 2, N, 3, -1, C.byref(_params(nufft))) == L.ERR_INVALID_ARG
    assert lib.nufft_coilmaps_create(C.byref(h), L.F64, 2, None, 3, -1, C.byref(_params(nufft))) == L.ERR_INVALID_ARG
    assert lib.nufft_coilmaps_create(C.byref(h), L.F64, 2, N, 3, -1, None) == L.ERR_INVALID_ARG
    # the arguments come before the limits: each of these with 33 coils as well
    for coils in (3, 33):
        assert create(coils, _params(nufft, struct_size=8)) == L.ERR_INVALID_ARG
        assert create(coils, dtype=7) == L.ERR_INVALID_ARG and create(coils, D=0) == L.ERR_INVALID_ARG and create(coils, D=4) == L.ERR_INVALID_ARG
        assert create(coils, n=(C.c_int64 * 3)(12, 0, 1)) == L.ERR_INVALID_ARG
        for box in ((4, 3, 1), (3, 0, 1), (3, -3, 1), (3, 3, 3)):
            assert create(coils, _params(nufft, box=box)) == L.ERR_INVALID_ARG, box
        for crop in (-0.1, float("nan"), float("inf")):
            assert create(coils, _params(nufft, crop=crop)) == L.ERR_INVALID_ARG, crop
    assert create(0) == L.ERR_INVALID_ARG and create(-1) == L.ERR_INVALID_ARG
    assert create(33) == L.ERR_UNSUPPORTED and b"33 coils" in lib.nufft_last_error_message()
    for box in ((11, 3, 1), (3, 11, 1), (9, 9, 1), (13, 3, 1)):                          # above 9, or above N_d (N_1 = 12, N_2 = 10: 11 is both)
        expect = L.ERR_NO_DEVICE if box == (9, 9, 1) else L.ERR_UNSUPPORTED
        assert create(3, _params(nufft, box=box)) == expect, box
    assert create(3, _params(nufft, box=(9, 9, 1)), n=(C.c_int64 * 3)(12, 7, 1)) == L.ERR_UNSUPPORTED     # 9 > N_2 = 7
    for coils in (1, 3, 32):
        assert create(coils) == L.ERR_NO_DEVICE and not h.value
    assert create(3, _params(nufft, box=(3, 3, 0))) == L.ERR_NO_DEVICE                   # 0 beyond the dimensions reads as 1
    # from a host-only operator
    plan = nufft.PlanNUFFT(np.complex128, (12, 10), backend=None)
    real = nufft.PlanNUFFT(np.float64, (12, 10), backend=None)
    op = nufft.ToeplitzOperator(plan)
    make = lib.nufft_coilmaps_create_for_operator
    assert make(C.byref(h), None, 3, C.byref(_params(nufft))) == L.ERR_INVALID_ARG and make(C.byref(h), op._handle, 3, None) == L.ERR_INVALID_ARG
    assert make(C.byref(h), op._handle, 3, C.byref(_params(nufft, box=(2, 3, 1)))) == L.ERR_INVALID_ARG
    assert make(C.byref(h), op._handle, 33, C.byref(_params(nufft))) == L.ERR_UNSUPPORTED
    assert make(C.byref(h), op._handle, 3, C.byref(_params(nufft))) == L.ERR_NO_DEVICE and not h.value
    # the layout alone: the same checks in the same order, and no device asked for
    info = L.NufftCoilmapsInfo()
    lay = lambda C_=3, prm=None, n=N: lib.nufft_coilmaps_layout(L.F64, 2, n, C_, C.byref(prm or _params(nufft)), C.byref(info))   # noqa: E731
    assert lib.nufft_coilmaps_layout(L.F64, 2, N, 3, C.byref(_params(nufft)), None) == L.ERR_INVALID_ARG
    assert lay(33, _params(nufft, box=(4, 3, 1))) == L.ERR_INVALID_ARG and lay(33) == L.ERR_UNSUPPORTED and lay(3, _params(nufft, box=(3, 11, 1))) == L.ERR_UNSUPPORTED
    assert lay(3, _params(nufft, crop=0.1)) == L.OK and (info.ncoils, info.cells, info.device, info.crop) == (3, 120, -1, 0.1)
    assert info.workspace_bytes >= 120 * 8 and info.struct_size == C.sizeof(info) and info.jacobi_sweeps_max == 24
    # the other entry points
    assert lib.nufft_coilmaps_apply_crop(None, None, None, 0.1, None) == L.ERR_INVALID_ARG
    assert lib.nufft_coilmaps_estimate(None, None, None, None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_coilmaps_get_info(None, None) == L.ERR_INVALID_ARG and lib.nufft_coilmaps_last_sweeps(None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_coilmaps_destroy(None) == L.OK
    # the Python layer refuses the same way; a real-data plan is refused there (the C call has no plan to look at)
    for bad in (lambda: nufft.CoilMapEstimator(plan, 3), lambda: nufft.CoilMapEstimator(op, 3), lambda: nufft.CoilMapEstimator(plan, 33),
                lambda: nufft.CoilMapEstimator(plan, 3, box=4), lambda: nufft.CoilMapEstimator(plan, 3, box=(3, 3, 3)),
                lambda: nufft.CoilMapEstimator(plan, 3, box=3.0), lambda: nufft.CoilMapEstimator(real, 3), lambda: nufft.CoilMapEstimator(None, 3),
                lambda: nufft.CoilMapEstimator(plan, True)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="complex plan"):
        nufft.CoilMapEstimator(real, 3)
    for o in (op, plan, real):
        o.close()
