"""Boundary and degenerate point sets (tests/boundary_cases.py) through every spreading and interpolation engine and every sort,
against the oracle at the bounds of tests/test_gpu_parity.py (the reference's own: rtol 1e-7 for Float64, 1e-5 for Float32 on the
2-norm).  The other parity tests draw continuous point distributions in the thousands; here the points sit ON the period boundary
and on bin / column / tile / layer edges, coincide, fill one plane / layer / column / line only, or are 0, 1, 2, 63, 64, 65 in number.

One test function per engine row, one plan per test, all point sets on that plan in the order of boundary_cases.ORDER; then the
stale-table sequence (a uniform set of 20 000 points, one point, no point, the uniform set again: task tables, offsets, device flags and
the steady-path streak of the large set must not leak into the small ones, nor theirs into it), then a second plan whose FIRST point
set is empty (no point buffers allocated yet) followed by `faces`.

Per set: set_points on the plan and the oracle; the engine / sort read-backs EQUAL what the row forces (an assertion, not a filter: the
forcing recipes are those of the instantiation tests of tests/test_gpu_parity.py, and a forced engine serves every point set); type 1
and / or type 2 against the oracle.  Outputs are pre-filled with NaN, so an element a kernel does not write fails the comparison.
Sets of boundary points and coincident sets: outputs finite; coincident sets: every type-2 output equals output 0; the empty set: the
type-1 output is exactly zero and the type-2 output is empty.  The oracle is the C one where it is built and the plan's oracle is
Float64, the numpy one otherwise; both are checked on these sets by tests/test_boundary_cases_host.py.

Every figure is printed before it is asserted (`pytest -s`); each test ends with a line `boundary <row> ...: worst ...`.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_cases as BC  # noqa: E402
from test_gpu_parity import _make_case, _oracle_inputs, _rel, _rtol, plan_real_dtype  # noqa: E402

from oracle import c_oracle as CO  # noqa: E402
from oracle import nufft_oracle as O  # noqa: E402

f32, c64, f64, c128 = np.float32, np.complex64, np.float64, np.complex128
DIRECT, FAST = O.DIRECT, O.FAST_APPROXIMATION
ALL_Z = [f32, c64, f64, c128]


def _mode(M):
    """Both window evaluations over the matrix: Direct for M <= 4, the piecewise polynomials (whose argument 2X - 1 is exactly 1 at the
    clamp) above."""
    return DIRECT if M <= 4 else FAST


def _is_f64(Z):
    return plan_real_dtype(Z) == np.float64


def _seed(row, Z, M, C=1):
    """One seed per (row, element type, M, components): stable across runs and processes."""
    return 5000 + 7 * sum(map(ord, row)) + 31 * M + 101 * C + np.dtype(Z).itemsize


def _assert(cond, *what):
    assert cond, what


class _Runner:
    """The steps of one row on one oracle plan; references are computed once per set name and kept."""

    def __init__(self, row, nufft, oplan, Z, C, seed, types, expect):
        self.row, self.nufft, self.oplan, self.Z, self.C, self.seed = row, nufft, oplan, np.dtype(Z), C, seed
        self.types, self.expect = types, expect
        self.backend = CO if (CO.available() and np.dtype(oplan.dtype) == np.float64) else O
        self.refs = {}
        self.worst = {1: (0.0, None), 2: (0.0, None)}
        self.readbacks = []
        self.ws = None

    def spectra(self, plan, sets):
        if self.oplan.is_real:
            exact = lambda xs, w: O.nudft_type2_real(self.oplan, xs, w)                        # noqa: E731
        else:
            exact = lambda xs, w: O.nudft_type2(self.oplan.ks, xs, w)                          # noqa: E731
        self.ws = [BC.spectrum(self.Z, plan.shape, self.seed + c, exact=exact, sets=sets) for c in range(self.C)]
        self.wd = tuple(torch.from_numpy(w).to(plan.device) for w in self.ws)

    def _tup(self, t):
        return t if self.C > 1 else t[0]

    def reference(self, name, xs):
        if name not in self.refs:
            Np = len(xs[0])
            vs = [BC.values(self.Z, Np, self.seed + c) for c in range(self.C)]
            O.set_points(self.oplan, xs)
            ref1 = ref2 = None
            if 1 in self.types:
                ref1 = self.backend.exec_type1(self.oplan, self._tup(_oracle_inputs(self.oplan, vs)))
                ref1 = ref1 if self.C > 1 else [ref1]
            if 2 in self.types:
                ref2 = self.backend.exec_type2(self.oplan, self._tup(_oracle_inputs(self.oplan, self.ws)))
                ref2 = ref2 if self.C > 1 else [ref2]
            self.refs[name] = (vs, ref1, ref2)
        return self.refs[name]

    def step(self, plan, name, xs, label=None):
        """set_points + read-backs + the row's transforms of set `name` on `plan`, against the oracle; returns the outputs (numpy)."""
        nufft, C, Z = self.nufft, self.C, self.Z
        label = label or name
        dev = plan.device
        Np = len(xs[0])
        vs, ref1, ref2 = self.reference(name, xs)
        nufft.set_points(plan, tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs))
        self.readbacks.append((label, self.expect(plan, name, Np)))
        tol = _rtol(Z)
        got1 = got2 = None
        if 1 in self.types:
            us = tuple(torch.full(plan.shape, float("nan"), dtype=plan.eltype, device=dev) for _ in range(C))
            nufft.exec_type1(self._tup(us), plan, self._tup(tuple(torch.from_numpy(v).to(dev) for v in vs)))
            got1 = [u.cpu().numpy() for u in us]
            for c in range(C):
                if Np == 0:
                    assert not got1[c].any() and not np.asarray(ref1[c]).any(), (self.row, label, c)      # exactly zero, both
                    continue
                e = _rel(got1[c], ref1[c])
                print(f"boundary {self.row} {Z.name} {label}[{c}]: type 1 against the oracle {e:.2e}")
                if e > self.worst[1][0] or not np.isfinite(e):
                    self.worst[1] = (e, label)
                assert e < tol, (self.row, label, "type 1", c, e)
                if name in BC.BOUNDARY_ONLY:
                    assert np.isfinite(got1[c]).all(), (self.row, label, "type 1", c)
        if 2 in self.types:
            outs = tuple(torch.full((Np,), float("nan"), dtype=plan.Z, device=dev) for _ in range(C))
            nufft.exec_type2(self._tup(outs), plan, self._tup(self.wd))
            got2 = [o.cpu().numpy() for o in outs]
            for c in range(C):
                assert got2[c].shape == (Np,) and len(ref2[c]) == Np
                if Np == 0:
                    continue
                e = _rel(got2[c], ref2[c])
                print(f"boundary {self.row} {Z.name} {label}[{c}]: type 2 against the oracle {e:.2e}")
                if e > self.worst[2][0] or not np.isfinite(e):
                    self.worst[2] = (e, label)
                assert e < tol, (self.row, label, "type 2", c, e)
                if name in BC.BOUNDARY_ONLY:
                    assert np.isfinite(got2[c]).all(), (self.row, label, "type 2", c)
                if name in BC.COINCIDENT:
                    spread = float(np.abs(got2[c] - got2[c][0]).max() / np.abs(got2[c][0]))
                    assert spread < tol, (self.row, label, "type-2 outputs of coincident points differ", c, spread)
        return got1, got2


def _drive(row, Z, dims, M, monkeypatch, *, env=None, types=(1,), expect, C=1, evalmode=None, check_info=None, before=None, after=None,
           on_set=None, **kw):
    """One row: the plan, every point set, the stale-table sequence, and the plan that starts empty.  `expect(plan, name, Np)` asserts
    the read-backs and returns what it read (kept for the messages); `before` / `after(plan, run, big)` are the row's own steps around the loop;
    `on_set(plan, name, xs)` its extra checks per set."""
    for var in ("NUFFT_INTERP_MARCH", "NUFFT_SMARCH_HALO", "NUFFT_SMARCH_SPLIT", "NUFFT_INTERP_SPLIT", "NUFFT_DENSE_MIN", "NUFFT_COARSE_SORT",
                "NUFFT_SLAB_SORT", "NUFFT_SLAB_MIN_POINTS", "NUFFT_PATCH_F32ACC", "NUFFT_SMARCH_HALO_FUSE", "NUFFT_STEADY_PATH", "NUFFT_SPREAD_METHOD"):
        monkeypatch.delenv(var, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    evalmode = _mode(M) if evalmode is None else evalmode
    seed = _seed(row, Z, M, C)
    nufft, plan, oplan, _, _ = _make_case(Z, dims, M, 2.0, evalmode, C, 1, seed, **kw)
    if check_info:
        check_info(plan.info())
    T, D = plan_real_dtype(Z), len(dims)
    geom = BC.geometry(plan.info(), D)
    sets = BC.point_sets(T, plan.oversampled_dims, geom, seed)
    big = BC.uniform_set(T, D, seed)
    run = _Runner(row, nufft, oplan, Z, C, seed, types, expect)
    if 2 in types:
        run.spectra(plan, sets)
    if before:
        before(plan, run, big)
    for name, xs in sets.items():
        run.step(plan, name, xs)
        if on_set:
            on_set(plan, name, xs)
    # stale tables: a large set, one point, no point, the large set again — all against the oracle, the two large results against each other
    first = run.step(plan, "uniform", big, "uniform (first)")
    run.step(plan, "tiny_1", sets["tiny_1"], "tiny_1 after uniform")
    run.step(plan, "tiny_0", sets["tiny_0"], "tiny_0 after tiny_1")
    again = run.step(plan, "uniform", big, "uniform (again)")
    same = 1e-12 if _is_f64(Z) else 5e-6          # (tests/test_gpu_robustness.py, tests/test_gpu_consistency.py: the same transform twice)
    for a, b in zip(first, again):
        if a is not None:
            for c in range(C):
                e = _rel(b[c], a[c])
                print(f"boundary {row} {np.dtype(Z).name} uniform again[{c}] against the first {e:.2e}")
                assert e < same, (row, "the uniform set after tiny_1 and tiny_0 against itself before them", c, e)
    if after:
        after(plan, run, big)
    plan.close()
    # a plan whose first point set is empty (nothing allocated for points yet), then boundary points
    _, plan2, _, _, _ = _make_case(Z, dims, M, 2.0, evalmode, C, 1, seed, **kw)
    run.step(plan2, "tiny_0", sets["tiny_0"], "tiny_0 first")
    run.step(plan2, "faces", sets["faces"], "faces after tiny_0 first")
    plan2.close()
    print(f"boundary {row} {np.dtype(Z).name} M={M} mode={evalmode}: worst type 1 {run.worst[1][0]:.2e} ({run.worst[1][1]}), "
          f"type 2 {run.worst[2][0]:.2e} ({run.worst[2][1]}) [bound {_rtol(Z):.0e}]")
    return run


def _spread_is(engine):
    def expect(plan, name, Np):
        got = plan.spread_engine_used()
        assert got == engine, (name, Np, got)
        return got
    return expect


def _interp_is(engine):
    def expect(plan, name, Np):
        got = plan.interp_engine_used()
        assert got == engine, (name, Np, got)
        return got
    return expect


# ---- row 1: LDS-tile spreading ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,evalmode", [(2, DIRECT), (2, FAST), (7, FAST)])
@pytest.mark.parametrize("Z", ALL_Z)
def test_lds_tile_spreading(Z, M, evalmode, monkeypatch):
    _drive("lds-tiles", Z, (48, 40, 56), M, monkeypatch, evalmode=evalmode, expect=_spread_is("lds_tiles"), spread_method="lds_tiles",
           check_info=lambda i: _assert(i.spread_method == 1))


# ---- row 2: MFMA patches (Float64 accumulators, Float32 accumulators, planar components) ----------------------------------------------
@pytest.mark.parametrize("Z,M", [(Z, M) for Z in (f32, c64, "complex64/f64acc", f64, c128) for M in (4, 7)] + [("float64/planar", 4)])
def test_mfma_patches(Z, M, monkeypatch):
    env, C, f32acc = {}, 1, None
    if Z == "complex64/f64acc":
        Z, f32acc, env = c64, 0, {"NUFFT_PATCH_F32ACC": "0"}
    elif Z == "float64/planar":
        Z, C = f64, 2
    elif np.dtype(Z) == c64:
        f32acc = 1

    def check_info(i):
        assert i.spread_method == 2 and i.patch_planar == (C if C > 1 else 0)
        if f32acc is not None:
            assert i.patch_f32acc == f32acc

    _drive("mfma-patches" + ("-f64acc" if f32acc == 0 else "-planar" if C > 1 else ""), Z, (48, 48, 48), M, monkeypatch, env=env, C=C,
           expect=_spread_is("mfma_patches"), spread_method="mfma_patches", check_info=check_info)


# ---- rows 3 - 5: the spreading window: clipped columns, halo variant, dense-set engine --------------------------------------------------
@pytest.mark.parametrize("M", [4, 7])
@pytest.mark.parametrize("Z", [f32, f64, c128])
def test_spreading_window_clipped(Z, M, monkeypatch):
    _drive("window-clipped", Z, (48, 40, 56), M, monkeypatch, env={"NUFFT_SMARCH_HALO": "0"}, expect=_spread_is("marching_ring"),
           spread_method="marching_ring", check_info=lambda i: _assert(i.spread_method == 3 and i.ring_column[0] > 0 and i.ring_halo == 0))


@pytest.mark.parametrize("M", [4, 7])
@pytest.mark.parametrize("Z", [f32, f64, c128])
def test_spreading_window_halo(Z, M, monkeypatch):
    _drive("window-halo", Z, (48, 48, 56), M, monkeypatch, env={"NUFFT_SMARCH_HALO": "2"}, expect=_spread_is("marching_ring"),
           spread_method="marching_ring", check_info=lambda i: _assert(i.spread_method == 3 and i.ring_halo == 1, list(i.ring_column)))


@pytest.mark.parametrize("M", [3, 5])
@pytest.mark.parametrize("Z", [f32, f64])
def test_dense_set_engine(Z, M, monkeypatch):
    _drive("window-dense", Z, (48, 48, 56), M, monkeypatch, env={"NUFFT_SMARCH_HALO": "2", "NUFFT_DENSE_MIN": "0"},
           expect=_spread_is("marching_ring_dense"), spread_method="marching_ring",
           check_info=lambda i: _assert(i.spread_method == 3 and i.ring_halo == 1, list(i.ring_column)))


# ---- rows 6 - 7: interpolation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [4, 7])
@pytest.mark.parametrize("Z", ALL_Z)
def test_interpolation_lds_tiles(Z, M, monkeypatch):
    _drive("interp-tiles", Z, (48, 40, 56), M, monkeypatch, env={"NUFFT_INTERP_MARCH": "0"}, types=(2,), expect=_interp_is("lds_tiles"))


@pytest.mark.parametrize("M", [4, 7])
@pytest.mark.parametrize("Z", ALL_Z)
def test_interpolation_ring(Z, M, monkeypatch):
    _drive("interp-ring", Z, (48, 40, 56), M, monkeypatch, env={"NUFFT_INTERP_MARCH": "2"}, types=(2,), expect=_interp_is("marching_ring"))


# ---- row 8: column-layer sort, staged interpolation ring, steady path of set_points ------------------------------------------------------
@pytest.mark.parametrize("Z", [f64, f32])
def test_column_layer_sort_staged_ring_and_steady_path(Z, monkeypatch):
    """(64, 64, 32): the smallest grid with a column-layer sort.  Both rings are forced, so both serve every point set and every set
    keeps the column-layer sort: asserted.  Whether a set takes the steady path of set_points depends on what the device reported for
    the sets before it; it is recorded (and printed) per set and asserted where the code makes it certain: after four uniform sets in a
    row it is taken, a set without points never takes it, and uniform sets behind the whole sequence re-enter it."""
    steady = []

    def expect(plan, name, Np):
        got = (plan.spread_engine_used(), plan.interp_engine_used(), plan.sort_columns_used(), plan.steady_path_used())
        steady.append((name, Np, got[3]))
        assert got[:3] == ("marching_ring", "marching_ring", True), (name, Np, got, steady)
        assert not (Np == 0 and got[3]), (name, steady)
        return got

    def check_info(i):
        assert i.spread_method == 3 and i.ring_halo == 1 and i.sort_column[0] > 0, (list(i.ring_column), list(i.sort_column))

    def to_steady(plan, run, big):
        for k in range(4):
            run.step(plan, "uniform", big, f"uniform (steady-path run-up {k + 1})")
        assert plan.steady_path_used(), steady

    def back_to_steady(plan, run, big):
        # ("uniform (again)" was the first uniform set behind tiny_0: three more on the full path at most, then the steady path)
        for k in range(4):
            run.step(plan, "uniform", big, f"uniform (re-entry {k + 1})")
        assert plan.steady_path_used(), steady

    run = _drive("column-layers", Z, (64, 64, 32), 4, monkeypatch, env={"NUFFT_SMARCH_HALO": "2", "NUFFT_INTERP_MARCH": "2"}, types=(1, 2),
                 evalmode=DIRECT if _is_f64(Z) else FAST, expect=expect, spread_method="marching_ring", check_info=check_info,
                 before=to_steady, after=back_to_steady)
    print("boundary column-layers steady path per set:", [(lab, rb[3]) for lab, rb in run.readbacks])


# ---- row 9: slab sort -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Z,M", [(f64, 4), (f32, 5)])
def test_slab_sort(Z, M, monkeypatch):
    """The two-level slab sort (forced as tests/test_gpu_parity.py::test_two_level_slab_sort_reproduces_the_fine_sort forces it) takes
    every set that has a point; the empty set takes the fine sort, whose launches all depend on Np > 0.  On the sets of edge points,
    the coincident sets and `column` the sort result is restated as in test_bin_sort_is_a_permutation_grouped_by_bin (which clamps like
    cell_of): a bijection, offsets = the bin counts.  On `nodes` a point counts as placed correctly if it lies in the bin of its oracle
    cell or, per dimension, of the neighbouring cell across the node it was built from (cell + 1 for the step below the node, cell - 1
    for the step above it) — an allowance for a last-bit difference in (x / 2 pi) N; bijection and total stay exact."""
    T = plan_real_dtype(Z)

    def expect(plan, name, Np):
        got = plan.sort_method_used()
        assert got == ("slabs" if Np > 0 else "fine_bins"), (name, Np, got)
        return got

    def on_set(plan, name, xs):
        if name not in ("faces", "nodes", "column") + BC.COINCIDENT:
            return
        from nufft_pkg import nufft
        Np = len(xs[0])
        perm, offs = nufft.sort_result(plan)
        offs = offs.astype(np.int64)
        assert np.array_equal(np.sort(perm), np.arange(Np)), name                                  # bijection
        assert offs[0] == 0 and offs[-1] == Np and np.all(np.diff(offs) >= 0), name
        info, Nover = plan.info(), plan.oversampled_dims
        cells = [np.minimum(O.point_to_cell(O.to_unit_cell(xs[d]), Nover[d])[0], Nover[d] - 1) for d in range(3)]

        def bins_of(cs):
            return sum(m * (c // info.bin_dims[d]) for d, (c, m) in enumerate(zip(cs, (1, info.nbins[0], info.nbins[0] * info.nbins[1]))))

        pos = np.empty(Np, dtype=np.int64)
        pos[perm] = np.arange(Np)
        got_bin = np.searchsorted(offs, pos, side="right") - 1                                      # the bin whose range holds the point
        if name != "nodes":
            assert np.array_equal(got_bin, bins_of(cells)), name
            assert np.array_equal(np.diff(offs), np.bincount(bins_of(cells), minlength=len(offs) - 1)), name
            return
        geom = BC.geometry(info, 3)
        _, nudges = BC.node_nudges(T, Nover, geom, _seed("slab-sort", Z, M))
        ok = np.zeros(Np, dtype=bool)
        for mask in range(8):                                                                       # every combination of allowed neighbours
            alt = [(cells[d] - nudges[d]) % Nover[d] if mask >> d & 1 else cells[d] for d in range(3)]
            ok |= got_bin == bins_of(alt)
        exact = int((got_bin == bins_of(cells)).sum())
        print(f"boundary slab-sort {np.dtype(Z).name} nodes: {exact} of {Np} points in the bin of their oracle cell, {int(ok.sum())} with the allowance")
        assert ok.all(), (name, np.flatnonzero(~ok)[:10])

    _drive("slab-sort", Z, (40, 36, 50), M, monkeypatch, env={"NUFFT_COARSE_SORT": "0", "NUFFT_SLAB_MIN_POINTS": "0"}, types=(1, 2),
           evalmode=FAST if _is_f64(Z) else DIRECT, expect=expect, on_set=on_set)


# ---- row 10: 1-D and 2-D tile kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Z", [c64, f64])
@pytest.mark.parametrize("dims", [(100,), (37, 41)])
def test_one_and_two_dimensional_tile_kernels(dims, Z, monkeypatch):
    def expect(plan, name, Np):
        got = (plan.spread_engine_used(), plan.interp_engine_used())
        assert got == ("lds_tiles", "lds_tiles"), (name, Np, got)
        return got

    _drive(f"tiles-{len(dims)}d", Z, dims, 4, monkeypatch, types=(1, 2), expect=expect)
