"""CPU side of tests/test_gpu_boundary.py: the point sets of tests/boundary_cases.py reach what they are for (the clamp of the cell
index, the period boundary, both sides of every bin / column / tile / layer edge of the plans that the GPU test creates), and the
reference itself is right on them: the Float64 oracle against the exact sums, the Float32 oracle against the Float64 oracle that
locates the points in Float32 — inside the bounds the GPU test holds the kernels to."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_cases as BC  # noqa: E402

from oracle import c_oracle as CO  # noqa: E402
from oracle import nufft_oracle as O  # noqa: E402

SEED = 4100
DIMS = (48, 40, 56)

# (dims, spread_method, switches) of the plans of tests/test_gpu_boundary.py whose edges differ
GEOMETRY_PLANS = [
    ((48, 40, 56), "lds_tiles", {}),
    ((48, 48, 48), "mfma_patches", {}),
    ((48, 40, 56), "marching_ring", {"NUFFT_SMARCH_HALO": "0"}),
    ((48, 48, 56), "marching_ring", {"NUFFT_SMARCH_HALO": "2"}),
    ((64, 64, 32), "marching_ring", {"NUFFT_SMARCH_HALO": "2", "NUFFT_INTERP_MARCH": "2"}),
    ((40, 36, 50), "auto", {"NUFFT_COARSE_SORT": "0", "NUFFT_SLAB_MIN_POINTS": "0"}),
    ((37, 41), "auto", {}),
    ((100,), "auto", {}),
]


def _clear_switches(nufft, monkeypatch):
    for var in list(os.environ):
        if var.startswith("NUFFT_") and var not in nufft.plan._HARNESS_ENV:
            monkeypatch.delenv(var)


def _cells(x, N):
    """The oracle's cell of every coordinate: fold, (x / 2 pi) N, truncate, clamp (oracle.evaluate_window)."""
    i, _ = O.point_to_cell(O.to_unit_cell(x), N)
    return np.minimum(i, N - 1)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_faces_reach_the_clamp_the_origin_and_the_last_number_of_the_period(T):
    L = T(O.TWO_PI)
    fv = BC.face_values(T)
    assert np.all(np.isfinite(fv)) and np.finfo(T).tiny < 1e-30           # -1e-30 is a normal number in both precisions
    assert O.to_unit_cell(np.array([T(-1e-30)], dtype=T))[0] == L            # L + r rounds to L: the clamp path, X = 1
    xs = BC.point_sets(T, [2 * n for n in DIMS], {"bin_dims": [4, 4, 4]}, SEED)["faces"]
    assert len(xs) == 3 and all(len(x) == BC.N_FACES for x in xs)
    for d, x in enumerate(xs):
        f = O.to_unit_cell(x)
        assert np.any(f == L) and np.any(x == 0) and np.any(np.signbit(x) & (x == 0)) and np.any(x == np.nextafter(L, T(0))), d
        N = 2 * DIMS[d]
        i, r = O.point_to_cell(f, N)
        assert np.any(i == N) and np.all(_cells(x, N) <= N - 1)                # r == N exists and is clamped to the last cell
        assert np.all((f >= 0) & (f <= L))
    # points with all D coordinates on a face value that folds to the period boundary exist too
    allL = np.logical_and.reduce([O.to_unit_cell(x) == L for x in xs])
    assert allL.any()


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("dims,method,switches", GEOMETRY_PLANS, ids=[f"{'x'.join(map(str, g[0]))}-{g[1]}" for g in GEOMETRY_PLANS])
def test_nodes_sit_on_both_sides_of_every_edge(dims, method, switches, T, monkeypatch):
    """For every edge distance of the plan's geometry and every dimension: at least one multiple m of it with a point whose oracle
    cell is m (the edge cell) and a point whose oracle cell is m - 1 (the cell below), and likewise at the period boundary (cells 0 and
    N - 1)."""
    from nufft_pkg import nufft
    _clear_switches(nufft, monkeypatch)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    plan = nufft.PlanNUFFT(T, dims, m=4, sigma=2.0, spread_method=method, backend=None)
    D = len(dims)
    Nover = plan.oversampled_dims
    geom = BC.geometry(plan.info(), D)
    assert all(geom["bin_dims"][d] > 0 for d in range(D))
    if "NUFFT_INTERP_MARCH" in switches:
        assert geom["sort_column"][0] > 0 and geom["ring_column"][0] > 0, geom      # the column-layer plan: its columns are edges too
    if method == "marching_ring":
        assert geom["ring_column"][0] > 0, geom
    xs = BC.point_sets(T, Nover, geom, SEED)["nodes"]
    nodes, nudges = BC.node_nudges(T, Nover, geom, SEED)
    for d in range(D):
        N = Nover[d]
        cells = _cells(xs[d], N)
        present = set(cells.tolist())
        assert 0 in present and N - 1 in present, d
        for name, s in BC.edge_strides(geom, d, N).items():
            both = [m for m in range(s, N, s) if m in present and m - 1 in present]
            assert both, (d, name, s)
        # every variant of node i lands in cell i or in the cell below it (the last cell for node 0): (x / 2 pi) N rounds, so one step
        # of the number format does not always change the cell — which side a point falls on is the oracle's to say, here and on the GPU
        assert np.all((cells == nodes[d]) | (cells == (nodes[d] - 1) % N)), d
        assert np.any(cells[nudges[d] == -1] == (nodes[d][nudges[d] == -1] - 1) % N) and np.any(cells[nudges[d] == 1] == nodes[d][nudges[d] == 1]), d


def _oracle_plans(M, evalmode):
    """The real Float64 plan of the exact-sum check."""
    return O.OraclePlan(DIMS, is_real=True, dtype=np.float64, M=M, sigma=2.0, evalmode=evalmode)


@pytest.fixture(scope="module")
def f64_case():
    oplan = _oracle_plans(7, O.DIRECT)
    sets = BC.point_sets(np.float64, oplan.Nover, {"bin_dims": [4, 4, 4], "ring_column": [32, 32, 0]}, SEED)
    w = BC.spectrum(np.float64, tuple(reversed(oplan.size)), SEED, exact=lambda xs, w: O.nudft_type2_real(oplan, xs, w), sets=sets)
    return oplan, sets, w


@pytest.mark.parametrize("name", BC.BOUNDARY_ONLY)
def test_float64_oracle_matches_the_exact_sums_on_boundary_points(f64_case, name):
    """Float64, M = 7, sigma = 2, Direct: both transforms of the oracle (numpy, and C where built) against the exact sums on the
    folded points, to the reference's own bound for points at the period boundary (test/near_2pi.jl:69: 1e-11)."""
    oplan, sets, w = f64_case
    xs = sets[name]
    v = BC.values(np.float64, len(xs[0]), SEED)
    folded = [O.to_unit_cell(x) for x in xs]
    exact1 = O.nudft_type1(oplan.ks, folded, v)
    exact2 = O.nudft_type2_real(oplan, folded, w)
    O.set_points(oplan, xs)
    e1, e2 = BC.rel(O.exec_type1(oplan, v), exact1), BC.rel(O.exec_type2(oplan, w), exact2)
    print(f"{name}: numpy oracle type 1 {e1:.2e}, type 2 {e2:.2e}")
    assert e1 < 1e-11 and e2 < 1e-11, (e1, e2)
    if CO.available():
        c1, c2 = BC.rel(CO.exec_type1(oplan, v), exact1), BC.rel(CO.exec_type2(oplan, w), exact2)
        print(f"{name}: C oracle type 1 {c1:.2e}, type 2 {c2:.2e}")
        assert c1 < 1e-11 and c2 < 1e-11, (c1, c2)


@pytest.fixture(scope="module")
def f32_case():
    M = 4                                                                 # (Float32 windows overflow from M = 6 on in three dimensions)
    o32 = O.OraclePlan(DIMS, is_real=True, dtype=np.float32, M=M, sigma=2.0, evalmode=O.DIRECT)
    o64 = O.OraclePlan(DIMS, is_real=True, dtype=np.float64, coord_dtype=np.float32, M=M, sigma=2.0, evalmode=O.DIRECT)
    assert o32.Nover == o64.Nover
    sets = BC.point_sets(np.float32, o32.Nover, {"bin_dims": [4, 4, 4], "ring_column": [32, 32, 0]}, SEED)
    w = BC.spectrum(np.float32, tuple(reversed(o32.size)), SEED, exact=lambda xs, w: O.nudft_type2_real(o64, xs, w), sets=sets)
    return o32, o64, sets, w


@pytest.mark.parametrize("name", BC.ORDER)
def test_float32_oracle_stays_within_the_float32_bound_of_the_float64_oracle(f32_case, name):
    """Every set: the Float32 oracle against the Float64 oracle that locates the Float32 points in Float32 (`coord_dtype`), bound 1e-5 —
    the reference alone stays inside the bound the GPU test applies to Float32 plans (many equal terms of one sign in a coincident
    set: the Float32 sums themselves)."""
    o32, o64, sets, w = f32_case
    xs = sets[name]
    Np = len(xs[0])
    v = BC.values(np.float32, Np, SEED)
    O.set_points(o32, xs)
    O.set_points(o64, xs)
    u32, u64 = O.exec_type1(o32, v), O.exec_type1(o64, v.astype(np.float64))
    out32, out64 = O.exec_type2(o32, w), O.exec_type2(o64, w.astype(np.complex128))
    assert u32.shape == u64.shape and len(out32) == len(out64) == Np
    if Np == 0:
        assert not u32.any() and not u64.any()
        if CO.available():
            assert not CO.exec_type1(o64, v.astype(np.float64)).any() and len(CO.exec_type2(o64, w.astype(np.complex128))) == 0
        return
    e1, e2 = BC.rel(u32, u64), BC.rel(out32, out64)
    print(f"{name}: Float32 oracle against Float64 oracle, type 1 {e1:.2e}, type 2 {e2:.2e}")
    assert e1 < 1e-5 and e2 < 1e-5, (e1, e2)
    if CO.available():
        c1 = BC.rel(CO.exec_type1(o64, v.astype(np.float64)), u64)
        c2 = BC.rel(CO.exec_type2(o64, w.astype(np.complex128)), out64)
        assert c1 < 1e-11 and c2 < 1e-11, (c1, c2)


def test_the_families_and_their_sizes():
    Nover = (96, 80, 112)
    geom = {"bin_dims": [4, 4, 4]}
    for T in (np.float32, np.float64):
        s3 = BC.point_sets(T, Nover, geom, SEED)
        assert list(s3) == BC.ORDER
        assert [len(s3[n][0]) for n in BC.ORDER] == [600, 600, 512, 512, 512, 800, 800, 800, 800, 0, 1, 2, 63, 64, 65]
        for name, const in BC.CONFINED.items():
            for d in range(3):
                assert (len(np.unique(s3[name][d])) == 1) == (d in const), (name, d)
        for name in BC.COINCIDENT:
            assert all(len(np.unique(x)) == 1 for x in s3[name])
        assert all(x[0] == 0 for x in s3["coincident_origin"]) and all(x[0] == np.nextafter(T(O.TWO_PI), T(0)) for x in s3["coincident_last"])
        s2 = BC.point_sets(T, Nover[:2], {"bin_dims": [8, 8]}, SEED)
        assert [n for n in BC.ORDER if n not in s2] == ["layer_z", "column"] and all(len(x) == 2 for x in s2.values())
        s1 = BC.point_sets(T, Nover[:1], {"bin_dims": [32]}, SEED)
        assert [n for n in BC.ORDER if n not in s1] == list(BC.CONFINED) and all(len(x) == 1 for x in s1.values())
        # seeded: the same sets again, other sets for another seed
        again = BC.point_sets(T, Nover, geom, SEED)
        assert all(np.array_equal(a, b) for n in BC.ORDER for a, b in zip(s3[n], again[n]))
        assert not np.array_equal(BC.point_sets(T, Nover, geom, SEED + 1)["tiny_65"][0], s3["tiny_65"][0])
