"""CPU side of tests/test_gpu_many_transforms.py: every case of tests/many_transforms_cases.py is eligible, by construction, for the
engine its name says (host-only plans, device = -1: the decisions of the plan that need no device), and the list covers what it
claims to cover.  A list whose cases would silently land on another engine fails here, on a machine without a GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import many_transforms_cases as MT  # noqa: E402


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


def _clear_switches(nufft, monkeypatch):
    harness = nufft.plan._HARNESS_ENV
    for var in list(os.environ):
        if var.startswith("NUFFT_") and var not in harness:
            monkeypatch.delenv(var)


@pytest.mark.parametrize("case", MT.CASES, ids=MT.IDS)
def test_every_case_is_eligible_for_the_engine_it_names(nufft, case, monkeypatch):
    name, Z, dims, M, sigma, evalmode, C, Np, spread_method, options, expected = case
    _clear_switches(nufft, monkeypatch)
    for k, v in options.items():
        monkeypatch.setenv(k, v)
    mode = nufft.Direct() if evalmode == MT.DIRECT else nufft.FastApproximation()
    plan = nufft.PlanNUFFT(Z, dims, m=M, sigma=sigma, ntransforms=C, kernel_evalmode=mode, spread_method=spread_method, backend=None)
    info = plan.info()
    assert info.ntransforms == C > 8
    for k in MT.INFO_KEYS:
        if k in expected:
            assert getattr(info, k) == expected[k], (name, k, getattr(info, k))
    assert not set(expected) - set(MT.INFO_KEYS) - {"spread_engine_used", "interp_engine_used"}
    if spread_method != "auto":
        assert "spread_method" in expected           # a forced engine is always asserted
    if expected.get("spread_method") == MT.MARCHING_RING:
        assert info.ring_column[0] > 0 and "ring_halo" in expected
    if expected.get("interp_engine_used") == "marching_ring":
        # the interpolation ring exists for this plan: bins of 4 cells on a 3-D grid (the device-side flag is read on the GPU)
        assert len(dims) == 3 and list(info.bin_dims) == [4, 4, 4]


def test_the_list_covers_what_it_claims():
    Cs = {c[6] for c in MT.CASES}
    assert Cs == {9, 16, 17}
    assert {np.dtype(c[1]).name for c in MT.CASES} == {"float32", "float64", "complex64", "complex128"}
    forced = {c[8] for c in MT.CASES}
    assert forced >= MT.ENGINE_NAMES
    assert {c[10].get("spread_engine_used") for c in MT.CASES} >= MT.ENGINE_NAMES | {"marching_ring_dense"}
    assert {c[10].get("interp_engine_used") for c in MT.CASES} >= {"lds_tiles", "marching_ring"}
    assert {len(c[2]) for c in MT.CASES} == {1, 2, 3}
    assert {c[5] for c in MT.CASES} == {MT.DIRECT, MT.FAST}
    assert len(set(MT.IDS)) == len(MT.IDS)
    # clipped and halo variants of the spreading ring, the halo variant with both consumers of its side buffer
    assert {c[10].get("ring_halo") for c in MT.CASES} >= {0, 1}
    assert {c[9].get("NUFFT_SMARCH_HALO_FUSE") for c in MT.CASES} >= {"0", "1"}
    # Np stays within what the numpy oracle does in seconds, except for the dense cases (20 points per bin, the C oracle)
    for c in MT.CASES:
        assert 3000 <= c[7] <= 5000 or c[0].startswith("dense-"), c[0]


def test_inputs_are_per_component_and_reproducible():
    c = MT.case("tiles-general-fft-c128")
    vs, again = MT.values(c), MT.values(c)
    assert len(vs) == 17 and all(np.array_equal(a, b) for a, b in zip(vs, again))
    MT.assert_distinguishable(vs)
    ws = MT.spectra(c, (30, 20, 24))
    MT.assert_distinguishable(ws)
    assert ws[0].dtype == np.complex128 and vs[0].dtype == np.complex128
    xs = MT.points(MT.case("ring-clipped-f32"))
    assert xs[0].dtype == np.float32 and min(x.min() for x in xs) < 0 and max(x.max() for x in xs) > MT.TWO_PI
    with pytest.raises(AssertionError):
        MT.assert_distinguishable([vs[0], vs[1], vs[0]])
