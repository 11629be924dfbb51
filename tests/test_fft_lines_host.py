"""CPU guard of the line-length matrix (tests/fft_lines_cases.py, run by tests/test_gpu_fft_lines.py): the matrix covers exactly the
lengths csrc/fft_lines.hip instantiates, every case's dims give the oversampled sizes it is meant to reach, and every length's
plan takes the halo variant at the shapes of the halo cases.  Adding a length to NUFFT_FFT_SIZES without tests fails here.
The tables of the coupled dimension-1 kernel and of the coil-map passes: every launchable (element type, length, tier) once, the
refused set, K against tier, the waves-per-workgroup and prefetch rules against a literal table, and the dims on host-only plans."""
import os
import re

import numpy as np
import pytest

import fft_lines_cases as FC
from oracle import nufft_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FFT_LINES = os.path.join(ROOT, "nonuniformffts.jl_amd", "csrc", "fft_lines.hip")
HEADER = os.path.join(ROOT, "include", "nufft_mi355x.h")


def _macro_sizes():
    text = open(FFT_LINES).read()
    m = re.findall(r"^#define\s+NUFFT_FFT_SIZES\(X\)\s+(.*)$", text, flags=re.M)
    assert len(m) == 1, "expected one definition of NUFFT_FFT_SIZES"
    body = m[0].strip()
    sizes = [int(s) for s in re.findall(r"X\((\d+)\)", body)]
    assert re.sub(r"X\(\d+\)", "", body).strip() == "", body        # nothing but X(n) items
    return sizes


def test_matrix_covers_exactly_the_instantiated_lengths():
    assert _macro_sizes() == list(FC.SIZES)
    for cases, kinds in ((FC.plan_cases(), set(FC.GROUPS)), (FC.mult_cases(), {"mult"}),
                         (FC.toeplitz_cases(), {"lines", "strided_2d", "strided_3d_dim2", "strided_3d_dim3"})):
        assert {c.kind for c in cases} == kinds
        types = {c.Z if isinstance(c.Z, str) else np.dtype(c.Z).name for c in cases}
        for kind in kinds:
            sub = [c for c in cases if c.kind == kind]
            for Z in {c.Z for c in sub}:
                assert sorted({c.n for c in sub if c.Z == Z}) == list(FC.SIZES), (kind, Z)
        # both precisions everywhere
        assert types in ({"float32", "float64", "complex64", "complex128"}, {"float32", "float64"}, {"c64", "c128"})


def test_size_rule_at_sigma_2():
    """What the dims of the tables rely on, for every length."""
    for n in FC.SIZES:
        assert n % 2 == 0 and (n // 2 - 1) % 2 == 1
        assert O.oversampled_size(n // 2, 2.0, False) == n and O.oversampled_size(n // 2 - 1, 2.0, False) == n
        assert O.oversampled_size(n, 2.0, True) == 2 * n and O.oversampled_size(n - 1, 2.0, True) == 2 * n


def _oversampled(Z, dims):
    is_real = not isinstance(Z, str) and np.dtype(Z).kind == "f"
    return tuple(O.oversampled_size(N, FC.SIGMA, is_real and d == 0) for d, N in enumerate(dims))


@pytest.mark.parametrize("cases", [FC.plan_cases(), FC.mult_cases()], ids=["plan", "mult"])
def test_plan_cases_reach_their_oversampled_sizes(cases):
    where = {"strided_2d": 1, "mult": 1, "strided_3d_dim2": 1, "strided_3d_dim3": 2, "real_dim1": 0, "cplx_dim1": 0, "cplx_strided": 1}
    for c in cases:
        assert _oversampled(c.Z, c.dims) == tuple(c.over), c
        assert c.over[where[c.kind]] == (2 * c.n if c.kind == "real_dim1" else c.n), c
        # every other axis of the own passes is an instantiated length too (the plan takes them), dimension 1 of the strided real
        # cases is not (80 = 2 x 40: rocFFT there)
        is_real = np.dtype(c.Z).kind == "f"
        for d, no in enumerate(c.over):
            if is_real and d == 0:
                assert (no // 2 in FC.SIZES) == (c.kind == "real_dim1"), c
            else:
                assert no in FC.SIZES, c
    # per kind: the odd kept count, fftshift and ntransforms = 2 all occur; ntransforms = 2 on every third length
    for kind in {c.kind for c in cases}:
        for Z in {c.Z for c in cases if c.kind == kind}:
            sub = [c for c in cases if c.kind == kind and c.Z == Z]
            axis = where[kind]
            if kind != "cplx_strided":                              # (that kind: the even kept count only)
                assert {c.dims[axis] % 2 for c in sub} == {0, 1}, kind
            if kind in ("strided_3d_dim2", "strided_3d_dim3", "cplx_strided"):
                assert {c.fftshift for c in sub} == {False, True}, kind
            if kind != "mult":
                twos = sorted({FC.SIZES.index(c.n) for c in sub if c.C == 2})
                assert len(twos) >= 4 and all(b - a == 3 for a, b in zip(twos, twos[1:])), (kind, twos)


def test_toeplitz_cases_reach_their_embedding_sizes():
    cases = FC.toeplitz_cases()
    where = {"lines": 0, "strided_2d": 1, "strided_3d_dim2": 1, "strided_3d_dim3": 2}
    for c in cases:
        assert 2 * c.dims[where[c.kind]] == c.n
        assert all(2 * N in FC.SIZES for N in c.dims), c           # fused path: every 2 N_d in the table
    for kind in where:
        assert {c.fftshift for c in cases if c.kind == kind} == {False, True}
    # consecutive pairs share a shape (and with it the exact reference)
    for a, b in zip(cases[0::2], cases[1::2]):
        assert (a.dims, a.fftshift, a.Z, b.Z) == (b.dims, b.fftshift, "c128", "c64")


def test_header_lists_the_fused_toeplitz_sizes():
    """include/nufft_mi355x.h describes the fused Toeplitz path by the N_d whose 2 N_d are line lengths: the same table."""
    text = open(HEADER).read()
    m = re.search(r"fused\s+—.*?N_d\s*∈\s*\{([^}]*)\}", text, flags=re.S)
    assert m, "the description of the fused Toeplitz path names its sizes"
    listed = [int(s) for s in re.findall(r"\d+", m.group(1))]
    assert [2 * n for n in listed] == list(FC.SIZES)


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft as mod
    return mod


# coupled_waves of csrc/toeplitz_coupled.hip over the thirteen lengths, evaluated from the C++ rule on the CPU: the literal table pins
# the Python restatement (fft_lines_cases.coupled_waves) against silent drift
TL_ROWS = {
    ("c128", 2): (16, 16, 16, 16, 8, 8, 8, 4, 4, 4, 4, 4, 4),
    ("c128", 4): (16, 8, 8, 8, 4, 4, 4, 4, 4, 4, 2, 2, 2),
    ("c128", 8): (8, 4, 4, 4, 4, 4, 4, 2, 2, 2, 1, 1, 1),
    ("c128", 16): (4, 4, 4, 4, 2, 2, 2, 1, 1, 1, 0, 0, 0),
    ("c64", 2): (16, 16, 16, 16, 16, 16, 16, 8, 8, 8, 4, 4, 4),
    ("c64", 4): (16, 16, 16, 16, 8, 8, 8, 4, 4, 4, 4, 4, 4),
    ("c64", 8): (16, 8, 8, 8, 4, 4, 4, 4, 4, 4, 2, 2, 2),
    ("c64", 16): (8, 4, 4, 4, 4, 4, 4, 2, 2, 2, 1, 1, 1),
}


def test_coupled_rules_match_the_quoted_rows():
    for (Z, kt), row in TL_ROWS.items():
        assert tuple(FC.coupled_waves(FC.CSIZE[Z], n, kt) for n in FC.SIZES) == row, (Z, kt)
    assert [FC.coupled_tier(K) for K in range(1, 17)] == [2, 2, 4, 4, 8, 8, 8, 8] + [16] * 8
    assert all(FC.coupled_tier(K) == tier for tier, ks in FC.TIER_KS.items() for K in ks)
    # PREFETCH: tiers 2 and 4 from 128 cells (ComplexF64: 2 cells per 16-byte load) / 256 cells (ComplexF32: 4) on
    for Z, first in (("c128", 128), ("c64", 256)):
        for kt in FC.TIERS:
            assert [FC.coupled_prefetch(FC.CSIZE[Z], n, kt) for n in FC.SIZES] == [kt <= 4 and n >= first for n in FC.SIZES], (Z, kt)


def test_coupled_cases_cover_every_launchable_instantiation():
    cases = FC.coupled_cases()
    flat, deep = [c for c in cases if len(c.dims) == 2], [c for c in cases if len(c.dims) == 3]
    assert {c.kind for c in cases} == {"coupled_lines"} and len(flat) == 101 and len(deep) == 4
    assert len({FC.case_id(c) for c in cases}) == len(cases)
    # completeness: every (type, length, tier) that fits exactly once, none that does not
    want = sorted((Z, n, kt) for Z in FC.CSIZE for n in FC.SIZES for kt in FC.TIERS if FC.coupled_waves(FC.CSIZE[Z], n, kt) > 0)
    assert sorted((c.Z, c.n, FC.coupled_tier(c.K)) for c in flat) == want
    # the refused set: ComplexF64, tier 16, from 640 cells on, and nothing else
    unfit = {(Z, n, kt) for Z in FC.CSIZE for n in FC.SIZES for kt in FC.TIERS if FC.coupled_waves(FC.CSIZE[Z], n, kt) == 0}
    assert unfit == {("c128", n, 16) for n in (640, 768, 1024)}
    refused = FC.coupled_refused()
    assert {(Z, n, FC.coupled_tier(K)) for Z, n, K in refused} == unfit
    assert sorted(refused) == sorted([("c128", n, 9) for n in (640, 768, 1024)] + [("c128", 640, 16)])
    for c in cases:
        assert c.n == 2 * c.dims[0] and c.n in FC.SIZES and all(2 * N in FC.SIZES for N in c.dims), c
        assert c.dims[0] % 2 == 0                                   # the even kept count (see the module docstring)
        assert int(np.prod([2 * N for N in c.dims[1:]])) == (64 if len(c.dims) == 2 else 4096)
        assert 2 <= c.K <= 16 and FC.coupled_waves(FC.CSIZE[c.Z], c.n, FC.coupled_tier(c.K)) > 0, c
    i_of = {n: i for i, n in enumerate(FC.SIZES)}
    for Z in FC.CSIZE:
        sub = [c for c in flat if c.Z == Z]
        # K and tier: the rule of the table, and every tier meets its smallest and its largest K
        for c in sub:
            ks = FC.TIER_KS[FC.coupled_tier(c.K)]
            assert c.K == ks[i_of[c.n] % len(ks)], c
        for tier, ks in FC.TIER_KS.items():
            assert {min(ks), max(ks)} <= {c.K for c in sub if FC.coupled_tier(c.K) == tier}, (Z, tier)
        assert {c.fftshift for c in sub} == {False, True}
        # the rules: every waves-per-workgroup value; prefetch on and off in tiers 2 and 4, off throughout tiers 8 and 16
        assert {FC.coupled_waves(FC.CSIZE[Z], c.n, FC.coupled_tier(c.K)) for c in sub} == {16, 8, 4, 2, 1}, Z
        for tier in FC.TIERS:
            pre = {FC.coupled_prefetch(FC.CSIZE[Z], c.n, tier) for c in sub if FC.coupled_tier(c.K) == tier}
            assert pre == ({False, True} if tier <= 4 else {False}), (Z, tier)
    # fftshift: opposite for the two types of a (length, tier)
    by = {(c.Z, c.n, FC.coupled_tier(c.K)): c.fftshift for c in flat}
    for (Z, n, kt), shift in by.items():
        if Z == "c128" and ("c64", n, kt) in by:
            assert by[("c64", n, kt)] != shift
    # the 3-D shapes: prefetch on for the first two, K = 7 and K = 9 (pair offsets of the tiers 8 and 16) for the others
    assert [(c.Z, c.dims, c.K) for c in deep] == [("c128", (64, 32, 32), 3), ("c64", (128, 32, 32), 2), ("c64", (32, 32, 32), 7),
                                                 ("c128", (40, 32, 32), 9)]
    assert [FC.coupled_prefetch(FC.CSIZE[c.Z], c.n, FC.coupled_tier(c.K)) for c in deep] == [True, True, False, False]


def test_maps_cases_reach_every_length():
    cases = FC.maps_cases()
    assert {c.kind for c in cases} == {"maps_2d", "maps_3d"} and len(cases) == 4 * len(FC.SIZES)
    for kind in ("maps_2d", "maps_3d"):
        for Z in ("c128", "c64"):
            assert [c.n for c in cases if c.kind == kind and c.Z == Z] == list(FC.SIZES), (kind, Z)
        assert {c.fftshift for c in cases if c.kind == kind} == {False, True}
    for c in cases:
        assert 2 * c.dims[-1] == c.n and all(2 * N in FC.SIZES for N in c.dims), c      # the outermost pass carries the map
        assert c.dims[:-1] == ((40,) if c.kind == "maps_2d" else (32, 32)), c
    for a, b in zip(cases[0::2], cases[1::2]):
        assert (a.dims, a.fftshift, a.Z, b.Z) == (b.dims, b.fftshift, "c128", "c64")
    two, three = [c for c in cases if c.kind == "maps_2d"], [c for c in cases if c.kind == "maps_3d"]
    assert any(a.fftshift != b.fftshift for a, b in zip(two, three))                    # the two kinds alternate differently


def test_coupled_and_maps_dims_take_the_fused_path(nufft):
    """Host-only plans of every case's dims (and of the refused triples): the operator reports twice the dims as its padded shape and
    the fused path."""
    seen = set()
    shapes = [(c.Z, c.dims, c.K) for c in FC.coupled_cases()] + [(c.Z, c.dims, 1) for c in FC.maps_cases()]
    shapes += [(Z, (n // 2, 32), K) for Z, n, K in FC.coupled_refused()]
    for Z, dims, K in shapes:
        if (Z, dims, K) in seen:
            continue
        seen.add((Z, dims, K))
        plan = nufft.PlanNUFFT(np.complex128 if Z == "c128" else np.complex64, dims, ntransforms=K, backend=None)
        op = nufft.ToeplitzOperator(plan)
        assert op.padded_shape == tuple(2 * N for N in reversed(dims)) and op.path == "fused", (Z, dims, K)
        op.close()
        plan.close()


def test_every_length_takes_the_halo_variant(nufft, monkeypatch):
    """Host-only plans (no device) take the same decision as plan.info() on the GPU: the halo variant at the shapes of the halo cases,
    for every length and element type — the halo list leaves none out."""
    monkeypatch.setenv("NUFFT_SMARCH_HALO", "2")
    assert tuple(FC.HALO_LENGTHS) == tuple(FC.SIZES) and len(FC.halo_cases()) == len(FC.HALO_TYPES) * len(FC.SIZES)
    for c in FC.halo_cases():
        assert _oversampled(c.Z, c.dims) == c.over, c
        i = nufft.PlanNUFFT(c.Z, c.dims, m=FC.HALF_SUPPORT, sigma=FC.SIGMA, kernel_evalmode=nufft.Direct(), spread_method="marching_ring",
                            backend=None).info()
        assert i.spread_method == 3 and i.ring_halo == 1, c
