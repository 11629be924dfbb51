"""CPU guard of the line-length matrix (tests/fft_lines_cases.py, run by tests/test_gpu_fft_lines.py): the matrix covers exactly the
lengths csrc/fft_lines.hip instantiates, every case's dims give the oversampled sizes it is meant to reach, and every length's
plan takes the halo variant at the shapes of the halo cases.  Adding a length to NUFFT_FFT_SIZES without tests fails here."""
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
