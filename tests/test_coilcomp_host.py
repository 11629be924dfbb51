"""Coil compression and noise pre-whitening without a GPU: the numpy reference (coilcomp_reference.py) against itself --
the kernel's Jacobi against ``np.linalg.eigh`` on every case --, exact properties of the compression matrix, the layout of the Gram
kernel over every coil count, and the C ABI (header, ctypes mirror, symbols, struct size, the refusals that need no device, in the
documented order, the checks of the noise covariance among them)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import coilcomp_cases as CC
import coilcomp_reference as CR
from llr_reference import jacobi_eigh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
ENTRY_POINTS = ("nufft_coilcomp_create", "nufft_coilcomp_destroy", "nufft_coilcomp_layout", "nufft_coilcomp_get_info",
                "nufft_coilcomp_whitening_matrix", "nufft_coilcomp_set_noise_covariance", "nufft_coilcomp_reset", "nufft_coilcomp_accumulate",
                "nufft_coilcomp_finish", "nufft_coilcomp_set_matrix", "nufft_coilcomp_apply", "nufft_coilcomp_get_gram",
                "nufft_coilcomp_get_matrix", "nufft_coilcomp_get_spectrum", "nufft_sizeof_coilcomp_info")


@pytest.fixture(scope="module")
def nufft():
    from nufft_pkg import nufft
    return nufft


@pytest.mark.parametrize("C_,n,noise", [c + (False,) for c in CC.CASES] + [c + (True,) for c in CC.NOISE_CASES])
def test_reference_against_itself(C_, n, noise):
    """compression_matrix(eigh=jacobi_eigh) against compression_matrix(eigh=np.linalg.eigh) on the reference's own Gram matrix: the
    rows compared up to a phase, the eigenvalues over λ_max, and A Aᴴ − I (A Ψ Aᴴ − I whitened).  The separation that makes the rows
    comparable is asserted here; the printed figures are what coilcomp_cases.SELF_EPS / SELF_ORTHO record and the GPU bars rest on.
    Measured: at most 65.9 ε on the rows and 62.0 ε λ_max on the eigenvalues (C = 64), 8.0 ε on A Aᴴ − I, at most 12 sweeps."""
    A, lam, R, _ = CC.reference(C_, n, "c128", noise)
    Aj, lamj, _, info = CC.reference(C_, n, "c128", noise, jacobi=True)
    rows = CC.rows_compared(C_, n)
    rd = float(CR.row_difference(Aj[:rows], A[:rows]).max()) / EPS
    ed = float(np.abs(lamj - lam).max() / lam[0]) / EPS
    psi = CC.psi(C_) if noise else np.eye(C_)
    if noise:                                                        # the other order of the two products, under LAPACK
        W = CR.whitening_matrix(psi)
        l2, U2 = CR.fix_vectors(*np.linalg.eigh(CR.whiten(R, W, left_first=False)))
        rd = max(rd, float(CR.row_difference((U2.conj().T @ W)[:rows], A[:rows]).max()) / EPS)
        ed = max(ed, float(np.abs(l2 - lam).max() / lam[0]) / EPS)
    ortho = float(np.abs(Aj @ psi @ Aj.conj().T - np.eye(C_)).max()) / EPS
    sep = CC.separation(lam, rows, min(C_, n))
    print(f"C={C_} n={n} noise={noise}: {rows} rows {rd:.1f} ε, eigenvalues {ed:.1f} ε λ_max, orthogonality {ortho:.1f} ε, "
          f"{info['sweeps']} sweeps, smallest ratio {sep:.3f}")
    assert sep >= CC.MIN_RATIO
    assert rd <= CC.SELF_EPS[(C_, n, noise)][0] and ed <= CC.SELF_EPS[(C_, n, noise)][1] and ortho <= CC.SELF_ORTHO[(C_, n, noise)]
    assert rd <= 512 and ed <= 512 and ortho <= 64
    assert (C_ == 1 and info["sweeps"] == 0) or 2 <= info["sweeps"] < 24
    # the designed spectrum, where the data have full rank
    if n >= C_:
        assert np.abs(lam / lam[0] - CC.RHO[(C_, n)] ** np.arange(C_)).max() <= 1e-12


def test_exact_properties():
    C_, n = 8, 210
    y = CC.data(C_, n)
    h = CC.weights(n)
    for eigh in (np.linalg.eigh, jacobi_eigh):
        R = CR.gram(y, h)
        A, lam = CR.compression_matrix(R, eigh=eigh)
        # A Aᴴ = I; the rows are unit vectors whose largest entry is real and positive; λ descending
        assert np.abs(A @ A.conj().T - np.eye(C_)).max() <= 16 * EPS
        k = np.argmax(np.abs(A), axis=1)
        big = A[np.arange(C_), k]
        assert np.abs(big.imag).max() == 0.0 and big.real.min() > 0 and (np.diff(lam) <= 0).all()
        # a positive scale of the data leaves A alone
        A2, lam2 = CR.compression_matrix(CR.gram(3.7 * y, h), eigh=eigh)
        assert CR.row_difference(A2[:4], A[:4]).max() <= 64 * EPS and np.abs(lam2 / 3.7 ** 2 - lam).max() <= 64 * EPS * lam[0]
        # permuting the coils permutes the columns of A
        perm = np.random.default_rng(1).permutation(C_)
        A3, _ = CR.compression_matrix(CR.gram(y[perm], h), eigh=eigh)
        assert CR.row_difference(A3[:4], A[:4][:, perm]).max() <= 64 * EPS
        # the retained energy is the weighted energy of the compressed data
        for V in (1, 3, C_):
            out = CR.apply(A, y, V)
            assert abs((h[None, :] * np.abs(out) ** 2).sum() - lam[:V].sum()) <= 64 * EPS * lam.sum()
        # whitened: A Ψ Aᴴ = I, and A = Uᴴ W with U unitary
        psi = CC.psi(C_)
        Aw, lamw = CR.compression_matrix(R, psi, eigh=eigh)
        err = np.abs(Aw @ psi @ Aw.conj().T - np.eye(C_)).max() / EPS
        print(f"{eigh.__name__}: A Ψ Aᴴ − I {err:.1f} ε")
        assert err <= 64
        U = Aw @ np.linalg.cholesky(psi)
        assert np.abs(U @ U.conj().T - np.eye(C_)).max() <= 64 * EPS
    # a zero Gram matrix: A = W (= I unwhitened), λ = 0, for both solvers
    for eigh in (np.linalg.eigh, jacobi_eigh):
        A, lam = CR.compression_matrix(np.zeros((3, 3)), eigh=eigh)
        assert np.array_equal(A, np.eye(3)) and not lam.any()
    # one coil: A is a phase of modulus 1 (here 1)
    A, lam = CR.compression_matrix(CR.gram(CC.data(1, 9)), eigh=jacobi_eigh)
    assert A.shape == (1, 1) and A[0, 0] == 1.0 and abs(lam[0] - 1.0) <= 8 * EPS


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
    assert nufft.lib.nufft_sizeof_coilcomp_info() == C.sizeof(L.NufftCoilcompInfo) == 112
    fields = re.search(r"typedef struct nufft_coilcomp_info \{(.*?)\}", header, flags=re.S).group(1)
    names = [re.sub(r"\[\d+\]", "", n.strip()) for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0].rstrip("_") for f in L.NufftCoilcompInfo._fields_]
    assert nufft.lib.nufft_version() == 104
    for name, value in (("NUFFT_COILCOMP_OK", L.COILCOMP_OK), ("NUFFT_COILCOMP_SWEEPS", L.COILCOMP_SWEEPS), ("NUFFT_COILCOMP_NONFINITE", L.COILCOMP_NONFINITE)):
        assert int(re.search(r"#define " + name + r" (\d+)", header).group(1)) == value
    for name in ("CoilCompressor", "compress_coils"):
        assert name in nufft.__all__ and hasattr(nufft, name)


def test_every_layout_fits(nufft):
    """nufft_coilcomp_layout is the function the Gram kernel launches with.  Over both element types, every C from 1 to 64 and n from 1 to
    1e7: the workgroup is whole waves, the tiles cover n and the workgroups cover the tiles within the partial sets the object holds,
    every entry of the upper triangle has an owner with at most 9 per thread, and LDS holds what DESIGN.md §29 lists -- the tile with
    its padding, the weights, the segment partials, the entry table; H, V, λ and the order of the eigen kernel -- within the 160 KiB of
    a compute unit."""
    L, lib = nufft._lib, nufft.lib
    info = L.NufftCoilcompInfo()
    lengths = (1, 2, 9, 31, 32, 33, 210, 1000, 1023, 1024, 1025, 16384, 40000, 524287, 524288, 524289, 10 ** 6, 10 ** 7)
    seen, multi = 0, 0
    for dtype, eb in ((L.F32, 8), (L.F64, 16)):
        for ncoils in range(1, 65):
            for n in lengths:
                info.struct_size = C.sizeof(info)
                assert lib.nufft_coilcomp_layout(dtype, ncoils, n, C.byref(info)) == L.OK
                np_ = ncoils * (ncoils + 1) // 2
                TC, S = info.tile_samples, info.segments
                assert info.threads % 64 == 0 and info.threads == 256 and (info.ncoils, info.dtype, info.device, info.n) == (ncoils, dtype, -1, n)
                assert 32 <= TC <= 1024 and TC & (TC - 1) == 0 and S >= 1 and TC % S == 0
                assert info.tiles * TC >= n > (info.tiles - 1) * TC
                assert info.workgroups * info.tiles_per_workgroup >= info.tiles > (info.workgroups - 1) * info.tiles_per_workgroup
                assert 1 <= info.workgroups <= info.max_workgroups == 512
                assert info.pairs == np_ and info.pairs_per_thread * info.threads >= np_ and info.pairs_per_thread <= 9
                need = ncoils * (TC + 1) * eb + TC * 8 + S * np_ * 16 + np_ * 2
                assert need <= info.lds_bytes_gram <= 160 << 10, (dtype, ncoils, n, need, info.lds_bytes_gram)
                assert ncoils * ncoils * 32 + ncoils * 12 <= info.lds_bytes_eigen <= 160 << 10
                assert ncoils <= info.jacobi_team_lanes <= 64 and info.jacobi_team_lanes < 2 * ncoils and info.jacobi_sweeps_max == 24
                assert info.apply_chunk == 16 and info.matrix_rows == 0 and info.has_noise == 0
                assert info.workspace_bytes >= info.max_workgroups * np_ * 16 + (5 * ncoils + 16) * ncoils * 16
                seen += 1
                multi += info.tiles_per_workgroup > 1
    print(f"{seen} layouts, {multi} with more than one tile per workgroup")
    assert seen == 2 * 64 * len(lengths) and 0 < multi < seen


def _cd(m):
    return np.ascontiguousarray(m, dtype=np.complex128).ctypes.data_as(C.POINTER(C.c_double))


def test_refusals_without_a_device(nufft):
    """Null arguments and the arguments (INVALID_ARG), then the limit (UNSUPPORTED), and the missing device last; the checks of a noise
    covariance: not finite, not Hermitian, not positive definite, in this order."""
    L, lib = nufft._lib, nufft.lib
    h = C.c_void_p()
    assert lib.nufft_coilcomp_create(None, L.F64, 3, -1) == L.ERR_INVALID_ARG
    for coils in (3, 65):
        assert lib.nufft_coilcomp_create(C.byref(h), 7, coils, -1) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_create(C.byref(h), L.F64, 0, -1) == L.ERR_INVALID_ARG and lib.nufft_coilcomp_create(C.byref(h), L.F32, -1, -1) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_create(C.byref(h), L.F64, 65, -1) == L.ERR_UNSUPPORTED and b"65 coils" in lib.nufft_last_error_message()
    for coils in (1, 33, 64):
        assert lib.nufft_coilcomp_create(C.byref(h), L.F32, coils, -1) == L.ERR_NO_DEVICE and not h.value
    info = L.NufftCoilcompInfo()
    assert lib.nufft_coilcomp_layout(L.F64, 3, 9, None) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_layout(7, 65, 0, C.byref(info)) == L.ERR_INVALID_ARG and lib.nufft_coilcomp_layout(L.F64, 0, 0, C.byref(info)) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_layout(L.F64, 65, 0, C.byref(info)) == L.ERR_INVALID_ARG          # n before the limit
    assert lib.nufft_coilcomp_layout(L.F64, 65, 9, C.byref(info)) == L.ERR_UNSUPPORTED
    assert lib.nufft_coilcomp_layout(L.F64, 64, 9, C.byref(info)) == L.OK and info.struct_size == C.sizeof(info)
    # the noise covariance
    psi = CC.psi(8)
    W = np.empty((8, 8), dtype=np.complex128)
    assert lib.nufft_coilcomp_whitening_matrix(8, None, _cd(W)) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_whitening_matrix(8, _cd(psi), None) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_whitening_matrix(0, _cd(psi), _cd(W)) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_whitening_matrix(65, _cd(psi), _cd(W)) == L.ERR_UNSUPPORTED
    bad = psi.copy()
    bad[2, 5] = np.nan                                              # neither Hermitian nor finite: reported as not finite
    assert lib.nufft_coilcomp_whitening_matrix(8, _cd(bad), _cd(W)) == L.ERR_INVALID_ARG and b"not finite" in lib.nufft_last_error_message()
    bad = psi.copy()
    bad[2, 5] += 1e-10 * np.abs(psi).max()
    bad[0, 0] = -1.0                                                # neither positive definite nor Hermitian: reported as not Hermitian
    assert lib.nufft_coilcomp_whitening_matrix(8, _cd(bad), _cd(W)) == L.ERR_INVALID_ARG and b"not Hermitian" in lib.nufft_last_error_message()
    bad = psi.copy()
    bad[2, 5] += 1e-14 * np.abs(psi).max()                          # Hermitian to 1e-12 ‖Ψ‖: accepted
    assert lib.nufft_coilcomp_whitening_matrix(8, _cd(bad), _cd(W)) == L.OK
    bad = psi - 1.5 * np.linalg.eigvalsh(psi)[0] * np.eye(8)        # the smallest eigenvalue made negative
    assert lib.nufft_coilcomp_whitening_matrix(8, _cd(bad), _cd(W)) == L.ERR_INVALID_ARG and b"not positive definite" in lib.nufft_last_error_message()
    assert lib.nufft_coilcomp_whitening_matrix(8, _cd(np.zeros((8, 8))), _cd(W)) == L.ERR_INVALID_ARG
    for C_ in (1, 8, 33, 64):                                        # and the factor itself against numpy
        psi = CC.psi(C_)
        W = np.empty((C_, C_), dtype=np.complex128)
        assert lib.nufft_coilcomp_whitening_matrix(C_, _cd(psi), _cd(W)) == L.OK
        want = CR.whitening_matrix(psi)
        err = np.abs(W - want).max() / np.abs(want).max() / EPS
        white = np.abs(W @ psi @ W.conj().T - np.eye(C_)).max() / EPS
        print(f"C={C_}: W against numpy {err:.1f} ε, W Ψ Wᴴ − I {white:.1f} ε")
        assert err <= 64 * CC.PSI_COND and white <= 64 and not np.triu(W, 1).any()
    # the other entry points
    assert lib.nufft_coilcomp_get_info(None, 1, None) == L.ERR_INVALID_ARG and lib.nufft_coilcomp_reset(None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_accumulate(None, None, None, 1, None) == L.ERR_INVALID_ARG and lib.nufft_coilcomp_finish(None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_apply(None, None, 1, None, 1, None) == L.ERR_INVALID_ARG and lib.nufft_coilcomp_set_matrix(None, None, 1, None) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_set_noise_covariance(None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_get_gram(None, None, None) == L.ERR_INVALID_ARG and lib.nufft_coilcomp_get_matrix(None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_get_spectrum(None, None, None, None, None) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_destroy(None) == L.OK
    # the Python layer refuses the same way; a real-data plan is refused there (the C call has no plan to look at)
    torch = pytest.importorskip("torch")
    plan = nufft.PlanNUFFT(np.complex128, (12, 10), backend=None)
    real = nufft.PlanNUFFT(np.float64, (12, 10), backend=None)
    op = nufft.ToeplitzOperator(plan)
    for bad in (lambda: nufft.CoilCompressor(plan, 3), lambda: nufft.CoilCompressor(op, 3), lambda: nufft.CoilCompressor(plan, 0),
                lambda: nufft.CoilCompressor(plan, 65), lambda: nufft.CoilCompressor(real, 3), lambda: nufft.CoilCompressor(None, 3),
                lambda: nufft.CoilCompressor(plan, True), lambda: nufft.CoilCompressor(plan, 3, device="cuda"),
                lambda: nufft.CoilCompressor(torch.float32, 3, device="cuda:0"), lambda: nufft.CoilCompressor(torch.complex64, 3, device="cpu"),
                lambda: nufft.compress_coils((), 1)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="complex plan"):
        nufft.CoilCompressor(real, 3)
    for o in (op, plan, real):
        o.close()
