"""Off-resonance correction by time segmentation without a GPU: the numpy reference (field_reference.py) against itself --
the fit's normal equations, the error falling with the segment count, a constant field map, the folded dense operator against the
segmented model's own Gram matrix, the segmented data against the exact model's -- and the refusals of the C layer that a host-only
object can check.
"""
import ctypes as C

import numpy as np
import pytest

import field_cases as FC
import field_reference as F
import subspace_reference as S


@pytest.fixture(autouse=True, scope="module")
def _library_has_the_feature():
    """The reference is that of a feature of the library: without it there is nothing these tests describe."""
    from nufft_pkg import nufft
    assert hasattr(nufft, "FieldSegments") and "nufft_toeplitz_create_segmented" in nufft._lib.SYMBOLS


def test_fit_satisfies_its_normal_equations():
    omega, times = FC.quality_case()
    for L in (1, 3, 8):
        tau = F.uniform_tau(L, 0.0, 1.0)
        counts, centres = F.histogram(omega, FC.NBINS)
        G = F.gram(counts, centres, tau)
        assert np.allclose(G, G.conj().T, rtol=0, atol=1e-9 * abs(G[0, 0]))
        phi = F.interpolators(F.solver_matrix(G, FC.RIDGE), counts, centres, tau, times)
        r = F.rhs(counts, centres, tau, times)
        res = np.linalg.norm(F.ridged(G, FC.RIDGE) @ phi - r) / np.linalg.norm(r)
        print(f"normal equations L={L}: relative residual {res:.3e}")
        assert res <= 1e-10


def test_error_falls_with_the_segment_count():
    """(ωmax − ωmin)(t_max − t_min) = 6π: the printed values are the bars of the quality test on the GPU (test_gpu_field.py)."""
    omega, times = FC.quality_case()
    assert abs((omega.max() - omega.min()) * (times.max() - times.min()) - 6 * np.pi) <= 1e-12
    errs = [FC.quality_reference(L) for L in FC.QUALITY_SEGMENTS]
    for L, e in zip(FC.QUALITY_SEGMENTS, errs):
        print(f"interpolation error at the occupied bin centres over 200 times, L={L}: {e:.3e}")
    assert errs[0] > errs[1] > errs[2]


def test_constant_field_map():
    """One bin: Gm = h v vᴴ with v_l = exp(i ω τ_l), so φ(t) = v exp(−i ω t) / (L + ridge) and the error is ridge / (L + ridge) in exact
    arithmetic: the reference's own figure at this ridge, printed.  The ridged matrix has condition number (L + ridge) / ridge, so its
    float64 inverse adds up to about L · 2⁻⁵² times that: the bar is the sum of the two."""
    times = FC.quality_case()[1]
    omega = np.full((8, 8), 2.5)
    for L in (1, 4):
        tau = F.uniform_tau(L, 0.0, 1.0)
        counts, centres = F.histogram(omega, FC.NBINS)
        assert counts.tolist() == [64] and centres.tolist() == [2.5]
        phi = F.fit(omega, tau, times, FC.NBINS, FC.RIDGE)
        err = F.interpolation_error(phi, centres, tau, times)
        own = FC.RIDGE / (L + FC.RIDGE)
        rounding = L * 2.0 ** -52 * (L + FC.RIDGE) / FC.RIDGE
        print(f"constant field map L={L}: error {err:.3e} (the reference's own at ridge {FC.RIDGE:g}: {own:.3e}, rounding of the inverse {rounding:.1e})")
        assert err <= own + rounding


def test_folded_dense_operator_is_the_gram_matrix_of_the_segmented_model():
    Ns, L, Np = (12, 10), 3, 150
    rng = np.random.default_rng(0)
    xs = [rng.random(Np) * 2 * np.pi for _ in Ns]
    w = rng.random(Np) + 0.1
    phi = rng.standard_normal((L, Np)) + 1j * rng.standard_normal((L, Np))
    B = rng.standard_normal((L,) + Ns[::-1]) + 1j * rng.standard_normal((L,) + Ns[::-1])
    n = int(np.prod(Ns))
    A = F.segmented_matrix(F.fourier_matrix(Ns, xs), phi, B)
    want = A.conj().T @ (w[:, None] * A)
    blocks = S.dense_block_gram(Ns, S.exact_spectra(Ns, xs, w, phi), L)
    got = np.zeros((n, n), dtype=np.complex128)
    for a in range(L):
        for b in range(L):
            got += np.conj(B[a]).ravel()[:, None] * blocks[a * n:(a + 1) * n, b * n:(b + 1) * n] * B[b].ravel()[None, :]
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"folded dense operator against A_segᴴ W A_seg on {Ns}: {err:.3e}")
    assert err <= 1e-12
    # and the two routes of the reference itself
    u = rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1])
    direct = F.folded_gram(Ns, xs, w, phi, B, u)
    assert np.linalg.norm(direct.ravel() - want @ u.ravel()) <= 1e-12 * np.linalg.norm(direct)
    fast = F.folded_apply(Ns, S.multipliers(Ns, S.exact_spectra(Ns, xs, w, phi)), B, u)
    assert np.linalg.norm(fast - direct) <= 1e-12 * np.linalg.norm(direct)


def test_segmented_data_against_the_exact_model():
    """|y_seg − y_exact|_j = |Σ_k (Σ_l φ_l(t_j) exp(−i ω_k τ_l) − exp(−i ω_k t_j)) F_jk u_k| <= (interpolation error at the values of ω
    and the sample times) · ‖u‖₁."""
    Ns, Np = (12, 10), 150
    rng = np.random.default_rng(1)
    xs = [rng.random(Np) * 2 * np.pi for _ in Ns]
    times = np.sort(rng.random(Np))
    omega = FC.smooth_field(Ns[::-1], 6 * np.pi)
    u = rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1])
    Fm = F.fourier_matrix(Ns, xs)
    exact = F.exact_matrix(Fm, omega, times) @ u.ravel()
    last = np.inf
    for L in (2, 4, 8):
        tau = F.uniform_tau(L, 0.0, 1.0)
        phi = F.fit(omega, tau, times, FC.NBINS, FC.RIDGE)
        seg = F.segmented_matrix(Fm, phi, F.factors(omega, tau)) @ u.ravel()
        err = F.interpolation_error(phi, omega.ravel(), tau, times)
        diff = float(np.max(np.abs(seg - exact)))
        print(f"segmented against exact data L={L}: max difference {diff:.3e}, bound {err * np.abs(u).sum():.3e}")
        assert diff <= err * np.abs(u).sum() * (1 + 1e-12)
        assert diff < last
        last = diff


def test_recovery_inputs():
    """The inputs of the recovery test on the GPU: the reference alone halves the uncorrected error."""
    c = FC.recovery_case()
    print(f"recovery reference: corrected {c['err_ref']:.3e}, uncorrected {c['err_plain']:.3e}")
    assert c["err_ref"] < 0.5 * c["err_plain"]


def test_abi_and_host_refusals():
    from nufft_pkg import nufft
    lib, L_ = nufft.lib, nufft._lib
    raw = C.CDLL(nufft.LIB_PATH)
    for name in ("nufft_toeplitz_create_segmented", "nufft_toeplitz_num_segments", "nufft_toeplitz_set_factors", "nufft_toeplitz_clear_factors",
                 "nufft_fieldseg_create", "nufft_fieldseg_destroy", "nufft_fieldseg_layout", "nufft_fieldseg_get_info", "nufft_fieldseg_fit",
                 "nufft_fieldseg_interpolators", "nufft_fieldseg_factors", "nufft_fieldseg_get_histogram", "nufft_fieldseg_get_gram",
                 "nufft_fieldseg_get_solver_matrix", "nufft_fieldseg_get_tau", "nufft_sizeof_fieldseg_info"):
        assert name in L_.SYMBOLS and hasattr(raw, name), name
    assert lib.nufft_sizeof_fieldseg_info() == C.sizeof(L_.NufftFieldsegInfo)
    assert lib.nufft_version() == 104

    # the fit object: layout without a device
    info = L_.NufftFieldsegInfo()
    info.struct_size = C.sizeof(info)
    for L, tier in ((1, 1), (2, 2), (3, 4), (8, 8), (9, 16), (16, 16)):
        assert lib.nufft_fieldseg_layout(L_.F32, L, 256, C.byref(info)) == L_.OK
        assert (info.nsegments, info.segment_tier, info.nbins, info.device, info.threads) == (L, tier, 256, -1, 256)
        assert info.lds_bytes_interpolators == info.reseed_bins * tier * 16 + info.reseed_bins * 8 + tier * tier * 16 <= 64 << 10
    assert lib.nufft_fieldseg_layout(L_.F64, 4, 1024, C.byref(info)) == L_.OK and info.lds_bytes_histogram == 4096
    for args, code in (((7, 4, 256), L_.ERR_INVALID_ARG), ((L_.F32, 0, 256), L_.ERR_INVALID_ARG), ((L_.F32, 4, 0), L_.ERR_INVALID_ARG),
                       ((L_.F32, 4, 1025), L_.ERR_INVALID_ARG), ((L_.F64, 17, 256), L_.ERR_UNSUPPORTED)):
        assert lib.nufft_fieldseg_layout(*args, C.byref(info)) == code, args
    assert lib.nufft_fieldseg_layout(L_.F32, 4, 256, None) == L_.ERR_INVALID_ARG
    h = C.c_void_p()
    assert lib.nufft_fieldseg_create(C.byref(h), L_.F32, 4, 256, -1) == L_.ERR_NO_DEVICE and not h.value
    assert lib.nufft_fieldseg_create(C.byref(h), L_.F32, 17, 256, -1) == L_.ERR_UNSUPPORTED
    assert lib.nufft_fieldseg_fit(None, None, None, 1, None, 0.0, None) == L_.ERR_INVALID_ARG

    # the segmented operator on host-only plans
    plan = nufft.PlanNUFFT(np.complex64, (48, 40), backend=None)
    for bad, exc in ((0, "at least 1"), (-1, "at least 1"), (17, "at most 16")):
        with pytest.raises(ValueError, match=exc):
            nufft.ToeplitzOperator(plan, segments=bad)
    with pytest.raises(ValueError):
        nufft.ToeplitzOperator(plan, segments=2.0)
    with pytest.raises(ValueError, match="ntransforms = 1"):
        nufft.ToeplitzOperator(nufft.PlanNUFFT(np.complex64, (48, 40), ntransforms=2, backend=None), segments=2)
    with pytest.raises(ValueError, match="complex plan"):
        nufft.ToeplitzOperator(nufft.PlanNUFFT(np.float32, (48, 40), backend=None), segments=2)
    with pytest.raises(ValueError, match="NUFFT_TOEPLITZ_FUSED=0"):          # 16 lines of 2 N_1 = 1024 ComplexF64 cells
        nufft.ToeplitzOperator(nufft.PlanNUFFT(np.complex128, (512, 32), backend=None), segments=16)
    big = nufft.ToeplitzOperator(nufft.PlanNUFFT(np.complex128, (512, 32), backend=None, options={"NUFFT_TOEPLITZ_FUSED": 0}), segments=16)
    assert big.path == "dense" and big.segments == 16
    op = nufft.ToeplitzOperator(plan, segments=5)
    i = op.info()
    assert op.segments == 5 and op.ntransforms == 1 and i.ntransforms == 1 and i.has_spectrum == 0 and op.path == "fused"
    assert lib.nufft_toeplitz_num_segments(op._handle) == 5 and lib.nufft_toeplitz_num_coupled(op._handle) == 0
    assert lib.nufft_toeplitz_num_frames(op._handle) == 0 and not op.coupled and not op.framed
    plain = nufft.ToeplitzOperator(plan)
    assert plain.segments == 0 and lib.nufft_toeplitz_num_segments(plain._handle) == 0 and lib.nufft_toeplitz_num_segments(None) == 0
    assert plain.info().workspace_bytes == i.workspace_bytes                 # at rest a segmented object holds what a plain one holds
    ptr, tab = C.c_void_p(), (C.c_void_p * 5)()
    assert lib.nufft_toeplitz_set_spectrum(op._handle, ptr, None) == L_.ERR_UNSUPPORTED
    assert lib.nufft_toeplitz_set_points(op._handle, None, 0, tab, None, None) == L_.ERR_UNSUPPORTED
    assert lib.nufft_toeplitz_set_spectra_frames(op._handle, tab, None) == L_.ERR_UNSUPPORTED
    assert lib.nufft_toeplitz_set_points_frames(op._handle, None, None, tab, None, None) == L_.ERR_UNSUPPORTED
    assert lib.nufft_toeplitz_multiplier_ptr(op._handle, C.byref(ptr), None) == L_.ERR_UNSUPPORTED
    assert b"segmented" in lib.nufft_last_error_message()
    assert lib.nufft_toeplitz_set_factors(op._handle, tab, None) == L_.ERR_NO_DEVICE
    assert lib.nufft_toeplitz_set_factors(op._handle, None, None) == L_.ERR_INVALID_ARG
    assert lib.nufft_toeplitz_set_factors(plain._handle, tab, None) == L_.ERR_INVALID_ARG
    assert lib.nufft_toeplitz_set_factors(None, tab, None) == L_.ERR_INVALID_ARG
    assert lib.nufft_toeplitz_clear_factors(op._handle) == L_.OK and lib.nufft_toeplitz_clear_factors(None) == L_.ERR_INVALID_ARG
    assert lib.nufft_toeplitz_set_spectra_coupled(op._handle, tab, None) == L_.ERR_NO_DEVICE          # a build it would take on a device
    with pytest.raises(ValueError):
        op.set_factors(None)
    with pytest.raises(ValueError):
        plain.set_factors(None)
    assert "5 time segments" in repr(op)
    assert nufft.FieldSegments.uniform_tau(1, 0.0, 3.0).tolist() == [1.5]
    assert nufft.FieldSegments.uniform_tau(3, 0.0, 3.0).tolist() == [0.0, 1.5, 3.0]
