"""Coil compression and noise pre-whitening on the GPU against numpy (coilcomp_reference.py, complex128 on the same data
rounded to the element type).  Cases and data: coilcomp_cases.py.

Every stage is compared against the reference fed with the GPU's own output of the stage before, so that a bar belongs to one kernel.
With ε = 2^-52 and ε_T = 2^-52 or 2^-23:
  * Gram: |ΔR[c,c']| <= (n + 8) ε sqrt(R_cc R_c'c'), the summation bound; ComplexF32 inputs and their products are exact in FP64, so it
    holds for both element types.
  * eigen stage, against ``np.linalg.eigh`` of the GPU's own Gram matrix: eigenvalues within max(64, 4 x recorded) ε λ_max, the rows
    compared up to a phase within max(16, 4 x recorded) ε, `recorded` being the reference's own Jacobi-against-LAPACK difference that
    test_coilcomp_host.py prints and checks against coilcomp_cases.SELF_EPS; A Aᴴ − I (A Ψ Aᴴ − I) within max(64, 4 x recorded) ε.
    The bars come from the reference, never from the kernel.
  * apply, against complex128 numpy with the matrix the GPU used: relative L2 <= 4 C ε_T (direct sums of C terms).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import coilcomp_cases as CC  # noqa: E402
import coilcomp_reference as CR  # noqa: E402

TYPES = ["c128", "c64"]
EPS = 2.0 ** -52
SMALL = (8, 210)


def _dev(y):
    """One 16-byte aligned allocation per vector."""
    return tuple(torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in y)


def _host(xs):
    return np.stack([v.cpu().numpy() for v in xs])


def _compressor(Z, ncoils):
    from nufft_pkg import nufft
    return nufft.CoilCompressor(torch.complex128 if Z == "c128" else torch.complex64, ncoils, device="cuda:0")


def _check_gram(tag, got, y, h=None, n=None):
    """``y``: the data as the device saw them."""
    want = CR.gram(y, h)
    n = y.shape[1] if n is None else n
    d = np.sqrt(np.abs(want.diagonal().real))
    scale = np.outer(d, d)
    err = float((np.abs(got - want) / np.where(scale > 0, scale, 1.0)).max()) / EPS
    print(f"{tag}: Gram {err:.2f} ε of sqrt(R_cc R_c'c') (bar {n + 8})")
    assert err <= n + 8
    assert np.array_equal(got, got.conj().T) and not got.diagonal().imag.any()


def _check_eigen(tag, C_, n, noise, R, A, lam, sweeps, status, psi=None):
    """The eigen stage against ``np.linalg.eigh`` of the Gram matrix the device itself accumulated."""
    want_A, want_lam = CR.compression_matrix(R, psi)
    rows = CC.rows_compared(C_, n)
    bar_rows, bar_eig, bar_ortho = CC.bars(C_, n, noise)
    ed = float(np.abs(lam - want_lam).max() / want_lam[0]) / EPS
    rd = float(CR.row_difference(A[:rows], want_A[:rows]).max()) / EPS
    ortho = float(np.abs(A @ (np.eye(C_) if psi is None else psi) @ A.conj().T - np.eye(C_)).max()) / EPS
    print(f"{tag}: eigenvalues {ed:.2f} ε λ_max (bar {bar_eig:.0f}), {rows} rows {rd:.2f} ε (bar {bar_rows:.0f}), orthogonality {ortho:.2f} ε "
          f"(bar {bar_ortho:.0f}), {sweeps} sweeps")
    assert ed <= bar_eig and rd <= bar_rows and ortho <= bar_ortho
    assert status == 0 and ((C_ == 1 and sweeps == 0) or 1 <= sweeps < 24)
    assert (np.diff(lam) <= 0).all()
    if psi is None:                                                  # the phase rule on its own: u_v is the conjugate of row v
        k = np.argmax(np.abs(A), axis=1)
        big = A[np.arange(C_), k]
        assert np.abs(big.imag).max() <= 2 * EPS and big.real.min() > 0
        assert np.abs(np.linalg.norm(A, axis=1) - 1).max() <= 8 * EPS


def _check_apply(tag, A, y, out, V, eps):
    want = CR.apply(A, y, V)
    got = out.astype(np.complex128)
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    bar = 4 * y.shape[0] * eps
    print(f"{tag}: apply V={V} relative L2 {err / eps:.2f} ε_T (bar {4 * y.shape[0]})")
    assert err <= bar


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("C_,n", CC.CASES)
def test_stages(C_, n, Z):
    _, Zc, _, eps = CC.dt(Z)
    y = CC.data(C_, n).astype(Zc)
    yd = _dev(y)
    cc = _compressor(Z, C_)
    assert cc.fit(yd) is cc
    R, A = cc.gram(), cc.matrix()
    lam, sweeps, status = cc.spectrum()
    info = cc.info(n)
    print(f"{Z} C={C_} n={n}: tiles of {info.tile_samples} samples in {info.segments} segments, {info.tiles} tiles, {info.workgroups} workgroups, "
          f"{info.lds_bytes_gram} / {info.lds_bytes_eigen} B of LDS")
    assert (info.ncoils, info.n, info.matrix_rows, info.has_noise, info.device) == (C_, n, C_, 0, 0)
    assert info.tiles == -(-n // info.tile_samples) and n % info.tile_samples != 0      # every case has a last tile that is not full
    tag = f"{Z} C={C_} n={n}"
    _check_gram(tag, R, y)
    _check_eigen(tag, C_, n, False, R, A, lam, sweeps, status)
    assert np.array_equal(cc.eigenvalues, lam) and cc.last_sweeps() == sweeps and np.array_equal(cc.matrix(1), A[:1])
    # apply with the GPU's own matrix, every virtual coil; the inputs are only read
    out = cc.apply(yd, C_)
    assert np.array_equal(_host(yd), y) and all(o.data_ptr() % 16 == 0 and o.shape == yd[0].shape for o in out)
    got = _host(out)
    _check_apply(tag, A, y, got, C_, eps)
    e_in = (np.abs(y.astype(np.complex128)) ** 2).sum(axis=0)
    e_out = (np.abs(got.astype(np.complex128)) ** 2).sum(axis=0)
    err = float((np.abs(e_out - e_in) / e_in).max()) / eps
    print(f"  Σ_v |out_v|² against Σ_c |in_c|² per sample: {err:.2f} ε_T (bar {8 * C_ + 128})")
    assert err <= 8 * C_ + 128
    cc.close()


@pytest.mark.parametrize("Z", TYPES)
def test_more_than_one_tile_per_workgroup(Z):
    """A workgroup takes more than one tile, and both the last tile and the last workgroup are partial (asserted through get_info);
    with weights that contain exact zeros."""
    _, Zc, _, eps = CC.dt(Z)
    C_, n = CC.BIG
    cc = _compressor(Z, C_)
    while True:
        i = cc.info(n)
        if i.tiles_per_workgroup > 1 and n % i.tile_samples and i.tiles % i.tiles_per_workgroup:
            break
        n -= 7
    assert n > 39000 and i.workgroups * i.tiles_per_workgroup > i.tiles > (i.workgroups - 1) * i.tiles_per_workgroup
    print(f"{Z}: n = {n}, {i.tiles} tiles of {i.tile_samples}, {i.tiles_per_workgroup} per workgroup, {i.workgroups} workgroups")
    y = CC.data(C_, CC.BIG[1])[:, :n].astype(Zc)
    h = CC.weights(n).astype(CC.dt(Z)[0])
    yd = _dev(y)
    cc.fit(yd, weights=torch.from_numpy(h).cuda())
    R = cc.gram()
    _check_gram(f"{Z} C={C_} n={n} weighted", R, y, h.astype(np.float64))
    cc.fit(yd)
    _check_gram(f"{Z} C={C_} n={n}", cc.gram(), y)
    cc.close()


@pytest.mark.parametrize("Z", TYPES)
def test_weights_with_exact_zeros(Z):
    T, Zc, _, eps = CC.dt(Z)
    C_, n = SMALL
    y = CC.data(C_, n).astype(Zc)
    h = CC.weights(n).astype(T)
    assert 0.1 < (h == 0).mean() < 0.5
    cc = _compressor(Z, C_)
    hd = torch.from_numpy(h).cuda()
    R = cc.fit(_dev(y), weights=hd).gram()
    _check_gram(f"{Z} weighted", R, y, h.astype(np.float64))
    # a zero weight contributes exactly nothing: other (finite) data under the zeros, the same bits
    y2 = y.copy()
    y2[:, h == 0] = (1e3 - 2e3j)
    assert np.array_equal(cc.fit(_dev(y2), weights=hd).gram(), R)
    # removed from the middle the order of the sums changes: within the bar
    keep = h != 0
    R3 = cc.fit(_dev(y[:, keep]), weights=torch.from_numpy(h[keep]).cuda()).gram()
    _check_gram(f"{Z} zero-weight samples removed", R3, y[:, keep], h[keep].astype(np.float64), n=n)
    # removed from the end of the last tile the tiling of the rest is unchanged: the same bits
    i = cc.info(n)
    cut = n - 10
    assert -(-cut // i.tile_samples) == i.tiles and cc.info(cut).tile_samples == i.tile_samples and cc.info(cut).segments == i.segments
    h4 = h.copy()
    h4[cut:] = 0
    full = cc.fit(_dev(y), weights=torch.from_numpy(h4).cuda()).gram()
    short = cc.fit(_dev(y[:, :cut]), weights=torch.from_numpy(h4[:cut]).cuda()).gram()
    assert np.array_equal(full, short)
    cc.close()


@pytest.mark.parametrize("Z", TYPES)
def test_two_sets_and_frames(Z):
    """Two sets of different length accumulated one after the other agree with the concatenation within the bar, and give the same bits
    in every run; the list form of fit with a matching list of weights."""
    T, Zc, _, eps = CC.dt(Z)
    C_, n = SMALL
    y = CC.data(C_, n).astype(Zc)
    h = CC.weights(n).astype(T)
    a, b = _dev(y[:, :77]), _dev(y[:, 77:])
    cc = _compressor(Z, C_)
    cc.reset()
    cc.accumulate(a)
    cc.accumulate(b)
    R = cc.gram()
    _check_gram(f"{Z} two sets", R, y)
    assert np.array_equal(cc.fit([a, b]).gram(), R)
    Rw = cc.fit([a, b], weights=[torch.from_numpy(h[:77]).cuda(), torch.from_numpy(h[77:]).cuda()]).gram()
    _check_gram(f"{Z} two weighted sets", Rw, y, h.astype(np.float64))
    with pytest.raises(ValueError):
        cc.fit([a, b], weights=[torch.from_numpy(h[:77]).cuda()])
    cc.close()


def test_scaled_float32_data_keep_the_bar():
    C_, n = SMALL
    y = (CC.data(C_, n).astype(np.complex64) * np.float32(2.0 ** 70)).astype(np.complex64)
    assert np.isfinite(y).all()
    cc = _compressor("c64", C_)
    R = cc.fit(_dev(y)).gram()
    assert np.isfinite(R).all() and R[0, 0].real > 2.0 ** 130
    _check_gram("c64 data x 2^70", R, y)
    cc.close()


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("C_,n", CC.NOISE_CASES)
def test_whitened(C_, n, Z):
    _, Zc, _, eps = CC.dt(Z)
    y = CC.data(C_, n, noise=True).astype(Zc)
    psi = CC.psi(C_)
    yd = _dev(y)
    cc = _compressor(Z, C_)
    cc.fit(yd, noise=psi)
    assert cc.info().has_noise == 1
    R, A = cc.gram(), cc.matrix()
    lam, sweeps, status = cc.spectrum()
    tag = f"{Z} C={C_} n={n} whitened"
    _check_gram(tag, R, y)
    _check_eigen(tag, C_, n, True, R, A, lam, sweeps, status, psi=psi)
    V = CC.rows_compared(C_, n)
    _check_apply(tag, A, y, _host(cc.apply(yd, V)), V, eps)
    # Ψ from a noise scan: its Gram matrix over its length, formed by the object
    rng = np.random.default_rng(5)
    L = np.linalg.cholesky(psi)
    scan = (L @ (rng.standard_normal((C_, 400)) + 1j * rng.standard_normal((C_, 400))) / np.sqrt(2)).astype(Zc)
    cc.fit(yd, noise=_dev(scan))
    A_scan = cc.matrix()
    est = CR.gram(scan) / 400
    err = float(np.abs(A_scan @ est @ A_scan.conj().T - np.eye(C_)).max())
    print(f"{tag}: A Ψ_scan Aᴴ − I {err / EPS:.1f} ε")
    assert err <= 1e4 * EPS                                           # about C cond(Ψ_scan) ε, and cond(Ψ_scan) is a few hundred at C = 33
    # back to W = I: the unwhitened matrix, bit for bit that of a fresh object
    cc.set_noise_covariance(None)
    plain = cc.fit(yd).matrix()
    other = _compressor(Z, C_)
    assert np.array_equal(plain, other.fit(yd).matrix()) and cc.info().has_noise == 0
    other.close()
    cc.close()


@pytest.mark.parametrize("Z", TYPES)
def test_apply_with_a_given_matrix(Z):
    """set_matrix with V = 1, 16, 17 (the second chunk of 16 virtual coils) and C at C = 33; outputs given; an image-shaped input."""
    _, Zc, _, eps = CC.dt(Z)
    C_, n = 33, 1000
    y = CC.data(C_, n).astype(Zc)
    yd = _dev(y)
    rng = np.random.default_rng(3)
    A = (rng.standard_normal((C_, C_)) + 1j * rng.standard_normal((C_, C_))) / np.sqrt(C_)
    cc = _compressor(Z, C_)
    with pytest.raises(ValueError, match="finish"):
        cc.apply(yd, 1)                                              # neither finish nor set_matrix yet
    for V in (1, 16, 17, C_):
        cc.set_matrix(A[:V])
        assert cc.info().matrix_rows == V and np.array_equal(cc.matrix()[:V], A[:V]) and not cc.matrix()[V:].any()
        out = tuple(torch.full((n,), 7, dtype=yd[0].dtype, device="cuda") for _ in range(V))
        assert cc.apply(yd, V, out=out) is out
        _check_apply(f"{Z} C={C_} given matrix", A, y, _host(out), V, eps)
        if V < C_:
            with pytest.raises(ValueError):
                cc.apply(yd, V + 1)
    assert np.array_equal(_host(yd), y)
    cc.close()
    # the same call compresses coil images: a (10, 12) image per coil gives what the flat vectors give, bit for bit
    C_ = 8
    img = CC.data(C_, 210)[:, :120].astype(Zc)
    cc = _compressor(Z, C_)
    flat = _dev(img)
    shaped = tuple(v.reshape(10, 12).clone() for v in flat)
    cc.fit(flat)
    Rf, Af = cc.gram(), cc.matrix()
    a = cc.apply(flat, 3)
    cc.fit(shaped)
    b = cc.apply(shaped, 3)
    assert np.array_equal(cc.gram(), Rf) and np.array_equal(cc.matrix(), Af)
    assert all(tuple(v.shape) == (10, 12) for v in b) and np.array_equal(_host(a), _host(b).reshape(3, 120))
    # a stacked tensor with an odd number of ComplexF32 elements per coil: every second slice is copied to an aligned place
    stacked = torch.from_numpy(np.ascontiguousarray(img[:, :119])).cuda()
    c = cc.fit(tuple(flat)).apply(stacked, 3)
    _check_apply(f"{Z} stacked", Af, img[:, :119], _host(c), 3, eps)
    cc.close()


@pytest.mark.parametrize("Z", TYPES)
def test_zero_data(Z):
    """A zero Gram matrix gives A = W, λ = 0 and status 0."""
    C_ = 5
    cc = _compressor(Z, C_)
    zeros = tuple(torch.zeros(40, dtype=cc.Z, device="cuda") for _ in range(C_))
    cc.fit(zeros)
    lam, sweeps, status = cc.spectrum()
    assert np.array_equal(cc.matrix(), np.eye(C_)) and not lam.any() and status == 0 and not cc.gram().any()
    with pytest.raises(ValueError):
        cc.choose()
    psi = CC.psi(8)[:C_, :C_]
    cc.fit(zeros, noise=psi)
    W = CR.whitening_matrix(psi)
    assert np.abs(cc.matrix() - W).max() <= 64 * EPS * np.abs(W).max() and not cc.eigenvalues.any()
    cc.close()


@pytest.mark.parametrize("Z", TYPES)
def test_repeatability(Z):
    """Repeated calls, a side stream and a torch.cuda.graph replay of reset + accumulate + finish + apply give the same bits."""
    T, Zc, _, eps = CC.dt(Z)
    C_, n = SMALL
    y = CC.data(C_, n, noise=True).astype(Zc)
    yd = _dev(y)
    hd = torch.from_numpy(CC.weights(n).astype(T)).cuda()
    cc = _compressor(Z, C_)
    cc.set_noise_covariance(CC.psi(C_))
    out = tuple(torch.empty(n, dtype=yd[0].dtype, device="cuda") for _ in range(3))

    def run():
        cc.reset()
        cc.accumulate(yd, hd)
        cc.finish()
        cc.apply(yd, 3, out=out)

    def state():
        return cc.gram(), cc.matrix(), cc.eigenvalues, _host(out)

    run()
    first = state()
    run()
    assert all(np.array_equal(a, b) for a, b in zip(first, state()))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for o in out:
            o.zero_()
        run()
        again = state()                                              # the host reads synchronise the side stream
    torch.cuda.current_stream().wait_stream(side)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
        for read in (cc.gram, cc.matrix, cc.spectrum, lambda: cc.set_matrix(first[1]), lambda: cc.set_noise_covariance(CC.psi(C_))):
            with pytest.raises(ValueError, match="capturing"):
                read()
    for o in out:
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(first, state()))
    g.replay()
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(first, state()))
    cc.close()


def test_choose_and_one_shot():
    from nufft_pkg import nufft
    C_, n = SMALL
    y = CC.data(C_, n).astype(np.complex64)
    yd = _dev(y)
    cc = _compressor("c64", C_)
    cc.fit(yd)
    lam = cc.eigenvalues
    for energy in (0.5, 0.9, 0.98, 1.0):
        V = cc.choose(energy)
        assert lam[:V].sum() >= energy * lam.sum() * (1 - 4 * EPS) and (V == 1 or lam[:V - 1].sum() < energy * lam.sum())
    assert cc.choose(0.5) == 2 and cc.choose(0.98) == 7                # ρ = 0.6: the shares accumulate to 0.41, 0.65, ..., 0.970, 0.989
    for bad in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError):
            cc.choose(bad)
    want = _host(cc.apply(yd, 4))
    assert np.array_equal(_host(nufft.compress_coils(yd, 4)), want)
    assert np.array_equal(_host(nufft.compress_coils(torch.stack(yd), nvirtual=4)), want)
    assert "8 coils" in repr(cc)
    cc.close()


def test_refusals():
    from nufft_pkg import nufft
    L, lib = nufft._lib, nufft.lib
    for bad in (0, 65, -3):
        with pytest.raises(ValueError):
            nufft.CoilCompressor(torch.complex64, bad, device="cuda:0")
    C_, n = 3, 35
    y = CC.data(C_, n).astype(np.complex64)
    yd = _dev(y)
    cc = _compressor("c64", C_)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = lambda ts: (C.c_void_p * len(ts))(*[t if isinstance(t, int) else t.data_ptr() for t in ts])   # noqa: E731
    h = cc._handle
    # apply before finish
    out = tuple(torch.empty(n, dtype=torch.complex64, device="cuda") for _ in range(C_))
    assert lib.nufft_coilcomp_apply(h, table(out), 1, table(yd), n, stream) == L.ERR_INVALID_ARG and b"finish" in lib.nufft_last_error_message()
    with pytest.raises(ValueError):
        cc.matrix()
    # accumulate: n, null and misaligned vectors, misaligned weights
    assert lib.nufft_coilcomp_accumulate(h, table(yd), None, 0, stream) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_accumulate(h, table([yd[0], 0, yd[2]]), None, n, stream) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_accumulate(h, table([yd[0], yd[1].data_ptr() + 8, yd[2]]), None, n - 1, stream) == L.ERR_INVALID_ARG
    w = torch.ones(n + 1, dtype=torch.float32, device="cuda")
    assert lib.nufft_coilcomp_accumulate(h, table(yd), C.c_void_p(w.data_ptr() + 2), n, stream) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_accumulate(h, table(yd), C.c_void_p(w.data_ptr() + 4), n, stream) == L.OK
    assert cc.gram().any()
    cc.fit(yd)
    # V out of range
    for V in (0, C_ + 1, -1):
        assert lib.nufft_coilcomp_apply(h, table(out), V, table(yd), n, stream) == L.ERR_INVALID_ARG
        with pytest.raises(ValueError):
            cc.apply(yd, V)
    assert lib.nufft_coilcomp_apply(h, table(out), 1, table(yd), 0, stream) == L.ERR_INVALID_ARG
    # misaligned and overlapping vectors
    big = torch.empty(2 * n + 2, dtype=torch.complex64, device="cuda")
    assert lib.nufft_coilcomp_apply(h, table([big.data_ptr() + 8]), 1, table(yd), n, stream) == L.ERR_INVALID_ARG
    assert lib.nufft_coilcomp_apply(h, table([yd[1]]), 1, table(yd), n, stream) == L.ERR_INVALID_ARG and b"overlaps an input" in lib.nufft_last_error_message()
    assert lib.nufft_coilcomp_apply(h, table([big, big.data_ptr() + 16]), 2, table(yd), n, stream) == L.ERR_INVALID_ARG and b"two outputs" in lib.nufft_last_error_message()
    with pytest.raises(ValueError):
        cc.apply(yd, 1, out=(yd[2],))
    with pytest.raises(ValueError):
        cc.apply(yd, 1, out=(big[1:n + 1],))                        # 8 bytes off a 16-byte boundary
    # wrong count, wrong type, wrong device, unequal lengths, not contiguous
    other = torch.zeros(n, dtype=torch.complex128, device="cuda")
    for bad in (yd[:2], yd + (yd[0],), (yd[0], yd[1], other), (yd[0], yd[1], yd[2][:-1]), (yd[0], yd[1], yd[2].cpu()),
                (yd[0], yd[1], torch.zeros(2 * n, dtype=torch.complex64, device="cuda")[::2])):
        for call in (cc.accumulate, lambda v: cc.apply(v, 1)):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError):
        cc.apply(yd, 2, out=out[:1])
    with pytest.raises(ValueError):
        cc.apply(yd, 1, out=(torch.empty(n + 1, dtype=torch.complex64, device="cuda"),))
    with pytest.raises(ValueError):
        cc.accumulate(yd, weights=torch.ones(n - 1, device="cuda"))
    with pytest.raises(ValueError):
        cc.accumulate(yd, weights=torch.ones(n))
    # set_matrix and the noise covariance
    for bad in (np.eye(C_)[:, :2], np.zeros((C_ + 1, C_)), np.full((1, C_), np.nan), np.zeros(C_)):
        with pytest.raises(ValueError):
            cc.set_matrix(bad)
    for bad in (np.eye(C_ + 1), -np.eye(C_), np.eye(C_) + np.triu(np.ones((C_, C_)), 1), np.full((C_, C_), np.inf)):
        with pytest.raises(ValueError):
            cc.set_noise_covariance(bad)
    assert cc.info().has_noise == 0
    # use after close
    cc.close()
    cc.close()
    for call in (cc.reset, cc.finish, cc.gram, cc.matrix, cc.spectrum, cc.info, lambda: cc.accumulate(yd), lambda: cc.apply(yd, 1),
                 lambda: cc.set_matrix(np.eye(C_)), lambda: cc.set_noise_covariance(None), lambda: cc.fit(yd), cc.choose):
        with pytest.raises(ValueError, match="closed"):
            call()
