"""The wavelet transform and its proximal map on the GPU, against the numpy reference (wavelet_reference.py) in float64,
and the power iteration of the Toeplitz operator against numpy on the exact matrix.

Bars, with ε = 2⁻⁵² (ComplexF64) / 2⁻²³ (ComplexF32): forward, inverse and shrink rel-L2 <= 64 ε (each of at most L · D = 9 stages sums
at most 4 products: about 36 ε in the worst case, the rest is room for the reference's own rounding); inverse(forward(a)) against a
128 ε; the ℓ1 sum 64 ε √n relative.  The shapes cover sub-boxes smaller than a tile, sides that are no multiple of the tile, a deepest
input exactly one filter long ((16,) at 3 levels, 8 at 2 levels), halos that wrap, and odd deepest sides (40 / 8 = 5).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import fista_cases as FC  # noqa: E402
import sense_reference as SR  # noqa: E402
import subspace_reference as SUB  # noqa: E402
import toeplitz_reference as R  # noqa: E402
import wavelet_reference as W  # noqa: E402

# (Ns, levels): slowest dimension last
SHAPES = [((16,), 3), ((48,), 3), ((24, 40), 3), ((48, 40), 3), ((64, 80), 3), ((8, 12, 20), 2), ((16, 16, 8), 2), ((64, 64, 64), 3)]
WAVELETS = ["haar", "db2"]
TYPES = ["c128", "c64"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _input(Ns, Z, seed=0):
    rng = np.random.default_rng(seed + sum(Ns))
    return (rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1])).astype(FC.dt(Z)[1])


_REFS = {}


def _reference(Ns, levels, Z, wavelet, seed=0):
    """(input in the element type, float64 coefficients of that input), computed once."""
    key = (Ns, levels, Z, wavelet, seed)
    if key not in _REFS:
        a = _input(Ns, Z, seed)
        _REFS[key] = (a, W.forward(a.astype(np.complex128), wavelet, levels))
    return _REFS[key]


def _transform(nufft, Ns, levels, Z, wavelet, C=1, **kw):
    plan = nufft.PlanNUFFT(FC.dt(Z)[1], Ns, backend=nufft.ROCBackend(0), ntransforms=C, **kw)
    wt = nufft.WaveletTransform(plan, wavelet, levels)
    plan.close()
    return wt


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("wavelet", WAVELETS)
@pytest.mark.parametrize("Ns,levels", SHAPES)
def test_forward_and_inverse(Ns, levels, wavelet, Z):
    from nufft_pkg import nufft
    eps = FC.dt(Z)[3]
    a, ref = _reference(Ns, levels, Z, wavelet)
    wt = _transform(nufft, Ns, levels, Z, wavelet)
    assert wt.levels == levels and wt.info().taps == (2 if wavelet == "haar" else 4)
    ad = _dev(a)
    c = wt.forward(ad)
    back = wt.inverse(c)
    inv = wt.inverse(_dev(ref.astype(a.dtype)))
    ef, eb, ei = R.rel(_host(c), ref), R.rel(_host(back), a), R.rel(_host(inv), W.inverse(ref.astype(a.dtype).astype(np.complex128), wavelet, levels))
    print(f"{wavelet} {Z} N={Ns} L={levels}: forward {ef / eps:.1f} ε, inverse {ei / eps:.1f} ε, round trip {eb / eps:.1f} ε")
    assert np.array_equal(_host(ad), a)                                      # the input is only read
    assert ef <= 64 * eps and ei <= 64 * eps and eb <= 128 * eps
    with pytest.raises(ValueError):
        wt.forward(ad, out=ad)
    wt.close()
    with pytest.raises(ValueError, match="closed"):
        wt.forward(ad)


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("wavelet", WAVELETS)
@pytest.mark.parametrize("Ns,levels", [((48,), 3), ((24, 40), 3), ((8, 12, 20), 2), ((64, 64, 64), 3)])
def test_three_components(Ns, levels, wavelet, Z):
    from nufft_pkg import nufft
    eps = FC.dt(Z)[3]
    refs = [_reference(Ns, levels, Z, wavelet, seed) for seed in (0, 1, 2)]
    wt = _transform(nufft, Ns, levels, Z, wavelet, C=3)
    cs = wt.forward(tuple(_dev(a) for a, _ in refs))
    back = wt.inverse(cs)
    for c, b, (a, ref) in zip(cs, back, refs):
        assert R.rel(_host(c), ref) <= 64 * eps and R.rel(_host(b), a) <= 128 * eps
    # per-component thresholds: component 1 is not thresholded at all, component 2 above its largest coefficient
    ts = [float(np.median(np.abs(refs[0][1]))), 0.0, 2 * float(np.abs(refs[2][1]).max())]
    ss, l1 = wt.shrink(tuple(_dev(a) for a, _ in refs), ts)
    mask = W.detail_mask(refs[0][0].shape, levels)
    assert np.array_equal(_host(ss[1]), _host(cs[1]))
    assert not _host(ss[2])[mask].any() and np.array_equal(_host(ss[2])[~mask], _host(cs[2])[~mask])
    want, want_l1 = W.shrink(refs[0][0].astype(np.complex128), wavelet, levels, ts[0])
    assert R.rel(_host(ss[0]), want) <= 64 * eps
    l1 = _host(l1)
    n = refs[0][0].size
    assert abs(l1[0] - want_l1) <= 64 * eps * np.sqrt(n) * want_l1 and l1[2] == 0.0
    assert abs(l1[1] - np.abs(refs[1][1][mask]).sum()) <= 64 * eps * np.sqrt(n) * l1[1]
    with pytest.raises(nufft.DimensionMismatch):
        wt.forward(_dev(refs[0][0]))
    with pytest.raises(nufft.DimensionMismatch):
        wt.shrink(tuple(_dev(a) for a, _ in refs), [0.1, 0.2])


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("wavelet", WAVELETS)
@pytest.mark.parametrize("Ns,levels", SHAPES)
def test_shrink(Ns, levels, wavelet, Z):
    from nufft_pkg import nufft
    eps = FC.dt(Z)[3]
    a, ref = _reference(Ns, levels, Z, wavelet)
    mask = W.detail_mask(a.shape, levels)
    wt = _transform(nufft, Ns, levels, Z, wavelet)
    ad = _dev(a)
    fwd = _host(wt.forward(ad))
    t = float(np.median(np.abs(ref[mask])))
    got, l1 = wt.shrink(ad, t)
    got, l1 = _host(got), float(_host(l1)[0])
    want, want_l1 = W.shrink(a.astype(np.complex128), wavelet, levels, t)
    err = R.rel(got, want)
    zeros = float(np.mean(got[mask] == 0))
    print(f"shrink {wavelet} {Z} N={Ns} L={levels}: values {err / eps:.1f} ε, l1 {abs(l1 - want_l1) / want_l1 / eps:.1f} ε, zero details {zeros:.2f}")
    assert err <= 64 * eps                                                   # values, not zero masks: the map is continuous
    assert 0.3 <= zeros <= 0.7                                               # the threshold is the median: about half are zero
    assert np.array_equal(got[~mask], fwd[~mask])                            # the approximation corner is never thresholded
    assert abs(l1 - want_l1) <= 64 * eps * np.sqrt(a.size) * want_l1
    zero_t, l1_0 = wt.shrink(ad, 0.0)
    assert np.array_equal(_host(zero_t), fwd)                                # t = 0 reproduces forward bit for bit
    assert abs(float(_host(l1_0)[0]) - np.abs(ref[mask]).sum()) <= 64 * eps * np.sqrt(a.size) * np.abs(ref[mask]).sum()
    big, l1_big = wt.shrink(ad, 1.001 * float(np.abs(fwd[mask]).max()))
    big = _host(big)
    assert not big[mask].any() and np.array_equal(big[~mask], fwd[~mask]) and float(_host(l1_big)[0]) == 0.0
    with pytest.raises(ValueError):
        wt.shrink(ad, -1.0)


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("wavelet", WAVELETS)
def test_shift_equivariance_between_fftshift_orders(wavelet, Z):
    """The storage orders of fftshift=True and False plans differ by a cyclic shift of N_d / 2 per axis: 32 and 40, multiples of 2^3, and
    2^4 divides 64 and 80.  So the proximal map of one order is the reordered proximal map of the other."""
    from nufft_pkg import nufft
    Ns, levels = (64, 80), 3
    eps = FC.dt(Z)[3]
    a, ref = _reference(Ns, levels, Z, wavelet)
    t = float(np.median(np.abs(ref)))
    outs = []
    for shift in (False, True):
        wt = _transform(nufft, Ns, levels, Z, wavelet, fftshift=shift)
        x = np.fft.fftshift(a) if shift else a
        y = _host(wt.inverse(wt.shrink(_dev(x), t)[0]))
        outs.append(np.fft.ifftshift(y) if shift else y)
    want = W.inverse(W.shrink(a.astype(np.complex128), wavelet, levels, t)[0], wavelet, levels)
    print(f"shift {wavelet} {Z}: orders differ by {R.rel(outs[1], outs[0]) / eps:.1f} ε, prox error {R.rel(outs[0], want) / eps:.1f} ε")
    assert R.rel(outs[1], outs[0]) <= 64 * eps and R.rel(outs[0], want) <= 64 * eps and R.rel(outs[1], want) <= 64 * eps


def _power(apply, v, iters):
    v = np.asarray(v).astype(np.complex128)
    rho = np.nan
    for _ in range(iters):
        g = apply(v)
        rho = float(np.real(np.vdot(v, g)) / np.real(np.vdot(v, v)))
        v = g / np.linalg.norm(g)
    return rho


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,path,iters", [((48, 40), "fused", 30), ((48,), "dense", 30), ((15, 9), "dense", 30), ((16, 16, 8), "dense", 40)])
def test_max_eigenvalue(Ns, path, iters, Z):
    from nufft_pkg import nufft
    import test_gpu_cg
    _, Zc, bar, _ = FC.dt(Z)
    s = test_gpu_cg._system(Ns)
    assert s.A is not None
    op = s.operator(nufft, Z, path, 2)
    v0 = [b.astype(Zc) for b in s.bs[:2]]
    got = op.max_eigenvalue(iters=iters, v0=tuple(_dev(v) for v in v0))
    for c in range(2):
        want = _power(s.apply, v0[c], iters)
        print(f"max_eigenvalue {Z} N={Ns} {path} c={c}: {got[c]:.6g} (numpy {want:.6g}, λmax {s.lmax:.6g}), rel {abs(got[c] - want) / want:.2e}")
        assert want >= 0.95 * s.lmax                                         # the reference alone gets there from this start
        assert abs(got[c] - want) <= 10 * bar * want
        assert got[c] <= s.lmax * (1 + 10 * bar)
    default = op.max_eigenvalue()
    assert len(default) == 2 and all(0.9 * s.lmax <= v <= s.lmax * (1 + 10 * bar) for v in default)
    assert op.max_eigenvalue() == default                                    # seeded start, fixed-order sums
    with pytest.raises(ValueError):
        op.max_eigenvalue(iters=0)
    with pytest.raises(nufft.DimensionMismatch):
        op.max_eigenvalue(v0=_dev(v0[0]))
    vd = tuple(_dev(v) for v in v0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    gd = tuple(torch.empty_like(v) for v in vd)
    with torch.cuda.graph(graph, stream=side):
        op.apply(vd, out=gd)
        with pytest.raises(ValueError, match="capturing"):                   # it synchronises: refused while capturing
            op.max_eigenvalue(iters=2, v0=vd)
    del graph


@pytest.mark.parametrize("Z", TYPES)
def test_max_eigenvalue_with_coil_maps(Z):
    from nufft_pkg import nufft
    import test_gpu_cg
    Ns, iters = (48, 40), 30
    _, Zc, bar, _ = FC.dt(Z)
    s = test_gpu_cg._system(Ns)
    maps = SR.smooth_maps(2, s.shape, seed=11).astype(Zc)
    op = s.operator(nufft, Z, "fused", 1)
    op.set_maps(_dev(maps))
    A = SR.dense_sense_gram(s.A, maps.astype(np.complex128))
    lmax = float(np.linalg.eigvalsh(A)[-1])
    v0 = s.bs[0].astype(Zc)
    got = op.max_eigenvalue(iters=iters, v0=_dev(v0))[0]
    want = _power(lambda v: (A @ v.ravel()).reshape(v.shape), v0, iters)
    print(f"max_eigenvalue with 2 coil maps {Z}: {got:.6g} (numpy {want:.6g}, λmax {lmax:.6g})")
    assert want >= 0.95 * lmax and abs(got - want) <= 10 * bar * want and got <= lmax * (1 + 10 * bar)


@pytest.mark.parametrize("Z", TYPES)
def test_max_eigenvalue_coupled(Z):
    from nufft_pkg import nufft
    import test_gpu_subspace as TS
    Ns, K, iters = (16, 12), 2, 30
    _, Zc, bar, _ = FC.dt(Z)
    sub = TS._system(Ns, K)
    op = sub.operator(nufft, Z, "dense")
    assert op.coupled
    A = SUB.dense_block_gram(Ns, sub.p.spectra, K)
    lmax = float(np.linalg.eigvalsh(A)[-1])
    v0 = [v.astype(Zc) for v in sub.bs]
    got = op.max_eigenvalue(iters=iters, v0=tuple(_dev(v) for v in v0))
    want = _power(lambda v: np.stack(sub.apply([v[a] for a in range(K)])), np.stack(v0), iters)
    print(f"max_eigenvalue coupled K=2 {Z}: {got} (numpy {want:.6g}, λmax {lmax:.6g})")
    assert got[0] == got[1]                                                  # one vector, one value
    assert want >= 0.95 * lmax and abs(got[0] - want) <= 10 * bar * want and got[0] <= lmax * (1 + 10 * bar)
