"""The global low-rank map and the temporal transform on the GPU against numpy (lps_reference.py).  Inputs: the
right-hand sides of lps_cases.py (n = 9, 35 and 210 cells leave a last tile that is not full; K = 17 and 32 use the wide Jacobi team;
K = 9 and 17 are DFT lengths that are no power of two; 32³ cells take more than one workgroup).

Bars:
  * map against ``np.linalg.svd`` with t at the median singular value: relative L2 and nuclear norm <= 256 ε of the element type (four
    times the locally low-rank bar: the Gram sums run over n cells); t = 0 returns the input within the bar; t > σ_max and a zero input
    give exact zeros; ComplexF32 data scaled by 2⁷⁰ keep the bar; in place, repeated and graph-replayed calls are bit-equal.
  * transform against ``np.fft``: relative L2 <= 4 K ε (direct sums of K terms with once-rounded twiddles), Parseval within the same bar;
    forward and inverse each on an input the host knows; the shrink and its 1-norm against ``tshrink`` within the same bar, relative
    to the thresholded reference; ``"identity"`` is bit-equal to the plain complex soft threshold.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import lps_cases as LC  # noqa: E402
import lps_reference as P  # noqa: E402

TYPES = ["c128", "c64"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(xs):
    return np.stack([v.cpu().numpy() for v in xs])


def _plan(nufft, Z, Ns, K):
    return nufft.PlanNUFFT(LC.dt(Z)[1], Ns, backend=nufft.ROCBackend(0), ntransforms=K)


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,K", LC.MAP_CASES)
def test_map_against_the_svd(Ns, K, Z):
    from nufft_pkg import nufft
    _, Zc, _, eps = LC.dt(Z)
    plan = _plan(nufft, Z, Ns, K)
    glr = nufft.GlobalLowRank(plan)
    plan.close()
    x = LC.case(Ns, K).b.astype(Zc)
    sv = P.singular_values(x)
    t = float(np.median(sv)) if K > 1 else 0.5 * float(sv[0])
    want, nuc, zeroed = P.svt(x, t)
    xd = tuple(_dev(v) for v in x)
    y, nd = glr.apply(xd, t)
    got, sweeps = _host(y), glr.last_sweeps()
    err, en = LC.rel(got, want), abs(float(nd.cpu()[0]) - nuc) / nuc
    info = glr.info()
    print(f"map {Z} N={Ns} K={K}: {err / eps:.1f} ε, nuclear norm {en / eps:.1f} ε (bar 256 ε), {sweeps} sweeps, {zeroed}/{K} zeroed, "
          f"tile {info.tile_cells} cells, {info.workgroups} workgroups")
    assert err <= 256 * eps and en <= 256 * eps
    assert (K == 1 and sweeps == 0) or 2 <= sweeps < info.jacobi_sweeps_max == 24
    assert K == 1 or 0 < zeroed < K
    assert (info.cells, info.ntransforms) == (int(np.prod(Ns)), K) and np.array_equal(_host(xd), x)      # the input is only read
    # t = 0: the input; t above σ_max and a zero input: exact zeros
    y0, n0 = glr.apply(xd, 0.0)
    assert LC.rel(_host(y0), x) <= 256 * eps and abs(float(n0.cpu()[0]) - sv.sum()) <= 256 * eps * sv.sum()
    yz, nz = glr.apply(xd, 1.01 * float(sv[0]))
    assert not _host(yz).any() and float(nz.cpu()[0]) == 0.0
    yz, nz = glr.apply(tuple(torch.zeros_like(v) for v in xd), t)
    assert not _host(yz).any() and float(nz.cpu()[0]) == 0.0
    # repeated and in place: the same bits
    y2, _ = glr.apply(xd, t)
    assert np.array_equal(_host(y2), got)
    xi = tuple(v.clone() for v in xd)
    yi, _ = glr.apply(xi, t, out=xi)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(yi, xi)) and np.array_equal(_host(xi), got)
    glr.close()


@pytest.mark.parametrize("Z", TYPES)
def test_more_than_one_tile_per_workgroup(Z):
    """A workgroup of the Gram kernel takes more than one tile, and both the last tile and the last workgroup are partial (asserted through
    get_info).  K = 32 frames of 300 x 219 = 65 700 cells: plain seeded data, every singular value present (a random mixing matrix with
    singular values from 1 down to 1/4), no operator."""
    from nufft_pkg import nufft
    _, Zc, _, eps = LC.dt(Z)
    Ns, K = (300, 219), 32
    plan = _plan(nufft, Z, Ns, K)
    glr = nufft.GlobalLowRank(plan)
    plan.close()
    info = glr.info()
    tiles = -(-info.cells // info.tile_cells)
    per_group = -(-tiles // info.workgroups)
    print(f"{Z}: {info.cells} cells, {tiles} tiles of {info.tile_cells}, {per_group} per workgroup, {info.workgroups} workgroups")
    assert info.cells == 65700 and info.workgroups < tiles and per_group > 1
    assert info.cells % info.tile_cells != 0                                              # the last tile is partial
    assert (info.workgroups - 1) * per_group < tiles < info.workgroups * per_group      # and so is the last workgroup
    rng = np.random.default_rng(65700)
    n = info.cells
    q, _ = np.linalg.qr(rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K)))
    mix = q * np.geomspace(1.0, 0.25, K)[None, :]
    x = (mix @ (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n)))).reshape((K,) + Ns[::-1]).astype(Zc)
    t = float(np.median(P.singular_values(x)))
    want, nuc, zeroed = P.svt(x, t)
    xd = tuple(_dev(v) for v in x)
    y, nd = glr.apply(xd, t)
    got = _host(y)
    err, en = LC.rel(got, want), abs(float(nd.cpu()[0]) - nuc) / nuc
    print(f"map {Z} N={Ns} K={K}: {err / eps:.1f} ε, nuclear norm {en / eps:.1f} ε (bar 256 ε), {glr.last_sweeps()} sweeps, {zeroed}/{K} zeroed")
    assert err <= 256 * eps and en <= 256 * eps
    assert 0 < zeroed < K
    y2, n2 = glr.apply(xd, t)
    assert np.array_equal(_host(y2), got) and np.array_equal(n2.cpu().numpy(), nd.cpu().numpy())
    glr.close()


@pytest.mark.parametrize("Ns,K", [((32, 40), 8), ((12, 10), 17)])
def test_large_values_in_single_precision(Ns, K):
    from nufft_pkg import nufft
    eps = LC.dt("c64")[3]
    plan = _plan(nufft, "c64", Ns, K)
    glr = nufft.GlobalLowRank(plan)
    plan.close()
    x = (LC.case(Ns, K).b.astype(np.complex64) * np.float32(2.0 ** 70)).astype(np.complex64)
    assert np.isfinite(x).all()
    t = float(np.median(P.singular_values(x)))
    want, nuc, _ = P.svt(x, t)
    y, nd = glr.apply(tuple(_dev(v) for v in x), t)
    err, en = LC.rel(_host(y), want), abs(float(nd.cpu()[0]) - nuc) / nuc
    print(f"2^70-scaled c64 N={Ns} K={K}: {err / eps:.1f} ε, nuclear norm {en / eps:.1f} ε")
    assert err <= 256 * eps and en <= 256 * eps
    glr.close()


@pytest.mark.parametrize("Z,Ns,K", [("c64", (32, 40), 3), ("c128", (12, 10), 17)])
def test_graph_replay_gives_the_same_bits(Z, Ns, K):
    from nufft_pkg import nufft
    Zc = LC.dt(Z)[1]
    plan = _plan(nufft, Z, Ns, K)
    glr, ts = nufft.GlobalLowRank(plan), nufft.TemporalSparsity(plan, "dft")
    plan.close()
    x = LC.case(Ns, K).b.astype(Zc)
    t = float(np.median(P.singular_values(x)))
    tc = float(np.median(np.abs(P.tdft(x))))
    xd = tuple(_dev(v) for v in x)
    y, nd = glr.apply(xd, t)
    c, l1 = ts.shrink(xd, tc)
    torch.cuda.synchronize()
    want, want_n, want_c, want_l = _host(y), nd.cpu().numpy(), _host(c), l1.cpu().numpy()
    out, oc = tuple(torch.zeros_like(v) for v in xd), tuple(torch.zeros_like(v) for v in xd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _, gn = glr.apply(xd, t, out=out)
        _, gl = ts.shrink(xd, tc, out=oc)
    for _ in range(2):
        for o in out + oc:
            o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_host(out), want) and np.array_equal(gn.cpu().numpy(), want_n)
        assert np.array_equal(_host(oc), want_c) and np.array_equal(gl.cpu().numpy(), want_l)
    del graph
    glr.close()
    ts.close()


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,K", LC.MAP_CASES)
def test_temporal_transform(Ns, K, Z):
    from nufft_pkg import nufft
    _, Zc, _, eps = LC.dt(Z)
    bar = 4 * K * eps
    plan = _plan(nufft, Z, Ns, K)
    ts, ident = nufft.TemporalSparsity(plan, "dft"), nufft.TemporalSparsity(plan, "identity")
    plan.close()
    x = LC.case(Ns, K).b.astype(Zc)
    xd = tuple(_dev(v) for v in x)
    want = P.tdft(x)
    c = ts.forward(xd)
    got = _host(c)
    back = _host(ts.inverse(c))
    ef, ei = LC.rel(got, want), LC.rel(back, x)
    ev = LC.rel(_host(ts.inverse(xd)), P.tdft(x, inverse=True))                          # the inverse on the host's input
    ep = abs(np.linalg.norm(got.astype(np.complex128)) - np.linalg.norm(x.astype(np.complex128))) / np.linalg.norm(x.astype(np.complex128))
    t = float(np.median(np.abs(want))) if K > 1 else float(np.median(np.abs(x)))
    s, l1 = ts.shrink(xd, t)
    ws, wl, share = P.tshrink(want.astype(Zc), t)
    es = LC.rel(_host(s), ws)
    el = abs(float(l1.cpu()[0]) - wl) / wl
    print(f"transform {Z} N={Ns} K={K}: forward {ef / eps:.2f} ε, inverse {ev / eps:.2f} ε, round trip {ei / eps:.2f} ε, Parseval {ep / eps:.2f} ε, shrink {es / eps:.2f} ε, "
          f"l1 {el / eps:.2f} ε (bar {4 * K} ε), zero share {share:.2f}, tile {ts.info().tile_cells} cells")
    assert ef <= bar and ev <= bar and ep <= bar and es <= bar and el <= bar
    assert ei <= 2 * bar                                                                 # the round trip is two transforms
    assert 0.2 <= share <= 0.95
    wd = tuple(_dev(v) for v in ws)                                                      # the proximal map: Tᴴ of the reference's coefficients
    assert LC.rel(_host(ts.inverse(wd)), P.tdft(ws, inverse=True)) <= bar
    # in place
    xi = tuple(v.clone() for v in xd)
    ts.forward(xi, out=xi)
    assert np.array_equal(_host(xi), got)
    # the identity: copies, and the plain complex soft threshold bit for bit
    assert np.array_equal(_host(ident.forward(xd)), x) and np.array_equal(_host(ident.inverse(xd)), x)
    ti = float(np.median(np.abs(x)))
    si, li = ident.shrink(xd, ti)
    wi, wli, share_i = P.tshrink(x, ti)
    assert np.array_equal(_host(si), wi) and 0.2 <= share_i <= 0.95
    assert abs(float(li.cpu()[0]) - wli) <= 64 * eps * np.sqrt(x.size) * wli
    ts.close()
    ident.close()


def test_refusals():
    from nufft_pkg import nufft
    lib, chk, tab = nufft.lib, nufft.plan._check, nufft.plan._ptr_table
    wide = _plan(nufft, "c128", (12, 10), 33)
    real = nufft.PlanNUFFT(np.float64, (12, 10), backend=nufft.ROCBackend(0), ntransforms=3)
    for make in (lambda: nufft.GlobalLowRank(wide), lambda: nufft.TemporalSparsity(wide), lambda: nufft.GlobalLowRank(real),
                 lambda: nufft.TemporalSparsity(real, "identity"), lambda: nufft.TemporalSparsity(wide, "difference")):
        with pytest.raises(ValueError):
            make()
    op = nufft.ToeplitzOperator(wide)
    with pytest.raises(ValueError, match="33 transforms"):
        nufft.ToeplitzLPS(op, 0.1, 0.1, step=0.5)
    op.close()
    wide.close()
    real.close()
    K, n = 3, 9
    plan = _plan(nufft, "c64", (n,), K)
    glr, ts = nufft.GlobalLowRank(plan), nufft.TemporalSparsity(plan)
    plan.close()
    x = tuple(torch.ones(n, dtype=torch.complex64, device="cuda") for _ in range(K))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            glr.apply(x, bad)
        with pytest.raises(ValueError):
            ts.shrink(x, bad)
    buf = torch.zeros(4 * n, dtype=torch.complex64, device="cuda")
    odd = (buf[1:1 + n],) + x[1:]                                                  # 8 bytes off a 16-byte boundary
    part = (x[0], buf[2:2 + n], buf[4:4 + n])                                      # two outputs that overlap each other
    for out in (odd, part):
        with pytest.raises(ValueError):
            glr.apply(x, 0.1, out=out)
        with pytest.raises(ValueError):
            ts.forward(x, out=out)
    with pytest.raises(ValueError):                                                # an output that is another frame's input
        chk(lib.nufft_glr_apply(glr._handle, tab((x[1], x[0], x[2])), tab(x), 0.1, None, glr._stream()))
    half = (buf[2 * n:3 * n], x[1], x[2])
    with pytest.raises(ValueError):                                                # partial overlap of an output with its own input
        glr.apply(half, 0.1, out=(buf[2 * n + 2:3 * n + 2], torch.empty_like(x[1]), torch.empty_like(x[2])))
    with pytest.raises(nufft.DimensionMismatch):
        glr.apply(x[:2], 0.1)
    with pytest.raises(ValueError):
        glr.apply(tuple(v.to(torch.complex128) for v in x), 0.1)
    y, nuc = glr.apply(x, 0.0)                                                     # rank 1: σ = sqrt(n K)
    torch.cuda.synchronize()
    assert abs(float(nuc.cpu()[0]) - np.sqrt(n * K)) <= 1e-6
    glr.close()
    ts.close()
    with pytest.raises(ValueError, match="closed"):
        glr.apply(x, 0.1)
