"""The framed Toeplitz operator on the GPU: one multiplier per component.

Systems: tvt_cases.frames (one analytic spectrum per frame, exact).  Bars:
  * apply: frame c of the framed operator runs the launches of a plain operator with the multiplier of T_c, so the outputs are
    bit-equal, also in place and with coil maps;
  * multipliers built from points: spreading uses atomics, so a frame's multiplier agrees with that of ``set_points`` on the same points
    within the operator's parity bar (1e-12 / 1e-5 relative), not to the bit; a frame without points is exactly zero;
  * CG: x within the solver bar (1e-11 / 1e-4) of K single-frame solves, statuses equal;
  * changes of build mode (plain, coupled, framed; points and spectra): after every build the operator holds the bytes and returns the
    bits of a fresh operator given that build alone, and a refused build changes nothing.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import sense_reference as SR  # noqa: E402
import subspace_reference as S  # noqa: E402
import toeplitz_reference as R  # noqa: E402
import tvt_cases as TC  # noqa: E402

TYPES = ["c128", "c64"]
SOLVER_BAR = {"c128": 1e-11, "c64": 1e-4}
# (Ns, K, path)
CASES = [((9,), 3, "dense"), ((12, 10), 3, "dense"), ((12, 10), 9, "dense"), ((32, 40), 3, "fused"), ((32, 32, 32), 3, "fused")]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _inputs(s, Zc, seed=1):
    rng = np.random.default_rng(seed)
    return tuple(_dev((rng.standard_normal(s.shape[1:]) + 1j * rng.standard_normal(s.shape[1:])).astype(Zc)) for _ in range(s.K))


def _plain(nufft, s, Z, path, c):
    """A plain one-component operator with frame c's spectrum."""
    Zc = TC.dt(Z)[1]
    opts = {"NUFFT_TOEPLITZ_FUSED": 0} if path == "dense" else {}
    plan = nufft.PlanNUFFT(Zc, s.Ns, backend=nufft.ROCBackend(0), options=opts)
    op = nufft.ToeplitzOperator(plan)
    plan.close()
    op.set_spectrum(_dev(s.spectra[c].astype(Zc)))
    assert op.path == path and not op.framed
    return op


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,K,path", CASES)
def test_apply_is_the_plain_apply_per_frame(Ns, K, path, Z):
    from nufft_pkg import nufft
    Zc = TC.dt(Z)[1]
    s = TC.frames(Ns, K)
    op = s.operator(nufft, Z, path)
    assert op.framed and not op.coupled and nufft.lib.nufft_toeplitz_num_frames(op._handle) == K
    u = _inputs(s, Zc)
    maps = _dev(SR.smooth_maps(2, s.shape[1:], seed=11).astype(Zc))
    got = tuple(v.cpu().numpy() for v in op(u))
    inplace = tuple(v.clone() for v in u)
    assert op(inplace, out=inplace) is inplace                                    # without maps the output may be the input
    op.set_maps(maps)
    got_maps = tuple(v.cpu().numpy() for v in op(u))
    with pytest.raises(ValueError):
        op(inplace, out=inplace)
    op.clear_maps()
    assert len({op.multiplier(frame=c).data_ptr() for c in range(K)}) == K
    for c in range(K):
        one = _plain(nufft, s, Z, path, c)
        want = one(u[c]).cpu().numpy()
        assert np.array_equal(got[c], want) and np.array_equal(inplace[c].cpu().numpy(), want), c
        assert torch.equal(op.multiplier(frame=c), one.multiplier())              # the same multiplier, bit for bit
        one.set_maps(maps)
        assert np.array_equal(got_maps[c], one(u[c]).cpu().numpy()), c
        one.close()
    # the frames differ (a test that compared equal multipliers would show nothing), and the result is G_c u_c of the exact system
    assert not np.array_equal(got[0], tuple(v.cpu().numpy() for v in op((u[0],) * K))[1])
    bar = TC.dt(Z)[2]
    assert max(R.rel(got[c], s.frames[c].apply(u[c].cpu().numpy())) for c in range(K)) <= bar
    with pytest.raises(ValueError):
        op.multiplier()
    with pytest.raises(ValueError):
        op.multiplier(frame=K)
    op.close()


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,path", [((9,), "dense"), ((12, 10), "dense"), ((32, 40), "fused")])
def test_multipliers_from_points(Ns, path, Z):
    from nufft_pkg import nufft
    T, Zc, bar, _ = TC.dt(Z)
    K, D = 3, len(Ns)
    rng = np.random.default_rng(sum(Ns))
    counts = [150, 0, 97]
    pts = [tuple(_dev((rng.random(n) * 2 * np.pi).astype(T)) for _ in range(D)) for n in counts]
    ws = [_dev((rng.random(counts[0]) + 0.1).astype(T)), None, None]
    opts = {"NUFFT_TOEPLITZ_FUSED": 0} if path == "dense" else {}
    plan = nufft.PlanNUFFT(Zc, Ns, backend=nufft.ROCBackend(0), options=opts, ntransforms=K)
    plan1 = nufft.PlanNUFFT(Zc, Ns, backend=nufft.ROCBackend(0), options=opts)
    op, one = nufft.ToeplitzOperator(plan), nufft.ToeplitzOperator(plan1)
    plan.close()
    plan1.close()
    rest = op.info().workspace_bytes
    op.set_points_frames(pts, ws)
    held = op.info().workspace_bytes
    pad = lambda v: (max(v, 16) + 255) // 256 * 256      # noqa: E731
    assert op.framed and held == rest + K * pad(op.info().multiplier_bytes)       # the K real grids and nothing else stay
    u = tuple(_dev((rng.standard_normal(Ns[::-1]) + 1j * rng.standard_normal(Ns[::-1])).astype(Zc)) for _ in range(K))
    out = op(u)
    worst = 0.0
    for c in (0, 2):
        one.set_points(pts[c], ws[c])
        worst = max(worst, R.rel(op.multiplier(frame=c).cpu().numpy(), one.multiplier().cpu().numpy()))
        worst = max(worst, R.rel(out[c].cpu().numpy(), one(u[c]).cpu().numpy()))
    print(f"frames from points {Z} N={Ns} {path}: multipliers and outputs against set_points per frame {worst:.3e} (bar {bar:g})")
    assert worst <= bar
    assert not op.multiplier(frame=1).cpu().numpy().any() and not out[1].cpu().numpy().any()      # no points: exactly zero
    op.set_points_frames(pts, None, m=6)                                          # a second framed build keeps the storage
    assert op.info().workspace_bytes == held
    with pytest.raises(nufft.DimensionMismatch):
        op.set_points_frames(pts[:2])
    with pytest.raises(nufft.DimensionMismatch):
        op.set_points_frames(pts, ws[:1])
    with pytest.raises(nufft.DimensionMismatch):
        op.set_points_frames(pts, [ws[0], ws[0], None])                           # 150 weights for 0 points
    one.close()
    op.close()


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,path", [((12, 10), "dense"), ((32, 40), "fused")])
def test_back_to_plain_and_round_trips(Ns, path, Z):
    from nufft_pkg import nufft
    Zc = TC.dt(Z)[1]
    K = 2
    s = TC.frames(Ns, K)
    u = _inputs(s, Zc)
    fresh = s.operator(nufft, Z, path, framed=False)
    want_plain = tuple(v.cpu().numpy() for v in fresh(u))
    rest = fresh.info().workspace_bytes
    op = s.operator(nufft, Z, path)
    want_framed = tuple(v.cpu().numpy() for v in op(u))
    # framed -> plain: bit-equal to an operator that never saw frames, and the K grids are gone
    op.set_spectrum(_dev(s.spectra[0].astype(Zc)))
    assert not op.framed and op.info().workspace_bytes == rest
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(op(u), want_plain))
    assert torch.equal(op.multiplier(), fresh.multiplier())
    with pytest.raises(ValueError):
        op.multiplier(frame=0)
    # framed -> coupled -> framed
    c = np.array([[1.0, 0.3], [0.3, 0.8]])
    pairs = [None] * 3
    for a in range(2):
        for b in range(a, 2):
            pairs[S.pair_index(a, b, 2)] = c[a, b] * s.spectra[0]
    op.set_spectra_frames([_dev(t.astype(Zc)) for t in s.spectra])
    assert op.framed and not op.coupled
    op.set_spectra(_dev(np.stack(pairs).astype(Zc)))
    assert op.coupled and not op.framed
    coupled = tuple(v.cpu().numpy() for v in op(u))
    bar = TC.dt(Z)[2]
    g = [s.frames[0].apply(v.cpu().numpy()) for v in u]
    assert max(R.rel(coupled[a], c[a, 0] * g[0] + c[a, 1] * g[1]) for a in range(2)) <= bar
    op.set_spectra_frames([_dev(t.astype(Zc)) for t in s.spectra])
    assert op.framed and not op.coupled
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(op(u), want_framed))
    fresh.close()
    op.close()


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,K,path", [((12, 10), 9, "dense"), ((32, 40), 3, "fused")])
def test_cg_and_the_refused_preconditioner(Ns, K, path, Z):
    from nufft_pkg import nufft
    Zc = TC.dt(Z)[1]
    s = TC.frames(Ns, K)
    op = s.operator(nufft, Z, path)
    b = tuple(_dev(v.astype(Zc)) for v in s.b)
    rtol = 1e-10 if Z == "c128" else 1e-5
    sol = nufft.ToeplitzCG(op, maxiter=400, rtol=rtol)
    x = sol.solve(b)
    torch.cuda.synchronize()
    its, st = sol.iterations, sol.status
    worst = 0.0
    for c in range(K):
        one = _plain(nufft, s, Z, path, c)
        alone = nufft.ToeplitzCG(one, maxiter=400, rtol=rtol)
        xc = alone.solve(b[c])
        torch.cuda.synchronize()
        assert alone.status == (st[c],), c
        worst = max(worst, R.rel(x[c].cpu().numpy(), xc.cpu().numpy()))
        alone.close()
        one.close()
    print(f"CG on {K} frames {Z} N={Ns}: iterations {its}, against single-frame solves {worst:.3e} (bar {SOLVER_BAR[Z]:g})")
    assert worst <= SOLVER_BAR[Z] and set(st) == {"converged"}
    lmax = op.max_eigenvalue()
    assert len(lmax) == K and len(set(lmax)) == K and all(v <= f.lmax for v, f in zip(lmax, s.frames))      # independent components
    sol.close()
    for kw in ({}, {"block": True}):
        with pytest.raises(ValueError, match="framed"):
            nufft.ToeplitzPreconditioner(op, **kw)
    op.set_spectrum(_dev(s.spectra[0].astype(Zc)))
    pc = nufft.ToeplitzPreconditioner(op)
    op.set_spectra_frames([_dev(t.astype(Zc)) for t in s.spectra])
    with pytest.raises(ValueError, match="framed"):
        pc.update()
    pc.close()
    op.close()


# ---- every change of build mode ----------------------------------------------------------------------------------------------------

# plain, coupled, framed: every ordered pair once, a mode after itself included; the steps alternate between points and spectra, which
# gives every mode both entry points
CHAIN = "PPCCFFPFCP"


class _Builds:
    """Seeded inputs of every build of a 3-component operator.  The point sets have at most two points: a sum of two terms does not
    depend on the order of the atomic adds of the spreading, so a build from them is the same to the bit every time."""

    def __init__(self, Ns, T, Zc, padded_shape):
        rng = np.random.default_rng(7 * sum(Ns))
        D = len(Ns)
        cplx = lambda *shape: _dev((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(Zc))      # noqa: E731
        pts = lambda n: tuple(_dev((rng.random(n) * 2 * np.pi).astype(T)) for _ in range(D))                       # noqa: E731
        self.spectrum, self.pairs, self.per_frame = cplx(*padded_shape), cplx(6, *padded_shape), cplx(3, *padded_shape)
        self.points, self.weights, self.basis = pts(2), _dev((rng.random(2) + 0.1).astype(T)), cplx(3, 2)
        self.frame_points, self.frame_weights = [pts(2), pts(1), pts(2)], [_dev((rng.random(2) + 0.1).astype(T)), None, None]
        self.u = tuple(cplx(*Ns[::-1]) for _ in range(3))

    def build(self, op, mode, by_points):
        if mode == "P":
            return op.set_points(self.points, self.weights) if by_points else op.set_spectrum(self.spectrum)
        if mode == "C":
            return op.set_points(self.points, self.weights, basis=self.basis) if by_points else op.set_spectra(self.pairs)
        return op.set_points_frames(self.frame_points, self.frame_weights) if by_points else op.set_spectra_frames(self.per_frame)


def _operator(nufft, Zc, Ns, path, ntransforms=1, segments=None):
    plan = nufft.PlanNUFFT(Zc, Ns, backend=nufft.ROCBackend(0), options={"NUFFT_TOEPLITZ_FUSED": 0} if path == "dense" else {},
                           ntransforms=ntransforms)
    op = nufft.ToeplitzOperator(plan, segments=segments)
    plan.close()
    assert op.path == path
    return op


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,path", [((12, 10), "dense"), ((32, 40), "fused")])
def test_every_change_of_build_mode(Ns, path, Z):
    """After each build of the chain the operator is what a fresh operator is after that build alone: the same bytes held, the same
    bits out of ``apply``, the mode reported."""
    from nufft_pkg import nufft
    T, Zc = TC.dt(Z)[:2]
    op = _operator(nufft, Zc, Ns, path, ntransforms=3)
    b = _Builds(Ns, T, Zc, op.padded_shape)
    for step, mode in enumerate(CHAIN):
        fresh = _operator(nufft, Zc, Ns, path, ntransforms=3)
        for o in (op, fresh):
            b.build(o, mode, by_points=step % 2 == 0)
            assert (o.coupled, o.framed) == (mode == "C", mode == "F"), (step, mode)
        assert op.info().workspace_bytes == fresh.info().workspace_bytes, (step, mode)
        assert all(torch.equal(x, y) for x, y in zip(op(b.u), fresh(b.u))), (step, mode)
        fresh.close()
    op.close()


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,path", [((12, 10), "dense"), ((32, 40), "fused")])
def test_a_refused_build_leaves_the_build_in_force(Ns, path, Z):
    from nufft_pkg import nufft
    T, Zc = TC.dt(Z)[:2]
    op = _operator(nufft, Zc, Ns, path, segments=3)                               # set_spectrum is refused before it touches anything
    b = _Builds(Ns, T, Zc, op.padded_shape)
    op.set_spectra(b.pairs).set_factors(b.u)
    held, want = op.info().workspace_bytes, op(b.u[0]).clone()
    with pytest.raises(ValueError, match="segmented"):
        op.set_spectrum(b.spectrum)
    assert op.info().has_spectrum == 1 and op.info().workspace_bytes == held and torch.equal(op(b.u[0]), want)
    op.close()
