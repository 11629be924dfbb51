"""The locally low-rank proximal map on the GPU against the numpy reference (llr_reference.prox: np.linalg.svd in
float64).  Cases, inputs and thresholds: llr_cases.py.

Bars, with ε = 2⁻⁵² (ComplexF64) / 2⁻²³ (ComplexF32): values rel-L2 <= 64 ε, as in test_gpu_wavelet.py (the Gram route itself measures
2 ... 19 ε₆₄ and 0.2 ε₃₂ against the SVD route on these inputs on the CPU, test_llr_host.py); the nuclear norm 64 ε √n relative.  Every
threshold is the median block singular value, for which the reference zeroes between 0.2 and 0.95 of them (asserted on the reference).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import llr_cases as LC  # noqa: E402
import llr_reference as L  # noqa: E402

TYPES = ["c128", "c64"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(ts):
    torch.cuda.synchronize()
    return np.stack([t.cpu().numpy() for t in ts])


def _straddle(block):
    """A shift whose blocks straddle the periodic boundary in every dimension with more than one cell."""
    return tuple(b // 2 if b > 1 else 0 for b in block)


_REFS = {}


def _reference(Ns, K, block, Z, shift=None):
    """(input in the element type, threshold, float64 result, nuclear norm, zero share), computed once."""
    key = (Ns, K, block, Z, shift)
    if key not in _REFS:
        x = LC.low_rank_input(Ns, K).astype(LC.CTYPE[Z])
        t = LC.median_threshold(x, block, shift)
        _REFS[key] = (x, t) + L.prox(x, block, t, shift)
    return _REFS[key]


def _map(nufft, Ns, K, block, Z, **kw):
    plan = nufft.PlanNUFFT(LC.CTYPE[Z], Ns, backend=nufft.ROCBackend(0), ntransforms=K)
    llr = nufft.LocallyLowRank(plan, block, **kw)
    plan.close()
    return llr


def _tuple(x):
    return tuple(_dev(v) for v in x)


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,K,block", LC.PROX_CASES)
def test_against_the_svd(Ns, K, block, Z):
    from nufft_pkg import nufft
    eps = LC.EPS[Z]
    llr = _map(nufft, Ns, K, block, Z)
    info = llr.info()
    assert tuple(info.block[: len(Ns)]) == block and info.blocks == np.prod([n // b for n, b in zip(Ns, block)]) and info.ntransforms == K
    assert info.jacobi_sweeps_max == L.SWEEPS_MAX and 4 <= info.waves_per_cu <= 32
    for shift in (None, _straddle(block)):
        x, t, want, want_nuc, zero = _reference(Ns, K, block, Z, shift)
        assert 0.2 <= zero <= 0.95, zero
        xd = _tuple(x)
        out, nuc = llr.apply(xd if K > 1 else xd[0], t, shift=shift)
        got = _host(out if K > 1 else (out,))
        nuc = float(nuc.cpu()[0])
        err = LC.rel(got, want)
        print(f"prox {Z} N={Ns} K={K} block={block} shift={shift}: values {err / eps:.1f} ε, nuc {abs(nuc - want_nuc) / want_nuc / eps:.1f} ε, "
              f"zero share {zero:.2f}, {info.waves_per_cu} waves per CU")
        assert np.array_equal(_host(xd), x)                                    # the input is only read
        assert err <= 64 * eps
        assert abs(nuc - want_nuc) <= 64 * eps * np.sqrt(x.size) * want_nuc
        if shift is None:
            zero_shift, nuc0 = llr.apply(xd if K > 1 else xd[0], t, shift=(0,) * len(Ns))
            assert np.array_equal(_host(zero_shift if K > 1 else (zero_shift,)), got) and float(nuc0.cpu()[0]) == nuc
    llr.close()
    with pytest.raises(ValueError, match="closed"):
        llr.apply(xd if K > 1 else xd[0], t)


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,K,block", [LC.PROX_CASES[1], LC.PROX_CASES[3], LC.PROX_CASES[8]])
def test_in_place_repeat_and_graph(Ns, K, block, Z):
    from nufft_pkg import nufft
    shift = _straddle(block)
    x, t, _, _, _ = _reference(Ns, K, block, Z, shift)
    llr = _map(nufft, Ns, K, block, Z)
    xd = _tuple(x)
    out, nuc = llr.apply(xd, t, shift=shift)
    first, first_nuc = _host(out), float(nuc.cpu()[0])
    again, nuc2 = llr.apply(xd, t, shift=shift)                                # two calls: the same bits
    assert np.array_equal(_host(again), first) and float(nuc2.cpu()[0]) == first_nuc
    inplace = _tuple(x)
    same, nuc3 = llr.apply(inplace, t, out=inplace, shift=shift)               # in place
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(same, inplace))
    assert np.array_equal(_host(inplace), first) and float(nuc3.cpu()[0]) == first_nuc
    gout = tuple(torch.zeros_like(v) for v in xd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _, gnuc = llr.apply(xd, t, out=gout, shift=shift)
    for _ in range(2):
        for o in gout:
            o.fill_(7.0)
        gnuc.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_host(gout), first) and float(gnuc.cpu()[0]) == first_nuc
    del graph


@pytest.mark.parametrize("Z", TYPES)
@pytest.mark.parametrize("Ns,K,block", [LC.PROX_CASES[0], LC.PROX_CASES[3], LC.PROX_CASES[8]])
def test_edge_thresholds(Ns, K, block, Z):
    from nufft_pkg import nufft
    eps = LC.EPS[Z]
    x, t, want, _, _ = _reference(Ns, K, block, Z)
    llr = _map(nufft, Ns, K, block, Z)
    zeros = tuple(torch.zeros_like(v) for v in _tuple(x))
    out, nuc = llr.apply(zeros, t)
    assert not _host(out).any() and float(nuc.cpu()[0]) == 0.0                 # an all-zero input: zeros, no NaN
    out, nuc = llr.apply(zeros, 0.0)
    assert not _host(out).any() and float(nuc.cpu()[0]) == 0.0
    out, nuc = llr.apply(_tuple(x), 0.0)
    sv = L.block_singular_values(x, block)
    err = LC.rel(_host(out), x)
    print(f"t = 0 {Z} N={Ns} K={K} block={block}: {err / eps:.1f} ε")
    assert err <= 64 * eps
    if np.prod(block) >= K:      # B < K: H has exact null directions, whose computed eigenvalues are rounding errors of size ε ‖H‖, that is
        assert abs(float(nuc.cpu()[0]) - sv.sum()) <= 64 * eps * np.sqrt(x.size) * sv.sum()      # sqrt(ε) σ_max: only t = 0 keeps them
    out, nuc = llr.apply(_tuple(x), 1.001 * float(sv.max()))
    assert not _host(out).any() and float(nuc.cpu()[0]) == 0.0                 # above the largest singular value: exact zeros
    if Z == "c64":                                                             # a Gram matrix kept in FP32 would overflow
        big = 2.0 ** 70
        out, nuc = llr.apply(_tuple((x * np.float32(big)).astype(np.complex64)), t * big)
        got = _host(out)
        assert np.isfinite(got).all()
        err = LC.rel(got.astype(np.complex128) / big, want)
        print(f"scaled by 2^70 {Z} N={Ns} K={K}: {err / eps:.1f} ε")
        assert err <= 64 * eps


def test_refusals_and_lifetime():
    from nufft_pkg import nufft
    Ns, K = (48, 40), 2
    plan = nufft.PlanNUFFT(np.complex64, Ns, backend=nufft.ROCBackend(0), ntransforms=K)
    for block in ((16, 16), (3, 4), (4, 3), (32, 4), (0, 4), (4,), (4, 4, 4), 2.0):
        with pytest.raises(ValueError):
            nufft.LocallyLowRank(plan, block)
    with pytest.raises(ValueError):
        nufft.LocallyLowRank(plan, 4, seed=-1)
    with pytest.raises(ValueError):
        nufft.LocallyLowRank(nufft.PlanNUFFT(np.float32, Ns, backend=nufft.ROCBackend(0)), 4)      # a real-data plan
    with pytest.raises(ValueError):
        nufft.LocallyLowRank(nufft.PlanNUFFT(np.complex64, Ns, backend=None), 4)                   # a host-only plan
    with pytest.raises(ValueError):
        nufft.LocallyLowRank("plan", 4)
    big = nufft.PlanNUFFT(np.complex64, (64, 64, 64), backend=nufft.ROCBackend(0), ntransforms=16)
    with pytest.raises(ValueError, match="8192"):                                                  # B · K = 1024 · 16
        nufft.LocallyLowRank(big, (16, 8, 8))
    with pytest.raises(ValueError):
        nufft.LocallyLowRank(big, (32, 2, 2))                                                      # side 32, though it divides 64
    nufft.LocallyLowRank(big, (8, 8, 8)).close()                                                   # B · K = 8192 is allowed
    big.close()
    llr = nufft.LocallyLowRank(plan, (4, 8))
    assert "LocallyLowRank" in repr(llr) and llr.block == (4, 8)
    op = nufft.ToeplitzOperator(plan)
    from_op = nufft.LocallyLowRank(op, (4, 8))
    assert from_op.info().blocks == llr.info().blocks == 12 * 5
    plan.close()                                                                                   # the plan is not kept
    n = 48 * 40
    x = tuple(_dev(v) for v in LC.low_rank_input(Ns, K).astype(np.complex64))
    for t in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            llr.apply(x, t)
    for shift in ((4, 0), (0, 8), (-1, 0)):
        with pytest.raises(ValueError):
            llr.apply(x, 0.1, shift=shift)
    with pytest.raises(nufft.DimensionMismatch):
        llr.apply(x, 0.1, shift=(0,))
    with pytest.raises(nufft.DimensionMismatch):
        llr.apply(x[0], 0.1)
    with pytest.raises(ValueError):
        llr.apply(tuple(v.to(torch.complex128) for v in x), 0.1)
    base = torch.zeros(n + 8, dtype=torch.complex64, device="cuda")
    inside = base[:n].view(40, 48)
    with pytest.raises(ValueError, match="overlap"):
        llr.apply((inside, x[1]), 0.1, out=(base[2:n + 2].view(40, 48), torch.empty_like(x[1])))    # a partial overlap
    with pytest.raises(ValueError, match="aligned"):
        llr.apply((base[1:n + 1].view(40, 48), x[1]), 0.1)
    with pytest.raises(ValueError, match="overlap"):
        llr.apply(x, 0.1, out=(x[1], x[0]))                                                        # another component's input
    with pytest.raises(ValueError, match="overlap"):
        o = torch.empty_like(x[0])
        llr.apply(x, 0.1, out=(o, o))
    torch.cuda.synchronize()
    assert not base.any()                                                                          # refused before anything was enqueued
    llr.close()
    llr.close()
    with pytest.raises(ValueError, match="closed"):
        llr.info()
    op.close()
    from_op.apply(x, 0.1)                                                                          # the operator is not kept either
    torch.cuda.synchronize()
