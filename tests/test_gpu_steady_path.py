"""set_points' steady path on plans of the column-layer sort (nufft_steady_path_used): once the device reports three
point sets in a row that both rings served from their equal-length task tables, the host enqueues the rings' path alone and forces the rings.

The smallest column-layer plan: Float64, m = 4, sigma = 2, Direct(), dims (64, 64, 32) -> 128 x 128 x 64 oversampled (64 columns of 16 x 16 cells,
16 layers of bins), Np = 20 000.  (dims (64, 64, 16) is not eligible: with 8 layers of bins the spreading window runs without its halo variant, and
the plan has no column-layer sort.)  Every result is compared with the oracle at the bound of the neighbouring parity tests (1e-7 for Float64,
test_gpu_parity.py) and with the full-path result of a plan that has the switch off, on the same set, at a relative 1e-12 (not bit-identical:
the LDS atomics of the spreading window reorder)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import nufft_oracle as O  # noqa: E402

DIMS, NP, M = (64, 64, 32), 20000, 4
TOL_ORACLE, TOL_FULL = 1e-7, 1e-12


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def _plan(**options):
    from nufft_pkg import nufft
    plan = nufft.PlanNUFFT(np.float64, DIMS, m=M, sigma=2.0, kernel_evalmode=nufft.Direct(), backend=nufft.ROCBackend(0), options=options or None)
    assert plan.info().sort_column[0] > 0
    return nufft, plan


class _Cases:
    """Point sets by name ("u0", "u1", ...: uniform, seeded; "corner": a quarter of every axis), one value vector and one spectrum — and, computed
    once per set and shared by every test, the oracle's results and those of a plan with the steady path switched off."""

    def __init__(self):
        self.nufft, self.full = _plan(NUFFT_STEADY_PATH=0)
        self.oplan = O.OraclePlan(DIMS, is_real=True, dtype=np.float64, M=M, sigma=2.0, evalmode=O.DIRECT)
        rng = np.random.default_rng(515)
        self.v = rng.standard_normal(NP)
        self.w = rng.standard_normal(self.full.shape) + 1j * rng.standard_normal(self.full.shape)
        self.dev = self.full.device
        self.vd = torch.from_numpy(self.v).to(self.dev)
        self.wd = torch.from_numpy(self.w).to(self.dev)
        self.sets = {}

    def points(self, name):
        if name == "corner":
            return [0.25 * x for x in self.points("u0")]
        rng = np.random.default_rng(9000 + int(name[1:]))
        return [rng.random(NP) * O.TWO_PI for _ in DIMS]

    def get(self, name):
        if name not in self.sets:
            xs = self.points(name)
            xd = tuple(torch.from_numpy(x).to(self.dev) for x in xs)
            O.set_points(self.oplan, xs)
            ref1, ref2 = O.exec_type1(self.oplan, self.v), O.exec_type2(self.oplan, self.w)
            u, out = self.outputs()
            self.nufft.set_points(self.full, xd)
            self.nufft.exec_type1(u, self.full, self.vd)
            self.nufft.exec_type2(out, self.full, self.wd)
            assert not self.full.steady_path_used()
            self.sets[name] = (xd, ref1, ref2, u.cpu().numpy(), out.cpu().numpy())
        return self.sets[name]

    def outputs(self):
        return torch.empty(self.full.shape, dtype=self.full.eltype, device=self.dev), torch.empty(NP, dtype=torch.float64, device=self.dev)

    def run(self, plan, name, outputs=None):
        """set_points + exec_type1 + exec_type2 of set `name` on `plan` (no synchronisation); returns the output tensors"""
        xd = self.get(name)[0]
        u, out = outputs or self.outputs()
        self.nufft.set_points(plan, xd)
        self.nufft.exec_type1(u, plan, self.vd)
        self.nufft.exec_type2(out, plan, self.wd)
        return u, out

    def check(self, name, u, out, what=""):
        _, ref1, ref2, full1, full2 = self.get(name)
        got1, got2 = u.cpu().numpy(), out.cpu().numpy()
        e = (_rel(got1, ref1), _rel(got2, ref2), _rel(got1, full1), _rel(got2, full2))
        print(f"{what}{name}: type 1 / type 2 against the oracle {e[0]:.2e} / {e[1]:.2e}, against the full path {e[2]:.2e} / {e[3]:.2e}")
        assert e[0] < TOL_ORACLE and e[1] < TOL_ORACLE, (what, name, e)
        assert e[2] < TOL_FULL and e[3] < TOL_FULL, (what, name, e)


@pytest.fixture(scope="module")
def cases():
    return _Cases()


def _engines(plan):
    return plan.spread_engine_used(), plan.interp_engine_used(), plan.sort_method_used()


RINGS = ("marching_ring", "marching_ring", "column_layers")


def _to_steady_state(cases, plan, fresh=True):
    """three uniform sets on the full path, the device's record of each seen by the next call: the fourth takes the steady path"""
    for k in range(3):
        cases.run(plan, f"u{k}")
        torch.cuda.synchronize()
        assert not (fresh and plan.steady_path_used()), k
    cases.run(plan, "u3")
    torch.cuda.synchronize()
    assert plan.steady_path_used()


def test_stationary_sets_take_the_steady_path_after_three(cases):
    nufft, plan = _plan()
    for k in range(5):
        u, out = cases.run(plan, f"u{k}")
        torch.cuda.synchronize()
        assert plan.steady_path_used() == (k >= 3), k
        assert _engines(plan) == RINGS, (k, _engines(plan))
        cases.check(f"u{k}", u, out, f"set {k + 1}, steady {plan.steady_path_used()}: ")


def test_distribution_change_is_served_by_the_forced_ring_then_takes_the_full_path(cases):
    nufft, plan = _plan()
    _to_steady_state(cases, plan)
    # a clustered set arrives while the host is on the steady path: the forced rings serve it, correctly
    u, out = cases.run(plan, "corner")
    torch.cuda.synchronize()
    assert plan.steady_path_used()
    assert _engines(plan) == RINGS
    cases.check("corner", u, out, "forced ring: ")
    # the device has reported it: the same set again is on the full path and ends where it does without the steady path
    u, out = cases.run(plan, "corner")
    torch.cuda.synchronize()
    assert not plan.steady_path_used()
    assert plan.sort_method_used() == "fine_bins" and plan.spread_engine_used() == "lds_tiles"
    cases.check("corner", u, out, "full path: ")
    # ... and so is a uniform set behind it: the streak restarts from there
    for k in range(4):
        u, out = cases.run(plan, f"u{k}")
        torch.cuda.synchronize()
        assert plan.steady_path_used() == (k == 3), k
        assert _engines(plan) == RINGS, k
        cases.check(f"u{k}", u, out, f"after the change, set {k + 1}: ")


def test_host_ahead_of_the_device(cases):
    nufft, plan = _plan()
    names = ["u0", "u1", "u2", "u3", "corner", "u4"]
    results = [cases.run(plan, name) for name in names]      # no synchronisation: whichever path each call took
    torch.cuda.synchronize()
    for name, (u, out) in zip(names, results):
        cases.check(name, u, out, "unsynchronised: ")
    # (and once more from whatever state that left, records arriving in between)
    results = []
    for name in names:
        results.append(cases.run(plan, name))
        torch.cuda.current_stream().synchronize()
    for name, (u, out) in zip(names, results):
        cases.check(name, u, out, "synchronised: ")


def test_a_captured_call_takes_the_full_path_and_bars_the_steady_path(cases):
    nufft, plan = _plan()
    _to_steady_state(cases, plan)
    xd = tuple(x.clone() for x in cases.get("u0")[0])
    u, _ = cases.outputs()

    def step():
        nufft.set_points(plan, xd)
        nufft.exec_type1(u, plan, cases.vd)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    assert not plan.steady_path_used()
    for name in ("u1", "corner", "u2"):
        for d in range(3):
            xd[d].copy_(cases.get(name)[0][d])
        u.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _, ref1, _, full1, _ = cases.get(name)
        got = u.cpu().numpy()
        assert _rel(got, ref1) < TOL_ORACLE and _rel(got, full1) < TOL_FULL, name
    for k in range(5):
        u2, out2 = cases.run(plan, f"u{k}")
        torch.cuda.synchronize()
        assert not plan.steady_path_used(), k
        cases.check(f"u{k}", u2, out2, "eager after a capture: ")


def test_exec_captured_on_a_steady_point_set_replays_behind_a_later_full_path_set(cases):
    """An exec captured while the point set has no tile tables carries every launch, gated on the device flags: replayed behind a later
    set_points (always the full path from then on) that hands its set to the tile kernels, it still transforms correctly."""
    nufft, plan = _plan()
    _to_steady_state(cases, plan)
    u, _ = cases.outputs()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nufft.exec_type1(u, plan, cases.vd)
    for name in ("u3", "corner", "u1"):
        if name != "u3":
            nufft.set_points(plan, cases.get(name)[0])
            assert not plan.steady_path_used()
        u.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _, ref1, _, full1, _ = cases.get(name)
        got = u.cpu().numpy()
        assert _rel(got, ref1) < TOL_ORACLE and _rel(got, full1) < TOL_FULL, name


def test_switch_off(cases):
    nufft, plan = _plan(NUFFT_STEADY_PATH=0)
    assert "NUFFT_STEADY_PATH=0" in plan.options
    for k in range(6):
        u, out = cases.run(plan, f"u{k % 5}")
        torch.cuda.synchronize()
        assert not plan.steady_path_used(), k
        assert _engines(plan) == RINGS, k
    cases.check(f"u{5 % 5}", u, out, "switch off: ")


def test_empty_and_shrinking_sets(cases):
    nufft, plan = _plan()
    _to_steady_state(cases, plan)
    empty = tuple(torch.empty(0, dtype=torch.float64, device=cases.dev) for _ in DIMS)
    nufft.set_points(plan, empty)
    torch.cuda.synchronize()
    assert not plan.steady_path_used()
    u, out = cases.run(plan, "u4")
    torch.cuda.synchronize()
    cases.check("u4", u, out, "behind an empty set: ")
    # a smaller set on the steady path (the buffers of the larger one stay)
    _to_steady_state(cases, plan, fresh=False)
    n = 17001
    xs = [x[:n].contiguous() for x in cases.get("u2")[0]]
    oplan = cases.oplan
    O.set_points(oplan, [x.cpu().numpy() for x in xs])
    ref1 = O.exec_type1(oplan, cases.v[:n])
    nufft.set_points(plan, tuple(xs))
    assert plan.steady_path_used()
    u, _ = cases.outputs()
    nufft.exec_type1(u, plan, cases.vd[:n].contiguous())
    torch.cuda.synchronize()
    assert _rel(u.cpu().numpy(), ref1) < TOL_ORACLE
