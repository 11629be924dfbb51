"""Point sets shared by tests/test_gpu_boundary.py and tests/test_boundary_cases_host.py: points ON the edges that the engines and
sorts cut the grid by, coincident points, point sets confined to a plane / layer / column / line, and very small point sets.  Pure
numpy, seeded, no GPU import.

Every other parity test draws its points from continuous distributions: no point lies on a cell, bin, column or period boundary, no
two points coincide, and Np is in the thousands.  Here every coordinate is finite and within +-1e3 * 2 pi (NaN, Inf and huge
coordinates have no defined behaviour in the library or the oracle and are not tested).

`geom` (see `geometry`) names, per dimension, the distances in cells between the edges a plan cuts its oversampled grid by: sort bins,
columns of the rings, columns of the column-layer sort (4 cells per bin), tiles, and the height of a layer of bins.

Families, in the order `point_sets` returns them (L = T(2 pi)):

  faces              Np = 600  every coordinate drawn independently from FACE_VALUES: 0, -0.0, prevfloat(L), L, -L, prevfloat(pi), pi,
                               -1e-30 (a normal number in both precisions; L + r rounds to L: the clamp of cell_of, cell N - 1 with
                               offset X = 1), 3 L + 0.1, -7.3
  nodes              Np = 600  per dimension x = L i / N_d for 200 node indices i: 0, N_d - 1, multiples of every entry of `geom`
                               (first and last multiple always), random ones; each value as computed, one step of the number format
                               below it and one above it.  Around x = 0 the two steps are +-(smallest normal number), not subnormal
                               ones: what a subnormal coordinate does is part of the undecided "hostile coordinates" contract.
  coincident_mid     Np = 512  all points at one interior location
  coincident_origin  Np = 512  all points at (0, 0, 0): the stencil wraps in every dimension
  coincident_last    Np = 512  all points at prevfloat(L) in every dimension
  plane_x            Np = 800  dimension 1 constant, the others uniform
  layer_z            Np = 800  dimension 3 constant
  column             Np = 800  dimensions 1 and 2 constant
  line_x             Np = 800  dimensions 2 and 3 constant
  tiny_0 .. tiny_65  uniform sets of 0, 1, 2, 63, 64, 65 points (either side of a wave)

For 1-D and 2-D plans the confined families are restricted to the existing dimensions; one that would confine nothing, or every
dimension (a coincident set again), is left out.
"""
import numpy as np

TWO_PI = 2.0 * np.pi

N_FACES, N_NODES, N_COINCIDENT, N_CONFINED = 600, 600, 512, 800
TINY = (0, 1, 2, 63, 64, 65)
N_UNIFORM = 20000           # the large set of the stale-table sequence (uniform, tiny_1, tiny_0, uniform)

# constant dimensions (0-based) of the confined families
CONFINED = {"plane_x": (0,), "layer_z": (2,), "column": (0, 1), "line_x": (1, 2)}
ORDER = (["faces", "nodes", "coincident_mid", "coincident_origin", "coincident_last"] + list(CONFINED) + [f"tiny_{n}" for n in TINY])
# sets made only of boundary points, and the coincident sets: the outputs are also checked for finiteness
BOUNDARY_ONLY = ("faces", "nodes", "coincident_mid", "coincident_origin", "coincident_last")
COINCIDENT = ("coincident_mid", "coincident_origin", "coincident_last")


def real_dtype(Z):
    return np.dtype(np.float32) if np.dtype(Z) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.dtype(np.float64)


def geometry(info, D):
    """The edges of a plan from `plan.info()` (host-only plans answer the same): per name a list of D distances in cells, 0 = no such
    edge along that dimension."""
    def pad(v):
        return [int(x) for x in v] + [0] * (D - len(v))
    g = {"bin_dims": pad([info.bin_dims[d] for d in range(D)]),
         "spread_tile": pad([info.spread_tile[d] for d in range(D)]),
         "interp_tile": pad([info.interp_tile[d] for d in range(D)]),
         "ring_column": pad([info.ring_column[d] for d in range(min(D, 2))]),
         "sort_column": pad([4 * info.sort_column[d] for d in range(min(D, 2))]),
         "bin_layer": [0] * (D - 1) + [int(info.bin_dims[D - 1])]}
    return {k: v[:D] for k, v in g.items()}


def edge_strides(geom, d, N):
    """Distinct distances between edges along dimension d that leave at least one edge inside an axis of N cells: {name: cells}."""
    out = {}
    for name, v in geom.items():
        s = int(v[d])
        if 0 < s < N:
            out[name] = s
    return out


def face_values(T):
    T = np.dtype(T).type
    L = T(TWO_PI)
    return np.array([T(0.0), T(-0.0), np.nextafter(L, T(0)), L, -L, np.nextafter(T(np.pi), T(0)), T(np.pi), T(-1e-30),
                     T(3) * L + T(0.1), T(-7.3)], dtype=T)


def _node_indices(N, strides, rng, count):
    idx = [0, N - 1]
    for s in sorted(set(strides)):
        mult = np.arange(s, N, s)
        if len(mult) > 8:
            mult = np.concatenate(([mult[0], mult[-1]], rng.choice(mult[1:-1], 6, replace=False)))
        idx += [int(m) for m in mult]
    idx = idx[:count]
    idx += [int(i) for i in rng.integers(0, N, count - len(idx))]
    return np.array(idx, dtype=np.int64)


def _nodes(T, Nover, geom, rng):
    """(coordinates, node index, nudge) per dimension: nudge -1 / 0 / +1 = one step below the node / as computed / one step above."""
    T = np.dtype(T).type
    L = T(TWO_PI)
    tiny = np.finfo(T).tiny
    xs, nodes, nudges = [], [], []
    for d, N in enumerate(Nover):
        i = _node_indices(N, edge_strides(geom, d, N).values(), rng, N_NODES // 3)
        x = ((L * i.astype(T)) / T(N)).astype(T)
        down = np.where(x == 0, -tiny, np.nextafter(x, T(-np.inf))).astype(T)
        up = np.where(x == 0, tiny, np.nextafter(x, T(np.inf))).astype(T)
        perm = rng.permutation(N_NODES)                      # independent per dimension: every combination of edge / interior
        xs.append(np.concatenate((x, down, up))[perm])
        nodes.append(np.concatenate((i, i, i))[perm])
        nudges.append(np.repeat(np.array([0, -1, 1]), len(i))[perm])
    return xs, nodes, nudges


def node_nudges(T, Nover, geom, seed):
    """(node index, nudge) per dimension of the `nodes` set of `point_sets(T, Nover, geom, seed)`."""
    rng = _family_rng(seed, "nodes")
    _, nodes, nudges = _nodes(T, Nover, geom, rng)
    return nodes, nudges


def _family_rng(seed, name):
    return np.random.default_rng([int(seed), ORDER.index(name)])


def uniform(T, D, Np, rng):
    """Points outside the unit cell too, as tests/test_gpu_parity.py::_make_case draws them."""
    return [((rng.random(Np) * 3 - 1) * TWO_PI).astype(T) for _ in range(D)]


def uniform_set(T, D, seed, Np=N_UNIFORM):
    return uniform(T, D, Np, np.random.default_rng([int(seed), 1000]))


def point_sets(T, Nover, geom, seed):
    """{name: list of D coordinate vectors of dtype T}, in the order of ORDER.  Every family has its own generator: a set does not
    depend on which others are drawn."""
    T = np.dtype(T).type
    D = len(Nover)
    L = T(TWO_PI)
    out = {}
    for name in ORDER:
        rng = _family_rng(seed, name)
        if name == "faces":
            fv = face_values(T)
            out[name] = [fv[rng.integers(0, len(fv), N_FACES)] for _ in range(D)]
        elif name == "nodes":
            out[name] = _nodes(T, Nover, geom, rng)[0]
        elif name in COINCIDENT:
            at = {"coincident_mid": [T(2.0 + 0.37 * d) for d in range(D)], "coincident_origin": [T(0.0)] * D,
                  "coincident_last": [np.nextafter(L, T(0))] * D}[name]
            out[name] = [np.full(N_COINCIDENT, at[d], dtype=T) for d in range(D)]
        elif name in CONFINED:
            const = [d for d in CONFINED[name] if d < D]
            if not const or len(const) == D:
                continue
            xs = uniform(T, D, N_CONFINED, rng)
            for d in const:
                xs[d] = np.full(N_CONFINED, xs[d][0], dtype=T)
            out[name] = xs
        else:
            out[name] = uniform(T, D, int(name.split("_")[1]), rng)
    for name, xs in out.items():
        for x in xs:
            assert x.dtype == np.dtype(T) and np.all(np.isfinite(x)) and np.all(np.abs(x) <= 1e3 * TWO_PI), name
    return out


def values(Z, Np, seed):
    """1 + 0.5 randn (+ i (1 + 0.5 randn) for complex data): the mean of 1 keeps the type-1 result of a coincident set away from a
    cancelling sum."""
    rng = np.random.default_rng([int(seed), 2000])
    v = 1.0 + 0.5 * rng.standard_normal(Np)
    if np.dtype(Z).kind == "c":
        v = v + 1j * (1.0 + 0.5 * rng.standard_normal(Np))
    return v.astype(Z)


FEW_LOCATIONS = COINCIDENT + ("tiny_1", "tiny_2")      # sets whose type-2 result is one or two numbers


def spectrum(Z, shape, seed, exact=None, sets=None):
    """randn + i randn in the plan's complex type (tensor shape = reversed size(plan)), as elsewhere in the suite.

    With `exact(xs, w)` (the exact type-2 sums at points xs, Float64) and the point sets: the first draw for which no set of
    FEW_LOCATIONS has a cancelling sum.  The suite's bounds are relative 2-norms over thousands of points, each a sum of random terms:
    an error of eps x (root mean square of the values) per point gives a relative error of eps.  The type-2 result of a coincident
    set is ONE such sum; where it happens to be a small fraction f of the root mean square, the same absolute error reads eps / f,
    and a comparison at the suite's bound would measure the draw, not the kernel (type 1 has the mean of 1 in `values` for the same
    reason).  Draws with f < 1 / 4 at any of those sets are passed over (a quarter of all draws for real data), decided from the
    exact sums alone: at most a factor of 4 between these sets and the many-point ones."""
    ctype = np.complex64 if real_dtype(Z) == np.float32 else np.complex128
    D = len(shape)
    probe = uniform(np.float64, D, 32, np.random.default_rng([int(seed), 3001]))
    for attempt in range(400):
        rng = np.random.default_rng([int(seed), 3000, attempt])
        w = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(ctype)
        if exact is None:
            return w
        rms = np.sqrt(np.mean(np.abs(exact(probe, w)) ** 2))
        few = [[x[:2].astype(np.float64) for x in sets[name]] for name in FEW_LOCATIONS]
        if all(np.sqrt(np.mean(np.abs(exact(xs, w)) ** 2)) >= 0.25 * rms for xs in few):
            return w
    raise AssertionError("no well-conditioned spectrum in 400 draws")


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))
