"""Numpy restatement of the sample-density compensation iteration (Pipe & Menon), the definition the GPU is tested against
(include/nufft_mi355x.h, density compensation section).

C is interpolation after spreading on the fine grid of a REAL-data oracle plan: (C w)_j = O.interpolate of the grid O.spread of w leaves,
no FFT and no deconvolution in between.

    w = 1 (or the caller's positive w0)
    for k = 0 ... max_iter − 1:
        v = C w
        δ_k = max_j |v_j − 1|          reported for k >= 1, and for k = 0 with a caller's w0
        stop if some v_j is not positive and finite (BREAKDOWN), or if k >= 1 and δ_k <= tol (CONVERGED): w stays
        w = w / v
    finish: w / Σ w ("sum") or w ("none"); not after a breakdown

The all-ones start stands for every constant start: w / (C w) does not depend on the scale of w.
"""
import numpy as np

from oracle import nufft_oracle as O

MAX_ITER, CONVERGED, BREAKDOWN = 0, 1, 2


def make_plan(Ns, dtype=np.float64, M=4, sigma=2.0, kernel=O.KERNEL_BKB, evalmode=O.DIRECT, point_transform=O.POINT_TRANSFORM_IDENTITY,
              kernel_param=None, coord_dtype=None):
    """The real-data plan of the iteration: precision, N, σ, half support, kernel, evaluation mode and point convention of the parent."""
    return O.OraclePlan(tuple(Ns), is_real=True, dtype=dtype, M=M, sigma=sigma, evalmode=evalmode, kernel=kernel,
                        kernel_param=kernel_param, point_transform=point_transform, coord_dtype=coord_dtype)


def apply_C(plan, w):
    """(C w)_j in the plan's precision."""
    return O.interpolate(plan, O.spread(plan, [np.asarray(w).astype(plan.dtype)]))[0]


def _positive_finite(a):
    return bool(np.all(np.isfinite(a) & (a > 0)))


def pipe_menon(plan, points, max_iter=20, tol=0.0, w0=None, normalize="sum"):
    """Returns dict(w, iterations, status, residual, history[max_iter]); `points` in the plan's coordinate precision."""
    O.set_points(plan, [np.ascontiguousarray(x) for x in points])
    Np = len(points[0])
    T = np.dtype(plan.dtype).type
    history = np.full(max_iter, np.nan)
    out = dict(iterations=0, status=MAX_ITER, residual=np.nan, history=history)
    w = np.ones(Np, dtype=T) if w0 is None else np.array(w0, dtype=T)
    if Np == 0 or not _positive_finite(w):
        out.update(w=w, status=MAX_ITER if Np == 0 else BREAKDOWN)
        return out
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for k in range(max_iter):
            v = apply_C(plan, w)
            if not _positive_finite(v):
                out["status"] = BREAKDOWN
                break
            delta = float(np.max(np.abs(v.astype(np.float64) - 1.0)))
            if k >= 1 or w0 is not None:
                history[k] = delta
                out["residual"] = delta
            if k >= 1 and delta <= tol:
                out["status"] = CONVERGED
                break
            w = (w / v).astype(T)
            out["iterations"] = k + 1
    if out["status"] != BREAKDOWN and normalize == "sum":
        w = (w / T(w.astype(np.float64).sum())).astype(T)
    elif normalize not in ("sum", "none"):
        raise ValueError('normalize must be "sum" or "none"')
    out["w"] = w
    return out
