"""Numpy restatement of the type-2 gradient gather (a plain helper of tests/test_gradient_host.py and tests/test_gpu_gradient.py).

``window_derivatives`` returns, next to the oracle's window values, their derivatives with respect to the cell fraction X of a
point (grid node i − M + 1 + j, window argument y = (M − 1 − j + X) / M); ``interpolate_grad`` gathers them from the oracle's
type-2 grids exactly as ``oracle.interpolate`` gathers the values, and converts to the caller's coordinates.
"""
import math

import numpy as np
from scipy.special import i1

from oracle import nufft_oracle as O


def _bkb_dratio(t):
    """(t cosh t − sinh t) / t³: the Taylor series Σ 2n / (2n+1)! t^(2n−2) below 1, the closed form above."""
    t = np.asarray(t, dtype=np.float64)
    z = t * t
    series = np.zeros_like(t)
    for n in range(10, 0, -1):
        series = series * z + 2.0 * n / math.factorial(2 * n + 1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        closed = (t * np.cosh(t) - np.sinh(t)) / (t * t * t)
    return np.where(t < 1.0, series, closed)


def window_derivatives(plan, d, x):
    """(cell index, values (Np, 2M), dφ/dX (Np, 2M)) along dimension d for folded coordinates x, in Float64."""
    x = np.asarray(x)
    i, vals = O.evaluate_window(plan, d, x)
    M = plan.M
    N = plan.Nover[d]
    _, r = O.point_to_cell(x, N)
    X = (r - np.minimum(i, N - 1).astype(r.dtype)).astype(np.float64)
    j = np.arange(2 * M, dtype=np.float64)[None, :]
    u = (M - 1 - j + X[:, None])                          # distance from the node in cells
    y = u / M
    vals = vals.astype(np.float64)
    if plan.kernel == O.KERNEL_BSPLINE:
        b = O.bspline_evaluate_all(1.0 - X, 2 * M - 1)    # order 2M − 1, the same recursion stopped one order earlier
        lo = np.concatenate([np.zeros((len(X), 1)), b], axis=1)
        hi = np.concatenate([b, np.zeros((len(X), 1))], axis=1)
        return i, vals, lo - hi
    if plan.kernel == O.KERNEL_GAUSSIAN:
        dx = O.TWO_PI / N
        tau = plan.taus[d]
        return i, vals, (-2.0 * (u * dx) * dx / tau) * vals
    if plan.evalmode != O.DIRECT:                           # piecewise polynomial of both Kaiser-Bessel kernels
        cs = plan.coefs[d].astype(np.float64)
        xx = (2.0 * X - 1.0)[:, None]
        p = np.broadcast_to(cs[-1][None, :], (len(X), 2 * M)).astype(np.float64)
        dp = np.zeros_like(p)
        for k in range(cs.shape[0] - 2, -1, -1):
            dp = xx * dp + p
            p = xx * p + cs[k][None, :]
        return i, vals, 2.0 * dp
    beta = plan.betas[d]
    s = np.sqrt(np.maximum(1.0 - y * y, 0.0))
    t = beta * s
    if plan.kernel == O.KERNEL_KB:
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(t > 0, i1(t) / np.where(t > 0, t, 1.0), 0.5)
        return i, vals, -(beta * beta * y) * ratio / M
    return i, vals, -(beta / math.pi) * beta * beta * y * _bkb_dratio(t) / M


def interpolate_grad(plan, grids):
    """For each component grid: (values, [∂_d v for d < D]) at plan.points, derivatives with respect to the caller's
    coordinates (the NFFT convention's internal point is −2π x, folded)."""
    D = plan.ndim
    M = plan.M
    L = 2 * M
    inds, vals, ders = [], [], []
    for d in range(D):
        x = plan.points[d]
        if plan.point_transform == O.POINT_TRANSFORM_NFFT:
            x = O.nfft_point_convention(x)
        x = O.to_unit_cell(x)
        i, v, dv = window_derivatives(plan, d, x)
        i = np.minimum(i, plan.Nover[d] - 1)
        inds.append((i[:, None] - M + 1 + np.arange(L)[None, :]) % plan.Nover[d])
        h = O.TWO_PI / plan.Nover[d]
        vals.append(v * h)
        ders.append(dv * h)
    chain = [plan.Nover[d] / O.TWO_PI * (-O.TWO_PI if plan.point_transform == O.POINT_TRANSFORM_NFFT else 1.0) for d in range(D)]

    def weights(dsel):
        w = ders[0] if dsel == 0 else vals[0]
        for d in range(1, D):
            wd = ders[d] if dsel == d else vals[d]
            w = w[:, None, ...] * wd.reshape((-1, L) + (1,) * d)
        return w.reshape(w.shape[0], -1)

    lin = inds[0]
    stride = plan.Nover[0]
    for d in range(1, D):
        lin = lin[:, None, ...] + stride * inds[d].reshape((-1, L) + (1,) * d)
        stride *= plan.Nover[d]
    lin = lin.reshape(lin.shape[0], -1)
    ws = [weights(-1)] + [weights(d) for d in range(D)]
    out = []
    for u in grids:
        g = np.asarray(u).reshape(-1)[lin]
        g = g.astype(np.complex128) if np.iscomplexobj(g) else g.astype(np.float64)
        v = (g * ws[0]).sum(axis=1)
        out.append((v, [(g * ws[1 + d]).sum(axis=1) * chain[d] for d in range(D)]))
    return out


def exact_type2_grad(plan, xp, uhat):
    """Σ i k_d û_k e^{i k·x} (complex plans) or its real part with the Hermitian weights (real plans): (values, [∂_d])."""
    D = plan.ndim
    uh = np.asarray(uhat).astype(np.complex128)
    if plan.is_real:
        uh = uh * O.hermitian_weights(plan)
    val = O.nudft_type2(plan.ks, xp, uh)
    grads = []
    for d in range(D):
        k = np.asarray(plan.ks[d], dtype=np.float64)
        shape = [1] * D
        shape[D - 1 - d] = len(k)                          # reversed axes: dimension 1 is the last tensor axis
        grads.append(O.nudft_type2(plan.ks, xp, uh * (1j * k).reshape(shape)))
    if plan.is_real:
        return val.real, [g.real for g in grads]
    return val, grads
