"""numpy restatement of the FISTA solver with an l1-wavelet prior, one system at a time, and its optimality check.

Arrays live in a chosen complex dtype; sums and scalars (change, ‖D W x‖₁, the momentum factor) are float64 for both dtypes, as in the
library.  A coupled operator is run by passing the stacked components as one array together with ``component_axis=0``: the transform
then acts on every component separately, the sums run over all of them.
"""
import numpy as np

import wavelet_reference as W

MAX_ITER, CONVERGED, BREAKDOWN = "max_iter", "converged", "breakdown"


def _per_component(fn, a, component_axis):
    if component_axis is None:
        return fn(a)
    return np.stack([fn(a[c]) for c in range(a.shape[0])])


def fista(apply, b, wavelet, levels, l1, step, lam=0.0, tol=1e-4, max_iter=100, x0=None, dtype=np.complex128, component_axis=None):
    """The algorithm of the header's FISTA section, literally.  ``apply(z)`` returns G z.  Returns a dict: x, iterations, status, change,
    history ([iterations, 2]: change and ‖D W x‖₁), zero_fraction (share of zero detail coefficients in the last iteration run)."""
    real = np.float32 if dtype == np.complex64 else np.float64
    tau, mu = real(step), real(lam)
    thr = float(real(step * l1))
    b = np.asarray(b).astype(dtype)
    x = np.zeros_like(b) if x0 is None else np.asarray(x0).astype(dtype).copy()
    z = x.copy()
    shape = b.shape if component_axis is None else b.shape[1:]
    mask = W.detail_mask(shape, levels)
    t, hist, iters, status, change, zero_fraction = 1.0, [], 0, MAX_ITER, np.nan, np.nan
    for it in range(1, max_iter + 1):
        t_next = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        beta = real((t - 1.0) / t_next)
        t = t_next
        q = np.asarray(apply(z)).astype(dtype)
        v = (z - tau * (q + mu * z - b)).astype(dtype)
        l1sum, zeros, count, cs = 0.0, 0, 0, []
        for comp in (v if component_axis is not None else [v]):
            c, s = W.shrink(comp, wavelet, levels, thr)
            l1sum += s
            zeros += int(np.sum(c[mask] == 0))
            count += int(mask.sum())
            cs.append(W.inverse(c, wavelet, levels))
        xp = (np.stack(cs) if component_axis is not None else cs[0]).astype(dtype)
        d = (xp - x).astype(dtype)
        dd = float(np.sum(np.abs(d.astype(np.complex128)) ** 2))
        xx = float(np.sum(np.abs(xp.astype(np.complex128)) ** 2))
        z = (xp + beta * d).astype(dtype)
        x = xp
        with np.errstate(divide="ignore", invalid="ignore"):
            change = 0.0 if (dd == 0.0 and xx == 0.0) else float(np.sqrt(np.float64(dd) / np.float64(xx)))
        hist.append((change, l1sum))
        iters, zero_fraction = it, zeros / max(count, 1)
        if not np.isfinite(change):
            status = BREAKDOWN
            break
        if change <= tol:
            status = CONVERGED
            break
    return {"x": x, "iterations": iters, "status": status, "change": change, "history": np.array(hist).reshape(-1, 2),
            "zero_fraction": zero_fraction}


def kkt_residual(apply, b, x, wavelet, levels, l1, lam=0.0, zero_tol=0.0):
    """Float64 optimality residual of x for ½<x,(G+μ)x> − Re<b,x> + l1 ‖D W x‖₁, relative to l1 (for l1 = 0: absolute).  With
    g = W((G + μ) x − b) and c = W x: on the detail bands max(|g_i| − l1, 0) where |c_i| <= zero_tol and |g_i + l1 c_i/|c_i|| elsewhere;
    on the approximation band |g_i|.  Returns the largest entry / l1."""
    x = np.asarray(x).astype(np.complex128)
    b = np.asarray(b).astype(np.complex128)
    g = W.forward(np.asarray(apply(x)).astype(np.complex128) + lam * x - b, wavelet, levels)
    c = W.forward(x, wavelet, levels)
    mask = W.detail_mask(x.shape, levels)
    res = np.abs(g)                                         # approximation band: g = 0
    zero = mask & (np.abs(c) <= zero_tol)
    res[zero] = np.maximum(np.abs(g[zero]) - l1, 0.0)
    on = mask & ~zero
    res[on] = np.abs(g[on] + l1 * c[on] / np.abs(c[on]))
    return float(res.max() / (l1 if l1 > 0 else 1.0))
