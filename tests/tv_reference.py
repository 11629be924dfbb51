"""numpy restatement of the primal-dual solver with a total-variation prior, one system at a time, and its optimality
check.

Arrays live in a chosen complex dtype; sums and scalars (change, Σ|∇x|₂) are float64 for both dtypes, as in the library.  Dimension 1
is the fastest one, the LAST axis of an array.  A coupled operator is run by passing the stacked components as one array together with
``component_axis=0``: the differences then act on every component separately, the sums run over all of them.
"""
import numpy as np

MAX_ITER, CONVERGED, BREAKDOWN = "max_iter", "converged", "breakdown"


def _real(dtype):
    return np.float32 if np.dtype(dtype) == np.complex64 else np.float64


def gradient(x, component_axis=None):
    """(∇x)_d[i] = x[i + e_d] − x[i], indices mod N_d: an array [D, ...] in the dtype of x, dimension 1 (the last axis) first."""
    D = x.ndim - (0 if component_axis is None else 1)
    return np.stack([np.roll(x, -1, axis=x.ndim - 1 - d) - x for d in range(D)])


def adjoint(y, component_axis=None):
    """(∇ᴴy)[i] = Σ_d (y_d[i − e_d] − y_d[i]), summed in the order d = 1 ... D in the dtype of y."""
    out = None
    for d in range(y.shape[0]):
        t = np.roll(y[d], 1, axis=y.ndim - 2 - d) - y[d]
        out = t if out is None else out + t
    return out


def cell_norms(g):
    """|(∇x)_i|₂ in float64 from the differences [D, ...]."""
    g = g.astype(np.complex128)
    return np.sqrt(np.sum(g.real ** 2 + g.imag ** 2, axis=0))


def norm(x, component_axis=None):
    """Σ_i |(∇x)_i|₂: differences in the dtype of x, squares, root and sum in float64."""
    return float(cell_norms(gradient(x, component_axis)).sum())


def tvpd(apply, b, tv, step, sigma=None, lam=0.0, tol=1e-4, max_iter=100, x0=None, dtype=np.complex128, component_axis=None):
    """The algorithm of the header's primal-dual section, literally.  ``apply(x)`` returns G x.  ``tv``: a scalar, or with
    ``component_axis`` one weight per component.  Returns a dict: x, y ([D, ...]), iterations, status, change, history ([iterations, 2]:
    change and Σ|∇x⁺|₂), clipped ([iterations]: share of cells whose dual vector the projection shortened)."""
    real = _real(dtype)
    b = np.asarray(b).astype(dtype)
    D = b.ndim - (0 if component_axis is None else 1)
    tau, mu = real(step), real(lam)
    sig = real(1.0 / (8.0 * D * step) if sigma is None else sigma)
    t = np.asarray(tv, dtype=np.float64).astype(real)
    if component_axis is not None:
        t = np.broadcast_to(t, (b.shape[0],)).reshape((b.shape[0],) + (1,) * D)
    x = np.zeros_like(b) if x0 is None else np.asarray(x0).astype(dtype).copy()
    y = np.zeros((D,) + b.shape, dtype=dtype)
    hist, clipped, iters, status, change = [], [], 0, MAX_ITER, np.nan
    for it in range(1, max_iter + 1):
        with np.errstate(all="ignore"):
            q = np.asarray(apply(x)).astype(dtype)
            xp = (x - tau * (q + mu * x - b + adjoint(y, component_axis))).astype(dtype)
            d = (xp - x).astype(dtype)
            xbar = (xp + d).astype(dtype)
            v = (y + sig * gradient(xbar, component_axis)).astype(dtype)
            nrm = np.sqrt(np.sum(v.real ** 2 + v.imag ** 2, axis=0, dtype=real)).astype(real)
            clip = nrm > t
            scale = np.where(clip, t / np.where(clip, nrm, real(1)), real(1)).astype(real)
            y = (v * scale).astype(dtype)
            dd = float(np.sum(np.abs(d.astype(np.complex128)) ** 2))
            xx = float(np.sum(np.abs(xp.astype(np.complex128)) ** 2))
            tvsum = norm(xp, component_axis)
            x = xp
            change = 0.0 if (dd == 0.0 and xx == 0.0) else float(np.sqrt(np.float64(dd) / np.float64(xx)))
        hist.append((change, tvsum))
        clipped.append(float(np.mean(clip)))
        iters = it
        if not np.isfinite(change):
            status = BREAKDOWN
            break
        if change <= tol:
            status = CONVERGED
            break
    return {"x": x, "y": y, "iterations": iters, "status": status, "change": change, "history": np.array(hist).reshape(-1, 2),
            "clipped": np.array(clipped)}


def optimality(apply, b, x, y, tv, lam=0.0, component_axis=None):
    """Float64 optimality of the pair (x, y) for ½<x,(G+μ)x> − Re<b,x> + tv Σ|∇x|₂ (tv > 0, a scalar):
        r = max|(G + μ) x − b + ∇ᴴy| / max|b|                       stationarity in x
        e = max(max_i |y_i|₂ / tv − 1, 0)                           y inside the dual ball
        g = (tv Σ|∇x|₂ − Re<y, ∇x>) / (tv Σ|∇x|₂)                   y attains the norm of ∇x
    """
    x = np.asarray(x).astype(np.complex128)
    y = np.asarray(y).astype(np.complex128)
    b = np.asarray(b).astype(np.complex128)
    r = float(np.abs(np.asarray(apply(x)).astype(np.complex128) + lam * x - b + adjoint(y, component_axis)).max() / np.abs(b).max())
    e = float(max(cell_norms(y).max() / tv - 1.0, 0.0))
    gx = gradient(x, component_axis)
    total = tv * float(cell_norms(gx).sum())
    g = float((total - np.real(np.vdot(y, gx))) / total)
    return r, e, g

