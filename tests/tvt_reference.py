"""numpy restatement of the primal-dual solver with a spatial and a temporal total-variation term, and its optimality
check.

The frames are axis 0 of every array ([K, ...], dimension 1 the LAST axis).  Arrays live in a chosen complex dtype; sums and scalars are
float64 for both dtypes, as in the library.  The spatial differences are those of tv_reference.py, acting on every frame separately.
"""
import numpy as np

import tv_reference as T

MAX_ITER, CONVERGED, BREAKDOWN = T.MAX_ITER, T.CONVERGED, T.BREAKDOWN


def gradient_t(x, periodic=False):
    """(∇_t x)_c = x_{c+1} − x_c for c < K − 1; the last one x_0 − x_{K−1} if periodic, else 0."""
    g = np.roll(x, -1, axis=0) - x
    if not periodic:
        g[-1] = 0
    return g


def adjoint_t(z, periodic=False):
    """(∇_tᴴ z)_c = z_{c−1} − z_c with z_{−1} = z_{K−1} if periodic, else z_{−1} = z_{K−1} = 0."""
    if not periodic:
        z = z.copy()
        z[-1] = 0
    return np.roll(z, 1, axis=0) - z


def frame_norms_t(x, periodic=False):
    """Σ_i |(∇_t x)_c[i]| per frame: differences in the dtype of x, modulus and sum in float64."""
    g = gradient_t(x, periodic).astype(np.complex128)
    return np.sqrt(g.real ** 2 + g.imag ** 2).reshape(x.shape[0], -1).sum(axis=1)


def frame_norms_s(x):
    """Σ_i |(∇x_c)_i|₂ per frame."""
    return T.cell_norms(T.gradient(x, component_axis=0)).reshape(x.shape[0], -1).sum(axis=1)


def tvpd_t(apply, b, tv, tv_t, step, periodic=False, spatial=None, sigma=None, lam=0.0, tol=1e-4, max_iter=100, x0=None, dtype=np.complex128):
    """The iteration of the header's temporal section, literally.  ``apply(x)`` returns G x for the stacked frames [K, ...].  ``tv``: a
    scalar or one spatial weight per frame; ``spatial``: None = on iff any tv > 0.  Returns a dict: x, y ([D, K, ...] or None), z, iterations,
    status, change, history ([iterations, K, 2]: the joint change and each frame's share of the prior), clipped_t / clipped_s
    ([iterations]: share of the live dual cells the projection shortened)."""
    real = T._real(dtype)
    b = np.asarray(b).astype(dtype)
    K, D = b.shape[0], b.ndim - 1
    tw = np.broadcast_to(np.asarray(tv, dtype=np.float64), (K,))
    if spatial is None:
        spatial = bool((tw > 0).any())
    tau, mu = real(step), real(lam)
    sig = real(1.0 / (8.0 * ((D + 1) if spatial else 1) * step) if sigma is None else sigma)
    t = tw.astype(real).reshape((K,) + (1,) * D)
    tt = real(tv_t)
    x = np.zeros_like(b) if x0 is None else np.asarray(x0).astype(dtype).copy()
    y = np.zeros((D,) + b.shape, dtype=dtype) if spatial else None
    z = np.zeros_like(b)
    live = K if periodic else K - 1                      # frames whose temporal difference exists
    hist, clipped_t, clipped_s, iters, status, change = [], [], [], 0, MAX_ITER, np.nan
    for it in range(1, max_iter + 1):
        with np.errstate(all="ignore"):
            q = np.asarray(apply(x)).astype(dtype)
            if spatial:
                # (q + ∇_tᴴz) first: the library adds the temporal term to q and hands the sum to the spatial kernel
                xp = (x - tau * ((q + adjoint_t(z, periodic)).astype(dtype) + mu * x - b + T.adjoint(y, 0))).astype(dtype)
            else:
                xp = (x - tau * (q + mu * x - b + adjoint_t(z, periodic))).astype(dtype)
            d = (xp - x).astype(dtype)
            xbar = (xp + d).astype(dtype)
            if spatial:
                v = (y + sig * T.gradient(xbar, 0)).astype(dtype)
                nrm = np.sqrt(np.sum(v.real ** 2 + v.imag ** 2, axis=0, dtype=real)).astype(real)
                clip = nrm > t
                y = (v * np.where(clip, t / np.where(clip, nrm, real(1)), real(1)).astype(real)).astype(dtype)
                clipped_s.append(float(np.mean(clip)))
            w = (z + sig * gradient_t(xbar, periodic)).astype(dtype)
            nrm = np.sqrt(w.real ** 2 + w.imag ** 2).astype(real)
            clip_t = nrm > tt
            z = (w * np.where(clip_t, tt / np.where(clip_t, nrm, real(1)), real(1)).astype(real)).astype(dtype)
            clipped_t.append(float(np.mean(clip_t[:live])))
            dd = float(np.sum(np.abs(d.astype(np.complex128)) ** 2))
            xx = float(np.sum(np.abs(xp.astype(np.complex128)) ** 2))
            prior = np.float64(tv_t) * frame_norms_t(xp, periodic)
            if spatial:
                prior = tw * frame_norms_s(xp) + prior
            x = xp
            change = 0.0 if (dd == 0.0 and xx == 0.0) else float(np.sqrt(np.float64(dd) / np.float64(xx)))
        hist.append(np.stack([np.full(K, change), prior], axis=1))
        iters = it
        if not np.isfinite(change):
            status = BREAKDOWN
            break
        if change <= tol:
            status = CONVERGED
            break
    return {"x": x, "y": y, "z": z, "iterations": iters, "status": status, "change": change, "history": np.array(hist).reshape(-1, K, 2),
            "clipped_t": np.array(clipped_t), "clipped_s": np.array(clipped_s), "spatial": spatial}


def optimality_t(apply, b, x, y, z, tv_t, periodic=False, lam=0.0):
    """Float64 optimality of (x, y, z) (tv_t > 0):
        r = max|(G + μ) x − b + ∇ᴴy + ∇_tᴴz| / max|b|               stationarity in x
        e = max(max |z| / tv_t − 1, 0)                              z inside its ball
        g = (tv_t ‖∇_t x‖₁ − Re<z, ∇_t x>) / (tv_t ‖∇_t x‖₁)        z attains the norm of ∇_t x (the temporal gap)
    """
    x = np.asarray(x).astype(np.complex128)
    z = np.asarray(z).astype(np.complex128)
    b = np.asarray(b).astype(np.complex128)
    res = np.asarray(apply(x)).astype(np.complex128) + lam * x - b + adjoint_t(z, periodic)
    if y is not None:
        res = res + T.adjoint(np.asarray(y).astype(np.complex128), 0)
    r = float(np.abs(res).max() / np.abs(b).max())
    live = z if periodic else z[:-1]
    e = float(max(np.abs(live).max() / tv_t - 1.0, 0.0))
    gx = gradient_t(x, periodic)
    total = tv_t * float(np.abs(gx).sum())
    g = float((total - np.real(np.vdot(z, gx))) / total)
    return r, e, g
