"""numpy restatement of the primal-dual solver with a second-order total-generalized-variation prior, one system at a
time, and its optimality check.

Arrays live in a chosen complex dtype; sums and scalars are float64 for both dtypes, as in the library.  Dimension 1 is the fastest
one, the LAST axis of an array.  A vector field is an array [D, ...], a symmetric tensor field an array [S, ...] with S = D (D + 1) / 2
entries in row-major upper-triangle order, (1,1), (1,2), (1,3), (2,2), (2,3), (3,3); its off-diagonal entries count twice in norms and
inner products.  A coupled operator is run with the stacked components as one array and ``component_axis=0``, as in tv_reference.py.
"""
import numpy as np

import tv_reference as T

MAX_ITER, CONVERGED, BREAKDOWN = T.MAX_ITER, T.CONVERGED, T.BREAKDOWN
_real = T._real


def pairs(D):
    """(d, e), d <= e, in the order of the S arrays."""
    return [(d, e) for d in range(D) for e in range(d, D)]


def sym_weights(D):
    """1 for a diagonal entry, 2 for an off-diagonal one: the weights of |·|_F² and of the inner product."""
    return np.array([1.0 if d == e else 2.0 for d, e in pairs(D)])


def _back(u, e):
    """(∂⁻_e u)[i] = u[i] − u[i − e_e]; dimension e is axis −1 − e."""
    return u - np.roll(u, 1, axis=u.ndim - 1 - e)


def sym_gradient(v, component_axis=None):
    """(E v)_de = ½((∂⁻_e v_d) + (∂⁻_d v_e)), in this order, in the dtype of v: an array [S, ...] from a field [D, ...]."""
    half = _real(v.dtype)(0.5)
    out = []
    for d, e in pairs(v.shape[0]):
        s = _back(v[d], e) + _back(v[e], d)
        out.append((half * s.real + 1j * (half * s.imag)).astype(v.dtype))
    return np.stack(out)


def sym_adjoint(r, D, component_axis=None):
    """(Eᴴr)_d[i] = Σ_e (r_de[i] − r_de[i + e_e]) with r_ed = r_de, summed in the order e = 1 ... D in the dtype of r: [D, ...]."""
    index = {p: s for s, p in enumerate(pairs(D))}
    out = []
    for d in range(D):
        acc = None
        for e in range(D):
            u = r[index[(min(d, e), max(d, e))]]
            t = u - np.roll(u, -1, axis=u.ndim - 1 - e)
            acc = t if acc is None else acc + t
        out.append(acc)
    return np.stack(out)


def frobenius_norms(w):
    """|W_i|_F in float64 from the entries [S, ...]."""
    D = int(round((np.sqrt(8 * w.shape[0] + 1) - 1) / 2))
    w = w.astype(np.complex128)
    wt = sym_weights(D).reshape((-1,) + (1,) * (w.ndim - 1))
    return np.sqrt(np.sum(wt * (w.real ** 2 + w.imag ** 2), axis=0))


def sym_inner(a, b):
    """The weighted inner product ⟨a, b⟩_F of two tensor fields (conjugate-linear in a)."""
    D = int(round((np.sqrt(8 * a.shape[0] + 1) - 1) / 2))
    return sum(w * np.vdot(u, v) for w, u, v in zip(sym_weights(D), a, b))


def _project(u, t, weights, real):
    """u_i · min(1, t / |u_i|) with the weighted norm over axis 0, in the precision `real`; returns (projected, clipped)."""
    wt = weights.astype(real).reshape((-1,) + (1,) * (u.ndim - 1))
    nrm = np.sqrt(np.sum(wt * (u.real ** 2 + u.imag ** 2), axis=0, dtype=real)).astype(real)
    clip = nrm > t
    scale = np.where(clip, t / np.where(clip, nrm, real(1)), real(1)).astype(real)
    return (u * scale).astype(u.dtype), clip


def tgvpd(apply, b, alpha1, alpha0, step, sigma=None, lam=0.0, tol=1e-4, max_iter=100, x0=None, dtype=np.complex128, component_axis=None):
    """The algorithm of the header's TGV section, literally.  ``apply(x)`` returns G x.  ``alpha1``, ``alpha0``: scalars, or with
    ``component_axis`` one weight per component.  Returns a dict: x, v ([D, ...]), p ([D, ...]), r ([S, ...]), iterations, status,
    change, history ([iterations, 3]: change, Σ|∇x⁺ − v⁺|₂, Σ|E v⁺|_F), clipped_p and clipped_r ([iterations]: share of cells whose dual
    vector / tensor the projection shortened)."""
    real = _real(dtype)
    b = np.asarray(b).astype(dtype)
    D = b.ndim - (0 if component_axis is None else 1)
    tau, mu = real(step), real(lam)
    sig = real(1.0 / (16.0 * D * step) if sigma is None else sigma)
    t1 = np.asarray(alpha1, dtype=np.float64).astype(real)
    t0 = np.asarray(alpha0, dtype=np.float64).astype(real)
    if component_axis is not None:
        t1 = np.broadcast_to(t1, (b.shape[0],)).reshape((b.shape[0],) + (1,) * D)
        t0 = np.broadcast_to(t0, (b.shape[0],)).reshape((b.shape[0],) + (1,) * D)
    x = np.zeros_like(b) if x0 is None else np.asarray(x0).astype(dtype).copy()
    S = D * (D + 1) // 2
    v = np.zeros((D,) + b.shape, dtype=dtype)
    p = np.zeros((D,) + b.shape, dtype=dtype)
    r = np.zeros((S,) + b.shape, dtype=dtype)
    hist, clipped_p, clipped_r, iters, status, change = [], [], [], 0, MAX_ITER, np.nan
    for it in range(1, max_iter + 1):
        with np.errstate(all="ignore"):
            q = np.asarray(apply(x)).astype(dtype)
            xp = (x - tau * (q + mu * x - b + T.adjoint(p, component_axis))).astype(dtype)
            d = (xp - x).astype(dtype)
            xbar = (xp + d).astype(dtype)
            vp = (v - tau * (sym_adjoint(r, D, component_axis) - p)).astype(dtype)
            vbar = (vp + (vp - v)).astype(dtype)
            p, clip_p = _project((p + sig * (T.gradient(xbar, component_axis) - vbar)).astype(dtype), t1, np.ones(D), real)
            r, clip_r = _project((r + sig * sym_gradient(vbar, component_axis)).astype(dtype), t0, sym_weights(D), real)
            dd = float(np.sum(np.abs(d.astype(np.complex128)) ** 2))
            xx = float(np.sum(np.abs(xp.astype(np.complex128)) ** 2))
            s1 = float(T.cell_norms(T.gradient(xp, component_axis) - vp).sum())
            s0 = float(frobenius_norms(sym_gradient(vp, component_axis)).sum())
            x, v = xp, vp
            change = 0.0 if (dd == 0.0 and xx == 0.0) else float(np.sqrt(np.float64(dd) / np.float64(xx)))
        hist.append((change, s1, s0))
        clipped_p.append(float(np.mean(clip_p)))
        clipped_r.append(float(np.mean(clip_r)))
        iters = it
        if not np.isfinite(change):
            status = BREAKDOWN
            break
        if change <= tol:
            status = CONVERGED
            break
    return {"x": x, "v": v, "p": p, "r": r, "iterations": iters, "status": status, "change": change,
            "history": np.array(hist).reshape(-1, 3), "clipped_p": np.array(clipped_p), "clipped_r": np.array(clipped_r)}


def optimality(apply, b, x, v, p, r, alpha1, alpha0, lam=0.0, component_axis=None):
    """Float64 optimality of (x, v, p, r) for the TGV² objective (scalar weights), a tuple (r_x, r_v, e_1, e_0, g_1, g_0):
        r_x = max|(G + μ) x − b + ∇ᴴp| / max|b|                      stationarity in x
        r_v = max|−p + Eᴴr| / α1                                     stationarity in v
        e_1 = max(max_i |p_i|₂ / α1 − 1, 0),  e_0 likewise with |r_i|_F / α0        the duals inside their balls
        g_1 = (α1 Σ|∇x − v|₂ − Re⟨p, ∇x − v⟩) / (α1 Σ|∇x − v|₂)      p attains the norm of ∇x − v
        g_0 = (α0 Σ|Ev|_F − Re⟨r, Ev⟩_F) / (α0 Σ|Ev|_F)              r attains the norm of E v (nan when E v = 0 or α0 = 0)
    """
    c = lambda a: np.asarray(a).astype(np.complex128)      # noqa: E731
    x, v, p, r, b = c(x), c(v), c(p), c(r), c(b)
    D = v.shape[0]
    r_x = float(np.abs(c(apply(x)) + lam * x - b + T.adjoint(p, component_axis)).max() / np.abs(b).max())
    r_v = float(np.abs(sym_adjoint(r, D, component_axis) - p).max() / alpha1)
    e_1 = float(max(T.cell_norms(p).max() / alpha1 - 1.0, 0.0))
    e_0 = float(max(frobenius_norms(r).max() / alpha0 - 1.0, 0.0)) if alpha0 > 0 else 0.0
    g = T.gradient(x, component_axis) - v
    total1 = alpha1 * float(T.cell_norms(g).sum())
    g_1 = float((total1 - np.real(np.vdot(p, g))) / total1)
    ev = sym_gradient(v, component_axis)
    total0 = alpha0 * float(frobenius_norms(ev).sum())
    with np.errstate(all="ignore"):
        g_0 = float((total0 - np.real(sym_inner(r, ev))) / total0) if total0 > 0 else float("nan")
    return r_x, r_v, e_1, e_0, g_1, g_0
