"""numpy restatement, in float64, of the locally low-rank proximal map and of FISTA with that prior.

Arrays are stacked: ``x[a]`` is component a, of shape ``Ns[::-1]`` (dimension 1 is the last, fastest axis); ``block`` and ``shift`` are
given per dimension, ``(b_1, …, b_D)``.  Storage index ``i_d`` belongs to block ``floor(((i_d − s_d) mod N_d) / b_d)``.
"""
import numpy as np

MAX_ITER, CONVERGED, BREAKDOWN = "max_iter", "converged", "breakdown"
SWEEPS_MAX = 24
SKIP_REL, SKIP_ABS = 2.0 ** -106, 2.0 ** -60
LCG_A, LCG_C, MASK = 6364136223846793005, 1442695040888963407, (1 << 64) - 1


def _casorati(x, block, shift):
    """[blocks, B, K] matrices of the stacked array x, and what ``_uncasorati`` needs to undo it."""
    K, shape, D = x.shape[0], x.shape[1:], x.ndim - 1
    b = [int(v) for v in block][::-1]                       # per axis
    s = [0] * D if shift is None else [int(v) for v in shift][::-1]
    assert len(b) == D and all(n % v == 0 for n, v in zip(shape, b)) and all(0 <= w < v for w, v in zip(s, b))
    y = np.roll(x, [-w for w in s], axis=tuple(range(1, D + 1)))
    split = [K]
    for n, v in zip(shape, b):
        split += [n // v, v]
    y = y.reshape(split)
    order = [2 * d + 1 for d in range(D)] + [2 * d + 2 for d in range(D)] + [0]
    y = y.transpose(order)
    nblocks, B = int(np.prod(y.shape[:D])), int(np.prod(b))
    return y.reshape(nblocks, B, K), (split, order, s, D)


def _uncasorati(m, meta):
    split, order, s, D = meta
    shape_t = [split[i] for i in order]
    y = m.reshape(shape_t).transpose(np.argsort(order))
    y = y.reshape([split[0]] + [split[1 + 2 * d] * split[2 + 2 * d] for d in range(D)])
    return np.roll(y, s, axis=tuple(range(1, D + 1)))


def block_singular_values(x, block, shift=None):
    m, _ = _casorati(np.asarray(x).astype(np.complex128), block, shift)
    return np.linalg.svd(m, compute_uv=False)


def prox(x, block, t, shift=None):
    """Singular-value soft-thresholding of every block through ``np.linalg.svd``.  Returns (out, Σ of the kept singular values, share of
    the singular values that were set to zero)."""
    x = np.asarray(x).astype(np.complex128)
    m, meta = _casorati(x, block, shift)
    u, sv, vh = np.linalg.svd(m, full_matrices=False)
    kept = np.maximum(sv - t, 0.0)
    out = (u * kept[:, None, :]) @ vh
    return _uncasorati(out, meta), float(kept.sum()), float(np.mean(kept == 0.0))


def jacobi_eigh(H):
    """The kernel's eigensolver, literally: cyclic-by-rows complex Jacobi on the Hermitian K × K matrix H in float64.  A rotation (p, q)
    is skipped when |h_pq|² <= max(2^-106 |h_pp h_qq|, (2^-60 trace H)²); the sweeps stop after the first one that rotates nothing, at
    most SWEEPS_MAX.  Returns (eigenvalues = the final diagonal, V with H = V diag(λ) V^H, sweeps run including the idle one)."""
    H = np.array(H, dtype=np.complex128)
    K = H.shape[0]
    V = np.eye(K, dtype=np.complex128)
    tr = float(sum(H[i, i].real for i in range(K)))
    floor2 = (SKIP_ABS * tr) * (SKIP_ABS * tr)
    sweeps = 0
    for _ in range(SWEEPS_MAX if K > 1 else 0):
        sweeps += 1
        rotated = False
        for p in range(K - 1):
            for q in range(p + 1, K):
                app, aqq, g = H[p, p].real, H[q, q].real, H[p, q]
                g2 = g.real * g.real + g.imag * g.imag
                if g2 <= max(SKIP_REL * abs(app * aqq), floor2):
                    continue
                rotated = True
                ag = np.sqrt(g2)
                tau = (aqq - app) / (2.0 * ag)
                tt = (1.0 if tau >= 0.0 else -1.0) / (abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + tt * tt)
                sp = (tt * c) * (g / ag)
                for A in (H, V):                                     # A <- A J,  J = [[c, sp], [−conj(sp), c]]
                    x, y = A[:, p].copy(), A[:, q].copy()
                    A[:, p] = c * x - np.conj(sp) * y
                    A[:, q] = sp * x + c * y
                x, y = H[p, :].copy(), H[q, :].copy()                # H <- J^H H
                H[p, :] = c * x - sp * y
                H[q, :] = np.conj(sp) * x + c * y
                H[p, q] = H[q, p] = 0.0
                H[p, p], H[q, q] = H[p, p].real, H[q, q].real
        if not rotated:
            break
    return np.array([H[i, i].real for i in range(K)]), V, sweeps


def shrink_matrix(lam, V, t):
    """P = V diag(f) V^H with f_i = σ_i > t ? 1 − t / σ_i : 0, σ_i = sqrt(max(λ_i, 0)); and Σ f_i σ_i."""
    sigma = np.sqrt(np.maximum(lam, 0.0))
    f = np.zeros_like(sigma)
    on = sigma > t
    f[on] = 1.0 - t / sigma[on]
    return (V * f[None, :]) @ V.conj().T, float(np.sum(f * sigma))


def prox_gram(x, block, t, shift=None, eigh=None):
    """The kernel's route: H = M^H M, H = V Λ V^H (``jacobi_eigh``, or ``eigh`` if given: a function H -> (λ, V)), M <- M P.  Returns
    (out, Σ kept singular values, the largest sweep count)."""
    x = np.asarray(x).astype(np.complex128)
    m, meta = _casorati(x, block, shift)
    out, nuc, most = np.empty_like(m), 0.0, 0
    for i in range(m.shape[0]):
        H = m[i].conj().T @ m[i]
        if eigh is None:
            lam, V, sweeps = jacobi_eigh(H)
            most = max(most, sweeps)
        else:
            lam, V = eigh(H)
        P, s = shrink_matrix(lam, V, t)
        out[i] = m[i] @ P
        nuc += s
    return _uncasorati(out, meta), nuc, most


def shift_sequence(seed, block, it):
    """The cyclic shift of iteration ``it`` (1-based): state_0 = seed; per iteration and dimension state <- state · a + c mod 2^64,
    s_d = (state >> 33) mod b_d."""
    state, s = int(seed) & MASK, None
    for _ in range(it):
        s = []
        for b in block:
            state = (state * LCG_A + LCG_C) & MASK
            s.append(int((state >> 33) % int(b)))
    return tuple(s)


def fista_llr(apply, b, block, nuc, step, lam=0.0, tol=1e-4, max_iter=100, shifts=False, seed=0, dtype=np.complex128):
    """The solver's iteration on the stacked right-hand side b ([K, ...]); ``apply(z)`` returns G z for a stacked z.  Arrays live in
    ``dtype``; sums, the threshold and the proximal map are float64.  Returns a dict shaped like fista_reference.fista's: x, iterations,
    status, change, history ([iterations, 2]: change and Σ_blocks ‖M‖_*), zero_fraction (share of zeroed singular values in the last
    iteration run)."""
    real = np.float32 if dtype == np.complex64 else np.float64
    tau, mu = real(step), real(lam)
    thr = float(step) * float(nuc)
    b = np.asarray(b).astype(dtype)
    x = np.zeros_like(b)
    z = x.copy()
    t, hist, iters, status, change, zero_fraction = 1.0, [], 0, MAX_ITER, np.nan, np.nan
    for it in range(1, max_iter + 1):
        t_next = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        beta = real((t - 1.0) / t_next)
        t = t_next
        q = np.asarray(apply(z)).astype(dtype)
        v = (z - tau * (q + mu * z - b)).astype(dtype)
        xp, nsum, zero_fraction = prox(v, block, thr, shift_sequence(seed, block, it) if shifts else None)
        xp = xp.astype(dtype)
        d = (xp - x).astype(dtype)
        dd = float(np.sum(np.abs(d.astype(np.complex128)) ** 2))
        xx = float(np.sum(np.abs(xp.astype(np.complex128)) ** 2))
        z = (xp + beta * d).astype(dtype)
        x = xp
        with np.errstate(divide="ignore", invalid="ignore"):
            change = 0.0 if (dd == 0.0 and xx == 0.0) else float(np.sqrt(np.float64(dd) / np.float64(xx)))
        hist.append((change, nsum))
        iters = it
        if not np.isfinite(change):
            status = BREAKDOWN
            break
        if change <= tol:
            status = CONVERGED
            break
    return {"x": x, "iterations": iters, "status": status, "change": change, "history": np.array(hist).reshape(-1, 2),
            "zero_fraction": zero_fraction}


def fixed_point_residual(apply, b, x, block, nuc, step, lam=0.0):
    """‖x − prox_{τ nuc}(x − τ ((G + μ) x − b))‖ / ‖x‖ in float64: zero exactly at a minimiser."""
    x = np.asarray(x).astype(np.complex128)
    b = np.asarray(b).astype(np.complex128)
    v = x - step * (np.asarray(apply(x)).astype(np.complex128) + lam * x - b)
    p, _, _ = prox(v, block, step * nuc)
    return float(np.linalg.norm(x - p) / np.linalg.norm(x))
