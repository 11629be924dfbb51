"""numpy restatement, in float64, of the low-rank plus sparse model of DESIGN.md §27: the global singular-value threshold, the temporal
transform with its shrink, and the proximal-gradient iteration on the pair (L, S).

Arrays are stacked: ``x[c]`` is frame c, of shape ``Ns[::-1]``.  ``C(x)`` is the n × K matrix whose column c is frame c.
"""
import numpy as np

import llr_reference as LR

MAX_ITER, CONVERGED, BREAKDOWN = "max_iter", "converged", "breakdown"
TRANSFORMS = ("dft", "identity")


def casorati(x):
    x = np.asarray(x)
    return x.reshape(x.shape[0], -1).T


def uncasorati(m, shape):
    return np.ascontiguousarray(m.T).reshape(shape)


def singular_values(x):
    return np.linalg.svd(casorati(np.asarray(x).astype(np.complex128)), compute_uv=False)


def svt(x, t):
    """Singular-value soft-thresholding of C(x) through ``np.linalg.svd``.  Returns (out, Σ of the kept singular values, number of
    singular values set to zero)."""
    x = np.asarray(x).astype(np.complex128)
    u, sv, vh = np.linalg.svd(casorati(x), full_matrices=False)
    kept = np.maximum(sv - t, 0.0)
    return uncasorati((u * kept[None, :]) @ vh, x.shape), float(kept.sum()), int(np.sum(kept == 0.0))


def svt_gram(x, t):
    """The kernels' route, literally: H = C^H C, H = V Λ V^H by ``llr_reference.jacobi_eigh``, P = V diag(f) V^H, C <- C P.  Returns (out,
    Σ f_i σ_i, sweeps)."""
    x = np.asarray(x).astype(np.complex128)
    m = casorati(x)
    lam, V, sweeps = LR.jacobi_eigh(m.conj().T @ m)
    P, nuc = LR.shrink_matrix(lam, V, t)
    return uncasorati(m @ P, x.shape), nuc, sweeps


def tdft(x, transform="dft", inverse=False):
    """T x (``inverse``: Tᴴ x) along axis 0 in float64: the DFT scaled by 1/√K, or the identity."""
    x = np.asarray(x).astype(np.complex128)
    if transform == "identity":
        return x.copy()
    assert transform == "dft"
    K = x.shape[0]
    return (np.fft.ifft(x, axis=0) * np.sqrt(K)) if inverse else (np.fft.fft(x, axis=0) / np.sqrt(K))


def tshrink(c, t):
    """The complex soft threshold as the kernel forms it, every operation rounded in the real type of ``c``:
    |c| = sqrt(re² + im²);  c · (1 − t / |c|) where |c| > t, else 0.  Returns (out, ‖out‖₁ in float64, share of zeros)."""
    c = np.asarray(c)
    real = np.float32 if c.dtype == np.complex64 else np.float64
    re, im, t = c.real.astype(real), c.imag.astype(real), real(t)
    mag = np.sqrt(re * re + im * im)
    on = mag > t
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(on, real(1) - t / mag, real(0)).astype(real)
    out = np.empty(c.shape, dtype=c.dtype)
    out.real, out.imag = np.where(on, re * s, real(0)), np.where(on, im * s, real(0))
    return out, float(np.abs(out.astype(np.complex128)).sum()), float(np.mean(~on))


def prox_sparse(v, t, transform):
    """Tᴴ soft_t(T v) in float64, the 1-norm of the coefficients and the share of zeroed ones."""
    c, l1, share = tshrink(tdft(v, transform), t)
    return tdft(c, transform, inverse=True), l1, share


def beta_of(it, momentum):
    """FISTA's β of iteration ``it`` (1-based): (t_it − 1) / t_{it+1}, t_1 = 1."""
    t = 1.0
    for _ in range(it - 1):
        t = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
    return (t - 1.0) / (0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))) if momentum else 0.0


def lps(apply, b, nuc, l1, step, transform="dft", momentum=True, lam=0.0, tol=1e-4, max_iter=100, x0=None, dtype=np.complex128):
    """The solver's iteration on the stacked right-hand side b ([K, ...]); ``apply(u)`` returns G u for a stacked u.  Arrays live in
    ``dtype``; sums, thresholds and the two proximal maps are float64.  Returns a dict: x, L, S, iterations, status, change, history
    ([iterations, 3]: change, ‖C(L)‖_*, ‖T S‖₁), zeroed_sv (singular values set to zero in the last iteration), zero_share (share of
    temporal coefficients set to zero in the last iteration)."""
    real = np.float32 if dtype == np.complex64 else np.float64
    tau, mu = real(step), real(lam)
    b = np.asarray(b).astype(dtype)
    L = np.zeros_like(b) if x0 is None else np.asarray(x0).astype(dtype)
    S = np.zeros_like(b)
    zL, zS = L.copy(), S.copy()
    hist, iters, status, change, zeroed, share = [], 0, MAX_ITER, np.nan, 0, np.nan
    for it in range(1, max_iter + 1):
        beta = real(beta_of(it, momentum))
        u = (zL + zS).astype(dtype)
        q = np.asarray(apply(u)).astype(dtype)
        g = (tau * (q + mu * u - b)).astype(dtype)
        Lp, nsum, zeroed = svt((zL - g).astype(dtype), float(step) * float(nuc))
        Lp = Lp.astype(dtype)
        Sp, l1sum, share = prox_sparse((zS - g).astype(dtype), float(step) * float(l1), transform)
        Sp = Sp.astype(dtype)
        dL, dS = (Lp - L).astype(dtype), (Sp - S).astype(dtype)
        dd = float(np.sum(np.abs(dL.astype(np.complex128)) ** 2) + np.sum(np.abs(dS.astype(np.complex128)) ** 2))
        xx = float(np.sum(np.abs(Lp.astype(np.complex128)) ** 2) + np.sum(np.abs(Sp.astype(np.complex128)) ** 2))
        zL, zS = (Lp + beta * dL).astype(dtype), (Sp + beta * dS).astype(dtype)
        L, S = Lp, Sp
        with np.errstate(divide="ignore", invalid="ignore"):
            change = 0.0 if (dd == 0.0 and xx == 0.0) else float(np.sqrt(np.float64(dd) / np.float64(xx)))
        hist.append((change, nsum, l1sum))
        iters = it
        if not np.isfinite(change):
            status = BREAKDOWN
            break
        if change <= tol:
            status = CONVERGED
            break
    return {"x": (L + S).astype(dtype), "L": L, "S": S, "iterations": iters, "status": status, "change": change,
            "history": np.array(hist).reshape(-1, 3), "zeroed_sv": zeroed, "zero_share": share}


def objective(apply, b, L, S, nuc, l1, transform="dft", lam=0.0):
    L, S, b = (np.asarray(v).astype(np.complex128) for v in (L, S, b))
    x = L + S
    smooth = 0.5 * np.vdot(x, np.asarray(apply(x)).astype(np.complex128) + lam * x).real - np.vdot(b, x).real
    return float(smooth + nuc * singular_values(L).sum() + l1 * np.abs(tdft(S, transform)).sum())


def fixed_point_residual(apply, b, L, S, nuc, l1, step, transform="dft", lam=0.0):
    """sqrt(‖L − L'‖² + ‖S − S'‖²) / sqrt(‖L‖² + ‖S‖²) in float64 with (L', S') one proximal-gradient step from (L, S): zero exactly at a
    minimiser."""
    L, S, b = (np.asarray(v).astype(np.complex128) for v in (L, S, b))
    x = L + S
    g = step * (np.asarray(apply(x)).astype(np.complex128) + lam * x - b)
    Lp = svt(L - g, step * nuc)[0]
    Sp = prox_sparse(S - g, step * l1, transform)[0]
    num = np.sqrt(np.linalg.norm(L - Lp) ** 2 + np.linalg.norm(S - Sp) ** 2)
    return float(num / np.sqrt(np.linalg.norm(L) ** 2 + np.linalg.norm(S) ** 2))
