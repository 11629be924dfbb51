"""numpy restatement of the conjugate-gradient solver on (G + λI) x = b, one component at a time, and the exact dense
Gram matrix of a point set.

Arrays live in a chosen complex dtype; sums and scalars (γ, α, ρ, β0, history) are float64 for both dtypes, as in the library.
"""
import numpy as np

import toeplitz_reference as R

MAX_ITER, CONVERGED, BREAKDOWN = "max_iter", "converged", "breakdown"


def _sum(a, b):
    """Σ Re(conj(a) b) in float64."""
    a = a.ravel().astype(np.complex128)
    b = b.ravel().astype(np.complex128)
    return float(np.sum(a.real * b.real) + np.sum(a.imag * b.imag))


def _rel(rho, beta0):
    return np.sqrt(rho / beta0) if beta0 > 0 else (0.0 if rho == 0 else np.inf)


def cg(apply, b, x0=None, lam=0.0, rtol=1e-6, max_iter=50, dtype=np.complex128):
    """The algorithm of the header's CG section, literally.  ``apply(p)`` returns G p.  Returns a dict: x, iterations, status,
    history (relative recursive residual, entry 0 the start, one entry per iteration run)."""
    real = np.float32 if dtype == np.complex64 else np.float64
    lam_t = real(lam)
    b = np.asarray(b).astype(dtype)
    if x0 is None:
        x = np.zeros_like(b)
        r = b.copy()
    else:
        x = np.asarray(x0).astype(dtype).copy()
        r = (b - (np.asarray(apply(x)).astype(dtype) + lam_t * x)).astype(dtype)
    p = r.copy()
    rho, beta0 = _sum(r, r), _sum(b, b)
    hist = [_rel(rho, beta0)]
    iters, broke = 0, False
    for it in range(1, max_iter + 1):
        if rho <= rtol * rtol * beta0:          # done: frozen from here on
            break
        q = np.asarray(apply(p)).astype(dtype)
        gamma = _sum(p, q) + lam * _sum(p, p)
        if not (gamma > 0 and np.isfinite(gamma)):
            broke = True
            break
        alpha = real(rho / gamma)
        x = (x + alpha * p).astype(dtype)
        r = (r - alpha * (q + lam_t * p)).astype(dtype)
        rho_new = _sum(r, r)
        p = (r + real(rho_new / rho) * p).astype(dtype)
        rho = rho_new
        hist.append(_rel(rho, beta0))
        iters = it
    status = BREAKDOWN if broke else (CONVERGED if rho <= rtol * rtol * beta0 else MAX_ITER)
    return {"x": x, "iterations": iters, "status": status, "history": np.array(hist)}


def dense_gram(Ns, xs, w, fftshift=False, spectrum=None):
    """The exact matrix G[k, k'] = T[k − k'] in the plan's mode order (rows and columns flattened like an array of shape N[::-1]):
    one direct sum on the 2N modes (toeplitz_reference.exact_spectrum), then indexing."""
    T = R.exact_spectrum(Ns, xs, w) if spectrum is None else np.asarray(spectrum)
    D = len(Ns)
    index = []
    for a, n in enumerate(reversed(Ns)):        # axis a of the arrays is dimension D − 1 − a
        k = np.asarray(R.modes(n, fftshift)).astype(np.int64)
        d = np.mod(k[:, None] - k[None, :], 2 * n)
        shape = [1] * (2 * D)
        shape[a], shape[D + a] = n, n
        index.append(d.reshape(shape))
    n_all = int(np.prod(Ns))
    return T[tuple(index)].reshape(n_all, n_all)


def matrix_apply(A, shape):
    """apply(p) for cg() from a dense matrix, in float64."""
    return lambda p: (A @ np.asarray(p).astype(np.complex128).ravel()).reshape(shape)


def true_residual(A, lam, x, b):
    """‖b − (A + λ)x‖ / ‖b‖ in float64."""
    x = np.asarray(x).astype(np.complex128).ravel()
    b = np.asarray(b).astype(np.complex128).ravel()
    return float(np.linalg.norm(b - (A @ x + lam * x)) / np.linalg.norm(b))
