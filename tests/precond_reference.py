"""numpy restatement of T. Chan's optimal circulant preconditioner of the Toeplitz normal operator and of preconditioned conjugate
gradients.

Arrays follow the oracle's layout: reversed axes, dimension 1 fastest (shape ``N[::-1]``).  ``F`` is the unnormalised N-point DFT over
the ARRAY indices of a component (``numpy.fft.fftn``), whatever the plan's ``fftshift``: for ``fftshift=True`` G is Toeplitz in the array
index, for ``fftshift=False`` it is that matrix with rows and columns rotated cyclically together, which leaves a circulant unchanged.
"""
import numpy as np

import cg_reference as CG


def generating_sequence(Ns, K):
    """``T = forwardDFT_2N(K)`` from the operator's multiplier K (shape ``(2N)[::-1]``): T[d mod 2N] = G[k, k'] for d = k − k'."""
    return np.fft.fftn(np.asarray(K).astype(np.complex128))


def chan_eigenvalues(Ns, spectrum):
    """``e = DFT_N(c)`` (complex: the imaginary part is round-off) with c the Fejér-weighted fold of the generating sequence ``spectrum``
    on the 2N grid (FFT order, shape ``(2N)[::-1]``; what ``toeplitz_reference.exact_spectrum`` returns, or ``generating_sequence``):

        c_j = Σ_{s ∈ {0,1}^D} Π_d ω_d(j_d, s_d) T[(j − s ⊙ N) mod 2N],   ω_d(j, 0) = (N_d − j) / N_d,   ω_d(j, 1) = j / N_d.

    ``e.real`` equals ``Re diag(F G F^H) / n``: the eigenvalues of ``argmin_{C circulant} ‖C − G‖_F``."""
    D = len(Ns)
    T = np.asarray(spectrum).astype(np.complex128)
    c = np.zeros(tuple(reversed(Ns)), dtype=np.complex128)
    for s in range(1 << D):
        w = np.ones_like(c, dtype=np.float64)
        index = []
        for a, n in enumerate(reversed(Ns)):            # axis a is dimension D − 1 − a
            sd = (s >> (D - 1 - a)) & 1
            j = np.arange(n)
            shape = [1] * D
            shape[a] = n
            w = w * ((j / n) if sd else ((n - j) / n)).reshape(shape)
            index.append(np.mod(j - sd * n, 2 * n))
        # (the Nyquist planes are read here with weight 0; they are finite)
        c += w * T[np.ix_(*index)]
    return np.fft.fftn(c)


def multiplier(e, mu=0.0, floor=1e-6):
    """``m = 1 / (n max(e + μ, floor max(e + μ)))``: the inverse eigenvalues with the 1/n of the inverse DFT folded in."""
    v = np.asarray(e).real + mu
    return 1.0 / (v.size * np.maximum(v, floor * v.max()))


def apply(m, d, r):
    """``M⁻¹ r = d ⊙ F⁻¹(m ⊙ F(d ⊙ r))`` with the unnormalised transforms (1/n is in m); ``d = None``: no scaling."""
    r = np.asarray(r).astype(np.complex128)
    v = r if d is None else d * r
    v = np.fft.ifftn(m * np.fft.fftn(v)) * v.size
    return v if d is None else d * v


def dense_inverse(m, d=None):
    """The matrix of ``apply`` (columns flattened like the arrays)."""
    n = m.size
    eye = np.eye(n, dtype=np.complex128)
    return np.stack([apply(m, d, eye[:, k].reshape(m.shape)).ravel() for k in range(n)], axis=1)


def coil_scaling(maps, lam=0.0):
    """``d = (max(Σ_c |S_c|², 1e-3 max))^(−1/2)`` and ``μ = λ / mean(Σ_c |S_c|²)`` for coil maps ``maps[c]``."""
    s = np.sum(np.abs(np.asarray(maps)) ** 2, axis=0)
    return 1.0 / np.sqrt(np.maximum(s, 1e-3 * s.max())), lam / s.mean()


def pcg(apply_G, apply_M, b, lam=0.0, rtol=1e-6, max_iter=50, x0=None, dtype=np.complex128):
    """Preconditioned CG with the recurrences of the header's Preconditioner section and the stopping rule of ``cg_reference.cg``
    (``‖r‖ / ‖b‖`` of the recursive residual).  ``apply_M(r)`` returns M⁻¹ r.  Returns the dict of ``cg_reference.cg``."""
    real = np.float32 if dtype == np.complex64 else np.float64
    lam_t = real(lam)
    b = np.asarray(b).astype(dtype)
    if x0 is None:
        x = np.zeros_like(b)
        r = b.copy()
    else:
        x = np.asarray(x0).astype(dtype).copy()
        r = (b - (np.asarray(apply_G(x)).astype(dtype) + lam_t * x)).astype(dtype)
    rho, beta0 = CG._sum(r, r), CG._sum(b, b)
    hist = [CG._rel(rho, beta0)]
    iters, broke = 0, False
    p = r.copy()
    rho_z = 0.0
    if not rho <= rtol * rtol * beta0:
        z = np.asarray(apply_M(r)).astype(dtype)
        rho_z = CG._sum(r, z)
        if rho_z > 0 and np.isfinite(rho_z):
            p = z.copy()
        else:
            broke = True
    for it in range(1, max_iter + 1):
        if broke or rho <= rtol * rtol * beta0:
            break
        q = np.asarray(apply_G(p)).astype(dtype)
        gamma = CG._sum(p, q) + lam * CG._sum(p, p)
        if not (gamma > 0 and np.isfinite(gamma)):
            broke = True
            break
        alpha = real(rho_z / gamma)
        x = (x + alpha * p).astype(dtype)
        r = (r - alpha * (q + lam_t * p)).astype(dtype)
        rho = CG._sum(r, r)
        z = np.asarray(apply_M(r)).astype(dtype)
        rho_z_new = CG._sum(r, z)
        hist.append(CG._rel(rho, beta0))
        iters = it
        if rho <= rtol * rtol * beta0:
            break
        if not (rho_z_new > 0 and np.isfinite(rho_z_new)):
            broke = True
            break
        p = (z + real(rho_z_new / rho_z) * p).astype(dtype)
        rho_z = rho_z_new
    status = CG.BREAKDOWN if broke else (CG.CONVERGED if rho <= rtol * rtol * beta0 else CG.MAX_ITER)
    return {"x": x, "iterations": iters, "status": status, "history": np.array(hist)}


def exact_spectrum_separable(Ns, xs, w):
    """``toeplitz_reference.exact_spectrum`` as one matrix product (the exponentials factor over the dimensions): the same direct sum,
    fast enough for tens of thousands of points.  Shape ``(2N)[::-1]``, FFT order."""
    D = len(Ns)
    ks = [np.fft.fftfreq(2 * n, 1.0 / (2 * n)) for n in Ns]
    first = np.exp(-1j * np.outer(ks[0], xs[0]))                    # [2N_1, Np]
    rest = np.asarray(w).astype(np.complex128)[None, :]
    for d in range(1, D):                                           # rows ordered with the LAST dimension slowest
        e = np.exp(-1j * np.outer(ks[d], xs[d]))
        rest = (e[:, None, :] * rest[None, :, :]).reshape(-1, rest.shape[1])
    return (rest @ first.T).reshape([2 * n for n in reversed(Ns)])
