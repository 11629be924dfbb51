"""numpy restatement of the Toeplitz normal operator and the exact Gram product from the oracle's direct sums.

Arrays follow the oracle's layout: reversed axes, dimension 1 fastest (shape ``N[::-1]``).
"""
import numpy as np

from oracle import nufft_oracle as O


def modes(N, fftshift=False):
    """Integer modes of an N-point axis in the plan's order."""
    k = O.fftfreq_int(N)
    return np.fft.fftshift(k) if fftshift else k


def mode_lists(Ns, fftshift=False):
    return [modes(n, fftshift).astype(np.float64) for n in Ns]


def exact_gram(Ns, xs, w, u, fftshift=False):
    """G u = nudft_type1(w · nudft_type2(u)) by direct sums: the answer every route is compared with."""
    ks = mode_lists(Ns, fftshift)
    return O.nudft_type1(ks, xs, w * O.nudft_type2(ks, xs, u))


def exact_spectrum(Ns, xs, w):
    """Step 1: T_d = Σ_j w_j exp(−i d·x_j) on the mode set of a 2N plan, FFT order."""
    return O.nudft_type1(mode_lists([2 * n for n in Ns]), xs, w)


def multiplier(Ns, T):
    """Step 2: K = backwardDFT_{2N}(T with its Nyquist planes zeroed) / Π 2N_d.  Returns (K complex, so that its imaginary part can be
    inspected)."""
    D = len(Ns)
    T = np.array(T, dtype=np.complex128)
    for d, n in enumerate(Ns):                  # dimension d is axis D − 1 − d
        idx = [slice(None)] * D
        idx[D - 1 - d] = n                      # d = −N_d sits at index N_d of the 2N grid
        T[tuple(idx)] = 0.0
    return np.fft.ifftn(T)                      # = backward DFT / Π 2N_d


def apply(Ns, K, u, fftshift=False):
    """Step 3: place mode k at index k mod 2N of a zero grid, unnormalised backward DFT, times K, forward DFT, read back."""
    D = len(Ns)
    idx = np.ix_(*[np.mod(np.asarray(modes(n, fftshift)).astype(np.int64), 2 * n) for n in reversed(Ns)])
    g = np.zeros([2 * n for n in reversed(Ns)], dtype=np.complex128)
    g[idx] = u
    g = np.fft.fftn(K * (np.fft.ifftn(g) * g.size))
    return g[idx]


def toeplitz_gram(Ns, xs, w, u, fftshift=False):
    """Steps 1 – 3 with the exact spectrum."""
    K = multiplier(Ns, exact_spectrum(Ns, xs, w))
    return apply(Ns, K.real, u, fftshift), K


# ---- the same construction for a real-data plan (why it is refused), one dimension ------------------------------------

def real_plan_gram_1d(N, x, w, u_half):
    """Exact type1(w · type2(û)) of a real-data plan: û holds k >= 0 only, type 2 extends it Hermitian-ly (nudft_type2_real)."""
    plan = O.OraclePlan((N,), is_real=True, M=4, sigma=2.0)
    v = O.nudft_type2_real(plan, [x], u_half)
    return O.nudft_type1(plan.ks, [x], w * v)


def real_plan_toeplitz_1d(N, x, w, u_half):
    """Steps 1 – 3 on the Hermitian extension of û over the N modes the embedding can hold, read back at k >= 0.  For even N the
    real type 2 also sums the mode +N/2, which the N-mode set (−N/2 … N/2 − 1) does not contain: it is dropped here, and whatever is
    done with it, differences of the modes actually summed reach ±N, beyond the 2N embedding."""
    nh = N // 2 + 1
    ext = np.zeros(N, dtype=np.complex128)
    for k in range(nh):
        if 2 * k < N:
            ext[k] += u_half[k]
        if k > 0:
            ext[N - k] += np.conj(u_half[k])
    g, _ = toeplitz_gram([N], [x], w, ext)
    out = g[:nh].copy()
    if N % 2 == 0:
        out[N // 2] = np.conj(g[N // 2])        # the output at +N/2 of a real v is the conjugate of the one at −N/2
    return out


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))
