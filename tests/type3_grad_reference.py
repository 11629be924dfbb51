"""Numpy restatement of the type-3 gradient (a plain helper of tests/test_type3_gradient_host.py and
tests/test_gpu_type3_gradient.py).

``phihat`` restates ``phihat_dev`` (csrc/type3_kernels.hip): ϕ̂ of the spreading plan's window at a real wavenumber k on a grid of
spacing dx, with β (Kaiser-Bessel windows) or τ (Gaussian) as ``param``.  ``dlogphihat`` is its logarithmic derivative d ln ϕ̂ / dk
in closed form.  ``direct3`` / ``direct3_grad`` are the exact sums f_k = Σ_j c_j e^{σ i s_k·x_j} and
∂f_k/∂s_{k,d} = Σ_j c_j (σ i x_{j,d}) e^{σ i s_k·x_j} in complex128.
"""
import math

import numpy as np
from scipy.special import i0, i1, j0, j1

KERNELS = ("bkb", "kb", "gauss", "bspline")


def phihat(kernel, M, dx, param, k):
    k = np.asarray(k, dtype=np.float64)
    if kernel in ("bkb", "kb"):
        w = M * dx
        z = param * param - (w * k) ** 2
        u = np.sqrt(np.abs(z))
        if kernel == "bkb":
            return np.where(z >= 0, w * i0(u), w * j0(u))
        with np.errstate(invalid="ignore", divide="ignore"):
            pos = 2.0 * w * np.sinh(u) / u
            neg = 2.0 * w * np.sin(u) / u
        return np.where(u == 0, 2.0 * w, np.where(z > 0, pos, neg))
    if kernel == "gauss":
        return np.exp(-param * k * k * 0.25) * math.sqrt(math.pi * param)
    a = k * dx * 0.5
    with np.errstate(invalid="ignore", divide="ignore"):
        sn = np.where(a == 0, 1.0, np.sin(a) / np.where(a == 0, 1.0, a))
    return sn ** (2 * M) * dx


def dlogphihat(kernel, M, dx, param, k):
    """d ln ϕ̂ / dk at k (same arguments as ``phihat``)."""
    k = np.asarray(k, dtype=np.float64)
    if kernel in ("bkb", "kb"):
        w = M * dx
        z = param * param - (w * k) ** 2
        u = np.sqrt(np.abs(z))
        us = np.where(u == 0, 1.0, u)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if kernel == "bkb":          # I1(u) / (u I0(u)) above the band edge, J1(u) / (u J0(u)) past it; → 1/2 at u → 0
                r = np.where(z >= 0, i1(us) / (us * i0(us)), j1(us) / (us * j0(us)))
                r = np.where(u < 1e-8, 0.5, r)
            else:                        # (s coth s − 1) / s² with s² = z, (1 − u cot u) / u² past the band; → 1/3 at z → 0
                r = np.where(z > 0, (us / np.tanh(us) - 1.0) / (us * us), (1.0 - us * np.cos(us) / np.sin(us)) / (us * us))
                r = np.where(np.abs(z) < 1e-4, 1.0 / 3.0 - z / 45.0 + 2.0 * z * z / 945.0, r)
        return -w * w * k * r
    if kernel == "gauss":
        return -0.5 * param * k
    a = k * dx * 0.5
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.cos(a) / np.sin(a) - 1.0 / np.where(a == 0, 1.0, a)
    g = np.where(np.abs(a) < 1e-3, -a * (1.0 / 3.0 + a * a / 45.0), g)
    return M * dx * g


def _chunks(np_, nk):
    step = max(1, int(4e6) // max(nk, 1))
    return [(j, min(j + step, np_)) for j in range(0, np_, step)]


def direct3(x, s, c, sign):
    """f_k = Σ_j c_j exp(sign i s_k·x_j); x (Np, D), s (Nk, D)."""
    s64, x64, cc = s.astype(np.float64), x.astype(np.float64), c.astype(np.complex128)
    out = np.zeros(s.shape[0], dtype=np.complex128)
    for a, b in _chunks(x.shape[0], s.shape[0]):
        out += np.exp(sign * 1j * (s64 @ x64[a:b].T)) @ cc[a:b]
    return out


def direct3_grad(x, s, c, sign):
    """(Nk, D): ∂f_k/∂s_{k,d} = Σ_j c_j (sign i x_{j,d}) exp(sign i s_k·x_j)."""
    D = s.shape[1]
    s64, x64, cc = s.astype(np.float64), x.astype(np.float64), c.astype(np.complex128)
    out = np.zeros((s.shape[0], D), dtype=np.complex128)
    for a, b in _chunks(x.shape[0], s.shape[0]):
        E = np.exp(sign * 1j * (s64 @ x64[a:b].T))
        for d in range(D):
            out[:, d] += E @ (cc[a:b] * (sign * 1j) * x64[a:b, d])
    return out


def post_factor(kernel, M, sign, s, src_center, tgt_center, gamma, h, param, scale_exp):
    """P(s) = e^{sign i s·C} Π_d h_d 2^{−k_d} / ϕ̂_d(γ_d t_d) and ρ (Nk, D) = γ_d (d ln ϕ̂_d / dk)(γ_d t_d), with t = s − D."""
    s = np.asarray(s, dtype=np.float64)
    D = s.shape[1]
    arg = s @ np.asarray(src_center[:D], dtype=np.float64)
    P = np.exp(sign * 1j * arg)
    rho = np.empty_like(s)
    for d in range(D):
        t = s[:, d] - tgt_center[d]
        k = gamma[d] * t
        P = P * (math.ldexp(h[d], -scale_exp[d]) / phihat(kernel, M, h[d], param[d], k))
        rho[:, d] = gamma[d] * dlogphihat(kernel, M, h[d], param[d], k)
    return P, rho


def finish(P, rho, v, dv, sign, src_center, theta_scale):
    """The finish kernel in float64: f = P v, ∂f/∂s_d = P [θs_d ∂_θd v + (sign i C_d − ρ_d) v], θs_d = sign γ_d h_d."""
    f = P * v
    grads = [P * (theta_scale[d] * dv[d] + (sign * 1j * src_center[d] - rho[:, d]) * v) for d in range(len(dv))]
    return f, grads
