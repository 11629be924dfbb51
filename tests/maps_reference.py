"""numpy restatement, in float64, of the coil sensitivity map estimate (Walsh, Gmitro & Marcellin 2000).

Arrays are stacked: ``a[c]`` is coil c, of shape ``Ns[::-1]`` (dimension 1 is the last, fastest axis); ``box`` is given per dimension,
``(b_1, …, b_D)``, odd sides; the box is centred at the cell and periodic on the array.
"""
import numpy as np


def covariance(a, box):
    """R[..., c, c'] = Σ_{x' ∈ box(x)} a_c(x') conj(a_c'(x')): products first, then one ``np.roll`` sum per axis."""
    a = np.asarray(a).astype(np.complex128)
    D = a.ndim - 1
    b = [int(v) for v in box][::-1]                          # per axis
    assert len(b) == D and all(v % 2 == 1 and 1 <= v <= n for v, n in zip(b, a.shape[1:]))
    R = a[:, None] * np.conj(a[None, :])
    for ax, v in enumerate(b):
        h = (v - 1) // 2
        R = sum(np.roll(R, -k, axis=2 + ax) for k in range(-h, h + 1))
    return np.moveaxis(R, (0, 1), (-2, -1))


def pca_reference(a):
    """The dominant eigenvector of the global Gram matrix G[c, c'] = Σ_x a_c conj(a_c'), its largest entry made real and positive."""
    m = np.asarray(a).astype(np.complex128).reshape(len(a), -1)
    p = np.linalg.eigh(m @ m.conj().T)[1][:, -1]
    k = int(np.argmax(np.abs(p)))
    return p * (np.conj(p[k]) / abs(p[k]))


def walsh(a, box, phase_ref=None, crop=0.0, eigh=np.linalg.eigh, info=None):
    """Returns (maps [C, ...], λ1 [...], λ2 [...]).  ``eigh``: ``np.linalg.eigh`` (batched over the cells) or a function of one matrix
    that returns (λ, V) or (λ, V, sweeps), such as ``llr_reference.jacobi_eigh``: the kernel's solver.  λ1 is the largest eigenvalue, the
    first index on a tie, λ2 the second largest (0 for one coil), v the column of λ1 scaled to unit length; s = Σ_c conj(p_c) v_c and v <- v conj(s) / |s|
    where |s| > 0; zeros where λ1 = 0 and, with crop > 0, where λ1 < crop² max λ1.  ``info`` (a dict) receives the largest sweep count
    and the smallest |s| and relative gap (λ1 − λ2) / λ1."""
    a = np.asarray(a).astype(np.complex128)
    C, shape = a.shape[0], a.shape[1:]
    R = covariance(a, box).reshape(-1, C, C)
    n = R.shape[0]
    p = np.zeros(C, dtype=np.complex128)
    if phase_ref is None:
        p[0] = 1.0
    else:
        p[:] = phase_ref
    sweeps = 0
    if eigh is np.linalg.eigh:
        w, V = np.linalg.eigh(R)
        lam1, v = w[:, -1].copy(), V[:, :, -1].copy()
        lam2 = w[:, -2].copy() if C > 1 else np.zeros(n)
    else:
        lam1, lam2, v = np.empty(n), np.zeros(n), np.empty((n, C), dtype=np.complex128)
        for i in range(n):
            res = eigh(R[i])
            lam, vec = np.asarray(res[0]), np.asarray(res[1])
            if len(res) > 2:
                sweeps = max(sweeps, res[2])
            k = int(np.argmax(lam))                          # the first index on a tie
            lam1[i], v[i] = lam[k], vec[:, k]
            if C > 1:
                lam2[i] = np.delete(lam, k).max()
    v /= np.sqrt((np.abs(v) ** 2).sum(axis=1))[:, None]          # the rotations of a Jacobi cost a column a few ε of its unit length
    s = v @ np.conj(p)
    mod = np.abs(s)
    on = mod > 0
    v[on] *= (np.conj(s[on]) / mod[on])[:, None]
    v[lam1 == 0] = 0.0
    if crop > 0:
        v[lam1 < crop * crop * lam1.max()] = 0.0
    if info is not None:
        keep = lam1 > 0
        info["sweeps"] = sweeps
        info["min_s"] = float(mod[keep].min()) if keep.any() else np.inf
        info["min_gap"] = float(((lam1[keep] - lam2[keep]) / lam1[keep]).min()) if keep.any() else np.inf
    return np.moveaxis(v.reshape(shape + (C,)), -1, 0), lam1.reshape(shape), lam2.reshape(shape)
