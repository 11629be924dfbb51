"""numpy restatement of the periodic orthogonal wavelet transform and its proximal map.

Arrays follow the library's layout (shape ``N[::-1]``, every axis transformed); one analysis stage along an axis of length n is

    lo[i] = Σ_k h[k] a[(2i + k) mod n],   hi[i] = Σ_k g[k] a[(2i + k) mod n],   g[k] = (−1)^k h[L − 1 − k]

and the output is the Mallat layout in one array of the input's shape.  Arithmetic runs in the array's own complex dtype with the filter
cast to its real type, as in the library; ℓ1 sums are float64.
"""
import numpy as np

_S2, _S3 = np.sqrt(2.0), np.sqrt(3.0)
LOWPASS = {
    "haar": np.array([1.0, 1.0]) / _S2,
    "db2": np.array([1 + _S3, 3 + _S3, 3 - _S3, 1 - _S3]) / (4 * _S2),
}


def filters(wavelet, real=np.float64):
    h = LOWPASS[wavelet]
    g = np.array([(-1) ** k * h[len(h) - 1 - k] for k in range(len(h))])
    return h.astype(real), g.astype(real)


def _real(dtype):
    return np.float32 if np.dtype(dtype) == np.dtype(np.complex64) else np.float64


def _analysis(a, axis, h, g):
    n = a.shape[axis]
    i = np.arange(n // 2)
    lo = sum(h[k] * np.take(a, (2 * i + k) % n, axis=axis) for k in range(len(h)))
    hi = sum(g[k] * np.take(a, (2 * i + k) % n, axis=axis) for k in range(len(h)))
    return np.concatenate([lo, hi], axis=axis).astype(a.dtype)


def _synthesis(c, axis, h, g):
    n = c.shape[axis]
    c = np.moveaxis(c, axis, 0)
    lo, hi = c[: n // 2], c[n // 2:]
    out = np.zeros_like(c)
    i = np.arange(n // 2)
    for k in range(len(h)):
        np.add.at(out, (2 * i + k) % n, h[k] * lo + g[k] * hi)
    return np.moveaxis(out, 0, axis).astype(c.dtype)


def _corner(shape, level):
    return tuple(slice(0, s >> level) for s in shape)


def forward(a, wavelet, levels):
    a = np.asarray(a)
    h, g = filters(wavelet, _real(a.dtype))
    out = a.copy()
    for lev in range(levels):
        sub = out[_corner(a.shape, lev)]
        for axis in reversed(range(a.ndim)):
            sub = _analysis(sub, axis, h, g)
        out[_corner(a.shape, lev)] = sub
    return out


def inverse(c, wavelet, levels):
    c = np.asarray(c)
    h, g = filters(wavelet, _real(c.dtype))
    out = c.copy()
    for lev in reversed(range(levels)):
        sub = out[_corner(c.shape, lev)]
        for axis in range(c.ndim):
            sub = _synthesis(sub, axis, h, g)
        out[_corner(c.shape, lev)] = sub
    return out


def detail_mask(shape, levels):
    """True on the detail bands, False on the approximation corner of the deepest level."""
    m = np.ones(shape, dtype=bool)
    m[_corner(shape, levels)] = False
    return m


def soft(c, t):
    """c · max(1 − t/|c|, 0) in c's dtype."""
    real = _real(c.dtype)
    mag = np.abs(c).astype(real)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(mag > real(t), real(1) - real(t) / mag, real(0)).astype(real)
    return (c * s).astype(c.dtype)


def shrink(a, wavelet, levels, t):
    """(coefficients with the detail bands soft-thresholded, Σ|shrunk detail| in float64)."""
    c = forward(a, wavelet, levels)
    d = detail_mask(c.shape, levels)
    if t > 0:
        c[d] = soft(c[d], t)
    return c, float(np.sum(np.abs(c[d].astype(np.complex128))))
