"""The float64 definition of K22 (``dnmf_high_pass_frames``): the spatial high-pass ``high_pass_filter_space`` of the reference
(``Demix/MotionCorrect.py:1262-1270``) -- ``cv2.filter2D`` of a frame with a zero-sum Gaussian disc, ``BORDER_REFLECT``, slice by
slice.  cv2 is not needed: the Gaussian, the correlation and the border are written out.  numpy only; nothing here calls a
library filter."""
import numpy as np


def high_pass_taps(gSig):
    """The (n, n) float64 kernel, :1263-1269 with ``cv2.getGaussianKernel(n, sigma)`` written out (for sigma > 0 OpenCV always takes
    ``exp(-x^2 / (2 sigma^2))`` at ``x = i - (n - 1) / 2``, divided by the sum).  Only entry 0 of ``gSig`` is used.  The operations
    are in OpenCV's order (``scale2X = -0.5 / sigma^2``, ``exp(scale2X x x)``, times the reciprocal of the sum): the rim of the disc
    has exact ties (6^2 + 8^2 = 10^2 at gSig 7) that the last bit decides -- 309 taps in this order."""
    try:
        sigma = float(gSig[0])
    except TypeError:
        sigma = float(gSig)
    n = int((3 * sigma) // 2 * 2 + 1)
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2
    ker = np.exp((-0.5 / (sigma * sigma)) * x * x)
    ker = ker * (1.0 / ker.sum())
    ker2D = np.outer(ker, ker)
    disc = ker2D >= ker2D[:, 0].max()
    out = np.zeros_like(ker2D)
    out[disc] = ker2D[disc] - ker2D[disc].mean()
    return out


def reflect_index(p, N):
    """cv2's borderInterpolate for BORDER_REFLECT (fedcba|abcdefgh|hgfedcb), as often as it takes: period 2 N."""
    m = np.mod(p, 2 * N)
    return np.where(m < N, m, 2 * N - 1 - m)


def filter_frames(frames, taps):
    """frames (..., X, Y, Z) -> the same shape, float64: out[x, y, z] = sum over the NON-ZERO taps (i, j) of
    taps[i, j] in[r_X(x + i - h), r_Y(y + j - h), z].  A tap that is zero is not applied, so a NaN spreads over the support only.
    Also returns S = sum |taps| |in| over the same taps (the scale of the rounding-error bound)."""
    a = np.asarray(frames, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    n = taps.shape[0]
    h = n // 2
    X, Y = a.shape[-3], a.shape[-2]
    out = np.zeros_like(a)
    S = np.zeros_like(a)
    xs, ys = np.arange(X), np.arange(Y)
    for j in range(n):
        iy = reflect_index(ys + j - h, Y)
        for i in range(n):
            if taps[i, j] == 0:
                continue
            ix = reflect_index(xs + i - h, X)
            v = a[..., ix, :, :][..., :, iy, :]
            out += taps[i, j] * v
            S += abs(taps[i, j]) * np.abs(v)
    return out, S


def high_pass_filter_space(img, gSig):
    """(X, Y) or (X, Y, Z) -> the filtered image, float64."""
    a = np.asarray(img, dtype=np.float64)
    if a.ndim == 2:
        return filter_frames(a[..., None], high_pass_taps(gSig))[0][..., 0]
    return filter_frames(a, high_pass_taps(gSig))[0]
