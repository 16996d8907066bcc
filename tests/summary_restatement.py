"""The definition of K18 (``dnmf_summary_images``) in float64 numpy, written plainly: the summary images of a video.

x[t, p]: T frames of a volume (X, Y, Z), voxel p = (x Y + y) Z + z.  With ``sub`` the input is the fp32 difference
``frames - sub`` (rounded once, to fp32).  Per voxel, over the T frames:

mean, std  two passes in float64: the mean, then the centred sum of squares over T (the population value, ddof = 0).
max        the largest sample.
corr       the mean, over the valid neighbours q of p, of the Pearson correlation of the two time series.  'face': the
           voxels that differ by +-1 on one axis (6; 4 at Z = 1); 'full': by at most 1 on every axis (26; 8 at Z = 1).  An
           axis of extent 1 has no neighbours along it; neighbours outside the volume do not exist (no padding, no wrap).
           A pair is valid when both voxels are finite in every frame and both variances are > 0.  A voxel without a valid
           pair gets NaN.
A voxel with a sample that is not finite in any frame is NaN in all four images and is nobody's neighbour.

The kernel accumulates one pass in float64 on d = x - x0, x0 = the voxel's value in the first frame (exact in float64):
sum d, sum d^2, sum d_p d_q; var = max(0, (sum d^2 - (sum d)^2 / T) / T).  The pivot makes the variance of a constant voxel
exactly 0, which it also is here.
"""
import itertools

import numpy as np


def offsets(neighbours, shape):
    """The (dx, dy, dz) of a neighbourhood in a volume of ``shape``: none along an axis of extent 1."""
    if neighbours not in ("face", "full"):
        raise ValueError(f"neighbours must be 'face' or 'full', got {neighbours!r}")
    out = []
    for d in itertools.product((-1, 0, 1), repeat=3):
        n = sum(abs(v) for v in d)
        if n == 0 or (neighbours == "face" and n != 1):
            continue
        if any(v != 0 and s == 1 for v, s in zip(d, shape)):
            continue
        out.append(d)
    return out


def input_rows(frames, sub=None):
    """(T, X, Y, Z) float64 of the fp32 values the kernel sees."""
    x = np.asarray(frames, dtype=np.float32)
    if sub is not None:
        with np.errstate(invalid="ignore"):
            x = (x - np.asarray(sub, dtype=np.float32)).astype(np.float32)
    return x.astype(np.float64)


def summary_images(frames, neighbours="full", sub=None):
    """frames (T, X, Y, Z) -> dict(mean, std, max, corr) of float64 (X, Y, Z) arrays."""
    x = input_rows(frames, sub)
    assert x.ndim == 4
    T, shape = x.shape[0], x.shape[1:]
    ok = np.isfinite(x).all(0)
    xs = np.where(ok[None], x, 0.0)
    mean = xs.sum(0) / T
    c = xs - mean[None]
    var = (c * c).sum(0) / T
    std = np.sqrt(var)
    mx = xs.max(0)
    use = ok & (var > 0)
    acc = np.zeros(shape)
    cnt = np.zeros(shape, dtype=np.int64)
    X, Y, Z = shape
    for dx, dy, dz in offsets(neighbours, shape):
        for i in range(max(0, -dx), min(X, X - dx)):
            for j in range(max(0, -dy), min(Y, Y - dy)):
                for k in range(max(0, -dz), min(Z, Z - dz)):
                    q = (i + dx, j + dy, k + dz)
                    if use[i, j, k] and use[q]:
                        cov = (c[:, i, j, k] * c[(slice(None),) + q]).sum() / T
                        acc[i, j, k] += cov / (std[i, j, k] * std[q])
                        cnt[i, j, k] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        corr = np.where(cnt > 0, acc / cnt, np.nan)
    nan = np.nan
    return dict(mean=np.where(ok, mean, nan), std=np.where(ok, std, nan), max=np.where(ok, mx, nan), corr=np.where(ok, corr, nan))


def planted_video(sz=(40, 36, 2), T=48, sigma=2.0, seed=5):
    """The use case both test files share: two Gaussian blobs with independent on/off traces and equal time-averaged
    brightness, on a static background that carries a third, constant blob brighter than both, plus small white noise.
    -> (video (T, X, Y, Z) fp32, active centres (2, 3), the constant blob's centre (3,), sigma)."""
    rng = np.random.RandomState(seed)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in sz], indexing="ij")

    def blob(c):
        return np.exp(-((g[0] - c[0]) ** 2 + (g[1] - c[1]) ** 2 + (g[2] - c[2]) ** 2) / sigma ** 2)

    active = np.array([[10.0, 9.0, 0.0], [28.0, 25.0, 1.0]])
    still = np.array([12.0, 27.0, 0.0])
    # on in half of the frames each, in patterns that are uncorrelated over the 48 frames
    on = np.stack([rng.permutation(T) < T // 2, rng.permutation(T) < T // 2]).astype(np.float64)
    video = 0.2 + 3.0 * blob(still)[None] + 0.01 * rng.randn(T, *sz)
    for c, tr in zip(active, on):
        video = video + 2.0 * tr[:, None, None, None] * blob(c)[None]       # time average 1.0 each
    return video.astype(np.float32), active, still, sigma
