"""The definition of K30 (``dnmf_temporal_select_*``, ``ops.temporal_quantiles``) and of the images ``robust_images`` builds on it,
in numpy, written plainly.  The kernel (dnmf_amd/csrc/robust_images.hip), the documents and the tests refer to this file.

R1  key.  ``key32`` maps an fp32 value to a 32-bit unsigned key with key(a) < key(b) <=> a < b for finite a, b: the bits with the
    sign bit set for a value >= 0, all bits inverted for a negative one; -0 is +0 first, so the two share a key.
R2  sources.  y[t, v]: the rows of the movie in the order they are given (``frame_ids`` order).  The sequence of voxel v is
      'value'    x_t = y_t;
      'absdev'   x_t = |y_t - c[v]|, c an fp32 image: one fp32 subtraction (round to nearest), then the sign off;
      'absdiff'  x_t = |y_{t+1} - y_t|, the same arithmetic: one term fewer than rows.
R3  omission.  Samples that are not finite (NaN, +-inf; for the two derived sources: the derived value) are left out; n[v]
    counts the others.
R4  ranks.  For a quantile q in [0, 1]: h = q (n - 1) in float64, lo = floor(h), hi = min(lo + 1, n - 1); a_lo and a_hi are the
    kept samples of ranks lo and hi in ascending order, from 0: fp32 input samples (a zero is +0), NaN where n = 0.
R5  value.  The line a_lo + (h - lo)(a_hi - a_lo) in float64, evaluated the way numpy's ``method='linear'`` evaluates it:
    with d = a_hi - a_lo and t = h - lo, a_lo + d t where t < 0.5 and a_hi - d (1 - t) where t >= 0.5.  It equals
    ``np.nanquantile(x[kept], q, method='linear')`` in float64 bit for bit (tests/test_robust_host.py).
R6  images (``robust_images``), all float64 (X, Y, Z):
      median, max      R5 of 'value' at q = 0.5 and q = 1;   n: R3's count of 'value';
      percentile[p]    R5 of 'value' at q = p / 100;
      mad              R5 of 'absdev' at q = 0.5 with c = fp32(median);
      noise            'diff': R5 of 'absdiff' at q = 0.5, times 1.4826 / sqrt(2), the constants of K21's estimate D2
                       (tests/deconv_restatement.py; K21 centres the differences on their median first, this does not: the two
                       differ by at most 1.4826 / sqrt(2) |median of the differences|);  'mad': 1.4826 mad;
      pnr              (max - median) / noise; NaN where noise is 0 or not finite, or n < 2.

``planted_case(seed, Z)`` is the use case the two detection tests share.  A 40 x 36 x Z volume, 48 frames: a floor of 0.2, a
static blob of amplitude 6 and sigma 2, two narrow cells (sigma 1) that are dark but for four isolated frames each, where they
reach 1.5, shot-like noise 0.1 sqrt(signal) N(0, 1) -- 0.045 on the floor, 0.25 on the blob -- and one NaN frame in the corner
voxel.  PLANTED_SEEDS are the first seeds for which the definition alone (this file, tests/detect_restatement.py and
tests/summary_restatement.py in float64) gives: K14 at shape_std 1 on ``pnr`` returns the two cells as its first two picks within
1.5 voxels, and K14 on ``max`` and on the mean returns the static blob first.  With them (tests/test_robust_host.py prints the
figures), image values at cell 0 / cell 1 / the static blob, each at the site's nearest voxel:
      Z = 1, seed 0:  pnr 31.89 / 29.85 / 1.88;   max 1.96 / 1.88 / 6.68;   mean 0.31 / 0.33 / 6.21;   corr 0.86 / 0.87 / 0.12
      Z = 2, seed 0:  pnr 29.96 / 35.67 / 1.99;   max 1.92 / 1.90 / 6.63;   mean 0.32 / 0.33 / 6.18;   corr 0.73 / 0.75 / 0.04
``corr`` (K18's local correlation image) finds both cells at both sizes with these seeds: recorded, not required -- these cells
are a Gaussian of sigma 1, wide enough for neighbours that co-vary.
"""
import math

import numpy as np

NOISE_DIFF_SCALE = 1.4826 / np.sqrt(2.0)      # K21's D2: 1.4826 median(|.|) / sqrt(2)
NOISE_MAD_SCALE = 1.4826
PLANTED_SEEDS = {1: 0, 2: 0}


def key32(x):
    """R1: uint32 keys of fp32 values."""
    x = np.asarray(x, dtype=np.float32)
    u = np.where(x == 0, np.float32(0), x).astype(np.float32).view(np.uint32)
    return np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def from_key32(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k >> np.uint32(31), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def samples(rows, source="value", centre=None, frame_ids=None):
    """R2: rows (T, ...) -> the fp32 sequences, (T, ...) or (T - 1, ...) for 'absdiff'."""
    y = np.asarray(rows, dtype=np.float32)
    if frame_ids is not None:
        y = y[np.asarray(frame_ids, dtype=np.int64)]
    with np.errstate(invalid="ignore", over="ignore"):
        if source == "value":
            return y
        if source == "absdev":
            return np.abs((y - np.asarray(centre, dtype=np.float32).reshape(y.shape[1:])[None]).astype(np.float32))
        if source == "absdiff":
            return np.abs((y[1:] - y[:-1]).astype(np.float32))
    raise ValueError(f"source must be 'value', 'absdev' or 'absdiff', got {source!r}")


def ranks(q, n):
    """R4: (h float64, lo, hi) for the count(s) ``n`` >= 1."""
    n = np.asarray(n, dtype=np.int64)
    h = np.float64(q) * (n - 1).astype(np.float64)
    lo = np.floor(h).astype(np.int64)
    return h, lo, np.minimum(lo + 1, n - 1)


def interpolate(a_lo, a_hi, h, lo):
    """R5."""
    a, b = np.asarray(a_lo, dtype=np.float64), np.asarray(a_hi, dtype=np.float64)
    t = np.asarray(h, dtype=np.float64) - np.asarray(lo, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = b - a
        return np.where(t >= 0.5, b - d * (1.0 - t), a + d * t)


def temporal_quantiles(rows, q, source="value", centre=None, frame_ids=None):
    """rows (T, ...) fp32, q a list of quantiles -> dict(lo, hi (Q, ...) fp32, n (...) int32, value (Q, ...) float64)."""
    q = [float(v) for v in np.atleast_1d(q)]
    assert all(0.0 <= v <= 1.0 for v in q)
    x = samples(rows, source, centre, frame_ids)
    shape = x.shape[1:]
    kept = np.isfinite(x)
    n = kept.sum(0)
    # ascending, the samples left out last; + 0 turns -0 into +0
    srt = np.sort(np.where(kept, x + np.float32(0), np.float32(np.inf)), axis=0) if x.shape[0] else x
    lo_img = np.full((len(q),) + shape, np.nan, dtype=np.float32)
    hi_img = np.full((len(q),) + shape, np.nan, dtype=np.float32)
    val = np.full((len(q),) + shape, np.nan, dtype=np.float64)
    some = n > 0
    if some.any():
        for i, qi in enumerate(q):
            h, lo, hi = ranks(qi, np.where(some, n, 1))
            a = np.take_along_axis(srt, lo[None], 0)[0]
            b = np.take_along_axis(srt, hi[None], 0)[0]
            lo_img[i] = np.where(some, a, np.nan)
            hi_img[i] = np.where(some, b, np.nan)
            val[i] = np.where(some, interpolate(a, b, h, lo), np.nan)
    return dict(lo=lo_img, hi=hi_img, n=n.astype(np.int32), value=val)


def robust_images(video, percentiles=(), noise="diff"):
    """R6: video (T, X, Y, Z) -> dict(median, max, mad, noise, pnr, n, percentile={p: image})."""
    if noise not in ("diff", "mad"):
        raise ValueError(f"noise must be 'diff' or 'mad', got {noise!r}")
    y = np.asarray(video, dtype=np.float32)
    assert y.ndim == 4
    ps = [float(p) for p in percentiles]
    base = temporal_quantiles(y, [0.5, 1.0] + [p / 100.0 for p in ps])
    median, mx, n = base["value"][0], base["value"][1], base["n"]
    mad = temporal_quantiles(y, [0.5], "absdev", centre=median.astype(np.float32))["value"][0]
    if noise == "diff":
        sigma = temporal_quantiles(y, [0.5], "absdiff")["value"][0] * NOISE_DIFF_SCALE
    else:
        sigma = NOISE_MAD_SCALE * mad
    with np.errstate(invalid="ignore", divide="ignore"):
        pnr = np.where(np.isfinite(sigma) & (sigma != 0) & (n >= 2), (mx - median) / sigma, np.nan)
    return dict(median=median, max=mx, mad=mad, noise=sigma, pnr=pnr, n=n,
                percentile={p: base["value"][2 + i] for i, p in enumerate(percentiles)})


def nan_to_min(image):
    """An image as ``detect_points`` searches it: what is not finite replaced by the finite minimum."""
    img = np.array(image, dtype=np.float64)
    ok = np.isfinite(img)
    img[~ok] = img[ok].min()
    return img


PLANTED_SIGMA = 1.0      # the cells' width and the shape_std of the search


def planted_case(seed, Z):
    """-> (video (48, 40, 36, Z) fp32, the two cells' centres (2, 3), the static blob's centre (3,), shape_std)."""
    sz, T = (40, 36, Z), 48
    rng = np.random.RandomState(seed)
    g = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sz], indexing="ij")

    def blob(c, sigma):
        return np.exp(-((g[0] - c[0]) ** 2 + (g[1] - c[1]) ** 2 + (g[2] - c[2]) ** 2) / sigma ** 2)

    cells = np.array([[10.0, 9.0, 0.0], [28.0, 25.0, float(Z - 1)]])
    still = np.array([12.0, 27.0, 0.0])
    signal = np.broadcast_to(0.2 + 6.0 * blob(still, 2.0), (T,) + sz).copy()
    # four isolated frames a cell: no two of them adjacent, none shared
    frames = rng.permutation(np.arange(1, T - 1, 2))[:8]
    for c, on in zip(cells, (frames[:4], frames[4:])):
        signal[on] += 1.5 * blob(c, PLANTED_SIGMA)[None]
    video = signal + 0.1 * np.sqrt(signal) * rng.randn(T, *sz)
    video[7, 0, 0, 0] = np.nan
    return video.astype(np.float32), cells, still, PLANTED_SIGMA


def nearest_voxel(c):
    return tuple(int(math.floor(v + 0.5)) for v in c)
