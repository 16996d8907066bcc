"""The definition of the component statistics (K24) and of the component evaluation built on them, in float64 numpy.

Everything lives in footprint coordinates.  For neuron k: a box ``(x0, x1, y0, y1, z0, z1)``, inclusive, of n voxels u in the
order x slowest, z fastest, and the footprint values a(u) = A_rows[k, u].  For frame t

    e_t(u) = (frames_t(u) - sub_t(u)) + a(u) C[k, t]        (frames_t(u) alone without ``sub``)

the residual with the neuron's own contribution put back.  Per (k, t) the three sums over the box -- sum e, sum e^2, sum a e --
and per k ``foot`` = (n, sum a, sum a^2) give

    frame_corr[k, t] = Pearson of a and e_t       raw[k, t] = (n sum ae - sum a sum e) / (n sum a^2 - (sum a)^2)

both NaN where a variance -- n sum x^2 - (sum x)^2 -- is not positive.  With weights w (K, T) >= 0

    image[k](u) = sum_t w[k, t] e_t(u) / sum_t w[k, t]        r_values[k] = Pearson of a and image[k]

NaN where the weights sum to 0 or a variance is not positive.  An (k, t) whose box holds a sample that is not finite is
invalid: its sums, frame_corr and raw are NaN, and it takes no part in image[k].

The Pearson correlation is evaluated from the sums, as the kernel does; the cancellation in n sum x^2 - (sum x)^2 loses
log10(mean square / variance) digits, so ``component_stats(check=True)`` asserts that on every box the variance of a, of every
valid e_t and of the image is either exactly zero (the NaN cases) or at least ``MIN_SPREAD`` of the mean square.
"""
import math

import numpy as np

MIN_SPREAD = 1e-6


def box_voxels(box, sz):
    """Flat voxel indices p = (x Y + y) Z + z of the box, x slowest, z fastest."""
    X, Y, Z = (int(s) for s in sz)
    x0, x1, y0, y1, z0, z1 = (int(b) for b in box)
    assert 0 <= x0 <= x1 < X and 0 <= y0 <= y1 < Y and 0 <= z0 <= z1 < Z, (box, sz)
    x, y, z = np.meshgrid(np.arange(x0, x1 + 1), np.arange(y0, y1 + 1), np.arange(z0, z1 + 1), indexing="ij")
    return ((x * Y + y) * Z + z).reshape(-1)


def pearson_from_sums(n, sa, saa, sb, sbb, sab):
    va, vb = n * saa - sa * sa, n * sbb - sb * sb
    if not (va > 0.0) or not (vb > 0.0):
        return math.nan
    return (n * sab - sa * sb) / math.sqrt(va * vb)


def _spread_ok(n, s1, s2):
    var = n * s2 - s1 * s1
    return var == 0.0 or var >= MIN_SPREAD * n * s2


def component_stats(frames, sz, A_rows, boxes, C, w, sub=None, check=True):
    """frames (T, P), A_rows (K, P), boxes (K, 6), C and w (K, T), sub (T, P) or None -> dict of float64 arrays: ``sums`` (K, T, 3),
    ``foot`` (K, 3), ``frame_corr`` and ``raw`` (K, T), ``image`` (K, vmax; NaN past a box's n), ``r_values`` (K), and what
    the image is made of: ``image_sums`` (K, vmax), ``wsum`` (K).  ``*_mag``: the sums of the magnitudes of the terms of
    ``sums``, ``foot`` and ``image_sums``, the scale their rounding is measured on."""
    frames = np.asarray(frames, dtype=np.float64)
    A_rows = np.asarray(A_rows, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    sub = None if sub is None else np.asarray(sub, dtype=np.float64)
    boxes = np.asarray(boxes)
    K, T = C.shape
    assert w.shape == (K, T) and A_rows.shape[0] == K and boxes.shape == (K, 6) and frames.shape[0] == T
    assert np.all(w >= 0) and np.all(np.isfinite(w))
    vox = [box_voxels(b, sz) for b in boxes]
    vmax = max(v.size for v in vox)
    out = dict(sums=np.full((K, T, 3), np.nan), foot=np.zeros((K, 3)), frame_corr=np.full((K, T), np.nan),
               raw=np.full((K, T), np.nan), image=np.full((K, vmax), np.nan), r_values=np.full(K, np.nan),
               image_sums=np.full((K, vmax), np.nan), wsum=np.zeros(K), sums_mag=np.zeros((K, T, 3)), foot_mag=np.zeros((K, 3)),
               image_sums_mag=np.zeros((K, vmax)))
    for k in range(K):
        u = vox[k]
        n = float(u.size)
        a = A_rows[k, u]
        sa, saa = a.sum(), (a * a).sum()
        out["foot"][k] = n, sa, saa
        out["foot_mag"][k] = n, np.abs(a).sum(), saa
        if check:
            assert _spread_ok(n, sa, saa), f"footprint {k}: variance below {MIN_SPREAD} of the mean square"
        va = n * saa - sa * sa
        acc, mag, wsum = np.zeros(u.size), np.zeros(u.size), 0.0
        with np.errstate(invalid="ignore"):
            for t in range(T):
                e = frames[t, u] if sub is None else frames[t, u] - sub[t, u]
                e = e + a * C[k, t]
                if not np.all(np.isfinite(e)):
                    continue
                se, see, sae = e.sum(), (e * e).sum(), (a * e).sum()
                out["sums"][k, t] = se, see, sae
                out["sums_mag"][k, t] = np.abs(e).sum(), see, np.abs(a * e).sum()
                if check:
                    assert _spread_ok(n, se, see), f"e of neuron {k}, frame {t}: variance below {MIN_SPREAD} of the mean square"
                out["frame_corr"][k, t] = pearson_from_sums(n, sa, saa, se, see, sae)
                if va > 0.0:
                    out["raw"][k, t] = (n * sae - sa * se) / va
                if w[k, t] != 0.0:
                    acc += w[k, t] * e
                    mag += w[k, t] * np.abs(e)
                    wsum += w[k, t]
        out["image_sums"][k, :u.size], out["image_sums_mag"][k, :u.size], out["wsum"][k] = acc, mag, wsum
        if wsum > 0.0:
            m = acc / wsum
            out["image"][k, :u.size] = m
            if check:
                assert _spread_ok(n, m.sum(), (m * m).sum()), f"image {k}: variance below {MIN_SPREAD} of the mean square"
            out["r_values"][k] = pearson_from_sums(n, sa, saa, m.sum(), (m * m).sum(), (a * m).sum())
    return out


# ---- which frames count as active --------------------------------------------------------------------------------------------
def leave_one_out_score(C):
    """l[k, t] = (C[k, t-1] + C[k, t+1]) / 2 over the frames served, in time order; at the two ends the one neighbour that
    exists (a single frame: its own value)."""
    C = np.asarray(C, dtype=np.float64)
    T = C.shape[1]
    if T == 1:
        return C.copy()
    s = np.empty_like(C)
    s[:, 1:-1] = 0.5 * (C[:, :-2] + C[:, 2:])
    s[:, 0], s[:, -1] = C[:, 1], C[:, -2]
    return s


def n_active(active, T):
    return min(T, max(1, int(math.ceil(active * T))))


def active_weights(score, active):
    """w (K, T): 1 on the ``ceil(active T)`` frames with the largest score of each row, ties to the lower t; else 0."""
    score = np.asarray(score, dtype=np.float64)
    K, T = score.shape
    m = n_active(active, T)
    w = np.zeros((K, T))
    for k in range(K):
        order = sorted(range(T), key=lambda t: (-score[k, t], t))
        w[k, order[:m]] = 1.0
    return w


# ---- the signal-to-noise figure ------------------------------------------------------------------------------------------------
def noise_mad(x):
    """MAD(diff(x)) / (0.6745 sqrt 2): the noise of a trace whose signal changes slowly (the estimator K21 documents)."""
    d = np.diff(np.asarray(x, dtype=np.float64))
    return np.median(np.abs(d - np.median(d))) / (0.6745 * math.sqrt(2.0))


def snr(raw, w):
    """(mean of raw[k, active and valid] - median of raw[k, valid]) / noise_k; NaN with fewer than 4 valid frames, without a
    valid active frame or with a zero noise."""
    raw = np.asarray(raw, dtype=np.float64)
    K = raw.shape[0]
    out = np.full(K, np.nan)
    for k in range(K):
        ok = np.isfinite(raw[k])
        act = ok & (np.asarray(w)[k] > 0)
        if ok.sum() < 4 or not act.any():
            continue
        noise = noise_mad(raw[k, ok])
        if noise > 0.0:
            out[k] = (raw[k, act].mean() - np.median(raw[k, ok])) / noise
    return out


def component_boxes(A, sz, floor=1e-3, margin=2):
    """(K, 6) per neuron the bounding box of A[:, k] > floor max A[:, k], grown by ``margin`` and cut to the volume.  A (P, K)."""
    X, Y, Z = (int(s) for s in sz)
    A = np.asarray(A, dtype=np.float64).reshape(X, Y, Z, -1)
    K = A.shape[-1]
    boxes = np.zeros((K, 6), dtype=np.int32)
    for k in range(K):
        on = A[..., k] > floor * A[..., k].max()
        for d, S in enumerate((X, Y, Z)):
            idx = np.nonzero(on.any(axis=tuple(i for i in range(3) if i != d)))[0]
            boxes[k, 2 * d] = max(0, idx.min() - margin)
            boxes[k, 2 * d + 1] = min(S - 1, idx.max() + margin)
    return boxes


def evaluate(frames, sz, A, C, active=0.25, margin=2, floor=1e-3, min_r=0.5, min_snr=1.0, sub=None, selection="loo", check=True):
    """The whole evaluation on registered frames (T, P), footprints A (P, K) and traces C (K, T): boxes, active frames by the
    leave-one-out score (``selection='top'``: by C itself, the biased choice), statistics, snr and keep."""
    A = np.asarray(A, dtype=np.float64)
    boxes = component_boxes(A, sz, floor, margin)
    w = active_weights(leave_one_out_score(C) if selection == "loo" else np.asarray(C, dtype=np.float64), active)
    st = component_stats(frames, sz, A.T, boxes, C, w, sub=sub, check=check)
    st["snr"] = snr(st["raw"], w)
    st["boxes"], st["w"] = boxes, w
    with np.errstate(invalid="ignore"):
        st["keep"] = (st["r_values"] >= min_r) & (st["snr"] >= min_snr)
    return st


# ---- the planted video -----------------------------------------------------------------------------------------------------------
CELLS = np.array([[5.0, 4.0], [5.0, 14.0], [12.0, 5.0], [12.0, 15.0], [19.0, 4.0], [19.0, 14.0]])
SPURIOUS = np.array([[8.5, 9.5], [15.5, 9.5]])       # between the cells


def planted_centres(depth):
    z = 0.5 * (depth - 1)
    return np.concatenate([np.concatenate([CELLS, SPURIOUS]), np.full((8, 1), z)], axis=1)


def gaussian_footprints(sz, centres, sigma=3.0):
    """(P, K): exp(-|u - centre|^2 / sigma^2), the footprints the model builds."""
    X, Y, Z = sz
    g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    d2 = ((g[:, None, :] - np.asarray(centres)[None, :, :]) ** 2).sum(-1)
    return np.exp(-d2 / sigma ** 2)


def planted_video(depth, T, seed, noise=0.3, g=0.74, rate=0.12):
    """Six Gaussian cells (sigma 3) with AR(1) traces (decay g, spikes of height 1..2 at ``rate`` a frame) and white noise, clamped
    at 0, in a 24 x 20 x depth volume -> ``(video (T, P), A8 (P, 8), traces (6, T), sz)``: A8 the eight-column model whose last
    two columns sit between the cells, on nothing."""
    rng = np.random.default_rng([seed, depth, T])
    sz = (24, 20, depth)
    A8 = gaussian_footprints(sz, planted_centres(depth))
    spikes = (rng.random((6, T)) < rate) * rng.uniform(1.0, 2.0, (6, T))
    spikes[:, 0] += rng.uniform(0.0, 1.0, 6)
    traces = np.zeros((6, T))
    for t in range(T):
        traces[:, t] = (g * traces[:, t - 1] if t else 0.0) + spikes[:, t]
    video = traces.T @ A8[:, :6].T + noise * rng.standard_normal((T, A8.shape[0]))
    return np.maximum(video, 0.0), A8, traces, sz


def nnls_traces(video, A):
    """The exact non-negative least-squares traces of every frame, (K, T)."""
    from scipy.optimize import nnls
    return np.stack([nnls(A, y)[0] for y in video], axis=1)
