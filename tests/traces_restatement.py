"""The definition of the trace clean-up (K20) in float64, numpy only: what ``Demix/Traces.py::cleanTraces`` of the reference
describes (its body is half-translated MATLAB and does not parse), statement by statement, with MATLAB's defaults pinned where
they are ambiguous (DESIGN.md section 4 lists each).  The kernel (dnmf_amd/csrc/clean_traces.hip), the documents and the tests
refer to this file.

``round(x)`` is ``floor(x + 0.5)``; frame ``t`` (from 0) has the abscissa ``x_t = t + 1``; a window of ``W`` frames around frame
``t`` is ``[t - W // 2, t - W // 2 + W - 1]``, cut at the two ends of the trace."""
import numpy as np

FIT_ITERS = 20       # damped Gauss-Newton steps of the exponential fit
FIT_HALVINGS = 10    # step halvings tried per step
FIT_SLACK = 1e-8     # a step may raise the squared error by this share of it: the comparison never sits on the rounding of a sum
# What the last clean_traces call met at its two thresholds, for tests that must not sit on one: ``tie`` = the smallest
# | |d_t| - thr | / thr over the frames S2 compared (inf without any), ``valid`` = the valid entries of every running median
# S3 counted against 0.1 T.
LAST = dict(tie=np.inf, valid=[])


def mround(v):
    return int(np.floor(v + 0.5))


def _windows(y, W, fill):
    """(T, W): row t holds the window of frame t, ``fill`` where it leaves the trace."""
    T, h = len(y), W // 2
    pad = np.concatenate([np.full(h, fill, y.dtype), y, np.full(max(W - 1 - h, 0), fill, y.dtype)])
    return np.lib.stride_tricks.sliding_window_view(pad, W)[:T]


def _row_median(win):
    """The median of every row's entries that are no NaN (NaN for none); an even count: the mean of the two middle ones."""
    s = np.sort(win, axis=1)                      # NaNs last
    n = (~np.isnan(win)).sum(axis=1)
    rows = np.arange(len(win))
    lo = s[rows, np.maximum((n - 1) // 2, 0)]
    hi = s[rows, np.maximum(n // 2, 0)]
    return np.where(n > 0, 0.5 * (lo + hi), np.nan)


def running_median(y, W, includenan=False):
    """Median over the W frames around every frame.  NaNs are left out (a window without a sample gives NaN); with
    ``includenan`` a window that holds one gives NaN."""
    y = np.asarray(y, np.float64)
    if W < 1:
        return np.full(len(y), np.nan)
    out = _row_median(_windows(y, W, np.nan))
    if includenan:
        out[_windows(np.isnan(y), W, False).any(axis=1)] = np.nan
    return out


def running_mean(y, W):
    """Mean over the W frames around every frame, added from the left; a window with a NaN gives NaN."""
    y = np.asarray(y, np.float64)
    T, h = len(y), W // 2
    t = np.arange(T)
    lo, hi = np.maximum(t - h, 0), np.minimum(t - h + W - 1, T - 1)
    acc = np.zeros(T)
    for j in range(W):                            # the j-th frame of every window
        idx = lo + j
        live = idx <= hi
        acc = np.where(live, acc + y[np.minimum(idx, T - 1)], acc)
    return np.where(hi >= lo, acc / (hi - lo + 1), np.nan)


def prctile(v, p):
    """MATLAB's prctile of the entries that are no NaN: sorted v_0..v_{n-1}, position n p / 100 - 0.5 clamped to [0, n - 1],
    linear interpolation; NaN for none."""
    v = np.sort(np.asarray(v, np.float64)[~np.isnan(v)])
    n = len(v)
    if n == 0:
        return np.nan
    pos = min(max(n * float(p) / 100.0 - 0.5, 0.0), float(n - 1))
    i = int(np.floor(pos))
    j = min(i + 1, n - 1)
    return v[i] + (pos - i) * (v[j] - v[i])


def nanmedian(v):
    v = np.sort(np.asarray(v, np.float64)[~np.isnan(v)])
    n = len(v)
    if n == 0:
        return np.nan
    return v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2])


def _fit_eval(x, y, b):
    """For the decay b: the least-squares amplitude a, the squared error and the Gauss-Newton step of b with a eliminated."""
    with np.errstate(all="ignore"):
        e = np.exp(b * x)
        see, sye, sxee = (e * e).sum(), (y * e).sum(), (x * e * e).sum()
        a, c = sye / see, sxee / see
        res, u = y - a * e, (x - c) * e
        f, num, den = (res * res).sum(), (u * res).sum(), (u * u).sum()
        q = num / (a * den) if a * den != 0.0 else 0.0
    return a, f, (q if np.isfinite(q) else 0.0)


def expfit(x, y):
    """Least-squares ``a exp(b x)`` on the samples (x, y): from the log-linear fit of the positive ones (b = 0 without two of
    them), FIT_ITERS damped Gauss-Newton steps on b with a eliminated; a step is halved until it raises the error by no more
    than FIT_SLACK of it (a comparison without slack would be decided by the rounding of the sums once the steps are small, and
    b would stop at the square root of the precision) and the iteration ends when no halving does.  -> (a, b)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    pos = y > 0
    b = 0.0
    if pos.sum() >= 2:
        dx = x[pos] - x[pos].sum() / pos.sum()
        den = (dx * dx).sum()
        if den > 0:
            b = (dx * (np.log(y[pos]) - np.log(y.max()))).sum() / den
    a, f, db = _fit_eval(x, y, b)
    for _ in range(FIT_ITERS):
        lam, moved = 1.0, False
        for _ in range(FIT_HALVINGS):
            bn = b + lam * db
            an, fn, dbn = _fit_eval(x, y, bn)
            if fn <= f * (1.0 + FIT_SLACK):
                a, b, f, db, moved = an, bn, fn, dbn, True
                break
            lam *= 0.5
        if not moved:
            break
    return a, b


def interp_linear(y):
    """NaNs between two samples lie on the line through the nearest ones; NaNs outside the samples stay."""
    y = np.array(y, np.float64)
    ok = np.flatnonzero(~np.isnan(y))
    if len(ok) == 0:
        return y
    t = np.arange(len(y))
    j = np.searchsorted(ok, t, side="right") - 1          # the last sample at or before t
    inside = np.isnan(y) & (j >= 0) & (j < len(ok) - 1)
    l, r = ok[np.clip(j, 0, len(ok) - 1)], ok[np.clip(j + 1, 0, len(ok) - 1)]
    with np.errstate(all="ignore"):
        slope = (y[r] - y[l]) / np.maximum(r - l, 1)
        fill = slope * (t - l) + y[l]
    y[inside] = fill[inside]
    return y


def _nanmin(v):
    return np.nan if np.isnan(v).all() else np.nanmin(v)


def _nanmax(v):
    return np.nan if np.isnan(v).all() else np.nanmax(v)


def _bleach_curve(y_filt, T):
    """-> (a, b, fitted): the curve of the valid entries of a running median, fitted when more than 0.1 T of them exist."""
    ok = ~np.isnan(y_filt)
    LAST["valid"].append(int(ok.sum()))
    if not ok.sum() > 0.1 * T:
        return np.nan, np.nan, False
    a, b = expfit(np.arange(1, T + 1, dtype=np.float64)[ok], y_filt[ok])
    return a, b, True


def clean_traces(traces, fps, sigma_threshold=10, detrend_mode=2, interp_method=None, smooth_method=None, smooth_window=None,
                 trim=True, floor=0.01):
    """-> (traces (K, T), scales (K,), offsets (K,), info) in float64; ``info``: per-neuron ``a``, ``b``, ``fitted``, ``F0``,
    ``n_outliers``.  The input is not modified."""
    if interp_method is not None and interp_method != "linear":
        raise ValueError(f"interp_method={interp_method!r}: 'linear' or None")
    if smooth_method in ("causal", "high", "low"):
        raise NotImplementedError(f"smooth_method={smooth_method!r} names a filter (causalBandpassFilter / highpassFilter / "
                                  "lowpassFilter) that the reference does not contain")
    if smooth_method is not None and smooth_method not in ("movmean", "movmedian"):
        raise ValueError(f"smooth_method={smooth_method!r}: 'movmean', 'movmedian' or None")
    if smooth_method is not None and smooth_window is not None and int(smooth_window) < 1:
        raise ValueError(f"smooth_window={smooth_window}")
    if detrend_mode not in (0, 1, 2, 3):
        raise ValueError(f"detrend_mode={detrend_mode}")
    x = np.array(traces, dtype=np.float64)
    K, T = x.shape
    xs = np.arange(1, T + 1, dtype=np.float64)
    sigma = 0.0 if sigma_threshold is None else float(sigma_threshold)
    W = mround(10.0 * fps)
    LAST.update(tie=np.inf, valid=[])
    if detrend_mode > 0 and W < 1:
        raise ValueError(f"fps={fps}: a running median over {W} frames")
    with np.errstate(all="ignore"):
        # S1
        x[~np.isfinite(x)] = np.nan
        x[x <= floor] = np.nan
        if trim:
            x[:, :min(mround(fps / 2.0), T)] = np.nan
            x[:, T - 1] = np.nan
        # S2
        n_outliers = np.zeros(K, np.int64)
        if sigma > 0:
            for k in range(K):
                v = x[k]
                ok = ~np.isnan(v)
                n = ok.sum()
                mean = v[ok].sum() / n if n else np.nan
                std = np.sqrt(((v[ok] - mean) ** 2).sum() / (n - 1)) if n > 1 else np.nan
                thr = sigma * std + mean
                d = np.diff(v)
                if T >= 3 and (~np.isnan(d)).any():
                    LAST["tie"] = min(LAST["tie"], np.nanmin(np.abs(np.abs(d) - thr) / abs(thr)))
                if T >= 3:
                    up, down = d > thr, d < -thr
                    extreme = np.flatnonzero((up[:-1] & down[1:]) | (down[:-1] & up[1:])) + 1
                    v[extreme] = np.nan
                    n_outliers[k] = len(extreme)
                x[k] = running_median(v, 3, includenan=True)
        offsets, detrend_offsets, scales = np.zeros(K), np.zeros(K), np.ones(K)
        a, b, fitted, F0 = np.full(K, np.nan), np.full(K, np.nan), np.zeros(K, bool), np.full(K, np.nan)
        # S3
        if detrend_mode > 0:
            for k in range(K):
                F0[k] = prctile(np.where(x[k] > 0.1, x[k], np.nan), 5)
            if detrend_mode == 1:
                offsets = np.array([_nanmin(v) for v in x])
                x = x - offsets[:, None]
                scales = np.array([_nanmax(v) for v in x])
                x = x / scales[:, None]
                s, n = np.zeros(T), np.zeros(T)
                for k in range(K):                 # the mean over the neurons, added in their order
                    ok = ~np.isnan(x[k])
                    s, n = np.where(ok, s + x[k], s), n + ok
                y = np.where(n > 0, s / np.maximum(n, 1), np.nan)
                ga, gb, gfit = _bleach_curve(running_median(y, W), T)
                a[:], b[:], fitted[:] = ga, gb, gfit
                if gfit and gb < 0:
                    x = x - (ga * np.exp(gb * xs))[None, :]
                    detrend_offsets[:] = ga
            else:
                for k in range(K):
                    a[k], b[k], fitted[k] = _bleach_curve(running_median(x[k], W), T)
                    if fitted[k] and b[k] < 0:
                        x[k] = x[k] - a[k] * np.exp(b[k] * xs)
                        detrend_offsets[k] = a[k]
            if detrend_mode == 3:
                F0[:] = nanmedian(F0)
                scales = np.where(F0 < 1, 1.0, F0)
                offsets = np.zeros(K)
                x = x / scales[:, None]
        # S4
        if interp_method == "linear":
            for k in range(K):
                x[k] = interp_linear(x[k])
        # S5
        if smooth_method is not None and smooth_window is not None:
            for k in range(K):
                x[k] = (running_mean(x[k], int(smooth_window)) if smooth_method == "movmean"
                        else running_median(x[k], int(smooth_window), includenan=True))
        # S6
        if detrend_mode < 3:
            new_off = np.array([_nanmin(v) for v in x])
            x = x - new_off[:, None]
            new_scale = np.array([_nanmax(v) for v in x])
            x = x / new_scale[:, None]
            offsets = offsets + (detrend_offsets + new_off) * scales
            scales = scales * new_scale
            x = x * 0.9 + 0.05
    return x, scales, offsets, dict(a=a, b=b, fitted=fitted, F0=F0, n_outliers=n_outliers)
