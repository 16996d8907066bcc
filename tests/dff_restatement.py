"""The definition of K31 (``dnmf_running_quantile`` / ``dnmf_baseline_apply``, ``ops.running_quantile`` / ``ops.baseline_apply``):
the running-percentile baseline of a movie and the movie read against it, in numpy float64, written plainly.  The kernels
(dnmf_amd/csrc/running_baseline.hip), the documents and the tests refer to this file.

D1  plan.  T frames, a window of W >= 1 frames, a stride S with 1 <= S <= W, integers throughout: J = 1 if T <= W, else
    ceil((T - W) / S) + 1.  Window j holds the frames [s_j, e_j), s_j = min(j S, max(T - W, 0)), e_j = min(s_j + W, T): the last
    window ends at T and is full-length whenever T >= W.  Its knot sits at c_j = (s_j + e_j - 1) / 2; the c_j increase strictly.
D2  knot.  Per voxel and window the quantile q of the window's finite samples, exactly K30's (tests/robust_restatement.py R3 - R5):
    n_j of them, lo and hi the kept samples of ranks floor(h) and min(floor(h) + 1, n_j - 1), h = q (n_j - 1), and the value b_j
    their float64 interpolation as np.nanquantile(method='linear') evaluates it; NaN where n_j < min_samples (>= 1).
D3  baseline.  F0_t = b_0 for t <= c_0 and b_{J-1} for t >= c_{J-1}; else with c_j <= t < c_{j+1} and
    w = (t - c_j) / (c_{j+1} - c_j) in float64: b_j where w = 0, else b_j + w (b_{j+1} - b_j), every operation rounded once.  A NaN
    knot spreads through this arithmetic and nowhere else.
D4  output, in float64 from the fp32 sample y and F0_t, rounded once to fp32:  'baseline' F0;  'df' y - F0;
    'dff' (y - F0) / (F0 + offset);  'dfsqrtf' (y - F0) / sqrt(F0 + offset).  NaN where y or F0 is not finite and, in the last
    two, where F0 + offset <= 0.

``bleaching_trace`` and ``bleaching_case`` are the planted use cases of tests/test_dff_host.py and tests/test_gpu_dff.py.
"""
import numpy as np

import robust_restatement as RR

MODES = ("baseline", "df", "dff", "dfsqrtf")
MAX_WINDOW = 2048


def window_plan(T, W, S):
    """D1 -> dict(J, starts, ends (J,) int64, centres (J,) float64)."""
    T, W, S = int(T), int(W), int(S)
    assert T >= 1 and W >= 1 and 1 <= S <= W
    J = 1 if T <= W else -((W - T) // S) + 1
    starts = np.minimum(np.arange(J, dtype=np.int64) * S, max(T - W, 0))
    ends = np.minimum(starts + W, T)
    return dict(J=J, starts=starts, ends=ends, centres=(starts + ends - 1).astype(np.float64) / 2.0)


def running_quantile(rows, W, S, q, min_samples=1, frame_ids=None):
    """D2: rows (T, ...) fp32 in time order -> dict(lo, hi (J, ...) fp32, n (J, ...) int32, value (J, ...) float64, centres,
    starts, ends)."""
    y = np.asarray(rows, dtype=np.float32)
    if frame_ids is not None:
        y = y[np.asarray(frame_ids, dtype=np.int64)]
    plan = window_plan(y.shape[0], W, S)
    lo, hi, n, value = [], [], [], []
    for s, e in zip(plan["starts"], plan["ends"]):
        r = RR.temporal_quantiles(y[s:e], [q])
        lo.append(r["lo"][0]), hi.append(r["hi"][0]), n.append(r["n"])
        value.append(np.where(r["n"] >= min_samples, r["value"][0], np.nan))
    return dict(lo=np.stack(lo), hi=np.stack(hi), n=np.stack(n), value=np.stack(value), centres=plan["centres"],
                starts=plan["starts"], ends=plan["ends"])


def baseline(value, centres, t):
    """D3: knots value (J, ...) float64 at centres (J,) -> F0 (len(t), ...) float64 at the frames t."""
    b = np.asarray(value, dtype=np.float64)
    c = np.asarray(centres, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    J = len(c)
    out = np.empty((len(t),) + b.shape[1:], dtype=np.float64)
    for i, ti in enumerate(t):
        j = int(np.searchsorted(c, ti, side="right")) - 1
        if j < 0:
            out[i] = b[0]
        elif j >= J - 1:
            out[i] = b[J - 1]
        else:
            w = (ti - c[j]) / (c[j + 1] - c[j])
            with np.errstate(invalid="ignore", over="ignore"):
                out[i] = b[j] if w == 0 else b[j] + w * (b[j + 1] - b[j])
    return out


def apply(rows, value, centres, mode="dff", offset=0.0, frame_ids=None, row0=0):
    """D4: rows (B, ...) fp32, the frames row0 .. row0 + B - 1 -> (out fp32, out float64 before the last rounding)."""
    assert mode in MODES
    y = np.asarray(rows, dtype=np.float32)
    if frame_ids is not None:
        y = y[np.asarray(frame_ids, dtype=np.int64)]
    f0 = baseline(value, centres, row0 + np.arange(y.shape[0]))
    yd = y.astype(np.float64)
    ok = np.isfinite(yd) & np.isfinite(f0)
    with np.errstate(all="ignore"):
        if mode == "baseline":
            r = f0
        elif mode == "df":
            r = yd - f0
        else:
            den = f0 + np.float64(offset)
            ok &= den > 0
            r = (yd - f0) / (den if mode == "dff" else np.sqrt(den))
        r = np.where(ok, r, np.nan)
        return r.astype(np.float32), r


def dff_movie(rows, W, S, q, mode="dff", offset=0.0, min_samples=1):
    """The whole of it -> (movie fp32, knots dict)."""
    knots = running_quantile(rows, W, S, q, min_samples)
    return apply(rows, knots["value"], knots["centres"], mode, offset)[0], knots


def bleaching_trace(T=600, B=10.0, tau=300.0, every=40, amplitude=5.0, seed=0):
    """-> (y (T,) fp32, planted baseline (T,) float64, transient mask (T,)): B exp(-t / tau) plus non-negative transients of one
    frame, one every ``every`` frames at a seeded phase."""
    rng = np.random.RandomState(seed)
    t = np.arange(T, dtype=np.float64)
    base = B * np.exp(-t / tau)
    on = np.zeros(T, dtype=bool)
    on[rng.randint(0, every) + np.arange(0, T - every, every)] = True
    y = base + np.where(on, amplitude * (0.5 + rng.rand(T)), 0.0)
    return y.astype(np.float32), base.astype(np.float32).astype(np.float64), on


BLEACH_FRAMES, BLEACH_WINDOW, BLEACH_STRIDE = 240, 60, 15
BLEACH_SEEDS = {1: 0, 2: 0}


def bleaching_case(seed, Z):
    """-> (video (240, 40, 36, Z) fp32, the two cells' centres (2, 3), the static blob's centre (3,), shape_std): K30's planted
    cells (tests/robust_restatement.py: a floor of 0.2, a static blob of amplitude 6, two narrow cells dark but for isolated
    frames where they reach 1.5, shot-like noise, one NaN sample) with eight firing frames a cell, at least 24 frames apart, and
    everything that is not a transient -- floor and blob -- halving over the session."""
    sz, T = (40, 36, Z), BLEACH_FRAMES
    rng = np.random.RandomState(seed)
    g = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sz], indexing="ij")

    def blob(c, sigma):
        return np.exp(-((g[0] - c[0]) ** 2 + (g[1] - c[1]) ** 2 + (g[2] - c[2]) ** 2) / sigma ** 2)

    cells = np.array([[10.0, 9.0, 0.0], [28.0, 25.0, float(Z - 1)]])
    still = np.array([12.0, 27.0, 0.0])
    decay = 0.5 ** (np.arange(T, dtype=np.float64) / T)
    signal = decay[:, None, None, None] * (0.2 + 6.0 * blob(still, 2.0))[None]
    for c, phase in zip(cells, (5, 17)):
        on = phase + 28 * np.arange(8) + rng.randint(0, 4, 8)
        signal[on] += 1.5 * blob(c, RR.PLANTED_SIGMA)[None]
    video = signal + 0.1 * np.sqrt(signal) * rng.randn(T, *sz)
    video[7, 0, 0, 0] = np.nan
    return video.astype(np.float32), cells, still, RR.PLANTED_SIGMA
