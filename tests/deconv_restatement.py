"""The definition of the spike deconvolution (K21) in float64, numpy only.  The kernel (dnmf_amd/csrc/deconvolve_traces.hip), the
documents and the tests refer to this file.

Per trace ``y`` of T frames; a frame is valid (w_t = 1) when ``y_t`` is finite, else w_t = 0.

D1  Given g in (0, 1), lam >= 0 and the baseline b, find c >= 0 minimising

        1/2 sum_t w_t (y_t - b - c_t)^2 + lam sum_t s_t,     s_0 = c_0,  s_t = c_t - g c_{t-1} >= 0.

    sum_t s_t = sum_t mu_t c_t with mu_t = 1 - g for t < T - 1 and mu_{T-1} = 1, so with x_t = c_t g^-t this is a weighted isotonic
    regression, solved by pool-adjacent-violators on the per-frame terms a_t = w_t (y_t - b) - lam mu_t and d_t = w_t:
      * a pool that starts at t0 and has l frames carries num = sum_k g^k a_{t0+k} and den = sum_k g^2k d_{t0+k}; its value is
        v = num / den, or -inf when den = 0;
      * pool q after pool p violates when v_q < v_p g^l_p; a pool without a valid frame (den = 0) is never merged INTO (it can
        only be a leading run of missing frames) and always merges backwards into a pool that has one;
      * the merge: num_p += g^l_p num_q, den_p += g^2l_p den_q, l_p += l_q.
    Consequences (tests/test_deconv_host.py checks each): a run of missing frames in the middle or at the end always merges
    backwards, the trace decays through the gap with s = 0; the frames of a leading run of missing frames stay pools of their
    own with c = s = 0 and the first valid frame starts a fresh pool; c_{t0+k} = max(v, 0) g^k; s is exactly 0 inside a pool; at a
    pool start s = max(c_t - g c_{t-1}, 0), and s_0 = c_0.
D2  noise, when not given: 1.4826 median(|d - median d|) / sqrt(2) over d_t = y_{t+1} - y_t of the adjacent valid pairs.
D3  decay, when not given: ac(2) / ac(1), ac(k) = the mean of (y_t - m)(y_{t+k} - m) over the pairs that are both valid, m = the
    mean of the valid frames.
D4  baseline, when not given: the ``baseline_percentile``-th percentile (hazen) of the valid frames.
D5  penalty, when not given: the smallest bracketed lam with RSS(lam) = sum w (y - b - c)^2 >= noise^2 n_valid (``search_penalty``).
D6  refused per trace (ok = False, NaN rows and estimates, nothing raised): fewer than 4 valid frames; fewer than 2 adjacent valid
    pairs when D2 or D3 is needed; ac(1) <= 0 or a decay outside (0, 1); a given penalty < 0 or a given baseline that is not
    finite.
"""
import numpy as np

DOUBLINGS = 64      # D5: at most this many doublings of the upper end
HALVINGS = 32       # D5: halvings of the bracket
MIN_VALID = 4       # D6


def valid_mask(y):
    return np.isfinite(np.asarray(y, np.float64))


def terms(y, g, lam, b):
    """D1's per-frame terms ``(a, d)``."""
    y = np.asarray(y, np.float64)
    w = valid_mask(y)
    T = len(y)
    mu = np.full(T, 1.0 - g)
    mu[T - 1] = 1.0
    a = np.where(w, np.where(w, y, 0.0) - b, 0.0) - lam * mu
    return a, w.astype(np.float64)


def _violates(num_p, den_p, len_p, num_q, den_q, g):
    if den_p <= 0.0:
        return False
    if den_q <= 0.0:
        return True
    return num_q / den_q < (num_p / den_p) * g ** len_p


def pava(a, d, g):
    """Sequential pool-adjacent-violators, frame by frame -> pools as ``(start, length, num, den)`` arrays."""
    a, d, g = [float(v) for v in a], [float(v) for v in d], float(g)
    T = len(a)
    gp = (g ** np.arange(T + 1, dtype=np.float64)).tolist()          # g^l, as ``g ** l`` gives it
    S, L, N, D = [], [], [], []
    for t in range(T):
        s, l, n, dd = t, 1, a[t], d[t]
        while S:
            dp = D[-1]
            if dp <= 0.0:
                break
            if dd > 0.0 and not (n / dd < (N[-1] / dp) * gp[L[-1]]):
                break
            lp = L[-1]
            n = N[-1] + gp[lp] * n
            dd = dp + gp[lp] * gp[lp] * dd
            l = lp + l
            s = S[-1]
            S.pop(), L.pop(), N.pop(), D.pop()
        S.append(s), L.append(l), N.append(n), D.append(dd)
    return np.array(S, np.int64), np.array(L, np.int64), np.array(N, np.float64), np.array(D, np.float64)


def pava_segments(a, d, g, seg, tree=False):
    """The same pools by the kernel's route: PAVA inside every segment of ``seg`` frames on its own, the records in the slots of
    the pool starts (``length`` 0 marks a slot that is no pool start, ``prev`` chains the stack), then a stitch over the segment
    boundaries from the left: the right segment's pools are appended to the stack one by one, merging backwards while they
    violate, until the first one that fits without a merge.  ``tree``: the kernel's order of the stitches -- neighbouring blocks
    of 1, 2, 4, ... segments pairwise, which a level can do side by side."""
    a, d = np.asarray(a, np.float64), np.asarray(d, np.float64)
    T = len(a)
    num, den = a.copy(), d.copy()
    length, prev = np.zeros(T, np.int64), np.full(T, -1, np.int64)

    def violates(p, q):
        return _violates(num[p], den[p], int(length[p]), num[q], den[q], g)

    def merge(p, q):
        gl = g ** int(length[p])
        num[p] += gl * num[q]
        den[p] += gl * gl * den[q]
        length[p] += length[q]
        length[q] = 0

    def settle(p):
        while prev[p] >= 0 and violates(prev[p], p):
            q, p = p, prev[p]
            merge(p, q)
        return p

    tops, firsts, ends = [], [], []
    for c0 in range(0, T, seg):
        c1 = min(T, c0 + seg)
        top = -1
        for t in range(c0, c1):
            length[t], prev[t] = 1, top
            top = settle(t)
        tops.append(top), firsts.append(c0), ends.append(c1)

    def stitch(top, first, end, rtop):
        p, q = top, first
        while q < end:
            if not violates(p, q):
                prev[q] = p
                break
            nxt = q + int(length[q])
            merge(p, q)
            p = settle(p)
            q = nxt
        return p if q >= end else rtop

    n = len(tops)
    if tree:
        step = 1
        while step < n:
            for i in range(0, n - step, 2 * step):
                tops[i] = stitch(tops[i], firsts[i + step], ends[min(i + 2 * step, n) - 1], tops[i + step])
            step *= 2
    else:
        top = tops[0]
        for i in range(1, n):
            top = stitch(top, firsts[i], ends[i], tops[i])
    S = np.flatnonzero(length > 0)
    return S, length[S], num[S], den[S]


def expand(pools, g, T):
    """Pools -> ``(c, s)`` of D1."""
    S, L, N, D = pools
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(D > 0, N / np.where(D > 0, D, 1.0), -np.inf)
    cv = np.maximum(v, 0.0)
    k = np.arange(T) - np.repeat(S, L)
    c = np.repeat(cv, L) * g ** k
    s = np.zeros(T)
    s[S] = np.maximum(c[S] - g * np.concatenate([[0.0], c[S[1:] - 1]]), 0.0)
    s[0] = c[0]
    return c, s


def solve(y, g, lam, b, seg=None, tree=False):
    """D1 for one trace -> ``(c, s, pools)``; ``seg``: by segments of that many frames and a stitch (``tree``: in the kernel's order)."""
    a, d = terms(y, g, lam, b)
    pools = pava(a, d, g) if seg is None else pava_segments(a, d, g, seg, tree)
    c, s = expand(pools, g, len(a))
    return c, s, pools


def rss(y, b, c):
    y = np.asarray(y, np.float64)
    w = valid_mask(y)
    r = np.where(w, y, 0.0) - b - c
    return float(np.sum(np.where(w, r * r, 0.0)))


def percentile(v, p):
    """Hazen: sorted v_0 .. v_{n-1}, position n p / 100 - 0.5 clamped to [0, n - 1], linear interpolation; NaN for none."""
    v = np.sort(np.asarray(v, np.float64))
    n = len(v)
    if n == 0:
        return np.nan
    pos = min(max(n * float(p) / 100.0 - 0.5, 0.0), float(n - 1))
    i = int(np.floor(pos))
    j = min(i + 1, n - 1)
    return float(v[i] + (pos - i) * (v[j] - v[i]))


def adjacent_differences(y):
    y = np.asarray(y, np.float64)
    w = valid_mask(y)
    both = w[1:] & w[:-1]
    return (y[1:] - y[:-1])[both]


def estimate_noise(y):
    """D2; NaN with fewer than 2 adjacent valid pairs."""
    d = adjacent_differences(y)
    if len(d) < 2:
        return np.nan
    return float(1.4826 * np.median(np.abs(d - np.median(d))) / np.sqrt(2.0))


def autocovariances(y):
    """D3's ``(ac(1), ac(2))``; NaN without a pair."""
    y = np.asarray(y, np.float64)
    w = valid_mask(y)
    if not w.any():
        return np.nan, np.nan
    z = np.where(w, y, 0.0) - y[w].mean()
    out = []
    for k in (1, 2):
        both = w[k:] & w[:-k] if len(y) > k else np.zeros(0, bool)
        out.append(float((z[k:] * z[:-k])[both].mean()) if both.any() else np.nan)
    return tuple(out)


def estimate_decay(y):
    ac1, ac2 = autocovariances(y)
    return ac2 / ac1 if ac1 > 0 else np.nan


def estimate_baseline(y, p=10.0):
    y = np.asarray(y, np.float64)
    return percentile(y[valid_mask(y)], p)


def search_penalty(y, g, b, sigma):
    """D5 -> ``(lam, width)``, ``width`` the final width of the bracket (0 when lam = 0)."""
    target = sigma * sigma * int(valid_mask(y).sum())
    if rss(y, b, solve(y, g, 0.0, b)[0]) >= target:
        return 0.0, 0.0
    lo, hi = 0.0, float(sigma)
    for _ in range(DOUBLINGS):
        c = solve(y, g, hi, b)[0]
        if rss(y, b, c) >= target or not (c > 0).any():
            break
        lo, hi = hi, 2.0 * hi
    for _ in range(HALVINGS):
        mid = 0.5 * (lo + hi)
        if rss(y, b, solve(y, g, mid, b)[0]) >= target:
            hi = mid
        else:
            lo = mid
    return hi, hi - lo


def _given(v):
    return v is not None and not np.isnan(v)


def deconvolve(y, g=None, penalty=None, baseline=None, noise=None, baseline_percentile=10.0):
    """One trace -> ``(c, s, info)``; ``info``: g, penalty, baseline, noise, rss, n_valid, n_pools, ok, width."""
    y = np.asarray(y, np.float64)
    T = len(y)
    w = valid_mask(y)
    n_valid = int(w.sum())
    n_pairs = int((w[1:] & w[:-1]).sum()) if T > 1 else 0
    nan = np.full(T, np.nan)
    bad = dict(g=np.nan, penalty=np.nan, baseline=np.nan, noise=np.nan, rss=np.nan, n_valid=n_valid, n_pools=0, ok=False, width=0.0)
    need_noise = not _given(penalty) and not _given(noise)
    if n_valid < MIN_VALID or ((need_noise or not _given(g)) and n_pairs < 2):
        return nan, nan.copy(), bad
    g = float(g) if _given(g) else estimate_decay(y)
    if not (g > 0.0 and g < 1.0):
        return nan, nan.copy(), bad
    b = float(baseline) if _given(baseline) else estimate_baseline(y, baseline_percentile)
    if not np.isfinite(b) or (_given(penalty) and penalty < 0):
        return nan, nan.copy(), bad
    sigma = float(noise) if _given(noise) else estimate_noise(y)
    width = 0.0
    if _given(penalty):
        lam = float(penalty)
    else:
        lam, width = search_penalty(y, g, b, sigma)
    c, s, pools = solve(y, g, lam, b)
    info = dict(g=g, penalty=lam, baseline=b, noise=sigma, rss=rss(y, b, c), n_valid=n_valid, n_pools=len(pools[0]), ok=True,
                width=width)
    return c, s, info


def deconvolve_traces(traces, g=None, penalty=None, baseline=None, noise=None, baseline_percentile=10.0):
    """(K, T) traces -> ``(c, s, info)``; each of the four options: None, a number or K numbers (NaN: estimate)."""
    traces = np.asarray(traces)
    K = len(traces)

    def per(v):
        return [None] * K if v is None else np.broadcast_to(np.asarray(v, np.float64), (K,)).tolist()

    rows = [deconvolve(traces[k], per(g)[k], per(penalty)[k], per(baseline)[k], per(noise)[k], baseline_percentile) for k in range(K)]
    info = {key: np.array([r[2][key] for r in rows]) for key in rows[0][2]} if K else {}
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), info


def kkt(y, g, lam, b, c, s=None):
    """The certificate of D1 that knows nothing of pools -> ``(min s, min grad, max |grad s|)``: with the dense lower-triangular
    K_ij = g^(i-j), c = K s, and the gradient of the objective with respect to s is K^T W (c - (y - b)) + lam.  c solves D1 when
    s >= 0, grad >= 0 and grad s = 0.  ``s``: the spikes that came with c (the caller checks c = K s); without them they are
    c_t - g c_{t-1}, which inside a pool is a rounding of either sign where the solver returns an exact 0."""
    y, c = np.asarray(y, np.float64), np.asarray(c, np.float64)
    T = len(y)
    w = valid_mask(y)
    i = np.arange(T)
    Kmat = np.tril(g ** np.clip(i[:, None] - i[None, :], 0, None).astype(np.float64))
    if s is None:
        s = c - g * np.concatenate([[0.0], c[:-1]])
    s = np.asarray(s, np.float64)
    grad = Kmat.T @ np.where(w, c - (np.where(w, y, 0.0) - b), 0.0) + lam
    return float(s.min()), float(grad.min()), float(np.abs(grad * s).max())
