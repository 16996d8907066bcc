"""The colour update of a multi-channel model (K29) in plain numpy float64: the definition csrc/colours.hip is held to, with
the sums in the kernel's order.

Channel c of frame t is modelled as sum_k colours[c, k] A_t[:, k] C[k, t], A_t the UNCOLOURED warped footprints.  With G_t =
A_t^T A_t and r_t^c = A_t^T y_t^c the squared error of channel c is 1/2 x^T M x - b_c^T x + const in x = colours[c, :]:

    M[k, l] = sum_t G_t[k, l] C[k, t] C[l, t]          b[c, k] = sum_t r_t^c[k] C[k, t]

``normal_eqs`` forms them, ``solve`` runs the cyclic coordinate sweeps, ``normalise`` fixes the scale freedom between a neuron's
colours and its trace, ``update`` is the three in a row.
"""
import numpy as np

SEG = 32          # frames of a segment: a segment is summed from 0.0 in the order of t, the segments are added in their order


def normal_eqs(G, r, C):
    """``G`` (B, K, K), ``r`` (NC, B, K), ``C`` (K, B) -> ``(M (K, K), b (NC, K), Mabs, babs)`` in float64; the last two are the
    sums of the terms' magnitudes, the scale of the rounding error of the first two."""
    G, r, C = (np.asarray(v, dtype=np.float64) for v in (G, r, C))
    B, K, _ = G.shape
    NC = r.shape[0]
    M, b = np.zeros((K, K)), np.zeros((NC, K))
    Mabs, babs = np.zeros((K, K)), np.zeros((NC, K))
    for s in range(0, B, SEG):
        pM, pb = np.zeros((K, K)), np.zeros((NC, K))
        for t in range(s, min(B, s + SEG)):
            tM = G[t] * (C[:, t][:, None] * C[:, t][None, :])
            tb = r[:, t, :] * C[:, t][None, :]
            pM, pb = pM + tM, pb + tb
            Mabs, babs = Mabs + np.abs(tM), babs + np.abs(tb)
        M, b = M + pM, b + pb
    return M, b, Mabs, babs


def kkt(M, b, x):
    """(NC): max_k |pg_k|, pg_k = (M x - b)[k] where x_k > 0, else min((M x - b)[k], 0), as hals_restatement.kkt; zero exactly at
    the solution.  ``x`` (NC, K)."""
    g = np.asarray(x, dtype=np.float64) @ np.asarray(M, dtype=np.float64).T - b
    return np.abs(np.where(x > 0, g, np.minimum(g, 0.0))).max(axis=1)


def solve(M, b, colours, sweeps):
    """``sweeps`` cyclic sweeps of x_k <- max(0, x_k + (b_k - M[k, :] x) / M[k, k]) per channel, from ``colours`` (NC, K), with
    the running h = M x updated by row k of M (M is symmetric) -> ``(x (NC, K), kkt (NC), ok (NC) bool)``.  A coordinate whose
    M[k, k] is not a positive finite number is left alone.  A channel whose b, or the shared M, holds an entry that is not
    finite keeps its row: ok False, kkt NaN."""
    M, b = np.asarray(M, dtype=np.float64), np.asarray(b, dtype=np.float64)
    x = np.array(colours, dtype=np.float64)
    NC, K = x.shape
    ok = np.isfinite(M).all() & np.isfinite(b).all(axis=1)
    out_kkt = np.full(NC, np.nan)
    for c in np.nonzero(ok)[0]:
        xc = x[c]
        h = np.zeros(K)
        for k in range(K):
            h = h + M[k, :] * xc[k]
        for _ in range(int(sweeps)):
            for k in range(K):
                d = M[k, k]
                if not (d > 0.0 and np.isfinite(d)):
                    continue
                xn = np.fmax(0.0, xc[k] + (b[c, k] - h[k]) / d)
                delta = xn - xc[k]
                if delta != 0.0:
                    h = h + delta * M[k, :]
                    xc[k] = xn
        g = h - b[c]
        out_kkt[c] = np.abs(np.where(xc > 0, g, np.minimum(g, 0.0))).max()
    return x, out_kkt, ok


def normalise(new, old, C, diag=None):
    """The largest colour of every neuron becomes 1: with s_k = max_c new[c, k] finite and positive, ``colours[:, k] = new[:, k]
    / s_k`` and ``C[k, :] *= s_k``; a neuron whose new colours are all zero or not finite, or whose ``diag[k]`` = M[k, k] is not a
    positive finite number (nothing was learnt about it: the sweeps left it alone), keeps its ``old`` column and its trace and
    has ``ok[k]`` False -> ``(colours, C, scale (K), ok (K) bool)``; scale is 1 where ok is False."""
    new, old, C = (np.array(v, dtype=np.float64) for v in (new, old, C))
    with np.errstate(invalid="ignore"):
        s = new.max(axis=0)
        ok = np.isfinite(new).all(axis=0) & np.isfinite(s) & (s > 0)
        if diag is not None:
            ok &= np.isfinite(diag) & (np.asarray(diag) > 0)
    scale = np.where(ok, s, 1.0)
    colours = np.where(ok[None, :], new / scale[None, :], old)
    return colours, C * scale[:, None], scale, ok


def objective(M, b, x):
    """sum over the channels of 1/2 x^T M x - b^T x: the squared error up to a constant and a factor 2."""
    x = np.asarray(x, dtype=np.float64)
    return float((0.5 * np.einsum("ck,kl,cl->c", x, M, x) - (b * x).sum(axis=1)).sum())


def update(G, r, C, colours, sweeps=10, normalise_=True):
    """One colour update -> dict(colours, C, M, b, kkt, ok, ok_channel, scale)."""
    M, b, _, _ = normal_eqs(G, r, C)
    x, k, okc = solve(M, b, colours, sweeps)
    x = np.where(okc[:, None], x, np.asarray(colours, dtype=np.float64))
    if normalise_:
        col, Cn, scale, ok = normalise(x, colours, C, np.diag(M))
    else:
        d = np.diag(M)
        col, Cn, scale, ok = x, np.array(C, dtype=np.float64), np.ones(x.shape[1]), np.isfinite(d) & (d > 0)
    return dict(colours=col, C=Cn, M=M, b=b, kkt=k, ok=ok, ok_channel=okc, scale=scale)


def gram_rhs(A, video, NC):
    """Identity warp: ``A`` (P, K) uncoloured footprints, ``video`` (T, NC P) -> ``G`` (T, K, K), ``r`` (NC, T, K)."""
    A = np.asarray(A, dtype=np.float64)
    T, P = video.shape[0], A.shape[0]
    G = np.broadcast_to(A.T @ A, (T, A.shape[1], A.shape[1])).copy()
    r = np.stack([np.asarray(video[:, c * P:(c + 1) * P], dtype=np.float64) @ A for c in range(NC)])
    return G, r


# ---- the planted model -----------------------------------------------------------------------------------------------------------
def planted(depth, seed, noise=0.0, T=40, NC=3):
    """The six cells and traces of components_restatement.planted_video in NC channels -> dict(video (T, NC P), A (P, 6), C (6, T),
    colours (NC, 6), sz).  The colours are drawn in [0.1, 1], one entry is set to zero and every neuron's largest colour is 1 (the
    normal form ``normalise`` leaves); channel c of frame t is sum_k colours[c, k] A[:, k] C[k, t] plus white noise of standard
    deviation ``noise``, clamped at 0 when there is noise, as that video is."""
    import components_restatement as CR
    _, A8, traces, sz = CR.planted_video(depth, T, seed)
    A = A8[:, :6]
    rng = np.random.default_rng([seed, depth, T, 29])
    colours = rng.uniform(0.1, 1.0, (NC, 6))
    colours[rng.integers(NC), rng.integers(6)] = 0.0
    colours /= colours.max(axis=0, keepdims=True)
    video = np.concatenate([(A * colours[c][None, :]) @ traces for c in range(NC)], axis=0).T
    if noise:
        video = np.maximum(video + noise * rng.standard_normal(video.shape), 0.0)
    return dict(video=np.ascontiguousarray(video), A=A, C=traces, colours=colours, sz=sz)
