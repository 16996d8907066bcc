"""The definition of K15 (``dnmf_track_neurons``) in float64 numpy, written plainly: K14's score volume of every frame
(``detect_restatement.score``), searched in a small window around a predicted position.  The kernel
(csrc/track_neurons.hip) computes the same thing in fp32.

For every neuron k < K and frame t < T, with g1(d) = exp(-d^2 / sigma^2), r = ceil(3 sigma):

score     S_t = detect_restatement.score(frame_t, sigma, background_t): taps g1 truncated at r, zero padding, per-axis weight
          sqrt(nmax / n(q)).
window    c = predict[k, :, t] rounded half to even; the voxels q of the volume with |q_d - c_d| <= search[d] on every axis.
pick      p* = argmax of S_t over the window, equal scores to the lowest linear index (x Y + y) Z + z; NaN scores never win.
refine    K14's rule unchanged: per axis the parabola through ln S_t at p* and its two neighbours; at the first or last voxel
          of an axis of three or more voxels the one through p* and the two voxels inward.  Only where those scores are > 0
          and the parabola is concave; delta clamped to +-0.5.  The neighbours are voxels of the volume: they may lie outside
          the window.  p^ = p* + delta, ln S^ = ln S_t(p*) + sum_axes (f(delta) - f(0)).
amplitude a = S^ / sqrt(prod_axis nmax sum_x g1(x - p^_axis)^2), x over the voxels of the volume within r of p*_axis.
NaN       a NaN voxel makes NaN the scores whose (truncated) sums contain it: those within r of it on every axis, and no
          others.  (``detect_restatement.score`` multiplies by the zeros of its band matrices and 0 NaN would spread to the whole
          volume, so it is called on the frame with its NaN voxels zeroed and those scores are set to NaN afterwards.)
outputs   positions[k, :, t] = p^, amplitudes[k, t] = a, peaks[k, t] = S_t(p*).
no result a row is NaN when the prediction is not finite, the window has no voxel inside the volume, S_t(p*) is not finite, or
          S_t(p*) <= threshold.

There is no subtraction and no exclusion: the K T searches are independent.  Neighbouring neurons are not removed from the
score, so a neuron within about 2 sigma of a brighter one can be captured by it; the search window is the guard against
that.  Frame t does not depend on frame t - 1: ``predict`` carries any prior.

``margin[k, t]`` = (best - best score in the window more than one voxel (Chebyshev) from p*) / best: how far the pick is
from being decided by rounding; +inf when the window has no such voxel.
"""
import math

import numpy as np

import detect_restatement as DR


def refine(S, p, sigma, nmax):
    """K14's refinement and amplitude at the voxel p of the score volume S -> (p^ (3,), amplitude)."""
    shape = S.shape
    r = DR.radius(sigma)
    c = S[tuple(p)]
    delta = np.zeros(3)
    ln_adj = 0.0
    for d in range(3):
        e = np.zeros(3, dtype=np.int64)
        e[d] = 1
        two = 0 < p[d] < shape[d] - 1
        if c <= 0 or not (two or shape[d] >= 3):
            continue
        inward = e if p[d] == 0 else -e
        m, q = (S[tuple(p - e)], S[tuple(p + e)]) if two else (S[tuple(p + inward)], S[tuple(p + 2 * inward)])
        if m > 0 and q > 0:
            lm, lc, lq = math.log(m), math.log(c), math.log(q)
            a2 = 0.5 * (lm - 2.0 * lc + lq) if two else 0.5 * (lc - 2.0 * lm + lq)
            b = 0.5 * (lq - lm) if two else (lm - lc) - a2
            if a2 < 0:
                t = min(0.5, max(-0.5, -b / (2.0 * a2)))
                ln_adj += b * t + a2 * t * t
                delta[d] = t if two or p[d] == 0 else -t
    phat = p + delta
    a = c * math.exp(ln_adj)
    for d in range(3):
        x = np.arange(max(0, p[d] - r), min(shape[d] - 1, p[d] + r) + 1)
        g = np.exp(-(x - phat[d]) ** 2 / sigma ** 2)
        a /= math.sqrt(nmax[d] * (g * g).sum())
    return phat, a


def frame_score(V, sigma, background):
    """K14's score volume of one frame; NaN where a NaN voxel lies within r on every axis."""
    V = np.asarray(V, dtype=np.float64)
    bad = np.isnan(V)
    if not bad.any():
        return DR.score(V, sigma, background)
    S = DR.score(np.where(bad, background, V), sigma, background)
    reach = [DR.band(n, sigma) > 0 for n in V.shape]
    hit = np.einsum('ia,jb,kc,abc->ijk', *[m.astype(np.float64) for m in reach], bad.astype(np.float64)) > 0
    S[hit] = np.nan
    return S


def track(frames, predict, sigma, search, threshold=0.0, background=None):
    """frames (T, X, Y, Z), predict (K,3,T) or (K,3) -> dict(positions (K,3,T), amplitudes (K,T), peaks (K,T), pstar (K,3,T)
    int (-1 where there is no result), margin (K,T) (NaN where there is no result))."""
    frames = np.asarray(frames)
    assert frames.ndim == 4 and sigma > 0
    T, shape = frames.shape[0], frames.shape[1:]
    sigma = float(sigma)
    predict = np.asarray(predict, dtype=np.float64)
    if predict.ndim == 2:
        predict = np.repeat(predict[:, :, None], T, axis=2)
    K = predict.shape[0]
    assert predict.shape == (K, 3, T)
    search = [int(s) for s in search]
    assert len(search) == 3 and min(search) >= 0
    bg = np.zeros(T) if background is None else np.broadcast_to(np.asarray(background, dtype=np.float64), (T,))
    _, nmax = DR.score_weights(shape, sigma)
    pos = np.full((K, 3, T), np.nan)
    amp = np.full((K, T), np.nan)
    peaks = np.full((K, T), np.nan)
    margin = np.full((K, T), np.nan)
    pstar = np.full((K, 3, T), -1, dtype=np.int64)
    for t in range(T):
        S = frame_score(frames[t], sigma, bg[t])
        for k in range(K):
            if not np.isfinite(predict[k, :, t]).all():
                continue
            c = np.rint(predict[k, :, t])                    # half to even
            lo = [int(max(0.0, c[d] - search[d])) if c[d] + search[d] >= 0 else 0 for d in range(3)]
            hi = [int(min(shape[d] - 1.0, c[d] + search[d])) if c[d] - search[d] <= shape[d] - 1 else -1 for d in range(3)]
            if any(c[d] + search[d] < 0 or c[d] - search[d] > shape[d] - 1 for d in range(3)):
                continue
            W = S[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
            i = np.unravel_index(int(np.argmax(np.where(np.isnan(W), -np.inf, W))), W.shape)   # C order = the volume's order
            best = W[i]
            if not np.isfinite(best) or best <= threshold:
                continue
            p = np.array([lo[d] + i[d] for d in range(3)])
            far = np.ones(W.shape, dtype=bool)
            far[tuple(slice(max(0, i[d] - 1), i[d] + 2) for d in range(3))] = False
            rest = np.where(np.isnan(W[far]), -np.inf, W[far])
            margin[k, t] = (best - rest.max()) / best if rest.size else np.inf
            pos[k, :, t], amp[k, t] = refine(S, p, sigma, nmax)
            peaks[k, t], pstar[k, :, t] = best, p
    return dict(positions=pos, amplitudes=amp, peaks=peaks, pstar=pstar, margin=margin)


# the moving planted cases both test files use: (volume, sigma, K, T, search, seed).  The last has an axis shorter than the
# filter window (2 r + 1 = 13 > 9).
CASES = [((40, 37, 2), 2.0, 5, 6, (4, 4, 1), 0), ((23, 45, 1), 1.5, 4, 5, (3, 3, 0), 1), ((34, 34, 3), 3.0, 3, 4, (5, 5, 1), 2),
         ((9, 50, 1), 2.0, 2, 3, (2, 3, 0), 3)]
NOISE = 0.002


def moving_case(i):
    """-> (frames (T,X,Y,Z) fp32, predict (K,3) the resting centres, truth (K,3,T) the planted centres, amplitudes (K,T), sigma,
    search).  Centres rest at least (5 + 2 max(search) / sigma) sigma apart in the plane and move by up to search - 0.6 voxels
    per axis around them, clipped to the volume, so some blobs are cut by the border; amplitudes 0.9^k times a per-frame
    factor in [0.8, 1.2]; noise 0.002 N(0, 1)."""
    sz, sigma, K, T, search, seed = CASES[i]
    rng = np.random.RandomState(1000 + seed)
    apart = 5.0 + 2.0 * max(search) / sigma
    rest = DR.scatter_centres(sz, K, sigma, seed, apart=apart)
    rest[:, 2] = np.rint(rest[:, 2])
    reach = np.maximum(np.array(search, dtype=np.float64) - 0.6, 0.0)
    truth = rest[:, :, None] + rng.uniform(-1.0, 1.0, (K, 3, T)) * reach[None, :, None]
    truth = np.clip(truth, 0.0, (np.array(sz, dtype=np.float64) - 1.0)[None, :, None])
    amps = 0.9 ** np.arange(K)[:, None] * rng.uniform(0.8, 1.2, (K, T))
    frames = np.stack([DR.plant(sz, truth[:, :, t], amps[:, t], sigma, noise=NOISE, seed=5000 + 100 * seed + t) for t in range(T)])
    return frames, rest, truth, amps, sigma, search
