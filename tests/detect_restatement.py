"""The definition of K14 (``dnmf_detect_neurons``) in float64 numpy, written plainly: a matched filter with the footprint
model's own Gaussian, then a greedy pursuit on the score volume.  The kernels (csrc/detect_neurons.hip) compute the same
thing in fp32.

With g1(d) = exp(-d^2 / sigma^2), r = ceil(3 sigma):

filter   R = G_x G_y G_z (V - background): one band matrix per axis, G[i, j] = g1(i - j) for |i - j| <= r, else 0 (zero
         padding outside the volume; an axis shorter than the window has fewer taps).
score    S(q) = R(q) prod_axis sqrt(nmax / n(q_axis)), n(q) = sum_x g1(x - q)^2 over the voxels x of the axis within r of q
         and nmax = n in the middle of the axis.  S = R wherever the window is inside the volume.  Under white noise S has
         the same variance everywhere, and for an isolated blob cut by the border S / sqrt(nmax n) = <f_q, V> / |f_q| peaks
         exactly at the blob's centre (Cauchy-Schwarz), where R peaks up to a voxel inside it: picking and refining on R
         returned the amplitude of such a blob 9 to 21 % low at sigma = 2.
pursuit  up to K times:
  pick      p* = argmax S, equal scores to the lowest linear index (NaN scores never win); stop when S(p*) <= threshold or
            S(p*) is not finite.
  refine    per axis, when S(p*) > 0: the parabola f(t) = ln c + b t + a2 t^2 through ln S at p* and its two neighbours (m,
            q); at the first or last voxel of an axis of three or more voxels the one through p* and the two voxels inward.
            Where those scores are > 0 and a2 < 0: delta = -b / (2 a2) clamped to +-0.5, else delta = 0;
            ln S^ = ln c + sum_axes f(delta) - ln c;  p^ = p* + delta.  Between two neighbours and unclamped this is
            delta = (ln m - ln q) / (2 (ln m - 2 ln c + ln q)), ln S^ = ln c - sum (ln m - ln q) delta / 4.  A refined centre
            that would lie within min_distance of an earlier one is dropped: that pick keeps p^ = p*, S^ = S(p*) (p* itself
            cannot be that close: such voxels are excluded), so no two returned centres are within min_distance.
  amplitude a = S^ / sqrt(prod_axis nmax sum_x g1(x - p^_axis)^2), x over the voxels of the volume within r of p*_axis: the
            least-squares amplitude of the footprint truncated like the filter.
  subtract  S(q) -= a prod_axis h_axis(q_axis) sqrt(nmax / n(q_axis)),  h(q) = sum_x g1(x - q) g1(x - p^) over the same x
            with |x - q| <= r: the score of that footprint (zero beyond 2 r of p*).
  exclude   S = -inf where |q - p^|_2 <= min_distance; -inf stays -inf under later subtractions.
Rows from ``count`` on are NaN.

``margin[k]`` = (best - best score at any voxel more than one voxel (Chebyshev) from p*) / best at pick k: how far the
pick is from being decided by rounding.
"""
import math

import numpy as np


def radius(sigma):
    return int(math.ceil(3.0 * float(sigma)))


def band(S, sigma):
    """(S, S) band matrix of the truncated taps."""
    d = np.arange(S)[:, None] - np.arange(S)[None, :]
    return np.where(np.abs(d) <= radius(sigma), np.exp(-d.astype(np.float64) ** 2 / float(sigma) ** 2), 0.0)


def lower_median(V):
    """torch.median's choice: the lower of the two middle values."""
    flat = np.sort(np.asarray(V).ravel())
    return flat[(flat.size - 1) // 2]


def matched_filter(V, sigma, background):
    V = np.asarray(V, dtype=np.float64) - float(background)
    X, Y, Z = V.shape
    return np.einsum('ia,jb,kc,abc->ijk', band(X, sigma), band(Y, sigma), band(Z, sigma), V, optimize=True)


def axis_norms(S, sigma):
    """n(q) for every voxel q of an axis of S voxels."""
    return (band(S, sigma) ** 2).sum(1)


def score_weights(shape, sigma):
    """Per axis sqrt(nmax / n(q)), and nmax."""
    n = [axis_norms(S, sigma) for S in shape]
    nmax = [v[(len(v) - 1) // 2] for v in n]
    return [np.sqrt(m / v) for v, m in zip(n, nmax)], nmax


def score(V, sigma, background):
    w, _ = score_weights(np.shape(V), sigma)
    return matched_filter(V, sigma, background) * w[0][:, None, None] * w[1][None, :, None] * w[2][None, None, :]


def detect(V, K, sigma, min_distance=None, threshold=0.0, background=None):
    """-> dict(positions (K,3), amplitudes (K,), count, pstar (K,3) int (-1 from count on), margin (K,), peaks (K,) = S(p*) at
    each pick, scores (X,Y,Z) as the pursuit left them)."""
    V = np.asarray(V)
    assert V.ndim == 3 and K >= 1 and sigma > 0
    S = V.shape
    sigma = float(sigma)
    r = radius(sigma)
    md = 2.0 * sigma if min_distance is None else float(min_distance)
    bg = float(lower_median(V)) if background is None else float(background)
    w, nmax = score_weights(S, sigma)
    R = score(V, sigma, bg)
    pos = np.full((K, 3), np.nan)
    amp = np.full((K,), np.nan)
    margin = np.full((K,), np.nan)
    peaks = np.full((K,), np.nan)
    pstar = np.full((K, 3), -1, dtype=np.int64)
    axes = [np.arange(n) for n in S]
    count = 0
    for k in range(K):
        p = np.array(np.unravel_index(int(np.argmax(np.where(np.isnan(R), -np.inf, R))), S))
        c = R[tuple(p)]
        if not np.isfinite(c) or c <= threshold:
            break
        far = np.ones(S, dtype=bool)
        far[tuple(slice(max(0, p[d] - 1), p[d] + 2) for d in range(3))] = False
        rest = np.where(np.isnan(R[far]), -np.inf, R[far])
        margin[k] = (c - rest.max()) / c if rest.size else np.inf
        delta = np.zeros(3)
        ln_adj = 0.0
        for d in range(3):
            e = np.zeros(3, dtype=np.int64)
            e[d] = 1
            two = 0 < p[d] < S[d] - 1
            if c <= 0 or not (two or S[d] >= 3):
                continue
            inward = e if p[d] == 0 else -e
            m, q = (R[tuple(p - e)], R[tuple(p + e)]) if two else (R[tuple(p + inward)], R[tuple(p + 2 * inward)])
            if m > 0 and q > 0:
                lm, lc, lq = math.log(m), math.log(c), math.log(q)
                a2 = 0.5 * (lm - 2.0 * lc + lq) if two else 0.5 * (lc - 2.0 * lm + lq)
                b = 0.5 * (lq - lm) if two else (lm - lc) - a2
                if a2 < 0:
                    t = min(0.5, max(-0.5, -b / (2.0 * a2)))
                    ln_adj += b * t + a2 * t * t
                    delta[d] = t if two or p[d] == 0 else -t
        phat = p + delta
        if count and (np.linalg.norm(pos[:count] - phat, axis=1) <= md).any():
            phat, ln_adj = p.astype(np.float64), 0.0
        a = c * math.exp(ln_adj)
        h = []
        for d in range(3):
            x = np.arange(max(0, p[d] - r), min(S[d] - 1, p[d] + r) + 1)
            e = np.exp(-(x - phat[d]) ** 2 / sigma ** 2)
            a /= math.sqrt(nmax[d] * (e * e).sum())
            D = x[None, :] - axes[d][:, None]
            h.append((np.where(np.abs(D) <= r, np.exp(-D.astype(np.float64) ** 2 / sigma ** 2), 0.0) * e[None, :]).sum(1) * w[d])
        R -= a * h[0][:, None, None] * h[1][None, :, None] * h[2][None, None, :]
        d2 = ((axes[0] - phat[0]) ** 2)[:, None, None] + ((axes[1] - phat[1]) ** 2)[None, :, None] \
            + ((axes[2] - phat[2]) ** 2)[None, None, :]
        R[d2 <= md * md] = -np.inf
        pos[k], amp[k], pstar[k], peaks[k] = phat, a, p, c
        count += 1
    return dict(positions=pos, amplitudes=amp, count=count, pstar=pstar, margin=margin, peaks=peaks, scores=R)


def plant(sz, centres, amplitudes, sigma, noise=0.0, seed=0, background=0.0):
    """float32 volume of Gaussian blobs exp(-|x - c|^2 / sigma^2) plus ``noise`` N(0, 1) plus ``background``."""
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in sz], indexing='ij')
    V = np.zeros(sz)
    for c, a in zip(np.asarray(centres, dtype=np.float64), amplitudes):
        V += a * np.exp(-((g[0] - c[0]) ** 2 + (g[1] - c[1]) ** 2 + (g[2] - c[2]) ** 2) / float(sigma) ** 2)
    V += noise * np.random.RandomState(seed).randn(*sz) + background
    return V.astype(np.float32)


def scatter_centres(sz, K, sigma, seed, apart=3.2, border=0.0):
    """K centres at least ``apart`` sigma from one another in the plane, anywhere in the volume (rejection sampling)."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(100000):
        c = np.array([rng.uniform(border, sz[0] - 1 - border), rng.uniform(border, sz[1] - 1 - border), rng.uniform(0, sz[2] - 1)])
        if all(np.hypot(*(c[:2] - o[:2])) >= apart * sigma for o in out):
            out.append(c)
            if len(out) == K:
                return np.array(out)
    raise ValueError(f"cannot place {K} centres {apart} sigma apart in {sz}")


# the planted cases both test files use: (volume, sigma, planted blobs, seed of the centres); amplitudes 0.9^k, noise
# 0.002 N(0, 1).  The last one has a window (4 r + 1 = 37) wider than a 16 x 16 x 4 tile of the kernel's table and a volume
# that is no multiple of the tile in any axis.
CASES = [((37, 29, 2), 2.0, 6, 0), ((21, 40, 1), 1.5, 5, 0), ((9, 50, 1), 2.0, 3, 0), ((70, 66, 1), 2.0, 12, 0),
         ((33, 33, 2), 3.0, 4, 1)]
EXTRA = 4      # picks asked for beyond the planted ones


def planted_case(i):
    """-> (volume fp32, centres (K,3), amplitudes (K,), sigma, K)."""
    sz, sigma, K, seed = CASES[i]
    centres = scatter_centres(sz, K, sigma, seed)
    amps = 0.9 ** np.arange(K)
    return plant(sz, centres, amps, sigma, noise=0.002, seed=seed + 100), centres, amps, sigma, K
