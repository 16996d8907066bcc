"""The definition of K15c (``dnmf_follow_neurons``) in float64 numpy, written plainly: K15's search
(``track_restatement.track``, built on ``frame_score`` and ``refine``) run frame after frame, every search around the position
the chain predicts from what it found before.  The kernel (csrc/follow_neurons.hip) runs the same recurrence in float64 on
the fp32 results of its searches.

Every neuron k < K runs two independent chains from the frame ``anchor``: the forward chain visits the frames anchor,
anchor + 1, ..., T - 1, the backward chain anchor, anchor - 1, ..., 0; the backward chain repeats the anchor search and writes
nothing for the anchor frame.  A chain starts with last = start[k], vel = 0, n = 0, miss = 0 and does, per visited frame j:

predict   pred = last + (momentum * vel) * n: every * and + one float64 rounding in the order written;
          predicted[k, :, j] = pred.
search    K15's search of frame j around pred, unchanged: window, pick, refinement, amplitude and NaN rules.
found     if n > 0: vel = (p^ - last) / n.  last = p^, n = 1, miss = 0; the row is written.
missed    the row is NaN; n += 1, miss += 1; if miss > max_gap the chain is lost: lost_at[k, direction] = j, and every later
          frame of the chain gets NaN rows and a NaN predicted.

A start row that is not finite loses both chains before their first search: lost_at = anchor and every frame is NaN,
predicted included.  There is no exclusion between neurons: two chains may follow the same blob.

``half[k, t]``: the smallest distance of a coordinate of predicted[k, :, t] from a half-integer, over the axes with
search > 0 (NaN where predicted is; +inf without such an axis): how far the window is from being moved by the rounding of a
position (the kernel's positions are fp32).
"""
import numpy as np

import detect_restatement as DR
import track_restatement as TR


def follow(frames, start, sigma, search, anchor=0, momentum=0.0, max_gap=5, threshold=0.0, background=None):
    """frames (T, X, Y, Z), start (K, 3) -> dict(positions (K,3,T), amplitudes (K,T), peaks (K,T), predicted (K,3,T), lost_at
    (K,2) int (forward, backward; -1: never lost), pstar (K,3,T) int, margin (K,T), half (K,T))."""
    frames = np.asarray(frames)
    T = frames.shape[0]
    start = np.asarray(start, dtype=np.float64)
    K = start.shape[0]
    assert frames.ndim == 4 and start.shape == (K, 3) and 0 <= anchor < T and 0.0 <= momentum <= 1.0 and max_gap >= 0
    momentum = np.float64(momentum)
    bg = np.zeros(T) if background is None else np.broadcast_to(np.asarray(background, dtype=np.float64), (T,))
    out = dict(positions=np.full((K, 3, T), np.nan), amplitudes=np.full((K, T), np.nan), peaks=np.full((K, T), np.nan),
               predicted=np.full((K, 3, T), np.nan), lost_at=np.full((K, 2), -1, dtype=np.int64),
               pstar=np.full((K, 3, T), -1, dtype=np.int64), margin=np.full((K, T), np.nan))
    for direction, visit in enumerate((range(anchor, T), range(anchor, -1, -1))):
        last = start.copy()
        vel = np.zeros((K, 3))
        n = np.zeros(K, dtype=np.int64)
        miss = np.zeros(K, dtype=np.int64)
        lost = ~np.isfinite(start).all(1)
        out["lost_at"][lost, direction] = anchor
        for j in visit:
            # the chains of one direction visit the same frames: one call of K15's definition serves them all (a lost chain
            # asks with NaN, which finds nothing)
            pred = last + (momentum * vel) * n[:, None].astype(np.float64)
            pred[lost] = np.nan
            res = TR.track(frames[j:j + 1], pred[:, :, None], sigma, search, threshold=threshold, background=bg[j:j + 1])
            found = np.isfinite(res["positions"][:, :, 0]).all(1)
            if not (direction == 1 and j == anchor):
                out["predicted"][:, :, j] = pred
                for name in ("positions", "pstar"):
                    out[name][:, :, j] = res[name][:, :, 0]
                for name in ("amplitudes", "peaks", "margin"):
                    out[name][:, j] = res[name][:, 0]
            for k in range(K):
                if lost[k]:
                    continue
                if found[k]:
                    p = res["positions"][k, :, 0]
                    if n[k] > 0:
                        vel[k] = (p - last[k]) / np.float64(n[k])
                    last[k], n[k], miss[k] = p, 1, 0
                else:
                    n[k] += 1
                    miss[k] += 1
                    if miss[k] > max_gap:
                        lost[k] = True
                        out["lost_at"][k, direction] = j
    on = [d for d in range(3) if int(search[d]) > 0]
    P = out["predicted"][:, on, :]
    out["half"] = np.abs(P - np.floor(P) - 0.5).min(1) if on else np.full((K, T), np.inf)
    return out


def predicted_from(positions, start, anchor, momentum, max_gap):
    """The recurrence alone, from the positions a run stored and their found / NaN pattern -> (predicted (K,3,T), lost_at
    (K,2)): what ``follow`` computes when its searches give exactly ``positions``."""
    positions = np.asarray(positions, dtype=np.float64)
    K, _, T = positions.shape
    start = np.asarray(start, dtype=np.float64)
    momentum = np.float64(momentum)
    predicted = np.full((K, 3, T), np.nan)
    lost_at = np.full((K, 2), -1, dtype=np.int64)
    for k in range(K):
        for direction, visit in enumerate((range(anchor, T), range(anchor, -1, -1))):
            if not np.isfinite(start[k]).all():
                lost_at[k, direction] = anchor
                continue
            last, vel, n, miss = start[k].copy(), np.zeros(3), 0, 0
            for j in visit:
                pred = last + (momentum * vel) * np.float64(n)
                if not (direction == 1 and j == anchor):
                    predicted[k, :, j] = pred
                p = positions[k, :, j]
                if np.isfinite(p).all():
                    if n > 0:
                        vel = (p - last) / np.float64(n)
                    last, n, miss = p.copy(), 1, 0
                else:
                    n += 1
                    miss += 1
                    if miss > max_gap:
                        lost_at[k, direction] = j
                        break
    return predicted, lost_at


# the drifting planted videos both test files use: (volume, T, drift per frame, search, anchor, momentum, seed of jitter and
# amplitudes, threshold, max_gap).  Four blobs of sigma = 2 that all move by the same drift per frame: little per frame, far
# in total -- and, in the third, further per frame than the window is wide.  (There the first step from the anchor has no
# velocity yet: the blob is 2.6 voxels plus rounding and jitter from the window's centre, and the window reaches 2.5.  The
# seed is one at which the definition finds it within half a voxel all the same; tests/test_follow_host.py asserts that.)
# In the last two blobs leave the volume through the far end of the y axis.
SIGMA, NOISE = 2.0, 0.002
CASES = [((56, 44, 2), 10, (1.3, 0.8), (3, 3, 1), 0, 0.0, 300, 0.0, 5), ((56, 44, 1), 10, (1.3, 0.8), (3, 3, 0), 4, 0.0, 301, 0.0, 5),
         ((64, 40, 1), 9, (2.6, 0.0), (2, 2, 0), 0, 1.0, 303, 0.0, 5), ((48, 40, 1), 12, (0.4, 3.0), (3, 3, 0), 0, 1.0, 304, 0.1, 2)]


def drifting_case(i, blank=None):
    """-> (frames (T,X,Y,Z) fp32, truth (K,3,T), amplitudes (K,T)).  Blobs at (10.3, 9.6, 0), (12.7, 28.2, Z-1), (27.4, 14.1, 0),
    (30.2, 31.5, Z-1) in frame 0, drifting by CASES[i][2] per frame with a jitter U(-0.3, 0.3) per in-plane axis; amplitudes
    0.9^k U(0.8, 1.2); noise 0.002 N(0, 1).  ``blank`` (k, frames): that neuron's amplitude is 0 in those frames."""
    sz, T, v, _, _, _, seed, _, _ = CASES[i]
    rng = np.random.RandomState(seed)
    Z = sz[2]
    base = np.array([[10.3, 9.6, 0.0], [12.7, 28.2, Z - 1.0], [27.4, 14.1, 0.0], [30.2, 31.5, Z - 1.0]])
    K = len(base)
    truth = np.repeat(base[:, :, None], T, axis=2)
    truth[:, 0, :] += v[0] * np.arange(T)[None, :]
    truth[:, 1, :] += v[1] * np.arange(T)[None, :]
    truth[:, :2, :] += rng.uniform(-0.3, 0.3, (K, 2, T))
    amps = 0.9 ** np.arange(K)[:, None] * rng.uniform(0.8, 1.2, (K, T))
    if blank is not None:
        amps[blank[0], list(blank[1])] = 0.0
    frames = np.stack([DR.plant(sz, truth[:, :, t], amps[:, t], SIGMA, noise=NOISE, seed=7000 + 100 * i + t) for t in range(T)])
    return frames, truth, amps
