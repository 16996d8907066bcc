"""The definition of K15x (``dnmf_track_neurons_exclusive``) in float64 numpy, on top of K15's (tests/track_restatement.py): K15's
search with the neighbours that are already placed in the frame taken off the searched data.  The kernel
(csrc/track_exclusive.hip) computes the same thing in fp32.

Every frame t on its own; sigma, r = ceil(3 sigma), window, pick, refine, amplitude, threshold and NaN rules are K15's.

order     order[:, t] is a permutation of the neurons: the sequence in which frame t's searches run, in every round.
model     a placed neuron j is its last result: the integer pick p*_j, the refined centre p^_j and the amplitude a_j.  Its
          footprint is  a_j prod_d exp(-(x_d - p^_{j,d})^2 / sigma^2)  at the voxels x of the volume with |x_d - p*_{j,d}| <= r on
          every axis and 0 elsewhere: the truncation of K15's amplitude formula.
round 1   for k in order[:, t]:  K15's search of neuron k (``track_restatement.track``) on  frame_t - the footprints of the
          neurons placed so far in this frame  (the background comes off inside the search as in K15).  A search with a result
          places k; one without (NaN prediction, window outside the volume, score not above the threshold or not finite)
          leaves it unplaced: it is never subtracted.
rounds    2 .. R, the same order: k is searched again on frame_t - the footprints of all *other* placed neurons at their
          latest result; the new result replaces the old one, and a search without a result makes k's outputs NaN and
          unplaces it.  The window is centred on predict[k, :, t] in every round.
outputs   positions, amplitudes, peaks, pstar: those of the last search of (k, t).  margin: the smallest ``track`` margin over
          the rounds of (k, t) (NaN once a round had no result).  n_subtracted[k, t]: how many placed neighbours' +-r boxes met
          the region of the last search -- the voxels the search reads, K15's window + ring, widened as K15 widens it at the
          ends of an axis, + r, clipped to the volume (``region``); 0 when the search had no window.

The default order of the class level (``default_order``) is by descending K15 peak of the unsubtracted search, stable,
neurons without a result last: the bright neuron is placed first and taken off before the dim one is looked for.

``PAIRS`` / ``pair_case`` are the planted two-neuron cases the change was made for, ``SENS`` how far a result moves when the
neighbours it had subtracted move by K15's tolerance (``sensitivity``).
"""
import numpy as np

import detect_restatement as DR
import track_restatement as TR


def region(c, search, r, S):
    """One axis of the voxels a search around the rounded prediction c reads: (lo, hi), or None without a window."""
    if not np.isfinite(c) or c + search < 0 or c - search > S - 1:
        return None
    wlo, whi = int(max(c - search, 0.0)), int(min(c + search, S - 1.0))
    slo, shi = max(0, wlo - 1), min(S - 1, whi + 1)
    if wlo == 0:
        shi = max(shi, min(S - 1, 2))
    if whi == S - 1:
        slo = min(slo, max(0, S - 3))
    return max(0, slo - r), min(S - 1, shi + r)


def footprint(shape, pstar, phat, a, sigma):
    """The truncated model footprint of one placed neuron -> (slices of its box, values)."""
    r = DR.radius(sigma)
    sl, g = [], []
    for d in range(3):
        lo, hi = max(0, int(pstar[d]) - r), min(shape[d] - 1, int(pstar[d]) + r)
        x = np.arange(lo, hi + 1, dtype=np.float64)
        sl.append(slice(lo, hi + 1))
        g.append(np.exp(-(x - phat[d]) ** 2 / sigma ** 2))
    return tuple(sl), a * g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]


def default_order(peaks):
    """(K, T) peaks of the unsubtracted K15 search -> order (K, T) int32: descending, stable, NaN last."""
    key = np.where(np.isnan(peaks), np.inf, -np.asarray(peaks, dtype=np.float64))
    return np.argsort(key, axis=0, kind='stable').astype(np.int32)


def track_exclusive(frames, predict, sigma, search, order=None, rounds=2, threshold=0.0, background=None, perturb=None):
    """frames (T, X, Y, Z), predict (K,3,T) or (K,3), order (K,T) int or None (``default_order`` of K15's peaks) -> dict(positions
    (K,3,T), amplitudes (K,T), peaks (K,T), pstar (K,3,T) int (-1: no result), margin (K,T), n_subtracted (K,T) int, order (K,T)).
    ``perturb`` = (dp (3,), da): every footprint is subtracted at p^ + dp with amplitude a (1 + da) (``sensitivity``)."""
    frames = np.asarray(frames)
    T, shape = frames.shape[0], frames.shape[1:]
    sigma = float(sigma)
    r = DR.radius(sigma)
    predict = np.asarray(predict, dtype=np.float64)
    if predict.ndim == 2:
        predict = np.repeat(predict[:, :, None], T, axis=2)
    K = predict.shape[0]
    assert predict.shape == (K, 3, T) and rounds >= 1
    search = [int(s) for s in search]
    bg = np.zeros(T) if background is None else np.broadcast_to(np.asarray(background, dtype=np.float64), (T,))
    if order is None:
        order = default_order(TR.track(frames, predict, sigma, search, threshold, background)["peaks"])
    order = np.asarray(order)
    assert order.shape == (K, T) and (np.sort(order, axis=0) == np.arange(K)[:, None]).all()
    dp, da = (np.zeros(3), 0.0) if perturb is None else (np.asarray(perturb[0], dtype=np.float64), float(perturb[1]))
    out = dict(positions=np.full((K, 3, T), np.nan), amplitudes=np.full((K, T), np.nan), peaks=np.full((K, T), np.nan),
               pstar=np.full((K, 3, T), -1, dtype=np.int64), margin=np.full((K, T), np.inf),
               n_subtracted=np.zeros((K, T), dtype=np.int32), order=order.astype(np.int32))
    for t in range(T):
        placed = {}                                            # k -> (pstar, phat, a)
        for _ in range(rounds):
            for k in order[:, t]:
                k = int(k)
                reg = [region(np.rint(predict[k, d, t]), search[d], r, shape[d]) for d in range(3)]
                V = frames[t].astype(np.float64)
                n = 0
                for j, (ps, ph, a) in placed.items():
                    if j == k:
                        continue
                    sl, g = footprint(shape, ps, ph + dp, a * (1.0 + da), sigma)
                    V[sl] -= g
                    n += all(reg[d] is not None and ps[d] + r >= reg[d][0] and ps[d] - r <= reg[d][1] for d in range(3))
                one = TR.track(V[None], predict[k:k + 1, :, t:t + 1], sigma, search, threshold, bg[t:t + 1])
                out["n_subtracted"][k, t] = n if all(v is not None for v in reg) else 0
                for name in ("positions", "amplitudes", "peaks", "pstar"):
                    out[name][k, ..., t] = one[name][0, ..., 0]
                out["margin"][k, t] = min(out["margin"][k, t], one["margin"][0, 0]) if one["pstar"][0, 0, 0] >= 0 else np.nan
                if one["pstar"][0, 0, 0] >= 0:
                    placed[k] = (one["pstar"][0, :, 0], one["positions"][0, :, 0], one["amplitudes"][0, 0])
                else:
                    placed.pop(k, None)
    return out


# the planted pairs: (volume, separation of the resting points in voxels, search, seed).  sigma = 2, amplitudes 1.0 and 0.5, noise
# 0.002, T = 3.  In the last one the two blobs sit on different slices.  The seeds are the first (from 0) at which the
# definition itself meets what tests/test_track_exclusive_host.py asks of the case: both centres move, so a pair "3 apart" at rest
# is between 1 and 5 voxels apart in a frame, K15 is more than 3 voxels off only where a frame has them about 3.6 or more apart,
# and two rounds recover the dim amplitude to 10 % only where every frame has them about 3.9 or more apart (seed 28: 4.0 to 4.6).
PAIRS = [((40, 36, 1), 3.0, (4, 4, 0), 28), ((40, 36, 1), 4.0, (4, 4, 0), 1), ((40, 36, 1), 5.0, (4, 4, 0), 0),
         ((40, 36, 2), 3.0, (4, 4, 1), 0)]
PAIR_SIGMA, PAIR_AMPS, PAIR_T = 2.0, (1.0, 0.5), 3


def pair_case(i):
    """-> (frames (T,X,Y,Z) fp32, predict (2,3) the resting points, truth (2,3,T), amplitudes (2,), sigma, search).  The resting
    points lie ``sep`` voxels apart along x around the middle of the volume; in every frame each centre is moved by up to +-1
    voxel in x and in y, the two independently."""
    sz, sep, search, seed = PAIRS[i]
    rng = np.random.RandomState(300 + seed)
    mid = np.array([19.3, 17.6, 0.0])
    rest = np.stack([mid - [sep / 2, 0, 0], mid + [sep / 2, 0, 0]])
    if sz[2] > 1:
        rest[1, 2] = 1.0
    step = np.zeros((2, 3, PAIR_T))
    step[:, :2] = rng.uniform(-1.0, 1.0, (2, 2, PAIR_T))
    truth = rest[:, :, None] + step
    amps = np.array(PAIR_AMPS)
    frames = np.stack([DR.plant(sz, truth[:, :, t], amps, PAIR_SIGMA, noise=TR.NOISE, seed=7000 + 10 * seed + t) for t in range(PAIR_T)])
    return frames, rest, truth, amps, PAIR_SIGMA, search


def pair_errors(out, truth):
    """Largest distance over the frames between the result and the planted centre, per neuron; NaN counts as +inf."""
    e = np.linalg.norm(out["positions"] - truth, axis=1)
    return np.where(np.isnan(e), np.inf, e).max(axis=1)


def sensitivity(cases, rounds=(1, 2), dp=1e-3, da=1e-3):
    """How far positions (voxels), amplitudes and peaks (relative) move when every footprint that is subtracted is moved by ``dp``
    voxel per axis and scaled by 1 +- ``da`` -- K15's asserted tolerance -- per round: the largest change over ``cases``
    (values of ``gpu_cases()``), the sign patterns of the
    perturbation and R in ``rounds``, divided by R.  From the definition alone."""
    worst = dict(positions=0.0, amplitudes=0.0, peaks=0.0)
    for case in cases:
        for R in rounds:
            base = reference(case, R)
            for sx, sy, sz, sa in ((1, 1, 1, 1), (1, -1, 1, -1), (-1, 1, 1, -1), (-1, -1, 1, 1), (1, 1, 1, -1), (-1, -1, 1, -1)):
                got = reference(case, R, perturb=(np.array([sx, sy, sz]) * dp, sa * da))
                np.testing.assert_array_equal(got["pstar"], base["pstar"])
                ok = base["pstar"][:, 0, :] >= 0
                worst["positions"] = max(worst["positions"], np.abs(got["positions"] - base["positions"])[np.isfinite(base["positions"])].max() / R)
                for name in ("amplitudes", "peaks"):
                    worst[name] = max(worst[name], np.abs(got[name][ok] / base[name][ok] - 1).max() / R)
    return worst


def crowd_case():
    """K = 70 on 64 x 64 x 1, sigma = 1.5: centres at least 2.4 sigma apart, amplitudes in [0.5, 1], each moved by up to 0.8 voxel
    per frame; more placed neurons than a wavefront has lanes, and most regions hold several neighbours."""
    sz, sigma, K, T, search = (64, 64, 1), 1.5, 70, 2, (2, 2, 0)
    rng = np.random.RandomState(77)
    rest = DR.scatter_centres(sz, K, sigma, 5, apart=2.4)
    truth = np.clip(rest[:, :, None] + rng.uniform(-0.8, 0.8, (K, 3, T)) * np.array([1.0, 1.0, 0.0])[None, :, None], 0.0, 63.0)
    amps = rng.uniform(0.5, 1.0, (K, T))
    frames = np.stack([DR.plant(sz, truth[:, :, t], amps[:, t], sigma, noise=TR.NOISE, seed=900 + t) for t in range(T)])
    return frames, rest, truth, amps, sigma, search


def border_case():
    """Two blobs 4 voxels apart next to the corner of the volume: the +-r boxes of both are cut by two borders."""
    sz, sigma, search = (30, 28, 1), 2.0, (3, 3, 0)
    rest = np.array([[1.4, 2.2, 0.0], [5.4, 2.6, 0.0]])
    truth = rest[:, :, None] + np.array([[[0.3, -0.4], [0.5, 0.2], [0.0, 0.0]], [[0.6, 0.1], [-0.3, 0.4], [0.0, 0.0]]])
    amps = np.array([1.0, 0.6])
    frames = np.stack([DR.plant(sz, truth[:, :, t], amps, sigma, noise=TR.NOISE, seed=950 + t) for t in range(2)])
    return frames, rest, truth, amps, sigma, search


def gpu_cases():
    """The cases tests/test_gpu_track_exclusive.py runs against this definition: name -> dict(frames, predict, sigma, search and
    optionally background (T values), times (slots -> rows of frames)).  ``SENS`` is taken over all of them."""
    out = {}
    for i in range(len(PAIRS)):
        frames, rest, _, _, sigma, search = pair_case(i)
        out[f"pair{i}"] = dict(frames=frames, predict=rest, sigma=sigma, search=search)
    for i in range(len(TR.CASES)):
        frames, rest, _, _, sigma, search = TR.moving_case(i)
        out[f"moving{i}"] = dict(frames=frames, predict=rest, sigma=sigma, search=search)
    frames, rest, _, _, sigma, search = crowd_case()
    out["crowd"] = dict(frames=frames, predict=rest, sigma=sigma, search=search)
    frames, rest, _, _, sigma, search = pair_case(1)
    out["times"] = dict(frames=frames, predict=rest, sigma=sigma, search=search, times=[2, 0])
    frames, rest, _, _, sigma, search = pair_case(2)
    out["background"] = dict(frames=frames + np.array([0.3, -0.2, 0.1], dtype=np.float32)[:, None, None, None], predict=rest, sigma=sigma,
                             search=search, background=np.array([0.3, -0.2, 0.1]))
    frames, rest, _, _, sigma, search = border_case()
    out["border"] = dict(frames=frames, predict=rest, sigma=sigma, search=search)
    return out


def reference(case, rounds=2, perturb=None):
    """``track_exclusive`` of one of ``gpu_cases()`` with the default order."""
    frames = case["frames"] if case.get("times") is None else case["frames"][case["times"]]
    return track_exclusive(frames, case["predict"], case["sigma"], case["search"], rounds=rounds, background=case.get("background"),
                           perturb=perturb)


# ``sensitivity(gpu_cases().values())``, rounded up (tests/test_track_exclusive_host.py recomputes it)
SENS = dict(positions=8e-3, amplitudes=5e-3, peaks=5e-3)
