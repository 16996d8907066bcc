"""Seeded inputs of the K32 tests (tests/test_ar1_host.py, tests/test_gpu_ar1.py, tests/test_gpu_ar1_fit.py): synthetic Gram data
with a sparse pattern, and the planted video of the host comparison with HALS.  numpy only."""
import numpy as np

G_TRUE = float(np.exp(-0.3))            # the decay of the simulator's traces


def ar1_traces(rng, K, T, g=G_TRUE, density=0.1, baseline=1.0):
    """Baseline plus unit spikes through the AR(1) decay g: the simulator's model (its kernel e^(-0.3 i), not cut after 10 taps)."""
    s = (rng.rand(K, T) < density).astype(np.float64)
    c = np.zeros((K, T))
    for t in range(T):
        c[:, t] = (g * c[:, t - 1] if t else 0.0) + s[:, t]
    return baseline + c


def band_pattern(K, edges=None):
    """(K, K) bool with the diagonal: ``edges`` pairs, or a band of half-width 2 with every third pair (k, k + 2) left out."""
    pat = np.eye(K, dtype=bool)
    if edges is None:
        edges = [(k, k + 1) for k in range(K - 1)] + [(k, k + 2) for k in range(K - 2) if k % 3]
    for k, l in edges:
        pat[k, l] = pat[l, k] = True
    return pat


def gram_data(K, T, seed, pattern=None, noise=0.05, baseline=1.0):
    """Symmetric, diagonally dominant G (T, K, K) fp32 on ``pattern`` (diagonal in [1, 2), off-diagonal entries in [0, 0.2)) and
    r = G c + noise (T, K) fp32 for AR(1) traces c -> ``(G, r, c, pattern)``."""
    rng = np.random.RandomState(seed)
    pat = band_pattern(K) if pattern is None else pattern
    G = np.zeros((T, K, K), np.float32)
    kk, ll = np.nonzero(np.triu(pat, 1))
    off = (0.2 * rng.rand(T, len(kk))).astype(np.float32)
    G[:, kk, ll] = off
    G[:, ll, kk] = off
    G[:, np.arange(K), np.arange(K)] = (1.0 + rng.rand(T, K)).astype(np.float32)
    c = ar1_traces(rng, K, T, baseline=baseline)
    r = np.einsum("tkl,lt->tk", G.astype(np.float64), c) + noise * rng.randn(T, K)
    return G, r.astype(np.float32), c, pat


def nbr_table(pattern, NN=None, pad=-1):
    """(K, NN) int32: per row the columns of the pattern, ascending, padded with ``pad``."""
    K = len(pattern)
    NN = int(pattern.sum(1).max()) + 1 if NN is None else NN
    nbr = np.full((K, NN), pad, np.int32)
    for k in range(K):
        cols = np.flatnonzero(pattern[k])
        nbr[k, :len(cols)] = cols
    return nbr


def without_weight(G, r, K, T):
    """Takes the weight of frames away, in place: neuron 0 loses a leading run, a run in the middle that empties whole segments of
    lanes and a trailing run (row and column of G zero there, as where a footprint leaves the field of view); the last neuron
    has a diagonal entry that is not finite (NaN, +inf) and a negative one."""
    runs = [np.arange(min(3, T - 1)), np.arange(T // 3, T // 3 + max(T // 8, 2)), np.arange(max(T - 2, 1), T)] if T > 1 else [np.arange(0)]
    for run in runs:
        run = run[(run >= 0) & (run < T)]
        G[run, 0, :] = 0.0
        G[run, :, 0] = 0.0
    k = K - 1
    if T > 6:
        G[5, k, k] = np.nan
        G[T // 2, k, k] = np.inf
        G[T - 2, k, k] = -0.5
    return G, r


def planted_video(Z, seed, noise, T=120):
    """The planted comparison of 'ar1' with HALS: 24 x 20 x Z voxels, K = 6 Gaussian footprints of which (0, 1) and (2, 3) overlap
    (centres 2 voxels apart at width 1.5, cut at 0.05; the other pairs share no voxel), AR(1) traces on the baseline 1, white noise of deviation ``noise`` a voxel, no motion
    -> ``(G (T, K, K), r (T, K), traces (K, T), pattern)``, G_t = A^T A for every frame and r_t = A^T y_t, float64."""
    rng = np.random.RandomState(seed)
    X, Y, K = 24, 20, 6
    centres = np.array([[4.0, 4.0], [6.0, 4.0], [14.0, 5.0], [14.0, 7.0], [5.0, 14.0], [18.0, 15.0]])
    xx, yy, zz = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    A = np.stack([np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2 + (zz - (Z - 1) / 2) ** 2) / (2 * 1.5 ** 2)).ravel() for cx, cy in centres], 1)
    A[A < 0.05] = 0.0
    C = ar1_traces(rng, K, T)
    frames = A @ C + noise * rng.randn(A.shape[0], T)
    G = np.broadcast_to(A.T @ A, (T, K, K)).copy()
    r = (A.T @ frames).T.copy()
    return G, r, C, (A.T @ A) != 0


def median_correlation(C, truth):
    return float(np.median([np.corrcoef(C[k], truth[k])[0, 1] for k in range(len(C))]))
