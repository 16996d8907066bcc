"""numpy float64 restatement of K6h, the exact NNLS footprint solver (HALS / cyclic coordinate descent) on the sums of K5,
beside the multiplicative update K6.  Per voxel p, over the neurons whose box holds p,

    F(a_p) = 1/2 a_p^T Cs a_p - A1[p]^T a_p + gamma D[p]^T a_p ,   a_p >= 0

(summed over the voxels this is 1/2 |Y_i - A C|^2 + gamma sum D o A up to the constant |Y_i|^2).  One sweep visits, for
every voxel independently, the neurons whose box holds it in ascending k:

    g      = sum_l a[p,l] Cs[l,k] - A1[p,k] + gamma D[p,k]     (l over the neurons whose box holds p, ascending, current values)
    a[p,k] <- max(0, a[p,k] - g / Cs[k,k])                     (Cs[k,k] <= 0 or not finite: a[p,k] stays)

Values outside a neuron's box are zero and stay zero.  A box is (xlo, xhi, ylo, yhi, zlo, zhi), inclusive, voxel p =
(x Y + y) Z + z; without boxes every voxel is free.  Nothing is normalised.  The tests compare the kernels against these
functions; nothing here is fast."""
import numpy as np


def box_mask(boxes, sz, P=None, K=None):
    """(P,K) bool: voxel p inside the box of neuron k.  ``boxes`` None: all True (``P``, ``K`` then give the shape)."""
    if boxes is None:
        return np.ones((P, K), dtype=bool)
    X, Y, Z = (int(s) for s in sz)
    b = np.asarray(boxes).reshape(-1, 6)
    x, y, z = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    x, y, z = x.reshape(-1, 1), y.reshape(-1, 1), z.reshape(-1, 1)
    return ((x >= b[None, :, 0]) & (x <= b[None, :, 1]) & (y >= b[None, :, 2]) & (y <= b[None, :, 3])
            & (z >= b[None, :, 4]) & (z <= b[None, :, 5]))


def dilate_boxes(boxes, sz, grow):
    """The boxes grown by ``grow`` (an int or (gx, gy, gz)) voxels on every side and clipped to the volume; an empty box
    (lo > hi on an axis) stays as it is."""
    b = np.array(boxes, dtype=np.int64).reshape(-1, 6)
    g = np.broadcast_to(np.asarray(grow, dtype=np.int64), (3,))
    full = (b[:, 0::2] <= b[:, 1::2]).all(1)
    out = b.copy()
    for ax in range(3):
        out[full, 2 * ax] = np.maximum(b[full, 2 * ax] - g[ax], 0)
        out[full, 2 * ax + 1] = np.minimum(b[full, 2 * ax + 1] + g[ax], int(sz[ax]) - 1)
    return out


def _inputs(A, A1, Cs, D, gamma, boxes, sz):
    A1 = np.asarray(A1, dtype=np.float64)
    P, K = A1.shape
    A = np.array(A, dtype=np.float64).reshape(P, K)
    Cs = np.asarray(Cs, dtype=np.float64)
    gamma = 0.0 if gamma is None else float(gamma)
    D = None if D is None else np.asarray(D, dtype=np.float64).reshape(P, K)
    M = box_mask(boxes, sz, P, K)
    A[~M] = 0.0
    return A, A1, Cs, D, gamma, M


def _column_gradient(A, A1, Cs, D, gamma, M, k):
    """g of neuron k at every voxel: the sum in ascending l over the neurons whose box holds the voxel."""
    s = np.zeros(A.shape[0])
    for l in range(A.shape[1]):
        s = np.where(M[:, l], s + A[:, l] * Cs[l, k], s)
    g = s - A1[:, k]
    if D is not None:
        g = g + gamma * D[:, k]
    return g


def hals_spatial(A, A1, Cs, D=None, gamma=0.0, sweeps=1, boxes=None, sz=None):
    """``sweeps`` sweeps from A (P,K); returns float64 (P,K)."""
    A, A1, Cs, D, gamma, M = _inputs(A, A1, Cs, D, gamma, boxes, sz)
    K = A.shape[1]
    for _ in range(int(sweeps)):
        for k in range(K):
            d = Cs[k, k]
            if not (d > 0 and np.isfinite(d)):
                continue
            g = _column_gradient(A, A1, Cs, D, gamma, M, k)
            A[:, k] = np.where(M[:, k], np.maximum(0.0, A[:, k] - g / d), 0.0)
    return A


def gradient(A, A1, Cs, D=None, gamma=0.0, boxes=None, sz=None):
    """g as (P,K) for the state A (zeroed outside the boxes)."""
    A, A1, Cs, D, gamma, M = _inputs(A, A1, Cs, D, gamma, boxes, sz)
    return np.stack([_column_gradient(A, A1, Cs, D, gamma, M, k) for k in range(A.shape[1])], axis=1)


def kkt(A, A1, Cs, D=None, gamma=0.0, boxes=None, sz=None):
    """(K): the largest |pg| over the neuron's support, pg = g where a > 0, else min(g, 0).  Zero exactly at a solution."""
    A, A1, Cs, D, gamma, M = _inputs(A, A1, Cs, D, gamma, boxes, sz)
    g = np.stack([_column_gradient(A, A1, Cs, D, gamma, M, k) for k in range(A.shape[1])], axis=1)
    pg = np.abs(np.where(A > 0, g, np.minimum(g, 0.0)))
    return np.where(M, pg, 0.0).max(0)


def term_sum(A, A1, Cs, D=None, gamma=0.0, boxes=None, sz=None):
    """(P,K): sum_l |a_l Cs[l,k]| + |A1| + gamma |D|, the magnitude of the terms g is made of (the scale of its rounding)."""
    A, A1, Cs, D, gamma, M = _inputs(A, A1, Cs, D, gamma, boxes, sz)
    t = np.abs(A) @ np.abs(Cs) + np.abs(A1)
    if D is not None:
        t = t + abs(gamma) * np.abs(D)
    return t


def objective(A, A1, Cs, D=None, gamma=0.0):
    """sum_p F(a_p), float64."""
    A1 = np.asarray(A1, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64).reshape(A1.shape)
    Cs = np.asarray(Cs, dtype=np.float64)
    f = 0.5 * np.einsum("pk,kl,pl->", A, Cs, A) - float((A1 * A).sum())
    if D is not None:
        f += float(gamma or 0.0) * float((np.asarray(D, dtype=np.float64).reshape(A1.shape) * A).sum())
    return float(f)


def mu_spatial(A, A1, Cs, D=None, gamma=0.0):
    """The multiplicative update K6 in float64: A * A1 / (A Cs + gamma D + 1e-32)."""
    A1 = np.asarray(A1, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64).reshape(A1.shape)
    den = A @ np.asarray(Cs, dtype=np.float64)
    if D is not None:
        den = den + float(gamma or 0.0) * np.asarray(D, dtype=np.float64).reshape(A1.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return A * A1 / (den + 1e-32)


def support_boxes(A, sz):
    """(K,6): the box of the non-zero values of every column of A (P,K); an empty column has lo > hi."""
    X, Y, Z = (int(s) for s in sz)
    nz = np.asarray(A).reshape(X, Y, Z, -1) != 0
    out = np.empty((nz.shape[-1], 6), dtype=np.int64)
    for ax in range(3):
        hit = nz.any(axis=tuple(a for a in range(3) if a != ax))        # (dim, K)
        at = np.arange(nz.shape[ax])[:, None]
        out[:, 2 * ax] = np.where(hit, at, nz.shape[ax]).min(0)
        out[:, 2 * ax + 1] = np.where(hit, at, -1).max(0)
    return out


# ---- the planted video of the ordering tests: footprints deliberately too narrow ------------------------------------
PLANTED_CENTRES = np.array([[5.0, 5.0], [12.0, 4.0], [19.0, 6.0], [6.0, 14.0], [13.0, 13.0], [18.0, 15.0]])
PLANTED_FLOOR = 1e-3      # the narrow footprints are cut here, so that they have a support to grow


def gaussian_footprints(sz, centres, sigma=3.0):
    """(P,K): exp(-|u - centre|^2 / sigma^2), the simulator's Gaussians as the model builds them."""
    X, Y, Z = sz
    g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    d2 = ((g[:, None, :] - np.asarray(centres)[None, :, :]) ** 2).sum(-1)
    return np.exp(-d2 / sigma ** 2)


def planted(depth, T=40, seed=0, noise=0.02):
    """Six Gaussian cells (sigma 3) in a 24 x 20 x depth volume, exact traces (baseline 0.2 plus decaying spikes) and a
    little white noise, clamped at 0 -> dict(video (T,P) float32, A_true (P,6), A_narrow (P,6) float32: sigma 3 / 1.5 and
    cut below PLANTED_FLOOR, C (6,T) float32, centres (6,3), sz)."""
    rng = np.random.default_rng([seed, depth, T])
    sz = (24, 20, depth)
    centres = np.concatenate([PLANTED_CENTRES, np.full((6, 1), 0.5 * (depth - 1))], axis=1)
    A_true = gaussian_footprints(sz, centres)
    A_narrow = gaussian_footprints(sz, centres, sigma=3.0 / 1.5)
    A_narrow[A_narrow < PLANTED_FLOOR] = 0.0
    spikes = (rng.random((6, T)) < 0.15) * rng.uniform(1.0, 2.0, (6, T))
    C = np.zeros((6, T))
    for t in range(T):
        C[:, t] = (0.7 * C[:, t - 1] if t else 0.0) + spikes[:, t]
    C = (C + 0.2).astype(np.float32)
    video = C.astype(np.float64).T @ A_true.T + noise * rng.standard_normal((T, A_true.shape[0]))
    return dict(video=np.maximum(video, 0.0).astype(np.float32), A_true=A_true, A_narrow=A_narrow.astype(np.float32), C=C,
                centres=centres, sz=sz)


def footprint_correlation(A, A_true):
    """Mean over the neurons of the Pearson correlation of a footprint with the true one."""
    A, A_true = np.asarray(A, dtype=np.float64), np.asarray(A_true, dtype=np.float64)
    a, b = A - A.mean(0), A_true - A_true.mean(0)
    return float(((a * b).sum(0) / np.sqrt((a * a).sum(0) * (b * b).sum(0))).mean())


def expand_entries(A1c, tables, ntiles, sz, K):
    """The compact buffer of the list form as (P,K): entry (tile q, slot i, lane, v) at tile_off[q] + 256 i + 4 lane + v
    belongs to voxel x = 4 (q / nu) + lane / 16, u = 64 (q % nu) + 4 (lane % 16) + v and neuron tile_list[q][i]; what no
    tile lists is 0.  ``tables`` as ``ops.spatial_lists_setup`` makes them (int array)."""
    X, Y, Z = (int(s) for s in sz)
    YZ = Y * Z
    nu = (YZ + 63) // 64
    t = np.asarray(tables)
    tile_n, tile_off, lists = t[:ntiles], t[ntiles:2 * ntiles + 1], t[2 * ntiles + 2:].reshape(ntiles, 32)
    out = np.zeros((X * YZ, K), dtype=np.asarray(A1c).dtype)
    for q in range(ntiles):
        for i in range(max(int(tile_n[q]), 0)):
            for lane in range(64):
                x = 4 * (q // nu) + lane // 16
                for v in range(4):
                    u = 64 * (q % nu) + 4 * (lane % 16) + v
                    if x < X and u < YZ:
                        out[x * YZ + u, lists[q, i]] = A1c[tile_off[q] + 256 * i + 4 * lane + v]
    return out
