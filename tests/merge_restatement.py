"""The definition of the merge of duplicate components (K26), in float64 numpy: the pair statistics, the groups, and the merged
component of a group as the rank-1 non-negative factor of sum_k a_k c_k^T, computed in coefficient space.

Boxes are those of K24 (``components_restatement.component_boxes``), by default with margin 0.  A candidate pair is i < j whose
inclusive boxes intersect; the diagonal pairs (k, k) carry the norms.  Per pair (i, j), with a_k = A_rows[k] and c_k = C[k]:

    saa    = sum a_i a_j over the intersection of the two boxes (0 when it is empty; (k, k): sum a_k^2 over the neuron's own box)
    n      = the frames where both traces are finite, t0 the first of them
    si, sj, sii, sjj, sij = sum d_i, d_j, d_i^2, d_j^2, d_i d_j over those frames, d = c - c[t0]: a constant trace has si = sii = 0
             exactly, whatever its value
    scc    = sum c_i c_j over those frames, not shifted
    overlap = saa_ij / sqrt(saa_ii saa_jj), 0 when a norm is 0
    corr    = (n sij - si sj) / sqrt((n sii - si^2)(n sjj - sj^2)), NaN when n < 2 or a variance is not positive

An edge is ``corr >= thr and overlap >= min_overlap`` (NaN fails).  Groups are the connected components of the edges, members
ascending, groups ordered by their lowest member.

A group g of m >= 2 members becomes a' = sum_k u_k a_k, c' = sum_k w_k c_k.  With S the m x m block of saa (every member pair, 0
where the boxes are disjoint) and Q that of scc, from u_k = sqrt(Q_kk), ``iters`` rounds of

    w = S u / (u^T S u)          u = Q w / (w^T Q w)

which are the alternating least-squares steps c' = M^T a' / |a'|^2, a' = M c' / |c'|^2 on M = sum_k a_k c_k^T written in the
coefficients: with A, C >= 0 every entry stays >= 0 and the clamp of the non-negative iteration never acts.  Then u is scaled so
that |a'|^2 = u^T S u equals saa_dd of the dominant member d, the one with the largest sqrt(saa_kk Q_kk), and w inversely.
pos' is the mean of the members' pos weighted by sqrt(saa_kk Q_kk), sigma' is member d's, D[..., g] = 1 - exp(-0.01 |voxel - pos'|).
A merged row of C with a negative or non-finite entry is refused.
"""
import math

import numpy as np

from components_restatement import box_voxels, component_boxes, gaussian_footprints  # noqa: F401  (the boxes are K24's)

SUMS = ("saa", "n", "si", "sj", "sii", "sjj", "sij", "scc")


def candidate_pairs(boxes):
    """(N, 2) int: every (k, k) and every i < j whose inclusive boxes intersect, i ascending, then j."""
    b = np.asarray(boxes).astype(np.int64)
    K = b.shape[0]
    out = []
    for i in range(K):
        for j in range(i, K):
            if all(b[i, 2 * d] <= b[j, 2 * d + 1] and b[j, 2 * d] <= b[i, 2 * d + 1] for d in range(3)):
                out.append((i, j))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def group_pairs(groups):
    """(N, 2): every i <= j of every group with two members or more, group by group."""
    out = [(g[a], g[b]) for g in groups if len(g) >= 2 for a in range(len(g)) for b in range(a, len(g))]
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def intersection(bi, bj):
    """The inclusive box both boxes share, or None."""
    q = []
    for d in range(3):
        lo, hi = max(int(bi[2 * d]), int(bj[2 * d])), min(int(bi[2 * d + 1]), int(bj[2 * d + 1]))
        if lo > hi:
            return None
        q += [lo, hi]
    return q


def pair_stats(A_rows, sz, boxes, C, pairs=None):
    """A_rows (K, P), boxes (K, 6), C (K, T; NaN allowed), pairs (N, 2) or None (``candidate_pairs``) -> dict of float64 arrays
    (N,): the eight sums of ``SUMS``, ``overlap`` and ``corr``, ``pairs`` (N, 2) int64, and ``<sum>_mag``, the sum of the magnitudes
    of the terms of each sum: the scale its rounding is measured on.  ``overlap`` of a pair whose diagonals are not listed is NaN."""
    A_rows = np.asarray(A_rows, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    boxes = np.asarray(boxes)
    pairs = candidate_pairs(boxes) if pairs is None else np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    N = pairs.shape[0]
    out = {k: np.zeros(N) for k in SUMS}
    out.update({k + "_mag": np.zeros(N) for k in SUMS})
    for p, (i, j) in enumerate(pairs):
        q = intersection(boxes[i], boxes[j])
        if q is not None:
            v = box_voxels(q, sz)
            out["saa"][p] = (A_rows[i, v] * A_rows[j, v]).sum()
            out["saa_mag"][p] = np.abs(A_rows[i, v] * A_rows[j, v]).sum()
        ok = np.isfinite(C[i]) & np.isfinite(C[j])
        out["n"][p] = out["n_mag"][p] = ok.sum()
        if ok.any():
            ci, cj = C[i, ok], C[j, ok]
            di, dj = ci - ci[0], cj - cj[0]
            for name, terms in (("si", di), ("sj", dj), ("sii", di * di), ("sjj", dj * dj), ("sij", di * dj), ("scc", ci * cj)):
                out[name][p], out[name + "_mag"][p] = terms.sum(), np.abs(terms).sum()
    out["pairs"] = pairs
    out["overlap"], out["corr"] = derived(pairs, out)
    return out


def derived(pairs, s):
    """``(overlap, corr)`` of the sums ``s``."""
    diag = {int(i): s["saa"][p] for p, (i, j) in enumerate(pairs) if i == j}
    N = len(pairs)
    overlap, corr = np.full(N, np.nan), np.full(N, np.nan)
    for p, (i, j) in enumerate(pairs):
        if int(i) in diag and int(j) in diag:
            den = diag[int(i)] * diag[int(j)]
            overlap[p] = s["saa"][p] / math.sqrt(den) if den > 0.0 else 0.0
        n = s["n"][p]
        va, vb = n * s["sii"][p] - s["si"][p] ** 2, n * s["sjj"][p] - s["sj"][p] ** 2
        if n >= 2 and va > 0.0 and vb > 0.0:
            corr[p] = (n * s["sij"][p] - s["si"][p] * s["sj"][p]) / math.sqrt(va * vb)
    return overlap, corr


def groups_of(stats, K, thr, min_overlap):
    """The connected components of the edges, as a list of lists of indices: members ascending, groups by their lowest member."""
    parent = list(range(K))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for (i, j), c, o in zip(stats["pairs"], stats["corr"], stats["overlap"]):
        if i != j and c >= thr and o >= min_overlap:           # a NaN compares False
            a, b = find(int(i)), find(int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)                   # the root is the lowest member
    members = {}
    for k in range(K):
        members.setdefault(find(k), []).append(k)
    return [members[r] for r in sorted(members)]


def rank1_coefficients(S, Q, iters=10):
    """The coefficient-space iteration, unscaled: ``(u, w)``."""
    S, Q = np.asarray(S, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    u = np.sqrt(np.diag(Q))
    w = np.zeros_like(u)
    for _ in range(iters):
        w = S @ u / (u @ S @ u)
        u = Q @ w / (w @ Q @ w)
    return u, w


def rank1_dense(A, C, iters=10):
    """The same rounds as explicit clamped iterations on the dense M = A C (A (P, m), C (m, T)) -> ``(a', c', clamped)``:
    ``clamped`` counts the entries a clamp changed."""
    M = A @ C
    a = A @ np.sqrt((C * C).sum(1))
    c, clamped = None, 0
    for _ in range(iters):
        c = M.T @ a / (a @ a)
        clamped += int((c < 0).sum())
        c = np.maximum(c, 0.0)
        a = M @ c / (c @ c)
        clamped += int((a < 0).sum())
        a = np.maximum(a, 0.0)
    return a, c, clamped


def block(stats, g, name):
    """The m x m symmetric block of ``stats[name]`` on the members g; a pair that is not listed is an error."""
    at = {(int(i), int(j)): p for p, (i, j) in enumerate(stats["pairs"])}
    m = len(g)
    B = np.zeros((m, m))
    for a in range(m):
        for b in range(a, m):
            B[a, b] = B[b, a] = stats[name][at[(g[a], g[b])]]
    return B


def merge_weights(S, Q, iters=10):
    """``(u, w, d, weight)`` of one group: the scaled coefficients, the position of the dominant member, sqrt(saa_kk Q_kk)."""
    u, w = rank1_coefficients(S, Q, iters)
    weight = np.sqrt(np.diag(S) * np.diag(Q))
    d = int(np.argmax(weight))                                   # the first of equals
    scale = math.sqrt(S[d, d] / (u @ S @ u))
    return u * scale, w / scale, d, weight


def plan(stats, K, thr, min_overlap, iters=10, group_stats=None):
    """dict(groups, u, w, dominant, weight): ``u``, ``w`` and ``weight`` lists of arrays in member order (1 for a singleton),
    ``dominant`` the old index of each group's dominant member.  S and Q come from ``group_stats`` (else ``stats``)."""
    gs = stats if group_stats is None else group_stats
    groups = groups_of(stats, K, thr, min_overlap)
    out = dict(groups=groups, u=[], w=[], dominant=[], weight=[])
    for g in groups:
        if len(g) == 1:
            u, w, d, weight = np.ones(1), np.ones(1), 0, np.ones(1)
        else:
            u, w, d, weight = merge_weights(block(gs, g, "saa"), block(gs, g, "scc"), iters)
        out["u"].append(u), out["w"].append(w), out["dominant"].append(g[d]), out["weight"].append(weight)
    return out


def apply(A, C, pl):
    """A (P, K), C (K, T) -> ``(A' (P, K'), C' (K', T))`` in float64."""
    A, C = np.asarray(A, dtype=np.float64), np.asarray(C, dtype=np.float64)
    for g in pl["groups"]:
        if len(g) >= 2 and not (np.isfinite(C[g]).all() and (C[g] >= 0).all()):
            raise ValueError(f"merge: the traces of the group {g} have negative or non-finite entries")
    A2 = np.stack([A[:, g] @ u for g, u in zip(pl["groups"], pl["u"])], axis=1)
    C2 = np.stack([w @ C[g] for g, w in zip(pl["groups"], pl["w"])], axis=0)
    return A2, C2


def merged_positions(pos, pl):
    pos = np.asarray(pos, dtype=np.float64)
    return np.stack([(wt[:, None] * pos[g]).sum(0) / wt.sum() for g, wt in zip(pl["groups"], pl["weight"])])


def distance_prior(sz, pos):
    """The constructor's D: 1 - exp(-0.01 |voxel - pos_k|), (X, Y, Z, K)."""
    X, Y, Z = sz
    g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).astype(np.float64)
    d = np.sqrt(((g[..., None, :] - np.asarray(pos, dtype=np.float64)[None, None, None]) ** 2).sum(-1))
    return 1 - np.exp(-.01 * d)


def merge(A, sz, C, thr=0.85, min_overlap=0.1, floor=1e-3, margin=0, traces=None, iters=10):
    """The whole merge of footprints A (P, K) and traces C (K, T): ``(stats, plan)``; the correlations on ``traces`` when given."""
    A = np.asarray(A, dtype=np.float64)
    boxes = component_boxes(A, sz, floor, margin)
    st = pair_stats(A.T, sz, boxes, C if traces is None else traces)
    groups = groups_of(st, A.shape[1], thr, min_overlap)
    gs = pair_stats(A.T, sz, boxes, C, pairs=group_pairs(groups))
    return st, plan(st, A.shape[1], thr, min_overlap, iters, group_stats=gs)


# ---- the planted model -------------------------------------------------------------------------------------------------------------
# six cells (x, y): 0 and 1 are each split into two components a voxel apart, 2 and 3 are distinct cells 1.5 sigma apart with
# independent traces, 4 and 5 share one trace and lie 8.6 voxels apart: their boxes intersect, their footprints hardly overlap
SIGMA = 3.0
PLANTED_CELLS = np.array([[6.0, 5.0], [17.0, 14.0], [5.0, 14.5], [9.5, 14.5], [19.0, 3.0], [12.0, 8.0]])
PLANTED_SPLITS = [[0, 1], [2, 3]]                    # component indices of the two split cells
PLANTED_CELL_OF = [0, 0, 1, 1, 2, 3, 4, 5]           # component -> cell
PLANTED_NOISE = 0.05


def planted_model(depth, seed, T=40, noise=PLANTED_NOISE, g=0.74, rate=0.25):
    """-> ``(A (P, 8), C (8, T), pos (8, 3), cell_traces (6, T), sz)``: Gaussian footprints of width ``SIGMA`` and AR(1) traces,
    built directly.  A split cell's two components sit half a voxel either side of its centre (along x for cell 0, along y for
    cell 1); their traces are f c and (1 - f) c with f uniform in [0.3, 0.7], plus white noise of ``noise`` times the component's own
    rms, clamped at 0.  (Noise in proportion to the component: the merged trace is close to the plain sum of the halves, which
    beats the better half where each half carries its share of the noise; with equal absolute noise on an uneven split the
    sum can fall just below the better half -- 0.9911 against 0.9923 was seen -- because the sum is not the noise-optimal
    combination, and the merge does not claim to be.)"""
    rng = np.random.default_rng([seed, depth, T])
    sz = (24, 20, depth)
    z = 0.5 * (depth - 1)
    spikes = (rng.random((6, T)) < rate) * rng.uniform(1.0, 2.0, (6, T))
    spikes[:, 0] += rng.uniform(0.5, 1.0, 6)
    cells = np.zeros((6, T))
    for t in range(T):
        cells[:, t] = (g * cells[:, t - 1] if t else 0.0) + spikes[:, t]
    cells[5] = cells[4]
    half = np.array([[0.5, 0.0], [0.0, 0.5]])
    centres, C = [], []
    for k, cell in enumerate(PLANTED_CELL_OF):
        if cell < 2:
            first = PLANTED_SPLITS[cell][0] == k
            centres.append(PLANTED_CELLS[cell] + (-half[cell] if first else half[cell]))
            if first:
                f = rng.uniform(0.3, 0.7)
            C.append((f if first else 1.0 - f) * cells[cell])
        else:
            centres.append(PLANTED_CELLS[cell])
            C.append(cells[cell].copy())
    C = np.stack(C)
    rms = np.sqrt((C ** 2).mean(1))
    C = np.maximum(C + noise * rms[:, None] * rng.standard_normal(C.shape), 0.0)
    pos = np.concatenate([np.stack(centres), np.full((8, 1), z)], axis=1)
    return gaussian_footprints(sz, pos, SIGMA), C, pos, cells, sz
