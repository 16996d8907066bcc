"""The definition of K28 -- new components from the residual -- in float64 numpy, written plainly: the candidate boxes, the
residual gathered on them (K28a), its non-negative rank-1 factor (K28b), and the arrays of the model that has grown by the
candidates kept.

Everything lives in footprint coordinates.  Candidate m has a centre, a box ``(x0, x1, y0, y1, z0, z1)``, inclusive, of n_m voxels
v_j in the order x slowest, z fastest (K24's numbering), and on it

    e[m, t, j] = frames_t(v_j) - sub_t(v_j)         one fp32 subtraction, as the kernel takes it; 0 for j >= n_m

The valid frames V of a candidate are those whose n_m samples are all finite.  From a start a0:

    repeat iters times    c_t = max(sum_j a_j e_tj, 0) / sum_j a_j^2   (t in V)
                          a_j = max(sum_{t in V} c_t e_tj, 0) / sum_{t in V} c_t^2
    finish                a *= sqrt(sum a0^2 / sum a^2), then the c-step once more

    energy = sum_{V, j} e^2        explained = 2 sum_{t in V} c_t <a, e_t> - |a|^2 |c|^2

``explained`` is what a c^T takes off the energy: |E|^2 - |E - a c^T|^2 over the valid frames.  At the exact c-step it equals
|a|^2 |c|^2, so 0 <= explained <= energy.  c is NaN outside V.  A candidate whose sum a^2 or sum c^2 is not a positive finite
number at any step, or whose V is empty, is refused: ``ok = 0``, a and c NaN, explained and the norms NaN; energy and n_valid
stay those of its frames.

All candidates are fitted on the same residual, independently.  The sequential greedy method (pick, fit, subtract, pick again)
is not this: two candidates on one cell both come out as that cell, and are left to ``merge_components``.
"""
import math

import numpy as np


# ---- boxes and the gather (K28a) -------------------------------------------------------------------------------------------------
def box_voxels(box, sz):
    """Flat voxel indices p = (x Y + y) Z + z of the box, x slowest, z fastest."""
    X, Y, Z = (int(s) for s in sz)
    x0, x1, y0, y1, z0, z1 = (int(b) for b in box)
    assert 0 <= x0 <= x1 < X and 0 <= y0 <= y1 < Y and 0 <= z0 <= z1 < Z, (box, sz)
    x, y, z = np.meshgrid(np.arange(x0, x1 + 1), np.arange(y0, y1 + 1), np.arange(z0, z1 + 1), indexing="ij")
    return ((x * Y + y) * Z + z).reshape(-1)


def box_coords(box):
    """(n, 3) float64 voxel coordinates of the box in the same order."""
    x0, x1, y0, y1, z0, z1 = (int(b) for b in box)
    x, y, z = np.meshgrid(np.arange(x0, x1 + 1), np.arange(y0, y1 + 1), np.arange(z0, z1 + 1), indexing="ij")
    return np.stack((x, y, z), -1).reshape(-1, 3).astype(np.float64)


def candidate_boxes(centres, sz, half):
    """(M, 6) int32: per centre the voxel floor(centre + 0.5), moved into the volume, +- ``half`` (one number or one per axis)
    voxels, cut to the volume."""
    centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    half = np.broadcast_to(np.asarray(half, dtype=np.int64), (3,))
    assert (half >= 0).all()
    boxes = np.zeros((centres.shape[0], 6), dtype=np.int32)
    for d, S in enumerate(int(s) for s in sz):
        c = np.clip(np.floor(centres[:, d] + 0.5).astype(np.int64), 0, S - 1)
        boxes[:, 2 * d] = np.maximum(c - half[d], 0)
        boxes[:, 2 * d + 1] = np.minimum(c + half[d], S - 1)
    return boxes


def box_sizes(boxes):
    b = np.asarray(boxes, dtype=np.int64)
    return (b[:, 1::2] - b[:, 0::2] + 1).prod(1)


def residual_boxes(frames, sz, boxes, sub=None, vmax=None):
    """frames (T, P), sub (T, P) or None -> E (M, T, vmax) float32, 0 past a box's n.  A sample that is not finite stays."""
    frames = np.asarray(frames, dtype=np.float32)
    boxes = np.asarray(boxes)
    nvox = box_sizes(boxes)
    vmax = int(nvox.max()) if vmax is None else int(vmax)
    E = np.zeros((boxes.shape[0], frames.shape[0], vmax), dtype=np.float32)
    for m, b in enumerate(boxes):
        u = box_voxels(b, sz)
        e = frames[:, u]
        if sub is not None:
            with np.errstate(invalid="ignore"):
                e = (e - np.asarray(sub, dtype=np.float32)[:, u]).astype(np.float32)
        E[m, :, :u.size] = e
    return E


# ---- the rank-1 factor (K28b) ----------------------------------------------------------------------------------------------------
def _positive(v):
    return bool(v > 0.0 and math.isfinite(v))


def rank1_one(e, a0, iters=5):
    """e (T, n) the residual on one box, a0 (n,) -> dict: a (n,), c (T,), energy, explained, saa, scc, n_valid, ok, and ``*_mag``:
    the sums of the magnitudes of the terms behind c, a and the four figures, the scale their rounding is measured on."""
    e = np.asarray(e, dtype=np.float64)
    a = np.asarray(a0, dtype=np.float64).copy()
    T, n = e.shape
    assert iters >= 1 and a.shape == (n,)
    V = np.isfinite(e).all(1)
    ev = e[V]
    nan = math.nan
    out = dict(a=np.full(n, nan), c=np.full(T, nan), energy=float((ev * ev).sum()), explained=nan, saa=nan, scc=nan,
               n_valid=int(V.sum()), ok=0, a_mag=np.full(n, nan), c_mag=np.full(T, nan), explained_mag=nan)
    norm0 = float((a * a).sum())
    if not _positive(norm0) or not V.any():
        return out
    saa, a_mag = norm0, None
    for it in range(iters + 1):
        if it == iters:
            s = math.sqrt(norm0 / saa)
            a, a_mag = a * s, a_mag * s
            saa = float((a * a).sum())
            if not _positive(saa):
                return out
        dot = ev @ a
        c = np.maximum(dot, 0.0) / saa
        scc = float((c * c).sum())
        if not _positive(scc):
            return out
        if it == iters:
            break
        num = c @ ev
        a_mag = np.abs(c[:, None] * ev).sum(0) / scc
        a = np.maximum(num, 0.0) / scc
        saa = float((a * a).sum())
        if not _positive(saa):
            return out
    mag_t = np.abs(ev * a[None, :]).sum(1)
    out.update(a=a, a_mag=a_mag, ok=1, saa=saa, scc=scc, explained=2.0 * float((c * dot).sum()) - saa * scc,
               explained_mag=2.0 * float((c * mag_t).sum()) + saa * scc)
    out["c"][V] = c
    out["c_mag"][V] = mag_t / saa
    return out


def rank1_nmf(E, nvox, a0, iters=5):
    """E (M, T, vmax), nvox (M,), a0 (M, vmax) -> dict of arrays over the candidates: a (M, vmax; 0 past a box's n), c (M, T),
    energy, explained, saa, scc (M,), n_valid, ok (M,) int, and the ``*_mag`` of ``rank1_one``."""
    E = np.asarray(E)
    M, T, vmax = E.shape
    out = dict(a=np.zeros((M, vmax)), c=np.zeros((M, T)), a_mag=np.zeros((M, vmax)), c_mag=np.zeros((M, T)),
               n_valid=np.zeros(M, dtype=np.int32), ok=np.zeros(M, dtype=np.int32))
    for name in ("energy", "explained", "saa", "scc", "explained_mag"):
        out[name] = np.zeros(M)
    for m in range(M):
        n = int(nvox[m])
        assert 1 <= n <= vmax
        r = rank1_one(E[m, :, :n], np.asarray(a0)[m, :n], iters)
        for name in ("a", "a_mag"):
            out[name][m, :n] = r[name]
        for name in ("c", "c_mag", "energy", "explained", "saa", "scc", "explained_mag", "n_valid", "ok"):
            out[name][m] = r[name]
    return out


def gaussian_start(boxes, centres, shape_std, vmax=None):
    """a0 (M, vmax) float32: exp(-|u - centre|^2 / shape_std^2) on the voxels u of each box -- the footprint the model builds -- 0 past
    a box's n."""
    boxes = np.asarray(boxes)
    centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    vmax = int(box_sizes(boxes).max()) if vmax is None else int(vmax)
    a0 = np.zeros((boxes.shape[0], vmax), dtype=np.float32)
    for m, b in enumerate(boxes):
        u = box_coords(b)
        a0[m, :u.shape[0]] = np.exp(-((u - centres[m][None, :]) ** 2).sum(1) / float(shape_std) ** 2)
    return a0


def default_half(shape_std, sz):
    """ceil(2 shape_std) voxels per axis, 0 along an axis of extent 1."""
    h = int(math.ceil(2.0 * float(shape_std)))
    return [0 if int(s) == 1 else h for s in sz]


# ---- the grown model ---------------------------------------------------------------------------------------------------------------
def centre_of_mass(a, box):
    a = np.asarray(a, dtype=np.float64)
    return (a[:, None] * box_coords(box)).sum(0) / a.sum()


def grown(A, C, pos, sigma, D, sz, boxes, a, c, kept, times, shape_std):
    """The arrays of the model after the candidates ``kept`` (indices) were appended: A (P, K) float32, C (K, T) float32, pos (K, 3)
    float32, sigma (K,) float32, D (X, Y, Z, K) float64 or None -> the same with K + len(kept).  a (M, vmax) and c (M, n) as the
    kernel returns them in fp32, c at the times ``times`` (n,); a frame outside V (c NaN) and a time that was not served get 0."""
    A, C = np.asarray(A, dtype=np.float32), np.asarray(C, dtype=np.float32)
    P, T = A.shape[0], C.shape[1]
    cols, rows, centres = [], [], []
    for m in kept:
        u = box_voxels(boxes[m], sz)
        col = np.zeros(P, dtype=np.float32)
        col[u] = np.asarray(a, dtype=np.float32)[m, :u.size]
        row = np.zeros(T, dtype=np.float32)
        row[np.asarray(times)] = np.nan_to_num(np.asarray(c, dtype=np.float32)[m], nan=0.0)
        cols.append(col), rows.append(row)
        centres.append(centre_of_mass(np.asarray(a)[m, :u.size], boxes[m]).astype(np.float32))
    A2 = np.concatenate([A, np.stack(cols, 1)], 1)
    C2 = np.concatenate([C, np.stack(rows, 0)], 0)
    pos2 = np.concatenate([np.asarray(pos, dtype=np.float32), np.stack(centres, 0)], 0)
    sigma2 = np.concatenate([np.asarray(sigma, dtype=np.float32), np.full(len(kept), shape_std, dtype=np.float32)])
    D2 = None
    if D is not None:
        X, Y, Z = (int(s) for s in sz)
        g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
        d = np.sqrt(((g[:, None, :] - np.stack(centres, 0).astype(np.float64)[None, :, :]) ** 2).sum(-1))
        D2 = np.concatenate([np.asarray(D), (1.0 - np.exp(-0.01 * d)).reshape(X, Y, Z, len(kept))], -1)
    return dict(A=A2, C=C2, pos=pos2, sigma=sigma2, D=D2)


def add_components(frames, sz, A, C, centres, shape_std, half=None, iters=5, min_explained=0.5, sub=None):
    """The whole step on registered frames (T, P), the model's footprints A (P, K) and traces C (K, T), and candidate centres (M, 3):
    boxes, the residual (``sub``: the model's prediction (T, P), default A C in float64 rounded to fp32), the Gaussian start, the
    factor, and ``kept``: ok and explained / energy >= min_explained."""
    boxes = candidate_boxes(centres, sz, default_half(shape_std, sz) if half is None else half)
    if sub is None:
        sub = (np.asarray(A, dtype=np.float64) @ np.asarray(C, dtype=np.float64)).T.astype(np.float32)
    E = residual_boxes(frames, sz, boxes, sub=sub)
    nvox = box_sizes(boxes)
    a0 = gaussian_start(boxes, centres, shape_std)
    fit = rank1_nmf(E, nvox, a0, iters)
    with np.errstate(invalid="ignore", divide="ignore"):
        fit["ratio"] = fit["explained"] / fit["energy"]
        fit["kept"] = (fit["ok"] == 1) & (fit["ratio"] >= min_explained)
    fit.update(boxes=boxes, nvox=nvox, a0=a0, E=E)
    return fit


# ---- the planted video -------------------------------------------------------------------------------------------------------------
CELLS = np.array([[5.0, 4.0], [5.0, 14.0], [12.0, 5.0], [12.0, 15.0], [19.0, 4.0], [19.0, 14.0]])
WIDTHS = np.array([[3.0, 3.0], [3.0, 3.0], [3.0, 3.0], [3.0, 3.0], [3.0, 1.8], [1.8, 2.8]])     # (x, y); z takes the mean of the two
MISSING = (4, 5)                                     # the cells the model does not have: the two anisotropic ones
NOTHING = np.array([[8.5, 9.5], [2.0, 9.5]])         # between cells the model has: boxes that reach none of the missing ones
SHAPE_STD = 3.0                                      # the width of the model's footprints, and of the start
NOISE, G, RATE = 0.1, 0.74, 0.12
# The seed of the GPU fit test per depth: one for which the float64 definition (detection on the residual image, then this file)
# keeps the two missing cells and nothing else out of four picks.  The third and fourth picks are noise peaks; where one lands
# within a box's reach of a missing cell it scores like that cell (tests/test_add_host.py prints every seed's).
FIT_SEED = {2: 1, 1: 0}


def planted_centres(depth, xy=CELLS):
    return np.concatenate([xy, np.full((len(xy), 1), 0.5 * (depth - 1))], axis=1)


def planted_footprints(sz, depth):
    """(P, 6): cell k = exp(-sum_d (u_d - centre_d)^2 / width_d^2); the first four are the model's own Gaussians of width 3."""
    X, Y, Z = sz
    g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    w = np.concatenate([WIDTHS, WIDTHS.mean(1, keepdims=True)], 1)
    d2 = (((g[:, None, :] - planted_centres(depth)[None, :, :]) / w[None, :, :]) ** 2).sum(-1)
    return np.exp(-d2)


def planted_video(depth, seed, T=40):
    """Six cells with AR(1) traces (decay 0.74, spikes of height 1..2 at 0.12 a frame) and white noise 0.1, clamped at 0, in a
    24 x 20 x depth volume -> ``(video (T, P) float32, A6 (P, 6), traces (6, T), sz)``."""
    rng = np.random.default_rng([seed, depth, T, 28])
    sz = (24, 20, depth)
    A6 = planted_footprints(sz, depth)
    spikes = (rng.random((6, T)) < RATE) * rng.uniform(1.0, 2.0, (6, T))
    spikes[:, 0] += rng.uniform(0.0, 1.0, 6)
    traces = np.zeros((6, T))
    for t in range(T):
        traces[:, t] = (G * traces[:, t - 1] if t else 0.0) + spikes[:, t]
    video = traces.T @ A6.T + NOISE * rng.standard_normal((T, A6.shape[0]))
    return np.maximum(video, 0.0).astype(np.float32), A6, traces, sz


def nnls_traces(video, A):
    """The exact non-negative least-squares traces of every frame, (K, T)."""
    from scipy.optimize import nnls
    return np.stack([nnls(np.asarray(A, dtype=np.float64), np.asarray(y, dtype=np.float64))[0] for y in video], axis=1)
