"""The definition of the footprint clean-up (K27), in numpy: median filter, energy (or maximum) cut, morphological closing, largest
face-connected part.  Every output is an integer or a bit pattern: the only floating-point arithmetic is one sequential float64
sum of squares and two float64 products, so an implementation either has these bits or is wrong -- there is no tolerance.

``clean_footprint(a, box, ...)`` takes one neuron: ``a`` its (X, Y, Z) fp32 volume, ``box`` inclusive (x0, x1, y0, y1, z0, z1).
A voxel's linear index is p = (x Y + y) Z + z; "box order" is ascending p.

1.  Validity.  ok = 0, and the column comes back bit for bit, when a value of ``a`` inside the box is not finite or is negative,
    when no value in the box is positive, or when nothing survives step 3.  The step never deletes a component.  (A median of
    step 2 can be non-finite or negative only through taps outside the box; such a neuron is ok = 0 as well.)
2.  Median (``median=True``).  m[v] = the median of the 3 x 3 x 3 neighbourhood of v in the VOLUME ``a`` (taps outside the box are
    the true values; an axis of extent 1 makes it 3 x 3 x 1; a coordinate outside the volume is clamped to it):
    ``scipy.ndimage.median_filter(a, size, mode='nearest')`` read on the box.  27 or 9 values: the median is one of them, nothing is
    computed.  The values are ordered as IEEE totalOrder does (-0.0 below +0.0, every NaN above +inf), so that the median's bits are
    unique.  ``median=False``: m = a.
3.  Cut, on the box voxels.  'nrg': v[0..n) = the box values of m, descending; cum[j] = the float64 sum of (double)v[i]^2, i <= j,
    added in that order (np.cumsum); j* = the first j with cum[j] >= nrgthr cum[n - 1]; thr = v[j*]; keep = (m >= thr) & (m > 0):
    every tie of the threshold is kept.  'max': thr = maxthr (double)max(m), keep = (double)m > thr.
4.  Closing (``closing=True``): dilation by the full 3 x 3 x 3 element with 0 outside the box, then erosion with 1 outside the box.
5.  Largest part: face-connected (6 neighbours) parts of the closed mask, size = voxels, a tie to the part with the lowest linear
    index.
6.  Values: on the chosen part m (``values='filtered'``) or a (``'original'``); 0 elsewhere in the column, outside the box too.

Statistics: int32 ok, n_box, n_cut, n_closed, n_parts, n_kept; float64 threshold; float64 energy = cum[j*] / cum[n - 1] (NaN for
'max').  With ok = 0 the four counts after n_box are 0 and threshold and energy are NaN.

Two deliberate departures from CaImAn's ``threshold_components``: the cut is ``>=`` at the first index that reaches the energy, all
ties kept (there: argmin |cum - thr| and ``>``), and a part's size is its voxel count (there: its energy).  Both make the result
exact.
"""
import numpy as np

STAT_INTS = ("ok", "n_box", "n_cut", "n_closed", "n_parts", "n_kept")
STAT_FLOATS = ("threshold", "energy")


def _keys(a):
    """fp32 -> uint32 keys in IEEE totalOrder, every NaN the top key."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    k = np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(a), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def _values(k):
    u = np.where(k >> 31 != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return np.where(k == np.uint32(0xFFFFFFFF), np.uint32(0x7FC00000), u).astype(np.uint32).view(np.float32)


def median3(a):
    """Step 2 on a whole (X, Y, Z) fp32 volume."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    k = _keys(a)
    idx = [np.arange(S) for S in a.shape]
    taps = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in ((-1, 0, 1) if a.shape[2] > 1 else (0,)):
                cl = [np.clip(i + d, 0, S - 1) for i, d, S in zip(idx, (dx, dy, dz), a.shape)]
                taps.append(k[np.ix_(*cl)])
    taps = np.sort(np.stack(taps), axis=0)
    return _values(taps[len(taps) // 2])


def _shifted(mask, d, axis, fill):
    """mask read at +d along axis, ``fill`` outside."""
    out = np.full_like(mask, fill)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    n = mask.shape[axis]
    if d > 0:
        src[axis], dst[axis] = slice(d, n), slice(0, n - d)
    elif d < 0:
        src[axis], dst[axis] = slice(0, n + d), slice(-d, n)
    out[tuple(dst)] = mask[tuple(src)]
    return out


def _morph(mask, fill):
    """Dilation (fill = False: or over the 27 taps) or erosion (fill = True: and), separably: the element is a full cube."""
    out = mask
    for axis in range(3):
        lo, hi = _shifted(out, -1, axis, fill), _shifted(out, 1, axis, fill)
        out = (out & lo & hi) if fill else (out | lo | hi)
    return out


def close3(keep):
    """Step 4 on a box mask."""
    return _morph(_morph(keep, False), True)


def label_faces(mask):
    """Step 5's labels: int64, -1 outside the mask, else the lowest box-linear index of the voxel's face-connected part."""
    n = mask.size
    lab = np.where(mask, np.arange(n).reshape(mask.shape), n)
    for _ in range(n + 1):
        new = lab
        for axis in range(3):
            for d in (-1, 1):
                new = np.minimum(new, _shifted(lab, d, axis, n))
        new = np.where(mask, new, n)
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(mask, lab, -1)


def cut_nrg(mb, nrgthr):
    """Step 3, 'nrg', on the box values mb (all finite and >= 0, one positive) -> (keep, thr, energy, cum, v)."""
    v = np.sort(mb.ravel())[::-1]
    cum = np.cumsum(v.astype(np.float64) ** 2)
    j = int(np.argmax(cum >= np.float64(nrgthr) * cum[-1]))
    thr = v[j]
    return (mb >= thr) & (mb > 0), float(thr), float(cum[j] / cum[-1]), cum, v


def clean_footprint(a, box, method='nrg', nrgthr=0.9999, maxthr=0.2, median=True, closing=True, values='filtered'):
    """One neuron -> (column (X, Y, Z) fp32, dict of the eight statistics).  See the module docstring."""
    if method not in ('nrg', 'max') or values not in ('filtered', 'original'):
        raise ValueError("method is 'nrg' or 'max', values 'filtered' or 'original'")
    if method == 'nrg' and not 0 < nrgthr <= 1:
        raise ValueError("nrgthr must be in (0, 1]")
    if method == 'max' and not maxthr >= 0:
        raise ValueError("maxthr must be >= 0")
    a = np.ascontiguousarray(a, dtype=np.float32)
    x0, x1, y0, y1, z0, z1 = (int(b) for b in box)
    sl = (slice(x0, x1 + 1), slice(y0, y1 + 1), slice(z0, z1 + 1))
    ab = a[sl]
    st = dict(ok=0, n_box=ab.size, n_cut=0, n_closed=0, n_parts=0, n_kept=0, threshold=float("nan"), energy=float("nan"))

    def good(b):
        return bool(np.isfinite(b).all() and not (b < 0).any() and (b > 0).any())

    if not good(ab):
        return a.copy(), st
    mb = median3(a)[sl] if median else ab
    if not good(mb):
        return a.copy(), st
    if method == 'nrg':
        keep, thr, energy, _, _ = cut_nrg(mb, nrgthr)
    else:
        thr = float(np.float64(maxthr) * np.float64(mb.max()))
        keep, energy = mb.astype(np.float64) > thr, float("nan")
    if not keep.any():
        return a.copy(), st
    closed = close3(keep) if closing else keep
    lab = label_faces(closed)
    roots, counts = np.unique(lab[closed], return_counts=True)         # roots ascending: argmax takes the lowest of a tie
    part = lab == roots[int(np.argmax(counts))]
    out = np.zeros_like(a)
    out[sl] = np.where(part, mb if values == 'filtered' else ab, np.float32(0))
    st.update(ok=1, n_cut=int(keep.sum()), n_closed=int(closed.sum()), n_parts=len(roots), n_kept=int(part.sum()), threshold=thr,
              energy=energy)
    return out, st


def clean_footprints(A, sz, boxes, **kw):
    """``A`` (P, K) or (X, Y, Z, K) fp32 -> (A_out of the same shape, dict of (K,) arrays: int32 and float64)."""
    A = np.ascontiguousarray(A, dtype=np.float32)
    X, Y, Z = (int(s) for s in sz)
    K = A.shape[-1]
    A4 = A.reshape(X, Y, Z, K)
    out = np.empty_like(A4)
    rows = []
    for k in range(K):
        out[..., k], st = clean_footprint(A4[..., k], np.asarray(boxes)[k], **kw)
        rows.append(st)
    stats = {n: np.array([r[n] for r in rows], dtype=np.int32) for n in STAT_INTS}
    stats.update({n: np.array([r[n] for r in rows], dtype=np.float64) for n in STAT_FLOATS})
    return out.reshape(A.shape), stats


# ---- the planted cases the host and the GPU tests share ---------------------------------------------------------------------------
def gaussian_cell(sz, centre, sigma=2.5, floor=0.02):
    """exp(-|v - centre|^2 / (2 sigma^2)) as fp32, values below ``floor`` set to 0."""
    g = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sz], indexing="ij")
    r2 = sum((c - float(m)) ** 2 for c, m in zip(g, centre))
    a = np.exp(-r2 / (2 * sigma ** 2)).astype(np.float32)
    a[a < floor] = 0
    return a


def planted_volume(Z):
    """24 x 20 x Z: a Gaussian cell at (11.3, 9.6, (Z - 1) / 2) with single-voxel speckles, a 2 x 2 island and a one-voxel pinhole ->
    (a, cell support (bool), pinhole index, whole-volume box)."""
    sz = (24, 20, Z)
    a = gaussian_cell(sz, (11.3, 9.6, (Z - 1) / 2))
    support = a > 0
    for (x, y), val in (((1, 2), 0.3), ((21, 16), 0.25), ((3, 17), 0.4), ((0, 10), 0.2)):
        a[x, y, Z - 1] = val
    a[21:23, 3:5, 0] = 0.35
    hole = (12, 10, 0)
    a[hole] = 0
    return a, support, hole, (0, sz[0] - 1, 0, sz[1] - 1, 0, Z - 1)


def spiral(n=16):
    """A one-voxel-wide square spiral in n x n x 1 -> (a, its length): one face-connected part with a long path.  The walk goes
    inwards and turns where the cell ahead is taken, outside, or would touch an earlier turn of the spiral."""
    a = np.zeros((n, n, 1), dtype=np.float32)
    taken = np.zeros((n, n), dtype=bool)

    def clear_ahead(px, py, ddx, ddy):
        nx, ny = px + ddx, py + ddy
        if not (0 <= nx < n and 0 <= ny < n) or taken[nx, ny]:
            return False
        for ex, ey in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            qx, qy = nx + ex, ny + ey
            if (qx, qy) != (px, py) and 0 <= qx < n and 0 <= qy < n and taken[qx, qy]:
                return False
        return True

    x, y, dx, dy = 0, 0, 0, 1
    path = [(0, 0)]
    taken[0, 0] = True
    while True:
        if not clear_ahead(x, y, dx, dy):
            dx, dy = dy, -dx
            if not clear_ahead(x, y, dx, dy):
                break
        x, y = x + dx, y + dy
        taken[x, y] = True
        path.append((x, y))
    for i, (px, py) in enumerate(path):
        a[px, py, 0] = 1.0 + 0.001 * i
    return a, len(path)


def island_volume(Z):
    """``planted_volume`` plus a 4 x 4 island of 0.5 in the volume's corner, more than 3 voxels from the cell: it survives the
    median and the closing as a part of its own."""
    a, support, hole, box = planted_volume(Z)
    a[20:24, 0:4, :] = 0.5
    return a, support, box


def two_equal_parts():
    """10 x 10 x 1, two 2 x 2 blocks: the one with the higher linear index has the larger values, and still loses the tie."""
    a = np.zeros((10, 10, 1), dtype=np.float32)
    a[1:3, 6:8, 0] = 1.0
    a[6:8, 1:3, 0] = 2.0
    return a, (0, 9, 0, 9, 0, 0)


def plateau():
    """12 x 12 x 1: a 3 x 3 core of 2 inside a ring of 16 voxels of 1 -> (a, box, nrgthr): the energy 0.8 x 52 = 41.6 is reached at
    the sixth voxel of the plateau (36 + 6), and all sixteen are kept."""
    a = np.zeros((12, 12, 1), dtype=np.float32)
    a[3:8, 4:9, 0] = 1.0
    a[4:7, 5:8, 0] = 2.0
    return a, (0, 11, 0, 11, 0, 0), 0.8
