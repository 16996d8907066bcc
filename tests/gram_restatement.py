"""Float64 definition of the per-frame Gram matrix and right-hand side that K3 (csrc/warp_gram_rhs.hip), K3s
(csrc/warp_gram_sparse.hip) and K3n (csrc/warp_gram_lists.*) compute, for the very fp32 footprints, frames and coefficients
the kernels get:   G_t[k,l] = sum_v a_k(v) a_l(v),   r_t[k] = sum_v a_k(v) y(v),   a_k = the zero-padded trilinear sample of
footprint k at the reference's fp32 source coordinates (gn_restatement.source_coords / sample: in-bounds corners only).
numpy only.  Also the cases the Gram tests share (``gram_case``) and the bound they hold every kernel form to (``tol``), so
that the host test of the conditions and the GPU test speak of the same numbers.  Nothing here is fast.

The bound, per frame and entry -- nothing in it comes from a kernel's output:

    tol_G[k,l] = C_SUM absG[k,l] + sum_v ( |a_k| e_l + |a_l| e_k + e_k e_l )
    tol_r[k]   = C_SUM absr[k]   + sum_v   |y| e_k
    e_k(v)     = 4 spacing_fp32(umax) L_k(v) + 1e-6 m_k(v)

absG / absr are the same sums of absolute values (footprints are non-negative, so absG == G: a plain per-entry relative
bound; the frames are uniform in (-1, 1), so r cancels and absr matters).  e_k(v) is what the sample of neuron k at voxel v
may be off by: L_k(v) is the sum over the active axes of the largest |difference| between neighbouring taps of v's 2 x 2 (x 2)
cell along that axis (the zero border counts as a neighbour), m_k(v) the largest |tap| of the cell -- the project's K2
reconstruction bound (k2_restatement.recon_tol: coordinate rounding times the steepest step, plus the rounding of the
blend), per voxel and per neuron instead of per frame.  umax is k2_restatement's: the largest |source coordinate| of a voxel
with a tap inside the volume.  C_SUM = 2e-5 is the project's stated Gram tolerance (header of tests/test_gpu_parity.py: "G,
r rtol 2e-5 fp32 MFMA chains + ordered chunk sums vs float64 einsum"), here times the entry's own absolute sum instead of the
largest entry.  An entry whose bound is 0 must come out as an exact 0.  The trilinear sample is continuous in the coordinate, so
a coordinate that differs by an ulp between the kernel's fused chain and the reference's sequence moves a sample by at most
step x slope even across a lattice plane: K2's tap-flip problem does not arise (tests/test_gram_restatement_host.py checks
it: one fp32 step on every coordinate moves every entry by at most a quarter of its bound).

``long`` (an axis of 65537 voxels) is a gross check: fp32 coordinates near 65536 are 0.0078 voxel apart, 4 spacings are 3 % of
a voxel, and the coordinate term is most of the bound there (the tests print its share)."""
import functools

import numpy as np

import gn_restatement as GN
import k2_restatement as K2R

F32 = np.float32
C_SUM = 2e-5
COLS = K2R.COL + [K2R.T_COLS]                         # column of beta of frame F0 .. F7 (F7 appended behind case_betas')
T_COLS, UNUSED = K2R.T_COLS + 1, K2R.UNUSED
ORDER = [3, 0, 7, 5, 1, 6, 2, 4]                      # the frames of a call, as indices into F0 .. F7: ``times`` is not monotone
ORDER_LARGE = [5, 0]
LISTS_RR, LISTS_RC, LISTS_NG, MAX_SLOTS = 12, 40, 4, 3800     # csrc/warp_gram_lists.hpp

CASES = {
    "z1": ((33, 257, 1), 40, 1.0),
    "z1-dense-lists": ((33, 70, 1), 12, 3.0),
    "z2": ((65, 300, 2), 40, 1.0),
    "z3": ((34, 90, 3), 30, 1.2),
    "thin": ((9, 7, 5), 3, 3.0),
    **{f"words-{K}": ((48, 64, 1), K, 0.7) for K in (64, 65, 128, 129, 256)},
    **{f"padK-{K}": ((21, 19, 2), K, 0.7) for K in (15, 16, 17, 127)},
    "long": ((65537, 5, 1), 4, 1.5),
    # halo images of exactly 2^24 bytes (HaloLayout::f32off false): (X + 4) rows of (Y + 4) Z floats = 2048 x 2048
    "large-1": ((2044, 2044, 1), 6, 8.0),
    "large-2": ((2044, 1020, 2), 6, 8.0),
    "large-4": ((2044, 508, 4), 6, 8.0),
}
SMALL = [n for n in CASES if not n.startswith("large")]
LARGE = [n for n in CASES if n.startswith("large")]
# Seeds chosen for the nudge condition (tests/test_gram_restatement_host.py); 0 where nothing is recorded.
SEED = {}


def tile_shape(sz):
    """Voxels of a K3n tile (lists_tile_shape): 8 x 32 x 1, 8 x 16 x 2, 4 x 16 x 4."""
    return (8, 32, 1) if sz[2] == 1 else ((8, 16, 2) if sz[2] == 2 else (4, 16, 4))


def footprints(sz, pos, sigma):
    """(X,Y,Z,K) fp32: K2R.gaussians' exp(-|v - pos_k|^2 / sigma^2) in float64, values below 1e-6 set to zero, rounded to
    fp32 -- built on the window where every axis factor is at least 1e-6 (outside it the product is below 1e-6 as well)."""
    A = np.zeros(tuple(sz) + (len(pos),), dtype=F32)
    for k, p in enumerate(pos):
        ax = [np.exp(-(np.arange(n) - p[d]) ** 2 / sigma ** 2) for d, n in enumerate(sz)]
        keep = [np.flatnonzero(a >= 1e-6) for a in ax]
        if min(len(i) for i in keep) == 0:
            continue
        w = [slice(i[0], i[-1] + 1) for i in keep]
        g = ax[0][w[0], None, None] * ax[1][None, w[1], None] * ax[2][None, None, w[2]]
        g[g < 1e-6] = 0.0
        A[w[0], w[1], w[2], k] = g
    return A


def bboxes(A):
    """(K,6) xlo, xhi, ylo, yhi, zlo, zhi of the non-zeros of every footprint; lo > hi for an all-zero one."""
    K = A.shape[-1]
    bb = np.zeros((K, 6), dtype=np.int64)
    for k in range(K):
        nz = np.nonzero(A[..., k])
        for d in range(3):
            bb[k, 2 * d], bb[k, 2 * d + 1] = (nz[d].min(), nz[d].max()) if len(nz[d]) else (1, 0)
    return bb


def pattern_slots(bb):
    """nslot of dnmf_pack_footprints_lists: K rhs slots, the pairs (k, l >= k) whose boxes are at most one voxel apart on
    every axis, one trash slot."""
    K = len(bb)
    ok = np.ones((K, K), bool)
    for d in range(3):
        lo, hi = bb[:, 2 * d], bb[:, 2 * d + 1]
        ok &= (lo <= hi)[:, None] & (lo <= hi)[None, :] & (lo[:, None] - 1 <= hi[None, :]) & (lo[None, :] - 1 <= hi[:, None])
    return K + K + int(np.triu(ok, 1).sum()) + 1


def _positions(name, sz, K, sigma, rng):
    """Centres: uniform over the volume and one voxel beyond (some footprints are cut by the border); the list cases get
    two clusters (twelve and six neurons within less than a tile) so that some tile lists more than eight and some five to
    eight; the large volumes: two neurons 45 voxels apart within 40 voxels of the far corner (a weak pair where the tap
    offsets are largest), two at the origin (one cut), one in the middle, one all zero."""
    X, Y, Z = sz
    if name.startswith("large"):
        far = np.array([X - 1, Y - 1, Z - 1], dtype=np.float64)
        return np.array([far - [6.3, 9.1, 0.4], far - [38.2, 39.4, 0.7 * (Z - 1)], [0.6, -2.2, 0.2], [31.7, 24.4, 0.5 * (Z - 1)],
                         [X / 2 + 0.3, Y / 2 - 0.4, 0.3 * (Z - 1)], [X / 3, Y / 3, 0.0]])
    pos = np.stack([rng.uniform(-1, s, K) for s in sz], 1)
    if name == "z1-dense-lists":                      # boxes of 23 columns around the middle: every tile of F0 lists them all
        pos[:, 1] = rng.uniform(0.25 * Y, 0.75 * Y, K)
    if name in ("z1", "z2"):
        tx, ty, _ = tile_shape(sz)
        pos[:12, 0], pos[:12, 1] = 2 * tx + rng.uniform(1, tx - 2, 12), 3 * ty + rng.uniform(2, ty - 3, 12)
        pos[12:18, 0], pos[12:18, 1] = 5 * tx + rng.uniform(1, tx - 2, 6), ty + rng.uniform(2, ty - 3, 6)
    return pos


@functools.lru_cache(maxsize=None)
def gram_case(name):
    """The inputs of one case (CASES): dict(sz, K, A (X,Y,Z,K) fp32, bbox, nslot, beta (10,3,T_COLS) fp32, used, times,
    frames (B,P) fp32).  Frame b of the call is F[used[b]] and uses column times[b] of beta; the frames F0 .. F6 are
    k2_restatement.case_betas', F7 scales x and y by 1.6 about the volume centre (a tile's taps then span 14 rows and 51
    columns: no tile fits the LISTS_RR x LISTS_RC staging region); the column UNUSED holds an extreme warp no call names.
    Neuron K - 1 is all zero.  The data are uniform in (-1, 1), for F6 as well (nothing in K3 reads traces)."""
    sz, K, sigma = CASES[name]
    rng = np.random.default_rng(SEED.get(name, 0))
    pos = _positions(name, sz, K, sigma, rng)
    A = footprints(sz, pos, sigma)
    A[..., K - 1] = 0
    b8 = K2R.case_betas(sz, rng)
    beta = np.concatenate([b8, b8[:, :, :1]], axis=2).astype(np.float64)
    ctr = (np.array(sz, dtype=np.float64) - 1) / 2
    f7 = np.zeros((10, 3))
    f7[1, 0], f7[2, 1], f7[3, 2] = 1.6, 1.6, 1.0
    f7[0] = [-0.6 * ctr[0] + 0.23, -0.6 * ctr[1] - 0.31, 0.3 if sz[2] > 1 else 0.0]
    beta[:, :, T_COLS - 1] = f7
    ext = np.zeros((10, 3))
    ext[0], ext[1, 0], ext[2, 1], ext[3, 2] = [1e5, -3e4, 7.0], -37.0, 0.01, 5.0
    beta[:, :, UNUSED] = ext
    used = ORDER_LARGE if name.startswith("large") else ORDER
    P = int(np.prod(sz))
    frames = rng.uniform(-1, 1, (len(used), P)).astype(F32)
    bb = bboxes(A)
    return {"name": name, "sz": sz, "K": K, "A": A, "bbox": bb, "nslot": pattern_slots(bb), "beta": beta.astype(F32), "used": used,
            "times": [COLS[i] for i in used], "frames": frames}


def cell_taps(s, u):
    """The 2 x 2 x 2 taps of the cell of every coordinate u (N,3) in the image s (zero outside): (N,2,2,2), [dx,dy,dz]."""
    p = np.pad(s, 1)
    f = np.floor(u).astype(np.int64)
    out = np.zeros((len(u), 2, 2, 2))
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                c = [np.clip(f[:, d] + o + 1, 0, p.shape[d] - 1) for d, o in enumerate((dx, dy, dz))]
                out[:, dx, dy, dz] = p[c[0], c[1], c[2]]
    return out


def gram(A, beta, sz, times, frames, nudge=0, rows=None):
    """G, r of the frames ``times`` (B of them): A (X,Y,Z,K) fp32, beta (10,3,T) fp32, frames (B,P) fp32 (frame b belongs to
    times[b]).  Returns a dict of arrays with the frame in front: G, absG, coordG (B,K,K); r, absr, coordr (B,K); umax (B).
    coordG / coordr are the coordinate allowance (the sums over e in the module docstring).  Neuron k is sampled only on the
    voxels whose source coordinate lies inside its bounding box widened by one voxel; elsewhere a_k is an exact zero.
    ``nudge``: every coordinate one fp32 step up (+1) or down (-1).  ``rows``: a slice of x -- the sums then run over those
    rows of voxels only."""
    sz = tuple(int(s) for s in sz)
    X, Y, Z = sz
    K = A.shape[-1]
    A = np.asarray(A).reshape(X, Y, Z, K)
    beta = np.asarray(beta, dtype=F32)
    bb = bboxes(A)
    rows = slice(0, X) if rows is None else rows
    nax = 3 if Z > 1 else 2
    crops = []
    for k in range(K):
        lo, hi = bb[k, 0::2], bb[k, 1::2]
        crops.append(None if lo[0] > hi[0] else A[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1, k].astype(np.float64))
    out = {k: [] for k in ("G", "absG", "coordG", "r", "absr", "coordr", "umax")}
    for b, t in enumerate(times):
        bt = beta[:, :, t]
        u = K2R.nudged(K2R._coords(np.ascontiguousarray(bt).tobytes(), sz)[rows], nudge, sz).reshape(-1, 3)
        y = np.asarray(frames[b], dtype=np.float64).reshape(X, -1)[rows].reshape(-1)
        hit = np.ones(len(u), bool)
        for d in range(3):
            hit &= (u[:, d] > -1) & (u[:, d] < sz[d])
        umax = float(np.abs(u[hit]).max()) if hit.any() else 0.0
        sp = float(np.spacing(F32(umax)))
        masks = []
        for k in range(K):
            m = np.zeros(len(u), bool) if crops[k] is None else np.ones(len(u), bool)
            if crops[k] is not None:
                for d in range(3):
                    m &= (u[:, d] > bb[k, 2 * d] - 1) & (u[:, d] < bb[k, 2 * d + 1] + 1)
            masks.append(m)
        union = np.flatnonzero(np.any(masks, axis=0)) if K else np.zeros(0, np.int64)
        a, e = np.zeros((len(union), K)), np.zeros((len(union), K))
        for k in range(K):
            sel = masks[k][union]
            if not sel.any():
                continue
            uk = u[union[sel]] - bb[k, 0::2]                       # exact: fp32 values minus small integers in float64
            a[sel, k] = GN.sample(crops[k], uk)[0]
            c = cell_taps(crops[k], uk)
            L = sum(np.abs(np.diff(c, axis=1 + d)).reshape(len(uk), -1).max(1) for d in range(nax))
            e[sel, k] = 4.0 * sp * L + 1e-6 * np.abs(c).reshape(len(uk), -1).max(1)
        yu, aa = y[union], np.abs(a)
        out["G"].append(a.T @ a)
        out["absG"].append(aa.T @ aa)
        out["coordG"].append(aa.T @ e + e.T @ aa + e.T @ e)
        out["r"].append(a.T @ yu)
        out["absr"].append(aa.T @ np.abs(yu))
        out["coordr"].append(e.T @ np.abs(yu))
        out["umax"].append(umax)
    return {k: np.array(v) for k, v in out.items()}


def tol(ref):
    """(tol_G (B,K,K), tol_r (B,K)), see the module docstring."""
    return C_SUM * ref["absG"] + ref["coordG"], C_SUM * ref["absr"] + ref["coordr"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 result of a case, made once and shared by every kernel form and test; (result, host seconds)."""
    import time
    c = gram_case(name)
    t0 = time.perf_counter()
    ref = gram(c["A"], c["beta"], c["sz"], c["times"], c["frames"])
    return ref, time.perf_counter() - t0


def worst(err, bound):
    """Largest err / bound over the entries with bound > 0 and its index; where bound == 0 the error must be an exact zero
    (asserted by the callers through the returned flag): (ratio, index, zeros_ok)."""
    zero = bound == 0
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, bound))
    idx = np.unravel_index(int(ratio.argmax()), ratio.shape) if ratio.size else ()
    return (float(ratio.max()) if ratio.size else 0.0), idx, bool((err[zero] == 0).all())


# ---- geometry of the K3n tiles (what the cases are meant to reach) ----------------------------------------------------
def tile_geometry(name, frame):
    """Per K3n tile of frame F[frame] of a case, from the coordinates alone: (count, rows, cols, full) arrays over the tiles --
    the neurons whose bounding box meets the exact tap box of the tile's voxels (a lower bound of the kernel's list length,
    which works from a conservative tap range), the tap rows and the tap floats of a halo row ((columns) x Z) the tile spans,
    and whether the tile has all its rows or all its columns (a ragged corner tile has neither)."""
    c = gram_case(name)
    sz = c["sz"]
    bt = c["beta"][:, :, COLS[frame]]
    u = K2R._coords(np.ascontiguousarray(bt).tobytes(), sz)
    f = np.floor(u)
    tx, ty, tz = tile_shape(sz)
    bb = c["bbox"]
    live = bb[:, 0] <= bb[:, 1]
    cnt, nrow, ncol, full = [], [], [], []
    for x0 in range(0, sz[0], tx):
        for y0 in range(0, sz[1], ty):
            for z0 in range(0, sz[2], tz):
                blk = f[x0:x0 + tx, y0:y0 + ty, z0:z0 + tz].reshape(-1, 3)
                lo, hi = blk.min(0), blk.max(0) + 1
                meet = live.copy()
                for d in range(3 if sz[2] > 1 else 2):
                    meet &= (bb[:, 2 * d] <= hi[d]) & (bb[:, 2 * d + 1] >= lo[d])
                cnt.append(int(meet.sum()))
                nrow.append(int(hi[0] - lo[0] + 1))
                ncol.append(int(hi[1] - lo[1] + 1) * sz[2])
                full.append(x0 + tx <= sz[0] or y0 + ty <= sz[1])
    return np.array(cnt), np.array(nrow), np.array(ncol), np.array(full)
