"""Float64 definition of K2 (``dnmf_warp_recon_grad``, csrc/warp_recon_grad.hip): the warped reconstruction, the loss, the
gradient with respect to beta in the raw basis and the corner regulariser, for the very fp32 images, frames and coefficients
the kernel gets.  numpy only; the sample, the coordinates and the images are gn_restatement's.  Also the case the K2 tests share
(``k2_case``) and the tolerances they hold the kernel to (``grad_tol``, ``recon_tol``), so that the host test of the flip
condition and the GPU test speak of the same numbers.  Nothing here is fast."""
import functools

import numpy as np

import gn_restatement as GN
from oracle import dnmf_oracle as orc

F32 = np.float32


@functools.lru_cache(maxsize=1)
def _phi(sz, lo, hi):
    """basis(v) in float64 for the rows lo <= x < hi, (voxels, 10), raw voxel coordinates."""
    return GN.basis64(orc.voxel_lattice(sz)[lo:hi]).reshape(-1, 10)


@functools.lru_cache(maxsize=4)
def _coords(bt_bytes, sz):
    """GN.source_coords of the coefficients with these bytes (the fit call and the call with an upstream gradient share them)."""
    return GN.source_coords(np.frombuffer(bt_bytes, dtype=F32).reshape(10, 3), sz)


def jacobian_det(bt, pt):
    """det J of the quadratic map at the point pt in float64, by the oracle's formula (oracle.dnmf_oracle.log_det_jac: rows 8 / 9
    of beta used as (yz, xz), like the reference and K2's finish kernel)."""
    b = np.asarray(bt, dtype=np.float64)
    x, y, z = (float(p) for p in pt)
    J = np.stack([b[1] + 2 * b[4] * x + b[7] * y + b[9] * z, b[2] + 2 * b[5] * y + b[7] * x + b[8] * z,
                  b[3] + 2 * b[6] * z + b[8] * y + b[9] * x])
    return float(np.linalg.det(J))


def nudged(u, step, sz):
    """Every fp32 source coordinate moved by ``step`` (+1 / -1) representable numbers (z stays pinned at Z == 1)."""
    if not step:
        return u
    out = np.nextafter(u.astype(F32), F32(np.inf if step > 0 else -np.inf)).astype(np.float64)
    if int(sz[2]) == 1:
        out[..., 2] = 0.0
    return out


def slope_of(s):
    """Largest |difference| between neighbouring voxels of s along any axis, the zero border being a neighbour."""
    p = np.pad(np.asarray(s, dtype=np.float64), 1)
    return float(max(np.abs(np.diff(p, axis=d)).max() for d in range(3)))


def k2(S, beta, sz, times, frames=None, gout=None, norm_frames=None, nudge=0, rows=None):
    """K2 on the frames ``times`` (B of them): S (B,X,Y,Z) the reconstruction images, beta (10,3,T) fp32, frames (B,X,Y,Z) or
    gout (B,X,Y,Z) (the upstream gradient; then the residual is gout and the gradient is not scaled).  Returns a dict of arrays
    with the frame in front:
      recon (B,X,Y,Z)   A_tC;      sse (B), frame_loss (B) = sse / (norm_frames P)
      grad (B,10,3)     scale * sum_v phi_a(v) r(v) dq_d(v), scale = 2 / (norm_frames P) (1 with gout), ``scale`` itself
      abs_sum (B,10,3)  sum_v |phi_a r dq_d|: what an entry's rounding error scales with
      reg (B), det (B,2)  the corner regulariser and det J at (the far corner, the origin)
      slope (B), umax (B)  slope_of(S[b]); the largest |source coordinate| of a voxel with a tap inside the volume
    ``nudge``: the coordinates moved by one fp32 step up (+1) or down (-1).  ``rows``: a slice of x -- recon and every sum then
    cover those rows only (the flip condition on a slab of a large volume)."""
    sz = tuple(int(s) for s in sz)
    X, Y, Z = sz
    P = X * Y * Z
    times = list(times)
    B = len(times)
    nf = B if not norm_frames else int(norm_frames)
    scale = 1.0 if gout is not None else 2.0 / (nf * P)
    rows = slice(0, X) if rows is None else rows
    phi = _phi(sz, rows.start, rows.stop)
    beta = np.asarray(beta, dtype=F32)
    out = {k: [] for k in ("recon", "sse", "grad", "abs_sum", "reg", "det", "slope", "umax")}
    for b, t in enumerate(times):
        bt = beta[:, :, t]
        s = np.asarray(S[b], dtype=np.float64).reshape(sz)
        u = nudged(_coords(np.ascontiguousarray(bt).tobytes(), sz)[rows], nudge, sz)
        rec, dq = GN.sample(s, u)
        other = gout if gout is not None else frames
        o = np.asarray(other[b], dtype=np.float64).reshape(sz)[rows]
        r = o if gout is not None else rec - o
        term = (r[None] * dq).reshape(3, -1).T                      # (voxels, 3): r dq_d
        out["recon"].append(rec)
        out["sse"].append(float((r ** 2).sum()))
        out["grad"].append(scale * (phi.T @ term))
        out["abs_sum"].append(np.abs(phi).T @ np.abs(term))
        dets = [jacobian_det(bt, [X - 1, Y - 1, Z - 1]), jacobian_det(bt, [0, 0, 0])]
        out["det"].append(dets)
        with np.errstate(divide="ignore"):
            out["reg"].append(float(sum(np.log(abs(d)) ** 2 for d in dets)))
        out["slope"].append(slope_of(s))
        hit = np.ones(u.shape[:-1], bool)                           # some tap of the voxel lies inside the volume
        for d in range(3):
            hit &= (u[..., d] > -1) & (u[..., d] < sz[d])
        out["umax"].append(float(np.abs(u[hit]).max()) if hit.any() else 0.0)
    out = {k: np.array(v) for k, v in out.items()}
    out["frame_loss"] = out["sse"] / (nf * P)
    out["scale"] = scale
    return out


# ---- the tolerances of the GPU test ----------------------------------------------------------------------------------
def grad_tol(ref):
    """Per frame and entry: 1e-4 * scale * abs_sum -- the project's K2 bound (fp32 sums of P terms in another order), scaled by
    the entry's own absolute sum instead of by the largest entry."""
    return 1e-4 * ref["scale"] * ref["abs_sum"]


def recon_tol(ref, smax):
    """Per frame: 4 spacing_fp32(max|u|) slope + 1e-6 max|S| -- coordinate rounding times the image's steepest step, plus the
    rounding of the blend."""
    return 4.0 * np.spacing(ref["umax"].astype(F32)).astype(np.float64) * ref["slope"] + 1e-6 * smax


# ---- the case the tests share ------------------------------------------------------------------------------------------
PLANE_ROWS, PLANE_COLS = 32, 256                      # csrc/warp_taps.hpp
T_COLS, UNUSED = 8, 3                                 # columns of beta; the one no call names
COL = [0, 1, 2, 4, 5, 6, 7]                           # column of frame F0 .. F6
SHAPES = [(33, 257, 1), (65, 300, 2), (34, 90, 3), (9, 7, 5)]
# Halo images of exactly 2^24 bytes (HaloLayout::f32off false): (X + 4) rows of (Y + 4) Z floats rounded up to 32 make 2048 x
# 2048 floats either way, and one row or one column less falls below.  They are the smallest such volumes with a square plane
# of floats (a sliver like 60 x 65532 has 6 % fewer voxels, and coordinates near 65536 whose fp32 spacing of 0.008 voxel would
# let the reconstruction bound say little).  The GPU test asserts the inequality.
LARGE = [(2044, 2044, 1), (2044, 1020, 2)]
LARGE_FRAMES = [0, 5]


def gaussians(sz, pos, sigma):
    """(K,X,Y,Z) float64: exp(-|v - pos_k|^2 / sigma^2), axis by axis."""
    ax = [np.exp(-(np.arange(n)[None, :] - pos[:, d:d + 1]) ** 2 / sigma ** 2) for d, n in enumerate(sz)]
    return ax[0][:, :, None, None] * ax[1][:, None, :, None] * ax[2][:, None, None, :]


def case_betas(sz, rng):
    """beta (10,3,T_COLS) fp32: the frames F0 .. F6 in the columns COL, see tests/test_gpu_k2_float64.py.  No shift is a whole
    number of voxels and at Z > 1 every frame moves z by a fraction: a coordinate on a lattice point is where the gradient jumps
    (left to fixture G3's identity cases)."""
    X, Y, Z = sz
    nd = 3 if Z > 1 else 2
    ext = np.array([max(s - 1, 1) for s in sz], dtype=np.float64)
    amp = np.minimum(1.0, ext / 8.0)                   # test_gpu_gn.k16_case: a thin axis is left by some samples, not by all
    b = orc.identity_beta(T_COLS).astype(np.float64)
    f = lambda i: (slice(None), slice(None), COL[i])
    zs = [0.6, 0.3, -0.6, 0.35, -0.25, 0.0, 0.2]       # z-shift of F0 .. F6 (F5 gets its own below)
    F = [b[f(i)] for i in range(7)]
    F[0][0, :2] += [0.37, -0.21]                       # F0: the base corner advances by one row per x everywhere
    F[1][0, :2] += [0.3137, 0.2]                         # F1: advance 2 at an x that depends on y
    F[1][1, 0], F[1][2, 0] = 1.03, 0.011
    F[2][0, :2] += [0.4, -0.3]                         # F2: advance 0 or 1
    F[2][1, 0] = 0.5
    F[3][0, :2] = [X - 1.3, 0.45]                      # F3: x reversed, advance -1
    F[3][1, 0] = -1.0
    F[4][0, :2] += [5.3, -(Y / 3.0 + 0.37)]            # F4: first rows wholly outside, many taps in the halo
    F[5][0] += rng.uniform(-3, 3, 3) * amp             # F5: k16_case's generic quadratic warp
    F[5][1:4] += rng.uniform(-0.15, 0.15, (3, 3)) * np.minimum(1.0, ext[None, :] / ext[:, None])
    for a in range(4, 10):
        F[5][a] += rng.uniform(-2, 2, 3) * amp / np.prod(ext ** GN.EXPO[a])
    F[6][0, :2] += [0.25, 0.15]                        # F6: all-zero traces
    for i in range(7):
        if i != 5:
            F[i][0, 2] += zs[i]
    b[:, :, UNUSED] += 0.1
    if nd == 2:
        b[:, 2] = orc.identity_beta(T_COLS)[:, 2]
    return b.astype(F32)


# Seeds chosen for the flip condition (tests/test_k2_restatement_host.py).  (34, 90, 3): seed 0 puts a coordinate of F5 one fp32
# step from an integer (gradient spread 50 times the allowance).  Where the three axes are of similar length the reconstruction
# allowance is tight by construction -- one step up against one step down on three coordinates of about the same spacing is up
# to 6 spacing slope, a quarter of the bound is 1 spacing slope + 0.25e-6 max|S| -- and holds only where the steepest voxels
# are not the farthest: seeds 0 and 1 miss it by 1.5 at (34, 90, 3), of the seeds 0 .. 59 only 20 is below 0.8 at (9, 7, 5).
# The large volumes: where an image is cut by the border, a sample one fp32 step (1.2e-4 voxel at 2043) from the last plane of
# voxels flips between a tap pair inside (d q = a difference of neighbours) and one half outside (d q = the voxel's value, 250
# times that for a Gaussian of sigma 250).  One such voxel of F5 moved the y-entries by 19 quarter-bounds at Z = 1, K2 on the GPU
# differed from the restatement by 5 bounds in exactly those entries, and which voxel it is depends on the last bit of the
# host's fp32 einsum (another CPU, another voxel).  No seed is safe from that, so the images of the large volumes go to zero at
# the border (k2_case: a 64-voxel taper); the cut images stay with the table's shapes.
SEED = {(34, 90, 3): 2, (9, 7, 5): 20}


@functools.lru_cache(maxsize=None)
def k2_case(sz):
    """The inputs of one shape: K = 5 Gaussians (sigma 3, some cut by the border; sigma 250 and tapered to zero at the border in
    the two large volumes, where five narrow ones would leave the image empty), computed in float64 and rounded to fp32; frames and an upstream gradient of uniform
    noise; B frames ``used`` (indices into F0 .. F6; the large volumes: F0 and F5) at the columns ``times`` of beta."""
    sz = tuple(int(s) for s in sz)
    rng = np.random.default_rng(SEED.get(sz, 0))
    large = sz in LARGE
    used = LARGE_FRAMES if large else list(range(7))
    K = 5
    pos = np.stack([rng.uniform(-1, s, K) for s in sz], 1)
    C = rng.uniform(0.5, 1.5, (K, 7))
    C[:, 6] = 0.0
    beta = case_betas(sz, rng)
    A = gaussians(sz, pos, 250.0 if large else 3.0)
    if large:                                          # sin^2 taper over 64 voxels along x and y: no step at the border (SEED)
        tx, ty = (np.sin(0.5 * np.pi * np.minimum(1.0, np.minimum(np.arange(n) + 1, n - np.arange(n)) / 64.0)) ** 2 for n in sz[:2])
        A = A * tx[None, :, None, None] * ty[None, None, :, None]
    S32 = np.stack([np.tensordot(C[:, i], A, 1) for i in used]).astype(F32)
    B = len(used)
    frames = rng.uniform(0, 1, (B, *sz)).astype(F32)
    gout = rng.uniform(-1, 1, (B, *sz)).astype(F32)
    return {"sz": sz, "beta": beta, "used": used, "times": [COL[i] for i in used], "S32": S32, "frames": frames, "gout": gout,
            "norm_frames": B + 3}
