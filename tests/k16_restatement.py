"""Float64 definition of K16 (``dnmf_warp_normal_eqs``, csrc/motion_gn.hip) with the sums of absolute values its entries'
rounding scales with, for the very fp32 images, frames and coefficients the kernel gets.  numpy only; the sample, the
coordinates and the centred basis are gn_restatement's, the nudge and the shared inputs k2_restatement's.  Also the case the K16
tests share (``k16_case``: ``k2_case`` unchanged plus three columns of beta, two of them not finite), the bounds they hold the kernel
to (``H_tol``, ``g_tol``, ``SSE_RTOL``) and ``assemble``, which builds H and g the way the kernel does -- distinct moments
spread into the matrix -- so that the host test can break that route on purpose and see whether the bound notices.  Nothing
here is fast."""
import functools

import numpy as np

import gn_restatement as GN
import k2_restatement as K2R
from oracle import dnmf_oracle as orc

F32 = np.float32
PLANE_ROWS, PLANE_COLS = K2R.PLANE_ROWS, K2R.PLANE_COLS
# (33, 257, 1)   Z = 1: two x-blocks with a one-row tail, two plane blocks with a one-lane tail
# (65, 300, 2)   Z = 2 (a lane owns both slices): three x-blocks, two plane blocks
# (34, 90, 5)    Z > 2: Y Z = 450, the plane-block boundary (position 256 = y 51, z 1) falls inside a z-column; two x-blocks
# (9, 7, 4)      thin, one block: z-taps outside on both sides
# The last two have Z >= 4 because at Z <= 3 the centred u_z only takes values of {-1, 0, 1}, where u_z^3 == u_z and
# u_z^4 == u_z^2: a z exponent of 3 or 4 read as 1 or 2 changes no sum there.  u_z is {-1, -1/2, 0, 1/2, 1} at Z = 5 and
# {+-1, +-1/3} at Z = 4.
SHAPES = [(33, 257, 1), (65, 300, 2), (34, 90, 5), (9, 7, 4)]
T_COLS = K2R.T_COLS + 3
LAST_COL, NAN_COL, INF_COL = K2R.T_COLS, K2R.T_COLS + 1, K2R.T_COLS + 2          # the columns of beta K16's case adds
SSE_RTOL = 1e-5


@functools.lru_cache(maxsize=16)
def _coords(bt_bytes, sz):
    return GN.source_coords(np.frombuffer(bt_bytes, dtype=F32).reshape(10, 3), sz)


@functools.lru_cache(maxsize=4)
def _phi(sz):
    return GN.basis64(GN.centred_lattice(sz)).reshape(-1, 10)


def frame_parts(S_b, bt, sz, frame, nudge=0):
    """One finite frame: (dq (P,3), r (P,)) -- the derivative of the sample by the source coordinate and the residual,
    voxels in the order of the lattice (x slowest)."""
    sz = tuple(int(s) for s in sz)
    u = K2R.nudged(_coords(np.ascontiguousarray(bt, dtype=F32).tobytes(), sz), nudge, sz)
    rec, dq = GN.sample(np.asarray(S_b, dtype=np.float64).reshape(sz), u)
    r = rec - np.asarray(frame, dtype=np.float64).reshape(rec.shape)
    return dq.reshape(3, -1).T, r.ravel()


def k16(S, beta, sz, times, frames, nudge=0):
    """K16 on the frames ``times`` (B of them): S (B,X,Y,Z) the reconstruction images, beta (10,3,T) fp32, frames (B,X,Y,Z).
    Returns a dict of arrays with the frame in front, exactly as GN.normal_eqs defines them (centred basis, parameter index
    a*3+d; a coefficient that is not finite gives H = g = 0 and sse = NaN):
      H (B,30,30), g (B,30), sse (B)
      absH (B,30,30) = sum_v |J_vi| |J_vj|,  absg (B,30) = sum_v |J_vi| |r_v|: what an entry's rounding error scales with
    ``nudge``: every fp32 source coordinate moved by one representable number up (+1) or down (-1)."""
    sz = tuple(int(s) for s in sz)
    times = list(times)
    B = len(times)
    phi = _phi(sz)
    beta = np.asarray(beta, dtype=F32)
    out = {"H": np.zeros((B, 30, 30)), "g": np.zeros((B, 30)), "sse": np.zeros(B), "absH": np.zeros((B, 30, 30)),
           "absg": np.zeros((B, 30))}
    for b, t in enumerate(times):
        bt = beta[:, :, t]
        if not np.isfinite(bt).all():
            out["sse"][b] = np.nan
            continue
        dq, r = frame_parts(S[b], bt, sz, frames[b], nudge)
        J = (phi[:, :, None] * dq[:, None, :]).reshape(-1, 30)
        aJ = np.abs(J)
        out["H"][b], out["g"][b], out["sse"][b] = J.T @ J, J.T @ r, float((r ** 2).sum())
        out["absH"][b], out["absg"][b] = aJ.T @ aJ, aJ.T @ np.abs(r)
    return out


def H_tol(ref):
    """Per frame and entry: 1e-4 absH -- the project's K2 / K16 figure (fp32 sums of P terms in another order), scaled by the
    entry's own absolute sum instead of by the diagonal.  A zero asks for an exact zero."""
    return 1e-4 * ref["absH"]


def g_tol(ref):
    """Per frame and entry: 1e-4 absg."""
    return 1e-4 * ref["absg"]


def worst(err, tol):
    """Largest err / tol over the entries with tol > 0; where tol == 0 the error must be an exact zero."""
    assert (err[tol == 0] == 0).all()
    return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


# ---- the kernel's route to H and g, open to being broken ---------------------------------------------------------------
def plane_position(sz):
    """(P,) the position in the (y, z) plane that the lane owning a voxel has: y Z + z, at Z == 2 (a lane owns both slices) y."""
    X, Y, Z = (int(s) for s in sz)
    lat = orc.voxel_lattice(sz).reshape(-1, 3).astype(np.int64)
    return lat[:, 1] if Z == 2 else lat[:, 1] * Z + lat[:, 2]


def assemble(sz, dq, r, zexp=None, pair=None, keep=None, uc=None):
    """(H (30,30), g (30)) of one frame from dq (P,3) and r (P,) the way csrc/motion_gn.hip gets there: the distinct sums
    (monomial u_x^i u_y^j u_z^k of degree <= 4) x (pair d <= e) and (degree <= 2) x d, spread into the matrix by the exponents
    of the two basis terms.  Unbroken it is J^T J and J^T r.  The hooks break it:
      zexp   k -> the exponent of u_z used where H asks for k
      pair   (d, e) with d <= e -> the pair whose sums are used for it
      keep   (P,) bool: the voxels that are summed
      uc     (P,3) the centred coordinates of the voxels instead of GN.centred_lattice(sz)"""
    uc = GN.centred_lattice(sz).reshape(-1, 3) if uc is None else uc
    zexp = zexp or (lambda k: k)
    pair = pair or (lambda d, e: (d, e))
    if keep is not None:
        dq, r = dq * keep[:, None], r * keep
    pw = [np.stack([uc[:, d] ** k for k in range(5)], 1) for d in range(3)]      # (P,5) powers per axis; 0 ** 0 == 1
    expo = sorted({(i, j, k) for i in range(5) for j in range(5 - i) for k in range(5 - i - j)})
    mono = np.stack([pw[0][:, i] * pw[1][:, j] * pw[2][:, k] for i, j, k in expo], 1)                    # (P,35)
    pairs = [(d, e) for d in range(3) for e in range(d, 3)]
    hs = mono.T @ np.stack([dq[:, d] * dq[:, e] for d, e in pairs], 1)           # the 35 x 6 distinct sums behind H
    gs = mono.T @ (dq * r[:, None])                                              # behind g: the rows of degree <= 2 are used
    H, g = np.zeros((30, 30)), np.zeros(30)
    for i in range(30):
        a, d = divmod(i, 3)
        g[i] = gs[expo.index(tuple(GN.EXPO[a])), d]
        for j in range(30):
            a2, e = divmod(j, 3)
            ex = GN.EXPO[a] + GN.EXPO[a2]
            H[i, j] = hs[expo.index((int(ex[0]), int(ex[1]), int(zexp(int(ex[2]))))), pairs.index(tuple(pair(min(d, e), max(d, e))))]
    return H, g


# ---- the case the tests share ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def k16_case(sz):
    """``k2_case(sz)`` as it is -- S32, frames and the seven warps F0 .. F6 in their columns -- and three frames more, each with
    F0's image and frame:
      F7 (column LAST_COL)  a sub-voxel shift that puts the image's largest voxel under the LAST position of the (y, z) plane
                            (y = Y - 1, z = Z - 1).  With k2_case's Gaussians no frame F0 .. F5 of (33, 257, 1) has a sample with
                            a slope at y = 256, the one-lane tail of the second plane block: dropping that lane changed no sum
                            (1e-5 of the bound, tests/test_k16_restatement_host.py mutant (c)) until this frame was added.
      F8 (column NAN_COL)   F0's warp with one coefficient NaN
      F9 (column INF_COL)   F1's warp with one coefficient +inf (the kernel's test is ``bt - bt == 0``, which must catch both)
    B = 10 frames at the columns ``times`` of a beta of T_COLS columns, the first ``finite`` of them with finite coefficients."""
    sz = tuple(int(s) for s in sz)
    c = K2R.k2_case(sz)
    assert c["used"] == list(range(7))
    s0 = c["S32"][0]
    peak = np.unravel_index(np.abs(s0).argmax(), s0.shape)
    last = orc.identity_beta(1)[:, :, 0].astype(np.float64)
    last[0, 0] += 0.21
    last[0, 1] += peak[1] - (sz[1] - 1) + 0.37
    if sz[2] > 1:
        last[0, 2] += peak[2] - (sz[2] - 1) + 0.3
    beta = np.concatenate([c["beta"], last.astype(F32)[:, :, None], c["beta"][:, :, [K2R.COL[0], K2R.COL[1]]]], axis=2)
    beta[7, 1, NAN_COL] = np.nan
    beta[4, 0, INF_COL] = np.inf
    extra = [0, 0, 0]
    return {"sz": sz, "beta": beta, "times": c["times"] + [LAST_COL, NAN_COL, INF_COL], "finite": 8,
            "S32": np.concatenate([c["S32"], c["S32"][extra]]), "frames": np.concatenate([c["frames"], c["frames"][extra]]),
            "norm_frames": c["norm_frames"]}


@functools.lru_cache(maxsize=None)
def reference(sz, nudge=0):
    """k16 of the shared case."""
    c = k16_case(sz)
    return k16(c["S32"], c["beta"], c["sz"], c["times"], c["frames"], nudge=nudge)
