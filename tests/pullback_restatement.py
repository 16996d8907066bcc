"""numpy float64 restatement of K17 (dnmf_warp_pullback), the trilinear registered movie under the quadratic warp, written
from its definition in include/dnmf_hip.h / DESIGN.md.  The tests compare the kernel against this; nothing here is fast.

Conventions are those of tests/tracks_restatement.py (csrc/tracks.hip): q_t(x) = basis(x) . beta[:, :, t] in voxel indices,
basis = [1, x, y, z, x^2, y^2, z^2, xy, xz, yz], the true Jacobian (row 8 = xz, row 9 = yz)."""
import numpy as np

from tracks_restatement import basis

TOL, CAP, DET_MIN = 1e-6, 32, 1e-12


def lattice(sz):
    """(P,3) float64 lattice points in voxel order p = (x Y + y) Z + z."""
    g = np.meshgrid(*(np.arange(int(s), dtype=np.float64) for s in sz), indexing="ij")
    return np.stack(g, -1).reshape(-1, 3)


def jacobians(b, x):
    """d q_d / d x_e at the points x (n,3): (n,3,3)."""
    b = np.asarray(b, dtype=np.float64)
    J = np.empty((x.shape[0], 3, 3))
    for d in range(3):
        J[:, d, 0] = b[1, d] + 2 * b[4, d] * x[:, 0] + b[7, d] * x[:, 1] + b[8, d] * x[:, 2]
        J[:, d, 1] = b[2, d] + 2 * b[5, d] * x[:, 1] + b[7, d] * x[:, 0] + b[9, d] * x[:, 2]
        J[:, d, 2] = b[3, d] + 2 * b[6, d] * x[:, 2] + b[8, d] * x[:, 0] + b[9, d] * x[:, 1]
    return J


def active_axes(sz):
    return [d for d in range(3) if int(sz[d]) > 1]


def lattice_abs_det(beta_t, sz):
    """|det J| of the active axes' block at every lattice point: the condition of the kernel's accuracy contract."""
    act = active_axes(sz)
    J = jacobians(beta_t, lattice(sz))[:, act][:, :, act]
    return np.abs(np.linalg.det(J))


def invert(beta_t, sz, tol=TOL, cap=CAP):
    """For every lattice point u the x with q_t(x) = u by Newton from x = u: (x (P,3), bad (P,) bool).  An axis of extent 1 is
    inactive: its coordinate stays 0 and its equation is dropped.  bad: |det J| < 1e-12, a non-finite iterate, or no step
    below ``tol`` in every coordinate within ``cap`` steps; x is NaN there."""
    b = np.asarray(beta_t, dtype=np.float64)
    u = lattice(sz)
    act = active_axes(sz)
    x = u.copy()
    n = x.shape[0]
    done, bad = np.zeros(n, bool), np.zeros(n, bool)
    if not act:
        return x, bad
    with np.errstate(all="ignore"):
        for _ in range(cap):
            go = np.flatnonzero(~(done | bad))
            if go.size == 0:
                break
            xg = x[go]
            J = jacobians(b, xg)[:, act][:, :, act]
            det = np.linalg.det(J)
            ok = np.abs(det) >= DET_MIN          # False for NaN
            bad[go[~ok]] = True
            go, xg, J = go[ok], xg[ok], J[ok]
            if go.size == 0:
                continue
            r = (basis(xg) @ b - u[go])[:, act]
            step = np.linalg.solve(J, r[:, :, None])[:, :, 0]
            xg[:, act] -= step
            x[go] = xg
            fin = np.isfinite(xg).all(1)
            bad[go[~fin]] = True
            done[go[fin]] = (np.abs(step[fin]) < tol).all(1)
    bad |= ~done
    x[bad] = np.nan
    return x, bad


def sample(frame, x):
    """Trilinear sample of frame (X,Y,Z) at x (n,3), zero padding (grid_sample, zeros, align_corners=True): sum over the 8 taps
    of w Y[tap], weights from floor(x) and x - floor(x); a tap outside the volume contributes 0, a NaN voxel propagates."""
    frame = np.asarray(frame, dtype=np.float64)
    S = frame.shape
    f = np.floor(x)
    w1 = x - f
    i0 = f.astype(np.int64)
    out = np.zeros(x.shape[0])
    with np.errstate(invalid="ignore"):
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    idx = i0 + np.array([dx, dy, dz])
                    inside = ((idx >= 0) & (idx < np.array(S))).all(1)
                    w = np.prod(np.where(np.array([dx, dy, dz]) == 1, w1, 1.0 - w1), 1)
                    ii = idx[inside]
                    out[inside] += w[inside] * frame[ii[:, 0], ii[:, 1], ii[:, 2]]
    return out


def pullback_frame(frame, beta_t, fill=None, tol=TOL, cap=CAP):
    """One frame (X,Y,Z) under beta_t (10,3): (out (X,Y,Z), coords (P,3), bad (P,) bool).  fill None: zero padding, bad points 0;
    a float: written where x lies outside [0, S_d - 1] on an active axis, and at bad points."""
    frame = np.asarray(frame, dtype=np.float64)
    sz = frame.shape
    x, bad = invert(beta_t, sz, tol, cap)
    good = ~bad
    out = np.zeros(x.shape[0])
    out[good] = sample(frame, x[good])
    if fill is not None:
        hi = np.array(sz, dtype=np.float64) - 1
        with np.errstate(invalid="ignore"):
            outside = ((x < 0) | (x > hi))[:, active_axes(sz)].any(1)
        out[outside | bad] = fill
    return out.reshape(sz), x, bad


def pullback(frames, beta, times=None, fill=None, tol=TOL, cap=CAP):
    """frames (B,X,Y,Z), beta (10,3,T), times (B) columns of beta (None: 0..B-1) -> (out (B,X,Y,Z), coords (B,P,3), bad points of
    the call)."""
    frames = np.asarray(frames)
    times = list(range(frames.shape[0])) if times is None else [int(t) for t in times]
    out, coords, nbad = [], [], 0
    for j, t in enumerate(times):
        o, x, bad = pullback_frame(frames[j], np.asarray(beta)[:, :, t], fill, tol, cap)
        out.append(o), coords.append(x)
        nbad += int(bad.sum())
    return np.stack(out), np.stack(coords), nbad
