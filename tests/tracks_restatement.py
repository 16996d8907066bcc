"""numpy float64 restatement of the three track operations (K11 fit, K12 inverse, K13 ROI read-out), written from their
definitions in include/dnmf_hip.h / DESIGN.md.  The tests compare the kernels against these; nothing here is fast."""
import numpy as np

ORDERS = {"translation": 0, "affine": 1, "quadratic": 2}
# rows of the basis that involve axis d
USES = ((1, 4, 7, 8), (2, 5, 7, 9), (3, 6, 8, 9))
IDENTITY = np.concatenate((np.zeros((1, 3)), np.eye(3), np.zeros((6, 3))), 0)


def basis(p):
    """(..., 3) -> (..., 10): [1, x, y, z, x^2, y^2, z^2, xy, xz, yz]."""
    p = np.asarray(p, dtype=np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack((np.ones_like(x), x, y, z, x * x, y * y, z * z, x * y, x * z, y * z), -1)


def warp(beta_t, p):
    """q_t(p) for one frame: beta_t (10,3), p (...,3)."""
    return basis(p) @ np.asarray(beta_t, dtype=np.float64)


def free_rows(sz, order):
    rows = {0: [0], 1: [0, 1, 2, 3], 2: list(range(10))}[ORDERS.get(order, order)]
    for d in range(3):
        if sz[d] == 1:
            rows = [r for r in rows if r not in USES[d]]
    return rows


def normalise(sz, p):
    """u = 2 p / (S - 1) - 1 per axis, 0 on an axis of extent 1."""
    sz = np.asarray(sz, dtype=np.float64)
    a = np.where(sz > 1, 2.0 / np.maximum(sz - 1, 1), 0.0)
    c = np.where(sz > 1, -1.0, 0.0)
    return np.asarray(p, dtype=np.float64) * a + c, a, c


def identity_normalised(sz):
    """B'_id: the identity map p = h u + h written on basis(u), h = (S - 1) / 2."""
    h = 0.5 * (np.asarray(sz, dtype=np.float64) - 1)
    B = np.zeros((10, 3))
    B[0] = h
    B[1:4] = np.diag(h)
    return B


def change_of_basis(sz):
    """M (10,10) with basis(u) = M basis(x) for u = a x + c: beta = M^T B'."""
    _, a, c = normalise(sz, np.zeros(3))
    M = np.zeros((10, 10))
    M[0, 0] = 1
    for d in range(3):
        M[1 + d, 0], M[1 + d, 1 + d] = c[d], a[d]
        M[4 + d, 0], M[4 + d, 1 + d], M[4 + d, 4 + d] = c[d] ** 2, 2 * a[d] * c[d], a[d] ** 2
    for row, (d, e) in ((7, (0, 1)), (8, (0, 2)), (9, (1, 2))):
        M[row, 0], M[row, 1 + d], M[row, 1 + e], M[row, row] = c[d] * c[e], a[d] * c[e], a[e] * c[d], a[d] * a[e]
    return M


def solve_pivoted(N, rhs, tiny):
    """Gaussian elimination with partial pivoting (the first of equal pivots); ok = every pivot above ``tiny``."""
    n = N.shape[0]
    M = np.concatenate((N, rhs), 1).astype(np.float64)
    ok = True
    with np.errstate(all="ignore"):
        for p in range(n):
            r = p + int(np.argmax(np.abs(M[p:, p])))
            M[[p, r]] = M[[r, p]]
            if not abs(M[p, p]) > tiny:
                ok = False
            for i in range(p + 1, n):
                M[i] -= (M[i, p] / M[p, p]) * M[p]
        x = np.zeros((n, rhs.shape[1]))
        for i in range(n - 1, -1, -1):
            x[i] = (M[i, n:] - M[i, i + 1:n] @ x[i + 1:]) / M[i, i]
    return x, ok


def fit_system(P_t, R, sz, order):
    """The least-squares system of one frame in normalised inputs: (Phi (n,nfree), E (n,3) = R - p of the tracked neurons,
    rows)."""
    P_t, R = np.asarray(P_t, dtype=np.float64), np.asarray(R, dtype=np.float64)
    rows = free_rows(sz, order)
    tracked = np.isfinite(P_t).all(1)
    u, _, _ = normalise(sz, P_t[tracked])
    h = 0.5 * (np.asarray(sz, dtype=np.float64) - 1)
    E = R[tracked] - (h * u + h)
    E[:, np.asarray(sz) == 1] = 0.0       # the output column of an axis of extent 1 stays at the identity
    return basis(u)[:, rows], E, rows


def fit_frame(P_t, R, sz, order="quadratic", ridge=0.0):
    """beta_t (10,3) float32 and ok for one frame: P_t (K,3) (NaN = not tracked), R (K,3)."""
    Phi, E, rows = fit_system(P_t, R, sz, order)
    N = Phi.T @ Phi + ridge * np.eye(len(rows))
    ok = not (ridge == 0 and Phi.shape[0] < len(rows))
    scale = N.diagonal().max() if len(rows) else 0.0
    D, solved = solve_pivoted(N, Phi.T @ E, 1e-12 * scale)
    ok = ok and solved and scale > 0 and np.isfinite(D).all()
    if not ok:
        return IDENTITY.astype(np.float32), False
    Bp = identity_normalised(sz)
    Bp[rows] += D
    beta = change_of_basis(sz).T @ Bp
    for d in range(3):
        if sz[d] == 1:
            beta[:, d] = IDENTITY[:, d]
    return beta.astype(np.float32), True


def fit_quadratic_warp(P, R, sz, order="quadratic", ridge=0.0):
    """P (K,3,T), R (K,3) -> beta (10,3,T) float32, ok (T) bool."""
    P = np.asarray(P, dtype=np.float64)
    T = P.shape[2]
    beta, ok = np.empty((10, 3, T), dtype=np.float32), np.empty(T, dtype=bool)
    for t in range(T):
        beta[:, :, t], ok[t] = fit_frame(P[:, :, t], R, sz, order, ridge)
    return beta, ok


def jacobian(b, x):
    """d q_d / d x_e of q = basis(x) b: the true Jacobian of the basis (row 8 = xz, row 9 = yz)."""
    J = np.empty((3, 3))
    for d in range(3):
        J[d, 0] = b[1, d] + 2 * b[4, d] * x[0] + b[7, d] * x[1] + b[8, d] * x[2]
        J[d, 1] = b[2, d] + 2 * b[5, d] * x[1] + b[7, d] * x[0] + b[9, d] * x[2]
        J[d, 2] = b[3, d] + 2 * b[6, d] * x[2] + b[8, d] * x[0] + b[9, d] * x[1]
    return J


def invert_point(b, r, start=None, tol=1e-6, cap=32):
    b, r = np.asarray(b, dtype=np.float64), np.asarray(r, dtype=np.float64)
    x = r.copy() if start is None else np.asarray(start, dtype=np.float64).copy()
    for _ in range(cap):
        J = jacobian(b, x)
        if not abs(np.linalg.det(J)) >= 1e-12:
            break
        step = np.linalg.solve(J, warp(b, x) - r)
        x = x - step
        if not np.isfinite(x).all():
            break
        if (np.abs(step) < tol).all():
            return x
    return np.full(3, np.nan)


def invert_quadratic_warp(beta, targets, times=None, start=None, tol=1e-6):
    """beta (10,3,T), targets (K,3) -> (K,3,B) float64: the x* with q_t(x*) = targets[k] for t in ``times``."""
    beta = np.asarray(beta, dtype=np.float64)
    times = list(range(beta.shape[2])) if times is None else [int(t) for t in times]
    K = len(targets)
    out = np.empty((K, 3, len(times)))
    for j, t in enumerate(times):
        for k in range(K):
            out[k, :, j] = invert_point(beta[:, :, t], targets[k], None if start is None else start[k, :, j], tol)
    return out


def roi_signals(video, P, window=(3, 3, 0)):
    """video (X,Y,Z,T), P (K,3,T) -> (K,T): mean of the box of 2 w + 1 voxels per axis around round-half-even(P); voxels of
    the box outside the volume are zeros that count, NaN voxels are left out; NaN for a centre outside the volume."""
    video, P = np.asarray(video, dtype=np.float64), np.asarray(P, dtype=np.float64)
    sz = video.shape[:3]
    K, _, T = P.shape
    w = [int(v) for v in window]
    out = np.full((K, T), np.nan)
    for t in range(T):
        for k in range(K):
            if not np.isfinite(P[k, :, t]).all():
                continue
            c = np.rint(P[k, :, t]).astype(np.int64)
            if any(c[d] < 0 or c[d] >= sz[d] for d in range(3)):
                continue
            box = np.zeros([2 * v + 1 for v in w])
            lo = [max(c[d] - w[d], 0) for d in range(3)]
            hi = [min(c[d] + w[d] + 1, sz[d]) for d in range(3)]
            dst = tuple(slice(lo[d] - (c[d] - w[d]), hi[d] - (c[d] - w[d])) for d in range(3))
            box[dst] = video[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2], t]
            good = ~np.isnan(box)
            if good.any():
                out[k, t] = box[good].sum() / good.sum()
    return out
