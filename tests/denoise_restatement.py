"""K34 restated in float64 numpy: local low-rank denoising of a registered movie -- per patch a truncated SVD by subspace
iteration and Rayleigh-Ritz, the patches blended by tent weights.  This file is the definition; csrc/lowrank_denoise.hip,
include/dnmf_hip.h and the tests refer to it.

L1  patch_plan: along each axis the stride is patch - overlap, patch i starts at min(i stride, max(extent - patch, 0)), the last
    patch ends at the extent, a patch larger than the axis is the axis; None in z is min(Z, 4).  n = the voxels of a patch, at
    most 1024.  Every patch has the same shape.  boxes (NP, 6) int32 inclusive [x0, x1, y0, y1, z0, z1], x slowest.
L2  D[v, t] = (y[v, t] - centre[v]) / scale[v], v the voxel's index in the patch (z fastest).  ok = 0 where the patch holds a
    sample or a centre that is not finite, or a scale that is not finite or <= 0: U = Q = 0, lam = 0, kept = 0.
L3  U0[v, j] = cos(pi (v + 1/2) j / n); U = MGS(U0); iters times U = MGS(D (D^T U)); Q = D^T U.  MGS in column order; a column
    whose norm after the projections is <= 1e-12 x its norm before becomes zero.
L4  B = Q^T Q, `sweeps` sweeps of cyclic Jacobi, lam descending (ties by index), U and Q rotated.  keep='auto': kept = the number
    of lam > (threshold (sqrt n + sqrt T))^2; keep=r: the number of lam > 0 among the first r.  explained = sum of the kept lam
    over sum D^2 (0 where that is 0).
L5  out[v, t] = fp32(sum_p w_p (centre[v] + scale[v] sum_{j < kept_p} U_p[v, j] Q_p[t, j]) / sum_p w_p) over the ok patches that
    hold v, w_p = prod_axes min(i + 1, len - i); the input sample where no ok patch holds v.
"""
import numpy as np

MAX_VOXELS = 1024
MAX_RANK = 8
SWEEPS = 10


def patch_plan(sz, patch=(16, 16, None), overlap=(8, 8, 0)):
    sz = [int(s) for s in sz]
    patch = [patch[0], patch[1], min(sz[2], 4) if patch[2] is None else patch[2]]
    starts, lens, strides = [], [], []
    for ext, pa, ov in zip(sz, patch, overlap):
        pa, ov = int(pa), int(ov)
        if ext < 1 or pa < 1 or not 0 <= ov < pa:
            raise ValueError(f"patch_plan: extent {ext}, patch {pa}, overlap {ov}")
        stride = pa - ov
        count = 1 if ext <= pa else -((pa - ext) // stride) + 1
        starts.append(np.minimum(np.arange(count, dtype=np.int64) * stride, max(ext - pa, 0)))
        lens.append(min(pa, ext))
        strides.append(stride)
    n = lens[0] * lens[1] * lens[2]
    if n > MAX_VOXELS:
        raise ValueError(f"patch_plan: a patch of {n} voxels, at most {MAX_VOXELS}")
    boxes = np.array([[x, x + lens[0] - 1, y, y + lens[1] - 1, z, z + lens[2] - 1]
                      for x in starts[0] for y in starts[1] for z in starts[2]], dtype=np.int32)
    return dict(boxes=boxes, counts=tuple(len(s) for s in starts), shape=tuple(lens), strides=tuple(strides), n=n,
                starts=tuple(starts))


def start_basis(n, R):
    v = np.arange(n, dtype=np.float64)[:, None]
    j = np.arange(R, dtype=np.float64)[None, :]
    return np.cos(np.pi * (v + 0.5) * j / n)


def mgs(W):
    U = np.array(W, dtype=np.float64)
    for j in range(U.shape[1]):
        before = np.sqrt(np.sum(U[:, j] * U[:, j]))
        for i in range(j):
            U[:, j] = U[:, j] - np.sum(U[:, i] * U[:, j]) * U[:, i]
        after = np.sqrt(np.sum(U[:, j] * U[:, j]))
        U[:, j] = 0.0 if after <= 1e-12 * before else U[:, j] / after
    return U


def jacobi(B, sweeps=SWEEPS):
    """(diagonal, V) after ``sweeps`` cyclic sweeps over the pairs (x < y) of the symmetric B: B -> J^T B J, V -> V J."""
    B = np.array(B, dtype=np.float64)
    R = B.shape[0]
    V = np.eye(R)
    for _ in range(sweeps):
        for x in range(R - 1):
            for y in range(x + 1, R):
                bxy = B[x, y]
                if bxy == 0.0:
                    continue
                with np.errstate(over="ignore", divide="ignore"):
                    tau = (B[y, y] - B[x, x]) / (2.0 * bxy)
                    t = (1.0 if tau >= 0.0 else -1.0) / (abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                for M, cols in ((B, True), (B, False), (V, True)):
                    if cols:
                        u, v = M[:, x].copy(), M[:, y].copy()
                        M[:, x], M[:, y] = c * u - s * v, s * u + c * v
                    else:
                        u, v = M[x, :].copy(), M[y, :].copy()
                        M[x, :], M[y, :] = c * u - s * v, s * u + c * v
    return np.diag(B).copy(), V


def edge(n, T, threshold=1.0):
    return (float(threshold) * (np.sqrt(float(n)) + np.sqrt(float(T)))) ** 2


def patch_voxels(box, sz):
    x, y, z = np.meshgrid(np.arange(box[0], box[1] + 1), np.arange(box[2], box[3] + 1), np.arange(box[4], box[5] + 1), indexing="ij")
    return ((x * sz[1] + y) * sz[2] + z).ravel()


def patch_weights(shape):
    w = [np.minimum(np.arange(n) + 1, n - np.arange(n)).astype(np.float64) for n in shape]
    return (w[0][:, None, None] * w[1][None, :, None] * w[2][None, None, :]).ravel()


def patch_factors(D, R, iters, keep, threshold, sweeps=SWEEPS):
    """L3, L4 of one patch: D (n, T) float64 -> U (n, R), Q (T, R), lam (R,), kept, explained."""
    n, T = D.shape
    U = mgs(start_basis(n, R))
    for _ in range(iters):
        U = mgs(D @ (D.T @ U))
    Q = D.T @ U
    lam, V = jacobi(Q.T @ Q, sweeps)
    order = sorted(range(R), key=lambda j: (-lam[j], j))
    lam, V = lam[order], V[:, order]
    U, Q = U @ V, Q @ V
    if keep == "auto":
        kept = int(np.sum(lam > edge(n, T, threshold)))
    else:
        kept = int(np.sum(lam[:int(keep)] > 0.0))
    energy = float(np.sum(D * D))
    return U, Q, lam, kept, (float(np.sum(lam[:kept])) / energy if energy > 0.0 else 0.0)


def denoise(rows, sz, centre, scale=None, patch=(16, 16, None), overlap=(8, 8, 0), rank=8, keep="auto", threshold=1.0, iters=4,
            sweeps=SWEEPS):
    """rows (T, P) fp32, centre / scale (X, Y, Z) float64 (scale None: ones) -> (out (T, P) fp32, info)."""
    rows = np.asarray(rows, dtype=np.float32)
    T, P = rows.shape
    sz = [int(s) for s in sz]
    if not 1 <= rank <= MAX_RANK:
        raise ValueError(f"denoise: rank={rank}")
    plan = patch_plan(sz, patch, overlap)
    NP, n, R = len(plan["boxes"]), plan["n"], rank
    c = np.asarray(centre, dtype=np.float64).reshape(P)
    s = np.ones(P) if scale is None else np.asarray(scale, dtype=np.float64).reshape(P)
    U, Q, lam = np.zeros((NP, n, R)), np.zeros((NP, T, R)), np.zeros((NP, R))
    kept, ok, explained = np.zeros(NP, np.int32), np.zeros(NP, np.int32), np.zeros(NP)
    num, den = np.zeros((P, T)), np.zeros(P)
    w = patch_weights(plan["shape"])
    for p, box in enumerate(plan["boxes"]):
        idx = patch_voxels(box, sz)
        y = rows[:, idx].astype(np.float64).T
        cp, sp = c[idx], s[idx]
        with np.errstate(invalid="ignore"):
            ok[p] = bool(np.isfinite(y).all() and np.isfinite(cp).all() and np.isfinite(sp).all() and (sp > 0).all())
        if not ok[p]:
            continue
        D = (y - cp[:, None]) / sp[:, None]
        U[p], Q[p], lam[p], kept[p], explained[p] = patch_factors(D, R, iters, keep, threshold, sweeps)
        k = kept[p]
        num[idx] += w[:, None] * (cp[:, None] + sp[:, None] * (U[p][:, :k] @ Q[p][:, :k].T))
        den[idx] += w
    out = rows.copy()
    covered = den > 0
    out[:, covered] = (num[covered] / den[covered][:, None]).T.astype(np.float32)
    return out, dict(plan=plan, U=U, Q=Q, lam=lam, kept=kept, ok=ok, explained=explained)


def planted_video(Z=1, seed=0, sz=(40, 36), T=120, noise=1.0):
    """The planted movie of the tests, (T, X, Y, Z): three static blobs with independent on/off time courses and a smooth rank-1
    background, plus unit-variance noise -> (noisy fp32, clean float64).  A blob is a Gaussian cut to one 8 x 8 cell of the
    stride grid of the default plan (patch 16, overlap 8), away from the clamped last row of patches: a patch holds a blob whole
    or not at all, so no patch sees a sliver of one near the noise edge.  Singular values of (y - mean) in a patch of n voxels:
    the background about 5 sqrt(T / 2) sqrt(n) (above 600), a blob amp x |blob| x |on - mean(on)|, about amp x 3.6 x 5 (above
    160), against sqrt(n) + sqrt(T) (27 at Z = 1, 34 at Z = 2); tests/test_denoise_host.py checks it with the SVD."""
    rng = np.random.default_rng(seed)
    X, Y = sz
    x, y = np.meshgrid(np.arange(X, dtype=np.float64), np.arange(Y, dtype=np.float64), indexing="ij")
    clean = np.zeros((T, X, Y, Z))
    t = np.arange(T, dtype=np.float64)
    bg = 1.0 + 0.2 * np.cos(np.pi * x / X) * np.cos(np.pi * y / Y)
    clean += (10.0 * (1.0 + 0.5 * np.sin(2 * np.pi * t / T)))[:, None, None, None] * bg[None, :, :, None]
    for cellx, celly, amp in ((1, 1, 12.0), (2, 0, 9.0), (3, 1, 15.0)):
        inside = (x // 8 == cellx) & (y // 8 == celly)
        blob = np.exp(-((x - 8 * cellx - 3.5) ** 2 + (y - 8 * celly - 3.5) ** 2) / (2 * 2.5 ** 2)) * inside
        on = (rng.random(T // 8 + 1) < 0.4).repeat(8)[:T].astype(np.float64)
        clean += amp * on[:, None, None, None] * blob[None, :, :, None]
    noisy = clean + noise * rng.standard_normal(clean.shape)
    return noisy.astype(np.float32), clean
