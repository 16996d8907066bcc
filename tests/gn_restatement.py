"""Float64 definition of K16 (``dnmf_warp_normal_eqs``), of ``dnmf_lm_step`` and of the loop ``update_motion(solver='gn')``
runs (include/dnmf_hip.h).  numpy only; the sample and its derivative follow
``oracle.dnmf_oracle.mse_beta_grad_analytic``: the same taps (positions from the reference's fp32 op sequence), in-bounds
corners only.  The tests compare the kernels against these; nothing here is fast."""
import numpy as np

from oracle import dnmf_oracle as orc

F32 = np.float32
# exponents of the reference's basis [1, x, y, z, x^2, y^2, z^2, xy, xz, yz]
EXPO = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0], [0, 2, 0], [0, 0, 2], [1, 1, 0], [1, 0, 1], [0, 1, 1]])


def basis64(P):
    """quadratic_basis in float64: (..., 3) -> (..., 10)."""
    P = np.asarray(P, dtype=np.float64)
    return np.stack([np.prod(P ** e, axis=-1) for e in EXPO], axis=-1)


def centre(sz):
    """(s, o) with u_d = s_d x_d + o_d = 2 x_d / (S_d - 1) - 1, and u_d = 0 on an axis of one voxel."""
    s = np.array([2.0 / (int(n) - 1) if int(n) > 1 else 0.0 for n in sz])
    o = np.array([-1.0 if int(n) > 1 else 0.0 for n in sz])
    return s, o


def centred_lattice(sz):
    s, o = centre(sz)
    return orc.voxel_lattice(sz).astype(np.float64) * s + o


def active(sz):
    """Parameter indices a*3+d that are unknowns: all 30, at Z == 1 the 12 without z."""
    if int(sz[2]) > 1:
        return np.arange(30)
    return np.array([a * 3 + d for a in range(10) if EXPO[a, 2] == 0 for d in range(2)])


def change_of_basis(sz):
    """M (10,10): basis(u(v)) . gamma == basis(v) . (M gamma).  Column c = the centred monomial c multiplied out."""
    s, o = centre(sz)
    M = np.zeros((10, 10))
    for c in range(10):
        poly = {(0, 0, 0): 1.0}           # exponents -> coefficient, in raw coordinates
        for d in range(3):
            for _ in range(EXPO[c, d]):   # times (s_d x_d + o_d)
                nxt = {}
                for e, v in poly.items():
                    up = tuple(e[k] + (k == d) for k in range(3))
                    nxt[up] = nxt.get(up, 0.0) + v * s[d]
                    nxt[e] = nxt.get(e, 0.0) + v * o[d]
                poly = nxt
        for e, v in poly.items():
            M[[tuple(x) for x in EXPO].index(e), c] += v
    return M


def to_raw_grad(g, sz):
    """Gradient w.r.t. the centred coefficients (30,) -> w.r.t. beta (10,3): g_centred = M^T g_beta on the active unknowns."""
    M = change_of_basis(sz)
    rows = sorted({int(i) // 3 for i in active(sz)})
    nd = 3 if int(sz[2]) > 1 else 2
    out = np.zeros((10, 3))
    out[np.ix_(rows, range(nd))] = np.linalg.solve(M[np.ix_(rows, rows)].T, np.asarray(g).reshape(10, 3)[np.ix_(rows, range(nd))])
    return out


def source_coords(beta_t, sz, exact=False):
    """Source coordinates (voxel units) (X,Y,Z,3) float64 of every voxel under beta_t (10,3).  Default: the reference's fp32 op
    sequence (einsum, normalise, un-normalise), which decides the taps; ``exact``: the same map in float64 (differentiable
    by finite differences).  Z == 1: z pinned to slice 0."""
    if exact:
        u = basis64(orc.voxel_lattice(sz)) @ np.asarray(beta_t, dtype=np.float64)
    else:
        basis = orc.quadratic_basis(orc.voxel_lattice(sz))
        _, n = orc.poly_grid(basis, np.ascontiguousarray(np.asarray(beta_t, dtype=F32)[:, :, None]), sz)
        u = np.stack([orc._unnormalize(n[..., d, 0], int(sz[d])).astype(np.float64) for d in range(3)], axis=-1)
    if int(sz[2]) == 1:
        u[..., 2] = 0.0
    return u


def sample(s, u):
    """Zero-padded trilinear sample of the image s (X,Y,Z) at u (X,Y,Z,3) and its derivative w.r.t. u: (rec, dq (3,X,Y,Z)),
    in-bounds corners only (ATen grid_sampler_3d forward / backward).  u may cover any block of voxels (..., 3): rec and dq
    then have its shape."""
    dims = s.shape
    f = np.floor(u)
    rec = np.zeros(u.shape[:-1])
    dq = np.zeros((3,) + u.shape[:-1])
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                off = (dx, dy, dz)
                c = [f[..., d] + off[d] for d in range(3)]
                ok = np.ones(u.shape[:-1], bool)
                for d in range(3):
                    ok &= (c[d] >= 0) & (c[d] <= dims[d] - 1)
                ci = [np.clip(c[d], 0, dims[d] - 1).astype(np.int64) for d in range(3)]
                val = np.where(ok, s[ci[0], ci[1], ci[2]], 0.0)
                w = [(u[..., d] - f[..., d]) if off[d] else (f[..., d] + 1 - u[..., d]) for d in range(3)]
                sg = [1.0 if off[d] else -1.0 for d in range(3)]
                rec += val * w[0] * w[1] * w[2]
                dq[0] += val * sg[0] * w[1] * w[2]
                dq[1] += val * w[0] * sg[1] * w[2]
                dq[2] += val * w[0] * w[1] * sg[2]
    if dims[2] == 1:
        dq[2] = 0.0
    return rec, dq


def recon_images(A, C, times):
    """S[b] = A . C[:, times[b]] in float64, (B,X,Y,Z)."""
    A = np.asarray(A, dtype=np.float64)
    return np.stack([A @ np.asarray(C, dtype=np.float64)[:, t] for t in times])


def residual(S_b, beta_t, sz, frame, exact=False):
    rec, dq = sample(np.asarray(S_b, dtype=np.float64), source_coords(beta_t, sz, exact))
    return rec - np.asarray(frame, dtype=np.float64).reshape(rec.shape), dq


def normal_eqs(A, C, beta, sz, times, frames, S=None):
    """H (B,30,30), g (B,30), sse (B) of the frames ``times`` at beta[:, :, times]; frames (B,X,Y,Z) (frame b belongs to
    times[b]).  ``S`` (B,X,Y,Z): the reconstruction images to use instead of A . C (the kernel's own fp32 input)."""
    times = list(times)
    B = len(times)
    S = recon_images(A, C, times) if S is None else np.asarray(S, dtype=np.float64)
    phi = basis64(centred_lattice(sz)).reshape(-1, 10)
    H, g, sse = np.zeros((B, 30, 30)), np.zeros((B, 30)), np.zeros(B)
    for b, t in enumerate(times):
        bt = np.asarray(beta, dtype=F32)[:, :, t]
        if not np.isfinite(bt).all():
            sse[b] = np.nan
            continue
        r, dq = residual(S[b], bt, sz, frames[b])
        J = (phi[:, :, None] * dq.reshape(3, -1).T[:, None, :]).reshape(-1, 30)
        H[b], g[b], sse[b] = J.T @ J, J.T @ r.ravel(), float((r ** 2).sum())
    return H, g, sse


def new_state(B):
    return {"H": np.zeros((B, 30, 30)), "g": np.zeros((B, 30)), "sse": np.zeros(B), "sse0": np.zeros(B), "lam": np.zeros(B),
            "beta": np.zeros((B, 30), dtype=F32), "counts": np.zeros((B, 3), dtype=np.int64)}


def damped_system(H, g, lam, sz):
    """(A_hat, rhs_hat, scale) of (H + lam diag(H) + tiny I) delta = -g on the active unknowns, scaled to a unit diagonal:
    delta[active] = scale * solve(A_hat, rhs_hat)."""
    act = active(sz)
    Ha = H[np.ix_(act, act)]
    dg = np.diag(Ha)
    tiny = 1e-12 * dg.max() + 1e-30
    Ad = Ha + np.diag(lam * dg + tiny)
    sc = 1.0 / np.sqrt(np.diag(Ad))
    return Ad * sc[:, None] * sc[None, :], -g[act] * sc, sc


def lm_step(state, H, g, sse, beta, times, sz, nu=10.0, lam0=1e-3, lam_min=1e-9, lam_max=1e9, accept_only=False):
    """dnmf_lm_step on numpy arrays: ``state`` as ``new_state``, the trial coefficients in beta (10,3,T) fp32 (rewritten in
    place).  Returns dict(accept (B) bool, dbeta (B,10,3))."""
    M = change_of_basis(sz)
    act = active(sz)
    B = len(times)
    accepted, dbeta = np.zeros(B, bool), np.zeros((B, 10, 3))
    for b, t in enumerate(times):
        first = state["counts"][b, 2] == 0
        acc = bool(first or (np.isfinite(sse[b]) and sse[b] < state["sse"][b]))
        if first:
            state["lam"][b], state["sse0"][b], state["counts"][b, 2] = lam0, sse[b], 1
        else:
            state["lam"][b] = max(state["lam"][b] / nu, lam_min) if acc else min(state["lam"][b] * nu, lam_max)
            state["counts"][b, 0 if acc else 1] += 1
        if acc:
            state["H"][b], state["g"][b], state["sse"][b] = H[b], g[b], sse[b]
            state["beta"][b] = beta[:, :, t].reshape(30)
        accepted[b] = acc
        if accept_only:
            beta[:, :, t] = state["beta"][b].reshape(10, 3)
            continue
        delta = np.zeros(30)
        Ah, rh, sc = damped_system(state["H"][b], state["g"][b], state["lam"][b], sz)
        try:
            with np.errstate(all="ignore"):
                if not np.isfinite(Ah).all():
                    raise np.linalg.LinAlgError
                L = np.linalg.cholesky(Ah)
                delta[act] = sc * np.linalg.solve(L.T, np.linalg.solve(L, rh))
        except np.linalg.LinAlgError:
            pass
        dbeta[b] = M @ delta.reshape(10, 3)
        beta[:, :, t] = (state["beta"][b].reshape(10, 3).astype(np.float64) + dbeta[b]).astype(F32)
    return {"accept": accepted, "dbeta": dbeta}


def fit_gn(A, C, beta, sz, times, frames, iters, damping=1e-3):
    """The loop of update_motion(solver='gn') for the frames ``times``: ``iters`` pairs normal_eqs -> lm_step, then one more
    normal_eqs and an accept-only step.  Returns (beta (10,3,T) fp32, state, history of state['sse'] after every step)."""
    beta = np.array(beta, dtype=F32)
    times = list(times)
    S = recon_images(A, C, times)
    state, hist = new_state(len(times)), []
    for it in range(iters + 1):
        H, g, sse = normal_eqs(None, None, beta, sz, times, frames, S=S)
        lm_step(state, H, g, sse, beta, times, sz, lam0=damping, accept_only=it == iters)
        hist.append(state["sse"].copy())
    return beta, state, hist


def field_error(beta, beta_ref, sz):
    """Largest distance (voxels) over the lattice and the frames between the points two sets of coefficients (10,3,T) map a
    voxel to (the z component is left out at Z == 1, where it is never used)."""
    bas = basis64(orc.voxel_lattice(sz)).reshape(-1, 10)
    nd = 3 if int(sz[2]) > 1 else 2
    d = np.einsum("pa,adt->pdt", bas, np.asarray(beta, np.float64) - np.asarray(beta_ref, np.float64))[:, :nd]
    return float(np.sqrt((d ** 2).sum(1)).max())


def fit_problem(sz, K=6, T=5, seed=0, affine=0.03, shift=0.6, quad=0.25, zpart=0.0):
    """A noise-free motion problem: K Gaussians (sigma 3), random traces in [0.5, 1.5], a warp beta* = identity + a shift of
    up to ``shift`` voxels + an affine part of up to ``affine`` + quadratic terms that displace the far corner by up to
    ``quad`` voxels each, the z component of all of them times ``zpart`` (default: none along z.  With two slices a z-tap that leaves the
    volume is dropped, so the loss has a kink exactly at "no motion along z" and no solver converges fast across it: with
    zpart = 0.1 the float64 fit below is still 0.03 .. 1.2 voxels off after 8 iterations; x and y still depend on the slice); frames = the oracle forward at beta*.  Returns dict(A, C, beta_true, frames (T,X,Y,Z) fp32, pos)."""
    rng = np.random.default_rng(seed)
    sz = [int(s) for s in sz]
    nd = 3 if sz[2] > 1 else 2
    pos = np.stack([rng.uniform(3, sz[d] - 4, K) if sz[d] > 8 else rng.uniform(0, sz[d] - 1, K) for d in range(3)], 1).astype(F32)
    A = orc.gaussian_footprints(sz, pos, np.full(K, 3.0, F32))
    C = rng.uniform(0.5, 1.5, (K, T)).astype(F32)
    beta = orc.identity_beta(T).astype(np.float64)
    ext = np.array([max(s - 1, 1) for s in sz], dtype=np.float64)
    for t in range(T):
        beta[0, :nd, t] += rng.uniform(-shift, shift, nd)
        beta[1:1 + nd, :nd, t] += rng.uniform(-affine, affine, (nd, nd))
        for a in range(4, 10):
            if nd == 2 and EXPO[a, 2]:
                continue
            beta[a, :nd, t] += rng.uniform(-quad, quad, nd) / np.prod(ext ** EXPO[a])
    ident = orc.identity_beta(T).astype(np.float64)
    beta[:, 2] = ident[:, 2] + zpart * (beta[:, 2] - ident[:, 2])
    beta = beta.astype(F32)
    basis = orc.quadratic_basis(orc.voxel_lattice(sz))
    frames = orc.forward(A, basis, beta, sz, list(range(T)), C)[0].astype(F32)
    return {"A": A, "C": C, "beta_true": beta, "frames": frames, "pos": pos}
