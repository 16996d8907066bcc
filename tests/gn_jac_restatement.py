"""Float64 definition of the volume-preserving prior of the Gauss-Newton motion solver (K16j: ``dnmf_lm_step_jac`` and the loop
``update_motion(solver='gn')`` runs when ``model.motion_jacobian`` is set; include/dnmf_hip.h).  numpy only, on top of
tests/gn_restatement.py, tests/gn_smooth_restatement.py and tests/gn_order_restatement.py.

theta (30, index a*3 + d) are a frame's coefficients in K16's centred basis on the active unknowns.  The frame's map is
q_d(u) = sum_a basis_a(u) theta[a,d], basis(u) = [1, u0, u1, u2, u0^2, u1^2, u2^2, u0 u1, u0 u2, u1 u2], u_d = 2 x_d / (S_d - 1) - 1;
Ju[d][e] = d q_d / d u_e and the Jacobian in voxel coordinates is Jx = Ju diag(1 / h), h_e = (S_e - 1) / 2 -- 3 x 3, or 2 x 2 over
(x, y) at Z == 1.  It is the TRUE Jacobian of the model's map, not the reference's ``log_det_jac`` (which swaps the xz and yz rows).
At the sample points ``points(sz)`` the residual is rho_p = log det Jx(u_p) = log det Ju(u_p) - sum_e log h_e, +inf where
det Jx(u_p) <= 0 or is not finite, and the prior of a frame with n residuals is J = m_j / NP sum_p rho_p^2, m_j = jacobian * n:
F / n = mse + jacobian * mean_p rho_p^2.  The columns of Ju are divided by h before the determinant is taken, so that the
identity gives rho = 0 exactly.

det Jx is a cubic polynomial in u: J finite says the map does not fold AT THE SAMPLE POINTS, no more."""
import itertools

import numpy as np

import gn_order_restatement as GO
import gn_restatement as GN
import gn_smooth_restatement as GS

F32 = np.float32


def naxes(sz):
    return 3 if int(sz[2]) > 1 else 2


def points(sz):
    """(NP,3) float64: the corners u in {-1, +1}^n in the order of counting, first axis slowest, then the centre u = 0.  NP = 9;
    5 at Z == 1, where u_2 = 0 throughout."""
    n = naxes(sz)
    pts = [list(c) + [0.0] * (3 - n) for c in itertools.product((-1.0, 1.0), repeat=n)]
    return np.array(pts + [[0.0, 0.0, 0.0]])


def half_extents(sz):
    """h_e = (S_e - 1) / 2 on the active axes."""
    return np.array([(int(sz[e]) - 1) / 2.0 for e in range(naxes(sz))])


def dbasis(u):
    """(10,3): d basis_a / d u_e at u."""
    u0, u1, u2 = (float(x) for x in u)
    D = np.zeros((10, 3))
    D[1, 0], D[2, 1], D[3, 2] = 1.0, 1.0, 1.0
    D[4, 0], D[5, 1], D[6, 2] = 2 * u0, 2 * u1, 2 * u2
    D[7, 0], D[7, 1] = u1, u0
    D[8, 0], D[8, 2] = u2, u0
    D[9, 1], D[9, 2] = u2, u1
    return D


def theta_identity(sz):
    """theta (30,) of the identity map x_d = h_d (u_d + 1), exactly."""
    th = np.zeros((10, 3))
    for d, h in enumerate(half_extents(sz)):
        th[0, d], th[1 + d, d] = h, h
    return th.reshape(30)


def theta_affine(sz, R, c):
    """theta (30,) of the map x -> R x + c in voxel coordinates (R (n,n), c (n,), n the active axes)."""
    n, h = naxes(sz), half_extents(sz)
    th = np.zeros((10, 3))
    th[0, :n] = R @ h + c                    # x = h (u + 1)
    for e in range(n):
        th[1 + e, :n] = R[:, e] * h[e]
    return th.reshape(30)


def jacobians(th, sz):
    """Jx (NP,n,n) of theta (30,) at the sample points."""
    n, h = naxes(sz), half_extents(sz)
    th = np.asarray(th, dtype=np.float64).reshape(10, 3)
    return np.stack([(th[:, :n].T @ dbasis(u)[:, :n]) / h[None, :] for u in points(sz)])


def residuals(th, sz):
    """(rho (NP), det Jx (NP)); rho = +inf where det Jx <= 0 or is not finite."""
    with np.errstate(all="ignore"):
        det = np.array([np.linalg.det(J) if np.isfinite(J).all() else np.nan for J in jacobians(th, sz)])
        ok = np.isfinite(det) & (det > 0)
        rho = np.where(ok, np.log(np.where(ok, det, 1.0)), np.inf)
    return rho, det


def rows(th, sz, act=None):
    """jrho (NP,30): the gradient of rho_p with respect to theta, jrho_p[a*3+d] = sum_e (Jx^-1)[e][d] (d basis_a / d u_e)(u_p) / h_e,
    on the unknowns ``act`` (default: every active one), zeros elsewhere and in the row of a point whose rho is not finite."""
    n, h = naxes(sz), half_extents(sz)
    act = GN.active(sz) if act is None else act
    rho, _ = residuals(th, sz)
    out = np.zeros((len(rho), 30))
    for p, (u, J) in enumerate(zip(points(sz), jacobians(th, sz))):
        if not np.isfinite(rho[p]):
            continue
        full = np.zeros((10, 3))
        full[:, :n] = (dbasis(u)[:, :n] / h[None, :]) @ np.linalg.inv(J)
        out[p, act] = full.reshape(30)[act]
    return out


def prior(th, sz, mj):
    """J = mj / NP sum_p rho_p^2 (0.0 with mj == 0)."""
    if mj == 0:
        return 0.0
    rho, _ = residuals(th, sz)
    with np.errstate(all="ignore"):
        return float((mj / len(rho)) * (rho ** 2).sum())


def prior_grad(th, sz, mj, act=None):
    """(gradient (30,) of ``prior`` / 2 -- what the step adds to g' -- and the Gauss-Newton term (30,30) it adds to H')."""
    rho, _ = residuals(th, sz)
    jr = rows(th, sz, act)
    w = mj / len(rho)
    gadd, Hadd = np.zeros(30), np.zeros((30, 30))
    for p in range(len(rho)):
        if np.isfinite(rho[p]):
            gadd += rho[p] * jr[p]
        Hadd += np.outer(jr[p], jr[p])
    return w * gadd, w * Hadd


def full_theta(beta_t, sz):
    """theta on every active unknown, whatever the order: rho sees the whole map."""
    return GS.theta(beta_t, sz)


def new_state(B):
    st = GS.new_state(B)
    st["jac"], st["min_det"] = np.zeros(B), np.zeros(B)
    return st


def lm_step(state, H, g, sse, beta, times, sz, order="quadratic", nu=10.0, lam0=1e-3, lam_min=1e-9, lam_max=1e9, accept_only=False,
            m=0.0, beta_ref=None, mj=0.0, rows_of=None):
    """dnmf_lm_step_jac on numpy arrays: ``GO.lm_step`` with J added to both sides of the accept test and its Gauss-Newton terms to
    the step system, both at the point kept and on the unknowns of ``order``.  ``mj`` == 0 takes ``GO.lm_step``'s steps, operation
    for operation.  ``state`` from ``new_state``; it receives ``jac`` and ``min_det`` when mj != 0.  Returns dict(accept (B) bool,
    dbeta (B,10,3), system (B) of (H', g'), folded (B) bool: the trial folds at a sample point)."""
    M = GN.change_of_basis(sz)
    act = GO.active(sz, order)
    B = len(times)
    rws = list(range(B)) if rows_of is None else list(rows_of)
    accepted, dbeta, systems, folded = np.zeros(B, bool), np.zeros((B, 10, 3)), [], np.zeros(B, bool)
    for i, t in enumerate(times):
        b = rws[i]
        ths = [GO.theta(beta_ref[:, :, s], sz, order) for s in GS.neighbours(t, beta_ref)] if m != 0 else []
        first = state["counts"][b, 2] == 0
        th_trial, th_acc = GO.theta(beta[:, :, t], sz, order), GO.theta(state["beta"][b], sz, order)
        p_trial, p_acc = GS.prior(th_trial, ths, m), GS.prior(th_acc, ths, m)
        tf_trial = full_theta(beta[:, :, t], sz)
        tf_acc = np.zeros(30) if first else full_theta(state["beta"][b], sz)
        j_trial, j_acc = prior(tf_trial, sz, mj), prior(tf_acc, sz, mj)
        folded[i] = not np.isfinite(residuals(tf_trial, sz)[0]).all()
        with np.errstate(all="ignore"):
            f_trial, f_acc = sse[i] + p_trial, state["sse"][b] + p_acc
            if mj != 0:
                f_trial, f_acc = f_trial + j_trial, f_acc + j_acc
        acc = bool(first or (np.isfinite(f_trial) and f_trial < f_acc))
        if first:
            state["lam"][b], state["sse0"][b], state["counts"][b, 2] = lam0, sse[i], 1
        else:
            state["lam"][b] = max(state["lam"][b] / nu, lam_min) if acc else min(state["lam"][b] * nu, lam_max)
            state["counts"][b, 0 if acc else 1] += 1
        if acc:
            state["H"][b], state["g"][b], state["sse"][b] = H[i], g[i], sse[i]
            state["beta"][b] = beta[:, :, t].reshape(30)
            if m != 0:
                beta_ref[:, :, t] = beta[:, :, t]
            th_acc, tf_acc = th_trial, tf_trial
        if m != 0:
            state["prior"][b] = p_trial if acc else p_acc
        if mj != 0:
            state["jac"][b] = j_trial if acc else j_acc
            state["min_det"][b] = np.min(residuals(tf_acc, sz)[1])
        accepted[i] = acc
        Hp, gp = state["H"][b].copy(), state["g"][b].copy()
        if ths:
            Hp[act, act] += m * len(ths)
            gp[act] += (m * sum(th_acc - ts for ts in ths))[act]
        if mj != 0:
            gadd, Hadd = prior_grad(tf_acc, sz, mj, act)
            Hp += Hadd
            gp += gadd
        systems.append((Hp, gp))
        if accept_only:
            beta[:, :, t] = state["beta"][b].reshape(10, 3)
            continue
        delta = np.zeros(30)
        try:
            with np.errstate(all="ignore"):
                Ah, rh, sc = GO.damped_system(Hp, gp, state["lam"][b], act)
                if not np.isfinite(Ah).all():
                    raise np.linalg.LinAlgError
                L = np.linalg.cholesky(Ah)
                delta[act] = sc * np.linalg.solve(L.T, np.linalg.solve(L, rh))
        except np.linalg.LinAlgError:
            pass
        dbeta[i] = M @ delta.reshape(10, 3)
        new = state["beta"][b].copy()
        new[act] = (state["beta"][b].astype(np.float64) + dbeta[i].reshape(30)).astype(F32)[act]
        beta[:, :, t] = new.reshape(10, 3)
    return {"accept": accepted, "dbeta": dbeta, "system": systems, "folded": folded}


def fit_gn_jac(A, C, beta, sz, times, frames, iters, jacobian, order="quadratic", damping=1e-3, nchan=1, trace=None):
    """The loop of update_motion(solver='gn') with ``model.motion_jacobian = jacobian`` and no temporal prior, one stage of
    ``order``: ``iters`` pairs normal_eqs -> lm_step and one more normal_eqs with an accept-only step.  m_j = jacobian * prod(sz) *
    nchan.  Returns (beta (10,3,T) fp32, state, F per frame after every step: accepted sse + J).  ``trace``: a list that receives
    every call's result dict."""
    beta = np.array(beta, dtype=F32)
    times = list(times)
    mj = float(jacobian) * int(np.prod(sz)) * nchan
    S = GN.recon_images(A, C, times)
    state, hist = new_state(len(times)), []
    for it in range(iters + 1):
        H, g, sse = GN.normal_eqs(None, None, beta, sz, times, frames, S=S)
        out = lm_step(state, H, g, sse, beta, times, sz, order, lam0=damping, accept_only=it == iters, mj=mj)
        if trace is not None:
            trace.append(out)
        hist.append(state["sse"] + state["jac"])
    return beta, state, hist


def scaled_problem(sz, s, T=3, seed=0):
    """A planted warp that does NOT preserve volume: ``GN.fit_problem(sz, T=T, seed=seed)``'s warps followed by an in-plane
    dilation by ``s`` about the centre of the volume (det Jx ~ s^2), the frames rendered again by the oracle forward."""
    from oracle import dnmf_oracle as orc
    sz = [int(n) for n in sz]
    p = GN.fit_problem(sz, T=T, seed=seed)
    beta = p["beta_true"].astype(np.float64)
    for d in range(2):
        c = (sz[d] - 1) / 2.0
        beta[:, d] *= s
        beta[0, d] += (1.0 - s) * c
    p["beta_true"] = beta.astype(F32)
    basis = orc.quadratic_basis(orc.voxel_lattice(sz))
    p["frames"] = orc.forward(p["A"], basis, p["beta_true"], sz, list(range(T)), p["C"])[0].astype(F32)
    return p


def min_det(beta, sz):
    """Per frame, the smallest det Jx over the sample points of the map beta[:, :, t]."""
    return np.array([np.min(residuals(full_theta(beta[:, :, t], sz), sz)[1]) for t in range(beta.shape[2])])
