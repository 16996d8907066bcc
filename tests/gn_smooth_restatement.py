"""Float64 definition of the temporal smoothness prior of the Gauss-Newton motion solver (K16s: ``dnmf_lm_step_smooth`` and
the red-black loop ``update_motion(solver='gn', smooth=...)`` runs; include/dnmf_hip.h).  numpy only, on top of
tests/gn_restatement.py.

theta_t (30, index a*3 + d) are frame t's coefficients in K16's centred basis on the active unknowns (all 30; the 12 without z
at Z = 1): beta[:, :, t] = M theta_t per coordinate.  With n residuals per frame and m = smooth * n the objective is
  F(beta) = sum_t sse_t(beta_t) + m sum_t |theta_t - theta_{t+1}|^2
and it is lowered by red-black block coordinate descent: the frames of one parity of t take an evaluate + step while their
neighbours t +- 1 are read, fixed, from ``beta_ref`` -- every frame's ACCEPTED coefficients."""
import numpy as np

import gn_restatement as GN

F32 = np.float32


def basis_inverse(sz):
    """Minv (10,10): the inverse of ``change_of_basis`` on the active monomials, zeros elsewhere (M itself is singular at
    Z = 1)."""
    M = GN.change_of_basis(sz)
    rows = sorted({int(i) // 3 for i in GN.active(sz)})
    Minv = np.zeros((10, 10))
    Minv[np.ix_(rows, rows)] = np.linalg.inv(M[np.ix_(rows, rows)])
    return Minv


def theta(beta_t, sz):
    """(10,3) coefficients beta (fp32 values) -> theta (30,) float64; exact zeros on the inactive unknowns."""
    th = (basis_inverse(sz) @ np.asarray(beta_t, dtype=np.float64).reshape(10, 3)).reshape(30)
    out = np.zeros(30)
    act = GN.active(sz)
    out[act] = th[act]
    return out


def neighbours(t, beta_ref):
    """The frames t +- 1 inside [0, T) whose column of beta_ref is finite."""
    T = beta_ref.shape[2]
    return [s for s in (t - 1, t + 1) if 0 <= s < T and np.isfinite(beta_ref[:, :, s]).all()]


def prior(th, ths, m):
    """m sum_s |theta - theta_s|^2 (0.0 without a neighbour)."""
    return float(m * sum(((th - ts) ** 2).sum() for ts in ths)) if ths else 0.0


def new_state(B):
    st = GN.new_state(B)
    st["prior"] = np.zeros(B)
    return st


def lm_step_smooth(state, H, g, sse, beta, beta_ref, times, sz, m, nu=10.0, lam0=1e-3, lam_min=1e-9, lam_max=1e9,
                   accept_only=False, rows=None):
    """dnmf_lm_step_smooth on numpy arrays.  As ``gn_restatement.lm_step`` with the prior m sum_{s in N_t} |theta - theta_s|^2
    added to both sides of the accept test and to the step system; ``beta_ref`` (10,3,T) fp32 is read at t +- 1 and receives
    the trial's column on accept.  ``times`` must be pairwise non-adjacent.  ``rows``: the rows of ``state`` the frames use
    (default 0..B-1).  Returns dict(accept (B) bool, dbeta (B,10,3), system (B) of (H', g') the step was solved for)."""
    M = GN.change_of_basis(sz)
    act = GN.active(sz)
    B = len(times)
    rows = list(range(B)) if rows is None else list(rows)
    accepted, dbeta, systems = np.zeros(B, bool), np.zeros((B, 10, 3)), []
    for i, t in enumerate(times):
        b = rows[i]
        ths = [theta(beta_ref[:, :, s], sz) for s in neighbours(t, beta_ref)] if m != 0 else []
        first = state["counts"][b, 2] == 0
        th_trial = theta(beta[:, :, t], sz)
        th_acc = theta(state["beta"][b], sz)
        p_trial, p_acc = prior(th_trial, ths, m), prior(th_acc, ths, m)
        with np.errstate(all="ignore"):
            f_trial, f_acc = sse[i] + p_trial, state["sse"][b] + p_acc
        acc = bool(first or (np.isfinite(f_trial) and f_trial < f_acc))
        if first:
            state["lam"][b], state["sse0"][b], state["counts"][b, 2] = lam0, sse[i], 1
        else:
            state["lam"][b] = max(state["lam"][b] / nu, lam_min) if acc else min(state["lam"][b] * nu, lam_max)
            state["counts"][b, 0 if acc else 1] += 1
        if acc:
            state["H"][b], state["g"][b], state["sse"][b] = H[i], g[i], sse[i]
            state["beta"][b] = beta[:, :, t].reshape(30)
            beta_ref[:, :, t] = beta[:, :, t]
            th_acc = th_trial
        state["prior"][b] = p_trial if acc else p_acc
        accepted[i] = acc
        Hp, gp = state["H"][b].copy(), state["g"][b].copy()
        if ths:
            Hp[act, act] += m * len(ths)
            gp[act] += (m * sum(th_acc - ts for ts in ths))[act]
        systems.append((Hp, gp))
        if accept_only:
            beta[:, :, t] = state["beta"][b].reshape(10, 3)
            continue
        delta = np.zeros(30)
        with np.errstate(all="ignore"):
            Ah, rh, sc = GN.damped_system(Hp, gp, state["lam"][b], sz)
        try:
            with np.errstate(all="ignore"):
                if not np.isfinite(Ah).all():
                    raise np.linalg.LinAlgError
                L = np.linalg.cholesky(Ah)
                delta[act] = sc * np.linalg.solve(L.T, np.linalg.solve(L, rh))
        except np.linalg.LinAlgError:
            pass
        dbeta[i] = M @ delta.reshape(10, 3)
        beta[:, :, t] = (state["beta"][b].reshape(10, 3).astype(np.float64) + dbeta[i]).astype(F32)
    return {"accept": accepted, "dbeta": dbeta, "system": systems}


def roughness(beta, sz):
    """sum_t |theta_t - theta_{t+1}|^2 over the adjacent pairs of finite columns of beta (10,3,T)."""
    T = beta.shape[2]
    fin = [np.isfinite(beta[:, :, t]).all() for t in range(T)]
    th = [theta(beta[:, :, t], sz) if fin[t] else None for t in range(T)]
    return float(sum(((th[t] - th[t + 1]) ** 2).sum() for t in range(T - 1) if fin[t] and fin[t + 1]))


def fit_gn_smooth(A, C, beta, sz, times, frames, iters, smooth, damping=1e-3, chunk=None, nchan=1):
    """The loop of update_motion(solver='gn', smooth=smooth) for the frames ``times`` (frames[b] belongs to times[b]):
    beta_ref = beta at entry; per chunk of ``chunk`` frames (default: all), ``iters`` + 1 iterations (the last accept-only) of
    [evaluate + step on the chunk's frames of even t, then on those of odd t].  m = smooth * n with n = prod(sz) * nchan.
    Returns (beta (10,3,T) fp32, state, F after every step): F = sum of the accepted sse (a frame not yet evaluated counts
    with its sse at entry) + m * roughness of beta_ref."""
    beta = np.array(beta, dtype=F32)
    beta_ref = beta.copy()
    times = [int(t) for t in times]
    B = len(times)
    m = float(smooth) * int(np.prod(sz)) * nchan
    S = GN.recon_images(A, C, times)
    state, hist = new_state(B), []
    sse_entry = GN.normal_eqs(None, None, beta, sz, times, frames, S=S)[2]
    chunk = B if chunk is None else int(chunk)
    for s0 in range(0, B, chunk):
        part = list(range(s0, min(B, s0 + chunk)))
        for it in range(iters + 1):
            for colour in (0, 1):
                sel = [b for b in part if times[b] % 2 == colour]
                if not sel:
                    continue
                tt = [times[b] for b in sel]
                H, g, sse = GN.normal_eqs(None, None, beta, sz, tt, frames[sel], S=S[sel])
                lm_step_smooth(state, H, g, sse, beta, beta_ref, tt, sz, m, lam0=damping, accept_only=it == iters, rows=sel)
                data = np.where(state["counts"][:, 2] == 1, state["sse"], sse_entry)
                hist.append(float(data.sum() + m * roughness(beta_ref, sz)))
    return beta, state, hist


def dark_frame_problem(sz, T=7, dark=3):
    """The issue's problem: beta* interpolated linearly in t between fit_problem(sz, T=2)'s two warps, the traces of frame
    ``dark`` all zero, frames = the oracle forward at beta*.  Returns dict(A, C, beta_true, frames (T,X,Y,Z) fp32, pos)."""
    from oracle import dnmf_oracle as orc
    p2 = GN.fit_problem(sz, T=2)
    w = np.linspace(0.0, 1.0, T)
    b0, b1 = p2["beta_true"][:, :, 0].astype(np.float64), p2["beta_true"][:, :, 1].astype(np.float64)
    beta = (b0[:, :, None] * (1 - w) + b1[:, :, None] * w).astype(F32)
    K = p2["A"].shape[-1]
    C = np.random.default_rng(1).uniform(0.5, 1.5, (K, T)).astype(F32)
    C[:, dark] = 0.0
    basis = orc.quadratic_basis(orc.voxel_lattice(sz))
    frames = orc.forward(p2["A"], basis, beta, [int(s) for s in sz], list(range(T)), C)[0].astype(F32)
    return {"A": p2["A"], "C": C, "beta_true": beta, "frames": frames, "pos": p2["pos"]}


def frame_errors(beta, beta_true, sz):
    """``field_error`` frame by frame."""
    return np.array([GN.field_error(beta[:, :, t:t + 1], beta_true[:, :, t:t + 1], sz) for t in range(beta.shape[2])])
