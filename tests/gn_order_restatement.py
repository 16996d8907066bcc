"""Float64 definition of the Gauss-Newton motion step for one warp order (K16o: ``dnmf_lm_step_order``) and of the staged loop
``update_motion(solver='gn')`` runs when ``model.motion_order`` is set (include/dnmf_hip.h).  numpy only, on top of
tests/gn_restatement.py and tests/gn_smooth_restatement.py.

The unknowns of an order are the rows of K16's centred basis of degree <= order -- translation: row 0, affine: rows 0 .. 3,
quadratic: all ten -- without the z rows and the z component at Z == 1.  K16's H and g are taken whole and restricted here."""
import numpy as np

import gn_restatement as GN
import gn_smooth_restatement as GS

F32 = np.float32
ORDERS = {"translation": 0, "affine": 1, "quadratic": 2}
GRADED = ("translation", "affine", "quadratic")


def active(sz, order):
    """Parameter indices a*3+d of the unknowns of ``order``: those of ``GN.active(sz)`` whose basis term has degree <= order.
    3, 12 or 30 of them; 2, 6 or 12 at Z == 1."""
    return np.array([i for i in GN.active(sz) if GN.EXPO[i // 3].sum() <= ORDERS[order]])


def theta(beta_t, sz, order):
    """``GS.theta`` with exact zeros outside the unknowns of ``order``."""
    out = np.zeros(30)
    act = active(sz, order)
    out[act] = GS.theta(beta_t, sz)[act]
    return out


def damped_system(H, g, lam, act):
    """``GN.damped_system`` on the unknowns ``act``: the diagonal scaling and tiny come from that block's own diagonal."""
    Ha = H[np.ix_(act, act)]
    dg = np.diag(Ha)
    tiny = 1e-12 * dg.max() + 1e-30
    Ad = Ha + np.diag(lam * dg + tiny)
    sc = 1.0 / np.sqrt(np.diag(Ad))
    return Ad * sc[:, None] * sc[None, :], -g[act] * sc, sc


def lm_step(state, H, g, sse, beta, times, sz, order, nu=10.0, lam0=1e-3, lam_min=1e-9, lam_max=1e9, accept_only=False, m=0.0,
            beta_ref=None, rows=None):
    """dnmf_lm_step_order on numpy arrays: ``GN.lm_step`` (m == 0) or ``GS.lm_step_smooth`` (m != 0: ``beta_ref`` as there, state
    from ``GS.new_state``) over the unknowns of ``order``.  The prior sees theta on those unknowns only; the entries of
    ``beta[:, :, t]`` that are no unknown are not written.  Returns dict(accept (B) bool, dbeta (B,10,3), system (B) of (H', g') the
    step is solved for on ``active(sz, order)``)."""
    M = GN.change_of_basis(sz)
    act = active(sz, order)
    B = len(times)
    rows = list(range(B)) if rows is None else list(rows)
    accepted, dbeta, systems = np.zeros(B, bool), np.zeros((B, 10, 3)), []
    for i, t in enumerate(times):
        b = rows[i]
        ths = [theta(beta_ref[:, :, s], sz, order) for s in GS.neighbours(t, beta_ref)] if m != 0 else []
        first = state["counts"][b, 2] == 0
        th_trial, th_acc = theta(beta[:, :, t], sz, order), theta(state["beta"][b], sz, order)
        p_trial, p_acc = GS.prior(th_trial, ths, m), GS.prior(th_acc, ths, m)
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
            if m != 0:
                beta_ref[:, :, t] = beta[:, :, t]
            th_acc = th_trial
        if m != 0:
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
        try:
            with np.errstate(all="ignore"):
                Ah, rh, sc = damped_system(Hp, gp, state["lam"][b], act)
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
    return {"accept": accepted, "dbeta": dbeta, "system": systems}


def schedule_of(order, iters):
    """The stages ``model.motion_order = order`` runs in a call with ``iters`` iterations: [(order name, iterations), ...]."""
    if order == "graded":
        return [(o, int(iters)) for o in GRADED]
    if isinstance(order, str):
        return [(order, int(iters))]
    return [(o, int(n)) for o, n in order]


def fit_gn_schedule(A, C, beta, sz, times, frames, schedule, damping=1e-3):
    """The staged loop: the reconstruction images once, then per stage (order, iters) a fresh state, ``iters`` pairs normal_eqs ->
    lm_step of that order and one more normal_eqs with an accept-only step, the next stage starting at what that left in beta.
    Returns (beta (10,3,T) fp32, the stages' states, history of state['sse'] after every step of every stage)."""
    beta = np.array(beta, dtype=F32)
    times = list(times)
    S = GN.recon_images(A, C, times)
    states, hist = [], []
    for order, iters in schedule:
        state = GN.new_state(len(times))
        for it in range(iters + 1):
            H, g, sse = GN.normal_eqs(None, None, beta, sz, times, frames, S=S)
            lm_step(state, H, g, sse, beta, times, sz, order, lam0=damping, accept_only=it == iters)
            hist.append(state["sse"].copy())
        states.append(state)
    return beta, states, hist


def shifted_problem(sz, L, seed):
    """A warp a translation away from the full-order basin: ``GN.fit_problem(sz, K=6, T=4, seed=seed, shift=0, affine=0.02,
    quad=0.25)`` plus, per frame, a shift of length ``L`` voxels in the x-y plane in a random direction, the frames rendered
    again by the oracle forward."""
    from oracle import dnmf_oracle as orc
    sz = [int(s) for s in sz]
    p = GN.fit_problem(sz, K=6, T=4, seed=seed, shift=0.0, affine=0.02, quad=0.25)
    rng = np.random.default_rng(seed + 100)
    beta = p["beta_true"].astype(np.float64)
    for t in range(beta.shape[2]):
        ang = rng.uniform(0, 2 * np.pi)
        beta[0, :2, t] += L * np.array([np.cos(ang), np.sin(ang)])
    p["beta_true"] = beta.astype(F32)
    basis = orc.quadratic_basis(orc.voxel_lattice(sz))
    p["frames"] = orc.forward(p["A"], basis, p["beta_true"], sz, list(range(beta.shape[2])), p["C"])[0].astype(F32)
    return p
