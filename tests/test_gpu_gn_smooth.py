"""The temporal smoothness prior of the Gauss-Newton motion solver on the GPU (K16s): dnmf_lm_step_smooth against
tests/gn_smooth_restatement.py on the same inputs, motion_smooth = 0 against the existing path, and update_motion(solver='gn')
with model.motion_smooth set on the dark-frame problem from every loader.

Tolerances of the step (everything the prior adds is float64):
  beta    as tests/test_gpu_gn.py: the device writes fp32(beta_acc + d beta); against fp32 of the restatement's float64 sum it may
          differ by 100 kappa 2.2e-16 max|d beta| (kappa: condition number of the damped scaled system H', g') plus one fp32 rounding
  prior   m sum_s sum_i d_i^2, d = theta - theta_s, in another order; theta = Minv beta is 10 products per entry, so a difference
          d_i carries an error delta_i <= 50 x 2.2e-16 x mag_i, mag = |Minv| |beta| + |Minv| |beta_s| (>= |d_i|, which also covers the
          rounding of the sum), and (d + delta)^2 - d^2 = 2 d delta + delta^2:  tol = m sum_s sum_i (2 |d_i| delta_i + delta_i^2)
  accept flags, lam, counts, the accepted coefficients and sse, beta_ref: exact
"""
import numpy as np
import pytest
import torch

import gn_restatement as GN
import gn_smooth_restatement as GS
from oracle import dnmf_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(24, 20, 1), (24, 20, 2)]
T, DARK, ITERS, SMOOTH = 7, 3, 8, 1e-4


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd.Demix import dNMF
    return dNMF


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


# ---- one step --------------------------------------------------------------------------------------------------------
def spd(sz, B, seed):
    rng = np.random.default_rng(seed)
    J = rng.normal(size=(B, 60, 30)) * rng.uniform(0.1, 10, (1, 1, 30))
    H, g = np.einsum("bpi,bpj->bij", J, J), rng.normal(size=(B, 30))
    off = np.setdiff1d(np.arange(30), GN.active(sz))
    H[:, off], H[:, :, off], g[:, off] = 0, 0, 0
    return H, g


@pytest.mark.parametrize("sz", SHAPES)
def test_step_against_the_restatement(M, sz):
    """T = 11, one launch of the frames 6, 0, 2, 4, 8, 10 (pairwise non-adjacent, not sorted); column 3 of beta_ref holds a NaN.
      frame 6: H = 0 (dark), two neighbours      frames 0 and 10 = T - 1: the end frames, one neighbour      frame 8: two
      neighbours      frames 2 and 4: one neighbour each beside the NaN column
    Four calls: the first (accepts), one whose sse is chosen so that the PRIOR decides frame 0 and 6 (sse alone would say
    otherwise or tie), NaN rejects frame 2, frame 4 rejects on sse and frames 8 and 10 accept on it; a third with fresh H, g; an
    accept-only one.  After each call the restatement continues from the device's fp32 trial, so both sides always step from
    the same input."""
    from dnmf_amd import ops
    Tn, times = 11, [6, 0, 2, 4, 8, 10]
    B, n = len(times), int(np.prod(sz))
    smooth = 2.0 ** -7
    m = smooth * n                                                       # 3.75 / 7.5, exact
    rng = np.random.default_rng(11)
    Mc = GN.change_of_basis(sz)

    def noise(scale):
        """Coefficients whose theta is N(0, scale^2) voxels."""
        return np.einsum("ac,cdt->adt", Mc, rng.normal(size=(10, 3, Tn)) * scale)

    beta0 = (O.identity_beta(Tn) + noise(1e-2)).astype(np.float32)
    ref0 = (beta0 + noise(3e-3)).astype(np.float32)
    ref0[:, :, times] = beta0[:, :, times]
    ref0[5, 0, 3] = np.nan
    Ha, ga = spd(sz, B, 1)
    Hb, gb = spd(sz, B, 2)
    Ha[0], ga[0], Hb[0], gb[0] = 0.0, 0.0, 0.0, 0.0
    Minv_abs = np.abs(GS.basis_inverse(sz))
    act = GN.active(sz)

    ref_beta, ref_ref, ref = beta0.copy(), ref0.copy(), GS.new_state(B)
    beta, bref, st = dev(ref_beta), dev(ref_ref), ops.lm_state(B, "cuda")
    tt = torch.tensor(times, dtype=torch.int32, device="cuda")

    def priors():
        """(p_acc, p_trial) of every frame against the restatement's current beta_ref."""
        out = []
        for b, t in enumerate(times):
            ths = [GS.theta(ref_ref[:, :, s], sz) for s in GS.neighbours(t, ref_ref)]
            out.append((GS.prior(GS.theta(ref["beta"][b], sz), ths, m), GS.prior(GS.theta(ref_beta[:, :, t], sz), ths, m)))
        return np.array(out)

    sse1 = np.array([1.0, 5.0, 6.0, 7.0, 8.0, 9.0])
    plan = [(Ha, ga, lambda: sse1, False),
            (Hb, gb, lambda: np.array([1.0, 5.0 + 0.5 * (priors()[1, 0] - priors()[1, 1]), np.nan, 7.5, 4.0, 4.5]), False),
            (Ha, gb, lambda: ref["sse"] + np.array([0.0, -0.5, -0.5, 1.0, 2.0, -0.5]) - 0.5 * (priors()[:, 1] - priors()[:, 0]), False),
            (Hb, ga, lambda: ref["sse"] + np.array([0.0, 1.0, -1.0, -1.0, 1.0, -1.0]), True)]
    decisions = []
    for call, (H, g, make_sse, last) in enumerate(plan):
        sse = np.asarray(make_sse(), dtype=np.float64)
        before = priors()
        plain_accept = np.isfinite(sse) & (sse < ref["sse"])
        out = GS.lm_step_smooth(ref, H, g, sse, ref_beta, ref_ref, times, sz, m, accept_only=last)
        ops.lm_step(st, {"H": dev(H, torch.float64), "g": dev(g, torch.float64), "sse": dev(sse, torch.float64)}, sz, beta, tt,
                    accept_only=last, smooth=smooth, n_residuals=n, beta_ref=bref)
        got, got_ref = beta.cpu().numpy(), bref.cpu().numpy()
        decisions.append(out["accept"].tolist())
        np.testing.assert_array_equal(st["counts"].cpu().numpy(), ref["counts"])          # identical decisions
        np.testing.assert_array_equal(st["lam"].cpu().numpy(), ref["lam"])
        np.testing.assert_array_equal(st["beta"].cpu().numpy(), ref["beta"])
        np.testing.assert_array_equal(st["sse"].cpu().numpy(), ref["sse"])
        np.testing.assert_array_equal(st["sse0"].cpu().numpy(), ref["sse0"])
        np.testing.assert_array_equal(got_ref, ref_ref)                                    # NaN column included
        prior = st["prior"].cpu().numpy()
        for b, t in enumerate(times):
            nb = GS.neighbours(t, ref_ref)
            mag = Minv_abs @ np.abs(ref["beta"][b].reshape(10, 3).astype(np.float64))
            th_acc, tol_p = GS.theta(ref["beta"][b], sz), 0.0
            for s in nb:
                delta = 50 * 2.2e-16 * (mag + Minv_abs @ np.abs(ref_ref[:, :, s].astype(np.float64))).reshape(30)[act]
                d = np.abs(th_acc - GS.theta(ref_ref[:, :, s], sz))[act]
                tol_p += m * float((2 * d * delta + delta ** 2).sum())
            print(f"call {call} frame {t}: prior {prior[b]:.17g} want {ref['prior'][b]:.17g} diff {abs(prior[b] - ref['prior'][b]):.3g} "
                  f"tol {tol_p:.3g}")
            assert abs(prior[b] - ref["prior"][b]) <= tol_p, (call, b, prior[b], ref["prior"][b], tol_p)
            assert len(nb) == (2 if t in (6, 8) else 1)
            Hp, gp = out["system"][b]
            Ah, _, _ = GN.damped_system(Hp, gp, ref["lam"][b], sz)
            kappa = np.linalg.cond(Ah)
            tol = 100 * kappa * 2.2e-16 * np.abs(out["dbeta"][b]).max() + 6e-8 * np.abs(ref_beta[:, :, t])
            err = np.abs(got[:, :, t].astype(np.float64) - ref_beta[:, :, t])
            assert (err <= tol).all(), (call, b, kappa, err.max())
            if sz[2] == 1 and not last:                                                    # the z unknowns: exact zeros in d beta
                off = np.setdiff1d(np.arange(30), act)
                np.testing.assert_array_equal(got[:, :, t].reshape(30)[off], ref["beta"][b][off])
        untouched = [t for t in range(Tn) if t not in times]
        np.testing.assert_array_equal(got[:, :, untouched], beta0[:, :, untouched])
        np.testing.assert_array_equal(got_ref[:, :, untouched], ref0[:, :, untouched])
        if call == 1:
            # the prior decided: row 0 (frame 6, dark) ties on sse (plain rule: reject) and steps towards its neighbours' mean;
            # row 1's (frame 0) sse rose by half of what its prior fell (or fell by half of what it rose)
            assert not plain_accept[0] and out["accept"][0] and before[0, 1] < before[0, 0]
            assert plain_accept[1] != out["accept"][1]
            assert out["accept"].tolist()[2:] == [False, False, True, True]
        ref_beta[:, :, times] = got[:, :, times]                                           # the same fp32 trial on both sides
    assert decisions[0] == [True] * B and any(decisions[2]) and not all(decisions[2])
    assert np.isfinite(beta.cpu().numpy()[:, :, times]).all() and (ref["prior"] > 0).all()
    # the dark frame moved, as far as the damped mean of its neighbours says
    assert np.abs(ref["beta"][0] - beta0[:, :, 6].reshape(30)).max() > 1e-4


# ---- the fit ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problems():
    """Per shape: the dark-frame problem and the restatement's per-frame errors with the prior (computed once)."""
    out = {}
    for sz in SHAPES:
        p = GS.dark_frame_problem(sz, T=T, dark=DARK)
        beta = GS.fit_gn_smooth(p["A"], p["C"], O.identity_beta(T), sz, range(T), p["frames"], ITERS, SMOOTH)[0]
        p["want"] = GS.frame_errors(beta, p["beta_true"], sz)
        out[sz] = p
    return out


def make_model(M, sz, p, cls=None, **kw):
    K, Tn = p["C"].shape
    model = (cls or M.DeformableNMF)(torch.tensor(sz), K, Tn, positions=torch.from_numpy(p["pos"]), **kw)
    model.fp.A = dev(p["A"])
    model.C = dev(p["C"])
    model.verbose = False
    assert model.motion_smooth == 0.0                                   # the default: no prior
    return model


def resident(M, sz, frames, batch=2):
    return M.ResidentLoader(dev(frames.reshape(frames.shape[0], -1)), sz, batch)


def objective(st, beta, sz, m, key):
    return float(st[key].sum()) + m * GS.roughness(beta, sz)


def check_fit(model, p, sz, nchan=1):
    """The host test's thresholds, and F(result) <= F(start); returns the per-frame errors."""
    beta = model.fp.beta.detach().cpu().numpy()
    err = GS.frame_errors(beta, p["beta_true"], sz)
    msg = f"{sz}: GPU per-frame error {np.round(err, 4).tolist()}, restatement {np.round(p['want'], 4).tolist()}"
    print("\n" + msg)
    assert err[DARK] < 0.1 and err.max() < 0.1, msg
    st = {k: v.cpu().numpy() for k, v in model.last_motion_gn.items()}
    m = SMOOTH * int(np.prod(sz)) * nchan
    assert objective(st, beta, sz, m, "sse") <= objective(st, O.identity_beta(T), sz, m, "sse0"), msg
    assert st["prior"].shape == (T,) and np.isfinite(st["prior"]).all() and (st["prior"] > 0).all()
    return err


@pytest.mark.parametrize("sz", SHAPES)
def test_dark_frame_end_to_end(M, problems, monkeypatch, sz):
    from dnmf_amd import ops
    p = problems[sz]
    plain = make_model(M, sz, p)
    plain.update_motion(resident(M, sz, p["frames"]), None, solver='gn', iters=ITERS)
    e0 = GS.frame_errors(plain.fp.beta.detach().cpu().numpy(), p["beta_true"], sz)
    assert e0[DARK] > 0.3, e0                                             # without the prior the dark frame keeps its start
    calls, real = [], ops.lm_step

    def spy(state, eqs, szl, beta, times, **kw):
        calls.append((times.tolist(), kw["beta_ref"].data_ptr() != beta.data_ptr()))
        return real(state, eqs, szl, beta, times, **kw)

    monkeypatch.setattr(ops, "lm_step", spy)
    model = make_model(M, sz, p)
    model.motion_smooth = SMOOTH
    grad_before = model.fp.beta.grad
    model.update_motion(resident(M, sz, p["frames"]), None, solver='gn', iters=ITERS)
    check_fit(model, p, sz)
    assert calls == [([0, 2, 4, 6], True), ([1, 3, 5], True)] * (ITERS + 1)     # even frames, then odd ones, every iteration
    assert model.fp.beta.requires_grad and model.fp.beta.grad is grad_before


def test_smooth_zero_is_the_existing_path(M, problems, monkeypatch):
    from dnmf_amd import ops
    sz = (24, 20, 2)
    p = problems[sz]
    calls, real = [], ops.lm_step

    def spy(state, *a, **kw):
        calls.append(kw.get("beta_ref"))
        return real(state, *a, **kw)

    def run(**attrs):
        model = make_model(M, sz, p)
        for k, v in attrs.items():
            setattr(model, k, v)
        model.update_motion(resident(M, sz, p["frames"]), None, solver='gn', iters=ITERS)
        return model.fp.beta.detach().cpu().numpy(), {k: v.cpu().numpy() for k, v in model.last_motion_gn.items()}

    beta_a, st_a = run()
    monkeypatch.setattr(ops, "lm_step", spy)
    beta_b, st_b = run(motion_smooth=0)
    monkeypatch.setattr(ops, "lm_step", real)
    np.testing.assert_array_equal(beta_a, beta_b)
    assert sorted(st_a) == sorted(st_b) == ["accepted", "lam", "rejected", "sse", "sse0"]       # no prior
    for k in st_a:
        np.testing.assert_array_equal(st_a[k], st_b[k])
    assert calls == [None] * (ITERS + 1)                                  # one colour, no beta_ref
    # ops.lm_step: smooth = 0 is dnmf_lm_step, whatever else is passed
    H, g = spd(sz, 3, 4)
    eqs = {"H": dev(H, torch.float64), "g": dev(g, torch.float64), "sse": dev(np.array([3.0, 2.0, 1.0]), torch.float64)}
    outs = []
    for kw in ({}, {"smooth": 0.0, "n_residuals": 7, "beta_ref": dev(O.identity_beta(5))}):
        beta, st = dev(O.identity_beta(5)), ops.lm_state(3, "cuda")
        ops.lm_step(st, eqs, sz, beta, [0, 1, 2], **kw)                   # adjacent frames are fine without the prior
        outs.append((beta.cpu().numpy(), {k: v.cpu().numpy() for k, v in st.items()}))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    assert sorted(outs[0][1]) == sorted(outs[1][1]) and "prior" not in outs[1][1]
    for k in ("H", "g", "sse", "sse0", "lam", "beta", "counts"):
        np.testing.assert_array_equal(outs[0][1][k], outs[1][1][k])


class HostFrames(torch.utils.data.Dataset):
    def __init__(self, frames):
        self.frames = torch.from_numpy(frames)

    def __len__(self):
        return self.frames.shape[0]

    def __getitem__(self, i):
        return self.frames[i], i


def test_fit_from_every_loader_and_chunking(M, problems):
    """Unchunked, a ResidentLoader and a staged stock DataLoader run the same schedule.  motion_chunk = 3 splits the 7 frames
    3 + 3 + 1 -- a boundary between adjacent frames, an odd T -- and so does a loader that cannot be staged and hands over
    [0, 1, 2], [3, 4, 5], [6]: another schedule (its result may differ from the unchunked one), the same thresholds."""
    sz = (24, 20, 2)
    p = problems[sz]

    def fit(loader, **attrs):
        model = make_model(M, sz, p)
        for k, v in attrs.items():
            setattr(model, k, v)
        model.motion_smooth = SMOOTH
        model.update_motion(loader, None, solver='gn', iters=ITERS)
        check_fit(model, p, sz)
        return model.fp.beta.detach().cpu().numpy()

    one = fit(resident(M, sz, p["frames"]))
    staged = fit(torch.utils.data.DataLoader(HostFrames(p["frames"]), batch_size=2, shuffle=True))
    assert GN.field_error(staged, one, sz) <= 1e-3
    chunked = fit(resident(M, sz, p["frames"]), motion_chunk=3)
    batches = [(torch.from_numpy(p["frames"][i:i + 3]), torch.arange(i, min(i + 3, T))) for i in range(0, T, 3)]
    host = fit(batches, stream_loader=False)
    assert GN.field_error(host, chunked, sz) <= 1e-3


def test_frames_not_served_report_nan(M, problems):
    """A loader that serves the frames 0, 1, 2 and 4, 5 of 7: the others keep their coefficients (and are read as neighbours at
    them), and last_motion_gn holds NaN / 0 for them, prior included."""
    sz = (24, 20, 1)
    p = problems[sz]
    model = make_model(M, sz, p)
    model.motion_smooth, model.stream_loader = SMOOTH, False
    batches = [(torch.from_numpy(p["frames"][b]), torch.tensor(b)) for b in ([0, 1, 2], [4, 5])]
    model.update_motion(batches, None, solver='gn', iters=2)
    st = {k: v.cpu().numpy() for k, v in model.last_motion_gn.items()}
    served, rest = [0, 1, 2, 4, 5], [3, 6]
    for k in ("prior", "sse", "sse0", "lam"):
        assert np.isnan(st[k][rest]).all() and np.isfinite(st[k][served]).all(), k
    assert not st["accepted"][rest].any() and not st["rejected"][rest].any() and st["accepted"][served].all()
    assert (st["prior"][served] > 0).all() and (st["sse"][served] < st["sse0"][served]).all()
    beta = model.fp.beta.detach().cpu().numpy()
    np.testing.assert_array_equal(beta[:, :, rest], O.identity_beta(T)[:, :, rest])
    assert np.isfinite(beta).all()


def test_fit_multichannel_counts_every_channel(M, problems):
    """Two identical channels (colours 1): H, g, sse and n all double, so F doubles and the fit is the one-channel fit."""
    sz = (24, 20, 1)
    p = problems[sz]
    K = p["C"].shape[0]
    one = make_model(M, sz, p)
    two = make_model(M, sz, p, cls=M.MultiChannelDNMF, colours=np.ones((2, K), np.float32))
    one.motion_smooth = two.motion_smooth = SMOOTH
    one.update_motion(resident(M, sz, p["frames"]), None, solver='gn', iters=ITERS)
    two.update_motion(resident(M, sz, np.stack([p["frames"], p["frames"]], 1)), None, solver='gn', iters=ITERS)
    check_fit(two, p, sz, nchan=2)
    assert GN.field_error(two.fp.beta.detach().cpu().numpy(), one.fp.beta.detach().cpu().numpy(), sz) <= 1e-3
    np.testing.assert_allclose(two.last_motion_gn["prior"].cpu().numpy(), 2 * one.last_motion_gn["prior"].cpu().numpy(), rtol=1e-3)


def test_refused_arguments(M, problems):
    from dnmf_amd import ops
    sz = (24, 20, 1)
    p = problems[sz]
    model = make_model(M, sz, p)
    start = model.fp.beta.detach().clone()
    loader = resident(M, sz, p["frames"])
    opt = torch.optim.Adam([model.fp.beta], lr=1e-3)
    model.motion_smooth = 1e-4
    with pytest.raises(ValueError, match="'gn' only"):
        model.update_motion(loader, opt, solver='adam', epochs=1)
    with pytest.raises(ValueError, match="'gn' only"):
        model.fit(loader, loader, opt, 2, outer=1)                      # the attribute counts in fit as well
    model.motion_smooth = -1e-4
    with pytest.raises(ValueError, match="motion_smooth"):
        model.update_motion(loader, None, solver='gn', iters=1)
    model.motion_smooth = 0.0
    with pytest.raises(ValueError, match="motion_smooth"):
        model.fit(loader, loader, None, 2, outer=1, motion_solver='adam', motion_smooth=1e-4)
    with pytest.raises(ValueError, match="motion_smooth"):
        model.fit(loader, loader, None, 2, outer=1, motion_solver='gn', motion_smooth=float("nan"))
    assert torch.equal(model.fp.beta.detach(), start) and model.motion_smooth == 0.0
    H, g = spd(sz, 2, 4)
    eqs = {"H": dev(H, torch.float64), "g": dev(g, torch.float64), "sse": dev(np.array([3.0, 2.0]), torch.float64)}
    beta, bref = dev(O.identity_beta(5)), dev(O.identity_beta(5))
    with pytest.raises(ValueError, match="non-adjacent"):
        ops.lm_step(ops.lm_state(2, "cuda"), eqs, sz, beta, [3, 2], smooth=1e-4, beta_ref=bref)
    with pytest.raises(ValueError, match="beta_ref"):
        ops.lm_step(ops.lm_state(2, "cuda"), eqs, sz, beta, [0, 2], smooth=1e-4)
    with pytest.raises(ValueError, match="beta_ref"):
        ops.lm_step(ops.lm_state(2, "cuda"), eqs, sz, beta, [0, 2], smooth=1e-4, beta_ref=beta)
    np.testing.assert_array_equal(beta.cpu().numpy(), O.identity_beta(5))
    ops.lm_step(ops.lm_state(2, "cuda"), eqs, sz, beta, [0, 2], smooth=1e-4, beta_ref=bref)           # accepted as given
    assert not np.array_equal(beta.cpu().numpy(), O.identity_beta(5))
