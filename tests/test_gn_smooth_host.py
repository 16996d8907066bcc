"""The temporal smoothness prior of the Gauss-Newton motion solver (K16s) without a GPU: the float64 restatement
(tests/gn_smooth_restatement.py) on the dark-frame problem, its descent, its reduction to the unsmoothed fit, its neighbour
handling, and the wiring of every layer."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import gn_restatement as GN
import gn_smooth_restatement as GS
from oracle import dnmf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(24, 20, 1), (24, 20, 2)]
T, DARK, ITERS, SMOOTH = 7, 3, 8, 1e-4


@pytest.fixture(scope="module")
def fits():
    """Per shape: the problem, and the fit from the identity without and with the prior."""
    out = {}
    for sz in SHAPES:
        p = GS.dark_frame_problem(sz, T=T, dark=DARK)
        run = {s: GS.fit_gn_smooth(p["A"], p["C"], O.identity_beta(T), sz, range(T), p["frames"], ITERS, s) for s in (0.0, SMOOTH)}
        out[sz] = (p, run)
    return out


@pytest.mark.parametrize("sz", SHAPES)
def test_dark_frame_is_carried_by_its_neighbours(fits, sz):
    """T = 7, beta* linear in t between fit_problem(sz, T=2)'s two warps, C[:, 3] = 0, identity start, 8 iterations.  Measured:
    frame 3 ends 0.512 (24x20x1) / 0.402 (24x20x2) voxel off without the prior, 0.027 / 0.030 with smooth = 1e-4; the other
    frames <= 0.028 with it."""
    p, run = fits[sz]
    e0 = GS.frame_errors(run[0.0][0], p["beta_true"], sz)
    e1 = GS.frame_errors(run[SMOOTH][0], p["beta_true"], sz)
    print(f"\n{sz}: smooth 0 {np.round(e0, 4)}, smooth {SMOOTH} {np.round(e1, 4)}")
    assert e0[DARK] > 0.3 and np.delete(e0, DARK).max() < 0.01
    assert e1[DARK] < 0.1 and e1.max() < 0.1
    # the dark frame kept its start without the prior: H = g = 0 there
    np.testing.assert_array_equal(run[0.0][0][:, :, DARK], O.identity_beta(T)[:, :, DARK])
    assert not run[0.0][1]["H"][DARK].any()


@pytest.mark.parametrize("sz", SHAPES)
@pytest.mark.parametrize("chunk", [None, 3])
def test_objective_never_increases(fits, sz, chunk):
    p, run = fits[sz]
    hist = run[SMOOTH][2] if chunk is None else GS.fit_gn_smooth(p["A"], p["C"], O.identity_beta(T), sz, range(T), p["frames"],
                                                                ITERS, SMOOTH, chunk=chunk)[2]
    assert len(hist) == (2 if chunk is None else 5) * (ITERS + 1)        # chunks of 3: 2 + 2 + 1 colours
    assert all(b <= a for a, b in zip(hist, hist[1:])), hist
    assert hist[-1] < 1e-2 * hist[0]


@pytest.mark.parametrize("sz", SHAPES)
def test_smooth_zero_is_the_unsmoothed_fit(fits, sz):
    p, run = fits[sz]
    beta, st, _ = run[0.0]
    want, wst, _ = GN.fit_gn(p["A"], p["C"], O.identity_beta(T), sz, range(T), p["frames"], ITERS)
    np.testing.assert_array_equal(beta, want)                            # same bits
    for k in ("counts", "lam", "sse", "sse0", "beta", "H", "g"):
        np.testing.assert_array_equal(st[k], wst[k])
    assert not st["prior"].any()


def step_case(sz, seed=0, Tn=4):
    """Synthetic input of one step: SPD H, random g, coefficients near the identity."""
    rng = np.random.default_rng(seed)
    J = rng.normal(size=(Tn, 60, 30))
    H, g = np.einsum("bpi,bpj->bij", J, J), rng.normal(size=(Tn, 30))
    off = np.setdiff1d(np.arange(30), GN.active(sz))
    H[:, off], H[:, :, off], g[:, off] = 0, 0, 0
    beta = (O.identity_beta(Tn) + rng.normal(size=(10, 3, Tn)) * 1e-2).astype(np.float32)
    return H, g, beta


@pytest.mark.parametrize("sz", [(12, 10, 1), (9, 7, 3)])
def test_end_frames_use_one_neighbour_and_a_nan_neighbour_is_skipped(sz):
    H, g, beta = step_case(sz)
    m, act = 2.5, GN.active(sz)
    ref = beta.copy()
    ref[4, 1, 2] = np.nan                                                # frame 2 is nobody's neighbour
    assert GS.neighbours(0, ref) == [1] and GS.neighbours(3, ref) == [] and GS.neighbours(1, ref) == [0]
    st = GS.new_state(2)
    trial = beta.copy()
    out = GS.lm_step_smooth(st, H[[0, 3]], g[[0, 3]], np.array([5.0, 6.0]), trial, ref, [0, 3], sz, m)
    for i, (t, nn) in enumerate([(0, 1), (3, 0)]):
        Hp, gp = out["system"][i]
        np.testing.assert_array_equal(np.diag(Hp)[act], np.diag(H[t])[act] + m * nn)
        np.testing.assert_array_equal(Hp - np.diag(np.diag(Hp)), H[t] - np.diag(np.diag(H[t])))
    th0, th1 = GS.theta(beta[:, :, 0], sz), GS.theta(beta[:, :, 1], sz)
    np.testing.assert_allclose(out["system"][0][1], g[0] + m * (th0 - th1), rtol=1e-15)
    np.testing.assert_array_equal(out["system"][1][1], g[3])             # no neighbour: the unsmoothed system
    np.testing.assert_allclose(st["prior"], [m * ((th0 - th1) ** 2).sum(), 0.0], rtol=1e-15)
    assert np.isfinite(trial[:, :, [0, 3]]).all() and np.isfinite(out["dbeta"]).all() and np.isfinite(st["prior"]).all()
    # frame 3 without a neighbour took gn_restatement's step, bit for bit
    plain, pst = beta.copy(), GN.new_state(1)
    GN.lm_step(pst, H[[3]], g[[3]], np.array([6.0]), plain, [3], sz)
    np.testing.assert_array_equal(trial[:, :, 3], plain[:, :, 3])
    np.testing.assert_array_equal(ref[:, :, [0, 3]], beta[:, :, [0, 3]])  # accepted columns written, the others untouched
    assert np.isnan(ref[4, 1, 2]) and np.array_equal(ref[:, :, 1], beta[:, :, 1])


def test_accept_test_uses_the_current_neighbours():
    """The accepted sse was stored before the neighbours moved: both priors are recomputed, so a trial with a HIGHER sse is
    accepted when it is that much closer to where the neighbours now are, and rejected without the prior."""
    sz = (9, 7, 3)
    H, g, beta = step_case(sz, Tn=3)
    ref, trial, st = beta.copy(), beta.copy(), GS.new_state(1)
    GS.lm_step_smooth(st, H[[1]], g[[1]], np.array([5.0]), trial, ref, [1], sz, 1.0)
    assert st["counts"].tolist() == [[0, 0, 1]]
    moved = trial[:, :, 1].copy()
    ref[:, :, 0], ref[:, :, 2] = moved, moved                            # the neighbours now sit at the trial
    far = st["prior"][0]
    out = GS.lm_step_smooth(st, H[[1]], g[[1]], np.array([5.0 + 0.5 * GS.prior(GS.theta(beta[:, :, 1], sz), [GS.theta(moved, sz)] * 2, 1.0)]),
                            trial, ref, [1], sz, 1.0)
    assert out["accept"][0] and st["counts"].tolist() == [[1, 0, 1]] and st["prior"][0] == 0.0 and far > 0
    np.testing.assert_array_equal(ref[:, :, 1], moved)
    st2, trial2 = GN.new_state(1), beta.copy()
    GN.lm_step(st2, H[[1]], g[[1]], np.array([5.0]), trial2, [1], sz)
    assert not GN.lm_step(st2, H[[1]], g[[1]], np.array([5.5]), trial2, [1], sz)["accept"][0]


def test_dark_frame_steps_to_the_neighbours_mean():
    sz = (9, 7, 3)
    _, _, beta = step_case(sz, Tn=3)
    ref, trial, st = beta.copy(), beta.copy(), GS.new_state(1)
    lam0 = 1e-3
    out = GS.lm_step_smooth(st, np.zeros((1, 30, 30)), np.zeros((1, 30)), np.array([1.0]), trial, ref, [1], sz, 0.7, lam0=lam0)
    th = [GS.theta(beta[:, :, t], sz) for t in range(3)]
    want = (0.5 * (th[0] + th[2]) - th[1]) / (1.0 + lam0)                # tiny = 1e-12 hmax moves the 13th digit
    got = GS.basis_inverse(sz) @ out["dbeta"][0]
    np.testing.assert_allclose(got.reshape(30), want, rtol=1e-10, atol=1e-14)
    assert np.abs(want).max() > 1e-3


def test_single_frame_has_no_neighbour():
    sz = (24, 20, 1)
    p = GN.fit_problem(sz, T=1)
    got, st, _ = GS.fit_gn_smooth(p["A"], p["C"], O.identity_beta(1), sz, [0], p["frames"], 4, 1e-2)
    want, wst, _ = GN.fit_gn(p["A"], p["C"], O.identity_beta(1), sz, [0], p["frames"], 4)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(st["counts"], wst["counts"])
    assert st["prior"][0] == 0.0


def test_z_unknowns_stay_out_at_one_slice(fits):
    sz = (24, 20, 1)
    off = np.setdiff1d(np.arange(30), GN.active(sz))
    H, g, beta = step_case(sz)
    ref, trial, st = beta.copy(), beta.copy(), GS.new_state(1)
    ref2 = ref.copy()
    ref2.reshape(30, -1)[off] += 7.0                                     # the neighbours' z entries: any value
    a = GS.lm_step_smooth(st, H[[1]], g[[1]], np.array([5.0]), trial, ref, [1], sz, 3.0)
    trial2, st2 = beta.copy(), GS.new_state(1)
    b = GS.lm_step_smooth(st2, H[[1]], g[[1]], np.array([5.0]), trial2, ref2, [1], sz, 3.0)
    np.testing.assert_array_equal(a["dbeta"], b["dbeta"])
    assert st["prior"][0] == st2["prior"][0] > 0
    assert not a["dbeta"].reshape(-1, 30)[:, off].any()                  # exact zeros in d beta
    assert not GS.theta(beta[:, :, 0], sz)[off].any() and beta[3, 2, 0] != 0
    # and in the whole fit: the z entries of beta are the start's, bit for bit
    p, run = fits[sz]
    np.testing.assert_array_equal(run[SMOOTH][0].reshape(30, -1)[off], O.identity_beta(T).reshape(30, -1)[off])


@pytest.mark.parametrize("sz", [(24, 20, 1), (24, 20, 2), (9, 7, 3)])
def test_centred_basis_inverse(sz):
    from dnmf_amd import ops
    M, Minv = ops.centred_basis_matrix(sz), ops.centred_basis_inverse(sz)
    rows = sorted({int(i) // 3 for i in GN.active(sz)})
    off = np.setdiff1d(np.arange(10), rows)
    np.testing.assert_allclose((Minv @ M)[np.ix_(rows, rows)], np.eye(len(rows)), atol=1e-12)
    assert not Minv[off].any() and not Minv[:, off].any()
    np.testing.assert_allclose(Minv, GS.basis_inverse(sz), rtol=1e-12, atol=1e-15)
    # theta is in voxels: the centred constant term of the identity's x coordinate is the middle of the axis
    th = GS.theta(O.identity_beta(1)[:, :, 0], sz)
    assert th[0] == pytest.approx((sz[0] - 1) / 2) and th[1 * 3 + 0] == pytest.approx((sz[0] - 1) / 2)


def test_abi_declares_and_binds_the_entry():
    header = open(os.path.join(ROOT, "include", "dnmf_hip.h")).read()
    assert "tests/gn_smooth_restatement.py" in header and "pairwise non-adjacent" in header
    from dnmf_amd import _lib, build
    res, args = _lib.SIGNATURES["dnmf_lm_step_smooth"]
    assert res is ctypes.c_int and args[17] is ctypes.c_double and args[23] is ctypes.c_double
    plain = _lib.SIGNATURES["dnmf_lm_step"][1]
    assert args[:6] == plain[:6] and args[7:22] == plain[6:21]           # dnmf_lm_step's arguments, Minv after M
    build.build_library()
    lib = _lib.load()
    buf = (ctypes.c_double * 1024)()
    p, q = ctypes.addressof(buf), ctypes.addressof(buf) + 4096
    ok = [p, p, p, 2, 1, p, p, p, 4, p, p, p, p, p, p, p, p, 10.0, 1e-3, 1e-9, 1e9, 0, q, 1.0, p, 0]
    for i in (0, 1, 2, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 22, 24):
        a = list(ok)
        a[i] = 0
        assert lib.dnmf_lm_step_smooth(*a) == -1 and lib.dnmf_last_error().decode().startswith("dnmf_lm_step_smooth:"), i
    for i, v in ((3, 0), (17, 1.0), (18, 0.0), (19, 0.0), (20, 1e-12), (23, -1.0), (23, float("nan")), (22, p)):
        a = list(ok)
        a[i] = v
        assert lib.dnmf_lm_step_smooth(*a) == -2 and lib.dnmf_last_error().decode().startswith("dnmf_lm_step_smooth:"), (i, v)


def test_public_signatures_and_refused_values():
    from dnmf_amd import ops
    from dnmf_amd.Demix import dNMF
    # the weight is the model's attribute motion_smooth; update_motion keeps the parameter list tests/test_gn_host.py pins
    assert "smooth" not in inspect.signature(dNMF.DeformableNMF.update_motion).parameters
    assert "self.motion_smooth = 0.0" in inspect.getsource(dNMF.DeformableNMF.__init__)
    assert inspect.signature(dNMF.DeformableNMF.fit).parameters["motion_smooth"].default is None
    pl = inspect.signature(ops.lm_step).parameters
    assert (pl["smooth"].default, pl["n_residuals"].default, pl["beta_ref"].default) == (0.0, None, None)
    assert dNMF._check_motion_smooth(0, "adam", "x") == 0.0 and dNMF._check_motion_smooth(1e-4, "gn", "x") == 1e-4
    for smooth, solver in ((1e-4, "adam"), (-1e-4, "gn"), (float("nan"), "gn"), (float("inf"), "gn")):
        with pytest.raises(ValueError, match="motion_smooth"):
            dNMF._check_motion_smooth(smooth, solver, "update_motion")
