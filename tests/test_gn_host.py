"""The Gauss-Newton motion solver (K16 + dnmf_lm_step) without a GPU: the float64 restatement (tests/gn_restatement.py) against
the oracle's gradient and against finite differences of its own forward, the step's bookkeeping, the change of basis, and the
wiring of every layer."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import gn_restatement as GN
from oracle import dnmf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_case(sz, seed=3, T=3):
    """K = 4 Gaussians, a warp off the identity whose samples sit on no lattice plane, random frames."""
    rng = np.random.default_rng(seed)
    sz = [int(s) for s in sz]
    pos = np.stack([rng.uniform(0, s - 1, 4) for s in sz], 1).astype(np.float32)
    A = O.gaussian_footprints(sz, pos, np.full(4, 3.0, np.float32))
    C = rng.uniform(0.5, 1.5, (4, T)).astype(np.float32)
    beta = O.identity_beta(T).astype(np.float64)
    beta[0] += rng.uniform(0.2, 0.45, (3, T))
    beta[1:4] += rng.uniform(-0.02, 0.02, (3, 3, T))
    beta[4:] += rng.uniform(-1e-3, 1e-3, (6, 3, T))
    frames = rng.uniform(0, 1, (T, *sz)).astype(np.float32)
    return A, C, beta.astype(np.float32), frames


@pytest.mark.parametrize("sz", [(12, 10, 2), (12, 10, 1)])
def test_gradient_and_loss_are_the_reference_ones(sz):
    A, C, beta, frames = small_case(sz)
    times = [2, 0, 1]
    fr = frames[times]
    basis = O.quadratic_basis(O.voxel_lattice(sz))
    loss, grad = O.mse_beta_grad_autograd(A, basis, beta, sz, times, C, fr)
    H, g, sse = GN.normal_eqs(A, C, beta, sz, times, fr)
    BP = len(times) * int(np.prod(sz))
    np.testing.assert_allclose(sse.sum() / BP, loss, rtol=1e-5)
    for b, t in enumerate(times):
        got = GN.to_raw_grad(g[b], sz) * 2.0 / BP
        np.testing.assert_allclose(got, grad[:, :, t], rtol=0, atol=1e-4 * np.abs(grad).max())
    if sz[2] == 1:   # the unknowns Z = 1 drops
        off = np.setdiff1d(np.arange(30), GN.active(sz))
        assert len(GN.active(sz)) == 12 and not H[:, off].any() and not H[:, :, off].any() and not g[:, off].any()


@pytest.mark.parametrize("sz", [(12, 10, 2), (12, 10, 1)])
def test_H_is_JtJ_of_the_forward(sz):
    """J column by column from central differences (step 1e-6) of the restatement's own forward in float64, in the centred
    basis: beta + M e_i h."""
    A, C, beta, frames = small_case(sz, T=1)
    S = GN.recon_images(A, C, [0])
    M = GN.change_of_basis(sz)
    b0 = beta[:, :, 0].astype(np.float64)
    h = 1e-6
    J = np.zeros((int(np.prod(sz)), 30))
    for i in GN.active(sz):
        e = np.zeros(30)
        e[i] = h
        db = M @ e.reshape(10, 3)
        rp, _ = GN.residual(S[0], b0 + db, sz, frames[0], exact=True)
        rm, _ = GN.residual(S[0], b0 - db, sz, frames[0], exact=True)
        J[:, i] = ((rp - rm) / (2 * h)).ravel()
    # the restatement at the same float64 coordinates
    r, dq = GN.residual(S[0], b0, sz, frames[0], exact=True)
    phi = GN.basis64(GN.centred_lattice(sz)).reshape(-1, 10)
    Jr = (phi[:, :, None] * dq.reshape(3, -1).T[:, None, :]).reshape(-1, 30)
    Hr, Hd = Jr.T @ Jr, J.T @ J
    act = GN.active(sz)
    scale = np.sqrt(np.outer(np.diag(Hr), np.diag(Hr)))[np.ix_(act, act)]
    assert (np.abs(Hr - Hd)[np.ix_(act, act)] <= 1e-5 * scale).all()
    # and normal_eqs (taps from the fp32 op sequence) builds the same matrix from the same formula
    H, g, sse = GN.normal_eqs(A, C, beta, sz, [0], frames[:1])
    assert (np.abs(H[0] - Hr)[np.ix_(act, act)] <= 1e-4 * scale).all()
    np.testing.assert_array_equal(H[0], H[0].T)


def test_change_of_basis_on_a_lattice():
    for sz in [(9, 7, 3), (9, 7, 1)]:
        M = GN.change_of_basis(sz)
        rng = np.random.default_rng(0)
        gamma = rng.normal(size=(10, 3))
        lhs = GN.basis64(GN.centred_lattice(sz)) @ gamma
        rhs = GN.basis64(O.voxel_lattice(sz)) @ (M @ gamma)
        assert np.abs(lhs - rhs).max() <= 1e-12
        from dnmf_amd import ops
        np.testing.assert_allclose(ops.centred_basis_matrix(sz), M, rtol=0, atol=1e-15)


def test_lm_step_bookkeeping():
    """A hand-made two-frame state: first call accepts, a lower sse accepts and relaxes the damping, a higher or NaN sse
    rejects, tightens it and steps again from the accepted point."""
    sz = (9, 7, 3)
    rng = np.random.default_rng(1)
    J = rng.normal(size=(2, 50, 30))
    H = np.einsum("bpi,bpj->bij", J, J)
    g = rng.normal(size=(2, 30))
    beta = O.identity_beta(4)
    times = [3, 1]
    st = GN.new_state(2)
    out = GN.lm_step(st, H, g, np.array([5.0, 7.0]), beta, times, sz)
    assert out["accept"].all() and (st["lam"] == 1e-3).all() and (st["counts"] == [[0, 0, 1], [0, 0, 1]]).all()
    np.testing.assert_array_equal(st["sse0"], [5.0, 7.0])
    trial1 = beta.copy()
    assert (trial1[:, :, times] != O.identity_beta(4)[:, :, times]).any()
    np.testing.assert_array_equal(trial1[:, :, [0, 2]], O.identity_beta(4)[:, :, [0, 2]])   # other frames untouched
    # frame 0 improves, frame 1 gets worse
    out = GN.lm_step(st, 2 * H, g, np.array([4.0, 7.5]), beta, times, sz)
    assert out["accept"].tolist() == [True, False]
    np.testing.assert_allclose(st["lam"], [1e-4, 1e-2])
    assert st["counts"].tolist() == [[1, 0, 1], [0, 1, 1]]
    np.testing.assert_array_equal(st["sse"], [4.0, 7.0])
    np.testing.assert_array_equal(st["beta"][0], trial1[:, :, 3].reshape(30))
    np.testing.assert_array_equal(st["beta"][1], O.identity_beta(4)[:, :, 1].reshape(30))
    np.testing.assert_array_equal(st["H"][1], H[1])
    # a NaN sse never accepts; accept_only leaves the accepted coefficients
    out = GN.lm_step(st, H, g, np.array([np.nan, 6.0]), beta, times, sz, accept_only=True)
    assert out["accept"].tolist() == [False, True] and st["counts"].tolist() == [[1, 1, 1], [1, 1, 1]]
    np.testing.assert_array_equal(beta[:, :, 3].reshape(30), st["beta"][0])
    # the damping stays inside its bounds
    for _ in range(14):
        GN.lm_step(st, H, g, np.array([np.nan, np.nan]), beta, times, sz)
    assert (st["lam"] == 1e9).all()


def test_lm_step_zero_H_and_nan_frame():
    sz = (12, 10, 1)
    beta = O.identity_beta(2)
    beta[:, :, 1] = np.nan
    st = GN.new_state(2)
    out = GN.lm_step(st, np.zeros((2, 30, 30)), np.zeros((2, 30)), np.array([0.0, np.nan]), beta, [0, 1], sz)
    assert not out["dbeta"].any()
    np.testing.assert_array_equal(beta[:, :, 0], O.identity_beta(1)[:, :, 0])
    assert np.isnan(beta[:, :, 1]).all()


def test_fit_gn_converges_on_the_test_problems():
    """The problems tests/test_gpu_gn.py fits on the GPU: float64 sums reach 0.01 voxel within 8 iterations."""
    for sz in [(24, 20, 2), (24, 20, 1), (24, 20, 5)]:
        p = GN.fit_problem(sz)
        T = p["C"].shape[1]
        beta, st, hist = GN.fit_gn(p["A"], p["C"], O.identity_beta(T), sz, range(T), p["frames"], iters=8)
        assert GN.field_error(O.identity_beta(T), p["beta_true"], sz) > 0.5     # the start is far off
        assert GN.field_error(beta, p["beta_true"], sz) < 0.01
        assert all((b <= a).all() for a, b in zip(hist, hist[1:]))
        assert (st["sse"] <= 1e-6 * st["sse0"]).all()


def test_abi_declares_and_binds_the_entries():
    assert "tests/gn_restatement.py" in open(os.path.join(ROOT, "include", "dnmf_hip.h")).read()
    from dnmf_amd import _lib, build
    res, args = _lib.SIGNATURES["dnmf_warp_normal_eqs"]
    assert res is ctypes.c_int and args[1] is ctypes.c_long and args[18] is ctypes.c_size_t
    res, args = _lib.SIGNATURES["dnmf_lm_step"]
    assert res is ctypes.c_int and args[16] is ctypes.c_double
    assert _lib.SIGNATURES["dnmf_warp_normal_eqs_workspace"][0] is ctypes.c_size_t
    assert "motion_gn.hip" in build.SOURCES
    build.build_library()
    lib = _lib.load()
    assert hasattr(lib, "dnmf_warp_normal_eqs") and hasattr(lib, "dnmf_lm_step")
    # the workspace holds the x table and one row of sums per block: 58 sums at Z = 1, 241 at Z > 1
    assert lib.dnmf_warp_normal_eqs_workspace(70, 300, 1, 3) == 1280 + 3 * 6 * 58 * 4
    assert lib.dnmf_warp_normal_eqs_workspace(40, 130, 2, 3) == 768 + 3 * 2 * 241 * 4
    assert lib.dnmf_warp_normal_eqs_workspace(0, 1, 1, 1) == 0


def test_argument_errors_name_the_call():
    from dnmf_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    buf = (ctypes.c_double * 1024)()
    p = ctypes.addressof(buf)
    ok = [p, 1000, 0, p, 200, 0, 12, 10, 1, p, 4, p, 3, p, p, p, 0, p, 1 << 20, 0]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        rc = lib.dnmf_warp_normal_eqs(*a)
        return rc, lib.dnmf_last_error().decode()

    for i in (0, 3, 9, 11, 13, 14, 15, 17):
        rc, msg = call(**{f"a{i}": 0})
        assert rc == -1 and msg.startswith("dnmf_warp_normal_eqs:"), (i, rc, msg)
    for kw in ({"a12": 0}, {"a12": 65536}, {"a6": 0}, {"a10": 0}, {"a1": 10}, {"a4": 119}):
        rc, msg = call(**kw)
        assert rc == -2 and msg.startswith("dnmf_warp_normal_eqs:"), (kw, rc, msg)
    rc, msg = call(a18=lib.dnmf_warp_normal_eqs_workspace(12, 10, 1, 3) - 1)
    assert rc == -4 and "workspace" in msg and msg.startswith("dnmf_warp_normal_eqs:")
    lm = [p, p, p, 2, 1, p, p, 4, p, p, p, p, p, p, p, p, 10.0, 1e-3, 1e-9, 1e9, 0, 0]
    for i in (0, 1, 2, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15):
        a = list(lm)
        a[i] = 0
        assert lib.dnmf_lm_step(*a) == -1 and lib.dnmf_last_error().decode().startswith("dnmf_lm_step:")
    for i, v in ((3, 0), (16, 1.0), (17, 0.0), (18, 0.0), (19, 1e-12)):
        a = list(lm)
        a[i] = v
        assert lib.dnmf_lm_step(*a) == -2 and lib.dnmf_last_error().decode().startswith("dnmf_lm_step:")


def test_public_signatures():
    from dnmf_amd import ops
    from dnmf_amd.Demix.dNMF import DeformableNMF, MultiChannelDNMF

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(DeformableNMF.update_motion) == [("self", E), ("dataloader", E), ("optimizer", E), ("gamma", 0), ("epochs", 20),
                                                   ("solver", "adam"), ("iters", None), ("damping", 1e-3)]
    assert ("motion_solver", "adam") in params(DeformableNMF.fit)
    assert MultiChannelDNMF.update_motion is DeformableNMF.update_motion
    assert params(ops.warp_normal_eqs)[:7] == [("S", E), ("s_ids", E), ("frames", E), ("frame_ids", E), ("sz", E), ("beta", E),
                                               ("times", E)]
    assert [n for n, _ in params(ops.lm_step)][:5] == ["state", "eqs", "sz", "beta", "times"]
    assert dict(params(ops.lm_step))["nu"] == 10.0 and dict(params(ops.lm_step))["lam0"] == 1e-3
    assert dict(params(ops.lm_step))["lam_min"] == 1e-9 and dict(params(ops.lm_step))["lam_max"] == 1e9
    # the solver is checked before anything touches the GPU or the loader
    model = DeformableNMF.__new__(DeformableNMF)
    with pytest.raises(ValueError, match="update_motion.*bogus"):
        model.update_motion(None, None, solver='bogus')
    with pytest.raises(ValueError, match="fit.*bogus"):
        model.fit(None, None, None, 1, motion_solver='bogus')
