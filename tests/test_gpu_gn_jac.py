"""The Gauss-Newton motion step with the volume-preserving prior (K16j, dnmf_lm_step_jac) on the GPU: against
tests/gn_jac_restatement.py on K16's own normal equations, ``jacobian=0.0`` against the call without the argument, run against run,
and update_motion(solver='gn') with model.motion_jacobian.

Shapes 24 x 20 x 2 and 24 x 20 x 1, K = 6, B in {1, 3, 5} frames: the smallest at which the 30- and the 12-unknown paths, the
corner points of a two-slice volume and the indexing of a several-frame state can go wrong.

Tolerances:
  trial    the next trial column is within one fp32 ulp of the restatement's float64 sum rounded to fp32
  jac      ten times the deviation measured on the MI355X against the restatement, both in units of m_j:
           JAC_TOL for |jac - restatement| / m_j, DET_TOL for |min_det - restatement|
"""
import numpy as np
import pytest
import torch

import gn_jac_restatement as GJ
import gn_order_restatement as GO
import gn_restatement as GN
import gn_smooth_restatement as GS
from oracle import dnmf_oracle as O

pytestmark = pytest.mark.gpu

SMOOTH, JACOBIAN = 1e-4, 1e-3
SHAPES = [(24, 20, 2), (24, 20, 1)]
JAC_TOL, DET_TOL = 10 * 4.4e-17, 10 * 2.3e-16      # ten times the largest measured (mean_p rho^2 up to 0.098): DESIGN 4, K16j


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd.Demix import dNMF
    return dNMF


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def halo_images(S32, sz):
    from dnmf_amd import ops
    out = torch.zeros((S32.shape[0], ops.halo_voxels(sz)), dtype=torch.float32, device="cuda")
    ops.halo_interior(out, sz).copy_(dev(S32))
    return out


@pytest.fixture(scope="module")
def problems():
    """fit_problem's defaults: K = 6, T = 5 frames, warps up to ~1.9 voxels from the identity; the images K16 reads."""
    out = {}
    for sz in SHAPES:
        p = GN.fit_problem(sz)
        p["S32"] = GN.recon_images(p["A"], p["C"], range(5)).astype(np.float32)
        out[sz] = p
    return out


def step_start(sz, Tn, times):
    """Coefficients to step from: the identity with small values in the quadratic rows (a map with rho != 0 at every sample
    point), other values in the columns that serve as neighbours only."""
    rng = np.random.default_rng(7)
    start = O.identity_beta(Tn)
    start[4:] = rng.normal(size=(6, 3, Tn)).astype(np.float32) * 1e-4
    ref = start.copy()
    ref[0] += rng.normal(size=(3, Tn)).astype(np.float32) * 0.3
    ref[:, :, times] = start[:, :, times]
    if sz[2] == 1:
        start[:, 2], ref[:, 2] = O.identity_beta(Tn)[:, 2], O.identity_beta(Tn)[:, 2]
    return start, ref


def reflected(sz):
    """The map x -> (X - 1) - x, y and z kept: det J = -1 everywhere."""
    col = O.identity_beta(1)[:, :, 0].copy()
    col[0, 0], col[1, 0] = float(sz[0] - 1), -1.0
    return col


def setup(p, sz, B):
    Tn, times = 2 * B, list(range(0, 2 * B, 2))
    start, ref0 = step_start(sz, Tn, times)
    S, frames = halo_images(p["S32"][:B], sz), dev(p["frames"][:B].reshape(B, -1))
    rows = torch.arange(B, dtype=torch.int32, device="cuda")
    tt = torch.tensor(times, dtype=torch.int32, device="cuda")
    return Tn, times, start, ref0, S, frames, rows, tt


def test_sample_points_are_the_restatements(M):
    from dnmf_amd import ops
    for sz in SHAPES + [(9, 7, 3)]:
        pts = ops.warp_jacobian_points(sz)
        assert pts.dtype == np.float64 and pts.shape == ((9, 3) if sz[2] > 1 else (5, 3))
        np.testing.assert_array_equal(pts, GJ.points(sz))


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("smooth", [0.0, SMOOTH])
@pytest.mark.parametrize("order", GO.GRADED)
@pytest.mark.parametrize("sz", SHAPES)
def test_step_against_the_restatement(M, problems, sz, order, smooth, B):
    """B frames in the even columns of a 2B-column beta (pairwise non-adjacent, as the temporal prior needs; the odd columns are
    neighbours).  Five calls of ``ops.lm_step(jacobian=...)`` on K16's normal equations at the current trial: a first one, a plain
    one, one in which frame 0's sse is raised (it rejects), one whose last frame's trial column is set to a reflected map with its
    sse set to 0 (folded: it must reject although the data term is the best possible), an accept-only one.  After each call
    the restatement continues from the device's fp32 trial."""
    from dnmf_amd import ops
    p = problems[sz]
    Tn, times, start, ref0, S, frames, rows, tt = setup(p, sz, B)
    n = int(np.prod(sz))
    m, mj = smooth * n, JACOBIAN * n
    ref_beta, ref_ref, ref = start.copy(), ref0.copy(), GJ.new_state(B)
    beta, bref, st = dev(ref_beta), dev(ref_ref), ops.lm_state(B, "cuda")
    frozen = {"translation": list(range(1, 10)), "affine": list(range(4, 10)), "quadratic": []}[order]
    decisions, worst = [], [0.0, 0.0, 0.0]
    for call in range(5):
        last = call == 4
        if call == 3:
            ref_beta[:, :, times[-1]] = reflected(sz)
            beta[:, :, times[-1]] = dev(reflected(sz))
        eqs = ops.warp_normal_eqs(S, rows, frames, rows, sz, beta, tt)
        if call == 2:
            eqs["sse"][0] += 1e6
        if call == 3:
            eqs["sse"][B - 1] = 0.0
        H, g, sse = (eqs[k].cpu().numpy() for k in ("H", "g", "sse"))
        out = GJ.lm_step(ref, H, g, sse, ref_beta, times, sz, order, accept_only=last, m=m, beta_ref=ref_ref if m else None, mj=mj)
        ops.lm_step(st, eqs, sz, beta, times, accept_only=last, smooth=smooth, beta_ref=bref if smooth else None, order=order,
                    jacobian=JACOBIAN)
        got = beta.cpu().numpy()
        decisions.append(out["accept"].tolist())
        assert out["folded"].tolist() == [call == 3 and b == B - 1 for b in range(B)]      # the hand-made trial folds, no other
        np.testing.assert_array_equal(st["counts"].cpu().numpy(), ref["counts"])          # identical decisions
        np.testing.assert_array_equal(st["lam"].cpu().numpy(), ref["lam"])
        np.testing.assert_array_equal(st["beta"].cpu().numpy(), ref["beta"])
        np.testing.assert_array_equal(st["sse"].cpu().numpy(), ref["sse"])
        np.testing.assert_array_equal(st["sse0"].cpu().numpy(), ref["sse0"])
        np.testing.assert_array_equal(st["H"].cpu().numpy(), ref["H"])
        np.testing.assert_array_equal(st["g"].cpu().numpy(), ref["g"])
        if m:
            np.testing.assert_array_equal(bref.cpu().numpy(), ref_ref)
        jac, mind = st["jac"].cpu().numpy(), st["min_det"].cpu().numpy()
        assert jac.shape == mind.shape == (B,)
        dj, dd = np.abs(jac - ref["jac"]) / mj, np.abs(mind - ref["min_det"])
        worst[0], worst[1] = max(worst[0], dj.max()), max(worst[1], dd.max())
        ref32 = ref_beta[:, :, times]
        ulps = np.abs(got[:, :, times].astype(np.float64) - ref32) / np.spacing(np.abs(ref32)).astype(np.float64)
        worst[2] = max(worst[2], ulps.max())
        print(f"\n{sz} {order} smooth {smooth} B {B} call {call}: |jac - ref| / mj {dj.max():.3g}, |min_det - ref| {dd.max():.3g}, "
              f"jac / mj {(ref['jac'] / mj).max():.3g}, trial {ulps.max():.3g} fp32 ulp")
        assert (ref["jac"] > 0).all() and np.isfinite(ref["jac"]).all() and (ref["min_det"] > 0).all()
        assert (dj <= JAC_TOL).all() and (dd <= DET_TOL).all(), (call, dj.max(), dd.max())
        assert ulps.max() <= 1.0, (call, ulps.max())                                       # the next trial: one fp32 ulp
        assert got[frozen][:, :, times].tobytes() == start[frozen][:, :, times].tobytes(), call
        untouched = [t for t in range(Tn) if t not in times]
        np.testing.assert_array_equal(got[:, :, untouched], start[:, :, untouched])
        ref_beta[:, :, times] = got[:, :, times]                                           # the same fp32 trial on both sides
    print(f"{sz} {order} smooth {smooth} B {B}: worst |jac - ref| / mj {worst[0]:.3g}, |min_det - ref| {worst[1]:.3g}, "
          f"trial {worst[2]:.3g} fp32 ulp")
    assert decisions[0] == [True] * B and not decisions[2][0]
    assert not decisions[3][B - 1]                                                         # the folded trial never got in
    assert int(st["counts"][0, 1]) >= 1 and int(st["counts"][B - 1, 1]) >= 1
    assert np.isfinite(beta.cpu().numpy()).all()
    # what is kept after the folded trial is the accepted point, not the reflected column
    assert got[1, 0, times[-1]] > 0


@pytest.mark.parametrize("sz", SHAPES)
def test_a_folded_start_is_beaten_by_any_admissible_trial(M, problems, sz):
    """The first call accepts whatever it is given: a reflected map, J = +inf, min_det = -1.  The next trial (an admissible map,
    put there by hand) is accepted although its sse is raised above the accepted one."""
    from dnmf_amd import ops
    p = problems[sz]
    Tn, times, start, ref0, S, frames, rows, tt = setup(p, sz, 1)
    beta, st = dev(start), ops.lm_state(1, "cuda")
    beta[:, :, 0] = dev(reflected(sz))
    eqs = ops.warp_normal_eqs(S, rows, frames, rows, sz, beta, tt)
    ops.lm_step(st, eqs, sz, beta, times, jacobian=JACOBIAN)
    assert float(st["jac"][0]) == float("inf") and float(st["min_det"][0]) == -1.0 and int(st["counts"][0, 2]) == 1
    beta[:, :, 0] = dev(start[:, :, 0])
    eqs = ops.warp_normal_eqs(S, rows, frames, rows, sz, beta, tt)
    eqs["sse"][0] = st["sse"][0] + 1e6
    ops.lm_step(st, eqs, sz, beta, times, jacobian=JACOBIAN, accept_only=True)
    assert st["counts"].cpu().tolist() == [[1, 0, 1]]
    assert np.isfinite(float(st["jac"][0])) and float(st["min_det"][0]) > 0.9
    assert beta.cpu().numpy()[:, :, 0].tobytes() == start[:, :, 0].tobytes()


@pytest.mark.parametrize("sz", SHAPES)
def test_zero_weight_is_the_call_without_the_argument(M, problems, sz):
    """``jacobian=0.0`` goes to the three existing entries: every output has the bits of the call that does not name it."""
    from dnmf_amd import ops
    p = problems[sz]
    B = 5
    Tn, times, start, ref0, S, frames, rows, tt = setup(p, sz, B)
    for order in GO.GRADED:
        for smooth in (0.0, SMOOTH):
            ba, bb, ra, rb = dev(start), dev(start), dev(ref0), dev(ref0)
            sa, sb = ops.lm_state(B, "cuda"), ops.lm_state(B, "cuda")
            for call in range(4):
                eqs = ops.warp_normal_eqs(S, rows, frames, rows, sz, ba, tt)
                if call == 2:
                    eqs["sse"][1] += 1e6
                kw = dict(accept_only=call == 3, smooth=smooth, order=order)
                ops.lm_step(sa, eqs, sz, ba, times, beta_ref=ra if smooth else None, jacobian=0.0, **kw)
                ops.lm_step(sb, eqs, sz, bb, times, beta_ref=rb if smooth else None, **kw)
                assert ba.cpu().numpy().tobytes() == bb.cpu().numpy().tobytes(), (order, smooth, call)
                assert torch.equal(ra, rb) and sorted(sa) == sorted(sb) and "jac" not in sa
                for k in sa:
                    assert sa[k].cpu().numpy().tobytes() == sb[k].cpu().numpy().tobytes(), (order, smooth, call, k)
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lm_step.*jacobian"):
            ops.lm_step(sa, eqs, sz, ba, times, jacobian=bad)


@pytest.mark.parametrize("sz", SHAPES)
def test_two_runs_give_the_same_bits(M, problems, sz):
    from dnmf_amd import ops
    p = problems[sz]
    B = 5
    Tn, times, start, ref0, S, frames, rows, tt = setup(p, sz, B)

    def run(order, smooth):
        beta, bref, st = dev(start), dev(ref0), ops.lm_state(B, "cuda")
        for call in range(4):
            eqs = ops.warp_normal_eqs(S, rows, frames, rows, sz, beta, tt)
            ops.lm_step(st, eqs, sz, beta, times, accept_only=call == 3, smooth=smooth, beta_ref=bref if smooth else None, order=order,
                        jacobian=JACOBIAN)
        return [beta.cpu().numpy().tobytes(), bref.cpu().numpy().tobytes()] + [st[k].cpu().numpy().tobytes() for k in sorted(st)]

    for order in GO.GRADED:
        for smooth in (0.0, SMOOTH):
            assert run(order, smooth) == run(order, smooth), (order, smooth)


# ---- the fit ---------------------------------------------------------------------------------------------------------
ITERS = 8


def make_model(M, sz, p, cls=None, **kw):
    K, T = p["C"].shape
    model = (cls or M.DeformableNMF)(torch.tensor(sz), K, T, positions=torch.from_numpy(p["pos"]), **kw)
    model.fp.A = dev(p["A"])
    model.C = dev(p["C"])
    model.verbose = False
    assert model.motion_jacobian == 0.0                                  # the default: no prior
    return model


def resident(M, sz, frames, batch=2):
    return M.ResidentLoader(dev(frames.reshape(frames.shape[0], -1)), sz, batch)


def test_update_motion_with_the_prior(M, problems):
    """The planted 24 x 20 x 2 problem of tests/test_gpu_gn.py, ``model.motion_jacobian = 1e-3``, 8 iterations from the identity:
    per-frame errors against the restatement's fit to four digits (5e-5 voxel), min_det > 0 on every frame, the prior's keys in
    ``last_motion_gn`` -- and none of them, nor another bit of beta, when the weight is left alone."""
    sz = (24, 20, 2)
    p = problems[sz]
    T = p["C"].shape[1]
    beta64, ref, _ = GJ.fit_gn_jac(p["A"], p["C"], O.identity_beta(T), sz, range(T), p["frames"], ITERS, JACOBIAN)
    want = GS.frame_errors(beta64, p["beta_true"], sz)
    model = make_model(M, sz, p)
    model.motion_jacobian = JACOBIAN
    model.motion_chunk = 2                                                # 2 + 2 + 1 frames
    grad_before = model.fp.beta.grad
    model.update_motion(resident(M, sz, p["frames"]), None, solver='gn', iters=ITERS)
    beta = model.fp.beta.detach().cpu().numpy()
    err = GS.frame_errors(beta, p["beta_true"], sz)
    print(f"\nGPU per-frame error {np.round(err, 5).tolist()}, restatement {np.round(want, 5).tolist()}")
    assert (np.abs(err - want) <= 5e-5).all()
    st = model.last_motion_gn
    assert sorted(st) == ["accepted", "jac", "lam", "min_det", "rejected", "sse", "sse0"]
    assert st["jac"].shape == st["min_det"].shape == (T,)
    assert bool((st["min_det"] > 0).all()) and bool(torch.isfinite(st["jac"]).all()) and bool((st["jac"] > 0).all())
    np.testing.assert_allclose(st["min_det"].cpu().numpy(), GJ.min_det(beta, sz), rtol=1e-12)
    np.testing.assert_allclose(st["min_det"].cpu().numpy(), ref["min_det"], atol=1e-4)
    assert model.fp.beta.requires_grad and model.fp.beta.grad is grad_before
    # frames not served: NaN
    part = make_model(M, sz, p)
    part.motion_jacobian = JACOBIAN
    part.update_motion(M.ResidentLoader(dev(p["frames"].reshape(T, -1))[:3], sz, 2), None, solver='gn', iters=2)
    assert bool(torch.isnan(part.last_motion_gn["min_det"][3:]).all()) and bool((part.last_motion_gn["min_det"][:3] > 0).all())
    # with the other two priors switched on as well the keys add up and the warp still does not fold
    model.motion_smooth, model.motion_order = SMOOTH, 'graded'
    model.update_motion(resident(M, sz, p["frames"]), None, solver='gn', iters=2)
    assert sorted(model.last_motion_gn) == ["accepted", "jac", "lam", "min_det", "prior", "rejected", "sse", "sse0", "stages"]
    assert bool((model.last_motion_gn["min_det"] > 0).all())
    # Adam has no such term
    model.motion_smooth, model.motion_order = 0.0, 'quadratic'
    opt = torch.optim.Adam([model.fp.beta], lr=1e-5)
    with pytest.raises(ValueError, match="update_motion.*motion_jacobian.*'gn' only"):
        model.update_motion(resident(M, sz, p["frames"]), opt, epochs=1)
    with pytest.raises(ValueError, match="fit.*motion_jacobian.*'gn' only"):
        make_model(M, sz, p).fit(None, None, opt, 2, motion_jacobian=JACOBIAN)


def test_two_channels_weigh_the_prior_by_their_residuals(M, problems):
    """Two identical colour channels: n_residuals is voxels x channels, so sse and J both double and the fit is the
    single-channel one."""
    sz = (24, 20, 2)
    p = problems[sz]
    K = p["C"].shape[0]
    one = make_model(M, sz, p)
    two = make_model(M, sz, p, cls=M.MultiChannelDNMF, colours=np.ones((2, K), np.float32))
    one.motion_jacobian = two.motion_jacobian = JACOBIAN
    one.update_motion(resident(M, sz, p["frames"]), None, solver='gn', iters=ITERS)
    two.update_motion(resident(M, sz, np.stack([p["frames"], p["frames"]], 1)), None, solver='gn', iters=ITERS)
    assert GN.field_error(two.fp.beta.detach().cpu().numpy(), one.fp.beta.detach().cpu().numpy(), sz) <= 1e-3
    np.testing.assert_allclose(two.last_motion_gn["jac"].cpu().numpy(), 2 * one.last_motion_gn["jac"].cpu().numpy(), rtol=1e-3)
    assert bool((two.last_motion_gn["min_det"] > 0).all())
