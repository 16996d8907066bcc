"""The Gauss-Newton motion step for one warp order (K16o, dnmf_lm_step_order) on the GPU: against tests/gn_order_restatement.py
on K16's own normal equations, order 2 against dnmf_lm_step / dnmf_lm_step_smooth, and update_motion(solver='gn') with
model.motion_order on warps six voxels from the start.

Tolerances:
  step   tests/test_gpu_gn.py's bound for dnmf_lm_step: the device writes the next trial as fp32(beta_acc + d beta); against fp32 of
         the restatement's float64 sum it may differ by 100 kappa 2.2e-16 max|d beta| (kappa: condition number of the damped scaled
         system, here the restricted one) plus one fp32 rounding, 6e-8 |beta|
  prior  tests/test_gpu_gn_smooth.py's: theta = Minv beta is a float64 dot product of ten terms on both sides, in another order
  order 2 against the two existing entries: the same device code after the bookkeeping, asserted bit for bit
"""
import numpy as np
import pytest
import torch

import gn_order_restatement as GO
import gn_restatement as GN
import gn_smooth_restatement as GS
from oracle import dnmf_oracle as O

pytestmark = pytest.mark.gpu

FROZEN = {"translation": list(range(1, 10)), "affine": list(range(4, 10)), "quadratic": []}
SMOOTH = 1e-4


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


def step_order(st, eqs, sz, beta, tt, order, accept_only=False, m=0.0, beta_ref=None, lam0=1e-3):
    """dnmf_lm_step_order itself, for every order (``ops.lm_step`` sends 'quadratic' to the two older entries)."""
    from dnmf_amd import _lib, ops
    Mc, Minv = ops._centred(sz, beta.device)
    if m and "prior" not in st:
        st["prior"] = torch.zeros((st["counts"].shape[0],), dtype=torch.float64, device="cuda")
    rc = _lib.load().dnmf_lm_step_order(eqs["H"].data_ptr(), eqs["g"].data_ptr(), eqs["sse"].data_ptr(), tt.numel(), int(sz[2]),
                                        GO.ORDERS[order], Mc.data_ptr(), Minv.data_ptr(), beta.data_ptr(), beta.shape[2],
                                        tt.data_ptr(), st["H"].data_ptr(), st["g"].data_ptr(), st["sse"].data_ptr(),
                                        st["sse0"].data_ptr(), st["lam"].data_ptr(), st["beta"].data_ptr(), st["counts"].data_ptr(),
                                        10.0, lam0, 1e-9, 1e9, 1 if accept_only else 0, beta_ref.data_ptr() if m else None, float(m),
                                        st["prior"].data_ptr() if m else None, None)
    _lib.check(rc, "dnmf_lm_step_order")


@pytest.fixture(scope="module")
def problems():
    """fit_problem's defaults: K = 6, T = 5 frames, warps up to ~1.9 voxels from the identity; the images K16 reads."""
    out = {}
    for sz in [(24, 20, 2), (24, 20, 1)]:
        p = GN.fit_problem(sz)
        p["S32"] = GN.recon_images(p["A"], p["C"], range(5)).astype(np.float32)
        out[sz] = p
    return out


def step_start(sz, Tn, times):
    """Coefficients to step from: the identity, small odd values in the quadratic rows and a negative zero among them (what a
    frozen row has to keep), other values in the columns that serve as neighbours only."""
    rng = np.random.default_rng(7)
    start = O.identity_beta(Tn)
    start[4:] = rng.normal(size=(6, 3, Tn)).astype(np.float32) * 1e-4
    start[5, 1, :] = -0.0
    ref = start.copy()
    ref[0] += rng.normal(size=(3, Tn)).astype(np.float32) * 0.3
    ref[:, :, times] = start[:, :, times]
    if sz[2] == 1:
        start[:, 2], ref[:, 2] = O.identity_beta(Tn)[:, 2], O.identity_beta(Tn)[:, 2]
    return start, ref


@pytest.mark.parametrize("smooth", [0.0, SMOOTH])
@pytest.mark.parametrize("order", GO.GRADED)
@pytest.mark.parametrize("sz", [(24, 20, 2), (24, 20, 1)])
def test_step_against_the_restatement(M, problems, sz, order, smooth):
    """B = 5 frames in the even columns of a 10-column beta (pairwise non-adjacent, as the prior needs; the odd columns are
    neighbours).  Four calls on K16's normal equations at the current trial: a first one, a plain one, one in which frame 1's sse
    is raised and frame 3's is NaN (both reject), an accept-only one.  After each call the restatement continues from the
    device's fp32 trial."""
    from dnmf_amd import ops
    p = problems[sz]
    B, Tn, times = 5, 10, [0, 2, 4, 6, 8]
    n = int(np.prod(sz))
    m = smooth * n
    start, ref0 = step_start(sz, Tn, times)
    S, frames = halo_images(p["S32"], sz), dev(p["frames"].reshape(B, -1))
    rows = torch.arange(B, dtype=torch.int32, device="cuda")
    tt = torch.tensor(times, dtype=torch.int32, device="cuda")
    ref_beta, ref_ref, ref = start.copy(), ref0.copy(), GS.new_state(B)
    beta, bref, st = dev(ref_beta), dev(ref_ref), ops.lm_state(B, "cuda")
    act, frozen = GO.active(sz, order), FROZEN[order]
    Minv_abs = np.abs(GS.basis_inverse(sz))
    decisions = []
    for call in range(4):
        last = call == 3
        eqs = ops.warp_normal_eqs(S, rows, frames, rows, sz, beta, tt)
        if call == 2:
            eqs["sse"][1] += 1e6
            eqs["sse"][3] = float("nan")
        H, g, sse = (eqs[k].cpu().numpy() for k in ("H", "g", "sse"))
        out = GO.lm_step(ref, H, g, sse, ref_beta, times, sz, order, accept_only=last, m=m, beta_ref=ref_ref if m else None)
        step_order(st, eqs, sz, beta, tt, order, accept_only=last, m=m, beta_ref=bref)
        got = beta.cpu().numpy()
        decisions.append(out["accept"].tolist())
        np.testing.assert_array_equal(st["counts"].cpu().numpy(), ref["counts"])          # identical decisions
        np.testing.assert_array_equal(st["lam"].cpu().numpy(), ref["lam"])
        np.testing.assert_array_equal(st["beta"].cpu().numpy(), ref["beta"])
        np.testing.assert_array_equal(st["sse"].cpu().numpy(), ref["sse"])
        np.testing.assert_array_equal(st["sse0"].cpu().numpy(), ref["sse0"])
        np.testing.assert_array_equal(st["H"].cpu().numpy(), ref["H"])
        if m:
            np.testing.assert_array_equal(bref.cpu().numpy(), ref_ref)
            prior = st["prior"].cpu().numpy()
        for b, t in enumerate(times):
            if m:
                mag = Minv_abs @ np.abs(ref["beta"][b].reshape(10, 3).astype(np.float64))
                th_acc, tol_p = GO.theta(ref["beta"][b], sz, order), 0.0
                for s in GS.neighbours(t, ref_ref):
                    delta = 50 * 2.2e-16 * (mag + Minv_abs @ np.abs(ref_ref[:, :, s].astype(np.float64))).reshape(30)[act]
                    d = np.abs(th_acc - GO.theta(ref_ref[:, :, s], sz, order))[act]
                    tol_p += m * float((2 * d * delta + delta ** 2).sum())
                assert abs(prior[b] - ref["prior"][b]) <= tol_p, (call, b, prior[b], ref["prior"][b], tol_p)
                assert ref["prior"][b] > 0
            Hp, gp = out["system"][b]
            Ah, _, _ = GO.damped_system(Hp, gp, ref["lam"][b], act)
            kappa = np.linalg.cond(Ah)
            tol = 100 * kappa * 2.2e-16 * np.abs(out["dbeta"][b]).max() + 6e-8 * np.abs(ref_beta[:, :, t])
            err = np.abs(got[:, :, t].astype(np.float64) - ref_beta[:, :, t])
            assert (err <= tol).all(), (call, b, kappa, err.max())
        # the rows above the order: the bits they came with
        assert got[frozen].tobytes() == start[frozen].tobytes(), call
        untouched = [t for t in range(Tn) if t not in times]
        np.testing.assert_array_equal(got[:, :, untouched], start[:, :, untouched])
        if not last:
            assert (got[0][:, times] != ref["beta"].reshape(B, 10, 3)[:, 0].T).any()       # a step was taken
        ref_beta[:, :, times] = got[:, :, times]                                           # the same fp32 trial on both sides
    assert decisions[0] == [True] * B and not decisions[2][1] and not decisions[2][3]
    assert np.isfinite(beta.cpu().numpy()).all()


@pytest.mark.parametrize("sz", [(24, 20, 2), (24, 20, 1)])
def test_ops_lm_step_order_is_the_entry(M, problems, sz):
    """``ops.lm_step(order=...)``: 'translation' and 'affine' through dnmf_lm_step_order, with and without the prior."""
    from dnmf_amd import ops
    p = problems[sz]
    B, Tn, times = 5, 10, [0, 2, 4, 6, 8]
    start, ref0 = step_start(sz, Tn, times)
    S, frames = halo_images(p["S32"], sz), dev(p["frames"].reshape(B, -1))
    rows = torch.arange(B, dtype=torch.int32, device="cuda")
    tt = torch.tensor(times, dtype=torch.int32, device="cuda")
    n = int(np.prod(sz))
    for order in ("translation", "affine"):
        for smooth in (0.0, SMOOTH):
            ba, bb, ra, rb = dev(start), dev(start), dev(ref0), dev(ref0)
            sa, sb = ops.lm_state(B, "cuda"), ops.lm_state(B, "cuda")
            for call in range(3):
                eqs = ops.warp_normal_eqs(S, rows, frames, rows, sz, ba, tt)
                ops.lm_step(sa, eqs, sz, ba, times, accept_only=call == 2, smooth=smooth, beta_ref=ra if smooth else None, order=order)
                step_order(sb, eqs, sz, bb, tt, order, accept_only=call == 2, m=smooth * n, beta_ref=rb)
                assert torch.equal(ba, bb) and torch.equal(ra, rb)
                assert all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize("sz", [(24, 20, 2), (24, 20, 1)])
def test_order_two_is_the_existing_steps_bit_for_bit(M, problems, sz):
    """dnmf_lm_step_order(order = 2) against dnmf_lm_step (m = 0) and dnmf_lm_step_smooth (m != 0) on the same inputs: after the
    bookkeeping all three run one device function with the same arguments, so every output is asserted equal in its bits --
    trial, accepted state, damping, counts, prior, beta_ref -- over a first, a plain, a rejecting and an accept-only call."""
    from dnmf_amd import ops
    p = problems[sz]
    B, Tn, times = 5, 10, [0, 2, 4, 6, 8]
    start, ref0 = step_start(sz, Tn, times)
    S, frames = halo_images(p["S32"], sz), dev(p["frames"].reshape(B, -1))
    rows = torch.arange(B, dtype=torch.int32, device="cuda")
    tt = torch.tensor(times, dtype=torch.int32, device="cuda")
    n = int(np.prod(sz))
    for smooth in (0.0, SMOOTH):
        ba, bb, ra, rb = dev(start), dev(start), dev(ref0), dev(ref0)
        sa, sb = ops.lm_state(B, "cuda"), ops.lm_state(B, "cuda")
        for call in range(4):
            eqs = ops.warp_normal_eqs(S, rows, frames, rows, sz, ba, tt)
            if call == 2:
                eqs["sse"][1] += 1e6
                eqs["sse"][3] = float("nan")
            ops.lm_step(sa, eqs, sz, ba, times, accept_only=call == 3, smooth=smooth, beta_ref=ra if smooth else None)
            step_order(sb, eqs, sz, bb, tt, "quadratic", accept_only=call == 3, m=smooth * n, beta_ref=rb)
            assert ba.cpu().numpy().tobytes() == bb.cpu().numpy().tobytes(), (smooth, call)
            assert torch.equal(ra, rb)
            for k in sa:
                assert sa[k].cpu().numpy().tobytes() == sb[k].cpu().numpy().tobytes(), (smooth, call, k)
        assert int(sa["counts"][1, 1]) >= 1 and int(sa["counts"][3, 1]) >= 1     # the two rejections were among the calls
        assert not torch.equal(ba, dev(start))


def test_zero_H_and_a_nan_frame(M):
    """H = 0: delta = 0 for every order, the coefficients keep their bits.  A frame whose coefficients hold a NaN stays NaN and
    the frame beside it steps as if it were alone."""
    from dnmf_amd import ops
    sz = (12, 10, 2)
    start = O.identity_beta(3)
    start[5, 1, :] = -0.0
    z = {"H": torch.zeros((2, 30, 30), dtype=torch.float64, device="cuda"), "g": torch.zeros((2, 30), dtype=torch.float64, device="cuda"),
         "sse": torch.ones((2,), dtype=torch.float64, device="cuda")}
    tt = torch.tensor([2, 0], dtype=torch.int32, device="cuda")
    for order in ("translation", "affine"):
        beta = dev(start)
        step_order(ops.lm_state(2, "cuda"), z, sz, beta, tt, order)
        assert beta.cpu().numpy().tobytes() == start.tobytes()
    rng = np.random.default_rng(3)
    J = rng.normal(size=(2, 60, 30))
    eqs = {"H": dev(np.einsum("bpi,bpj->bij", J, J), torch.float64), "g": dev(rng.normal(size=(2, 30)), torch.float64),
           "sse": dev(np.array([np.nan, 3.0]), torch.float64)}
    eqs["H"][0], eqs["g"][0] = 0.0, 0.0                                   # what K16 gives for a NaN frame
    bad = start.copy()
    bad[0, 1, 2] = np.nan
    pair, alone = dev(bad), dev(start)
    step_order(ops.lm_state(2, "cuda"), eqs, sz, pair, tt, "affine")
    one = {k: v[1:].contiguous() for k, v in eqs.items()}
    step_order(ops.lm_state(1, "cuda"), one, sz, alone, tt[1:].contiguous(), "affine")
    pair, alone = pair.cpu().numpy(), alone.cpu().numpy()
    assert np.isnan(pair[0, 1, 2]) and pair[:, :, 0].tobytes() == alone[:, :, 0].tobytes()
    assert (alone[:4, :, 0] != start[:4, :, 0]).any() and alone[4:].tobytes() == start[4:].tobytes()


# ---- the fit ---------------------------------------------------------------------------------------------------------
def make_model(M, sz, p):
    K, T = p["C"].shape
    model = M.DeformableNMF(torch.tensor(sz), K, T, positions=torch.from_numpy(p["pos"]))
    model.fp.A = dev(p["A"])
    model.C = dev(p["C"])
    model.verbose = False
    assert model.motion_order == 'quadratic'                            # the default: every coefficient
    return model


def resident(M, sz, frames, batch=2):
    return M.ResidentLoader(dev(frames.reshape(frames.shape[0], -1)), sz, batch)


@pytest.mark.parametrize("seed", [0, 1])
def test_graded_schedule_end_to_end(M, seed):
    """48 x 40 x 2, K = 6, T = 4, every frame's warp a 6-voxel shift (plus affine 0.02, quadratic 0.25 voxel) from the identity
    start.  The float64 definition (tests/test_gn_order_host.py): graded 6 + 6 + 6 ends 1.3e-5 / 3.0e-5 voxel off (seed 0 / 1), 16
    full-order iterations end 81.9 / 611.8 voxels off.  Asserted here: graded <= 0.05 voxel, tests/test_gpu_gn.py's bar; the
    default order > 5 voxels.  Measured on the MI355X: graded 1.3e-5 / 1.6e-5, default order 82.3 / 159."""
    sz = (48, 40, 2)
    p = GO.shifted_problem(sz, 6, seed)
    T = p["C"].shape[1]
    model = make_model(M, sz, p)
    model.motion_order = 'graded'
    grad_before = model.fp.beta.grad
    model.update_motion(resident(M, sz, p["frames"]), None, solver='gn', iters=6)
    graded = GN.field_error(model.fp.beta.detach().cpu().numpy(), p["beta_true"], sz)
    st = model.last_motion_gn
    full = make_model(M, sz, p)
    full.update_motion(resident(M, sz, p["frames"]), None, solver='gn', iters=16)
    err_full = GN.field_error(full.fp.beta.detach().cpu().numpy(), p["beta_true"], sz)
    print(f"\nseed {seed}: graded 6+6+6 field error {graded:.3g} voxel, full order 16 iterations {err_full:.3g}; stage sse "
          + ", ".join(f"{s['order']} {float(s['sse0'].sum()):.4g} -> {float(s['sse'].sum()):.4g}" for s in st["stages"]))
    assert graded <= 0.05
    assert err_full > 5
    assert model.fp.beta.requires_grad and model.fp.beta.grad is grad_before
    assert [s["order"] for s in st["stages"]] == ["translation", "affine", "quadratic"]
    for s in st["stages"]:
        assert s["sse0"].shape == s["sse"].shape == (T,) and bool((s["sse"] <= s["sse0"]).all())
    for a, b in zip(st["stages"], st["stages"][1:]):
        assert torch.equal(b["sse0"], a["sse"])                           # a stage starts where the last one ended
    assert torch.equal(st["sse0"], st["stages"][0]["sse0"]) and torch.equal(st["sse"], st["stages"][2]["sse"])
    assert bool((st["accepted"] + st["rejected"] == 3 * 6).all())
    assert "stages" not in full.last_motion_gn


def test_fixed_orders_leave_the_other_rows(M, problems):
    """A single order and a hand-written schedule through the model, from every kind of loader state the default path has: the
    rows above the order keep the start's bits, every frame's sse falls."""
    sz = (24, 20, 2)
    p = problems[sz]
    T = p["C"].shape[1]
    ident = O.identity_beta(T)
    for order, frozen in (("translation", FROZEN["translation"]), ("affine", FROZEN["affine"]),
                          ([("translation", 2), ("affine", 3)], FROZEN["affine"])):
        model = make_model(M, sz, p)
        model.motion_order, model.motion_chunk = order, 2                 # 2 + 2 + 1 frames
        model.update_motion(resident(M, sz, p["frames"]), None, solver='gn', iters=4)
        beta = model.fp.beta.detach().cpu().numpy()
        assert beta[frozen].tobytes() == ident[frozen].tobytes()
        st = model.last_motion_gn
        assert bool((st["sse"] < st["sse0"]).all()) and len(st["stages"]) == (1 if isinstance(order, str) else 2)
    model.motion_smooth = SMOOTH                                          # with the prior: red-black colours inside every stage
    model.update_motion(resident(M, sz, p["frames"]), None, solver='gn', iters=2)
    assert model.fp.beta.detach().cpu().numpy()[frozen].tobytes() == ident[frozen].tobytes()
    assert bool(torch.isfinite(model.last_motion_gn["prior"]).all())


def test_default_order_is_the_loop_as_it_was(M, problems, monkeypatch):
    """``motion_order`` left alone: ``fp.beta`` has the bits of the loop written out here with the calls the driver made before
    the attribute existed (K16 + ``ops.lm_step`` without ``order``), and of a model whose attribute is set to the default."""
    from dnmf_amd import ops
    sz, iters = (24, 20, 2), 8
    p = problems[sz]
    T = p["C"].shape[1]
    hand = make_model(M, sz, p)
    frames = dev(p["frames"].reshape(T, -1))
    tt = torch.arange(T, dtype=torch.int32, device="cuda")
    beta = hand.fp.beta.detach()
    with torch.no_grad():
        S = hand.fp.recon_image(hand.C.to("cuda", torch.float32).contiguous(), tt)
        state, eqs = ops.lm_state(T, "cuda"), None
        for it in range(iters + 1):
            eqs = ops.warp_normal_eqs(S, None, frames, tt, sz, beta, tt, out=eqs)
            ops.lm_step(state, eqs, sz, beta, tt, lam0=1e-3, accept_only=it == iters)
    want = beta.cpu().numpy()
    orders, real = [], ops.lm_step

    def spy(*a, **kw):
        orders.append(kw.get("order"))
        return real(*a, **kw)

    monkeypatch.setattr(ops, "lm_step", spy)
    left = make_model(M, sz, p)
    left.update_motion(resident(M, sz, p["frames"]), None, solver='gn', iters=iters)
    named = make_model(M, sz, p)
    named.motion_order = 'quadratic'
    named.update_motion(resident(M, sz, p["frames"]), None, solver='gn', iters=iters)
    for model in (left, named):
        assert model.fp.beta.detach().cpu().numpy().tobytes() == want.tobytes()
        assert sorted(model.last_motion_gn) == ["accepted", "lam", "rejected", "sse", "sse0"]
    assert orders == ["quadratic"] * (2 * (iters + 1))
    assert torch.equal(left.last_motion_gn["sse"], state["sse"]) and GN.field_error(want, p["beta_true"], sz) < 0.05
