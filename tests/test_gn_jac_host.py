"""The volume-preserving prior of the Gauss-Newton motion fit (K16j) without a GPU: the float64 definition
(tests/gn_jac_restatement.py) on maps whose log det J is known, against finite differences and against the older restatements,
its invariants over whole fits, what it buys on the warps of tests/test_gn_order_host.py, what it costs on a warp that does not
preserve volume, and the wiring of every layer."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import gn_jac_restatement as GJ
import gn_order_restatement as GO
import gn_restatement as GN
import gn_smooth_restatement as GS
from oracle import dnmf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(24, 20, 2), (24, 20, 1)]


def rotation(n, rng):
    if n == 2:
        a = rng.uniform(-0.4, 0.4)
        return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q * np.sign(np.linalg.det(Q))


def test_sample_points():
    p3, p2 = GJ.points((24, 20, 2)), GJ.points((24, 20, 1))
    assert p3.shape == (9, 3) and p2.shape == (5, 3) and p3.dtype == np.float64
    assert p3[:8].tolist() == [[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)] and not p3[8].any()
    assert p2[:4].tolist() == [[a, b, 0] for a in (-1, 1) for b in (-1, 1)] and not p2[4].any()
    from dnmf_amd import ops
    for sz in SHAPES:
        np.testing.assert_array_equal(ops.warp_jacobian_points(sz), GJ.points(sz))


@pytest.mark.parametrize("sz", SHAPES + [(48, 40, 2), (9, 7, 3), (512, 512, 1)])
def test_identity_is_exactly_zero(sz):
    for th in (GJ.theta_identity(sz), GJ.full_theta(O.identity_beta(1)[:, :, 0], sz)):
        rho, det = GJ.residuals(th, sz)
        assert not rho.any() and (det == 1.0).all()
        gadd, Hadd = GJ.prior_grad(th, sz, 3.0)
        assert not gadd.any() and GJ.prior(th, sz, 3.0) == 0.0
        assert Hadd.any()                                                 # the curvature is there all the same


@pytest.mark.parametrize("sz", SHAPES)
def test_rigid_motions_and_shears_cost_nothing(sz):
    """A rotation plus a translation in VOXEL coordinates on an anisotropic volume: in centred coordinates the map is no
    rotation (24 x 20 x 2: its determinant is 11.5 * 9.5 * 0.5), and rho = 0 only because L0 takes the extents out."""
    rng = np.random.default_rng(0)
    n = GJ.naxes(sz)
    for _ in range(5):
        R, c = rotation(n, rng), rng.uniform(-3, 3, n)
        rho, det = GJ.residuals(GJ.theta_affine(sz, R, c), sz)
        assert np.abs(rho).max() <= 1e-13 and np.abs(det - 1).max() <= 1e-13
        Ju = GJ.jacobians(GJ.theta_affine(sz, R, c), sz) * GJ.half_extents(sz)[None, None, :]
        np.testing.assert_allclose(np.log(np.linalg.det(Ju)) - np.log(GJ.half_extents(sz)).sum(), rho, atol=1e-13)
    shear = np.eye(n)
    shear[0, 1] = 0.3
    assert np.abs(GJ.residuals(GJ.theta_affine(sz, shear, np.zeros(n)), sz)[0]).max() <= 1e-13
    # through beta: the raw coefficients of the same rotation
    R, c = rotation(n, rng), rng.uniform(-3, 3, n)
    beta = O.identity_beta(1).astype(np.float64)[:, :, 0]
    beta[0, :n], beta[1:1 + n, :n] = c, R.T
    np.testing.assert_allclose(GJ.full_theta(beta, sz), GJ.theta_affine(sz, R, c), atol=1e-12)


@pytest.mark.parametrize("sz", SHAPES)
def test_uniform_scaling(sz):
    n = GJ.naxes(sz)
    for s in (0.5, 0.97, 1.25):
        rho, det = GJ.residuals(GJ.theta_affine(sz, s * np.eye(n), np.zeros(n)), sz)
        np.testing.assert_allclose(rho, n * np.log(s), rtol=0, atol=1e-14)
        np.testing.assert_allclose(det, s ** n, rtol=1e-14)
    mirror = np.eye(n)
    mirror[0, 0] = -1.0
    rho, det = GJ.residuals(GJ.theta_affine(sz, mirror, np.zeros(n)), sz)
    assert (rho == np.inf).all() and (det == -1.0).all() and GJ.prior(GJ.theta_affine(sz, mirror, np.zeros(n)), sz, 2.0) == np.inf
    assert not GJ.rows(GJ.theta_affine(sz, mirror, np.zeros(n)), sz).any()      # a folded point adds nothing to the step


@pytest.mark.parametrize("sz", SHAPES)
def test_gradient_against_central_differences(sz):
    """h = 1e-5 on theta (entries of order 1 to 10): truncation O(h^2) ~ 1e-10, rounding ~ 1e-11 of the function's scale.
    Asserted: 1e-7 of the largest gradient entry, for every row jrho_p and for the prior's gradient 2 gadd."""
    rng = np.random.default_rng(1)
    act, h, mj = GN.active(sz), 1e-5, 7.0
    # a perturbation of about 1 % of every entry of Jx: theta[a, d] enters column e of Jx over h_e for the axes e of its term
    he = GJ.half_extents(sz)
    scale = np.array([min([he[e] for e in range(len(he)) if GN.EXPO[a, e]] or [1.0]) for a in range(10)])
    for _ in range(4):
        th = GJ.theta_identity(sz)
        th[act] += (rng.normal(size=(10, 3)) * 0.01 * scale[:, None]).reshape(30)[act]
        rho0, _ = GJ.residuals(th, sz)
        assert np.isfinite(rho0).all() and np.abs(rho0).max() > 1e-3
        jr = GJ.rows(th, sz)
        gadd, Hadd = GJ.prior_grad(th, sz, mj)
        fd_rows, fd_grad = np.zeros_like(jr), np.zeros(30)
        for i in act:
            e = np.zeros(30)
            e[i] = h
            fd_rows[:, i] = (GJ.residuals(th + e, sz)[0] - GJ.residuals(th - e, sz)[0]) / (2 * h)
            fd_grad[i] = (GJ.prior(th + e, sz, mj) - GJ.prior(th - e, sz, mj)) / (2 * h)
        assert np.abs(jr - fd_rows).max() <= 1e-7 * np.abs(jr).max()
        assert np.abs(2 * gadd - fd_grad).max() <= 1e-7 * np.abs(gadd).max() * 2
        assert not np.delete(jr, act, axis=1).any()
        np.testing.assert_allclose(Hadd, (mj / len(rho0)) * jr.T @ jr, rtol=0, atol=1e-13 * np.abs(Hadd).max())
        # the value: mj / NP sum rho^2, and the rows of one order are the leading part of the full ones
        np.testing.assert_allclose(GJ.prior(th, sz, mj), mj * np.mean(rho0 ** 2), rtol=1e-14)
        for order in GO.GRADED:
            sel = GO.active(sz, order)
            part = GJ.rows(th, sz, sel)
            np.testing.assert_array_equal(part[:, sel], jr[:, sel])
            assert not np.delete(part, sel, axis=1).any()


def bookkeeping_calls():
    """tests/test_gn_order_host.py's hand-made two-frame calls."""
    rng = np.random.default_rng(1)
    J = rng.normal(size=(2, 50, 30))
    H = np.einsum("bpi,bpj->bij", J, J)
    g = rng.normal(size=(2, 30))
    nan = np.nan
    return [(H, g, [5.0, 7.0], False), (2 * H, g, [4.0, 7.5], False), (H, g, [nan, 6.0], True)] + [(H, g, [nan, nan], False)] * 3


@pytest.mark.parametrize("sz", [(9, 7, 3), (9, 7, 1)])
def test_zero_weight_is_the_older_definitions_bit_for_bit(sz):
    times = [3, 1]
    for order in GO.GRADED:
        for m in (0.0, 2.5):
            start = (O.identity_beta(5) + np.random.default_rng(3).normal(size=(10, 3, 5)) * 1e-3).astype(np.float32)
            ba, bb, ra, rb, sa, sb = start.copy(), start.copy(), start.copy(), start.copy(), GS.new_state(2), GJ.new_state(2)
            for H, g, sse, last in bookkeeping_calls():
                a = GO.lm_step(sa, H, g, np.array(sse), ba, times, sz, order, accept_only=last, m=m, beta_ref=ra if m else None)
                b = GJ.lm_step(sb, H, g, np.array(sse), bb, times, sz, order, accept_only=last, m=m, beta_ref=rb if m else None, mj=0.0)
                np.testing.assert_array_equal(a["accept"], b["accept"])
                assert a["dbeta"].tobytes() == b["dbeta"].tobytes() and ba.tobytes() == bb.tobytes() and ra.tobytes() == rb.tobytes()
                for k in sa:
                    assert sa[k].tobytes() == sb[k].tobytes(), (order, m, k)
                for (Ha, ga), (Hb, gb) in zip(a["system"], b["system"]):
                    assert Ha.tobytes() == Hb.tobytes() and ga.tobytes() == gb.tobytes()
            assert not sb["jac"].any() and not sb["min_det"].any()        # never written
    # and, all rows selected and no temporal prior, tests/gn_restatement.py's step
    ba, bb, sa, sb = O.identity_beta(4), O.identity_beta(4), GN.new_state(2), GJ.new_state(2)
    for H, g, sse, last in bookkeeping_calls():
        GN.lm_step(sa, H, g, np.array(sse), ba, times, sz, accept_only=last)
        GJ.lm_step(sb, H, g, np.array(sse), bb, times, sz, accept_only=last)
        assert ba.tobytes() == bb.tobytes() and all(sa[k].tobytes() == sb[k].tobytes() for k in sa)


def test_the_barrier_in_one_step():
    """A folded trial with the best possible data term is rejected; a folded accepted point is beaten by a worse data term."""
    sz = (9, 7, 3)
    rng = np.random.default_rng(0)
    J = rng.normal(size=(1, 60, 30))
    H, g = np.einsum("bpi,bpj->bij", J, J), rng.normal(size=(1, 30))
    mirror = O.identity_beta(1)
    mirror[0, 0, 0], mirror[1, 0, 0] = 8.0, -1.0
    beta, st = O.identity_beta(1), GJ.new_state(1)
    GJ.lm_step(st, H, g, np.array([5.0]), beta, [0], sz, mj=1.0)
    assert st["jac"][0] == 0.0 and st["min_det"][0] == 1.0
    beta[:] = mirror
    out = GJ.lm_step(st, H, g, np.array([0.0]), beta, [0], sz, mj=1.0)
    assert out["folded"][0] and not out["accept"][0] and st["counts"][0].tolist() == [0, 1, 1] and st["min_det"][0] == 1.0
    beta, st = mirror.copy(), GJ.new_state(1)
    out = GJ.lm_step(st, H, g, np.array([5.0]), beta, [0], sz, mj=1.0)                 # the first call accepts anything
    assert out["accept"][0] and st["jac"][0] == np.inf and st["min_det"][0] == -1.0
    Hp, gp = out["system"][0]
    assert Hp.tobytes() == H[0].tobytes() and gp.tobytes() == g[0].tobytes()             # non-finite rho: nothing added
    beta[:] = O.identity_beta(1)
    out = GJ.lm_step(st, H, g, np.array([500.0]), beta, [0], sz, mj=1.0)
    assert out["accept"][0] and st["jac"][0] == 0.0 and st["sse"][0] == 500.0


# ---- whole fits ------------------------------------------------------------------------------------------------------
WEIGHTS = (0.0, 1e-4, 1e-3, 1e-2)
CELLS = [(Z, L, seed) for Z in (2, 1) for L in (3, 6) for seed in (0, 1, 2)]
# measured in float64, 48 x 40 x Z, K = 6, T = 4, 16 full-order iterations from the identity: field_error (voxels) per weight
MEASURED = {
    (2, 3, 0): (2.1e-5, 0.015, 0.048, 0.043), (2, 3, 1): (19.0, 0.039, 0.031, 0.057), (2, 3, 2): (19.9, 0.076, 0.120, 0.110),
    (2, 6, 0): (81.9, 8.78, 7.03, 16.1), (2, 6, 1): (611.8, 20.6, 41.8, 48.9), (2, 6, 2): (3270.0, 16.2, 0.069, 0.259),
    (1, 3, 0): (1.1e-5, 0.0018, 0.017, 0.124), (1, 3, 1): (2.1e-5, 0.0028, 0.023, 0.104), (1, 3, 2): (7.4e-6, 0.0036, 0.031, 0.151),
    (1, 6, 0): (73.4, 52.6, 68.1, 38.8), (1, 6, 1): (52.7, 42.0, 48.6, 44.8), (1, 6, 2): (1.0e-5, 0.0099, 0.069, 0.205),
}
# cells the prior turns from divergent into converged: (cell, index of the weight)
RESCUED = [((2, 3, 1), 1), ((2, 3, 1), 2), ((2, 3, 1), 3), ((2, 3, 2), 1), ((2, 3, 2), 2), ((2, 3, 2), 3), ((2, 6, 2), 2), ((2, 6, 2), 3)]


@pytest.fixture(scope="module")
def fits():
    """Per (Z, L, seed, weight): field_error, min_det per frame, the per-frame F history and the calls' results."""
    out = {}
    for Z, L, seed in CELLS:
        sz = (48, 40, Z)
        p = GO.shifted_problem(sz, L, seed)
        T = p["C"].shape[1]
        for w in WEIGHTS:
            trace = []
            beta, st, hist = GJ.fit_gn_jac(p["A"], p["C"], O.identity_beta(T), sz, range(T), p["frames"], 16, w, trace=trace)
            out[(Z, L, seed, w)] = (GN.field_error(beta, p["beta_true"], sz), GJ.min_det(beta, sz), hist, trace, st)
    return out


def test_no_fit_folds_at_the_sample_points(fits):
    """The README's K16o problems with ``motion_jacobian`` in {0, 1e-4, 1e-3, 1e-2}; the table (field_error, smallest det Jx
    over frames and sample points) is in ``_update_motion_gn``'s docstring and the README.  By construction: from the identity
    start every frame of every cell with a weight ends with min_det > 0, and state's min_det is that of the result.  Without
    the prior six of the twelve cells end folded (min_det down to -1430)."""
    folded_without = 0
    for Z, L, seed in CELLS:
        line = []
        for w in WEIGHTS:
            err, md, hist, trace, st = fits[(Z, L, seed, w)]
            line.append(f"{w:g}: {err:.3g} / {md.min():.3g}")
            if w:
                assert (md > 0).all(), (Z, L, seed, w, md)
                np.testing.assert_allclose(st["min_det"], md, rtol=1e-12)
                assert np.isfinite(st["jac"]).all()
            else:
                folded_without += bool((md <= 0).any())
        print(f"\n48x40x{Z} L={L} seed {seed}  weight: field_error / min_det   " + "   ".join(line))
    assert folded_without >= 6


def test_what_the_prior_rescues(fits):
    """At two slices the full order leaves the basin from 3 voxels away on seeds 1 and 2 (19.0 / 19.9 voxels off, folded); with
    any of the three weights it ends 0.03 .. 0.12 voxel off.  At 6 voxels it rescues seed 2 with 1e-3 and 1e-2 (3270 -> 0.069 /
    0.26) and no other cell: those end unfolded but 7 .. 68 voxels off, and ``motion_order = 'graded'`` stays the advice for far
    starts.  Each rescued cell is asserted at half the measured gap to the fit without the prior, which is asserted above it."""
    for cell, k in RESCUED:
        without, with_prior = MEASURED[cell][0], MEASURED[cell][k]
        middle = 0.5 * (without + with_prior)
        assert fits[cell + (WEIGHTS[k],)][0] < middle, (cell, WEIGHTS[k])
        assert fits[cell + (0.0,)][0] > 5 and (fits[cell + (0.0,)][1] < 0).any(), cell       # tests/test_gn_order_host.py's bar; folded
    # (a fit that leaves the basin is chaotic: its figure, and the second digit of a rescued cell's, change with the BLAS's
    # rounding -- 3270 or 1390 voxels, 0.039 or 0.047 -- so the recorded table is not asserted cell by cell)
    # where the plain fit converges the prior costs a bias of its own: below 0.21 voxel at 1e-2, 0.07 at 1e-3, 0.01 at 1e-4
    for cell in ((2, 3, 0), (1, 3, 0), (1, 3, 1), (1, 3, 2), (1, 6, 2)):
        assert fits[cell + (0.0,)][0] < 1e-4
        for w, bound in ((1e-4, 0.02), (1e-3, 0.07), (1e-2, 0.21)):
            assert fits[cell + (w,)][0] < bound, (cell, w)


def test_invariants_of_every_fit(fits):
    for key, (err, md, hist, trace, st) in fits.items():
        if not key[3]:
            continue
        F = np.array(hist)                                                # (17, T): accepted sse + J after every call
        assert (np.diff(F, axis=0) <= 0).all(), key                       # no accepted step raises F; a rejected one keeps it
        for out in trace[1:]:
            assert not (out["folded"] & out["accept"]).any(), key         # a folded trial is never accepted after the first call
        assert not trace[0]["folded"].any()                               # the identity start
        assert (st["counts"][:, 0] + st["counts"][:, 1] == 16).all()
    assert any(out["folded"].any() for key, v in fits.items() if key[3] for out in v[3])   # the barrier was needed somewhere


def test_bias_on_a_warp_that_does_not_preserve_volume():
    """``GJ.scaled_problem``: tests/gn_restatement.py's planted warps followed by an in-plane dilation by 1.03 (det Jx 1.01 ..
    1.09 over the sample points), 3 frames, 8 iterations from the identity.  Largest distance (voxels) between the fitted and
    the true warp per frame, measured:
        24x20x1  0     0       0       0             24x20x2  0     0       0       0
        24x20x1  1e-4  0.0004  0.0006  0.0011        24x20x2  1e-4  0.019   0.044   0.036
        24x20x1  1e-3  0.0042  0.0057  0.0102        24x20x2  1e-3  0.051   0.082   0.140
        24x20x1  1e-2  0.041   0.047   0.070         24x20x2  1e-2  0.065   0.137   0.164
    (0: below 5e-5).  Two slices carry little information about d q_z / d z, so the prior moves that entry to buy det = 1."""
    want = {(24, 20, 1): {0.0: [0, 0, 0], 1e-4: [0.0004, 0.0006, 0.0011], 1e-3: [0.0042, 0.0057, 0.0102], 1e-2: [0.0407, 0.0472, 0.0704]},
            (24, 20, 2): {0.0: [0, 0, 0], 1e-4: [0.019, 0.0439, 0.0357], 1e-3: [0.0507, 0.0819, 0.1399], 1e-2: [0.0649, 0.137, 0.1644]}}
    for sz in SHAPES[::-1]:
        p = GJ.scaled_problem(sz, 1.03)
        T = p["C"].shape[1]
        true_det = GJ.min_det(p["beta_true"], sz)
        assert (true_det > 1.005).all()
        for w, rec in want[sz].items():
            beta = GJ.fit_gn_jac(p["A"], p["C"], O.identity_beta(T), sz, range(T), p["frames"], 8, w)[0]
            err = GS.frame_errors(beta, p["beta_true"], sz)
            print(f"\n{sz} weight {w:g}: per-frame error {np.round(err, 4).tolist()}, min_det {np.round(GJ.min_det(beta, sz), 4).tolist()}")
            np.testing.assert_allclose(err, rec, atol=1e-4 + 0.02 * np.max(rec))
            assert (GJ.min_det(beta, sz) > 0.9).all()


# ---- the wiring ----------------------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_entry():
    header = open(os.path.join(ROOT, "include", "dnmf_hip.h")).read()
    assert "tests/gn_jac_restatement.py" in header and "lm_step_jac_kernel" in header
    from dnmf_amd import _lib, build
    res, args = _lib.SIGNATURES["dnmf_lm_step_jac"]
    order = _lib.SIGNATURES["dnmf_lm_step_order"][1]
    i, d, vp = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    # dnmf_lm_step_order's list with X, Y, Z for Z and mj, jac, min_det before the stream
    assert res is i and args == order[:4] + [i, i, i] + order[5:-1] + [d, vp, vp, vp]
    build.build_library()
    lib = _lib.load()
    assert lib.dnmf_version() == 7 == _lib.ABI_VERSION
    buf = (ctypes.c_double * 1024)()
    p, q = ctypes.addressof(buf), ctypes.addressof(buf) + 4096
    ok = [p, p, p, 2, 9, 7, 1, 0, p, p, p, 4, p, p, p, p, p, p, p, p, 10.0, 1e-3, 1e-9, 1e9, 0, q, 1.0, p, 1.0, p, p, 0]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.dnmf_lm_step_jac(*a), lib.dnmf_last_error().decode()

    for k in (0, 1, 2, 8, 9, 10, 12, 13, 14, 15, 16, 17, 18, 19, 25, 27, 29, 30):
        rc, msg = call(**{f"a{k}": 0})
        assert rc == -1 and msg.startswith("dnmf_lm_step_jac:"), (k, rc, msg)
    for k, v in ((7, 3), (7, -1), (3, 0), (4, 1), (5, 1), (6, 0), (11, 0), (20, 1.0), (21, 0.0), (22, 0.0), (23, 1e-12), (26, -1.0),
                 (26, float("nan")), (28, -1.0), (28, float("inf")), (28, float("nan")), (25, p)):
        rc, msg = call(**{f"a{k}": v})
        assert rc == -2 and msg.startswith("dnmf_lm_step_jac:"), (k, v, rc, msg)
    # without the temporal prior its two buffers may be NULL: the next refusal is another argument's
    rc, msg = call(a26=0.0, a25=0, a27=0, a7=7)
    assert rc == -2 and "order=7" in msg


def test_ops_lm_step_takes_the_weight():
    from dnmf_amd import ops
    pl = inspect.signature(ops.lm_step).parameters
    assert pl["jacobian"].default == 0.0 and list(pl)[-1] == "order"
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lm_step.*jacobian"):
            ops.lm_step(None, None, (9, 7, 3), None, None, jacobian=bad)


def test_driver_checks_the_weight_before_anything_else():
    from dnmf_amd.Demix import dNMF
    assert "self.motion_jacobian = 0.0" in inspect.getsource(dNMF.DeformableNMF.__init__)
    assert "motion_jacobian" not in inspect.signature(dNMF.DeformableNMF.update_motion).parameters
    assert inspect.signature(dNMF.DeformableNMF.fit).parameters["motion_jacobian"].default is None
    assert dNMF.MultiChannelDNMF.fit is dNMF.DeformableNMF.fit and dNMF.MultiChannelDNMF.update_motion is dNMF.DeformableNMF.update_motion
    chk = dNMF._check_motion_jacobian
    assert chk(0, "adam", "x") == 0.0 and chk(1e-3, "gn", "x") == 1e-3
    for value, solver in ((1e-3, "adam"), (-1e-3, "gn"), (float("nan"), "gn"), (float("inf"), "gn")):
        with pytest.raises(ValueError, match="motion_jacobian"):
            chk(value, solver, "update_motion")
    # through the public calls, on a model that has neither a GPU nor a loader
    model = dNMF.DeformableNMF.__new__(dNMF.DeformableNMF)
    model.motion_smooth, model.motion_order, model.motion_jacobian = 0.0, "quadratic", 1e-3
    with pytest.raises(ValueError, match="update_motion.*motion_jacobian.*'gn' only"):
        model.update_motion(None, None)
    model.motion_jacobian = -1.0
    with pytest.raises(ValueError, match="update_motion.*motion_jacobian.*finite"):
        model.update_motion(None, None, solver='gn')
    model.motion_jacobian = 0.0
    with pytest.raises(ValueError, match="fit.*motion_jacobian.*'gn' only"):
        model.fit(None, None, None, 1, motion_jacobian=1e-3)
    with pytest.raises(ValueError, match="fit.*motion_jacobian.*finite"):
        model.fit(None, None, None, 1, motion_solver='gn', motion_jacobian=float("nan"))
    assert model.motion_jacobian == 0.0
    # the residual count the weight is scaled by is voxels x channels, the one K16s uses
    src = inspect.getsource(dNMF.DeformableNMF._update_motion_gn)
    assert "row = sum(f.P for f, _ in chans)" in src and "n_residuals=row" in src and 'step_kw["jacobian"] = jacobian' in src
