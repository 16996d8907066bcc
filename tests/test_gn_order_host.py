"""The Gauss-Newton motion step for one warp order and the graded schedule (K16o) without a GPU: the float64 definition
(tests/gn_order_restatement.py) against tests/gn_restatement.py, what the schedule reaches and the full order does not, and the
wiring of every layer."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import gn_order_restatement as GO
import gn_restatement as GN
import gn_smooth_restatement as GS
from oracle import dnmf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FROZEN = {"translation": list(range(1, 10)), "affine": list(range(4, 10)), "quadratic": []}


def test_active_sets():
    for sz, counts in (((9, 7, 3), (3, 12, 30)), ((9, 7, 1), (2, 6, 12))):
        sets = [GO.active(sz, o) for o in GO.GRADED]
        assert tuple(len(s) for s in sets) == counts
        np.testing.assert_array_equal(sets[2], GN.active(sz))
        for s in sets:                                                   # each a leading part of the full list
            np.testing.assert_array_equal(s, GN.active(sz)[:len(s)])
    assert GO.active((9, 7, 3), "translation").tolist() == [0, 1, 2] and GO.active((9, 7, 1), "translation").tolist() == [0, 1]
    assert GO.active((9, 7, 1), "affine").tolist() == [0, 1, 3, 4, 6, 7]
    # M maps a centred term to raw rows of its degree or lower: what keeps the rows above the order out of d beta
    for sz in ((9, 7, 3), (9, 7, 1)):
        M, deg = GN.change_of_basis(sz), GN.EXPO.sum(1)
        assert not M[deg[:, None] > deg[None, :]].any()


def bookkeeping_calls():
    """The hand-made two-frame state of tests/test_gn_host.py::test_lm_step_bookkeeping: its inputs, call by call."""
    rng = np.random.default_rng(1)
    J = rng.normal(size=(2, 50, 30))
    H = np.einsum("bpi,bpj->bij", J, J)
    g = rng.normal(size=(2, 30))
    nan = np.nan
    return [(H, g, [5.0, 7.0], False), (2 * H, g, [4.0, 7.5], False), (H, g, [nan, 6.0], True)] + [(H, g, [nan, nan], False)] * 14


def test_quadratic_is_the_existing_definition():
    sz, times = (9, 7, 3), [3, 1]
    ba, bb, sa, sb = O.identity_beta(4), O.identity_beta(4), GN.new_state(2), GN.new_state(2)
    for H, g, sse, last in bookkeeping_calls():
        a = GN.lm_step(sa, H, g, np.array(sse), ba, times, sz, accept_only=last)
        b = GO.lm_step(sb, H, g, np.array(sse), bb, times, sz, "quadratic", accept_only=last)
        np.testing.assert_array_equal(a["accept"], b["accept"])
        np.testing.assert_array_equal(a["dbeta"], b["dbeta"])
        np.testing.assert_array_equal(ba, bb)
        for k in sa:
            np.testing.assert_array_equal(sa[k], sb[k])
    assert (sb["lam"] == 1e9).all() and sb["counts"][:, 2].tolist() == [1, 1]


@pytest.mark.parametrize("sz", [(9, 7, 3), (9, 7, 1)])
@pytest.mark.parametrize("order", ["translation", "affine"])
def test_lower_orders_move_their_rows_only(sz, order):
    """On the same calls: the bookkeeping is the full order's, and only rows 0 (translation) / 0 .. 3 (affine) of the trial and
    of the accepted coefficients ever differ from the start -- a start with signed zeros and odd values in the frozen rows."""
    times = [3, 1]
    start = O.identity_beta(4)
    start[4:, :, :] = np.random.default_rng(2).normal(size=(6, 3, 4)).astype(np.float32) * 1e-3
    start[5, 1, :] = -0.0
    beta, st, full, sf = start.copy(), GN.new_state(2), start.copy(), GN.new_state(2)
    frozen, free = FROZEN[order], [r for r in range(10) if r not in FROZEN[order]]
    moved = False
    for n, (H, g, sse, last) in enumerate(bookkeeping_calls()[:4]):
        out = GO.lm_step(st, H, g, np.array(sse), beta, times, sz, order, accept_only=last)
        GN.lm_step(sf, H, g, np.array(sse), full, times, sz, accept_only=last)
        for k in ("counts", "lam", "sse", "sse0"):                       # decisions depend on sse alone
            np.testing.assert_array_equal(st[k], sf[k])
        assert beta[frozen].tobytes() == start[frozen].tobytes()         # bits, the sign of a zero included
        assert st["beta"].reshape(2, 10, 3)[:, frozen].tobytes() == np.moveaxis(start[frozen][:, :, times], 2, 0).tobytes()
        assert not out["dbeta"][:, frozen].any()
        np.testing.assert_array_equal(beta[:, :, [0, 2]], start[:, :, [0, 2]])
        if sz[2] == 1:                                                   # the z rows and the z component stay out
            assert beta[3].tobytes() == start[3].tobytes() and beta[:, 2].tobytes() == start[:, 2].tobytes()
        moved = moved or (beta[free][:, :, times] != start[free][:, :, times]).any()
        # the restricted system is the full one's leading block with its own scaling
        act = GO.active(sz, order)
        Ah, rh, sc = GO.damped_system(st["H"][0], st["g"][0], st["lam"][0], act)
        np.testing.assert_allclose(np.diag(Ah), 1.0, rtol=1e-14)
        assert Ah.shape == (len(act), len(act))
    assert moved


def test_prior_acts_on_the_selected_rows_only():
    sz = (9, 7, 3)
    rng = np.random.default_rng(0)
    J = rng.normal(size=(1, 60, 30))
    H, g = np.einsum("bpi,bpj->bij", J, J), rng.normal(size=(1, 30))
    beta = (O.identity_beta(3) + rng.normal(size=(10, 3, 3)) * 1e-2).astype(np.float32)
    m, Mc = 2.5, GN.change_of_basis(sz)
    for order in GO.GRADED:
        ref, trial, st = beta.copy(), beta.copy(), GS.new_state(1)
        # the neighbours' CENTRED rows above the order: any value (their raw rows do enter theta's selected rows).  ref2 is
        # rounded to fp32 again, which moves the selected theta by ~1e-6 voxel
        ref2 = (ref + (0.5 * Mc[:, FROZEN[order]].sum(1))[:, None, None]).astype(np.float32)
        a = GO.lm_step(st, H, g, np.array([5.0]), trial, [1], sz, order, m=m, beta_ref=ref)
        trial2, st2 = beta.copy(), GS.new_state(1)
        b = GO.lm_step(st2, H, g, np.array([5.0]), trial2, [1], sz, order, m=m, beta_ref=ref2)
        np.testing.assert_allclose(a["dbeta"], b["dbeta"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(st["prior"][0], st2["prior"][0], rtol=1e-3)
        assert st["prior"][0] > 0 and (order == "quadratic" or np.abs(ref2 - ref).max() > 0.4)
        act = GO.active(sz, order)
        th = [GO.theta(beta[:, :, t], sz, order) for t in range(3)]
        np.testing.assert_allclose(st["prior"][0], m * (((th[1] - th[0]) ** 2).sum() + ((th[1] - th[2]) ** 2).sum()), rtol=1e-14)
        assert not np.delete(th[1], act).any() and th[1][act].all()
    # all rows selected: tests/gn_smooth_restatement.py's step
    ref, trial, st = beta.copy(), beta.copy(), GS.new_state(1)
    GS.lm_step_smooth(st, H, g, np.array([5.0]), trial, ref, [1], sz, m)
    np.testing.assert_array_equal(trial, trial2)
    assert st["prior"][0] == st2["prior"][0]


# ---- the schedule on warps several voxels away -----------------------------------------------------------------------
SZ2, SZ1 = (48, 40, 2), (48, 40, 1)
CASES = [(SZ2, 6, 0), (SZ2, 6, 1), (SZ2, 6, 2), (SZ2, 3, 0), (SZ2, 3, 1), (SZ2, 3, 2), (SZ1, 6, 2)]


@pytest.fixture(scope="module")
def fits():
    """Per (sz, L, seed): field_error of 16 full-order iterations and of translation 6 + affine 6 + quadratic 6 from the
    identity, the graded fit's stage states and sse history."""
    out = {}
    for sz, L, seed in CASES:
        p = GO.shifted_problem(sz, L, seed)
        T = p["C"].shape[1]
        full = GN.fit_gn(p["A"], p["C"], O.identity_beta(T), sz, range(T), p["frames"], iters=16)[0]
        beta, states, hist = GO.fit_gn_schedule(p["A"], p["C"], O.identity_beta(T), sz, range(T), p["frames"], GO.schedule_of("graded", 6))
        out[(sz, L, seed)] = (GN.field_error(full, p["beta_true"], sz), GN.field_error(beta, p["beta_true"], sz), states, hist)
    return out


def test_graded_schedule_reaches_six_voxels_and_the_full_order_does_not(fits):
    """48 x 40 x 2, K = 6, T = 4, a shift of length L in a random in-plane direction per frame on top of affine 0.02 and
    quadratic 0.25 voxel, identity start.  Measured field_error (voxels), full order 16 iterations / graded 6 + 6 + 6:
      L = 6  seed 0: 81.9 / 1.3e-5   seed 1: 611.8 / 3.0e-5   seed 2: 3270 / 2.0e-5
      L = 3  seed 0: 2.1e-5 / 1.2e-5   seed 1: 19.0 / 2.8e-5   seed 2: 19.9 / 1.0e-5
    At L = 3 the full order is asserted for seed 0 only: on seeds 1 and 2 it leaves the basin at 3 voxels already (figures
    above), the schedule does not."""
    for seed in (0, 1, 2):
        full, graded, _, _ = fits[(SZ2, 6, seed)]
        print(f"\nL=6 seed {seed}: full order {full:.4g}, graded {graded:.4g}")
        assert graded < 0.01
        if seed < 2:
            assert full > 5
    for seed in (0, 1, 2):
        full, graded, _, _ = fits[(SZ2, 3, seed)]
        print(f"L=3 seed {seed}: full order {full:.4g}, graded {graded:.4g}")
        assert graded < 0.01
    assert fits[(SZ2, 3, 0)][0] < 0.01


def test_graded_schedule_at_one_slice(fits):
    """48 x 40 x 1, L = 6: seed 2 only.  On seeds 0 and 1 both solvers fail: measured field_error 73.4 / 52.7 voxels for the full
    order and 32.1 / 71.5 for the schedule (its translation stage does not get near enough at one slice); seed 2 ends 1.0e-5 /
    1.1e-5."""
    full, graded, _, _ = fits[(SZ1, 6, 2)]
    print(f"\n48x40x1 L=6 seed 2: full order {full:.4g}, graded {graded:.4g}")
    assert graded < 0.01


def test_every_stage_descends_from_where_the_last_one_ended(fits):
    for key in ((SZ2, 6, 0), (SZ1, 6, 2)):
        _, _, states, hist = fits[key]
        assert len(states) == 3 and len(hist) == 3 * 7
        assert all((b <= a).all() for a, b in zip(hist, hist[1:]))      # across the stage boundaries too
        for a, b in zip(states, states[1:]):
            np.testing.assert_array_equal(b["sse0"], a["sse"])           # a stage's first evaluation is the last one's result
        ident = O.identity_beta(4)
        np.testing.assert_array_equal(states[0]["beta"].reshape(4, 10, 3)[:, 1:], np.moveaxis(ident, 2, 0)[:, 1:])
        np.testing.assert_array_equal(states[1]["beta"].reshape(4, 10, 3)[:, 4:], np.moveaxis(ident, 2, 0)[:, 4:])


def test_schedule_of():
    assert GO.schedule_of("graded", 6) == [("translation", 6), ("affine", 6), ("quadratic", 6)]
    assert GO.schedule_of("affine", 4) == [("affine", 4)]
    assert GO.schedule_of([("translation", 2), ("quadratic", 5)], 9) == [("translation", 2), ("quadratic", 5)]


# ---- the wiring ----------------------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_entry():
    header = open(os.path.join(ROOT, "include", "dnmf_hip.h")).read()
    assert "tests/gn_order_restatement.py" in header and "csrc/motion_gn.hip" in header
    from dnmf_amd import _lib, build
    res, args = _lib.SIGNATURES["dnmf_lm_step_order"]
    smooth = _lib.SIGNATURES["dnmf_lm_step_smooth"][1]
    assert res is ctypes.c_int and args[:5] == smooth[:5] and args[5] is ctypes.c_int and args[6:] == smooth[5:]   # order after Z
    build.build_library()
    lib = _lib.load()
    assert lib.dnmf_version() == 7 == _lib.ABI_VERSION
    buf = (ctypes.c_double * 1024)()
    p, q = ctypes.addressof(buf), ctypes.addressof(buf) + 4096
    ok = [p, p, p, 2, 1, 0, p, p, p, 4, p, p, p, p, p, p, p, p, 10.0, 1e-3, 1e-9, 1e9, 0, q, 1.0, p, 0]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.dnmf_lm_step_order(*a), lib.dnmf_last_error().decode()

    for i in (0, 1, 2, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 23, 25):
        rc, msg = call(**{f"a{i}": 0})
        assert rc == -1 and msg.startswith("dnmf_lm_step_order:"), (i, rc, msg)
    for i, v in ((5, 3), (5, -1), (3, 0), (4, 0), (9, 0), (18, 1.0), (19, 0.0), (20, 0.0), (21, 1e-12), (24, -1.0), (24, float("nan")),
                 (23, p)):
        rc, msg = call(**{f"a{i}": v})
        assert rc == -2 and msg.startswith("dnmf_lm_step_order:"), (i, v, rc, msg)
    assert "order=3" in call(a5=3)[1]
    # without the prior its three buffers may be NULL: the next refusal is another argument's
    rc, msg = call(a24=0.0, a7=0, a23=0, a25=0, a5=7)
    assert rc == -2 and "order=7" in msg


def test_ops_lm_step_takes_the_order():
    from dnmf_amd import ops
    pl = inspect.signature(ops.lm_step).parameters
    assert list(pl)[-1] == "order" and pl["order"].default == "quadratic"
    assert ops.WARP_ORDERS == GO.ORDERS
    with pytest.raises(ValueError, match="lm_step.*cubic"):
        ops.lm_step(None, None, (9, 7, 3), None, None, order="cubic")
    for sz in ((9, 7, 3), (9, 7, 1)):                                    # the rows the other layers free for an order
        for order in GO.GRADED:
            assert sorted({int(i) // 3 for i in GO.active(sz, order)}) == ops.warp_free_rows(sz, order)


def test_driver_checks_the_order_before_anything_else():
    from dnmf_amd.Demix import dNMF
    assert "self.motion_order = 'quadratic'" in inspect.getsource(dNMF.DeformableNMF.__init__)
    assert "motion_order" not in inspect.signature(dNMF.DeformableNMF.update_motion).parameters
    params = inspect.signature(dNMF.DeformableNMF.fit).parameters
    assert list(params)[-1] == "motion_order" and params["motion_order"].default is None
    assert dNMF.MultiChannelDNMF.fit is dNMF.DeformableNMF.fit
    chk = dNMF._check_motion_order
    for name in ("translation", "affine", "quadratic", "graded"):
        assert chk(name, "gn", "x") == name
    assert chk("quadratic", "adam", "x") == "quadratic"
    assert chk([("translation", 3), ["quadratic", np.int64(5)]], "gn", "x") == (("translation", 3), ("quadratic", 5))
    assert chk((("affine", 0),), "gn", "x") == (("affine", 0),)
    bad = ["cubic", "", None, 2, [], [("cubic", 3)], [("affine", -1)], [("affine", 1.5)], [("affine",)], ["affine"], [("affine", "x")]]
    for value in bad:
        with pytest.raises(ValueError, match="motion_order"):
            chk(value, "gn", "update_motion")
    for value in ("translation", "graded", [("quadratic", 3)]):
        with pytest.raises(ValueError, match="motion_order.*'gn' only"):
            chk(value, "adam", "update_motion")
    # through the public calls, on a model that has neither a GPU nor a loader
    model = dNMF.DeformableNMF.__new__(dNMF.DeformableNMF)
    model.motion_smooth, model.motion_order = 0.0, "cubic"
    with pytest.raises(ValueError, match="update_motion.*motion_order.*cubic"):
        model.update_motion(None, None, solver='gn')
    model.motion_order = "graded"
    with pytest.raises(ValueError, match="update_motion.*motion_order.*'gn' only"):
        model.update_motion(None, None)
    model.motion_order = "quadratic"
    with pytest.raises(ValueError, match="fit.*motion_order.*'gn' only"):
        model.fit(None, None, None, 1, motion_order="affine")
    with pytest.raises(ValueError, match="fit.*motion_order.*cubic"):
        model.fit(None, None, None, 1, motion_solver='gn', motion_order="cubic")
    assert model.motion_order == "quadratic"
