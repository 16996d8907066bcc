"""tests/iwarp_restatement.py, the float64 definition the GPU test holds K7 (``dnmf_image_iwarp``) to, pinned without a GPU:
against the oracle's fp32 positions and scipy's search, against a three-loop search where distances tie exactly, and that
every warp family is what its name says (computed from the coefficients and the positions alone).  Nothing here runs a kernel."""
import numpy as np
import pytest

import iwarp_restatement as IR
from conftest import golden
from oracle import dnmf_oracle as O


def oracle_positions(beta, sz):
    """(P, 3) fp32: the reference's flow_ of one frame (Demix/dNMF.py:54-55, 81-83) by the oracle."""
    lat = O.voxel_lattice(sz)
    _, n = O.poly_grid(O.quadratic_basis(lat), np.asarray(beta, dtype=np.float32)[:, :, None], sz)
    return O.pushforward_flow(n, sz)[..., 0].reshape(-1, 3)


def test_positions64_against_the_oracle():
    """Fixture G6 (12x10x2, eight frames) and the first two ``mixed`` warps of every full shape of the GPU test: positions64
    within DELTA0 of the oracle's fp32 ``pushforward_flow``.  Worst absolute difference delta_0 = 6.6e-5 voxels (at 20x300x1,
    where |s| passes 256 and an fp32 step is 3e-5; 1.8e-5 at 18x70x5, 1.4e-5 at 64x64x1, 1.0e-5 at 33x40x2, 3.6e-6 on G6).
    DELTA0 = 8e-5, that figure with room for another einsum order of the oracle's torch, is what the margin of the GPU test is
    made of."""
    g = golden("G6_pushforward")
    worst = {}
    d = [np.abs(oracle_positions(g["beta"][:, :, t], g["sz"]) - IR.positions64(g["beta"][:, :, t], g["sz"])).max()
         for t in range(g["beta"].shape[2])]
    worst["G6"] = float(max(d))
    for sz in IR.SHAPES:
        beta = IR.case(sz, "mixed")[1]
        worst[sz] = float(max(np.abs(oracle_positions(beta[:, :, i], sz) - IR.positions64(beta[:, :, i], sz)).max()
                              for i in range(2)))
    print("\ndelta_0 per volume:", {str(k): f"{v:.3g}" for k, v in worst.items()})
    assert max(worst.values()) <= IR.DELTA0, worst
    assert max(worst.values()) >= 0.25 * IR.DELTA0, worst          # DELTA0 is the measured size, not a loose guess


def test_positions64_identity_is_the_scaled_lattice():
    for sz in IR.SHAPES + IR.TIE_SHAPES:
        want = IR.lattice64(sz) * [sz[0] / (sz[0] - 1.0), sz[1] / (sz[1] - 1.0), sz[2] / (sz[2] - 1.0) if sz[2] > 1 else 0.0]
        np.testing.assert_allclose(IR.positions64(O.identity_beta(1)[:, :, 0], sz), want, rtol=0, atol=1e-12)
    thin = IR.positions64(O.identity_beta(1)[:, :, 0], (1, 60, 3))
    assert not np.isfinite(thin[:, 0]).any() and np.isfinite(thin[:, 1:]).all()   # 0 / 0 along the axis of one voxel


@pytest.mark.parametrize("sz", [(12, 9, 3), (30, 26, 1)])
def test_nearest64_against_scipy_on_jittered_lattices(sz):
    """No ties: scipy's choice (the oracle's ``image_iwarp``, the reference's NearestNDInterpolator) is the only one."""
    rng = np.random.default_rng(sum(sz))
    lat = O.voxel_lattice(sz)
    flow = (lat + rng.uniform(-0.4, 0.4, lat.shape) * [1, 1, sz[2] > 1]).astype(np.float32)
    P = int(np.prod(sz))
    idx, best, second = IR.nearest64(flow.reshape(-1, 3), lat.reshape(-1, 3), chunk=1000)     # (several chunks)
    assert IR.tie_share(best, second) == 0.0
    want = O.image_iwarp(np.arange(P, dtype=np.float64).reshape(sz), flow, lat.astype(np.int64))
    np.testing.assert_array_equal(idx, want.reshape(-1).astype(np.int64))
    d = ((lat.reshape(-1, 1, 3).astype(np.float64) - flow.reshape(1, -1, 3).astype(np.float64)) ** 2).sum(2)
    np.testing.assert_allclose(best, d.min(1), rtol=1e-14)
    np.testing.assert_allclose(second, np.sort(d, 1)[:, 1], rtol=1e-14)
    np.testing.assert_array_equal(IR.chosen_d2(flow.reshape(-1, 3).astype(np.float64), IR.lattice64(sz), idx), best)


def test_nearest64_torch_is_nearest64():
    import torch
    for sz, kind in (((18, 70, 5), "mixed"), ((33, 40, 2), "identity"), ((1, 60, 3), "shift")):
        p = IR.positions64(IR.case(sz, kind)[1][:, :, 0], sz)
        lat = IR.lattice64(sz)
        a = IR.nearest64(p, lat)
        b = IR.nearest64_torch(torch.from_numpy(p), torch.from_numpy(lat), chunk=100000)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y.numpy())
    assert (a[0] == 0).all() and np.isinf(a[1]).all()              # the thin volume: no finite distance, voxel 0


def test_nearest64_against_three_loops_with_exact_ties():
    """5x4x2 under the identity: every lattice point of the odd slice is exactly midway between both slices."""
    sz = (5, 4, 2)
    p = IR.positions64(O.identity_beta(1)[:, :, 0], sz)
    lat = IR.lattice64(sz)
    idx, best, second = IR.nearest64(p, lat)
    want = []
    for g in lat:
        arg, low = 0, float("inf")
        for i, s in enumerate(p):
            d = ((g[0] - s[0]) ** 2 + (g[1] - s[1]) ** 2) + (g[2] - s[2]) ** 2
            if d < low:
                arg, low = i, d
        want.append(arg)
    np.testing.assert_array_equal(idx, want)
    ties = second == best
    assert ties.sum() >= len(lat) // 2 and (idx[ties] % 2 == 0).all()     # the lower slice wins


def test_min_stretch64_of_known_maps():
    for sz in IR.SHAPES:
        one = IR.min_stretch64(O.identity_beta(1)[:, :, 0], sz)
        assert abs(one["m"] - 0.98) < 1e-8 and one["drift"] == 0.0 and abs(one["det"] - 1.0) < 1e-12
        mirror = IR.min_stretch64(IR.case(sz, "mirror")[1][:, :, 0], sz)
        assert mirror["det"] < 0 and mirror["m"] > 0.6                      # an isometry: a bound, no fold
        half = IR.min_stretch64(IR.case(sz, "bend")[1][:, :, 1], sz)
        assert abs(half["drift"] - 0.5) < 1e-5 and abs(half["smin"] - 1.0) < 1e-5


# ---- the families are what they are named for -----------------------------------------------------------------------------------
def test_the_case_table():
    ids = [IR.case_id(c) for c in IR.cases()]
    assert len(set(ids)) == len(ids) == 4 * 11 - 2 + 3 * 3
    for sz, kind in IR.cases():
        labels, beta = IR.case(sz, kind)
        assert beta.dtype == np.float32 and beta.shape == (10, 3, len(labels)) and np.isfinite(beta).all()
        if sz[2] == 1:
            np.testing.assert_array_equal(beta[:, 2], O.identity_beta(len(labels))[:, 2])
        assert int(np.prod(sz)) <= 6300
    assert len(IR.case((64, 64, 1), "shift")[0]) == 13 and len(IR.case((18, 70, 5), "shift")[0]) == 19


@pytest.mark.parametrize("sz", IR.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_families_reach_what_they_are_named_for(sz):
    lat = IR.lattice64(sz)
    axes = [0, 1]
    # zoom 0.7: a band of lattice points outside the hull of the positions, on every side of x and y
    p = IR.positions64(IR.case(sz, "zoom")[1][:, :, 0], sz)
    for d in axes:
        assert p[:, d].min() > 1.0 and p[:, d].max() < sz[d] - 2.0, (d, p[:, d].min(), p[:, d].max())
    # the shift of 12.4 voxels along +y (on its rotation of 8 degrees): the lattice rows 0 .. 8 lose their pre-image at every x, at
    # Z = 1 nine or more neighbouring lanes of a wave (IW_SHARE = 8)
    labels, beta = IR.case(sz, "shift")
    p = IR.positions64(beta[:, :, labels.index("shift y+12.4")], sz)
    assert p[:, 1].min() > 8.0
    pure = beta[:, :, labels.index("shift y+3.7")].astype(np.float64)
    np.testing.assert_allclose(pure[1:], O.identity_beta(1)[1:, :, 0], atol=1e-7)
    # fold: the determinant is negative at the centre and changes sign inside the volume; the kernel has no bound
    fold = IR.case(sz, "fold")[1][:, :, 0]
    st = IR.min_stretch64(fold, sz)
    assert st["det"] < 0 and st["m"] < 0
    px = IR.positions64(fold, sz)[:, 0].reshape(sz)
    steps = np.diff(px, axis=0)
    assert (steps < 0).any() and (steps > 0).any()
    # nearfold: the pair straddles the threshold, by 5 % each way
    pair = [IR.min_stretch64(IR.case(sz, "nearfold")[1][:, :, i], sz)["m"] for i in range(2)]
    assert 1.04 * IR.GIVE_UP < pair[0] < 1.06 * IR.GIVE_UP and 0.94 * IR.GIVE_UP < pair[1] < 0.96 * IR.GIVE_UP, pair
    # ... and lattice points within 0.03 voxels of a warped voxel exist (the ones a box still serves above the threshold)
    best = IR.nearest64(IR.positions64(IR.case(sz, "nearfold")[1][:, :, 0], sz), lat)[1]
    assert (np.sqrt(best) < 0.03).sum() >= 4
    # bend: the largest just below the amplitude at which the kernel gives up, the smallest mild
    m = [IR.min_stretch64(IR.case(sz, "bend")[1][:, :, i], sz)["m"] for i in range(3)]
    assert m[0] > 0.9 and IR.GIVE_UP < m[2] < 3 * IR.GIVE_UP, m
    # rotate / shear / tilt: the Jacobian at the centre
    for i, deg in enumerate((2.0, 10.0, 30.0)):
        b = IR.case(sz, "rotate")[1][:, :, i].astype(np.float64)
        np.testing.assert_allclose(b[1:3, :2].T, IR.rot_z(deg)[:2, :2], atol=1e-6)
    assert abs(IR.case(sz, "shear")[1][2, 0, 0] - 0.2) < 1e-6
    if sz[2] > 1:
        t = IR.case(sz, "tilt")[1][:, :, 0]
        assert abs(t[1, 2] - 0.02) < 1e-6 and abs(t[2, 2] + 0.015) < 1e-6 and abs(t[3, 0] - 0.3) < 1e-6


@pytest.mark.parametrize("c", IR.cases(), ids=IR.case_id)
def test_near_ties_stay_below_the_cap(c):
    """The condition on the inputs of check (a) of the GPU test: in every frame of every case but ``identity`` fewer than 1 %
    of the lattice points have their two best distances (on positions64) within 1e-6.  (The two nearest by a k-d tree: the
    same two distances as the brute force, which the GPU test uses.)"""
    from scipy.spatial import cKDTree
    sz, kind = c
    labels, beta = IR.case(sz, kind)
    lat = IR.lattice64(sz)
    for i, label in enumerate(labels):
        p = IR.positions64(beta[:, :, i], sz)
        if not np.isfinite(p).all():
            assert sz in IR.THIN                                   # no finite distance at all: no tie (tie_share)
            continue
        d = cKDTree(p).query(lat, k=2)[0] ** 2
        share = IR.tie_share(d[:, 0], d[:, 1])
        if kind == "identity":
            assert share >= (0.5 if sz[2] == 2 else 0.0)           # the designed tie case
        else:
            assert share <= IR.TIE_CAP, (label, share)


def test_exact_tie_cases_tie_exactly():
    for sz in IR.TIE_SHAPES:
        labels, beta = IR.tie_case(sz)
        lat = IR.lattice64(sz)
        for i in range(len(labels)):
            p = IR.positions64(beta[:, :, i], sz)
            np.testing.assert_array_equal(p, p.astype(np.float32).astype(np.float64))    # exact in fp32
            idx, best, second = IR.nearest64(p, lat)
            if i == 0:                                                    # the identity: every axis of 2 ties
                assert (best == second).sum() >= len(lat) // 2, (sz, labels[i])
    # 2x17x2 under the identity: x and z both put the odd plane midway -- four voxels at the same distance
    sz = (2, 17, 2)
    p = IR.positions64(IR.tie_case(sz)[1][:, :, 0], sz)
    d = ((IR.lattice64(sz)[:, None, :] - p[None, :, :]) ** 2).sum(2)
    assert ((d == d.min(1, keepdims=True)).sum(1) >= 4).any()


def test_many_frames_case():
    beta = IR.many_frames_case()
    assert beta.shape == (10, 3, 70)
    for b in range(70):
        m = IR.min_stretch64(beta[:, :, b], IR.MANY_SZ)["m"]
        assert (m < 0) == (b in IR.MANY_FOLDS) and (m < 0 or m > 0.75)
