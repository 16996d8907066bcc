"""tests/forward_restatement.py, the float64 definitions the GPU test holds ``dnmf_recon_image``, K1 and ``dnmf_render_frames``
to, pinned without a GPU: against the oracle and the committed fixtures, that the case tables reach what they claim (computed
from the tables alone), and that every case tells a deliberately wrong kernel from the right one by at least ten bounds.
Nothing here runs a kernel."""
import numpy as np
import pytest

import forward_restatement as FR
import k2_restatement as K2R
from conftest import golden
from oracle import dnmf_oracle as O


# ---- agreement with what the project already trusts ---------------------------------------------------------------------------
def test_k1_and_recon_against_the_oracle_and_fixture_G2():
    """Fixture G2 (grid, A_t, A_tC of the reference's forward): the float64 A_t and A_tC = sum_k A_t[k] C[k, t] at the
    fixture's tolerances (2e-7, 5e-7: its fp32 blend against ours in float64); the fp32 grid of the fixture, which the oracle
    reproduces bit for bit, within the grid bound of the restatement."""
    g = golden("G2_forward")
    sz = tuple(int(s) for s in g["sz"])
    times = g["times"].tolist()
    A = O.gaussian_footprints(sz, g["positions"], np.full(3, 3.0))
    ref = FR.warp_gather(A, g["beta"], sz, times)
    A_tC, A_t, n, _ = O.forward(A, O.quadratic_basis(O.voxel_lattice(sz)), g["beta"], sz, times, g["C"])
    np.testing.assert_array_equal(n, g["grid"])
    for fp32_grid in (n, g["grid"]):
        ratio, idx, zeros_ok = FR.worst(np.abs(fp32_grid.astype(np.float64) - ref["grid"]), ref["tol_grid"])
        assert zeros_ok and ratio <= 1.0, (idx, ratio)
    for want in (A_t, g["A_t"]):
        np.testing.assert_allclose(ref["A_t"], want, rtol=0, atol=2e-7)
    mine = np.stack([FR.recon(np.moveaxis(ref["A_t"][b], 0, -1), g["C"], [t])[0].reshape(sz) for b, t in enumerate(times)])
    for want in (A_tC, g["A_tC"]):
        np.testing.assert_allclose(mine, want, rtol=0, atol=5e-7)
    print(f"\nG2: fp32 grid within {ratio:.3g} of the grid bound")


def test_k1_against_the_oracle_on_a_test_case():
    """The thin case of the GPU test itself: the oracle's fp32 A_t within the per-channel bound, its grid within the grid bound."""
    sz = (9, 7, 5)
    c = FR.k1_case(sz)
    ref, _ = FR.k1_reference(sz)
    _, A_t, n, _ = O.forward(c["A"], O.quadratic_basis(O.voxel_lattice(sz)), c["beta"], sz, c["times"], np.zeros((5, 8), np.float32))
    err = np.abs(A_t.astype(np.float64) - ref["A_t"]).reshape(len(c["times"]), 5, -1).max(-1)
    ra, _, _ = FR.worst(err, ref["tol_A"])
    rg, _, zeros_ok = FR.worst(np.abs(n.astype(np.float64) - ref["grid"]), ref["tol_grid"])
    print(f"\n(9, 7, 5): oracle A_t {ra:.3g} of its bound, grid {rg:.3g}")
    assert ra <= 1.0 and rg <= 1.0 and zeros_ok


@pytest.mark.parametrize("name", ["19x23x1-K3-t0", "9x7x5-K3-t4"])
def test_render_against_the_oracle(name):
    """oracle.render_video on the same positions and traces without noise: the restatement after the simulator's
    normalisation (v / sum v^2, then / max) at fixture G8's tolerance."""
    c = FR.render_case(name)
    (video, _), _ = FR.render_reference(name)
    T = video.shape[0]
    sl = slice(c["t0"], c["t0"] + T)
    want = O.render_video(c["positions"][:, :, sl], c["traces"][:, sl], c["sz"], c["shape_std"], np.zeros(c["sz"] + (T,), np.float32))
    v = np.moveaxis(video.reshape((T,) + c["sz"]), 0, -1)
    v = v / (v ** 2).sum(dtype=np.float32)
    np.testing.assert_allclose(v / v.max(), want, rtol=2e-6, atol=1e-9)


# ---- reach --------------------------------------------------------------------------------------------------------------------
def test_recon_tables_reach_every_edge():
    cases = FR.CASES_RECON
    assert [FR.padded_k(K) for K in FR.RECON_K] == [16, 16, 32, 32, 48, 48, 64, 64, 80, 80, 96, 96, 112, 112, 128, 128]
    for Kp in range(16, 129, 16):                                  # both ends of every padded width, in both frame forms
        lo, hi = max(1, Kp - 16), Kp - 1
        assert FR.padded_k(lo) == Kp == FR.padded_k(hi) and FR.padded_k(hi + 1) == Kp + 16 and (lo == 1 or FR.padded_k(lo - 1) == Kp - 16)
        for K in (lo, hi):
            mine = [c for c in cases if c[1] == K]
            assert any(c[2] <= 16 for c in mine) and any(c[2] > 16 for c in mine), K
            assert len({c[0] for c in mine}) >= 2
    assert FR.padded_k(127) == 128 and FR.padded_k(128) > 128
    Bs = {c[2] for c in cases}
    assert {16, 17, 64, 65} <= Bs and min(Bs) == 1
    for sz in FR.RECON_VOLUMES:                                    # every volume at two K and every B
        mine = [c for c in cases if c[0] == sz]
        assert len({c[1] for c in mine}) >= 2 and {c[2] for c in mine} >= set(FR.RECON_B)
    P = lambda c: int(np.prod(c[0]))
    assert [int(np.prod(s)) for s in FR.RECON_VOLUMES] == [15, 16, 17, 1024, 1025, 315, 2046, 4095, 4096, 4097]
    small, large = [c for c in cases if c[2] <= 16], [c for c in cases if c[2] > 16]
    for group, block in ((small, 1024), (large, 4096)):            # a block is 4 waves of 16 | 64 groups of 16 voxels
        assert {block, block + 1} <= {P(c) for c in group}
        assert any(P(c) < 16 for c in group) and any(P(c) % 16 for c in group) and any(P(c) % 16 == 0 for c in group)
    for K in FR.RECON_K:                                           # every K meets a ragged last group
        assert all(P(c) % 16 for c in FR.SWEEP_K[K])
    for sz, K, B in cases:                                         # the one-hot family names every channel
        calls = FR.recon_case(sz, K, B, "onehot")["calls"]
        assert {t for c in calls for t in c} == set(range(K)) and all(len(c) == B for c in calls)
        tt, = FR.recon_case(sz, K, B, "random")["calls"]
        assert len(tt) == B and (B < 2 or (len(set(tt)) == B - 1 and tt != sorted(tt) or B == 2)) and max(tt) < B + 3
    assert FR.CHUNK_CASE[2] > 32768 + 1
    assert [[min(FR.GROUP, K - s) for s in range(0, K, FR.GROUP)] for K in FR.GROUPED_K] == [[112, 16], [112, 18], [112, 112, 1]]
    assert min(FR.GROUPED_B) <= 16 < max(FR.GROUPED_B)


def test_k1_and_render_tables_reach_every_edge():
    Ps = [int(np.prod(s)) for s in FR.CASES_K1]
    assert all(p > 256 and p % 256 for p in Ps) and {1, 2, 3, 5} == {s[2] for s in FR.CASES_K1}
    assert all(s[0] > 1 and s[1] > 1 for s in FR.CASES_K1)
    c = FR.k1_case((9, 7, 5))
    tt = c["times"]
    assert K2R.UNUSED not in tt and tt != sorted(tt) and len(set(tt)) == 7 and tt[FR.K1_REPEAT[0]] == tt[FR.K1_REPEAT[1]]
    assert np.abs(c["beta"][:, :, K2R.UNUSED]).max() >= 1e5
    Ks = {v[1] for v in FR.CASES_RENDER.values()}
    assert min(Ks) <= 256 < max(Ks) <= 2048 < FR.RENDER_REFUSED_K
    assert {(v[2], v[3]) for v in FR.CASES_RENDER.values()} == set(FR.WINDOWS)
    assert {v[0] for v in FR.CASES_RENDER.values()} == {(19, 23, 1), (9, 7, 5)}
    for name in FR.CASES_RENDER:
        c = FR.render_case(name)
        p, ext = c["positions"].astype(np.float64), np.array(c["sz"])[None, :, None]
        inside = ((p >= 0) & (p <= ext - 1)).all(1)
        far = (np.abs(p) > 5e3).any(1)
        assert inside.any() and far.any() and (~inside & ~far).any(), name
        assert c["traces"].dtype == np.float64 and c["positions"].dtype == np.float32


# ---- discrimination -----------------------------------------------------------------------------------------------------------
def far_off(err, bound):
    """Some entry is off by at least ten bounds (a zero bound: by anything at all)."""
    return bool(((err >= 10.0 * bound) & (err > 0)).any())


@pytest.mark.parametrize("group", [f"K{K}" for K in FR.SWEEP_K] + ["x".join(map(str, sz)) for sz in FR.SWEEP_VOLUME])
def test_recon_cases_tell_a_wrong_kernel(group):
    cases = FR.SWEEP_K[int(group[1:])] if group.startswith("K") else FR.SWEEP_VOLUME[tuple(int(s) for s in group.split("x"))]
    for sz, K, B in cases:
        for family in FR.FAMILIES:
            c = FR.recon_case(sz, K, B, family)
            seen = {w: False for w in ("swap", "slot", "row")}
            for times in c["calls"]:
                S, ab = FR.recon(c["A"], c["C"], times)
                bound = np.zeros_like(ab) if c["exact"] else FR.recon_tol(K, ab)
                if c["exact"]:
                    assert np.array_equal(S.astype(np.float32).astype(np.float64), S)          # fp32 holds it exactly
                for w in seen:
                    seen[w] |= far_off(np.abs(FR.recon_wrong(c["A"], c["C"], times, K, w) - S), bound)
            assert all(seen.values()), (sz, K, B, family, seen)


def test_recon_grouped_bound_and_discrimination():
    """K > 127: the grouped sum is the plain product; its bound is below twice the single-launch one would be; a swap of two
    channels across the group boundary is seen."""
    rng = np.random.default_rng(3)
    for K in FR.GROUPED_K:
        A, C = rng.uniform(-1, 1, (50, K)).astype(np.float32), rng.uniform(-1, 1, (K, 4)).astype(np.float32)
        S, bound = FR.recon_grouped(A, C, [2, 0, 3])
        S1, ab = FR.recon(A, C, [2, 0, 3])
        np.testing.assert_allclose(S, S1, rtol=0, atol=1e-12)
        assert (bound <= (FR.padded_k(FR.GROUP) + 4) * FR.U * ab).all() and (bound > 0).all()
        A2 = A.copy()
        A2[:, [0, K - 1]] = A2[:, [K - 1, 0]]
        assert far_off(np.abs(FR.recon(A2, C, [2, 0, 3])[0] - S), bound)


@pytest.mark.parametrize("sz", FR.CASES_K1, ids=lambda s: "x".join(map(str, s)))
def test_k1_cases_tell_a_wrong_kernel(sz):
    """``times`` taken in sorted order: A_t and grid off by ten bounds; the x and y components of the grid exchanged: grid."""
    c = FR.k1_case(sz)
    ref, _ = FR.k1_reference(sz)
    order = np.argsort(np.array(c["times"]), kind="stable")
    assert far_off(np.abs(ref["A_t"][order] - ref["A_t"]).reshape(len(order), 5, -1).max(-1), ref["tol_A"])
    assert far_off(np.abs(ref["grid"][..., order] - ref["grid"]), ref["tol_grid"])
    assert far_off(np.abs(ref["grid"][..., [1, 0, 2], :] - ref["grid"]), ref["tol_grid"])
    a, b = FR.K1_REPEAT
    assert np.array_equal(ref["A_t"][a], ref["A_t"][b]) and np.array_equal(ref["grid"][..., a], ref["grid"][..., b])
    assert (ref["A_t"].reshape(len(order), 5, -1).max(-1) > 0).any(0).all()           # every footprint is seen in some frame


@pytest.mark.parametrize("name", list(FR.CASES_RENDER))
def test_render_cases_tell_a_wrong_kernel(name):
    """Neuron 0 (always inside the volume) dropped: off by ten bounds.  The two 1e30 cases: the cut-off of an amplitude of 1
    (what a cut-off from the largest signed trace gives at -1e30) drops terms worth ten bounds and more, and the frame of
    the large amplitude has no voxel without a term."""
    c = FR.render_case(name)
    (video, ab), _ = FR.render_reference(name)
    bound = FR.render_tol(c["positions"].shape[0], ab)
    K = c["positions"].shape[0]
    wrong, _ = FR.render(c["positions"], c["traces"], c["sz"], c["shape_std"], c["t0"], c["T"], order=range(1, K))
    assert far_off(np.abs(wrong.astype(np.float64) - video), bound)
    if name.startswith("amp"):
        amp = np.abs(c["traces"]).max()
        assert amp == 1e30 and FR.render_cut(3.0, 1.0) < 630 and 1040 < FR.render_cut(3.0, amp) < 1050
        full, _ = FR.render(c["positions"], c["traces"], c["sz"], c["shape_std"], c["t0"], c["T"], r2_cut=FR.render_cut(3.0, amp))
        assert np.array_equal(full, video)                          # the widened cut-off drops nothing that fp32 holds
        cut, _ = FR.render(c["positions"], c["traces"], c["sz"], c["shape_std"], c["t0"], c["T"], r2_cut=FR.render_cut(3.0, 1.0))
        err = np.abs(cut.astype(np.float64) - video)
        assert far_off(err[FR.BIG_FRAME], bound[FR.BIG_FRAME]) and (ab[FR.BIG_FRAME] > 0).all()
        assert np.array_equal(np.delete(cut, FR.BIG_FRAME, 0), np.delete(video, FR.BIG_FRAME, 0))


def test_render_order_matters_at_k300():
    """The fp32 sum is taken in neuron order: the reverse order gives other bits in some entries (what a bit-equal share near 1
    on the GPU then says about the kernel's order), yet stays inside the bound."""
    name = "19x23x1-K300-t4"
    c = FR.render_case(name)
    (video, ab), _ = FR.render_reference(name)
    rev, _ = FR.render(c["positions"], c["traces"], c["sz"], c["shape_std"], c["t0"], c["T"], order=range(299, -1, -1))
    assert (rev != video).mean() > 0.05
    assert (np.abs(rev.astype(np.float64) - video) <= FR.render_tol(300, ab)).all()
