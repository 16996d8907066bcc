"""The float64 restatement of the dense K5 / K6 (tests/spatial_restatement.py) and its cases, held to what they claim, without
a GPU: every case reaches what it is named for (computed from its shape by the kernel's own rules, so a change of a case or of
a rule fails here instead of emptying a GPU test), the restatement is the oracle's ``update_spatial``, the input condition
of the K6 bound holds, every bound is positive where the reference is not zero, and the index rule is ``ops._ids``'s."""
import numpy as np
import pytest

import hals_spatial_restatement as HS
import spatial_restatement as SR


def geo(name):
    return SR.geometry(SR.k5_case(name))


def test_nb_cases_reach_every_instantiation_full_and_ragged():
    seen = {(geo(f"nb-{K}-{lay}")["nb"], geo(f"nb-{K}-{lay}")["full_block"]) for K in SR.NB_K for lay in ("plain", "idx")}
    assert seen == {(nb, full) for nb in range(1, 9) for full in (False, True)}
    for K in SR.NB_K:
        for lay, wide in (("plain", 4), ("idx", 4)):       # ldy = 300 and 304: both allow the 16-byte loads
            g = geo(f"nb-{K}-{lay}")
            assert (g["workgroups"], g["waves"], g["full_waves"], g["wide_waves"], g["ragged_voxels"]) == (2, 5, 4, wide, 44)
            assert (g["iters"], g["last_iter_frames"], g["last_step_frames"]) == (2, 5, 1)
    assert {1, 15, 16, 17, 32, 33, 48, 64, 65, 80, 96, 100, 112, 127, 128} <= set(SR.NB_K)


def test_tail_cases_reach_every_step_and_iteration_edge():
    assert set(SR.TAIL_T) == {1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49}
    g = {T: geo(f"tail-{T}-idx") for T in SR.TAIL_T}
    # a last MFMA step of 1, 2, 3 and 4 frames; a last iteration of 1 .. 16 frames that is full, one short, one over
    assert {v["last_step_frames"] for v in g.values()} == {1, 2, 3, 4}
    assert {v["last_iter_frames"] for v in g.values()} == {1, 2, 3, 4, 5, 15, 16}
    assert {v["iters"] for v in g.values()} == {1, 2, 3, 4}
    # one iteration: both prefetches lie past the end from the start; T = 16 k: the loop ends on a full iteration
    assert g[1]["iters"] == g[16]["iters"] == 1 and g[16]["last_iter_frames"] == 16 and g[17]["iters"] == 2
    assert all(g[T]["last_iter_frames"] == 16 for T in (16, 32, 48))
    for T in SR.TAIL_T:
        # P = 70: one full wave and one of 6 voxels; the padded layout takes the 16-byte loads, the plain one (ldy 70) cannot
        assert (g[T]["full_waves"], g[T]["wide_waves"], g[T]["ragged_voxels"], g[T]["nb"]) == (1, 1, 6, 2)
        assert geo(f"tail-{T}-plain")["wide_waves"] == 0 and geo(f"tail-{T}-plain")["full_waves"] == 1


def test_voxel_cases_reach_every_wave_and_workgroup_edge():
    assert set(SR.VOX_P) == {1, 3, 4, 63, 64, 65, 127, 128, 255, 256, 257, 320}
    g = {P: geo(f"vox-{P}-idx") for P in SR.VOX_P}
    assert [g[P]["waves"] for P in SR.VOX_P] == [1, 1, 1, 1, 1, 2, 2, 2, 4, 4, 5, 5]
    assert [g[P]["workgroups"] for P in SR.VOX_P] == [1] * 10 + [2, 2]
    assert [g[P]["ragged_voxels"] for P in SR.VOX_P] == [1, 3, 4, 63, 0, 1, 63, 0, 63, 0, 1, 0]
    assert all(g[P]["wide_waves"] == P // 64 for P in SR.VOX_P)
    # the plain layout allows the wide loads exactly where P is a multiple of 4
    assert all((geo(f"vox-{P}-plain")["wide_waves"] > 0) == (P % 4 == 0 and P >= 64) for P in SR.VOX_P)


def test_addressing_cases_reach_both_load_paths_and_every_index_form():
    for P, K, T in SR.ADDR_SHAPES:
        wide = {n: geo(n)["wide_ok"] for n in SR.K5_CASES if n.startswith(f"addr-{P}-")}
        # ldy = P, P+4, P+1, P+3: 300 and 304 allow the 16-byte loads, 301 and 303 do not; of 65, 69, 66, 68 only 68 does
        assert [wide[f"addr-{P}-ldy+{pad}"] for pad in (0, 4, 1, 3)] == [(P + pad) % 4 == 0 for pad in (0, 4, 1, 3)]
        assert sum(wide[f"addr-{P}-ldy+{pad}"] for pad in (0, 4, 1, 3)) == (2 if P == 300 else 1)
        assert wide[f"addr-{P}-base+1"] is False and wide[f"addr-{P}-base+4"] is True
        assert geo(f"addr-{P}-base+4")["full_waves"] >= 1 and geo(f"addr-{P}-ldy+0")["nb"] == 3
        for ids in ("fid", "times", "both"):
            c = SR.k5_case(f"addr-{P}-{ids}")
            fid, tt = c["frame_ids"], c["times"]
            assert (fid is not None) == (ids != "times") and (tt is not None) == (ids != "fid")
            if fid is not None:     # a permutation into a buffer with two spare rows, which hold NaN
                assert c["nrows"] == T + 2 and len(set(fid)) == T and (np.diff(fid) < 0).any()
                spare = np.setdiff1d(np.arange(c["nrows"]), fid)
                assert len(spare) == 2 and np.isnan(SR.frame_rows(c)[spare]).all()
            if tt is not None:      # not monotone, into traces with three spare columns
                assert c["C"].shape[1] == T + 3 and len(set(tt)) == T and (np.diff(tt) < 0).any()
                assert np.isnan(c["C"][:, np.setdiff1d(np.arange(T + 3), tt)]).all()
            if ids == "both":
                assert not np.array_equal(fid, tt)
            if ids == "fid":        # col_b = b: the three columns behind the frames are NaN
                assert c["C"].shape[1] == T + 3 and np.isnan(c["C"][:, T:]).all()
    g64, g65 = geo("chan-64"), geo("chan-65")
    assert (g64["wide_ok"], g64["wide_waves"], g64["ragged_voxels"]) == (True, 1, 0)
    assert (g65["wide_ok"], g65["wide_waves"], g65["full_waves"], g65["ragged_voxels"]) == (False, 0, 1, 1)
    for P in (64, 65):
        c = SR.k5_case(f"chan-{P}")
        two = c["buf"][:2 * P * c["T"]].reshape(c["T"], 2 * P)
        assert np.isnan(two[:, :P]).all() and np.array_equal(two[:, P:], SR.frame_rows(c))


def test_named_data_is_finite_and_the_rest_is_nan():
    """Magnitudes within [2^-4, 4] or zero, about a tenth zeros, a zero trace and a zero voxel; everything no frame names NaN."""
    for name in SR.K5_CASES:
        c = SR.k5_case(name)
        fid, col = SR.index_rule(c["nrows"], c["frame_ids"], c["times"])
        Y, C = SR.frame_rows(c)[fid], c["C"][:, col]
        for v in (Y, C):
            nz = np.abs(v[v != 0])
            assert np.isfinite(v).all() and (nz.size == 0 or (nz.min() >= 2.0 ** -4 and nz.max() <= 4.0))
        assert (c["P"] == 1 or not Y[:, c["P"] // 2].any()) and (c["K"] == 1 or not C[1].any()) and C.any() and Y.any()
        assert int(np.isnan(c["buf"]).sum()) == c["buf"].size - Y.size
        assert int(np.isnan(c["C"]).sum()) == c["C"].size - C.size
        if Y.size >= 1000:
            assert 0.05 < (Y == 0).mean() < 0.2 and (Y < 0).any() and (Y > 0).any()


def test_big_cases_are_the_three_index_forms():
    for K in SR.BIG_K:
        assert SR.k5_case(f"big-{K}-none")["frame_ids"] is None and SR.k5_case(f"big-{K}-none")["times"] is None
        c = SR.k5_case(f"big-{K}-fid")
        assert c["times"] is None and c["nrows"] == c["T"] + 2 and c["C"].shape[1] == c["T"] + 3   # spare rows, C wider than T
        assert SR.k5_case(f"big-{K}-both")["times"] is not None
    assert set(SR.BIG_K) == {128, 129, 256}


def test_restatement_is_the_oracles_update_spatial():
    from oracle import dnmf_oracle as O
    c = SR.k5_case("addr-65-both")
    ref = SR.k5_reference("addr-65-both")
    fid, col = SR.index_rule(c["nrows"], c["frame_ids"], c["times"])
    rng = np.random.default_rng(3)
    A, D = rng.random((5, 13, c["K"])), rng.random((5, 13, c["K"]))
    Yi = SR.frame_rows(c)[fid].astype(np.float64).T.reshape(5, 13, c["T"])
    Cn = c["C"][:, col].astype(np.float64)
    for Dk, gamma in ((None, None), (D, 0.3)):
        want = O.update_spatial(A, Cn, Yi, D=Dk, gamma=gamma)
        got = HS.mu_spatial(A.reshape(65, -1), ref["A1"], ref["Cs"], None if Dk is None else Dk.reshape(65, -1), gamma)
        np.testing.assert_allclose(got.reshape(want.shape), want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(ref["Cs"], np.einsum("kt,pt->kp", Cn, Cn), rtol=1e-13)
    np.testing.assert_allclose(ref["A1"].reshape(5, 13, -1), np.einsum("mnt,kt->mnk", Yi, Cn), rtol=1e-12, atol=1e-13)


def test_k5_bounds_are_positive_where_the_reference_is_not_zero():
    for name in SR.K5_CASES:
        ref = SR.k5_reference(name)
        for v, s, t in ((ref["A1"], ref["S1"], SR.tol_A1(ref)), (ref["Cs"], ref["Sc"], SR.tol_Cs(ref))):
            assert (t[v != 0] > 0).all() and (np.abs(v) <= s * (1 + 1e-12)).all() and np.isfinite(v).all(), name
            assert (t[s == 0] == 0).all()
        # the zero trace and the zero voxel: whole rows of exact zeros are asked for
        c = SR.k5_case(name)
        assert (c["P"] == 1 or not SR.tol_A1(ref)[c["P"] // 2].any()) and (c["K"] == 1 or not SR.tol_A1(ref)[:, 1].any())
        assert ref["A1"].any() and ref["Cs"].any()
        assert ref["B"] == c["T"]
    ref = SR.k5_reference("addr-300-ldy+0")
    assert np.array_equal(SR.tol_A1(ref, 3), (21 + 3 + 2) * 2 * SR.U * ref["S1"]) and np.array_equal(SR.tol_Cs(ref, 3), 6 * SR.U * ref["Sc"])


@pytest.mark.parametrize("P,K", SR.K6_CASES)
def test_k6_input_condition_and_bounds(P, K):
    c = SR.k6_case(P, K)
    assert all((v >= 0).all() for v in c.values())
    assert (c["A1"] == 0).any() or P * K < 20
    for mode, (withD, gamma) in SR.K6_MODES.items():
        want, tol, q = SR.k6_reference(c["A"], c["A1"], c["Cs"], c["D"] if withD else None, gamma)
        assert q <= 4.0, (mode, q)
        assert np.isfinite(want).all() and (tol[want != 0] > 0).all() and (tol[want == 0] == 0).all()
        zero = (c["A"] == 0) | (c["A1"] == 0)
        assert not want[zero].any() and (want[~zero] > 0).all()
        if P > 1:
            assert not want[P // 2].any()
    assert set(SR.K6_CASES) == {(p, k) for p in (1, 15, 16, 17, 33) for k in (1, 17, 100, 128, 129, 256)} | {(17, 1024)}


def test_index_rule_is_ops_ids():
    import torch
    from dnmf_amd import ops
    frames = torch.zeros(9, 4)
    for fid, tt in ((None, None), ([4, 0, 7, 2], None), ([4, 0, 7, 2], [5, 1, 3, 0]), (None, [5, 1, 3]), ([4, 0, 7, 2, 6], [5, 1, 3])):
        f, t, B = ops._ids(frames, fid, tt, frames.device)
        rows, cols = SR.index_rule(frames.shape[0], fid, tt)
        assert len(rows) == len(cols) == B
        assert np.array_equal(rows, f.numpy()[:B] if f is not None else np.arange(B))     # the kernel reads frame_ids[0 .. B-1]
        assert np.array_equal(cols, t.numpy() if t is not None else np.arange(B))
