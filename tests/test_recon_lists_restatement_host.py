"""tests/recon_lists_restatement.py, the float64 definition the GPU test holds ``dnmf_recon_image_lists`` to, pinned without a
GPU: that the case tables reach what they claim (computed from ``tile_lists`` and the restated launch arithmetic), and that the
cases tell a deliberately wrong kernel from the right one by at least ten bounds (one-hot and integers: by any difference at
all).  Nothing here runs a kernel.

A planted fault can only show where the geometry lets it: 'first8' and 'overwrite' need a list longer than eight, 'z1' a Z > 1
with a listed neuron in a second run of 64 positions, 'zerobox' an all-zero neuron and an empty tile, 'times' two frames.
Each fault is asserted in EVERY case and family where it can show (``can_show``, computed from the true lists), 'rim' and
'times' in all of them, and every fault in at least the cases the tables were built for."""
import numpy as np
import pytest

import recon_lists_restatement as R


def lists_of(name):
    sz = R.CASES[name][0]
    return R.tile_lists(R.case_boxes(name), sz)


def tags(name):
    return [t for _, t in R.CASES[name][1]]


# ---- the restatement itself ---------------------------------------------------------------------------------------------------
def test_layout_and_boxes():
    g = R.geometry((9, 20, 3))
    assert (g["rowf"], g["Pp"], g["nu"], g["nqx"]) == (96, 13 * 96, 2, 4)
    assert [R.geometry(s)["rowf"] for s in R.VOLUMES] == [32, 32, 64, 64, 64, 96, 96, 96, 160, 128, 128]
    idx = R.halo_index((9, 20, 3)).reshape(9, 20, 3)
    assert idx[0, 0, 0] == 2 * 96 + 2 * 3 and idx[8, 19, 2] == 10 * 96 + 21 * 3 + 2
    A = np.zeros((5 * 7 * 3, 3), dtype=np.float32)
    A.reshape(5, 7, 3, 3)[1:3, 2:6, 1, 0] = 1.0
    A.reshape(5, 7, 3, 3)[4, 6, 2, 2] = -2.0
    A.reshape(5, 7, 3, 3)[0, 0, 0, 1] = -0.0                      # -0.0 is no non-zero
    assert R.support_boxes(A, (5, 7, 3)).tolist() == [[1, 2, 2, 5, 1, 1], list(R.EMPTY) * 3, [4, 4, 6, 6, 2, 2]]


@pytest.mark.parametrize("sz", R.VOLUMES, ids=lambda s: "x".join(map(str, s)))
def test_tile_rule_is_the_stated_one(sz):
    """``tile_member`` (by marks) against the interval rule of the module docstring, for every single-voxel box of the volume's
    (x, y) plane and a few wide ones."""
    g = R.geometry(sz)
    X, Y, Z = sz
    boxes = [(x, x, y, y, 0, 0) for x in range(X) for y in range(Y)]
    boxes += [R.full_box(sz), (0, X - 1, Y - 1, Y - 1, 0, Z - 1), (X - 1, X - 1, 0, Y - 1, 0, 0), R.EMPTY * 3]
    member = R.tile_member(boxes, sz)
    assert member.shape == (g["ntile"], len(boxes))
    for qx in range(g["nqx"]):
        for qu in range(g["nu"]):
            xlo, xhi = 4 * qx - 2, min(4 * qx + 3, g["Xp"] - 1) - 2
            ylo, yhi = (64 * qu) // Z - 2, min(64 * qu + 63, g["Yp"] * Z - 1) // Z - 2
            want = [b[0] <= b[1] and b[0] <= xhi and b[1] >= xlo and b[2] <= yhi and b[3] >= ylo for b in boxes]
            assert member[qx * g["nu"] + qu].tolist() == want, (qx, qu)
    assert not member[:, -1].any() and member[:, len(boxes) - 4].sum() >= 1
    tid = R.tile_of_position(sz)
    for k in (0, X * Y - 1):                                           # a voxel's tile lists its neuron
        p = R.halo_index(sz).reshape(X, Y, Z)[boxes[k][0], boxes[k][2], 0]
        assert member[tid[p], k]


@pytest.mark.parametrize("name", list(R.CASES))
def test_inputs_are_what_the_tables_say(name):
    """The boxes of the non-zeros are the boxes placed; the tiled sum is the dense product; the exact families are exact."""
    sz, boxes, B = R.CASES[name]
    for family in R.FAMILIES:
        c = R.case_inputs(name, family)
        assert c["A"].dtype == np.float32 and c["C"].dtype == np.float32
        assert np.array_equal(R.support_boxes(c["A"], sz), R.case_boxes(name))
        named = set()
        for times in c["calls"]:
            assert len(times) == B
            S = R.recon(c["A"], c["C"], times, sz)
            tiled = R.recon_tiled(c["A"], c["C"], times, sz)
            if c["exact"]:
                assert np.array_equal(S, tiled) and np.array_equal(S.astype(np.float32).astype(np.float64), S)
                assert not R.bound(c["A"], c["C"], times, sz)[S == 0].any() or family == "integers"
            else:
                assert np.abs(S - tiled).max() <= 1e-13 * max(1.0, np.abs(S).max())
                assert (np.signbit(c["A"]) & (c["A"] == 0)).any() or (c["A"] != 0).sum() < 100       # some -0.0
                bnd = R.bound(c["A"], c["C"], times, sz)
                assert ((bnd == 0) <= (S == 0)).all() and (bnd >= 0).all()
            if family == "onehot":
                for b, t in enumerate(times):
                    k = int(np.flatnonzero(c["C"][:, t])[0])
                    named.add(k)
                    assert np.array_equal(S[b], R.to_halo(c["A"][:, k].astype(np.float64), sz))
            else:
                assert B < 2 or (len(set(times)) == B - 1 and times[-1] == times[0]) and max(times) < B + 3
        if family == "onehot":
            assert named == set(range(len(boxes)))


# ---- reach --------------------------------------------------------------------------------------------------------------------
def test_volumes_cover_every_z_and_both_kinds_of_row():
    gs = [R.geometry(s) for s in R.VOLUMES]
    assert {g["Z"] for g in gs} == {1, 2, 3, 5}
    assert any(g["Xp"] % 4 == 0 for g in gs) and {g["Xp"] % 4 for g in gs} >= {0, 1, 2, 3}
    assert any(g["Yp"] * g["Z"] == g["rowf"] and g["rowf"] % 64 == 0 for g in gs)          # a row ends on a tile, no excess
    assert any(g["rowf"] % 64 == 32 and g["nu"] >= 2 for g in gs)                          # a last tile cut at u < rowf
    assert any(g["rowf"] > g["Yp"] * g["Z"] for g in gs) and any(g["nu"] == 3 for g in gs) and any(g["rowf"] < 64 for g in gs)
    assert set(R.PACK_CASES) == set(R.VOLUMES)
    for B in R.FRAMES:                                                                     # every B at two volumes
        assert len({R.CASES[n][0] for n in R.EDGE_CASES if R.CASES[n][2] == B}) >= 2


def test_list_length_classes():
    for name in R.STACK_CASES:
        sz = R.CASES[name][0]
        lens = sorted({len(l) for l in lists_of(name)})
        assert lens[:6] == [0, 1, 8, 9, 16, 17] and lens[6] >= 25 and len(lens) == 7, lens
        for (qx, qu), n in R.STACKS[sz].items():
            l = lists_of(name)[qx * R.geometry(sz)["nu"] + qu]
            assert len(l) == n and (n < 2 or (np.diff(l) > 1).any())                       # not a run of neighbours
        assert R.kernel_form(len(R.CASES[name][1])) == 2
    name = "K256-5x7x3-B5"
    assert sorted({len(l) for l in lists_of(name)}) == [0, 256] and 256 // R.RL_NG == 32   # (0: the tiles of border rows alone)
    assert any(len(l) > 8 for l in R.tile_lists(R.support_boxes(R.long_inputs()["A"], R.LONG_CASE["sz"]), R.LONG_CASE["sz"]))


def test_every_kernel_form_and_its_ends():
    Ks = sorted({len(R.CASES[n][1]) for n in R.KFORM_CASES})
    assert Ks == [1, 64, 65, 128, 129, 256]
    assert [R.kernel_form(K) for K in Ks] == [1, 1, 2, 2, 4, 4] and R.kernel_form(R.REFUSED_K) is None
    for name in R.KFORM_CASES:
        K = len(R.CASES[name][1])
        listed = set(np.concatenate(lists_of(name)).tolist())
        assert listed == set(range(K))                                # every slot of every ballot word, both ends of each
    for K in Ks:
        assert len({R.CASES[n][0] for n in R.KFORM_CASES if len(R.CASES[n][1]) == K}) == 2
    assert R.MODEL_K == (65, 129)


def test_both_sides_of_every_tile_boundary():
    seen_y = {Z: set() for Z in (1, 2, 3, 5)}
    seen_x = {Z: set() for Z in (1, 2, 3, 5)}
    for name in R.EDGE_CASES:
        sz = R.CASES[name][0]
        g = R.geometry(sz)
        member, rim = R.tile_member(R.case_boxes(name), sz, want_rim=True)
        member, rim = member.reshape(g["nqx"], g["nu"], -1), rim.reshape(g["nqx"], g["nu"], -1)
        cols = R.tile_columns(sz)
        boxes = R.case_boxes(name)
        kinds = {t for t in tags(name)}
        assert {"corner", "zero", "full"} <= kinds and tags(name).count("corner") == 8
        holds_voxel = np.zeros(g["ntile"], bool)
        holds_voxel[R.tile_of_position(sz)[R.halo_index(sz)]] = True
        assert np.array_equal(member[:, :, tags(name).index("full")].reshape(-1), holds_voxel)
        assert not member[:, :, tags(name).index("zero")].any()
        for k, t in enumerate(tags(name)):
            b = boxes[k]
            if t.startswith(("ends", "begins")):
                qu = int(t.rsplit("-", 1)[1])
                in0, in1 = member[:, qu, k].any(), member[:, qu + 1, k].any()
                if t.startswith("ends-before"):
                    assert b[3] == cols[qu + 1, 0] - 1 and in0 and not in1
                elif t.startswith("ends-on"):
                    assert b[3] == cols[qu + 1, 0] and in0 and in1 and rim[:, qu + 1, k].any()
                elif t.startswith("begins-on"):
                    assert b[2] == cols[qu, 1] and in0 and in1 and rim[:, qu, k].any()
                else:
                    assert b[2] == cols[qu, 1] + 1 and in1 and not in0
                seen_y[g["Z"]].add(t.rsplit("-", 1)[0])
            if t.startswith("xends"):
                last = int(t.split("-")[1])                             # volume row 1 | 5 = padded row 3 | 7
                assert b[1] + R.HALO in (3, 7) and member[(last + 2) // 4, :, k].any() and not member[(last + 2) // 4 + 1, :, k].any()
                seen_x[g["Z"]].add(t)
            if t.startswith("xbegins"):
                first = int(t.split("-")[1])
                assert b[0] + R.HALO in (4, 8) and member[(first + 2) // 4, :, k].any() and not member[(first + 2) // 4 - 1, :, k].any()
                seen_x[g["Z"]].add(t)
    for Z in (1, 2, 3, 5):
        assert seen_y[Z] == {"ends-before", "ends-on", "begins-on", "begins-after"}, (Z, seen_y[Z])
        assert seen_x[Z] == {"xends-1", "xbegins-2", "xends-5", "xbegins-6"}, (Z, seen_x[Z])
    # at Z | 64 the boundary is the pair of positions 63 | 64; at Z = 3 and 5 one column owns both
    for sz, same in (((41, 130, 1), False), ((33, 31, 2), False), ((5, 30, 3), True), ((6, 20, 5), True)):
        cols = R.tile_columns(sz)
        assert (cols[0, 1] == cols[1, 0]) == same and cols[0, 1] == 63 // sz[2] - 2 and 0 <= cols[1, 0] <= sz[1] - 1


def test_ragged_and_exact_last_tiles():
    empties = {}
    for name in R.EDGE_CASES + R.STACK_CASES:
        sz = R.CASES[name][0]
        g = R.geometry(sz)
        ll = lists_of(name)
        empties[name] = sum(len(l) == 0 for l in ll)
        if name in R.EDGE_CASES and g["Xp"] % 4 in (1, 2):               # the last rows of tiles hold border rows alone
            assert all(len(l) == 0 for l in ll[-g["nu"]:])
    assert all(empties[n] > 10 for n in R.STACK_CASES)
    assert any(empties[n] == 0 for n in R.EDGE_CASES) and any(empties[n] > 0 for n in R.EDGE_CASES)
    g = R.geometry((41, 130, 1))
    assert g["rowf"] - 64 * (g["nu"] - 1) == 32 and g["Xp"] % 4 == 1   # last tile of a row: 8 of 16 lanes; last tile row: 1 of 4


def test_frame_partition():
    """fpw and the (block, wave) pairs that leave at once, for every B of the table (small volumes: fpw is 16, or B below it)."""
    want = {1: (1, 1, {1, 2, 3}, [1]), 15: (15, 1, {1, 2, 3}, [15]), 16: (16, 1, {1, 2, 3}, [16]), 17: (16, 1, {2, 3}, [16, 1]),
            63: (16, 1, set(), [16, 16, 16, 15]), 64: (16, 1, set(), [16] * 4), 65: (16, 2, {5, 6, 7}, [16] * 4 + [1]),
            70: (16, 2, {5, 6, 7}, [16] * 4 + [6])}
    for name in R.EDGE_CASES:
        sz, _, B = R.CASES[name]
        L = R.launch(sz, B)
        fpw, ny, leave, frames = want[B]
        assert (L["fpw"], L["ny"]) == (fpw, ny), (name, L)
        assert {by * 4 + w for by, w in L["leave"]} == leave
        assert [L["frames"][k] for k in sorted(L["frames"])] == frames and sum(frames) == B
    c = R.LONG_CASE
    L = R.launch(c["sz"], c["B"])
    ntile = R.geometry(c["sz"])["ntile"]
    assert L["fpw"] == 65 and R.launch(c["sz"], c["B"] - 1)["fpw"] == 64 and ntile == 3
    assert min(B * n for n in (1, 2, 3, 4) for B in (-(-(64 * 16384 + 1) // n),)) <= c["B"] * ntile <= 64 * 16384 + ntile
    assert L["ny"] <= 65535 and len(L["leave"]) > 0 and 1 <= min(L["frames"].values()) < 65
    assert c["B"] * R.geometry(c["sz"])["Pp"] * 4 < 2 ** 29             # 0.4 GiB of images: short rows, a last tile of one row


# ---- discrimination -----------------------------------------------------------------------------------------------------------
def far_off(err, bnd):
    """Some entry is off by at least ten bounds (a zero bound: by anything at all)."""
    return bool(((err >= 10.0 * bnd) & (err > 0)).any())


def can_show(name, fault, family="random"):
    sz, boxes, B = R.CASES[name]
    g = R.geometry(sz)
    ll = lists_of(name)
    empty = np.array([len(l) == 0 for l in ll])
    if fault in ("first8", "overwrite"):
        return max(len(l) for l in ll) > R.RL_NG
    if fault == "times":
        return B >= 2 and (family != "onehot" or len(boxes) > 1)           # one neuron: every one-hot column is the same
    if fault == "z1":
        member = R.tile_member(R.case_boxes(name), sz).reshape(g["nqx"], g["nu"], -1)
        return g["Z"] > 1 and g["nu"] > 1 and bool(member[:, 1:].any())
    if fault == "zerobox":
        return "zero" in tags(name) and bool((empty & R.tile_member([R.full_box(sz)], sz)[:, 0]).any())   # an empty tile with voxels
    return bool(R.tile_member(R.case_boxes(name), sz, want_rim=True)[1].any())


@pytest.mark.parametrize("name", list(R.CASES))
def test_cases_tell_a_wrong_kernel(name):
    sz = R.CASES[name][0]
    assert can_show(name, "times") or R.CASES[name][2] == 1
    assert can_show(name, "rim") or name == "K256-5x7x3-B5"               # (every box there spans two rows of a tile at least)
    for family in R.FAMILIES:
        c = R.case_inputs(name, family)
        seen = {f: False for f in R.FAULTS if can_show(name, f, family)}
        for times in c["calls"]:
            preset = R.PATTERN
            S = R.recon_tiled(c["A"], c["C"], times, sz, preset=preset)
            bnd = np.zeros_like(S) if c["exact"] else R.bound(c["A"], c["C"], times, sz)
            for f in seen:
                wrong = R.recon_tiled(c["A"], c["C"], times, sz, fault=f, preset=preset)
                seen[f] |= far_off(np.abs(wrong - S), bnd)
        assert all(seen.values()), (name, family, seen)


def test_every_fault_has_its_cases():
    for f in ("first8", "overwrite"):
        assert all(can_show(n, f) for n in R.STACK_CASES) and can_show("K256-5x7x3-B5", f)
    for Z in (2, 3, 5):
        assert any(can_show(n, "z1") for n in R.EDGE_CASES if R.CASES[n][0][2] == Z), Z
    assert all(can_show(n, "zerobox") for n in R.STACK_CASES)
    c = R.model_inputs(65, "integers")
    assert len(c["boxes"]) == 65 and sum((b[1] - b[0] + 1) * (b[3] - b[2] + 1) for b in c["boxes"]) < 2 * 41 * 130
