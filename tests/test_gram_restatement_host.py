"""tests/gram_restatement.py, the float64 definition the GPU test holds K3, K3s and K3n to, pinned without a GPU: against the
oracle's fp32 warp and float64 contraction, the nudge condition of every case, and that the cases reach what they are meant to
reach -- computed from geometry alone, nothing here runs a kernel.

Which cases must show which list lengths.  z1 and z2 are the list cases: their tiles' lower-bound counts must include 0, a
value in 1..4, one in 5..8 and one >= 9 (the empty tile, one group of four, two groups, the cross-group sums past eight).
z1-dense-lists (12 neurons listed nearly everywhere) must reach >= 9 and 5..8; the other Z <= 2 cases have too few neurons
for every class by design (padK-15, the large volumes' six) and are held to what their own row of the table says."""
import numpy as np
import pytest

import gram_restatement as GR
import k2_restatement as K2R
from oracle import dnmf_oracle as O


def check(name, what, err, bound):
    ratio, idx, zeros_ok = GR.worst(err, bound)
    assert zeros_ok, f"{name} {what}: an entry with a zero bound is not an exact zero"
    assert ratio <= 1.0, f"{name} {what}: entry {idx}: |difference| = {ratio:.3g} of the bound"
    return ratio


@pytest.mark.parametrize("name", ["thin", "padK-15", "z1-dense-lists"])
def test_restatement_against_the_oracle(name):
    """oracle.forward's A_t (the reference's fp32 warp, the arithmetic of the committed goldens) contracted by oracle.gram_rhs
    in float64: the restatement differs by the fp32 rounding of A_t only, far inside the bound."""
    c = GR.gram_case(name)
    sz, K, times = c["sz"], c["K"], c["times"]
    ref, _ = GR.reference(name)
    basis = O.quadratic_basis(O.voxel_lattice(sz))
    _, A_t, _, _ = O.forward(c["A"], basis, c["beta"], sz, times, np.zeros((K, GR.T_COLS), np.float32))
    Y = np.moveaxis(c["frames"].reshape(len(times), *sz), 0, -1).astype(np.float64)
    G, r = O.gram_rhs(np.transpose(A_t.astype(np.float64), [2, 3, 4, 1, 0]), Y)
    tG, tr = GR.tol(ref)
    rg = check(name, "G", np.abs(np.moveaxis(G, 2, 0) - ref["G"]), tG)
    rr = check(name, "r", np.abs(r.T - ref["r"]), tr)
    assert ref["G"].max() > 0 and np.abs(ref["r"]).max() > 0
    print(f"\n{name}: |restatement - oracle| / bound <= {rg:.3g} (G), {rr:.3g} (r)")


def slab_of(name):
    """Rows of a large volume that contain every footprint's samples under F0 and F5: the sums over the other rows are exact
    zeros, so the slab's sums are the volume's."""
    c = GR.gram_case(name)
    keep = np.zeros(c["sz"][0], bool)
    for t in c["times"]:
        u = K2R._coords(np.ascontiguousarray(c["beta"][:, :, t]).tobytes(), c["sz"])
        for k in range(c["K"]):
            bb = c["bbox"][k]
            if bb[0] > bb[1]:
                continue
            m = np.ones(u.shape[:-1], bool)
            for d in range(3):
                m &= (u[..., d] > bb[2 * d] - 1) & (u[..., d] < bb[2 * d + 1] + 1)
            keep |= m.any(axis=(1, 2))
    return keep


@pytest.mark.parametrize("name", list(GR.CASES))
def test_nudge_condition(name):
    """Every fp32 source coordinate one representable step up, then one step down: every entry of G and r moves by at most a
    quarter of its bound, and the set of zero-bound entries stays.  The kernels' fused coordinate chain may differ from the
    reference's sequence by an ulp; this is the room the bound leaves for it.  The large volumes: on the rows that hold the
    footprints' samples, cut into runs (every other row adds exact zeros)."""
    c = GR.gram_case(name)
    base, _ = GR.reference(name)
    tG, tr = GR.tol(base)
    runs = [None]
    if name in GR.LARGE:
        keep = slab_of(name)
        edges = np.flatnonzero(np.diff(np.concatenate([[0], keep.astype(int), [0]])))
        runs = [slice(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2])]
        assert 0 < keep.sum() < 0.25 * len(keep)
    worst_g = worst_r = 0.0
    for n in (1, -1):
        parts = [GR.gram(c["A"], c["beta"], c["sz"], c["times"], c["frames"], nudge=n, rows=rw) for rw in runs]
        got = {k: sum(p[k] for p in parts) for k in ("G", "r", "absG", "absr", "coordG", "coordr")}
        worst_g = max(worst_g, check(name, f"G nudged {n:+d}", np.abs(got["G"] - base["G"]), 0.25 * tG))
        worst_r = max(worst_r, check(name, f"r nudged {n:+d}", np.abs(got["r"] - base["r"]), 0.25 * tr))
        nG, nr = GR.C_SUM * got["absG"] + got["coordG"], GR.C_SUM * got["absr"] + got["coordr"]
        assert np.array_equal(nG == 0, tG == 0) and np.array_equal(nr == 0, tr == 0), f"{name}: the zero-bound set moved"
    share = float((base["coordG"].sum() / tG.sum())) if tG.sum() else 0.0
    print(f"\n{name}: one fp32 step moves G by <= {worst_g:.3g}, r by <= {worst_r:.3g} of a quarter bound; "
          f"coordinate term = {share:.2f} of the summed bound of G")


@pytest.mark.parametrize("name", ["z1", "z1-dense-lists", "z2"])
def test_list_lengths(name):
    counts = np.concatenate([GR.tile_geometry(name, f)[0] for f in range(8)])
    has = {"0": (counts == 0).any(), "1..4": ((counts >= 1) & (counts <= 4)).any(), "5..8": ((counts >= 5) & (counts <= 8)).any(),
           ">=9": (counts >= 9).any()}
    print(f"\n{name}: list lengths (lower bound) up to {counts.max()}, classes {has}")
    need = ["5..8", ">=9"] if name == "z1-dense-lists" else list(has)
    assert all(has[k] for k in need), has


@pytest.mark.parametrize("name", [n for n in GR.SMALL if GR.CASES[n][0][2] <= 2 and n != "long"])
def test_staging_region_fits_f0_and_not_f7(name):
    """F7 (scale 1.6): every tile with all its rows or all its columns spans more than LISTS_RR tap rows or more than LISTS_RC
    floats of a halo row, so it takes the direct gathers (only a ragged corner tile, which has neither, can fit); F0 (a
    sub-voxel shift): no tile spans more than 9 rows or 33 columns (at Z = 2: 17 columns of two slices)."""
    cnt, rows, cols, full = GR.tile_geometry(name, 7)
    assert full.any() and ((rows[full] > GR.LISTS_RR) | (cols[full] > GR.LISTS_RC)).all(), (rows[full].min(), cols[full].min())
    cnt, rows, cols, full = GR.tile_geometry(name, 0)
    Z = GR.CASES[name][0][2]
    assert rows.max() <= 9 and cols.max() <= 33 * Z and cols.max() < GR.LISTS_RC - 3, (rows.max(), cols.max())


def test_k_edges():
    """Each K of ``words`` and ``padK`` lies on the stated side of its edge: lists_words is 1 | 2 | 4 by K <= 64, K <= 128;
    K3 pads to Kp = 16 ceil((K + 1) / 16) (the frame rides in column Kp - 1); every layout keeps nslot <= 3800."""
    words = lambda K: 1 if K <= 64 else (2 if K <= 128 else 4)
    assert [words(GR.CASES[f"words-{K}"][1]) for K in (64, 65, 128, 129, 256)] == [1, 2, 2, 4, 4]
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import ops
    assert [ops.padded_k(GR.CASES[f"padK-{K}"][1]) for K in (15, 16, 17, 127)] == [16, 32, 32, 128]
    assert ops.padded_k(128) > 128 and ops.padded_k(65) <= 128          # words: K3 takes 64 and 65, not 128 and beyond
    for n in GR.SMALL:
        assert GR.gram_case(n)["nslot"] <= GR.MAX_SLOTS, (n, GR.gram_case(n)["nslot"])


@pytest.mark.parametrize("name", ["z1", "z2", "z3"] + GR.LARGE)
def test_some_tested_entry_is_weak(name):
    """An entry below 1e-4 max|G| with a non-zero bound: what the older bounds (2e-5 max|G| against float64, 2e-6 max|G|
    between kernels) cannot see at all -- and the new bound pins one to 5 % of its own value or better, so a tile or a tap
    row dropped from such a pair fails.  (Measured: every weak entry of z1, z3 and the large volumes and 99 % of z2's are
    within 5 %; medians 0.15 %, 0.5 %, 0.13 %, 0.1 .. 0.2 %.)"""
    ref, _ = GR.reference(name)
    tG, _ = GR.tol(ref)
    weak = (tG > 0) & (ref["G"] < 1e-4 * ref["G"].max()) & (ref["G"] > 0)
    hidden = weak & (ref["G"] < 2e-6 * ref["G"].max())
    print(f"\n{name}: {int(weak.sum())} entries below 1e-4 max|G|, {int(hidden.sum())} of them below 2e-6 max|G|, smallest "
          f"{ref['G'][weak].min() / ref['G'].max():.3g} max|G|")
    assert weak.any()
    assert (tG[weak] <= 0.05 * ref["G"][weak]).any(), "no weak entry is pinned to 5 % of its value"
