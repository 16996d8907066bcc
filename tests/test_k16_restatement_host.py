"""tests/k16_restatement.py, the float64 definition the GPU test holds K16 to, pinned without a GPU: that it is
GN.normal_eqs, the symmetry and the exact zeros, the flip condition of every (shape, frame) the GPU test uses, and that the
bound ``1e-4 * (the entry's own absolute sum)`` sees the mistakes it is there for.

Mutants.  Each is applied to the float64 sums on the route the kernel takes (k16_restatement.assemble) and must leave some entry
of H or g at least ten bounds off at the shapes named:
  (a) a z exponent >= 3 lowered by 2             visible at (34, 90, 5) and (9, 7, 4); NOT visible (< 1e-6 of the bound) at
                                                 (65, 300, 2), (34, 90, 3), (9, 7, 3): at Z <= 3 the centred u_z is -1, 0 or 1,
                                                 where u_z^3 == u_z and u_z^4 == u_z^2 -- why the shapes with Z >= 4 exist
  (b) the pair (d, e) of an off-diagonal block   (0, 2) read as (1, 2); at Z = 1, whose only such pair is (0, 1), read as (0, 0)
  (c) the last plane position dropped            every shape
  (d) the last x-row dropped                     every shape
  (e) the voxels of plane positions >= 256 given y, z as if Z were Z - 1: a wrong division at (34, 90, 5)
Every test prints what it measured."""
import time

import numpy as np
import pytest

import gn_restatement as GN
import k16_restatement as K16R
import k2_restatement as K2R
from oracle import dnmf_oracle as O


@pytest.mark.parametrize("sz", K16R.SHAPES)
def test_same_definition_symmetry_and_exact_zeros(sz):
    c = K16R.k16_case(sz)
    ref = K16R.reference(sz)
    H, g, sse = GN.normal_eqs(None, None, c["beta"], sz, c["times"], c["frames"], S=c["S32"])
    np.testing.assert_allclose(ref["H"], H, rtol=1e-12, atol=0)
    np.testing.assert_allclose(ref["g"], g, rtol=1e-12, atol=0)
    np.testing.assert_allclose(ref["sse"], sse, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(ref["H"], np.swapaxes(ref["H"], 1, 2))
    np.testing.assert_array_equal(ref["absH"], np.swapaxes(ref["absH"], 1, 2))
    assert (np.abs(ref["H"]) <= ref["absH"] * (1 + 1e-12)).all() and (np.abs(ref["g"]) <= ref["absg"] * (1 + 1e-12)).all()
    # the frames: F0 .. F5 and F7 see an image, F6 has all-zero traces, the last two have a coefficient that is not finite
    assert c["times"] == [K2R.COL[i] for i in range(7)] + [K16R.LAST_COL, K16R.NAN_COL, K16R.INF_COL]
    assert K2R.UNUSED not in c["times"] and c["finite"] == 8
    assert np.isnan(c["beta"][:, :, K16R.NAN_COL]).sum() == 1 and np.isposinf(c["beta"][:, :, K16R.INF_COL]).sum() == 1
    assert np.isfinite(c["beta"][:, :, :K16R.NAN_COL]).all()
    np.testing.assert_array_equal(c["beta"][:, :, :K2R.T_COLS], K2R.k2_case(sz)["beta"])
    act = GN.active(sz)
    for b in (0, 1, 2, 3, 4, 5, 7):
        assert (ref["absH"][b][np.ix_(act, act)] > 0).all() and (ref["absg"][b][act] > 0).all()
    assert ref["sse"][6] > 0 and not ref["absH"][6].any() and not ref["absg"][6].any()
    for b in (8, 9):
        assert np.isnan(ref["sse"][b]) and not ref["H"][b].any() and not ref["g"][b].any() and not ref["absH"][b].any()
    if sz[2] == 1:   # the unknowns Z = 1 drops: exact zeros, also in the sums of absolute values
        off = np.setdiff1d(np.arange(30), act)
        assert len(act) == 12
        for k in ("H", "absH"):
            assert not ref[k][:, off].any() and not ref[k][:, :, off].any()
        assert not ref["g"][:, off].any() and not ref["absg"][:, off].any()


@pytest.mark.parametrize("sz", K16R.SHAPES)
def test_flip_condition(sz):
    """H and g jump where a source coordinate crosses an integer, and the kernel's fused coordinate chain may differ from the
    reference's by an ulp.  So the restatement is evaluated at its own coordinates and with every coordinate one fp32 step up,
    then down: each nudged result must stay within a quarter of what the GPU test allows the kernel, entry by entry.  A case
    that fails gets another seed (k2_restatement.SEED), never another factor.  Worst ratios (of the quarter) measured on the
    CPU with the present seeds: H 0.24 / 0.50 / 0.13 / 0.064, g 0.31 / 0.44 / 0.11 / 0.052, sse 0.010 / 0.004 / 0.005 / 0.088
    in the order of k16_restatement.SHAPES."""
    t0 = time.perf_counter()
    ref = K16R.reference(sz)
    fin = slice(0, K16R.k16_case(sz)["finite"])
    rh = rg = rs = 0.0
    for n in (1, -1):
        run = K16R.reference(sz, nudge=n)
        rh = max(rh, K16R.worst(np.abs(run["H"] - ref["H"]), 0.25 * K16R.H_tol(ref)))
        rg = max(rg, K16R.worst(np.abs(run["g"] - ref["g"]), 0.25 * K16R.g_tol(ref)))
        rs = max(rs, float((np.abs(run["sse"][fin] - ref["sse"][fin]) / (0.25 * K16R.SSE_RTOL * ref["sse"][fin])).max()))
        assert np.isnan(run["sse"][fin.stop:]).all()
    print(f"\n{sz}: nudged / (0.25 tol): H {rh:.3g}, g {rg:.3g}, sse {rs:.3g}; {time.perf_counter() - t0:.2f} s")
    assert rh <= 1.0 and rg <= 1.0 and rs <= 1.0


# ---- the bound sees what it is for -------------------------------------------------------------------------------------
def mutant_ratios(sz, mutants):
    """{name: largest |mutant - unbroken| / bound over the finite frames and the entries of H and g}; ``mutants``: {name: the
    hooks of k16_restatement.assemble that make it}."""
    c = K16R.k16_case(sz)
    ref = K16R.reference(sz)
    Ht, gt = K16R.H_tol(ref), K16R.g_tol(ref)
    worst = {k: 0.0 for k in mutants}
    for b in range(c["finite"]):
        dq, r = K16R.frame_parts(c["S32"][b], c["beta"][:, :, c["times"][b]], sz, c["frames"][b])
        H0, g0 = K16R.assemble(sz, dq, r)
        # the unbroken route is the definition (to a millionth of the bound: the sums are added in another order)
        assert K16R.worst(np.abs(H0 - ref["H"][b]), 1e-6 * Ht[b]) <= 1.0 and K16R.worst(np.abs(g0 - ref["g"][b]), 1e-6 * gt[b]) <= 1.0
        for k, hooks in mutants.items():
            H1, g1 = K16R.assemble(sz, dq, r, **hooks)
            worst[k] = max(worst[k], K16R.worst(np.abs(H1 - H0), Ht[b]), K16R.worst(np.abs(g1 - g0), gt[b]))
    return worst


LOWER_Z = {"zexp": lambda k: k - 2 if k >= 3 else k}


@pytest.mark.parametrize("sz", [(34, 90, 5), (9, 7, 4)])
def test_mutant_a_z_exponent_is_visible_at_four_slices_and_more(sz):
    ratio = mutant_ratios(sz, {"a": LOWER_Z})["a"]
    print(f"\n(a) {sz}: {ratio:.3g} bounds")
    assert ratio >= 10.0


@pytest.mark.parametrize("sz", [(65, 300, 2), (34, 90, 3), (9, 7, 3)])
def test_mutant_a_z_exponent_is_invisible_up_to_three_slices(sz):
    """The documented reason the shapes with Z >= 4 exist."""
    ratio = mutant_ratios(sz, {"a": LOWER_Z})["a"]
    print(f"\n(a) {sz}: {ratio:.3g} bounds")
    assert ratio < 1e-6


@pytest.mark.parametrize("sz", K16R.SHAPES)
def test_mutants_b_c_d_are_visible(sz):
    X, Y, Z = sz
    swap = ((0, 2), (1, 2)) if Z > 1 else ((0, 1), (0, 0))
    lat = O.voxel_lattice(sz).reshape(-1, 3)
    pos = K16R.plane_position(sz)
    ratios = mutant_ratios(sz, {"b": {"pair": lambda d, e: swap[1] if (d, e) == swap[0] else (d, e)},
                                "c": {"keep": pos != pos.max()}, "d": {"keep": lat[:, 0] != X - 1}})
    print(f"\n{sz}: " + ", ".join(f"({k}) {v:.3g} bounds" for k, v in ratios.items()))
    assert pos.max() == (Y if Z == 2 else Y * Z) - 1
    assert all(v >= 10.0 for v in ratios.values()), ratios


def test_mutant_e_wrong_division_is_visible():
    sz = (34, 90, 5)
    X, Y, Z = sz
    pos = K16R.plane_position(sz)
    assert Y * Z > K16R.PLANE_COLS and K16R.PLANE_COLS % Z != 0          # the block boundary falls inside a z-column
    y, z = np.where(pos >= K16R.PLANE_COLS, pos // (Z - 1), pos // Z), np.where(pos >= K16R.PLANE_COLS, pos % (Z - 1), pos % Z)
    s, o = GN.centre(sz)
    uc = GN.centred_lattice(sz).reshape(-1, 3).copy()
    uc[:, 1], uc[:, 2] = y * s[1] + o[1], z * s[2] + o[2]
    ratio = mutant_ratios(sz, {"e": {"uc": uc}})["e"]
    print(f"\n(e) {sz}: {ratio:.3g} bounds")
    assert ratio >= 10.0
