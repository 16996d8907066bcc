"""The float64 restatement of K6h (tests/hals_spatial_restatement.py), the exact NNLS footprint solver, held to what it
claims: it reaches scipy's NNLS, it never raises the objective, it revives zeros, respects the boxes, survives a dead
trace and sums of any sign, and on footprints planted too narrow it beats the multiplicative update sweep for sweep."""
import numpy as np
import pytest

import hals_spatial_restatement as R


def small_problem(seed):
    """P <= 40 voxels, K <= 6 neurons, T >= 4 K frames of independent non-negative traces -> (C, Y, A1, Cs, A0)."""
    rng = np.random.default_rng(seed)
    K, P = int(rng.integers(2, 7)), int(rng.integers(10, 41))
    T = 4 * K + int(rng.integers(0, 8))
    C = rng.random((K, T))
    Y = rng.standard_normal((P, T)) + 0.5
    return C, Y, Y @ C.T, C @ C.T, rng.random((P, K))


@pytest.mark.parametrize("seed", range(6))
def test_enough_sweeps_reach_scipy_nnls(seed):
    """Measured on these six problems (cond(Cs) 25 .. 93): 97 .. 159 sweeps bring every entry within 1e-12 of scipy's NNLS
    solution relative to its largest entry, and from 400 sweeps on the distance stays at 6.6e-16 .. 2.5e-15 (the rounding of
    the two solvers).  Asserted: ten times the largest measured distance, 2.5e-14, after 400 sweeps."""
    from scipy.optimize import nnls
    C, Y, A1, Cs, A0 = small_problem(seed)
    assert np.linalg.cond(Cs) < 1e3          # independent traces, T >= 4 K: the problem has one solution and HALS a rate
    ref = np.stack([nnls(C.T, y)[0] for y in Y])
    A = R.hals_spatial(A0, A1, Cs, sweeps=400)
    dist = np.abs(A - ref).max() / np.abs(ref).max()
    print(f"\nseed {seed}: cond {np.linalg.cond(Cs):.1f}, distance after 400 sweeps {dist:.3e}")
    assert dist <= 2.5e-14


def test_kkt_falls_to_rounding_with_a_penalty():
    """With D and gamma > 0 the KKT figure falls below 1e-10 of the magnitude of the gradient's terms."""
    C, Y, A1, Cs, A0 = small_problem(11)
    rng = np.random.default_rng(12)
    D, gamma = rng.random(A0.shape), 0.7
    A = R.hals_spatial(A0, A1, Cs, D=D, gamma=gamma, sweeps=600)
    kkt, terms = R.kkt(A, A1, Cs, D=D, gamma=gamma), R.term_sum(A, A1, Cs, D=D, gamma=gamma).max(0)
    print("\nkkt / terms", kkt / terms)
    assert (kkt <= 1e-10 * terms).all() and (A >= 0).all()
    # the penalty is in the solution: without it the footprints are larger
    assert R.hals_spatial(A0, A1, Cs, sweeps=600).sum() > A.sum()


@pytest.mark.parametrize("penalty", [False, True])
def test_the_objective_never_rises(penalty):
    C, Y, A1, Cs, A = small_problem(21)
    D = np.random.default_rng(22).random(A.shape) if penalty else None
    f = R.objective(A, A1, Cs, D, 0.5)
    for _ in range(30):
        A = R.hals_spatial(A, A1, Cs, D=D, gamma=0.5, sweeps=1)
        f_new = R.objective(A, A1, Cs, D, 0.5)
        assert f_new <= f + 1e-12 * abs(f)
        f = f_new


def test_zeros_revive_inside_the_box_and_stay_outside():
    sz = (6, 5, 1)
    C, Y, A1, Cs, _ = small_problem(31)
    K = Cs.shape[0]
    rng = np.random.default_rng(32)
    A1 = np.abs(rng.standard_normal((30, K))) + 1.0          # every gradient at a zero state is negative
    boxes = np.tile(np.array([1, 4, 0, 3, 0, 0]), (K, 1))
    M = R.box_mask(boxes, sz)
    A = R.hals_spatial(np.zeros((30, K)), A1, Cs, sweeps=1, boxes=boxes, sz=sz)
    assert (R.gradient(np.zeros((30, K)), A1, Cs)[:, 0] < 0).all()
    assert (A[M[:, 0], 0] > 0).all()                         # revived: the first neuron moves wherever its box allows
    assert (A[~M] == 0).all() and M.sum() == 16 * K          # outside the box nothing, whatever the gradient says
    # a non-zero start outside the box is zeroed, not kept
    A = R.hals_spatial(np.ones((30, K)), A1, Cs, sweeps=2, boxes=boxes, sz=sz)
    assert (A[~M] == 0).all()
    # the multiplicative update keeps the zero for ever
    assert (R.mu_spatial(np.zeros((30, K)), A1, Cs) == 0).all()


def test_a_dead_trace_leaves_its_column():
    C, Y, A1, Cs, A0 = small_problem(41)
    C[1] = 0.0
    A1, Cs = Y @ C.T, C @ C.T
    assert Cs[1, 1] == 0
    A = R.hals_spatial(A0, A1, Cs, sweeps=3)
    assert (A[:, 1] == A0[:, 1]).all() and np.isfinite(A).all()
    assert not (A[:, 0] == A0[:, 0]).all()
    Cs[1, 1] = np.inf
    assert (R.hals_spatial(A0, A1, Cs, sweeps=1)[:, 1] == A0[:, 1]).all()


def test_negative_sums_give_zero_where_mu_breaks():
    C, Y, A1, Cs, A0 = small_problem(51)
    A1 = A1.copy()
    A1[3, 0] = -5.0                    # e.g. after background_subtract(clamp=False)
    A1[4, :] = -1.0
    A = R.hals_spatial(A0, A1, Cs, sweeps=50)
    assert np.isfinite(A).all() and (A >= 0).all() and A[3, 0] == 0 and (A[4] == 0).all()
    mu = R.mu_spatial(A0, A1, Cs)
    assert mu[3, 0] < 0 and (mu[4] < 0).all()                # the multiplicative update leaves the cone


@pytest.mark.parametrize("depth", [2, 1])
def test_narrow_footprints_recover_faster_than_under_mu(depth):
    """24 x 20 x depth, K = 6, T = 40, footprints planted 1.5 x too narrow (cut at 1e-3), exact traces.  Measured after 5
    HALS sweeps with grow=2 against 5 multiplicative updates: depth 2 objective -4809.53 against -4798.24, correlation with
    the truth 0.9997 against 0.9976; depth 1 -1807.71 against -1803.06, 0.9997 against 0.9970.  Asserted: the ordering."""
    pl = R.planted(depth)
    Y, C = pl["video"].astype(np.float64), pl["C"].astype(np.float64)
    A1, Cs = Y.T @ C.T, C @ C.T
    boxes = R.dilate_boxes(R.support_boxes(pl["A_narrow"], pl["sz"]), pl["sz"], 2)
    mu = pl["A_narrow"].astype(np.float64)
    for _ in range(5):
        mu = R.mu_spatial(mu, A1, Cs)
    hals = R.hals_spatial(pl["A_narrow"], A1, Cs, sweeps=5, boxes=boxes, sz=pl["sz"])
    f_mu, f_hals = R.objective(mu, A1, Cs), R.objective(hals, A1, Cs)
    r_mu, r_hals = R.footprint_correlation(mu, pl["A_true"]), R.footprint_correlation(hals, pl["A_true"])
    print(f"\ndepth {depth}: objective hals {f_hals:.2f} mu {f_mu:.2f}; correlation hals {r_hals:.4f} mu {r_mu:.4f}")
    assert f_hals <= f_mu and r_hals > r_mu
    # the grown support is used: values where the narrow footprint had none
    assert ((hals > 0) & (pl["A_narrow"] == 0)).any()


def test_the_library_refuses_bad_arguments_without_a_gpu():
    """Validation happens before any HIP call: NULL buffers, sweeps < 1, boxes without their volume, a missing workspace."""
    import ctypes
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    assert lib.dnmf_hals_spatial(None, a, a, None, 0.0, 4, 2, 1, None, 0, 0, 0, None, None) == -1
    assert lib.dnmf_hals_spatial(a, a, a, None, 0.0, 4, 2, 0, None, 0, 0, 0, None, None) == -2 and b"sweeps" in lib.dnmf_last_error()
    assert lib.dnmf_hals_spatial(a, a, a, None, 0.0, 4, 2, 1, a, 2, 3, 1, None, None) == -2 and b"boxes" in lib.dnmf_last_error()
    assert lib.dnmf_hals_spatial(a, a, a, None, 0.0, 4, 70000, 1, None, 0, 0, 0, None, None) != 0
    assert lib.dnmf_hals_spatial_kkt(a, a, a, None, 0.0, 4, 2, None, 0, 0, 0, None, None) == -1
    assert lib.dnmf_hals_spatial_lists(a, a, a, a, None, 0.0, 4, 4, 1, 2, a, None, 1, None, None, 0, None) == -1
    assert lib.dnmf_hals_spatial_lists(a, a, a, a, None, 0.0, 4, 4, 1, 2, a, a, 0, None, None, 0, None) == -2
    rc = lib.dnmf_hals_spatial_lists(a, a, a, a, None, 0.0, 4, 4, 1, 2, a, a, 1, a, None, 0, None)
    assert rc != 0 and b"workspace" in lib.dnmf_last_error()
    assert lib.dnmf_hals_spatial_lists_workspace(512, 512, 1) == 128 * 8 * 32 * 8 and lib.dnmf_hals_spatial_lists_workspace(0, 4, 1) == 0


def test_boxes_and_entries_helpers():
    sz = (9, 7, 2)
    b = np.array([[0, 2, 1, 3, 0, 1], [7, 8, 5, 6, 1, 1], [9, -1, 7, -1, 2, -1]])
    g = R.dilate_boxes(b, sz, (2, 1, 0))
    assert g.tolist() == [[0, 4, 0, 4, 0, 1], [5, 8, 4, 6, 1, 1], [9, -1, 7, -1, 2, -1]]     # clipped; the empty box stays
    M = R.box_mask(g, sz)
    assert M.shape == (126, 3) and M[:, 0].sum() == 5 * 5 * 2 and M[:, 1].sum() == 4 * 3 and M[:, 2].sum() == 0
    A = np.zeros((126, 3))
    A[M[:, 1], 1] = 1.0
    assert R.support_boxes(A, sz).tolist()[1] == g[1].tolist() and R.support_boxes(A, sz)[2, 0] > R.support_boxes(A, sz)[2, 1]
