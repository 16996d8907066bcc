"""The AR(1)-constrained trace update (K32) without a GPU: the float64 restatement (tests/ar1_restatement.py) against K21's
restatement on unit weights, against scikit-learn's weighted isotonic regression and the KKT conditions of the row problem, against
the HALS restatement at g = 0, its objective, constraints and colouring, the planted comparison with HALS, and the ABI, the argument
checks and the solver names on the library as built.

The planted comparison (``ar1_cases.planted_video``: 24 x 20 x {1, 2}, K = 6 with two overlapping pairs, T = 120, noise 1.0 a
voxel, 3 sweeps from C = 1, penalty 1, the true g and baseline): median correlation of the traces with the planted ones, measured

    Z  seed   HALS     'ar1'    gap
    1   0    0.7660   0.9106   0.1446
    1   1    0.7242   0.8907   0.1664
    1   2    0.7076   0.8886   0.1811
    2   0    0.8228   0.9405   0.1178
    2   1    0.8066   0.9400   0.1334
    2   2    0.8230   0.9453   0.1223

the smallest gap 0.1178: the test asserts half of it, 0.0589, as the margin.  (At noise 0.5 the smallest gap is 0.044, at noise 2.0
it is 0.161: the gap grows with the noise, as it should where the AR(1) model is what tells a neuron's light from the noise.)
"""
import ctypes
import functools
import inspect

import numpy as np
import pytest

import ar1_cases as AC
import ar1_restatement as R
import deconv_restatement as DR
import hals_restatement as H

G = AC.G_TRUE
PLANTED_NOISE, PLANTED_SWEEPS, PLANTED_PENALTY, PLANTED_MARGIN = 1.0, 3, 1.0, 0.0589


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


def noisy_trace(T, seed, noise=0.1, baseline=1.0):
    rng = np.random.RandomState(seed)
    return AC.ar1_traces(rng, 1, T, baseline=baseline)[0] + noise * rng.randn(T)


# ---- 1. the row step against independent statements ----------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 0.5, 2.0])
def test_unit_weights_give_the_k21_solve(lam):
    T = 300
    y = noisy_trace(T, 21)
    y[[4, 100, 101, T - 1]] = np.nan                            # K21's missing frames are K32's frames without weight
    want_c, want_s, pools = DR.solve(y, G, lam, 1.0)
    row, s, n_pools, n_weightless = R.row_step(np.ones(T), y, G, lam, 1.0)
    assert np.array_equal(row, 1.0 + want_c) and np.array_equal(s, want_s)
    assert n_pools == len(pools[0]) and n_weightless == 4
    # the same through the whole update: K = 1, G = 1, r = y, from C = 0 the target is r itself
    ok = np.isfinite(y)
    Gm, r = np.where(ok, 1.0, 0.0)[:, None, None], np.where(ok, y, 5.0)[:, None]
    C, s1, info = R.ar1_temporal(Gm, r, np.zeros((1, T)), G, lam, 1.0)
    assert np.array_equal(C[0], row) and np.array_equal(s1[0], s)
    assert info["n_colours"] == 1 and info["n_pools"][0] == n_pools and info["n_weightless"][0] == 4


@pytest.mark.parametrize("lam", [0.0, 0.5, 2.0])
def test_weighted_rows_are_the_weighted_isotonic_regression(lam):
    isotonic = pytest.importorskip("sklearn.isotonic")
    T = 300
    assert T * abs(np.log(G)) < 300                             # g^-t stays finite
    rng = np.random.RandomState(22)
    y, w, b = noisy_trace(T, 23), 0.2 + 3.0 * rng.rand(T), 1.0
    a, d, _ = R.row_pools(w, y, G, lam, b)
    t = np.arange(T)
    # x_t = c_t g^-t: minimise sum d_t g^2t (a_t / (d_t g^t) - x_t)^2 under x increasing
    x = isotonic.isotonic_regression(a / (d * G ** t), sample_weight=d * G ** (2 * t), increasing=True)
    want = np.maximum(x, 0.0) * G ** t
    row, s, _, _ = R.row_step(w, y, G, lam, b)
    assert np.abs(row - b - want).max() <= 1e-12 * np.abs(y).max()


@pytest.mark.parametrize("lam", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("g", [G, 0.5, 0.0])
def test_row_step_meets_the_kkt_conditions(g, lam):
    T = 300
    rng = np.random.RandomState(24)
    y, w, b = noisy_trace(T, 25), 0.2 + 3.0 * rng.rand(T), 1.0
    w[[0, 1, 50, 51, 52, T - 1]] = 0.0                          # leading, in the middle, trailing
    w[120], y[130] = np.nan, np.inf
    row, s, _, n_weightless = R.row_step(w, y, g, lam, b)
    assert n_weightless == 8
    smin, gmin, comp = R.row_kkt(w, y, g, lam, b, row, s)
    scale = 3.2 * np.abs(y[np.isfinite(y)]).max()
    assert smin >= 0.0 and gmin >= -1e-11 * scale and comp <= 1e-11 * scale
    # c = K s: s are the spikes of the row
    assert np.abs(R.spikes(row[None], g, b)[0] - s).max() <= 1e-12 * scale


# ---- 2. g = 0 is the HALS sweep ------------------------------------------------------------------------------------------------
def test_plain_sweep_is_hals_with_one_colour_per_neuron():
    K, T = 5, 40
    Gm, r, c, _ = AC.gram_data(K, T, 31, pattern=np.ones((K, K), bool))
    C0 = np.abs(np.random.RandomState(32).randn(K, T))
    C, s, info = R.ar1_temporal(Gm, r, C0, 0.0, 0.0, 0.0, sweeps=2)
    assert info["n_colours"] == K and np.array_equal(info["colour"], np.arange(K))
    want = H.hals_temporal(Gm, r, C0, 0.0, 2)
    assert np.abs(C - want).max() <= 1e-13 * np.abs(want).max()
    assert np.array_equal(s, C)                                  # g = 0, b = 0: the spikes are the trace


def test_plain_sweep_is_hals_where_the_colours_keep_the_ascending_order():
    # a triangle, a pair and a lone neuron: every edge (k, l), k < l, has colour[k] < colour[l], so the colour order visits the
    # two ends of every edge in ascending order and Gauss-Seidel cannot tell the two sweeps apart
    K, T = 6, 40
    pat = AC.band_pattern(K, edges=[(0, 1), (0, 2), (1, 2), (3, 4)])
    Gm, r, c, _ = AC.gram_data(K, T, 33, pattern=pat)
    C0 = np.abs(np.random.RandomState(34).randn(K, T))
    for nbr in (None, AC.nbr_table(pat)):
        C, s, info = R.ar1_temporal(Gm, r, C0, 0.0, 0.0, 0.0, sweeps=2, nbr=nbr)
        assert np.array_equal(info["colour"], [0, 1, 2, 0, 1, 0]) and info["n_colours"] == 3
        want = H.hals_temporal(Gm, r, C0, 0.0, 2)
        assert np.abs(C - want).max() <= 1e-13 * np.abs(want).max()


# ---- 3. objective, constraints, colouring --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def general_case():
    K, T = 7, 90
    Gm, r, c, pat = AC.gram_data(K, T, 41)
    g = np.array([G, 0.5, 0.0, G, 0.9, G, 0.3])
    lam = np.array([0.0, 0.3, 0.2, 1.0, 0.0, 0.1, 0.5])
    b = np.array([1.0, 0.5, 1.0, 0.0, 1.0, 1.2, 1.0])
    return Gm.astype(np.float64), r.astype(np.float64), np.full((K, T), 1.5), g, lam, b, pat


def test_no_row_step_raises_the_objective():
    Gm, r, C, g, lam, b, pat = general_case()
    K = len(C)
    lists = R.neighbour_lists(K, AC.nbr_table(pat))
    C = C.copy()
    f = R.objective(Gm, r, C, g, lam, b)
    scale = abs(f)
    for sweep in range(3):
        for k in range(K):
            w, y = R.row_terms(Gm, r, C, k, lists[k])
            C[k] = R.row_step(w, y, g[k], lam[k], b[k])[0]
            f1 = R.objective(Gm, r, C, g, lam, b)
            assert f1 <= f + 1e-12 * scale, (sweep, k)
            f = f1
    assert f < -0.1 * scale or f < 0.9 * scale                  # and it went somewhere


def test_constraints_hold_after_every_sweep():
    Gm, r, C, g, lam, b, pat = general_case()
    for sweeps in (1, 2, 3):
        C1, s, info = R.ar1_temporal(Gm, r, C, g, lam, b, sweeps=sweeps, nbr=AC.nbr_table(pat))
        scale = np.abs(C1).max()
        assert s.min() >= 0.0                                    # the solver's own spikes: exact zeros inside a pool
        recomputed = R.spikes(C1, g, b)                          # from the expanded rows: zero up to their rounding
        assert recomputed.min() >= -1e-14 * scale and (C1[:, 0] - b).min() >= 0.0
        assert np.abs(recomputed - s).max() <= 1e-14 * scale


def test_no_two_neighbours_share_a_colour():
    from dnmf_amd import ops
    for K, seed in ((1, 0), (2, 1), (9, 2), (40, 3)):
        rng = np.random.RandomState(seed)
        pat = np.eye(K, dtype=bool) | (rng.rand(K, K) < 0.15)
        nbr = AC.nbr_table(pat)                                  # not symmetric: either direction makes neighbours
        adj = R.adjacency(K, nbr)
        colour, n = R.trace_colours(adj)
        assert n == colour.max() + 1 and (colour >= 0).all()
        kk, ll = np.nonzero(adj)
        assert (colour[kk] != colour[ll]).all()
        for k in range(K):                                       # greedy: every smaller colour is held by a neighbour
            assert set(range(colour[k])) <= set(colour[np.flatnonzero(adj[k])].tolist())
        for arg in (nbr, pat | pat.T):
            got, gn = ops.trace_colours(arg)
            assert got.dtype == np.int32 and gn == n and np.array_equal(got, colour)


def test_a_colour_gives_the_same_bits_in_any_order():
    Gm, r, C, g, lam, b, pat = general_case()
    nbr = AC.nbr_table(pat)
    want = R.ar1_temporal(Gm, r, C, g, lam, b, sweeps=2, nbr=nbr)
    rng = np.random.RandomState(5)
    for order in (lambda ids: ids[::-1], lambda ids: rng.permutation(ids)):
        got = R.ar1_temporal(Gm, r, C, g, lam, b, sweeps=2, nbr=nbr, order=order)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert want[2]["n_colours"] < len(C)                         # some colour holds several neurons


# ---- 4. planted data: the AR(1) update reads the traces out better than HALS -----------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("Z", [1, 2])
def test_planted_traces_are_read_out_better_than_by_hals(Z, seed):
    Gm, r, truth, pat = AC.planted_video(Z, seed, PLANTED_NOISE)
    assert pat[0, 1] and pat[2, 3] and not pat[0, 2] and not pat[4, 5]
    C0 = np.ones_like(truth)
    hals = H.hals_temporal(Gm, r, C0, 0.0, PLANTED_SWEEPS)
    ar1 = R.ar1_temporal(Gm, r, C0, G, PLANTED_PENALTY, 1.0, sweeps=PLANTED_SWEEPS)[0]
    ch, ca = AC.median_correlation(hals, truth), AC.median_correlation(ar1, truth)
    print(f"planted Z={Z} seed={seed}: HALS {ch:.4f} ar1 {ca:.4f} gap {ca - ch:.4f}")
    assert ca >= ch + PLANTED_MARGIN


# ---- 5. the ABI, the argument checks, the solver names -----------------------------------------------------------------------------
def test_abi_entry(lib):
    from dnmf_amd import _lib, build
    res, args = _lib.SIGNATURES["dnmf_ar1_temporal_step"]
    assert res is ctypes.c_int and len(args) == 17
    assert lib.dnmf_ar1_temporal_step
    assert "ar1_temporal.hip" in build.SOURCES


def test_library_argument_errors_without_a_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    run = lib.dnmf_ar1_temporal_step
    # every call here is refused before a launch; nbr may be NULL (the shape errors below are reached with it), nothing else
    for i in (0, 1, 2, 6, 8, 9, 10, 13, 15):
        args = [a, a, a, 4, 3, 4, a, 1, a, a, a, None, 0, a, 4, a, None]
        args[i] = None
        assert run(*args) == -1, i
    assert run(a, a, a, 3, 3, 4, a, 1, a, a, a, None, 0, a, 4, a, None) == -2            # ldc < T
    assert run(a, a, a, 4, 3, 4, a, 1, a, a, a, None, 0, a, 3, a, None) == -2            # lds < T
    assert run(a, a, a, 4, 3, 4, a, 0, a, a, a, None, 0, a, 4, a, None) == -2            # no neuron listed
    assert run(a, a, a, 4, 3, 4, a, 4, a, a, a, None, 0, a, 4, a, None) == -2            # more listed than there are
    assert run(a, a, a, 4, 3, 4, a, 1, a, a, a, a, 0, a, 4, a, None) == -2               # a table without columns
    assert run(a, a, a, 6145, 3, 6145, a, 1, a, a, a, None, 0, a, 6145, a, None) == -3   # T > 6144: refused, not cut
    assert b"dnmf_ar1_temporal_step" in lib.dnmf_last_error() and b"6144" in lib.dnmf_last_error()
    assert run(a, a, a, 4, 4097, 4, a, 1, a, a, a, None, 0, a, 4, a, None) == -3         # K > 4096


def test_ops_signatures_and_checks():
    import torch
    from dnmf_amd import ops

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(ops.trace_colours) == [("nbr_or_pattern", E)]
    assert params(ops.ar1_temporal_step) == [("G", E), ("r", E), ("C64", E), ("ids", E), ("g", E), ("penalty", E), ("baseline", E),
                                             ("nbr", None), ("s", None)]
    assert params(ops.ar1_temporal) == [("G", E), ("r", E), ("C", E), ("g", E), ("penalty", 0.0), ("baseline", 0.0), ("sweeps", 1),
                                        ("nbr", None)]
    assert ops.AR1_MAX_FRAMES == 6144 and ops.AR1_MAX_K == 4096
    K, T = 3, 4
    Gm, r = torch.zeros(T, K, K), torch.zeros(T, K)
    with pytest.raises(ValueError, match="ar1_temporal: C must be float32 CUDA"):
        ops.ar1_temporal(Gm, r, torch.zeros(K, T), 0.5)
    with pytest.raises(ValueError, match="ar1_temporal_step: the state must be float64 CUDA"):
        ops.ar1_temporal_step(Gm, r, torch.zeros(K, T, dtype=torch.float64), [0], 0.5, 0.0, 0.0)
    with pytest.raises(ValueError, match="trace_colours"):
        ops.trace_colours(np.zeros(3, np.int32))
    for name, bad in (("g", 1.0), ("g", -0.1), ("g", float("nan")), ("g", [0.5, 0.5, 1.5]), ("penalty", -1.0), ("penalty", [0.0, 0.0]),
                      ("baseline", float("inf"))):
        kw = dict(g=0.5, penalty=0.0, baseline=0.0)
        kw[name] = bad
        with pytest.raises(ValueError, match=f"ar1: {name}"):
            ops._ar1_params("ar1", K, "cpu", **kw)
    got = ops._ar1_params("ar1", K, "cpu", 0.0, [0.0, 1.0, 2.0], np.float32(1.5))
    assert [t.dtype for t in got] == [torch.float64] * 3 and got[1].tolist() == [0.0, 1.0, 2.0] and got[2].tolist() == [1.5] * 3


def test_neighbour_lists_as_the_kernel_walks_them():
    import torch
    from dnmf_amd import ops
    rng = np.random.RandomState(7)
    K = 9
    nbr = rng.randint(-2, K + 2, size=(K, 5)).astype(np.int32)   # padding on both sides, repeats, rows without themselves
    got = ops._ar1_lists(torch.from_numpy(nbr), K).numpy()
    assert got.dtype == np.int32 and got.shape == (K, 6)
    for k, want in enumerate(R.neighbour_lists(K, nbr)):
        assert np.array_equal(got[k, :len(want)], want) and (got[k, len(want):] == -1).all()


def test_solver_names():
    from dnmf_amd.Demix import dNMF as M
    assert M.TRACE_SOLVERS == ('mu', 'hals', 'ar1') and M.SOLVERS == ('mu', 'hals')
    M._check_trace_solver('ar1')
    with pytest.raises(ValueError, match="solver='ar1'"):
        M._check_solver('ar1')                                   # the footprint solvers and the static updates do not take it
    with pytest.raises(ValueError, match="solver='ar2'"):
        M._check_trace_solver('ar2')
    with pytest.raises(ValueError, match="solver="):
        M.DeformableNMF.update_temporal(np.zeros((2, 2, 1, 2, 1)), np.zeros((2, 1)), np.zeros((2, 2, 1, 1)), solver='ar1')
    with pytest.raises(ValueError, match="solver="):
        M.DeformableNMF.update_spatial(np.zeros((2, 2, 2)), np.zeros((2, 1)), np.zeros((2, 2, 1)), solver='ar1')
    for fn in (M.DeformableNMF.update_footprints, M.DeformableNMF.fit):
        p = inspect.signature(fn).parameters
        assert (p["ar_g"].default, p["ar_penalty"].default, p["ar_baseline"].default) == (None, 0.0, 0.0) and p["solver"].default == 'mu'
    assert "ar1" not in str(inspect.signature(M.DeformableNMF.update_temporal))


def test_objective_in_chunks_is_the_restatement():
    import torch
    from dnmf_amd.Demix import dNMF as M
    Gm, r, C, g, lam, b, pat = general_case()
    C = C + np.random.RandomState(3).rand(*C.shape)
    want = R.objective(Gm, r, C, g, lam, b)
    got = M._ar1_objective(torch.from_numpy(Gm).float(), torch.from_numpy(r).float(), torch.from_numpy(C), torch.from_numpy(g),
                           torch.from_numpy(lam), torch.from_numpy(b), chunk=32)
    assert abs(got - want) <= 1e-12 * abs(want)
    assert abs(M._ar1_objective(torch.from_numpy(Gm).float(), torch.from_numpy(r).float(), torch.from_numpy(C), 0.5, 0.1, 1.0)
               - R.objective(Gm, r, C, 0.5, 0.1, 1.0)) <= 1e-12 * abs(want)
