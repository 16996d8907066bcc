"""Colour learning (K29) without a GPU: the ABI entries, the float64 restatement (tests/colours_restatement.py) against
scipy's NNLS, the planted three-channel model on the restatement alone, the edge rules, and the argument checks of the C entries."""
import ctypes
import inspect

import numpy as np
import pytest

import colours_restatement as R


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


def test_abi_entries_are_declared_and_bound(lib):
    from dnmf_amd import _lib, build, ops
    from dnmf_amd.Demix.dNMF import DeformableNMF, MultiChannelDNMF
    import os
    header = open(os.path.join(os.path.dirname(build.HERE), "include", "dnmf_hip.h")).read()
    for name in ("dnmf_colour_normal_eqs_workspace", "dnmf_colour_normal_eqs", "dnmf_colour_solve"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["dnmf_colour_normal_eqs_workspace"][0] is ctypes.c_size_t
    assert _lib.SIGNATURES["dnmf_colour_normal_eqs"][1][10] is ctypes.c_size_t
    assert "colours.hip" in build.SOURCES
    assert lib.dnmf_version() == _lib.ABI_VERSION == 7

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(ops.colour_normal_eqs) == [("G", E), ("r", E), ("C", E), ("state", None), ("first", True), ("finish", True),
                                             ("out", None)]
    assert params(ops.colour_solve) == [("M", E), ("b", E), ("colours", E), ("sweeps", 10)]
    assert params(ops.colour_kkt) == [("M", E), ("b", E), ("colours", E)]
    assert params(MultiChannelDNMF.update_colours) == [("self", E), ("loader", E), ("sweeps", 10), ("normalise", True),
                                                       ("dry_run", False)]
    assert not hasattr(DeformableNMF, "update_colours")
    assert MultiChannelDNMF.fit is DeformableNMF.fit
    assert inspect.signature(DeformableNMF.fit).parameters["learn_colours"].default == 0


def _random_system(seed, K=7, NC=3, B=45):
    rng = np.random.default_rng(seed)
    At = rng.random((B, 30, K)) * (rng.random((B, 30, K)) < 0.5)
    G = np.einsum("tpk,tpl->tkl", At, At)
    r = rng.standard_normal((NC, B, K)) + 0.4          # a mixed sign: some colours end at zero
    C = rng.random((K, B))
    return G, r, C


def test_normal_eqs_equal_their_definition():
    G, r, C = _random_system(0)
    M, b, Mabs, babs = R.normal_eqs(G, r, C)
    np.testing.assert_allclose(M, np.einsum("tkl,kt,lt->kl", G, C, C), rtol=1e-13)
    np.testing.assert_allclose(b, np.einsum("ctk,kt->ck", r, C), rtol=0, atol=1e-13 * babs.max())
    assert (M == M.T).all()                             # the inner product C[k, t] C[l, t] is formed first
    assert (Mabs >= np.abs(M) * (1 - 1e-14)).all() and (babs >= np.abs(b) * (1 - 1e-14)).all()


def test_restatement_matches_scipy_nnls():
    """1/2 x^T M x - b^T x with M = L L^T is 1/2 |L^T x - L^-1 b|^2 up to a constant: scipy's active-set NNLS on that."""
    from scipy.optimize import nnls
    clamped = 0
    for seed in range(4):
        G, r, C = _random_system(seed)
        M, b, _, _ = R.normal_eqs(G, r, C)
        x, kkt, ok = R.solve(M, b, np.ones_like(b), sweeps=400)
        assert ok.all() and (kkt <= 1e-12).all(), kkt
        assert np.abs(R.kkt(M, b, x) - kkt).max() <= 1e-12
        L = np.linalg.cholesky(M)
        for c in range(b.shape[0]):
            want = nnls(L.T, np.linalg.solve(L, b[c]))[0]
            np.testing.assert_allclose(x[c], want, rtol=0, atol=1e-10)
            assert ((x[c] == 0) == (want == 0)).all()
            clamped += int((want == 0).sum())
    assert clamped > 0                                   # the bound was active somewhere


@pytest.mark.parametrize("depth", [2, 1])
def test_noise_free_planted_model_is_recovered(depth):
    """24 x 20 x depth, K = 6, T = 40, NC = 3, from all-ones colours, one update of 10 sweeps.  Measured, seeds 0-2: colour error
    5.6e-16 .. 1.7e-15, trace error 1.8e-15 .. 4.4e-15 (depth 2 and 1).  The bound is round-off of float64 sums of 40 x 480 (960)
    terms through a system of condition ~ 1, not the measured value."""
    for seed in (0, 1, 2):
        p = R.planted(depth, seed)
        G, r = R.gram_rhs(p["A"], p["video"], 3)
        u = R.update(G, r, p["C"], np.ones((3, 6)), sweeps=10)
        err, errc = np.abs(u["colours"] - p["colours"]).max(), np.abs(u["C"] - p["C"]).max()
        print(f"\ndepth {depth} seed {seed}: colour error {err:.2e}, trace error {errc:.2e}, zero entry "
              f"{u['colours'][p['colours'] == 0]}")
        assert (p["colours"] == 0).sum() == 1
        assert err <= 1e-12 and errc <= 1e-12            # the planted zero included
        assert u["ok"].all() and u["ok_channel"].all()
        assert u["colours"].max(axis=0).tolist() == [1.0] * 6


# the smallest factor start error / error after one update over the seeds 0-2 in float64 (test below), halved
NOISY_FACTOR = {2: 5.44 / 2, 1: 4.55 / 2}


@pytest.mark.parametrize("depth", [2, 1])
def test_noisy_planted_model_moves_towards_the_colours(depth):
    """Noise 0.3 (components_restatement.planted_video's), clamped at 0, true traces, all-ones start (error 1.0).  Measured
    largest colour error after one update of 10 sweeps, seeds 0, 1, 2: depth 2: 0.184, 0.120, 0.150 (factors 5.44, 8.34, 6.66);
    depth 1: 0.163, 0.198, 0.219 (factors 6.12, 5.06, 4.56).  Asserted: below the start's error by the smallest factor, halved."""
    for seed in (0, 1, 2):
        p = R.planted(depth, seed, noise=0.3)
        G, r = R.gram_rhs(p["A"], p["video"], 3)
        u = R.update(G, r, p["C"], np.ones((3, 6)), sweeps=10)
        start, err = np.abs(1.0 - p["colours"]).max(), np.abs(u["colours"] - p["colours"]).max()
        print(f"\ndepth {depth} seed {seed}: colour error {start:.3f} -> {err:.3f} (factor {start / err:.2f})")
        assert err < start / NOISY_FACTOR[depth]
        assert R.objective(u["M"], u["b"], u["colours"] * u["scale"]) < R.objective(u["M"], u["b"], np.ones((3, 6)))


def test_edge_rules():
    G, r, C = _random_system(5)
    old = 0.25 + np.random.default_rng(6).random((3, 7))
    # a neuron with a zero trace: its row and column of M and its b are zero, the sweeps leave it alone, it keeps colours and trace
    C0 = C.copy()
    C0[2] = 0.0
    u = R.update(G, r, C0, old, sweeps=20)
    assert u["ok"].tolist() == [True, True, False, True, True, True, True]
    assert (u["colours"][:, 2] == old[:, 2]).all() and (u["C"][2] == 0).all() and u["scale"][2] == 1.0
    assert u["ok_channel"].all() and np.isfinite(u["kkt"]).all()
    # a NaN in b[c]: the channel keeps its row (then normalised with the others' new entries), and says so
    M, b, _, _ = R.normal_eqs(G, r, C)
    bn = b.copy()
    bn[1, 3] = np.nan
    x, kkt, okc = R.solve(M, bn, old, sweeps=5)
    assert okc.tolist() == [True, False, True] and np.isnan(kkt[1]) and np.isfinite(kkt[[0, 2]]).all()
    assert (x[1] == old[1]).all() and not (x[0] == old[0]).any()
    Mn = M.copy()
    Mn[0, 0] = np.inf
    x, kkt, okc = R.solve(Mn, b, old, sweeps=5)
    assert not okc.any() and (x == old).all() and np.isnan(kkt).all()
    # a coordinate whose M[k, k] is not positive is left alone, the others move
    Mz = M.copy()
    Mz[4, 4] = 0.0
    x, _, okc = R.solve(Mz, b, old, sweeps=3)
    assert okc.all() and (x[:, 4] == old[:, 4]).all() and not (x[:, 0] == old[:, 0]).all()
    # all of a neuron's new colours zero: it keeps its old column and trace
    new = old.copy()
    new[:, 5] = 0.0
    new[1, 6] = np.nan
    col, Cn, scale, ok = R.normalise(new, old, C)
    assert ok.tolist() == [True] * 5 + [False, False]
    assert (col[:, 5:] == old[:, 5:]).all() and (Cn[5:] == C[5:]).all() and (scale[5:] == 1.0).all()
    # normalisation leaves colours[c, k] C[k, t] unchanged to round-off, and the largest colour is 1
    assert (col[:, :5].max(axis=0) == 1.0).all()
    np.testing.assert_allclose(col[:, :, None] * Cn[None, :, :], np.where(ok[None, :, None], new[:, :, None], old[:, :, None])
                               * C[None, :, :], rtol=4e-16)
    # sweeps is what moves the state: more sweeps, a smaller kkt, never a larger objective
    k1, k20 = R.solve(M, b, old, 1)[1], R.solve(M, b, old, 20)[1]
    assert (k20 < k1).all()
    assert R.objective(M, b, R.solve(M, b, old, 20)[0]) <= R.objective(M, b, R.solve(M, b, old, 1)[0]) <= R.objective(M, b, old)


def test_argument_errors_are_reported_without_a_gpu(lib):
    """Every refusal comes before the first HIP call, so it shows on a box without a GPU."""
    buf = ctypes.create_string_buffer(1 << 12)
    addr = ctypes.addressof(buf)

    def eqs(K=4, NC=3, B=8, ldc=8, G=addr, r=addr, C=addr, state=addr, nbytes=1 << 30, M=addr, b=addr, finish=1):
        return lib.dnmf_colour_normal_eqs(G, r, C, ldc, K, NC, B, 1, finish, state, nbytes, M, b, None)

    need = lib.dnmf_colour_normal_eqs_workspace(4, 3, 8)
    # header, the closed sum, the open segment and 2 partial slabs of 16 + 12 doubles, each rounded up to 256 bytes
    assert need == 256 + 4 * 256
    assert lib.dnmf_colour_normal_eqs_workspace(4, 3, 32) == need and lib.dnmf_colour_normal_eqs_workspace(4, 3, 33) == need + 256
    assert eqs(nbytes=need - 1) == -4 and b"state of" in lib.dnmf_last_error()
    assert eqs(state=addr + 4) == -4 and b"aligned" in lib.dnmf_last_error()
    assert eqs(G=None) == -1 and eqs(r=None) == -1 and eqs(C=None) == -1 and eqs(state=None) == -1
    assert eqs(M=None) == -1 and eqs(b=None) == -1
    assert eqs(M=None, b=None, finish=0, nbytes=8) == -4               # both may be NULL without finish
    assert eqs(K=0) == -2 and eqs(NC=0) == -2 and eqs(B=0) == -2 and eqs(ldc=7) == -2
    assert eqs(K=4097) == -3 and b"K=4097" in lib.dnmf_last_error()
    assert eqs(NC=17) == -3 and b"NC=17" in lib.dnmf_last_error()
    assert eqs(B=32 * 65535, ldc=32 * 65535) == -3 and b"segments" in lib.dnmf_last_error()
    for bad in ((0, 3, 8), (4, 0, 8), (4, 3, 0), (4097, 3, 8), (4, 17, 8)):
        assert lib.dnmf_colour_normal_eqs_workspace(*bad) == 0

    def solve(K=4, NC=3, sweeps=2, M=addr, b=addr, col=addr, out=addr, kkt=addr, ok=addr):
        return lib.dnmf_colour_solve(M, b, col, K, NC, sweeps, out, kkt, ok, None)

    assert solve(M=None) == -1 and solve(b=None) == -1 and solve(col=None) == -1 and solve(kkt=None) == -1 and solve(ok=None) == -1
    assert solve(out=None) == -1 and b"out is NULL" in lib.dnmf_last_error()
    assert solve(K=0) == -2 and solve(NC=0) == -2 and solve(sweeps=-1) == -2
    assert solve(K=4097) == -3 and solve(NC=17) == -3
