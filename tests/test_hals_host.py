"""K4h without a GPU: the float64 restatement the GPU tests compare against (tests/hals_restatement.py) reaches the
solution of the non-negative least-squares problem it is written for, and the new wrappers refuse bad arguments before
any launch.

Problems: K overlapping Gaussian bumps on a line of P samples (neighbouring bumps overlap by e^-1, the next ones by
e^-4), G = M^T M and r = M^T y ROUNDED TO fp32 as the kernels receive them, y = M c_true + noise with a third of c_true
zero and noise large enough to pull some coordinates negative (active constraints).  The Gram matrix of such bumps has
its eigenvalues within about 1 -+ 0.8 of the diagonal, so Gauss-Seidel contracts by roughly 0.6 per sweep: 200 sweeps are
far past fp64 convergence.  scipy solves the SAME rounded problem through the Cholesky factor G = L L^T:
min |L^T c - L^-1 r|, c >= 0.

Tolerances: coordinates 1e-9 of max|c| -- scipy's active-set solve and 200 sweeps
each carry fp64 rounding amplified by cond(G) <= ~10 and K <= 40 terms, i.e. ~1e-14, with five orders of room for the
triangular solves; objective 1e-12 relative; kkt after convergence 1e-10 of max|r| (the gradient is a difference of
terms of that size)."""
import ctypes

import numpy as np
import pytest
import torch

import hals_restatement as H


def bumps(K, P, seed, T=3):
    rng = np.random.RandomState(seed)
    spacing = P / (K + 1.0)
    centres = spacing * (1 + np.arange(K)) + rng.uniform(-0.15, 0.15, K) * spacing
    sigma = spacing / 2.0
    M = np.exp(-(np.arange(P)[:, None] - centres[None, :]) ** 2 / (2 * sigma ** 2))
    c_true = rng.rand(K, T) * (rng.rand(K, T) > 0.33)
    Y = M @ c_true + 0.3 * rng.randn(P, T)
    G64 = M.T @ M
    G = np.broadcast_to(((G64 + G64.T) / 2).astype(np.float32), (T, K, K)).copy()
    r = (M.T @ Y).T.astype(np.float32).copy()
    return G, r


def scipy_nnls(G, r):
    from scipy.linalg import solve_triangular
    from scipy.optimize import nnls
    L = np.linalg.cholesky(G.astype(np.float64))
    return nnls(L.T, solve_triangular(L, r.astype(np.float64), lower=True), maxiter=100 * G.shape[0])[0]


@pytest.mark.parametrize("K,P,seed", [(1, 50, 0), (5, 120, 1), (12, 400, 2), (40, 900, 3)])
def test_restatement_reaches_scipy_nnls(K, P, seed):
    G, r = bumps(K, P, seed)
    T = r.shape[0]
    C0 = np.full((K, T), 0.5)
    C = H.hals_temporal(G, r, C0, 0.0, 200)
    want = np.stack([scipy_nnls(G[t], r[t]) for t in range(T)], 1)
    assert (want == 0).any() or K == 1          # the constraint is active somewhere
    dev = np.abs(C - want).max()
    print("K=%d max|dc| %.3e of max|c| %.3e" % (K, dev, np.abs(want).max()))
    assert dev <= 1e-9 * np.abs(want).max()
    f, fw = H.objective(G, r, C), H.objective(G, r, want)
    assert abs(f - fw) <= 1e-12 * abs(fw)
    k = H.kkt(G, r, C)
    print("kkt %.3e of max|r| %.3e" % (k.max(), np.abs(r).max()))
    assert k.max() <= 1e-10 * np.abs(r).max()
    # the start is far from it, and the measure says so
    assert H.kkt(G, r, C0).min() > 1e-3 * np.abs(r).max()


def test_one_sweep_is_the_formula_in_ascending_order():
    """Two coordinates by hand: the second sees the first one's new value."""
    G = np.array([[[2.0, 1.0], [1.0, 4.0]]])
    r = np.array([[2.0, -1.0]])
    C = H.hals_temporal(G, r, np.array([[3.0], [1.0]]), 0.0, 1)
    c0 = (2.0 - 1.0 * 1.0) / 2.0
    c1 = max(0.0, (-1.0 - 1.0 * c0) / 4.0)
    assert C[0, 0] == c0 and C[1, 0] == c1 == 0.0
    # clamped coordinate: its positive gradient does not count, the free one's is zero after one more sweep
    C = H.hals_temporal(G, r, C, 0.0, 1)
    assert H.gradient(G, r, C)[1, 0] > 0 and H.kkt(G, r, C)[0] == 0.0
    # an all-zero row and column with r = 0: d == 0 gives 0
    G3 = np.zeros((1, 3, 3))
    G3[0, :2, :2] = G[0]
    C3 = H.hals_temporal(G3, np.array([[2.0, -1.0, 0.0]]), np.full((3, 1), 0.7), 0.0, 2)
    assert C3[2, 0] == 0.0 and np.array_equal(C3[:2], C)


@pytest.mark.parametrize("T", [1, 2, 3, 6, 9])
def test_objective_never_increases_with_gamma(T):
    """Every coordinate update minimises F along its coordinate, so F is non-increasing sweep by sweep; the red-black
    order and the end frames (n_t = 1; T = 1: n_t = 0) included.  At convergence kkt is at rounding level."""
    G, r = bumps(7, 150, 10 + T, T=T)
    gamma = 3.0
    C = np.full((7, T), 0.5)
    f = [H.objective(G, r, C, gamma)]
    for _ in range(60):
        C = H.hals_temporal(G, r, C, gamma, 1)
        f.append(H.objective(G, r, C, gamma))
    d = np.diff(f)
    assert d.max() <= 1e-13 * abs(f[-1]), d.max()
    assert f[-1] < f[0]
    C = H.hals_temporal(G, r, C, gamma, 400)
    assert H.kkt(G, r, C, gamma).max() <= 1e-10 * np.abs(r).max()
    if T > 1:   # the neighbour term is felt
        assert np.abs(C - H.hals_temporal(G, r, C, 0.0, 400)).max() > 1e-3
    # the gradient of the restatement is the gradient of its objective (central differences on a smooth point)
    Cp = C + 0.25
    g = H.gradient(G, r, Cp, gamma)
    for (k, t) in [(0, 0), (3, T - 1), (6, T // 2)]:
        e = np.zeros_like(Cp)
        e[k, t] = 1e-5
        num = (H.objective(G, r, Cp + e, gamma) - H.objective(G, r, Cp - e, gamma)) / 2e-5
        assert abs(num - g[k, t]) <= 1e-6 * max(1.0, abs(g[k, t]))


# ---- the new wrappers refuse bad arguments before any launch ------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


def test_library_argument_errors_without_a_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    # K > 256: unsupported, and the message names the call
    assert lib.dnmf_hals_temporal(a, a, a, 4, 257, 4, 1, None, 0, None, None) == -3
    assert b"dnmf_hals_temporal:" in lib.dnmf_last_error()
    assert lib.dnmf_hals_temporal_slots(a, 1, 300, a, a, 4, 257, 4, 1, a, 8, None, None) == -3
    assert b"dnmf_hals_temporal_slots" in lib.dnmf_last_error()
    assert lib.dnmf_hals_temporal_step(a, a, a, 4, 257, 4, 0.5, 0, None, 0, None) == -3
    assert b"dnmf_hals_temporal_step" in lib.dnmf_last_error()
    assert lib.dnmf_hals_temporal_kkt(a, a, a, 4, 257, 4, 0.5, None, 0, a, None) == -3
    # NULL buffers, shapes, parity, list widths
    assert lib.dnmf_hals_temporal(None, a, a, 4, 3, 4, 1, None, 0, None, None) == -1
    assert lib.dnmf_hals_temporal(a, a, a, 3, 3, 4, 1, None, 0, None, None) == -2      # ldc < T
    assert lib.dnmf_hals_temporal(a, a, a, 4, 3, 4, -1, None, 0, None, None) == -2     # iters < 0
    assert lib.dnmf_hals_temporal(a, a, a, 4, 3, 4, 1, a, 5, None, None) == -3         # NN not 8 / 16 / 32
    assert lib.dnmf_hals_temporal_slots(a, 1, 300, a, a, 4, 3, 4, 1, None, 8, None, None) == -1   # slots need nbr
    assert lib.dnmf_hals_temporal_slots(a, 1, 3, a, a, 4, 3, 4, 1, a, 8, None, None) == -2        # nslot <= K
    assert lib.dnmf_hals_temporal_step(a, a, a, 4, 3, 4, 0.5, 2, None, 0, None) == -2
    assert b"parity" in lib.dnmf_last_error()
    assert lib.dnmf_hals_temporal_kkt(a, a, a, 4, 3, 4, 0.5, None, 0, None, None) == -1           # kkt is the output


def test_ops_wrappers_check_their_tensors():
    from dnmf_amd import ops
    K, T = 3, 4
    G, r = torch.zeros(T, K, K), torch.zeros(T, K)
    with pytest.raises(ValueError, match="hals_temporal: C must be float32 CUDA"):
        ops.hals_temporal(G, r, torch.zeros(K, T), 1)
    with pytest.raises(ValueError, match="hals_temporal_step: C must be float64 CUDA"):
        ops.hals_temporal_step(G, r, torch.zeros(K, T, dtype=torch.float64), 0.5, 0)
    with pytest.raises(ValueError, match="hals_temporal_kkt: C must be float64 CUDA"):
        ops.hals_temporal_kkt(G, r, torch.zeros(K, T, dtype=torch.float64), 0.5)
    with pytest.raises(ValueError, match="hals_temporal_slots: C must be float32 CUDA"):
        ops.hals_temporal_slots({"nbr": None}, torch.zeros(8), [4, 4, 1], torch.zeros(K, T), 1)
    for fn in (ops.hals_temporal, ops.hals_temporal_slots, ops.hals_temporal_step, ops.hals_temporal_kkt):
        assert callable(fn)


def test_solver_names():
    from dnmf_amd.Demix import dNMF as M
    assert M.SOLVERS == ('mu', 'hals')
    M._check_solver('mu'), M._check_solver('hals')
    with pytest.raises(ValueError, match="solver='newton'"):
        M._check_solver('newton')
    with pytest.raises(ValueError, match="solver="):
        M.DeformableNMF.update_temporal(np.zeros((2, 2, 1, 2, 1)), np.zeros((2, 1)), np.zeros((2, 2, 1, 1)), solver='als')
    # gamma_c != 0 on a sharded time axis is refused, not half-built; everything else passes the gate
    M._hals_refuse_shards(0.5, None), M._hals_refuse_shards(0, object()), M._hals_refuse_shards(None, object())
