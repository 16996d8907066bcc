"""The definition of the AR(1)-constrained trace update (K32) in float64, numpy only.  The kernel (dnmf_amd/csrc/ar1_temporal.hip),
``ops.ar1_temporal``, the documents and the tests refer to this file.

The state is C (K, T) for T consecutive frames in time order, on the Gram data G (T, K, K), r (T, K).  Per neuron a decay g_k in
[0, 1), a penalty lam_k >= 0 and a baseline b_k.  With x = C[k, :] - b_k, s_{k,0} = x_0 >= 0 and s_{k,t} = x_t - g_k x_{t-1} >= 0,

    F(C) = sum_t (1/2 c_t^T G_t c_t - r_t^T c_t) + sum_k lam_k sum_t s_{k,t}.

A1  The list of row k: the columns the neighbour table names for it and k itself, ascending, each once; entries outside [0, K) are
    padding.  Without a table: every column.
A2  The terms of row k: w_t = G_t[k, k], y_t = C[k, t] + (r_t[k] - sum_l G_t[k, l] C[l, t]) / w_t, the sum over the list in its order,
    one product and one addition a term, from 0.  A frame with w_t not finite or <= 0, or with y_t not finite, carries no weight.
A3  The row step: row k becomes the exact minimiser of F over that row, the others fixed.  With g_k > 0 that is b_k plus the
    minimiser of 1/2 sum_t w_t (y_t - b_k - x_t)^2 + lam_k sum_t s_t under the constraints: D1 of tests/deconv_restatement.py with
    the per-frame terms a_t = w_t (y_t - b_k) - lam_k mu_t and d_t = w_t (a_t = -lam_k mu_t, d_t = 0 without weight; mu_t = 1 - g_k,
    1 on the last frame), solved by its pool-adjacent-violators and expanded by its ``expand``: the trace decays through a frame
    without weight as K21's does through a missing frame.  With g_k = 0 the constraints couple nothing and the step is the plain
    coordinate step x_t = max(0, y_t - b_k - lam_k / w_t), x_t = 0 without weight, s = x: a branch of its own that never forms
    log 0 (with b_k = 0 this is max(0, y_t - lam_k / w_t); the baseline enters as it must for the step to minimise F).
A4  The colours: a greedy colouring of the overlap graph -- k ascending, the smallest colour no neighbour holds.  k and l are
    neighbours when the list of one names the other; without a table, when G_t[k, l] != 0 or G_t[l, k] != 0 in any frame.
A5  One sweep: the colours in ascending order; the neurons of one colour share no Gram entry, so their row steps do not see each
    other -- here they run k ascending.
"""
import numpy as np

import deconv_restatement as DR


def per_neuron(v, K):
    return np.broadcast_to(np.asarray(v, np.float64), (K,)).copy()


def neighbour_lists(K, nbr=None):
    """A1 -> K int arrays."""
    if nbr is None:
        return [np.arange(K)] * K
    nbr = np.asarray(nbr)
    out = []
    for k in range(K):
        row = nbr[k]
        out.append(np.unique(np.concatenate([row[(row >= 0) & (row < K)], [k]])).astype(np.int64))
    return out


def pattern_of(G):
    """The overlap pattern (K, K) bool of Gram data (T, K, K): an entry that is not zero in any frame, either way round."""
    nz = (np.asarray(G) != 0).any(0)
    return nz | nz.T


def adjacency(K, nbr=None, pattern=None):
    """A4's graph (K, K) bool, symmetric, without the diagonal."""
    if nbr is not None:
        adj = np.zeros((K, K), bool)
        for k, lst in enumerate(neighbour_lists(K, nbr)):
            adj[k, lst] = True
    else:
        adj = np.array(pattern, bool)
    adj = adj | adj.T
    adj[np.arange(K), np.arange(K)] = False
    return adj


def trace_colours(adj):
    """A4 -> ``(colour (K,) int32, n_colours)``."""
    K = len(adj)
    colour = np.full(K, -1, np.int32)
    for k in range(K):
        taken = set(colour[np.flatnonzero(adj[k])].tolist())
        c = 0
        while c in taken:
            c += 1
        colour[k] = c
    return colour, int(colour.max()) + 1 if K else 0


def row_terms(G, r, C, k, lst):
    """A2 -> ``(w, y)`` (T,) each; G (T, K, K), r (T, K), C (K, T) float64."""
    w = G[:, k, k]
    acc = np.zeros(C.shape[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        for l in lst:
            acc = acc + G[:, k, l] * C[l]
        y = C[k] + (r[:, k] - acc) / w
    return w, y


def weighted(w, y):
    return np.isfinite(w) & (w > 0) & np.isfinite(y)


def row_pools(w, y, g, lam, b):
    """A3's terms and pools for g > 0 -> ``(a, d, pools)``."""
    T = len(y)
    ok = weighted(w, y)
    mu = np.full(T, 1.0 - g)
    mu[T - 1] = 1.0
    a = np.where(ok, np.where(ok, w, 0.0) * (np.where(ok, y, 0.0) - b), 0.0) - lam * mu
    d = np.where(ok, w, 0.0)
    return a, d, DR.pava(a, d, g)


def row_step(w, y, g, lam, b):
    """A3 -> ``(row, s, n_pools, n_weightless)``."""
    w, y = np.asarray(w, np.float64), np.asarray(y, np.float64)
    T = len(y)
    ok = weighted(w, y)
    if not g > 0.0:
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.where(ok, np.maximum(0.0, (np.where(ok, y, 0.0) - b) - lam / np.where(ok, w, 1.0)), 0.0)
        return x + b, x.copy(), T, int((~ok).sum())
    _, _, pools = row_pools(w, y, g, lam, b)
    c, s = DR.expand(pools, g, T)
    return b + c, s, len(pools[0]), int((~ok).sum())


def ar1_temporal(G, r, C, g, penalty=0.0, baseline=0.0, sweeps=1, nbr=None, order=None):
    """``sweeps`` sweeps (A5) from C (K, T) -> ``(C (K, T) float64, s (K, T), info)``; ``info``: ``colour``, ``n_colours``, ``n_pools``
    and ``n_weightless`` (K,) of the last step of every row.  ``order``: per colour the order of its neurons (a test's argument: the
    result does not depend on it); default ascending."""
    G, r = np.asarray(G, np.float64), np.asarray(r, np.float64)
    C = np.array(C, np.float64)
    K, T = C.shape
    g, lam, b = per_neuron(g, K), per_neuron(penalty, K), per_neuron(baseline, K)
    lists = neighbour_lists(K, nbr)
    colour, n_colours = trace_colours(adjacency(K, nbr, None if nbr is not None else pattern_of(G)))
    s = np.zeros((K, T))
    n_pools, n_weightless = np.zeros(K, np.int32), np.zeros(K, np.int32)
    for _ in range(int(sweeps)):
        for c in range(n_colours):
            ids = np.flatnonzero(colour == c)
            for k in (ids if order is None else order(ids)):
                w, y = row_terms(G, r, C, k, lists[k])
                C[k], s[k], n_pools[k], n_weightless[k] = row_step(w, y, g[k], lam[k], b[k])
    return C, s, dict(colour=colour, n_colours=n_colours, n_pools=n_pools, n_weightless=n_weightless)


def spikes(C, g, b):
    """s of the definition from a state: s_{k,0} = x_0, s_{k,t} = x_t - g_k x_{t-1}."""
    C = np.asarray(C, np.float64)
    K = len(C)
    x = C - per_neuron(b, K)[:, None]
    s = x.copy()
    s[:, 1:] -= per_neuron(g, K)[:, None] * x[:, :-1]
    return s


def objective(G, r, C, g, penalty=0.0, baseline=0.0):
    """F(C), float64."""
    G, r, C = np.asarray(G, np.float64), np.asarray(r, np.float64), np.asarray(C, np.float64)
    K = len(C)
    f = 0.5 * np.einsum("kt,tkl,lt->", C, G, C) - np.einsum("tk,kt->", r, C)
    return float(f + (per_neuron(penalty, K) * spikes(C, g, baseline).sum(1)).sum())


def row_kkt(w, y, g, lam, b, row, s):
    """The certificate of one row step that knows nothing of pools -> ``(min s, min grad, max |grad s|)``: with the lower-triangular
    K_ij = g^(i-j), x = K s, and the gradient of 1/2 sum w (y - b - x)^2 + lam sum s with respect to s is K^T W (x - (y - b)) + lam.
    The row solves A3 when s >= 0, grad >= 0 and grad s = 0."""
    w, y = np.asarray(w, np.float64), np.asarray(y, np.float64)
    T = len(y)
    ok = weighted(w, y)
    i = np.arange(T)
    Kmat = np.tril(g ** np.clip(i[:, None] - i[None, :], 0, None).astype(np.float64)) if g > 0 else np.eye(T)
    x = np.asarray(row, np.float64) - b
    grad = Kmat.T @ np.where(ok, np.where(ok, w, 0.0) * (x - (np.where(ok, y, 0.0) - b)), 0.0) + lam
    s = np.asarray(s, np.float64)
    return float(s.min()), float(grad.min()), float(np.abs(grad * s).max())
