"""numpy float64 restatement of K4h, the exact NNLS trace solver (HALS / cyclic coordinate descent), written from the
contract in include/dnmf_hip.h:

    F(C) = sum_t ( 1/2 c_t^T G_t c_t - r_t^T c_t ) + gamma/2 sum_{t=0..T-2} |c_{t+1} - c_t|^2 ,   C >= 0

    d   = G_t[k,k] + gamma n_t                       (n_t real neighbours of frame t: 2 inside, 1 at an end, 0 for T = 1)
    c_k <- d > 0 ? max(0, (r_t[k] - sum_{l != k} G_t[k,l] c_l + gamma (c_{k,t-1} + c_{k,t+1}, real ones only)) / d) : 0

One sweep: k = 0 .. K-1 ascending in every frame; with gamma != 0 all even frames first, then all odd frames.
The tests compare the kernels against these functions; nothing here is fast."""
import numpy as np


def _neighbours(C, ts):
    """(n_t, sum of the real neighbours' columns) for the frames ``ts`` of C (K,T)."""
    T = C.shape[1]
    n = (ts > 0).astype(np.float64) + (ts + 1 < T).astype(np.float64)
    nb = np.zeros((C.shape[0], ts.size))
    has_l, has_r = ts > 0, ts + 1 < T
    nb[:, has_l] += C[:, ts[has_l] - 1]
    nb[:, has_r] += C[:, ts[has_r] + 1]
    return n, nb


def _pass(G, r, C, gamma, ts):
    """k ascending over the frames ``ts`` (which do not see each other), in place on C (K,T) float64."""
    if ts.size == 0:
        return
    K = C.shape[0]
    if gamma != 0:
        n, nb = _neighbours(C, ts)
    else:
        n, nb = np.zeros(ts.size), np.zeros((K, ts.size))
    c = C[:, ts].copy()                       # (K, len(ts))
    Gs, rs = G[ts], r[ts]
    for k in range(K):
        c[k] = 0.0                            # the sum below runs over l != k
        s = np.einsum("tl,lt->t", Gs[:, k, :], c)
        d = Gs[:, k, k] + gamma * n
        num = rs[:, k] - s + gamma * nb[k]
        with np.errstate(divide="ignore", invalid="ignore"):
            c[k] = np.where(d > 0, np.maximum(0.0, num / np.where(d > 0, d, 1.0)), 0.0)
    C[:, ts] = c


def hals_temporal(G, r, C, gamma=0.0, iters=1):
    """``iters`` sweeps from C (K,T); G (T,K,K), r (T,K) any float dtype (taken as float64).  Returns float64 (K,T)."""
    G, r = np.asarray(G, dtype=np.float64), np.asarray(r, dtype=np.float64)
    C = np.array(C, dtype=np.float64)
    gamma = 0.0 if gamma is None else float(gamma)
    T = C.shape[1]
    t = np.arange(T)
    for _ in range(int(iters)):
        if gamma == 0:
            _pass(G, r, C, 0.0, t)
        else:
            _pass(G, r, C, gamma, t[0::2])
            _pass(G, r, C, gamma, t[1::2])
    return C


def gradient(G, r, C, gamma=0.0):
    """grad F as (K,T): G c - r + gamma (n_t c - real neighbours)."""
    G, r = np.asarray(G, dtype=np.float64), np.asarray(r, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    gamma = 0.0 if gamma is None else float(gamma)
    g = np.einsum("tkl,lt->kt", G, C) - r.T
    if gamma != 0:
        n, nb = _neighbours(C, np.arange(C.shape[1]))
        g = g + gamma * (n[None, :] * C - nb)
    return g


def kkt(G, r, C, gamma=0.0):
    """(T): max_k |pg_k|, pg_k = grad_k where c_k > 0, else min(grad_k, 0).  Zero exactly at a solution."""
    C = np.asarray(C, dtype=np.float64)
    g = gradient(G, r, C, gamma)
    return np.abs(np.where(C > 0, g, np.minimum(g, 0.0))).max(0)


def objective(G, r, C, gamma=0.0):
    """F(C), float64."""
    G, r = np.asarray(G, dtype=np.float64), np.asarray(r, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    gamma = 0.0 if gamma is None else float(gamma)
    f = 0.5 * np.einsum("kt,tkl,lt->", C, G, C) - np.einsum("tk,kt->", r, C)
    if gamma != 0 and C.shape[1] > 1:
        f += 0.5 * gamma * float(((C[:, 1:] - C[:, :-1]) ** 2).sum())
    return float(f)
