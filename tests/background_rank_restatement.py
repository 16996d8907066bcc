"""The definition of K23 (``dnmf_background_dots_rank / _accum_rank / _subtract_rank``, ``ops.background_fit_rank``) in float64
numpy, written plainly: a static, non-negative, rank-R background ``sum_j b_j (x) f_j`` fitted on the residual ``r = frames - sub``
by alternating block steps, each block step solved by cyclic coordinate sweeps, and its subtraction.

frames, sub and r as in tests/background_restatement.py.  B is (R, P) fp32, F is (R, T) fp32, 2 <= R <= 8.  Every product and sum
is float64; a value is rounded to fp32 only where the GPU stores it as fp32: the new F after an f-step, the new B after a b-step, and
the output of ``subtract``.

    f-step   N[j, t] = sum_p b_j[p] r[t, p],  Q = B B^T (R x R);  per frame, from the frame's current f, ``inner`` sweeps
             f_j <- max(0, (N_j - sum_{i != j} Q_ji f_i) / Q_jj), j = 0 .. R-1, 0 where Q_jj == 0;  then one rounding to fp32
    b-step   N[j, p] = sum_t f_j[t] r[t, p],  W = F F^T;  per voxel the same sweeps from the voxel's current b

A sweep is exact coordinate descent on ``|r_t - sum_j b_j f_j|^2`` over f >= 0 (on ``|r_p - ...|^2`` over b >= 0): no coordinate
update raises the squared error.  ``inner`` is a parameter of the algorithm, not a tolerance.
"""
import numpy as np

from background_restatement import residual

R_MIN, R_MAX = 2, 8


def _rows(x, R=None):
    x = np.asarray(x, dtype=np.float32)
    x = x.reshape(x.shape[0], -1).astype(np.float64)
    assert R is None or x.shape[0] == R
    return x


def dots(frames, B, sub=None):
    """-> (N (R, T) float64, Q (R, R) float64): N[j, t] = sum_p b_j[p] r[t, p], Q = B B^T."""
    r, Bd = residual(frames, sub), _rows(B)
    return np.stack([(r * Bd[j][None, :]).sum(1) for j in range(len(Bd))]), gram(Bd)


def accum(frames, F, sub=None):
    """-> (N (R, P) float64, W (R, R) float64): N[j, p] = sum_t f_j[t] r[t, p], W = F F^T."""
    r, Fd = residual(frames, sub), _rows(F)
    return np.stack([(r * Fd[j][:, None]).sum(0) for j in range(len(Fd))]), gram(Fd)


def gram(X):
    """X X^T of (R, n) rows, float64."""
    X = _rows(X)
    return np.array([[(X[j] * X[i]).sum() for i in range(len(X))] for j in range(len(X))])


def dots_terms(frames, B, sub=None):
    """(R, T): sum_p |b_j[p] r[t, p]|, what the error of a float64 sum of these terms scales with."""
    r, Bd = residual(frames, sub), _rows(B)
    return np.stack([np.abs(r * Bd[j][None, :]).sum(1) for j in range(len(Bd))])


def accum_terms(frames, F, sub=None):
    """(R, P): sum_t |f_j[t] r[t, p]|."""
    r, Fd = residual(frames, sub), _rows(F)
    return np.stack([np.abs(r * Fd[j][:, None]).sum(0) for j in range(len(Fd))])


def gram_terms(X):
    """(R, R): sum_n |x_j[n] x_i[n]|."""
    X = _rows(X)
    return np.array([[np.abs(X[j] * X[i]).sum() for i in range(len(X))] for j in range(len(X))])


def sweep64(N, G, x0, inner=3):
    """``inner`` cyclic sweeps over j = 0 .. R-1 for every column of N (R, n) from x0 (R, n), in float64 -> (R, n) float64.  The
    products and differences are taken one by one, i ascending: the GPU does the same operations in the same order."""
    N, G = np.asarray(N, dtype=np.float64), np.asarray(G, dtype=np.float64)
    x = np.array(x0, dtype=np.float64)
    R = len(G)
    assert N.shape == x.shape and N.shape[0] == R and G.shape == (R, R)
    for _ in range(int(inner)):
        for j in range(R):
            if G[j, j] == 0:
                x[j] = 0.0
                continue
            s = N[j].copy()
            for i in range(R):
                if i != j:
                    s = s - G[j, i] * x[i]
            x[j] = np.maximum(0.0, s / G[j, j])
    return x


def sweep(N, G, x0, inner=3):
    """``sweep64`` from the fp32 values x0, rounded once to fp32."""
    return sweep64(N, G, np.asarray(x0, dtype=np.float32).astype(np.float64), inner).astype(np.float32)


def f_step(r, B, F, inner=3):
    """The f-step on the residual r (T, P) float64 -> F (R, T) fp32."""
    Bd = _rows(B)
    return sweep(np.stack([(r * Bd[j][None, :]).sum(1) for j in range(len(Bd))]), gram(Bd), F, inner)


def b_step(r, B, F, inner=3):
    """The b-step on the residual r -> B (R, P) fp32."""
    Fd = _rows(F)
    return sweep(np.stack([(r * Fd[j][:, None]).sum(0) for j in range(len(Fd))]), gram(Fd), B, inner)


def sqerr(r, B, F):
    """sum (r - sum_j b_j f_j)^2 in float64."""
    return float(((r - _rows(F).T @ _rows(B)) ** 2).sum())


def start(T, P, R):
    """F = the indicators of R contiguous blocks of the frame times (component j owns the t with (t R) // T == j), B = 0."""
    if not R_MIN <= R <= R_MAX:
        raise ValueError(f"rank {R} outside {R_MIN} .. {R_MAX}")
    if R > T:
        raise ValueError(f"rank {R} for {T} frames")
    F = np.zeros((R, T), dtype=np.float32)
    F[(np.arange(T) * R) // T, np.arange(T)] = 1.0
    return np.zeros((R, P), dtype=np.float32), F


def fit(frames, iters, rank, inner=3, sub=None, history=None):
    """The start, one b-step (W is diagonal there: b_j is the clipped mean residual of block j), ``iters`` times (f-step, b-step),
    then per component the scale that makes mean(f_j) = 1 (skipped where f_j is all zero) -> (B (R, P) fp32, F (R, T) fp32).
    ``history``: a list that receives the squared error after the start and after every half-step."""
    r = residual(frames, sub)
    T, P = r.shape
    B, F = start(T, P, int(rank))
    B = b_step(r, B, F, inner)
    if history is not None:
        history.append(sqerr(r, B, F))
    for _ in range(int(iters)):
        F = f_step(r, B, F, inner)
        if history is not None:
            history.append(sqerr(r, B, F))
        B = b_step(r, B, F, inner)
        if history is not None:
            history.append(sqerr(r, B, F))
    return rescale(B, F)


def rescale(B, F):
    """Per component (b_j s_j, f_j / s_j) in fp32 with s_j = the fp32 mean of f_j; unchanged where f_j is all zero."""
    B, F = B.copy(), F.copy()
    for j in range(len(F)):
        s = np.float32(F[j].astype(np.float64).mean())
        if s > 0:
            B[j], F[j] = (B[j] * s).astype(np.float32), (F[j] / s).astype(np.float32)
    return B, F


def subtract(frames, B, F, clamp=True):
    """fp32(float64(y) - sum_j float64(b_j) float64(f_j[t])), the products added one by one with j ascending, max(., 0) with
    ``clamp``; the shape of ``frames``."""
    y = np.asarray(frames, dtype=np.float32)
    Bd, Fd = _rows(B), _rows(F)
    s = np.zeros((y.shape[0], Bd.shape[1]))
    for j in range(len(Bd)):
        s = s + Fd[j][:, None] * Bd[j][None, :]
    out = y.reshape(y.shape[0], -1).astype(np.float64) - s
    if clamp:
        out = np.maximum(out, 0.0)
    return out.astype(np.float32).reshape(y.shape)
