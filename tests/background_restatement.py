"""The definition of K19 (``dnmf_background_dots / _accum / _subtract``, ``ops.background_fit``) in float64 numpy, written
plainly: a static, non-negative, rank-1 background ``b (x) f`` fitted on the residual ``r = frames - sub`` by alternating exact
coordinate steps (rank-1 HALS), and its subtraction.

frames[t, p]: T frames of P voxels (any trailing shape is flattened), fp32.  ``sub`` (same shape, fp32) is what the model already
predicts; None = nothing.  r = float64(frames) - float64(sub) is exact.  Every product and sum is float64; a value is rounded to
fp32 only where the GPU stores it as fp32: the new f after a ``dots`` step, the new b after an ``accum`` step, and the output of
``subtract``.

    f-step   f_t = fp32(max(0, sum_p b_p r_tp) / sum_p b_p^2), 0 when the denominator is 0
    b-step   b_p = fp32(max(0, sum_t f_t r_tp) / sum_t f_t^2), 0 when the denominator is 0

Each is the exact minimiser of sum_tp (r_tp - b_p f_t)^2 over f >= 0 (over b >= 0) with the other factor held.
"""
import numpy as np


def residual(frames, sub=None):
    """(T, P) float64: float64(frames) - float64(sub)."""
    y = np.asarray(frames, dtype=np.float32)
    r = y.reshape(y.shape[0], -1).astype(np.float64)
    if sub is not None:
        m = np.asarray(sub, dtype=np.float32)
        r = r - m.reshape(m.shape[0], -1).astype(np.float64)
    return r


def dots(frames, b, sub=None):
    """-> (num (T,) float64, bb): num_t = sum_p b_p r_tp, bb = sum_p b_p^2."""
    r = residual(frames, sub)
    bd = np.asarray(b, dtype=np.float32).reshape(-1).astype(np.float64)
    return (r * bd[None, :]).sum(1), float((bd * bd).sum())


def accum(frames, f, sub=None):
    """-> (num (P,) float64, ff): num_p = sum_t f_t r_tp, ff = sum_t f_t^2."""
    r = residual(frames, sub)
    fd = np.asarray(f, dtype=np.float32).reshape(-1).astype(np.float64)
    return (r * fd[:, None]).sum(0), float((fd * fd).sum())


def step(num, den):
    """fp32(max(0, num) / den), 0 when den == 0."""
    if den == 0:
        return np.zeros(num.shape, dtype=np.float32)
    return (np.maximum(num, 0.0) / den).astype(np.float32)


def dots_terms(frames, b, sub=None):
    """sum_p |b_p r_tp| per frame: what the error of a float64 sum of these terms scales with."""
    r = residual(frames, sub)
    bd = np.asarray(b, dtype=np.float32).reshape(-1).astype(np.float64)
    return np.abs(r * bd[None, :]).sum(1)


def accum_terms(frames, f, sub=None):
    """sum_t |f_t r_tp| per voxel."""
    r = residual(frames, sub)
    fd = np.asarray(f, dtype=np.float32).reshape(-1).astype(np.float64)
    return np.abs(r * fd[:, None]).sum(0)


def fit(frames, iters, sub=None):
    """``iters`` times (f-step, b-step) from b = 1, then the scale that makes mean(f) = 1 (skipped when f is all zero)
    -> (b (P,) fp32, f (T,) fp32)."""
    r = residual(frames, sub)
    T, P = r.shape
    b = np.ones(P, dtype=np.float32)
    f = np.zeros(T, dtype=np.float32)
    for _ in range(int(iters)):
        bd = b.astype(np.float64)
        f = step((r * bd[None, :]).sum(1), float((bd * bd).sum()))
        fd = f.astype(np.float64)
        b = step((r * fd[:, None]).sum(0), float((fd * fd).sum()))
    return rescale(b, f)


def rescale(b, f):
    """(b s, f / s) in fp32 with s = the fp32 mean of f; unchanged when f is all zero."""
    s = np.float32(f.astype(np.float64).mean())
    if not s > 0:
        return b, f
    return (b * s).astype(np.float32), (f / s).astype(np.float32)


def subtract(frames, b, f, clamp=True):
    """fp32(float64(y) - float64(b) float64(f)), max(., 0) with ``clamp``; the shape of ``frames``."""
    y = np.asarray(frames, dtype=np.float32)
    bd = np.asarray(b, dtype=np.float32).reshape(-1).astype(np.float64)
    fd = np.asarray(f, dtype=np.float32).reshape(-1).astype(np.float64)
    out = y.reshape(y.shape[0], -1).astype(np.float64) - fd[:, None] * bd[None, :]
    if clamp:
        out = np.maximum(out, 0.0)
    return out.astype(np.float32).reshape(y.shape)
