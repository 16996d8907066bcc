"""The definition of the quantile-matched rescaling of a trace (K25, ``histogram_match``) in float64, numpy only.  The kernel
(dnmf_amd/csrc/histogram_match.hip), the documents and the tests refer to this file.

Per row: a moving trace ``a`` of Ta samples, a reference trace ``b`` of Tb samples, ``nbins`` >= 2 and ``nonneg``.

H1  Valid samples: those of ``a``, and separately of ``b``, that are finite; their counts are na and nb.  (The reference's
    ``Demix/Traces.py::histogram_match`` drops NaN only; one infinite sample would make every fit NaN.)  With na = 0 or nb = 0 the
    row is refused: ok = 0, beta, the distance and the whole output row are NaN, nothing is raised.
H2  Quantiles: with the n valid samples sorted ascending, x_0 <= .. <= x_{n-1}, the j-th of the nbins quantiles sits at the exact
    rational index j (n - 1) / (nbins - 1):
        lo = (j (n - 1)) // (nbins - 1),  frac = ((j (n - 1)) % (nbins - 1)) / (nbins - 1),  hi = min(lo + 1, n - 1),
        q_j = x_lo + (x_hi - x_lo) frac.
    The two samples are picked by integers; only ``frac`` and the interpolation are rounded.  This is
    ``np.quantile(x, np.linspace(0, 1, nbins))`` up to the rounding of numpy's own index.
H3  The regression of qb on [qa, 1], centred: am and bm are the means over the bins, Saa = sum (qa - am)^2 and
    Sab = sum (qa - am)(qb - bm).  A moving trace whose quantiles are all one value (qa_0 == qa_{nbins-1}; they are sorted) is
    constant: Saa and Sab are then 0 by definition, whatever the rounding of am leaves.
      regular        beta0 = Sab / Saa, beta1 = bm - beta0 am;  with Saa == 0: beta0 = 0, beta1 = bm.
      non-negative   the exact minimiser of |[qa, 1] beta - qb|^2 over beta0 >= 0, beta1 >= 0: the regular solution where it is
                     feasible (with Saa == 0: beta0 = 0, beta1 = max(bm, 0)); else the better of the two boundary solutions
                     (0, max(bm, 0)) and (max(sum qa qb / sum qa^2, 0), 0) -- (0, 0) when sum qa^2 == 0 -- by the residual sum of
                     squares sum (beta0 qa + beta1 - qb)^2, the first on a tie.  (qa and qb both ascend, so Sab >= 0 and the regular
                     beta0 is never negative: on quantiles the constraint can only bind through the offset.  ``regress`` is
                     nevertheless exact for any design.)
H4  out_t = a_t beta0 + beta1 in float64, rounded once to fp32; NaN wherever a_t is not finite.
H5  distance = sqrt(mean_j (beta0 qa_j + beta1 - qb_j)^2), the RMS mismatch of the matched quantiles.  (The reference declares a
    "histogram distance between atransform and b" and returns NaN.)

``LAST`` keeps, for the tests, what the last ``histogram_match`` call decided per row: ``branch`` (0 refused, 1 the regular
solution, 2 a constant moving trace, 3 the boundary beta0 = 0, 4 the boundary beta1 = 0) and ``margin``, the smallest relative
distance of a quantity that a decision rests on from the value at which the decision would change (inf where none was made).
"""
import numpy as np

LAST = {}


def valid(x):
    """H1: the finite samples of ``x`` as float64, in their order."""
    x = np.asarray(x, np.float64)
    return x[np.isfinite(x)]


def quantiles(x, nbins):
    """H2 on the valid samples ``x`` (n >= 1) -> (nbins,) float64."""
    xs = np.sort(np.asarray(x, np.float64))
    n = len(xs)
    j = np.arange(nbins, dtype=np.int64)
    num = j * (n - 1)
    lo = num // (nbins - 1)
    frac = (num % (nbins - 1)).astype(np.float64) / float(nbins - 1)
    hi = np.minimum(lo + 1, n - 1)
    return xs[lo] + (xs[hi] - xs[lo]) * frac


def _rss(beta, qa, qb):
    r = beta[0] * qa + beta[1] - qb
    return float(np.sum(r * r))


def _rel(x, scale):
    return abs(x) / scale if scale > 0 else np.inf


def regress(qa, qb, nonneg):
    """H3 -> ((beta0, beta1), branch, margin)."""
    nbins = len(qa)
    am, bm = float(np.sum(qa)) / nbins, float(np.sum(qb)) / nbins
    if qa[0] == qa[-1]:
        Saa = Sab = 0.0
    else:
        Saa = float(np.sum((qa - am) * (qa - am)))
        Sab = float(np.sum((qa - am) * (qb - bm)))
    sb = float(np.abs(qb).max())
    if Saa == 0.0:
        if nonneg:
            return (0.0, max(bm, 0.0)), 2, _rel(bm, sb)
        return (0.0, bm), 2, np.inf
    b0 = Sab / Saa
    b1 = bm - b0 * am
    if not nonneg:
        return (b0, b1), 1, np.inf
    # how far the regular solution is from the edge of the feasible set, in units of what its terms are made of
    s0 = np.sqrt(float(np.sum((qb - bm) * (qb - bm))) / Saa)
    s1 = max(abs(bm), abs(b0 * am))
    margin = min(_rel(b0, s0), _rel(b1, s1))
    if b0 >= 0.0 and b1 >= 0.0:
        return (b0, b1), 1, margin
    Paa, Pab = float(np.sum(qa * qa)), float(np.sum(qa * qb))
    first = (0.0, max(bm, 0.0))
    second = (max(Pab / Paa, 0.0), 0.0) if Paa != 0.0 else (0.0, 0.0)
    r1, r2 = _rss(first, qa, qb), _rss(second, qa, qb)
    margin = min(margin, _rel(bm, sb))
    if Paa != 0.0:
        margin = min(margin, _rel(Pab, np.sqrt(Paa * float(np.sum(qb * qb)))))
    if first != second:
        margin = min(margin, _rel(r1 - r2, max(r1, r2)))
    return (second, 4, margin) if r2 < r1 else (first, 3, margin)


def match_row(a, b, nbins, nonneg=False):
    """One row -> dict(out (Ta,) float32, beta (2,), distance, na, nb, ok, qa, qb (nbins,), branch, margin)."""
    nbins = int(nbins)
    if nbins < 2:
        raise ValueError(f"nbins={nbins}: at least 2")
    a = np.asarray(a, np.float64)
    xa, xb = valid(a), valid(b)
    na, nb = len(xa), len(xb)
    nan = np.full(nbins, np.nan)
    qa = quantiles(xa, nbins) if na else nan
    qb = quantiles(xb, nbins) if nb else nan
    if na == 0 or nb == 0:
        return dict(out=np.full(len(a), np.nan, np.float32), beta=np.array([np.nan, np.nan]), distance=np.nan, na=na, nb=nb, ok=0,
                    qa=qa, qb=qb, branch=0, margin=np.inf)
    beta, branch, margin = regress(qa, qb, nonneg)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.where(np.isfinite(a), a * beta[0] + beta[1], np.nan).astype(np.float32)
    distance = float(np.sqrt(_rss(beta, qa, qb) / nbins))
    return dict(out=out, beta=np.array(beta), distance=distance, na=na, nb=nb, ok=1, qa=qa, qb=qb, branch=branch, margin=margin)


def histogram_match(a, b, nbins, nonneg=False):
    """``a`` (K, Ta) and ``b`` (K, Tb) or (Tb,), one row shared by all -> ``(out (K, Ta) float32, beta (K, 2), distance (K,),
    info (K, 3) int32: na, nb, ok, qa (K, nbins), qb (K, nbins))``."""
    a = np.atleast_2d(np.asarray(a))
    b = np.asarray(b)
    K = a.shape[0]
    rows = [match_row(a[k], b if b.ndim == 1 else b[k], nbins, nonneg) for k in range(K)]
    LAST["branch"] = np.array([r["branch"] for r in rows])
    LAST["margin"] = np.array([r["margin"] for r in rows])
    return (np.stack([r["out"] for r in rows]), np.stack([r["beta"] for r in rows]), np.array([r["distance"] for r in rows]),
            np.array([[r["na"], r["nb"], r["ok"]] for r in rows], np.int32), np.stack([r["qa"] for r in rows]),
            np.stack([r["qb"] for r in rows]))
