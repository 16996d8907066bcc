"""K25 on the GPU: ``ops.histogram_match`` against the float64 restatement (tests/histmatch_restatement.py) on identical seeded fp32
inputs, its refusals, and the wrappers ``Demix.Traces.histogram_match`` and ``DeformableNMF.match_traces``.

Every input row is a view into a wider buffer filled with NaN, so that a read past a row shows; ``out`` is a view into a wider
buffer too, whose margin must stay as it was.  ``info`` (na, nb, ok) must be equal.  The quantiles pick their two samples by
integer arithmetic, so they agree within one rounding of the interpolation, ``2 eps max(|x_lo|, |x_hi|)`` (a fused multiply-add is
the only freedom).  The branch of H3 shows in which coefficients are exactly 0 and must be equal; the inputs sit on no branch
boundary (asserted on the restatement: every margin is at least 1e-9).  ``beta`` and ``distance`` come from the same float64
formulas and differ by the order of the sums.

Worst relative deviation measured on these inputs on the MI355X: 3.2e-14 (beta1 of the case K = 65, Ta = 63, where the offset is
the difference of two larger numbers, bm - beta0 am; every other case stays below 2e-15: beta0 5.6e-16, beta1 1.5e-15, distance
1.0e-15).  Ten times the worst is allowed (MEASURED below), and at most 1e-9.
A distance that is itself rounding (an exact fit: two bins, or a constant row against a constant mean) has no relative deviation:
where the restatement's is at most ``16 eps S``, S the largest of max|qb|, |beta0| max|qa| and |beta1| -- each residual is a sum of
three numbers of at most that size -- the GPU's must be at most that too, and the row takes no part in the figure.
``out`` is within one fp32 ulp of the restatement's value plus that allowance carried through ``|a_t| d(beta0) + d(beta1)``.
"""
import functools

import numpy as np
import pytest
import torch

import histmatch_restatement as HR

pytestmark = pytest.mark.gpu

MEASURED = 3.2e-14      # worst relative deviation of beta and distance over CASES, as printed by the tests on the MI355X
TOL = min(10 * MEASURED, 1e-9)
EPS = np.finfo(np.float64).eps

# (K, Ta, Tb, nbins, b is one shared row).  Up to 1024 samples a row the kernel runs 256 lanes, above 1024 lanes: both sides of it.
CASES = [
    (1, 1, 1, 2, False),
    (3, 2, 5, 2, False),
    (3, 7, 7, 7, False),
    (1, 64, 64, 3, False),
    (65, 63, 65, 100, False),
    (3, 257, 1000, 100, False),
    (3, 1000, 257, 1024, False),
    (2, 1024, 1025, 64, False),
    (1, 4099, 2500, 257, False),
    (2, 16384, 16384, 100, False),
    (3, 1000, 1000, 100, True),
]


def make_rows(K, T, seed, moving):
    """Traces with transients on a baseline, of a scale and an offset per row; from K = 3 on special rows: one of mixed signs with
    both zeros, a constant one (the moving side only: a constant reference has no spread to fit), one quantised to a few levels (ties
    across the bin edges); from K = 65 on also an all-NaN row (row 60 of the moving side, row 59 of the reference), a row with one
    valid sample, a row with +-inf entries and a row at 30 % NaN."""
    rng = np.random.RandomState(seed)
    x = rng.gamma(2.0, 1.0, (K, T)) * rng.uniform(0.2, 5.0, (K, 1)) + rng.uniform(-3.0, 8.0, (K, 1)) + 0.1 * rng.randn(K, T)
    if K >= 3:
        x[0] = np.round(rng.randn(T) * 2.0) / 2.0
        x[0, ::3] = 0.0
        x[0, 1::3][::2] = -0.0
        if moving:
            x[1] = 7.1
        x[2] = 0.75 * np.round(x[2] / 0.75)
    if K >= 65:
        x[60 if moving else 59] = np.nan
        if moving:
            x[61] = np.nan
            x[61, T // 2] = 3.3
        x[62, rng.rand(T) < 0.1] = np.inf
        x[62, rng.rand(T) < 0.1] = -np.inf
        x[62, 0] = np.inf
        x[63, rng.rand(T) < 0.3] = np.nan
    x[rng.rand(K, T) < 0.01] = np.nan
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(i, nonneg):
    """The restatement on case i -> (a, b, its result, branch, margin); computed once, never changed."""
    K, Ta, Tb, nbins, shared = CASES[i]
    a = make_rows(K, Ta, 300 + i, True)
    b = make_rows(K, Tb, 400 + i, False)
    if shared:
        b = b[K - 1]
    res = HR.histogram_match(a, b, nbins, nonneg)
    return a, b, res, HR.LAST["branch"].copy(), HR.LAST["margin"].copy()


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def padded(x, extra):
    """``x`` on the GPU as a view into a buffer with ``extra`` more NaN columns -> (view, buffer)."""
    x = np.atleast_2d(x)
    buf = torch.full((x.shape[0], x.shape[1] + extra), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    return buf[:, :x.shape[1]], buf


def rel(got, want):
    """Worst relative deviation over the entries where ``want`` is a number (0 where both are equal); the NaNs must coincide."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want) & (want != got)
    return float((np.abs(got - want)[ok] / np.abs(want)[ok]).max()) if ok.any() else 0.0


def bracket(x, nbins):
    """Per row of ``x`` and per bin, max(|x_lo|, |x_hi|) of H2 (NaN for a row without a valid sample)."""
    out = np.full((x.shape[0], nbins), np.nan)
    for k, row in enumerate(x):
        xs = np.sort(HR.valid(row))
        n = len(xs)
        if n:
            lo = (np.arange(nbins, dtype=np.int64) * (n - 1)) // (nbins - 1)
            out[k] = np.maximum(np.abs(xs[lo]), np.abs(xs[np.minimum(lo + 1, n - 1)]))
    return out


@pytest.mark.parametrize("nonneg", [False, True], ids=["regular", "non-negative"])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_histogram_match_against_the_restatement(ops, i, nonneg):
    K, Ta, Tb, nbins, shared = CASES[i]
    a, b, (want, w_beta, w_dist, w_info, w_qa, w_qb), branch, margin = reference(i, nonneg)
    assert margin.min() >= 1e-9, (margin, branch)                 # the inputs sit on no branch boundary

    av, abuf = padded(a, 5)
    bv, bbuf = padded(b, 3)
    if shared:
        bv = bv[0]
    obuf = torch.full((K, Ta + 4), -7.0, dtype=torch.float32, device="cuda")
    before = abuf.clone(), bbuf.clone()
    out, beta, dist, info, qa, qb = ops.histogram_match(av, bv, nbins, nonneg=nonneg, out=obuf[:, :Ta], quantiles=True)
    again = ops.histogram_match(av, bv, nbins, nonneg=nonneg, quantiles=True)
    torch.cuda.synchronize()
    assert out.data_ptr() == obuf.data_ptr() and out.shape == (K, Ta) and out.dtype == torch.float32
    assert beta.shape == (K, 2) and dist.shape == (K,) and beta.dtype == dist.dtype == qa.dtype == torch.float64
    assert info.shape == (K, 3) and info.dtype == torch.int32 and qa.shape == qb.shape == (K, nbins)
    # the inputs are unchanged, nothing is written past a row of out, a second call returns the same bits
    assert torch.equal(abuf.view(torch.int32), before[0].view(torch.int32)) and torch.equal(bbuf.view(torch.int32), before[1].view(torch.int32))
    assert bool((obuf[:, Ta:] == -7.0).all())
    assert torch.equal(out.view(torch.int32), again[0].view(torch.int32)) and torch.equal(info, again[3])
    for u, v in ((beta, again[1]), (dist, again[2]), (qa, again[4]), (qb, again[5])):
        assert torch.equal(u.view(torch.int64), v.view(torch.int64))

    got = out.cpu().numpy().astype(np.float64)
    beta, dist, info, qa, qb = (t.cpu().numpy() for t in (beta, dist, info, qa, qb))
    # equal: the counts and flags, the NaN sets, the branch
    np.testing.assert_array_equal(info, w_info)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.isnan(beta), np.isnan(w_beta))
    np.testing.assert_array_equal(beta == 0, w_beta == 0)
    # the quantiles: one rounding of the interpolation
    for name, g, w, x in (("qa", qa, w_qa, a), ("qb", qb, w_qb, np.atleast_2d(b))):
        w = np.broadcast_to(w, g.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), name
        ok = ~np.isnan(w)
        allow = 2 * EPS * np.broadcast_to(bracket(x, nbins), g.shape)
        print(f"case {i} {name}: {int((g[ok] != w[ok]).sum())} of {int(ok.sum())} quantiles differ from the restatement's")
        assert (np.abs(g - w)[ok] <= allow[ok]).all(), (name, float(np.abs(g - w)[ok].max()))
    # beta and the distance
    valid = w_info[:, 2] == 1
    S = np.maximum(np.nanmax(np.abs(np.broadcast_to(w_qb, qb.shape)), axis=1, initial=0.0),
                   np.maximum(np.abs(w_beta[:, 0]) * np.nanmax(np.abs(w_qa), axis=1, initial=0.0), np.abs(w_beta[:, 1])))
    noise = valid & (w_dist <= 16 * EPS * S)                      # an exact fit: the distance is rounding
    assert (dist[noise] <= 16 * EPS * S[noise]).all(), (dist[noise], S[noise])
    devs = dict(beta0=rel(beta[:, 0], w_beta[:, 0]), beta1=rel(beta[:, 1], w_beta[:, 1]), distance=rel(dist[~noise], w_dist[~noise]))
    print(f"case {i} K={K} Ta={Ta} Tb={Tb} nbins={nbins} nonneg={nonneg}: relative deviation "
          + ", ".join(f"{k} {v:.2e}" for k, v in devs.items()) + f"; branches {np.bincount(branch, minlength=5).tolist()}, "
          f"smallest margin {margin.min():.1e}, {int(noise.sum())} exact fits")
    assert max(devs.values()) <= TOL, devs
    # the traces: one fp32 ulp of the restatement's value plus the allowance carried through the map
    with np.errstate(all="ignore"):
        allow = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + \
            TOL * (np.abs(a.astype(np.float64)) * np.abs(w_beta[:, :1]) + np.abs(w_beta[:, 1:]))
    ok = ~np.isnan(want)
    worst = float((np.abs(got - want)[ok] / allow[ok]).max()) if ok.any() else 0.0
    print(f"case {i}: traces at most {worst:.3f} of the allowance, {int(ok.sum())} of {K * Ta} entries valid")
    assert worst <= 1.0


def test_the_special_rows_are_what_they_are_meant_to_be():
    """On the restatement (no GPU needed for the statement, but the cases are this file's)."""
    i = [c[:4] for c in CASES].index((65, 63, 65, 100))
    a, b, (want, beta, dist, info, qa, qb), branch, _ = reference(i, False)
    assert branch[1] == 2 and beta[1, 0] == 0.0                                       # constant
    assert len(np.unique(a[2][np.isfinite(a[2])])) < 40 and (np.diff(qa[2]) == 0).sum() > 50   # ties across the bin edges
    assert (a[0] == 0).sum() > 10 and np.signbit(a[0][a[0] == 0]).any() and not np.signbit(a[0][a[0] == 0]).all()
    assert (a[0] < 0).any() and (a[0] > 0).any()
    assert info[60].tolist() == [0, int(np.isfinite(b[60]).sum()), 0] and np.isnan(want[60]).all()      # all-NaN moving row
    assert info[59, 1] == 0 and info[59, 2] == 0 and np.isnan(want[59]).all() and np.isnan(beta[59]).all()   # all-NaN reference
    assert info[61, 0] == 1 and branch[61] == 2 and np.isfinite(want[61]).sum() == 1   # one valid sample
    assert np.isinf(a[62]).sum() >= 3 and info[62, 2] == 1 and np.isfinite(beta[62]).all()
    assert np.array_equal(np.isnan(want[62]), ~np.isfinite(a[62]))
    assert 0.15 * 63 < np.isnan(a[63]).sum() < 0.5 * 63 and info[63, 2] == 1
    nn = reference(i, True)[3]
    assert (nn[info[:, 2] == 1] >= 1).all() and (nn >= 3).any()                       # the constraint binds somewhere


def test_refusals_are_raised_from_the_error_code_with_nothing_written(ops):
    from dnmf_amd._lib import DnmfHipError
    b = torch.zeros((2, 50), dtype=torch.float32, device="cuda")

    def refused(a, b, nbins, code, **kw):
        out = torch.full(tuple(a.shape), -7.0, dtype=torch.float32, device="cuda")
        with pytest.raises(DnmfHipError, match=rf"argument error {code}\)"):
            ops.histogram_match(a, b, nbins, out=out, **kw)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())

    a = torch.ones((2, 40), dtype=torch.float32, device="cuda")
    refused(torch.ones((2, 16385), dtype=torch.float32, device="cuda"), b, 10, -3)
    refused(a, torch.ones((16385,), dtype=torch.float32, device="cuda"), 10, -3)
    refused(a, b, 1, -2)
    refused(a, b, 1025, -3)
    wide = torch.ones((100,), dtype=torch.float32, device="cuda")
    refused(torch.as_strided(wide, (2, 40), (39, 1)), b, 10, -2)                      # rows that overlap: lda < Ta
    refused(a, torch.as_strided(wide, (2, 50), (49, 1)), 10, -2)
    from Demix.Traces import histogram_match
    with pytest.raises(ValueError, match="type"):
        histogram_match(a, b, 10, "nonneg")
    ops.histogram_match(torch.ones((1, 16384), dtype=torch.float32, device="cuda"), b[0], 1024)      # the limits themselves pass
    torch.cuda.synchronize()


def test_the_reference_entry_point(ops):
    """``from Demix.Traces import histogram_match``: numpy 1-D in, numpy out and a scalar distance; CUDA in, CUDA out; rows."""
    from Demix.Traces import histogram_match
    i = [c[:4] for c in CASES].index((3, 257, 1000, 100))
    a, b, (want, w_beta, w_dist, w_info, _, _), _, _ = reference(i, False)
    a0 = a[0].copy()
    tr, d = histogram_match(a[0], b[0], 100, "regular")
    assert isinstance(tr, np.ndarray) and tr.dtype == np.float32 and tr.shape == (257,) and isinstance(d, float)
    assert np.array_equal(a[0].view(np.int32), a0.view(np.int32))                     # the input is not modified
    full = ops.histogram_match(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), 100)
    assert np.array_equal(tr.view(np.int32), full[0][0].cpu().numpy().view(np.int32)) and d == float(full[2][0])
    assert abs(d - w_dist[0]) <= TOL * w_dist[0]
    tr, d = histogram_match(a, b, 100, "non-negative")
    assert tr.shape == (3, 257) and tr.dtype == np.float32 and d.shape == (3,) and d.dtype == np.float64
    tr1, d1 = histogram_match(a, b[2], 100, "regular")                                # one reference for all
    assert np.array_equal(tr1[2].view(np.int32), full[0][2].cpu().numpy().view(np.int32)) and d1[2] == float(full[2][2])
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    tr2, d2 = histogram_match(ta, tb, 100, "regular")
    assert tr2.is_cuda and d2.is_cuda and torch.equal(tr2.view(torch.int32), full[0].view(torch.int32)) and torch.equal(d2, full[2])
    tr3, d3 = histogram_match(ta[1], tb[1], 100, "regular")
    assert tr3.shape == (257,) and d3.dim() == 0 and torch.equal(tr3.view(torch.int32), full[0][1].view(torch.int32))


def test_model_match_traces(ops):
    """``DeformableNMF.match_traces`` on a small fitted model returns what ``ops.histogram_match(model.C, reference)`` returns,
    fills ``last_match`` and leaves ``model.C`` bit-identical; the matched traces are closer to the truth than ``C``."""
    from dnmf_amd.Demix import dNMF as M
    sz, K, T = (24, 20, 2), 6, 40
    pos = torch.tensor([[5.0, 5.0, 0.0], [12.0, 6.0, 1.0], [19.0, 5.0, 0.0], [6.0, 14.0, 1.0], [12.0, 14.0, 0.0], [18.0, 15.0, 1.0]])
    rng = np.random.RandomState(7)
    truth = M.DeformableNMF(torch.tensor(sz), K, T, positions=pos)
    truth.C = torch.from_numpy((0.6 + 0.3 * rng.rand(K, T)) * np.exp(-np.arange(T) / 60.0)[None, :]).to("cuda", torch.float32)
    with torch.no_grad():
        video = truth.fp.forward(range(T), truth.C)[0].reshape(T, -1).clone()
    model = M.DeformableNMF(torch.tensor(sz), K, T, positions=pos)
    model.verbose = False
    model.update_footprints(M.ResidentLoader(video, sz, 8), 8, torch.tensor(sz), iter_c=20)
    C = model.C.clone()
    assert model.last_match is None
    ref = 3.0 * truth.C + 2.0                                                          # the truth in other units
    out = model.match_traces(ref, nbins=20)
    assert torch.equal(model.C.view(torch.int32), C.view(torch.int32))
    want = ops.histogram_match(C, ref, 20)
    assert torch.equal(out.view(torch.int32), want[0].view(torch.int32))
    assert sorted(model.last_match) == ["beta", "distance", "ok"]
    assert torch.equal(model.last_match["beta"].view(torch.int64), want[1].view(torch.int64))
    assert torch.equal(model.last_match["distance"].view(torch.int64), want[2].view(torch.int64))
    assert model.last_match["ok"].dtype == torch.bool and bool(model.last_match["ok"].all())
    rms = lambda X: float(((X - ref) ** 2).mean(dim=1).sqrt().median())                # noqa: E731
    assert rms(out) < 0.25 * rms(C)
    # given traces, one reference for all, the other type; numpy in
    out2 = model.match_traces(ref[0].cpu().numpy(), nbins=20, type="non-negative", traces=C.cpu().numpy())
    want2 = ops.histogram_match(C, ref[0], 20, nonneg=True)
    assert torch.equal(out2.view(torch.int32), want2[0].view(torch.int32))
    with pytest.raises(ValueError, match="type"):
        model.match_traces(ref, type="positive")
