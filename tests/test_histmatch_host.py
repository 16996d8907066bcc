"""The definition of histogram_match (K25, tests/histmatch_restatement.py) against numpy and scipy, its edge cases, and the ABI of
the entry on the library as built.  No GPU.

H2 against ``np.quantile``: numpy forms the virtual index ``q (n - 1)`` from the rounded ``q = linspace(0, 1, nbins)[j]``; it
carries a relative error of eps, so the fraction numpy interpolates with is off by up to about ``n eps`` and the quantile by that
times a gap ``|x_hi - x_lo| <= 2 max|x|``: within ``4 n eps max|x|`` (measured on these cases: the first test prints it).  Where
``nbins - 1`` divides ``n - 1`` the index is a whole number and the quantile is a sample, bit for bit.

H3 on sorted quantiles never clips the slope: qa and qb both ascend, so Sab >= 0 (Chebyshev's sum inequality) and the free
beta0 is never negative; through H2, 'non-negative' can only bind on the offset (or take (0, 0)).  H3 is stated for any design,
though, and is held to ``nnls`` on any: the rows that make beta0 clip negate the quantiles of b, not b.
"""
import ctypes
import inspect

import numpy as np
import pytest
from scipy.optimize import nnls

import histmatch_restatement as HR

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


def design(qa):
    return np.stack([qa, np.ones_like(qa)], axis=1)


# ---- H2 ------------------------------------------------------------------------------------------------------------------------
def test_quantiles_against_numpy():
    rng = np.random.RandomState(0)
    worst = 0.0
    for case in range(400):
        n, nbins = rng.randint(1, 300), rng.randint(2, 400)
        x = rng.randn(n) * 10.0 ** rng.randint(-3, 4) + rng.randn() * 5.0
        if case % 7 == 0:
            x = np.round(x)                                      # ties
        got = HR.quantiles(x, nbins)
        want = np.quantile(x, np.linspace(0, 1, nbins))
        diff, unit = np.abs(got - want).max(), EPS * np.abs(x).max()      # a rounded row may be all zeros
        assert diff <= 4 * n * unit, (n, nbins, diff, unit)
        worst = max(worst, diff / unit if unit > 0 else 0.0)
        assert got[0] == x.min() and got[-1] == x.max()
        assert (np.diff(got) >= 0).all()
    print(f"largest difference from np.quantile: {worst:.1f} eps max|x|")


def test_quantiles_are_samples_where_the_index_is_whole():
    """Equal to the samples at stride (n - 1) / (nbins - 1), bit for bit.  ``np.quantile`` is not held to that: its index
    ``linspace(0, 1, nbins)[j] (n - 1)`` can miss the whole number by a rounding, and it then interpolates one ulp away."""
    rng = np.random.RandomState(1)
    exact = total = 0
    for n, nbins in ((1, 2), (1, 9), (2, 2), (7, 7), (7, 4), (13, 5), (101, 101), (101, 51), (257, 17), (299, 150)):
        assert (n - 1) % (nbins - 1) == 0
        x = rng.randn(n)
        got = HR.quantiles(x, nbins)
        np.testing.assert_array_equal(got, np.sort(x)[:: (n - 1) // (nbins - 1)] if n > 1 else np.full(nbins, x[0]))
        want = np.quantile(x, np.linspace(0, 1, nbins))
        exact += int((got == want).sum())
        total += nbins
        assert np.abs(got - want).max() <= 4 * n * EPS * np.abs(x).max()
    print(f"np.quantile returns the sample itself in {exact} of {total} of these quantiles")


def test_two_bins_are_min_and_max():
    rng = np.random.RandomState(2)
    a, b = rng.randn(50).astype(np.float32), (3.0 + rng.rand(31)).astype(np.float32)
    r = HR.match_row(a, b, 2)
    np.testing.assert_array_equal(r["qa"], [a.min(), a.max()])
    np.testing.assert_array_equal(r["qb"], [b.min(), b.max()])
    # two points: the line through them
    scale = (float(b.max()) - float(b.min())) / (float(a.max()) - float(a.min()))
    assert abs(r["beta"][0] - scale) <= 4 * EPS * scale and r["distance"] <= 1e-14


def test_more_bins_than_samples():
    a, b = np.array([3.0, 1.0, 2.0], np.float32), np.array([10.0, 30.0], np.float32)
    r = HR.match_row(a, b, 9)
    np.testing.assert_allclose(r["qa"], np.linspace(1.0, 3.0, 9), rtol=0, atol=4 * EPS)
    np.testing.assert_allclose(r["qb"], np.linspace(10.0, 30.0, 9), rtol=0, atol=40 * EPS)
    np.testing.assert_allclose(r["beta"], [10.0, 0.0], rtol=0, atol=1e-13)
    np.testing.assert_allclose(r["out"], [30.0, 10.0, 20.0], rtol=1e-6)
    r = HR.match_row(a[:1], b, 5)                                # a single sample: a constant moving trace
    assert r["branch"] == 2 and r["beta"][0] == 0.0 and r["beta"][1] == 20.0 and r["out"][0] == 20.0


def test_both_zeros_are_one_value():
    a = np.array([-0.0, 0.0, -0.0, 0.0, 1.0], np.float32)
    q = HR.quantiles(HR.valid(a), 9)
    np.testing.assert_array_equal(q[:6], 0.0)                     # whichever zero the sort puts first
    assert HR.match_row(np.array([-0.0, 0.0], np.float32), a, 4)["branch"] == 2     # -0 == +0: constant


# ---- H3 ------------------------------------------------------------------------------------------------------------------------
def spread_rows(seed, count):
    rng = np.random.RandomState(seed)
    for i in range(count):
        na, nb, nbins = rng.randint(5, 300), rng.randint(5, 300), rng.randint(2, 120)
        a = (rng.randn(na) * rng.uniform(0.1, 10.0) + rng.uniform(-20.0, 20.0)).astype(np.float32)
        b = (rng.gamma(2.0, 1.0, nb) * rng.uniform(0.1, 10.0) + rng.uniform(-20.0, 20.0)).astype(np.float32)
        if i % 4 == 2:
            b = b - b.mean() + 0.01                              # offsets of both signs
        if i % 4 == 3:
            a, b = np.abs(a) + 1.0, -np.abs(b) - 1.0             # everything wants to be negative: both clipped
        yield a, b, nbins


def test_regular_against_lstsq():
    for a, b, nbins in spread_rows(3, 200):
        r = HR.match_row(a, b, nbins)
        want = np.linalg.lstsq(design(r["qa"]), r["qb"], rcond=None)[0]
        assert r["branch"] == 1
        np.testing.assert_allclose(r["beta"], want, rtol=1e-9, atol=1e-9 * np.abs(want).max())


def test_non_negative_against_nnls_in_every_outcome():
    seen = set()
    worst = 0.0
    for i, (a, b, nbins) in enumerate(spread_rows(4, 400)):
        r = HR.match_row(a, b, nbins, nonneg=True)
        qa, qb, beta = r["qa"], r["qb"], r["beta"]
        if i % 4 == 1:                                           # b negated at the level of H3: a decreasing map, beta0 clipped
            qb = -qb
            beta = np.array(HR.regress(qa, qb, True)[0])
        want = nnls(design(qa), qb)[0]
        assert (beta >= 0).all()
        err = np.abs(beta - want).max() / max(np.abs(want).max(), 1e-300)
        worst = max(worst, err)
        assert err <= 1e-9, (beta, want)
        seen.add((bool(beta[0] == 0), bool(beta[1] == 0)))
    print(f"largest relative difference from scipy's nnls: {worst:.1e}; outcomes {sorted(seen)}")
    assert seen == {(False, False), (True, False), (False, True), (True, True)}


def test_a_constant_moving_trace():
    rng = np.random.RandomState(5)
    b = rng.randn(40).astype(np.float32) + 2.0
    for value in (0.1, -3.7, 0.0, 1e-30):                        # 0.1: the mean of equal values is not that value in float64
        a = np.full(17, value, np.float32)
        for nbins in (2, 3, 10, 100):
            r = HR.match_row(a, b, nbins)
            bm = np.sum(HR.quantiles(HR.valid(b), nbins)) / nbins
            assert r["branch"] == 2 and r["beta"][0] == 0.0 and r["beta"][1] == bm
            np.testing.assert_array_equal(r["out"], np.float32(bm))
            n = HR.match_row(a, -b, nbins, nonneg=True)
            assert n["branch"] == 2 and n["beta"].tolist() == [0.0, 0.0] and (n["out"] == 0).all()


def test_an_affine_copy_comes_back():
    rng = np.random.RandomState(6)
    for s, o in ((2.5, -3.0), (0.01, 40.0), (7.0, 0.0)):
        b = rng.gamma(2.0, 3.0, 500)
        a = s * b + o
        for nbins in (2, 10, 100, 1000):
            for nonneg in (False, True):
                # the inverse map has a non-negative offset only for o <= 0
                if nonneg and o > 0:
                    continue
                r = HR.match_row(a, b, nbins, nonneg)
                assert r["distance"] <= 1e-12 * np.abs(b).max(), (s, o, nbins, r["distance"])
                back = a * r["beta"][0] + r["beta"][1]
                assert np.abs(back - b).max() <= 1e-9 * np.abs(b).max()


# ---- H1, H4 --------------------------------------------------------------------------------------------------------------------
def test_samples_that_are_not_finite():
    rng = np.random.RandomState(7)
    a, b = rng.randn(60).astype(np.float32), rng.randn(45).astype(np.float32) * 2 + 1
    clean = HR.match_row(a, b, 20)
    a2, b2 = np.concatenate([a, [np.nan, np.inf, -np.inf]]).astype(np.float32), np.concatenate([[np.inf, np.nan], b, [-np.inf]]).astype(np.float32)
    order = rng.permutation(len(a2))
    r = HR.match_row(a2[order], b2, 20)
    assert (r["na"], r["nb"], r["ok"]) == (60, 45, 1)
    np.testing.assert_array_equal(r["beta"], clean["beta"])       # what is not finite counts for nothing, wherever it sits
    assert r["distance"] == clean["distance"]
    np.testing.assert_array_equal(np.isnan(r["out"]), ~np.isfinite(a2[order]))
    kept = order < 60                                             # entry i of the shuffled row is sample order[i] of a
    np.testing.assert_array_equal(r["out"][kept], clean["out"][order[kept]])
    assert r["out"].dtype == np.float32


def test_a_row_without_a_valid_sample_is_refused_not_raised():
    a, b = np.array([1.0, 2.0, np.nan], np.float32), np.array([np.nan, np.inf], np.float32)
    for x, y, na, nb in ((a, b, 2, 0), (b, a, 0, 2), (b, b, 0, 0)):
        r = HR.match_row(x, y, 5)
        assert (r["na"], r["nb"], r["ok"], r["branch"]) == (na, nb, 0, 0)
        assert np.isnan(r["out"]).all() and len(r["out"]) == len(x) and np.isnan(r["beta"]).all() and np.isnan(r["distance"])
    # it does not disturb its neighbours; b may be one row for all
    A = np.stack([a, np.full(3, np.nan, np.float32), a])
    out, beta, distance, info, qa, qb = HR.histogram_match(A, np.array([5.0, 7.0], np.float32), 3)
    assert info.tolist() == [[2, 2, 1], [0, 2, 0], [2, 2, 1]] and info.dtype == np.int32
    np.testing.assert_array_equal(out[0], out[2])
    assert np.isnan(out[1]).all() and np.isnan(qa[1]).all() and not np.isnan(qb[1]).any()
    np.testing.assert_allclose(out[0][:2], [5.0, 7.0], rtol=1e-6)
    with pytest.raises(ValueError):
        HR.match_row(a, a, 1)


# ---- the ABI on the library as built ---------------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_entry(lib):
    from dnmf_amd import _lib, build
    res, args = _lib.SIGNATURES["dnmf_histogram_match"]
    assert res is ctypes.c_int and args[1] is args[4] is args[10] is ctypes.c_long
    assert lib.dnmf_histogram_match
    assert "histogram_match.hip" in build.SOURCES


def test_argument_errors_are_reported_without_a_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def call(a=p, lda=8, Ta=8, b=p, ldb=8, Tb=8, K=1, nbins=4, nonneg=0, out=p, ldo=8, beta=p, distance=p, info=p, qa=None, qb=None):
        return lib.dnmf_histogram_match(a, lda, Ta, b, ldb, Tb, K, nbins, nonneg, out, ldo, beta, distance, info, qa, qb, None)

    for name in ("a", "b", "out", "beta", "distance", "info"):
        assert call(**{name: None}) == -1 and b"NULL" in lib.dnmf_last_error()
    for bad in (dict(K=0), dict(Ta=0), dict(Tb=0), dict(nbins=1), dict(nbins=0), dict(nonneg=2), dict(lda=7), dict(ldo=7), dict(ldb=7),
                dict(ldb=-1)):
        assert call(**bad) == -2, bad
    assert b"nbins" in (call(nbins=1), lib.dnmf_last_error())[1]
    for bad in (dict(Ta=16385, lda=16385, ldo=16385), dict(Tb=16385, ldb=16385), dict(Tb=16385, ldb=0), dict(nbins=1025), dict(K=18433)):
        assert call(**bad) == -3, bad
    assert b"16384" in lib.dnmf_last_error() or b"18432" in lib.dnmf_last_error()


def test_public_signatures():
    from dnmf_amd import ops
    from dnmf_amd.Demix.dNMF import DeformableNMF
    from dnmf_amd.Demix.Traces import histogram_match
    import Demix.Traces as shim

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(ops.histogram_match) == [("a", E), ("b", E), ("nbins", E), ("nonneg", False), ("out", None), ("quantiles", False)]
    assert params(histogram_match) == [("a", E), ("b", E), ("nbins", E), ("type", E)]
    assert params(HR.histogram_match) == [("a", E), ("b", E), ("nbins", E), ("nonneg", False)]
    assert shim.histogram_match is histogram_match
    assert params(DeformableNMF.match_traces) == [("self", E), ("reference", E), ("nbins", 100), ("type", "regular"), ("traces", None)]
    assert "self.last_match = None" in inspect.getsource(DeformableNMF.__init__)
    y = np.ones(8, np.float32)
    for bad in ("nonnegative", "Regular", None):
        with pytest.raises(ValueError, match="type"):
            histogram_match(y, y, 10, bad)
