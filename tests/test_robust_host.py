"""The restatement of K30 and of ``robust_images`` (tests/robust_restatement.py) pinned against numpy, scipy and K21's noise
estimate, and the conditions of the planted detection case on the float64 definition alone.  No GPU."""
import functools

import numpy as np
import pytest
import scipy.stats

import deconv_restatement as DCR
import detect_restatement as DR
import robust_restatement as RR
import summary_restatement as SR

F32_HALF_ULP = 2.0 ** -24       # the relative error of one fp32 rounding


def mixed_rows(T=41, P=23, seed=0):
    """(T, P) fp32: negative, zero and positive values with both signs of zero, denormals, ties, +-inf and NaN in some frames of
    some voxels, one voxel without a finite sample, one constant."""
    rng = np.random.RandomState(seed)
    x = (rng.randn(T, P) * 10.0 ** rng.randint(-3, 4, (1, P))).astype(np.float32)
    x[rng.rand(T, P) < 0.1] = 0.0
    x[rng.rand(T, P) < 0.05] = -0.0
    x[:, 1] = rng.randint(0, 2, T)                        # two values only
    x[:, 2] = (rng.randint(-3, 4, T) * 1e-42).astype(np.float32)      # denormals
    x[:, 3] = 2.5                                         # constant
    x[rng.rand(T, P) < 0.08] = np.nan
    x[rng.rand(T, P) < 0.03] = np.inf
    x[rng.rand(T, P) < 0.03] = -np.inf
    x[:, 4] = np.nan
    x[1:, 5] = np.nan                                     # one sample
    x.setflags(write=False)
    return x


def test_key_order():
    rng = np.random.RandomState(1)
    x = np.concatenate([rng.randn(500).astype(np.float32), (rng.randn(200) * 1e-41).astype(np.float32),
                        np.array([0.0, -0.0, np.finfo(np.float32).max, -np.finfo(np.float32).max, np.finfo(np.float32).tiny,
                                  1e-45, -1e-45, 1.0, np.nextafter(np.float32(1), np.float32(2))], dtype=np.float32)])
    k = RR.key32(x)
    assert k.dtype == np.uint32
    i, j = np.meshgrid(np.arange(len(x)), np.arange(len(x)), indexing="ij")
    np.testing.assert_array_equal(k[i] < k[j], x[i] < x[j])
    np.testing.assert_array_equal(k[i] == k[j], x[i] == x[j])          # -0 and +0 are one value
    back = RR.from_key32(k)
    np.testing.assert_array_equal(back, x)
    assert not np.signbit(back[x == 0]).any()


def test_sources_are_fp32_arithmetic():
    rng = np.random.RandomState(2)
    y = (rng.randn(9, 6) * 100).astype(np.float32)
    c = (rng.randn(6) * 100).astype(np.float32)
    dev = RR.samples(y, "absdev", c)
    assert dev.dtype == np.float32 and dev.shape == (9, 6)
    for t in range(9):
        for v in range(6):
            assert dev[t, v] == abs(np.float32(y[t, v] - c[v]))
    # not the float64 difference rounded twice: the fp32 difference is the exact one rounded once
    np.testing.assert_array_equal(dev, np.abs(y.astype(np.float64) - c.astype(np.float64)[None]).astype(np.float32))
    ids = rng.permutation(9)
    dif = RR.samples(y, "absdiff", frame_ids=ids)
    assert dif.dtype == np.float32 and dif.shape == (8, 6)
    for t in range(8):
        np.testing.assert_array_equal(dif[t], np.abs(y[ids[t + 1]] - y[ids[t]]))
    np.testing.assert_array_equal(RR.samples(y, "value", frame_ids=ids), y[ids])
    with pytest.raises(ValueError, match="source"):
        RR.samples(y, "square")


@pytest.mark.parametrize("source", ["value", "absdev", "absdiff"])
def test_ranks_equal_sorted_samples_and_value_equals_nanquantile(source):
    """lo, hi and n for equality against np.sort of the finite samples; ``value`` EQUAL (not within an ulp) to
    np.nanquantile(method='linear') in float64 -- R5 evaluates the line as numpy does."""
    y = mixed_rows()
    c = np.nan_to_num(np.nanmedian(np.where(np.isfinite(y), y, np.nan), 0), nan=0.0).astype(np.float32) if source == "absdev" else None
    qs = [0.0, 0.08, 0.5, 1.0]
    got = RR.temporal_quantiles(y, qs, source, c)
    x = RR.samples(y, source, c)
    for v in range(y.shape[1]):
        kept = np.sort(x[np.isfinite(x[:, v]), v])
        assert got["n"][v] == len(kept)
        for i, q in enumerate(qs):
            if len(kept) == 0:
                assert np.isnan(got["lo"][i, v]) and np.isnan(got["hi"][i, v]) and np.isnan(got["value"][i, v])
                continue
            h = q * (len(kept) - 1)
            lo = int(np.floor(h))
            hi = min(lo + 1, len(kept) - 1)
            assert got["lo"][i, v] == kept[lo] and got["hi"][i, v] == kept[hi], (source, v, q)
            assert got["lo"][i, v] == np.partition(kept, lo)[lo]
            assert not np.signbit(got["lo"][i, v]) or got["lo"][i, v] != 0
            want = np.nanquantile(kept.astype(np.float64), q, method="linear")
            assert got["value"][i, v] == want, (source, v, q, got["value"][i, v], want)
    assert got["n"][4] == 0 and (got["n"][5] == (1 if source != "absdiff" else 0))


def test_rank_arithmetic():
    for n in (1, 2, 3, 4, 47, 48, 255, 256, 257, 70000):
        for q in (0.0, 0.08, 0.5, 1.0):
            h, lo, hi = RR.ranks(q, n)
            assert h == q * (n - 1) and lo == int(np.floor(h)) and hi == min(lo + 1, n - 1) and 0 <= lo <= hi <= n - 1
        h, lo, hi = RR.ranks(0.5, n)
        assert (h == lo) == (n % 2 == 1)            # an odd count: the median is a sample
        assert RR.ranks(1.0, n)[1] == n - 1 and RR.ranks(0.0, n)[1] == 0


def test_mad_against_scipy():
    """``mad`` subtracts c = fp32(median) in fp32; scipy subtracts the float64 median in float64.  The median moves by no more than
    its arguments do, so |mad - scipy| <= |c - median| + one fp32 rounding of the largest |y - c|."""
    rng = np.random.RandomState(3)
    for T in (48, 47):
        y = (5 + rng.randn(T, 4, 3, 2) * np.array([0.1, 3.0])).astype(np.float32)
        y[5, 1, 1, 1] = np.nan
        im = RR.robust_images(y)
        want = scipy.stats.median_abs_deviation(y.astype(np.float64), axis=0, nan_policy="omit")
        med = np.nanmedian(y.astype(np.float64), axis=0)
        np.testing.assert_array_equal(im["median"], med)
        c = med.astype(np.float32).astype(np.float64)
        bound = np.abs(c - med) + F32_HALF_ULP * np.nanmax(np.abs(y - c[None]), axis=0)
        err = np.abs(im["mad"] - want)
        print(f"T={T}: worst |mad - scipy| / bound = {(err / bound).max():.3f}, worst relative {np.max(err / want):.2e}")
        assert (err <= bound).all()
        if T == 47:       # an odd count: the median is a sample, c = median exactly
            assert (c == med)[np.isfinite(y).all(0)].all()
        np.testing.assert_array_equal(RR.robust_images(y, noise="mad")["noise"], 1.4826 * im["mad"])


def test_noise_against_k21_on_single_series():
    """K21's D2 centres the differences on their median before the MAD; the noise image does not.  The two differ by no more
    than 1.4826 / sqrt(2) (|median d| + one fp32 rounding of the largest |d|), and share the constants."""
    rng = np.random.RandomState(4)
    y = (3 + np.cumsum(rng.randn(60, 5, 4, 1) * 0.01, axis=0) + rng.randn(60, 5, 4, 1) * 0.3).astype(np.float32)
    y[7, 2, 2, 0] = np.nan
    y[30, 0, 1, 0] = np.inf
    noise = RR.robust_images(y)["noise"]
    assert RR.NOISE_DIFF_SCALE == 1.4826 / np.sqrt(2.0)
    for p in np.ndindex(5, 4, 1):
        series = np.where(np.isfinite(y[(slice(None),) + p]), y[(slice(None),) + p], np.nan).astype(np.float64)
        d = DCR.adjacent_differences(series)
        want = DCR.estimate_noise(series)
        bound = RR.NOISE_DIFF_SCALE * (abs(np.median(d)) + F32_HALF_ULP * np.abs(d).max())
        assert abs(noise[p] - want) <= bound, (p, noise[p], want, bound)
        # and on differences of median exactly 0 the two agree to the fp32 rounding alone
    sym = np.array([0, 1, 0, -1, 0, 1, 0, -1, 0], dtype=np.float32).reshape(9, 1, 1, 1) * 0.25
    assert RR.robust_images(sym)["noise"][0, 0, 0] == DCR.estimate_noise(sym.ravel().astype(np.float64))


def test_robust_images_definition():
    y = mixed_rows(33, 24, seed=5).reshape(33, 4, 3, 2)
    im = RR.robust_images(y, percentiles=(8, 92.5))
    x = np.where(np.isfinite(y), y, np.nan).astype(np.float64)
    with np.errstate(all="ignore"), pytest.warns(RuntimeWarning):
        np.testing.assert_array_equal(im["median"], np.nanmedian(x, 0))
        np.testing.assert_array_equal(im["max"], np.nanmax(x, 0))
        np.testing.assert_array_equal(im["percentile"][8], np.nanquantile(x, 8 / 100.0, axis=0))
        np.testing.assert_array_equal(im["percentile"][92.5], np.nanquantile(x, 92.5 / 100.0, axis=0))
    np.testing.assert_array_equal(im["n"], np.isfinite(y).sum(0))
    bad = ~(np.isfinite(im["noise"]) & (im["noise"] != 0) & (im["n"] >= 2))
    np.testing.assert_array_equal(np.isnan(im["pnr"]), bad)
    ok = ~bad
    np.testing.assert_array_equal(im["pnr"][ok], ((im["max"] - im["median"]) / im["noise"])[ok])
    flat = {k: im[k].reshape(-1) for k in ("pnr", "noise", "n", "mad")}
    assert flat["noise"][3] == 0 and flat["mad"][3] == 0 and np.isnan(flat["pnr"][3])        # the constant voxel
    assert flat["n"][4] == 0 and flat["n"][5] == 1 and np.isnan(flat["pnr"][4]) and np.isnan(flat["pnr"][5])
    with pytest.raises(ValueError, match="noise"):
        RR.robust_images(y, noise="std")


@functools.lru_cache(maxsize=None)
def planted(Z):
    video, cells, still, sigma = RR.planted_case(RR.PLANTED_SEEDS[Z], Z)
    images = RR.robust_images(video)
    k18 = SR.summary_images(video, "full")
    return video, cells, still, sigma, images, k18


def first_picks(image, K, sigma):
    return DR.detect(RR.nan_to_min(image), K, sigma)["positions"]


@pytest.mark.parametrize("Z", [1, 2])
def test_planted_case_conditions(Z):
    """On the float64 definition alone: pnr finds the two dim, active cells first; max and the mean find the static blob first.
    Whether corr finds both cells is printed, not required."""
    video, cells, still, sigma, im, k18 = planted(Z)
    assert video.shape == (48, 40, 36, Z) and np.isnan(video).sum() == 1 and np.isnan(video[7, 0, 0, 0])
    got = first_picks(im["pnr"], 2, sigma)
    dist = np.linalg.norm(got[None] - cells[:, None], axis=2)
    sites = [RR.nearest_voxel(c) for c in cells] + [RR.nearest_voxel(still)]
    mean = np.where(np.isfinite(video).all(0), video.astype(np.float64).mean(0), np.nan)
    np.testing.assert_allclose(k18["mean"][np.isfinite(mean)], mean[np.isfinite(mean)], rtol=1e-12)
    for name, img in (("pnr", im["pnr"]), ("max", im["max"]), ("mean", mean), ("corr", k18["corr"])):
        print(f"Z={Z} {name} at cell 0 / cell 1 / static blob: " + " / ".join(f"{img[s]:.2f}" for s in sites))
    assert np.isfinite(got).all() and dist.min(1).max() <= 1.5 and sorted(dist.argmin(1)) == [0, 1], got
    assert np.linalg.norm(first_picks(im["max"], 1, sigma)[0] - still) <= 1.5
    assert np.linalg.norm(first_picks(k18["mean"], 1, sigma)[0] - still) <= 1.5
    pc = first_picks(k18["corr"], 2, sigma)
    dc = np.linalg.norm(pc[None] - cells[:, None], axis=2)
    print(f"Z={Z} corr finds both cells: {bool(np.isfinite(pc).all() and dc.min(1).max() <= 1.5 and sorted(dc.argmin(1)) == [0, 1])}")
    assert im["n"][0, 0, 0] == 47 and (im["n"].reshape(-1)[1:] == 48).all()


def test_planted_seeds_are_the_first():
    """No smaller seed meets the conditions (the stated seeds are 0 at both sizes, so there is none to try)."""
    assert RR.PLANTED_SEEDS == {1: 0, 2: 0}
