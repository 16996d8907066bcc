"""The spike deconvolution (K21) without a GPU: the float64 restatement (tests/deconv_restatement.py) against scikit-learn's isotonic
regression, against itself by segments, against the KKT conditions of the convex problem, its estimators against numpy and scipy, a
planted case whose answer is known, and the ABI and the argument checks of the C entries on the library as built."""
import ctypes
import inspect

import numpy as np
import pytest

import deconv_restatement as DR

G = float(np.exp(-0.3))


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


def simulated(T, seed, noise=0.1, density=0.1, baseline=1.0, g=G):
    """Unit spikes at ``density`` through the AR(1) decay g, on a baseline, plus white noise -> ``(y, spikes)``."""
    rng = np.random.RandomState(seed)
    s = (rng.rand(T) < density).astype(np.float64)
    c = np.zeros(T)
    for t in range(T):
        c[t] = (g * c[t - 1] if t else 0.0) + s[t]
    return baseline + c + noise * rng.randn(T), s


def missing_patterns(y, seed=5):
    """The trace with a leading run, an interior gap longer than a segment (of 8 or 17 frames), the last frame and 10 % at random
    missing -- one pattern each, then all together."""
    T = len(y)
    rng = np.random.RandomState(seed)
    masks = dict(leading=np.arange(T) < 6, gap=(np.arange(T) >= T // 3) & (np.arange(T) < T // 3 + 40), last=np.arange(T) == T - 1,
                 random=rng.rand(T) < 0.1)
    masks["all"] = masks["leading"] | masks["gap"] | masks["last"] | masks["random"]
    out = {}
    for name, m in masks.items():
        out[name] = np.where(m, np.nan, y)
    return out


# ---- 1. D1 against independent statements --------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 0.5, 2.0])
def test_solution_is_the_isotonic_regression_under_the_x_mapping(lam):
    from sklearn.isotonic import isotonic_regression
    T = 300
    assert T * abs(np.log(G)) < 300                    # g^-t stays finite
    y, _ = simulated(T, 11)
    a, d = DR.terms(y, G, lam, 1.0)
    t = np.arange(T)
    x = isotonic_regression(a / G ** t, sample_weight=G ** (2 * t), increasing=True)
    want = np.maximum(x, 0.0) * G ** t
    c, s, _ = DR.solve(y, G, lam, 1.0)
    assert np.abs(c - want).max() <= 1e-12 * np.abs(y).max()


@pytest.mark.parametrize("tree", [False, True])
@pytest.mark.parametrize("seg", [1, 8, 17])
def test_segments_and_stitch_give_the_sequential_result(seg, tree):
    y, _ = simulated(300, 12)
    for name, ym in dict(missing_patterns(y), full=y).items():
        for lam in (0.0, 0.5):
            c0, s0, p0 = DR.solve(ym, G, lam, 1.0)
            c1, s1, p1 = DR.solve(ym, G, lam, 1.0, seg=seg, tree=tree)
            bound = 1e-12 * np.nanmax(np.abs(ym))
            assert np.abs(c1 - c0).max() <= bound and np.abs(s1 - s0).max() <= bound, (name, lam)
            assert np.array_equal(p0[0], p1[0]), (name, lam)          # the same pools


@pytest.mark.parametrize("name", ["leading", "gap", "last", "random", "all"])
@pytest.mark.parametrize("seg", [None, 8, 17])
def test_kkt_with_missing_frames(name, seg):
    y, _ = simulated(300, 13)
    ym = missing_patterns(y)[name]
    for lam in (0.0, 0.5, 2.0):
        c, s, _ = DR.solve(ym, G, lam, 1.0, seg=seg)
        min_s, min_grad, comp = DR.kkt(ym, G, lam, 1.0, c, s)
        assert min_s >= 0 and min_grad >= -1e-10 and comp <= 1e-10, (lam, min_s, min_grad, comp)
        # the spikes that came with c are its own: c = K s
        rebuilt = np.zeros(len(c))
        for t in range(len(c)):
            rebuilt[t] = (G * rebuilt[t - 1] if t else 0.0) + s[t]
        assert np.abs(rebuilt - c).max() <= 1e-12 * np.abs(y).max()
        # and the certificate from c alone differs only by roundings inside the pools
        loose = DR.kkt(ym, G, lam, 1.0, c)
        assert loose[0] >= -1e-12 and loose[1] >= -1e-10 and loose[2] <= 1e-10


def test_kkt_rejects_what_is_not_the_solution():
    y, _ = simulated(300, 13)
    c, s, _ = DR.solve(y, G, 0.5, 1.0)
    worse = c * 1.01
    assert DR.kkt(y, G, 0.5, 1.0, worse)[2] > 1e-4
    assert DR.kkt(y, G, 0.5, 1.0, np.maximum(y - 1.0, 0.0))[0] < -1e-3        # the clipped data decay too fast: s < 0


def test_consequences_of_d1():
    y, _ = simulated(300, 14)
    ym = missing_patterns(y)["all"]
    lead = 6
    c, s, (S, L, N, D) = DR.solve(ym, G, 0.5, 1.0)
    starts = np.zeros(300, bool)
    starts[S] = True
    assert S[0] == 0 and (S[1:] == S[:-1] + L[:-1]).all() and S[-1] + L[-1] == 300
    # a leading run of missing frames: pools of their own, c = s = 0; the first valid frame starts a fresh pool
    assert np.isnan(ym[:lead]).all() and not np.isnan(ym[lead])
    assert starts[:lead + 1].all() and (D[:lead] == 0).all() and (c[:lead] == 0).all() and (s[:lead] == 0).all()
    # missing frames in the middle and at the end merge backwards: they start no pool, s = 0, c decays through them
    later = np.flatnonzero(np.isnan(ym))
    later = later[later > lead]
    assert len(later) > 40 and np.isnan(ym[-1])
    assert not starts[later].any() and (s[later] == 0).all()
    assert np.abs(c[later] - G * c[later - 1]).max() <= 1e-15 * c.max()
    assert (D > 0)[lead:].all()
    # c = max(v, 0) g^k over a pool; s exactly 0 inside it; at its start s = max(c_t - g c_{t-1}, 0); s_0 = c_0
    for t0, l, n, d in zip(S, L, N, D):
        v = n / d if d > 0 else -np.inf
        assert np.array_equal(c[t0:t0 + l], max(v, 0.0) * G ** np.arange(l))
        assert (s[t0 + 1:t0 + l] == 0).all()
        assert s[t0] == (c[0] if t0 == 0 else max(c[t0] - G * c[t0 - 1], 0.0))
    assert (s >= 0).all() and (c >= 0).all()
    # without a leading run s_0 = c_0 is the first sample's own
    c2, s2, _ = DR.solve(y, G, 0.0, 1.0)
    assert s2[0] == c2[0]
    # a negative trace: c = 0 everywhere
    c3, s3, _ = DR.solve(-np.abs(y), G, 0.3, 0.0)
    assert (c3 == 0).all() and (s3 == 0).all()


# ---- 2. the estimators ----------------------------------------------------------------------------------------------------------
def test_noise_baseline_and_decay_estimates():
    from scipy.stats import median_abs_deviation
    y, _ = simulated(1000, 15, noise=0.3)
    ym = missing_patterns(y)["all"]
    for v in (y, ym):
        w = np.isfinite(v)
        d = (v[1:] - v[:-1])[w[1:] & w[:-1]]
        want = 1.4826 * median_abs_deviation(d) / np.sqrt(2.0)
        assert abs(DR.estimate_noise(v) - want) <= 4 * np.finfo(float).eps * want
        for p in (10.0, 0.0, 37.5, 100.0):
            want = np.nanpercentile(v, p, method="hazen")
            assert abs(DR.estimate_baseline(v, p) - want) <= 4 * np.finfo(float).eps * abs(want), p
        # D3 by plain loops
        m = v[w].mean()
        ac = []
        for k in (1, 2):
            terms = [(v[t] - m) * (v[t + k] - m) for t in range(len(v) - k) if w[t] and w[t + k]]
            ac.append(sum(terms) / len(terms))
        assert abs(DR.estimate_decay(v) - ac[1] / ac[0]) <= 1e-12
    # white noise enters lag 0 only, so the estimate has no bias from it; its scatter: an autocovariance of T samples of variance
    # var has the standard error var / sqrt(T), the ratio of two the relative errors of both -- three of those are allowed
    for noise in (0.1, 0.3, 1.0):
        T = 4000
        got = DR.estimate_decay(simulated(T, 16, noise=noise)[0])
        signal = 0.1 * 0.9 / (1.0 - G * G)        # variance of the calcium trace: density (1 - density) / (1 - g^2)
        se = (signal + noise ** 2) / np.sqrt(T)
        allowed = 3.0 * G * np.hypot(se / (signal * G), se / (signal * G * G))
        print(f"decay estimate at noise {noise}: {got:.3f} (true {G:.3f}, allowed deviation {allowed:.3f})")
        assert abs(got - G) <= allowed
    # the noise estimate is of the right size (spikes widen the differences a little)
    for noise in (0.1, 0.3, 1.0):
        got = DR.estimate_noise(simulated(4000, 16, noise=noise)[0])
        assert noise <= got <= 1.6 * noise, (noise, got)


@pytest.mark.parametrize("noise", [0.1, 0.3])
def test_penalty_search_brackets_the_noise_level(noise):
    y, _ = simulated(1000, 17, noise=noise)
    ym = missing_patterns(y)["all"]
    for v in (y, ym):
        b, sigma = DR.estimate_baseline(v), DR.estimate_noise(v)
        target = sigma ** 2 * np.isfinite(v).sum()
        r0 = DR.rss(v, b, DR.solve(v, G, 0.0, b)[0])
        assert r0 < target                                   # the search is exercised, not skipped
        lam, width = DR.search_penalty(v, G, b, sigma)
        assert lam > 0 and 0 < width <= 2 * max(lam, sigma) / 2 ** DR.HALVINGS

        def rss(l):
            return DR.rss(v, b, DR.solve(v, G, l, b)[0])
        assert rss(lam) >= target > rss(lam - 2 * width)
        # RSS does not fall as the penalty grows
        grid = [rss(l) for l in np.linspace(0.0, 2 * lam, 9)]
        assert all(b_ >= a_ - 1e-12 * target for a_, b_ in zip(grid, grid[1:]))
        c, s, info = DR.deconvolve(v, g=G)
        assert info["ok"] and info["penalty"] == lam and info["baseline"] == b and info["noise"] == sigma and info["rss"] == rss(lam)
    # nothing to remove: RSS(0) >= target gives 0
    assert DR.search_penalty(y, G, DR.estimate_baseline(y), 0.0) == (0.0, 0.0)
    const = np.full(50, 7.25)
    c, s, info = DR.deconvolve(const, g=G)
    assert info["ok"] and info["noise"] == 0 and info["penalty"] == 0 and np.abs(c).max() == 0


def test_refusals_per_trace():
    y, _ = simulated(64, 18)

    def refused(v, **kw):
        c, s, info = DR.deconvolve(v, **kw)
        assert np.isnan(c).all() and np.isnan(s).all() and len(c) == len(v)
        assert all(np.isnan(info[k]) for k in ("g", "penalty", "baseline", "noise", "rss"))
        return not info["ok"]

    three = np.full(64, np.nan)
    three[[3, 4, 5]] = y[[3, 4, 5]]
    assert refused(three, g=G, penalty=0.1, baseline=1.0)                    # fewer than 4 valid frames
    assert refused(np.full(64, np.nan), g=G) and refused(np.full(1, 2.0), g=G, penalty=0.0) and refused(y[:2], g=G, penalty=0.0)
    apart = np.full(64, np.nan)
    apart[::3] = y[::3]                                                      # valid frames, no adjacent pair
    assert refused(apart, g=G) and refused(apart, penalty=0.1) and refused(apart)
    assert DR.deconvolve(apart, g=G, penalty=0.1)[2]["ok"]                   # nothing to estimate from pairs
    assert DR.deconvolve(apart, g=G, noise=0.1)[2]["ok"]
    assert refused(np.full(64, 7.25))                                        # ac(1) = 0
    rng = np.random.RandomState(3)
    zigzag = 1.0 + 0.5 * (-1.0) ** np.arange(64) + 0.01 * rng.randn(64)
    assert DR.autocovariances(zigzag)[0] < 0 and refused(zigzag)             # ac(1) < 0
    assert refused(y, g=1.0) and refused(y, g=0.0) and refused(y, g=1.5)
    assert refused(y, g=G, penalty=-1.0) and refused(y, g=G, baseline=np.inf)
    # a refused trace does not disturb its neighbours
    c, s, info = DR.deconvolve_traces(np.stack([y, three, y]), g=[G, G, np.nan], penalty=0.2)
    assert info["ok"].tolist() == [True, False, True] and np.isnan(c[1]).all() and not np.isnan(c[[0, 2]]).any()
    assert info["g"][0] == G and info["g"][2] == DR.estimate_decay(y)


# ---- 3. a planted case -----------------------------------------------------------------------------------------------------------
def test_planted_spikes_are_found():
    """Unit spikes at density 0.1, g = e^-0.3, baseline 1, T = 4000, g known, everything else estimated."""
    for noise in (0.1, 0.3):
        y, spikes = simulated(4000, 19, noise=noise)
        c, s, info = DR.deconvolve(y, g=G)
        planted = spikes > 0
        found = s > 0.5
        hits, false = int((found & planted).sum()), int((found & ~planted).sum())
        print(f"noise {noise}: {hits} of {int(planted.sum())} planted spikes found, {false} false detections; "
              f"penalty {info['penalty']:.3f}, baseline {info['baseline']:.3f}, noise estimate {info['noise']:.3f}")
        if noise == 0.1:
            assert hits >= 0.95 * planted.sum() and false <= 0.02 * planted.sum()
            assert info["baseline"] < 1.0 and info["baseline"] > 1.0 - 3 * noise     # below the truth by a fraction of the noise


# ---- 4. the ABI on the library as built -------------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_entries(lib):
    from dnmf_amd import _lib, build
    assert _lib.SIGNATURES["dnmf_deconvolve_traces_workspace"] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int])
    res, args = _lib.SIGNATURES["dnmf_deconvolve_traces"]
    assert res is ctypes.c_int and args[8] is ctypes.c_double
    assert lib.dnmf_deconvolve_traces_workspace and lib.dnmf_deconvolve_traces          # exported
    assert "deconvolve_traces.hip" in build.SOURCES


def test_public_signatures():
    from dnmf_amd import ops
    from dnmf_amd.Demix.dNMF import DeformableNMF, MultiChannelDNMF
    from dnmf_amd.Demix.Traces import deconvolveTraces
    import Demix.Traces as shim

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    common = [("g", None), ("penalty", None), ("baseline", None), ("noise", None), ("baseline_percentile", 10.0)]
    assert params(ops.deconvolve_traces) == [("traces", E)] + common + [("workspace", None)]
    assert params(deconvolveTraces) == [("traces", E), ("fps", None), ("decay_time", None)] + common
    assert params(DR.deconvolve_traces) == [("traces", E)] + common
    assert shim.deconvolveTraces is deconvolveTraces
    assert [p[0] for p in params(DeformableNMF.deconvolve)] == ["self", "fps", "decay_time", "traces", "kw"]
    assert MultiChannelDNMF.deconvolve is DeformableNMF.deconvolve
    assert "self.last_deconv = None" in inspect.getsource(DeformableNMF.__init__)
    y = np.ones((2, 8), np.float32)
    with pytest.raises(ValueError, match="not both"):
        deconvolveTraces(y, fps=4.0, decay_time=1.0, g=0.5)
    with pytest.raises(ValueError, match="needs fps"):
        deconvolveTraces(y, decay_time=1.0)

    class FakeRows:     # enough of a tensor to reach the option checks without a GPU
        is_cuda, shape, device = True, (2, 8), "cpu"

        def dim(self):
            return 2

        def stride(self, i):
            return 1

    import torch
    FakeRows.dtype = torch.float32
    for kw in (dict(g=1.0), dict(g=0.0), dict(penalty=-0.5), dict(noise=-1.0), dict(baseline_percentile=101.0), dict(g=[0.5, 0.5, 0.5])):
        with pytest.raises(ValueError, match="deconvolve_traces: "):
            ops.deconvolve_traces(FakeRows(), **kw)


def test_argument_errors_of_the_entries(lib):
    """Validation happens before any HIP call, so it can be exercised without a GPU."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    ws, run = lib.dnmf_deconvolve_traces_workspace, lib.dnmf_deconvolve_traces

    def al(n):
        return (n + 255) // 256 * 256

    assert ws(3, 7) == 256 and ws(200, 6144) == 256                      # the records fit LDS
    assert ws(3, 6145) == 256 + al(3 * 6145 * 24)
    assert ws(2, 18432) == 256 + al(2 * 18432 * 24)
    assert ws(18432, 18432) == 256 + 18432 * 18432 * 24
    assert ws(0, 7) == 0 and lib.dnmf_last_error().startswith(b"dnmf_deconvolve_traces_workspace: ") and b"K=0" in lib.dnmf_last_error()
    assert ws(3, 0) == 0 and b"T=0" in lib.dnmf_last_error()
    assert ws(3, -1) == 0 and ws(-1, 3) == 0
    assert ws(3, 18433) == 0 and b"LDS" in lib.dnmf_last_error()         # refused, never truncated
    assert ws(18433, 8) == 0
    need = ws(3, 7)
    names = ["traces", "ldt", "K", "T", "g", "penalty", "baseline", "noise", "pct", "c", "s", "ldo", "info", "workspace", "bytes", "stream"]
    ok = (p, 7, 3, 7, None, None, None, None, 10.0, p, p, 7, p, p, need, None)

    def call(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return run(*args)

    for name in ("traces", "c", "s", "info", "workspace"):
        assert call(**{name: None}) == -1 and lib.dnmf_last_error().startswith(b"dnmf_deconvolve_traces: "), name
    assert call(K=0) == -2 and call(T=0) == -2
    assert call(ldt=6) == -2 and b"ldt" in lib.dnmf_last_error()
    assert call(ldo=6) == -2
    assert call(pct=-1.0) == -2 and b"baseline_percentile" in lib.dnmf_last_error()
    assert call(pct=100.5) == -2 and call(pct=float("nan")) == -2
    assert call(T=18433, ldt=18433, ldo=18433) == -3 and lib.dnmf_last_error().startswith(b"dnmf_deconvolve_traces: ")
    assert call(K=18433) == -3
    assert call(bytes=need - 1) == -4 and str(need).encode() in lib.dnmf_last_error()
    assert call(T=6145, ldt=6145, ldo=6145, bytes=need) == -4                # the workspace form needs its records
    assert call(workspace=p + 4) == -4 and b"aligned" in lib.dnmf_last_error()
