"""The trace clean-up (K20) without a GPU: the float64 restatement (tests/traces_restatement.py) against independent
compositions of numpy and scipy, a planted case whose answer is known, the refusals, and the ABI and the argument checks of
the C entries on the library as built."""
import ctypes
import inspect

import numpy as np
import pytest

import traces_restatement as TR

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


def window(t, W, T):
    lo = t - (W - 1) // 2 if W % 2 else t - W // 2
    hi = t + (W - 1) // 2 if W % 2 else t + W // 2 - 1
    return max(lo, 0), min(hi, T - 1)


# ---- 1. the pieces against independent compositions -----------------------------------------------------------------------------
@pytest.mark.parametrize("T,W", [(37, 7), (37, 10), (37, 1), (37, 2), (5, 40), (6, 41), (1, 3), (2, 3), (64, 40)])
def test_running_median_against_nanmedian_over_window_slices(T, W):
    rng = np.random.RandomState(T * 100 + W)
    y = rng.uniform(0.5, 2.0, T)
    y[rng.rand(T) < 0.3] = np.nan
    if T > 20:
        y[8:8 + min(W + 3, 12)] = np.nan           # a stretch longer than a short window: all-NaN windows
        y[20] = y[21] = y[22]                      # equal values around a median
    got = TR.running_median(y, W)
    got_inc = TR.running_median(y, W, includenan=True)
    empty = 0
    for t in range(T):
        lo, hi = window(t, W, T)
        v = y[lo:hi + 1]
        if np.isnan(v).all():
            empty += 1
            assert np.isnan(got[t])
        else:
            want = np.nanmedian(v)
            assert abs(got[t] - want) <= EPS * abs(want), (t, got[t], want)
        if np.isnan(v).any():
            assert np.isnan(got_inc[t])
        else:
            assert abs(got_inc[t] - np.median(v)) <= EPS * abs(np.median(v))
    if T > 20 and W <= 7:
        assert empty > 0


def test_running_mean_against_window_slices():
    rng = np.random.RandomState(5)
    y = rng.uniform(0.5, 2.0, 41)
    y[[7, 30]] = np.nan
    for W in (1, 4, 5, 60):
        got = TR.running_mean(y, W)
        for t in range(len(y)):
            lo, hi = window(t, W, len(y))
            want = y[lo:hi + 1].mean()
            assert (np.isnan(got[t]) and np.isnan(want)) or abs(got[t] - want) <= 4 * EPS * abs(want) * (hi - lo + 1)


def test_percentile_against_numpy_hazen():
    rng = np.random.RandomState(6)
    for n in (1, 2, 3, 9, 10, 11, 19, 20, 21, 200, 1001):
        v = rng.uniform(0.2, 3.0, n)
        v[rng.rand(n) < 0.2] = np.nan
        if np.isnan(v).all():
            v[0] = 1.0
        for p in (5, 50, 95):
            want = np.nanpercentile(v, p, method="hazen")
            assert abs(TR.prctile(v, p) - want) <= 4 * EPS * abs(want), (n, p)
    assert np.isnan(TR.prctile(np.full(4, np.nan), 5))
    assert TR.nanmedian([3.0, np.nan, 1.0, 2.0, 7.0]) == 2.5 and TR.nanmedian([4.0, np.nan, 1.0]) == 2.5
    assert np.isnan(TR.nanmedian([np.nan]))


@pytest.mark.parametrize("seed", range(6))
def test_exponential_fit_against_curve_fit(seed):
    """Same model, float64.  The squared error of the restatement's fit is at most curve_fit's times (1 + 1e-10): comparing the
    objective, not the parameters, does not depend on where each solver stops."""
    from scipy.optimize import curve_fit
    rng = np.random.RandomState(seed)
    n = (50, 400, 1000, 400, 400, 30)[seed]
    x = np.sort(rng.choice(np.arange(1, 2 * n + 1), n, replace=False)).astype(np.float64)
    a0, b0 = rng.uniform(0.5, 50.0), (-1.0 / rng.uniform(0.3 * n, 3 * n) if seed != 4 else 1.0 / (2.0 * n))
    noise = (0.02, 0.2, 0.05, 0.5, 0.05, 0.1)[seed]
    y = a0 * np.exp(b0 * x) * (1 + noise * rng.standard_normal(n))
    if seed == 3:
        y[::7] = -0.1                              # samples the log-linear start has to leave out
    a, b = TR.expfit(x, y)

    def sse(a, b):
        return ((y - a * np.exp(b * x)) ** 2).sum()

    p, _ = curve_fit(lambda x, a, b: a * np.exp(b * x), x, y, p0=(a, b * (1 + 1e-3)), xtol=1e-15, ftol=1e-15, gtol=1e-15,
                     maxfev=20000)
    assert sse(a, b) <= sse(*p) * (1 + 1e-10), (sse(a, b), sse(*p))
    # and from curve_fit's own start, the crude log-linear one
    ok = y > 0
    slope, icpt = np.polyfit(x[ok], np.log(y[ok]), 1)
    p2, _ = curve_fit(lambda x, a, b: a * np.exp(b * x), x, y, p0=(np.exp(icpt), slope), xtol=1e-15, ftol=1e-15, gtol=1e-15,
                      maxfev=20000)
    assert sse(a, b) <= sse(*p2) * (1 + 1e-10), (sse(a, b), sse(*p2))


def test_exponential_fit_of_a_constant_is_exactly_flat():
    """A constant gives b == 0 exactly (never a decay of rounding size, which would be subtracted): the start is relative to the
    largest sample and the step is a sum of residuals that are exactly zero."""
    for c in (np.float64(np.float32(0.7)), 3.0, np.float64(np.float32(123.456))):
        a, b = TR.expfit(np.arange(3, 300, dtype=np.float64), np.full(297, c))
        assert b == 0.0 and a == c


def test_interpolation_against_numpy_interp():
    rng = np.random.RandomState(8)
    y = rng.uniform(0.5, 2.0, 80)
    y[rng.rand(80) < 0.4] = np.nan
    y[:3] = np.nan
    y[-4:] = np.nan
    y[40:52] = np.nan
    got = TR.interp_linear(y)
    ok = np.flatnonzero(~np.isnan(y))
    t = np.arange(80)
    inside = (t >= ok[0]) & (t <= ok[-1])
    want = np.interp(t, ok, y[ok])
    assert np.isnan(got[~inside]).all() and not np.isnan(got[inside]).any()
    np.testing.assert_allclose(got[inside], want[inside], rtol=4 * EPS)
    np.testing.assert_array_equal(got[ok], y[ok])
    assert np.isnan(TR.interp_linear(np.full(5, np.nan))).all()


# ---- 2. a planted case ---------------------------------------------------------------------------------------------------------
def planted(seed=0, K=6, T=400):
    """(baseline + activity) exp(-t / tau_k), one single-frame spike in four of the neurons -- the mean plus 20 standard
    deviations of the clean trace on top of it: the reference's threshold is sigma standard deviations from the mean -- and a few
    dropouts to 0.  The activity is a transient every 50 frames that decays within about 9 frames to below the baseline's own
    change per frame: a window of the running median (40 frames) then holds at most one, over less than half its length, so
    the median follows the baseline and the fitted decay is the planted one."""
    rng = np.random.RandomState(seed)
    t = np.arange(T)
    tau = rng.uniform(150.0, 400.0, K)
    activity = np.zeros((K, T))
    for k in range(K):
        for s in range(12 + 7 * k, T - 12, 50):
            activity[k, s:] += rng.uniform(4.0, 12.0) * np.exp(-(t[s:] - s) / 2.0)
    clean = (40.0 + activity) * np.exp(-t[None, :] / tau[:, None])
    traces = clean.copy()
    spikes = {0: 57, 2: 201, 3: 333, 5: 120}
    for k, s in spikes.items():
        traces[k, s] += clean[k].mean() + 20.0 * clean[k].std()
    drops = [(1, 90), (1, 91), (4, 250), (2, 20)]
    for k, s in drops:
        traces[k, s] = 0.0
    return traces.astype(np.float32), activity, tau, spikes, drops


def corr(u, v):
    ok = ~np.isnan(u) & ~np.isnan(v)
    return np.corrcoef(u[ok], v[ok])[0, 1]


def test_planted_case_mode_2():
    traces, activity, tau, spikes, drops = planted()
    before = traces.copy()
    out, scales, offsets, info = TR.clean_traces(traces, 4.0)
    np.testing.assert_array_equal(traces, before)                      # the input is never modified
    K, T = traces.shape
    assert out.shape == (K, T) and out.dtype == np.float64 and scales.shape == offsets.shape == (K,)
    # exactly the planted spikes are flagged
    assert info["n_outliers"].tolist() == [1 if k in spikes else 0 for k in range(K)]
    for k, s in spikes.items():
        assert np.isnan(out[k, s - 1:s + 2]).all()                     # the median of three spreads the hole
    for k, s in drops:
        assert np.isnan(out[k, s])
    assert np.isnan(out[:, :2]).all() and np.isnan(out[:, -1]).all()   # round(4 / 2) = 2 leading frames, the last one
    assert not np.isnan(out[:, 3:10]).any()
    assert info["fitted"].all()
    np.testing.assert_allclose(info["b"], -1.0 / tau, rtol=0.02)
    valid = ~np.isnan(out)
    assert out[valid].min() >= 0.05 - 1e-12 and out[valid].max() <= 0.95 + 1e-12
    for k in range(K):
        assert abs(np.nanmin(out[k]) - 0.05) <= 1e-12 and abs(np.nanmax(out[k]) - 0.95) <= 1e-12
        assert corr(out[k], activity[k]) > corr(traces[k].astype(np.float64), activity[k]), k
    # scales and offsets undo the normalisation: x = (out - 0.05) / 0.9 scale + offset is the trace minus its curve plus a
    x = (out - 0.05) / 0.9 * scales[:, None] + offsets[:, None]
    xs = np.arange(1, T + 1)
    curve = info["a"][:, None] * np.exp(info["b"][:, None] * xs[None, :])
    want = traces.astype(np.float64) - curve + info["a"][:, None]
    ok = valid.copy()
    for k, s in spikes.items():
        ok[k, s - 1:s + 2] = False
    inner = ok & np.roll(ok, 1, axis=1) & np.roll(ok, -1, axis=1)
    med3 = np.median(np.stack([np.roll(want, 1, axis=1), want, np.roll(want, -1, axis=1)]), axis=0)
    # the median of three commutes with the subtraction of a curve only up to the curve's change over a frame
    assert np.abs(x - med3)[inner].max() <= 0.02 * np.abs(want[inner]).max()


def test_planted_case_mode_3_and_mode_0():
    traces, activity, tau, spikes, drops = planted(seed=1)
    out2, _, _, info2 = TR.clean_traces(traces, 4.0, detrend_mode=2)
    out3, scales, offsets, info3 = TR.clean_traces(traces, 4.0, detrend_mode=3)
    F0 = info2["F0"]                                    # per neuron: the same percentile in both modes
    med = np.median(F0)
    assert med > 1 and (scales == max(med, 1.0)).all() and (offsets == 0).all() and (info3["F0"] == med).all()
    np.testing.assert_array_equal(info3["b"], info2["b"])
    # dF/F0 units: not rescaled to [0.05, 0.95]
    xs = np.arange(1, traces.shape[1] + 1)
    k = 0
    ok = ~np.isnan(out3[k])
    resid = out3[k][ok] * med + info3["a"][k] * np.exp(info3["b"][k] * xs[ok])
    assert np.nanmax(np.abs(resid)) > 1.0
    # a small F0 is lifted to 1
    _, s_small, _, i_small = TR.clean_traces(traces / 100.0, 4.0, detrend_mode=3)
    assert i_small["F0"][0] < 1 and (s_small == 1.0).all()
    # mode 0: masks, outliers and the rescale only
    out0, s0, o0, info0 = TR.clean_traces(traces, 4.0, detrend_mode=0)
    assert np.isnan(info0["F0"]).all() and not info0["fitted"].any() and np.isnan(info0["a"]).all()
    np.testing.assert_array_equal(info0["n_outliers"], info2["n_outliers"])
    np.testing.assert_array_equal(np.isnan(out0), np.isnan(out2))
    x0 = (out0 - 0.05) / 0.9 * s0[:, None] + o0[:, None]
    ok = ~np.isnan(out0) & (np.arange(traces.shape[1])[None, :] > 3)
    assert np.abs(x0 - traces)[ok].max() <= 0.05 * traces.max()        # up to the median of three


def test_planted_case_mode_1_interpolation_and_smoothing():
    traces, activity, tau, spikes, drops = planted(seed=2)
    tau_common = 250.0
    t = np.arange(traces.shape[1])
    common = ((40.0 + activity) * np.exp(-t / tau_common)[None, :]).astype(np.float32)
    out, scales, offsets, info = TR.clean_traces(common, 4.0, detrend_mode=1)
    assert info["fitted"].all() and len(set(info["b"].tolist())) == 1 and len(set(info["a"].tolist())) == 1
    assert info["b"][0] < 0        # the scaled traces are a decay plus an offset: the rate is not the planted one
    valid = ~np.isnan(out)
    assert out[valid].min() >= 0.05 - 1e-12 and out[valid].max() <= 0.95 + 1e-12
    # linear interpolation fills every hole between the first and the last valid frame and nothing else
    plain = TR.clean_traces(traces, 4.0)[0]
    filled = TR.clean_traces(traces, 4.0, interp_method="linear")[0]
    for k in range(len(traces)):
        ok = np.flatnonzero(~np.isnan(plain[k]))
        assert not np.isnan(filled[k, ok[0]:ok[-1] + 1]).any()
        assert np.isnan(filled[k, :ok[0]]).all() and np.isnan(filled[k, ok[-1] + 1:]).all()
    # smoothing: a window with a NaN gives NaN, so the holes grow by the window
    for method in ("movmean", "movmedian"):
        sm = TR.clean_traces(traces, 4.0, smooth_method=method, smooth_window=5)[0]
        assert np.isnan(sm).sum() > np.isnan(plain).sum()
        assert np.nanmin(sm) >= 0.05 - 1e-12 and np.nanmax(sm) <= 0.95 + 1e-12
    # without a window nothing is smoothed, as in the reference
    np.testing.assert_array_equal(TR.clean_traces(traces, 4.0, smooth_method="movmean")[0], plain)


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    traces = planted()[0]
    for name in ("causal", "high", "low"):
        with pytest.raises(NotImplementedError, match="reference does not contain"):
            TR.clean_traces(traces, 4.0, smooth_method=name, smooth_window=3)
    with pytest.raises(ValueError, match="interp_method"):
        TR.clean_traces(traces, 4.0, interp_method="cubic")
    with pytest.raises(ValueError, match="smooth_method"):
        TR.clean_traces(traces, 4.0, smooth_method="gaussian", smooth_window=3)
    from dnmf_amd import ops

    class FakeRows:     # enough of a tensor to reach the option checks without a GPU
        dtype, is_cuda, shape = None, True, (2, 8)

        def dim(self):
            return 2

        def stride(self, i):
            return 1

    import torch
    FakeRows.dtype = torch.float32
    for name in ("causal", "high", "low"):
        with pytest.raises(NotImplementedError, match="reference does not contain"):
            ops.clean_traces(FakeRows(), 4.0, smooth_method=name, smooth_window=3)
    with pytest.raises(ValueError, match="interp_method"):
        ops.clean_traces(FakeRows(), 4.0, interp_method="cubic")


# ---- 4. the ABI on the library as built -----------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_entries(lib):
    from dnmf_amd import _lib, build
    assert _lib.SIGNATURES["dnmf_clean_traces_workspace"] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int])
    assert _lib.SIGNATURES["dnmf_clean_traces"][0] is ctypes.c_int
    assert lib.dnmf_clean_traces_workspace and lib.dnmf_clean_traces          # exported
    assert "clean_traces.hip" in build.SOURCES


def test_public_signatures():
    from dnmf_amd import ops
    from dnmf_amd.Demix.dNMF import DeformableNMF, MultiChannelDNMF
    from dnmf_amd.Demix.Traces import cleanTraces
    import Demix.Traces as shim

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    common = [("sigma_threshold", 10), ("detrend_mode", 2), ("interp_method", None), ("smooth_method", None), ("smooth_window", None)]
    assert params(cleanTraces) == [("traces", E), ("fps", E)] + common
    assert shim.cleanTraces is cleanTraces
    assert params(ops.clean_traces) == [("traces", E), ("fps", E)] + common + [("trim", True), ("floor", 0.01), ("workspace", None)]
    assert params(TR.clean_traces) == [("traces", E), ("fps", E)] + common + [("trim", True), ("floor", 0.01)]
    assert [p[0] for p in params(DeformableNMF.clean_traces)] == ["self", "fps", "kw"]
    assert MultiChannelDNMF.clean_traces is DeformableNMF.clean_traces


def test_argument_errors_of_the_entries(lib):
    """Validation happens before any HIP call, so it can be exercised without a GPU."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    ws, run = lib.dnmf_clean_traces_workspace, lib.dnmf_clean_traces

    def al(n):
        return (n + 255) // 256 * 256

    assert ws(3, 7) == 256 + 2 * al(3 * 7 * 8)
    assert ws(256, 16000) == 256 + 2 * 256 * 16000 * 8
    assert ws(0, 7) == 0 and lib.dnmf_last_error().startswith(b"dnmf_clean_traces_workspace: ") and b"K=0" in lib.dnmf_last_error()
    assert ws(3, 0) == 0 and b"T=0" in lib.dnmf_last_error()
    assert ws(3, 18432) > 0
    assert ws(3, 18433) == 0 and b"LDS" in lib.dnmf_last_error()          # refused, never truncated
    assert ws(18433, 8) == 0
    need = ws(3, 7)
    names = ["traces", "ldt", "K", "T", "fps", "sigma", "mode", "interp", "smooth", "window", "trim", "floor", "out", "ldo", "scales",
             "offsets", "a", "b", "F0", "fitted", "n_outliers", "workspace", "bytes", "stream"]
    ok = (p, 7, 3, 7, 4.0, 10.0, 2, 0, 0, 0, 1, 0.01, p, 7, p, p, p, p, p, p, p, p, need, None)

    def call(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return run(*args)

    for name in ("traces", "out", "scales", "offsets", "a", "b", "F0", "fitted", "n_outliers", "workspace"):
        assert call(**{name: None}) == -1 and lib.dnmf_last_error().startswith(b"dnmf_clean_traces: "), name
    assert call(K=0) == -2 and call(T=0) == -2
    assert call(ldt=6) == -2 and b"ldt" in lib.dnmf_last_error()
    assert call(ldo=6) == -2
    assert call(fps=0.0) == -2 and b"fps" in lib.dnmf_last_error()
    assert call(fps=0.04) == -2 and b"running median" in lib.dnmf_last_error()        # W = round(0.4) = 0
    assert call(sigma=-1.0) == -2
    assert call(floor=float("nan")) == -2
    assert call(mode=4) == -2 and call(mode=-1) == -2
    assert call(interp=2) == -2
    assert call(smooth=3) == -2
    assert call(smooth=1, window=0) == -2 and b"smooth_window" in lib.dnmf_last_error()
    assert call(T=18433, ldt=18433, ldo=18433) == -3
    assert call(bytes=need - 1) == -4 and str(need).encode() in lib.dnmf_last_error()
    assert call(workspace=p + 4) == -4 and b"aligned" in lib.dnmf_last_error()
