"""The restatement of K31 (tests/dff_restatement.py) pinned against numpy and scipy, the window plan of ``ops`` and of the
library against it, the derived bounds of the planted bleaching trace, the refusals and the ABI additions.  No GPU."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import scipy.ndimage
import torch

import detect_restatement as DR
import dff_restatement as DF
import robust_restatement as RR
from conftest import ROOT
from dnmf_amd.ops import baseline_apply, running_quantile, running_window_plan  # noqa: F401  (the entry points this file is about)


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


def plan_cases():
    for W in (1, 2, 3, 64):
        for S in sorted({1, 2, max(1, W // 2), W}):
            if S > W:
                continue
            for T in sorted({1, W - 1, W, W + 1, W + S, W + S + 1}):
                if T >= 1:
                    yield T, W, S


def test_window_plan(lib):
    from dnmf_amd import ops
    n = 0
    for T, W, S in plan_cases():
        p = DF.window_plan(T, W, S)
        J, s, e, c = p["J"], p["starts"], p["ends"], p["centres"]
        assert J == (1 if T <= W else -(-(T - W) // S) + 1), (T, W, S)
        assert len(s) == len(e) == len(c) == J and s[0] == 0 and e[-1] == T
        assert ((e - s) == min(W, T)).all()                           # every window is full-length (T >= W) or the movie
        covered = np.zeros(T, dtype=bool)
        for a, b in zip(s, e):
            covered[a:b] = True
        assert covered.all(), (T, W, S)
        assert (np.diff(c) > 0).all() and (np.diff(s) <= S).all()
        got = ops.running_window_plan(T, W, S)
        assert got["J"] == J and lib.dnmf_running_windows(T, W, S) == J
        for k in ("starts", "ends", "centres"):
            np.testing.assert_array_equal(got[k], p[k])
        n += 1
    assert n >= 50
    assert ops.running_window_plan(100, 40)["starts"].tolist() == [0, 10, 20, 30, 40, 50, 60]       # stride=None: window // 4
    assert ops.running_window_plan(5, 3)["starts"].tolist() == [0, 1, 2]                            # max(1, 3 // 4)


def edge_rows(T=47, P=12, seed=0):
    rng = np.random.RandomState(seed)
    x = (rng.randn(T, P) * 10.0 ** rng.randint(-3, 4, (1, P))).astype(np.float32)
    x[rng.rand(T, P) < 0.1] = 0.0
    x[rng.rand(T, P) < 0.05] = -0.0
    x[:, 1] = rng.randint(0, 2, T)                                    # ties
    x[:, 2] = (rng.randint(-3, 4, T) * 1e-42).astype(np.float32)      # denormals
    x[rng.rand(T, P) < 0.08] = np.nan
    x[rng.rand(T, P) < 0.03] = np.inf
    x[rng.rand(T, P) < 0.03] = -np.inf
    x[:, 4] = np.nan
    x[1:, 5] = np.nan                                                 # one sample, in the first frame
    return x


@pytest.mark.parametrize("W,S", [(1, 1), (8, 2), (9, 9), (16, 5), (64, 16)])
def test_knots_equal_nanquantile(W, S):
    x = edge_rows()
    clean = np.where(np.isfinite(x), x, np.nan).astype(np.float64)
    for q in (0.0, 0.08, 0.5, 1.0):
        r = DF.running_quantile(x, W, S, q)
        assert r["value"].shape == (len(r["centres"]), x.shape[1]) and r["lo"].dtype == np.float32
        for j, (s, e) in enumerate(zip(r["starts"], r["ends"])):
            for v in range(x.shape[1]):
                kept = clean[s:e, v][~np.isnan(clean[s:e, v])]
                assert r["n"][j, v] == len(kept)
                if len(kept) == 0:
                    assert np.isnan(r["value"][j, v]) and np.isnan(r["lo"][j, v])
                    continue
                want = np.nanquantile(kept, q, method="linear")
                assert r["value"][j, v] == want and not (r["lo"][j, v] == 0 and np.signbit(r["lo"][j, v])), (W, S, q, j, v)
                assert r["lo"][j, v] == np.sort(kept)[int(np.floor(q * (len(kept) - 1)))]
    few = DF.running_quantile(x, 16, 5, 0.5, min_samples=12)
    full = DF.running_quantile(x, 16, 5, 0.5)
    np.testing.assert_array_equal(np.isnan(few["value"]), full["n"] < 12)
    np.testing.assert_array_equal(few["lo"], full["lo"])


@pytest.mark.parametrize("W", [1, 5, 21])
def test_stride_one_is_a_median_filter(W):
    rng = np.random.RandomState(W)
    y = rng.randn(200).astype(np.float32)
    movie, knots = DF.dff_movie(y[:, None], W, 1, 0.5, mode="baseline")
    want = scipy.ndimage.median_filter(y.astype(np.float64), size=W, mode="nearest")
    h = W // 2
    np.testing.assert_array_equal(movie[h:200 - h, 0], want[h:200 - h].astype(np.float32))
    assert knots["centres"].tolist() == [float(h + j) for j in range(200 - W + 1)]
    assert (movie[:h, 0] == movie[h, 0]).all() and (movie[200 - h:, 0] == movie[199 - h, 0]).all()


def test_baseline_interpolation_and_modes():
    c = np.array([1.5, 4.5, 6.0])
    b = np.array([[1.0, np.nan], [4.0, 2.0], [1.0, 2.0]])
    f0 = DF.baseline(b, c, np.arange(8))
    np.testing.assert_array_equal(f0[:, 0], [1.0, 1.0, 1.0 + (0.5 / 3.0) * 3.0, 1.0 + (1.5 / 3.0) * 3.0, 1.0 + (2.5 / 3.0) * 3.0,
                                             4.0 + (0.5 / 1.5) * -3.0, 1.0, 1.0])
    np.testing.assert_array_equal(np.isnan(f0[:, 1]), [True, True, True, True, True, False, False, False])   # a NaN knot: its lines only
    np.testing.assert_array_equal(DF.baseline(b[::-1], [0.0, 2.0, 4.0], [2.0])[0], b[1])                   # w = 0: the knot itself
    y = np.array([[3.0, 3.0], [np.inf, 1.0], [2.0, np.nan], [1.0, 1.0]], dtype=np.float32)
    k = np.array([[2.0, -1.0]])
    for mode, want in (("baseline", [[2, -1], [np.nan, -1], [2, np.nan], [2, -1]]),
                       ("df", [[1, 4], [np.nan, 2], [0, np.nan], [-1, 2]]),
                       ("dff", [[0.5, np.nan], [np.nan, np.nan], [0, np.nan], [-0.5, np.nan]]),
                       ("dfsqrtf", [[1 / np.sqrt(2.0), np.nan], [np.nan, np.nan], [0, np.nan], [-1 / np.sqrt(2.0), np.nan]])):
        got, _ = DF.apply(y, k, [0.0], mode)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, np.array(want, dtype=np.float64).astype(np.float32), err_msg=mode)
    got, _ = DF.apply(y, k, [0.0], "dff", offset=1.0)
    np.testing.assert_array_equal(got[:, 1], [np.nan, np.nan, np.nan, np.nan])          # F0 + offset = 0: still refused
    got, _ = DF.apply(y, k, [0.0], "dff", offset=3.0)
    np.testing.assert_array_equal(got[:, 1], np.array([2.0, 1.0, np.nan, 1.0], dtype=np.float32))


def test_planted_bleaching_bounds():
    """B exp(-t / tau) plus non-negative transients that take fewer than percentile % of every window: the 8th percentile of a
    window is then a sample of the decaying baseline itself, so every knot lies within [min, max] of the planted baseline over
    its window, and every F0_t, a convex combination of two knots, within that of the two bracketing windows.  No measured
    constant.  The one global 8th percentile violates the bound in the early frames."""
    W, S, pct = 120, 30, 8.0
    y, base, on = DF.bleaching_trace()
    T = len(y)
    knots = DF.running_quantile(y[:, None], W, S, pct / 100.0)
    for s, e in zip(knots["starts"], knots["ends"]):
        assert on[s:e].sum() < pct / 100.0 * (e - s - 1), "the condition of the bound"
    lo = np.array([base[s:e].min() for s, e in zip(knots["starts"], knots["ends"])])
    hi = np.array([base[s:e].max() for s, e in zip(knots["starts"], knots["ends"])])
    b = knots["value"][:, 0]
    assert ((lo <= b) & (b <= hi)).all()
    f0 = DF.baseline(knots["value"], knots["centres"], np.arange(T))[:, 0]
    j = np.clip(np.searchsorted(knots["centres"], np.arange(T), side="right") - 1, 0, len(b) - 1)
    j2 = np.minimum(j + 1, len(b) - 1)
    assert ((np.minimum(lo[j], lo[j2]) <= f0) & (f0 <= np.maximum(hi[j], hi[j2]))).all()
    one = DF.running_quantile(y[:, None], T, T, pct / 100.0)["value"][0, 0]
    early = np.arange(T) < T // 4
    assert (one < np.minimum(lo[j], lo[j2])[early]).all()             # the global F0: below the baseline of every early frame
    df, _ = DF.apply(y[:, None], knots["value"], knots["centres"], "dff")
    glob, _ = DF.apply(y[:, None], np.array([[one]]), [0.0], "dff")
    print(f"median dF/F of the quiet early frames: running {np.median(df[early & ~on]):.3f}, global {np.median(glob[early & ~on]):.3f}")
    # a low percentile of a decaying window sits near the window's end: the running baseline lags by about half a window
    # (exp(50 / 300) - 1 = 0.18 here), the global one misses by the whole decay
    assert np.median(glob[early & ~on]) > 1.0 > 0.5 > np.abs(np.median(df[early & ~on]))


@functools.lru_cache(maxsize=None)
def bleaching(Z):
    return DF.bleaching_case(DF.BLEACH_SEEDS[Z], Z)


@pytest.mark.parametrize("Z", [1, 2])
def test_bleaching_case_on_the_definition(Z):
    """K14's definition on the max image of the raw movie returns the bright static blob first: the half that shows the
    feature is needed.  On the max image of the dF/F movie it returns the two firing cells."""
    video, cells, still, sigma = bleaching(Z)
    assert video.shape == (DF.BLEACH_FRAMES, 40, 36, Z) and np.isnan(video).sum() == 1
    raw_max = np.nanmax(video.astype(np.float64), axis=0)
    first = DR.detect(RR.nan_to_min(raw_max), 1, sigma)["positions"]
    assert np.linalg.norm(first[0] - still) <= 1.5
    movie, _ = DF.dff_movie(video, DF.BLEACH_WINDOW, DF.BLEACH_STRIDE, 0.08)
    with np.errstate(invalid="ignore"):
        dff_max = movie.astype(np.float64).max(0)                     # NaN where a sample is
    got = DR.detect(RR.nan_to_min(dff_max), 2, sigma)["positions"]
    dist = np.linalg.norm(got[None] - cells[:, None], axis=2)
    sites = [RR.nearest_voxel(c) for c in cells] + [RR.nearest_voxel(still)]
    for name, img in (("raw max", raw_max), ("dF/F max", dff_max)):
        print(f"Z={Z} {name} at cell 0 / cell 1 / static blob: " + " / ".join(f"{img[s]:.2f}" for s in sites))
    assert np.isfinite(got).all() and dist.min(1).max() <= 1.5 and sorted(dist.argmin(1)) == [0, 1], got


def test_refusals(lib):
    from dnmf_amd import ops
    rows = torch.zeros(4, 6)
    with pytest.raises(ValueError, match="running_quantile: window=2049"):
        ops.running_quantile(rows, (6, 1, 1), 2049)
    with pytest.raises(ValueError, match="running_quantile: stride=5"):
        ops.running_quantile(rows, (6, 1, 1), 4, 5)
    with pytest.raises(ValueError, match="running_quantile: stride=0"):
        ops.running_quantile(rows, (6, 1, 1), 4, 0)
    for q in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"running_quantile: q must lie in \[0, 1\]"):
            ops.running_quantile(rows, (6, 1, 1), 4, q=q)
    with pytest.raises(ValueError, match="running_quantile: frames must be float32 CUDA"):
        ops.running_quantile(rows, (6, 1, 1), 4)
    with pytest.raises(ValueError, match="running_window_plan: window=0"):
        ops.running_window_plan(10, 0)
    with pytest.raises(ValueError, match="baseline_apply: mode"):
        ops.baseline_apply(rows, (6, 1, 1), None, [0.0], mode="ratio")
    with pytest.raises(ValueError, match="baseline_apply: offset"):
        ops.baseline_apply(rows, (6, 1, 1), None, [0.0], offset=float("inf"))
    assert ops._overlap(rows[1:], rows[:2]) and not ops._overlap(rows, torch.zeros(4, 6))
    # the library's own checks, before any HIP call
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.addressof(buf)
    three, win = (ctypes.c_int * 3)(6, 1, 1), (ctypes.c_long * 2)(-1, -1)
    rq = lambda T, W, S, q, B=4, row0=0, run=0: lib.dnmf_running_quantile(a, 6, None, three, B, row0, T, W, S, q, run, a, a, a, 6, win, None)
    assert rq(5000, 2049, 512, 0.08) == -3 and b"at most 2048" in lib.dnmf_last_error()
    assert rq(4, 4, 5, 0.08) == -2 and b"stride=5" in lib.dnmf_last_error()
    assert rq(4, 4, 0, 0.08) == -2
    for q in (-0.1, 1.5, float("nan")):
        assert rq(4, 4, 1, q) == -2 and b"outside [0, 1]" in lib.dnmf_last_error()
    assert rq(4, 4, 1, 0.5, B=4, row0=1) == -2 and b"rows" in lib.dnmf_last_error()
    assert rq(4, 4, 1, 0.5, run=-1) == -2
    assert lib.dnmf_running_quantile(None, 6, None, three, 4, 0, 4, 4, 1, 0.5, 0, a, a, a, 6, win, None) == -1
    assert lib.dnmf_running_windows(10, 2049, 1) == 0 and lib.dnmf_running_windows(10, 4, 5) == 0 and lib.dnmf_running_windows(0, 4, 1) == 0
    # rows that hold no whole window: the range is reported and nothing is launched
    assert rq(100, 8, 2, 0.5, B=4, row0=3) == 0 and (win[0], win[1]) == (2, 2)
    ba = lambda out, mode=2, offset=0.0, ldo=6: lib.dnmf_baseline_apply(a, 6, None, three, 4, 0, a + 2048, 6, a + 3072, 2, mode, offset,
                                                                        out, ldo, None)
    assert ba(a) == -2 and b"aliases" in lib.dnmf_last_error()
    assert ba(a + 4 * 20) == -2 and b"aliases" in lib.dnmf_last_error()          # the last frame row overlaps the first out row
    assert ba(a + 1024, mode=4) == -2 and b"mode=4" in lib.dnmf_last_error()
    assert ba(a + 1024, offset=float("nan")) == -2 and ba(a + 1024, ldo=5) == -2
    assert ba(None) == -1


def test_windows_inside_a_piece(lib):
    """dnmf_running_quantile reports exactly the windows that lie wholly inside the rows given (checked where that is none, so
    nothing is launched), and ``ops._running_pieces`` cuts a movie so that every window is whole in one piece."""
    from dnmf_amd import ops
    for T, W, S, limit in ((300, 64, 16, 100), (301, 65, 33, 65), (70, 64, 64, 64), (5, 8, 2, 3), (1000, 64, 1, 70)):
        plan, pieces = ops._running_pieces(T, 10, W, S, limit)
        assert [p[2] for p in pieces] == [0] + [p[3] for p in pieces[:-1]] and pieces[-1][3] == plan["J"]
        for r0, r1, j0, j1 in pieces:
            assert r0 == plan["starts"][j0] and r1 == plan["ends"][j1 - 1] and (r1 - r0 <= max(limit, min(W, T)))
            inside = [j for j in range(plan["J"]) if plan["starts"][j] >= r0 and plan["ends"][j] <= r1]
            assert inside[0] <= j0 and j1 - 1 <= inside[-1]
        for a, b in zip(pieces[:-1], pieces[1:]):
            # the overlap the plan demands: W - S rows, more only before the last window, which is clamped to end at T
            assert 0 <= a[1] - b[0] <= (W - S if b[2] < plan["J"] - 1 else W - 1)
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    three, win = (ctypes.c_int * 3)(2, 1, 1), (ctypes.c_long * 2)()
    p = DF.window_plan(300, 64, 16)
    for row0, B in ((1, 63), (17, 62), (250, 50), (237, 62)):
        assert lib.dnmf_running_quantile(a, 2, None, three, B, row0, 300, 64, 16, 0.5, 0, a, a, a, 2, win, None) == 0
        inside = [j for j in range(p["J"]) if p["starts"][j] >= row0 and p["ends"][j] <= row0 + B]
        assert not inside and win[0] == win[1]


def test_abi_additions(lib):
    from dnmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "dnmf_hip.h")).read()
    for name in ("dnmf_running_windows", "dnmf_running_quantile", "dnmf_baseline_apply"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert re.search(r"^#define\s+DNMF_ABI_VERSION\s+7\s*$", header, re.M) and _lib.ABI_VERSION == 7 == lib.dnmf_version()
    from dnmf_amd import build, ops
    assert "running_baseline.hip" in build.SOURCES
    assert ops.BASELINE_MODES == {"baseline": 0, "df": 1, "dff": 2, "dfsqrtf": 3} and ops.RUNNING_MAX_WINDOW == 2048 == DF.MAX_WINDOW
    for mode, value in ops.BASELINE_MODES.items():
        assert re.search(rf"^#define\s+DNMF_BASELINE_{'F0' if mode == 'baseline' else mode.upper()}\s+{value}\s*$", header, re.M)
    from Demix.Traces import detrend_df_f
    from dnmf_amd.Demix import Traces
    assert detrend_df_f is Traces.detrend_df_f
