"""Chained neuron tracking (K15c) without a GPU: the float64 definition (tests/follow_restatement.py) on drifting planted
Gaussians -- where K15 around the start position fails and the chain does not -- its gap and loss rules, and the wiring and
argument checks of every layer."""
import ctypes
import inspect

import numpy as np
import pytest

import detect_restatement as DR
import follow_restatement as FR
import track_restatement as TR


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def videos():
    """The three drifting videos, the start (the rounded truth at the anchor) and the chained run: computed once, never changed."""
    out = []
    for i in range(3):
        sz, T, v, search, anchor, momentum, _, threshold, max_gap = FR.CASES[i]
        frames, truth, amps = FR.drifting_case(i)
        start = np.rint(truth[:, :, anchor])
        run = FR.follow(frames, start, FR.SIGMA, search, anchor=anchor, momentum=momentum, max_gap=max_gap, threshold=threshold)
        out.append((frames, truth, start, run))
    return out


def worst(positions, truth):
    """Largest distance of a coordinate from the truth; a NaN row counts as +inf."""
    err = np.abs(positions - truth)
    return float(np.where(np.isnan(err), np.inf, err).max())


@pytest.mark.parametrize("case", range(3))
def test_chain_follows_where_the_search_around_the_start_fails(videos, case):
    """Thresholds from float64 runs of these recipes: chained 0.004, 0.007 and 0.112 voxel; K15 around the start position 17.8,
    3.75 and 21.9; the third video at momentum 0: 4.87."""
    sz, T, v, search, anchor, momentum, _, _, _ = FR.CASES[case]
    frames, truth, start, run = videos[case]
    chained = worst(run["positions"], truth)
    alone = TR.track(frames, start, FR.SIGMA, search)
    unchained = worst(alone["positions"], truth)
    within = (np.nan_to_num(np.abs(alone["positions"] - truth).max(1), nan=np.inf) <= 0.5).sum()
    print(f"case {FR.CASES[case]}: chained worst {chained:.3f} voxel; unchained {within} of {truth.shape[0] * T} rows within 0.5, worst "
          f"{unchained:.2f}")
    assert chained <= 0.5
    assert unchained > 3.0
    assert (run["lost_at"] == -1).all() and np.isfinite(run["predicted"]).all()
    if case == 2:
        still = FR.follow(frames, start, FR.SIGMA, search, anchor=anchor, momentum=0.0)
        print(f"    momentum 0: worst {worst(still['positions'], truth):.2f}")
        assert worst(still["positions"], truth) > 3.0


def test_recurrence_alone_reproduces_the_run(videos):
    for case, (frames, truth, start, run) in enumerate(videos):
        _, _, _, _, anchor, momentum, _, _, max_gap = FR.CASES[case]
        predicted, lost_at = FR.predicted_from(run["positions"], start, anchor, momentum, max_gap)
        np.testing.assert_array_equal(predicted, run["predicted"])
        np.testing.assert_array_equal(lost_at, run["lost_at"])


def test_gap_is_coasted_and_a_longer_one_loses_the_chain():
    """Neuron 1 dark in frames 4 and 5 of the first video.  The threshold lies halfway between the largest score of the noise
    alone and the weakest peak of a planted blob, which are measured here and lie a factor 10 apart at the least."""
    sz, T, v, search, anchor, _, _, _, _ = FR.CASES[0]
    frames, truth, amps = FR.drifting_case(0)
    start = np.rint(truth[:, :, anchor])
    noise = max(float(TR.frame_score(DR.plant(sz, truth[:, :, t], 0.0 * amps[:, t], FR.SIGMA, noise=FR.NOISE, seed=7000 + t), FR.SIGMA,
                                     0.0).max()) for t in range(T))
    weakest = float(FR.follow(frames, start, FR.SIGMA, search, anchor=anchor, momentum=1.0)["peaks"].min())
    print(f"largest noise-only score {noise:.4f}, weakest planted peak {weakest:.4f}")
    assert weakest >= 10.0 * noise
    threshold = 0.5 * (noise + weakest)
    dark, _, _ = FR.drifting_case(0, blank=(1, (4, 5)))
    coast = FR.follow(dark, start, FR.SIGMA, search, anchor=anchor, momentum=1.0, max_gap=2, threshold=threshold)
    found = np.isfinite(coast["positions"]).all(1)
    expect = np.ones((4, T), dtype=bool)
    expect[1, 4:6] = False
    np.testing.assert_array_equal(found, expect)
    assert (coast["lost_at"] == -1).all() and np.isfinite(coast["predicted"]).all()
    assert worst(coast["positions"][:, :, 6:], truth[:, :, 6:]) <= 0.5
    # the coasting prediction carries the last step on: frame 6 is searched three steps from frame 3
    step = coast["positions"][1, :, 3] - coast["positions"][1, :, 2]
    np.testing.assert_array_equal(coast["predicted"][1, :, 6], coast["positions"][1, :, 3] + (np.float64(1.0) * step) * 3.0)
    lose = FR.follow(dark, start, FR.SIGMA, search, anchor=anchor, momentum=1.0, max_gap=1, threshold=threshold)
    np.testing.assert_array_equal(lose["lost_at"], [[-1, -1], [5, -1], [-1, -1], [-1, -1]])
    assert np.isnan(lose["positions"][1, :, 4:]).all() and np.isnan(lose["predicted"][1, :, 6:]).all()
    assert np.isfinite(lose["predicted"][1, :, :6]).all() and np.isnan(lose["amplitudes"][1, 4:]).all()
    others = [0, 2, 3]
    np.testing.assert_array_equal(lose["positions"][others], coast["positions"][others])


@pytest.mark.parametrize("anchor", ["first", "last"])
def test_anchor_at_an_end_leaves_the_unused_direction_alone(videos, anchor):
    frames, truth, _, _ = videos[1]
    T = frames.shape[0]
    a = 0 if anchor == "first" else T - 1
    run = FR.follow(frames, np.rint(truth[:, :, a]), FR.SIGMA, FR.CASES[1][3], anchor=a)
    assert (run["lost_at"] == -1).all()
    assert np.isfinite(run["positions"]).all() and np.isfinite(run["predicted"]).all() and np.isfinite(run["amplitudes"]).all()
    assert worst(run["positions"], truth) <= 0.5
    np.testing.assert_array_equal(run["predicted"][:, :, a], np.rint(truth[:, :, a]))
    # every frame once: the frame next to the anchor is searched around what the anchor frame gave
    nxt = 1 if a == 0 else T - 2
    np.testing.assert_array_equal(run["predicted"][:, :, nxt], run["positions"][:, :, a])


def test_start_that_is_not_finite_and_half():
    frames, truth, _ = FR.drifting_case(1)
    start = np.rint(truth[:, :, 4])
    start[2, 1] = np.nan
    out = FR.follow(frames, start, FR.SIGMA, FR.CASES[1][3], anchor=4)
    np.testing.assert_array_equal(out["lost_at"], [[-1, -1], [-1, -1], [4, 4], [-1, -1]])
    assert np.isnan(out["positions"][2]).all() and np.isnan(out["predicted"][2]).all() and np.isnan(out["half"][2]).all()
    assert np.isfinite(out["positions"][[0, 1, 3]]).all()
    # half: the distance from a half-integer on the axes that are searched (x and y here)
    P = out["predicted"][0, :, 7]
    assert out["half"][0, 7] == min(abs(P[0] - np.floor(P[0]) - 0.5), abs(P[1] - np.floor(P[1]) - 0.5))
    assert 0.0 <= np.nanmin(out["half"]) and np.nanmax(out["half"]) <= 0.5


def test_abi_declares_and_binds_the_entry(lib):
    from dnmf_amd import _lib, build
    res, args = _lib.SIGNATURES["dnmf_follow_neurons"]
    assert res is ctypes.c_int and len(args) == 20 and args[1] is ctypes.c_long and args[7] is ctypes.c_double and args[10] is ctypes.c_double
    assert "follow_neurons.hip" in build.SOURCES and hasattr(lib, "dnmf_follow_neurons")


def test_public_signatures():
    from dnmf_amd import ops
    from dnmf_amd.Demix.dNMF import DeformableNMF, ExponentialFP

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.kind is not p.VAR_KEYWORD]

    E = inspect.Parameter.empty
    assert params(ops.follow_neurons) == [("frames", E), ("sz", E), ("start", E), ("shape_std", 3), ("search", (3, 3, 1)), ("anchor", 0),
                                          ("momentum", 0.0), ("max_gap", 5), ("threshold", 0.0), ("background", None), ("times", None)]
    assert isinstance(inspect.getattr_static(ExponentialFP, "follow_positions"), staticmethod)
    assert params(ExponentialFP.follow_positions) == [("video", E), ("points", E), ("shape_std", 3), ("search", (3, 3, 1)), ("anchor", 0),
                                                      ("momentum", 0.0), ("max_gap", 5), ("threshold", 0.0), ("background", None)]
    assert params(DeformableNMF.follow) == [("self", E), ("frames", E), ("anchor", 0), ("start", None), ("search", (3, 3, 1))]
    for fn in (ops.follow_neurons, ExponentialFP.follow_positions, DeformableNMF.follow):
        assert "captured" in fn.__doc__                 # still no exclusion between neurons


def test_argument_errors_of_the_follow_entry(lib):
    """Validation happens before any HIP call, so it can be exercised on a CPU-only box."""
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    I3 = ctypes.c_int * 3
    names = ["frames", "ldf", "sz", "T", "times", "start", "K", "sigma", "search", "anchor", "momentum", "max_gap", "threshold",
             "background", "positions", "amplitudes", "peaks", "predicted", "lost_at", "stream"]
    ok = (a, 40 * 37 * 2, I3(40, 37, 2), 6, None, a, 5, 2.0, I3(3, 3, 1), 0, 0.0, 5, 0.0, None, a, None, None, a, a, None)

    def call(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.dnmf_follow_neurons(*args)

    for name in ("frames", "sz", "start", "search", "positions", "predicted", "lost_at"):
        assert call(**{name: None}) == -1 and name.encode() in lib.dnmf_last_error(), name
    for anchor in (-1, 6, 1 << 30):
        assert call(anchor=anchor) == -2 and b"anchor" in lib.dnmf_last_error(), anchor
    for momentum in (-0.25, 1.5, float("nan"), float("inf"), float("-inf")):
        assert call(momentum=momentum) == -2 and b"momentum" in lib.dnmf_last_error(), momentum
    assert call(max_gap=-1) == -2 and b"max_gap" in lib.dnmf_last_error()
    # K15's own checks come with the shared geometry
    assert call(sigma=0.0) == -2 and b"sigma" in lib.dnmf_last_error()
    assert call(search=I3(4, -1, 1)) == -2 and b"search" in lib.dnmf_last_error()
    assert call(ldf=40 * 37 * 2 - 1) == -2 and b"ldf" in lib.dnmf_last_error()
    assert call(sz=I3(64, 64, 4), ldf=64 * 64 * 4, sigma=8.0, search=I3(12, 12, 1)) == -3
    assert b"64 x 64 x 4" in lib.dnmf_last_error() and b"LDS" in lib.dnmf_last_error()
