"""Neuron tracking (K15) without a GPU: the ABI and the wiring of every layer, the float64 restatement
(tests/track_restatement.py) against K14's restatement and on moving planted Gaussians, and the argument checks of the C entry."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import detect_restatement as DR
import track_restatement as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def moving():
    """The moving planted cases and their restatement: computed once, never changed."""
    out = []
    for i in range(len(TR.CASES)):
        frames, rest, truth, amps, sigma, search = TR.moving_case(i)
        out.append((frames, rest, truth, amps, sigma, search, TR.track(frames, rest, sigma, search)))
    return out


def test_abi_declares_and_binds_the_entry(lib):
    assert "tests/track_restatement.py" in open(os.path.join(ROOT, "include", "dnmf_hip.h")).read()
    from dnmf_amd import _lib
    res, args = _lib.SIGNATURES["dnmf_track_neurons"]
    assert res is ctypes.c_int and args[1] is ctypes.c_long and args[9] is ctypes.c_double and args[11] is ctypes.c_double
    from dnmf_amd import build
    assert "track_neurons.hip" in build.SOURCES
    assert hasattr(lib, "dnmf_track_neurons")           # exported by the built library


def test_public_signatures():
    from dnmf_amd import ops
    from dnmf_amd.Demix.dNMF import DeformableNMF, ExponentialFP
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.kind is not p.VAR_KEYWORD]

    E = inspect.Parameter.empty
    assert params(ops.track_neurons) == [("frames", E), ("sz", E), ("predict", E), ("shape_std", 3), ("search", (6, 6, 1)),
                                         ("threshold", 0.0), ("background", None), ("times", None)]
    assert isinstance(inspect.getattr_static(ExponentialFP, "track_positions"), staticmethod)
    assert params(ExponentialFP.track_positions) == [("video", E), ("points", E), ("shape_std", 3), ("search", (6, 6, 1)),
                                                     ("predict", None), ("threshold", 0.0), ("background", None)]
    assert params(DeformableNMF.track) == [("self", E), ("frames", E), ("search", (6, 6, 1)), ("predict", None)]
    assert params(MotionCorrect.track_points) == [("self", E), ("video", E), ("points", E), ("search", None), ("shape_std", 3)]
    for fn in (DeformableNMF.track, MotionCorrect.track_points):
        assert any(p.kind is p.VAR_KEYWORD for p in inspect.signature(fn).parameters.values())
    for fn in (ops.track_neurons, ExponentialFP.track_positions, DeformableNMF.track, MotionCorrect.track_points):
        assert "captured" in fn.__doc__                 # the docstrings say what the tracker does not guard against


def test_argument_errors_of_the_track_entry(lib):
    """Validation happens before any HIP call, so it can be exercised on a CPU-only box."""
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    I3 = ctypes.c_int * 3
    names = ["frames", "ldf", "sz", "T", "times", "predict", "predict_f64", "predict_per_frame", "K", "sigma", "search", "threshold",
             "background", "positions", "amplitudes", "peaks", "stream"]
    ok = (a, 40 * 37 * 2, I3(40, 37, 2), 6, None, a, 1, 0, 5, 2.0, I3(4, 4, 1), 0.0, None, a, None, None, None)

    def call(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.dnmf_track_neurons(*args)

    for name in ("frames", "sz", "predict", "search", "positions"):
        assert call(**{name: None}) == -1 and name.encode() in lib.dnmf_last_error(), name
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        assert call(sigma=sigma) == -2 and b"sigma" in lib.dnmf_last_error(), sigma
    assert call(K=0) == -2 and b"K=0" in lib.dnmf_last_error()
    assert call(T=0) == -2 and b"T=0" in lib.dnmf_last_error()
    assert call(sz=I3(40, 0, 2), ldf=1 << 20) == -2 and b"sz" in lib.dnmf_last_error()
    assert call(search=I3(4, -1, 1)) == -2 and b"search" in lib.dnmf_last_error()
    assert call(threshold=float("nan")) == -2 and b"threshold" in lib.dnmf_last_error()
    assert call(threshold=float("inf")) == -2 and b"threshold" in lib.dnmf_last_error()
    assert call(ldf=40 * 37 * 2 - 1) == -2 and b"ldf" in lib.dnmf_last_error()
    assert call(sigma=40.0) == -3 and b"sigma" in lib.dnmf_last_error()
    # a region over the LDS budget: 64 x 64 x 4 voxels = 64 KiB; the message names its size
    assert call(sz=I3(64, 64, 4), ldf=64 * 64 * 4, sigma=8.0, search=I3(12, 12, 1)) == -3
    assert b"64 x 64 x 4" in lib.dnmf_last_error() and b"LDS" in lib.dnmf_last_error()
    assert call(sz=I3(512, 512, 2), ldf=1 << 19, sigma=3.0, search=I3(1 << 30, 1 << 30, 1)) == -3


@pytest.mark.parametrize("case", range(4))
def test_restatement_with_the_whole_volume_as_window_is_the_first_pick_of_k14(case):
    V, _, _, sigma, _ = DR.planted_case(case)
    ref = DR.detect(V, 1, sigma, background=0.25)
    out = TR.track(V[None], np.array([[1.0, 2.0, 0.0]]), sigma, V.shape, background=0.25)
    np.testing.assert_array_equal(out["pstar"][0, :, 0], ref["pstar"][0])
    np.testing.assert_allclose(out["positions"][0, :, 0], ref["positions"][0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(out["amplitudes"][0, 0], ref["amplitudes"][0], rtol=1e-12)
    np.testing.assert_allclose(out["peaks"][0, 0], ref["peaks"][0], rtol=1e-12)
    np.testing.assert_allclose(out["margin"][0, 0], ref["margin"][0], rtol=1e-12)


def test_restatement_is_exact_for_an_isolated_gaussian():
    """Window inside the volume, blob more than r from every border: centre within 2e-4 voxel, as K14's own test."""
    sigma, c = 2.0, np.array([[20.3, 17.6, 0.0]])
    V = DR.plant((41, 36, 1), c, [0.7], sigma).astype(np.float64)
    out = TR.track(V[None], np.array([[19.0, 19.0, 0.0]]), sigma, (3, 3, 0))
    np.testing.assert_allclose(out["positions"][0, :, 0], c[0], atol=2e-4)
    np.testing.assert_allclose(out["amplitudes"][0, 0], 0.7, rtol=1e-3)
    assert out["margin"][0, 0] > 0


@pytest.mark.parametrize("case", range(len(TR.CASES)))
def test_restatement_follows_moving_planted_gaussians(moving, case):
    """Every (k, t) found, in-plane error <= 0.25 voxel, amplitude within 8 %; no pick decided by rounding (what the GPU
    tests rely on)."""
    frames, rest, truth, amps, sigma, search, out = moving[case]
    sz, _, K, T, _, _ = TR.CASES[case]
    d = np.linalg.norm(rest[:, None, :2] - rest[None, :, :2], axis=2) + 1e9 * np.eye(K)
    assert d.min() >= (5.0 + 2.0 * max(search) / sigma) * sigma
    assert (np.abs(truth - rest[:, :, None]) <= np.maximum(np.array(search) - 0.6, 0)[None, :, None] + 1e-12).all()
    assert np.isfinite(out["positions"]).all() and np.isfinite(out["amplitudes"]).all()
    err = np.linalg.norm(out["positions"][:, :2, :] - truth[:, :2, :], axis=1).max()
    da = np.abs(out["amplitudes"] / amps - 1).max()
    print(f"case {TR.CASES[case]}: worst in-plane error {err:.3f} voxel, worst amplitude deviation {da:.4f}, smallest margin "
          f"{out['margin'].min():.3e}")
    assert err <= 0.25
    assert da <= 0.08
    assert out["margin"].min() >= 1e-3


def test_no_result_rules():
    frames, rest, _, _, sigma, search, = TR.moving_case(0)
    X, Y, Z = frames.shape[1:]
    pred = np.repeat(rest[:3, :, None], frames.shape[0], axis=2)
    pred[0, 1, 2] = np.nan                                 # a prediction that is not finite
    pred[1, :, 1] = [X + search[0] + 0.6, 5.0, 0.0]        # rounds to X + search + 1: the window ends one voxel outside
    pred[1, :, 3] = [-search[0] - 0.4, 5.0, 0.0]           # rounds to -search: the window is the first plane
    pred[2, :, 0] = [5.0, 1e30, 0.0]
    out = TR.track(frames, pred, sigma, search)
    bad = np.zeros(pred.shape[::2], dtype=bool)
    bad[0, 2] = bad[1, 1] = bad[2, 0] = True
    np.testing.assert_array_equal(np.isnan(out["positions"]).all(1), bad)
    np.testing.assert_array_equal(np.isnan(out["positions"]).any(1), bad)
    np.testing.assert_array_equal(np.isnan(out["amplitudes"]), bad)
    np.testing.assert_array_equal(np.isnan(out["peaks"]), bad)
    assert out["pstar"][1, 0, 3] == 0
    # a threshold above the peak of one (k, t) only
    thr = 0.5 * (np.sort(out["peaks"][~bad])[-1] + np.sort(out["peaks"][~bad])[-2])
    high = TR.track(frames, pred, sigma, search, threshold=thr)
    assert np.isfinite(high["peaks"]).sum() == 1 and np.nanmax(high["peaks"]) == np.nanmax(out["peaks"])
    # an all-NaN frame gives NaN rows, the other frames are unaffected
    poisoned = frames.copy()
    poisoned[2] = np.nan
    nanf = TR.track(poisoned, pred, sigma, search)
    assert np.isnan(nanf["positions"][:, :, 2]).all() and np.isnan(nanf["peaks"][:, 2]).all()
    keep = [t for t in range(frames.shape[0]) if t != 2]
    np.testing.assert_array_equal(nanf["positions"][:, :, keep], out["positions"][:, :, keep])


def test_constant_frame_picks_the_lowest_index_of_the_window():
    """Well inside a constant frame every score is the same sum of the same products, so the scores of the window are equal:
    p* is the window's lowest voxel index, and a flat neighbourhood is not concave: delta = 0."""
    V = np.full((1, 40, 36, 2), 0.5)
    out = TR.track(V, np.array([[20.0, 18.0, 1.0], [19.5, 16.5, 0.0]]), 1.5, (3, 2, 1))
    np.testing.assert_array_equal(out["pstar"][:, :, 0], [[17, 16, 0], [17, 14, 0]])     # 19.5 -> 20, 16.5 -> 16: half to even
    np.testing.assert_array_equal(out["positions"][:, :, 0], [[17, 16, 0], [17, 14, 0]])
