"""Exclusive neuron tracking (K15x) without a GPU: the float64 definition (tests/track_exclusive_restatement.py) on the planted
pairs it was made for, against K15's definition where there is nothing to exclude, its no-result rule and its sensitivity; the
wiring of every layer and the argument checks of the C entry."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import track_exclusive_restatement as TX
import track_restatement as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", range(3))
def test_two_rounds_find_both_neurons_of_a_planted_pair(case):
    """40 x 36 x 1, resting points 3, 4 and 5 voxels apart (1.5 to 2.5 sigma), amplitudes 1.0 and 0.5.  Largest distance from the
    planted centre over the frames, bright / dim neuron, measured:
        rest 3 (frames 4.0 to 4.6 apart)   K15 0.40 / 4.41   one round 0.40 / 0.34   two rounds 0.121 / 0.133   amplitudes 3.9 %
        rest 4 (4.2 to 5.1)                K15 0.39 / 4.99   one round 0.39 / 0.37   two rounds 0.102 / 0.108   amplitudes 3.1 %
        rest 5 (4.3 to 5.8)                K15 0.32 / 4.96   one round 0.32 / 0.27   two rounds 0.070 / 0.072   amplitudes 1.9 %
    K15 gives the dim neuron the bright one's position and amplitude wherever the dim neuron's window reaches the bright peak, and
    the edge of the window next to it where it does not."""
    frames, rest, truth, amps, sigma, search = TX.pair_case(case)
    k15 = TR.track(frames, rest, sigma, search)
    e15 = TX.pair_errors(k15, truth)
    one = TX.pair_errors(TX.track_exclusive(frames, rest, sigma, search, rounds=1), truth)
    out = TX.track_exclusive(frames, rest, sigma, search, rounds=2)
    err = TX.pair_errors(out, truth)
    da = np.abs(out["amplitudes"] / amps[:, None] - 1).max()
    apart = np.linalg.norm(truth[0] - truth[1], axis=0)
    print(f"pair {TX.PAIRS[case]}: frames {apart.min():.2f} to {apart.max():.2f} apart, K15 {e15[0]:.3f} / {e15[1]:.3f}, one round "
          f"{one[0]:.3f} / {one[1]:.3f}, two rounds {err[0]:.3f} / {err[1]:.3f}, amplitude deviation {da:.4f}")
    assert e15[1] > 3.0
    assert err.max() < 0.5
    assert da < 0.1
    np.testing.assert_array_equal(out["n_subtracted"], 1)


def test_pair_on_two_slices_is_better_but_not_good():
    """40 x 36 x 2, the blobs on different slices, resting points 3 apart in the plane, search (4, 4, 1).  Measured: K15
    0.62 / 3.49 voxels off (bright / dim), two rounds 0.444 / 0.955: two slices carry little information about z, and the
    in-plane error of the dim neuron stays near a voxel."""
    frames, rest, truth, amps, sigma, search = TX.pair_case(3)
    e15 = TX.pair_errors(TR.track(frames, rest, sigma, search), truth)
    err = TX.pair_errors(TX.track_exclusive(frames, rest, sigma, search, rounds=2), truth)
    print(f"two slices: K15 {e15[0]:.3f} / {e15[1]:.3f}, two rounds {err[0]:.3f} / {err[1]:.3f}")
    assert err[1] < 0.5 * e15[1] and err.max() < 0.5 * e15.max()


def test_one_neuron_is_k15():
    frames, rest, _, _, sigma, search = TR.moving_case(0)
    for k in range(2):
        ref = TR.track(frames, rest[k:k + 1], sigma, search)
        out = TX.track_exclusive(frames, rest[k:k + 1], sigma, search, rounds=3)
        for name in ("positions", "amplitudes", "peaks", "pstar", "margin"):
            np.testing.assert_array_equal(out[name], ref[name])
        np.testing.assert_array_equal(out["n_subtracted"], 0)


@pytest.mark.parametrize("case", range(len(TR.CASES)))
def test_neurons_five_sigma_apart_are_left_where_k15_finds_them(case):
    frames, rest, _, _, sigma, search = TR.moving_case(case)
    ref = TR.track(frames, rest, sigma, search)
    out = TX.track_exclusive(frames, rest, sigma, search, rounds=2)
    np.testing.assert_array_equal(out["pstar"], ref["pstar"])
    dp = np.abs(out["positions"] - ref["positions"]).max()
    print(f"case {TR.CASES[case]}: exclusive against K15 {dp:.2e} voxel")
    assert dp <= 0.05


def test_a_neuron_without_a_result_is_never_subtracted():
    """A NaN prediction, and a search below the threshold: the neighbour's result is the one with that neuron removed from the
    input, in every round."""
    frames, rest, _, _, sigma, search = TX.pair_case(1)
    alone = TX.track_exclusive(frames, rest[1:], sigma, search, rounds=2)
    pred = np.repeat(rest[:, :, None], frames.shape[0], axis=2)
    pred[0, 1, :] = np.nan
    out = TX.track_exclusive(frames, pred, sigma, search, order=np.zeros((2, 3), dtype=np.int32) + [[0], [1]], rounds=2)
    assert np.isnan(out["positions"][0]).all() and np.isnan(out["amplitudes"][0]).all() and (out["pstar"][0] == -1).all()
    for name in ("positions", "amplitudes", "peaks", "pstar"):
        np.testing.assert_array_equal(out[name][1], alone[name][0])
    np.testing.assert_array_equal(out["n_subtracted"], 0)
    # a window that holds only noise, searched first and below the threshold
    far = np.array([[4.0, 30.0, 0.0], rest[1]])
    out = TX.track_exclusive(frames, far, sigma, search, order=np.zeros((2, 3), dtype=np.int32) + [[0], [1]], rounds=2, threshold=0.05)
    alone = TX.track_exclusive(frames, far[1:], sigma, search, rounds=2, threshold=0.05)
    assert np.isnan(out["positions"][0]).all() and np.isnan(out["peaks"][0]).all()
    for name in ("positions", "amplitudes", "peaks", "pstar"):
        np.testing.assert_array_equal(out[name][1], alone[name][0])
    assert np.isnan(out["margin"][0]).all() and np.isfinite(out["margin"][1]).all()


def test_default_order_is_by_descending_peak_stable_nan_last():
    peaks = np.array([[0.5, np.nan, 1.0], [0.7, 0.2, 1.0], [np.nan, 0.9, 0.3], [0.7, np.nan, 2.0]])
    np.testing.assert_array_equal(TX.default_order(peaks), [[1, 2, 3], [3, 1, 0], [0, 0, 1], [2, 3, 2]])


def test_sensitivity_is_what_the_module_records():
    """SENS from the definition alone: every subtracted neighbour moved by K15's asserted tolerance (1e-3 voxel, 1e-3 relative).
    Measured over the GPU test's cases: positions 6.9e-3 voxel, amplitudes 3.7e-3, peaks 4.8e-3 per round, the crowd of 70 with
    up to 18 neighbours in a region the worst; no pick changes."""
    worst = TX.sensitivity(TX.gpu_cases().values())
    print("sensitivity per round:", {k: f"{v:.2e}" for k, v in worst.items()})
    for name, v in worst.items():
        assert 0.5 * TX.SENS[name] <= v <= TX.SENS[name], name


def test_abi_declares_and_binds_the_entry(lib):
    assert "tests/track_exclusive_restatement.py" in open(os.path.join(ROOT, "include", "dnmf_hip.h")).read()
    from dnmf_amd import _lib, build
    res, args = _lib.SIGNATURES["dnmf_track_neurons_exclusive"]
    assert res is ctypes.c_int and args[1] is ctypes.c_long and args[10] is ctypes.c_int and args[11] is ctypes.c_double
    assert "track_exclusive.hip" in build.SOURCES and hasattr(lib, "dnmf_track_neurons_exclusive")


def test_public_signatures():
    from dnmf_amd import ops
    from dnmf_amd.Demix.dNMF import ExponentialFP
    E = inspect.Parameter.empty
    assert [(p.name, p.default) for p in inspect.signature(ops.track_neurons_exclusive).parameters.values()] == [
        ("frames", E), ("sz", E), ("predict", E), ("order", E), ("shape_std", 3), ("search", (6, 6, 1)), ("rounds", 2), ("threshold", 0.0),
        ("background", None), ("times", None)]
    assert "exclude" in ExponentialFP.track_positions.__doc__
    with pytest.raises(TypeError, match="excluded"):
        ExponentialFP.track_positions(np.zeros((1, 4, 4, 1), dtype=np.float32), np.zeros((1, 3)), excluded=1)


def test_argument_errors_of_the_entry(lib):
    """Validation happens before any HIP call, so it can be exercised without a GPU."""
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    I3 = ctypes.c_int * 3
    names = ["frames", "ldf", "sz", "T", "times", "predict", "predict_f64", "predict_per_frame", "K", "order", "rounds", "sigma", "search",
             "threshold", "background", "positions", "amplitudes", "peaks", "n_subtracted", "stream"]
    ok = (a, 40 * 37 * 2, I3(40, 37, 2), 6, None, a, 1, 0, 5, a, 2, 2.0, I3(4, 4, 1), 0.0, None, a, None, None, None, None)

    def call(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.dnmf_track_neurons_exclusive(*args)

    for name in ("frames", "sz", "predict", "order", "search", "positions"):
        assert call(**{name: None}) == -1 and name.encode() in lib.dnmf_last_error(), name
    for rounds in (0, -1):
        assert call(rounds=rounds) == -2 and b"rounds" in lib.dnmf_last_error()
    assert call(sigma=0.0) == -2 and b"sigma" in lib.dnmf_last_error()
    assert call(K=0) == -2 and b"K=0" in lib.dnmf_last_error()
    assert call(ldf=40 * 37 * 2 - 1) == -2 and b"ldf" in lib.dnmf_last_error()
    assert call(K=1025) == -3 and b"1024" in lib.dnmf_last_error()
    # K15's region over the budget, and a region that fits K15 but not with the list of 1024 neurons beside it
    assert call(sz=I3(64, 64, 4), ldf=64 * 64 * 4, sigma=8.0, search=I3(12, 12, 1)) == -3 and b"LDS" in lib.dnmf_last_error()
    assert call(sz=I3(512, 512, 2), ldf=1 << 19, sigma=3.0, search=I3(6, 6, 1), K=1024) == -3
    assert b"placed list" in lib.dnmf_last_error() and b"LDS" in lib.dnmf_last_error()
