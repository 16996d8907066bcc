"""Neuron detection (K14) without a GPU: the ABI and the wiring of every layer, the float64 restatement
(tests/detect_restatement.py) on planted Gaussians, and the argument checks of the two C entries."""
import ctypes
import inspect

import numpy as np
import pytest

import detect_restatement as DR


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def planted():
    """The four planted cases with EXTRA picks asked for beyond the planted ones: computed once, never changed."""
    out = []
    for i in range(4):
        V, centres, amps, sigma, K = DR.planted_case(i)
        out.append((V, centres, amps, sigma, K, DR.detect(V, K + DR.EXTRA, sigma)))
    return out


def test_abi_declares_and_binds_the_two_entries():
    from dnmf_amd import _lib
    assert _lib.SIGNATURES["dnmf_detect_neurons_workspace"][0] is ctypes.c_size_t
    res, args = _lib.SIGNATURES["dnmf_detect_neurons"]
    assert res is ctypes.c_int and args[3:7] == [ctypes.c_double] * 4
    from dnmf_amd import build
    assert "detect_neurons.hip" in build.SOURCES


def test_public_signatures():
    from dnmf_amd import ops
    from dnmf_amd.Demix.dNMF import DeformableNMF, ExponentialFP
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.kind is not p.VAR_KEYWORD]

    E = inspect.Parameter.empty
    assert params(ops.detect_neurons) == [("image", E), ("sz", E), ("K", E), ("shape_std", 3), ("min_distance", None),
                                          ("threshold", 0.0), ("background", None), ("workspace", None)]
    assert isinstance(inspect.getattr_static(ExponentialFP, "detect_positions"), staticmethod)
    assert params(ExponentialFP.detect_positions) == [("image", E), ("K", E), ("shape_std", 3)]
    assert isinstance(inspect.getattr_static(DeformableNMF, "from_image"), classmethod)
    assert params(DeformableNMF.from_image) == [("image", E), ("K", E), ("T", E), ("shape_std", 3)]
    assert params(MotionCorrect.detect_points) == [("self", E), ("K", E), ("shape_std", 3)]
    for fn in (ExponentialFP.detect_positions, DeformableNMF.from_image, MotionCorrect.detect_points):
        assert any(p.kind is p.VAR_KEYWORD for p in inspect.signature(fn).parameters.values())


def test_filter_of_the_restatement_is_the_plain_triple_sum():
    """The band-matrix product against the definition written as loops, on a volume with an axis shorter than the window."""
    rng = np.random.RandomState(3)
    V, sigma, bg = rng.rand(7, 5, 2), 1.5, 0.25
    r = DR.radius(sigma)
    assert r == 5
    ref = np.zeros(V.shape)
    for x in range(7):
        for y in range(5):
            for z in range(2):
                for a in range(7):
                    for b in range(5):
                        for c in range(2):
                            if max(abs(x - a), abs(y - b), abs(z - c)) <= r:
                                ref[x, y, z] += np.exp(-((x - a) ** 2 + (y - b) ** 2 + (z - c) ** 2) / sigma ** 2) * (V[a, b, c] - bg)
    np.testing.assert_allclose(DR.matched_filter(V, sigma, bg), ref, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("case", range(4))
def test_restatement_recovers_planted_gaussians(planted, case):
    """Every planted centre has a pick within 1.2 voxels in the plane (the issue's cap; the worst of these cases is 0.09);
    every pick beyond the K-th is below 5 % of the dimmest planted amplitude."""
    V, centres, amps, sigma, K, out = planted[case]
    d = np.linalg.norm(centres[:, None, :2] - centres[None, :, :2], axis=2) + 1e9 * np.eye(K)
    assert d.min() >= 3.2 * sigma
    assert out["count"] >= K
    got = out["positions"][:K]
    dist = np.linalg.norm(got[None, :, :2] - centres[:, None, :2], axis=2)
    print(f"case {DR.CASES[case]}: worst in-plane error {dist.min(1).max():.3f}, count {out['count']}, largest pick beyond K "
          f"{np.nanmax(np.r_[out['amplitudes'][K:], 0.0]) / amps[-1]:.4f} of the dimmest, smallest margin {np.nanmin(out['margin'][:K]):.2e}")
    assert dist.min(1).max() <= 1.2
    assert sorted(dist.argmin(1)) == list(range(K))           # one pick each
    beyond = out["amplitudes"][K:out["count"]]
    assert (np.abs(beyond) < 0.05 * amps[-1]).all()
    # what the GPU tests rely on: no pick of the planted blobs is decided by rounding
    assert np.nanmin(out["margin"][:K]) >= 1e-3
    assert np.isnan(out["positions"][out["count"]:]).all() and np.isnan(out["amplitudes"][out["count"]:]).all()


def test_restatement_stops_early(planted):
    V, _, _, sigma, K, out = planted[0]
    stop = DR.detect(V, K, sigma, threshold=2.0 * np.nanmax(out["peaks"]))
    assert stop["count"] == 0 and np.isnan(stop["positions"]).all() and np.isnan(stop["amplitudes"]).all()
    # between the second and the third peak: two picks
    two = DR.detect(V, K, sigma, threshold=0.5 * (out["peaks"][1] + out["peaks"][2]))
    assert two["count"] == 2
    np.testing.assert_array_equal(two["positions"][:2], out["positions"][:2])
    # scores that are not finite stop it too
    bad = V.astype(np.float64).copy()
    bad[:] = np.inf
    assert DR.detect(bad, 3, sigma, background=0.0)["count"] == 0


@pytest.mark.parametrize("case", range(4))
def test_restatement_keeps_centres_apart(planted, case):
    """No two returned centres within min_distance, the noise-level picks beyond K included (they crowd around the
    exclusion balls of the real ones)."""
    V, _, _, sigma, K, out = planted[case]
    P = out["positions"][:out["count"]]
    d = np.linalg.norm(P[:, None] - P[None], axis=2) + 1e9 * np.eye(len(P))
    assert d.min() > 2.0 * sigma
    wide = DR.detect(V, K + DR.EXTRA, sigma, min_distance=4.5 * sigma)
    P = wide["positions"][:wide["count"]]
    d = np.linalg.norm(P[:, None] - P[None], axis=2) + 1e9 * np.eye(len(P))
    assert wide["count"] >= 1 and d.min() > 4.5 * sigma


def test_restatement_is_exact_for_an_isolated_gaussian():
    """The log-parabola is exact for a blob whose window is inside the volume: centre to 1e-6 voxel (the truncated tails of
    the filter, e^-9 each), amplitude to 1e-4."""
    sigma, c = 2.0, np.array([[20.3, 17.6, 0.0]])
    out = DR.detect(DR.plant((41, 36, 1), c, [0.7], sigma).astype(np.float64), 1, sigma, background=0.0)
    assert out["count"] == 1
    np.testing.assert_allclose(out["positions"][0], c[0], atol=2e-4)
    np.testing.assert_allclose(out["amplitudes"][0], 0.7, rtol=1e-3)


def test_argument_errors_of_the_detect_entries(lib):
    """Validation happens before any HIP call, so it can be exercised on a CPU-only box."""
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    I3 = ctypes.c_int * 3
    ws, det = lib.dnmf_detect_neurons_workspace, lib.dnmf_detect_neurons
    sz = I3(37, 29, 2)
    need = ws(sz, 6, 2.0)
    P, tiles = 37 * 29 * 2, 3 * 2 * 1
    assert need == 2 * ((4 * P + 255) // 256 * 256) + 2 * 256 and tiles * 4 <= 256
    assert ws(sz, 6, 0.0) == 0 and b"sigma" in lib.dnmf_last_error()
    assert ws(sz, 0, 2.0) == 0 and b"K=0" in lib.dnmf_last_error()
    assert ws(I3(37, 0, 2), 6, 2.0) == 0
    assert ws(None, 6, 2.0) == 0
    ok = (a, sz, 6, 2.0, 4.0, 0.0, 0.0, a, a, a, a, need, None)

    def call(**kw):
        names = ["img", "sz", "K", "sigma", "min_distance", "threshold", "background", "positions", "amplitudes", "count", "workspace",
                 "bytes", "stream"]
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return det(*args)

    for name in ("img", "positions", "amplitudes", "count", "workspace", "sz"):
        assert call(**{name: None}) == -1, name
    assert call(sigma=0.0) == -2 and b"sigma" in lib.dnmf_last_error()
    assert call(sigma=-1.0) == -2
    assert call(sigma=float("nan")) == -2
    assert call(sigma=40.0) == -3 and b"sigma" in lib.dnmf_last_error()
    assert call(K=0) == -2 and b"K=0" in lib.dnmf_last_error()
    assert call(min_distance=-1.0) == -2 and b"min_distance" in lib.dnmf_last_error()
    assert call(min_distance=1e6) == -3
    assert call(background=float("nan")) == -2 and b"background" in lib.dnmf_last_error()
    assert call(background=float("inf")) == -2
    assert call(threshold=float("nan")) == -2 and b"threshold" in lib.dnmf_last_error()
    assert call(bytes=need - 1) == -4 and b"workspace" in lib.dnmf_last_error() and str(need).encode() in lib.dnmf_last_error()
    assert call(sz=I3(1 << 12, 1 << 12, 1 << 7)) == -3
