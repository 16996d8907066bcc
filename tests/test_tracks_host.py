"""Tracks <-> warp and the ROI read-out without a GPU: the numpy restatement (tests/tracks_restatement.py) of K11 / K12 / K13
against independent references -- the fixture G12 captured from the reference's get_roi_signals, numpy.linalg.lstsq on the
stacked least-squares system, scipy.optimize.root -- and the argument checks of the three C entries."""
import ctypes

import numpy as np
import pytest

import tracks_restatement as TR
from conftest import golden


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


def test_roi_restatement_equals_the_reference_fixture():
    """G12: the reference sums the box in float32 (np.nanmean of a float32 tensor), the restatement in float64: N 2^-23
    relative, N the voxels of the box (the video is positive: no cancellation)."""
    g = golden("G12_roi")
    assert g["video"].shape == (20, 16, 2, 5) and g["P"].shape == (6, 3, 5) and not np.isnan(g["video"]).any()
    for i in (0, 1):
        w = g[f"window{i}"]
        n = int(np.prod(2 * w + 1))
        got = TR.roi_signals(g["video"], g["P"], w)
        print(f"window {w.tolist()}: max relative error {np.abs(got / g[f'signals{i}'] - 1).max():.3e}, bound {n * 2.0 ** -23:.3e}")
        np.testing.assert_allclose(got, g[f"signals{i}"], rtol=n * 2.0 ** -23, atol=0)


def test_roi_restatement_rounding_padding_and_nan():
    video = np.arange(4 * 3 * 2 * 1, dtype=np.float64).reshape(4, 3, 2, 1) + 1
    P = np.array([[0.5, 1.5, 0.0], [2.5, 0.49, 1.0], [3.0, 2.0, 1.0], [3.51, 0.0, 0.0], [np.nan, 0.0, 0.0]])[:, :, None]
    out = TR.roi_signals(video, P, (0, 0, 0))[:, 0]
    # half to even: (0.5, 1.5) -> (0, 2), (2.5, 0.49) -> (2, 0); 3.51 -> 4 is outside
    np.testing.assert_array_equal(out[:3], [video[0, 2, 0, 0], video[2, 0, 1, 0], video[3, 2, 1, 0]])
    assert np.isnan(out[3]) and np.isnan(out[4])
    # the corner voxel with window (1, 1, 0): 4 voxels inside, 5 padded zeros in the mean
    got = TR.roi_signals(video, np.array([[[0.0], [0.0], [0.0]]]), (1, 1, 0))[0, 0]
    assert got == video[:2, :2, 0, 0].sum() / 9
    video[1, 1, 0, 0] = np.nan
    assert TR.roi_signals(video, np.array([[[0.0], [0.0], [0.0]]]), (1, 1, 0))[0, 0] == (video[0, 0, 0, 0] + video[0, 1, 0, 0]
                                                                                       + video[1, 0, 0, 0]) / 8


def random_tracks(rng, sz, K, T=1, amp=0.03):
    """Targets inside the volume and tracks that a near-identity quadratic map sends onto them (up to noise)."""
    sz = np.asarray(sz, dtype=np.float64)
    R = rng.rand(K, 3) * (sz - 1)
    P = R[:, :, None] + rng.randn(K, 3, T) * amp * sz[None, :, None]
    P[:, sz == 1] = 0.0
    R[:, sz == 1] = 0.0
    return P, R


@pytest.mark.parametrize("sz", [(40, 30, 1), (40, 30, 2), (512, 512, 2)])
@pytest.mark.parametrize("order", ["translation", "affine", "quadratic"])
@pytest.mark.parametrize("ridge", [0.0, 0.5])
def test_fit_restatement_equals_lstsq_on_the_stacked_system(sz, order, ridge):
    """The normal equations + pivoted elimination of the restatement against numpy.linalg.lstsq (an SVD) on the stacked
    system [Phi; sqrt(ridge) I] D = [R - p; 0] in normalised inputs, compared as warps at the corners of the volume.  The
    normal equations square the condition number (about 1e2 for a quadratic basis on scattered points in [-1, 1]^3): 1e-9
    voxel at S = 512 leaves four digits of room."""
    rng = np.random.RandomState(4)
    P, R = random_tracks(rng, sz, 24)
    P[3] = np.nan
    beta, ok = TR.fit_frame(P[:, :, 0], R, sz, order, ridge)
    assert ok
    Phi, E, rows = TR.fit_system(P[:, :, 0], R, sz, order)
    assert Phi.shape[0] == 23
    n = len(rows)
    D = np.linalg.lstsq(np.concatenate((Phi, np.sqrt(ridge) * np.eye(n))), np.concatenate((E, np.zeros((n, 3)))), rcond=None)[0]
    Bp = TR.identity_normalised(sz)
    Bp[rows] += D
    ref = TR.change_of_basis(sz).T @ Bp
    corners = np.array([[x, y, z] for x in (0, sz[0] - 1) for y in (0, sz[1] - 1) for z in (0, sz[2] - 1)], dtype=np.float64)
    # beta is rounded to fp32: 10 products of size <= S
    bound = 10 * 2.0 ** -24 * max(sz) + 1e-9
    assert np.abs(TR.warp(beta, corners) - TR.warp(ref, corners))[:, np.asarray(sz) > 1].max() < bound
    free = set(rows)
    for i in range(10):
        if i not in free and order != "translation":
            np.testing.assert_array_equal(beta[i], TR.IDENTITY[i].astype(np.float32))
    if sz[2] == 1:
        np.testing.assert_array_equal(beta[:, 2], TR.IDENTITY[:, 2].astype(np.float32))
        np.testing.assert_array_equal(beta[[3, 6, 8, 9]], TR.IDENTITY[[3, 6, 8, 9]].astype(np.float32))


def test_fit_restatement_singular_frames():
    sz = (40, 30, 1)
    R = np.array([[5.0, 5.0, 0.0], [10.0, 10.0, 0.0], [20.0, 20.0, 0.0]])
    beta, ok = TR.fit_frame(R + [1.0, 0.0, 0.0], R, sz, "affine", 0.0)          # three collinear points
    assert not ok
    np.testing.assert_array_equal(beta, TR.IDENTITY.astype(np.float32))
    beta, ok = TR.fit_frame(R + [1.0, 0.0, 0.0], R, sz, "affine", 1e-3)         # the ridge makes it regular
    assert ok and abs(TR.warp(beta, R + [1.0, 0.0, 0.0]) - R).max() < 0.05
    beta, ok = TR.fit_frame(R + [1.0, 0.0, 0.0], R, sz, "translation", 0.0)
    assert ok
    np.testing.assert_allclose(beta[0], [-1.0, 0.0, 0.0], atol=1e-6)
    assert not TR.fit_frame(R[:2], R[:2], sz, "affine", 0.0)[1]                 # fewer points than free rows


def test_inverse_restatement_equals_scipy_root():
    from scipy.optimize import root
    rng = np.random.RandomState(9)
    sz = np.array([64.0, 48.0, 4.0])
    for _ in range(20):
        b = TR.IDENTITY + rng.randn(10, 3) * np.array([1.0, 2e-2, 2e-2, 2e-2, 2e-4, 2e-4, 2e-4, 2e-4, 2e-4, 2e-4])[:, None]
        r = rng.rand(3) * (sz - 1)
        x = TR.invert_point(b, r, tol=1e-9)
        sol = root(lambda v: TR.warp(b, v) - r, r, jac=lambda v: TR.jacobian(b, v), tol=1e-13)
        assert sol.success
        np.testing.assert_allclose(x, sol.x, rtol=0, atol=1e-8)
        np.testing.assert_allclose(TR.warp(b, x), r, rtol=0, atol=1e-8)
    np.testing.assert_array_equal(TR.invert_point(TR.IDENTITY, r), r)
    flat = TR.IDENTITY.copy()
    flat[1, 0] = 0.0                                                            # q_x does not depend on x: det J = 0
    assert np.isnan(TR.invert_point(flat, r)).all()


def test_jacobian_of_the_restatement_is_the_true_one():
    rng = np.random.RandomState(2)
    b, x = rng.randn(10, 3), rng.randn(3)
    num = np.stack([(TR.warp(b, x + 1e-6 * e) - TR.warp(b, x - 1e-6 * e)) / 2e-6 for e in np.eye(3)], 1)
    np.testing.assert_allclose(TR.jacobian(b, x), num, atol=1e-8)


def test_round_trip_of_the_restatement():
    """positions(beta_from_positions(P)) equals P within the fit's own residual: tracks made by a quadratic map are
    recovered to the rounding of the fp32 coefficients."""
    rng = np.random.RandomState(5)
    sz = (64, 48, 2)
    b = (TR.IDENTITY + rng.randn(10, 3) * np.array([1.0, 1e-2, 1e-2, 1e-2, 1e-4, 1e-4, 1e-4, 1e-4, 1e-4, 1e-4])[:, None])
    R = rng.rand(16, 3) * (np.array(sz) - 1)
    P = TR.invert_quadratic_warp(b[:, :, None], R, tol=1e-10)
    beta, ok = TR.fit_quadratic_warp(P, R, sz)
    assert ok.all()
    back = TR.invert_quadratic_warp(beta, R, tol=1e-10)
    assert np.abs(back - P).max() < 100 * 2.0 ** -24 * 64


def test_argument_errors_of_the_track_entries(lib):
    """Validation happens before any HIP call, so it can be exercised on a CPU-only box."""
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    I3 = ctypes.c_int * 3
    fit, inv, roi = lib.dnmf_fit_quadratic_warp, lib.dnmf_invert_quadratic_warp, lib.dnmf_roi_signals
    assert fit(None, 0, 4, 2, a, 8, 8, 2, 2, 0.0, a, a, None) == -1 and b"NULL" in lib.dnmf_last_error()
    assert fit(a, 0, 4, 2, a, 8, 8, 2, 2, 0.0, a, None, None) == -1
    assert fit(a, 0, 0, 2, a, 8, 8, 2, 2, 0.0, a, a, None) == -2                 # K = 0
    assert fit(a, 0, 4, 2, a, 8, 0, 2, 2, 0.0, a, a, None) == -2
    assert fit(a, 0, 4, 2, a, 8, 8, 2, 2, -1.0, a, a, None) == -2 and b"ridge" in lib.dnmf_last_error()
    assert fit(a, 0, 4, 2, a, 8, 8, 2, 3, 0.0, a, a, None) == -3 and b"order" in lib.dnmf_last_error()
    assert fit(a, 1, 4, 2, a, 8, 8, 2, -1, 0.0, a, a, None) == -3
    assert inv(None, 2, None, 2, a, 4, None, 1e-6, a, None) == -1
    assert inv(a, 2, None, 2, a, 4, None, 1e-6, None, None) == -1
    assert inv(a, 2, None, 2, a, 0, None, 1e-6, a, None) == -2                   # K = 0
    assert inv(a, 2, None, 3, a, 4, None, 1e-6, a, None) == -2                   # more frames than beta has, no times
    assert inv(a, 2, None, 2, a, 4, None, 0.0, a, None) == -2 and b"tol" in lib.dnmf_last_error()
    assert inv(a, 2, None, 0, a, 4, None, 1e-6, a, None) == 0                    # nothing to do
    assert roi(None, 128, 8, 8, 2, a, 0, 4, 2, I3(3, 3, 0), a, None) == -1
    assert roi(a, 128, 8, 8, 2, a, 0, 4, 2, None, a, None) == -1
    assert roi(a, 128, 8, 8, 2, a, 0, 0, 2, I3(3, 3, 0), a, None) == -2          # K = 0
    assert roi(a, 127, 8, 8, 2, a, 0, 4, 2, I3(3, 3, 0), a, None) == -2          # a row shorter than a frame
    assert roi(a, 128, 8, 8, 2, a, 0, 4, 2, I3(3, -1, 0), a, None) == -2
    assert roi(a, 128, 8, 8, 2, a, 0, 4, 2, I3(8, 7, 8), a, None) == -3 and b"4096" in lib.dnmf_last_error()   # 17 * 15 * 17
    assert roi(a, 128, 8, 8, 2, a, 0, 4, 2, I3(1 << 30, 1 << 30, 1 << 30), a, None) == -3
