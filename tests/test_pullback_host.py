"""K17 (dnmf_warp_pullback, the trilinear registered movie) without a GPU: the float64 restatement (tests/pullback_restatement.py)
on the cases with a known answer, and the wiring of every layer."""
import ctypes
import inspect

import numpy as np
import pytest

import pullback_restatement as PB
from tracks_restatement import IDENTITY, warp


def shifted(frame, k, fill=0.0):
    """out(u) = frame(u - k) for an integer k per axis, ``fill`` where u - k is outside."""
    out = np.full(frame.shape, fill, dtype=np.float64)
    src = tuple(slice(max(-k[d], 0), frame.shape[d] - max(k[d], 0)) for d in range(3))
    dst = tuple(slice(max(k[d], 0), frame.shape[d] - max(-k[d], 0)) for d in range(3))
    out[dst] = frame[src]
    return out


def bent_beta(sz, seed):
    """A warp off the identity by about a voxel with affine and quadratic terms, invertible on the volume."""
    rng = np.random.default_rng(seed)
    ext = np.array([max(s - 1, 1) for s in sz], dtype=np.float64)
    b = IDENTITY.copy()
    b[0] += rng.uniform(-1.5, 1.5, 3)
    b[1:4] += rng.uniform(-0.1, 0.1, (3, 3)) * np.minimum(1.0, ext[None, :] / ext[:, None])
    b[4:] += rng.uniform(-0.5, 0.5, (6, 3)) / ext.max() ** 2
    return b


@pytest.mark.parametrize("sz", [(7, 6, 3), (9, 8, 1)])
def test_identity_returns_the_frame(sz):
    frame = np.random.default_rng(0).uniform(0, 1, sz)
    for fill in (None, np.nan):
        out, x, bad = PB.pullback_frame(frame, IDENTITY, fill=fill)
        assert not bad.any() and np.array_equal(x, PB.lattice(sz)) and np.array_equal(out, frame)


@pytest.mark.parametrize("sz,k", [((7, 6, 3), (2, -1, 1)), ((9, 8, 1), (-3, 2, 0))])
def test_integer_shift_returns_the_shifted_frame(sz, k):
    frame = np.random.default_rng(1).uniform(0.5, 1, sz)
    b = IDENTITY.copy()
    b[0] = k                                    # q(x) = x + k: out(u) = frame(u - k)
    out, _, bad = PB.pullback_frame(frame, b)
    assert not bad.any() and np.array_equal(out, shifted(frame, k))
    out, _, _ = PB.pullback_frame(frame, b, fill=np.nan)
    assert np.array_equal(out, shifted(frame, k, np.nan), equal_nan=True)
    out, _, _ = PB.pullback_frame(frame, b, fill=-7.0)
    assert np.array_equal(out, shifted(frame, k, -7.0))


@pytest.mark.parametrize("sz", [(9, 7, 3), (12, 10, 1)])
def test_coords_invert_the_warp(sz):
    b = bent_beta(sz, 2)
    x, bad = PB.invert(b, sz)
    assert not bad.any()
    act = PB.active_axes(sz)
    assert np.abs(warp(b, x) - PB.lattice(sz))[:, act].max() <= 1e-9
    assert all((x[:, d] == 0).all() for d in range(3) if d not in act)


def test_z1_equals_the_duplicated_slice_form():
    """The G10 idea: a volume of one slice is the Z = 2 volume of two equal slices under a warp that leaves z alone."""
    sz1, sz2 = (12, 10, 1), (12, 10, 2)
    b = bent_beta(sz1, 3)
    b[[3, 6, 8, 9]] = IDENTITY[[3, 6, 8, 9]]      # no z in any term
    b[:, 2] = IDENTITY[:, 2]                      # and z maps to itself
    frame = np.random.default_rng(3).uniform(0, 1, sz1)
    for fill in (None, np.nan):
        o1, x1, bad1 = PB.pullback_frame(frame, b, fill=fill)
        o2, x2, bad2 = PB.pullback_frame(np.repeat(frame, 2, 2), b, fill=fill)
        assert not bad1.any() and not bad2.any()
        for z in (0, 1):
            np.testing.assert_allclose(o2[:, :, z], o1[:, :, 0], rtol=0, atol=1e-12, equal_nan=True)
        np.testing.assert_allclose(x2.reshape(12, 10, 2, 3)[:, :, 0, :2], x1.reshape(12, 10, 3)[:, :, :2], rtol=0, atol=1e-12)


def test_a_folded_warp_reports_bad_points():
    sz = (16, 6, 1)
    b = IDENTITY.copy()
    b[4, 0] = -0.08                               # q_x = x - 0.08 x^2: dq/dx < 0 beyond x = 6.25, nothing maps above 3.125
    assert (np.linalg.det(PB.jacobians(b, PB.lattice(sz))[:, :2, :2]) < 0).any()
    frame = np.random.default_rng(4).uniform(0, 1, sz)
    out, x, bad = PB.pullback_frame(frame, b)
    assert 0 < bad.sum() < bad.size and np.isfinite(out).all() and (out.reshape(-1)[bad] == 0).all()
    assert np.isnan(x[bad]).all() and np.isfinite(x[~bad]).all()
    out, _, _ = PB.pullback_frame(frame, b, fill=np.nan)
    assert np.isnan(out.reshape(-1)[bad]).all()
    _, _, n = PB.pullback(frame[None], b[:, :, None])
    assert n == bad.sum()


def test_nan_voxels_propagate():
    frame = np.ones((5, 4, 1))
    frame[2, 1, 0] = np.nan
    b = IDENTITY.copy()
    b[0, 0] = 0.5
    out, _, _ = PB.pullback_frame(frame, b)
    assert np.isnan(out[2:4, 1, 0]).all() and np.isfinite(out[:, 3, 0]).all()


# ---- wiring ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


def test_symbol_is_declared_built_and_exported(lib):
    from dnmf_amd import _lib, build
    assert "warp_pullback.hip" in build.SOURCES
    assert "dnmf_warp_pullback" in _lib.SIGNATURES and hasattr(lib, "dnmf_warp_pullback")


def test_argument_errors_without_a_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)

    def call(frames=a, ldf=8, ldc_in=8, nchan=1, X=2, Y=2, Z=2, beta=a, T=1, times=None, B=1, out=a, ldo=8, ldc_out=8, mode=0):
        return lib.dnmf_warp_pullback(frames, ldf, ldc_in, nchan, None, X, Y, Z, beta, T, times, B, out, ldo, ldc_out, mode, 0.0,
                                      None, None, None)
    assert call(frames=None) == -1 and lib.dnmf_last_error().decode().startswith("dnmf_warp_pullback:")
    assert call(beta=None) == -1 and call(out=None) == -1
    assert call(nchan=0) == -2 and call(nchan=-1) == -2
    assert call(B=-1) == -2
    assert call(ldf=7) == -2 and call(ldo=7) == -2                                   # strides shorter than P
    assert call(nchan=2, ldf=16, ldo=16, ldc_in=7) == -2 and call(nchan=2, ldf=16, ldo=16, ldc_out=7) == -2
    assert call(nchan=2, ldf=15, ldo=16) == -2 and call(nchan=2, ldf=16, ldo=15) == -2
    assert call(X=0) == -2 and call(T=0) == -2 and call(mode=2) == -2
    assert call(B=2) == -2                                                           # two frames, one column, no times
    assert call(B=70000, times=a) == -3
    assert call(B=0) == 0                                                            # nothing to do, nothing launched


def test_public_keywords():
    from dnmf_amd import ops
    from dnmf_amd.Demix.dNMF import DeformableNMF, ExponentialFP, MultiChannelDNMF

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    for cls in (DeformableNMF, MultiChannelDNMF):
        assert ("registered", "nearest") in params(cls.update_footprints)
    assert ("registered", "nearest") in params(DeformableNMF.fit)
    assert params(ops.warp_pullback) == [("frames", E), ("frame_ids", E), ("sz", E), ("beta", E), ("times", E), ("out", None),
                                         ("nchan", 1), ("fill", None), ("coords", None), ("count", None)]
    assert params(ExponentialFP.registered_video) == [("self", E), ("frames", E), ("times", None), ("interpolation", "linear"),
                                                      ("fill", None), ("nchan", 1)]
    assert params(DeformableNMF.registered_video) == [("self", E), ("loader", E), ("interpolation", "linear"), ("fill", None)]
