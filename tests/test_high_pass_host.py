"""The spatial high-pass (K22) without a GPU: the taps of ``ops.high_pass_taps`` and of the float64 definition
(tests/high_pass_restatement.py), the definition against scipy and numpy's own border handling, a constant image, one NaN, and
the argument checks of the C entry (it refuses before it launches anything)."""
import ctypes

import numpy as np
import pytest

import high_pass_restatement as HR

# (X, Y), gSig: scipy's 'reflect' equals the period-2N reflection in the first five; at (3, 4) gSig 10 -- a radius of five times
# the extent -- it does not (3e-3), numpy's 'symmetric' padding does in all six
AGREEING = [((5, 37), 7), ((40, 33), 3), ((1, 9), 3), ((2, 2), 2), ((6, 5), 10)]
ALL_SIX = AGREEING + [((3, 4), 10)]
COUNTS = {1: (3, 5), 2: (7, 29), 3: (9, 49), 4: (13, 113), 7: (21, 309), 10: (31, 709)}


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


def _image(shape, seed):
    return np.random.default_rng(seed).normal(size=shape) * 3.0 + 10.0


@pytest.mark.parametrize("gsig", sorted(COUNTS))
def test_taps_size_count_symmetry_and_zero_sum(gsig):
    from dnmf_amd import ops
    n, count = COUNTS[gsig]
    for taps in (ops.high_pass_taps((gsig, gsig)), ops.high_pass_taps(gsig), HR.high_pass_taps((gsig, 99))):
        assert taps.dtype == np.float64 and taps.shape == (n, n)
        assert np.count_nonzero(taps) == count
        assert np.array_equal(taps, taps.T) and np.array_equal(taps, taps[::-1]) and np.array_equal(taps, taps[:, ::-1])
        assert abs(taps.sum()) <= 1e-15
    assert np.array_equal(ops.high_pass_taps((gsig, gsig)), HR.high_pass_taps(gsig))


def test_taps_of_gsig_1_are_the_plus_shape():
    from dnmf_amd import ops
    g = np.array([np.exp(-0.5), 1.0, np.exp(-0.5)])
    g /= g.sum()
    m = (g[1] * g[1] + 4 * g[0] * g[1]) / 5
    want = np.array([[0, g[0] * g[1] - m, 0], [g[0] * g[1] - m, g[1] * g[1] - m, g[0] * g[1] - m], [0, g[0] * g[1] - m, 0]])
    assert np.abs(ops.high_pass_taps((1, 1)) - want).max() <= 1e-15
    assert np.abs(HR.high_pass_taps(1) - want).max() <= 1e-15


@pytest.mark.parametrize("bad", [0, -1.0, float("nan"), float("inf"), (0, 3), (float("nan"), 3), ()])
def test_taps_refuse_a_bad_gsig(bad):
    from dnmf_amd import ops
    with pytest.raises(ValueError):
        ops.high_pass_taps(bad)


@pytest.mark.parametrize("shape,gsig", AGREEING)
def test_definition_against_scipy_correlate(shape, gsig):
    from scipy import ndimage
    img = _image(shape, 1)
    got = HR.high_pass_filter_space(img, (gsig, gsig))
    want = ndimage.correlate(img, HR.high_pass_taps(gsig), mode="reflect")
    assert np.abs(got - want).max() <= 1e-13


@pytest.mark.parametrize("shape,gsig", ALL_SIX)
def test_definition_against_symmetric_padding(shape, gsig):
    """The same sum over windows of np.pad(mode='symmetric'), taps in the definition's order: exactly equal."""
    img = _image(shape, 2)
    taps = HR.high_pass_taps(gsig)
    n, h = taps.shape[0], taps.shape[0] // 2
    pad = np.pad(img, h, mode="symmetric")
    want = np.zeros(shape)
    for j in range(n):
        for i in range(n):
            if taps[i, j] != 0:
                want += taps[i, j] * pad[i:i + shape[0], j:j + shape[1]]
    assert np.array_equal(HR.high_pass_filter_space(img, gsig), want)
    idx = HR.reflect_index(np.arange(-h, shape[0] + h), shape[0])
    assert np.array_equal(pad[:, h], img[idx, 0])


def test_three_dimensional_images_are_filtered_slice_by_slice():
    vol = _image((7, 9, 3), 3)
    got = HR.high_pass_filter_space(vol, (2, 2))
    for z in range(3):
        assert np.array_equal(got[..., z], HR.high_pass_filter_space(vol[..., z], (2, 2)))


@pytest.mark.parametrize("shape,gsig", ALL_SIX)
def test_a_constant_image_is_removed(shape, gsig):
    c = 1234.5
    assert np.abs(HR.high_pass_filter_space(np.full(shape, c), gsig)).max() <= 1e-13 * c


def test_one_nan_spreads_over_the_disc_only():
    img = _image((40, 33), 4)
    img[20, 15] = np.nan
    taps = HR.high_pass_taps(3)
    got = HR.high_pass_filter_space(img, 3)
    want = np.zeros(img.shape, bool)
    want[16:25, 11:20] = taps[::-1, ::-1] != 0
    assert np.array_equal(np.isnan(got), want) and want.sum() == 49


def test_c_entry_refuses_before_it_launches(lib):
    from dnmf_amd import _lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def call(sz, B, n, ldf=64, ldo=64, frames=p, taps=p, out=p):
        return lib.dnmf_high_pass_frames(frames, ldf, None, (ctypes.c_int * 3)(*sz), B, taps, n, out, ldo, None)

    E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
    assert call((2, 3, 4), 1, 33) == E_UNSUPPORTED and b"33" in lib.dnmf_last_error()
    assert call((2, 3, 4), 1, 35) == E_UNSUPPORTED
    for n in (0, -1, 2, 32):
        assert call((2, 3, 4), 1, n) == E_SHAPE
    for sz in ((0, 3, 4), (2, 0, 4), (2, 3, 0)):
        assert call(sz, 1, 3) == E_SHAPE
    assert call((2, 3, 4), 0, 3) == E_SHAPE
    assert call((2, 3, 4), 1, 3, ldf=23) == E_SHAPE and call((2, 3, 4), 1, 3, ldo=23) == E_SHAPE
    assert call((2, 3, 4), 1, 3, frames=None) == E_NULL and call((2, 3, 4), 1, 3, taps=None) == E_NULL
    assert call((2, 3, 4), 1, 3, out=None) == E_NULL
    assert call((1 << 11, 1 << 10, 1 << 10), 1, 3, ldf=1 << 31, ldo=1 << 31) == E_UNSUPPORTED
    assert _lib.SIGNATURES["dnmf_high_pass_frames"][0] is ctypes.c_int
