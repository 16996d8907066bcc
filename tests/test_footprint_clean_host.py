"""K27's definition (tests/footprint_clean_restatement.py) pinned step by step against scipy.ndimage and np.cumsum, and shown to do
what it is for on planted volumes: a Gaussian cell with speckles, an island and a pinhole.  No GPU; nothing here has a tolerance.

The median alone removes single voxels and a 2 x 2 island, so the largest-part step has cases of its own, and each asserts that
it reaches that step: ``n_parts >= 2`` after the closing."""
import ctypes

import numpy as np
import pytest
import scipy.ndimage as ndi

import footprint_clean_restatement as R

DEPTHS = [2, 1]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("sz", [(9, 7, 4), (9, 7, 2), (9, 7, 1), (1, 7, 3), (5, 1, 1)])
def test_median_is_scipy_median_filter_nearest(sz):
    rng = np.random.default_rng(sum(sz))
    a = rng.random(sz).astype(np.float32)
    a[rng.random(sz) < 0.4] = 0
    size = (3, 3, 3) if sz[2] > 1 else (3, 3, 1)
    assert np.array_equal(bits(R.median3(a)), bits(ndi.median_filter(a, size=size, mode='nearest')))


def test_median_orders_signed_zeros_and_nan():
    a = np.zeros((3, 3, 1), dtype=np.float32)
    a[0, :, 0] = -0.0
    a[1, 0, 0] = -0.0
    assert bits(R.median3(a))[1, 1, 0] == 0                      # four -0.0 below five +0.0: the fifth value is +0.0
    a[1, 1, 0] = -0.0
    assert bits(R.median3(a))[1, 1, 0] == 0x80000000
    a[:] = np.nan
    a[0, 0, 0] = 1.0
    assert np.isnan(R.median3(a)).all()


@pytest.mark.parametrize("shape", [(8, 7, 3), (8, 7, 1), (1, 1, 1), (1, 9, 2)])
def test_closing_is_scipy_dilation_then_erosion_with_border_1(shape):
    rng = np.random.default_rng(shape[0] * 31 + shape[2])
    se = np.ones((3, 3, 3), dtype=bool)
    for density in (0.1, 0.4, 0.8):
        keep = rng.random(shape) < density
        ref = ndi.binary_erosion(ndi.binary_dilation(keep, se), se, border_value=1)
        got = R.close3(keep)
        assert np.array_equal(got, ref) and (got | keep).sum() == got.sum()         # the closing contains keep
        if shape[2] == 1:
            flat = np.ones((3, 3, 1), dtype=bool)
            assert np.array_equal(got, ndi.binary_erosion(ndi.binary_dilation(keep, flat), flat, border_value=1))


@pytest.mark.parametrize("shape", [(8, 7, 3), (16, 16, 1), (1, 1, 1)])
def test_labels_are_scipy_label_with_the_lowest_index(shape):
    rng = np.random.default_rng(shape[0])
    for density in (0.3, 0.6):
        mask = rng.random(shape) < density
        lab = R.label_faces(mask)
        ref, count = ndi.label(mask)
        assert np.array_equal(lab >= 0, mask)
        lin = np.arange(mask.size).reshape(shape)
        for q in range(1, count + 1):
            assert (lab[ref == q] == lin[ref == q].min()).all()
        assert len(np.unique(lab[mask])) == count


def test_labels_of_the_spiral_are_one_part():
    a, length = R.spiral(16)
    assert length >= 100
    lab = R.label_faces(a > 0)
    assert ndi.label(a > 0)[1] == 1 and (lab[a > 0] == 0).all()


def test_cut_is_np_cumsum_and_keeps_every_tie():
    rng = np.random.default_rng(5)
    mb = rng.random((6, 5, 2)).astype(np.float32)
    mb[rng.random(mb.shape) < 0.3] = 0
    mb[0, 0, 0] = mb[1, 1, 1] = mb[2, 2, 0]                      # ties
    for nrgthr in (0.5, 0.9, 0.9999, 1.0):
        keep, thr, energy, cum, v = R.cut_nrg(mb, nrgthr)
        assert (np.diff(v) <= 0).all()
        s, seq = 0.0, []
        for x in v:                                              # the additions one by one, in float64
            s = s + float(x) * float(x)
            seq.append(s)
        assert np.array_equal(cum, np.array(seq)) and np.array_equal(cum, np.cumsum(v.astype(np.float64) ** 2))
        j = int(np.nonzero(cum >= nrgthr * cum[-1])[0][0])
        assert thr == float(v[j]) and energy == cum[j] / cum[-1] and energy >= nrgthr
        assert j == 0 or cum[j - 1] < nrgthr * cum[-1]
        assert np.array_equal(keep, (mb >= v[j]) & (mb > 0)) and keep.sum() >= j + 1


@pytest.mark.parametrize("Z", DEPTHS)
def test_planted_volume_is_cleaned(Z):
    a, support, hole, box = R.planted_volume(Z)
    assert a[hole] == 0 and support[hole] and ((a > 0) & ~support).sum() == 4 + 4
    out, st = R.clean_footprint(a, box)
    kept = out > 0
    print(f"\ndepth {Z}: kept {kept.sum()} of {support.sum()} voxels of the cell, {(kept & ~support).sum()} outside, pinhole {out[hole]:.3f}")
    assert st["ok"] == 1 and st["n_box"] == a.size and st["n_kept"] == kept.sum()
    assert not (kept & ~support).any()                           # inside the cell's support: no speckle, no island
    assert kept.sum() >= 0.95 * support.sum()
    assert out[hole] > 0.5                                       # the pinhole is filled, by the median of its neighbours
    assert st["energy"] >= 0.9999 and st["threshold"] > 0
    assert np.array_equal(bits(out[kept]), bits(R.median3(a)[kept]))
    orig, _ = R.clean_footprint(a, box, values='original')
    assert np.array_equal(orig > 0, kept & (a > 0)) and np.array_equal(bits(orig[orig > 0]), bits(a[orig > 0]))
    # the same volume read through a box that only just holds the cell gives the same column
    xs, ys, zs = np.nonzero(support)
    tight = (xs.min() - 1, xs.max() + 1, ys.min() - 1, ys.max() + 1, 0, Z - 1)
    out2, st2 = R.clean_footprint(a, tight)
    assert np.array_equal(bits(out2), bits(out)) and st2["n_box"] < st["n_box"]


@pytest.mark.parametrize("Z", DEPTHS)
def test_the_largest_part_step_is_reached(Z):
    a, support, hole, box = R.planted_volume(Z)
    out, st = R.clean_footprint(a, box, median=False)            # without the median the speckles reach the labelling
    assert st["n_parts"] >= 2 and st["n_kept"] < st["n_closed"] and not ((out > 0) & ~support).any()
    a, support, box = R.island_volume(Z)
    for median in (True, False):
        out, st = R.clean_footprint(a, box, median=median)
        assert st["n_parts"] >= 2 and st["n_kept"] < st["n_closed"], (median, st)
        assert (out > 0).any() and not ((out > 0) & ~support).any()


def test_a_tie_in_size_goes_to_the_lowest_index():
    a, box = R.two_equal_parts()
    out, st = R.clean_footprint(a, box, nrgthr=1.0, median=False, closing=False)
    assert st["n_parts"] == 2 and st["n_kept"] == 4 and st["n_closed"] == 8
    assert (out[1:3, 6:8, 0] == 1.0).all() and out.sum() == 4.0  # the part of 1.0 (lower index), not the one of 2.0


def test_a_plateau_across_the_cut_is_kept_whole():
    a, box, nrgthr = R.plateau()
    out, st = R.clean_footprint(a, box, nrgthr=nrgthr, median=False, closing=False)
    assert st["threshold"] == 1.0 and st["n_cut"] == 25 and st["n_kept"] == 25 and st["energy"] == 42 / 52
    assert np.array_equal(bits(out), bits(a))


def test_max_method():
    a, support, hole, box = R.planted_volume(2)
    out, st = R.clean_footprint(a, box, method='max', maxthr=0.2)
    m = R.median3(a)
    assert st["threshold"] == 0.2 * float(m.max()) and np.isnan(st["energy"])
    assert st["n_cut"] == (m.astype(np.float64) > st["threshold"]).sum()
    none, st0 = R.clean_footprint(a, box, method='max', maxthr=1.0)       # nothing is above the maximum: refused, not deleted
    assert st0["ok"] == 0 and np.array_equal(bits(none), bits(a))


@pytest.mark.parametrize("what", ["zeros", "nan", "inf", "negative", "negative zero"])
def test_a_column_that_cannot_be_cleaned_comes_back(what):
    a, _, _, box = R.planted_volume(2)
    if what == "zeros":
        a[:] = 0
    elif what == "negative zero":
        a[:] = -0.0
    else:
        a[10, 9, 1] = dict(nan=np.nan, inf=np.inf, negative=-1e-6)[what]
    out, st = R.clean_footprint(a, box)
    assert st["ok"] == 0 and st["n_box"] == a.size and st["n_kept"] == 0 and np.isnan(st["threshold"]) and np.isnan(st["energy"])
    assert np.array_equal(bits(out), bits(a))
    if what in ("nan", "negative"):                              # outside the box it is no reason
        out, st = R.clean_footprint(a, (0, 23, 0, 19, 0, 0), median=False)
        assert st["ok"] == 1


def test_columns_are_independent():
    vols = [R.planted_volume(2)[0], np.zeros((24, 20, 2), np.float32), R.island_volume(2)[0]]
    A = np.stack(vols, axis=3)
    boxes = np.array([[0, 23, 0, 19, 0, 1]] * 3)
    out, st = R.clean_footprints(A, (24, 20, 2), boxes)
    assert st["ok"].tolist() == [1, 0, 1] and st["ok"].dtype == np.int32 and st["threshold"].dtype == np.float64
    for k, v in enumerate(vols):
        assert np.array_equal(bits(out[..., k]), bits(R.clean_footprint(v, boxes[k])[0]))


def test_the_library_refuses_bad_boxes_without_a_gpu():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    lib = _lib.load()
    assert lib.dnmf_clean_footprints_workspace(3) == 3 * 4096 * 4 and lib.dnmf_clean_footprints_workspace(0) == 0
    sz = (ctypes.c_int * 3)(70, 70, 1)

    def call(box, nrgthr=0.9, K=1, lda=1):
        b = (ctypes.c_int * 6)(*box)
        return lib.dnmf_clean_footprints(64, lda, sz, b, 64, K, 0, nrgthr, 0.2, 1, 1, 0, 128, lda, 64, 64, 64, 1 << 20, None)

    assert call((0, 64, 0, 63, 0, 0)) < 0 and b"4096" in lib.dnmf_last_error()
    assert call((0, 70, 0, 3, 0, 0)) < 0 and b"outside the volume" in lib.dnmf_last_error()
    assert call((3, 2, 0, 3, 0, 0)) < 0 and b"empty" in lib.dnmf_last_error()
    assert call((0, 3, 0, 3, 0, 0), nrgthr=1.5) < 0 and b"nrgthr" in lib.dnmf_last_error()
    assert call((0, 3, 0, 3, 0, 0), lda=0) < 0 and b"lda" in lib.dnmf_last_error()
