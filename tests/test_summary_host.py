"""Summary images (K18) without a GPU: the ABI and the wiring, the argument checks of the two C entries, the float64
restatement (tests/summary_restatement.py) against independent numpy, and the use case -- neurons that a mean image hides
and the local correlation image shows -- on the restatement alone."""
import ctypes
import inspect

import numpy as np
import pytest

import detect_restatement as DR
import summary_restatement as SR


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def planted():
    """The planted video and the restatement's images of it: computed once, never changed."""
    video, active, still, sigma = SR.planted_video()
    return video, active, still, sigma, SR.summary_images(video, "full")


def test_abi_declares_and_binds_the_two_entries(lib):
    from dnmf_amd import _lib, build
    assert _lib.SIGNATURES["dnmf_summary_images_workspace"][0] is ctypes.c_size_t
    res, args = _lib.SIGNATURES["dnmf_summary_images"]
    assert res is ctypes.c_int and args[12] is ctypes.c_size_t
    assert "summary_images.hip" in build.SOURCES
    assert lib.dnmf_summary_images and lib.dnmf_summary_images_workspace      # exported


def test_public_signatures():
    from dnmf_amd import ops
    from dnmf_amd.Demix.dNMF import DeformableNMF, ExponentialFP
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.kind is not p.VAR_KEYWORD]

    E = inspect.Parameter.empty
    assert params(ops.summary_images) == [("frames", E), ("sz", E), ("sub", None), ("frame_ids", None), ("neighbours", "full"),
                                          ("state", None), ("first", True), ("finish", True), ("segment", 0)]
    assert isinstance(inspect.getattr_static(ExponentialFP, "summary_images"), staticmethod)
    assert params(ExponentialFP.summary_images) == [("video", E), ("neighbours", "full")]
    assert params(DeformableNMF.summary_images) == [("self", E), ("loader", E), ("source", "video"), ("registered", None),
                                                    ("neighbours", "full")]
    assert params(MotionCorrect.summary_images) == [("self", E), ("video", None), ("neighbours", "full")]


def test_argument_errors_of_the_summary_entries(lib):
    """Validation happens before any HIP call, so it can be exercised on a CPU-only box."""
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    I3 = ctypes.c_int * 3
    ws, run = lib.dnmf_summary_images_workspace, lib.dnmf_summary_images
    sz = I3(20, 17, 1)
    P = 20 * 17

    def al(n):
        return (n + 255) // 256 * 256

    def size(nd, segs):
        return 256 + (1 + segs) * (al((2 + nd) * P * 8) + al(P * 4)) + al(P * 4)

    # 20 x 17 voxels are 2 tiles of 16 x 64: up to 1024 / 2 = 512 segments, of 16 frames or more
    assert ws(sz, 1, 37, 0) == size(4, 3)
    assert ws(sz, 0, 37, 0) == size(2, 3)
    assert ws(I3(9, 7, 3), 1, 37, 8) == 256 + 6 * (al(15 * 189 * 8) + al(189 * 4)) + al(189 * 4)
    assert ws(I3(9, 7, 3), 0, 1, 0) == 256 + 2 * (al(5 * 189 * 8) + al(189 * 4)) + al(189 * 4)
    # it does not grow with B beyond the partial sums of the segments, and never shrinks with B
    assert ws(sz, 1, 10 ** 4, 0) == ws(sz, 1, 10 ** 6, 0) == size(4, 512)
    sizes = [ws(sz, 1, B, 0) for B in range(1, 200)]
    assert sizes == sorted(sizes)
    assert ws(sz, 1, 0, 0) == 0 and lib.dnmf_last_error().startswith(b"dnmf_summary_images_workspace: B=0")
    assert ws(I3(20, 0, 1), 1, 4, 0) == 0 and b"volume" in lib.dnmf_last_error()
    assert ws(sz, 7, 4, 0) == 0 and b"neighbours=7" in lib.dnmf_last_error()
    assert ws(sz, 1, 4, -1) == 0 and b"segment" in lib.dnmf_last_error()
    assert ws(None, 1, 4, 0) == 0
    assert ws(I3(4, 4, 138), 1, 4, 0) == 0 and b"Z=138" in lib.dnmf_last_error()
    assert ws(I3(1 << 12, 1 << 12, 1 << 7), 1, 4, 0) == 0
    assert ws(sz, 1, 10 ** 6, 1) == 0 and b"segments" in lib.dnmf_last_error()

    need = ws(sz, 1, 4, 0)
    names = ["frames", "ldf", "sub", "lds", "frame_ids", "sz", "B", "neighbours", "first", "finish", "segment", "state", "bytes",
             "images", "stream"]
    ok = (a, P, None, 0, None, sz, 4, 1, 1, 1, 0, a, need, a, None)

    def call(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return run(*args)

    for name in ("frames", "state", "sz", "images"):
        assert call(**{name: None}) == -1 and lib.dnmf_last_error().startswith(b"dnmf_summary_images: "), name
    assert call(sz=I3(20, 17, 0)) == -2 and lib.dnmf_last_error().startswith(b"dnmf_summary_images: volume")
    assert call(B=0) == -2 and b"B=0" in lib.dnmf_last_error()
    assert call(neighbours=7) == -2 and b"neighbours=7" in lib.dnmf_last_error()
    assert call(segment=-2) == -2
    assert call(ldf=P - 1) == -2 and b"ldf" in lib.dnmf_last_error()
    assert call(sub=a, lds=P - 1) == -2
    assert call(sz=I3(4, 4, 138)) == -3
    assert call(bytes=need - 1) == -4 and str(need).encode() in lib.dnmf_last_error()
    assert call(state=a + 4) == -4 and b"aligned" in lib.dnmf_last_error()


def _corrcoef_mean(x, p, offs):
    vals = []
    for d in offs:
        q = tuple(np.add(p, d))
        if all(0 <= c < n for c, n in zip(q, x.shape[1:])):
            vals.append(np.corrcoef(x[(slice(None),) + p], x[(slice(None),) + q])[0, 1])
    return np.mean(vals), len(vals)


@pytest.mark.parametrize("shape,neighbours,count", [((6, 5, 1), "full", 8), ((5, 4, 3), "full", 26), ((6, 5, 1), "face", 4),
                                                    ((5, 4, 3), "face", 6)])
def test_restatement_is_the_mean_of_corrcoef(shape, neighbours, count):
    rng = np.random.RandomState(1)
    x = (3.0 + rng.randn(23, *shape)).astype(np.float32)
    x[:, 1:, 1:, :] += 0.7 * x[:, :-1, :-1, :]          # some correlation between neighbours
    im = SR.summary_images(x, neighbours)
    offs = SR.offsets(neighbours, shape)
    assert len(offs) == count
    x64 = x.astype(np.float64)
    inner = (2, 2, 1 if shape[2] > 1 else 0)
    want, n = _corrcoef_mean(x64, inner, offs)
    assert n == count
    assert abs(im["corr"][inner] - want) <= 1e-12
    corner, n = _corrcoef_mean(x64, (0, 0, 0), offs)    # a corner has fewer: no padding, no wrap
    assert n == {8: 3, 26: 7, 4: 2, 6: 3}[count]
    assert abs(im["corr"][0, 0, 0] - corner) <= 1e-12
    np.testing.assert_allclose(im["mean"], x64.mean(0), rtol=1e-14)
    np.testing.assert_allclose(im["std"], x64.std(0), rtol=1e-12)
    np.testing.assert_array_equal(im["max"], x64.max(0))


def test_restatement_special_voxels():
    rng = np.random.RandomState(2)
    x = (1.0 + rng.randn(12, 5, 5, 2)).astype(np.float32)
    x[:, 2, 2, 0] = 0.1                      # constant
    x[5, 0, 1, 1] = np.nan
    x[0, 4, 3, 0] = np.inf
    im = SR.summary_images(x, "full")
    assert im["std"][2, 2, 0] == 0.0 and im["mean"][2, 2, 0] == np.float64(np.float32(0.1)) and np.isnan(im["corr"][2, 2, 0])
    for p in ((0, 1, 1), (4, 3, 0)):
        assert all(np.isnan(im[k][p]) for k in ("mean", "std", "max", "corr"))
    assert np.isnan(im["corr"]).sum() == 3 and np.isnan(im["mean"]).sum() == 2
    # each of the three is left out of its neighbours' means
    x64 = x.astype(np.float64)
    special = {(2, 2, 0), (0, 1, 1), (4, 3, 0)}
    for p, left in (((2, 3, 1), 16), ((1, 1, 1), 15), ((3, 3, 1), 15)):        # of 17 neighbours inside the volume
        offs = [d for d in SR.offsets("full", x.shape[1:]) if tuple(int(v) for v in np.add(p, d)) not in special]
        want, n = _corrcoef_mean(x64, p, offs)
        assert n == left and abs(im["corr"][p] - want) <= 1e-12


def test_restatement_single_frame_and_line():
    rng = np.random.RandomState(3)
    one = SR.summary_images(rng.rand(1, 4, 3, 2).astype(np.float32), "full")
    assert np.isnan(one["corr"]).all() and (one["std"] == 0).all()
    line = rng.rand(9, 1, 7, 1).astype(np.float32)
    for nb in ("face", "full"):
        assert SR.offsets(nb, (1, 7, 1)) == [(0, -1, 0), (0, 1, 0)]
        im = SR.summary_images(line, nb)
        x64 = line.astype(np.float64)[:, 0, :, 0]
        want = 0.5 * (np.corrcoef(x64[:, 3], x64[:, 2])[0, 1] + np.corrcoef(x64[:, 3], x64[:, 4])[0, 1])
        assert abs(im["corr"][0, 3, 0] - want) <= 1e-12


def test_restatement_with_sub_rounds_the_difference_to_fp32():
    rng = np.random.RandomState(4)
    fr, sb = rng.rand(6, 3, 3, 1).astype(np.float32) * 1000, rng.rand(6, 3, 3, 1).astype(np.float32)
    a, b = SR.summary_images(fr, "face", sub=sb), SR.summary_images((fr - sb).astype(np.float32), "face")
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def test_correlation_image_shows_what_the_mean_hides(planted):
    """The input conditions of the GPU test: K14's definition on the restatement's corr image returns the two active
    centres within 1.5 voxels; on the mean image its first pick is the constant blob."""
    video, active, still, sigma, im = planted
    assert video.shape == (48, 40, 36, 2)
    out = DR.detect(im["corr"], 2, sigma)
    assert out["count"] == 2
    dist = np.linalg.norm(out["positions"][None] - active[:, None], axis=2)
    print("corr picks", out["positions"].tolist(), "worst distance", dist.min(1).max())
    assert dist.min(1).max() <= 1.5 and sorted(dist.argmin(1)) == [0, 1]
    first = DR.detect(im["mean"], 1, sigma)["positions"][0]
    assert np.linalg.norm(first - still) <= 1.5
    # equal time-averaged brightness: the mean image ranks the two active blobs the same
    m = im["mean"]
    assert abs(m[10, 9, 0] - m[28, 25, 1]) <= 0.02 and m[12, 27, 0] > m[10, 9, 0] + 1.5
