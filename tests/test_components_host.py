"""Component evaluation (K24) without a GPU: the float64 restatement (tests/components_restatement.py) against outside
definitions, its edge cases, the use case -- six planted cells and two components on nothing -- on the restatement alone,
the torch helpers of the front end on the CPU, and the argument checks of the two C entries."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import components_restatement as CR


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


def _random_case(seed=0, sz=(7, 6, 2), K=3, T=5):
    rng = np.random.default_rng(seed)
    P = sz[0] * sz[1] * sz[2]
    frames, sub = rng.random((T, P)) + 0.5, 0.3 * rng.random((T, P))
    A_rows, C, w = rng.random((K, P)), rng.random((K, T)), rng.integers(0, 3, (K, T)).astype(float)
    boxes = np.array([[0, 3, 1, 4, 0, 1], [2, 6, 0, 5, 1, 1], [0, 6, 0, 5, 0, 1]])
    return frames, sub, A_rows, C, w, boxes, sz


def test_restatement_against_outside_definitions():
    from scipy.stats import median_abs_deviation
    frames, sub, A_rows, C, w, boxes, sz = _random_case()
    for s in (sub, None):
        st = CR.component_stats(frames, sz, A_rows, boxes, C, w, sub=s)
        for k in range(3):
            u = CR.box_voxels(boxes[k], sz)
            a = A_rows[k, u]
            acc = np.zeros(u.size)
            for t in range(5):
                e = frames[t, u] - (0 if s is None else s[t, u]) + a * C[k, t]
                assert st["frame_corr"][k, t] == pytest.approx(np.corrcoef(a, e)[0, 1], abs=1e-12)
                amp = np.linalg.lstsq(np.stack([a, np.ones_like(a)], 1), e, rcond=None)[0][0]
                assert st["raw"][k, t] == pytest.approx(amp, rel=1e-11, abs=1e-12)
                np.testing.assert_allclose(st["sums"][k, t], [e.sum(), (e * e).sum(), (a * e).sum()], rtol=1e-13)
                acc += w[k, t] * e
            image = acc / w[k].sum()
            np.testing.assert_allclose(st["image"][k, :u.size], image, rtol=1e-13)
            assert np.isnan(st["image"][k, u.size:]).all()
            assert st["r_values"][k] == pytest.approx(np.corrcoef(a, image)[0, 1], abs=1e-12)
            np.testing.assert_allclose(st["foot"][k], [u.size, a.sum(), (a * a).sum()], rtol=1e-14)
    x = np.random.default_rng(1).standard_normal(200).cumsum()
    assert CR.noise_mad(x) == pytest.approx(median_abs_deviation(np.diff(x)) / (0.6745 * math.sqrt(2)), rel=1e-14)
    # white noise of std s: diff has std s sqrt 2, and MAD / 0.6745 estimates a std
    z = np.random.default_rng(2).standard_normal(20000) * 0.3
    assert CR.noise_mad(z) == pytest.approx(0.3, rel=0.05)


def test_box_order_is_x_slowest():
    u = CR.box_voxels((1, 2, 0, 1, 1, 2), (4, 3, 3))
    assert u.tolist() == [(x * 3 + y) * 3 + z for x in (1, 2) for y in (0, 1) for z in (1, 2)]


def test_leave_one_out_ranking_with_ties_and_both_ends():
    C = np.array([[5.0, 1.0, 1.0, 1.0, 3.0, 0.0, 3.0, 9.0]])
    s = CR.leave_one_out_score(C)
    # the ends take their one neighbour; frame 0's own 5 and frame 7's own 9 count for their neighbours only
    assert s.tolist() == [[1.0, 3.0, 1.0, 2.0, 0.5, 3.0, 4.5, 3.0]]
    assert CR.n_active(0.25, 8) == 2 and CR.n_active(0.26, 8) == 3 and CR.n_active(1e-9, 8) == 1 and CR.n_active(1.0, 8) == 8
    assert CR.active_weights(s, 0.25).tolist() == [[0, 1, 0, 0, 0, 0, 1, 0]]         # 4.5, then the first of the three 3s
    assert CR.active_weights(s, 0.5).tolist() == [[0, 1, 0, 0, 0, 1, 1, 1]]          # all three 3s
    assert CR.active_weights(s, 0.3).tolist() == [[0, 1, 0, 0, 0, 1, 1, 0]]          # ties go to the lower t
    assert CR.leave_one_out_score(np.array([[2.0, 7.0]])).tolist() == [[7.0, 2.0]]
    assert CR.leave_one_out_score(np.array([[2.0]])).tolist() == [[2.0]]
    # top-C selection, the biased choice, takes the frames themselves
    assert CR.active_weights(C, 0.25).tolist() == [[1, 0, 0, 0, 0, 0, 0, 1]]


def test_nan_rules():
    sz = (3, 3, 1)
    rng = np.random.default_rng(3)
    frames = rng.random((4, 9)) + 1.0
    A_rows = np.tile(np.round(rng.random(9) * 64) / 64 + 1 / 64, (4, 1))     # dyadic: (2 - a) + a is exactly 2
    C, w = np.ones((4, 4)), np.ones((4, 4))
    boxes = np.array([[1, 1, 1, 1, 0, 0],      # one voxel: no variance
                      [0, 2, 0, 2, 0, 0],      # the whole volume
                      [0, 1, 0, 1, 0, 0],      # a constant e in frame 2
                      [0, 2, 0, 1, 0, 0]])     # zero weights
    w[3] = 0.0
    frames[1, 8] = np.nan                      # inside box 1 only
    u2 = CR.box_voxels(boxes[2], sz)
    frames[2, u2] = 2.0 - A_rows[2, u2]        # e = frames + a C = 2 on box 2
    st = CR.component_stats(frames, sz, A_rows, boxes, C, w, check=False)
    # one voxel: both variances are zero
    assert np.isnan(st["frame_corr"][0]).all() and np.isnan(st["raw"][0]).all() and np.isnan(st["r_values"][0])
    assert np.isfinite(st["sums"][0]).all() and st["foot"][0, 0] == 1
    # the NaN sample: that (k, t) alone is invalid, and takes no part in the image
    bad = np.zeros((4, 4), bool)
    bad[1, 1] = True
    assert (np.isnan(st["sums"][..., 0]) == bad).all() and np.isnan(st["sums"][1, 1]).all()
    assert np.isnan(st["frame_corr"][1, 1]) and np.isnan(st["raw"][1, 1]) and st["wsum"][1] == 3.0
    assert np.isfinite(st["image"][1]).all() and np.isfinite(st["r_values"][1])
    u1 = CR.box_voxels(boxes[1], sz)
    e = frames[:, u1] + A_rows[1, u1]
    np.testing.assert_allclose(st["image"][1], e[[0, 2, 3]].mean(0), rtol=1e-14)
    # a constant e: no correlation, but a raw amplitude (0: the offset explains it)
    assert np.isnan(st["frame_corr"][2, 2]) and st["raw"][2, 2] == 0.0 and np.isfinite(st["frame_corr"][2, [0, 1, 3]]).all()
    # zero weights
    assert st["wsum"][3] == 0.0 and np.isnan(st["r_values"][3]) and np.isnan(st["image"][3]).all()
    assert np.isfinite(st["frame_corr"][3]).all()
    # snr: fewer than 4 valid frames, no active frame, zero noise
    raw = np.array([[1.0, np.nan, 2.0, 3.0, np.nan], [1.0, 2.0, 4.0, 3.0, 9.0], [1.0, 2.0, 3.0, 4.0, 5.0], [1.0, 5.0, 2.0, 7.0, 3.0]])
    ww = np.array([[1, 0, 0, 0, 0], [0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 1, 0, 1, 0]], float)
    s = CR.snr(raw, ww)
    assert np.isnan(s[:3]).all()
    d = np.diff(raw[3])
    assert s[3] == pytest.approx((6.0 - 3.0) / (np.median(np.abs(d - np.median(d))) / (0.6745 * math.sqrt(2))))
    # the input condition the comparison with the kernel relies on is asserted
    with pytest.raises(AssertionError, match="variance below"):
        CR.component_stats(1e4 + 1e-3 * frames[[0, 3]], sz, A_rows[:1], boxes[1:2], C[:1, :2], w[:1, :2])


@pytest.fixture(scope="module")
def planted():
    """(depth, seed) -> the restatement's evaluation of the planted video at T = 40, exact NNLS traces: computed once."""
    out = {}
    for depth in (2, 1):
        for seed in (0, 1, 2):
            video, A8, _, sz = CR.planted_video(depth, 40, seed)
            C = CR.nnls_traces(video, A8)
            out[depth, seed] = CR.evaluate(video, sz, A8, C, sub=(A8 @ C).T)
    return out


def test_planted_video_keeps_exactly_the_six_cells(planted):
    """Measured on the restatement, T = 40, both depths, seeds 0-2: true cells r_values 0.85-0.99 and snr 2.2-19.2; components
    on nothing r_values 0.08-0.17 and snr 0.01-0.76."""
    r_true = np.array([st["r_values"][:6] for st in planted.values()])
    r_spur = np.array([st["r_values"][6:] for st in planted.values()])
    s_true = np.array([st["snr"][:6] for st in planted.values()])
    s_spur = np.array([st["snr"][6:] for st in planted.values()])
    print(f"\nplanted video, leave-one-out selection: true cells r_values {r_true.min():.2f}..{r_true.max():.2f}, snr "
          f"{s_true.min():.1f}..{s_true.max():.1f}; spurious r_values {r_spur.min():.2f}..{r_spur.max():.2f}, snr "
          f"{s_spur.min():.2f}..{s_spur.max():.2f}")
    assert (r_true > 0.5).all() and (np.abs(r_spur) < 0.5).all()
    assert r_true.min() - np.abs(r_spur).max() >= 0.2          # the seeds leave a gap
    for st in planted.values():
        assert st["keep"].tolist() == [True] * 6 + [False] * 2
        assert st["boxes"].shape == (8, 6) and (st["w"].sum(1) == 10).all()


@pytest.mark.parametrize("depth", [2, 1])
def test_top_c_selection_is_biased_towards_the_footprint(depth):
    """The frames where a component's own trace is largest are those whose noise looks like its footprint: on a component on
    nothing their mean image correlates with the footprint, more so the more frames there are to choose from.  Measured at
    T = 400, seed 0: largest spurious r_value 0.35 (depth 2) and 0.44 (depth 1) under top-C selection against 0.19 and 0.21
    under the leave-one-out score; snr 1.2-1.4 against 0.05-0.16."""
    video, A8, _, sz = CR.planted_video(depth, 400, 0)
    C = CR.nnls_traces(video, A8)
    sub = (A8 @ C).T
    loo = CR.evaluate(video, sz, A8, C, sub=sub, selection="loo")
    top = CR.evaluate(video, sz, A8, C, sub=sub, selection="top")
    print(f"\ndepth {depth}, T = 400: spurious r_values top-C {top['r_values'][6:]}, leave-one-out {loo['r_values'][6:]}; snr "
          f"{top['snr'][6:]}, {loo['snr'][6:]}")
    assert top["r_values"][6:].max() > loo["r_values"][6:].max()
    assert top["snr"][6:].max() > loo["snr"][6:].max()
    assert loo["keep"].tolist() == [True] * 6 + [False] * 2
    assert not (top["snr"][6:] < 1.0).all()        # top-C selection would pass a component on nothing through min_snr


def test_torch_helpers_match_the_restatement_on_the_cpu():
    from dnmf_amd import ops
    sz = (24, 20, 2)
    A8 = CR.gaussian_footprints(sz, CR.planted_centres(2)).astype(np.float32)
    A8[:, 7] = 0.0                                 # an empty footprint gets the whole volume
    for floor, margin in ((1e-3, 2), (0.1, 0), (0.5, 30)):
        got = ops.component_boxes(torch.from_numpy(A8).reshape(24, 20, 2, 8), sz, floor=floor, margin=margin)
        assert got.dtype == torch.int32 and tuple(got.shape) == (8, 6)
        want = CR.component_boxes(A8[:, :7], sz, floor, margin)
        assert got[:7].tolist() == want.tolist()
        assert got[7].tolist() == [0, 23, 0, 19, 0, 1]
    rng = np.random.default_rng(5)
    raw = rng.standard_normal((6, 30)).cumsum(1)
    raw[1, [3, 4, 17]] = np.nan
    raw[2, 3:] = np.nan
    raw[3] = 1.0
    w = (rng.random((6, 30)) < 0.3).astype(np.float32)
    w[4] = 0
    got = ops.component_snr(torch.from_numpy(raw), torch.from_numpy(w)).numpy()
    want = CR.snr(raw, w)
    assert (np.isnan(got) == np.isnan(want)).all() and np.isnan(want).tolist() == [False, False, True, True, True, False]
    np.testing.assert_allclose(got[~np.isnan(want)], want[~np.isnan(want)], rtol=1e-13)


def test_public_signatures():
    from dnmf_amd import ops, _lib, build
    from dnmf_amd.Demix.dNMF import DeformableNMF

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(ops.component_stats) == [("frames", E), ("sz", E), ("A_rows", E), ("boxes", E), ("C", E), ("w", E), ("sub", None),
                                           ("frame_ids", None), ("state", None), ("first", True), ("finish", True), ("segment", 0)]
    assert params(ops.component_boxes) == [("A", E), ("sz", E), ("floor", 1e-3), ("margin", 2)]
    assert params(DeformableNMF.evaluate_components) == [("self", E), ("loader", E), ("registered", "linear"), ("active", 0.25),
                                                         ("margin", 2), ("floor", 1e-3), ("min_r", 0.5), ("min_snr", 1.0)]
    assert params(DeformableNMF.select_components) == [("self", E), ("keep", E)]
    assert "component_stats.hip" in build.SOURCES
    res, args = _lib.SIGNATURES["dnmf_component_stats"]
    assert res is ctypes.c_int and args[20] is ctypes.c_size_t
    assert _lib.SIGNATURES["dnmf_component_stats_workspace"][0] is ctypes.c_size_t


def test_argument_errors_are_reported_without_a_gpu(lib):
    """Every refusal comes before the first HIP call, so it shows on a box without a GPU."""
    buf = ctypes.create_string_buffer(1 << 12)
    addr = ctypes.addressof(buf)
    sz = (ctypes.c_int * 3)(16, 16, 17)
    P = 16 * 16 * 17

    def boxes(*rows):
        flat = [v for r in rows for v in r]
        return (ctypes.c_int * len(flat))(*flat)

    def call(bx, K=1, B=4, state=addr, nbytes=1 << 30, sz=sz, ldf=P, lds=P, lda=P, ldc=4, ldw=4, ldi=4096, segment=0, frames=addr,
             sub=addr, image=addr, finish=1):
        return lib.dnmf_component_stats(frames, ldf, sub, lds, None, sz, B, addr, lda, bx, addr, K, addr, ldc, addr, ldw, 1, finish,
                                        segment, state, nbytes, addr, addr, addr, addr, image, ldi, addr, None)

    full = boxes((0, 15, 0, 15, 0, 15))            # exactly 4096 voxels
    assert lib.dnmf_component_stats_workspace(sz, full, 1, 4, 0) > 0
    # a state too short for it: refused, like every case below, before a launch
    assert call(full, nbytes=64) == -4 and b"state of 64 bytes" in lib.dnmf_last_error()
    assert call(full, state=addr + 4) == -4 and b"aligned" in lib.dnmf_last_error()
    over = boxes((0, 15, 0, 15, 0, 16))            # 4352 voxels
    assert call(over) == -3 and b"4352 voxels, at most 4096" in lib.dnmf_last_error()
    assert lib.dnmf_component_stats_workspace(sz, over, 1, 4, 0) == 0
    for bad in ((0, 16, 0, 3, 0, 3), (-1, 3, 0, 3, 0, 3), (0, 3, 0, 3, 0, 17), (4, 3, 0, 3, 0, 3), (0, 3, 2, 1, 0, 3)):
        assert call(boxes((0, 1, 0, 1, 0, 1), bad), K=2) == -2 and b"box 1" in lib.dnmf_last_error(), bad
        assert lib.dnmf_component_stats_workspace(sz, boxes((0, 1, 0, 1, 0, 1), bad), 2, 4, 0) == 0
    ok = boxes((0, 1, 0, 1, 0, 1))
    assert call(ok, frames=None) == -1 and call(ok, state=None) == -1 and call(ok, image=None) == -1
    assert call(None) == -1
    assert call(ok, image=None, finish=0, nbytes=64) == -4       # image may be NULL without finish
    assert call(ok, sub=None, lds=0, nbytes=64) == -4            # and sub always
    assert call(ok, K=0) == -2 and call(ok, B=0) == -2 and call(ok, segment=-1) == -2
    assert call(ok, ldf=P - 1) == -2 and call(ok, lds=P - 1) == -2 and call(ok, lda=P - 1) == -2
    assert call(ok, ldc=3) == -2 and call(ok, ldw=3) == -2 and call(ok, ldi=7) == -2
    assert call(ok, sz=(ctypes.c_int * 3)(16, 0, 17)) == -2
    assert call(ok, B=70000, ldc=70000, ldw=70000, segment=1) == -3 and b"segments" in lib.dnmf_last_error()
    # the state: per neuron a weight sum and vstride image sums, and the same again for each of the segments of a call; it does
    # not decrease with B
    one = lib.dnmf_component_stats_workspace(sz, full, 1, 4, 4)
    assert one == 256 + 4096 * 8 + 256 + 4096 * 8
    assert lib.dnmf_component_stats_workspace(sz, full, 1, 8, 4) == 256 + 4096 * 8 + 256 + 2 * 4096 * 8
    three = boxes((0, 1, 0, 1, 0, 1), (2, 9, 0, 15, 3, 3), (5, 5, 5, 5, 5, 5))
    sizes = [lib.dnmf_component_stats_workspace(sz, three, 3, B, 0) for B in (1, 15, 16, 17, 100, 1000, 100000)]
    assert sizes == sorted(sizes) and sizes[0] > 0
