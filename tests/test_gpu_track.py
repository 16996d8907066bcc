"""K15 on the GPU against its float64 restatement (tests/track_restatement.py), and the public entry points built on it."""
import ctypes

import numpy as np
import pytest
import torch

import detect_restatement as DR
import track_restatement as TR

pytestmark = pytest.mark.gpu


def rows_of(frames, pad=3):
    """(T, X, Y, Z) -> padded CUDA rows: a (T, P) view of (T, P + pad) floats, the padding poisoned."""
    T = frames.shape[0]
    P = int(np.prod(frames.shape[1:]))
    buf = torch.full((T, P + pad), float("nan"), device="cuda")
    buf[:, :P] = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32).reshape(T, P)).cuda()
    return buf[:, :P]


def gpu_track(frames, predict, sigma, search, **kw):
    from dnmf_amd import ops
    pred = predict if isinstance(predict, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(predict)).cuda()
    pos, amp, peak = ops.track_neurons(rows_of(frames), frames.shape[1:], pred, shape_std=sigma, search=search, **kw)
    assert pos.dtype == torch.float64 and amp.dtype == torch.float32 and peak.dtype == torch.float32 and pos.is_cuda
    return pos.cpu().numpy(), amp.cpu().numpy().astype(np.float64), peak.cpu().numpy().astype(np.float64)


def compare(ref, got, what):
    """Wherever the restatement's margin is >= 1e-3: the same p*, centre within 1e-3 voxel, amplitude and peak at rtol 1e-3
    (K14's documented fp32 bound for a (2 r + 1)-term sum per axis); the NaN rows are the same set.  Returns the share of
    results the margin leaves out."""
    pos, amp, peak = got
    nan_ref = np.isnan(ref["positions"]).any(1)
    np.testing.assert_array_equal(np.isnan(pos).any(1), nan_ref)
    np.testing.assert_array_equal(np.isnan(pos).all(1), nan_ref)
    np.testing.assert_array_equal(np.isnan(amp), nan_ref)
    np.testing.assert_array_equal(np.isnan(peak), nan_ref)
    sure = ~nan_ref & (np.nan_to_num(ref["margin"], nan=0.0) >= 1e-3)
    k, t = np.nonzero(sure)
    if len(k) == 0:
        return 1.0 if (~nan_ref).any() else 0.0
    dp = np.abs(pos[k, :, t] - ref["positions"][k, :, t]).max()
    da = np.abs(amp[k, t] / ref["amplitudes"][k, t] - 1).max()
    ds = np.abs(peak[k, t] / ref["peaks"][k, t] - 1).max()
    print(f"{what}: {len(k)} results compared, max |p^ - p^_ref| {dp:.2e} voxel, amplitude deviation {da:.2e}, peak deviation {ds:.2e}")
    # |delta| <= 1/2: the integer voxel is the rounded centre unless delta is within 1e-3 of a half; compare it where it is not
    delta = ref["positions"][k, :, t] - ref["pstar"][k, :, t]
    clear = np.abs(delta) < 0.499
    np.testing.assert_array_equal(np.rint(pos[k, :, t])[clear], ref["pstar"][k, :, t][clear])
    assert dp <= 1e-3
    assert da <= 1e-3
    assert ds <= 1e-3
    return 1.0 - sure.sum() / max(1, (~nan_ref).sum())


@pytest.mark.parametrize("case", range(len(TR.CASES)))
def test_gpu_equals_restatement_on_moving_planted_gaussians(case):
    frames, rest, truth, amps, sigma, search = TR.moving_case(case)
    T = frames.shape[0]
    times = None
    if case == 0:
        # a subset of the rows in reverse order: slot j of every output is row times[j]
        times = [4, 2, 1]
        ref = TR.track(frames[times], rest, sigma, search)
    else:
        ref = TR.track(frames, rest, sigma, search)
    # conditions on the input, met by the restatement alone: everything found, no pick decided by rounding
    assert np.isfinite(ref["positions"]).all() and ref["margin"].min() >= 1e-3
    left_out = compare(ref, gpu_track(frames, rest, sigma, search, times=times), f"case {TR.CASES[case]}")
    assert left_out == 0.0
    if case == 0:
        full = TR.track(frames, rest, sigma, search)
        assert compare(full, gpu_track(frames, rest, sigma, search), "case 0, every row") == 0.0
        # a per-frame background is taken off before the filter
        bg = np.linspace(-0.2, 0.3, T)
        refb = TR.track(frames, rest, sigma, search, background=bg)
        assert compare(refb, gpu_track(frames, rest, sigma, search, background=torch.from_numpy(bg)), "case 0, background") == 0.0


EDGE_SZ, EDGE_SIGMA = (20, 18, 2), 1.5


def edge_frames():
    centres = np.array([[0.4, 0.7, 0.0], [19.0, 17.0, 1.0], [9.6, 8.3, 0.6]])
    return np.stack([DR.plant(EDGE_SZ, centres + [0.3 * t, -0.2 * t, 0.0], [1.0, 0.8, 0.9], EDGE_SIGMA, noise=0.002, seed=40 + t)
                     for t in range(2)])


def test_window_edges():
    """Predictions at a corner, one voxel outside, far outside (NaN), and at x.5 (half to even)."""
    frames = edge_frames()
    X, Y, Z = EDGE_SZ
    pred = np.array([[0.0, 0.0, 0.0], [X - 1.0, Y - 1.0, Z - 1.0], [-1.0, -1.0, 0.0], [float(X), float(Y), Z - 1.0],
                     [X + 40.0, 5.0, 0.0], [-1e30, 5.0, 0.0], [9.5, 8.5, 0.0], [10.5, 7.5, 1.0], [float("nan"), 3.0, 0.0],
                     [3.0, float("inf"), 0.0]])
    for search in ((2, 2, 1), (3, 1, 0)):
        ref = TR.track(frames, pred, EDGE_SIGMA, search)
        assert np.isnan(ref["positions"][[4, 5, 8, 9]]).all() and np.isfinite(ref["positions"][[0, 1, 2, 3, 6, 7]]).all()
        compare(ref, gpu_track(frames, pred, EDGE_SIGMA, search), f"edges, search {search}")


def test_zero_search_reads_the_score_at_the_rounded_prediction():
    frames = edge_frames()
    pred = np.array([[9.5, 8.5, 0.4], [10.5, 7.5, 0.6], [0.0, 0.0, 0.0], [19.0, 17.0, 1.0], [19.4, 0.2, 1.4], [20.0, 3.0, 0.0]])
    ref = TR.track(frames, pred, EDGE_SIGMA, (0, 0, 0), threshold=-1e30)
    np.testing.assert_array_equal(ref["pstar"][:5, :, 0], [[10, 8, 0], [10, 8, 1], [0, 0, 0], [19, 17, 1], [19, 0, 1]])
    assert np.isnan(ref["positions"][5]).all() and np.isinf(ref["margin"][:5]).all()
    pos, amp, peak = gpu_track(frames, pred, EDGE_SIGMA, (0, 0, 0), threshold=-1e30)
    np.testing.assert_array_equal(np.rint(pos[:5]), ref["pstar"][:5])
    assert np.isnan(pos[5]).all() and np.isnan(peak[5]).all()
    score = np.stack([DR.score(frames[t], EDGE_SIGMA, 0.0) for t in range(2)])
    for k in range(5):
        x, y, z = ref["pstar"][k, :, 0]
        np.testing.assert_allclose(peak[k], score[:, x, y, z], rtol=1e-3, atol=1e-6)
    np.testing.assert_allclose(pos[:4], ref["positions"][:4], atol=1e-3)     # the four on a blob: a well-conditioned parabola


def test_ties_and_nan_scores():
    """A constant frame: the lowest index of the window, delta = 0.  One NaN voxel inside the region: the poisoned scores never
    win.  An all-NaN frame: a NaN row, and the frames after it are unaffected."""
    sigma, search = 1.5, (3, 2, 1)
    frames = np.full((4, 40, 36, 2), 0.5, dtype=np.float32)
    pred = np.array([[20.0, 18.0, 1.0], [19.5, 16.5, 0.0]])
    frames[1, 12, 18, 0] = np.nan
    frames[2] = np.nan
    frames[3, :, :, :] = DR.plant((40, 36, 2), [[21.2, 17.4, 0.8], [18.1, 15.2, 0.1]], [1.0, 0.7], sigma, noise=0.002, seed=9)
    ref = TR.track(frames, pred, sigma, search)
    pos, amp, peak = gpu_track(frames, pred, sigma, search)
    np.testing.assert_array_equal(pos[:, :, 0], [[17, 16, 0], [17, 14, 0]])
    np.testing.assert_array_equal(ref["pstar"][:, :, 0], [[17, 16, 0], [17, 14, 0]])
    assert np.isnan(pos[:, :, 2]).all() and np.isnan(amp[:, 2]).all() and np.isnan(peak[:, 2]).all()
    assert np.isnan(ref["positions"][:, :, 2]).all()
    # frame 1: the scores within r = 5 of the NaN voxel are NaN, the plane x = 17 of both windows among them -- the plane that
    # wins the constant frame; the pick is the lowest index among the others
    np.testing.assert_array_equal(ref["pstar"][:, :, 1], [[18, 16, 0], [18, 14, 0]])
    np.testing.assert_array_equal(np.rint(pos[:, :, 1]), ref["pstar"][:, :, 1])
    np.testing.assert_allclose(peak[:, 1], ref["peaks"][:, 1], rtol=1e-3)
    # frame 3 comes after the NaN frame
    np.testing.assert_array_equal(np.rint(pos[:, :, 3]), ref["pstar"][:, :, 3])
    np.testing.assert_allclose(pos[:, :, 3], ref["positions"][:, :, 3], atol=1e-3)
    np.testing.assert_allclose(amp[:, 3], ref["amplitudes"][:, 3], rtol=1e-3)


def raw_call(rows, sz, T, pred, per_frame, sigma, search, want_amp=True, want_peak=True, guard=5):
    """The C entry itself on output buffers with ``guard`` canary values (-7) on either side."""
    from dnmf_amd import _lib
    lib = _lib.load()
    K = pred.shape[0]
    pos = torch.full((guard + K * 3 * T + guard,), -7.0, dtype=torch.float64, device="cuda")
    amp = torch.full((guard + K * T + guard,), -7.0, device="cuda")
    peak = torch.full((guard + K * T + guard,), -7.0, device="cuda")
    I3 = ctypes.c_int * 3
    rc = lib.dnmf_track_neurons(rows.data_ptr(), rows.stride(0), I3(*sz), T, None, pred.data_ptr(), int(pred.dtype == torch.float64),
                                int(per_frame), K, sigma, I3(*search), 0.0, None, pos[guard:].data_ptr(),
                                amp[guard:].data_ptr() if want_amp else None, peak[guard:].data_ptr() if want_peak else None,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, lib.dnmf_last_error(), pos.cpu().numpy(), amp.cpu().numpy(), peak.cpu().numpy()


def test_predict_forms_and_canaries():
    """(K,3) against (K,3,T) repeated, fp32 against fp64: bit-identical; amplitudes and peaks NULL: the positions unchanged;
    nothing is written around any output buffer."""
    frames, rest, _, _, sigma, search = TR.moving_case(1)
    T, sz = frames.shape[0], frames.shape[1:]
    K, g = rest.shape[0], 5
    rows = rows_of(frames)
    p64 = torch.from_numpy(rest.astype(np.float32).astype(np.float64)).cuda()      # values both formats hold
    forms = [(p64, False), (p64.float(), False), (p64[:, :, None].repeat(1, 1, T).contiguous(), True),
             (p64.float()[:, :, None].repeat(1, 1, T).contiguous(), True)]
    outs = [raw_call(rows, sz, T, p, per, sigma, search) for p, per in forms]
    for rc, _, pos, amp, peak in outs:
        assert rc == 0
        assert (pos[:g] == -7).all() and (pos[-g:] == -7).all() and (amp[:g] == -7).all() and (amp[-g:] == -7).all()
        assert (peak[:g] == -7).all() and (peak[-g:] == -7).all()
        assert np.isfinite(pos[g:-g]).all() and np.isfinite(amp[g:-g]).all() and np.isfinite(peak[g:-g]).all()
        for a, b in zip((pos, amp, peak), outs[0][2:]):
            np.testing.assert_array_equal(a, b)
    rc, _, pos, amp, peak = raw_call(rows, sz, T, p64, False, sigma, search, want_amp=False, want_peak=False)
    assert rc == 0 and (amp == -7).all() and (peak == -7).all()
    np.testing.assert_array_equal(pos, outs[0][2])
    rc, _, pos, amp, peak = raw_call(rows, sz, T, p64, False, sigma, search, want_amp=False)
    assert rc == 0 and (amp == -7).all()
    np.testing.assert_array_equal(peak, outs[0][4])
    ref = TR.track(frames, p64.cpu().numpy(), sigma, search)
    np.testing.assert_allclose(outs[0][2][g:-g].reshape(K, 3, T), ref["positions"], atol=1e-3)


def test_region_over_the_lds_budget_is_refused_before_any_launch():
    sz, T = (64, 64, 4), 2
    rows = torch.zeros((T, 64 * 64 * 4), device="cuda")
    pred = torch.full((2, 3), 30.0, dtype=torch.float64, device="cuda")
    rc, text, pos, amp, peak = raw_call(rows, sz, T, pred, False, 8.0, (12, 12, 1))
    assert rc == -3 and b"64 x 64 x 4" in text
    assert (pos == -7).all() and (amp == -7).all() and (peak == -7).all()
    from dnmf_amd import _lib, ops
    with pytest.raises(_lib.DnmfHipError, match="LDS"):
        ops.track_neurons(rows, sz, pred, shape_std=8.0, search=(12, 12, 1))
    with pytest.raises(ValueError, match="times"):
        ops.track_neurons(rows, sz, pred, times=[0, 2])
    with pytest.raises(ValueError, match="search"):
        ops.track_neurons(rows, sz, pred, search=(1, -1, 0))
    # the same volume with a region that fits runs
    pos, amp, peak = ops.track_neurons(rows, sz, pred, shape_std=2.0, search=(3, 3, 1))
    assert np.isnan(pos.cpu().numpy()).all()          # a zero frame: no score above the threshold 0


def test_public_entry_points():
    from dnmf_amd import ops
    from dnmf_amd.Demix.dNMF import DeformableNMF, ExponentialFP, ResidentLoader
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect
    sz, K, T, sigma = (32, 32, 2), 4, 5, 2.0
    rng = np.random.RandomState(11)
    rest = np.array([[8.0, 8.0, 0.0], [8.0, 23.0, 1.0], [23.0, 8.0, 1.0], [23.0, 23.0, 0.0]])
    truth = rest[:, :, None] + rng.uniform(-1, 1, (K, 3, T)) * np.array([2.0, 2.0, 0.0])[None, :, None]
    video = np.stack([DR.plant(sz, truth[:, :, t], 0.9 ** np.arange(K), sigma, noise=0.002, seed=70 + t) for t in range(T)])
    # numpy in, numpy out; CUDA in, CUDA out; resident rows
    pos, amp = ExponentialFP.track_positions(video, rest, shape_std=sigma, search=(3, 3, 0))
    assert isinstance(pos, np.ndarray) and pos.dtype == np.float64 and pos.shape == (K, 3, T) and amp.shape == (K, T)
    assert np.abs(pos[:, :2] - truth[:, :2]).max() <= 0.25
    vt = torch.from_numpy(video).cuda()
    pos_t, amp_t = ExponentialFP.track_positions(vt, torch.from_numpy(rest).cuda(), shape_std=sigma, search=(3, 3, 0))
    assert pos_t.is_cuda and amp_t.is_cuda and pos_t.dtype == torch.float64
    np.testing.assert_array_equal(pos_t.cpu().numpy(), pos)
    pos_r, _ = ExponentialFP.track_positions((vt.reshape(T, -1), sz), rest, shape_std=sigma, search=(3, 3, 0))
    np.testing.assert_array_equal(pos_r.cpu().numpy(), pos)
    pos_p, _ = ExponentialFP.track_positions(video, rest, shape_std=sigma, search=(1, 1, 0), predict=np.rint(truth))
    np.testing.assert_allclose(pos_p, pos, atol=1e-6)
    # the model's own tracker feeds init_motion unchanged
    torch.manual_seed(0)
    dn = DeformableNMF(torch.tensor(sz), K, T, positions=torch.from_numpy(rest).float())
    dn.verbose = False
    P_T, A_T = dn.track(ResidentLoader(vt, sz, T), search=(3, 3, 0))
    assert P_T.is_cuda and tuple(P_T.shape) == (K, 3, T) and P_T.dtype == torch.float64
    # fp.sigma is the constructor's 3, not the planted 2: a wider filter finds the same blobs
    assert np.abs(P_T.cpu().numpy()[:, :2] - truth[:, :2]).max() <= 0.5
    ok = dn.init_motion(P_T, order='affine', ridge=1e-3)
    assert bool(ok.all())
    where = dn.positions()
    assert where.shape == (K, 3, T) and np.isfinite(where).all()
    P_M, _ = dn.track(video, search=(2, 2, 0), predict='model')
    assert isinstance(P_M, np.ndarray) and P_M.shape == (K, 3, T) and np.isfinite(P_M).any()
    with pytest.raises(ValueError, match="predict"):
        dn.track(video, predict='warp')
    # MotionCorrect: the predictor is apply_shifts_points when piecewise shifts are stored, else the points
    mc = MotionCorrect(video, max_shifts=(3, 3, 1), strides=(12, 12, 1), overlaps=(6, 6, 1), max_deviation_rigid=2, is3D=True,
                       pw_rigid=True)
    plain, _ = mc.track_points(video, rest, shape_std=sigma)
    direct, _, _ = ops.track_neurons(vt.reshape(T, -1), sz, torch.from_numpy(rest).cuda(), shape_std=sigma, search=(3, 3, 1))
    np.testing.assert_array_equal(plain, direct.cpu().numpy())
    mc.min_mov = float(video.min())
    mc.motion_correct_pwrigid(template=video[0])
    got, amp = mc.track_points(video, rest, shape_std=sigma)
    assert got.dtype == np.float64 and got.shape == (K, 3, T) and amp.shape == (K, T)
    pred = torch.from_numpy(mc.apply_shifts_points(video, rest)).cuda()
    direct, damp, _ = ops.track_neurons(vt.reshape(T, -1), sz, pred, shape_std=sigma, search=(3, 3, 1))
    np.testing.assert_array_equal(got, direct.cpu().numpy())
    np.testing.assert_array_equal(amp, damp.cpu().numpy())
    with pytest.raises(NotImplementedError):
        MotionCorrect(video[..., 0], is3D=False).track_points(video[..., 0], rest)
