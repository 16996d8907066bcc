"""K14 on the GPU against its float64 restatement (tests/detect_restatement.py), and the public entry points built on it."""
import ctypes

import numpy as np
import pytest
import torch

import detect_restatement as DR

pytestmark = pytest.mark.gpu


def gpu_detect(V, K, sigma, **kw):
    from dnmf_amd import ops
    pos, amp, count = ops.detect_neurons(torch.from_numpy(np.ascontiguousarray(V, dtype=np.float32)).cuda(), V.shape, K, shape_std=sigma,
                                         **kw)
    return pos.cpu().numpy().astype(np.float64), amp.cpu().numpy().astype(np.float64), int(count)


def compare(V, K, sigma, ref, got, upto):
    """The first ``upto`` picks: centre within 1e-3 voxel, amplitude at rtol 1e-3 -- fp32 rounding of a (2 r + 1)-term sum per
    axis, about 1e-5 relative, divided by the log-curvature 1 / sigma^2.  The kernel returns p^ only, so the integer voxel p*
    is compared through it: |delta| <= 1/2, so centres this close have the same p* unless delta is within 1e-3 of a half."""
    pos, amp, count = got
    assert np.nanmin(ref["margin"][:upto]) >= 1e-3             # a condition on the input, met by the restatement alone
    assert count >= upto
    dp = np.abs(pos[:upto] - ref["positions"][:upto]).max()
    da = np.abs(amp[:upto] / ref["amplitudes"][:upto] - 1).max()
    print(f"{V.shape} sigma {sigma}: count {count} (restatement {ref['count']}), max |p^ - p^_ref| {dp:.2e} voxel, max amplitude "
          f"deviation {da:.2e}")
    assert dp <= 1e-3
    assert da <= 1e-3
    assert np.isnan(pos[count:]).all() and np.isnan(amp[count:]).all()
    assert np.isfinite(pos[:count]).all() and np.isfinite(amp[:count]).all()


@pytest.mark.parametrize("case", range(len(DR.CASES)))
def test_gpu_equals_restatement_on_planted_gaussians(case):
    V, centres, amps, sigma, K = DR.planted_case(case)
    ref = DR.detect(V, K + DR.EXTRA, sigma)
    compare(V, K, sigma, ref, gpu_detect(V, K + DR.EXTRA, sigma), K)


def test_equal_scores_go_to_the_lowest_index():
    """Two single voxels of equal value, far apart and r = 6 or more from the border in x and y: each score is the one product
    tap(0)^3 * value (times weights of exactly 1), so the two are equal bit for bit; the first pick is the lower linear
    index, the second the other voxel."""
    V = np.zeros((40, 24, 2), dtype=np.float32)
    V[30, 15, 0] = V[7, 6, 1] = 0.75
    pos, amp, count = gpu_detect(V, 2, 2.0, background=0.0)
    assert count == 2
    np.testing.assert_array_equal(pos, [[7, 6, 1], [30, 15, 0]])
    ref = DR.detect(V, 2, 2.0, background=0.0)
    np.testing.assert_array_equal(ref["pstar"], [[7, 6, 1], [30, 15, 0]])
    np.testing.assert_allclose(amp, ref["amplitudes"], rtol=1e-5)


BORDER_SZ, BORDER_SIGMA = (30, 28, 2), 2.0


def border_case():
    X, Y, Z = BORDER_SZ
    centres = np.array([[0.3, 10.0, 0.0], [X - 1.0, Y - 1.4, Z - 1.0]])
    amps = np.array([1.0, 0.8])
    return DR.plant(BORDER_SZ, centres, amps, BORDER_SIGMA), centres, amps


def test_blob_cut_by_the_border_agrees_with_the_restatement():
    V, centres, amps = border_case()
    ref = DR.detect(V, 2, BORDER_SIGMA, background=0.0)
    compare(V, 2, BORDER_SIGMA, ref, gpu_detect(V, 2, BORDER_SIGMA, background=0.0), 2)


def test_blob_cut_by_the_border_amplitude_within_5_percent():
    """The amplitude of a blob cut by the border within 5 % of the planted one: it checks the truncated norm and, with it, the
    centre the norm is taken at -- picked and refined on the raw filter response the centres sit up to a voxel inside the
    volume and the amplitudes come out 9 % and 21 % low at this sigma; on the noise-normalised score the restatement gives
    1.000 and 0.971 of the planted ones."""
    V, centres, amps = border_case()
    pos, amp, count = gpu_detect(V, 2, BORDER_SIGMA, background=0.0)
    print(f"border blobs: centres {pos.tolist()}, amplitudes {amp.tolist()} for planted {amps.tolist()}")
    assert count == 2
    np.testing.assert_allclose(amp, amps, rtol=0.05)


def raw_call(V, K, sigma, rows, short=0, threshold=0.0):
    """The C entry itself on buffers of ``rows`` rows filled with a sentinel; ``short``: bytes the workspace is declared short."""
    from dnmf_amd import _lib
    lib = _lib.load()
    sz = (ctypes.c_int * 3)(*V.shape)
    need = lib.dnmf_detect_neurons_workspace(sz, K, sigma)
    img = torch.from_numpy(np.ascontiguousarray(V, dtype=np.float32)).cuda()
    pos = torch.full((rows, 3), -7.0, device="cuda")
    amp = torch.full((rows,), -7.0, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(((need + 3) // 4,), dtype=torch.float32, device="cuda")
    rc = lib.dnmf_detect_neurons(img.data_ptr(), sz, K, sigma, 2.0 * sigma, threshold, 0.0, pos.data_ptr(), amp.data_ptr(), count.data_ptr(),
                                 ws.data_ptr(), need - short, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, lib.dnmf_last_error(), pos.cpu().numpy(), amp.cpu().numpy(), int(count)


def test_fewer_blobs_than_asked_for():
    """Three blobs, eight asked for, a threshold at half the smallest planted score: three rows, five rows of NaN, and nothing
    written past row K."""
    sz, sigma = (44, 31, 2), 2.0
    centres = np.array([[9.3, 8.1, 0.2], [30.6, 20.4, 1.0], [12.8, 23.5, 0.6]])
    V = DR.plant(sz, centres, [1.0, 0.9, 0.81], sigma, noise=0.002, seed=5)
    free = DR.detect(V, 3, sigma, background=0.0)
    thr = 0.5 * float(free["peaks"].min())
    ref = DR.detect(V, 8, sigma, background=0.0, threshold=thr)
    assert ref["count"] == 3
    rc, _, pos, amp, count = raw_call(V, 8, sigma, rows=10, threshold=thr)
    assert rc == 0 and count == 3
    assert np.isnan(pos[3:8]).all() and np.isnan(amp[3:8]).all()
    assert (pos[8:] == -7.0).all() and (amp[8:] == -7.0).all()
    compare(V, 8, sigma, ref, (pos[:8].astype(np.float64), amp[:8].astype(np.float64), count), 3)


def test_short_workspace_is_refused_before_any_launch():
    V = DR.planted_case(0)[0]
    rc, text, pos, amp, count = raw_call(V, 4, 2.0, rows=4, short=1)
    assert rc == -4 and b"workspace" in text
    assert (pos == -7.0).all() and (amp == -7.0).all() and count == -7
    from dnmf_amd import _lib, ops
    with pytest.raises(ValueError):
        ops.detect_neurons(torch.zeros(8, 8, 1, device="cuda"), (8, 8, 1), 2, shape_std=0.0)
    with pytest.raises(_lib.DnmfHipError, match="background"):
        ops.detect_neurons(torch.zeros(8, 8, 1, device="cuda"), (8, 8, 1), 2, background=float("nan"))


def test_default_background_is_the_median_and_the_workspace_is_reused():
    from dnmf_amd import ops
    V, _, _, sigma, K = DR.planted_case(1)
    V = V + np.float32(3.5)
    ref = DR.detect(V, K, sigma)
    img = torch.from_numpy(V).cuda()
    ws = torch.empty((1 << 16,), dtype=torch.float32, device="cuda")
    pos, amp, count = ops.detect_neurons(img, V.shape, K, shape_std=sigma, workspace=ws)
    compare(V, K, sigma, ref, (pos.cpu().numpy().astype(np.float64), amp.cpu().numpy().astype(np.float64), int(count)), K)
    assert count.is_cuda and count.dtype == torch.int32 and pos.is_cuda and amp.is_cuda


def test_public_entry_points():
    from dnmf_amd.Demix.dNMF import DeformableNMF, ExponentialFP, SimulatedVideoDataset
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect
    V, centres, amps, sigma, K = DR.planted_case(0)
    pos, amp = ExponentialFP.detect_positions(V, K, shape_std=sigma)
    assert isinstance(pos, np.ndarray) and isinstance(amp, np.ndarray) and pos.shape == (K, 3) and amp.shape == (K,)
    pos_t, amp_t = ExponentialFP.detect_positions(torch.from_numpy(V).cuda(), K, shape_std=sigma)
    assert pos_t.is_cuda and amp_t.is_cuda
    np.testing.assert_array_equal(pos_t.cpu().numpy(), pos)
    dn = DeformableNMF.from_image(V, K + DR.EXTRA, 5, shape_std=sigma, threshold=0.5 * float(amps[-1]))
    assert dn.fp.K == K and tuple(dn.C.shape) == (K, 5) and tuple(dn.fp.beta.shape) == (10, 3, 5)
    np.testing.assert_array_equal(dn.fp.pos.cpu().numpy(), pos)
    assert float(dn.fp.sigma[0]) == sigma and tuple(dn.fp.A.shape) == V.shape + (K,)
    with pytest.raises(ValueError, match="no neuron"):
        DeformableNMF.from_image(V, 3, 5, shape_std=sigma, threshold=1e9)
    torch.manual_seed(0)
    np.random.seed(0)
    sz, T = torch.tensor([40, 36, 2]), 6
    ds = SimulatedVideoDataset(K=5, T=T, sz=sz, shape_std=3, density=.2, bg_snr=-120, traces='exp', motion='gp',
                               motion_par={'sigma': [2, 2, .01], 'ls': [10, 10, 10]})
    video = np.moveaxis(np.asarray(ds.video), -1, 0)
    mc = MotionCorrect(video, max_shifts=(5, 5, 1), strides=(16, 12, 1), overlaps=(8, 8, 1), max_deviation_rigid=3, is3D=True, pw_rigid=True)
    with pytest.raises(ValueError, match="template"):
        mc.detect_points(5)
    mc.motion_correct()
    pts = mc.detect_points(5, shape_std=3)
    assert pts.dtype == np.float64 and pts.ndim == 2 and pts.shape[1] == 3 and 1 <= len(pts) <= 5 and np.isfinite(pts).all()
    tracks = mc.apply_shifts_points(video, pts)
    assert tracks.shape == (len(pts), 3, T) and np.isfinite(tracks).all()
    with pytest.raises(NotImplementedError):
        MotionCorrect(video[..., 0], is3D=False).detect_points(5)
