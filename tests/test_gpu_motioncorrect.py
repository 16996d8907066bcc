"""K8, the position initialiser: dnmf_register_patches / dnmf_apply_shifts_points and the
MotionCorrect-shaped front end against oracle/motion_oracle.py, a numpy restatement of the reference's
Demix/MotionCorrect.py (register_translation_3d :648-797, _upsampled_dft :498-614, sliding_window_3d :1190-1221,
tile_and_correct_3d :1518-1608, apply_shifts_points :351-371).

**Parity unpinned**: the reference module cannot be imported here (cv2 / skimage / past absent, np.int) and holds no
fixture; these tests pin the HIP path to the restatement only.  The shifts are quantised to 1 / upsample_factor = 0.1
voxel; the GPU works in fp32 where the restatement (like the reference) uses complex128, so a shift may land in the
neighbouring bin where two bins of the upsampled correlation tie to ~1e-6: the tests ask for identical shifts in at
least 97 % of the patches and never more than one bin apart.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def MO():
    from oracle import motion_oracle
    return motion_oracle


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def synthetic_video(sz, T, K, seed, piecewise=True, amp=2.5):
    """Gaussian blobs on a dim background; frame t = the template moved by a smooth, piecewise different displacement
    (one shift per quadrant of the volume, blended) of up to ~amp + 1 voxels in x, y and a fraction of a slice in z."""
    rng = np.random.RandomState(seed)
    X, Y, Z = sz
    gx, gy, gz = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    pos = rng.rand(K, 3) * np.array([X, Y, Z])

    def render(shift_of):
        v = np.full(sz, 0.02)
        for k in range(K):
            d = shift_of(pos[k])
            v += np.exp(-(((gx - pos[k, 0] - d[0]) / 2.5) ** 2 + ((gy - pos[k, 1] - d[1]) / 2.5) ** 2 + ((gz - pos[k, 2] - d[2]) / 1.5) ** 2))
        return v

    template = render(lambda p: np.zeros(3))
    video, truth = [], []
    for t in range(T):
        base = rng.uniform(-amp, amp, 3) * np.array([1, 1, 0.15])
        quad = rng.uniform(-1.0, 1.0, (2, 2, 3)) * np.array([1, 1, 0.0]) if piecewise else np.zeros((2, 2, 3))

        def shift_of(p, base=base, quad=quad):
            return base + quad[int(p[0] >= X / 2), int(p[1] >= Y / 2)]

        video.append(render(shift_of) + 0.002 * rng.randn(*sz))
        truth.append((base, quad))
    return np.array(video, dtype=np.float32), template.astype(np.float32), pos, truth


@pytest.mark.parametrize("sz,strides,overlaps,max_shifts", [
    ([48, 40, 2], (16, 12, 1), (8, 8, 1), (5, 5, 1)),       # two slices like the reference's demo volume
    ([40, 36, 5], (12, 12, 2), (8, 6, 1), (6, 4, 2)),       # odd sizes, several patch layers in z
    ([64, 64, 1], (24, 24, 1), (8, 8, 0), (6, 6, 0)),       # a single slice
])
def test_register_patches_vs_oracle(ops, MO, sz, strides, overlaps, max_shifts):
    T = 6
    video, template, _, _ = synthetic_video(sz, T, 40, seed=sum(sz))
    add = -float(video.min())
    sx, sy, sz_, rig = MO.pw_rigid_shifts(video, template, strides, overlaps, max_shifts, 10, 3, add)
    frames = torch.from_numpy(video.reshape(T, -1)).cuda()
    rigid, patch = ops.register_patches(frames, torch.from_numpy(template).cuda(), sz, strides, overlaps, max_shifts, 3, 10, add)
    dims, starts = ops.patch_grid(sz, strides, overlaps)
    ref_grid = MO.sliding_window_3d(sz, overlaps, strides)
    assert len(starts) == len(ref_grid) == sx.shape[1]
    np.testing.assert_array_equal(starts, np.array([g[3:6] for g in ref_grid]))
    np.testing.assert_array_equal(dims, np.array(ref_grid[-1][:3]) + 1)
    got = patch.cpu().numpy().astype(np.float64)
    ref = np.stack([sx, sy, sz_], 2)
    bins = np.abs(got - ref) * 10
    assert bins.max() <= 1.0 + 1e-3, bins.max()                       # never more than one bin of 0.1 voxel apart
    assert (bins < 1e-3).mean() >= 0.97, (bins < 1e-3).mean()
    rbins = np.abs(rigid.cpu().numpy() - rig) * 10
    assert rbins.max() <= 1.0 + 1e-3 and (rbins < 1e-3).mean() >= 0.9
    # the shifts are not trivial: the video moves by voxels
    assert np.abs(ref[..., :2]).max() > 1.0


def test_known_piecewise_shifts_are_recovered(ops):
    """A video built from known displacements: the recovered patch shifts follow them to within a few tenths of a voxel
    (the registration of a patch that holds blobs from two quadrants is a blend), and frame-to-frame position changes of
    points inside one quadrant match the truth."""
    sz, T = [64, 64, 2], 8
    video, template, pos, truth = synthetic_video(sz, T, 60, seed=5, piecewise=False)
    frames = torch.from_numpy(video.reshape(T, -1)).cuda()
    rigid, patch = ops.register_patches(frames, torch.from_numpy(template).cuda(), sz, (16, 16, 1), (16, 16, 1), (5, 5, 1), 3, 10,
                                        -float(video.min()))
    rigid = rigid.cpu().numpy()
    for t in range(T):
        base = truth[t][0]
        # src = frame, target = template: the shift that registers the template with the frame = the frame's displacement
        np.testing.assert_allclose(rigid[t, :2], base[:2], atol=0.3)
    p = patch.cpu().numpy()
    for t in range(T):   # every patch sees the same rigid displacement; total_shifts = (-x, -y, +z).  (A 32 x 32 x 2 patch holds a
        # handful of blobs, some cut by its border, and its circular correlation is biased by a few tenths of a voxel.)
        for d in range(2):
            assert abs(np.median(p[t, :, d]) + truth[t][0][d]) <= 0.3, (t, d)
            np.testing.assert_allclose(p[t, :, d], -truth[t][0][d], atol=1.0)


def test_motioncorrect_front_end_and_apply_shifts_points(ops, MO):
    """The class surface (reference MotionCorrect.py:64-385): motion_correct_pwrigid fills x/y/z_shifts_els, apply_shifts_points
    returns (K,3,T) positions equal to the oracle's on the same shift tables, and DeformableNMF accepts the first frame's
    positions."""
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect
    from dnmf_amd.Demix import dNMF as M
    sz, T, K = [48, 40, 2], 5, 12
    video, template, pos, _ = synthetic_video(sz, T, 30, seed=9)
    mc = MotionCorrect(video, max_shifts=(5, 5, 1), strides=(16, 12, 1), overlaps=(8, 8, 1), max_deviation_rigid=3, is3D=True,
                       pw_rigid=True)
    mc.motion_correct(template=template)
    assert len(mc.x_shifts_els) == len(mc.y_shifts_els) == len(mc.z_shifts_els) == T
    NP = len(MO.sliding_window_3d(sz, mc.overlaps, mc.strides))
    assert mc.x_shifts_els[0].shape == (NP,) and mc.border_to_0 >= 1
    points = np.random.RandomState(1).rand(K, 3) * np.array(sz)
    P_T = mc.apply_shifts_points(video, points)
    ref = MO.apply_shifts_points(np.stack(mc.x_shifts_els), np.stack(mc.y_shifts_els), np.stack(mc.z_shifts_els), sz, mc.overlaps,
                                 mc.strides, points)
    assert P_T.shape == (K, 3, T)
    np.testing.assert_allclose(P_T, ref, rtol=0, atol=2e-5)
    np.testing.assert_allclose(P_T[:, :, 0], points, atol=1e-5)       # frame 0 is the reference frame
    A = mc.apply_shifts_frame(video, points, 2)          # reference :330-349: frame 2's shifts added, all signs +
    idx = ((MO.patch_centers(sz, mc.overlaps, mc.strides)[:, None, :] - points[None]) ** 2).sum(2).argmin(0)
    expect = points + np.stack([mc.x_shifts_els[2][idx], mc.y_shifts_els[2][idx], mc.z_shifts_els[2][idx]], 1)
    np.testing.assert_allclose(A, expect, atol=1e-6)
    dn = M.DeformableNMF(torch.tensor(sz), K, T, positions=torch.from_numpy(P_T[:, :, 0]).float())
    assert tuple(dn.fp.A.shape) == (*sz, K)
    with pytest.raises(NotImplementedError):
        MotionCorrect(video[..., 0], is3D=False).apply_shifts_points(video, points)


@pytest.mark.parametrize("sz,max_shifts", [([48, 40, 2], (5, 5, 1)), ([40, 36, 5], (6, 4, 2)), ([64, 64, 1], (6, 6, 0))])
def test_rigid_correction_vs_oracle(ops, MO, sz, max_shifts):
    """dnmf_rigid_correct against the restatement of tile_and_correct_3d's rigid branch + apply_shifts_dft (:1518-1574,
    :1028-1157): same shifts (to a bin of 0.1 voxel), the frames moved through their spectra equal to 2e-4 of the frame's
    range where both are finite (fp32 transforms against complex128), the same NaN borders -- including the reference's
    pairing of the border of axis 0 with the shift of axis 1 -- and the NaN-aware sums behind the next template."""
    T = 6
    video, template, _, _ = synthetic_video(sz, T, 40, seed=sum(sz) + 1, piecewise=False)
    add = float(np.float32(-video.min()))
    ref_frames, ref_shifts = [], []
    for img in video:
        f, sh = MO.rigid_correct_3d(img, template, max_shifts, 10, add, True)
        ref_frames.append(f), ref_shifts.append(sh)
    ref_frames, ref_shifts = np.array(ref_frames), -np.array(ref_shifts)
    frames = torch.from_numpy(video.reshape(T, -1)).cuda()
    rigid, out, tsum, tcount = ops.rigid_correct(frames, torch.from_numpy(template).cuda(), sz, max_shifts, 10, add, True, want_frames=True)
    rigid, out = rigid.cpu().numpy(), out.cpu().numpy().reshape(T, *sz)
    same = np.abs(rigid - ref_shifts).max(1) < 1e-3
    assert same.mean() >= 0.8 and np.abs(rigid - ref_shifts).max() <= 0.1 + 1e-3
    assert np.abs(ref_shifts[:, :2]).max() > 1.0
    scale = float(video.max() - video.min())
    for t in np.flatnonzero(same):
        np.testing.assert_array_equal(np.isnan(out[t]), np.isnan(ref_frames[t]), err_msg=str(t))
        ok = ~np.isnan(out[t])
        assert ok.any()
        np.testing.assert_allclose(out[t][ok], ref_frames[t][ok], rtol=0, atol=2e-4 * scale, err_msg=str(t))
    np.testing.assert_array_equal(tcount.cpu().numpy().reshape(sz), (~np.isnan(out)).sum(0))
    np.testing.assert_allclose(tsum.cpu().numpy().reshape(sz), np.nansum(out, 0), rtol=1e-5, atol=1e-5)
    # a frame moved by its own shift lines up with the template: the registration of the corrected frame is ~zero
    filled = np.where(np.isnan(out), template[None], out).astype(np.float32)
    r2, _, _, _ = ops.rigid_correct(torch.from_numpy(filled.reshape(T, -1)).cuda(), torch.from_numpy(template).cuda(), sz, max_shifts,
                                    10, add, True)
    assert np.abs(r2.cpu().numpy()).max() <= 0.3


def test_motioncorrect_without_a_template(ops, MO):
    """template=None (reference :298-301): the rigid pre-pass builds the template -- the binned median, one rigid
    correction of every frame against it, the NaN-aware mean of the moved frames -- and the piecewise pass starts from
    there.  Against oracle.rigid_template on the same video; then the class with pw_rigid=False (rigid only)."""
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect
    sz, T = [48, 40, 2], 23            # 23 frames: two bins of ten, three frames left out of the first template
    video, _, _, _ = synthetic_video(sz, T, 30, seed=21, piecewise=False)
    templ, shifts, moved = MO.rigid_template(video, (5, 5, 1), add_to_movie=-float(video.min()))
    mc = MotionCorrect(video, max_shifts=(5, 5, 1), strides=(16, 12, 1), overlaps=(8, 8, 1), is3D=True, pw_rigid=False,
                       save_corrected=True)
    mc.motion_correct()
    got = np.array(mc.shifts_rig)
    assert got.shape == (T, 3)
    bins = np.abs(got - shifts) * 10
    assert bins.max() <= 1.0 + 1e-3 and (bins < 1e-3).mean() >= 0.85
    scale = float(video.max() - video.min())
    # (a frame whose shift landed in the neighbouring bin moves the mean by 0.1 voxel / T of a gradient)
    np.testing.assert_allclose(mc.total_template_rig, templ, rtol=0, atol=5e-3 * scale)
    assert np.abs(mc.total_template_rig - templ).mean() <= 2e-4 * scale
    assert mc.mc[0].shape == (*sz, T) and mc.border_to_0 >= 1
    same = np.flatnonzero(bins.max(1) < 1e-3)
    t = int(same[0])
    ok = ~np.isnan(moved[t])
    np.testing.assert_allclose(mc.mc[0][..., t][ok], moved[t][ok], atol=2e-4 * scale)
    first = mc._bin_median_3d(torch.from_numpy(video.reshape(T, -1)).cuda()).cpu().numpy().reshape(sz)
    np.testing.assert_allclose(first, MO.bin_median_3d(video), rtol=1e-6, atol=1e-7)
    # the piecewise pass on top of it
    mc2 = MotionCorrect(video, max_shifts=(5, 5, 1), strides=(16, 12, 1), overlaps=(8, 8, 1), is3D=True, pw_rigid=True)
    mc2.motion_correct()
    np.testing.assert_allclose(mc2.total_template_els.cpu().numpy(), mc.total_template_rig, atol=1e-6)
    sx, sy, sz_, _ = MO.pw_rigid_shifts(video, mc.total_template_rig, (16, 12, 1), (8, 8, 1), (5, 5, 1), 10, 3, -float(video.min()))
    pb = np.abs(np.stack(mc2.x_shifts_els) - sx) * 10
    assert pb.max() <= 1.0 + 1e-3 and (pb < 1e-3).mean() >= 0.95


@pytest.mark.parametrize("border", [False, "min", "copy"])
def test_rigid_correction_border_modes(ops, MO, border):
    """border_nan False / 'min' / 'copy' of apply_shifts_dft (:1098-1145) against the restatement."""
    sz, max_shifts, T = [40, 36, 5], (6, 4, 2), 5
    video, template, _, _ = synthetic_video(sz, T, 40, seed=77, piecewise=False)
    add = float(np.float32(-video.min()))
    ref = [MO.rigid_correct_3d(img, template, max_shifts, 10, add, border) for img in video]
    frames = torch.from_numpy(video.reshape(T, -1)).cuda()
    rigid, out, tsum, tcount = ops.rigid_correct(frames, torch.from_numpy(template).cuda(), sz, max_shifts, 10, add, border, want_frames=True)
    rigid, out = rigid.cpu().numpy(), out.cpu().numpy().reshape(T, *sz)
    scale = float(video.max() - video.min())
    checked = 0
    for t in range(T):
        if np.abs(rigid[t] + np.array(ref[t][1])).max() > 1e-3:      # (ref holds the flipped sign)
            continue
        assert not np.isnan(out[t]).any()
        np.testing.assert_allclose(out[t], ref[t][0], rtol=0, atol=3e-4 * scale, err_msg=str(t))
        checked += 1
    assert checked >= 3
    assert int(tcount.min()) == T


def test_two_dimensional_video(ops, MO):
    """is3D=False: a (T, X, Y) video through register_translation / tile_and_correct (reference :801-1024, :1272-1418) =
    the same kernels on one slice; x_shifts_els / y_shifts_els against oracle.tile_shifts_2d."""
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect
    sz, T = [64, 56, 1], 5
    video, template, _, _ = synthetic_video(sz, T, 40, seed=31)
    video2, template2 = video[..., 0], template[..., 0]
    mc = MotionCorrect(video2, max_shifts=(6, 6), strides=(24, 20), overlaps=(8, 8), max_deviation_rigid=3, is3D=False, pw_rigid=True)
    mc.motion_correct(template=template2)
    assert not hasattr(mc, "z_shifts_els") and len(mc.x_shifts_els) == T and len(mc.coord_shifts_els[0][0]) == 2
    ref = np.array([MO.tile_shifts_2d(img, template2, (24, 20), (8, 8), (6, 6), 10, 3, -float(video2.min()))[1] for img in video2])
    got = np.stack([np.stack(mc.x_shifts_els), np.stack(mc.y_shifts_els)], 2)
    bins = np.abs(got - ref) * 10
    assert bins.max() <= 1.0 + 1e-3 and (bins < 1e-3).mean() >= 0.95
    assert np.abs(ref).max() > 1.0 and tuple(mc.total_template_els.shape) == (64, 56)
    with pytest.raises(NotImplementedError):
        mc.motion_correct_rigid()


def test_matrix_pipe_kernel_equals_the_vector_kernel(ops):
    """K8's axis transform runs as f32 MFMAs (mc_axis_mfma_kernel); valu=True selects the vector-ALU kernel it replaced.
    Same shifts (a bin apart at most, 98 % identical: the sums over j run in a different order) and the same moved frames to
    1e-5 of the range, on a volume with odd sizes, a patch grid and every pass (forward, windowed inverse, upsampled inverse,
    the full inverse on a shifted grid)."""
    sz, T = [72, 50, 3], 6
    video, template, _, _ = synthetic_video(sz, T, 40, seed=12)
    frames, tm = torch.from_numpy(video.reshape(T, -1)).cuda(), torch.from_numpy(template).cuda()
    add = -float(video.min())
    res = {}
    for mode in ("0", "1"):
        rigid, patch = ops.register_patches(frames, tm, sz, (20, 14, 2), (10, 8, 1), (6, 5, 1), 3, 10, add, valu=mode == "1")
        r2, out, _, _ = ops.rigid_correct(frames, tm, sz, (6, 5, 1), 10, add, False, want_frames=True, valu=mode == "1")
        res[mode] = (rigid.cpu().numpy(), patch.cpu().numpy(), r2.cpu().numpy(), out.cpu().numpy())
    for a, b in zip(res["0"][:3], res["1"][:3]):
        assert np.abs(a - b).max() <= 0.1 + 1e-4 and (np.abs(a - b) < 1e-4).mean() >= 0.98
    same = np.abs(res["0"][2] - res["1"][2]).max(1) < 1e-4
    scale = float(video.max() - video.min())
    np.testing.assert_allclose(res["0"][3][same], res["1"][3][same], rtol=0, atol=1e-5 * scale)


# ---- K8 off the beaten path: short axes, window edges, other upsample factors, chunks, and its workspace ------------------

def sparse_video(sz, T, K, seed, amp=2.5):
    """synthetic_video for large volumes: every blob is drawn into an 18 x 18 window around its centre (the Gaussians of
    synthetic_video are < 1e-5 beyond it), so a 512 x 512 x 2 frame takes a few milliseconds."""
    rng = np.random.RandomState(seed)
    X, Y, Z = sz
    pos = rng.rand(K, 3) * np.array([X, Y, Z])
    gz = np.arange(Z)

    def render(shift_of):
        v = np.full(sz, 0.02)
        for k in range(K):
            c = pos[k] + shift_of(pos[k])
            xs, ys = np.arange(int(c[0]) - 8, int(c[0]) + 10), np.arange(int(c[1]) - 8, int(c[1]) + 10)
            xs, ys = xs[(xs >= 0) & (xs < X)], ys[(ys >= 0) & (ys < Y)]
            v[np.ix_(xs, ys, gz)] += (np.exp(-((xs - c[0]) / 2.5) ** 2)[:, None, None] * np.exp(-((ys - c[1]) / 2.5) ** 2)[None, :, None]
                                      * np.exp(-((gz - c[2]) / 1.5) ** 2)[None, None, :])
        return v

    template = render(lambda p: np.zeros(3))
    video = []
    for t in range(T):
        base = rng.uniform(-amp, amp, 3) * np.array([1, 1, 0.15])
        quad = rng.uniform(-1.0, 1.0, (2, 2, 3)) * np.array([1, 1, 0.0])
        video.append(render(lambda p: base + quad[int(p[0] >= X / 2), int(p[1] >= Y / 2)]) + 0.002 * rng.randn(*sz))
    return np.array(video, dtype=np.float32), template.astype(np.float32)


def assert_bins(got, ref, uf, same=0.97, what=""):
    """Shifts quantised to 1 / uf: never more than one bin apart, at least `same` of them identical.  Returns that fraction."""
    bins = np.abs(np.asarray(got, np.float64) - ref) * uf
    frac = float((bins < 1e-3).mean())
    assert bins.max() <= 1.0 + 1e-3, (what, bins.max())
    assert frac >= same, (what, frac)
    return frac


def check_patches(ops, MO, video, template, sz, strides, overlaps, max_shifts, uf=10, dev=3):
    """register_patches against oracle.pw_rigid_shifts with the bin criteria of test_register_patches_vs_oracle; returns
    the oracle's rigid shifts."""
    T = video.shape[0]
    add = -float(video.min())
    sx, sy, sz_, rig = MO.pw_rigid_shifts(video, template, strides, overlaps, max_shifts, uf, dev, add)
    rigid, patch = ops.register_patches(torch.from_numpy(video.reshape(T, -1)).cuda(), torch.from_numpy(template).cuda(), sz, strides,
                                        overlaps, max_shifts, dev, uf, add)
    assert_bins(patch.cpu().numpy(), np.stack([sx, sy, sz_], 2), uf, 0.97, "patches")
    assert_bins(rigid.cpu().numpy(), rig, uf, 0.9, "rigid")
    return rig


def check_rigid(ops, MO, video, template, sz, max_shifts, uf=10):
    """rigid_correct against oracle.rigid_correct_3d as test_rigid_correction_vs_oracle checks it: shifts to a bin, moved frames
    to 2e-4 of the frame's range where both are finite, the same NaN borders, and the NaN-aware sums.  Returns the oracle's
    shifts."""
    T = video.shape[0]
    add = float(np.float32(-video.min()))
    ref = [MO.rigid_correct_3d(img, template, max_shifts, uf, add, True) for img in video]
    ref_frames, ref_shifts = np.array([r[0] for r in ref]), -np.array([r[1] for r in ref])
    rigid, out, tsum, tcount = ops.rigid_correct(torch.from_numpy(video.reshape(T, -1)).cuda(), torch.from_numpy(template).cuda(), sz,
                                                 max_shifts, uf, add, True, want_frames=True)
    rigid, out = rigid.cpu().numpy(), out.cpu().numpy().reshape(T, *sz)
    same = np.abs(rigid - ref_shifts).max(1) < 1e-3
    assert same.mean() >= 0.8 and np.abs(rigid - ref_shifts).max() <= 1.0 / uf + 1e-3, (rigid, ref_shifts)
    scale = float(video.max() - video.min())
    for t in np.flatnonzero(same):
        np.testing.assert_array_equal(np.isnan(out[t]), np.isnan(ref_frames[t]), err_msg=str(t))
        ok = ~np.isnan(out[t])
        assert ok.any()
        np.testing.assert_allclose(out[t][ok], ref_frames[t][ok], rtol=0, atol=2e-4 * scale, err_msg=str(t))
    np.testing.assert_array_equal(tcount.cpu().numpy().reshape(sz), (~np.isnan(out)).sum(0))
    np.testing.assert_allclose(tsum.cpu().numpy().reshape(sz), np.nansum(out, 0), rtol=1e-5, atol=1e-5)
    return ref_shifts


@pytest.mark.parametrize("valu", ["0", "1"])
@pytest.mark.parametrize("sz,strides,overlaps,max_shifts", [
    ([20, 20, 1], (8, 8, 1), (4, 4, 0), (3, 3, 0)),         # a small 2-D video: the volume and the patches below 32 voxels
    ([36, 20, 8], (12, 6, 4), (6, 4, 4), (4, 3, 2)),        # patches of 18 x 10 x 8
    ([40, 20, 3], (28, 12, 2), (12, 8, 1), (4, 3, 1)),      # one patch: the whole volume
])
def test_short_axes_register_patches_vs_oracle(ops, MO, monkeypatch, valu, sz, strides, overlaps, max_shifts):
    """Boxes whose second axis is shorter than the 32 kept window indices: the partial inverses hold (items, 32, 32, n2),
    more than the (items, 32, n1, n2) of a long axis.  Both axis kernels (ops.K8_VALU)."""
    monkeypatch.setattr(ops, "K8_VALU", valu == "1")
    video, template, _, _ = synthetic_video(sz, 6, 30, seed=sum(sz) + 3)
    rig = check_patches(ops, MO, video, template, sz, strides, overlaps, max_shifts)
    assert np.abs(rig[:, :2]).max() > 1.0


@pytest.mark.parametrize("valu", ["0", "1"])
@pytest.mark.parametrize("sz,max_shifts", [([64, 16, 4], (5, 3, 1)), ([20, 20, 1], (3, 3, 0)), ([40, 8, 16], (4, 2, 3))])
def test_short_axes_rigid_correct_vs_oracle(ops, MO, monkeypatch, valu, sz, max_shifts):
    monkeypatch.setattr(ops, "K8_VALU", valu == "1")
    video, template, _, _ = synthetic_video(sz, 6, 30, seed=sum(sz) + 4, piecewise=False)
    ref = check_rigid(ops, MO, video, template, sz, max_shifts)
    assert np.abs(ref[:, :2]).max() > 1.0


def test_short_two_dimensional_video(ops, MO):
    """A 20 x 20 video through MotionCorrect(is3D=False) against oracle.tile_shifts_2d."""
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect
    sz, T = [20, 20, 1], 6
    video, template, _, _ = synthetic_video(sz, T, 12, seed=44)
    video2, template2 = video[..., 0], template[..., 0]
    mc = MotionCorrect(video2, max_shifts=(3, 3), strides=(8, 8), overlaps=(4, 4), max_deviation_rigid=3, is3D=False, pw_rigid=True)
    mc.motion_correct(template=template2)
    ref = np.array([MO.tile_shifts_2d(img, template2, (8, 8), (4, 4), (3, 3), 10, 3, -float(video2.min()))[1] for img in video2])
    got = np.stack([np.stack(mc.x_shifts_els), np.stack(mc.y_shifts_els)], 2)
    assert_bins(got, ref, 10)
    assert np.abs(ref).max() > 1.0


def test_window_edges_vs_oracle(ops, MO):
    """Motion beyond max_shifts (the peak sits on the window's edge), max_shifts = 0 on an axis of 4 slices (numpy's cc[0:-0]
    is empty: the whole axis is searched), 2 max_shifts >= n on a 12-voxel axis (the whole axis again), and patches of 4
    voxels, narrower than |rigid| + max_deviation_rigid on either side (the clipped slices of the patch window)."""
    sz = [48, 40, 4]
    video, template, _, _ = synthetic_video(sz, 6, 40, seed=60, amp=6.0)
    rig = check_patches(ops, MO, video, template, sz, (16, 12, 2), (8, 8, 2), (3, 3, 0))
    assert (rig[:, :2] == -3).any() and (rig[:, :2] == 2).any()       # on both edges of the window [-3, 2]
    check_rigid(ops, MO, video, template, sz, (3, 3, 0))
    sz, dev = [40, 12, 3], 3
    video, template, _, _ = synthetic_video(sz, 8, 30, seed=61, amp=6.0)
    rig = check_patches(ops, MO, video, template, sz, (12, 2, 1), (8, 2, 1), (4, 6, 1), dev=dev)
    assert (rig[:, 1] + dev > 4).any() and (rig[:, 1] - dev < -4).any()
    check_rigid(ops, MO, video, template, sz, (4, 6, 1))


@pytest.mark.parametrize("uf", [1, 2, 3, 21])
def test_upsample_factors_vs_oracle(ops, MO, uf):
    """Upsample factors other than 10, against the oracle at the same factor; 21 gives the largest upsampled grid (32).  At
    factor 1 the reference keeps the integer peak of the window (no upsampled pass): with motion beyond max_shifts that
    peak is on the window's edge, and a grid around it would step outside."""
    sz = [48, 40, 2]
    amp, ms = (6.0, (3, 3, 1)) if uf == 1 else (2.5, (5, 5, 1))
    video, template, _, _ = synthetic_video(sz, 6, 40, seed=70 + uf, amp=amp)
    rig = check_patches(ops, MO, video, template, sz, (16, 12, 1), (8, 8, 1), ms, uf=uf)
    if uf == 1:
        assert (rig[:, :2] == -3).any()
    check_rigid(ops, MO, video, template, sz, ms, uf=uf)


def test_chunks_frame_ids_and_strides_at_full_size(ops, MO):
    """512 x 512 x 2, the size the README gives, with (24, 24, 1) + (8, 8, 1) patches: a video long enough for two chunks
    of dnmf_register_patches (the first length at which the workspace stops growing, plus three frames).  One call equals
    single-frame calls bit for bit; frame_ids over rows of a wider buffer (ldf > P) equal the permuted contiguous video
    bit for bit; the frames on both sides of the chunk boundary against the oracle; and the rigid correction across its own
    chunk boundary through frame_ids."""
    from dnmf_amd import _lib
    lib = _lib.load()
    import ctypes
    sz, strides, overlaps, ms = [512, 512, 2], (24, 24, 1), (8, 8, 1), (6, 6, 1)
    I3 = ctypes.c_int * 3
    ws = [lib.dnmf_register_patches_workspace(*sz, I3(*strides), I3(*overlaps), b) for b in range(1, 200)]
    Bc = next(b for b in range(1, 199) if ws[b] == ws[b - 1])          # ws[b] is for b + 1 frames
    B = Bc + 3
    P = 512 * 512 * 2
    video, template = sparse_video(sz, B, 1500, seed=8)
    add = -float(video.min())
    frames = torch.from_numpy(video.reshape(B, -1)).cuda()
    tm = torch.from_numpy(template).cuda()
    call = lambda f, ids=None: ops.register_patches(f, tm, sz, strides, overlaps, ms, 3, 10, add, frame_ids=ids)
    rigid, patch = call(frames)
    for t in range(B):
        r1, p1 = call(frames[t:t + 1])
        assert torch.equal(r1[0], rigid[t]) and torch.equal(p1[0], patch[t]), t
    perm = torch.from_numpy(np.random.RandomState(1).permutation(B)).cuda()
    wide = torch.full((B, P + 96), float("nan"), device="cuda")
    wide[:, :P] = frames
    rp, pp = call(wide[:, :P], perm.int())
    rc, pc = call(frames[perm].contiguous())
    assert torch.equal(rp, rc) and torch.equal(pp, pc)
    assert torch.equal(rc, rigid[perm]) and torch.equal(pc, patch[perm])
    # the oracle on both sides of the boundary
    near = np.arange(Bc - 3, Bc + 3)
    sx, sy, sz_, rig = MO.pw_rigid_shifts(video[near], template, strides, overlaps, ms, 10, 3, add)
    got = patch[torch.from_numpy(near).cuda()].cpu().numpy()
    frac = assert_bins(got, np.stack([sx, sy, sz_], 2), 10, 0.97, "patches at 512 x 512 x 2")
    print(f"\n512 x 512 x 2: {frac:.4f} of {got.size} patch shift components in the oracle's 0.1-voxel bin")
    assert_bins(rigid[torch.from_numpy(near).cuda()].cpu().numpy(), rig, 10, 0.9, "rigid at 512 x 512 x 2")
    # rigid correction: 64 frames per chunk at this size; rows 62..65 of a list of ids that cycles through the video
    ids = torch.arange(68, device="cuda", dtype=torch.int32) % B
    r_all, out_all, _, _ = ops.rigid_correct(frames, tm, sz, ms, 10, add, True, frame_ids=ids, want_frames=True)
    assert torch.equal(r_all[B:], r_all[:68 - B])
    rows = [62, 63, 64, 65]
    sub = video[[int(ids[r]) for r in rows]]
    ref = [MO.rigid_correct_3d(img, template, ms, 10, add, True) for img in sub]
    scale = float(video.max() - video.min())
    for k, r in enumerate(rows):
        if np.abs(r_all[r].cpu().numpy() + np.array(ref[k][1])).max() > 1e-3:
            assert np.abs(r_all[r].cpu().numpy() + np.array(ref[k][1])).max() <= 0.1 + 1e-3, r
            continue
        o = out_all[r].cpu().numpy().reshape(sz)
        np.testing.assert_array_equal(np.isnan(o), np.isnan(ref[k][0]), err_msg=str(r))
        ok = ~np.isnan(o)
        np.testing.assert_allclose(o[ok], ref[k][0][ok], rtol=0, atol=2e-4 * scale, err_msg=str(r))


@pytest.mark.parametrize("kind", ["patches", "rigid"])
def test_workspace_tail_untouched_and_unwritten_rows_unread(ops, kind):
    """The ABI called through _lib with need + 1 MiB of workspace: a sentinel in the last MiB survives, and a workspace of
    0xFF bytes (NaN everywhere) gives the same results, bit for bit, as a zeroed one -- nothing reads a row no pass wrote."""
    import ctypes
    from dnmf_amd import _lib
    lib = _lib.load()
    I3 = ctypes.c_int * 3
    sz = [36, 20, 8] if kind == "patches" else [64, 16, 4]
    T, P = 5, sz[0] * sz[1] * sz[2]
    video, template, _, _ = synthetic_video(sz, T, 30, seed=90)
    frames, tm = torch.from_numpy(video.reshape(T, -1)).cuda(), torch.from_numpy(template).cuda()
    add = -float(video.min())
    strides, overlaps, ms = I3(12, 6, 4), I3(6, 4, 4), I3(4, 3, 2)
    if kind == "patches":
        need = lib.dnmf_register_patches_workspace(*sz, strides, overlaps, T)
        NP = lib.dnmf_register_patches_grid(*sz, strides, overlaps, None, None)
    else:
        need = lib.dnmf_rigid_correct_workspace(*sz, T)
    tail = 1 << 20
    sentinel = torch.from_numpy(np.random.RandomState(3).randint(0, 256, tail).astype(np.uint8)).cuda()
    res = []
    for fill in (0x00, 0xFF):
        ws = torch.full((need + tail,), fill, dtype=torch.uint8, device="cuda")
        ws[need:] = sentinel
        rigid = torch.empty((T, 3), device="cuda")
        if kind == "patches":
            out = torch.empty((T, NP, 3), device="cuda")
            rc = lib.dnmf_register_patches(frames.data_ptr(), P, None, T, tm.data_ptr(), *sz, strides, overlaps, ms, 3, 10, add,
                                           rigid.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), 0, ops._stream())
        else:
            out = torch.empty((T, P), device="cuda")
            tsum, tcount = torch.zeros(P, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")
            rc = lib.dnmf_rigid_correct(frames.data_ptr(), P, None, T, tm.data_ptr(), *sz, I3(5, 3, 1), 10, add, 1, rigid.data_ptr(),
                                        out.data_ptr(), P, tsum.data_ptr(), tcount.data_ptr(), ws.data_ptr(), ws.numel(), 0, ops._stream())
        _lib.check(rc, kind)
        torch.cuda.synchronize()
        assert torch.equal(ws[need:], sentinel), fill
        res.append((rigid.cpu().numpy(), out.cpu().numpy()))
    for a, b in zip(res[0], res[1]):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
