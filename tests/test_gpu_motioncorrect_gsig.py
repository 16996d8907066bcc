"""``MotionCorrect(..., gSig_filt=...)``: registration on the high-pass-filtered frames (K22), the shifts applied to the
original frames.  The class against ``ops`` calls made by hand (bit for bit), against oracle/motion_oracle.py run on the
float64 definition's filtered frames (tests/high_pass_restatement.py), and the case the feature exists for."""
import functools

import numpy as np
import pytest
import torch

import high_pass_restatement as HR
from test_gpu_motioncorrect import synthetic_video

pytestmark = pytest.mark.gpu

# shape, strides, overlaps, max_shifts, seed (as tests/test_gpu_motioncorrect.py registers these shapes), gSig
COMPOSE = {
    "3d": ([48, 40, 2], (16, 12, 1), (8, 8, 1), (5, 5, 1), 90, 3),
    "2d": ([64, 56, 1], (24, 20), (8, 8), (6, 6), 31, 3),
}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


@pytest.fixture(scope="module")
def MO():
    from oracle import motion_oracle
    return motion_oracle


def p3(v, fill):
    return tuple(v) + (fill,) * (3 - len(v))


@functools.lru_cache(maxsize=None)
def compose_case(kind):
    """(video (T, X, Y, Z) fp32, the definition's filtered template fp32): computed once, never changed."""
    sz, _, _, _, seed, gsig = COMPOSE[kind]
    video, template, _, _ = synthetic_video(sz, 6, 40, seed=seed)
    tmpl = HR.filter_frames(template, HR.high_pass_taps(gsig))[0].astype(np.float32)
    video.setflags(write=False), tmpl.setflags(write=False)
    return video, tmpl


@functools.lru_cache(maxsize=None)
def planted(bg_amp=4.0, seed=7, sz=(48, 40, 2), K=14, shifts=((0, 0), (2, -3), (-3, 1), (3, 2), (-2, -2), (1, 3), (-3, -3), (2, 2))):
    """Small blobs (sigma 1.5) translating by known integer shifts of up to 3 voxels on a static smooth background -- a fixed
    Gaussian hump plus a ramp -- whose peak is 6.3 times a blob's: (video, background, shifts (T, 2))."""
    rng = np.random.RandomState(seed)
    X, Y, Z = sz
    gx, gy, gz = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    bg = bg_amp * (np.exp(-(((gx - 0.45 * X) / (0.35 * X)) ** 2 + ((gy - 0.55 * Y) / (0.35 * Y)) ** 2)) + 0.5 * gx / X + 0.25 * gy / Y + 0.2 * gz)
    pos = np.column_stack([rng.uniform(8, X - 8, K), rng.uniform(8, Y - 8, K), rng.uniform(0, Z - 1, K)])
    shifts = np.array(shifts)
    video = []
    for t in range(len(shifts)):
        v = bg.copy()
        for k in range(K):
            v += np.exp(-(((gx - pos[k, 0] - shifts[t, 0]) / 1.5) ** 2 + ((gy - pos[k, 1] - shifts[t, 1]) / 1.5) ** 2 + ((gz - pos[k, 2]) / 1.0) ** 2))
        video.append(v + 0.01 * rng.randn(*sz))
    video, bg = np.array(video, dtype=np.float32), bg.astype(np.float32)
    video.setflags(write=False), bg.setflags(write=False)
    return video, bg, shifts


RESTING = ((0, 0), (0, 0), (2, -3), (0, 0), (-3, 1), (0, 0), (3, 2), (0, 0), (-2, -2), (0, 0), (1, 3), (0, 0))


def test_constructor_takes_gsig_filt_and_still_refuses_dview(ops):
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect
    video = np.zeros((2, 8, 8, 1), np.float32)
    mc = MotionCorrect(video, gSig_filt=(3, 3))
    assert mc.gSig_filt == (3.0, 3.0) and mc.get_params()["gSig_filt"] == (3.0, 3.0)
    assert MotionCorrect(video).gSig_filt is None and MotionCorrect(video).get_params()["gSig_filt"] is None
    with pytest.raises(NotImplementedError, match="dview"):
        MotionCorrect(video, dview=object())
    with pytest.raises(NotImplementedError, match="dview"):
        MotionCorrect(video, dview=object(), gSig_filt=(3, 3))
    for bad in ((0, 3), (-1, -1), (float("nan"), 2)):
        with pytest.raises(ValueError):
            MotionCorrect(video, gSig_filt=bad)


@pytest.mark.parametrize("kind", ["3d", "2d"])
def test_pwrigid_is_k22_then_k8_then_k9_on_the_originals(ops, MO, kind):
    """The stored shifts are bit-equal to register_patches of high_pass_frames by hand; mc_els to apply_pwrigid of the ORIGINAL
    rows with those shifts; and the shifts agree with the oracle's tile shifts on the definition's filtered frames by K8's
    criterion (at most one 1/10-voxel bin anywhere, at least 95 % exact) -- as does, first, the oracle on K22's own frames."""
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect
    sz, strides, overlaps, ms, _, gsig = COMPOSE[kind]
    is3D = kind == "3d"
    video, tmpl = compose_case(kind)
    T, P = video.shape[0], int(np.prod(sz))
    vid = video if is3D else video[..., 0]
    mc = MotionCorrect(vid, max_shifts=ms, strides=strides, overlaps=overlaps, max_deviation_rigid=3, is3D=is3D, pw_rigid=True,
                       gSig_filt=(gsig, gsig), save_corrected=True)
    mc.motion_correct(template=tmpl if is3D else tmpl[..., 0])
    s3, o3, m3 = p3(strides, 1), p3(overlaps, 0), p3(ms, 0)
    add = -float(video.min())
    frames = torch.from_numpy(video.reshape(T, P)).cuda()
    filtered = ops.high_pass_frames(frames, sz, (gsig, gsig))
    _, patch = ops.register_patches(filtered, torch.from_numpy(tmpl).cuda(), sz, s3, o3, m3, 3, 10, add_to_movie=add)
    got = np.stack([np.stack(mc.x_shifts_els), np.stack(mc.y_shifts_els)] + ([np.stack(mc.z_shifts_els)] if is3D else []), 2)
    assert np.array_equal(got, patch.cpu().numpy()[..., :got.shape[2]])
    assert tuple(mc.total_template_els.shape) == tuple(sz if is3D else sz[:2])
    assert np.array_equal(mc.total_template_els.cpu().numpy().reshape(sz), tmpl)
    if is3D:
        moved, _, _ = ops.apply_pwrigid(frames, patch, sz, s3, o3, add_to_movie=float(np.float32(add)))
        assert np.array_equal(mc.mc_els[0], moved.view(T, *sz).permute(1, 2, 3, 0).cpu().numpy(), equal_nan=True)
    else:
        assert not hasattr(mc, "mc_els")

    # the oracle on the definition's frames, on K22's frames, and the class
    fdef = HR.filter_frames(video, HR.high_pass_taps(gsig))[0]
    fk22 = filtered.cpu().numpy().reshape(T, *sz)
    if is3D:
        ref, own = [np.stack(MO.pw_rigid_shifts(f, tmpl, strides, overlaps, ms, 10, 3, add)[:3], 2) for f in (fdef, fk22)]
    else:
        ref, own = [np.array([MO.tile_shifts_2d(img[..., 0], tmpl[..., 0], strides, overlaps, ms, 10, 3, add)[1] for img in f])
                    for f in (fdef, fk22)]
    for what, a in (("oracle on K22's frames", own), ("the class", got.astype(np.float64))):
        bins = np.abs(a - ref) * 10
        print(f"{kind} {what}: largest bin distance {bins.max():.3f}, exact {(bins < 1e-3).mean():.4f}")
        assert bins.max() <= 1.0 + 1e-3 and (bins < 1e-3).mean() >= 0.95, what
    assert np.abs(ref[..., :2]).max() > 1.0


def test_a_bright_static_background_needs_the_filter(ops):
    """Why the feature exists.  On the planted video (blobs moving by up to 3 voxels on a static background 6.3 times as bright),
    template = frame 0, the oracle's rigid shifts (register_translation_3d, upsampling 10, max_shifts (5, 5, 1)) miss the planted
    shifts by [0, 3, 3, 3, 2, 2.9, 3, 2] voxels (largest axis) on the raw frames -- 7 of 8 frames by more than 1 -- and by at most
    0.1 voxel on the definition's gSig 2 filtered frames.  The GPU class must show the same two facts."""
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect
    video, _, shifts = planted()
    errs = {}
    for gsig in (None, (2, 2)):
        tmpl = video[0] if gsig is None else HR.filter_frames(video[0], HR.high_pass_taps(2))[0].astype(np.float32)
        mc = MotionCorrect(video, max_shifts=(5, 5, 1), strides=(16, 12, 1), overlaps=(8, 8, 1), is3D=True, gSig_filt=gsig)
        mc.motion_correct_rigid(template=tmpl)
        got = -np.array(mc.shifts_rig)                       # shifts_rig holds the registration's shift with its sign flipped
        errs[gsig] = np.abs(got[:, :2] - shifts).max(1)
        print(f"gSig_filt={gsig}: shift errors per frame {np.round(errs[gsig], 2).tolist()}, z {np.abs(got[:, 2]).max()}")
    assert (errs[None] > 1.0).sum() > len(shifts) // 2       # most frames
    assert (errs[(2, 2)] <= 0.25).all()


def test_without_a_template(ops):
    """template=None with gSig_filt: the rigid pass measures on the filtered frames and moves the originals (K9), its template is
    the filtered NaN-aware mean of the moved originals -- rebuilt here from ops calls, bit for bit -- and mc keeps the background.
    The video rests in 7 of its 12 frames, so that the first template, the mean of the filtered frames (one bin of ten frames), has
    one dominant copy of every blob: on the CPU the oracle's shifts against bin_median_3d of the definition's frames are within 0.2
    voxel of the planted ones, both relative to their median."""
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect, high_pass_filter_space
    video, bg, shifts = planted(shifts=RESTING)
    T, sz = video.shape[0], list(video.shape[1:])
    P = int(np.prod(sz))
    strides, overlaps, ms, gsig = (16, 12, 1), (8, 8, 1), (5, 5, 1), (2, 2)
    mc = MotionCorrect(video, max_shifts=ms, strides=strides, overlaps=overlaps, is3D=True, gSig_filt=gsig, save_corrected=True,
                       pw_rigid=True)
    mc.motion_correct()
    got = -np.array(mc.shifts_rig)[:, :2]
    rel = (got - np.median(got, 0)) - (shifts - np.median(shifts, 0))
    print(f"template=None: shifts_rig against the planted shifts, both relative to their median: largest error {np.abs(rel).max():.3f}")
    assert len(mc.shifts_rig) == T and np.abs(rel).max() <= 0.5

    # the rigid pass by hand
    frames = torch.from_numpy(video.reshape(T, P)).cuda()
    add = float(np.float32(-float(video.min())))
    filtered = ops.high_pass_frames(frames, sz, gsig)
    first = MotionCorrect._bin_median_3d(filtered)
    rigid = ops.rigid_correct(filtered, first, sz, ms, 10, add_to_movie=add, border_nan=True, want_frames=False)[0]
    NP = len(ops.patch_grid(sz, strides, overlaps)[1])
    table = (rigid * torch.tensor([-1.0, -1.0, 1.0], device="cuda"))[:, None, :].expand(-1, NP, -1).contiguous()
    moved, tsum, tcount = ops.apply_pwrigid(frames, table, sz, strides, overlaps, add_to_movie=add)
    mean = tsum / tcount
    mean = torch.where(torch.isnan(mean), mean[~torch.isnan(mean)].min(), mean)
    want = high_pass_filter_space(mean.view(*sz), gsig)
    assert np.array_equal(mc.total_template_rig, want.cpu().numpy())
    assert np.array_equal(mc.templates_rig[0], mc.total_template_rig)
    assert np.array_equal(np.array(mc.shifts_rig, dtype=np.float32), -rigid.cpu().numpy())
    # mc holds moved ORIGINALS: their mean keeps the background the filter removes
    assert mc.mc[0].shape == (*sz, T) and np.array_equal(mc.mc[0], moved.view(T, *sz).permute(1, 2, 3, 0).cpu().numpy(), equal_nan=True)
    corr = np.corrcoef(np.nanmean(mc.mc[0], 3).ravel(), bg.ravel())[0, 1]
    print(f"template=None: correlation of mc's time mean with the planted background {corr:.4f}")
    assert corr >= 0.9
    # and the move went the right way: the cells of every moved frame lie on those of a resting frame.  (Filtered, inside the border
    # the move leaves; blobs of sigma 1.5 apart by 2.8 voxels or more correlate below exp(-2.8^2 / (4 1.5^2)) = 0.42.)
    hp = ops.high_pass_frames(moved.nan_to_num(0.0), sz, gsig).view(T, *sz)[:, 6:-6, 6:-6].reshape(T, -1).double().cpu().numpy()
    raw = filtered.view(T, *sz)[:, 6:-6, 6:-6].reshape(T, -1).double().cpu().numpy()
    after = [np.corrcoef(hp[t], hp[0])[0, 1] for t in range(T)]
    before = [np.corrcoef(raw[t], raw[0])[0, 1] for t in range(T)]
    print(f"template=None: correlation of the filtered frames with frame 0, moved {np.round(after, 3).tolist()}, "
          f"unmoved {np.round(before, 3).tolist()}")
    assert min(after) >= 0.8 and min(before) < 0.5
    assert abs(float(mc.total_template_rig.mean())) < 0.05 * float(bg.mean())
    # the piecewise pass registered against the filtered template, and made its own from the corrected originals
    _, patch = ops.register_patches(filtered, want.reshape(-1), sz, strides, overlaps, ms, 3, 10, add_to_movie=-float(video.min()))
    assert np.array_equal(np.stack(mc.x_shifts_els), patch.cpu().numpy()[..., 0])
    assert np.corrcoef(mc.total_template_els.cpu().numpy().ravel(), bg.ravel())[0, 1] >= 0.9


def test_default_path_is_unchanged(ops):
    """gSig_filt=None: the shifts of register_patches on the raw rows, bit for bit."""
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect
    sz, strides, overlaps, ms, _, _ = COMPOSE["3d"]
    video, _ = compose_case("3d")
    template = video[0]
    mc = MotionCorrect(video, max_shifts=ms, strides=strides, overlaps=overlaps, max_deviation_rigid=3, is3D=True, pw_rigid=True)
    mc.motion_correct(template=template)
    frames = torch.from_numpy(video.reshape(video.shape[0], -1)).cuda()
    _, patch = ops.register_patches(frames, torch.from_numpy(template).cuda(), sz, strides, overlaps, ms, 3, 10,
                                    add_to_movie=-float(video.min()))
    got = np.stack([np.stack(mc.x_shifts_els), np.stack(mc.y_shifts_els), np.stack(mc.z_shifts_els)], 2)
    assert np.array_equal(got, patch.cpu().numpy())
