"""K9, the piecewise-rigid corrected movie: ``dnmf_apply_pwrigid`` / ``ops.apply_pwrigid`` and the
``MotionCorrect`` surface (``mc_els``, ``templates_els``, ``apply_shifts_movie``) against the G11 fixtures -- the reference's
own ``motion_correct_batch_pwrigid(..., shifts_opencv=True, is3D=True)``, captured by tests/golden/make_golden_motion.py --
and against ``restate_pwrigid`` below, a scipy restatement of ``tile_and_correct_3d`` :1639-1654 that the CPU tests pin to
the fixtures.

The CPU tests (not marked ``gpu``) check the restatement and K8's oracle on the fixtures; the GPU tests check the kernel.
"""
import ctypes

import numpy as np
import pytest
import torch


def restate_field(shifts, dims, shape):
    """The shift field that moves the image, (3, X, Y, Z) float32: the stored patch shifts (NP, 3) (-x, -y, +z) as (+x, +y,
    +z) on the patch grid, each resized as skimage's resize (order 1, mode 'reflect') does -- linear interpolation at
    c_d = (dims_d / N_d) (o + 0.5) - 0.5 with the edge mirrored."""
    from scipy.ndimage import map_coordinates
    sh = np.asarray(shifts, dtype=np.float32).reshape(*dims, 3)
    comps = [-sh[..., 0], -sh[..., 1], sh[..., 2]]
    axes = [(dims[d] / shape[d]) * (np.arange(shape[d]) + 0.5) - 0.5 for d in range(3)]
    c = np.array(np.meshgrid(*axes, indexing="ij"))
    return np.stack([map_coordinates(f.astype(np.float32), c, order=1, mode="mirror") for f in comps]).astype(np.float32)


def restate_coords(shifts, dims, shape):
    """Sample positions (3, X, Y, Z) float32: voxel index + field, added in float32 (:1644-1649)."""
    f = restate_field(shifts, dims, shape)
    grid = np.array(np.meshgrid(*[np.arange(n, dtype=np.float32) for n in shape], indexing="ij"))
    return grid + f


def restate_pwrigid(img, shifts, dims, add):
    """One frame (X, Y, Z) corrected by its patch shifts (NP, 3): skimage's warp (order 3, mode 'constant', cval 0 =
    map_coordinates with the B-spline prefilter; any coordinate outside [0, n-1] gives 0), _clip_warp_output (0 stays 0,
    the rest clipped to the range of img + add), minus add.  float32."""
    from scipy.ndimage import map_coordinates
    src = np.asarray(img, dtype=np.float64) + add
    coords = restate_coords(shifts, dims, src.shape).astype(np.float64)
    w = map_coordinates(src, coords, order=3, mode="constant", cval=0.0, prefilter=True)
    keep = w == 0
    w = np.clip(w, src.min(), src.max())
    w[keep] = 0
    return (w - add).astype(np.float32)


def restate_template(movie):
    """tile_and_correct_wrapper :2057-2058 on (X, Y, Z, T): nanmean over time, NaN -> nanmin."""
    t = np.nanmean(movie, -1)
    t[np.isnan(t)] = np.nanmin(t)
    return t


def cut_fraction(shifts, dims, shape, eps=1e-5):
    """Voxels whose restated coordinate lies within eps of a cut (0 or n - 1) on some axis of length > 1, but not on it:
    where the fp32 sums of the kernel and the float64 ones of the reference may fall on different sides.  (A coordinate
    exactly on the cut -- a voxel the field leaves in place, say -- is the same in both.)"""
    c = restate_coords(shifts, dims, shape)
    near = np.zeros(shape, dtype=bool)
    for d in range(3):
        if shape[d] > 1:
            for edge in (0.0, shape[d] - 1.0):
                near |= (np.abs(c[d] - edge) < eps) & (c[d] != edge)
    return near


def fixture_shifts(G, t):
    return np.stack([G["x_shifts_els"][t], G["y_shifts_els"][t], G["z_shifts_els"][t]], 1)


def grid_dims(G):
    from oracle import motion_oracle as MO
    sz = G["video"].shape[1:]
    win = MO.sliding_window_3d(sz, tuple(G["overlaps"]), tuple(G["strides"]))
    return tuple(int(v) + 1 for v in win[-1][:3])


FIXTURES = ["G11_pwrigid_3d", "G11_pwrigid_z1"]


# ---------------------------------------------------------------- CPU: the restatement and K8's oracle against the fixtures

@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_reference(load_golden, name):
    G = load_golden(name)
    video = G["video"]
    T = video.shape[0]
    add = float(np.float32(-G["min_mov"]))
    dims = grid_dims(G)
    scale = float(video.max() - video.min())
    mine = np.stack([restate_pwrigid(video[t], fixture_shifts(G, t), dims, add) for t in range(T)], -1)
    assert mine.shape == G["mc"].shape
    np.testing.assert_allclose(mine, G["mc"], rtol=0, atol=1e-6 * scale)
    np.testing.assert_allclose(restate_template(mine), G["chunk_template"], rtol=0, atol=1e-6 * scale)
    # the reference's chunk template is the nanmean of its own movie, and its total template the dstack collapse of it
    np.testing.assert_array_equal(restate_template(G["mc"].astype(np.float32)), G["chunk_template"])
    assert G["total_template"].shape == video.shape[1:3]
    # the fixtures exercise the cut: samples from outside the volume come out as min_mov
    assert (G["mc"] == np.float32(G["min_mov"])).mean() > 0.005


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_shifts_match_reference(load_golden, name):
    """oracle.motion_oracle.pw_rigid_shifts -- the restatement K8 is tested against -- equals the reference's shifts."""
    from oracle import motion_oracle as MO
    G = load_golden(name)
    add = -float(G["min_mov"])
    sx, sy, sz_, _ = MO.pw_rigid_shifts(G["video"], G["template"], tuple(G["strides"]), tuple(G["overlaps"]),
                                       tuple(G["max_shifts"]), 10, int(G["max_deviation_rigid"]), add)
    np.testing.assert_array_equal(sx, G["x_shifts_els"])
    np.testing.assert_array_equal(sy, G["y_shifts_els"])
    np.testing.assert_array_equal(sz_, G["z_shifts_els"])
    assert np.abs(G["x_shifts_els"]).max() > 1.0


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_kernel_matches_reference_movie(ops, load_golden, name):
    G = load_golden(name)
    video = G["video"]
    T, sz = video.shape[0], list(video.shape[1:])
    add = float(np.float32(-G["min_mov"]))
    shifts = np.stack([fixture_shifts(G, t) for t in range(T)])
    out, tsum, tcount = ops.apply_pwrigid(_gpu(video.reshape(T, -1)), _gpu(shifts), sz, tuple(G["strides"]), tuple(G["overlaps"]), add)
    got = out.cpu().numpy().reshape(T, *sz).transpose(1, 2, 3, 0)
    scale = float(video.max() - video.min())
    dims = grid_dims(G)
    near = np.stack([cut_fraction(shifts[t], dims, sz) for t in range(T)], -1)
    bad = np.abs(got - G["mc"]) > 1e-5 * scale
    assert (bad & ~near).sum() == 0, np.abs(got - G["mc"])[~near].max() / scale
    assert near.mean() <= 1e-3
    tmpl = (tsum / tcount).cpu().numpy().reshape(sz)
    np.testing.assert_allclose(tmpl, G["chunk_template"], rtol=0, atol=1e-5 * scale)
    assert int(tcount.min()) == T


def _random_case(sz, strides, overlaps, T, amp, seed):
    from oracle import motion_oracle as MO
    rng = np.random.RandomState(seed)
    X, Y, Z = sz
    g = np.meshgrid(*[np.arange(n) for n in sz], indexing="ij")
    video = np.stack([np.sin(0.3 * g[0] + 0.2 * t) * np.cos(0.25 * g[1]) + 0.5 * np.cos(0.7 * g[2] + t) + 0.1 * rng.randn(*sz)
                      for t in range(T)]).astype(np.float32)
    NP = len(MO.sliding_window_3d(sz, overlaps, strides))
    sh = rng.uniform(-amp, amp, (T, NP, 3)).astype(np.float32)
    sh[..., 2] *= 0.3 if Z > 1 else 0.0
    sh = np.round(sh * 10) / 10          # multiples of 0.1 as the registration returns them
    dims = tuple(int(v) + 1 for v in MO.sliding_window_3d(sz, overlaps, strides)[-1][:3])
    return video, sh.astype(np.float32), dims


def _check_against_restatement(got, video, sh, dims, add, limit=1e-3):
    scale = float(video.max() - video.min())
    T = video.shape[0]
    for t in range(T):
        ref = restate_pwrigid(video[t], sh[t], dims, add)
        near = cut_fraction(sh[t], dims, video.shape[1:])
        bad = np.abs(got[t] - ref) > 1e-5 * scale
        assert (bad & ~near).sum() == 0, (t, np.abs(got[t] - ref)[~near].max() / scale)
        assert near.mean() <= limit


@pytest.mark.gpu
@pytest.mark.parametrize("sz,strides,overlaps,amp", [
    ([33, 29, 1], (10, 8, 1), (6, 6, 0), 9.0),        # one slice, odd sizes, many samples cut
    ([31, 27, 2], (12, 10, 1), (6, 6, 1), 4.0),       # two slices, two patch layers in z
    ([24, 21, 3], (24, 8, 1), (0, 6, 1), 3.0),        # one patch along x
    ([20, 18, 7], (8, 9, 3), (4, 4, 2), 6.0),
    ([16, 24, 16], (6, 24, 6), (4, 0, 4), 2.5),       # one patch along y
])
def test_kernel_matches_restatement(ops, sz, strides, overlaps, amp):
    T = 3
    video, sh, dims = _random_case(sz, strides, overlaps, T, amp, seed=sum(sz))
    add = float(np.float32(-video.min()))
    out, _, _ = ops.apply_pwrigid(_gpu(video.reshape(T, -1)), _gpu(sh), sz, strides, overlaps, add)
    _check_against_restatement(out.cpu().numpy().reshape(T, *sz), video, sh, dims, add, limit=5e-3)


@pytest.mark.gpu
def test_frame_ids_strides_and_accumulation(ops):
    sz, strides, overlaps, T = [21, 19, 5], (8, 8, 2), (4, 4, 1), 5
    video, sh, dims = _random_case(sz, strides, overlaps, T, 5.0, seed=3)
    P = int(np.prod(sz))
    add = float(np.float32(-video.min()))
    # rows of ldf > P in an order given by frame_ids; out rows of ldo > P
    order = np.array([3, 0, 4, 2, 1])
    big = np.zeros((T, P + 37), dtype=np.float32)
    big[order, :P] = video.reshape(T, -1)
    frames = _gpu(big)
    outbig = torch.full((T, P + 11), -7.0, device="cuda")
    out, tsum, tcount = ops.apply_pwrigid(frames, _gpu(sh), sz, strides, overlaps, add, frame_ids=order, out=outbig)
    got = outbig[:, :P].cpu().numpy().reshape(T, *sz)
    assert (outbig[:, P:] == -7.0).all()
    _check_against_restatement(got, video, sh, dims, add, limit=5e-3)
    # B = 1, and one batch split into two calls with tsum / tcount accumulation
    one, _, _ = ops.apply_pwrigid(frames, _gpu(sh[:1]), sz, strides, overlaps, add, frame_ids=order[:1])
    np.testing.assert_array_equal(one.cpu().numpy()[0], outbig[0, :P].cpu().numpy())
    _, s2, c2 = ops.apply_pwrigid(frames, _gpu(sh[:2]), sz, strides, overlaps, add, frame_ids=order[:2])
    _, s2, c2 = ops.apply_pwrigid(frames, _gpu(sh[2:]), sz, strides, overlaps, add, frame_ids=order[2:], tsum=s2, tcount=c2)
    np.testing.assert_array_equal(c2.cpu().numpy(), tcount.cpu().numpy())
    np.testing.assert_allclose(s2.cpu().numpy(), tsum.cpu().numpy(), rtol=1e-6, atol=1e-6 * float(np.abs(video).max()) * T)


@pytest.mark.gpu
def test_properties(ops):
    sz, strides, overlaps, T = [26, 22, 4], (10, 8, 2), (6, 6, 1), 2
    video, sh, _ = _random_case(sz, strides, overlaps, T, 5.0, seed=9)
    scale = float(video.max() - video.min())
    add = float(np.float32(-video.min()))
    # zero shifts: the identity
    out, _, _ = ops.apply_pwrigid(_gpu(video.reshape(T, -1)), _gpu(np.zeros_like(sh)), sz, strides, overlaps, add)
    np.testing.assert_allclose(out.cpu().numpy().reshape(T, *sz), video, rtol=0, atol=1e-6 * scale)
    # a constant frame stays constant where no sample is cut, and is min_mov where one is
    min_mov = -1.5
    const = np.full((T, *sz), 2.25, dtype=np.float32)
    out, _, _ = ops.apply_pwrigid(_gpu(const.reshape(T, -1)), _gpu(sh), sz, strides, overlaps, -min_mov)
    got = out.cpu().numpy().reshape(T, *sz)
    dims = grid_dims({"video": const, "overlaps": np.array(overlaps), "strides": np.array(strides)})
    for t in range(T):
        c = restate_coords(sh[t], dims, sz)
        cut = np.zeros(sz, dtype=bool)
        for d in range(3):
            cut |= (c[d] < 0) | (c[d] > sz[d] - 1)
        near = cut_fraction(sh[t], dims, sz)
        assert cut.any() and (~cut).any()
        np.testing.assert_array_equal(got[t][cut & ~near], np.float32(min_mov))
        np.testing.assert_allclose(got[t][~cut & ~near], 2.25, rtol=0, atol=1e-6)


@pytest.mark.gpu
def test_motioncorrect_pwrigid_movie(ops, load_golden):
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect
    G = load_golden("G11_pwrigid_3d")
    video = G["video"]
    T, sz = video.shape[0], list(video.shape[1:])
    scale = float(video.max() - video.min())
    kw = dict(max_shifts=tuple(G["max_shifts"]), strides=tuple(G["strides"]), overlaps=tuple(G["overlaps"]),
              max_deviation_rigid=int(G["max_deviation_rigid"]), is3D=True)
    mc = MotionCorrect(video, save_corrected=True, **kw)
    mc.min_mov = float(G["min_mov"])
    mc.motion_correct_pwrigid(template=G["template"])
    bins = []
    for key in ("x_shifts_els", "y_shifts_els", "z_shifts_els"):
        bins.append(np.abs(np.stack(getattr(mc, key)) - G[key]) * 10)
    bins = np.stack(bins, -1)
    assert bins.max() <= 1.0 + 1e-3 and (bins < 1e-3).mean() >= 0.97
    assert len(mc.mc_els) == 1 and mc.mc_els[0].shape == (*sz, T) and mc.mc_els[0].dtype == np.float32
    same = [t for t in range(T) if bins[t].max() < 1e-3]
    assert same
    dims = grid_dims(G)
    for t in same:
        near = cut_fraction(fixture_shifts(G, t), dims, sz)
        bad = np.abs(mc.mc_els[0][..., t] - G["mc"][..., t]) > 1e-5 * scale
        assert (bad & ~near).sum() == 0
    # a frame whose shift landed in the neighbouring bin moves by 0.1 voxel: the template moves by a gradient / T
    np.testing.assert_allclose(mc.templates_els[0], G["chunk_template"], rtol=0, atol=0.1 * scale / T)
    assert np.abs(mc.templates_els[0] - G["chunk_template"]).mean() <= 2e-3 * scale
    # a template given: total_template_els stays at it
    np.testing.assert_array_equal(torch.as_tensor(mc.total_template_els).cpu().numpy(), G["template"])

    # without a template: the rigid pre-pass, then total_template_els = the template of the corrected frames
    mc2 = MotionCorrect(video, save_corrected=True, **kw)
    mc2.min_mov = float(G["min_mov"])
    mc2.motion_correct_pwrigid(template=None)
    assert torch.is_tensor(mc2.total_template_els) and tuple(mc2.total_template_els.shape) == tuple(sz)
    np.testing.assert_allclose(mc2.total_template_els.cpu().numpy(), restate_template(mc2.mc_els[0]), rtol=0, atol=1e-6 * scale)
    np.testing.assert_array_equal(mc2.templates_els[0], mc2.total_template_els.cpu().numpy())
    assert mc2.mc[0].shape == (*sz, T)                # mc keeps the rigid pass's movie


@pytest.mark.gpu
def test_apply_shifts_movie(ops, load_golden):
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect
    G = load_golden("G11_pwrigid_3d")
    video = G["video"]
    T, sz = video.shape[0], list(video.shape[1:])
    scale = float(video.max() - video.min())
    mc = MotionCorrect(video, max_shifts=tuple(G["max_shifts"]), strides=tuple(G["strides"]), overlaps=tuple(G["overlaps"]), is3D=True)
    mc.min_mov = float(G["min_mov"])
    mc.motion_correct_pwrigid(template=G["template"])
    assert not hasattr(mc, "mc_els")                   # save_corrected=False: nothing new is filled
    # the stored shifts, edited: the movie follows the edit
    for t in range(T):
        mc.x_shifts_els[t] = G["x_shifts_els"][t].copy()
        mc.y_shifts_els[t] = G["y_shifts_els"][t].copy()
        mc.z_shifts_els[t] = G["z_shifts_els"][t].copy()
    mc.x_shifts_els[1] = mc.x_shifts_els[1] + np.float32(1.5)
    got = mc.apply_shifts_movie(video)
    assert got.shape == (*sz, T) and got.dtype == np.float32
    add = float(np.float32(-G["min_mov"]))
    dims = grid_dims(G)
    for t in range(T):
        sh = np.stack([mc.x_shifts_els[t], mc.y_shifts_els[t], mc.z_shifts_els[t]], 1)
        ref = restate_pwrigid(video[t], sh, dims, add)
        near = cut_fraction(sh, dims, sz)
        assert ((np.abs(got[..., t] - ref) > 1e-5 * scale) & ~near).sum() == 0
        if t != 1:
            assert ((np.abs(got[..., t] - G["mc"][..., t]) > 1e-5 * scale) & ~cut_fraction(fixture_shifts(G, t), dims, sz)).sum() == 0
    assert np.abs(got[..., 1] - G["mc"][..., 1]).max() > 0.05 * scale
    # 2-D videos: not built
    mc2 = MotionCorrect(video[..., 0], max_shifts=(5, 5), strides=(12, 10), overlaps=(6, 6), is3D=False)
    with pytest.raises(NotImplementedError):
        mc2.apply_shifts_movie(video[..., 0])


@pytest.mark.gpu
def test_abi_rejects_bad_arguments(ops):
    from dnmf_amd import _lib
    lib = _lib.load()
    X, Y, Z, B = 16, 12, 2, 2
    P = X * Y * Z
    st = (ctypes.c_int * 3)(8, 6, 1)
    ov = (ctypes.c_int * 3)(4, 4, 1)
    NP = lib.dnmf_register_patches_grid(X, Y, Z, st, ov, None, None)
    frames = torch.zeros((B, P), device="cuda")
    sh = torch.zeros((B, NP, 3), device="cuda")
    out = torch.empty((B, P), device="cuda")
    tsum = torch.zeros(P, device="cuda")
    need = lib.dnmf_apply_pwrigid_workspace(X, Y, Z, st, ov, B)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    s = ops._stream()

    def call(frames_p=frames.data_ptr(), shifts_p=sh.data_ptr(), out_p=out.data_ptr(), x=X, ldf=P, ldo=P, tsum_p=0, tcount_p=0,
             ws_bytes=need, strides=st):
        return lib.dnmf_apply_pwrigid(frames_p, ldf, None, B, x, Y, Z, strides, ov, shifts_p, 0.0, out_p, ldo, tsum_p, tcount_p,
                                      ws.data_ptr(), ws_bytes, s)
    assert call() == 0
    assert call(frames_p=None) == -1 and call(shifts_p=None) == -1 and call(out_p=None) == -1
    assert call(tsum_p=tsum.data_ptr()) == -1                       # tsum without tcount
    assert call(ws_bytes=need - 1) == -4
    assert call(ldf=P - 1) == -2 and call(ldo=P - 1) == -2 and call(x=0) == -2
    assert call(strides=(ctypes.c_int * 3)(40, 6, 1)) == -2         # windows larger than the volume
    torch.cuda.synchronize()
