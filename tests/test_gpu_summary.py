"""Summary images (K18, ``dnmf_summary_images``) on the GPU against the float64 definition (tests/summary_restatement.py),
and the public surface built on it.

Tolerances: ``max`` bit for bit, ``mean`` rtol 1e-12, ``std`` rtol 1e-6, ``corr`` atol 1e-6, the NaN pattern identical.  The
kernel sums one pass in float64; at most 64 frames at mean^2 / var <= 1e6 err by about 64 x 2.2e-16 x 1e6 = 1.4e-8 even
before the pivot helps, so 1e-6 keeps a 30-fold margin.  The inputs are a seeded mean + noise with |mean| / std <= 1e3 per
voxel, asserted on the restatement's output."""
import functools

import numpy as np
import pytest
import torch

import summary_restatement as SR

pytestmark = pytest.mark.gpu

# the last shape is this file's own: beyond Z = 23 a tile's halo no longer fits the values a thread stages through registers
SHAPES = [(20, 17, 1), (9, 7, 3), (33, 5, 2), (1, 40, 1), (3, 4, 26)]
FRAMES = [1, 2, 37]
NEIGHBOURS = ["full", "face"]
KEYS = ("mean", "std", "max", "corr")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


# seeds for which the input conditions hold at T = 2 as well, where two samples decide a voxel's std (asserted in reference())
SEEDS = {(20, 17, 1): 5, (9, 7, 3): 2, (33, 5, 2): 1, (1, 40, 1): 0, (3, 4, 26): 0}


@functools.lru_cache(maxsize=None)
def video(sz, T=37):
    """(T, X, Y, Z) fp32: per voxel a mean in [0.5, 1.5] plus noise of a std in [0.5, 1]."""
    rng = np.random.RandomState(SEEDS[sz])
    x = rng.uniform(0.5, 1.5, sz)[None] + rng.uniform(0.5, 1, sz)[None] * rng.randn(T, *sz)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(sz, T, neighbours):
    """The restatement on the first T frames: computed once, never changed."""
    x = video(sz)[:T]
    ref = SR.summary_images(x, neighbours)
    # the input conditions of the tolerances: |mean| / std <= 1e3, and no mean below 1 % of the voxel's largest sample (the
    # sums carry about T x 1.1e-16 of that: 4e-13 of the mean at T = 37, within rtol 1e-12)
    if T >= 2:
        assert (np.abs(ref["mean"]) / ref["std"]).max() <= 1e3
    assert (np.abs(x).max(0) / np.abs(ref["mean"])).max() < 1e2
    for v in ref.values():
        v.setflags(write=False)
    return ref


def host(images):
    return {k: images[k].cpu().numpy() for k in KEYS}


def compare(got, want, what, exact=False):
    """``got`` against ``want`` at the tolerances of this file (``exact``: every image bit for bit)."""
    worst = {}
    for k in KEYS:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == np.float64
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f"{what}: NaN pattern of {k}")
        ok = ~np.isnan(w)
        if k == "corr":
            worst[k] = np.abs(g[ok] - w[ok]).max() if ok.any() else 0.0
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = np.abs(g[ok] - w[ok]) / np.abs(w[ok])
            worst[k] = np.where(g[ok] == w[ok], 0.0, rel).max() if ok.any() else 0.0
    print(f"{what}: worst deviation mean {worst['mean']:.2e} (rel), std {worst['std']:.2e} (rel), max {worst['max']:.2e} (rel), "
          f"corr {worst['corr']:.2e} (abs)")
    for k in KEYS:
        if exact or k == "max":
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")
    assert worst["mean"] <= 1e-12 and worst["std"] <= 1e-6 and worst["corr"] <= 1e-6, what


def rows(x):
    return dev(x.reshape(x.shape[0], -1))


@pytest.mark.parametrize("neighbours", NEIGHBOURS)
@pytest.mark.parametrize("T", FRAMES)
@pytest.mark.parametrize("sz", SHAPES)
def test_images_match_the_restatement(ops, sz, T, neighbours):
    images, state = ops.summary_images(rows(video(sz)[:T]), sz, neighbours=neighbours)
    assert all(images[k].shape == sz and images[k].dtype == torch.float64 and images[k].is_cuda for k in KEYS)
    got = host(images)
    compare(got, reference(sz, T, neighbours), f"{sz} T={T} {neighbours}")
    if T == 1:
        assert np.isnan(got["corr"]).all() and (got["std"] == 0).all()


@pytest.mark.parametrize("neighbours", NEIGHBOURS)
@pytest.mark.parametrize("sz", SHAPES[:4])
def test_forced_segments(ops, sz, neighbours):
    """Five segments of 8 frames, the last of 5, against the kernel's own choice and the restatement."""
    fr = rows(video(sz))
    forced = host(ops.summary_images(fr, sz, neighbours=neighbours, segment=8)[0])
    compare(forced, reference(sz, 37, neighbours), f"{sz} {neighbours} segment=8")
    compare(forced, host(ops.summary_images(fr, sz, neighbours=neighbours)[0]), f"{sz} {neighbours} segment=8 against 0")


@pytest.mark.parametrize("neighbours", NEIGHBOURS)
@pytest.mark.parametrize("sz", SHAPES[:4])
def test_chunked_state(ops, sz, neighbours):
    """20 + 17 frames through the state against one call of 37."""
    fr = rows(video(sz))
    none, state = ops.summary_images(fr[:20], sz, neighbours=neighbours, finish=False)
    assert none is None
    images, state2 = ops.summary_images(fr[20:], sz, neighbours=neighbours, state=state, first=False)
    assert state2 is state
    compare(host(images), reference(sz, 37, neighbours), f"{sz} {neighbours} 20 + 17 frames")
    compare(host(images), host(ops.summary_images(fr, sz, neighbours=neighbours)[0]), f"{sz} {neighbours} 20 + 17 against 37")
    with pytest.raises(ValueError, match="first=False"):
        ops.summary_images(fr, sz, neighbours=neighbours, first=False)


def test_same_bits_on_every_run(ops):
    for sz in SHAPES[:2]:
        fr = rows(video(sz))
        a = host(ops.summary_images(fr, sz, segment=8)[0])
        b = host(ops.summary_images(fr, sz, segment=8)[0])
        for k in KEYS:
            np.testing.assert_array_equal(a[k], b[k])


@pytest.mark.parametrize("sz", SHAPES[:2])
def test_padded_rows_and_frame_ids(ops, sz):
    x = video(sz)
    P = int(np.prod(sz))
    padded = torch.full((37, P + 13), float("nan"), device="cuda")
    padded[:, :P] = rows(x)
    want = reference(sz, 37, "full")
    plain = host(ops.summary_images(padded[:, :P], sz)[0])
    assert padded[:, :P].stride(0) == P + 13
    compare(plain, want, f"{sz} ldf = P + 13")
    perm = np.random.RandomState(1).permutation(37)
    shuffled = host(ops.summary_images(padded[:, :P], sz, frame_ids=perm.tolist())[0])
    compare(shuffled, want, f"{sz} permuted frame_ids")
    compare(shuffled, plain, f"{sz} permuted against in order")
    subset = perm[:11]
    some = host(ops.summary_images(padded[:, :P], sz, frame_ids=torch.from_numpy(subset))[0])
    compare(some, SR.summary_images(x[subset], "full"), f"{sz} 11 of 37 frames")


@pytest.mark.parametrize("sz", SHAPES[:3])
def test_sub_equals_subtracted_rows(ops, sz):
    fr = rows(video(sz))
    sub = torch.rand(37, fr.shape[1] + 5, device="cuda")[:, :fr.shape[1]] * 3      # a row stride of its own
    for nb in NEIGHBOURS:
        a = host(ops.summary_images(fr, sz, sub=sub, neighbours=nb, segment=8)[0])
        b = host(ops.summary_images(fr - sub, sz, neighbours=nb, segment=8)[0])
        compare(a, b, f"{sz} {nb} sub", exact=True)
        compare(a, SR.summary_images(video(sz), nb, sub=sub.cpu().numpy().reshape(37, *sz)), f"{sz} {nb} sub against the restatement")


@pytest.mark.parametrize("segment", [0, 8])
def test_special_voxels(ops, segment):
    sz = (9, 7, 3)
    x = video(sz).copy()
    x[:, 4, 3, 1] = 2.5                 # constant
    x[5, 2, 5, 0] = np.nan              # one NaN
    x[0, 7, 1, 2] = np.inf              # +inf in the pivot frame
    for nb in NEIGHBOURS:
        want = SR.summary_images(x, nb)
        got = host(ops.summary_images(rows(x), sz, neighbours=nb, segment=segment)[0])
        compare(got, want, f"special voxels {nb} segment={segment}")
        assert got["std"][4, 3, 1] == 0.0 and got["mean"][4, 3, 1] == 2.5 and got["max"][4, 3, 1] == 2.5 and np.isnan(got["corr"][4, 3, 1])
        for p in ((2, 5, 0), (7, 1, 2)):
            assert all(np.isnan(got[k][p]) for k in KEYS)
        assert np.isnan(got["mean"]).sum() == 2 and np.isnan(got["corr"]).sum() == 3
    # the same voxels through the state: both bad samples arrive in the first piece
    _, state = ops.summary_images(rows(x[:20]), sz, finish=False, segment=segment)
    images, _ = ops.summary_images(rows(x[20:]), sz, state=state, first=False, segment=segment)
    compare(host(images), SR.summary_images(x, "full"), f"special voxels in two pieces segment={segment}")


def test_exponentialfp_summary_images(ops):
    from dnmf_amd.Demix.dNMF import ExponentialFP
    sz = (9, 7, 3)
    out = ExponentialFP.summary_images(video(sz))
    assert all(isinstance(out[k], np.ndarray) and out[k].dtype == np.float64 and out[k].shape == sz for k in KEYS)
    compare(out, reference(sz, 37, "full"), "ExponentialFP.summary_images numpy")
    cuda = ExponentialFP.summary_images(dev(video(sz)), neighbours="face")
    assert all(torch.is_tensor(cuda[k]) and cuda[k].is_cuda and cuda[k].shape == sz for k in KEYS)
    compare(host(cuda), reference(sz, 37, "face"), "ExponentialFP.summary_images CUDA")
    with pytest.raises(ValueError, match="neighbours"):
        ExponentialFP.summary_images(video(sz), neighbours="edge")


def test_deformable_nmf_summary_images(ops):
    from dnmf_amd.Demix import dNMF as M
    rng = np.random.RandomState(3)
    sz, K, T = [20, 16, 2], 3, 12
    P = int(np.prod(sz))
    pos = (np.array([4, 4, 0]) + rng.rand(K, 3) * np.array([12, 8, 1])).astype(np.float32)
    dn = M.DeformableNMF(torch.tensor(sz), K, T, positions=torch.from_numpy(pos))
    dn.verbose = False
    dn.C = dev(0.3 + rng.rand(K, T))
    frames = dev(1.0 + rng.rand(T, P))
    loader = M.ResidentLoader(frames, sz, 4)
    plain = dn.summary_images(loader)
    want, _ = ops.summary_images(frames, sz)
    assert all(torch.equal(plain[k], want[k]) for k in KEYS)
    # the residual: the model's own reconstruction as sub
    times = torch.arange(T, dtype=torch.int32, device="cuda")
    S = ops.halo_interior(dn.fp.recon_image(dn.C, times), sz).reshape(T, P)
    assert float(S.max()) > 0.1
    want, _ = ops.summary_images(frames, sz, sub=S)
    res = dn.summary_images(loader, source='residual')
    for k in KEYS:
        np.testing.assert_array_equal(res[k].cpu().numpy(), want[k].cpu().numpy())
    assert not torch.equal(res["mean"], plain["mean"])
    compare(host(res), SR.summary_images(frames.cpu().numpy().reshape(T, *sz), "full", sub=S.cpu().numpy().reshape(T, *sz)),
            "DeformableNMF residual")
    # at the identity warp K17 returns the input: registered = unregistered, bit for bit
    for source in ('video', 'residual'):
        a, b = dn.summary_images(loader, source=source, registered='linear'), dn.summary_images(loader, source=source)
        for k in KEYS:
            np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy())
    face = dn.summary_images(loader, neighbours='face')
    assert torch.equal(face["corr"], ops.summary_images(frames, sz, neighbours='face')[0]["corr"])
    with pytest.raises(ValueError, match="source"):
        dn.summary_images(loader, source='model')
    with pytest.raises(ValueError, match="registered"):
        dn.summary_images(loader, registered='cubic')


def test_motioncorrect_summary_images_and_detect_points(ops):
    from dnmf_amd.Demix.dNMF import ExponentialFP, SimulatedVideoDataset
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect
    torch.manual_seed(0)
    np.random.seed(0)
    sz, T = torch.tensor([40, 36, 2]), 6
    ds = SimulatedVideoDataset(K=5, T=T, sz=sz, shape_std=3, density=.2, bg_snr=-120, traces='exp', motion='gp',
                               motion_par={'sigma': [2, 2, .01], 'ls': [10, 10, 10]})
    moving = np.moveaxis(np.asarray(ds.video), -1, 0)
    kw = dict(max_shifts=(5, 5, 1), strides=(16, 12, 1), overlaps=(8, 8, 1), max_deviation_rigid=3, is3D=True, pw_rigid=True)
    bare = MotionCorrect(moving, **kw)
    with pytest.raises(ValueError, match="save_corrected"):
        bare.summary_images()
    with pytest.raises(ValueError, match="save_corrected"):
        bare.detect_points(5, image='corr')
    with pytest.raises(ValueError, match="image must be"):
        bare.detect_points(5, image='median')
    mc = MotionCorrect(moving, save_corrected=True, **kw)
    mc.motion_correct()
    # the default is today's path
    np.testing.assert_array_equal(mc.detect_points(5, shape_std=3, image='template'), mc.detect_points(5, shape_std=3))
    tmpl = mc.total_template_els
    tmpl = tmpl.cpu().numpy() if torch.is_tensor(tmpl) else np.asarray(tmpl)
    np.testing.assert_array_equal(mc.detect_points(5, shape_std=3, image=tmpl), mc.detect_points(5, shape_std=3))
    # a given video
    given = mc.summary_images(moving, neighbours='face')
    want = ExponentialFP.summary_images(moving, neighbours='face')
    assert all(isinstance(given[k], np.ndarray) and np.array_equal(given[k], want[k], equal_nan=True) for k in KEYS)

    # the stored corrected movie: mc_els before mc
    kept = mc
    stored = kept.summary_images()
    want = ExponentialFP.summary_images(np.moveaxis(kept.mc_els[0], 3, 0))
    assert all(stored[k].shape == (40, 36, 2) and np.array_equal(stored[k], want[k], equal_nan=True) for k in KEYS)
    pts = kept.detect_points(5, shape_std=3, image='std')
    assert pts.dtype == np.float64 and pts.ndim == 2 and pts.shape[1] == 3 and 1 <= len(pts) <= 5 and np.isfinite(pts).all()

    # the planted video of the host test, fed as the corrected movie: the correlation image finds the two active neurons
    planted, active, still, sigma = SR.planted_video()
    kept.mc_els = [np.ascontiguousarray(np.moveaxis(planted, 0, 3))]
    got = kept.detect_points(2, shape_std=sigma, image='corr')
    dist = np.linalg.norm(got[None] - active[:, None], axis=2)
    print("image='corr' picks", got.tolist(), "worst distance", dist.min(1).max())
    assert len(got) == 2 and dist.min(1).max() <= 1.5 and sorted(dist.argmin(1)) == [0, 1]
    first = kept.detect_points(1, shape_std=sigma, image='max')
    assert len(first) == 1
    del kept.mc_els
    kept.mc = [np.ascontiguousarray(np.moveaxis(planted, 0, 3))]
    np.testing.assert_array_equal(kept.detect_points(2, shape_std=sigma, image='corr'), got)
