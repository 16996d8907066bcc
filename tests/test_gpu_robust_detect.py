"""``robust_images`` (K30) on the GPU against its definition, and the use it is for: on the planted video of
tests/robust_restatement.py a search of the peak-to-noise image finds the two dim, active cells first.

Tolerances, as ulp of float64 from the operation count: ``median``, ``mad`` and the percentiles are one interpolation of two
exact samples and ``noise`` is that times a constant, all written as the definition writes them -- 1 ulp; ``pnr`` adds one
subtraction and one division -- 4 ulp; ``max`` and ``n`` are equal.  Measured on the MI355X: 0 ulp on every image."""
import functools

import numpy as np
import pytest
import torch

import robust_restatement as RR

pytestmark = pytest.mark.gpu

ULPS = dict(median=1, mad=1, noise=1, pnr=4, max=0)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def planted(Z):
    video, cells, still, sigma = RR.planted_case(RR.PLANTED_SEEDS[Z], Z)
    ref = RR.robust_images(video, percentiles=(8, 50))
    return video, cells, still, sigma, ref


def assert_images(got, want, what):
    """Every failing voxel is reported."""
    failures = []

    def check(name, g, w, ulps):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == np.float64, (what, name)
        nan = np.isnan(g) != np.isnan(w)
        with np.errstate(invalid="ignore"):
            err = np.abs(g - w) / np.spacing(np.abs(w))
        err = np.where(g == w, 0.0, err)
        bad = nan | (~np.isnan(w) & ~np.isnan(g) & ~(err <= ulps))
        print(f"{what}: {name} worst {np.nanmax(err) if np.isfinite(err).any() else 0.0:.2f} ulp (allowed {ulps})")
        for p in zip(*np.nonzero(bad)):
            failures.append(f"{name}{p}: got {g[p]!r}, want {w[p]!r}")

    for name, ulps in ULPS.items():
        check(name, got[name], want[name], ulps)
    for p in want["percentile"]:
        check(f"percentile[{p}]", got["percentile"][p], want["percentile"][p], 1)
    if not np.array_equal(got["n"], want["n"]):
        failures.extend(f"n{p}: got {got['n'][p]}, want {want['n'][p]}" for p in zip(*np.nonzero(got["n"] != want["n"])))
    assert not failures, f"{what}: {len(failures)} voxels\n" + "\n".join(failures)


def picks_are_the_cells(pts, cells):
    dist = np.linalg.norm(np.asarray(pts)[None] - cells[:, None], axis=2)
    return len(pts) == 2 and np.isfinite(pts).all() and dist.min(1).max() <= 1.5 and sorted(dist.argmin(1)) == [0, 1]


@pytest.mark.parametrize("Z", [1, 2])
def test_robust_images_match_the_restatement(ops, Z):
    from dnmf_amd.Demix.dNMF import ExponentialFP
    video, cells, still, sigma, ref = planted(Z)
    out = ExponentialFP.robust_images(video, percentiles=(8, 50))
    assert all(isinstance(out[k], np.ndarray) and out[k].shape == (40, 36, Z) for k in ("median", "max", "mad", "noise", "pnr", "n"))
    assert out["n"].dtype == np.int32 and out["n"][0, 0, 0] == 47 and set(out["percentile"]) == {8, 50}
    assert_images(out, ref, f"Z={Z} numpy in")
    np.testing.assert_array_equal(out["percentile"][50], out["median"])
    cuda = ExponentialFP.robust_images(torch.from_numpy(video).cuda(), noise="mad")
    assert all(torch.is_tensor(cuda[k]) and cuda[k].is_cuda for k in ("median", "max", "mad", "noise", "pnr", "n"))
    want = RR.robust_images(video, noise="mad")
    assert_images({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in cuda.items()}, want, f"Z={Z} CUDA in, noise='mad'")
    with pytest.raises(ValueError, match="noise"):
        ExponentialFP.robust_images(video, noise="std")
    with pytest.raises(ValueError, match="percentiles"):
        ExponentialFP.robust_images(video, percentiles=(101,))


@pytest.mark.parametrize("Z", [1, 2])
def test_pnr_finds_the_dim_active_cells(ops, Z):
    from dnmf_amd.Demix.dNMF import ExponentialFP
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect
    video, cells, still, sigma, ref = planted(Z)
    images = ExponentialFP.robust_images(video)
    pos, _ = ExponentialFP.detect_positions(RR.nan_to_min(images["pnr"]), 2, shape_std=sigma)
    print(f"Z={Z} detect_positions on pnr:", pos.tolist())
    assert picks_are_the_cells(pos, cells)
    first, _ = ExponentialFP.detect_positions(RR.nan_to_min(images["max"]), 1, shape_std=sigma)
    assert np.linalg.norm(first[0] - still) <= 1.5          # the max image shows what is bright and noisy

    mc = MotionCorrect(video, max_shifts=(5, 5, 1), strides=(16, 12, 1), overlaps=(8, 8, 1), max_deviation_rigid=3, is3D=True,
                       pw_rigid=True)
    for name in ("pnr", "temporal_median", "corr_pnr"):
        with pytest.raises(ValueError, match="save_corrected"):
            mc.detect_points(2, image=name)
    with pytest.raises(ValueError, match="save_corrected"):
        mc.robust_images()
    for name in ("median", "snr"):
        with pytest.raises(ValueError, match="image must be"):
            mc.detect_points(2, image=name)
    mc.mc_els = [np.ascontiguousarray(np.moveaxis(video, 0, 3))]
    got = mc.detect_points(2, shape_std=sigma, image="pnr")
    print(f"Z={Z} MotionCorrect.detect_points(image='pnr'):", got.tolist())
    assert picks_are_the_cells(got, cells)
    np.testing.assert_array_equal(got, pos.astype(np.float64))
    stored = mc.robust_images(percentiles=(8, 50))
    assert_images(stored, ref, f"Z={Z} the stored movie")
    np.testing.assert_array_equal(mc.robust_images(video)["pnr"], images["pnr"])
    assert picks_are_the_cells(mc.detect_points(2, shape_std=sigma, image="corr_pnr"), cells)
    med = mc.detect_points(1, shape_std=sigma, image="temporal_median")
    assert len(med) == 1 and np.linalg.norm(med[0] - still) <= 1.5      # the baseline image: the static blob
    del mc.mc_els
    mc.mc = [np.ascontiguousarray(np.moveaxis(video, 0, 3))]
    np.testing.assert_array_equal(mc.detect_points(2, shape_std=sigma, image="pnr"), got)


def test_deformable_nmf_robust_images(ops):
    from dnmf_amd.Demix import dNMF as M
    rng = np.random.RandomState(3)
    sz, K, T = [20, 16, 2], 3, 12
    P = int(np.prod(sz))
    pos = (np.array([4, 4, 0]) + rng.rand(K, 3) * np.array([12, 8, 1])).astype(np.float32)
    dn = M.DeformableNMF(torch.tensor(sz), K, T, positions=torch.from_numpy(pos))
    dn.verbose = False
    frames = torch.from_numpy(1.0 + rng.rand(T, P)).to("cuda", torch.float32)
    loader = M.ResidentLoader(frames, sz, 4)
    plain = dn.robust_images(loader, percentiles=(8,))
    want = ops.robust_images(frames, sz, percentiles=(8,))
    want_np = RR.robust_images(frames.cpu().numpy().reshape(T, *sz), percentiles=(8,))
    for k in ("median", "max", "mad", "noise", "pnr", "n"):
        assert torch.equal(plain[k], want[k]), k
    assert torch.equal(plain["percentile"][8], want["percentile"][8])
    assert_images({k: (v.cpu().numpy() if torch.is_tensor(v) else {p: i.cpu().numpy() for p, i in v.items()}) for k, v in plain.items()},
                  want_np, "DeformableNMF.robust_images")
    # at the identity warp K17 returns the input: registered = unregistered, bit for bit
    reg = dn.robust_images(loader, registered='linear')
    for k in ("median", "pnr"):
        np.testing.assert_array_equal(reg[k].cpu().numpy(), plain[k].cpu().numpy())
    with pytest.raises(ValueError, match="registered"):
        dn.robust_images(loader, registered='cubic')
    # the refusals of _single_model_only
    nchan = dn._nchan
    dn._nchan = lambda: 2
    with pytest.raises(NotImplementedError, match="one channel"):
        dn.robust_images(loader)
    dn._nchan = nchan
    loader.T_total = 2 * loader.T
    with pytest.raises(NotImplementedError, match="shard"):
        dn.robust_images(loader)
