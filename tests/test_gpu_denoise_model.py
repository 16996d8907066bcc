"""The class surfaces of K34 on the planted 40 x 36 x 2 x 120 movie: ``DeformableNMF.denoise_movie`` (identity warp,
``registered='linear'``), ``ExponentialFP.denoise_movie`` and ``MotionCorrect.denoise_movie`` give what ``ops.lowrank_denoise`` gives
on the same rows with K18's mean and K30's noise, bit for bit."""
import numpy as np
import pytest
import torch

import denoise_restatement as DN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def planted():
    from dnmf_amd import ops
    noisy, clean = DN.planted_video(2, 0)                                 # (T, X, Y, Z)
    T, sz = noisy.shape[0], list(noisy.shape[1:])
    rows = torch.from_numpy(noisy.reshape(T, -1)).cuda()
    mean = ops.summary_images(rows, sz, neighbours='face')[0]["mean"]
    noise = ops.noise_image(rows, sz)
    want, info = ops.lowrank_denoise(rows, sz, mean, noise)
    return dict(noisy=noisy, clean=clean.reshape(T, -1), rows=rows, sz=sz, T=T, want=want, info=info)


def same(info, want):
    for k in ("U", "Q", "lam", "explained", "kept", "ok"):
        got = info[k] if isinstance(info[k], np.ndarray) else info[k].cpu().numpy()
        assert np.array_equal(got, want[k].cpu().numpy()), k
    np.testing.assert_array_equal(info["plan"]["boxes"], want["plan"]["boxes"])


def test_the_planted_movie_is_denoised(planted):
    out = planted["want"].cpu().numpy().astype(np.float64)
    raw = np.mean((planted["noisy"].reshape(planted["T"], -1) - planted["clean"]) ** 2)
    den = np.mean((out - planted["clean"]) ** 2)
    print(f"mse raw {raw:.4f}, denoised {den:.4f}, gain {raw / den:.1f}, kept {np.bincount(planted['info']['kept'].cpu().numpy())}")
    assert raw / den >= 0.5 * 36.3                                        # the bound of tests/test_denoise_host.py
    assert int(planted["info"]["ok"].min()) == 1


def test_deformable_nmf(planted):
    from dnmf_amd import ops
    from dnmf_amd.Demix import dNMF as M
    sz, T = planted["sz"], planted["T"]
    pos = torch.tensor([[11.5, 11.5, 0.5], [19.5, 3.5, 0.5], [27.5, 11.5, 0.5]])
    dn = M.DeformableNMF(torch.tensor(sz), 3, T, positions=pos)
    dn.verbose = False
    assert dn.last_denoise is None
    loader = M.ResidentLoader(planted["rows"], sz, 8)
    movie = dn.denoise_movie(loader)
    assert movie.is_cuda and movie.shape == (T, sz[0] * sz[1] * sz[2])
    assert torch.equal(movie.view(torch.int32), planted["want"].view(torch.int32))
    same(dn.last_denoise, planted["info"])
    # at the identity warp K17 returns the input: registered = unregistered, bit for bit
    reg = dn.denoise_movie(loader, registered='linear', rank=4, scale=None)
    want, info = ops.lowrank_denoise(planted["rows"], sz, ops.summary_images(planted["rows"], sz, neighbours='face')[0]["mean"], None, rank=4)
    assert torch.equal(reg.view(torch.int32), want.view(torch.int32))
    same(dn.last_denoise, info)
    assert dn.last_denoise["U"].shape[2] == 4
    with pytest.raises(ValueError, match="registered"):
        dn.denoise_movie(loader, registered='cubic')
    with pytest.raises(ValueError, match="scale"):
        dn.denoise_movie(loader, scale='mad')
    # MultiChannelDNMF is refused, and so is a sharded loader
    assert issubclass(M.MultiChannelDNMF, M.DeformableNMF)
    mc = M.MultiChannelDNMF(torch.tensor(sz), 3, T, torch.tensor([[1.0, 0.5, 0.2], [0.3, 0.9, 0.6]]), positions=pos)
    mc.verbose = False
    with pytest.raises(NotImplementedError, match="one channel"):
        mc.denoise_movie(loader)
    assert mc.last_denoise is None
    loader.T_total = 2 * loader.T
    with pytest.raises(NotImplementedError, match="shard"):
        dn.denoise_movie(loader)


def test_static_and_motion_correct_surfaces(planted):
    from dnmf_amd.Demix.dNMF import ExponentialFP
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect
    sz, T = planted["sz"], planted["T"]
    xyzt = np.ascontiguousarray(np.moveaxis(planted["noisy"], 0, 3))      # (X, Y, Z, T), the layout of MotionCorrect's mc
    want = np.moveaxis(planted["want"].cpu().numpy().reshape(T, *sz), 0, 3)
    movie, info = ExponentialFP.denoise_movie(xyzt)
    assert isinstance(movie, np.ndarray) and movie.dtype == np.float32 and movie.shape == xyzt.shape
    np.testing.assert_array_equal(movie, want)
    assert isinstance(info["U"], np.ndarray)
    same(info, planted["info"])
    cuda, cinfo = ExponentialFP.denoise_movie((planted["rows"], sz))
    assert cuda.is_cuda and cinfo["Q"].is_cuda and torch.equal(cuda.view(torch.int32), planted["want"].view(torch.int32))
    mc = MotionCorrect(planted["noisy"][:8], max_shifts=(2, 2, 1), strides=(12, 12, 1), overlaps=(4, 4, 1), max_deviation_rigid=1, is3D=True,
                       pw_rigid=True)
    got, _ = mc.denoise_movie(xyzt)
    np.testing.assert_array_equal(got, want)
    with pytest.raises(ValueError, match="save_corrected"):
        mc.denoise_movie()
    mc.mc = [xyzt[..., :50].copy(), xyzt[..., 50:].copy()]                # two stored videos count as one movie
    stored, sinfo = mc.denoise_movie()
    np.testing.assert_array_equal(stored, want)
    same(sinfo, planted["info"])
