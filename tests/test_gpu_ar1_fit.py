"""The AR(1)-constrained trace update (K32) through the model: ``update_footprints(solver='ar1')`` and ``fit(solver='ar1')`` on a
planted video of 24 x 20 x {1, 2} voxels, K = 6 neurons of which (0, 1) and (2, 3) overlap, T = 40 frames rendered by the model's
own forward pass from AR(1) traces."""
import functools

import numpy as np
import pytest
import torch

import ar1_cases as AC

pytestmark = pytest.mark.gpu

G = AC.G_TRUE
K, T = 6, 40
POS = [[5.0, 5.0], [7.5, 5.0], [16.0, 6.0], [16.0, 8.5], [6.0, 14.0], [18.0, 15.0]]


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd.Demix import dNMF as M
    return M


def positions(Z):
    return torch.tensor([[x, y, float(k % Z)] for k, (x, y) in enumerate(POS)])


@functools.lru_cache(maxsize=None)
def planted(Z):
    """(sz, video (T, P) fp32 CUDA, traces (K, T)); rendered once."""
    from dnmf_amd.Demix import dNMF as M
    sz = (24, 20, Z)
    rng = np.random.RandomState(50 + Z)
    traces = AC.ar1_traces(rng, K, T, baseline=0.2)
    truth = M.DeformableNMF(torch.tensor(sz), K, T, positions=positions(Z))
    truth.C = torch.from_numpy(traces).to("cuda", torch.float32)
    with torch.no_grad():
        video = truth.fp.forward(range(T), truth.C)[0].reshape(T, -1).clone()
    video += 0.05 * torch.from_numpy(rng.randn(*video.shape)).to(video)
    return sz, video, traces


def start(M, Z):
    sz, video, traces = planted(Z)
    model = M.DeformableNMF(torch.tensor(sz), K, T, positions=positions(Z))
    model.verbose = False
    model.C = torch.ones((K, T), dtype=torch.float32, device="cuda")
    return model, sz, video


@pytest.mark.parametrize("Z", [1, 2])
def test_update_footprints_is_the_op_on_the_models_gram_data(M, Z):
    from dnmf_amd import ops
    model, sz, video = start(M, Z)
    kw = dict(ar_g=G, ar_penalty=0.05, ar_baseline=0.2)
    model.update_footprints(M.ResidentLoader(video, sz, 8), 8, torch.tensor(sz), gamma_c=0, iter_c=2, solver='ar1', **kw)
    got = model.C.clone()
    ar = model.last_temporal_ar
    assert model.last_temporal_kkt is None and got.dtype == torch.float32 and tuple(got.shape) == (K, T)
    # the same on the model's own Gram data
    other, _, _ = start(M, Z)
    Gm, r = other._gram_rhs(video, torch.arange(T, dtype=torch.int32, device="cuda"))
    C = torch.ones((K, T), dtype=torch.float32, device="cuda")
    want, s, info = ops.ar1_temporal(Gm, r, C, G, 0.05, 0.2, sweeps=2, nbr=other._gram_nbr)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(ar["s"].view(torch.int64), s.view(torch.int64)) and tuple(ar["s"].shape) == (K, T)
    assert np.array_equal(ar["colour"], info["colour"]) and ar["n_colours"] == info["n_colours"] >= 2
    assert ar["colour"][0] != ar["colour"][1] and ar["colour"][2] != ar["colour"][3]      # the overlapping pairs
    assert ar["g"].tolist() == [G] * K and ar["penalty"].tolist() == [0.05] * K and ar["baseline"].tolist() == [0.2] * K
    f0, f1 = ar["F"]
    print(f"Z={Z}: F {f0:.6e} -> {f1:.6e}, colours {ar['colour'].tolist()}")
    assert np.isfinite(f0) and f1 <= f0 and f1 < f0 - 0.01 * abs(f0)                      # F does not rise (and falls from C = 1)
    model.update_footprints(M.ResidentLoader(video, sz, 8), 8, torch.tensor(sz), gamma_c=0, iter_c=1, solver='ar1', **kw)
    assert model.last_temporal_ar["F"][1] <= model.last_temporal_ar["F"][0] and abs(model.last_temporal_ar["F"][0] - f1) <= 1e-5 * abs(f1)
    assert bool(torch.isfinite(model.C).all()) and bool((model.C >= 0.2).all())
    # another solver afterwards: the record of this one goes
    model.update_footprints(M.ResidentLoader(video, sz, 8), 8, torch.tensor(sz), gamma_c=0, iter_c=1, solver='hals')
    assert model.last_temporal_ar is None and model.last_temporal_kkt is not None


def test_a_shuffled_loader_gives_the_same_traces(M):
    model, sz, video = start(M, 2)
    kw = dict(gamma_c=0, iter_c=2, solver='ar1', ar_g=G, ar_penalty=0.05, ar_baseline=0.2)
    model.update_footprints(M.ResidentLoader(video, sz, 8), 8, torch.tensor(sz), **kw)
    perm = np.random.RandomState(3).permutation(T)
    batches = [(video[torch.from_numpy(perm[i:i + 8]).cuda()].view(-1, *sz), torch.from_numpy(perm[i:i + 8].astype(np.int32)))
               for i in range(0, T, 8)]
    other, _, _ = start(M, 2)
    other.update_footprints(batches, 8, torch.tensor(sz), **kw)
    assert torch.equal(model.C.view(torch.int32), other.C.view(torch.int32))
    assert torch.equal(model.last_temporal_ar["s"].view(torch.int64), other.last_temporal_ar["s"].view(torch.int64))


def test_estimated_decay(M):
    """``ar_g=None``: K21's estimator on the current traces; a trace it cannot treat (constant: no autocovariance) gets g = 0."""
    from dnmf_amd import ops
    model, sz, video = start(M, 1)
    loader = M.ResidentLoader(video, sz, 8)
    model.update_footprints(loader, 8, torch.tensor(sz), gamma_c=0, iter_c=5, solver='hals')
    C = model.C.clone()
    C[5] = 1.0
    model.C = C.clone()
    model.update_footprints(loader, 8, torch.tensor(sz), gamma_c=0, iter_c=1, solver='ar1')
    est = ops.deconvolve_traces(C, penalty=0.0, baseline=0.0)[2]
    g = model.last_temporal_ar["g"]
    ok = est["ok"].cpu()
    assert not bool(ok[5]) and g[5] == 0.0 and bool(ok[:5].any())
    assert torch.equal(g[ok], est["g"].cpu()[ok]) and bool(((g[ok] > 0) & (g[ok] < 1)).all()) and bool((g[~ok] == 0).all())
    assert bool(torch.isfinite(model.C).all()) and model.last_temporal_ar["F"][1] <= model.last_temporal_ar["F"][0]


def test_refusals(M):
    model, sz, video = start(M, 2)
    loader = M.ResidentLoader(video, sz, 8)
    C = model.C.clone()
    with pytest.raises(ValueError, match="gamma_c"):
        model.update_footprints(loader, 8, torch.tensor(sz), gamma_c=0.01, solver='ar1', ar_g=G)
    with pytest.raises(ValueError, match="gamma_c"):
        model.fit(loader, loader, None, 8, outer=1, motion_solver='gn', gamma_c=0.01, solver='ar1', ar_g=G)
    gap = [(video[:8].view(-1, *sz), torch.arange(0, 8, dtype=torch.int32)), (video[9:17].view(-1, *sz), torch.arange(9, 17, dtype=torch.int32))]
    with pytest.raises(ValueError, match="consecutive"):
        model.update_footprints(gap, 8, torch.tensor(sz), gamma_c=0, solver='ar1', ar_g=G)
    shard = M.ResidentLoader(video[:20], sz, 8, t0=0, T_total=T)
    with pytest.raises(ValueError, match="shard"):
        model.update_footprints(shard, 8, torch.tensor(sz), gamma_c=0, solver='ar1', ar_g=G)
    model.group = object()
    with pytest.raises(ValueError, match="shard"):
        model.update_footprints(loader, 8, torch.tensor(sz), gamma_c=0, solver='ar1', ar_g=G)
    model.group = None
    multi = M.MultiChannelDNMF(torch.tensor(sz), K, T, torch.ones((2, K)), positions=positions(2))
    two = M.ResidentLoader(torch.cat((video, video), 1), sz, 8)
    with pytest.raises(ValueError, match="single-channel"):
        multi.update_footprints(two, 8, torch.tensor(sz), gamma_c=0, solver='ar1')
    with pytest.raises(ValueError, match="one channel"):
        multi.fit(two, two, None, 8, outer=1, motion_solver='gn', gamma_c=0, solver='ar1')
    with pytest.raises(ValueError, match="ar1_temporal: g"):
        model.update_footprints(loader, 8, torch.tensor(sz), gamma_c=0, solver='ar1', ar_g=1.0)
    with pytest.raises(ValueError, match="solver="):
        model.update_footprints(loader, 8, torch.tensor(sz), gamma_c=0, live_spatial=True, spatial_solver='ar1')
    assert torch.equal(model.C, C) and model.last_temporal_ar is None


def test_fit_runs_two_sweeps(M):
    model, sz, video = start(M, 2)
    loader = M.ResidentLoader(video, sz, 8)
    model.fit(loader, loader, None, 8, outer=1, epochs=1, gamma_c=0, iter_c=2, solver='ar1', motion_solver='gn', ar_g=G,
              ar_penalty=0.05, ar_baseline=0.2)
    ar = model.last_temporal_ar
    assert ar is not None and ar["F"][1] <= ar["F"][0] and tuple(model.C.shape) == (K, T)
    assert bool(torch.isfinite(model.C).all()) and bool(torch.isfinite(ar["s"]).all()) and bool((ar["s"] >= 0).all())
    print("median correlation with the planted traces: %.4f" % AC.median_correlation(model.C.cpu().numpy().astype(np.float64), planted(2)[2]))
