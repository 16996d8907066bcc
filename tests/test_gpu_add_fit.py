"""``DeformableNMF.add_components`` on the planted video of tests/add_restatement.py: a model built on four of the six cells, at the
identity warp, grows by exactly the two it lacks.  The seed per depth is ``AR.FIT_SEED``: tests/test_add_host.py shows on the float64
definition that its four picks are the two cells and two noise peaks whose boxes reach neither."""
import numpy as np
import pytest
import torch

import add_restatement as AR
from test_gpu_add import ulp32

pytestmark = pytest.mark.gpu

T = 40


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd.Demix import dNMF
    return dNMF


def four_cell_model(M, depth):
    video, A6, traces, sz = AR.planted_video(depth, AR.FIT_SEED[depth])
    frames = torch.from_numpy(video).to("cuda")
    loader = M.ResidentLoader(frames, sz, 8)
    model = M.DeformableNMF(torch.tensor(sz), 4, T, positions=torch.from_numpy(AR.planted_centres(depth)[:4]).float())
    model.verbose = False
    torch.manual_seed(0)
    model.C = torch.rand(4, T, device="cuda")
    model.update_footprints(loader, 8, sz, gamma_c=0, iter_c=30, solver='hals')
    return model, loader, frames, A6, sz


def sse(model, frames):
    A = model.fp.A.reshape(model.fp.P, model.fp.K).double()
    return float(((frames.double() - (A @ model.C.double()).t()) ** 2).sum())


def state(model):
    fp = model.fp
    return dict(A=fp.A.clone(), pos=fp.pos.clone(), sigma=fp.sigma.clone(), C=model.C.clone(), A_unused=model.A.clone(),
                beta=fp.beta.detach().clone(), D=torch.from_numpy(model.D.copy()), K=torch.tensor([fp.K, model.C.shape[0]]))


@pytest.mark.parametrize("depth", [2, 1])
def test_adds_exactly_the_two_missing_cells(M, depth):
    from dnmf_amd import ops
    model, loader, frames, A6, sz = four_cell_model(M, depth)
    P = model.fp.P
    before, sse4 = state(model), sse(model, frames)
    model.last_evaluation = "kept until the model changes"

    dry = model.add_components(loader, n=4, dry_run=True)
    after = state(model)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert model.last_add is dry and model.last_evaluation is not None and model.fp.K == 4
    ratio = (dry["explained"] / dry["energy"]).cpu().numpy()
    print(f"\ndepth {depth}: centres {dry['centres'].cpu().numpy().round(1).tolist()} explained/energy {ratio.round(3)}")
    assert dry["added"] == 2 and dry["K"] == 6 and dry["kept"].tolist() == [True, True] + [False] * (len(ratio) - 2)
    assert dry["boxes"].dtype == torch.int32 and dry["ok"].dtype == torch.int32 and dry["kept"].dtype == torch.bool

    # the definition on what the method read: the frames registered as it registers them, the model's own fp32 prediction
    order = torch.arange(T, dtype=torch.int32, device="cuda")
    reg = model.registered_video(loader, interpolation='linear').cpu().numpy()
    sub = ops.halo_interior(model.fp.recon_image(model.C.contiguous(), order), sz).reshape(T, P).cpu().numpy()
    centres = dry["centres"].cpu().numpy().astype(np.float64)
    boxes = AR.candidate_boxes(centres, sz, AR.default_half(3.0, sz))
    assert dry["boxes"].tolist() == boxes.tolist()
    ref = AR.rank1_nmf(AR.residual_boxes(reg, sz, boxes, sub=sub), AR.box_sizes(boxes), AR.gaussian_start(boxes, centres, 3.0))
    for name in ("explained", "energy"):
        mag = ref["explained_mag"] if name == "explained" else ref["energy"]
        assert (np.abs(dry[name].cpu().numpy() - ref[name]) <= 1e-12 * mag).all(), name

    res = model.add_components(loader, n=4)
    assert res["added"] == 2 and model.last_add is res and model.last_evaluation is None and model.fp._layouts == {}
    fp = model.fp
    assert fp.K == 6 and tuple(fp.A.shape) == tuple(sz) + (6,) and fp.A.is_contiguous() and tuple(fp.pos.shape) == (6, 3)
    assert tuple(fp.sigma.shape) == (6,) and fp.sigma[4:].tolist() == [3.0, 3.0] and tuple(model.C.shape) == (6, T)
    assert tuple(model.A.shape) == (6, sz[0], sz[1]) and bool((model.A[4:] == 0).all()) and model.D.shape == tuple(sz) + (6,)
    assert torch.equal(fp.A[..., :4], before["A"]) and torch.equal(model.C[:4], before["C"]) and torch.equal(fp.pos[:4], before["pos"])
    assert np.array_equal(model.D[..., :4], before["D"].numpy()) and torch.equal(fp.beta.detach(), before["beta"])
    truth = AR.planted_centres(depth)[list(AR.MISSING)]
    grown = AR.grown(before["A"].reshape(P, 4).cpu().numpy(), before["C"].cpu().numpy(), before["pos"].cpu().numpy(),
                     before["sigma"].cpu().numpy(), before["D"].numpy(), sz, boxes, ref["a"].astype(np.float32),
                     ref["c"].astype(np.float32), [0, 1], np.arange(T), 3.0)
    A_new, C_new = fp.A.reshape(P, 6).cpu().numpy(), model.C.cpu().numpy()
    for q in range(2):
        com = fp.pos[4 + q].cpu().numpy()
        d = np.abs(com[None, :2] - truth[:, :2]).max(1)
        assert d.min() <= 1.0, (com, truth)
        u = AR.box_voxels(boxes[q], sz)
        n = u.size
        off = np.setdiff1d(np.arange(P), u)
        assert (A_new[off, 4 + q] == 0).all()
        assert (np.abs(A_new[u, 4 + q] - ref["a"][q, :n]) <= ulp32(ref["a"][q, :n]) + 1e-12 * ref["a_mag"][q, :n]).all()
        assert (np.abs(C_new[4 + q] - ref["c"][q]) <= ulp32(ref["c"][q]) + 1e-12 * ref["c_mag"][q]).all()
        cell = AR.MISSING[int(d.argmin())]
        print(f"depth {depth}: new component {4 + q} at {com.round(2)}: footprint corr with planted cell {cell} "
              f"{np.corrcoef(A_new[u, 4 + q], A6[u, cell])[0, 1]:.3f}")
        assert np.corrcoef(A_new[u, 4 + q], A6[u, cell])[0, 1] >= 0.95
    assert sorted(np.abs(fp.pos[4:, None, :2].cpu().numpy() - truth[None, :, :2]).max(2).argmin(1).tolist()) == [0, 1]
    np.testing.assert_allclose(fp.pos[4:].cpu().numpy(), grown["pos"][4:], atol=1e-5)
    np.testing.assert_allclose(model.D[..., 4:], grown["D"][..., 4:], atol=1e-6)

    # the grown model goes on, and explains more of the video than the four-component one did
    model.update_footprints(loader, 8, sz, gamma_c=0, iter_c=30, solver='hals')
    sse6 = sse(model, frames)
    print(f"depth {depth}: squared error {sse4:.2f} -> {sse6:.2f} (ratio {sse6 / sse4:.4f})")
    assert tuple(model.C.shape) == (6, T) and sse6 < sse4
    # nothing is left to add: the same call keeps nothing and leaves the model as it is
    again_before = state(model)
    again = model.add_components(loader, n=4)
    print(f"depth {depth}: second call explained/energy {(again['explained'] / again['energy']).cpu().numpy().round(3)}")
    assert again["added"] == 0 and again["K"] == 6
    for k, v in state(model).items():
        assert torch.equal(again_before[k], v), k


def test_given_centres_and_refusals(M):
    model, loader, frames, A6, sz = four_cell_model(M, 1)
    centres = np.concatenate([AR.planted_centres(1)[4:], AR.planted_centres(1, AR.NOTHING)])
    dry = model.add_components(loader, n=1, centres=centres, dry_run=True)
    assert dry["kept"].tolist() == [True, True, False, False] and dry["ok"].tolist() == [1, 1, 1, 1]
    # min_explained is a parameter: the same figures, another verdict
    strict = model.add_components(loader, n=1, centres=centres, min_explained=0.999, dry_run=True)
    assert strict["added"] == 0 and torch.equal(strict["explained"], dry["explained"])
    with pytest.raises(ValueError, match="n=0"):
        model.add_components(loader, n=0)
    with pytest.raises(ValueError, match="registered"):
        model.add_components(loader, n=2, registered='cubic')
    shard = M.ResidentLoader(loader.frames_2d()[:20], sz, 8, t0=0, T_total=T)
    with pytest.raises(NotImplementedError, match="shard"):
        model.add_components(shard, n=2)
    multi = M.MultiChannelDNMF(torch.tensor(sz), 2, T, torch.ones(2, 2), positions=torch.tensor([[5.0, 5.0, 0.0], [12.0, 6.0, 0.0]]))
    with pytest.raises(NotImplementedError, match="one channel"):
        multi.add_components(loader, n=2)
    assert model.fp.K == 4
