"""Component evaluation through the model: ``DeformableNMF.evaluate_components`` and ``select_components`` on the planted
video of tests/components_restatement.py -- six cells and a model of eight components, the last two on nothing -- after
a few sweeps of ``fit``.  The traces are the fitted ones, not the exact NNLS solution of the host test.

The video is made in footprint coordinates, so the fit has to find the warp that is the identity map.  At depth 2 that is
not the start: under the reference's un-normalisation the identity coefficients sample the two slices half a voxel off, and
the motion step has to move them -- Gauss-Newton does in three sweeps (measured on this seed: true cells r_values
0.91-0.98 and snr 3.4-8.0, the two on nothing 0.34-0.37 and 0.59-0.78; with Adam at lr 1e-3 the warp stays where it started
and five of the six cells fall below 0.5).  At depth 1 the z rows of the warp have nothing to hold them on this noise and
Gauss-Newton's free steps spoil the registration (measured: r_values of true cells down to 0.49, snr to 0.73), while
Adam's small steps stay at the start, which is right there up to half a voxel (true cells 0.90-0.99 and 2.7-8.7, on nothing
0.14-0.23 and -0.12-0.04).  So each depth is fitted with the motion solver that registers it; the thresholds are the defaults.
A known weakness, then, of the pair: the default thresholds separate the two groups only where the registration is good, and
neither motion solver registers both depths of this video in three sweeps."""
import functools

import numpy as np
import pytest
import torch

import components_restatement as CR

pytestmark = pytest.mark.gpu

T = 40
SEED = 0
DEPTHS = [2, 1]
MOTION = {2: "gn", 1: "adam"}


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd.Demix import dNMF
    return dNMF


@functools.lru_cache(maxsize=None)
def fitted(M, depth):
    """The fitted eight-component model, its loader and its evaluation -- made once; the tests that change a model copy it."""
    video, _, _, sz = CR.planted_video(depth, T, SEED)
    frames = torch.from_numpy(video).to("cuda", torch.float32)
    loader = M.ResidentLoader(frames, sz, 8)
    model = M.DeformableNMF(torch.tensor(sz), 8, T, positions=torch.from_numpy(CR.planted_centres(depth)).float())
    model.verbose = False
    torch.manual_seed(0)
    model.C = torch.rand(8, T, device="cuda")
    optimizer = torch.optim.Adam([model.fp.beta], lr=1e-3) if MOTION[depth] == "adam" else None
    model.fit(loader, loader, optimizer, 8, outer=3, epochs=2, iter_c=30, motion_solver=MOTION[depth])
    ev = model.evaluate_components(loader)
    return model, loader, sz, ev


@pytest.mark.parametrize("depth", DEPTHS)
def test_evaluate_keeps_the_six_cells_and_matches_the_restatement(M, depth):
    model, loader, sz, ev = fitted(M, depth)
    assert model.last_evaluation is ev
    print(f"\ndepth {depth}: r_values {ev['r_values'].cpu().numpy().round(3)}, snr {ev['snr'].cpu().numpy().round(2)}")
    assert ev["keep"].dtype == torch.bool and ev["keep"].tolist() == [True] * 6 + [False] * 2
    assert ev["n_active"] == 10 and tuple(ev["boxes"].shape) == (8, 6) and ev["boxes"].dtype == torch.int32
    assert tuple(ev["raw"].shape) == (8, T) and tuple(ev["frame_corr"].shape) == (8, T)
    assert tuple(ev["images"].shape) == (8, int((ev["boxes"][:, 1::2] - ev["boxes"][:, 0::2] + 1).prod(1).max()))
    # the same figures from the restatement on the model's own fp32 footprints and traces, the frames registered as the method
    # registers them
    P = sz[0] * sz[1] * sz[2]
    A = model.fp.A.reshape(P, 8).cpu().numpy()
    C = model.C.cpu().numpy()
    reg = model.registered_video(loader, interpolation='linear').cpu().numpy()
    sub = (A.astype(np.float64) @ C.astype(np.float64)).T
    ref = CR.evaluate(reg, sz, A, C, sub=sub)
    assert ev["boxes"].tolist() == ref["boxes"].tolist()
    assert ref["keep"].tolist() == ev["keep"].tolist()
    # S_t is an fp32 sum in the kernel's reconstruction image and float64 here: 8 terms of at most ~3, 1e-6 on e of order 1
    np.testing.assert_allclose(ev["r_values"].cpu().numpy(), ref["r_values"], atol=1e-4)
    np.testing.assert_allclose(ev["raw"].cpu().numpy(), ref["raw"], atol=1e-4)
    np.testing.assert_allclose(ev["snr"].cpu().numpy(), ref["snr"], rtol=1e-3, atol=1e-3)
    # registered=None is the same thing at the identity warp only; 'nearest' runs
    for registered in (None, 'nearest'):
        other = model.evaluate_components(loader, registered=registered)
        assert other["keep"].tolist() == [True] * 6 + [False] * 2
    model.last_evaluation = ev
    # thresholds are parameters
    assert model.evaluate_components(loader, min_r=-1.0, min_snr=-1e9)["keep"].all()
    assert not model.evaluate_components(loader, min_r=1.1)["keep"].any()
    model.last_evaluation = ev


@pytest.mark.parametrize("depth", DEPTHS)
def test_select_components_shrinks_the_model_in_place(M, depth):
    import copy
    base, loader, sz, ev = fitted(M, depth)
    model = copy.copy(base)
    model.fp = copy.copy(base.fp)
    model.fp.invalidate_layouts()
    model._warned = set()
    with torch.no_grad():
        model.fp.beta = base.fp.beta.detach().clone().requires_grad_(True)
    old_A, old_C, old_beta = base.fp.A.clone(), base.C.clone(), base.fp.beta.detach().clone()
    old_pos, old_D = base.fp.pos.clone(), None if base.D is None else base.D.copy()
    assert model.select_components(ev["keep"]) == 6
    assert model.fp.K == 6 and tuple(model.C.shape) == (6, T) and tuple(model.fp.A.shape) == tuple(sz) + (6,)
    assert torch.equal(model.C, old_C[:6]) and torch.equal(model.fp.A, old_A[..., :6]) and model.fp.A.is_contiguous()
    assert torch.equal(model.fp.pos, old_pos[:6]) and tuple(model.fp.sigma.shape) == (6,)
    assert torch.equal(model.fp.beta.detach(), old_beta) and model.fp.beta.requires_grad
    assert old_D is None or (model.D.shape[-1] == 6 and np.array_equal(model.D, old_D[..., :6]))
    assert model.last_evaluation is None and model._ws_k3 is None and model._S_bufs is None and model.fp._layouts == {}
    assert base.fp.K == 8 and tuple(base.C.shape) == (8, T)            # the copy's owner is untouched
    # the shrunk model goes on: a footprint / trace update, a motion update, and an evaluation that keeps all six
    model.update_footprints(loader, 8, sz, gamma_c=0, iter_c=5)
    model.update_motion(loader, None, epochs=1, solver='gn')
    assert bool(torch.isfinite(model.fp.beta).all())
    assert tuple(model.C.shape) == (6, T)
    again = model.evaluate_components(loader)
    assert again["keep"].tolist() == [True] * 6
    # indices, in the order given
    two = copy.copy(model)
    two.fp = copy.copy(model.fp)
    kept_C = model.C.clone()
    assert two.select_components([4, 1]) == 2
    assert torch.equal(two.C, kept_C[[4, 1]]) and torch.equal(two.fp.A, model.fp.A[..., [4, 1]])


def test_refusals(M):
    model, loader, sz, ev = fitted(M, 1)
    import copy
    m = copy.copy(model)
    m.fp = copy.copy(model.fp)
    for bad in ([], torch.zeros(8, dtype=torch.bool), [8], [-1], torch.ones(7, dtype=torch.bool), [0.5]):
        with pytest.raises(ValueError):
            m.select_components(bad)
    assert m.fp.K == 8
    with pytest.raises(ValueError, match="registered"):
        model.evaluate_components(loader, registered='cubic')
    with pytest.raises(ValueError, match="active"):
        model.evaluate_components(loader, active=0)
    shard = M.ResidentLoader(loader.frames_2d()[:20], sz, 8, t0=0, T_total=T)
    with pytest.raises(NotImplementedError, match="shard"):
        model.evaluate_components(shard)
    multi = M.MultiChannelDNMF(torch.tensor(sz), 2, T, torch.ones(2, 2), positions=torch.tensor([[5.0, 5.0, 0.0], [12.0, 6.0, 0.0]]))
    with pytest.raises(NotImplementedError, match="one channel"):
        multi.evaluate_components(loader)
    with pytest.raises(NotImplementedError, match="one channel"):
        multi.select_components([0])


def test_demo_prints_the_evaluation():
    """``examples/demo_headless.py --evaluate`` on its shortest fit: the three lines are there and hold one entry per neuron."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "demo_headless.py"), "--quiet", "--outer", "1", "--epochs", "1",
                          "--iter-c", "5", "--evaluate"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    lines = out.stdout.splitlines()
    r = [ln for ln in lines if ln.startswith("component evaluation over 25 active frames each: r_values")]
    snr = [ln for ln in lines if ln.startswith("snr ")]
    keep = [ln for ln in lines if ln.startswith("keep ")]
    assert len(r) == 1 and len(snr) == 1 and len(keep) == 1, out.stdout[-1500:]
    assert len(r[0].split("[")[1].split("]")[0].split()) == 10 and len(snr[0].split("[")[1].split("]")[0].split()) == 10
    flags = keep[0].split("[")[1].split("]")[0].split()
    assert len(flags) == 10 and set(flags) <= {"0", "1"} and keep[0].endswith("(%d of 10)" % flags.count("1"))
