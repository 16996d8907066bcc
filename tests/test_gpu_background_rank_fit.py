"""The rank-R background term on the public surface (K23): ``DeformableNMF.update_background_rank`` / ``background_loader`` /
``fit(background=, background_rank=)``, the unchanged defaults and the refusals.

The videos are those of tests/test_gpu_background_fit.py (the model's own forward at a known ``C`` and a warp near the identity,
plus the planted decaying background ``b0 f0``) with a second, rising component ``b1 f1`` added: b1 a ramp the other way, f1 from
0.2 to 1.8 (mean 1).

Figures of the comparison as measured on the MI355X (outer=6, iter_c=30, Gauss-Newton motion with 4 iterations; median per-neuron
correlation of the traces with those of the same fit on the background-free video, and squared error |Y - M - background|^2):
  (24, 20, 2): background_rank=1  median 0.9260, squared error 1.308e+02;  background_rank=2  median 0.9113, squared error 6.399e+01
  (24, 20, 1): background_rank=1  median -0.1169, squared error 3.868e+02;  background_rank=2  median -0.1677, squared error 3.065e+02
The second component lowers the squared error on both; it does not improve the traces, which the first sweep has already fitted
to the raw frames.  On the exact model ``update_background`` leaves 3.964e+02 of the planted background's energy 7.620e+04 with rank
1 and 7.365e+01 with rank 2 at (24, 20, 2); 1.982e+02 and 3.683e+01 of 3.810e+04 at (24, 20, 1).
"""
import functools

import numpy as np
import pytest
import torch

import background_rank_restatement as RR
from test_gpu_background_fit import FIT, K, M, SHAPES, T, positions, prediction, problem, start, trace_correlations  # noqa: F401

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def problem2(M, sz):
    """The true model, the background-free video, and the video with both background components -- made once, never changed."""
    model, clean, b0, f0, dirty = problem(M, sz)
    g = np.meshgrid(*[np.linspace(0.0, 1.0, n) for n in sz], indexing="ij")
    b1 = torch.from_numpy((0.9 - 0.5 * g[0] - 0.2 * g[1]).reshape(-1)).to("cuda", torch.float32)
    f1 = torch.linspace(0.2, 1.8, T, device="cuda")
    return model, clean, dirty + f1[:, None] * b1[None, :]


def background_of(model):
    b, f = model.background
    if f.dim() == 1:
        return f[:, None] * b.reshape(-1)[None, :]
    return (f.double().t() @ b.reshape(b.shape[0], -1).double()).float()


# ---- 1. the exact model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sz", SHAPES)
def test_update_background_of_rank_two_and_its_loader(M, sz):
    """On the exact model Y - M is the planted rank-2 background: rank 2 must leave less of it than rank 1, and the loader serves
    max(Y - sum_j b_j f_j, 0) as the restatement computes it from the stored factors."""
    model, clean, dirty = problem2(M, sz)
    model.background = None
    loader = M.ResidentLoader(dirty, sz, 7)
    b, f = model.update_background_rank(loader, iters=6, rank=2)
    assert model.background[0] is b and model.background[1] is f
    assert tuple(b.shape) == (2,) + tuple(sz) and tuple(f.shape) == (2, T) and b.dtype == f.dtype == torch.float32 and b.is_cuda and f.is_cuda
    assert (b >= 0).all() and (f >= 0).all()
    assert (f.double().mean(1) - 1).abs().max().item() <= 1e-6
    left2 = ((dirty - clean - background_of(model)).double() ** 2).sum().item()
    cleaned = model.background_loader(loader)
    model.update_background(loader, iters=6)
    assert model.background[0].shape == tuple(sz) and model.background[1].shape == (T,)
    left1 = ((dirty - clean - background_of(model)).double() ** 2).sum().item()
    planted = ((dirty - clean).double() ** 2).sum().item()
    print(f"{sz}: of the planted background's energy {planted:.3e} rank 1 leaves {left1:.3e}, rank 2 leaves {left2:.3e}")
    assert left2 < left1

    assert isinstance(cleaned, M.ResidentLoader) and cleaned.batch_size == 7 and cleaned.sz == list(sz) and cleaned.T == T
    rows = cleaned.frames_2d()
    assert rows.data_ptr() != dirty.data_ptr() and float(rows.min()) >= 0
    want = RR.subtract(dirty.cpu().numpy(), b.cpu().numpy(), f.cpu().numpy())
    got = rows.cpu().numpy()
    assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))).all()
    served = list(zip(loader, cleaned))
    assert len(served) == 6 and [len(a[1]) for a, _ in served] == [7, 7, 7, 7, 7, 5]
    for (fr, idx), (fr_c, idx_c) in served:
        assert torch.equal(idx, idx_c) and torch.equal(fr_c.reshape(len(idx), -1), rows[idx.long()])
    assert torch.equal(loader.frames_2d(), dirty)
    model.background = None


def test_update_background_orders_a_shuffled_loader_by_time(M):
    """The blocks of the start are blocks of frame times: a loader that serves the frames in another order gives the same fit."""
    from torch.utils.data import DataLoader
    sz = SHAPES[0]
    model, _, dirty = problem2(M, sz)
    b, f = model.update_background_rank(M.ResidentLoader(dirty, sz, 7), iters=2, rank=2)
    host = dirty.cpu().reshape(T, *sz)

    class Shuffled(torch.utils.data.Dataset):
        def __len__(self):
            return T

        def __getitem__(self, i):
            return host[i], i

    served = DataLoader(Shuffled(), batch_size=7, shuffle=True, generator=torch.Generator().manual_seed(1))
    b2, f2 = model.update_background_rank(served, iters=2, rank=2)
    assert torch.equal(b, b2) and torch.equal(f, f2)
    model.background = None


# ---- 2. the comparison ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sz", SHAPES)
def test_fit_with_two_components_leaves_less_than_with_one(M, sz):
    _, clean, dirty = problem2(M, sz)

    def run(video, **kw):
        model = start(M, sz)
        loader = M.ResidentLoader(video, sz, 8)
        model.fit(loader, loader, None, 8, **kw, **FIT)
        return model

    C_clean = run(clean).C
    one, two = run(dirty, background=2, background_rank=1), run(dirty, background=2, background_rank=2)
    assert one.background[1].shape == (T,) and two.background[1].shape == (2, T) and two.background[0].shape == (2,) + tuple(sz)
    med = [float(np.median(trace_correlations(m.C, C_clean))) for m in (one, two)]
    err = [((dirty - prediction(m) - background_of(m)).double() ** 2).sum().item() for m in (one, two)]
    print(f"{sz}: background_rank=1  median correlation {med[0]:.4f}, squared error {err[0]:.3e};  "
          f"background_rank=2  median correlation {med[1]:.4f}, squared error {err[1]:.3e}")
    assert err[1] < err[0]
    assert (two.background[0] >= 0).all() and (two.background[1] >= 0).all()


# ---- 3. the defaults ------------------------------------------------------------------------------------------------------------
def test_rank_one_is_the_rank_one_path(M):
    """``update_background`` / ``ExponentialFP.background`` keep their signatures; rank 1 through the rank-R entry points and
    ``fit(background_rank=1)`` give their results bit for bit."""
    sz = SHAPES[0]
    model, _, dirty = problem2(M, sz)
    loader = M.ResidentLoader(dirty, sz, 7)
    b, f = (t.clone() for t in model.update_background(loader, 3))
    b1, f1 = model.update_background_rank(loader, 3, rank=1)
    assert torch.equal(b, b1) and torch.equal(f, f1)
    b1, f1 = model.update_background_rank(loader, 3, rank=1, inner=9)
    assert torch.equal(b, b1) and torch.equal(f, f1)
    model.background = None
    out = []
    for kw in ({}, {"background_rank": 1}):
        m = start(M, sz)
        loader = M.ResidentLoader(dirty, sz, 8)
        m.fit(loader, loader, None, 8, outer=2, epochs=2, iter_c=5, motion_solver='gn', background=2, **kw)
        out.append((m.background[0].clone(), m.background[1].clone(), m.C.clone(), m.fp.beta.detach().clone()))
    for x, y in zip(*out):
        assert torch.equal(x, y)
    video = dirty.reshape(T, *sz)
    for x, y in zip(M.ExponentialFP.background(video, iters=3), M.ExponentialFP.background_rank(video, iters=3, rank=1)):
        assert torch.equal(x, y)
    b2, f2 = M.ExponentialFP.background_rank(video.cpu().numpy(), iters=2, rank=2)
    assert isinstance(b2, np.ndarray) and b2.shape == (2,) + tuple(sz) and f2.shape == (2, T)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(M):
    sz = SHAPES[0]
    _, _, dirty = problem2(M, sz)
    loader = M.ResidentLoader(dirty, sz, 8)
    model = start(M, sz)
    shard = M.ResidentLoader(dirty[:20], sz, 8, t0=0, T_total=T)
    with pytest.raises(NotImplementedError, match="shard"):
        model.update_background_rank(shard, rank=2)
    with pytest.raises(NotImplementedError, match="shard"):
        model.fit(shard, shard, None, 8, outer=1, motion_solver='gn', background=1, background_rank=2)
    for rank in (0, 9, 1.5):
        with pytest.raises(ValueError, match="rank"):
            model.update_background_rank(loader, rank=rank)
        with pytest.raises(ValueError, match="background_rank"):
            model.fit(loader, loader, None, 8, outer=1, motion_solver='gn', background=1, background_rank=rank)
    few = M.DeformableNMF(torch.tensor(sz), K, 3, positions=positions(sz))
    few.C = torch.full((K, 3), 0.5, device="cuda")
    with pytest.raises(ValueError, match="rank=4 for the 3 frames"):
        few.update_background_rank(M.ResidentLoader(dirty[:3], sz, 3), rank=4)
    multi = M.MultiChannelDNMF(torch.tensor(sz), K, T, torch.ones(2, K), positions=positions(sz))
    two = M.ResidentLoader(torch.cat((dirty, dirty), 1), sz, 8)
    with pytest.raises(NotImplementedError, match="one channel only"):
        multi.update_background_rank(two, rank=2)
    with pytest.raises(NotImplementedError, match="one channel only"):
        multi.fit(two, two, None, 8, outer=1, motion_solver='gn', background=1, background_rank=2)
    assert model.background is None and multi.background is None
