"""The rank-1 background term on the public surface (K19): ``DeformableNMF.update_background`` / ``background_loader`` /
``fit(background=)`` and the refusals.

The videos are the model's own forward at a known ``C`` and a warp near the identity, plus a planted background ``b0 f0``: b0 a
smooth ramp of the order of the footprint peaks, f0 decaying from 1.3 to 0.7 (mean 1).

Figures of the comparison as measured on the MI355X (outer=6, iter_c=30, Gauss-Newton motion with 4 iterations; median per-neuron
correlation of the traces with those of the same fit on the background-free video, and squared error):
  (24, 20, 2): background=0  median 0.6923, |Y - M|^2 = 4.549e+03;  background=2  median 0.8744, |Y - M - b f|^2 = 2.037e+01
  (24, 20, 1): background=0  median 0.0784, |Y - M|^2 = 8.963e+02;  background=2  median 0.1885, |Y - M - b f|^2 = 1.675e+02
The fit on the background-free video recovers the true traces (correlation >= 0.999).  At Z = 1 the six footprints of width 3
cover most of the 24 x 20 plane: the first sweep's traces absorb most of the background, little of it is left in the residual
for b, and the traces recover only in part; more sweeps do not change that.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(24, 20, 2), (24, 20, 1)]
K, T = 6, 40


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd.Demix import dNMF
    return dNMF


def positions(sz):
    z = [0.0, 1.0, 0.0, 1.0, 0.0, 1.0] if sz[2] > 1 else [0.0] * 6
    return torch.tensor([[5.0, 5.0, z[0]], [12.0, 6.0, z[1]], [19.0, 5.0, z[2]], [6.0, 14.0, z[3]], [12.0, 14.0, z[4]], [18.0, 15.0, z[5]]])


def new_model(M, sz):
    model = M.DeformableNMF(torch.tensor(sz), K, T, positions=positions(sz))
    model.verbose = False
    return model


@functools.lru_cache(maxsize=None)
def problem(M, sz):
    """The true model, its video (T, P) without background, the planted b0 (P,) and f0 (T,), and the contaminated video -- made
    once, never changed."""
    rng = np.random.RandomState(3 + sz[2])
    model = new_model(M, sz)
    # traces: a baseline with independent events, stationary over the session
    C = 0.4 + 0.2 * rng.rand(K, T)
    for k in range(K):
        for t0 in rng.choice(T - 4, 5, replace=False):
            C[k, t0:t0 + 4] += rng.uniform(0.6, 1.2) * np.array([1.0, 0.7, 0.45, 0.25])
    model.C = torch.from_numpy(C).to("cuda", torch.float32)
    shift = 0.25 * np.stack([np.sin(np.arange(T) / 5.0), np.cos(np.arange(T) / 7.0), np.zeros(T)])      # voxels; none along z
    with torch.no_grad():
        model.fp.beta[0] += torch.from_numpy(shift).to("cuda", torch.float32)
        clean = model.fp.forward(range(T), model.C)[0].reshape(T, -1).clone()
    g = np.meshgrid(*[np.linspace(0.0, 1.0, n) for n in sz], indexing="ij")
    b0 = torch.from_numpy((0.5 + 0.4 * g[0] + 0.3 * g[1]).reshape(-1)).to("cuda", torch.float32)
    f0 = torch.linspace(1.3, 0.7, T, device="cuda")
    dirty = clean + f0[:, None] * b0[None, :]
    assert float(clean.min()) >= 0 and float(clean.max()) <= 10 * float(b0.min() * f0.min())
    return model, clean, b0, f0, dirty


def prediction(model):
    with torch.no_grad():
        return model.fp.forward(range(T), model.C)[0].reshape(T, -1)


# ---- 1. the exact model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sz", SHAPES)
def test_update_background_recovers_the_planted_background(M, sz):
    """Y - M is b0 f0 up to the fp32 rounding of Y = M + b0 f0 (6e-8 |Y| / |b0 f0| <= 7e-7 per entry): one iteration from b = 1 is
    exact for a rank-1 residual."""
    model, clean, b0, f0, dirty = problem(M, sz)
    model.background = None
    loader = M.ResidentLoader(dirty, sz, 7)
    b, f = model.update_background(loader, iters=1)
    assert model.background[0] is b and model.background[1] is f
    assert tuple(b.shape) == sz and tuple(f.shape) == (T,) and b.dtype == f.dtype == torch.float32 and b.is_cuda and f.is_cuda
    got, want = (f[:, None] * b.reshape(-1)[None, :]).double(), (f0[:, None] * b0[None, :]).double()
    rel = ((got - want).abs() / want).max().item()
    print(f"{sz}: worst relative error of b f {rel:.2e}, mean f {f.double().mean().item():.8f}")
    assert rel <= 1e-5
    assert abs(f.double().mean().item() - 1) <= 1e-6

    cleaned = model.background_loader(loader)
    assert isinstance(cleaned, M.ResidentLoader) and cleaned.batch_size == 7 and cleaned.sz == list(sz) and cleaned.T == T
    assert not cleaned.shuffle and cleaned.generator is None
    rows = cleaned.frames_2d()
    assert rows.data_ptr() != dirty.data_ptr() and float(rows.min()) >= 0
    worst = (rows - clean).abs().max().item()
    print(f"{sz}: cleaned frames within {worst:.2e} of the background-free video (max {clean.max().item():.3f})")
    assert worst <= 1e-5 * clean.max().item()
    # the loader's order and batch boundaries
    served = list(zip(loader, cleaned))
    assert len(served) == 6 and [len(a[1]) for a, _ in served] == [7, 7, 7, 7, 7, 5]
    for (fr, idx), (fr_c, idx_c) in served:
        assert torch.equal(idx, idx_c) and fr_c.shape == fr.shape
        assert (fr_c.reshape(len(idx), -1) - clean[idx.long()]).abs().max().item() <= 1e-5 * clean.max().item()
    # the raw frames are untouched
    assert torch.equal(loader.frames_2d(), dirty)


def test_background_loader_keeps_a_shuffled_order(M):
    sz = SHAPES[0]
    model, clean, b0, f0, dirty = problem(M, sz)
    gen = torch.Generator().manual_seed(5)
    loader = M.ResidentLoader(dirty, sz, 7, shuffle=True, generator=gen)
    model.update_background(loader, iters=1)
    cleaned = model.background_loader(loader)
    assert cleaned.shuffle and cleaned.generator is gen
    gen.manual_seed(5)
    raw = [idx.tolist() for _, idx in loader]
    gen.manual_seed(5)
    got = [(fr, idx) for fr, idx in cleaned]
    assert [idx.tolist() for _, idx in got] == raw and sorted(t for b in raw for t in b) == list(range(T))
    assert raw != [list(range(s, min(T, s + 7))) for s in range(0, T, 7)]
    for fr, idx in got:
        assert (fr.reshape(len(idx), -1) - clean[idx.long()]).abs().max().item() <= 1e-5 * clean.max().item()


# ---- 2. the default of fit ------------------------------------------------------------------------------------------------------
def start(M, sz):
    """A model at the true positions with the identity warp and flat traces."""
    model = new_model(M, sz)
    model.C = torch.full((K, T), 0.5, device="cuda")
    return model


FIT = dict(outer=6, epochs=4, iter_c=30, motion_solver='gn')


@pytest.mark.parametrize("sz", SHAPES)
def test_fit_without_a_background_is_the_call_without_the_argument(M, sz):
    _, _, _, _, dirty = problem(M, sz)
    out = []
    for kw in ({}, {"background": 0}):
        model = start(M, sz)
        loader = M.ResidentLoader(dirty, sz, 8)
        model.fit(loader, loader, None, 8, outer=2, epochs=2, iter_c=5, motion_solver='gn', **kw)
        assert model.background is None
        out.append((model.fp.beta.detach().clone(), model.C.clone(), model.fp.A.clone()))
    for x, y in zip(*out):
        assert torch.equal(x, y)


# ---- 3. the comparison ----------------------------------------------------------------------------------------------------------
def trace_correlations(C, C_ref):
    C, C_ref = C.double().cpu().numpy(), C_ref.double().cpu().numpy()
    return np.array([np.corrcoef(C[k], C_ref[k])[0, 1] for k in range(K)])


@pytest.mark.parametrize("sz", SHAPES)
def test_fit_with_a_background_beats_the_fit_without(M, sz):
    """The yardstick is the existing fit on the background-free video.  On the contaminated video the fit with the background
    term must end closer to it, in the traces and in the squared error, than the fit without."""
    _, clean, b0, f0, dirty = problem(M, sz)

    def run(video, background):
        model = start(M, sz)
        loader = M.ResidentLoader(video, sz, 8)
        model.fit(loader, loader, None, 8, background=background, **FIT)
        return model

    C_clean = run(clean, 0).C
    plain, withbg = run(dirty, 0), run(dirty, 2)
    assert plain.background is None and withbg.background is not None
    med_plain = float(np.median(trace_correlations(plain.C, C_clean)))
    med_bg = float(np.median(trace_correlations(withbg.C, C_clean)))
    err_plain = ((dirty - prediction(plain)).double() ** 2).sum().item()
    b, f = withbg.background
    err_bg = ((dirty - prediction(withbg) - f[:, None] * b.reshape(-1)[None, :]).double() ** 2).sum().item()
    print(f"{sz}: background=0  median correlation {med_plain:.4f}, |Y - M|^2 = {err_plain:.3e};  "
          f"background=2  median correlation {med_bg:.4f}, |Y - M - b f|^2 = {err_bg:.3e}")
    assert med_bg > med_plain
    assert err_bg < err_plain
    assert (b >= 0).all() and (f >= 0).all()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(M):
    sz = SHAPES[0]
    _, _, _, _, dirty = problem(M, sz)
    loader = M.ResidentLoader(dirty, sz, 8)
    with pytest.raises(ValueError, match="no background"):
        start(M, sz).background_loader(loader)
    shard = M.ResidentLoader(dirty[:20], sz, 8, t0=0, T_total=T)
    model = start(M, sz)
    with pytest.raises(NotImplementedError, match="shard"):
        model.update_background(shard)
    with pytest.raises(NotImplementedError, match="shard"):
        model.fit(shard, shard, None, 8, outer=1, motion_solver='gn', background=1)
    with pytest.raises(ValueError, match="background"):
        model.fit(loader, loader, None, 8, outer=1, motion_solver='gn', background=-1)
    multi = M.MultiChannelDNMF(torch.tensor(sz), K, T, torch.ones(2, K), positions=positions(sz))
    two = M.ResidentLoader(torch.cat((dirty, dirty), 1), sz, 8)
    with pytest.raises(NotImplementedError, match="one channel only"):
        multi.update_background(two)
    with pytest.raises(NotImplementedError, match="one channel only"):
        multi.fit(two, two, None, 8, outer=1, motion_solver='gn', background=1)
    assert model.background is None and multi.background is None
