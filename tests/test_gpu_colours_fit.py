"""MultiChannelDNMF.update_colours and fit(learn_colours=) on the planted three-channel model of tests/colours_restatement.py:
24 x 20 x 2 and 24 x 20 x 1, K = 6, T = 40, NC = 3, identity warp."""
import numpy as np
import pytest
import torch

import colours_restatement as R
from test_gpu_colours import SOLVE_COLOUR_DEV, SOLVE_KKT_DEV

pytestmark = pytest.mark.gpu

NC, K, T = 3, 6, 40


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd.Demix import dNMF
    return dNMF


_PLANTED = {}


def planted(depth, seed, noise=0.0):
    if (depth, seed, noise) not in _PLANTED:
        _PLANTED[depth, seed, noise] = R.planted(depth, seed, noise=noise, T=T, NC=NC)
    return _PLANTED[depth, seed, noise]


def model(M, depth, C, colours=None, cls=None):
    import components_restatement as CR
    sz = [24, 20, depth]
    pos = torch.from_numpy(CR.planted_centres(depth)[:K]).float()
    if cls is None:
        dn = M.MultiChannelDNMF(torch.tensor(sz), K, T, torch.ones(NC, K) if colours is None else colours, positions=pos)
    else:
        dn = cls(torch.tensor(sz), K, T, positions=pos)
    dn.verbose = False
    dn.C = torch.from_numpy(np.ascontiguousarray(C)).to("cuda", torch.float32)
    return dn, sz


def frames_of(p):
    return torch.from_numpy(p["video"]).to("cuda", torch.float32)


@pytest.mark.parametrize("depth", [2, 1])
def test_update_colours_reproduces_the_restatement(M, depth):
    """From all-ones colours on the noise-free planted video: the model's result against the restatement fed with the model's own
    G and r (fp32, from the Gram kernel the model chose) and its fp32 traces, within the bound of test_gpu_colours (colours
    and traces rounded to fp32 as the model rounds its own); the planted colours come back to the fp32 floor of G and r."""
    p = planted(depth, 0)
    dn, sz = model(M, depth, p["C"])
    P = 24 * 20 * depth
    frames = frames_of(p)
    loader = M.ResidentLoader(frames, sz, 8)
    order = torch.arange(T, dtype=torch.int32, device="cuda")
    G = r = None
    rs = []
    for c in range(NC):
        Gc, rc = dn._gram_rhs_one(dn.fp, frames[:, c * P:(c + 1) * P], order)
        G = Gc if G is None else G
        rs.append(rc.cpu().numpy())
    C0, A0 = dn.C.clone(), dn.fp.A.clone()
    want = R.update(G.cpu().numpy(), np.stack(rs), C0.cpu().numpy(), np.ones((NC, K), np.float32), sweeps=10, normalise_=False)
    x32 = want["colours"].astype(np.float32).astype(np.float64)              # the solver's one rounding, then the driver's
    col, Cn, scale, ok = R.normalise(x32, np.ones((NC, K)), C0.cpu().numpy().astype(np.float64), np.diag(want["M"]))
    out = dn.update_colours(loader, sweeps=10)
    assert out is dn.last_colours and out["colours"] is dn.colours and dn.colours.dtype == torch.float32
    dc = np.abs(dn.colours.cpu().numpy().astype(np.float64) - col.astype(np.float32)).max()
    dC = np.abs(dn.C.cpu().numpy().astype(np.float64) - Cn.astype(np.float32)).max()
    dk = np.abs(out["kkt"].cpu().numpy() - want["kkt"]).max()
    ds = np.abs(out["scale"].cpu().numpy() - scale).max()
    err = np.abs(dn.colours.cpu().numpy() - p["colours"]).max()
    print(f"\ndepth {depth}: colours deviate by {dc:.3e}, traces {dC:.3e}, kkt {dk:.3e}, scale {ds:.3e}; colour error against the "
          f"planted colours {err:.3e}; kkt {out['kkt_before'].cpu().numpy()} -> {out['kkt'].cpu().numpy()}")
    assert dc <= 10 * SOLVE_COLOUR_DEV and dC <= 10 * SOLVE_COLOUR_DEV and dk <= 10 * SOLVE_KKT_DEV and ds <= 10 * SOLVE_COLOUR_DEV
    assert out["ok"].cpu().tolist() == ok.tolist() == [True] * K and out["ok_channel"].cpu().tolist() == [True] * NC
    assert torch.equal(out["colours_before"], torch.ones(NC, K, device="cuda"))
    assert out["objective"] < out["objective_before"] and bool((out["kkt"] < out["kkt_before"]).all())
    # fp32 footprints, G, r and traces: at worst n 2^-24 relative over the n <= 960 voxels of a sum, once for G and once for r
    assert err <= 2 * 960 * 2.0 ** -24
    assert torch.equal(dn.fp.A, A0) and dn.colours.max(0).values.tolist() == [1.0] * K
    # the channel cache serves the new colours
    for c, (f, cols) in enumerate(dn._channels()):
        assert torch.equal(f.A, dn.fp.A * dn.colours[c]) and cols == slice(c * P, (c + 1) * P)


def test_dry_run_leaves_the_model_bit_for_bit(M):
    p = planted(2, 1, 0.3)
    dn, sz = model(M, 2, p["C"])
    loader = M.ResidentLoader(frames_of(p), sz, 8, shuffle=True, generator=torch.Generator().manual_seed(3))
    chans = dn._channels()
    col, C, A, nbr = dn.colours, dn.C, dn.fp.A, dn._gram_nbr
    c0, C0, A0 = col.clone(), C.clone(), A.clone()
    dry = dn.update_colours(loader, sweeps=10, dry_run=True)
    assert dn.colours is col and dn.C is C and dn.fp.A is A and dn._gram_nbr is nbr and dn.last_colours is None
    assert torch.equal(col, c0) and torch.equal(C, C0) and torch.equal(A, A0) and dn._channels() is chans
    real = dn.update_colours(loader, sweeps=10)                         # the loader's order does not matter: frames go by time
    assert torch.equal(real["colours"], dry["colours"]) and torch.equal(real["kkt"], dry["kkt"])
    assert not torch.equal(dn.colours, c0) and dn.colours is not col and dn._channels() is not chans
    # the model is the same model: colours[c, k] C[k, t] moved by the fp32 roundings only
    before = (real["colours_before"].double()[:, :, None] * C0.double()[None]).cpu().numpy()
    prod = (dn.colours.double()[:, :, None] * dn.C.double()[None]).cpu().numpy()
    unnorm = (dn.colours.double() * real["scale"][None, :])[:, :, None].cpu().numpy() * C0.double()[None].cpu().numpy()
    np.testing.assert_allclose(prod, unnorm, rtol=3 * 2.0 ** -24)
    assert np.abs(prod - before).max() > 0.1


def test_refusals(M):
    p = planted(1, 0)
    dn, sz = model(M, 1, p["C"])
    frames = frames_of(p)
    with pytest.raises(ValueError, match="rows of"):
        dn.update_colours(M.ResidentLoader(frames[:, :2 * 480].contiguous(), sz, 8))
    with pytest.raises(ValueError, match="sweeps"):
        dn.update_colours(M.ResidentLoader(frames, sz, 8), sweeps=0)
    with pytest.raises(NotImplementedError, match="shard of the frames"):
        dn.update_colours(M.ResidentLoader(frames[:20].contiguous(), sz, 8, t0=0, T_total=T))
    dn.group = object()
    with pytest.raises(NotImplementedError, match="shard of the frames"):
        dn.update_colours(M.ResidentLoader(frames, sz, 8))
    single, _ = model(M, 1, p["C"], cls=M.DeformableNMF)
    assert not hasattr(single, "update_colours")
    one = M.ResidentLoader(frames[:, :480].contiguous(), sz, 8)
    with pytest.raises(ValueError, match="learn_colours"):
        single.fit(one, one, torch.optim.Adam([single.fp.beta], lr=1e-3), 8, outer=1, epochs=1, learn_colours=3)
    with pytest.raises(ValueError, match="learn_colours"):
        dn.fit(one, one, None, 8, learn_colours=-1)


def restatement_fit(p, learn, outer=2, iter_c=5):
    """The alternation fit() runs, in float64 under the identity warp: ``iter_c`` multiplicative trace updates on the channel
    sums, then (``learn`` > 0) a colour update of ``learn`` sweeps -> (colour error, squared error)."""
    A, video = p["A"], p["video"]
    P = A.shape[0]
    rng = np.random.default_rng(17)
    C = 0.3 + rng.random((K, T))
    col = np.ones((NC, K))
    Gu, r = R.gram_rhs(A, video, NC)
    for _ in range(outer):
        Gc = sum(Gu[0] * np.outer(col[c], col[c]) for c in range(NC))
        rc = sum(r[c] * col[c][None, :] for c in range(NC))
        for _ in range(iter_c):
            C = C * rc.T / (Gc @ C + 1e-32)
        if learn:
            u = R.update(Gu, r, C, col, sweeps=learn)
            col, C = u["colours"], u["C"]
    sq = sum(((video[:, c * P:(c + 1) * P].T - (A * col[c][None, :]) @ C) ** 2).sum() for c in range(NC))
    return np.abs(col - p["colours"]).max(), sq, C


@pytest.mark.parametrize("depth,seed", [(2, 0), (2, 1), (1, 0), (1, 2)])
def test_fit_learns_the_colours(M, depth, seed):
    """fit(learn_colours=5) against fit(learn_colours=0) from all-ones colours on the noisy planted video (noise 0.3), Adam with
    lr = 1e-3, outer = 2, epochs = 1, iter_c = 5 as the fit of tests/test_gpu_multichannel_footprints.py: a smaller colour error
    and a smaller squared error.  Seeds checked on the CPU with ``restatement_fit`` (the same alternation in float64, identity
    warp): 0, 1, 2 at both depths, all six showing the same ordering (colour error 1.0 -> 0.14 .. 0.28, squared error 13 .. 26 %
    lower); used here, and asserted on the restatement first: (depth 2: 0, 1), (depth 1: 0, 2).  Measured on the MI355X: colour
    error 1.0 -> 0.255, 0.159, 0.320, 0.324; squared error 9.0, 10.9, 11.4, 14.0 % lower."""
    p = planted(depth, seed, 0.3)
    e5, s5, _ = restatement_fit(p, 5)
    e0, s0, _ = restatement_fit(p, 0)
    assert e5 < e0 and s5 < s0
    frames = frames_of(p)
    C0 = 0.3 + np.random.default_rng(17).random((K, T))
    res = {}
    for learn in (0, 5):
        dn, sz = model(M, depth, C0)
        P = dn.fp.P
        train = M.ResidentLoader(frames, sz, 8, shuffle=True, generator=torch.Generator().manual_seed(0))
        test = M.ResidentLoader(frames, sz, 8)
        opt = torch.optim.Adam([dn.fp.beta], lr=1e-3)
        dn.fit(train, test, opt, 8, outer=2, gamma=1, epochs=1, gamma_c=0, iter_c=5, learn_colours=learn)
        with torch.no_grad():
            G, r = dn._gram_rhs(frames, torch.arange(T, dtype=torch.int32, device="cuda"))
            Cd = dn.C.double()
            sq = float(torch.einsum("kt,tkl,lt->", Cd, G.double(), Cd) - 2 * (r.double().T * Cd).sum() + (frames.double() ** 2).sum())
        res[learn] = (float((dn.colours.cpu() - torch.from_numpy(p["colours"])).abs().max()), sq, dn)
    print(f"\ndepth {depth} seed {seed}: colour error {res[0][0]:.3f} -> {res[5][0]:.3f} (float64 {e0:.3f} -> {e5:.3f}); squared "
          f"error {res[0][1]:.2f} -> {res[5][1]:.2f} (float64 {s0:.2f} -> {s5:.2f})")
    assert res[5][0] < res[0][0] and res[5][1] < res[0][1]
    assert torch.equal(res[0][2].colours, torch.ones(NC, K, device="cuda")) and res[0][2].last_colours is None
    assert res[5][2].last_colours is not None


def test_learn_colours_zero_is_the_path_without_the_keyword(M):
    p = planted(2, 0, 0.3)
    frames = frames_of(p)
    C0 = 0.3 + np.random.default_rng(17).random((K, T))
    got = []
    for kw in ({}, dict(learn_colours=0)):
        dn, sz = model(M, 2, C0)
        train = M.ResidentLoader(frames, sz, 8, shuffle=True, generator=torch.Generator().manual_seed(0))
        test = M.ResidentLoader(frames, sz, 8)
        dn.fit(train, test, torch.optim.Adam([dn.fp.beta], lr=1e-3), 8, outer=2, gamma=1, epochs=1, gamma_c=0, iter_c=5, **kw)
        got.append(dn)
    a, b = got
    assert torch.equal(a.fp.beta, b.fp.beta) and torch.equal(a.C, b.C) and torch.equal(a.colours, b.colours)
