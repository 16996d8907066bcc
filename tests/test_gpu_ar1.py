"""K32 on the GPU: ``ops.ar1_temporal`` and ``ops.ar1_temporal_step`` against the float64 restatement (tests/ar1_restatement.py) on
identical seeded Gram data (``ar1_cases.gram_data``: symmetric, positive diagonal, a sparse band pattern).

Per size K x T two variants.  'nbr': the neighbour table is given (padded with -1), penalties 0 and > 0 and baselines 0 and != 0
mixed over the neurons, one neuron with g = 0 (K > 1).  'dense': no table, penalty 0, baseline 0, and at K = 1 the one neuron has
g = 0.  In both, neuron 0 has frames without weight leading, in the middle (whole segments of lanes) and trailing, the last neuron a
NaN, an infinite and a negative diagonal entry.  C is a view into a wider buffer filled with 1e6, so that a read or a write past a
row shows.

The float64 state and s after 1 and 3 sweeps: the kernel forms w, y and the pool records with the restatement's operations in the
restatement's order, so they enter the solve with equal bits; the two then differ in g^l alone (``exp(l log g)`` here, ``g ** l``
there) and in what follows from it.  The largest deviation from the restatement, relative to max |y - b| of the row, measured on the
MI355X over all the cases below: 1.25e-15 (``MEASURED_DEV``); ten times that is asserted.  Pool counts,
weightless counts and colours are equal, and two runs give the same bits.
"""
import functools

import numpy as np
import pytest
import torch

import ar1_cases as AC
import ar1_restatement as R

pytestmark = pytest.mark.gpu

G = AC.G_TRUE
KS = [1, 6, 65]
TS = [1, 2, 7, 1023, 1024, 1025, 4099, 6144]
MEASURED_DEV = 1.25e-15   # K = 65, T = 4099, no table, after one sweep
BOUND = 10 * MEASURED_DEV


def parameters(K, variant):
    k = np.arange(K)
    if variant == "dense":
        return np.full(K, 0.0 if K == 1 else G), np.zeros(K), np.zeros(K)
    g = np.where(k % 3 == 2, 0.6, G)
    if K > 1:
        g[K // 2] = 0.0
    return g, np.where(k % 2 == 0, 0.3, 0.0), np.where(k % 4 == 1, 0.0, 1.0 - 0.25 * (k % 3))


@functools.lru_cache(maxsize=None)
def case(K, T, variant):
    """The inputs and the restatement's states after 1 and 3 sweeps; computed once, never changed."""
    Gm, r, _, pat = AC.gram_data(K, T, 100 * K + T, baseline=1.0 if variant == "nbr" else 0.0)
    AC.without_weight(Gm, r, K, T)
    nbr = AC.nbr_table(pat) if variant == "nbr" else None
    g, lam, b = parameters(K, variant)
    C0 = (1.0 + np.random.RandomState(T).rand(K, T)).astype(np.float32)
    one = R.ar1_temporal(Gm, r, C0, g, lam, b, sweeps=1, nbr=nbr)
    three = R.ar1_temporal(Gm, r, one[0], g, lam, b, sweeps=2, nbr=nbr)
    for v in (Gm, r, C0):
        v.setflags(write=False)
    return Gm, r, C0, nbr, (g, lam, b), one, three, row_scale(Gm, r, C0, nbr, b)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def strided(x, pad=5):
    buf = torch.full((x.shape[0], x.shape[1] + pad), 1.0e6, dtype=torch.float32, device="cuda")
    buf[:, :x.shape[1]] = torch.tensor(x).cuda()
    return buf, buf[:, :x.shape[1]]


def row_scale(Gm, r, C_before, nbr, b):
    """max |y - b| per row over the weighted frames of the first step's terms, at least 1."""
    K = len(C_before)
    lists = R.neighbour_lists(K, nbr)
    out = np.ones(K)
    G64, r64, C64 = Gm.astype(np.float64), r.astype(np.float64), C_before.astype(np.float64)
    for k in range(K):
        w, y = R.row_terms(G64, r64, C64, k, lists[k])
        ok = R.weighted(w, y)
        if ok.any():
            out[k] = max(1.0, np.abs(y[ok] - b[k]).max())
    return out


def deviation(got, want, scale):
    return float((np.abs(got - want) / scale[:, None]).max())


@pytest.mark.parametrize("variant", ["nbr", "dense"])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("K", KS)
def test_sweeps_against_the_restatement(ops, K, T, variant):
    Gm, r, C0, nbr, (g, lam, b), one, three, scale = case(K, T, variant)
    Gd, rd = torch.tensor(Gm).cuda(), torch.tensor(r).cuda()
    nd = None if nbr is None else torch.from_numpy(nbr).cuda()
    worst = 0.0
    for sweeps, want in ((1, one), (3, three)):
        buf, view = strided(C0)
        C, s, info = ops.ar1_temporal(Gd, rd, view, g, lam, torch.from_numpy(b), sweeps=sweeps, nbr=nd)
        buf2, view2 = strided(C0)
        again = ops.ar1_temporal(Gd, rd, view2, g, lam, torch.from_numpy(b), sweeps=sweeps, nbr=nd)
        torch.cuda.synchronize()
        assert C is view and bool((buf[:, T:] == 1.0e6).all())                      # in place, nothing past a row
        assert s.dtype == torch.float64 and info["state"].dtype == torch.float64 and tuple(s.shape) == (K, T)
        assert torch.equal(C, info["state"].float())                                # one rounding to fp32 at the end
        for x, y in ((C, again[0]), (s, again[1]), (info["state"], again[2]["state"])):
            assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))   # the same bits
        wC, ws, winfo = want
        assert np.array_equal(info["colour"], winfo["colour"]) and info["n_colours"] == winfo["n_colours"]
        assert np.array_equal(info["n_weightless"].cpu().numpy(), winfo["n_weightless"])
        assert np.array_equal(info["n_pools"].cpu().numpy(), winfo["n_pools"])
        state, sg = info["state"].cpu().numpy(), s.cpu().numpy()
        assert np.isfinite(state).all() and np.isfinite(sg).all()
        dC, ds = deviation(state, wC, scale), deviation(sg, ws, scale)
        worst = max(worst, dC, ds)
        print(f"K={K} T={T} {variant} sweeps={sweeps}: state {dC:.2e} s {ds:.2e}")
        assert dC <= BOUND and ds <= BOUND
        assert sg.min() >= 0.0 and (state[:, 0] - b).min() >= 0.0
    print(f"K={K} T={T} {variant}: largest deviation {worst:.2e}")


def test_the_cases_contain_what_they_claim():
    """Host only: the frames without weight, the pools across lane segments and the colours of the inputs above."""
    Gm, r, C0, nbr, (g, lam, b), one, three, scale = case(6, 4099, "nbr")
    K, T = C0.shape
    info = one[2]
    assert info["n_colours"] == 3 and (g[K // 2] == 0.0) and (lam > 0).any() and (lam == 0).any() and (b != 0).any() and (b == 0).any()
    assert (nbr == -1).any()
    gap = T // 8
    assert info["n_weightless"][0] == 3 + gap + 2 and gap > 100 * 5                 # a hundred lanes of 5 frames without weight
    assert info["n_weightless"][K - 1] == 3 and (info["n_weightless"][1:K - 1] == 0).all()
    assert info["n_pools"][K // 2] == T                                             # g = 0: every frame its own pool
    assert (info["n_pools"][[0, 4]] < 0.9 * T).all() and (info["n_pools"][[0, 4]] > T // 20).all()   # pools across the lane segments
    s = one[1]
    assert (s[0, T // 3:T // 3 + gap] == 0).all() and (one[0][0, :3] == b[0]).all()  # decays through the gap; leading: baseline
    assert case(1, 7, "dense")[4][0][0] == 0.0 and case(65, 7, "dense")[5][2]["n_colours"] == 3


def test_step_runs_one_colour(ops):
    """``ar1_temporal_step`` on the neurons of one colour is the restatement's row steps on them; the other rows keep their bits."""
    K, T = 6, 1025
    Gm, r, C0, nbr, (g, lam, b), one, three, scale = case(K, T, "nbr")
    Gd, rd, nd = torch.tensor(Gm).cuda(), torch.tensor(r).cuda(), torch.from_numpy(nbr).cuda()
    colour, n = ops.trace_colours(nd)
    ids = np.flatnonzero(colour == 1)
    assert len(ids) >= 2
    state = torch.from_numpy(C0.astype(np.float64)).cuda()
    before = state.clone()
    C, s, counts = ops.ar1_temporal_step(Gd, rd, state, ids, g, lam, b, nbr=nd)
    torch.cuda.synchronize()
    assert C is state and counts.dtype == torch.int32 and tuple(counts.shape) == (K, 2)
    rest = np.setdiff1d(np.arange(K), ids)
    assert torch.equal(state[rest], before[rest]) and bool((s[rest] == 0).all()) and bool((counts[rest] == 0).all())
    lists = R.neighbour_lists(K, nbr)
    for k in ids:
        w, y = R.row_terms(Gm.astype(np.float64), r.astype(np.float64), C0.astype(np.float64), k, lists[k])
        row, sk, n_pools, n_weightless = R.row_step(w, y, g[k], lam[k], b[k])
        assert counts[k].tolist() == [n_pools, n_weightless]
        assert np.abs(state[k].cpu().numpy() - row).max() <= BOUND * scale[k] and np.abs(s[k].cpu().numpy() - sk).max() <= BOUND * scale[k]
    with pytest.raises(ValueError, match="ids are distinct"):
        ops.ar1_temporal_step(Gd, rd, state, [0, 0], g, lam, b, nbr=nd)
    with pytest.raises(ValueError, match="ids are distinct"):
        ops.ar1_temporal_step(Gd, rd, state, [K], g, lam, b, nbr=nd)


def test_refusals(ops):
    """T = 6145 is refused, never cut; so are K > 4096, a decay outside [0, 1) and a negative penalty; nothing is written."""
    K, T = 2, 6145
    Gd, rd = torch.zeros((T, K, K), dtype=torch.float32, device="cuda"), torch.zeros((T, K), dtype=torch.float32, device="cuda")
    C = torch.ones((K, T), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="6144"):
        ops.ar1_temporal(Gd, rd, C, G)
    with pytest.raises(ValueError, match="6144"):
        ops.ar1_temporal_step(Gd, rd, C.double(), [0], G, 0.0, 0.0)
    K, T = 4097, 1
    with pytest.raises(ValueError, match="4096"):
        ops.ar1_temporal(torch.zeros((T, K, K), dtype=torch.float32, device="cuda"), torch.zeros((T, K), dtype=torch.float32, device="cuda"),
                         torch.ones((K, T), dtype=torch.float32, device="cuda"), G)
    K, T = 2, 8
    Gd, rd = torch.zeros((T, K, K), dtype=torch.float32, device="cuda"), torch.zeros((T, K), dtype=torch.float32, device="cuda")
    C = torch.ones((K, T), dtype=torch.float32, device="cuda")
    for kw in (dict(g=1.0), dict(g=-0.1), dict(g=[0.5, 1.0]), dict(g=G, penalty=-1.0), dict(g=G, baseline=float("nan")), dict(g=G, sweeps=-1)):
        with pytest.raises(ValueError, match="ar1_temporal: "):
            ops.ar1_temporal(Gd, rd, C, **kw)
    with pytest.raises(ValueError, match="do not match"):
        ops.ar1_temporal(Gd[:4], rd, C, G)
    assert bool((C == 1).all())
