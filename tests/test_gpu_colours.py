"""K29 on the GPU against tests/colours_restatement.py: the normal equations of the colours (K29a) on synthetic symmetric Gram
matrices -- entry by entry, the same bits on two runs and however the frames are cut into pieces -- and the non-negative solve
(K29b) on both sides of the K at which it stops holding M in LDS (K <= 128 in LDS; 65 and 200 are the two sides)."""
import numpy as np
import pytest
import torch

import colours_restatement as R

pytestmark = pytest.mark.gpu

KS, BS, NCS = (1, 6, 65, 200), (1, 7, 40, 257), (1, 3)      # B: one partly filled segment of 32, one full + a part, 8 + a part


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    assert ops.COLOUR_LDS_MAX_K == 128 and min(KS) <= 128 < max(KS)
    return ops


_CASES = {}


def case(K, B, NC):
    """fp32 inputs and the restatement's float64 sums of them, made once per shape."""
    if (K, B, NC) not in _CASES:
        rng = np.random.default_rng([K, B, NC])
        At = rng.random((B, 24, K)) * (rng.random((B, 24, K)) < 0.4)
        G = np.einsum("tpk,tpl->tkl", At, At).astype(np.float32)
        assert (G == G.transpose(0, 2, 1)).all()
        r = (rng.standard_normal((NC, B, K)) + 0.5).astype(np.float32)
        C = (rng.random((K, B)) * (rng.random((K, B)) < 0.8)).astype(np.float32)
        _CASES[K, B, NC] = (G, r, C) + R.normal_eqs(G, r, C)
    return _CASES[K, B, NC]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("NC", NCS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("K", KS)
def test_normal_eqs_against_float64(ops, K, B, NC):
    """Every entry within 1e-12 of the sum of its terms' magnitudes; the same bits on a second run; the same bits when the frames
    come in two uneven pieces, the smaller first (into a state sized for the whole) and the larger first."""
    from dnmf_amd import _lib
    G, r, C, M, b, Mabs, babs = case(K, B, NC)
    Gd, rd, Cd = dev(G), dev(r), dev(C)
    M1, b1, _ = ops.colour_normal_eqs(Gd, rd, Cd)
    assert M1.dtype == torch.float64 and tuple(M1.shape) == (K, K) and tuple(b1.shape) == (NC, K)
    eM, eb = np.abs(M1.cpu().numpy() - M), np.abs(b1.cpu().numpy() - b)
    print(f"\nK={K} B={B} NC={NC}: largest |M - M64| / sum|terms| {np.max(eM / np.maximum(Mabs, 1e-300)):.2e}, b "
          f"{np.max(eb / np.maximum(babs, 1e-300)):.2e}")
    assert (eM <= 1e-12 * Mabs).all() and (eb <= 1e-12 * babs).all()
    assert torch.equal(M1, M1.T)
    M2, b2, _ = ops.colour_normal_eqs(Gd, rd, Cd)
    assert torch.equal(M1, M2) and torch.equal(b1, b2)
    if B < 2:
        return
    whole = torch.empty(_lib.load().dnmf_colour_normal_eqs_workspace(K, NC, B) // 4, dtype=torch.float32, device="cuda")
    for cut, state in ((B // 3, whole), (B - B // 3, None)):
        parts = ((0, cut, True, False), (cut, B, False, True))
        for s, e, first, finish in parts:
            # C goes as a strided view of the whole (K, B), r as the frames' contiguous copy
            Mp, bp, state = ops.colour_normal_eqs(Gd[s:e], rd[:, s:e].contiguous(), Cd[:, s:e], state=state, first=first,
                                                  finish=finish)
            assert (Mp is None) == (not finish) and (bp is None) == (not finish)
        assert torch.equal(Mp, M1) and torch.equal(bp, b1), (K, B, NC, cut)
    out = (torch.full((K, K), -1.0, dtype=torch.float64, device="cuda"), torch.full((NC, K), -1.0, dtype=torch.float64, device="cuda"))
    Mo, bo, _ = ops.colour_normal_eqs(Gd, rd, Cd, out=out)
    assert Mo is out[0] and bo is out[1] and torch.equal(Mo, M1) and torch.equal(bo, b1)


def test_three_pieces_and_a_missing_state(ops):
    K, B, NC = 6, 257, 3
    G, r, C, M, b, _, _ = case(K, B, NC)
    Gd, rd, Cd = dev(G), dev(r), dev(C)
    M1, b1, _ = ops.colour_normal_eqs(Gd, rd, Cd)
    state = None
    for s, e in ((0, 131), (131, 150), (150, 257)):          # cuts inside a segment, and a piece that closes none
        Mp, bp, state = ops.colour_normal_eqs(Gd[s:e], rd[:, s:e].contiguous(), Cd[:, s:e], state=state, first=s == 0, finish=e == B)
    assert torch.equal(Mp, M1) and torch.equal(bp, b1)
    with pytest.raises(ValueError, match="first=False needs the state"):
        ops.colour_normal_eqs(Gd, rd, Cd, first=False)
    with pytest.raises(ValueError, match="first=False needs the state"):      # a later call larger than the first
        ops.colour_normal_eqs(Gd, rd, Cd, state=state, first=False)


# measured on the MI355X over every (K, NC) below, sweeps 1 and 10: the largest deviation of the colours and of kkt from the
# restatement's sweep -- see test_solve_against_the_restatement
SOLVE_COLOUR_DEV, SOLVE_KKT_DEV = 0.0, 0.0


@pytest.mark.parametrize("NC", NCS)
@pytest.mark.parametrize("K", KS)
def test_solve_against_the_restatement(ops, K, NC):
    """K29b on the restatement's own M and b (B = 40).  ``ok`` and the set of zero colours are equal; the colours (the
    restatement's rounded to fp32 as the kernel rounds its own) and kkt are compared with the restatement's sweep.  The kernel
    performs the restatement's IEEE float64 operations in the restatement's order (no contraction into fused multiply-adds, a
    correctly rounded division), so the deviation to expect is none.  Measured on the MI355X, every K in (1, 6, 65, 200), NC in
    (1, 3), sweeps 1 and 10: colours 0.0, kkt 0.0 -- ten times that is asserted: equal bits."""
    _, _, _, M, b, _, _ = case(K, 40, NC)
    rng = np.random.default_rng([K, NC, 7])
    col = (0.2 + rng.random((NC, K))).astype(np.float32)
    Md, bd, cd = dev(M), dev(b), dev(col)
    for sweeps in (1, 10):
        want, kkt, okc = R.solve(M, b, col, sweeps)
        got = ops.colour_solve(Md, bd, cd, sweeps=sweeps)
        assert got["colours"].dtype == torch.float32 and got["colours"].data_ptr() != cd.data_ptr()
        assert torch.equal(cd, dev(col))                                  # the input is left as it is
        x = got["colours"].cpu().numpy()
        assert got["ok"].cpu().numpy().astype(bool).tolist() == okc.tolist() == [True] * NC
        assert ((x == 0) == (want == 0)).all()
        dc = np.abs(x.astype(np.float64) - want.astype(np.float32).astype(np.float64)).max()
        dk = np.abs(got["kkt"].cpu().numpy() - kkt).max()
        print(f"\nK={K} NC={NC} sweeps={sweeps}: colours deviate by {dc:.3e}, kkt by {dk:.3e} (kkt {kkt.max():.3e}, zeros "
              f"{int((want == 0).sum())})")
        assert dc <= 10 * SOLVE_COLOUR_DEV and dk <= 10 * SOLVE_KKT_DEV
        # the kkt of any colours: that of the solver's result after its rounding, and of the start
        k_start = ops.colour_kkt(Md, bd, cd).cpu().numpy()
        np.testing.assert_allclose(k_start, R.solve(M, b, col, 0)[1], rtol=0, atol=10 * SOLVE_KKT_DEV)
        again = ops.colour_solve(Md, bd, cd, sweeps=sweeps)
        assert torch.equal(again["colours"], got["colours"]) and torch.equal(again["kkt"], got["kkt"])


@pytest.mark.parametrize("K", [6, 200])
def test_solve_edge_rules(ops, K):
    NC = 3
    _, _, _, M, b, _, _ = case(K, 40, NC)
    col = (0.2 + np.random.default_rng(K).random((NC, K))).astype(np.float32)
    # a NaN in b[1]: that channel keeps its row
    bn = b.copy()
    bn[1, K // 2] = np.nan
    got = ops.colour_solve(dev(M), dev(bn), dev(col), sweeps=3)
    want, kkt, okc = R.solve(M, bn, col, 3)
    assert got["ok"].cpu().tolist() == [1, 0, 1] and okc.tolist() == [True, False, True]
    x = got["colours"].cpu().numpy()
    assert (x[1] == col[1]).all() and (x == want.astype(np.float32)).all()
    k = got["kkt"].cpu().numpy()
    assert np.isnan(k[1]) and (k[[0, 2]] == kkt[[0, 2]]).all()
    assert np.isnan(ops.colour_kkt(dev(M), dev(bn), dev(col)).cpu().numpy()).tolist() == [False, True, False]
    # an infinite entry of M: every channel
    Mn = M.copy()
    Mn[K - 1, 0] = np.inf
    got = ops.colour_solve(dev(Mn), dev(b), dev(col), sweeps=3)
    assert got["ok"].cpu().tolist() == [0, 0, 0] and (got["colours"].cpu().numpy() == col).all()
    # a neuron without a trace (zero row, column and b): left alone; a non-positive diagonal likewise
    Mz, bz = M.copy(), b.copy()
    Mz[1, :] = 0.0
    Mz[:, 1] = 0.0
    bz[:, 1] = 0.0
    Mz[K - 2, K - 2] = -1.0
    got = ops.colour_solve(dev(Mz), dev(bz), dev(col), sweeps=4)
    want, kkt, _ = R.solve(Mz, bz, col, 4)
    x = got["colours"].cpu().numpy()
    assert (x[:, 1] == col[:, 1]).all() and (x[:, K - 2] == col[:, K - 2]).all()
    assert (x == want.astype(np.float32)).all() and (got["kkt"].cpu().numpy() == kkt).all()


def test_bad_arguments_are_refused(ops):
    f32, f64 = dict(dtype=torch.float32, device="cuda"), dict(dtype=torch.float64, device="cuda")
    G, r, C = torch.zeros((5, 4, 4), **f32), torch.zeros((3, 5, 4), **f32), torch.zeros((4, 5), **f32)
    ops.colour_normal_eqs(G, r, C)
    with pytest.raises(ValueError, match="NC=17"):
        ops.colour_normal_eqs(G, torch.zeros((17, 5, 4), **f32), C)
    with pytest.raises(ValueError, match="K=4097"):
        ops.colour_normal_eqs(torch.zeros((1, 4097, 4097), **f32), torch.zeros((1, 1, 4097), **f32), torch.zeros((4097, 1), **f32))
    for bad in (dict(G=G.double()), dict(G=G[:, :, :3]), dict(G=G[0]), dict(r=r[:, :4]), dict(r=r[..., :3]), dict(C=C[:3]),
                dict(C=C[:, :4]), dict(C=C.double()), dict(C=C.t().contiguous().t()), dict(G=G.cpu())):
        with pytest.raises(ValueError):
            ops.colour_normal_eqs(**{**dict(G=G, r=r, C=C), **bad})
    with pytest.raises(ValueError, match="out M"):
        ops.colour_normal_eqs(G, r, C, out=(torch.zeros((4, 4), **f32), torch.zeros((3, 4), **f64)))
    M, b, col = torch.eye(4, **f64), torch.zeros((3, 4), **f64), torch.ones((3, 4), **f32)
    ops.colour_solve(M, b, col)
    with pytest.raises(ValueError, match="NC=17"):
        ops.colour_solve(M, torch.zeros((17, 4), **f64), torch.ones((17, 4), **f32))
    with pytest.raises(ValueError, match="K=4097"):
        ops.colour_solve(M, b, torch.ones((1, 4097), **f32))
    for bad in (dict(M=M.float()), dict(M=M[:3]), dict(b=b[:2]), dict(b=b.float()), dict(colours=col.double()), dict(colours=col[0]),
                dict(sweeps=0), dict(sweeps=1.5), dict(M=M.cpu())):
        with pytest.raises(ValueError):
            ops.colour_solve(**{**dict(M=M, b=b, colours=col), **bad})
    with pytest.raises(ValueError):
        ops.colour_kkt(M, b[:2], col)
