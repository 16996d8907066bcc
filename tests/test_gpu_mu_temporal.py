"""K4 (multiplicative trace update, csrc/mu_temporal.hip) in its four forms -- dnmf_mu_temporal, _nbr, _slots, _step -- on
the GPU against the float64 definition oracle.dnmf_oracle.mu_temporal_from_gram on the very same G, r, C0.

Tolerances (derived, not taken from the kernels):
  fp32 state (dense, nbr, slots)  the kernels do float64 arithmetic and round once at the end: every finite entry within
           ONE fp32 ulp (np.spacing of the float32 value) of the oracle's float64 value -- half an ulp for the rounding, the
           rest for a value that sits on a rounding boundary.  The non-finite sets must be equal.
  fp64 state (step)  |d| <= 1e-12 |want| entrywise.  On the problem family used here (r > 0, so the update stays positive
           and does not amplify rounding) float64 against long double and against the reversed summation order differ by
           at most 5.2e-15 entrywise on the CPU, K up to 256, up to 50 rounds, with and without gamma: 1e-12 is about 200
           times that order sensitivity.  (On the very instances problem() makes here the same measurement gives 7.0e-15
           up to 7 rounds and 1.8e-14 at 50 rounds, K = 256, T = 70: the bound keeps a factor above 50.)

That each test can fail (CPU, on the oracle alone; the numbers are from this file's problem(33, 3) and (5, 3)):
  * one G entry across a variant boundary, G[t, 32, k] at K = 33 (read by the <64> instantiation only), moved by one fp32
    ulp: the worst (t, k) moves the 7-round result by 1.12 fp32 ulps of the result (more than the allowance of 1); row
    32 dropped altogether -- what a lane split that misreads does -- moves it by 7.4e7 ulps.
  * the step form without the gamma neighbour term at t = 0 (gamma = 0.7, 3 rounds, K = 5, T = 3) moves the result by 0.75
    relative (neuron 1, which lives on that term alone, left out), against the allowance of 1e-12.

Measured on the MI355X (kept apart from the limits above, which they did not set; every test prints its own): worst
fp32 deviation 0.500 ulp in the dense form and 0.496 ulp in the nbr and slot forms, the one rounding; worst fp64 deviation
of the step form 3.5e-15 relative = 3.5e-3 of the allowance (K = 256, T = 1, gamma = 0.7).

The overflow finding (test_overflowing_trace).  The comment above mu_temporal_nbr_kernel used to call the list forms
"bit-identical" to the dense form because a term with G = 0 "adds an exact zero".  That holds while every trace of the frame
is finite.  When G[k0, k0] = 0 and r[k0] > 0, c[k0] grows by 1/1e-32 per round and is inf in float64 after round 10; from
round 11 on the dense form (and the reference's numpy) computes 0 * inf = NaN for EVERY neuron of the frame, the list forms
only for the rows whose list names k0.  On the NN = 16 chain (K = 20, T = 6, k0 = 10): after 11 rounds 120 of 120 entries
are non-finite in the dense form and 96 of 120 in the nbr form (rows 0..15).  The containment does not last: a NaN row
spreads to every row that lists it, through real couplings and through the padding columns (0 * NaN) alike, so on this
connected chain the nbr form is at 120 of 120 from round 12 on, and after the 14 rounds the two sets are equal.
"""
import numpy as np
import pytest
import torch

from test_gpu_hals import chain, host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


@pytest.fixture(scope="module")
def O():
    from oracle import dnmf_oracle
    return dnmf_oracle


DEVICE = "cuda"


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEVICE, dtype)


def want64(O, G, r, C0, gamma, iters):
    """The float64 definition on G (T,K,K), r (T,K) as the kernels take them."""
    return O.mu_temporal_from_gram(np.moveaxis(np.asarray(G, np.float64), 0, 2), np.asarray(r, np.float64).T, C0, gamma, iters)


def mu_listed(G, r, C, iters, nbr=None):
    """mu_temporal_from_gram's formula without gamma, G (T,K,K), r (T,K); with ``nbr`` (K,NN) the sum G_t c of row k runs
    over the columns nbr[k] only (all of them, padding included: 0 * inf is NaN there as anywhere)."""
    G, r = np.asarray(G, np.float64), np.asarray(r, np.float64)
    C = np.asarray(C, np.float64).copy()
    K = C.shape[0]
    rows = np.arange(K)[:, None]
    with np.errstate(all="ignore"):
        for _ in range(iters):
            if nbr is None:
                C2 = np.einsum("tkl,lt->kt", G, C)
            else:
                C2 = np.einsum("tkj,kjt->kt", G[:, nbr, rows], C[nbr])   # column k for row k, as the kernels read
            C = C * r.T / (C2 + 1e-32)
    return C


def ulp_ratio(got, want):
    """got fp32 numpy, want float64: the non-finite sets are equal, and the worst |got - want| over the finite entries as a
    fraction of one fp32 ulp of got (the allowance is 1)."""
    assert got.dtype == np.float32 and want.dtype == np.float64
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), "non-finite sets differ: %d against %d" % ((~np.isfinite(got)).sum(),
                                                                                           (~fin).sum())
    if not fin.any():
        return 0.0
    d = np.abs(got[fin].astype(np.float64) - want[fin])
    return float((d / np.spacing(np.abs(got[fin])).astype(np.float64)).max())


def rel_ratio(got, want):
    """got, want float64: the worst |got - want| as a fraction of the allowance 1e-12 |want| (0 where both are 0)."""
    d, lim = np.abs(got - want), 1e-12 * np.abs(want)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    if ((d > 0) & (lim == 0)).any():
        return np.inf
    return float((d[lim > 0] / lim[lim > 0]).max()) if (lim > 0).any() else 0.0


_problems = {}


def problem(K, T):
    """(G (T,K,K), r (T,K), C0 (K,T)) fp32 numpy, made once per shape.  G as in test_gpu_hals.problem: G_t = a_t G0 +
    diag(b_t), G0 = M^T M of a sparse non-negative M -- symmetric, non-negative, different in every frame.  r = (G c*) (1 +
    0.1 u) with c* > 0 and u in [0, 1): r > 0 everywhere, no additive noise.  From K = 5 on neuron 1 has an all-zero row
    and column and r = 0 (it must be exactly 0 after one round) and neuron 2 starts at C0 = 0 (it must stay 0)."""
    if (K, T) not in _problems:
        rng = np.random.RandomState(2000 * K + T)
        Mx = rng.rand(2 * K + 20, K) * (rng.rand(2 * K + 20, K) < 0.3)
        G0 = Mx.T @ Mx
        G0 = (G0 + G0.T) / 2
        G = rng.uniform(0.5, 1.5, (T, 1, 1)) * G0[None] + np.eye(K)[None] * rng.uniform(0.2, 1.0, (T, K))[:, :, None]
        if K >= 5:
            G[:, 1, :] = 0
            G[:, :, 1] = 0
        cs = 0.05 + rng.rand(K, T)
        r = np.einsum("tkl,lt->tk", G, cs) * (1 + 0.1 * rng.rand(T, K))
        C0 = 0.05 + rng.rand(K, T)
        if K >= 5:
            assert (r[:, 1] == 0).all()
            C0[2] = 0
        G32, r32 = G.astype(np.float32), r.astype(np.float32)
        assert np.array_equal(G32, G32.transpose(0, 2, 1)) and (G32 >= 0).all()
        assert (np.delete(r32, 1, 1) > 0).all() if K >= 5 else (r32 > 0).all()
        assert T == 1 or not np.array_equal(G32[0], G32[1])
        _problems[(K, T)] = (G32, r32, C0.astype(np.float32))
    return _problems[(K, T)]


def in_view(C0, pad_left, pad_right, dtype=torch.float32):
    """A buffer filled with -7 and the view of it that holds C0: ldc = T + pad_left + pad_right > T."""
    K, T = C0.shape
    buf = torch.full((K, T + pad_left + pad_right), -7.0, device=DEVICE, dtype=dtype)
    C = buf[:, pad_left:pad_left + T]
    C.copy_(dev(C0, dtype))
    return buf, C


def untouched_outside(buf, pad_left, T):
    return bool((buf[:, :pad_left] == -7).all()) and bool((buf[:, pad_left + T:] == -7).all())


# ---- the dense form: <32>, <64>, <128>, <0> ------------------------------------------------------------------------

def dense_case(ops, O, K, T, rounds):
    G, r, C0 = problem(K, T)
    Gd, rd = dev(G), dev(r)
    worst = 0.0
    for iters in rounds:
        buf, C = in_view(C0, 2, 3)
        out = ops.mu_temporal(Gd, rd, C, iters)
        assert out is C
        assert untouched_outside(buf, 2, T), (K, T, iters)
        got = C.contiguous().cpu().numpy()
        if iters == 0:
            assert np.array_equal(got.view(np.uint32), C0.view(np.uint32))
            continue
        ratio = ulp_ratio(got, want64(O, G, r, C0, None, iters))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (K, T, iters, ratio)
        if K >= 5:
            assert (got[1] == 0).all() and (got[2] == 0).all()
        assert (np.delete(got, [1, 2], 0) > 0).all() if K >= 5 else (got > 0).all()
        if iters >= 7:   # a contiguous C: the same bits as the view
            assert torch.equal(ops.mu_temporal(Gd, rd, dev(C0), iters), C)
    print("K=%d T=%d rounds %s: worst deviation %.3f of one fp32 ulp" % (K, T, rounds, worst))


@pytest.mark.parametrize("T", [1, 3, 70])
@pytest.mark.parametrize("K", [1, 5, 32, 33, 64, 65, 128, 129, 255, 256])
def test_dense_form(ops, O, K, T):
    """Both sides of every variant boundary (<32> | <64> | <128> | <0>; blocks of 64, 64, 128, 256 threads with padded lanes
    and KREG > K) and the limits K = 1 and K = 256; one frame, a few, many; iters 0, 1 and 7; C a view with ldc > T whose
    other columns stay as they are."""
    dense_case(ops, O, K, T, (0, 1, 7))


def test_dense_form_fifty_rounds(ops, O):
    """The round count bench.py runs."""
    dense_case(ops, O, 129, 3, (50,))


# ---- the step form: one round on a float64 state with gamma ---------------------------------------------------------

def step_rounds(ops, Gd, rd, a, b, gamma, rounds, edges=None):
    """``rounds`` launches a -> b -> a ...; returns the tensor that holds the result.  edges(Cin) -> (c_left, c_right)."""
    for _ in range(rounds):
        left, right = edges(a) if edges is not None else (None, None)
        out = ops.mu_temporal_step(Gd, rd, a, b, gamma, left, right)
        assert out is b
        a, b = b, a
    return a


@pytest.mark.parametrize("gamma", [0.0, 1e-2, 0.7])
@pytest.mark.parametrize("T", [1, 2, 3, 6])
@pytest.mark.parametrize("K", [1, 5, 65, 129, 256])
def test_step_form(ops, O, K, T, gamma):
    """Blocks of 64, 128 and 256 threads; T = 1 is both replicated edges in one frame, T = 2 two edge frames, from T = 3 on
    inner frames; Cin and Cout two views with the same ldc > T."""
    G, r, C0 = problem(K, T)
    Gd, rd = dev(G), dev(r)
    bufa, a = in_view(C0, 1, 2, torch.float64)
    bufb, b = in_view(np.full_like(C0, -3.0), 1, 2, torch.float64)
    assert a.stride(0) == b.stride(0) == T + 3
    res = step_rounds(ops, Gd, rd, a, b, gamma, 3)
    assert res is b
    assert untouched_outside(bufa, 1, T) and untouched_outside(bufb, 1, T)
    got = host(res)
    ratio = rel_ratio(got, want64(O, G, r, C0, gamma, 3))
    if gamma == 0:
        ratio = max(ratio, rel_ratio(got, want64(O, G, r, C0, None, 3)))
    print("K=%d T=%d gamma=%g: worst deviation %.3e of the allowance 1e-12 |want|" % (K, T, gamma, ratio))
    assert ratio <= 1.0, (K, T, gamma, ratio)
    if K >= 5:
        assert (got[2] == 0).all()
        assert (got[1] == 0).all() == (gamma == 0)    # without a footprint: the neighbour term alone keeps it alive
    if gamma == 0.7 and T > 1:   # the term is felt, the edges included
        assert rel_ratio(want64(O, G, r, C0, None, 3)[:, [0, -1]], want64(O, G, r, C0, gamma, 3)[:, [0, -1]]) > 1e6


@pytest.mark.parametrize("K", [5, 129])
def test_step_form_shard_edges(ops, O, K):
    """[0, 7) as [0, 3) and [3, 7): with the neighbours' columns handed over as c_right / c_left the shards equal the
    one-launch round on the whole axis bit for bit (every entry sees the same operands in the same order); with None the
    shard's own edge is replicated, the reference's behaviour at t = 0 and t = T - 1."""
    T, cut, gamma = 7, 3, 0.7
    G, r, C0 = problem(K, T)
    Gd, rd = dev(G), dev(r)
    parts = ((slice(0, cut), Gd[:cut].contiguous(), rd[:cut].contiguous()), (slice(cut, T), Gd[cut:].contiguous(), rd[cut:].contiguous()))

    def whole_round(cin):
        return ops.mu_temporal_step(Gd, rd, cin, torch.full_like(cin, -7.0), gamma)

    def shard_round(cin, exchange):
        out = torch.full_like(cin, -7.0)
        for i, (sl, Gs, rs) in enumerate(parts):   # views of the whole state: ldc = T, wider than either shard
            left = cin[:, cut - 1].contiguous() if (exchange and i == 1) else None
            right = cin[:, cut].contiguous() if (exchange and i == 0) else None
            ops.mu_temporal_step(Gs, rs, cin[:, sl], out[:, sl], gamma, left, right)
        return out

    w = s = dev(C0, torch.float64)
    for n in range(3):   # one round, then two more, the edges exchanged before each
        w, s = whole_round(w), shard_round(s, True)
        assert torch.equal(w, s), n
    ratio = rel_ratio(host(w), want64(O, G, r, C0, gamma, 3))
    print("K=%d whole axis, 3 rounds: %.3e of the allowance" % (K, ratio))
    assert ratio <= 1.0

    whole, alone = host(whole_round(dev(C0, torch.float64))), host(shard_round(dev(C0, torch.float64), False))
    live = np.array([k for k in range(K) if k != 2])      # (neuron 2 starts at 0 and is 0 either way)
    assert (alone[live][:, [cut - 1, cut]] != whole[live][:, [cut - 1, cut]]).all()
    inner = [t for t in range(T) if t not in (cut - 1, cut)]
    assert np.array_equal(alone[:, inner], whole[:, inner])
    for sl, _, _ in parts:
        ratio = rel_ratio(alone[:, sl], want64(O, G[sl], r[sl], C0[:, sl], gamma, 1))
        print("K=%d shard %s alone: %.3e of the allowance" % (K, sl, ratio))
        assert ratio <= 1.0


def test_step_refuses_mismatched_strides(ops):
    K, T = 5, 3
    G, r, C0 = problem(K, T)
    _, a = in_view(C0, 1, 2, torch.float64)
    buf = torch.full((K, T), -7.0, device=DEVICE, dtype=torch.float64)
    assert a.stride(0) == 6 and buf.stride(0) == 3
    for cin, cout in ((a, buf), (buf, a)):
        before = cout.clone()
        with pytest.raises(ValueError, match=r"mu_temporal_step: .*stride\(0\)=%d .*stride\(0\)=%d" % (cin.stride(0), cout.stride(0))):
            ops.mu_temporal_step(dev(G), dev(r), cin, cout, 0.1)
        assert torch.equal(cout, before)


# ---- compact footprints: the nbr and slot forms on K3n's data -------------------------------------------------------

@pytest.mark.parametrize("NN", [8, 16, 32])   # 20x16x2 K=9, 48x16x2 K=20 and 52x12x1 K=40 (Z = 1)
def test_nbr_and_slot_forms(ops, O, NN):
    c = chain(ops, NN)
    ly, sz, K, C0 = c["ly"], c["sz"], c["K"], c["C0"]
    G, r, nbr = c["G"], c["r"], ly["nbr"]
    Gh, rh = G.cpu().numpy(), r.cpu().numpy()
    assert np.array_equal(Gh, Gh.transpose(0, 2, 1))
    _, _, ws = ops.warp_gram_rhs_lists(ly, K, sz, c["beta"], None, c["frames"], finish=False)
    for iters in (1, 9):
        want = want64(O, Gh, rh, C0, None, iters)
        dense = ops.mu_temporal(G, r, dev(C0), iters)
        for name, got in (("nbr", ops.mu_temporal(G, r, dev(C0), iters, nbr=nbr)),
                          ("slots", ops.mu_temporal_slots(ly, ws, sz, dev(C0), iters))):
            ratio = ulp_ratio(got.cpu().numpy(), want)
            print("NN=%d %s, %d rounds: worst deviation %.3f of one fp32 ulp" % (NN, name, iters, ratio))
            assert ratio <= 1.0, (NN, name, iters, ratio)
            assert torch.equal(got, dense), (NN, name, iters)   # holds while everything is finite
    buf, C = in_view(C0, 2, 3)   # the list forms on a view, and iters = 0
    assert ops.mu_temporal(G, r, C, 9, nbr=nbr) is C and torch.equal(C, dense) and untouched_outside(buf, 2, c["T"])
    buf, C = in_view(C0, 2, 3)
    assert ops.mu_temporal_slots(ly, ws, sz, C, 9) is C and torch.equal(C, dense) and untouched_outside(buf, 2, c["T"])
    assert torch.equal(ops.mu_temporal(G, r, dev(C0), 0, nbr=nbr), dev(C0))
    assert torch.equal(ops.mu_temporal_slots(ly, ws, sz, dev(C0), 0), dev(C0))


def test_overflowing_trace(ops, O):
    """A neuron k0 whose warped footprint underflowed (G[k0, :] = G[:, k0] = 0 in fp32) while r[k0] > 0: see the module
    docstring.  Dense kernel = dense definition, nbr kernel = the definition restricted to the listed columns, in their
    non-finite sets and, where finite, to one fp32 ulp."""
    c = chain(ops, 16)
    K, T, C0, nbr = c["K"], c["T"], c["C0"], c["ly"]["nbr"]
    k0 = K // 2
    G, r = c["G"].clone(), c["r"].clone()
    G[:, k0, :] = 0
    G[:, :, k0] = 0
    r[:, k0] = 1
    Gh, rh, nh = G.cpu().numpy(), r.cpu().numpy(), nbr.cpu().numpy().astype(np.int64)
    assert ((nh >= 0) & (nh < K)).all()
    lists_k0 = (nh == k0).any(1)
    assert lists_k0[k0] and 0 < lists_k0.sum() < K

    def run(iters):
        with np.errstate(all="ignore"):
            want_d = want64(O, Gh, rh, C0, None, iters)
        same = mu_listed(Gh, rh, C0, iters)     # the helper without a table is the definition
        assert np.array_equal(np.isnan(same), np.isnan(want_d)) and np.array_equal(np.isinf(same), np.isinf(want_d))
        assert rel_ratio(same[np.isfinite(same)], want_d[np.isfinite(same)]) <= 1.0
        want_n = mu_listed(Gh, rh, C0, iters, nh)
        got_d = ops.mu_temporal(G, r, dev(C0), iters).cpu().numpy()
        got_n = ops.mu_temporal(G, r, dev(C0), iters, nbr=nbr).cpu().numpy()
        ratios = ulp_ratio(got_d, want_d), ulp_ratio(got_n, want_n)     # asserts the non-finite sets equal
        print("%d rounds: non-finite %d (dense) and %d (nbr) of %d; finite entries %.3f / %.3f of one fp32 ulp"
              % (iters, (~np.isfinite(want_d)).sum(), (~np.isfinite(want_n)).sum(), K * T, *ratios))
        assert max(ratios) <= 1.0
        return want_d, want_n, got_d, got_n

    # one round: c[k0] ~ 1e32 is finite, in fp32 too, and all forms agree bit for bit
    want_d, want_n, got_d, got_n = run(1)
    assert np.isfinite(want_d).all() and (want_d[k0] > 1e30).all()
    assert np.array_equal(got_d.view(np.uint32), got_n.view(np.uint32))
    # ten rounds: c[k0] is inf, nothing else has seen it yet
    want_d, want_n, _, _ = run(10)
    assert np.isinf(want_d[k0]).all() and np.isfinite(np.delete(want_d, k0, 0)).all()
    # eleven: the dense form loses the whole frame to 0 * inf, the nbr form the rows that list k0
    want_d, want_n, _, got_n = run(11)
    assert np.isnan(want_d).all()
    assert np.array_equal(np.isfinite(want_n), np.broadcast_to(~lists_k0[:, None], (K, T)))
    assert (~np.isfinite(got_n)).sum() < (~np.isfinite(want_d)).sum()   # strictly smaller: 96 of 120 against 120
    # fourteen: every entry of every frame is NaN in the dense definition; by now the NaN rows have reached, through
    # the lists that name them, the rest of this (connected) chain as well
    want_d, want_n, _, _ = run(14)
    assert np.isnan(want_d).all()
    assert (~np.isfinite(want_n)).sum() <= (~np.isfinite(want_d)).sum()


# ---- refusals -------------------------------------------------------------------------------------------------------

def test_unsupported_sizes_name_the_call(ops):
    from dnmf_amd._lib import DnmfHipError
    T = 2

    def args(K, NN):
        G, r = torch.zeros(T, K, K, device=DEVICE), torch.zeros(T, K, device=DEVICE)
        nbr = torch.zeros(K, NN, dtype=torch.int32, device=DEVICE)
        ly = {"nslot": K + 2, "pair_slot": torch.zeros(K, K, dtype=torch.int32, device=DEVICE), "nbr": nbr}
        ws = torch.zeros(T * 64 * (K + 2), device=DEVICE)
        return G, r, nbr, ly, ws

    K = 257
    G, r, nbr, ly, ws = args(K, 8)
    C = torch.full((K, T), 0.5, device=DEVICE)
    with pytest.raises(DnmfHipError, match=r"argument error -3\): dnmf_mu_temporal: K=257"):
        ops.mu_temporal(G, r, C, 1)
    with pytest.raises(DnmfHipError, match=r"argument error -3\): dnmf_mu_temporal_nbr: K=257"):
        ops.mu_temporal(G, r, C, 1, nbr=nbr)
    with pytest.raises(DnmfHipError, match=r"argument error -3\): dnmf_mu_temporal_slots: K=257"):
        ops.mu_temporal_slots(ly, ws, [8, 8, 1], C, 1)
    with pytest.raises(DnmfHipError, match=r"argument error -3\): dnmf_mu_temporal_step: K=257"):
        ops.mu_temporal_step(G, r, C.double(), C.double(), 0.1)
    K = 20
    G, r, nbr, ly, ws = args(K, 12)
    C2 = torch.full((K, T), 0.5, device=DEVICE)
    with pytest.raises(DnmfHipError, match=r"argument error -3\): dnmf_mu_temporal_nbr: K=20 \(<= 256\), NN=12"):
        ops.mu_temporal(G, r, C2, 1, nbr=nbr)
    with pytest.raises(DnmfHipError, match=r"argument error -3\): dnmf_mu_temporal_slots: K=20 \(<= 256\), NN=12"):
        ops.mu_temporal_slots(ly, ws, [8, 8, 1], C2, 1)
    assert bool((C == 0.5).all()) and bool((C2 == 0.5).all())
