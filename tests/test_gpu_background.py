"""The rank-1 background kernels (K19: ``dnmf_background_dots / _accum / _subtract``) and ``ops.background_fit`` on the GPU against
the float64 definition (tests/background_restatement.py), each on identical inputs.

Tolerances.  The partial sums ``num``, ``bb``, ``ff`` are float64 sums of N <= 10^4 float64 terms; in any order two such sums
differ by at most N x 1.1e-16 of the sum of the terms' magnitudes, so 1e-12 of that sum leaves a tenfold margin.  ``f`` and ``b``
are one float64 division rounded to fp32: within one fp32 ulp of the restatement's value plus the bound of the numerator divided
by the denominator.  ``subtract`` is one correctly rounded fp32 operation: within one fp32 ulp of the float64 value."""
import functools

import numpy as np
import pytest
import torch

import background_restatement as BR

pytestmark = pytest.mark.gpu

TILE = 1024    # voxels of a workgroup of accum and subtract (include/dnmf_hip.h); dots cuts segments at multiples of it
# (9, 7, 3): P = 189 is odd, every row but the first starts off a 16-byte boundary; (64, 48, 1): three tiles and three
# segments; (41, 25, 1): P = TILE + 1, a last tile of one voxel
SHAPES = [(20, 17, 1), (9, 7, 3), (33, 5, 2), (1, 40, 1), (64, 48, 1), (41, 25, 1)]
FRAMES = [1, 2, 37]
SUM_TOL = 1e-12


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def padded(x, pad):
    """(T, P) values as CUDA rows of P + pad floats (a view of a larger buffer filled with NaN: reading beyond a row shows)."""
    T, P = x.shape
    buf = torch.full((T, P + pad), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :P] = dev(x)
    return buf[:, :P]


@functools.lru_cache(maxsize=None)
def inputs(sz, T=37):
    """Seeded inputs of a shape, computed once, never changed: frames Y and model M (T, P), b (P,), f (T,).  Y - M takes both
    signs, so the clamps of both steps are met."""
    assert sz[0] * sz[1] * sz[2] != 0
    P = sz[0] * sz[1] * sz[2]
    rng = np.random.RandomState(P)
    Y = rng.uniform(0.0, 2.0, (T, P)).astype(np.float32)
    M = rng.uniform(0.0, 1.5, (T, P)).astype(np.float32)
    b = rng.uniform(0.2, 1.0, P).astype(np.float32)
    f = rng.uniform(0.5, 1.5, T).astype(np.float32)
    for a in (Y, M, b, f):
        a.setflags(write=False)
    return Y, M, b, f


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def check_sums(got, want, terms, what):
    got, want, terms = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (got, want, terms))
    worst = (np.abs(got - want) / terms).max()
    print(f"{what}: worst |sum - restatement| / sum|terms| = {worst:.2e}")
    assert worst <= SUM_TOL, what


def check_step(got, num, den, terms, what):
    """A new f or b (fp32) against the restatement's, within one ulp plus the numerator's bound over the denominator."""
    want = BR.step(num, den)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert (got >= 0).all(), what
    excess = np.abs(got.astype(np.float64) - want.astype(np.float64)) - (ulp(want) + SUM_TOL * terms / den)
    print(f"{what}: worst excess over the tolerance {excess.max():.2e} (<= 0 passes), {int((want == 0).sum())} of {want.size} clamped")
    assert excess.max() <= 0, what


def check_dots(ops, fr, b, sub, fid, Yh, Mh, what):
    f, num, bb = ops.background_dots(fr, dev(b), sub=sub, frame_ids=fid)
    torch.cuda.synchronize()
    assert f.dtype == torch.float32 and num.dtype == torch.float64 and bb.dtype == torch.float64 and bb.numel() == 1
    want, wbb = BR.dots(Yh, b, sub=Mh)
    terms = BR.dots_terms(Yh, b, sub=Mh)
    check_sums(num.cpu().numpy(), want, terms, what + " num")
    check_sums(bb.item(), wbb, wbb, what + " bb")
    check_step(f.cpu().numpy(), want, wbb, terms, what + " f")


def check_accum(got, f, Yh, Mh, sz, what):
    b, num, ff = got
    assert b.dtype == torch.float32 and num.dtype == torch.float64 and ff.dtype == torch.float64 and ff.numel() == 1
    assert tuple(b.shape) == tuple(sz) and tuple(num.shape) == tuple(sz)
    want, wff = BR.accum(Yh, f, sub=Mh)
    terms = BR.accum_terms(Yh, f, sub=Mh)
    check_sums(num.cpu().numpy().reshape(-1), want, terms, what + " num")
    check_sums(ff.item(), wff, wff, what + " ff")
    check_step(b.cpu().numpy().reshape(-1), want, wff, terms, what + " b")


# ---- dots -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_sub", [False, True])
@pytest.mark.parametrize("T", FRAMES)
@pytest.mark.parametrize("sz", SHAPES)
def test_dots_match_the_restatement(ops, sz, T, with_sub):
    Y, M, b, _ = inputs(sz)
    Y, M = Y[:T], (M[:T] if with_sub else None)
    check_dots(ops, dev(Y), b, None if M is None else dev(M), None, Y, M, f"dots {sz} T={T} sub={with_sub}")


@pytest.mark.parametrize("pads", [(3, 5), (4, 8), (1, 0)])
@pytest.mark.parametrize("with_sub", [False, True])
@pytest.mark.parametrize("sz", SHAPES)
def test_dots_with_padded_rows_and_permuted_frames(ops, sz, with_sub, pads):
    """ldf > P and lds > P (pads that keep and that break the 16-byte phase of the rows, alike and differently for the two), the
    frames taken in a permuted order; row j of sub belongs to the j-th frame of the call."""
    Y, M, b, _ = inputs(sz)
    perm = np.random.RandomState(7).permutation(len(Y))
    sub = padded(M, pads[1]) if with_sub else None
    check_dots(ops, padded(Y, pads[0]), b, sub, dev(perm, torch.int32), Y[perm], M if with_sub else None,
               f"dots {sz} pads={pads} permuted sub={with_sub}")


def test_dots_of_a_zero_image_are_zero(ops):
    Y, _, b, _ = inputs((9, 7, 3))
    f, num, bb = ops.background_dots(dev(Y), dev(np.zeros_like(b)))
    assert bb.item() == 0 and (num == 0).all() and (f == 0).all()


# ---- accum ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segment", [0, 5])
@pytest.mark.parametrize("with_sub", [False, True])
@pytest.mark.parametrize("T", FRAMES)
@pytest.mark.parametrize("sz", SHAPES)
def test_accum_matches_the_restatement(ops, sz, T, with_sub, segment):
    """segment = 5: eight segments at T = 37, the last of two frames; 0: the kernel's choice (three of 13, 13 and 11)."""
    Y, M, _, f = inputs(sz)
    Y, M, f = Y[:T], (M[:T] if with_sub else None), f[:T]
    got, state = ops.background_accum(dev(Y), dev(f), sz, sub=None if M is None else dev(M), segment=segment)
    torch.cuda.synchronize()
    check_accum(got, f, Y, M, sz, f"accum {sz} T={T} sub={with_sub} segment={segment}")


@pytest.mark.parametrize("pads", [(3, 5), (4, 8), (1, 0)])
@pytest.mark.parametrize("with_sub", [False, True])
@pytest.mark.parametrize("sz", SHAPES)
def test_accum_with_padded_rows_and_permuted_frames(ops, sz, with_sub, pads):
    Y, M, _, f = inputs(sz)
    perm = np.random.RandomState(8).permutation(len(Y))
    sub = padded(M, pads[1]) if with_sub else None
    got, _ = ops.background_accum(padded(Y, pads[0]), dev(f), sz, sub=sub, frame_ids=dev(perm, torch.int32), segment=5)
    torch.cuda.synchronize()
    check_accum(got, f, Y[perm], M if with_sub else None, sz, f"accum {sz} pads={pads} permuted sub={with_sub}")


@pytest.mark.parametrize("segment", [0, 5])
@pytest.mark.parametrize("with_sub", [False, True])
@pytest.mark.parametrize("sz", SHAPES)
def test_accum_in_three_pieces_through_the_state(ops, sz, with_sub, segment):
    """13 + 13 + 11 frames through one state give what one call gives, up to the order of the sums."""
    Y, M, _, f = inputs(sz)
    Yd, Md, fd = dev(Y), (dev(M) if with_sub else None), dev(f)
    state = ops.background_state(sz, 13, segment=segment)
    got = None
    for s, e in ((0, 13), (13, 26), (26, 37)):
        got, state = ops.background_accum(Yd[s:e], fd[s:e], sz, sub=None if Md is None else Md[s:e], state=state, first=s == 0,
                                          finish=e == 37, segment=segment)
        assert (got is None) == (e != 37)
    torch.cuda.synchronize()
    check_accum(got, f, Y, M if with_sub else None, sz, f"accum {sz} in three pieces sub={with_sub} segment={segment}")
    # a reused state starts afresh with first=True
    again, _ = ops.background_accum(Yd[:13], fd[:13], sz, sub=None if Md is None else Md[:13], state=state, segment=segment)
    check_accum(again, f[:13], Y[:13], M[:13] if with_sub else None, sz, f"accum {sz} on the reused state")


def test_accum_with_a_zero_trace_is_zero(ops):
    Y, _, _, f = inputs((9, 7, 3))
    (b, num, ff), _ = ops.background_accum(dev(Y), dev(np.zeros_like(f)), (9, 7, 3))
    assert ff.item() == 0 and (num == 0).all() and (b == 0).all()


def test_a_later_piece_may_not_be_larger(ops):
    Y, _, _, f = inputs((9, 7, 3))
    _, state = ops.background_accum(dev(Y[:16]), dev(f[:16]), (9, 7, 3), finish=False)
    with pytest.raises(ValueError, match="larger"):
        ops.background_accum(dev(Y), dev(f), (9, 7, 3), state=state, first=False)
    with pytest.raises(ValueError, match="one value"):
        ops.background_accum(dev(Y), dev(f[:5]), (9, 7, 3))


# ---- subtract -------------------------------------------------------------------------------------------------------------------
def check_subtract(got, Yh, b, f, clamp, what):
    want = Yh.astype(np.float64) - f.astype(np.float64)[:, None] * b.astype(np.float64)[None, :]
    if clamp:
        want = np.maximum(want, 0.0)
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    excess = np.abs(got.astype(np.float64) - want) - ulp(want)
    print(f"{what}: worst excess over one ulp {excess.max():.2e} (<= 0 passes), {int((want == 0).sum())} clamped of {want.size}")
    assert excess.max() <= 0, what
    if clamp:
        assert (got >= 0).all()


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("T", FRAMES)
@pytest.mark.parametrize("sz", SHAPES)
def test_subtract_matches_the_restatement(ops, sz, T, clamp):
    Y, _, b, f = inputs(sz)
    Y, f = Y[:T], f[:T]
    b2 = (2 * b).astype(np.float32)            # b f reaches 3: a good part of the differences is negative
    out = ops.background_subtract(dev(Y), dev(b2), dev(f), clamp=clamp)
    check_subtract(out, Y, b2, f, clamp, f"subtract {sz} T={T} clamp={clamp}")
    # in place, on rows with ld > P
    rows = padded(Y, 3)
    res = ops.background_subtract(rows, dev(b2), dev(f), out=rows, clamp=clamp)
    assert res.data_ptr() == rows.data_ptr()
    check_subtract(rows, Y, b2, f, clamp, f"subtract {sz} T={T} clamp={clamp} in place")


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("sz", SHAPES)
def test_subtract_with_frame_ids_and_times(ops, sz, clamp):
    """Rows taken in a permuted order, each with the entry of f its time names (f has more entries than the call has frames)."""
    Y, _, b, f = inputs(sz)
    b2 = (2 * b).astype(np.float32)
    rng = np.random.RandomState(9)
    rows_taken = rng.permutation(len(Y))[:20]
    times = rng.permutation(len(f))[:20]
    out = torch.full((20, Y.shape[1] + 5), float("nan"), dtype=torch.float32, device="cuda")[:, :Y.shape[1]]
    ops.background_subtract(padded(Y, 1), dev(b2), dev(f), frame_ids=dev(rows_taken, torch.int32), times=dev(times, torch.int32), out=out,
                            clamp=clamp)
    check_subtract(out, Y[rows_taken], b2, f[times], clamp, f"subtract {sz} frame_ids + times clamp={clamp}")
    # times alone: frames 0..19 with those entries of f
    out = ops.background_subtract(dev(Y), dev(b2), dev(f), times=dev(times, torch.int32), clamp=clamp)
    check_subtract(out, Y[:20], b2, f[times], clamp, f"subtract {sz} times clamp={clamp}")


def test_subtract_marks_a_time_without_an_entry(ops):
    Y, _, b, f = inputs((9, 7, 3))
    out = ops.background_subtract(dev(Y[:3]), dev(b), dev(f[:2]), times=dev(np.array([1, 2, 0]), torch.int32))
    got = out.cpu().numpy()
    assert np.isnan(got[1]).all() and not np.isnan(got[[0, 2]]).any()


# ---- determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sz", [(9, 7, 3), (64, 48, 1)])
def test_two_runs_give_the_same_bits(ops, sz):
    Y, M, b, f = inputs(sz)
    Yd, Md, bd, fd = dev(Y), dev(M), dev(b), dev(f)
    runs = []
    for _ in range(2):
        f1, num1, bb1 = ops.background_dots(Yd, bd, sub=Md)
        (b2, num2, ff2), _ = ops.background_accum(Yd, fd, sz, sub=Md)
        bf, ff = ops.background_fit(Yd, sz, 2, sub_fn=lambda s, e: Md[s:e], piece=13)
        runs.append([t.clone() for t in (f1, num1, bb1, b2, num2, ff2, bf, ff)])
    for x, y in zip(*runs):
        assert torch.equal(x, y)


# ---- the alternation ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fit_problem(sz=(20, 17, 1), T=37):
    """A seeded positive background b0 f0 on a model M plus noise, its restatement fit of three iterations, and the check that
    every half-step sum on the way is well conditioned (sum |terms| <= 10 |sum terms| for every f_t and for the b_p above 1e-3
    of the largest): there the fp32 roundings of the six half-steps propagate as 6 x 10 x 6e-8 < 1e-5."""
    P = sz[0] * sz[1] * sz[2]
    rng = np.random.RandomState(11)
    g = np.linspace(0.0, 1.0, P)
    b0 = 0.5 + g + 0.3 * np.sin(9 * g)
    b0[:7] = 0.0                                    # voxels without background: b stays near 0 there
    f0 = np.linspace(1.3, 0.7, T)
    M = rng.uniform(0.0, 2.0, (T, P)).astype(np.float32)
    Y = (M.astype(np.float64) + f0[:, None] * b0[None, :] + 0.002 * rng.randn(T, P)).astype(np.float32)
    r = BR.residual(Y, M)
    b = np.ones(P, dtype=np.float32)
    for _ in range(3):
        num, bb = BR.dots(Y, b, sub=M)
        assert (BR.dots_terms(Y, b, sub=M) <= 10 * np.abs(num)).all()
        f = BR.step(num, bb)
        num, ff = BR.accum(Y, f, sub=M)
        b = BR.step(num, ff)
        big = b > 1e-3 * b.max()
        assert big.sum() >= P - 7 and (BR.accum_terms(Y, f, sub=M)[big] <= 10 * np.abs(num[big])).all()
    want_b, want_f = BR.fit(Y, 3, sub=M)
    assert r.shape == (T, P) and abs(want_f.astype(np.float64).mean() - 1) <= 1e-6
    for a in (Y, M, want_b, want_f):
        a.setflags(write=False)
    return Y, M, want_b, want_f


@pytest.mark.parametrize("piece", [None, 13])
def test_background_fit_matches_the_restatement(ops, piece):
    sz = (20, 17, 1)
    Y, M, want_b, want_f = fit_problem()
    Yd, Md = dev(Y), dev(M)
    calls = []

    def sub_fn(s, e):
        calls.append((s, e))
        return Md[s:e]

    b, f = ops.background_fit(Yd, sz, 3, sub_fn=sub_fn, piece=piece)
    assert tuple(b.shape) == sz and tuple(f.shape) == (37,) and b.dtype == f.dtype == torch.float32
    assert calls == (3 * 2 * [(0, 13), (13, 26), (26, 37)] if piece else 6 * [(0, 37)])
    b, f = b.cpu().numpy().reshape(-1), f.cpu().numpy()
    assert (b >= 0).all() and (f >= 0).all()
    big = want_b > 1e-3 * want_b.max()
    print(f"fit piece={piece}: worst rel f {np.abs(f / want_f - 1).max():.2e}, worst rel b (large) {np.abs(b[big] / want_b[big] - 1).max():.2e}, "
          f"worst abs b (small) {np.abs(b[~big] - want_b[~big]).max():.2e}, mean f {f.astype(np.float64).mean():.8f}")
    np.testing.assert_allclose(f, want_f, rtol=1e-5)
    np.testing.assert_allclose(b[big], want_b[big], rtol=1e-5)
    np.testing.assert_allclose(b[~big], want_b[~big], rtol=0, atol=1e-5 * want_b.max())


def test_background_fit_without_a_model(ops):
    """No sub: the movie as it is, through ExponentialFP.background (numpy in, numpy out; CUDA in, CUDA out)."""
    from dnmf_amd.Demix.dNMF import ExponentialFP
    sz = (20, 17, 1)
    Y, M, _, _ = fit_problem()
    video = Y.reshape(37, *sz)
    want_b, want_f = BR.fit(video, 3)
    b, f = ExponentialFP.background(video, iters=3)
    assert isinstance(b, np.ndarray) and b.shape == sz and f.shape == (37,)
    np.testing.assert_allclose(f, want_f, rtol=1e-5)
    np.testing.assert_allclose(b.reshape(-1), want_b, rtol=1e-5)
    bd, fd = ExponentialFP.background(dev(video), iters=3)
    assert bd.is_cuda and fd.is_cuda
    np.testing.assert_array_equal(bd.cpu().numpy(), b)
    np.testing.assert_array_equal(fd.cpu().numpy(), f)
