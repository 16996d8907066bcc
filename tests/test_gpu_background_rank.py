"""The rank-R background kernels (K23: ``dnmf_background_dots_rank / _accum_rank / _subtract_rank``) and ``ops.background_fit_rank``
on the GPU against the float64 definition (tests/background_rank_restatement.py), each on identical inputs.

Tolerances.  ``num``, ``q`` and ``w`` are float64 sums of N <= 10^4 float64 terms: 1e-12 of the sum of the terms' magnitudes, K19's
bound.  The solve is checked on the GPU's own sums: the restatement's sweep, fed the ``num`` and ``q`` (``w``) the GPU returned and
the same start, does the same float64 operations in the same order, so the fp32 results agree to one ulp whatever the order of
the sums was.  ``subtract`` is float64 arithmetic rounded once: within one fp32 ulp of the restatement.

The whole fit, as measured on the MI355X: see ``test_fit_of_the_planted_video``."""
import functools

import numpy as np
import pytest
import torch

import background_restatement as BR
import background_rank_restatement as RR
from test_background_rank_host import SZ as PLANTED_SZ, planted, planted_fits, rank_entry_refusals

pytestmark = pytest.mark.gpu

# P = 7 and 1023: P % 4 != 0 (every other row starts off a 16-byte boundary: the float-by-float rows), below one tile of 1024 voxels;
# 1025: a second tile (and a second segment of dots) of one voxel; 24 x 20 x 2: two tiles, 16-byte rows
SHAPES = [(7, 1, 1), (1023, 1, 1), (41, 25, 1), (24, 20, 2)]
RANKS = [2, 3, 8]
T = 7
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
    n, P = x.shape
    buf = torch.full((n, P + pad), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :P] = dev(x)
    return buf[:, :P]


@functools.lru_cache(maxsize=None)
def inputs(sz, R):
    """Seeded inputs, computed once, never changed: frames Y and model M (T, P), images b (R, P), time courses f (R, T), and a
    permutation of the frames.  Y - M takes both signs and the components overlap, so the clamps of the sweeps are met."""
    P = sz[0] * sz[1] * sz[2]
    rng = np.random.RandomState(100 * R + P % 97)
    Y = rng.uniform(0.0, 2.0, (T, P)).astype(np.float32)
    M = rng.uniform(0.0, 1.5, (T, P)).astype(np.float32)
    b = rng.uniform(0.0, 1.0, (R, P)).astype(np.float32)
    f = rng.uniform(0.0, 1.5, (R, T)).astype(np.float32)
    perm = rng.permutation(T)
    for a in (Y, M, b, f, perm):
        a.setflags(write=False)
    return Y, M, b, f, perm


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def check_sums(got, want, terms, what):
    got, want, terms = (np.asarray(v, dtype=np.float64) for v in (got, want, terms))
    assert got.shape == want.shape, what
    worst = (np.abs(got - want) / np.maximum(terms, 1e-300)).max()
    print(f"{what}: worst |sum - restatement| / sum|terms| = {worst:.2e}")
    assert worst <= SUM_TOL, what


def check_solve(got, num, G, x0, inner, what):
    """The fp32 result against the restatement's sweep on the GPU's own sums."""
    want = RR.sweep(num, G, x0, inner)
    assert got.dtype == np.float32 and got.shape == want.shape and (got >= 0).all(), what
    excess = np.abs(got.astype(np.float64) - want.astype(np.float64)) - ulp(want)
    print(f"{what}: worst excess over one ulp {excess.max():.2e} (<= 0 passes), {int((want == 0).sum())} of {want.size} at the bound, "
          f"{int((got != want).sum())} differ at all")
    assert excess.max() <= 0, what


def check_dots(ops, sz, R, n, with_sub, permuted, inner=3):
    Y, M, b, f, perm = inputs(sz, R)
    rows = perm[:n] if permuted else np.arange(n)
    Yh, Mh, fh = Y[rows], (M[:n] if with_sub else None), np.ascontiguousarray(f[:, :n])
    fr = padded(Y, 3) if permuted else dev(Y[:n])
    sub = None if not with_sub else (padded(M[:n], 5) if permuted else dev(M[:n]))
    fd = dev(fh)
    got, num, q = ops.background_dots_rank(fr, dev(b), fd, sub=sub, frame_ids=dev(rows, torch.int32) if permuted else None, inner=inner)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and num.dtype == q.dtype == torch.float64
    assert tuple(got.shape) == tuple(num.shape) == (R, n) and tuple(q.shape) == (R, R)
    assert torch.equal(fd, dev(fh))                                             # the start is not changed
    what = f"dots {sz} R={R} B={n} sub={with_sub} permuted={permuted}"
    wantN, wantQ = RR.dots(Yh, b, sub=Mh)
    check_sums(num.cpu().numpy(), wantN, RR.dots_terms(Yh, b, sub=Mh), what + " num")
    check_sums(q.cpu().numpy(), wantQ, RR.gram_terms(b), what + " q")
    check_solve(got.cpu().numpy(), num.cpu().numpy(), q.cpu().numpy(), fh, inner, what + " f")


# ---- dots -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_sub", [False, True])
@pytest.mark.parametrize("R", RANKS)
@pytest.mark.parametrize("sz", SHAPES)
def test_dots_match_the_restatement(ops, sz, R, with_sub):
    """Seven frames taken in a permuted order from rows with ldf > P (the pads break the 16-byte phase, differently for frames and
    sub), and one frame from plain rows."""
    check_dots(ops, sz, R, T, with_sub, permuted=True)
    check_dots(ops, sz, R, 1, with_sub, permuted=False)


def test_dots_with_another_number_of_sweeps(ops):
    check_dots(ops, (41, 25, 1), 3, T, True, permuted=False, inner=1)
    check_dots(ops, (41, 25, 1), 3, T, True, permuted=False, inner=7)


# ---- accum ----------------------------------------------------------------------------------------------------------------------
def check_accum(got, b0, f, Yh, Mh, sz, R, inner, what):
    b, num, w = got
    assert b.dtype == torch.float32 and num.dtype == w.dtype == torch.float64
    assert tuple(b.shape) == tuple(num.shape) == (R,) + tuple(sz) and tuple(w.shape) == (R, R)
    wantN, wantW = RR.accum(Yh, f, sub=Mh)
    num, w = num.cpu().numpy().reshape(R, -1), w.cpu().numpy()
    check_sums(num, wantN, RR.accum_terms(Yh, f, sub=Mh), what + " num")
    check_sums(w, wantW, RR.gram_terms(f), what + " w")
    check_solve(b.cpu().numpy().reshape(R, -1), num, w, b0, inner, what + " b")


@pytest.mark.parametrize("with_sub", [False, True])
@pytest.mark.parametrize("R", RANKS)
@pytest.mark.parametrize("sz", SHAPES)
def test_accum_matches_the_restatement(ops, sz, R, with_sub):
    """Seven permuted frames in segments of three (three segments, the last of one frame) from padded rows, and one frame with the
    kernel's own segments."""
    Y, M, b, f, perm = inputs(sz, R)
    sub = padded(M, 5) if with_sub else None
    got, _ = ops.background_accum_rank(padded(Y, 3), dev(f), sz, b=dev(b).reshape(R, *sz), sub=sub, frame_ids=dev(perm, torch.int32),
                                       segment=3)
    torch.cuda.synchronize()
    check_accum(got, b, f, Y[perm], M if with_sub else None, sz, R, 3, f"accum {sz} R={R} B={T} segment=3 permuted sub={with_sub}")
    got, _ = ops.background_accum_rank(dev(Y[:1]), dev(f[:, :1]), sz, b=dev(b).reshape(R, *sz), sub=dev(M[:1]) if with_sub else None)
    check_accum(got, b, f[:, :1], Y[:1], M[:1] if with_sub else None, sz, R, 3, f"accum {sz} R={R} B=1 sub={with_sub}")


@pytest.mark.parametrize("R", RANKS)
@pytest.mark.parametrize("sz", [(1023, 1, 1), (41, 25, 1)])
def test_accum_in_two_pieces_through_the_state(ops, sz, R):
    """4 + 3 frames through one state, the time courses as views of the (R, 7) rows, against the restatement and against one call:
    the same sums up to their order, and from them the same solve.  No b: the solve starts from zero."""
    Y, M, _, f, _ = inputs(sz, R)
    Yd, Md, fd = dev(Y), dev(M), dev(f)
    state = ops.background_state_rank(sz, 4, R, segment=3)
    got = None
    for s, e in ((0, 4), (4, 7)):
        got, state = ops.background_accum_rank(Yd[s:e], fd[:, s:e], sz, sub=Md[s:e], state=state, first=s == 0, finish=e == 7, segment=3)
        assert (got is None) == (e != 7)
    torch.cuda.synchronize()
    zero = np.zeros((R, Y.shape[1]), np.float32)
    check_accum(got, zero, f, Y, M, sz, R, 3, f"accum {sz} R={R} in two pieces")
    one, _ = ops.background_accum_rank(Yd, fd, sz, sub=Md, segment=3)
    check_sums(got[1].cpu().numpy(), one[1].cpu().numpy(), RR.accum_terms(Y, f, sub=M).reshape(got[1].shape), "pieces against one call: num")
    check_sums(got[2].cpu().numpy(), one[2].cpu().numpy(), RR.gram_terms(f), "pieces against one call: w")
    # a reused state starts afresh with first=True
    again, _ = ops.background_accum_rank(Yd[:4], fd[:, :4], sz, sub=Md[:4], state=state, segment=3)
    check_accum(again, zero, f[:, :4], Y[:4], M[:4], sz, R, 3, f"accum {sz} R={R} on the reused state")
    with pytest.raises(ValueError, match="larger"):
        ops.background_accum_rank(Yd, fd, sz, state=ops.background_state_rank(sz, 2, R, segment=3), first=False, segment=3)


ONE_KERNEL_CASES = [(sz, segment, with_sub, 1) for sz in [(9, 7, 3), (1023, 1, 1)] for segment in (0, 5) for with_sub in (False, True)]
ONE_KERNEL_CASES.append(((1023, 1, 1), 5, True, 3))


@pytest.mark.parametrize("sz,segment,with_sub,pieces", ONE_KERNEL_CASES)
def test_rank_one_and_rank_r_run_one_accumulate_kernel(ops, sz, segment, with_sub, pieces):
    """K19's accumulate pass is the R = 1 instantiation of K23's: with a signed trace in row 0 of f and zeros in row 1, ``num[0]`` of
    the rank-2 call is ``num`` of the rank-1 call bit for bit -- the same subtraction, the same fma, the same segments added in the
    same order.  37 frames from rows padded by 3 (frames) and 5 (sub) floats, P % 4 != 0; once in three pieces through the states."""
    n, P = 37, sz[0] * sz[1] * sz[2]
    rng = np.random.RandomState(P + segment)
    Y = padded(rng.uniform(0.0, 2.0, (n, P)).astype(np.float32), 3)
    M = padded(rng.uniform(0.0, 1.5, (n, P)).astype(np.float32), 5) if with_sub else None
    f2 = torch.zeros((2, n), dtype=torch.float32, device="cuda")
    f2[0] = dev(rng.uniform(-1.0, 1.0, n))
    step = -(-n // pieces)
    state_r = ops.background_state_rank(sz, step, 2, segment=segment)
    state_1 = ops.background_state(sz, step, segment=segment)
    for s in range(0, n, step):
        e = min(n, s + step)
        sub = None if M is None else M[s:e]
        rank, state_r = ops.background_accum_rank(Y[s:e], f2[:, s:e], sz, sub=sub, state=state_r, first=s == 0, finish=e == n, segment=segment)
        one, state_1 = ops.background_accum(Y[s:e], f2[0, s:e], sz, sub=sub, state=state_1, first=s == 0, finish=e == n, segment=segment)
    torch.cuda.synchronize()
    assert rank[1].shape == (2, *sz) and one[1].shape == tuple(sz)
    assert bool(one[1].abs().max() > 0)
    assert torch.equal(rank[1][0], one[1]), f"{sz} segment={segment} sub={with_sub} pieces={pieces}"


# ---- zero diagonals -------------------------------------------------------------------------------------------------------------
def test_zero_diagonals_give_zero(ops):
    sz, R = (41, 25, 1), 3
    Y, _, b, f, _ = inputs(sz, R)
    b0, f0 = b.copy(), f.copy()
    b0[1], f0[2] = 0.0, 0.0
    got, num, q = ops.background_dots_rank(dev(Y), dev(b0), dev(f))
    assert q[1, 1].item() == 0 and (got[1] == 0).all() and (got[0] > 0).any() and torch.isfinite(got).all()
    (bn, num, w), _ = ops.background_accum_rank(dev(Y), dev(f0), sz, b=dev(b).reshape(R, *sz))
    assert w[2, 2].item() == 0 and (bn[2] == 0).all() and (bn[0] > 0).any() and torch.isfinite(bn).all()


# ---- subtract -------------------------------------------------------------------------------------------------------------------
def check_subtract(got, Yh, b, f, clamp, what):
    want = RR.subtract(Yh, b, f, clamp=clamp).astype(np.float64)
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    excess = np.abs(got.astype(np.float64) - want) - ulp(want)
    print(f"{what}: worst excess over one ulp {excess.max():.2e} (<= 0 passes), {int((want == 0).sum())} clamped of {want.size}")
    assert excess.max() <= 0, what
    if clamp:
        assert (got >= 0).all()


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("R", RANKS)
@pytest.mark.parametrize("sz", SHAPES)
def test_subtract_matches_the_restatement(ops, sz, R, clamp):
    Y, _, b, f, perm = inputs(sz, R)
    out = ops.background_subtract(dev(Y), dev(b), dev(f), clamp=clamp)              # dispatches on f (R, T)
    check_subtract(out, Y, b, f, clamp, f"subtract {sz} R={R} clamp={clamp}")
    # in place, on rows with ld > P
    rows = padded(Y, 3)
    res = ops.background_subtract_rank(rows, dev(b).reshape(R, *sz), dev(f), out=rows, clamp=clamp)
    assert res.data_ptr() == rows.data_ptr()
    check_subtract(rows, Y, b, f, clamp, f"subtract {sz} R={R} clamp={clamp} in place")
    # rows in a permuted order, each with the entry of f its time names
    times = np.random.RandomState(9).permutation(T)[:5]
    out = ops.background_subtract_rank(padded(Y, 1), dev(b), dev(f), frame_ids=dev(perm[:5], torch.int32), times=dev(times, torch.int32),
                                       clamp=clamp)
    check_subtract(out, Y[perm[:5]], b, f[:, times], clamp, f"subtract {sz} R={R} frame_ids + times clamp={clamp}")


def test_subtract_marks_a_time_without_an_entry(ops):
    Y, _, b, f, _ = inputs((1023, 1, 1), 3)
    out = ops.background_subtract_rank(dev(Y[:3]), dev(b), dev(np.ascontiguousarray(f[:, :2])), times=dev(np.array([1, 2, 0]), torch.int32))
    got = out.cpu().numpy()
    assert np.isnan(got[1]).all() and not np.isnan(got[[0, 2]]).any()
    out = ops.background_subtract_rank(dev(Y[:2]), dev(b), dev(f), times=dev(np.array([-1, 0]), torch.int32), clamp=False)
    assert torch.isnan(out[0]).all() and not torch.isnan(out[1]).any()


# ---- determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [2, 8])
def test_two_runs_give_the_same_bits(ops, R):
    sz = (41, 25, 1)
    Y, M, b, f, _ = inputs(sz, R)
    Yd, Md, bd, fd = dev(Y), dev(M), dev(b), dev(f)
    runs = []
    for _ in range(2):
        f1, num1, q1 = ops.background_dots_rank(Yd, bd, fd, sub=Md)
        (b2, num2, w2), _ = ops.background_accum_rank(Yd, fd, sz, b=bd.reshape(R, *sz), sub=Md, segment=3)
        bf, ff = ops.background_fit_rank(Yd, sz, 2, min(R, T), sub_fn=lambda s, e: Md[s:e], piece=3)
        runs.append([t.clone() for t in (f1, num1, q1, b2, num2, w2, bf, ff)])
    for x, y in zip(*runs):
        assert torch.equal(x, y)


# ---- the whole fit --------------------------------------------------------------------------------------------------------------
FIT_DEVIATION = 2.3e-9    # measured on the MI355X, see the docstring below


@pytest.mark.parametrize("piece", [None, 13])
def test_fit_of_the_planted_video(ops, piece):
    """``ops.background_fit_rank(rank=2)`` on the planted rank-2 video of tests/test_background_rank_host.py: the squared error after six
    alternations relative to the restatement's, and the planted ratios on the GPU result (rank 1 leaves at least 5 times the noise
    energy, rank 2 at most 1.2 times).  Measured on the MI355X, for both ``piece``: rank 1 leaves 28.2793 times the noise energy,
    rank 2 0.9729 times; squared error 1.494328119e+01 against the restatement's 1.494328116e+01, a relative deviation of 2.252e-09
    (the two differ in the order of the float64 sums and in the fp32 mean of the rescale).  Asserted: ten times that."""
    Y, noise = planted()
    _, want_err2, _, _, _ = planted_fits()
    Yd = dev(Y)
    r = BR.residual(Y)
    B, F = ops.background_fit_rank(Yd, PLANTED_SZ, 6, 2, piece=piece)
    assert tuple(B.shape) == (2,) + PLANTED_SZ and tuple(F.shape) == (2, Y.shape[0]) and B.dtype == F.dtype == torch.float32
    assert (B >= 0).all() and (F >= 0).all()
    np.testing.assert_allclose(F.double().mean(1).cpu().numpy(), 1.0, atol=1e-6)
    err2 = RR.sqerr(r, B.cpu().numpy(), F.cpu().numpy())
    b1, f1 = ops.background_fit(Yd, PLANTED_SZ, 6, piece=piece)
    err1 = float(((r - f1.double().cpu().numpy()[:, None] * b1.double().cpu().numpy().reshape(-1)[None, :]) ** 2).sum())
    deviation = abs(err2 - want_err2) / want_err2
    print(f"planted fit piece={piece}: rank 1 leaves {err1 / noise:.4f} x the noise energy, rank 2 {err2 / noise:.4f} x; "
          f"squared error {err2:.9e} against the restatement's {want_err2:.9e}: relative deviation {deviation:.3e}")
    assert err1 >= 5 * noise
    assert err2 <= 1.2 * noise
    assert deviation <= 10 * FIT_DEVIATION


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(ops):
    from dnmf_amd import _lib
    rank_entry_refusals(_lib.load())          # the C entries: each code, nothing launched
    sz = (7, 1, 1)
    Y, _, b, f, _ = inputs(sz, 2)
    Yd = dev(Y)
    for R in (1, 9):
        bb, ff = torch.ones((R, 7), device="cuda"), torch.ones((R, T), device="cuda")
        with pytest.raises(ValueError, match="components"):
            ops.background_dots_rank(Yd, bb, ff)
        with pytest.raises(ValueError, match="components"):
            ops.background_accum_rank(Yd, ff, sz)
        with pytest.raises(ValueError, match="components"):
            ops.background_subtract_rank(Yd, bb, ff)
    with pytest.raises(ValueError, match="components"):
        ops.background_fit_rank(Yd, sz, 1, 9)
    with pytest.raises(ValueError, match="rank=8 for 7 frames"):
        ops.background_fit_rank(Yd, sz, 1, 8)
    with pytest.raises(ValueError, match="inner"):
        ops.background_dots_rank(Yd, dev(b), dev(f), inner=0)
    with pytest.raises(ValueError, match="time courses"):
        ops.background_dots_rank(Yd, dev(b), torch.ones((3, T), device="cuda"))
    with pytest.raises(ValueError, match="frames"):
        ops.background_dots_rank(Yd, dev(b), dev(f[:, :5].copy()))
    torch.cuda.synchronize()
