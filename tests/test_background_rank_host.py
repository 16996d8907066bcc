"""The rank-R background (K23) without a GPU: the float64 restatement (tests/background_rank_restatement.py) on cases whose answer
is known -- the optimality conditions of the solve, the monotone descent of the alternation, a planted rank-2 video that a rank-1
term cannot explain, the degenerate cases -- and the ABI and the argument checks of the C entries on the library as built."""
import ctypes
import functools
import inspect

import numpy as np
import pytest

import background_restatement as BR
import background_rank_restatement as RR


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


# ---- 1. the solve ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [2, 3, 8])
def test_many_sweeps_satisfy_the_kkt_conditions(R):
    """A frame's problem min |r - sum_j b_j f_j|^2 over f >= 0 is 1/2 f^T Q f - N^T f with Q = B^T B, N = B^T r, and N - Q f is its
    negative gradient: at the minimum g = Q f - N has g_j = 0 where f_j > 0 and g_j >= 0 where f_j = 0.  200 sweeps reach that to
    1e-10 of |N|.  The rows of B are Gaussian, 100 long: Q has a condition number of about (1 + sqrt(R / 100))^2 /
    (1 - sqrt(R / 100))^2 <= 3.2, so that coordinate descent contracts by a constant factor per sweep; the targets mix signs so that
    some coordinates end at the bound."""
    rng = np.random.RandomState(R)
    B = rng.randn(R, 100).astype(np.float32)
    Q = RR.gram(B)
    N = rng.randn(R, 64) * np.sqrt(np.diag(Q))[:, None]
    f = RR.sweep64(N, Q, np.zeros_like(N), inner=200)
    g = Q @ f - N
    scale = np.abs(N).max()
    assert (f >= 0).all()
    clamped = f == 0
    assert clamped.any() and (~clamped).any()
    print(f"R={R}: worst |g| on the free set {np.abs(g[~clamped]).max() / scale:.2e}, least g on the bound {g[clamped].min() / scale:.2e}")
    assert np.abs(g[~clamped]).max() <= 1e-10 * scale
    assert g[clamped].min() >= -1e-10 * scale


def test_the_default_sweeps_are_a_parameter_not_a_tolerance():
    """Three sweeps are three sweeps: the result differs from the converged one and is the same every time."""
    rng = np.random.RandomState(0)
    Q = RR.gram(rng.uniform(0, 1, (3, 20)).astype(np.float32))
    N = Q @ rng.uniform(0.5, 1.5, (3, 5))          # the minimum is interior, and Q's rows are far from orthogonal
    a, b = RR.sweep64(N, Q, np.zeros_like(N)), RR.sweep64(N, Q, np.zeros_like(N), inner=3)
    np.testing.assert_array_equal(a, b)
    assert np.abs(a - RR.sweep64(N, Q, np.zeros_like(N), inner=200)).max() > 1e-6
    assert inspect.signature(RR.fit).parameters["inner"].default == 3


def test_zero_diagonals_give_zero():
    Q = np.array([[2.0, 0.0, 1.0], [0.0, 0.0, 0.0], [1.0, 0.0, 3.0]])
    N = np.array([[1.0], [5.0], [2.0]])
    f = RR.sweep(N, Q, np.ones((3, 1), np.float32))
    assert f.dtype == np.float32 and f[1, 0] == 0 and np.isfinite(f).all() and f[0, 0] > 0 and f[2, 0] > 0


# ---- 2. the planted rank-2 video ------------------------------------------------------------------------------------------------
SZ, T, SIGMA = (24, 20, 2), 40, 0.02


@functools.lru_cache(maxsize=None)
def planted():
    """24 x 20 x 2 x 40 frames: two non-negative images with nearly disjoint support (a bump on either side of the plane over a
    small common floor), one time course e^{-t/15}, one rising t/T, Gaussian noise of sigma 0.02 added, clipped at 0.  The common
    floor of 0.2 keeps the clip rare (10 sigma).  Made once, never changed."""
    rng = np.random.RandomState(23)
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in SZ], indexing="ij")
    b1 = (0.2 + 1.0 * np.exp(-((x - 6) ** 2 + (y - 10) ** 2) / 30.0)).reshape(-1)
    b2 = (0.2 + 0.8 * np.exp(-((x - 18) ** 2 + (y - 9) ** 2) / 30.0)).reshape(-1) * (1.0 + 0.1 * z.reshape(-1))
    t = np.arange(T, dtype=np.float64)
    f1, f2 = np.exp(-t / 15.0), t / T
    Y = np.maximum(f1[:, None] * b1[None, :] + f2[:, None] * b2[None, :] + SIGMA * rng.randn(T, b1.size), 0.0).astype(np.float32)
    Y.setflags(write=False)
    return Y, SIGMA ** 2 * T * b1.size


@functools.lru_cache(maxsize=None)
def planted_fits():
    """The restatement's rank-1 (K19) and rank-2 fits of six alternations, with the rank-2 history of the squared error."""
    Y, _ = planted()
    r = BR.residual(Y)
    b, f = BR.fit(Y, 6)
    err1 = float(((r - f.astype(np.float64)[:, None] * b.astype(np.float64)[None, :]) ** 2).sum())
    history = []
    B, F = RR.fit(Y, 6, 2, history=history)
    return err1, RR.sqerr(r, B, F), tuple(history), B, F


def test_rank_two_explains_what_rank_one_cannot():
    """The reason the feature exists: after six alternations the rank-1 term leaves at least 5 times the planted noise energy
    sigma^2 T P, the rank-2 term at most 1.2 times."""
    _, noise = planted()
    err1, err2, _, B, F = planted_fits()
    print(f"planted rank-2 video: rank 1 leaves {err1 / noise:.3f} x the noise energy, rank 2 leaves {err2 / noise:.3f} x")
    assert err1 >= 5 * noise
    assert err2 <= 1.2 * noise
    assert B.shape == (2, 960) and F.shape == (2, T) and B.dtype == F.dtype == np.float32
    assert (B >= 0).all() and (F >= 0).all()
    np.testing.assert_allclose(F.astype(np.float64).mean(1), 1.0, atol=1e-6)


def monotone(history, what):
    """No half-step raises the squared error, up to the fp32 rounding of the factors it stores (1e-6 of the error it starts from:
    rounding b or f by 6e-8 relative moves a term of the error by as much)."""
    h = np.array(history)
    print(f"{what}: squared error {h[0]:.6e} -> {h[-1]:.6e} over {len(h) - 1} half-steps, largest rise {np.diff(h).max():.2e}")
    assert len(h) >= 3 and (np.diff(h) <= 1e-6 * h[0]).all(), what


def test_every_half_step_descends():
    _, _, history, _, _ = planted_fits()
    assert len(history) == 13
    monotone(history, "planted")
    # with a subtracted model and three components
    rng = np.random.RandomState(5)
    Y = rng.uniform(0, 2, (17, 45)).astype(np.float32)
    M = rng.uniform(0, 1, (17, 45)).astype(np.float32)
    history = []
    RR.fit(Y, 4, 3, sub=M, history=history)
    monotone(history, "random, sub, R=3")


# ---- 3. degenerate cases --------------------------------------------------------------------------------------------------------
def test_a_component_without_an_image_gets_no_time_course():
    """The frames of the first block are below the model: its clipped block mean is b_0 = 0, Q_00 = 0, so f_0 = 0, and it stays
    there (W_00 = 0 gives b_0 = 0); everything stays finite and the rescale skips the component."""
    rng = np.random.RandomState(6)
    Y = rng.uniform(1.0, 2.0, (12, 30)).astype(np.float32)
    M = np.zeros_like(Y)
    M[:6] = 5.0
    history = []
    B, F = RR.fit(Y, 3, 2, sub=M, history=history)
    assert (B[0] == 0).all() and (F[0] == 0).all()
    assert (B[1] > 0).all() and np.isfinite(B).all() and np.isfinite(F).all()
    monotone(history, "one empty component")


def test_a_constant_background_stays_finite_and_monotone():
    """A background that does not change in time: the block means are equal up to noise, the starts nearly collinear and Q
    nearly singular.  The sweeps divide by the diagonal only, so nothing blows up."""
    rng = np.random.RandomState(7)
    b0 = rng.uniform(0.5, 1.5, 60)
    Y = (b0[None, :] + 1e-4 * rng.randn(20, 60)).astype(np.float32)
    for R in (2, 3):
        history = []
        B, F = RR.fit(Y, 6, R, history=history)
        assert np.isfinite(B).all() and np.isfinite(F).all() and (B >= 0).all() and (F >= 0).all()
        monotone(history, f"constant background, R={R}")
        assert history[-1] <= 2 * 1e-8 * Y.size


def test_start_and_refusals():
    B, F = RR.start(7, 5, 3)
    assert (B == 0).all() and B.shape == (3, 5)
    np.testing.assert_array_equal(F.argmax(0), [0, 0, 0, 1, 1, 2, 2])
    assert (F.sum(0) == 1).all()
    for R in (1, 9):
        with pytest.raises(ValueError, match="outside"):
            RR.start(40, 5, R)
    with pytest.raises(ValueError, match="frames"):
        RR.start(2, 5, 3)


def test_subtract_adds_the_components_in_their_order():
    rng = np.random.RandomState(8)
    Y = rng.uniform(0, 1, (7, 5, 3, 2)).astype(np.float32)
    B = rng.uniform(0, 0.6, (3, 5, 3, 2)).astype(np.float32)
    F = rng.uniform(0.5, 1.5, (3, 7)).astype(np.float32)
    raw, cl = RR.subtract(Y, B, F, clamp=False), RR.subtract(Y, B, F)
    assert raw.dtype == np.float32 and raw.shape == Y.shape and (raw < 0).any() and (raw > 0).any() and (cl >= 0).all()
    np.testing.assert_array_equal(cl, np.maximum(raw, 0))
    s = sum(F[j].astype(np.float64)[:, None, None, None] * B[j].astype(np.float64)[None] for j in range(3))
    np.testing.assert_array_equal(raw, (Y.astype(np.float64) - s).astype(np.float32))


# ---- 4. the ABI on the library as built -----------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_entries(lib):
    from dnmf_amd import _lib
    for name in ("dnmf_background_dots_rank", "dnmf_background_accum_rank", "dnmf_background_subtract_rank"):
        assert _lib.SIGNATURES[name][0] is ctypes.c_int, name
        assert getattr(lib, name)


def test_public_signatures():
    from dnmf_amd import ops
    from dnmf_amd.Demix.dNMF import DeformableNMF, ExponentialFP

    def default(fn, name):
        return inspect.signature(fn).parameters[name].default

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    # the rank-1 entry points keep their signatures; the rank-R ones stand beside them
    assert params(ops.background_fit) == [("frames", E), ("sz", E), ("iters", E), ("sub_fn", None), ("piece", None)]
    assert params(ops.background_fit_rank) == [("frames", E), ("sz", E), ("iters", E), ("rank", E), ("sub_fn", None), ("piece", None),
                                               ("inner", 3)]
    assert params(DeformableNMF.update_background_rank) == [("self", E), ("loader", E), ("iters", 3), ("rank", 2), ("inner", 3)]
    assert isinstance(inspect.getattr_static(ExponentialFP, "background_rank"), staticmethod)
    assert params(ExponentialFP.background_rank) == [("video", E), ("iters", 3), ("rank", 2), ("inner", 3)]
    assert default(DeformableNMF.fit, "background_rank") == 1
    for name in ("background_dots_rank", "background_accum_rank", "background_subtract_rank", "background_state_rank"):
        assert callable(getattr(ops, name))
    assert default(ops.background_dots_rank, "inner") == 3 and default(ops.background_accum_rank, "inner") == 3


def rank_entry_refusals(lib):
    """Every refusal of the three entries, on host pointers: validation happens before any HIP call, nothing is launched."""
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    P = 20 * 17

    def call(fn, names, ok, **kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return fn(*args)

    # ---- dots
    ws, run = lib.dnmf_background_dots_rank_workspace, lib.dnmf_background_dots_rank
    for R in (1, 9, 0, -1):
        assert ws(P, 4, R) == 0 and b"components" in lib.dnmf_last_error(), R
    assert ws(P, 0, 2) == 0 and ws(0, 4, 2) == 0 and ws(1 << 31, 4, 2) == 0
    sizes = [ws(P, 4, R) for R in range(2, 9)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
    need = ws(P, 4, 3)
    names = ["frames", "ldf", "sub", "lds", "frame_ids", "b", "ldb", "R", "P", "B", "inner", "f", "ldf_t", "num", "q", "workspace", "bytes",
             "stream"]
    ok = (a, P, None, 0, None, a, P, 3, P, 4, 3, a, 4, a, a, a, need, None)
    for name in ("frames", "b", "f", "workspace"):
        assert call(run, names, ok, **{name: None}) == -1 and lib.dnmf_last_error().startswith(b"dnmf_background_dots_rank: "), name
    for R in (1, 9):
        assert call(run, names, ok, R=R) == -3 and b"components" in lib.dnmf_last_error()
    assert call(run, names, ok, inner=0) == -2 and b"inner=0" in lib.dnmf_last_error()
    assert call(run, names, ok, B=0) == -2
    assert call(run, names, ok, ldf=P - 1) == -2
    assert call(run, names, ok, sub=a, lds=P - 1) == -2
    assert call(run, names, ok, ldb=P - 1) == -2 and b"ldb" in lib.dnmf_last_error()
    assert call(run, names, ok, ldf_t=3) == -2 and b"ldf_t" in lib.dnmf_last_error()
    assert call(run, names, ok, P=1 << 31, ldf=1 << 31, ldb=1 << 31) == -3
    assert call(run, names, ok, bytes=need - 1) == -4 and str(need).encode() in lib.dnmf_last_error()
    assert call(run, names, ok, workspace=a + 4) == -4 and b"aligned" in lib.dnmf_last_error()

    # ---- accum
    ws, run = lib.dnmf_background_accum_rank_workspace, lib.dnmf_background_accum_rank
    for R in (1, 9):
        assert ws(P, 4, R, 0) == 0 and b"components" in lib.dnmf_last_error()
    assert ws(P, 0, 2, 0) == 0 and ws(P, 4, 2, -1) == 0 and ws(1 << 31, 4, 2, 0) == 0 and ws(P, 10 ** 6, 2, 1) == 0
    sizes = [ws(P, B, 3, 0) for B in range(1, 200)]
    assert sizes[0] > 0 and sizes == sorted(sizes)
    need = ws(P, 4, 3, 0)
    names = ["frames", "ldf", "sub", "lds", "frame_ids", "f", "ldf_t", "R", "P", "B", "first", "finish", "segment", "inner", "state", "bytes",
             "b", "ldb", "num", "w", "stream"]
    ok = (a, P, None, 0, None, a, 4, 3, P, 4, 1, 1, 0, 3, a, need, a, P, a, a, None)
    for name in ("frames", "f", "state", "b"):
        assert call(run, names, ok, **{name: None}) == -1 and lib.dnmf_last_error().startswith(b"dnmf_background_accum_rank: "), name
    for R in (1, 9):
        assert call(run, names, ok, R=R) == -3 and b"components" in lib.dnmf_last_error()
    assert call(run, names, ok, inner=0) == -2
    assert call(run, names, ok, B=0) == -2
    assert call(run, names, ok, segment=-2) == -2
    assert call(run, names, ok, ldf=P - 1) == -2
    assert call(run, names, ok, sub=a, lds=P - 1) == -2
    assert call(run, names, ok, ldb=P - 1) == -2
    assert call(run, names, ok, ldf_t=3) == -2
    assert call(run, names, ok, B=10 ** 6, ldf_t=10 ** 6, segment=1) == -3
    assert call(run, names, ok, bytes=need - 1) == -4 and str(need).encode() in lib.dnmf_last_error()
    assert call(run, names, ok, state=a + 4) == -4 and b"aligned" in lib.dnmf_last_error()

    # ---- subtract
    run = lib.dnmf_background_subtract_rank
    names = ["frames", "ldf", "frame_ids", "b", "ldb", "f", "ldf_t", "R", "nf", "times", "P", "B", "out", "ldo", "clamp", "stream"]
    ok = (a, P, None, a, P, a, 4, 3, 4, None, P, 4, a + 32, P, 1, None)
    for name in ("frames", "b", "f", "out"):
        assert call(run, names, ok, **{name: None}) == -1 and lib.dnmf_last_error().startswith(b"dnmf_background_subtract_rank: "), name
    for R in (1, 9):
        assert call(run, names, ok, R=R) == -3 and b"components" in lib.dnmf_last_error()
    assert call(run, names, ok, B=0) == -2
    assert call(run, names, ok, nf=0) == -2
    assert call(run, names, ok, ldf=P - 1) == -2
    assert call(run, names, ok, ldo=P - 1) == -2
    assert call(run, names, ok, ldb=P - 1) == -2
    assert call(run, names, ok, ldf_t=3) == -2
    assert call(run, names, ok, B=5) == -2 and b"times" in lib.dnmf_last_error()
    assert call(run, names, ok, out=a, frame_ids=a) == -2 and b"in place" in lib.dnmf_last_error()
    assert call(run, names, ok, out=a, ldo=P + 4) == -2
    assert call(run, names, ok, P=1 << 31, ldf=1 << 31, ldo=1 << 31, ldb=1 << 31) == -3


def test_argument_errors_of_the_rank_entries(lib):
    rank_entry_refusals(lib)
