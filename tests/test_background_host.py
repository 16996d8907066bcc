"""The rank-1 background (K19) without a GPU: the float64 restatement (tests/background_restatement.py) on cases whose answer is
known in closed form, and the ABI, the wiring and the argument checks of the C entries on the library as built."""
import ctypes
import inspect

import numpy as np
import pytest

import background_restatement as BR


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


def rank_one(T=23, sz=(6, 5, 2), seed=0):
    rng = np.random.RandomState(seed)
    b0 = rng.uniform(0.5, 2.0, sz)
    f0 = rng.uniform(0.7, 1.3, T)
    return b0, f0, (f0[:, None, None, None] * b0[None]).astype(np.float32)


# ---- 1. exact recovery ----------------------------------------------------------------------------------------------------------
def test_one_iteration_recovers_a_rank_one_residual():
    """From b = 1 the f-step gives f proportional to f0 and the b-step then b0 times the inverse factor: one iteration is exact,
    only the fp32 rounding of R, f and b remains."""
    b0, f0, R = rank_one()
    b, f = BR.fit(R, iters=1)
    assert b.dtype == np.float32 and f.dtype == np.float32 and b.shape == (b0.size,) and f.shape == f0.shape
    got = f.astype(np.float64)[:, None] * b.astype(np.float64)[None, :]
    np.testing.assert_allclose(got, R.reshape(len(f0), -1).astype(np.float64), rtol=1e-6)
    np.testing.assert_allclose(got, f0[:, None] * b0.reshape(-1)[None, :], rtol=1e-6)
    assert abs(f.astype(np.float64).mean() - 1.0) <= 1e-6
    # more iterations stay there
    b3, f3 = BR.fit(R, iters=3)
    np.testing.assert_allclose(f3.astype(np.float64)[:, None] * b3.astype(np.float64)[None, :], got, rtol=1e-6)


def test_recovery_under_a_subtracted_model():
    """frames = fp32(M + R) with |M| <= 10 |R|: the fp32 storage of the sum costs 6e-8 |Y| / |R| <= 7e-7 of R per entry."""
    b0, f0, R = rank_one(seed=1)
    rng = np.random.RandomState(2)
    M = (rng.uniform(0.0, 10.0, R.shape) * R.min()).astype(np.float32)
    assert np.abs(M).max() <= 10 * np.abs(R).min()
    Y = (M.astype(np.float64) + f0[:, None, None, None] * b0[None]).astype(np.float32)
    b, f = BR.fit(Y, iters=1, sub=M)
    got = f.astype(np.float64)[:, None] * b.astype(np.float64)[None, :]
    np.testing.assert_allclose(got, f0[:, None] * b0.reshape(-1)[None, :], rtol=1e-5)
    assert abs(f.astype(np.float64).mean() - 1.0) <= 1e-6


def test_half_steps_are_the_least_squares_minimisers():
    rng = np.random.RandomState(3)
    Y = rng.uniform(0, 2, (9, 4, 3, 1)).astype(np.float32)
    M = rng.uniform(0, 1, Y.shape).astype(np.float32)
    b = rng.uniform(0, 1, 12).astype(np.float32)
    r = Y.reshape(9, -1).astype(np.float64) - M.reshape(9, -1).astype(np.float64)
    num, bb = BR.dots(Y, b, sub=M)
    np.testing.assert_allclose(num, r @ b.astype(np.float64), rtol=1e-13)
    assert abs(bb - float(b.astype(np.float64) @ b.astype(np.float64))) <= 1e-13 * bb
    f = BR.step(num, bb)
    num_p, ff = BR.accum(Y, f, sub=M)
    np.testing.assert_allclose(num_p, f.astype(np.float64) @ r, rtol=1e-13)
    assert abs(ff - float(f.astype(np.float64) @ f.astype(np.float64))) <= 1e-13 * ff
    # a step is the minimiser: moving any coordinate either way does not lower the squared error
    bn = BR.step(num_p, ff).astype(np.float64)
    base = ((r - f.astype(np.float64)[:, None] * bn[None, :]) ** 2).sum()
    for p in range(12):
        for d in (-1e-3, 1e-3):
            moved = bn.copy()
            moved[p] = max(0.0, moved[p] + d)
            assert ((r - f.astype(np.float64)[:, None] * moved[None, :]) ** 2).sum() >= base - 1e-12


# ---- 2. non-negativity and degenerate cases -------------------------------------------------------------------------------------
def test_negative_residual_gives_zero_never_a_negative_value():
    b0, f0, R = rank_one(seed=4)
    M = np.zeros_like(R)
    M[:, :2] = 2 * R[:, :2]              # the model over-explains the voxels of the first two x planes: r < 0 there
    b, f = BR.fit(R, iters=2, sub=M)
    b = b.reshape(b0.shape)
    assert (b[:2] == 0).all() and (b[2:] > 0).all() and (b >= 0).all() and (f >= 0).all()
    num, ff = BR.accum(R, f, sub=M)
    assert (num.reshape(b0.shape)[:2] < 0).all()
    # and the other way round: frames below the model give f = 0
    M2 = np.zeros_like(R)
    M2[3] = 2 * R[3]
    _, f2 = BR.fit(R, iters=1, sub=M2)
    assert f2[3] == 0 and (np.delete(f2, 3) > 0).all()


def test_zero_factors():
    _, _, R = rank_one(seed=5)
    T, P = R.shape[0], R[0].size
    num, ff = BR.accum(R, np.zeros(T, np.float32))
    assert ff == 0 and (BR.step(num, ff) == 0).all() and BR.step(num, ff).dtype == np.float32
    num, bb = BR.dots(R, np.zeros(P, np.float32))
    assert bb == 0 and (BR.step(num, bb) == 0).all()
    # an all-negative residual: f = 0 after the first half-step, then b = 0, and the scale is skipped
    b, f = BR.fit(np.zeros_like(R), iters=2, sub=R)
    assert (b == 0).all() and (f == 0).all()


def test_subtract_and_its_clamp():
    rng = np.random.RandomState(6)
    Y = rng.uniform(0, 1, (7, 5, 3, 2)).astype(np.float32)
    b = rng.uniform(0, 1.5, (5, 3, 2)).astype(np.float32)
    f = rng.uniform(0.5, 1.5, 7).astype(np.float32)
    raw, cl = BR.subtract(Y, b, f, clamp=False), BR.subtract(Y, b, f)
    assert raw.dtype == np.float32 and raw.shape == Y.shape and cl.shape == Y.shape
    assert (raw < 0).any() and (raw > 0).any()
    assert (cl >= 0).all()
    np.testing.assert_array_equal(cl[raw >= 0], raw[raw >= 0])
    assert (cl[raw < 0] == 0).all()
    want = Y.astype(np.float64) - f.astype(np.float64)[:, None, None, None] * b.astype(np.float64)[None]
    np.testing.assert_array_equal(raw, want.astype(np.float32))


# ---- 3. the ABI on the library as built -----------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_entries(lib):
    from dnmf_amd import _lib, build
    assert _lib.SIGNATURES["dnmf_background_dots_workspace"] == (ctypes.c_size_t, [ctypes.c_long, ctypes.c_int])
    assert _lib.SIGNATURES["dnmf_background_accum_workspace"] == (ctypes.c_size_t, [ctypes.c_long, ctypes.c_int, ctypes.c_int])
    for name in ("dnmf_background_dots", "dnmf_background_accum", "dnmf_background_subtract"):
        assert _lib.SIGNATURES[name][0] is ctypes.c_int, name
        assert getattr(lib, name)          # exported
    assert "background.hip" in build.SOURCES


def test_public_signatures():
    from dnmf_amd import ops
    from dnmf_amd.Demix.dNMF import DeformableNMF, ExponentialFP

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(ops.background_state) == [("sz", E), ("B", E), ("segment", 0), ("device", "cuda")]
    assert params(ops.background_dots) == [("frames", E), ("b", E), ("sub", None), ("frame_ids", None)]
    assert params(ops.background_accum) == [("frames", E), ("f", E), ("sz", E), ("sub", None), ("frame_ids", None), ("state", None),
                                            ("first", True), ("finish", True), ("segment", 0)]
    assert params(ops.background_subtract) == [("frames", E), ("b", E), ("f", E), ("frame_ids", None), ("times", None), ("out", None),
                                               ("clamp", True)]
    assert params(ops.background_fit) == [("frames", E), ("sz", E), ("iters", E), ("sub_fn", None), ("piece", None)]
    assert isinstance(inspect.getattr_static(ExponentialFP, "background"), staticmethod)
    assert params(ExponentialFP.background) == [("video", E), ("iters", 3)]
    assert params(DeformableNMF.update_background) == [("self", E), ("loader", E), ("iters", 3)]
    assert params(DeformableNMF.background_loader) == [("self", E), ("loader", E)]
    assert inspect.signature(DeformableNMF.fit).parameters["background"].default == 0


def test_argument_errors_of_the_background_entries(lib):
    """Validation happens before any HIP call, so it can be exercised on a CPU-only box."""
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    P = 20 * 17

    def al(n):
        return (n + 255) // 256 * 256

    # ---- dots
    ws, run = lib.dnmf_background_dots_workspace, lib.dnmf_background_dots
    # segments are multiples of 1024 voxels, as many as give 4096 workgroups: P = 340 is one, 3072 voxels are three
    assert ws(P, 37) == al(37 * 8) + al(8)
    assert ws(3072, 37) == al(37 * 3 * 8) + al(3 * 8)
    assert ws(1 << 18, 4000) == al(4000 * 2 * 8) + al(2 * 8)
    assert ws(P, 0) == 0 and lib.dnmf_last_error().startswith(b"dnmf_background_dots_workspace: ") and b"B=0" in lib.dnmf_last_error()
    assert ws(0, 4) == 0 and b"P=0" in lib.dnmf_last_error()
    assert ws(1 << 31, 4) == 0 and b"32-bit" in lib.dnmf_last_error()
    need = ws(P, 4)
    names = ["frames", "ldf", "sub", "lds", "frame_ids", "b", "P", "B", "num", "bb", "f", "workspace", "bytes", "stream"]
    ok = (a, P, None, 0, None, a, P, 4, a, a, a, a, need, None)

    def call(fn, names, ok, **kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return fn(*args)

    for name in ("frames", "b", "f", "workspace"):
        assert call(run, names, ok, **{name: None}) == -1 and lib.dnmf_last_error().startswith(b"dnmf_background_dots: "), name
    assert call(run, names, ok, B=0) == -2 and b"B=0" in lib.dnmf_last_error()
    assert call(run, names, ok, P=0, ldf=0) == -2
    assert call(run, names, ok, ldf=P - 1) == -2 and b"ldf" in lib.dnmf_last_error()
    assert call(run, names, ok, sub=a, lds=P - 1) == -2
    assert call(run, names, ok, P=1 << 31, ldf=1 << 31) == -3
    assert call(run, names, ok, bytes=need - 1) == -4 and str(need).encode() in lib.dnmf_last_error()
    assert call(run, names, ok, workspace=a + 4) == -4 and b"aligned" in lib.dnmf_last_error()

    # ---- accum
    ws, run = lib.dnmf_background_accum_workspace, lib.dnmf_background_accum

    def size(P, segs):
        return 256 + (1 + segs) * al(P * 8)

    # one tile of 1024 voxels: up to 2048 segments, of 16 frames or more
    assert ws(P, 37, 0) == size(P, 3)
    assert ws(P, 37, 5) == size(P, 8)
    assert ws(P, 1, 0) == size(P, 1)
    assert ws(P, 10 ** 5, 0) == ws(P, 10 ** 6, 0) == size(P, 2048)
    sizes = [ws(P, B, 0) for B in range(1, 200)]
    assert sizes == sorted(sizes)
    assert ws(P, 0, 0) == 0 and b"B=0" in lib.dnmf_last_error()
    assert ws(P, 4, -1) == 0 and b"segment=-1" in lib.dnmf_last_error()
    assert ws(1 << 31, 4, 0) == 0
    assert ws(P, 10 ** 6, 1) == 0 and b"segments" in lib.dnmf_last_error()
    need = ws(P, 4, 0)
    names = ["frames", "ldf", "sub", "lds", "frame_ids", "f", "P", "B", "first", "finish", "segment", "state", "bytes", "b", "num", "ff",
             "stream"]
    ok = (a, P, None, 0, None, a, P, 4, 1, 1, 0, a, need, a, a, a, None)
    for name in ("frames", "f", "state", "b"):
        assert call(run, names, ok, **{name: None}) == -1 and lib.dnmf_last_error().startswith(b"dnmf_background_accum: "), name
    assert call(run, names, ok, B=0) == -2
    assert call(run, names, ok, segment=-2) == -2 and b"segment=-2" in lib.dnmf_last_error()
    assert call(run, names, ok, ldf=P - 1) == -2
    assert call(run, names, ok, sub=a, lds=P - 1) == -2
    assert call(run, names, ok, P=1 << 31, ldf=1 << 31) == -3
    assert call(run, names, ok, B=10 ** 6, segment=1) == -3
    assert call(run, names, ok, bytes=need - 1) == -4 and str(need).encode() in lib.dnmf_last_error()
    assert call(run, names, ok, state=a + 4) == -4 and b"aligned" in lib.dnmf_last_error()

    # ---- subtract
    run = lib.dnmf_background_subtract
    names = ["frames", "ldf", "frame_ids", "b", "f", "nf", "times", "P", "B", "out", "ldo", "clamp", "stream"]
    out = a + 32
    ok = (a, P, None, a, a, 4, None, P, 4, out, P, 1, None)
    for name in ("frames", "b", "f", "out"):
        assert call(run, names, ok, **{name: None}) == -1 and lib.dnmf_last_error().startswith(b"dnmf_background_subtract: "), name
    assert call(run, names, ok, B=0) == -2
    assert call(run, names, ok, nf=0) == -2
    assert call(run, names, ok, ldf=P - 1) == -2
    assert call(run, names, ok, ldo=P - 1) == -2
    assert call(run, names, ok, B=5) == -2 and b"times" in lib.dnmf_last_error()         # five frames, four values of f
    assert call(run, names, ok, out=a, frame_ids=a) == -2 and b"in place" in lib.dnmf_last_error()
    assert call(run, names, ok, out=a, ldo=P + 4) == -2
    assert call(run, names, ok, P=1 << 31, ldf=1 << 31, ldo=1 << 31) == -3
