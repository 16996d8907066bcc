"""K31 (``ops.running_quantile`` / ``ops.baseline_apply``, csrc/running_baseline.hip) on the GPU against its definition
(tests/dff_restatement.py), and the surfaces built on it.

K31a: ``lo`` and ``hi`` are input samples and ``n`` a count -- numeric equality, the NaN pattern identical; ``value`` is the
wrapper's float64 interpolation, written as the definition writes it: within 1 ulp of float64.  K31b: a handful of float64
operations and one rounding to fp32, against the definition's float64 value rounded to fp32: within 1 ulp of fp32, the NaN
pattern identical."""
import functools

import numpy as np
import pytest
import torch

import dff_restatement as DF
import robust_restatement as RR

pytestmark = pytest.mark.gpu

QS = [0.0, 0.08, 0.5, 1.0]
SHAPES = [(7, 5, 1), (9, 7, 2), (33, 20, 2)]      # 35 voxels: less than a tile; 126; 1320: twenty tiles and a part of one
SMALL = [(1, 1, 1), (5, 8, 2), (64, 64, 64), (65, 64, 1), (300, 64, 16), (301, 65, 33)]
LARGE = [(1100, 513, 128), (4100, 2048, 512)]     # the 32-voxel tile; the 16-voxel tile at the limit


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


@functools.lru_cache(maxsize=None)
def video(sz, T):
    """(T, P) fp32 rows: scales 1e-3 .. 1e3 with ties, both zeros, NaN and +-inf in some frames; voxels 0 .. 8 the edge cases."""
    P = int(np.prod(sz))
    rng = np.random.RandomState(T % 1000 + P)
    x = (rng.randn(T, P) * 10.0 ** rng.randint(-3, 4, (1, P))).astype(np.float32)
    x[rng.rand(T, P) < 0.1] = 0.0
    x[rng.rand(T, P) < 0.05] = -0.0
    x[rng.rand(T, P) < 0.06] = np.nan
    x[rng.rand(T, P) < 0.02] = np.inf
    x[rng.rand(T, P) < 0.02] = -np.inf
    x[:, 0] = 2.5                                                               # all samples equal
    x[:, 1] = rng.randint(0, 2, T) * 3.0 - 1.0                                  # two values only, heavy ties
    x[:, 2] = rng.randint(-2, 3, T) * np.where(rng.rand(T) < 0.5, 1.0, -1.0)    # negative, zero, positive, both zeros
    x[:, 3] = (rng.randint(-9, 10, T) * 1e-42).astype(np.float32)               # denormals
    x[:, 4] = np.nan                                                            # no finite sample
    x[:, 5] = np.where(np.arange(T) % 3 == 0, np.nan, x[:, 5])                  # NaN in a third of the frames
    x[:, 6] = np.where(np.arange(T) % 2 == 0, np.inf, -np.inf)                  # nothing but infinities
    x[:, 7] = RR.from_key32((np.uint32(0xbf800000) + rng.randint(0, 16, T).astype(np.uint32)))     # the lowest key bits only
    x[0, 8] = 4.0
    x[1:, 8] = np.nan                                                           # one sample
    x[:, 9] = 5.0 + np.abs(x[:, 9])                                             # positive: a baseline dF/F can divide by
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(sz, T, W, S, q, min_samples=1):
    """The restatement: computed once, never changed."""
    ref = DF.running_quantile(video(sz, T), W, S, q, min_samples)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def host(result, sz):
    P = int(np.prod(sz))
    assert result["lo"].dtype == torch.float32 and result["hi"].dtype == torch.float32 and result["n"].dtype == torch.int32
    assert result["value"].dtype == torch.float64 and result["lo"].shape[1:] == tuple(sz) == result["n"].shape[1:]
    return {k: result[k].cpu().numpy().reshape(-1, P) for k in ("lo", "hi", "n", "value")}


def compare(got, want, what):
    np.testing.assert_array_equal(got["n"], want["n"], err_msg=f"{what}: n")
    for k in ("lo", "hi"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")      # numeric equality, NaN where NaN
    g, w = got["value"], want["value"]
    np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f"{what}: NaN pattern of value")
    ok = ~np.isnan(w)
    worst = (np.abs(g[ok] - w[ok]) / np.spacing(np.abs(w[ok]))).max() if ok.any() else 0.0
    print(f"{what}: value worst {worst:.2f} ulp")
    assert worst <= 1.0, what


def same_bits(a, b, what):
    for k in ("lo", "hi", "n", "value"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: {k}"


@pytest.mark.parametrize("sz", SHAPES)
@pytest.mark.parametrize("TWS", SMALL)
def test_knots_small(ops, sz, TWS):
    T, W, S = TWS
    rows = dev(video(sz, T))
    for q in QS:
        r = ops.running_quantile(rows, sz, W, S, q)
        want = reference(sz, T, W, S, q)
        assert r["windows"] == (0, len(want["centres"]))
        np.testing.assert_array_equal(r["centres"], want["centres"])
        compare(host(r, sz), want, f"{sz} {TWS} q={q}")


@pytest.mark.parametrize("sz,TWS", [(SHAPES[0], LARGE[0]), (SHAPES[1], LARGE[0]), (SHAPES[2], LARGE[0]), (SHAPES[0], LARGE[1])])
def test_knots_large(ops, sz, TWS):
    T, W, S = TWS
    r = ops.running_quantile(dev(video(sz, T)), sz, W, S, 0.08)
    compare(host(r, sz), reference(sz, T, W, S, 0.08), f"{sz} {TWS} q=0.08")


def test_run_lengths_and_a_second_run(ops):
    for sz, (T, W, S) in ((SHAPES[2], SMALL[4]), (SHAPES[1], SMALL[3]), (SHAPES[0], LARGE[0])):
        rows = dev(video(sz, T))
        a = ops.running_quantile(rows, sz, W, S, 0.08, run=1)
        compare(host(a, sz), reference(sz, T, W, S, 0.08), f"{sz} T={T} run=1")
        for run in (3, 0, 0):
            same_bits(a, ops.running_quantile(rows, sz, W, S, 0.08, run=run), f"{sz} T={T} run={run} against run=1")


def test_min_samples_padded_rows_and_frame_ids(ops):
    sz, (T, W, S) = SHAPES[1], SMALL[4]
    P = int(np.prod(sz))
    x = video(sz, T)
    r = ops.running_quantile(dev(x), sz, W, S, 0.5, min_samples=50)
    want = reference(sz, T, W, S, 0.5, 50)
    compare(host(r, sz), want, "min_samples=50")
    assert np.isnan(want["value"][:, 5]).all() and not np.isnan(want["value"][:, 0]).any()      # 64 - 22 < 50 <= 64
    padded = torch.full((T, P + 13), 777.0, device="cuda")
    padded[:, :P] = dev(x)
    before = padded.clone()
    compare(host(ops.running_quantile(padded[:, :P], sz, W, S, 0.08), sz), reference(sz, T, W, S, 0.08), "ld = P + 13")
    perm = np.random.RandomState(1).permutation(T)
    got = ops.running_quantile(padded[:, :P], sz, W, S, 0.08, frame_ids=perm.tolist())
    compare(host(got, sz), DF.running_quantile(x, W, S, 0.08, frame_ids=perm), "permuted frame_ids")
    some = perm[:100]
    got = ops.running_quantile(padded[:, :P], sz, W, S, 0.08, frame_ids=torch.from_numpy(some))
    compare(host(got, sz), DF.running_quantile(x, W, S, 0.08, frame_ids=some), "100 of 300 rows")
    assert torch.equal(padded.view(torch.int32), before.view(torch.int32))
    with pytest.raises(ValueError, match="frame_ids"):
        ops.running_quantile(padded[:, :P], sz, W, S, frame_ids=[0, T])
    with pytest.raises(ValueError, match="window=2049"):
        ops.running_quantile(padded[:, :P], sz, 2049)
    with pytest.raises(ValueError, match="rows 290"):
        ops.running_quantile(padded[:, :P], sz, W, S, row0=290, T=500)


def ulps32(got, want):
    """|got - want| in ulp of fp32 at want, 0 where the two are equal (infinities included)."""
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    return np.where(got == want, 0.0, err)


def check_applied(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    got, want = got.reshape(want.shape), np.asarray(want)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{what}: NaN pattern")
    ok = ~np.isnan(want)
    worst = ulps32(got[ok], want[ok]).max() if ok.any() else 0.0
    print(f"{what}: worst {worst:.2f} ulp of fp32")
    assert worst <= 1.0, what


@pytest.mark.parametrize("sz,TWS", [(SHAPES[0], SMALL[1]), (SHAPES[1], SMALL[3]), (SHAPES[2], SMALL[4]), (SHAPES[1], SMALL[5]),
                                    (SHAPES[0], SMALL[0])])
def test_apply_modes(ops, sz, TWS):
    T, W, S = TWS
    x = video(sz, T)
    rows = dev(x)
    want_knots = reference(sz, T, W, S, 0.08)
    knots = ops.running_quantile(rows, sz, W, S, 0.08)
    # against the definition's own knots, so that the comparison is of K31b alone
    value = dev(want_knots["value"], torch.float64).reshape(-1, *sz)
    for mode, offset in (("baseline", 0.0), ("df", 0.0), ("dff", 0.0), ("dfsqrtf", 0.0), ("dff", 2.5), ("dfsqrtf", 0.75)):
        want, _ = DF.apply(x, want_knots["value"], want_knots["centres"], mode, offset)
        got = ops.baseline_apply(rows, sz, value, want_knots["centres"], mode, offset)
        assert got.shape == (T, int(np.prod(sz))) and got.dtype == torch.float32
        check_applied(got, want, f"{sz} {TWS} {mode} offset={offset}")
        if mode in ("dff", "dfsqrtf") and T > 1:
            _, f0 = DF.apply(x, want_knots["value"], want_knots["centres"], "baseline")
            refused = np.isfinite(f0) & (f0 + offset <= 0)
            assert refused.any() and np.isnan(want[refused]).all()                 # the F0 + offset <= 0 case is in the data
        chained = ops.baseline_apply(rows, sz, knots["value"], knots["centres"], mode, offset)      # K31a's knots: within 1 ulp
        check_applied(chained, want, f"{sz} {TWS} {mode} offset={offset}, the kernel's knots")


def test_apply_frame_ids_out_and_refusals(ops):
    sz, (T, W, S) = SHAPES[1], SMALL[4]
    P = int(np.prod(sz))
    x = video(sz, T)
    rows = dev(x)
    knots = reference(sz, T, W, S, 0.08)
    value = dev(knots["value"], torch.float64).reshape(-1, *sz)
    perm = np.random.RandomState(2).permutation(T)[:77]
    want, _ = DF.apply(x, knots["value"], knots["centres"], "dff", 1.0, frame_ids=perm, row0=40)
    got = ops.baseline_apply(rows, sz, value, knots["centres"], "dff", 1.0, frame_ids=perm.tolist(), row0=40)
    assert got.shape == (77, P)
    check_applied(got, want, "frame_ids, row0=40")
    out = torch.full((T + 2, P + 5), 777.0, device="cuda")
    ret = ops.baseline_apply(rows, sz, value, knots["centres"], "df", out=out[1:, :P])
    assert ret.data_ptr() == out[1:].data_ptr() and ret.shape == (T, P)
    check_applied(out[1:T + 1, :P].contiguous(), DF.apply(x, knots["value"], knots["centres"], "df")[0], "out=")
    assert bool((out[0] == 777.0).all()) and bool((out[T + 1] == 777.0).all()) and bool((out[:, P:] == 777.0).all())
    with pytest.raises(ValueError, match="share memory"):
        ops.baseline_apply(rows, sz, value, knots["centres"], out=rows)
    with pytest.raises(ValueError, match="share memory"):
        ops.baseline_apply(out[:T, :P], sz, value, knots["centres"], out=out[2:, :P])
    with pytest.raises(ValueError, match="strictly increasing"):
        ops.baseline_apply(rows, sz, value, knots["centres"][::-1].copy())
    with pytest.raises(ValueError, match="float64"):
        ops.baseline_apply(rows, sz, value.float(), knots["centres"])


def test_pieces_give_the_same_bits(ops):
    """The (300, 64, 16) movie cut at rows that are no window starts, with the overlap the plan demands."""
    sz, (T, W, S) = SHAPES[1], SMALL[4]
    rows = dev(video(sz, T))
    whole = ops.running_quantile(rows, sz, W, S, 0.08)
    J = whole["windows"][1]
    assert whole["windows"] == (0, 16)
    lo = torch.full_like(whole["lo"], float("nan"))
    hi, n, value = lo.clone(), torch.zeros_like(whole["n"]), torch.full_like(whole["value"], float("nan"))
    seen = []
    # no cut is a window start (a multiple of 16, or 236): a piece starts at or before the first window the one before it left
    # out, W - S = 48 rows before the last window end it held, and a few more rows here
    for r0, r1 in ((0, 101), (45, 203), (141, 300)):
        r = ops.running_quantile(rows[r0:r1], sz, W, S, 0.08, row0=r0, T=T)
        j0, j1 = r["windows"]
        inside = [j for j in range(J) if whole["starts"][j] >= r0 and whole["ends"][j] <= r1]
        assert (j0, j1) == (inside[0], inside[-1] + 1)
        for full, piece in ((lo, r["lo"]), (hi, r["hi"]), (n, r["n"]), (value, r["value"])):
            full[j0:j1] = piece[j0:j1]
        outside = torch.ones(J, dtype=torch.bool)
        outside[j0:j1] = False
        assert bool(torch.isnan(r["lo"][outside]).all()) and bool((r["n"][outside] == 0).all())
        seen.extend(range(j0, j1))
    assert sorted(set(seen)) == list(range(J))
    same_bits(dict(lo=lo, hi=hi, n=n, value=value), whole, "assembled from three pieces")
    applied = ops.baseline_apply(rows, sz, whole["value"], whole["centres"], "dff", 1.0)
    parts = torch.cat([ops.baseline_apply(rows[a:b], sz, value, whole["centres"], "dff", 1.0, row0=a) for a, b in ((0, 33), (33, 34), (34, 300))])
    assert torch.equal(applied.view(torch.int32), parts.view(torch.int32))
    movie, info = ops.dff_rows(lambda a, b: rows[a:b], T, sz, W, S, 0.08, "dff", 1.0, limit=100)
    assert len(ops._running_pieces(T, 126, W, S, 100)[1]) > 3
    assert torch.equal(movie.view(torch.int32), applied.view(torch.int32))
    assert torch.equal(info["knots"].view(torch.int32), whole["value"].view(torch.int32)) and torch.equal(info["n"], whole["n"])


def test_class_surfaces(ops):
    from dnmf_amd.Demix.dNMF import ExponentialFP
    from dnmf_amd.Demix.MotionCorrect import MotionCorrect
    sz, (T, W, S) = SHAPES[1], SMALL[4]
    x = video(sz, T)
    vid = x.reshape(T, *sz)
    want, knots = DF.dff_movie(x, W, S, 0.08, "dff", 1.0)
    movie, info = ExponentialFP.dff_movie(vid, W, S, mode="dff", offset=1.0)
    assert isinstance(movie, np.ndarray) and movie.shape == (T, *sz) and movie.dtype == np.float32
    check_applied(movie, want.reshape(T, *sz), "ExponentialFP.dff_movie numpy in")
    assert set(info) == {"knots", "centres", "n", "starts", "ends"} and isinstance(info["knots"], np.ndarray)
    np.testing.assert_array_equal(info["n"].reshape(-1, x.shape[1]), knots["n"])
    cuda, cinfo = ExponentialFP.dff_movie(torch.from_numpy(vid).cuda(), W, S, mode="dff", offset=1.0)
    assert torch.is_tensor(cuda) and cuda.is_cuda and cuda.shape == (T, x.shape[1]) and cinfo["knots"].is_cuda
    np.testing.assert_array_equal(cuda.cpu().numpy().reshape(T, *sz), movie)
    with pytest.raises(ValueError, match="percentile"):
        ExponentialFP.dff_movie(vid, W, percentile=101)
    mc = MotionCorrect(vid, max_shifts=(2, 2, 1), strides=(6, 4, 1), overlaps=(2, 2, 1), max_deviation_rigid=1, is3D=True, pw_rigid=True)
    got, _ = mc.dff_movie(vid, window=W, stride=S, mode="dff", offset=1.0)
    np.testing.assert_array_equal(got, movie)
    with pytest.raises(ValueError, match="save_corrected"):
        mc.dff_movie(window=W)
    mc.mc = [np.ascontiguousarray(np.moveaxis(vid[:120], 0, 3)), np.ascontiguousarray(np.moveaxis(vid[120:], 0, 3))]
    stored, sinfo = mc.dff_movie(window=W, stride=S, mode="dff", offset=1.0)
    np.testing.assert_array_equal(stored, movie)
    np.testing.assert_array_equal(sinfo["knots"], info["knots"])


def test_deformable_nmf_surfaces(ops):
    from dnmf_amd.Demix import dNMF as M
    from dnmf_amd.Demix.Traces import detrend_df_f
    rng = np.random.RandomState(3)
    sz, K, T = [20, 16, 2], 3, 40
    P = int(np.prod(sz))
    pos = (np.array([4, 4, 0]) + rng.rand(K, 3) * np.array([12, 8, 1])).astype(np.float32)
    dn = M.DeformableNMF(torch.tensor(sz), K, T, positions=torch.from_numpy(pos))
    dn.verbose = False
    frames = torch.from_numpy(1.0 + rng.rand(T, P)).to("cuda", torch.float32)
    loader = M.ResidentLoader(frames, sz, 4)
    movie = dn.dff_movie(loader, window=16, stride=4)
    knots = ops.running_quantile(frames, sz, 16, 4, 0.08)
    want = ops.baseline_apply(frames, sz, knots["value"], knots["centres"], "dff")
    assert torch.equal(movie.view(torch.int32), want.view(torch.int32))
    assert torch.equal(dn.last_dff["knots"].view(torch.int32), knots["value"].view(torch.int32))
    check_applied(movie, DF.dff_movie(frames.cpu().numpy(), 16, 4, 0.08)[0], "DeformableNMF.dff_movie")
    # at the identity warp K17 returns the input: registered = unregistered, bit for bit
    reg = dn.dff_movie(loader, registered='linear', window=16, stride=4)
    assert torch.equal(reg.view(torch.int32), movie.view(torch.int32))
    with pytest.raises(ValueError, match="registered"):
        dn.dff_movie(loader, registered='cubic', window=16)
    # traces: (K, T) with NaNs, row by row against the definition
    C = (5.0 + rng.rand(K, T) * np.array([[1.0], [10.0], [100.0]])).astype(np.float32)
    C[1, 7] = np.nan
    C[2, ::3] = np.nan
    for mode, offset in (("df", 0.0), ("dff", 0.5)):
        out, base = detrend_df_f(C, 9, 1, percentile=20.0, mode=mode, offset=offset)
        assert isinstance(out, np.ndarray) and out.shape == (K, T) == base.shape and out.dtype == np.float32
        for k in range(K):
            w_out, kn = DF.dff_movie(C[k][:, None], 9, 1, 0.2, mode, offset)
            check_applied(out[k], w_out[:, 0], f"detrend_df_f {mode} row {k}")
            check_applied(base[k], DF.apply(C[k][:, None], kn["value"], kn["centres"], "baseline")[0][:, 0], f"baseline row {k}")
    one, base1 = detrend_df_f(torch.from_numpy(C[0]).cuda(), 9, 1, percentile=20.0)
    assert one.is_cuda and one.shape == (T,) and base1.shape == (T,)
    np.testing.assert_array_equal(one.cpu().numpy(), detrend_df_f(C, 9, 1, percentile=20.0)[0][0])
    dn.C = torch.from_numpy(C.astype(np.float64))
    before = dn.C.clone()
    got = dn.detrend_traces(9, stride=1, percentile=20.0)
    assert torch.equal(dn.C.view(torch.int64), before.view(torch.int64))
    np.testing.assert_array_equal(got.cpu().numpy(), detrend_df_f(C, 9, 1, percentile=20.0)[0])
    np.testing.assert_array_equal(dn.last_detrend["baseline"].cpu().numpy(), detrend_df_f(C, 9, 1, percentile=20.0)[1])
    given = dn.detrend_traces(9, traces=C[:2], stride=1, percentile=20.0, mode="dff")
    np.testing.assert_array_equal(given.cpu().numpy(), detrend_df_f(C[:2], 9, 1, percentile=20.0, mode="dff")[0])
    # the refusals of _single_model_only: what MultiChannelDNMF meets
    nchan = dn._nchan
    dn._nchan = lambda: 2
    with pytest.raises(NotImplementedError, match="one channel"):
        dn.dff_movie(loader, window=16)
    with pytest.raises(NotImplementedError, match="one channel"):
        dn.detrend_traces(9)
    dn._nchan = nchan
    assert issubclass(M.MultiChannelDNMF, M.DeformableNMF) and M.MultiChannelDNMF.dff_movie is M.DeformableNMF.dff_movie
    loader.T_total = 2 * loader.T
    with pytest.raises(NotImplementedError, match="shard"):
        dn.dff_movie(loader, window=16)


def picks_are_the_cells(pts, cells):
    dist = np.linalg.norm(np.asarray(pts)[None] - cells[:, None], axis=2)
    return len(pts) == 2 and np.isfinite(pts).all() and dist.min(1).max() <= 1.5 and sorted(dist.argmin(1)) == [0, 1]


@pytest.mark.parametrize("Z", [1, 2])
def test_dff_finds_the_firing_cells_of_a_bleaching_video(ops, Z):
    from dnmf_amd.Demix.dNMF import ExponentialFP
    video4, cells, still, sigma = DF.bleaching_case(DF.BLEACH_SEEDS[Z], Z)
    T, sz = video4.shape[0], video4.shape[1:]
    movie, _ = ExponentialFP.dff_movie(video4, DF.BLEACH_WINDOW, DF.BLEACH_STRIDE)
    check_applied(movie, DF.dff_movie(video4.reshape(T, -1), DF.BLEACH_WINDOW, DF.BLEACH_STRIDE, 0.08)[0].reshape(T, *sz), f"Z={Z} dF/F movie")
    dff_max = ExponentialFP.summary_images(movie)["max"]
    pos, _ = ExponentialFP.detect_positions(RR.nan_to_min(dff_max), 2, shape_std=sigma)
    print(f"Z={Z} detect_positions on the max of dF/F:", pos.tolist())
    assert picks_are_the_cells(pos, cells)
    raw_max = ExponentialFP.robust_images(video4)["max"]
    first, _ = ExponentialFP.detect_positions(RR.nan_to_min(raw_max), 1, shape_std=sigma)
    assert np.linalg.norm(first[0] - still) <= 1.5          # the raw movie: the bright static blob
