"""K30 (``ops.temporal_quantiles``, csrc/robust_images.hip) on the GPU against its definition (tests/robust_restatement.py).

No tolerance on the kernel's outputs: ``lo`` and ``hi`` are input samples and ``n`` is a count, compared for numeric equality
(-0 and +0 are one value), the NaN pattern identical.  ``value`` is the wrapper's float64 interpolation, one subtraction, one
product and one sum, written as the definition writes it: compared within 1 ulp of float64."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import robust_restatement as RR

pytestmark = pytest.mark.gpu

QS = [0.0, 0.08, 0.5, 1.0]
SOURCES = ["value", "absdev", "absdiff"]
SHAPES = [(7, 5, 1), (9, 7, 2), (33, 20, 2)]      # 35 voxels: less than a tile; 126; 1320: five tiles and a part of one
FRAMES = [1, 2, 3, 255, 256, 257, 70000]          # 70000: past any 16-bit counter, and more than one segment of frames


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
    """(T, P) fp32 rows.  Voxels 0 .. 11 carry the edge cases, the others a seeded mix of scales with ties, both zeros, NaN and
    +-inf in some frames (so n differs from voxel to voxel inside one tile)."""
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
    x[:, 7] = RR.from_key32((np.uint32(0xbf800000) + rng.randint(0, 16, T).astype(np.uint32)))     # the lowest key digit only
    x[:, 8] = RR.from_key32((rng.randint(0, 16, T).astype(np.uint32) << np.uint32(28)) | np.uint32(0x0812345))   # the highest only
    x[:, 9] = np.arange(T, dtype=np.float32)[::-1]                              # distinct, descending
    x[0, 10] = 4.0
    x[1:, 10] = np.nan                                                          # one sample
    x[:, 11] = -np.abs(x[:, 11])                                                # negative only
    assert np.isfinite(x[:, 7]).all() and np.isfinite(x[:, 8]).all()
    x.setflags(write=False)
    return x


def centre_of(sz, T):
    """The fp32 median image 'absdev' is used with (0 where a voxel has no finite sample)."""
    med = RR.temporal_quantiles(video(sz, T), [0.5])["value"][0]
    return np.nan_to_num(med, nan=0.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(sz, T, source, qs=tuple(QS)):
    """The restatement: computed once, never changed."""
    ref = RR.temporal_quantiles(video(sz, T), list(qs), source, centre_of(sz, T) if source == "absdev" else None)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def host(result, sz):
    P = int(np.prod(sz))
    out = {k: result[k].cpu().numpy() for k in ("lo", "hi", "n", "value")}
    assert result["lo"].dtype == torch.float32 and result["hi"].dtype == torch.float32 and result["n"].dtype == torch.int32
    assert result["value"].dtype == torch.float64 and result["n"].shape == tuple(sz) and result["lo"].shape[1:] == tuple(sz)
    return {k: v.reshape(-1, P) if k != "n" else v.reshape(P) for k, v in out.items()}


def compare(got, want, what):
    np.testing.assert_array_equal(got["n"], want["n"], err_msg=f"{what}: n")
    for k in ("lo", "hi"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")      # numeric equality, NaN where NaN
    g, w = got["value"], want["value"]
    np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f"{what}: NaN pattern of value")
    ok = ~np.isnan(w)
    ulps = np.abs(g[ok] - w[ok]) / np.spacing(np.abs(w[ok]))
    worst = ulps.max() if ok.any() else 0.0
    print(f"{what}: value worst {worst:.2f} ulp")
    assert worst <= 1.0, what


def run(ops, sz, T, source, qs=QS, **kw):
    c = dev(centre_of(sz, T)) if source == "absdev" else None
    result, state = ops.temporal_quantiles(dev(video(sz, T)), sz, qs, source, c, **kw)
    return result


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("sz", SHAPES)
def test_volumes_and_sources(ops, sz, source):
    compare(host(run(ops, sz, 37, source), sz), reference(sz, 37, source), f"{sz} T=37 {source}")


@pytest.mark.parametrize("source", ["value", "absdiff"])
@pytest.mark.parametrize("T", FRAMES)
def test_frame_counts(ops, T, source):
    sz = SHAPES[0]
    got = host(run(ops, sz, T, source), sz)
    compare(got, reference(sz, T, source), f"{sz} T={T} {source}")
    if source == "absdiff" and T == 1:
        assert (got["n"] == 0).all() and np.isnan(got["lo"]).all()


@pytest.mark.parametrize("T", [36, 37])
def test_the_median_alone_at_even_and_odd_counts(ops, T):
    sz = SHAPES[1]
    got = host(run(ops, sz, T, "value", [0.5]), sz)
    want = reference(sz, T, "value", (0.5,))
    compare(got, want, f"{sz} T={T} q=0.5")
    assert got["n"][9] == T and (got["lo"][0, 9] == got["hi"][0, 9]) == (T == 1)      # voxel 9: distinct samples
    assert got["value"][0, 9] == (T - 1) / 2.0


def test_edge_values_by_voxel(ops):
    """The edge-case voxels one by one (they are part of every comparison above as well)."""
    sz, T = SHAPES[0], 257
    got = host(run(ops, sz, T, "value"), sz)
    x = video(sz, T)
    assert (got["lo"][:, 0] == 2.5).all() and (got["hi"][:, 0] == 2.5).all() and got["n"][0] == T
    assert set(got["lo"][:, 1]) <= {-1.0, 2.0} and got["lo"][0, 1] == -1.0 and got["hi"][3, 1] == 2.0
    assert got["n"][4] == 0 and np.isnan(got["lo"][:, 4]).all() and np.isnan(got["value"][:, 4]).all()
    assert got["n"][6] == 0 and got["n"][10] == 1 and (got["lo"][:, 10] == x[0, 10]).all()
    assert got["n"][5] == np.isfinite(x[:, 5]).sum() <= T - (T + 2) // 3
    for v in (3, 7, 8):
        np.testing.assert_array_equal(got["lo"][[0, 3], v], [x[:, v].min(), x[:, v].max()])
    zero = got["lo"][:, 2][got["lo"][:, 2] == 0]
    assert not np.signbit(zero).any()


def test_forced_segments_and_a_second_run(ops):
    sz = SHAPES[2]
    for source in SOURCES:
        a = run(ops, sz, 37, source, segment=8)
        b = run(ops, sz, 37, source, segment=8)
        c = run(ops, sz, 37, source)
        compare(host(a, sz), reference(sz, 37, source), f"{sz} {source} segment=8")
        for k in ("lo", "hi", "n", "value"):
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{source} {k}: a second run"
            assert torch.equal(a[k].view(torch.int32), c[k].view(torch.int32)), f"{source} {k}: segment=8 against 0"
    compare(host(run(ops, SHAPES[0], 3, "absdiff", segment=1), SHAPES[0]), reference(SHAPES[0], 3, "absdiff"), "T=3 segment=1")


def in_pieces(ops, rows, sz, cuts, source, c, frame_ids=None):
    """The movie fed in pieces cut at ``cuts``, once per pass."""
    T = rows.shape[0] if frame_ids is None else len(frame_ids)
    edges = [0, *cuts, T]
    state = result = None
    for p in range(ops.temporal_quantiles_passes()):
        for i, (s, e) in enumerate(zip(edges[:-1], edges[1:])):
            kw = dict(frame_ids=frame_ids[s:e]) if frame_ids is not None else {}
            piece = rows if frame_ids is not None else rows[s:e]
            result, state = ops.temporal_quantiles(piece, sz, QS, source, c, state=state, first=p == 0 and i == 0,
                                                   finish=i == len(edges) - 2, **kw)
            assert (result is None) == (p < ops.temporal_quantiles_passes() - 1 or i < len(edges) - 2)
    return result


@pytest.mark.parametrize("source", SOURCES)
def test_pieces_give_the_same_bits(ops, source):
    sz, T = SHAPES[1], 37
    rows = dev(video(sz, T))
    c = dev(centre_of(sz, T)) if source == "absdev" else None
    whole, _ = ops.temporal_quantiles(rows, sz, QS, source, c)
    compare(host(whole, sz), reference(sz, T, source), f"{sz} {source} whole")
    for cuts in ([1], [T - 1], [18], [5, 6, 23], [1, 2, 36]):
        got = in_pieces(ops, rows, sz, cuts, source, c)
        for k in ("lo", "hi", "n", "value"):
            assert torch.equal(got[k].view(torch.int32), whole[k].view(torch.int32)), f"{source} cuts {cuts}: {k}"


def test_padded_rows_and_frame_ids(ops):
    sz, T = SHAPES[1], 37
    P = int(np.prod(sz))
    x = video(sz, T)
    padded = torch.full((T, P + 13), 777.0, device="cuda")
    padded[:, :P] = dev(x)
    before = padded.clone()
    perm = np.random.RandomState(1).permutation(T)
    for source in SOURCES:
        c = dev(centre_of(sz, T)) if source == "absdev" else None
        plain, _ = ops.temporal_quantiles(padded[:, :P], sz, QS, source, c)
        assert padded[:, :P].stride(0) == P + 13
        compare(host(plain, sz), reference(sz, T, source), f"{sz} {source} ld = P + 13")
        want = RR.temporal_quantiles(x, QS, source, centre_of(sz, T) if source == "absdev" else None, frame_ids=perm)
        shuffled, _ = ops.temporal_quantiles(padded[:, :P], sz, QS, source, c, frame_ids=perm.tolist())
        compare(host(shuffled, sz), want, f"{sz} {source} permuted frame_ids")
        cut = in_pieces(ops, padded[:, :P], sz, [4, 20], source, c, frame_ids=perm.tolist())
        for k in ("lo", "hi", "n"):
            assert torch.equal(cut[k].view(torch.int32), shuffled[k].view(torch.int32)), f"{source} permuted, in pieces: {k}"
    assert torch.equal(padded.view(torch.int32), before.view(torch.int32))      # the rows and their padding: untouched
    some = perm[:11]
    got, _ = ops.temporal_quantiles(padded[:, :P], sz, QS, "absdiff", frame_ids=torch.from_numpy(some))
    compare(host(got, sz), RR.temporal_quantiles(x, QS, "absdiff", frame_ids=some), f"{sz} 11 of 37 rows")


def test_refusals(ops):
    sz, T = SHAPES[0], 37
    rows = dev(video(sz, T))
    with pytest.raises(ValueError, match="centre"):
        ops.temporal_quantiles(rows, sz, [0.5], "absdev")
    for q in ([-0.1], [1.5], [0.5, float("nan")]):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            ops.temporal_quantiles(rows, sz, q)
    with pytest.raises(ValueError, match="quantiles"):
        ops.temporal_quantiles(rows, sz, [0.1, 0.2, 0.3, 0.4, 0.5])
    with pytest.raises(ValueError, match="quantiles"):
        ops.temporal_quantiles(rows, sz, [])
    with pytest.raises(ValueError, match="float32"):
        ops.temporal_quantiles(rows.double(), sz, [0.5])
    with pytest.raises(ValueError, match="source"):
        ops.temporal_quantiles(rows, sz, [0.5], "square")
    with pytest.raises(ValueError, match="first=False"):
        ops.temporal_quantiles(rows, sz, [0.5], first=False)
    with pytest.raises(ValueError, match="frame_ids"):
        ops.temporal_quantiles(rows, sz, [0.5], frame_ids=[0, T])
    # a later pass that brings more rows, or fewer, than pass 0
    _, state = ops.temporal_quantiles(rows[:20], sz, [0.5], finish=False)
    _, state = ops.temporal_quantiles(rows[20:], sz, [0.5], state=state, first=False)
    assert state.pass_index == 1 and state.rows_per_pass == T
    with pytest.raises(ValueError, match="same rows"):
        ops.temporal_quantiles(rows[:36], sz, [0.5], state=state, first=False)
    _, state = ops.temporal_quantiles(rows[:30], sz, [0.5], state=state, first=False, finish=False)
    with pytest.raises(ValueError, match="same rows"):
        ops.temporal_quantiles(rows[:8], sz, [0.5], state=state, first=False, finish=False)
    with pytest.raises(ValueError, match="started with"):
        ops.temporal_quantiles(rows[30:], sz, [0.25], state=state, first=False)
    # the library's own limits
    from dnmf_amd import _lib
    lib = _lib.load()
    three, q, buf = (ctypes.c_int * 3)(*sz), (ctypes.c_double * 1)(0.5), state.buffer
    args = (rows.data_ptr(), rows.stride(0), None, three, T, 0, None, q, 1, 0)
    assert lib.dnmf_temporal_select_pass(*args, 2 ** 31 - T, 0, buf.data_ptr(), buf.numel() * 4, None) != 0
    assert b"32-bit counters" in lib.dnmf_last_error()
    assert lib.dnmf_temporal_select_pass(*args, 0, 0, buf.data_ptr(), 16, None) != 0
    assert lib.dnmf_temporal_select_workspace(three, 5) == 0 and lib.dnmf_temporal_select_workspace(three, 0) == 0
    assert ops.temporal_quantiles_passes() == 9


def test_state_size(ops):
    """(8 + 76 Q) bytes a voxel and the 256-byte granules of its seven arrays: 80 MiB for 512 x 512 x 2 and two quantiles."""
    from dnmf_amd import _lib
    need = _lib.load().dnmf_temporal_select_workspace((ctypes.c_int * 3)(512, 512, 2), 2)
    assert need == 512 * 512 * 2 * (8 + 76 * 2) == 80 << 20
