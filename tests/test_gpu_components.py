"""Component statistics (K24, ``dnmf_component_stats``) on the GPU against the float64 definition
(tests/components_restatement.py) applied to the same fp32 inputs.

Tolerances.  The three per-frame sums, ``foot`` and the image sums: within 1e-12 of the sum of the magnitudes of their terms,
the bound the K19 / K23 tests put on the same kind of float64 sum (the terms themselves are formed exactly alike; only the
order of the additions differs).  The NaN patterns are identical.  ``frame_corr``, ``raw`` and ``r_values`` are quotients of
differences of those sums, n sum xy - sum x sum y, whose rounding grows with the cancellation, so their bound is measured:
the largest deviation from the restatement over every case of this file is MEASURED below, and PEARSON_TOL, ten times
that, is asserted.  The restatement asserts the input condition the figure depends on: on every box the variance of a, of
every e_t and of the image is exactly zero or at least 1e-6 of the mean square."""
import functools

import numpy as np
import pytest
import torch

import components_restatement as CR

pytestmark = pytest.mark.gpu

MEASURED = 1.03e-14      # largest |kernel - restatement| of frame_corr, raw (relative to 1 + |raw|) and r_values, all cases
PEARSON_TOL = 10 * MEASURED
SUM_TOL = 1e-12

SHAPES = [(20, 17, 1), (9, 7, 3), (33, 5, 2)]
FRAMES = [1, 2, 37]
SEGMENTS = [1, 5, 0]
K = 5
DEVIATIONS = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def boxes_of(sz):
    """One box cut by two borders, one covering the whole volume, one of a single voxel, two inside."""
    X, Y, Z = sz
    return np.array([[0, 3, Y - 3, Y - 1, 0, Z - 1],
                     [0, X - 1, 0, Y - 1, 0, Z - 1],
                     [X // 2, X // 2, Y // 2, Y // 2, Z - 1, Z - 1],
                     [1, X - 2, 1, 3, 0, 0],
                     [2, 6, 0, Y - 2, 0, Z - 1]], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def problem(sz, B, with_sub):
    """fp32 inputs and the restatement's answer -- made once, never changed.  The rows of ``frames`` are longer than a frame and
    are taken through a permutation; neuron 3 has zero weights; with B >= 2 one sample of frame 1 inside box 4 is NaN."""
    rng = np.random.RandomState(sz[0] + 7 * B)
    P = sz[0] * sz[1] * sz[2]
    ld = P + 5
    rows = B + 2
    store = (0.5 + rng.rand(rows, ld)).astype(np.float32)
    perm = rng.permutation(rows)[:B].astype(np.int32)
    sub = (0.4 * rng.rand(B, ld)).astype(np.float32) if with_sub else None
    A_rows = rng.rand(K, P).astype(np.float32)
    C = rng.rand(K, B).astype(np.float32)
    w = (rng.rand(K, B) < 0.6).astype(np.float32) * rng.randint(1, 3, (K, B)).astype(np.float32)
    w[0, 0] = 1.0
    w[3] = 0.0
    boxes = boxes_of(sz)
    if B >= 2:
        store[perm[1], CR.box_voxels(boxes[4], sz)[3]] = np.nan
    ref = CR.component_stats(store[perm][:, :P], sz, A_rows, boxes, C, w, sub=None if sub is None else sub[:, :P])
    for a in (store, perm, A_rows, C, w, boxes):
        a.setflags(write=False)
    return store, perm, sub, A_rows, C, w, boxes, ref


def run(ops, sz, prob, segment=0, **kw):
    store, perm, sub, A_rows, C, w, boxes, _ = prob
    return ops.component_stats(dev(store), sz, dev(A_rows), torch.from_numpy(boxes), dev(C), dev(w), sub=None if sub is None else dev(sub),
                               frame_ids=dev(perm, torch.int32), segment=segment, **kw)


def compare(out, ref, tag):
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for name in ("sums", "foot", "frame_corr", "raw", "image", "r_values"):
        assert got[name].shape == ref[name].shape, name
        assert (np.isnan(got[name]) == np.isnan(ref[name])).all(), f"{tag}: NaN pattern of {name}"
    ok = ~np.isnan(ref["sums"])
    err = np.abs(got["sums"] - ref["sums"])[ok] / ref["sums_mag"][ok]
    assert err.size == 0 or err.max() <= SUM_TOL, (tag, "sums", err.max())
    assert (np.abs(got["foot"] - ref["foot"]) <= SUM_TOL * ref["foot_mag"]).all(), (tag, "foot")
    ok = ~np.isnan(ref["image"])
    scale = (ref["image_sums_mag"] / np.where(ref["wsum"] > 0, ref["wsum"], 1.0)[:, None])[ok]
    assert (np.abs(got["image"] - ref["image"])[ok] <= SUM_TOL * scale).all(), (tag, "image")
    worst = 0.0
    for name in ("frame_corr", "raw", "r_values"):
        ok = ~np.isnan(ref[name])
        if ok.any():
            worst = max(worst, float((np.abs(got[name] - ref[name])[ok] / (1.0 + np.abs(ref[name][ok]))).max()))
    DEVIATIONS[tag] = worst
    print(f"{tag}: largest deviation of frame_corr / raw / r_values {worst:.3e} (all cases so far {max(DEVIATIONS.values()):.3e})")
    assert worst <= PEARSON_TOL, (tag, worst)


@pytest.mark.parametrize("with_sub", [True, False])
@pytest.mark.parametrize("segment", SEGMENTS)
@pytest.mark.parametrize("B", FRAMES)
@pytest.mark.parametrize("sz", SHAPES)
def test_against_the_restatement(ops, sz, B, segment, with_sub):
    prob = problem(sz, B, with_sub)
    out, state = run(ops, sz, prob, segment=segment)
    assert all(v.dtype == torch.float64 and v.is_cuda for v in out.values())
    compare(out, prob[-1], f"{sz} B={B} segment={segment} sub={with_sub}")
    ref = prob[-1]
    assert np.isnan(ref["r_values"][3]) and np.isnan(ref["r_values"][2])          # zero weights; one voxel
    if B >= 2:
        assert np.isnan(ref["sums"][4, 1]).all() and np.isnan(ref["sums"][1, 1]).all() and np.isfinite(ref["sums"][0]).all()


def test_a_box_of_4096_voxels(ops):
    """The largest box: 16 voxels a lane, every register slot in use."""
    sz, B = (16, 16, 16), 3
    rng = np.random.RandomState(11)
    frames, sub = (0.5 + rng.rand(B, 4096)).astype(np.float32), (0.4 * rng.rand(B, 4096)).astype(np.float32)
    A_rows, C = rng.rand(2, 4096).astype(np.float32), rng.rand(2, B).astype(np.float32)
    w = np.array([[1, 0, 2], [1, 1, 1]], dtype=np.float32)
    boxes = np.array([[0, 15, 0, 15, 0, 15], [3, 9, 14, 15, 2, 12]], dtype=np.int32)
    ref = CR.component_stats(frames, sz, A_rows, boxes, C, w, sub=sub)
    out, _ = ops.component_stats(dev(frames), sz, dev(A_rows), boxes, dev(C), dev(w), sub=dev(sub))
    assert out["image"].shape == (2, 4096)
    compare(out, ref, "4096 voxels")


def test_two_pieces_give_the_bits_of_one_call(ops):
    sz, B = (33, 5, 2), 37
    prob = problem(sz, B, True)
    store, perm, sub, A_rows, C, w, boxes, _ = prob
    one, _ = run(ops, sz, prob, segment=5)
    again, _ = run(ops, sz, prob, segment=5)
    for name in one:
        assert torch.equal(one[name].view(torch.int64), again[name].view(torch.int64)), name      # bits, NaN included
    args = (sz, dev(A_rows), boxes)
    first, state = ops.component_stats(dev(store), *args, dev(C[:, :20]), dev(w[:, :20]), sub=dev(sub[:20]),
                                       frame_ids=dev(perm[:20], torch.int32), segment=5, finish=False)
    assert first["image"] is None and first["r_values"] is None
    second, state2 = ops.component_stats(dev(store), *args, dev(C[:, 20:]), dev(w[:, 20:]), sub=dev(sub[20:]),
                                         frame_ids=dev(perm[20:], torch.int32), segment=5, state=state, first=False)
    assert state2 is state
    for name in ("image", "r_values", "foot"):
        assert torch.equal(second[name].view(torch.int64), one[name].view(torch.int64)), name
    for name in ("sums", "frame_corr", "raw"):
        both = torch.cat((first[name], second[name]), 1)
        assert torch.equal(both.view(torch.int64), one[name].view(torch.int64)), name


def test_refusals_launch_nothing(ops):
    from dnmf_amd import _lib
    lib = _lib.load()
    sz = (17, 241, 1)
    P, B = 17 * 241, 2
    frames, A_rows = torch.rand(B, P, device="cuda"), torch.rand(1, P, device="cuda")
    C = w = torch.ones(1, B, device="cuda")
    f64 = dict(dtype=torch.float64, device="cuda")
    outs = [torch.full(s, -7.0, **f64) for s in ((1, B, 3), (1, 3), (1, B), (1, B), (1, 4097), (1,))]
    state = torch.full((1 << 16,), -7.0, **f64)

    def call(box, nbytes):
        bh = torch.tensor([box], dtype=torch.int32)
        bd = bh.cuda()
        rc = lib.dnmf_component_stats(frames.data_ptr(), P, None, 0, None, ops._int3(sz), B, A_rows.data_ptr(), P, bh.data_ptr(),
                                      bd.data_ptr(), 1, C.data_ptr(), B, w.data_ptr(), B, 1, 1, 0, state.data_ptr(), nbytes,
                                      *[o.data_ptr() for o in outs[:5]], 4097, outs[5].data_ptr(), None)
        torch.cuda.synchronize()
        return rc

    assert call((0, 16, 0, 240, 0, 0), state.numel() * 8) == -3 and b"4097 voxels" in lib.dnmf_last_error()     # DNMF_E_UNSUPPORTED
    assert call((0, 17, 0, 3, 0, 0), state.numel() * 8) == -2 and b"outside" in lib.dnmf_last_error()           # DNMF_E_SHAPE
    assert call((0, 3, 0, 3, 0, 0), 64) == -4 and b"state of 64 bytes" in lib.dnmf_last_error()                 # DNMF_E_WORKSPACE
    assert all(bool((o == -7.0).all()) for o in outs) and bool((state == -7.0).all())
    with pytest.raises(_lib.DnmfHipError, match="4097 voxels"):
        ops.component_stats(frames, sz, A_rows, [(0, 16, 0, 240, 0, 0)], C, w)
    ok, st = ops.component_stats(frames, sz, A_rows, [(0, 3, 0, 3, 0, 0)], C, w, finish=False)
    with pytest.raises(_lib.DnmfHipError, match="-4"):
        ops.component_stats(frames, sz, A_rows, [(0, 16, 0, 200, 0, 0)], C, w, state=st, first=False)
    with pytest.raises(ValueError, match="first=False"):
        ops.component_stats(frames, sz, A_rows, [(0, 3, 0, 3, 0, 0)], C, w, first=False)
    with pytest.raises(ValueError):
        ops.component_stats(frames, sz, A_rows, [(0, 3, 0, 3, 0, 0)], C[:, :1], w)
    with pytest.raises(ValueError, match="A_rows are rows"):
        ops.component_stats(frames, sz, A_rows[0], [(0, 3, 0, 3, 0, 0)], C, w)
