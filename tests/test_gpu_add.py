"""K28 on the GPU against tests/add_restatement.py: the gather (K28a) bit for bit -- it is a subtraction and a copy -- and the rank-1
factor (K28b) within the project's bounds for float64 sums in a fixed order and one rounding to fp32:

    |c_t - ref| <= ulp32(ref) + 1e-12 sum_j |a_j e_tj| / sum a^2        (the same form for a and for the float64 sums)
"""
import functools

import numpy as np
import pytest
import torch

import add_restatement as AR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def cuda(x, dtype=torch.float32):
    return torch.from_numpy(np.array(x)).to("cuda", dtype)      # a copy: the shared cases are read-only


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# (sz, centres, half, n frames): boxes clipped at the volume's corners and a one-voxel box among five; one 16 x 16 x 16 box with
# three frames; a single frame; 65 frames (more than one run of 8, and of 64) on one box
GATHER = {
    "corners": ((11, 9, 3), [[0, 0, 0], [10, 8, 2], [5, 4, 1], [10, 0, 2], [3.4, 7.6, 0.2]], [2, 3, 1], 7),
    "one-voxel": ((11, 9, 3), [[4, 4, 1], [0, 8, 2]], 0, 5),
    "4096": ((20, 18, 17), [[8, 8, 8]], None, 3),
    "n=1": ((7, 6, 1), [[3, 3, 0], [6, 0, 0], [0, 5, 0], [2, 2, 0], [5, 4, 0]], [2, 1, 0], 1),
    "n=65": ((7, 6, 2), [[3, 3, 1]], [2, 2, 1], 65),
}


def gather_case(name):
    sz, centres, half, n = GATHER[name]
    rng = np.random.default_rng(len(name))
    P = sz[0] * sz[1] * sz[2]
    frames = rng.standard_normal((n, P)).astype(np.float32)
    sub = rng.standard_normal((n, P)).astype(np.float32)
    frames[n // 2, P // 3] = np.nan
    frames[0, P - 1] = np.inf
    if half is None:
        boxes = np.array([[0, 15, 1, 16, 1, 16]], dtype=np.int32)
    else:
        boxes = AR.candidate_boxes(centres, sz, half)
    return sz, frames, sub, boxes


@pytest.mark.parametrize("name", list(GATHER))
def test_gather_is_the_definition_bit_for_bit(ops, name):
    sz, frames, sub, boxes = gather_case(name)
    n = frames.shape[0]
    nvox = AR.box_sizes(boxes)
    if name == "4096":
        assert nvox.tolist() == [4096]
    if name == "one-voxel":
        assert nvox.tolist() == [1, 1]
    for s in (None, sub):
        want = AR.residual_boxes(frames, sz, boxes, sub=s)
        got = ops.residual_boxes(cuda(frames), sz, boxes, sub=None if s is None else cuda(s))
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # sub given = frames subtracted beforehand
    with np.errstate(invalid="ignore"):
        pre = (frames - sub).astype(np.float32)
    assert torch.equal(ops.residual_boxes(cuda(pre), sz, boxes).view(torch.int32), got.view(torch.int32))
    # two pieces with t0 = one piece; rows picked by frame_ids from a strided buffer; a wider vmax is zero-filled
    if n >= 2:
        cut = n // 2 + 1
        E = torch.full((boxes.shape[0], n, min(int(nvox.max()) + 3, 4096)), 7.0, device="cuda")
        wide = torch.zeros((n + 2, frames.shape[1] + 5), device="cuda")
        order = np.random.default_rng(1).permutation(n)
        wide[torch.from_numpy(order).cuda() + 2, :frames.shape[1]] = cuda(frames)
        rows = wide[:, :frames.shape[1]]
        ids = torch.from_numpy(order + 2).to(torch.int32)
        ops.residual_boxes(rows, sz, boxes, sub=cuda(sub)[cut:], frame_ids=ids[cut:], out=E, t0=cut, n_total=n)
        ops.residual_boxes(rows, sz, boxes, sub=cuda(sub)[:cut], frame_ids=ids[:cut], out=E, t0=0, n_total=n)
        assert torch.equal(E[:, :, :got.shape[2]].contiguous().view(torch.int32), got.view(torch.int32))
        assert bool((E[:, :, got.shape[2]:] == 0).all())


def test_gather_refusals(ops):
    sz, frames, sub, boxes = gather_case("corners")
    fr = cuda(frames)
    with pytest.raises(ValueError, match="outside the volume"):
        ops.residual_boxes(fr, sz, [[0, 11, 0, 1, 0, 1]])
    with pytest.raises(ValueError, match="4096"):
        ops.residual_boxes(torch.zeros((1, 20 * 18 * 17), device="cuda"), (20, 18, 17), [[0, 16, 0, 15, 0, 15]])
    with pytest.raises(ValueError, match="do not fit"):
        ops.residual_boxes(fr, sz, boxes, t0=3, n_total=8)
    with pytest.raises(ValueError, match="out must be"):
        ops.residual_boxes(fr, sz, boxes, out=torch.zeros((5, 7, 3), device="cuda"))
    with pytest.raises(ValueError, match="18432"):
        ops.residual_boxes(fr, sz, boxes, t0=0, n_total=18433)


# ---- K28b ------------------------------------------------------------------------------------------------------------------------
# (M, n frames, vmax, voxels of each box): one and five candidates, one and 65 frames, a one-voxel box, a 4096-voxel box with three
# frames, boxes on both sides of the a-step's tile of 64 and of the c-step's 64 lanes
FACTOR = {
    "M=1": (1, 12, 30, [30]),
    "M=5": (5, 65, 130, [1, 63, 64, 65, 130]),
    "n=1": (2, 1, 9, [9, 4]),
    "4096": (1, 3, 4096, [4096]),
    "n<waves": (2, 5, 70, [70, 2]),
}


@functools.lru_cache(maxsize=None)
def factor_case(name):
    """E, nvox, a0 and the definition's result -- made once."""
    M, n, vmax, nvox = FACTOR[name]
    rng = np.random.default_rng(len(name) + 11)
    E = np.zeros((M, n, vmax), dtype=np.float32)
    a0 = np.zeros((M, vmax), dtype=np.float32)
    for m, k in enumerate(nvox):
        a, c = rng.uniform(0.0, 1.0, k), rng.uniform(0.0, 2.0, n)
        E[m, :, :k] = np.outer(c, a) + 0.3 * rng.standard_normal((n, k))
        a0[m, :k] = rng.uniform(0.2, 1.0, k)
    E.setflags(write=False), a0.setflags(write=False)
    return E, np.array(nvox), a0, AR.rank1_nmf(E, nvox, a0, iters=5)


def check_factor(got, ref, nvox):
    g = {k: v.cpu().numpy() for k, v in got.items()}
    assert g["ok"].tolist() == ref["ok"].tolist() and g["n_valid"].tolist() == ref["n_valid"].tolist()
    assert g["a"].dtype == np.float32 and g["c"].dtype == np.float32 and g["energy"].dtype == np.float64
    worst = {}
    for name, mag in (("a", ref["a_mag"]), ("c", ref["c_mag"])):
        assert np.array_equal(np.isnan(g[name]), np.isnan(ref[name])), name
        on = ~np.isnan(ref[name])
        bound = ulp32(ref[name][on]) + 1e-12 * mag[on]
        dev = np.abs(g[name][on].astype(np.float64) - ref[name][on])
        worst[name] = float((dev / np.maximum(ulp32(ref[name][on]), 1e-300)).max()) if on.any() else 0.0
        assert (dev <= bound).all(), (name, float((dev - bound).max()))
    for m, k in enumerate(nvox):
        assert (g["a"][m, k:] == 0).all()
    for name, mag in (("energy", ref["energy"]), ("explained", ref["explained_mag"]), ("saa", ref["saa"]), ("scc", ref["scc"])):
        assert np.array_equal(np.isnan(g[name]), np.isnan(ref[name])), name
        on = ~np.isnan(ref[name])
        dev = np.abs(g[name][on] - ref[name][on])
        worst[name] = float((dev / np.maximum(mag[on], 1e-300)).max()) if on.any() else 0.0
        assert (dev <= 1e-12 * mag[on]).all(), (name, dev, mag[on])
    return worst


@pytest.mark.parametrize("name", list(FACTOR))
def test_factor_is_the_definition(ops, name):
    E, nvox, a0, ref = factor_case(name)
    assert ref["ok"].all()
    got = ops.rank1_nmf(cuda(E), nvox, cuda(a0), iters=5)
    worst = check_factor(got, ref, nvox)
    print(f"\n{name}: a and c within {worst['a']:.2f} and {worst['c']:.2f} ulp32 of the definition; float64 sums within "
          f"{max(worst[k] for k in ('energy', 'explained', 'saa', 'scc')):.1e} of their magnitude")
    again = ops.rank1_nmf(cuda(E), nvox, cuda(a0), iters=5)
    for k in got:
        assert torch.equal(got[k].view(torch.int32 if got[k].element_size() == 4 else torch.int64),
                           again[k].view(torch.int32 if got[k].element_size() == 4 else torch.int64)), k
    one = ops.rank1_nmf(cuda(E), nvox, cuda(a0), iters=1)
    check_factor(one, AR.rank1_nmf(E, nvox, a0, iters=1), nvox)


def test_factor_nan_frames_and_refused_candidates(ops):
    E, nvox, a0, _ = factor_case("M=5")
    E, a0 = E.copy(), a0.copy()
    E[3, 7, 10] = np.nan                 # one frame of candidate 3 only
    E[3, 64, 0] = np.inf
    E[4, 7, 129] = -np.inf
    E[1, 9, 63] = np.nan                 # past the 63 voxels of candidate 1: not a sample of its box
    E[2] = 0.0                           # an all-zero box
    E[0] = -np.abs(E[0])                 # a one-voxel box that is never positive
    ref = AR.rank1_nmf(E, nvox, a0, iters=5)
    assert ref["ok"].tolist() == [0, 1, 0, 1, 1] and ref["n_valid"].tolist() == [65, 65, 65, 63, 64]
    got = ops.rank1_nmf(cuda(E), nvox, cuda(a0), iters=5)
    check_factor(got, ref, nvox)
    c = got["c"].cpu().numpy()
    assert np.isnan(c[3]).nonzero()[0].tolist() == [7, 64] and np.isnan(c[4]).nonzero()[0].tolist() == [7] and not np.isnan(c[1]).any()
    assert np.isnan(c[0]).all() and np.isnan(c[2]).all() and np.isnan(got["a"][2, :64].cpu().numpy()).all()
    assert float(got["energy"][2]) == 0.0 and float(got["energy"][0]) > 0.0
    # no valid frame at all, and a start of zeros
    E[1, :, 0] = np.nan
    a0[3] = 0.0
    ref = AR.rank1_nmf(E, nvox, a0, iters=5)
    assert ref["ok"].tolist() == [0, 0, 0, 0, 1] and ref["n_valid"].tolist() == [65, 0, 65, 63, 64]
    check_factor(ops.rank1_nmf(cuda(E), nvox, cuda(a0), iters=5), ref, nvox)


def test_factor_refusals(ops):
    E, nvox, a0, _ = factor_case("M=1")
    with pytest.raises(ValueError, match="iters"):
        ops.rank1_nmf(cuda(E), nvox, cuda(a0), iters=0)
    with pytest.raises(ValueError, match="nvox"):
        ops.rank1_nmf(cuda(E), [31], cuda(a0))
    with pytest.raises(ValueError, match="nvox"):
        ops.rank1_nmf(cuda(E), [0], cuda(a0))
    with pytest.raises(ValueError, match="a0 must be"):
        ops.rank1_nmf(cuda(E), nvox, cuda(a0)[:, :29].contiguous())
    with pytest.raises(ValueError, match="limits"):
        ops.rank1_nmf(torch.zeros((1, 1, 4097), device="cuda"), [1], torch.ones((1, 4097), device="cuda"))
