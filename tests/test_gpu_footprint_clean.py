"""K27 on the GPU: ``ops.clean_footprints`` against its definition (tests/footprint_clean_restatement.py) on identical fp32 inputs, and
``DeformableNMF.clean_footprints`` on a small model with planted speckles.

Every output of the definition is an integer or a bit pattern, so everything is compared for equality: the fp32 bits of ``A_out``,
the six int32 statistics, and ``threshold`` and ``energy`` as float64 (NaN equal to NaN).  Nothing here has a tolerance."""
import copy
import functools
import itertools

import numpy as np
import pytest
import torch

import footprint_clean_restatement as R

pytestmark = pytest.mark.gpu

OPTIONS = [dict(method=me, median=md, closing=cl, values=va)
           for me, md, cl, va in itertools.product(("nrg", "max"), (True, False), (True, False), ("filtered", "original"))]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd.Demix import dNMF
    return dNMF


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def whole(sz):
    return (0, sz[0] - 1, 0, sz[1] - 1, 0, sz[2] - 1)


def stack(vols):
    return np.ascontiguousarray(np.stack(vols, axis=3), dtype=np.float32)


def tight_box(support, margin=1):
    idx = np.nonzero(support)
    return tuple(int(v) for i, s in zip(idx, support.shape) for v in (max(i.min() - margin, 0), min(i.max() + margin, s - 1)))


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (A (X, Y, Z, K) fp32, boxes (K, 6)); built once, never modified."""
    rng = np.random.default_rng(len(name))
    if name in ("planted2", "planted1"):
        Z = int(name[-1])
        a, support, hole, box = R.planted_volume(Z)
        b, _, _ = R.island_volume(Z)
        return stack([a, b, a, b]), np.array([box, box, tight_box(support), tight_box(support, 3)])
    if name == "corner":          # boxes in the corners of the volume, noise outside them: clamped taps, erosion at the box edge
        sz = (12, 11, 3)
        vols, boxes = [], []
        for centre, box in (((0.5, 0.7, 0.2), (0, 5, 0, 6, 0, 1)), ((11, 10, 2), (6, 11, 5, 10, 1, 2)), ((0, 10, 1), (0, 4, 6, 10, 0, 2))):
            v = R.gaussian_cell(sz, centre, sigma=2.0) + (0.3 * rng.random(sz) * (rng.random(sz) < 0.25)).astype(np.float32)
            vols.append(v)
            boxes.append(box)
        return stack(vols), np.array(boxes)
    if name == "full2d":          # a box of exactly 4096 voxels: the whole sort, the whole LDS
        sz = (70, 70, 1)
        v = R.gaussian_cell(sz, (34.2, 35.1, 0), sigma=9.0, floor=0.05) + (0.5 * rng.random(sz) * (rng.random(sz) < 0.3)).astype(np.float32)
        w = (rng.random(sz) * (rng.random(sz) < 0.55)).astype(np.float32)      # many parts near the percolation threshold
        return stack([v, w]), np.array([(3, 66, 3, 66, 0, 0)] * 2)
    if name == "full3d":
        sz = (18, 17, 18)
        v = R.gaussian_cell(sz, (8.4, 8.1, 9.3), sigma=4.0, floor=0.05) + (0.5 * rng.random(sz) * (rng.random(sz) < 0.2)).astype(np.float32)
        return stack([v]), np.array([(1, 16, 0, 15, 2, 17)])
    if name == "one voxel":
        sz = (5, 4, 2)
        v = rng.random(sz).astype(np.float32) + 0.1
        z = v.copy()
        z[2, 1, 1] = 0
        return stack([v, z, v]), np.array([(2, 2, 1, 1, 1, 1), (2, 2, 1, 1, 1, 1), (0, 0, 0, 0, 0, 0)])
    if name == "spiral":
        a, _ = R.spiral(16)
        return stack([a, a[::-1].copy()]), np.array([whole(a.shape)] * 2)
    if name == "tie":
        a, box = R.two_equal_parts()
        return stack([a, a[::-1, ::-1].copy()]), np.array([box, box])
    if name == "plateau":
        a, box, _ = R.plateau()
        return stack([a]), np.array([box])
    if name == "refused":         # zeros, a NaN, an inf and a negative value between neurons that are cleaned
        a, _, _, box = R.planted_volume(2)
        b, _, _ = R.island_volume(2)
        nan, inf, neg, negzero = a.copy(), a.copy(), a.copy(), a.copy()
        nan[10, 9, 1], inf[3, 3, 0], neg[11, 10, 0] = np.nan, np.inf, -1e-6
        negzero[a == 0] = -0.0
        return stack([a, np.zeros_like(a), b, nan, inf, a, neg, negzero]), np.array([box] * 8)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, items):
    A, boxes = case(name)
    return R.clean_footprints(A, A.shape[:3], boxes, **dict(items))


def check(ops, name, flat=False, **kw):
    A, boxes = case(name)
    sz, K = A.shape[:3], A.shape[3]
    ref, rst = reference(name, tuple(sorted(kw.items())))
    dev = torch.from_numpy(A).cuda()
    if flat:
        dev = dev.reshape(-1, K)
    out, st = ops.clean_footprints(dev, sz, torch.from_numpy(boxes), **kw)
    assert out.shape == dev.shape and out.dtype == torch.float32
    got = out.cpu().numpy().reshape(A.shape)
    for n in R.STAT_INTS:
        assert st[n].dtype == torch.int32 and st[n].cpu().tolist() == rst[n].tolist(), (name, kw, n, st[n].cpu().tolist(), rst[n].tolist())
    for n in R.STAT_FLOATS:
        assert st[n].dtype == torch.float64
        assert np.array_equal(st[n].cpu().numpy(), rst[n], equal_nan=True), (name, kw, n, st[n].cpu().tolist(), rst[n].tolist())
    wrong = np.nonzero(bits(got) != bits(ref))
    assert np.array_equal(bits(got), bits(ref)), (name, kw, [w[:5].tolist() for w in wrong])
    assert np.array_equal(bits(dev.cpu().numpy()), bits(A).reshape(dev.shape))               # the input is only read
    return rst


@pytest.mark.parametrize("name", ["planted2", "planted1", "corner"])
@pytest.mark.parametrize("kw", OPTIONS, ids=lambda kw: "-".join(str(v) for v in kw.values()))
def test_every_option_on_the_planted_volumes_and_in_the_corners(ops, name, kw):
    rst = check(ops, name, flat=kw["median"], **kw)
    assert rst["ok"].all()
    if name != "corner" and not kw["median"] and kw["method"] == "nrg":
        assert (rst["n_parts"][:2] >= 2).all()                   # the speckles reach the largest-part step


@pytest.mark.parametrize("name", ["full2d", "full3d"])
@pytest.mark.parametrize("kw", [dict(), dict(median=False, closing=False), dict(method="max", maxthr=0.3, values="original")],
                         ids=["default", "bare", "max"])
def test_a_box_of_4096_voxels(ops, name, kw):
    A, boxes = case(name)
    assert all((b[1::2] - b[0::2] + 1).prod() == 4096 for b in boxes)
    rst = check(ops, name, **kw)
    assert rst["ok"].all() and (rst["n_box"] == 4096).all()
    if name == "full2d" and kw.get("median") is False:
        assert rst["n_parts"][1] >= 50                           # many parts: the sizes and the tie rule are at work


def test_a_box_of_one_voxel(ops):
    for kw in (dict(), dict(method="max"), dict(median=False, closing=False)):
        rst = check(ops, "one voxel", **kw)
        assert rst["n_box"].tolist() == [1, 1, 1] and rst["ok"][0] == 1 and rst["ok"][2] == 1
        if not kw.get("median", True):
            assert rst["ok"][1] == 0 and rst["n_kept"].tolist() == [1, 0, 1]      # the voxel that is 0 cannot be cleaned


def test_the_spiral_converges_to_one_part(ops):
    rst = check(ops, "spiral", nrgthr=1.0, median=False, closing=False)
    length = R.spiral(16)[1]
    assert rst["n_parts"].tolist() == [1, 1] and rst["n_kept"].tolist() == [length, length] and length >= 100
    check(ops, "spiral", method="max", maxthr=0.0, median=False, closing=False)


def test_two_parts_of_equal_size(ops):
    rst = check(ops, "tie", nrgthr=1.0, median=False, closing=False)
    assert rst["n_parts"].tolist() == [2, 2] and rst["n_kept"].tolist() == [4, 4]
    ref = reference("tie", (("closing", False), ("median", False), ("nrgthr", 1.0)))[0]
    assert set(ref[..., 0][ref[..., 0] > 0]) == {1.0} and set(ref[..., 1][ref[..., 1] > 0]) == {2.0}   # the lowest index, whatever its values


def test_a_plateau_across_the_cut(ops):
    nrgthr = R.plateau()[2]
    rst = check(ops, "plateau", nrgthr=nrgthr, median=False, closing=False)
    assert rst["n_cut"].tolist() == [25] and rst["threshold"].tolist() == [1.0] and rst["energy"].tolist() == [42 / 52]
    check(ops, "plateau", nrgthr=nrgthr)


@pytest.mark.parametrize("kw", [dict(), dict(median=False), dict(method="max", closing=False)], ids=["default", "nomedian", "max"])
def test_refused_columns_come_back_and_leave_the_others_alone(ops, kw):
    rst = check(ops, "refused", **kw)
    assert rst["ok"].tolist() == [1, 0, 1, 0, 0, 1, 0, 1]
    A, boxes = case("refused")
    ref = reference("refused", tuple(sorted(kw.items())))[0]
    for k in (1, 3, 4, 6):
        assert np.array_equal(bits(ref[..., k]), bits(A[..., k]))
    assert np.array_equal(bits(ref[..., 0]), bits(ref[..., 5]))                             # the same column between other neighbours
    assert np.array_equal(bits(ref[..., 0]), bits(R.clean_footprint(A[..., 0], boxes[0], **kw)[0]))


def test_nothing_above_the_maximum_is_refused(ops):
    rst = check(ops, "planted2", method="max", maxthr=1.0)
    assert not rst["ok"].any()


def test_argument_errors_come_before_any_launch(ops):
    A, boxes = case("full2d")
    sz = A.shape[:3]
    dev = torch.from_numpy(A).cuda()
    b = boxes.copy()
    b[1] = (3, 67, 3, 66, 0, 0)
    with pytest.raises(ValueError, match="4160 voxels, at most 4096"):
        ops.clean_footprints(dev, sz, b)
    for bad in ((3, 70, 3, 6, 0, 0), (-1, 5, 3, 6, 0, 0), (5, 4, 3, 6, 0, 0), (3, 6, 3, 6, 0, 1)):
        b[1] = bad
        with pytest.raises(ValueError, match="empty or outside the volume"):
            ops.clean_footprints(dev, sz, b)
    with pytest.raises(ValueError, match="boxes must be"):
        ops.clean_footprints(dev, sz, boxes[:1])
    with pytest.raises(ValueError, match="float32"):
        ops.clean_footprints(dev.double(), sz, boxes)
    with pytest.raises(ValueError, match="float32"):
        ops.clean_footprints(dev.cpu(), sz, boxes)
    with pytest.raises(ValueError, match="A must be"):
        ops.clean_footprints(dev.reshape(-1, 2)[:-1], sz, boxes)
    with pytest.raises(ValueError, match="A must be"):
        ops.clean_footprints(dev.reshape(35, 140, 1, 2), sz, boxes)
    with pytest.raises(ValueError, match=r"\(P, K\) or \(X, Y, Z, K\)"):
        ops.clean_footprints(dev.reshape(-1), sz, boxes)
    with pytest.raises(ValueError, match="out must be"):
        ops.clean_footprints(dev, sz, boxes, out=torch.empty(5, 2, device="cuda"))
    for kw, text in ((dict(method="energy"), "method"), (dict(values="raw"), "values"), (dict(nrgthr=0.0), "nrgthr"),
                     (dict(nrgthr=1.5), "nrgthr"), (dict(method="max", maxthr=-0.1), "maxthr")):
        with pytest.raises(ValueError, match=text):
            ops.clean_footprints(dev, sz, boxes, **kw)
    assert np.array_equal(bits(dev.cpu().numpy()), bits(A))


def test_two_runs_give_the_same_bits_and_out_may_be_A(ops):
    for name in ("full2d", "refused"):
        A, boxes = case(name)
        sz = A.shape[:3]
        dev = torch.from_numpy(A).cuda()
        first, st1 = ops.clean_footprints(dev, sz, boxes)
        second, st2 = ops.clean_footprints(dev, sz, boxes)
        assert torch.equal(first.view(torch.int32), second.view(torch.int32))
        for n in st1:
            assert torch.equal(st1[n].view(torch.int64 if st1[n].dtype == torch.float64 else torch.int32),
                               st2[n].view(torch.int64 if st2[n].dtype == torch.float64 else torch.int32)), n
        given = torch.full_like(dev, 7.0)
        out, _ = ops.clean_footprints(dev, sz, boxes, out=given)
        assert out is given and torch.equal(out.view(torch.int32), first.view(torch.int32))
        out, st3 = ops.clean_footprints(dev, sz, boxes, out=dev)
        assert out is dev and torch.equal(dev.view(torch.int32), first.view(torch.int32))
        assert st3["n_kept"].tolist() == st1["n_kept"].tolist()


# ---- the model ----------------------------------------------------------------------------------------------------------------------
SZ, K, T = (24, 20, 2), 6, 12
POSITIONS = [[5.0, 5.0, 0.5], [5.0, 14.0, 0.5], [12.0, 5.0, 0.5], [12.0, 14.0, 0.5], [19.0, 5.0, 0.5], [19.0, 14.0, 0.5]]
SPECKLES = {0: [(22, 18, 1), (15, 10, 0)], 3: [(1, 1, 0)], 4: [(2, 17, 1), (8, 12, 0)]}      # neuron -> far voxels set to 0.3
MODEL_TENSORS = ("fp.A", "fp.pos", "fp.sigma", "fp.beta", "C", "A")


def planted_model(M):
    torch.manual_seed(3)
    model = M.DeformableNMF(torch.tensor(SZ), K, T, positions=torch.tensor(POSITIONS))
    model.verbose = False
    with torch.no_grad():
        model.fp.A[model.fp.A < 0.02] = 0                       # compact cells, as a fit leaves them
        for k, voxels in SPECKLES.items():
            for v in voxels:
                model.fp.A[v + (k,)] = 0.3
        model.fp.A[5, 5, 0, 0] = 0                              # a pinhole
    frames = (model.C.t() @ model.fp.A.reshape(-1, K).t()).contiguous()
    return model, M.ResidentLoader(frames, SZ, 4)


def snapshot(model):
    get = lambda name: functools.reduce(getattr, name.split("."), model)
    other = {n: v for n, v in vars(model).items() if not torch.is_tensor(v) and not isinstance(v, np.ndarray) and n != "fp"}
    return {name: (get(name), get(name).detach().clone()) for name in MODEL_TENSORS}, model.D.copy(), other


def assert_untouched(model, snap, but=()):
    tensors, D, other = snap
    for name, (obj, value) in tensors.items():
        if name in but:
            continue
        now = functools.reduce(getattr, name.split("."), model)
        assert now is obj and torch.equal(now.detach().view(torch.int32), value.view(torch.int32)), name
    assert np.array_equal(model.D, D)
    for n, v in other.items():
        if n not in but:
            assert getattr(model, n) is v, n


def test_model_clean_footprints(ops, M):
    model, loader = planted_model(M)
    P = SZ[0] * SZ[1] * SZ[2]
    before = model.fp.A.detach().clone()
    boxes_before = ops.component_boxes(before, SZ)
    snap = snapshot(model)
    model.last_clean = "kept"
    snap[2]["last_clean"] = "kept"
    layouts = model.fp._layouts
    dry = model.clean_footprints(dry_run=True)
    assert_untouched(model, snap)
    assert model.last_footprint_clean is None and model.fp._layouts is layouts
    boxes = ops.component_boxes(before, SZ, floor=1e-3, margin=1)
    want, wst = ops.clean_footprints(before.reshape(P, K), SZ, boxes)
    ref, rst = R.clean_footprints(before.cpu().numpy(), SZ, boxes.cpu().numpy())
    assert np.array_equal(bits(want.cpu().numpy().reshape(ref.shape)), bits(ref))
    assert dry["ok"].tolist() == [1] * K and torch.equal(dry["boxes"], boxes)
    for n in R.STAT_INTS:
        assert dry[n].tolist() == rst[n].tolist() == wst[n].tolist()

    model._ws_k3 = "stale"
    A_obj = model.fp.A
    out = model.clean_footprints()
    assert model.last_footprint_clean is out and model.last_clean is None and model._ws_k3 is None and model.fp._layouts == {}
    assert model.fp.A is A_obj and torch.equal(model.fp.A.reshape(P, K).view(torch.int32), want.view(torch.int32))
    assert_untouched(model, snap, but=("fp.A", "last_clean", "last_footprint_clean") + model._K_SHAPED)
    for n in R.STAT_INTS:
        assert out[n].tolist() == rst[n].tolist()
    assert model.fp.A[5, 5, 0, 0] > 0.5                          # the pinhole is filled
    for k, voxels in SPECKLES.items():
        for v in voxels:
            assert model.fp.A[v + (k,)] == 0
    boxes_after = ops.component_boxes(model.fp.A, SZ)
    size = lambda b: (b[:, 1::2] - b[:, 0::2] + 1).long().prod(1)
    assert bool((boxes_after[:, 0::2] >= boxes_before[:, 0::2]).all()) and bool((boxes_after[:, 1::2] <= boxes_before[:, 1::2]).all())
    assert bool((size(boxes_after)[list(SPECKLES)] < size(boxes_before)[list(SPECKLES)]).all())
    # the cleaned model goes on: the layouts were really forgotten
    model.update_footprints(loader, 4, SZ, gamma_c=0, gamma_a=0.2, iter_c=3, live_spatial=True)
    assert bool(torch.isfinite(model.C).all()) and bool(torch.isfinite(model.fp.A).all())


def test_model_hopeless_columns_and_refusals(ops, M):
    model, loader = planted_model(M)
    with torch.no_grad():
        model.fp.A[..., 1] = 0
        model.fp.A[7, 3, 1, 2] = float("nan")
    before = model.fp.A.detach().clone()
    out = model.clean_footprints()
    assert out["ok"].tolist() == [1, 0, 0, 1, 1, 1] and out["n_box"].tolist()[1:3] == [1, 1]
    assert out["boxes"][2].tolist() == [7, 7, 3, 3, 1, 1]
    for k in (1, 2):
        assert torch.equal(model.fp.A[..., k].view(torch.int32), before[..., k].view(torch.int32))
    big = M.DeformableNMF(torch.tensor((70, 70, 1)), 1, 4, positions=torch.tensor([[35.0, 35.0, 0.0]]))
    with torch.no_grad():
        big.fp.A[...] = 0.5                                     # a cell as large as the volume
    kept = big.fp.A.clone()
    with pytest.raises(ValueError, match="clean_footprints: the box of neuron 0 holds 4900 voxels, at most 4096"):
        big.clean_footprints()
    assert torch.equal(big.fp.A, kept) and big.last_footprint_clean is None
    multi = M.MultiChannelDNMF(torch.tensor(SZ), 2, T, torch.ones(2, 2), positions=torch.tensor(POSITIONS[:2]))
    with pytest.raises(NotImplementedError, match="one channel"):
        multi.clean_footprints()
    shard = copy.copy(model)
    shard.group = object()
    with pytest.raises(NotImplementedError, match="shard"):
        shard.clean_footprints()
