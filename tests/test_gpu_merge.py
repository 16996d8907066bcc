"""K26 on the GPU: ``ops.component_pairs`` and ``ops.merge_apply`` against the float64 restatement (tests/merge_restatement.py) on
identical seeded fp32 inputs, and ``DeformableNMF.merge_components`` on the planted model.

Every input is a view into a wider buffer filled with NaN, so that a read past a row shows; the outputs of ``merge_apply`` are views
into wider buffers whose margins must stay as they were.  ``n`` and the NaN pattern of ``corr`` must be equal.  Every raw sum
must be within 1e-12 of the sum of its terms' magnitudes (the bound of K19 / K24: the two sides add the same float64 terms in
another order).  ``overlap`` and ``corr`` are ratios of those sums, of order 1.

Worst absolute deviation of ``overlap`` and ``corr`` measured on these cases on the MI355X: 1.46e-15 (the case 24 x 20 x 1, K = 65,
T = 63; the planted models stay at 4.4e-16).  Ten times the worst is allowed (MEASURED below), and at most 1e-9.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import merge_restatement as MR

pytestmark = pytest.mark.gpu

MEASURED = 1.5e-15      # worst deviation of overlap and corr over CASES, as printed by the tests on the MI355X
TOL = min(10 * MEASURED, 1e-9)

DEPTHS = [2, 1]
KS = [1, 3, 9, 65]           # 65: more neurons than a wave has lanes
TS = [1, 2, 63, 257, 1025]   # both sides of the 256-lane stride, and four rounds of it
CASES = [(d, K, T) for d in DEPTHS for K in KS for T in TS]


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


def make_boxes(K, sz, rng):
    """Boxes 0 and 1 are disjoint, 2 shares exactly one voxel with 0, 3 lies inside 4, 5 is the whole volume; the rest are random."""
    X, Y, Z = sz
    b = np.zeros((K, 6), dtype=np.int32)
    for k in range(K):
        lo = [rng.randint(0, S) for S in sz]
        hi = [rng.randint(l, min(S, l + 9)) for l, S in zip(lo, sz)]
        b[k] = [lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]]
    # boxes 0 and 2 lie in the plane z = 0 and meet in the corner (6, 7, 0) alone
    fixed = [[2, 6, 3, 7, 0, 0], [12, 20, 9, 13, 0, Z - 1], [6, 9, 7, 12, 0, 0], [15, 17, 4, 6, 0, 0], [13, 19, 2, 8, 0, Z - 1],
             [0, X - 1, 0, Y - 1, 0, Z - 1]]
    for k, f in enumerate(fixed[:K] if K > 1 else fixed[5:6]):
        b[k] = f
    return b


def make_traces(K, T, rng):
    """Positive traces of a scale and an offset per row; from K = 3 on row 0 is constant, row 1 has 30 % NaN and row 2 is finite
    only where row 1 is not: no common finite frame; from K = 9 on row 6 has an inf and row 7 is all NaN."""
    c = rng.gamma(2.0, 1.0, (K, T)) * rng.uniform(0.2, 5.0, (K, 1)) + rng.uniform(0.0, 8.0, (K, 1))
    if K >= 3:
        c[0] = 7.1
        gone = rng.rand(T) < 0.3
        c[1, gone] = np.nan
        c[2, ~gone] = np.nan
    if K >= 9:
        c[6, T // 2] = np.inf
        c[7] = np.nan
    return c.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(i):
    """Case i -> (A_rows, boxes, C, pairs, the restatement's statistics); computed once, never changed."""
    depth, K, T = CASES[i]
    sz = (24, 20, depth)
    rng = np.random.RandomState(500 + i)
    A = rng.uniform(0.0, 1.0, (K, sz[0] * sz[1] * sz[2])).astype(np.float32)
    A[rng.rand(*A.shape) < 0.2] = 0.0
    if K >= 9:
        A[8] = 0.0                                # a norm of 0: overlap 0
    boxes = make_boxes(K, sz, rng)
    C = make_traces(K, T, rng)
    pairs = np.array([(i, j) for i in range(K) for j in range(i, K)], dtype=np.int32)
    if K >= 3:
        pairs[1] = pairs[1][::-1]                 # (1, 0): the order inside a pair is the caller's
    return sz, A, boxes, C, pairs, MR.pair_stats(A, sz, boxes, C, pairs=pairs)


def padded(x, fill=np.nan, left=3, right=5):
    """The rows of x as a view into a wider buffer of ``fill``."""
    buf = torch.full((x.shape[0], x.shape[1] + left + right), fill, dtype=torch.float32, device="cuda")
    view = buf[:, left:left + x.shape[1]]
    view.copy_(torch.as_tensor(x))
    return buf, view


def bits(t):
    return t.contiguous().view(torch.int64)


WORST = {}


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"z{d}-K{K}-T{T}" for d, K, T in CASES])
def test_component_pairs_against_the_restatement(ops, i):
    sz, A, boxes, C, pairs, ref = reference(i)
    K = A.shape[0]
    if K >= 3:
        assert MR.intersection(boxes[0], boxes[1]) is None
        q = MR.intersection(boxes[0], boxes[2])
        assert q is not None and len(MR.box_voxels(q, sz)) == 1
    if K >= 9:
        assert MR.intersection(boxes[3], boxes[4]) == [int(v) for v in boxes[3]] and len(MR.box_voxels(boxes[5], sz)) == A.shape[1]
        assert ref["n"][[tuple(p) for p in pairs.tolist()].index((1, 2))] == 0
    _, Ad = padded(A)
    _, Cd = padded(C)
    got = ops.component_pairs(Ad, sz, boxes, Cd, pairs=pairs)
    again = ops.component_pairs(Ad, sz, boxes, Cd, pairs=pairs)
    assert got["pairs"].tolist() == pairs.tolist()
    for name in MR.SUMS + ("overlap", "corr"):
        assert got[name].dtype == torch.float64 and tuple(got[name].shape) == (len(pairs),)
        assert torch.equal(bits(got[name]), bits(again[name])), name            # the same input gives the same bits
    g = {name: got[name].cpu().numpy() for name in MR.SUMS + ("overlap", "corr")}
    np.testing.assert_array_equal(g["n"], ref["n"])
    for name in MR.SUMS:
        err = np.abs(g[name] - ref[name])
        assert np.isfinite(g[name]).all() and (err <= 1e-12 * ref[name + "_mag"]).all(), (name, err.max())
    worst = 0.0
    for name in ("overlap", "corr"):
        np.testing.assert_array_equal(np.isnan(g[name]), np.isnan(ref[name]))
        ok = ~np.isnan(ref[name])
        if ok.any():
            worst = max(worst, float(np.abs(g[name][ok] - ref[name][ok]).max()))
    WORST[i] = worst
    print(f"\ncase {CASES[i]}: worst deviation of overlap and corr {worst:.3g}; over the cases so far {max(WORST.values()):.3g}")
    assert worst <= TOL
    assert not np.isnan(ref["overlap"]).any() and (K < 3 or np.isnan(ref["corr"]).any())


def test_default_pairs_and_refusals(ops):
    sz, A, boxes, C, pairs, _ = reference(CASES.index((2, 9, 63)))
    _, Ad = padded(A)
    _, Cd = padded(C)
    got = ops.component_pairs(Ad, sz, boxes, Cd)
    want = MR.pair_stats(A, sz, boxes, C)
    assert got["pairs"].tolist() == want["pairs"].tolist() and len(want["pairs"]) < len(pairs)
    np.testing.assert_array_equal(got["n"].cpu().numpy(), want["n"])
    np.testing.assert_allclose(got["overlap"].cpu().numpy(), want["overlap"], atol=TOL, rtol=0)
    # without the diagonals a pair has no overlap
    lone = ops.component_pairs(Ad, sz, boxes, Cd, pairs=[(0, 2), (3, 3), (3, 4)])
    assert torch.isnan(lone["overlap"]).tolist() == [True, False, True] and not bool(torch.isnan(lone["saa"]).any())
    from dnmf_amd._lib import DnmfHipError
    with pytest.raises(DnmfHipError, match="dnmf_component_pairs: pair 1"):
        ops.component_pairs(Ad, sz, boxes, Cd, pairs=[(0, 0), (0, 9)])
    bad = boxes.copy()
    bad[4, 1] = 24
    with pytest.raises(DnmfHipError, match="dnmf_component_pairs: box 4"):
        ops.component_pairs(Ad, sz, bad, Cd)
    with pytest.raises(ValueError, match="component_pairs: C must be"):
        ops.component_pairs(Ad, sz, boxes, Cd[:5])
    with pytest.raises(ValueError, match="at most 4096"):
        ops.component_pairs(torch.zeros((4097, 4), device="cuda"), (2, 2, 1), np.zeros((4097, 6), dtype=np.int32), torch.zeros((4097, 2), device="cuda"))


def test_merge_apply_groups_of_1_2_3_17(ops):
    rng = np.random.RandomState(77)
    P, K, T = 777, 26, 130
    order = rng.permutation(K).tolist()
    sizes = [1, 2, 1, 3, 17, 1, 1]
    groups, at = [], 0
    for m in sizes:
        groups.append(sorted(order[at:at + m]))
        at += m
    A = rng.uniform(0.0, 1.0, (P, K)).astype(np.float32)
    C = rng.gamma(2.0, 1.0, (K, T)).astype(np.float32)
    lone = groups[0][0]
    A[5, lone], A[6, lone], C[lone, 3], C[lone, 4] = -0.0, np.nan, -0.0, np.inf     # a singleton is a copy, whatever it holds
    u = [np.ones(1) if m == 1 else rng.uniform(0.1, 1.0, m) for m in sizes]
    w = [np.ones(1) if m == 1 else rng.uniform(0.5, 2.0, m) for m in sizes]
    plan = dict(groups=groups, offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                members=np.array([k for g in groups for k in g], dtype=np.int32), u=np.concatenate(u), w=np.concatenate(w))
    A_ref, C_ref = MR.apply(np.nan_to_num(A, nan=0.0), np.where(np.isfinite(C), C, 0.0), dict(groups=groups, u=u, w=w))
    _, Ad = padded(A, left=1, right=2)
    _, Cd = padded(C)
    Ao_buf, Ao = padded(np.zeros((P, len(sizes)), dtype=np.float32), fill=123.0, left=2, right=3)
    Co_buf, Co = padded(np.zeros((len(sizes), T), dtype=np.float32), fill=123.0)
    ra, rc = ops.merge_apply(Ad, Cd, plan, A_out=Ao, C_out=Co)
    assert ra is Ao and rc is Co
    for buf, view, left in ((Ao_buf, Ao, 2), (Co_buf, Co, 3)):
        assert bool((buf[:, :left] == 123.0).all()) and bool((buf[:, left + view.shape[1]:] == 123.0).all())
    a2, c2 = Ao.cpu().numpy(), Co.cpu().numpy()
    for q, g in enumerate(groups):
        if len(g) == 1:
            assert a2[:, q].tobytes() == A[:, g[0]].tobytes() and c2[q].tobytes() == C[g[0]].tobytes()
        else:
            for got, ref in ((a2[:, q], A_ref[:, q]), (c2[q], C_ref[q])):
                assert (np.abs(got.astype(np.float64) - ref) <= np.spacing(np.abs(ref).astype(np.float32))).all()
    # new outputs without ``out``; the same bits
    b2, d2 = ops.merge_apply(Ad, Cd, plan)
    assert b2.is_contiguous() and torch.equal(b2.view(torch.int32), Ao.contiguous().view(torch.int32))
    assert torch.equal(d2.view(torch.int32), Co.contiguous().view(torch.int32))
    from dnmf_amd._lib import DnmfHipError
    with pytest.raises(DnmfHipError, match="dnmf_merge_apply: A_out or C_out overlaps"):
        ops.merge_apply(Ad, Cd, plan, A_out=Ad[:, :len(sizes)], C_out=Co)
    with pytest.raises(DnmfHipError, match="dnmf_merge_apply: A_out or C_out overlaps"):
        ops.merge_apply(Ad, Cd, plan, A_out=Ao, C_out=Cd[:len(sizes)])


# ---- through the model --------------------------------------------------------------------------------------------------------------
T = 40
MODEL_TENSORS = ("fp.A", "fp.pos", "fp.sigma", "fp.beta", "C", "A")


def planted(M, depth):
    """A model built directly on the planted components (no fit), its loader and the planted arrays."""
    A, C, pos, cells, sz = MR.planted_model(depth, 0, T=T)
    model = M.DeformableNMF(torch.tensor(sz), 8, T, positions=torch.from_numpy(pos).float())
    model.verbose = False
    model.C = torch.from_numpy(C).to("cuda", torch.float32)
    frames = (model.C.t() @ model.fp.A.reshape(-1, 8).t()).contiguous()
    return model, M.ResidentLoader(frames, sz, 8), sz, cells


def snapshot(model):
    get = lambda name: functools.reduce(getattr, name.split("."), model)
    return {name: (get(name), get(name).detach().clone()) for name in MODEL_TENSORS}, model.D.copy(), model.fp.K


def assert_untouched(model, snap):
    tensors, D, K = snap
    for name, (obj, value) in tensors.items():
        now = functools.reduce(getattr, name.split("."), model)
        assert now is obj and torch.equal(now.detach().view(torch.int32), value.view(torch.int32)), name
    assert np.array_equal(model.D, D) and model.fp.K == K


@pytest.mark.parametrize("depth", DEPTHS)
def test_merge_components_on_the_planted_model(M, depth):
    model, loader, sz, cells = planted(M, depth)
    P = sz[0] * sz[1] * sz[2]
    A = model.fp.A.reshape(P, 8).cpu().numpy()
    C = model.C.cpu().numpy()
    st, pl = MR.merge(A, sz, C)
    assert pl["groups"] == [[0, 1], [2, 3], [4], [5], [6], [7]]
    snap = snapshot(model)
    model.last_clean = "kept"
    dry = model.merge_components(dry_run=True)
    assert dry["groups"] == pl["groups"] and dry["merged"] == 2 and dry["K"] == 6 and model.last_merge is dry
    assert dry["pairs"].tolist() == st["pairs"].tolist()
    np.testing.assert_array_equal(np.isnan(dry["corr"].cpu().numpy()), np.isnan(st["corr"]))
    worst = max(float(np.nanmax(np.abs(dry[name].cpu().numpy() - st[name]))) for name in ("corr", "overlap"))
    WORST["planted", depth] = worst
    print(f"\nplanted model, depth {depth}: worst deviation of overlap and corr {worst:.3g}")
    assert worst <= TOL
    assert_untouched(model, snap)
    none = model.merge_components(thr=2.0)
    assert none["merged"] == 0 and none["K"] == 8 and none["groups"] == [[k] for k in range(8)]
    assert_untouched(model, snap)
    assert model.last_clean == "kept"
    # traces with NaN frames decide the same groups; the merge still combines model.C
    tr = model.C.clone()
    tr[:, 5] = float("nan")
    tr[1, 11:14] = float("nan")
    assert model.merge_components(traces=tr, dry_run=True)["groups"] == pl["groups"]
    with pytest.raises(ValueError, match="traces must be"):
        model.merge_components(traces=tr[:, :-1])

    model._ws_k3 = "stale"
    out = model.merge_components(traces=tr)
    assert out["groups"] == pl["groups"] and out["merged"] == 2 and out["K"] == 6 and model.last_merge is out
    assert model.fp.K == 6 and tuple(model.C.shape) == (6, T) and tuple(model.fp.A.shape) == tuple(sz) + (6,) and model.fp.A.is_contiguous()
    assert tuple(model.fp.pos.shape) == (6, 3) and tuple(model.fp.sigma.shape) == (6,) and model.A.shape[0] == 6 and model.D.shape == tuple(sz) + (6,)
    assert model.last_clean is None and model._ws_k3 is None and model.fp._layouts == {}
    old = snap[0]
    assert torch.equal(model.fp.beta.detach(), old["fp.beta"][1]) and model.fp.beta.requires_grad
    A_ref, C_ref = MR.apply(A, C, pl)
    a2, c2 = model.fp.A.reshape(P, 6).cpu().numpy(), model.C.cpu().numpy()
    assert (np.abs(a2 - A_ref) <= np.spacing(np.abs(A_ref).astype(np.float32))).all()
    assert (np.abs(c2 - C_ref) <= np.spacing(np.abs(C_ref).astype(np.float32))).all()
    pos_ref = MR.merged_positions(old["fp.pos"][1].cpu().numpy(), pl)
    np.testing.assert_allclose(model.fp.pos.cpu().numpy(), pos_ref, atol=1e-5)
    # the constructor's torch.cdist forms |x - y|^2 through a float64 matrix product: 1e-13 |x|^2 = 1e-10 on d^2, 5e-10 on a d of
    # 0.1 (a merged centre is no lattice point), times the 0.01 of the formula
    merged_cols = [q for q, g in enumerate(pl["groups"]) if len(g) >= 2]
    D_ref = MR.distance_prior(sz, model.fp.pos.cpu().numpy().astype(np.float64))
    np.testing.assert_allclose(model.D[..., merged_cols], D_ref[..., merged_cols], atol=1e-9)
    for q, g in enumerate(pl["groups"]):
        if len(g) == 1:                                              # an unmerged component keeps its bits
            assert torch.equal(model.fp.A[..., q], old["fp.A"][1][..., g[0]]) and torch.equal(model.C[q], old["C"][1][g[0]])
            assert torch.equal(model.fp.pos[q], old["fp.pos"][1][g[0]]) and np.array_equal(model.D[..., q], snap[1][..., g[0]])
        else:
            truth = cells[MR.PLANTED_CELL_OF[g[0]]]
            assert np.corrcoef(c2[q], truth)[0, 1] >= max(np.corrcoef(C[k], truth)[0, 1] for k in g)
        assert torch.equal(model.A[q], old["A"][1][pl["dominant"][q]])
    # the shrunk model goes on: the layouts were really forgotten
    model.update_footprints(loader, 8, sz, gamma_c=0, iter_c=5)
    assert tuple(model.C.shape) == (6, T) and bool(torch.isfinite(model.C).all())
    assert model.merge_components()["merged"] == 0


def test_merge_components_refusals(M):
    model, loader, sz, _ = planted(M, 1)
    model.C[1, 7] = -0.5
    snap = snapshot(model)
    with pytest.raises(ValueError, match="merge_components.*negative or non-finite"):
        model.merge_components(thr=0.5)
    assert_untouched(model, snap)
    multi = M.MultiChannelDNMF(torch.tensor(sz), 2, T, torch.ones(2, 2), positions=torch.tensor([[5.0, 5.0, 0.0], [12.0, 6.0, 0.0]]))
    with pytest.raises(NotImplementedError, match="one channel"):
        multi.merge_components()
    shard = copy.copy(model)
    shard.group = object()
    with pytest.raises(NotImplementedError, match="shard"):
        shard.merge_components()
