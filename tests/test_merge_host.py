"""The merge of duplicate components (K26) without a GPU: the float64 definition (tests/merge_restatement.py) on exact and planted
cases, the host half of the product (``ops.merge_groups`` / ``ops.merge_plan``) against it, and the wiring of every layer."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import merge_restatement as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exact_rank_one_group():
    """Members that are multiples of one footprint and one trace: the merged component is their sum, exactly."""
    rng = np.random.default_rng(3)
    a, c = rng.uniform(0.1, 1.0, 40), rng.uniform(0.0, 2.0, 30)
    alpha, gamma = np.array([0.7, 1.3, 0.2]), np.array([1.1, 0.4, 2.5])
    A, C = a[:, None] * alpha[None, :], gamma[:, None] * c[None, :]
    u, w, d, weight = MR.merge_weights(A.T @ A, C @ C.T, iters=10)
    M = A @ C
    got = np.outer(A @ u, w @ C)
    assert np.abs(got - M).max() <= 1e-12 * np.abs(M).max()
    assert d == int(np.argmax(alpha * gamma)) and abs((A @ u) @ (A @ u) - (A[:, d] ** 2).sum()) <= 1e-12 * (A[:, d] ** 2).sum()


def test_coefficient_space_is_the_dense_iteration():
    rng = np.random.default_rng(5)
    A, C = rng.uniform(0.0, 1.0, (40, 3)), rng.uniform(0.0, 1.0, (3, 30))
    u, w = MR.rank1_coefficients(A.T @ A, C @ C.T, iters=10)
    a, c, clamped = MR.rank1_dense(A, C, iters=10)
    assert clamped == 0
    assert np.abs(A @ u - a).max() <= 1e-10 * np.abs(a).max()
    assert np.abs(w @ C - c).max() <= 1e-10 * np.abs(c).max()
    assert (u >= 0).all() and (w >= 0).all()


@pytest.mark.parametrize("depth", [2, 1])
def test_planted_model_merges_exactly_the_splits(depth):
    """The gap the defaults of ``merge_components`` sit in: printed, and recorded in its docstring.  The defaults 0.85 / 0.1 lay
    inside from the first planted noise tried (PLANTED_NOISE = 0.05); what the noise is proportional to was changed for the
    merged-trace assertion, see ``planted_model``."""
    from dnmf_amd.Demix import dNMF
    sig = inspect.signature(dNMF.DeformableNMF.merge_components).parameters
    thr, min_overlap = sig["thr"].default, sig["min_overlap"].default
    assert (thr, min_overlap, sig["margin"].default, sig["iters"].default) == (0.85, 0.1, 0, 10)
    low_split, high_indep, low_overlap, high_far = [], [], [], []
    for seed in range(3):
        A, C, pos, cells, sz = MR.planted_model(depth, seed)
        assert sz == (24, 20, depth) and C.shape == (8, 40)
        st, pl = MR.merge(A, sz, C, thr=thr, min_overlap=min_overlap)
        assert pl["groups"] == [[0, 1], [2, 3], [4], [5], [6], [7]]
        pairs = st["pairs"].tolist()
        split = np.array([p in MR.PLANTED_SPLITS for p in pairs])
        off = np.array([i != j for i, j in pairs]) & ~split
        low_split.append(st["corr"][split].min())
        low_overlap.append(st["overlap"][split].min())
        high_indep.append(np.nanmax(st["corr"][off & (st["overlap"] >= min_overlap)]))
        high_far.append(st["overlap"][off & (st["corr"] >= thr)].max())          # the two cells that share a trace
        assert [6, 7] in pairs and st["corr"][pairs.index([6, 7])] >= thr
        A2, C2 = MR.apply(A, C, pl)
        assert A2.shape == (A.shape[0], 6) and C2.shape == (6, 40) and (A2 >= 0).all() and (C2 >= 0).all()
        for q, g in enumerate(pl["groups"]):
            if len(g) == 1:
                np.testing.assert_array_equal(A2[:, q], A[:, g[0]])
                np.testing.assert_array_equal(C2[q], C[g[0]])
                continue
            truth = cells[MR.PLANTED_CELL_OF[g[0]]]
            halves = [np.corrcoef(C[k], truth)[0, 1] for k in g]
            assert np.corrcoef(C2[q], truth)[0, 1] >= max(halves)
            # the merged footprint has the dominant member's norm and sits between the halves
            assert pl["dominant"][q] in g
            p2 = MR.merged_positions(pos, pl)[q]
            assert np.all(p2 >= pos[g].min(0) - 1e-12) and np.all(p2 <= pos[g].max(0) + 1e-12)
    print(f"depth {depth}: split pairs corr >= {min(low_split):.3f}, overlap >= {min(low_overlap):.3f}; overlapping independent pairs "
          f"corr <= {max(high_indep):.3f}; correlated distant pair overlap <= {max(high_far):.4f}")
    assert max(high_indep) < thr < min(low_split)
    assert max(high_far) < min_overlap < min(low_overlap)


def _stats(pairs, corr, overlap):
    return dict(pairs=np.asarray(pairs), corr=np.asarray(corr, dtype=float), overlap=np.asarray(overlap, dtype=float))


def test_groups_chain_order_and_nan():
    from dnmf_amd import ops
    # 1-4 and 4-2 chain into one group of three; 0, 3, 5 stay single and keep their order; a NaN and a low overlap are no edges
    st = _stats([(1, 4), (2, 4), (0, 3), (3, 5), (0, 5), (0, 0)], [0.9, 0.95, np.nan, 0.99, 0.84, 1.0], [0.5, 0.2, 0.9, 0.05, 0.9, 1.0])
    want = [[0], [1, 2, 4], [3], [5]]
    assert MR.groups_of(st, 6, 0.85, 0.1) == want
    assert ops.merge_groups(st, 6, 0.85, 0.1) == want
    assert ops.merge_group_pairs(want).tolist() == MR.group_pairs(want).tolist() == [[1, 1], [1, 2], [1, 4], [2, 2], [2, 4], [4, 4]]
    assert ops.merge_groups(st, 6, 2.0, 0.1) == [[k] for k in range(6)]
    with pytest.raises(ValueError, match=r"merge_plan.*\(1, 1\)"):
        ops.merge_plan(st, 6, 0.85, 0.1)                                  # S and Q of the group are not among the statistics


@pytest.mark.parametrize("depth", [2, 1])
def test_merge_plan_is_the_restatement(depth):
    from dnmf_amd import ops
    A, C, pos, cells, sz = MR.planted_model(depth, 1)
    # a chain: component 8 copies component 1's neighbourhood, two voxels further along x than component 0 is
    extra = MR.gaussian_footprints(sz, [pos[1] + [1.0, 0.0, 0.0]], MR.SIGMA)
    A, C = np.concatenate([A, extra], 1), np.concatenate([C, 0.5 * C[1:2]], 0)
    boxes = MR.component_boxes(A, sz, 1e-3, 0)
    st = MR.pair_stats(A.T, sz, boxes, C)
    want = MR.merge(A, sz, C)[1]
    assert want["groups"] == [[0, 1, 8], [2, 3], [4], [5], [6], [7]]
    gs = MR.pair_stats(A.T, sz, boxes, C, pairs=ops.merge_group_pairs(want["groups"]).numpy())
    got = ops.merge_plan(st, 9, 0.85, 0.1, iters=10, group_stats=gs)
    assert got["groups"] == want["groups"] and got["merged"] == 2
    assert got["offsets"].tolist() == [0, 3, 5, 6, 7, 8, 9] and got["members"].tolist() == [0, 1, 8, 2, 3, 4, 5, 6, 7]
    assert got["dominant"].tolist() == want["dominant"]
    for name in ("u", "w", "weight"):
        ref = np.concatenate(want[name])
        assert np.abs(got[name] - ref).max() <= 1e-12 * np.abs(ref).max(), name
    assert got["offsets"].dtype == np.int32 and got["members"].dtype == np.int32 and got["u"].dtype == np.float64


def test_negative_traces_are_refused():
    A, C, pos, cells, sz = MR.planted_model(1, 0)
    st, pl = MR.merge(A, sz, C)
    C[1, 7] = -0.25
    with pytest.raises(ValueError, match="negative or non-finite"):
        MR.apply(A, C, pl)
    C[1, 7], C[5, 3] = 0.25, -1.0                                        # a singleton's row is not the merge's business
    MR.apply(A, C, pl)


# ---- the wiring ----------------------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_entries():
    header = open(os.path.join(ROOT, "include", "dnmf_hip.h")).read()
    assert "tests/merge_restatement.py" in header and "csrc/merge_components.hip" in header
    assert "int dnmf_component_pairs(" in header and "int dnmf_merge_apply(" in header
    from dnmf_amd import _lib, build
    assert "merge_components.hip" in build.SOURCES
    vp, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert _lib.SIGNATURES["dnmf_component_pairs"] == (i, [vp, l, vp, vp, vp, i, vp, l, i, vp, vp, i, vp, vp])
    assert _lib.SIGNATURES["dnmf_merge_apply"] == (i, [vp, l, l, i, vp, l, i, vp, vp, vp, vp, i, vp, vp, vp, l, vp, l, vp])
    build.build_library()
    lib = _lib.load()
    assert lib.dnmf_version() == 7 == _lib.ABI_VERSION

    buf = (ctypes.c_double * 4096)()
    base = ctypes.addressof(buf)
    p, q, r = base, base + 8192, base + 16384                             # three areas that do not overlap
    sz = (ctypes.c_int * 3)(6, 5, 2)
    boxes = (ctypes.c_int * 12)(0, 2, 0, 4, 0, 1, 1, 5, 2, 3, 1, 1)
    pairs = (ctypes.c_int * 4)(0, 1, 1, 1)
    B, PR, SZ = ctypes.addressof(boxes), ctypes.addressof(pairs), ctypes.addressof(sz)

    def refused(fn, ok, code, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        rc, msg = getattr(lib, fn)(*a), lib.dnmf_last_error().decode()
        assert rc == code and msg.startswith(fn + ":"), (fn, kw, rc, msg)
        return msg

    fn = "dnmf_component_pairs"
    ok = [p, 60, SZ, B, B, 2, q, 8, 8, PR, PR, 2, r, 0]
    for at in (0, 2, 3, 4, 6, 9, 10, 12):
        refused(fn, ok, -1, **{f"a{at}": 0})
    for at, v in ((5, 0), (8, 0), (11, 0), (1, 59), (7, 7)):
        refused(fn, ok, -2, **{f"a{at}": v})
    for bad in ((0, 2), (0, -1), (1, 2), (1, 7)):                          # (position in pairs, value)
        pp = (ctypes.c_int * 4)(0, 1, 1, 1)
        pp[bad[0]] = bad[1]
        assert "pair" in refused(fn, ok, -2, a9=ctypes.addressof(pp))
    for at, v in ((0, 3), (1, 6), (2, -1), (5, 2), (6, 6), (8, 4)):        # inverted, outside the volume
        bb = (ctypes.c_int * 12)(*boxes)
        bb[at] = v
        assert "box" in refused(fn, ok, -2, a3=ctypes.addressof(bb))
    big_sz = (ctypes.c_int * 3)(64, 65, 1)
    big = (ctypes.c_int * 12)(0, 63, 0, 64, 0, 0, 0, 0, 0, 0, 0, 0)       # 4160 voxels
    assert "4096" in refused(fn, ok, -2, a2=ctypes.addressof(big_sz), a3=ctypes.addressof(big), a1=4160)
    refused(fn, ok, -2, a2=ctypes.addressof((ctypes.c_int * 3)(6, 0, 2)))

    fn = "dnmf_merge_apply"
    offsets, members = (ctypes.c_int * 3)(0, 2, 3), (ctypes.c_int * 3)(0, 2, 1)
    OF, ME = ctypes.addressof(offsets), ctypes.addressof(members)
    # A (10, 3) at p, C (3, 8) at p + 2048, u and w at q, A_out (10, 2) at r, C_out (2, 8) at r + 2048
    ok = [p, 3, 10, 3, p + 2048, 8, 8, OF, ME, OF, ME, 2, q, q, r, 2, r + 2048, 8, 0]
    for at in (0, 4, 7, 8, 9, 10, 12, 13, 14, 16):
        refused(fn, ok, -1, **{f"a{at}": 0})
    for at, v in ((2, 0), (3, 0), (6, 0), (11, 0), (11, 4), (1, 2), (15, 1), (5, 7), (17, 7)):
        refused(fn, ok, -2, **{f"a{at}": v})
    for arr, at, v in ((offsets, 0, 1), (offsets, 1, 0), (offsets, 2, 2), (offsets, 2, 4), (members, 1, 3), (members, 0, -1)):
        cp = (ctypes.c_int * 3)(*arr)
        cp[at] = v
        refused(fn, ok, -2, **{"a7" if arr is offsets else "a8": ctypes.addressof(cp)})
    for kw in (dict(a14=p), dict(a14=p + 4 * 29), dict(a14=p + 2048), dict(a16=p + 2048 + 4 * 23), dict(a16=p), dict(a16=r + 4 * 19),
               dict(a14=r + 2048)):
        assert "overlaps" in refused(fn, ok, -2, **kw)


def test_ops_and_driver_refuse_before_the_gpu():
    import torch
    from dnmf_amd import ops
    from dnmf_amd.Demix import dNMF
    assert ops.MERGE_MAX_K == 4096 and ops.PAIR_SUMS == MR.SUMS
    boxes = torch.tensor([[0, 2, 0, 4, 0, 1], [1, 5, 2, 3, 1, 1], [4, 5, 0, 1, 0, 0], [2, 2, 4, 4, 1, 1]])
    assert ops.candidate_pairs(boxes).tolist() == MR.candidate_pairs(boxes.numpy()).tolist()
    assert [0, 3] in ops.candidate_pairs(boxes).tolist()                   # they share exactly one voxel
    src = inspect.getsource(ops)
    assert "import merge_restatement" not in src and "from merge_restatement" not in src
    sig = inspect.signature(ops.merge_plan).parameters
    assert list(sig)[:5] == ["stats", "K", "thr", "min_overlap", "iters"] and sig["iters"].default == 10
    assert list(inspect.signature(ops.component_pairs).parameters) == ["A_rows", "sz", "boxes", "C", "pairs"]
    params = inspect.signature(dNMF.DeformableNMF.merge_components).parameters
    assert list(params) == ["self", "thr", "min_overlap", "floor", "margin", "traces", "iters", "dry_run"]
    assert params["floor"].default == 1e-3 and params["traces"].default is None and params["dry_run"].default is False
    assert "self.last_merge = None" in inspect.getsource(dNMF.DeformableNMF.__init__)
    doc = dNMF.DeformableNMF.merge_components.__doc__
    assert "0.981" in doc and "0.75" in doc and "0.946" in doc and "0.016" in doc      # the gap the host test measures

    class Two(dNMF.DeformableNMF):
        def _nchan(self):
            return 2
    model = Two.__new__(Two)
    with pytest.raises(NotImplementedError, match="merge_components: one channel only"):
        model.merge_components()
    model = dNMF.DeformableNMF.__new__(dNMF.DeformableNMF)
    model.group = object()
    with pytest.raises(NotImplementedError, match="merge_components.*shard"):
        model.merge_components()
    assert dNMF.MultiChannelDNMF.merge_components is dNMF.DeformableNMF.merge_components
