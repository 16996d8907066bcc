"""New components from the residual (K28) without a GPU: the float64 definition (tests/add_restatement.py) on exact and planted
cases, its edge cases, and the wiring of every layer."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import add_restatement as AR
import detect_restatement as DR
import summary_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exact_rank_one_is_recovered():
    """E = c a^T >= 0: the factor is a at the norm of the start, and it explains everything."""
    rng = np.random.default_rng(2)
    a, c = rng.uniform(0.1, 1.0, 37), rng.uniform(0.0, 2.0, 30)
    a0 = rng.uniform(0.5, 1.0, 37)
    r = AR.rank1_one(np.outer(c, a), a0, iters=5)
    assert r["ok"] == 1 and r["n_valid"] == 30
    want = a * np.linalg.norm(a0) / np.linalg.norm(a)
    assert np.abs(r["a"] - want).max() <= 1e-12 * want.max()
    assert abs(r["explained"] - r["energy"]) <= 1e-12 * r["energy"]
    assert np.abs(np.outer(r["c"], r["a"]) - np.outer(c, a)).max() <= 1e-12 * np.outer(c, a).max()
    assert abs(r["saa"] - (a0 * a0).sum()) <= 1e-12 * (a0 * a0).sum()


def test_agrees_with_the_leading_singular_pair():
    """On non-negative data the leading singular pair is non-negative (Perron-Frobenius), so the clamps never act and the
    alternation is the power iteration."""
    rng = np.random.default_rng(4)
    E = rng.uniform(0.0, 1.0, (25, 18)) + np.outer(rng.uniform(0, 2, 25), rng.uniform(0, 1, 18))
    a0 = np.ones(18)
    r = AR.rank1_one(E, a0, iters=60)
    U, S, Vt = np.linalg.svd(E, full_matrices=False)
    v, u = np.abs(Vt[0]), np.abs(U[:, 0])
    assert np.abs(r["a"] - v * np.linalg.norm(a0)).max() <= 1e-10
    assert np.abs(r["c"] - u * S[0] / np.linalg.norm(a0)).max() <= 1e-10 * S[0]
    assert abs(r["explained"] - S[0] ** 2) <= 1e-10 * S[0] ** 2 and abs(r["energy"] - (S ** 2).sum()) <= 1e-10 * r["energy"]
    # every round explains at least as much as the one before
    ex = [AR.rank1_one(E, a0, iters=k)["explained"] for k in (1, 2, 3, 5)]
    assert all(b >= a - 1e-12 for a, b in zip(ex, ex[1:]))


@pytest.mark.parametrize("depth", [2, 1])
def test_planted_video_learns_the_missing_cells(depth):
    """The figures the default of ``min_explained`` rests on: printed, and recorded in the docstring of ``add_components``."""
    from dnmf_amd.Demix import dNMF
    sig = inspect.signature(dNMF.DeformableNMF.add_components).parameters
    min_explained, image = sig["min_explained"].default, sig["image"].default
    assert (sig["iters"].default, sig["registered"].default, sig["threshold"].default) == (5, 'linear', 0.0)
    cells, nothing, learned, start, trace = [], [], [], [], []
    for seed in range(3):
        video, A6, traces, sz = AR.planted_video(depth, seed)
        assert sz == (24, 20, depth) and video.shape == (40, 24 * 20 * depth) and video.dtype == np.float32
        A4 = A6[:, :4].astype(np.float32)
        C4 = AR.nnls_traces(video, A4).astype(np.float32)
        sub = (A4.astype(np.float64) @ C4.astype(np.float64)).T.astype(np.float32)
        # the residual image the method detects on: the two missing cells are its first two picks, far above the third
        img = SR.summary_images(video.reshape(40, *sz), sub=sub.reshape(40, *sz))[image]
        img = np.where(np.isnan(img), np.nanmedian(img), img)
        det = DR.detect(img.astype(np.float32), 4, AR.SHAPE_STD)
        truth = AR.planted_centres(depth)[list(AR.MISSING)]
        assert det["count"] >= 2
        d = np.linalg.norm(det["positions"][:2, None, :2] - truth[None, :, :2], axis=2)
        assert d.min(1).max() <= 1.0 and sorted(d.argmin(1)) == [0, 1], det["positions"]
        third = det["peaks"][2] if det["count"] > 2 else 0.0
        assert third < 0.1 * det["peaks"][1]
        # the two missing cells and two boxes on nothing, fitted from their true centres
        centres = np.concatenate([truth, AR.planted_centres(depth, AR.NOTHING)])
        fit = AR.add_components(video, sz, A4, C4, centres, AR.SHAPE_STD, min_explained=min_explained)
        assert fit["ok"].tolist() == [1, 1, 1, 1] and fit["kept"].tolist() == [True, True, False, False]
        assert (fit["explained"] <= fit["energy"] * (1 + 1e-12)).all() and (fit["explained"] >= 0).all()
        for q, m in enumerate(AR.MISSING):
            u = AR.box_voxels(fit["boxes"][q], sz)
            learned.append(np.corrcoef(fit["a"][q, :u.size], A6[u, m])[0, 1])
            start.append(np.corrcoef(fit["a0"][q, :u.size], A6[u, m])[0, 1])
            trace.append(np.corrcoef(fit["c"][q], traces[m])[0, 1])
            com = AR.centre_of_mass(fit["a"][q, :u.size], fit["boxes"][q])
            assert np.abs(com[:2] - truth[q, :2]).max() <= 1.0
        cells += fit["ratio"][:2].tolist()
        nothing += fit["ratio"][2:].tolist()
        # the picks of the detection: its first two are kept.  A later, weak pick is kept exactly when its box takes in part of
        # a missing cell (it then scores like the cell: the case left to merge_components, or to ``threshold``); the seed of the
        # GPU fit test is one whose later picks reach neither cell
        pick = AR.add_components(video, sz, A4, C4, det["positions"][:det["count"]], AR.SHAPE_STD, min_explained=min_explained)
        assert pick["kept"][:2].tolist() == [True, True]
        for q in range(2, det["count"]):
            reach = A6[AR.box_voxels(pick["boxes"][q], sz)][:, list(AR.MISSING)].max()
            print(f"depth {depth} seed {seed}: pick {q} at {det['positions'][q].round(1)} reaches {reach:.3f} of a missing cell, "
                  f"explained/energy {pick['ratio'][q]:.3f}")
            assert reach >= 0.1 if pick["kept"][q] else reach < 0.5
        if seed == AR.FIT_SEED[depth]:
            assert det["count"] == 4 and pick["kept"].tolist() == [True, True, False, False], pick["ratio"]
    print(f"\ndepth {depth}: learned footprint corr {min(learned):.3f}-{max(learned):.3f} (Gaussian start {min(start):.3f}-"
          f"{max(start):.3f}), trace corr >= {min(trace):.4f}; explained/energy cells {min(cells):.3f}-{max(cells):.3f}, boxes on "
          f"nothing {min(nothing):.3f}-{max(nothing):.3f}")
    assert min(learned) >= 0.95 and min(trace) >= 0.95 and min(learned) > max(start)
    assert max(nothing) < min_explained < min(cells)


def test_nan_frames_zero_boxes_one_voxel_boxes():
    rng = np.random.default_rng(7)
    sz = (6, 5, 2)
    frames = rng.uniform(0.0, 1.0, (9, 60)).astype(np.float32)
    boxes = AR.candidate_boxes([[0, 0, 0], [5, 4, 1], [3, 2, 1], [2.6, 2.4, 0.2]], sz, [1, 1, 0])
    assert boxes.tolist() == [[0, 1, 0, 1, 0, 0], [4, 5, 3, 4, 1, 1], [2, 4, 1, 3, 1, 1], [2, 4, 1, 3, 0, 0]]     # clipped at two corners
    assert AR.candidate_boxes([[-3.0, 9.0, 0.49]], sz, 0).tolist() == [[0, 0, 4, 4, 0, 0]]                    # one voxel, moved inside
    assert AR.candidate_boxes([[2, 2, 0]], sz, 9).tolist() == [[0, 5, 0, 4, 0, 1]]
    # a NaN in one voxel of one frame: that frame is invalid for the boxes that hold the voxel, and for no other
    p = (3 * 5 + 2) * 2 + 1
    frames[4, p] = np.nan
    frames[6, p] = np.inf
    E = AR.residual_boxes(frames, sz, boxes)
    assert E.shape == (4, 9, 9) and E.dtype == np.float32 and (E[0, :, 4:] == 0).all() and (E[1, :, 4:] == 0).all()
    assert np.array_equal(E[2, :, 4], frames[:, p], equal_nan=True)
    nvox = AR.box_sizes(boxes)
    assert nvox.tolist() == [4, 4, 9, 9]
    fit = AR.rank1_nmf(E, nvox, np.ones((4, 9), dtype=np.float32))
    assert fit["ok"].tolist() == [1, 1, 1, 1] and fit["n_valid"].tolist() == [9, 9, 7, 9]
    assert np.isnan(fit["c"][2]).tolist() == [t in (4, 6) for t in range(9)] and not np.isnan(fit["c"][[0, 1, 3]]).any()
    assert (fit["a"][0, 4:] == 0).all() and np.isfinite(fit["a"]).all()
    # sub given = frames subtracted beforehand, in fp32
    sub = rng.uniform(0.0, 1.0, (9, 60)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(AR.residual_boxes(frames, sz, boxes, sub=sub), AR.residual_boxes(frames - sub, sz, boxes), equal_nan=True)
    # an all-zero box, a box that is <= 0 everywhere, a start of zeros, no valid frame: refused, nothing raised
    zero = np.zeros((9, 4))
    for e, a0 in ((zero, np.ones(4)), (zero - 1.0, np.ones(4)), (zero + 1.0, np.zeros(4)), (zero + np.nan, np.ones(4))):
        r = AR.rank1_one(e, a0)
        assert r["ok"] == 0 and np.isnan(r["a"]).all() and np.isnan(r["c"]).all() and np.isnan(r["explained"])
    assert AR.rank1_one(zero - 1.0, np.ones(4))["energy"] == 36.0 and AR.rank1_one(zero + np.nan, np.ones(4))["n_valid"] == 0
    # a one-voxel box: c is the clamped sample over the start, a the start
    one = AR.rank1_one(np.array([[2.0], [-1.0], [4.0]]), np.array([0.5]))
    assert one["ok"] == 1 and np.allclose(one["a"], [0.5]) and np.allclose(one["c"], [4.0, 0.0, 8.0])
    assert np.isclose(one["energy"], 21.0) and np.isclose(one["explained"], 20.0)


def test_grown_model_arrays():
    depth, sz = 1, (24, 20, 1)
    video, A6, traces, _ = AR.planted_video(depth, 0)
    A4, C4 = A6[:, :4].astype(np.float32), AR.nnls_traces(video, A6[:, :4]).astype(np.float32)
    pos = AR.planted_centres(depth)[:4].astype(np.float32)
    g = np.stack(np.meshgrid(np.arange(24), np.arange(20), np.arange(1), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    D = (1 - np.exp(-0.01 * np.sqrt(((g[:, None, :] - pos[None].astype(np.float64)) ** 2).sum(-1)))).reshape(24, 20, 1, 4)
    centres = np.concatenate([AR.planted_centres(depth)[4:], AR.planted_centres(depth, AR.NOTHING)])
    fit = AR.add_components(video[::2], sz, A4, C4[:, ::2], centres, AR.SHAPE_STD)
    kept = np.nonzero(fit["kept"])[0].tolist()
    assert kept == [0, 1]
    c32 = fit["c"].astype(np.float32)
    c32[1, 3] = np.nan
    new = AR.grown(A4, C4, pos, np.full(4, 3.0), D, sz, fit["boxes"], fit["a"].astype(np.float32), c32, kept, np.arange(0, 40, 2), 3.0)
    assert new["A"].shape == (480, 6) and new["C"].shape == (6, 40) and new["pos"].shape == (6, 3) and new["sigma"].shape == (6,)
    assert new["D"].shape == (24, 20, 1, 6) and new["A"].dtype == np.float32 and new["C"].dtype == np.float32
    assert np.array_equal(new["A"][:, :4], A4) and np.array_equal(new["C"][:4], C4) and np.array_equal(new["D"][..., :4], D)
    assert (new["C"][4:, 1::2] == 0).all() and new["C"][5, 6] == 0 and np.array_equal(new["C"][4, ::2], c32[0])
    u = AR.box_voxels(fit["boxes"][1], sz)
    assert np.array_equal(new["A"][u, 5], fit["a"][1, :u.size].astype(np.float32)) and new["A"][:, 5].sum() == new["A"][u, 5].sum()
    assert np.abs(new["pos"][4:, :2] - AR.planted_centres(depth)[4:, :2]).max() <= 1.0
    at = tuple(np.floor(new["pos"][4] + 0.5).astype(int))
    assert new["D"][at + (4,)] == new["D"][..., 4].min() < 0.01


# ---- the wiring ----------------------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_entries():
    header = open(os.path.join(ROOT, "include", "dnmf_hip.h")).read()
    assert "tests/add_restatement.py" in header and "csrc/add_components.hip" in header
    assert "int dnmf_residual_boxes(" in header and "int dnmf_rank1_nmf(" in header and "size_t dnmf_rank1_nmf_workspace(" in header
    from dnmf_amd import _lib, build
    assert "add_components.hip" in build.SOURCES
    vp, i, l, sz_t = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_size_t
    assert _lib.SIGNATURES["dnmf_residual_boxes"] == (i, [vp, l, vp, l, vp, vp, i, vp, vp, i, vp, i, i, i, vp])
    assert _lib.SIGNATURES["dnmf_rank1_nmf_workspace"] == (sz_t, [i, i])
    assert _lib.SIGNATURES["dnmf_rank1_nmf"] == (i, [vp, i, i, i, vp, vp, i, vp, vp, vp, vp, vp, vp, sz_t, vp])
    build.build_library()
    lib = _lib.load()
    assert lib.dnmf_version() == 7 == _lib.ABI_VERSION

    buf = (ctypes.c_double * 4096)()
    base = ctypes.addressof(buf)
    p, q, r = base, base + 8192, base + 16384
    sz = (ctypes.c_int * 3)(6, 5, 2)
    boxes = (ctypes.c_int * 12)(0, 2, 0, 4, 0, 1, 1, 5, 2, 3, 1, 1)          # 30 and 10 voxels
    B, SZ = ctypes.addressof(boxes), ctypes.addressof(sz)

    def refused(fn, ok, code, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        rc, msg = getattr(lib, fn)(*a), lib.dnmf_last_error().decode()
        assert rc == code and msg.startswith(fn + ":"), (fn, kw, rc, msg)
        return msg

    fn = "dnmf_residual_boxes"
    #     frames ldf sub lds ids sz  B  boxes dev M  E  n  vmax t0 stream
    ok = [p, 60, q, 60, 0, SZ, 4, B, B, 2, r, 8, 30, 2, 0]
    for at in (0, 5, 7, 8, 10):
        refused(fn, ok, -1, **{f"a{at}": 0})
    for at, v in ((6, 0), (9, 0), (11, 0), (12, 0), (13, -1), (13, 5), (1, 59), (3, 59)):
        refused(fn, ok, -2, **{f"a{at}": v})
    assert "vmax=29" in refused(fn, ok, -2, a12=29)                           # the first box holds 30 voxels
    for at, v in ((0, 3), (1, 6), (2, -1), (5, 2), (6, 6), (8, 4)):            # inverted, outside the volume
        bb = (ctypes.c_int * 12)(*boxes)
        bb[at] = v
        assert "box" in refused(fn, ok, -2, a7=ctypes.addressof(bb))
    assert "4096" in refused(fn, ok, -3, a12=4097)
    assert "4096" in refused(fn, ok, -3, a9=4097)
    assert "18432" in refused(fn, ok, -3, a11=18433)
    flat = (ctypes.c_int * 3)(6, 0, 2)                                        # kept alive for the call
    refused(fn, ok, -2, a5=ctypes.addressof(flat))

    assert lib.dnmf_rank1_nmf_workspace(3, 10) == 256 and lib.dnmf_rank1_nmf_workspace(40, 4000) == 40 * 4000 * 8
    for bad in ((0, 10), (3, 0), (4097, 10), (3, 18433)):
        assert lib.dnmf_rank1_nmf_workspace(*bad) == 0
    fn = "dnmf_rank1_nmf"
    #     E  M  n  vmax nvox a0 iters a  c  stats n_valid ok ws bytes stream
    ok = [p, 2, 8, 30, q, q, 5, r, r, r, r, r, q, 256, 0]
    for at in (0, 4, 5, 7, 8, 9, 10, 11, 12):
        refused(fn, ok, -1, **{f"a{at}": 0})
    for at, v in ((1, 0), (2, 0), (3, 0), (6, 0), (6, -2)):
        refused(fn, ok, -2, **{f"a{at}": v})
    assert "4096" in refused(fn, ok, -3, a3=4097)
    assert "4096" in refused(fn, ok, -3, a1=4097)
    assert "18432" in refused(fn, ok, -3, a2=18433)
    refused(fn, ok, -4, a13=255)
    refused(fn, ok, -4, a12=q + 4)


def test_ops_and_driver_refuse_before_the_gpu():
    import torch
    from dnmf_amd import ops
    from dnmf_amd.Demix import dNMF
    assert ops.COMPONENT_MAX_VOXELS == 4096 and ops.ADD_MAX_CANDIDATES == 4096 and ops.ADD_MAX_FRAMES == 18432
    sz = (6, 5, 2)
    centres = [[0, 0, 0], [5, 4, 1], [3, 2, 1], [2.6, 2.4, 0.2], [-3.0, 9.0, 0.49], [2.5, 1.5, 0.5]]
    for half in (0, 1, [1, 1, 0], [9, 0, 2]):
        got = ops.candidate_boxes(torch.tensor(centres), sz, half)
        assert got.dtype == torch.int32 and got.tolist() == AR.candidate_boxes(centres, sz, half).tolist()
    with pytest.raises(ValueError, match="half"):
        ops.candidate_boxes(torch.tensor(centres), sz, -1)
    with pytest.raises(ValueError, match=r"\(M, 3\)"):
        ops.candidate_boxes(torch.zeros(3), sz, 1)
    with pytest.raises(ValueError, match="finite"):
        ops.candidate_boxes(torch.tensor([[0.0, float("nan"), 0.0]]), sz, 1)
    src = inspect.getsource(ops)
    assert "import add_restatement" not in src and "from add_restatement" not in src
    assert list(inspect.signature(ops.candidate_boxes).parameters) == ["centres", "sz", "half"]
    assert list(inspect.signature(ops.residual_boxes).parameters) == ["frames", "sz", "boxes", "sub", "frame_ids", "out", "t0", "n_total"]
    sig = inspect.signature(ops.rank1_nmf).parameters
    assert list(sig) == ["E", "nvox", "a0", "iters", "workspace"] and sig["iters"].default == 5
    params = inspect.signature(dNMF.DeformableNMF.add_components).parameters
    assert list(params) == ["self", "loader", "n", "image", "registered", "shape_std", "half", "min_distance", "threshold", "iters",
                            "min_explained", "centres", "dry_run"]
    assert params["image"].default == 'corr' and params["centres"].default is None and params["dry_run"].default is False
    assert "self.last_add = None" in inspect.getsource(dNMF.DeformableNMF.__init__)
    # select_components ends in the shared tail of every change of the component count, and that tail forgets
    assert "_components_changed(" in inspect.getsource(dNMF.DeformableNMF.select_components)
    assert "_forget_k_shaped()" in inspect.getsource(dNMF.DeformableNMF._components_changed)
    assert "_components_changed(" in inspect.getsource(dNMF.DeformableNMF.add_components)
    doc = dNMF.DeformableNMF.add_components.__doc__
    assert "merge_components" in doc and "tests/test_add_host.py" in doc

    class Loader:
        T = T_total = 40

    class Two(dNMF.DeformableNMF):
        def _nchan(self):
            return 2
    model = Two.__new__(Two)
    with pytest.raises(NotImplementedError, match="add_components: one channel only"):
        model.add_components(Loader(), 2)
    assert dNMF.MultiChannelDNMF.add_components is dNMF.DeformableNMF.add_components
    model = dNMF.DeformableNMF.__new__(dNMF.DeformableNMF)
    model.group = object()
    with pytest.raises(NotImplementedError, match="add_components.*shard"):
        model.add_components(Loader(), 2)
    model.group = None
    shard = Loader()
    shard.T = 20
    with pytest.raises(NotImplementedError, match="add_components.*shard"):
        model.add_components(shard, 2)
    with pytest.raises(ValueError, match="n=0"):
        model.add_components(Loader(), 0)
    with pytest.raises(ValueError, match="image"):
        model.add_components(Loader(), 1, image='median')
