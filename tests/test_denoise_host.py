"""The restatement of K34 (tests/denoise_restatement.py) pinned against ``np.linalg.svd`` per patch, the patch plan of ``ops`` and
of the library against it, the effect on the planted movie, the exactness cases and the refusals.  No GPU."""
import ctypes
import functools

import numpy as np
import pytest

import denoise_restatement as DN


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


def plan9(plan):
    return (ctypes.c_int * 9)(*[v for a in range(3) for v in (plan["counts"][a], plan["strides"][a], plan["shape"][a])])


def test_patch_plan(lib):
    from dnmf_amd import ops
    # extents on (x) and off (y) the stride grid
    p = ops.lowrank_patch_plan((20, 18, 1), (8, 8, 1), (4, 4, 0))
    assert [s.tolist() for s in p["starts"]] == [[0, 4, 8, 12], [0, 4, 8, 10], [0]]
    assert p["counts"] == (4, 4, 1) and p["shape"] == (8, 8, 1) and p["n"] == 64 and p["boxes"].dtype == np.int32
    assert p["boxes"][0].tolist() == [0, 7, 0, 7, 0, 0] and p["boxes"][3].tolist() == [0, 7, 10, 17, 0, 0]      # x slowest
    assert p["boxes"][-1].tolist() == [12, 19, 10, 17, 0, 0]
    # a patch larger than the volume is the volume
    p = ops.lowrank_patch_plan((12, 10, 1), (16, 16, None))
    assert p["boxes"].tolist() == [[0, 11, 0, 9, 0, 0]] and p["n"] == 120 and p["shape"] == (12, 10, 1)
    # Z = 2 with a z patch of 2 and of 1; None is min(Z, 4)
    assert ops.lowrank_patch_plan((24, 20, 2), (16, 16, 2))["boxes"][:, 4:].tolist() == [[0, 1]] * 4
    assert ops.lowrank_patch_plan((24, 20, 2), (16, 16, 1))["boxes"][:, 4:].tolist() == [[0, 0], [1, 1]] * 4
    assert ops.lowrank_patch_plan((24, 20, 2))["shape"] == (16, 16, 2) and ops.lowrank_patch_plan((24, 20, 9))["shape"] == (16, 16, 4)
    # a patch is never cut
    for bad in (dict(patch=(32, 33, 1)), dict(patch=(16, 16, 5)), dict(overlap=(16, 8, 0)), dict(overlap=(-1, 8, 0)), dict(patch=(0, 16, 1))):
        with pytest.raises(ValueError):
            ops.lowrank_patch_plan((64, 64, 8), **bad)
        with pytest.raises(ValueError):
            DN.patch_plan((64, 64, 8), **{"patch": (16, 16, None), "overlap": (8, 8, 0), **bad})
    # ops, the restatement and the library agree; every voxel is covered and every patch has the plan's shape
    n = 0
    for sz in ((20, 18, 1), (12, 10, 1), (24, 20, 2), (40, 36, 2), (17, 33, 5), (1, 1, 1)):
        for patch, overlap in (((16, 16, None), (8, 8, 0)), ((8, 8, 1), (4, 4, 0)), ((5, 7, 2), (4, 1, 1)), ((16, 16, 2), (12, 0, 1))):
            a, b = ops.lowrank_patch_plan(sz, patch, overlap), DN.patch_plan(sz, patch, overlap)
            np.testing.assert_array_equal(a["boxes"], b["boxes"])
            assert a["counts"] == b["counts"] and a["shape"] == b["shape"] and a["n"] == b["n"] and a["strides"] == b["strides"]
            assert lib.dnmf_lowrank_patches((ctypes.c_int * 3)(*sz), plan9(a)) == len(a["boxes"])
            covered = np.zeros(sz, dtype=bool)
            for x0, x1, y0, y1, z0, z1 in a["boxes"]:
                assert (x1 - x0 + 1, y1 - y0 + 1, z1 - z0 + 1) == a["shape"] and x0 >= 0 and x1 < sz[0] and y1 < sz[1] and z1 < sz[2]
                covered[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1] = True
            assert covered.all()
            n += 1
    assert n == 24


def test_library_refuses_without_a_gpu(lib):
    from dnmf_amd import ops
    sz = (ctypes.c_int * 3)(20, 18, 1)
    good = plan9(ops.lowrank_patch_plan((20, 18, 1), (8, 8, 1), (4, 4, 0)))
    assert lib.dnmf_lowrank_patches(sz, good) == 16
    for at, v in ((0, 3), (0, 5), (1, 9), (2, 21), (2, 0), (3, 0)):      # too few patches, one too many, a gap, a patch beyond the axis
        bad = (ctypes.c_int * 9)(*good)
        bad[at] = v
        assert lib.dnmf_lowrank_patches(sz, bad) == 0, (at, v)
    assert lib.dnmf_lowrank_patches((ctypes.c_int * 3)(64, 64, 1), (ctypes.c_int * 9)(2, 32, 33, 2, 31, 33, 1, 1, 1)) == 0     # n > 1024
    assert b"1024" in lib.dnmf_last_error()
    assert [lib.dnmf_lowrank_tile_frames(n) for n in (0, 1, 256, 257, 512, 513, 1024, 1025)] == [0, 32, 32, 16, 16, 8, 8, 0]
    import torch
    if torch.cuda.is_available():      # with a device the launching entries are refused on real allocations: tests/test_gpu_denoise.py
        return
    one = 1 << 4      # a pointer that is never followed: every check comes first, and without a device nothing could be launched
    assert lib.dnmf_lowrank_accumulate(one, 360, None, sz, 4, good, 9, one, None, one, one, one, None) < 0          # rank
    assert lib.dnmf_lowrank_accumulate(one, 359, None, sz, 4, good, 8, one, None, one, one, one, None) < 0          # ldf < P
    assert lib.dnmf_lowrank_accumulate(None, 360, None, sz, 4, good, 8, one, None, one, one, one, None) < 0         # NULL
    assert lib.dnmf_lowrank_project(one, 360, None, sz, 4, 5, 8, good, 8, one, None, one, one, one, one, None) < 0  # rows past T
    assert lib.dnmf_lowrank_ritz(16, 64, 8, 8, -1, -1.0, 10, one, one, one, one, one, one, one, None) < 0            # no edge
    assert lib.dnmf_lowrank_ritz(16, 64, 8, 8, 2, 0.0, 65, one, one, one, one, one, one, one, None) < 0              # sweeps
    assert lib.dnmf_lowrank_reconstruct(one, 360, None, sz, 4, 0, 4, good, 8, one, None, one, one, one, one, one, 359, None) < 0
    assert lib.dnmf_lowrank_orthonormalise(16, 1025, 8, one, one, one, None) < 0


@functools.lru_cache(maxsize=None)
def planted(Z, seed):
    noisy, clean = DN.planted_video(Z, seed)
    T = noisy.shape[0]
    rows = noisy.reshape(T, -1)
    return rows, clean.reshape(T, -1), noisy.shape[1:], rows.astype(np.float64).mean(0)


# The top singular value of n x T unit noise sits at (0.99 +- 0.013) (sqrt n + sqrt T) for these n and T (Tracy-Widom), so among
# the 16 patches of a movie some cross the edge of threshold = 1: no choice of the planted amplitudes puts "the next one" safely
# below sqrt n + sqrt T itself.  The comparison therefore runs at threshold = 1.1; the test checks with the SVD that the planted
# values are above 2 x and the next one below 1.05 x (sqrt n + sqrt T) (measured: at least 5.1 x, at most 1.010 x).
SVD_THRESHOLD = 1.1
LAM_MEASURED, PROJ_MEASURED = 4.1e-14, 4.8e-8


@pytest.mark.parametrize("Z", [1, 2])
def test_restatement_against_svd(Z):
    """iters = 4 against the exact SVD of every patch.  Measured on the development machine, Z = 1 / 2: |lam - s^2| / s_0^2 at
    most 4.05e-14 / 4.3e-15 over the kept columns, the projector U U^T off by at most 4.72e-8 / 1.09e-8 in any entry (four
    iterations leave (s_noise / s_kept)^8 of the noise directions in a kept column); ten times the larger figure is asserted."""
    rows, _, sz, centre = planted(Z, 0)
    T = rows.shape[0]
    out, info = DN.denoise(rows, sz, centre, None, threshold=SVD_THRESHOLD)
    plan = info["plan"]
    n = plan["n"]
    assert n == 256 * Z and len(plan["boxes"]) == 16
    bare, e = np.sqrt(n) + np.sqrt(T), np.sqrt(DN.edge(n, T, SVD_THRESHOLD))
    lam_dev = proj_dev = 0.0
    planted_counts = set()
    for p, box in enumerate(plan["boxes"]):
        idx = DN.patch_voxels(box, sz)
        D = rows[:, idx].astype(np.float64).T - centre[idx][:, None]
        u, s, _ = np.linalg.svd(D, full_matrices=False)
        k = int(np.sum(s > e))
        assert 1 <= k <= 3 and s[k - 1] > 2.0 * bare and s[k] < 1.05 * bare, (p, s[:5] / bare)
        assert info["kept"][p] == k and info["ok"][p] == 1
        planted_counts.add(k)
        U = info["U"][p][:, :k]
        lam_dev = max(lam_dev, float(np.max(np.abs(info["lam"][p][:k] - s[:k] ** 2)) / s[0] ** 2))
        proj_dev = max(proj_dev, float(np.max(np.abs(U @ U.T - u[:, :k] @ u[:, :k].T))))
        assert abs(info["explained"][p] - np.sum(s[:k] ** 2) / np.sum(s ** 2)) < 1e-9
    print(f"Z={Z}: lam deviation {lam_dev:.3e}, projector deviation {proj_dev:.3e}, kept counts {sorted(planted_counts)}")
    assert planted_counts == {1, 2, 3}
    assert lam_dev <= 10 * LAM_MEASURED and proj_dev <= 10 * PROJ_MEASURED


@pytest.mark.parametrize("Z", [1, 2])
def test_default_edge_against_svd_where_it_is_clear(Z):
    """threshold = 1, the default: over the patches whose singular values have no member within 3 % of sqrt n + sqrt T -- checked
    with the SVD here -- ``kept`` is the SVD's count above the edge.  (A Ritz value never exceeds the singular value it
    approximates, so a noise value below 0.97 of the edge stays below it however far four iterations have come.)"""
    clear = total = 0
    for seed in (0, 1, 2):
        rows, _, sz, centre = planted(Z, seed)
        T = rows.shape[0]
        out, info = DN.denoise(rows, sz, centre, None)
        plan = info["plan"]
        bare = np.sqrt(plan["n"]) + np.sqrt(T)
        assert DN.edge(plan["n"], T) == bare ** 2
        for p, box in enumerate(plan["boxes"]):
            idx = DN.patch_voxels(box, sz)
            s = np.linalg.svd(rows[:, idx].astype(np.float64).T - centre[idx][:, None], compute_uv=False)
            total += 1
            if np.any(np.abs(s / bare - 1.0) <= 0.03):
                continue
            clear += 1
            assert info["kept"][p] == int(np.sum(s > bare)), (seed, p, s[:5] / bare)
    print(f"Z={Z}: {clear} of {total} patches have no singular value within 3 % of the edge")
    assert clear >= 1                      # measured: 15 of 48 at Z = 1, 3 of 48 at Z = 2 -- the comparison is not empty


# mse(raw) / mse(denoised) against the noise-free planted movie, defaults (threshold 1, scale None), measured:
#            seed 0   seed 1   seed 2
#   Z = 1    36.3     37.1     36.8
#   Z = 2    41.8     41.2     41.4
GAIN_MEASURED_MIN = 36.3


@pytest.mark.parametrize("Z", [1, 2])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_denoising_lowers_the_error(Z, seed):
    rows, clean, sz, centre = planted(Z, seed)
    out, info = DN.denoise(rows, sz, centre, None)
    raw, den = np.mean((rows - clean) ** 2), np.mean((out - clean) ** 2)
    print(f"Z={Z} seed={seed}: mse raw {raw:.4f} denoised {den:.4f} gain {raw / den:.2f}")
    assert den < raw and raw / den >= 0.5 * GAIN_MEASURED_MIN


def test_constant_movie_comes_back_bit_for_bit():
    rows = np.full((9, 20 * 18), 3.7, dtype=np.float32)
    for scale in (None, np.zeros((20, 18, 1))):      # unit scale: D = 0, nothing kept; zero noise: no patch is usable
        out, info = DN.denoise(rows, (20, 18, 1), rows.astype(np.float64).mean(0), scale, (8, 8, 1), (4, 4, 0))
        assert (out.view(np.int32) == rows.view(np.int32)).all() and (info["kept"] == 0).all()
        assert (info["ok"] == (0 if scale is not None else 1)).all() and (info["U"] == 0).all()


def test_exact_rank_two_movie_within_one_ulp():
    rng = np.random.default_rng(5)
    T, sz = 40, (20, 18, 1)
    # dyadic factors: their products are fp32 values, so the fp32 movie is rank 2 exactly, not up to 2^-24
    a, f = np.round((rng.random((2, 360)) + 0.5) * 64) / 64, np.round((rng.random((T, 2)) + 0.5) * 64) / 64
    rows = (f @ a).astype(np.float32)
    exact = f @ a
    assert (rows.astype(np.float64) == exact).all()
    out, info = DN.denoise(rows, sz, np.zeros(sz), None, (8, 8, 1), (4, 4, 0), keep=2)
    assert (info["kept"] == 2).all()
    ulp = np.spacing(np.abs(rows))
    assert (np.abs(out.astype(np.float64) - exact) <= ulp).all()
    assert np.all(info["lam"][:, 2:] < 1e-20 * info["lam"][:, :1])


def test_nan_sample_marks_exactly_the_covering_patches():
    rng = np.random.default_rng(2)
    sz, T = (20, 18, 1), 12
    rows = rng.standard_normal((T, 360)).astype(np.float32) + np.linspace(0, 8, T, dtype=np.float32)[:, None]
    centre = rows.astype(np.float64).mean(0)
    plan = DN.patch_plan(sz, (8, 8, 1), (4, 4, 0))

    def covering(x, y):
        return [p for p, b in enumerate(plan["boxes"]) if b[0] <= x <= b[1] and b[2] <= y <= b[3]]
    # a corner voxel has one patch: it and every voxel only that patch covers pass through
    bad = rows.copy()
    bad[3, 0 * 18 + 0] = np.nan
    out, info = DN.denoise(bad, sz, centre, None, (8, 8, 1), (4, 4, 0), keep=1)
    assert covering(0, 0) == [0] and np.flatnonzero(info["ok"] == 0).tolist() == [0]
    alone = [x * 18 + y for x in range(4) for y in range(4)]
    assert (out[:, alone].view(np.int32) == bad[:, alone].view(np.int32)).all()
    others = np.setdiff1d(np.arange(360), alone)
    assert np.isfinite(out[:, others]).all() and (out[:, others] != bad[:, others]).any()
    # an interior voxel has four; the NaN is in patches that overlap others everywhere, so every voxel is still denoised
    bad = rows.copy()
    bad[5, 9 * 18 + 9] = np.inf
    out, info = DN.denoise(bad, sz, centre, None, (8, 8, 1), (4, 4, 0), keep=1)
    assert np.flatnonzero(info["ok"] == 0).tolist() == covering(9, 9) and len(covering(9, 9)) == 4
    cover_count = np.zeros(sz[:2], int)
    for p, b in enumerate(plan["boxes"]):
        cover_count[b[0]:b[1] + 1, b[2]:b[3] + 1] += info["ok"][p]
    lost = np.flatnonzero(cover_count.ravel() == 0)
    assert 9 * 18 + 9 in lost                                        # all four of its patches are out: it passes through
    assert (out[:, lost].view(np.int32) == bad[:, lost].view(np.int32)).all()
    kept = np.flatnonzero(cover_count.ravel() > 0)
    assert np.isfinite(out[:, kept]).all()
    # a voxel with a NaN that another usable patch covers does not exist (a patch that holds it is out): but its neighbour in a
    # patch without the NaN is denoised from that patch alone
    assert cover_count[5, 9] > 0 and cover_count[5, 9] < len(covering(5, 9))


def test_fewer_frames_than_columns():
    rng = np.random.default_rng(3)
    for T in (1, 2, 5):
        rows = rng.standard_normal((T, 360)).astype(np.float32)
        out, info = DN.denoise(rows, (20, 18, 1), np.zeros(360), None, (8, 8, 1), (4, 4, 0), rank=8, keep=8)
        assert (info["kept"] <= T).all() and (info["kept"] >= 1).all()
        zero_cols = (np.abs(info["U"]).max(1) == 0).sum(1)
        assert (zero_cols >= 8 - T).all() and (info["lam"][:, T:] == 0).all()
