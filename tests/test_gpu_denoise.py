"""K34 (csrc/lowrank_denoise.hip) against its float64 restatement (tests/denoise_restatement.py) at the smallest shapes where the
kernels can go wrong: patches off the stride grid, a patch of 512 voxels (tiles of 16 frames), patches of 1024 voxels (tiles of
8 frames, all four voxel slots of a thread, 128 KiB of LDS; one patch and four overlapping ones), a patch larger than the volume,
frame counts around the tile sizes, every rank path, strided rows, frame_ids, patches that cannot be used, and a movie cut into
pieces.

Bounds.  Both sides run the same algorithm in float64; they differ in the order of the sums (the kernels add the voxels and
the frames one by one with fused multiply-adds, numpy in blocks), so the deviations are rounding amplified by the conditioning
of the Ritz step.  Measured on an MI355X over every case below: |lam - lam'| / lam_0 <= 3.1e-15, |explained - explained'| <=
9.6e-15, kept columns |U - U'| <= 3.5e-15 and |Q - Q'| / sqrt(lam_0) <= 1.2e-15; ten times each is asserted.  (The 1024-voxel
patches alone: lam 2.6e-15, explained 9.6e-15, U 1.1e-15, Q 1.2e-15; the 512-voxel ones: 3.1e-15, 7.7e-15, 1.1e-15, 1.2e-15; the
smaller ones: 1.3e-15, 1.4e-15, 3.5e-15, 6.3e-16.)  The fp32 movie came
out equal in every sample (deviation 0): ten times that is no bound a float64 difference of 1e-15 could keep at a rounding tie,
so the movie is held to one fp32 ulp of its largest value, relative to max|D| -- what one flipped rounding costs."""
import functools

import numpy as np
import pytest
import torch

import denoise_restatement as DN

pytestmark = pytest.mark.gpu

MEASURED = dict(lam=3.1e-15, explained=9.6e-15, U=3.5e-15, Q=1.2e-15)
CASES = {"off-grid": ((20, 18, 1), (8, 8, 1), (4, 4, 0)), "n512": ((24, 20, 2), (16, 16, 2), (8, 8, 0)),
         "whole": ((12, 10, 1), (16, 16, None), (8, 8, 0)), "n1024-one": ((16, 16, 4), (16, 16, None), (8, 8, 0)),
         "n1024": ((24, 20, 4), (16, 16, None), (8, 8, 0))}
# the tiles are 32 frames, 16 for the 512-voxel patch, 8 for the 1024-voxel ones: each +- 1
FRAMES = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 70)


@functools.lru_cache(maxsize=None)
def movie(case, T, seed=0):
    """A background and two blobs of different strength plus unit noise -> rows (T, P) fp32, centre (P,) float64."""
    sz = CASES[case][0]
    rng = np.random.default_rng(1000 * seed + T)
    x, y, z = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sz], indexing="ij")
    t = np.arange(T, dtype=np.float64)
    v = 6.0 * (1.0 + 0.5 * np.sin(0.7 * t))[:, None, None, None] * (1.0 + 0.1 * np.cos(x / 5.0) + 0.05 * z)[None]
    for cx, cy, amp in ((5.0, 6.0, 9.0), (sz[0] - 6.0, sz[1] - 5.0, 14.0)):
        on = (rng.random(T) < 0.5).astype(np.float64)
        v = v + amp * on[:, None, None, None] * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / 8.0)[None]
    rows = (v + rng.standard_normal(v.shape)).astype(np.float32).reshape(T, -1)
    return rows, rows.astype(np.float64).mean(0)


@functools.lru_cache(maxsize=None)
def reference(case, T, R, keep="auto"):
    rows, centre = movie(case, T)
    sz, patch, overlap = CASES[case]
    return DN.denoise(rows, sz, centre, None, patch, overlap, rank=R, keep=keep)


def gpu(rows, sz, centre, scale, patch, overlap, **kw):
    from dnmf_amd import ops
    out, info = ops.lowrank_denoise(torch.from_numpy(np.ascontiguousarray(rows)).cuda(), sz, centre, scale, patch, overlap, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in info.items()}


def deviations(got, ginfo, want, winfo, rows, centre):
    """The integers are equal; -> the five deviations of the docstring."""
    np.testing.assert_array_equal(ginfo["ok"], winfo["ok"])
    np.testing.assert_array_equal(ginfo["kept"], winfo["kept"])
    np.testing.assert_array_equal(np.abs(ginfo["U"]).max(1) == 0, np.abs(winfo["U"]).max(1) == 0)      # the zero columns
    np.testing.assert_array_equal(ginfo["plan"]["boxes"], winfo["plan"]["boxes"])
    dev = dict(lam=0.0, explained=0.0, U=0.0, Q=0.0)
    for p in np.flatnonzero(winfo["ok"]):
        k, l0 = winfo["kept"][p], max(winfo["lam"][p][0], 1e-300)
        dev["lam"] = max(dev["lam"], np.max(np.abs(ginfo["lam"][p] - winfo["lam"][p])) / l0)
        dev["explained"] = max(dev["explained"], abs(ginfo["explained"][p] - winfo["explained"][p]))
        if k:
            dev["U"] = max(dev["U"], np.max(np.abs(ginfo["U"][p][:, :k] - winfo["U"][p][:, :k])))
            dev["Q"] = max(dev["Q"], np.max(np.abs(ginfo["Q"][p][:, :k] - winfo["Q"][p][:, :k])) / np.sqrt(l0))
    dmax = max(float(np.max(np.abs(rows.astype(np.float64) - centre))), 1.0)
    dev["movie"] = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)))) / dmax
    dev["ulp"] = float(np.spacing(np.float32(np.max(np.abs(want))))) / dmax
    return dev


def check(dev, what):
    print(what, {k: f"{v:.2e}" for k, v in dev.items()})
    for k, bound in MEASURED.items():
        assert dev[k] <= 10 * bound, (what, k, dev[k])
    assert dev["movie"] <= dev["ulp"], (what, dev["movie"], dev["ulp"])


@pytest.mark.parametrize("R", [1, 4, 8])
@pytest.mark.parametrize("case", list(CASES))
def test_against_the_restatement(case, R):
    sz, patch, overlap = CASES[case]
    worst = dict.fromkeys((*MEASURED, 'movie', 'ulp'), 0.0)
    kept = set()
    for T in FRAMES:
        rows, centre = movie(case, T)
        want, winfo = reference(case, T, R)
        got, ginfo = gpu(rows, sz, centre, None, patch, overlap, rank=R)
        dev = deviations(got, ginfo, want, winfo, rows, centre)
        assert dev["movie"] <= dev["ulp"], (T, dev)
        worst = {k: max(worst[k], dev[k]) for k in dev}
        kept |= set(winfo["kept"].tolist())
    assert max(kept) >= 1 and 0 in kept                  # T = 1 keeps nothing (D = 0); the long movies keep what is planted
    check(worst, f"{case} R={R}")


@pytest.mark.parametrize("case", list(CASES))
def test_fixed_keep_and_few_frames(case):
    """keep=r, and T < R: columns beyond the rank of D are zero on both sides."""
    sz, patch, overlap = CASES[case]
    worst = dict.fromkeys((*MEASURED, 'movie', 'ulp'), 0.0)
    for T in (2, 7, 33):
        rows, centre = movie(case, T)
        want, winfo = reference(case, T, 8, keep=3)
        got, ginfo = gpu(rows, sz, centre, None, patch, overlap, rank=8, keep=3)
        assert (winfo["kept"] <= min(3, T)).all()
        dev = deviations(got, ginfo, want, winfo, rows, centre)
        assert dev["movie"] <= dev["ulp"], (T, dev)
        worst = {k: max(worst[k], dev[k]) for k in dev}
    check(worst, f"{case} keep=3")


def test_strided_rows_and_frame_ids():
    from dnmf_amd import ops
    case, T, R = "off-grid", 33, 4
    sz, patch, overlap = CASES[case]
    rows, centre = movie(case, T)
    P = rows.shape[1]
    plain, pinfo = gpu(rows, sz, centre, None, patch, overlap, rank=R)
    rng = np.random.default_rng(0)
    perm = rng.permutation(T + 3)[:T]
    buf = torch.full((T + 3, P + 5), float("nan"), device="cuda")
    buf[torch.from_numpy(perm).cuda(), :P] = torch.from_numpy(rows).cuda()
    plan = ops.lowrank_patch_plan(sz, patch, overlap)
    state = ops.lowrank_state(plan, R, T)
    for _ in range(4):
        ops.lowrank_accumulate(buf, sz, plan, state, centre.reshape(sz), None, frame_ids=perm)
        ops.lowrank_orthonormalise(state)
    ops.lowrank_project(buf, sz, plan, state, centre.reshape(sz), None, frame_ids=perm)
    ops.lowrank_ritz(state)
    out = torch.full((T, P + 7), -1.0, device="cuda")
    got = ops.lowrank_reconstruct(buf, sz, plan, state, centre.reshape(sz), None, frame_ids=perm, out=out)
    assert (got.cpu().numpy().view(np.int32) == plain.view(np.int32)).all() and bool((out[:, P:] == -1.0).all())
    for k in ("U", "Q", "lam", "explained", "kept", "ok"):
        assert np.array_equal(state[k].cpu().numpy(), pinfo[k]), k
    assert int(state["ok"].min()) == 1                     # the NaN padding and the unused rows were never read


def test_unusable_patches_pass_through():
    case, T, R = "off-grid", 17, 4
    sz, patch, overlap = CASES[case]
    rows, centre = movie(case, T)
    bad = rows.copy()
    bad[4, 0] = np.nan                                      # the corner voxel: patch 0 alone
    bad[9, 9 * 18 + 9] = np.inf                             # an interior voxel: four patches
    scale = np.ones(sz)
    scale[19, 17, 0] = 0.0                                  # the opposite corner: the last patch alone
    want, winfo = DN.denoise(bad, sz, centre, scale, patch, overlap, rank=R)
    got, ginfo = gpu(bad, sz, centre, scale, patch, overlap, rank=R)
    assert np.flatnonzero(winfo["ok"] == 0).tolist() == [0, 5, 6, 9, 10, 15]
    finite = np.isfinite(bad)
    dev = deviations(np.where(finite, got, 0), ginfo, np.where(finite, want, 0), winfo, np.where(finite, bad, 0), centre)
    check(dev, "unusable patches")
    through = [0, 9 * 18 + 9, 19 * 18 + 17, 3 * 18 + 3]     # voxels only unusable patches hold
    assert (got[:, through].view(np.int32) == bad[:, through].view(np.int32)).all()
    assert (got.view(np.int32) == want.view(np.int32))[~finite].all()
    assert (ginfo["lam"][winfo["ok"] == 0] == 0).all() and (ginfo["U"][winfo["ok"] == 0] == 0).all()


def test_constant_movie_bit_for_bit():
    sz, patch, overlap = CASES["off-grid"]
    rows = np.full((9, 360), 3.7, dtype=np.float32)
    centre = rows.astype(np.float64).mean(0)
    for scale in (None, np.zeros(sz)):
        got, info = gpu(rows, sz, centre, scale, patch, overlap)
        assert (got.view(np.int32) == rows.view(np.int32)).all() and (info["kept"] == 0).all()
        assert (info["ok"] == (1 if scale is None else 0)).all()


@pytest.mark.parametrize("case", ["off-grid", "n512", "n1024"])
def test_same_bits_on_every_run_and_for_every_cut(case):
    sz, patch, overlap = CASES[case]
    rows, centre = movie(case, 70)
    one, info = gpu(rows, sz, centre, None, patch, overlap)
    again, ainfo = gpu(rows, sz, centre, None, patch, overlap)
    assert (one.view(np.int32) == again.view(np.int32)).all()
    for limit in (1, 7, 8, 9, 31, 32, 33):
        cut, cinfo = gpu(rows, sz, centre, None, patch, overlap, limit=limit)
        assert (cut.view(np.int32) == one.view(np.int32)).all(), limit
        for k in ("U", "Q", "lam", "explained", "kept", "ok"):
            assert np.array_equal(cinfo[k], info[k]) and np.array_equal(ainfo[k], info[k]), (limit, k)


def test_refusals():
    from dnmf_amd import ops
    sz, patch, overlap = CASES["off-grid"]
    rows, centre = movie("off-grid", 7)
    fr = torch.from_numpy(rows).cuda()
    with pytest.raises(ValueError):
        ops.lowrank_denoise(fr, sz, centre, rank=9)
    with pytest.raises(ValueError):
        ops.lowrank_denoise(fr, sz, centre, iters=0)
    with pytest.raises(ValueError):
        ops.lowrank_denoise(fr, sz, centre, overlap=(16, 8, 0))
    with pytest.raises(ValueError):
        ops.lowrank_denoise(fr, sz, centre[:-1])
    with pytest.raises(ValueError):
        ops.lowrank_denoise(fr, sz, centre, keep="most")
    # the library's own refusals, on real allocations: nothing is launched and the state stays as it was
    import ctypes
    from dnmf_amd import _lib
    lib = _lib.load()
    plan = ops.lowrank_patch_plan(sz, patch, overlap)
    state = ops.lowrank_state(plan, 8, 7)
    torch.cuda.synchronize()
    before = {k: state[k].clone() for k in ("U", "W", "Q", "energy", "lam", "kept", "ok", "explained")}
    c = torch.from_numpy(centre).cuda()
    out = torch.zeros_like(fr)
    plan9, isz = ops._lowrank_plan(plan)[0], (ctypes.c_int * 3)(*sz)
    f, cp, U, W, Q, E, ok, lam, kept, ex = (t.data_ptr() for t in (fr, c, state["U"], state["W"], state["Q"], state["energy"], state["ok"],
                                                                state["lam"], state["kept"], state["explained"]))
    assert lib.dnmf_lowrank_accumulate(f, 360, None, isz, 7, plan9, 9, cp, None, U, W, ok, None) < 0                     # rank
    assert lib.dnmf_lowrank_accumulate(f, 359, None, isz, 7, plan9, 8, cp, None, U, W, ok, None) < 0                     # ldf < P
    assert lib.dnmf_lowrank_accumulate(None, 360, None, isz, 7, plan9, 8, cp, None, U, W, ok, None) < 0                  # NULL
    assert lib.dnmf_lowrank_project(f, 360, None, isz, 7, 1, 7, plan9, 8, cp, None, U, Q, E, ok, None) < 0               # rows past T
    assert lib.dnmf_lowrank_ritz(16, 64, 7, 8, -1, -1.0, 10, U, Q, E, ok, lam, kept, ex, None) < 0                       # no edge
    assert lib.dnmf_lowrank_ritz(16, 64, 7, 8, 2, 0.0, 65, U, Q, E, ok, lam, kept, ex, None) < 0                         # sweeps
    assert lib.dnmf_lowrank_reconstruct(f, 360, None, isz, 7, 0, 7, plan9, 8, cp, None, U, Q, kept, ok, out.data_ptr(), 359, None) < 0
    assert lib.dnmf_lowrank_orthonormalise(16, 1025, 8, U, W, ok, None) < 0
    torch.cuda.synchronize()
    assert all(torch.equal(state[k], v) for k, v in before.items()) and not bool(out.any())
