"""K7 (``dnmf_image_iwarp``, csrc/image_iwarp.hip) held to a float64 brute force, lattice point by lattice point, over the warp
families of tests/iwarp_restatement.py (pinned without a GPU by tests/test_iwarp_restatement_host.py).

The frames hold the voxel index (exact below 2^24), so the registered frame IS the voxel K7 chose.  For every frame of every
case, every lattice point is checked twice, none left out:

  (a) against ``nearest64`` on the fp32 positions of the K1 grid, scaled as the reference scales it (Demix/dNMF.py:81-83): the
      same voxel, or else a d2 (float64, on those positions) within NEAR_TIE = 1e-6 of the minimum -- the bound the project uses
      between K7, K10 and scipy;
  (b) against ``positions64`` alone, no project kernel in the reference: d2(chosen) <= d2_min + margin, margin =
      2 (2 sqrt(d2_min) delta + delta^2), delta = 4 delta_0.  The factor 4 covers the kernel's other fp32 order (the division
      shortcut, the fused multiply-adds).  A missed neighbour is off by the spacing of d2 between adjacent voxels, 1e-2 to 1.

A d2 without a finite value counts as +inf on both sides (an axis of one voxel along x or y: the reference's 0 / 0; every point
then takes voxel 0), which is why (b) is written as a comparison and not as a difference.

Every case also asserts window search == exhaustive search bit for bit, ``count`` == 0 for the mild entries (identity, rotate
2, shear, the smallest bend), == B P for ``fold`` and for the thin volumes (hk is infinite: every point is marked), and the
condition on the inputs of (a): except under ``identity`` (the designed tie case, see iwarp_restatement) fewer than 1 % of the
lattice points of a frame have their two best float64 distances within 1e-6.

Figures (MI355X, the product library; the test prints them per frame):
  delta_0 = 6.6e-5 voxels measured by the host test, DELTA0 = 8e-5 used, delta = 3.2e-4.
  Largest margin that occurs: 0.098 (rotate 30 at 20x300x1, a lattice point 76 voxels from the nearest warped voxel -- the margin
  grows with the distance); over the lattice points with d2_min < 1 it is 1.28e-3.
  (a): the chosen voxel equals the brute force's at every lattice point of every frame -- no tie proof was needed.
  (b): the largest d2(chosen) - d2_min is 1.4e-4 (bend 0.998 at 20x300x1), the largest share of its margin 0.0056 (shear at
  20x300x1, 8.8e-5).
  Near-tie share per frame: 0 in every frame of shift, rotate, zoom, shear, tilt, bend, fold, mirror and mixed at every volume
  and of nearfold at 20x300x1, 18x70x5 and 33x40x2; nearfold at 64x64x1 0.05 % (above) and 0.10 % (below): the lattice points on
  the compressed band.  identity: 3.1 % (64x64x1), 5.3 % (20x300x1), 6.9 % (18x70x5), 51.3 % (33x40x2), 0 on the thin volumes (no
  finite distance).
  Against a library built with -DDNMF_IW_NOBOX (the cell only, never the box): (a) and (b) both fail for zoom 0.7, every shift
  of 12.4 voxels and nearfold above at all four full volumes, and for rotate 30, shear, bend 0.5 (not at 33x40x2), mirror and
  at least one mixed entry; identity, the pure shifts, rotate 2, tilt, bend 0.05, fold and nearfold below (every point already
  goes to the exhaustive kernel) pass, as do the thin volumes (the one-point-per-thread kernel has no such switch).
"""
import numpy as np
import pytest
import torch

import iwarp_restatement as IR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def cuda(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


def index_frames(B, P):
    assert P < 2 ** 24
    return torch.arange(P, device="cuda", dtype=torch.float32).repeat(B, 1)


def k1_positions(ops, sz, beta, times):
    """(B, P, 3) fp32: the K1 grid scaled by sz like the reference's flow_."""
    B, P = len(times), int(np.prod(sz))
    _, grid = ops.warp_gather(torch.zeros((*sz, 1), device="cuda"), beta, times, want_A_t=False)
    szt = torch.tensor([float(s) for s in sz], device="cuda")
    flow = ((grid + 1) / 2) * szt[None, None, None, :, None]
    return flow.permute(4, 0, 1, 2, 3).reshape(B, P, 3).contiguous()


def check_frame(chosen, pts32, p64, lat):
    """Checks (a) and (b) of one frame: dict of counts and figures."""
    ia, best_a, _ = IR.nearest64_torch(pts32, lat)
    da = IR.chosen_d2(pts32.double(), lat, chosen)
    bad_a = (chosen != ia) & ~(da <= best_a + IR.NEAR_TIE)
    _, best_b, second_b = IR.nearest64_torch(p64, lat)
    db = IR.chosen_d2(p64, lat, chosen)
    mg = IR.margin(best_b)
    bad_b = ~(db <= best_b + mg)
    fin = torch.isfinite(best_b)
    excess = torch.where(fin, db - best_b, torch.zeros_like(db))
    return {"differ": int((chosen != ia).sum()), "bad_a": int(bad_a.sum()), "bad_b": int(bad_b.sum()),
            "worst_a": float(torch.where(torch.isfinite(best_a), da - best_a, torch.zeros_like(da)).max()),
            "worst_b": float(excess.max()), "ratio_b": float((excess / mg.clamp_min(1e-300)).max()),
            "margin": float(torch.where(fin, mg, torch.zeros_like(mg)).max()),
            "margin_inside": float(torch.where(fin & (best_b < 1), mg, torch.zeros_like(mg)).max()),
            "ties": IR.tie_share(best_b, second_b)}


@pytest.mark.parametrize("c", IR.cases(), ids=IR.case_id)
def test_every_lattice_point_against_float64(ops, c):
    sz, kind = c
    labels, beta_np = IR.case(sz, kind)
    B, P = len(labels), int(np.prod(sz))
    beta, times = cuda(beta_np), list(range(B))
    vals = index_frames(B, P)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    win = ops.image_iwarp(vals, None, sz, beta, times, count=count)
    full = ops.image_iwarp(vals, None, sz, beta, times, exhaustive=True)
    pts = k1_positions(ops, sz, beta, times)
    lat = cuda(IR.lattice64(sz))
    problems = []
    same = (win == full).all(1).cpu().numpy()
    for b, label in enumerate(labels):
        r = check_frame(win[b].long(), pts[b], cuda(IR.positions64(beta_np[:, :, b], sz)), lat)
        one = torch.zeros(1, dtype=torch.int64, device="cuda")
        ops.image_iwarp(vals, [b], sz, beta, [b], count=one)
        r["count"] = int(one)
        print(f"K7F64 {IR.case_id(c)} | {label} | differ {r['differ']} bad_a {r['bad_a']} (worst {r['worst_a']:.3g}) bad_b "
              f"{r['bad_b']} (worst {r['worst_b']:.3g}, {r['ratio_b']:.3g} of the margin; largest margin {r['margin']:.3g}, "
              f"{r['margin_inside']:.3g} at d2 < 1) ties {r['ties']:.4f} count {r['count']} of {P} window==full {bool(same[b])}")
        if r["bad_a"]:
            problems.append(f"{label}: (a) {r['bad_a']} points, worst excess {r['worst_a']:.3g}")
        if r["bad_b"]:
            problems.append(f"{label}: (b) {r['bad_b']} points, worst excess {r['worst_b']:.3g}")
        if not same[b]:
            problems.append(f"{label}: window != exhaustive")
        if kind != "identity" and r["ties"] > IR.TIE_CAP:
            problems.append(f"{label}: near ties {r['ties']:.4f}")
        if IR.is_mild(kind, b) and sz not in IR.THIN and r["count"] != 0:
            problems.append(f"{label}: mild, count {r['count']}")
        if (kind == "fold" or sz in IR.THIN) and r["count"] != P:
            problems.append(f"{label}: count {r['count']} != P")
    if kind == "fold" or sz in IR.THIN:
        assert int(count) == B * P
    assert not problems, problems


@pytest.mark.parametrize("sz", IR.TIE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_ties_go_to_the_lowest_voxel_index(ops, sz):
    """S - 1 a power of two on every axis, identity and integer shifts: the K1-scaled fp32 positions ARE positions64, every d2 is
    exact, and the chosen voxel must be nearest64's -- the lowest index among equals -- with no tolerance."""
    labels, beta_np = IR.tie_case(sz)
    B, P = len(labels), int(np.prod(sz))
    beta, times = cuda(beta_np), list(range(B))
    vals = index_frames(B, P)
    win = ops.image_iwarp(vals, None, sz, beta, times)
    full = ops.image_iwarp(vals, None, sz, beta, times, exhaustive=True)
    assert torch.equal(win, full)
    pts = k1_positions(ops, sz, beta, times)
    lat = cuda(IR.lattice64(sz))
    most = 0
    for b in range(B):
        p64 = cuda(IR.positions64(beta_np[:, :, b], sz))
        assert torch.equal(pts[b].double(), p64), labels[b]
        idx, best, second = IR.nearest64_torch(p64, lat)
        assert torch.equal(win[b].long(), idx), (labels[b], int((win[b].long() != idx).sum()))
        d = IR._d2(lat, p64, torch)
        ways = (d == best[:, None]).sum(1)
        most = max(most, int(ways.max()))
        if b == 0:
            assert int((best == second).sum()) >= P // 2          # the identity: an axis of 2 ties half the lattice
    assert most >= (4 if sz == (2, 17, 2) else 2), most


def test_more_than_64_frames(ops):
    """B = 70 in one call: the exhaustive kernel's blocks walk frames b, b + 64; marked frames at 3, 66 and 69.  Frames through a
    ``frame_ids`` permutation, the output with a wider row stride."""
    sz, B = IR.MANY_SZ, IR.MANY_B
    P = int(np.prod(sz))
    beta = cuda(IR.many_frames_case())
    rng = np.random.default_rng(70)
    frames = torch.from_numpy(rng.random((B, P), dtype=np.float32)).cuda()
    perm = [int(i) for i in rng.permutation(B)]
    out = torch.full((B, P + 7), -3.0, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.image_iwarp(frames, perm, sz, beta, list(range(B)), out=out, count=count)
    for b in range(B):
        ref = ops.image_iwarp(frames, [perm[b]], sz, beta, [b], exhaustive=True)
        assert torch.equal(out[b, :P], ref[0]), b
    assert int(count) == len(IR.MANY_FOLDS) * P
    assert bool((out[:, P:] == -3.0).all())


def test_channels_under_zoom(ops):
    """20x300x1 (nyb = 2, a ragged second plane block), three channels, zoom 0.7: one search per lattice point, gathered from
    every channel = three single-channel calls, bit for bit."""
    sz, NC = (20, 300, 1), 3
    P = int(np.prod(sz))
    labels, beta_np = IR.case(sz, "zoom")
    beta = cuda(beta_np[:, :, [labels.index("zoom 0.7")]])
    frames = torch.from_numpy(np.random.default_rng(3).random((2, NC * P), dtype=np.float32)).cuda()
    for exhaustive in (False, True):
        out = ops.image_iwarp(frames, None, sz, beta, [0, 0], nchan=NC, exhaustive=exhaustive)
        for ch in range(NC):
            one = ops.image_iwarp(frames[:, ch * P:(ch + 1) * P], None, sz, beta, [0, 0])
            assert torch.equal(out[:, ch * P:(ch + 1) * P], one), (exhaustive, ch)
