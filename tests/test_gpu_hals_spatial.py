"""K6h, the exact NNLS footprint solver (``dnmf_hals_spatial_lists`` / ``dnmf_hals_spatial``, csrc/spatial_update.hip),
both forms held to the float64 restatement tests/hals_spatial_restatement.py fed the device's own fp32 sums, upcast.

  24x20x2 K=6, 24x20x1 K=6   the planted geometry
  22x19x1 K=5                X no multiple of 4, Y Z no multiple of 4 or 64
  8x70x1  K=4                two (y,z) tiles per x row
  24x20x1 K=12 'cluster'     one tile lists 12 neurons, another lists none
  12x10x1 K=130 'wide'       dense form with boxes, beyond the 128-neuron grouping of K5

Every case has one all-zero trace (Cs[k,k] = 0: the column stays), sums of both signs (the frames are not clamped), zeros
inside the boxes that the first sweep revives, and a footprint at the border whose grown box is clipped.  Each runs as
(D None, 1 sweep, grow 0) and (D, gamma, 7 sweeps, grow 2).

Bounds, as set for this solver: every entry within one fp32 ulp of the restatement's value; where the restatement is exactly
0 the kernel may hold at most 1e-12 (sum_l |a_l Cs[l,k]| + |A1| + gamma |D|) / Cs[k,k]; the KKT figure within 1e-12 of the
same term sum.  The list form and the dense form on the same boxes and sums agree bit for bit, and so do two runs.

Measured on MI355X, every case and both forms: the largest |kernel - restatement| is 1.4e-8 .. 2.9e-8 = 0.49 .. 0.50 ulp,
which is the one rounding of the float64 state to fp32 (the restatement's value is kept in float64); where the restatement
is exactly 0 (1557 .. 14955 entries per case) the kernels hold exactly 0; the KKT figures deviate by exactly 0 on terms up
to 31.  The kernels evaluate the restatement's operations one by one in float64 (no contraction), so their float64 state
has the restatement's bits."""
import functools

import numpy as np
import pytest
import torch

import hals_spatial_restatement as R

pytestmark = pytest.mark.gpu

T = 48
GAMMA = 0.3
CASES = {
    # name: (sz, K, centres (x, y) or None for random ones, sigma)
    "24x20x2": ((24, 20, 2), 6, R.PLANTED_CENTRES, 2.0),
    "24x20x1": ((24, 20, 1), 6, R.PLANTED_CENTRES, 2.0),
    "22x19x1": ((22, 19, 1), 5, np.array([[1.0, 1.0], [10.0, 9.0], [20.0, 17.0], [6.0, 15.0], [16.0, 4.0]]), 2.0),
    "8x70x1": ((8, 70, 1), 4, np.array([[1.0, 3.0], [5.0, 30.0], [3.0, 62.0], [6.0, 68.0]]), 2.0),
    "cluster": ((24, 20, 1), 12, np.array([[1.0 + 0.5 * (i % 6), 2.0 + 1.4 * i] for i in range(12)]), 1.5),
}
VARIANTS = {"plain": (False, 1, 0), "penalty-7-grow": (True, 7, 2)}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def footprints(sz, centres, sigma, rng):
    """(P,K) fp32 Gaussians cut at 1e-3, with a few zeros punched inside every support (the first sweep revives them)."""
    c3 = np.concatenate([centres, np.full((len(centres), 1), 0.5 * (sz[2] - 1))], axis=1)
    A = R.gaussian_footprints(sz, c3, sigma=sigma)
    A[A < 1e-3] = 0.0
    holes = (rng.random(A.shape) < 0.1) & (A > 0) & (A < 0.5)
    A[holes] = 0.0
    return A.astype(np.float32)


def movie(P, K, rng):
    frames = (0.5 * rng.standard_normal((T, P)) + 0.2).astype(np.float32)       # not clamped: sums of both signs
    C = (0.1 + rng.random((K, T))).astype(np.float32)
    C[1] = 0.0                                                                   # a dead trace
    return frames, C


@functools.lru_cache(maxsize=None)
def solved(name, variant):
    """One case solved by both forms (twice the list form) and by the restatement on the device's sums -- made once."""
    from dnmf_amd import ops
    sz, K, centres, sigma = CASES[name]
    with_D, sweeps, grow = VARIANTS[variant]
    rng = np.random.default_rng([sorted(CASES).index(name), sweeps])
    P = sz[0] * sz[1] * sz[2]
    A = footprints(sz, centres, sigma, rng)
    frames, C = movie(P, K, rng)
    D = rng.random((P, K)).astype(np.float32) if with_D else None
    gamma = GAMMA if with_D else 0.0
    A_dev, D_dev = dev(A), (dev(D) if with_D else None)
    layout = ops.pack_footprints_lists(A_dev, sz)
    assert layout["bbox"].cpu().numpy().tolist() == R.support_boxes(A, sz).tolist()
    boxes = ops.dilate_boxes(layout["bbox"], sz, grow)
    assert boxes.cpu().numpy().tolist() == R.dilate_boxes(R.support_boxes(A, sz), sz, grow).tolist()
    sl = ops.spatial_lists_setup({"bbox": boxes}, K, sz)
    assert sl["total"] > 0
    A1c, Cs, _ = ops.spatial_accum_lists(dev(frames), dev(C), sl, sz, K)
    tables = sl["tables"].cpu().numpy()
    A1 = R.expand_entries(A1c.cpu().numpy(), tables, sl["ntiles"], sz, K)
    # the list form, twice
    runs = []
    for _ in range(2):
        A_l, ent = A_dev.clone(), A1c.clone()
        _, kkt_l = ops.hals_spatial_lists(A_l, layout, sl, ent, Cs, sz, D_dev, gamma, sweeps=sweeps, kkt=True, bbox=boxes)
        runs.append((A_l.cpu().numpy(), kkt_l.cpu().numpy(), ent.cpu().numpy()))
    # the dense form on the same sums and boxes
    A_d = A_dev.clone()
    _, kkt_d = ops.hals_spatial(A_d, dev(A1), Cs, D_dev, gamma, sweeps=sweeps, boxes=boxes, kkt=True, sz=sz)
    stored_kkt = ops.hals_spatial_kkt(A_d, dev(A1), Cs, D_dev, gamma, boxes=boxes, sz=sz).cpu().numpy()
    b, Cs64 = boxes.cpu().numpy(), Cs.cpu().numpy().astype(np.float64)
    want = R.hals_spatial(A, A1, Cs64, D=D, gamma=gamma, sweeps=sweeps, boxes=b, sz=sz)
    return dict(sz=sz, K=K, A=A, A1=A1, Cs=Cs64, D=D, gamma=gamma, boxes=b, tables=tables, ntiles=sl["ntiles"], runs=runs,
                dense=(A_d.cpu().numpy(), kkt_d.cpu().numpy()), stored_kkt=stored_kkt, want=want,
                want_kkt=R.kkt(want, A1, Cs64, D=D, gamma=gamma, boxes=b, sz=sz),
                terms=R.term_sum(want, A1, Cs64, D=D, gamma=gamma, boxes=b, sz=sz))


def assert_entries(got, s, what):
    """One fp32 ulp of the restatement's value; where that is exactly 0, 1e-12 of the gradient's terms over Cs[k,k]."""
    want, terms = s["want"], s["terms"]
    d = np.where(np.diag(s["Cs"]) > 0, np.diag(s["Cs"]), 1.0)
    err = np.abs(got.astype(np.float64) - want)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    bound = np.where(want == 0, 1e-12 * terms / d[None, :], ulp)
    print(f"\n{what}: largest |kernel - restatement| {err.max():.3e} ({(err / ulp).max():.3f} ulp); "
          f"{int((want == 0).sum())} exact zeros, largest kernel value there {np.abs(got[want == 0]).max():.3e}")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} entries off, worst {err.max():.3e}"


def assert_kkt(got, s, what):
    scale = np.where(R.box_mask(s["boxes"], s["sz"]), s["terms"], 0.0).max(0)
    err = np.abs(got - s["want_kkt"])
    print(f"{what}: kkt {np.array2string(got, precision=3)}; largest deviation {err.max():.3e} (terms up to {scale.max():.3e})")
    assert got.shape == (s["K"],) and got.dtype == np.float64 and (err <= 1e-12 * scale).all()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_both_forms_equal_the_restatement(ops, name, variant):
    s = solved(name, variant)
    A_l, kkt_l, ent = s["runs"][0]
    A_d, kkt_d = s["dense"]
    assert_entries(A_l, s, f"{name} {variant} lists")
    assert_entries(A_d, s, f"{name} {variant} dense")
    assert_kkt(kkt_l, s, "lists")
    assert_kkt(kkt_d, s, "dense")
    # the entries the list form leaves in A1c are the values it scattered
    assert np.array_equal(R.expand_entries(ent, s["tables"], s["ntiles"], s["sz"], s["K"]), A_l)
    # what the case is for
    M, A, want = R.box_mask(s["boxes"], s["sz"]), s["A"], s["want"]
    assert (A_l[~M] == 0).all() and (A_d[~M] == 0).all()
    assert (A_l[:, 1] == np.where(M[:, 1], A[:, 1], 0)).all() and s["Cs"][1, 1] == 0          # the dead trace's column stays
    assert (s["A1"][M] < 0).any() and (s["A1"][M] > 0).any() and (A_l >= 0).all() and np.isfinite(A_l).all()
    assert ((A == 0) & M & (A_l > 0)).any()                                                   # a zero revived
    tile_n = s["tables"][:s["ntiles"]]
    if name == "cluster":
        assert tile_n.max() == 12 and tile_n.min() == 0
    if name == "8x70x1":
        assert s["ntiles"] == 4 and (tile_n > 0).all()
    if variant == "penalty-7-grow":
        grown = R.support_boxes(A, s["sz"])
        grown[:, 0::2] -= 2
        assert (grown[:, 0::2] < 0).any() and (s["boxes"][:, 0::2] >= 0).all()                # clipped at a border


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_forms_and_runs_agree_bit_for_bit(ops, name, variant):
    s = solved(name, variant)
    (A1_, k1, e1), (A2_, k2, e2) = s["runs"]
    assert np.array_equal(A1_.view(np.uint32), A2_.view(np.uint32)) and np.array_equal(k1.view(np.uint64), k2.view(np.uint64))
    assert np.array_equal(e1.view(np.uint32), e2.view(np.uint32))
    A_d, kkt_d = s["dense"]
    assert np.array_equal(A1_.view(np.uint32), A_d.view(np.uint32))
    assert np.array_equal(k1.view(np.uint64), kkt_d.view(np.uint64))


@pytest.mark.parametrize("name", ["24x20x2", "22x19x1"])
def test_kkt_of_the_stored_footprints(ops, name):
    """``hals_spatial_kkt`` on the rounded fp32 result: the restatement's figure for that state; it sits at the rounding floor
    of fp32 (1e-7 of the terms), above the float64 state's."""
    s = solved(name, "penalty-7-grow")
    want = R.kkt(s["dense"][0], s["A1"], s["Cs"], D=s["D"], gamma=s["gamma"], boxes=s["boxes"], sz=s["sz"])
    scale = s["terms"].max(0)
    print(f"\n{name}: stored kkt {s['stored_kkt']}, state kkt {s['dense'][1]}")
    assert (np.abs(s["stored_kkt"] - want) <= 1e-12 * scale).all()


@functools.lru_cache(maxsize=None)
def wide():
    """12x10x1, K = 130: no list form of K5 (the dense K5 goes by groups of 128 neurons); boxes from the values."""
    from dnmf_amd import ops
    from dnmf_amd.Demix import dNMF
    sz, K = (12, 10, 1), 130
    rng = np.random.default_rng(130)
    centres = np.stack([rng.uniform(0, 11, K), rng.uniform(0, 9, K)], axis=1)
    A = footprints(sz, centres, 1.2, rng)
    frames, C = movie(120, K, rng)
    D = rng.random((120, K)).astype(np.float32)
    A1 = torch.empty((120, K), dtype=torch.float32, device="cuda")
    Cs = torch.empty((K, K), dtype=torch.float32, device="cuda")
    dNMF.DeformableNMF._spatial_accum_dense(dev(frames), dev(C), A1, Cs, None, None)
    boxes = R.dilate_boxes(R.support_boxes(A, sz), sz, (2, 1, 0))
    out = []
    for _ in range(2):
        A_d = dev(A)
        _, kkt = ops.hals_spatial(A_d, A1, Cs, dev(D), GAMMA, sweeps=7, boxes=boxes, kkt=True, sz=sz)
        out.append((A_d.cpu().numpy(), kkt.cpu().numpy()))
    free = dev(A)
    ops.hals_spatial(free, A1, Cs, None, 0.0, sweeps=1)
    A1n, Csn = A1.cpu().numpy(), Cs.cpu().numpy().astype(np.float64)
    want = R.hals_spatial(A, A1n, Csn, D=D, gamma=GAMMA, sweeps=7, boxes=boxes, sz=sz)
    s = dict(sz=sz, K=K, A=A, A1=A1n, Cs=Csn, D=D, gamma=GAMMA, boxes=boxes, want=want,
             want_kkt=R.kkt(want, A1n, Csn, D=D, gamma=GAMMA, boxes=boxes, sz=sz),
             terms=R.term_sum(want, A1n, Csn, D=D, gamma=GAMMA, boxes=boxes, sz=sz))
    s_free = dict(s, want=R.hals_spatial(A, A1n, Csn, sweeps=1), terms=R.term_sum(R.hals_spatial(A, A1n, Csn, sweeps=1), A1n, Csn))
    return s, out, s_free, free.cpu().numpy()


def test_dense_form_with_boxes_beyond_128_neurons(ops):
    s, out, s_free, free = wide()
    assert_entries(out[0][0], s, "wide dense, boxes")
    assert_kkt(out[0][1], s, "wide dense")
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert np.array_equal(out[0][1].view(np.uint64), out[1][1].view(np.uint64))
    M = R.box_mask(s["boxes"], s["sz"])
    assert (out[0][0][~M] == 0).all() and M.sum(1).max() > 32          # more neurons on a voxel than a tile list holds
    # without boxes every voxel is free: all 130 neurons at every voxel
    assert_entries(free, s_free, "wide dense, no boxes")


def test_refusals(ops):
    A = torch.rand(20, 3, device="cuda")
    A1, Cs = torch.rand(20, 3, device="cuda"), torch.eye(3, device="cuda")
    ok = torch.tensor([[0, 4, 0, 3, 0, 0]] * 3)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="sweeps"):
            ops.hals_spatial(A, A1, Cs, sweeps=bad)
    with pytest.raises(ValueError, match="float32"):
        ops.hals_spatial(A.double(), A1, Cs)
    with pytest.raises(ValueError, match="do not match"):
        ops.hals_spatial(A, A1[:, :2].contiguous(), Cs)
    with pytest.raises(ValueError, match="D "):
        ops.hals_spatial(A, A1, Cs, D=torch.rand(20, 2, device="cuda"))
    with pytest.raises(ValueError, match="outside the volume"):
        ops.hals_spatial(A, A1, Cs, boxes=torch.tensor([[0, 5, 0, 3, 0, 0]] * 3), sz=(5, 4, 1))
    with pytest.raises(ValueError, match="outside the volume"):
        ops.hals_spatial_kkt(A, A1, Cs, boxes=torch.tensor([[-1, 4, 0, 3, 0, 0]] * 3), sz=(5, 4, 1))
    with pytest.raises(ValueError, match="sz"):
        ops.hals_spatial(A, A1, Cs, boxes=ok)
    with pytest.raises(ValueError, match="voxels"):
        ops.hals_spatial(A, A1, Cs, boxes=ok, sz=(5, 5, 1))
    with pytest.raises(ValueError, match="shape"):
        ops.hals_spatial(A, A1, Cs, boxes=ok[:2], sz=(5, 4, 1))
    before = A.clone()
    layout = ops.pack_footprints_lists(A, (5, 4, 1))
    sl = ops.spatial_lists_setup(layout, 3, (5, 4, 1))
    ent = torch.zeros(sl["total"], device="cuda")
    with pytest.raises(ValueError, match="sweeps"):
        ops.hals_spatial_lists(A, layout, sl, ent, Cs, (5, 4, 1), sweeps=0)
    with pytest.raises(ValueError, match="outside the volume"):
        ops.hals_spatial_lists(A, layout, sl, ent, Cs, (5, 4, 1), bbox=torch.tensor([[0, 4, 0, 4, 0, 0]] * 3))
    with pytest.raises(ValueError, match="A1c"):
        ops.hals_spatial_lists(A, layout, sl, ent[:5].clone(), Cs, (5, 4, 1))
    assert torch.equal(A, before)                                        # refused, never truncated: nothing was written
