"""The list-form reconstruction image -- ``dnmf_recon_image_lists[_ex]`` (ops.recon_image_lists, ExponentialFP.recon_image with
use_lists, the forward kernel of every fused motion epoch) and the layout it reads (ops.pack_footprints_lists: At, bbox) --
against the float64 definition of tests/recon_lists_restatement.py, entry by entry: every float of every image, border and
row excess included.  What the case tables reach, and that the cases tell a wrong kernel from the right one by ten bounds, is
checked without a GPU in tests/test_recon_lists_restatement_host.py.

Cases (recon_lists_restatement.CASES):
  edge    the volumes (1,1,1) (4,12,1) (8,60,1) (6,28,2) (5,7,3) (9,20,3) (7,9,5) (33,31,2) (41,130,1) and (5,30,3) (6,20,5)
          (Z = 3 and 5 with volume columns on both sides of the positions 63 | 64), B = 1, 15 | 16 | 17, 63 | 64 | 65, 70 each
          at two volumes.  Neurons: single voxels at the eight corners, one all zero, one that fills the volume, boxes that
          end / begin on either side of every boundary between two runs of 64 positions and of the padded rows 3 | 4, 7 | 8.
  stack   (41,130,1) and (33,31,2): boxes stacked on single tiles, lists of 0, 1, 8, 9, 16, 17, 25 | 26 neurons in a shuffled
          neuron order, every other tile empty, one all-zero neuron (K = 77: the NW = 2 form).
  K       1, 64 | 65, 128 | 129, 256 at two volumes each (NW = 1 | 2 | 4 on both sides of every threshold), among them 256
          neurons that all cover (5,7,3): 32 groups of read-modify-write; K = 257 is refused by name.
  Every case in three families, footprints dense and signed inside their boxes: one-hot traces (frame b names neuron
  (s + b) mod K, as many calls as name every neuron: S[b] is A[:, k(b)] bit for bit), integers 0 .. 15 (bit-equal to the
  integer product), random signed fp32 with exact zeros and -0.0 inside the boxes (the bound).  ``times`` is a permutation
  with one repeat out of a C of B + 3 columns, C a column window of a wider table (ldc > T), ``out`` has two spare rows and a
  row stride 24 floats wider, all preset to 7; out = None and a second call give the same bits.
  skip_empty  into rows preset to 7: exactly the empty tiles of ``tile_lists`` still hold 7, everything else is the image;
          after a full call, a call with other traces and skip_empty equals a fresh image bit for bit.
  model   ExponentialFP.recon_image, use_lists, K = 65 and 129 at (41,130,1) with a zero_state: the bits of
          ops.recon_image_lists; integers: also the bits of the dense path (use_lists = False).
  long    (5,12,2), K = 20, B = 349526, integers: B ntile = 1048578, the smallest product past 64 * 16384 with three tiles,
          fpw = 65 (a second run of 64 frames of one frame).  Short rows and a last tile of one row keep the images to
          0.4 GB; compared on the device in float64, in pieces.

Bound (recon_lists_restatement.bound; U = 2^-24; not tuned): n U sum_k |A C| (1 + n U) per entry, n the non-zero terms -- one
rounding per term of the fmaf chain; no term, exact zero.
Every test prints its worst |error| / bound, its bit-equal share and its host and GPU seconds.

Measured on the MI355X (kept apart from the bound above, which they did not set):
54 tests, 3.3 s in all (the slowest 0.44 s, the first use of the model; every float64 reference under 0.1 s of host time).
  one-hot, integers   bit-equal in every case, the 349526 frames of the long case (100663488 floats, under 10 ms) included
  random, |error| / bound   edge cases 0.957 .. 0.997 ((1,1,1): 0.028 and 0.12), stacks 0.986 and 0.973, K 1: 0.47 and 0.89,
                      K 64 .. 129: 0.76 .. 0.99, K 256: 0.0094 at (5,7,3) (all 256 terms in every entry), 0.995 at (41,130,1);
                      model path 0.984 (K 65) and 0.997 (K 129).  The bound is sharp where one neuron alone reaches a voxel
                      (n = 1: one rounding, U |a c|), and such voxels are in nearly every case: a ratio just under 1 is what
                      a right kernel gives there.  Bit-equal share of the random images 0.82 .. 1.0.
  pack                At bit-equal with the sign of -0.0 kept, bbox equal, at all eleven volumes and the two stack cases
  skip_empty          floats an image in empty tiles, all still 7: 5792 of 7200, 2016 of 3552 (stacks), 160 of 7200, 352 of
                      1056, 0 of 768 (no empty tile: everything is written), 64 of 576
No defect was found in the kernel or in the pack step.  The wrapper refused a C that is a column window of a wider table
although the kernel takes ldc; it now takes any row stride, as ops.recon_image does."""
import time

import numpy as np
import pytest
import torch

import recon_lists_restatement as R

pytestmark = pytest.mark.gpu
F32 = np.float32
SPARE, PAD = 2, 24


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def window(a, extra=4, fill=-3.5):
    """``a`` (rows, cols) on the device as the first columns of a buffer ``extra`` columns wider (they hold ``fill``)."""
    buf = torch.full((a.shape[0], a.shape[1] + extra), fill, device="cuda")
    buf[:, :a.shape[1]] = dev(a)
    return buf[:, :a.shape[1]]


def layout_of(ops, A, sz):
    return ops.pack_footprints_lists(dev(A), list(sz))


def images(ops, call, sz, B, what):
    """``call(out)`` writes B halo images into the first rows of a buffer preset to 7 -> (B, Pp) numpy, after checking that
    the spare rows and the floats beyond Pp still hold 7."""
    Pp = R.geometry(sz)["Pp"]
    assert ops.halo_voxels(sz) == Pp
    buf = torch.full((B + SPARE, Pp + PAD), R.PATTERN, device="cuda")
    res = call(buf)
    assert res.data_ptr() == buf.data_ptr()
    got = buf.cpu().numpy()
    assert (got[B:] == R.PATTERN).all() and (got[:, Pp:] == R.PATTERN).all(), f"{what}: spare rows or floats beyond Pp were written"
    return got[:B, :Pp]


def compare(got, c, times, sz, what):
    """The whole images against the definition -> (|error| / bound, bit-equal share)."""
    S = R.recon(c["A"], c["C"], times, sz)
    share = float((got == S.astype(F32)).mean())
    if c["exact"]:
        assert np.array_equal(got.astype(np.float64), S), f"{what}: not bit-equal (share {share:.6f})"
        return 0.0, share
    ratio, idx, zeros_ok = R.worst(np.abs(got.astype(np.float64) - S), R.bound(c["A"], c["C"], times, sz))
    assert zeros_ok, f"{what}: an entry without a term (border, excess, outside every box) is not an exact zero"
    assert ratio <= 1.0, f"{what}: entry {idx}: |error| = {ratio:.3g} of the bound"
    return ratio, share


def product_check(ops, name):
    sz = R.CASES[name][0]
    K, B = len(R.CASES[name][1]), R.CASES[name][2]
    top, low, host = 0.0, 1.0, 0.0
    t0 = time.perf_counter()
    for family in R.FAMILIES:
        c = R.case_inputs(name, family)
        ly = layout_of(ops, c["A"], sz)
        Cw = window(c["C"])
        assert Cw.stride(0) > Cw.shape[1] and not Cw.is_contiguous() or K == 1
        for times in c["calls"]:
            what = f"{name} {family}"
            tt = dev(np.array(times), torch.int32)
            got = images(ops, lambda out: ops.recon_image_lists(ly, K, sz, Cw, tt, out=out), sz, B, what)
            h0 = time.perf_counter()
            ratio, share = compare(got, c, times, sz, what)
            host += time.perf_counter() - h0
            top, low = max(top, ratio), min(low, share)
            own = ops.recon_image_lists(ly, K, sz, Cw, tt)
            assert tuple(own.shape) == (B, R.geometry(sz)["Pp"])
            assert np.array_equal(own.cpu().numpy(), got), f"{what}: out = None and a caller's wider out differ"
            again = ops.recon_image_lists(ly, K, sz, dev(c["C"]), tt, out=own)
            assert np.array_equal(again.cpu().numpy(), got), f"{what}: a second call gives other bits"
    total = time.perf_counter() - t0
    print(f"\nrecon lists {name}: K {K}, one-hot and integers bit-equal, random |error| / bound {top:.3g}, bit-equal share >= {low:.6f}; "
          f"host {host:.2f} s, GPU {total - host:.2f} s")


@pytest.mark.parametrize("sz", R.VOLUMES, ids=lambda s: "x".join(map(str, s)))
def test_pack_layout(ops, sz):
    """At: the interior is A transposed bit for bit, border and row excess are zero; bbox is ``support_boxes``."""
    g = R.geometry(sz)
    for name in (R.PACK_CASES[sz],) + tuple(n for n in R.STACK_CASES if R.CASES[n][0] == sz):
        c = R.case_inputs(name, "random")
        ly = layout_of(ops, c["A"], sz)
        At = ly["At"].cpu().numpy()
        assert At.shape == (c["A"].shape[1], g["Pp"])
        want = R.to_halo(np.ascontiguousarray(c["A"].T), sz)
        assert np.array_equal(At.view(np.uint32), want.view(np.uint32)), f"{name}: At is not A transposed in the halo layout, bit for bit"
        assert np.array_equal(ly["bbox"].cpu().numpy().astype(np.int64), R.support_boxes(c["A"], sz)), f"{name}: bbox"
    print(f"\npack {sz}: At bit-equal (sign of zero included), bbox equal")


@pytest.mark.parametrize("name", R.EDGE_CASES)
def test_product_at_every_edge(ops, name):
    product_check(ops, name)


@pytest.mark.parametrize("name", R.STACK_CASES)
def test_product_at_every_list_length(ops, name):
    product_check(ops, name)


@pytest.mark.parametrize("name", R.KFORM_CASES)
def test_product_in_every_kernel_form(ops, name):
    product_check(ops, name)


def test_k257_is_refused_by_name(ops):
    from dnmf_amd import _lib
    sz, K = (5, 7, 3), R.REFUSED_K
    g = R.geometry(sz)
    ly = {"At": torch.zeros(K, g["Pp"], device="cuda"), "bbox": torch.zeros(K, 6, dtype=torch.int32, device="cuda")}
    out = torch.full((2, g["Pp"]), R.PATTERN, device="cuda")
    with pytest.raises(_lib.DnmfHipError, match=f"K={K} > 256"):
        ops.recon_image_lists(ly, K, sz, torch.ones(K, 4, device="cuda"), [0, 1], out=out)
    assert (out == R.PATTERN).all()


def test_wrapper_takes_a_row_stride_and_checks_the_shape(ops):
    name = "K65-6x28x2-B5"
    sz, K = R.CASES[name][0], 65
    c = R.case_inputs(name, "integers")
    ly = layout_of(ops, c["A"], sz)
    with pytest.raises(ValueError, match="C must be"):
        ops.recon_image_lists(ly, K, sz, dev(c["C"])[:K - 1], [0])
    with pytest.raises(ValueError, match="C must be"):
        ops.recon_image_lists(ly, K, sz, dev(c["C"]).reshape(-1), [0])
    with pytest.raises(ValueError, match="unit inner stride"):
        ops.recon_image_lists(ly, K, sz, dev(c["C"].T.copy()).T, [0])
    more = torch.cat([dev(c["C"]), torch.full((3, c["C"].shape[1]), 9.0, device="cuda")])          # rows past K are not read
    a = ops.recon_image_lists(ly, K, sz, more, c["calls"][0])
    b = ops.recon_image_lists(ly, K, sz, window(c["C"]), c["calls"][0])
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", R.STACK_CASES + ["edge-41x130x1-B1", "edge-7x9x5-B65", "edge-8x60x1-B16", "K256-5x7x3-B5"])
def test_skip_empty_leaves_exactly_the_empty_tiles(ops, name):
    """skip_empty into rows preset to 7: the tiles that ``tile_lists`` calls empty still hold 7 in every float, every other
    float of the image is written (and right)."""
    sz = R.CASES[name][0]
    K, B = len(R.CASES[name][1]), R.CASES[name][2]
    t0 = time.perf_counter()
    for family in ("integers", "random"):
        c = R.case_inputs(name, family)
        times = c["calls"][0]
        ly = layout_of(ops, c["A"], sz)
        tt = dev(np.array(times), torch.int32)
        got = images(ops, lambda out: ops.recon_image_lists(ly, K, sz, window(c["C"]), tt, out=out, skip_empty=True), sz, B, name)
        empty = np.array([len(l) == 0 for l in R.tile_lists(R.support_boxes(c["A"], sz), sz)])[R.tile_of_position(sz)]
        assert (got[:, empty] == R.PATTERN).all(), f"{name} {family}: an empty tile was written"
        full = ops.recon_image_lists(ly, K, sz, window(c["C"]), tt).cpu().numpy()
        assert np.array_equal(got[:, ~empty], full[:, ~empty]), f"{name} {family}: a listed tile differs from the full call"
        assert not full[:, empty].any()
        compare(full, c, times, sz, f"{name} {family}")
    print(f"\nskip_empty {name}: {int(empty.sum())} of {empty.size} floats an image in empty tiles, all kept; host + GPU "
          f"{time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("name", R.STACK_CASES)
def test_skip_empty_after_a_full_call_is_a_fresh_image(ops, name):
    sz = R.CASES[name][0]
    K, B = len(R.CASES[name][1]), R.CASES[name][2]
    c, c2 = R.case_inputs(name, "random"), R.case_inputs(name, "integers")
    ly = layout_of(ops, c["A"], sz)
    tt = dev(np.array(c["calls"][0]), torch.int32)
    buf = torch.full((B + SPARE, R.geometry(sz)["Pp"] + PAD), R.PATTERN, device="cuda")
    ops.recon_image_lists(ly, K, sz, dev(c["C"]), tt, out=buf)
    ops.recon_image_lists(ly, K, sz, dev(c2["C"]), tt, out=buf, skip_empty=True)
    fresh = ops.recon_image_lists(ly, K, sz, dev(c2["C"]), tt)
    assert torch.equal(buf[:B, :fresh.shape[1]], fresh)
    assert bool((buf[B:] == R.PATTERN).all()) and bool((buf[:, fresh.shape[1]:] == R.PATTERN).all())
    c3 = dict(c, C=c2["C"])
    compare(fresh.cpu().numpy(), c3, c["calls"][0], sz, name)


@pytest.mark.parametrize("K", R.MODEL_K)
def test_model_path(ops, K):
    """ExponentialFP.recon_image with use_lists and a zero_state (the second call skips the empty tiles): the bits of
    ops.recon_image_lists; integers: the bits of the dense path as well."""
    from dnmf_amd.Demix.dNMF import ExponentialFP
    sz = R.MODEL_SZ
    t0 = time.perf_counter()
    fp = ExponentialFP(list(sz), K, 4, positions=torch.zeros(K, 3))
    top = 0.0
    for family in ("integers", "random"):
        c = R.model_inputs(K, family)
        times, B = c["calls"][0], len(c["calls"][0])
        tt = dev(np.array(times), torch.int32)
        fp.A = dev(c["A"]).reshape(*sz, K)
        fp.invalidate_layouts()
        fp.use_lists = True
        ly = fp.lists_layout()
        assert ly is not None and ly["boxfrac"] < 6.0
        state = [None]
        buf = torch.full((B + SPARE, R.geometry(sz)["Pp"] + PAD), R.PATTERN, device="cuda")
        for n, Cn in enumerate((c["C"], c["C2"])):
            res = fp.recon_image(dev(Cn), tt, out=buf, zero_state=state)
            assert res.data_ptr() == buf.data_ptr() and state[0] is ly
            direct = ops.recon_image_lists(ly, K, sz, dev(Cn), tt)
            assert torch.equal(buf[:B, :direct.shape[1]], direct), f"K {K} {family} call {n}: the model path and ops.recon_image_lists differ"
            assert bool((buf[B:] == R.PATTERN).all()) and bool((buf[:, direct.shape[1]:] == R.PATTERN).all())
            ratio, _ = compare(direct.cpu().numpy(), dict(c, C=Cn), times, sz, f"model K {K} {family} call {n}")
            top = max(top, ratio)
            if family == "integers":
                fp.use_lists = False
                dense = fp.recon_image(dev(Cn), tt)
                fp.use_lists = True
                assert torch.equal(dense[:, :direct.shape[1]], direct), f"K {K} call {n}: the list path and the dense path differ"
    print(f"\nmodel path K {K}: integers bit-equal to the dense path, random |error| / bound {top:.3g}; host + GPU {time.perf_counter() - t0:.2f} s")


def test_long_frame_runs(ops):
    """fpw = 65: a wave sweeps a run of 64 frames and one frame more (``LONG_CASE``).  Integers; there are only 64 different
    images, made on the host in float64, and every one of the B images is compared with its own on the device."""
    L = R.LONG_CASE
    sz, K, B = L["sz"], L["K"], L["B"]
    assert R.launch(sz, B)["fpw"] == 65
    c = R.long_inputs()
    h0 = time.perf_counter()
    ref = dev(R.recon(c["A"], c["C"], range(L["T"]), sz), torch.float64)                  # (T, Pp)
    host = time.perf_counter() - h0
    t0 = time.perf_counter()
    ly = layout_of(ops, c["A"], sz)
    tt = dev(c["times"], torch.int32)
    Pp = R.geometry(sz)["Pp"]
    buf = torch.full((B + 1, Pp + 4), R.PATTERN, device="cuda")
    ops.recon_image_lists(ly, K, sz, window(c["C"]), tt, out=buf)
    bad = 0
    for s in range(0, B, 32768):
        e = min(B, s + 32768)
        bad += int((buf[s:e, :Pp].double() != ref[tt[s:e].long()]).sum())
    assert bool((buf[B:] == R.PATTERN).all()) and bool((buf[:, Pp:] == R.PATTERN).all())
    torch.cuda.synchronize()
    print(f"\nlong frame runs: B {B}, fpw 65, {bad} of {B * Pp} floats differ; host {host:.2f} s, GPU {time.perf_counter() - t0:.2f} s")
    assert bad == 0
