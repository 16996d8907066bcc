"""K16 (dnmf_warp_normal_eqs) against its float64 definition tests/k16_restatement.py, entry by entry.

Shapes (k16_restatement.SHAPES; PLANE_ROWS = 32 x-rows by PLANE_COLS = 256 plane positions a block):
  (33, 257, 1)    Z = 1: two x-blocks with a one-row tail, two plane blocks with a one-lane tail
  (65, 300, 2)    Z = 2 (a lane owns both slices): three x-blocks, two plane blocks
  (34, 90, 5)     Z > 2: Y Z = 450, the plane-block boundary (position 256 = y 51, z 1) falls inside a z-column; two x-blocks
  (9, 7, 4)       thin: one block, z-taps outside on both sides
Z >= 4 in the last two because at Z <= 3 the centred u_z cannot tell exponents 1 from 3 or 2 from 4 (it is -1, 0 or 1): the
z-power chain of the kernel and the monomial index of its finish kernel are checked for exponents 3 and 4 only here.
Frames (k16_restatement.k16_case): k2_restatement's F0 .. F6 in their columns of beta, F7 that puts the image under the last
plane position, F8 with a NaN coefficient, F9 with a +inf coefficient.  S rows are addressed through s_ids in a buffer of B + 2
rows with lds = halo_voxels + 32 (7.0 outside the interiors), frames through frame_ids in a buffer of B + 2 rows with
ldf = P + 8 (even at Z = 2, whose kernel reads a column's two slices as one aligned pair; 5.0 in the spare rows and the padding).

Bounds (k16_restatement.H_tol / g_tol / SSE_RTOL):
  H, g   |got - want| <= 1e-4 absH[i, j], 1e-4 absg[i] per frame and entry -- the project's K2 / K16 figure by the entry's own
         absolute sum; a zero sum (all-zero traces, the unknowns Z = 1 drops) asks for an exact zero
  sse    rtol 1e-5
  F8, F9 H = g = 0 bit for bit, sse NaN
Everything else is bit for bit: H == H^T, out / accumulate, the workspace, repeats and the batch a frame is launched in.
The first test prints its largest |error| / bound and its host and GPU seconds.  Measured on the MI355X, H / g / sse of the bound:
(33, 257, 1) 0.024 / 0.015 / 0.0082, (65, 300, 2) 0.030 / 0.023 / 0.0070, (34, 90, 5) 0.0067 / 0.0052 / 0.0026,
(9, 7, 4) 0.0029 / 0.0017 / 0.0074."""
import time

import numpy as np
import pytest
import torch

import k16_restatement as K16R

pytestmark = pytest.mark.gpu
F32 = np.float32
KEYS = ("H", "g", "sse")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def device_inputs(ops, c):
    """S and the frames in rows of larger buffers, addressed through ids; the spare rows and the padding hold other numbers."""
    sz, B = c["sz"], len(c["times"])
    P = int(np.prod(sz))
    rng = np.random.default_rng(7)
    s_rows, f_rows = rng.permutation(B + 2)[:B], rng.permutation(B + 2)[:B]
    Sbuf = torch.full((B + 2, ops.halo_voxels(sz) + 32), 7.0, device="cuda")
    Fbuf = torch.full((B + 2, P + 8), 5.0, device="cuda")
    for b in range(B):
        Sbuf[s_rows[b]].zero_()
        ops.halo_interior(Sbuf[s_rows[b]], sz).copy_(dev(c["S32"][b]))
        Fbuf[f_rows[b], :P] = dev(c["frames"][b].reshape(-1))
    assert (sz[2] != 2 or Fbuf.stride(0) % 2 == 0) and list(c["times"]) != list(range(B))
    return {"S": Sbuf, "s_rows": s_rows, "frames": Fbuf, "f_rows": f_rows, "beta": dev(c["beta"]), "sz": sz, "times": c["times"]}


def launch(ops, d, sel=None, **kw):
    """K16 on the frames ``sel`` (positions in the case's list; default all of them); the result on the host as numpy."""
    sel = list(range(len(d["times"]))) if sel is None else list(sel)
    res = ops.warp_normal_eqs(d["S"], dev(d["s_rows"][sel], torch.int32), d["frames"], dev(d["f_rows"][sel], torch.int32), d["sz"],
                              d["beta"], dev(np.array(d["times"])[sel], torch.int32), **kw)
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in KEYS}


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def assert_bits(a, b, what):
    """The same bits; a NaN (the sse of F8 and F9) where the other has one, whatever its payload."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(b)
    np.testing.assert_array_equal(np.isnan(a), nan, err_msg=what)
    np.testing.assert_array_equal(bits(np.where(nan, 0.0, a)), bits(np.where(nan, 0.0, b)), err_msg=what)


def assert_same_bits(a, b, what):
    for k in KEYS:
        assert_bits(a[k], b[k], f"{what}: {k}")


@pytest.fixture(scope="module")
def once(ops):
    """{sz: (the device inputs, the result of one plain launch of the whole list)}, made on first use."""
    made = {}

    def get(sz):
        if sz not in made:
            d = device_inputs(ops, K16R.k16_case(sz))
            made[sz] = (d, launch(ops, d))
        return made[sz]
    return get


@pytest.mark.parametrize("sz", K16R.SHAPES)
def test_entry_by_entry(ops, once, sz):
    c = K16R.k16_case(sz)
    t0 = time.perf_counter()
    ref = K16R.reference(sz)
    host = time.perf_counter() - t0
    t0 = time.perf_counter()
    d, got = once(sz)
    gpu = time.perf_counter() - t0
    B, fin = len(c["times"]), c["finite"]
    Ht, gt = K16R.H_tol(ref), K16R.g_tol(ref)
    print()
    for b in range(B):
        print(f"  {sz} frame {b}: H {K16R.worst(np.abs(got['H'][b] - ref['H'][b]), np.where(Ht[b] > 0, Ht[b], 1)):.3g}, "
              f"g {K16R.worst(np.abs(got['g'][b] - ref['g'][b]), np.where(gt[b] > 0, gt[b], 1)):.3g}, "
              f"sse {got['sse'][b]:.9g} / {ref['sse'][b]:.9g}")
    wh = wg = ws = 0.0
    for b in range(B):
        np.testing.assert_array_equal(bits(got["H"][b]), bits(got["H"][b].T), err_msg=f"frame {b}: H != H^T")
        if b >= fin:       # a coefficient that is not finite: zeros bit for bit, sse NaN
            assert np.isnan(ref["sse"][b]) and np.isnan(got["sse"][b])
            assert not bits(got["H"][b]).any() and not bits(got["g"][b]).any()
            continue
        for k, tol in (("H", Ht[b]), ("g", gt[b])):
            zero = tol == 0
            assert not got[k][b][zero].any(), f"frame {b}: {k} is not an exact zero where its absolute sum is"
            ratio = np.where(zero, 0.0, np.abs(got[k][b] - ref[k][b]) / np.where(zero, 1.0, tol))
            at = np.unravel_index(ratio.argmax(), ratio.shape)
            assert ratio.max() <= 1.0, f"frame {b} (column {c['times'][b]}) {k}{at}: |error| = {ratio.max():.3g} of the bound"
            if k == "H":
                wh = max(wh, float(ratio.max()))
            else:
                wg = max(wg, float(ratio.max()))
        np.testing.assert_allclose(got["sse"][b], ref["sse"][b], rtol=K16R.SSE_RTOL)
        ws = max(ws, abs(got["sse"][b] / ref["sse"][b] - 1) / K16R.SSE_RTOL)
    assert not ref["absH"][6].any() and not got["H"][6].any() and not got["g"][6].any()             # F6: all-zero traces
    if sz[2] == 1:
        assert (ref["absH"][:fin].reshape(fin, 10, 3, 10, 3)[:, :, 2] == 0).all()                     # checked above as zeros
    print(f"{sz}: H {wh:.3g}, g {wg:.3g}, sse {ws:.3g} of the bound; host {host:.2f} s, GPU {gpu:.2f} s")


def preset(rows):
    """A fixed non-zero pattern for an ``out`` of ``rows`` frames."""
    f = lambda n: ((np.arange(n) % 13 + 1) / 8.0) * np.where(np.arange(n) % 2, -1.0, 1.0)
    return {"H": f(rows * 900).reshape(rows, 30, 30), "g": f(rows * 30).reshape(rows, 30), "sse": f(rows) + 3.0}


@pytest.mark.parametrize("sz", K16R.SHAPES)
def test_out_and_accumulate(ops, once, sz):
    """``out`` longer than the batch: the rows past it are not touched; accumulate adds to what is there in float64, once."""
    d, plain = once(sz)
    B = len(d["times"])
    pre = preset(B + 3)
    for accumulate in (False, True):
        out = {k: dev(pre[k], torch.float64) for k in KEYS}
        got = launch(ops, d, out=out, accumulate=accumulate)
        for k in KEYS:
            assert_bits(got[k][B:], pre[k][B:], f"{k}: a row past the batch was written")
            assert_bits(got[k][:B], pre[k][:B] + plain[k] if accumulate else plain[k], f"{k}, accumulate={accumulate}")


@pytest.mark.parametrize("sz", K16R.SHAPES)
def test_workspace(ops, once, sz):
    """A workspace of exactly the bytes asked for plus a guard tail: the tail is not written, and what the workspace held
    before -- zeros or NaN bit patterns -- changes no bit of the result: the finish kernel reads only what that launch wrote."""
    from dnmf_amd import _lib
    d, plain = once(sz)
    need = _lib.load().dnmf_warp_normal_eqs_workspace(*sz, len(d["times"]))
    assert need > 0 and need % 4 == 0
    guard = 1024
    for fill in (0, -1):                                        # int32 -1: every float a NaN
        ws = torch.full((need // 4 + guard,), fill, dtype=torch.int32, device="cuda")
        ws[need // 4:] = 0x5A5A5A5A
        got = launch(ops, d, workspace=ws.view(torch.float32))
        assert_same_bits(got, plain, f"workspace preset to {fill}")
        assert bool((ws[need // 4:] == 0x5A5A5A5A).all()), "the guard tail was written"
        if fill:
            assert not bool((ws[:need // 4] == fill).all())


@pytest.mark.parametrize("sz", K16R.SHAPES)
def test_order_and_batch_independence(ops, once, sz):
    """The same call twice, the list in another order, and every frame alone (B = 1): the same bits for the same frame."""
    d, plain = once(sz)
    B = len(d["times"])
    assert_same_bits(launch(ops, d), plain, "the same call again")
    order = list(np.random.default_rng(3).permutation(B))
    assert order != list(range(B))
    shuffled = launch(ops, d, sel=order)
    assert_same_bits(shuffled, {k: plain[k][order] for k in KEYS}, "the list in another order")
    for b in range(B):
        assert_same_bits(launch(ops, d, sel=[b]), {k: plain[k][b:b + 1] for k in KEYS}, f"frame {b} alone")


@pytest.mark.parametrize("sz", [(34, 90, 5), (9, 7, 4)])
def test_k2_and_k16_see_the_same_sample_at_four_slices_and_more(ops, once, sz):
    """tests/test_gpu_gn.py::test_k2_and_k16_see_the_same_sample_bit_for_bit at Z > 3: K2's per-frame sum of squares
    (frame_loss norm_frames P) is K16's sse, here over more than one block a frame, so to rtol 1e-5."""
    c = K16R.k16_case(sz)
    d, plain = once(sz)
    fin = list(range(c["finite"]))
    P = int(np.prod(sz))
    grad = torch.zeros_like(d["beta"])
    k2 = ops.warp_recon_grad(d["S"], dev(d["s_rows"][fin], torch.int32), d["frames"], dev(d["f_rows"][fin], torch.int32), sz, d["beta"],
                             dev(np.array(d["times"])[fin], torch.int32), grad=grad, norm_frames=c["norm_frames"])
    torch.cuda.synchronize()
    sse2 = k2["frame_loss"].cpu().numpy().astype(np.float64) * c["norm_frames"] * P
    assert (plain["sse"][fin] > 0).all()
    np.testing.assert_allclose(sse2, plain["sse"][fin], rtol=1e-5)
