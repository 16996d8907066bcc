"""K2 (dnmf_warp_recon_grad) against its float64 definition tests/k2_restatement.py, output by output and entry by entry.

Shapes (k2_restatement.SHAPES / LARGE; PLANE_ROWS = 32 x-rows by PLANE_COLS = 256 plane positions a block):
  (33, 257, 1)    Z = 1: two x-blocks with a one-row tail (the loop that is not unrolled), two plane blocks with a one-lane tail
  (65, 300, 2)    Z = 2 (a lane owns both slices): three x-blocks, two plane blocks
  (34, 90, 3)     Z > 2: Y Z = 270, the plane-block boundary falls inside a z-column
  (9, 7, 5)       thin: one block, z-taps outside on both sides
  (2044, 2044, 1), (2044, 1020, 2)   halo images of 2^24 bytes: the F32OFF = false kernels (asserted below), frames F0 and F5
Frames, the columns COL of one beta (10, 3, 8) whose column UNUSED no call names (k2_restatement.case_betas):
  F0 sub-voxel shift (the Z = 1 tap-row reuse holds everywhere)      F1 x-scale 1.03 + xy-shear 0.011 (waves mix reuse and gather)
  F2 x-scale 0.5 (advance 0 or 1)    F3 x reversed (advance -1)      F4 +5.3 along x, -Y/3 along y (rows wholly outside, halo taps)
  F5 the generic quadratic warp of test_gpu_gn.k16_case              F6 all-zero traces;   at Z > 1 every frame also moves z
S rows are addressed through s_ids in a buffer with lds = halo_voxels + 32, frames through frame_ids in a buffer of two spare
rows with ldf = P + 8 (even: the Z = 2 kernels read a column's two slices as one aligned pair), norm_frames = B + 3.

Bounds (k2_restatement.grad_tol / recon_tol):
  gradient   |got - preset - want| <= 1e-4 scale abs_sum[a, d] per frame and entry: the project's K2 bound, by the entry's own
             absolute sum.  grad is preset: got = fp32(preset + g) carries half an ulp of that sum, so the preset of an entry is
             0.37 scale abs_sum (the size of the entry: the rounding is 1e-3 of the bound) and a fixed non-zero pattern where
             abs_sum == 0 -- there, and in the unused column, the result must be the preset bit for bit.
  frame_loss rtol 1e-5; loss[0] the sum of frame_loss at rtol 1e-5
  reg        rtol 1e-4 / atol 1e-8 on the frames with |det J| >= 0.1 at both corners (float64); at most two may drop out
  recon      |d| <= 4 spacing_fp32(max|u|) slope + 1e-6 max|S| per voxel
Every test prints its largest |error| / bound and its host and GPU seconds."""
import functools
import time

import numpy as np
import pytest
import torch

import k2_restatement as K2R

pytestmark = pytest.mark.gpu
F32 = np.float32
ALL = K2R.SHAPES + K2R.LARGE


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


@functools.lru_cache(maxsize=None)
def reference(sz, call):
    """The float64 result of the fit call ('fit') or of the call with an upstream gradient ('gout'); (result, host seconds)."""
    c = K2R.k2_case(sz)
    t0 = time.perf_counter()
    kw = {"frames": c["frames"], "norm_frames": c["norm_frames"]} if call == "fit" else {"gout": c["gout"]}
    ref = K2R.k2(c["S32"], c["beta"], sz, c["times"], **kw)
    return ref, time.perf_counter() - t0


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
    return {"S": Sbuf, "s_ids": dev(s_rows, torch.int32), "frames": Fbuf, "frame_ids": dev(f_rows, torch.int32),
            "beta": dev(c["beta"]), "times": dev(np.array(c["times"]), torch.int32)}


def preset_for(ref, times):
    """(10, 3, T) fp32: 0.37 scale abs_sum with alternating signs at the entries of the frames, a fixed non-zero pattern where
    that is zero and in every other column."""
    pat = ((np.arange(30 * K2R.T_COLS).reshape(10, 3, K2R.T_COLS) % 7 + 1) / 8.0) * np.where(np.arange(K2R.T_COLS) % 2, -1.0, 1.0)
    sized = 0.37 * ref["scale"] * ref["abs_sum"] * np.where(np.arange(30).reshape(10, 3) % 2, -1.0, 1.0)
    for b, t in enumerate(times):
        pat[:, :, t] = np.where(ref["abs_sum"][b] > 0, sized[b], pat[:, :, t])
    pat = pat.astype(F32)
    assert (pat != 0).all()
    return pat


def check_grad(got, preset, ref, times, what):
    """The bound per frame and entry, exact zeros and the untouched columns; returns the largest |error| / bound."""
    tol = K2R.grad_tol(ref)
    worst = 0.0
    for b, t in enumerate(times):
        err = np.abs(got[:, :, t].astype(np.float64) - preset[:, :, t].astype(np.float64) - ref["grad"][b])
        zero = ref["abs_sum"][b] == 0
        np.testing.assert_array_equal(got[:, :, t][zero], preset[:, :, t][zero], err_msg=f"{what}: frame {b}, exact zeros")
        ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, tol[b]))
        a, d = np.unravel_index(ratio.argmax(), ratio.shape)
        assert ratio.max() <= 1.0, f"{what}: frame {b} (column {t}) entry ({a}, {d}): |error| = {ratio.max():.3g} of the bound"
        worst = max(worst, float(ratio.max()))
    rest = [t for t in range(K2R.T_COLS) if t not in times]
    assert K2R.UNUSED in rest
    np.testing.assert_array_equal(got[:, :, rest], preset[:, :, rest], err_msg=f"{what}: a column no call names was written")
    return worst


def test_large_volumes_are_past_the_offset_threshold(ops):
    """HaloLayout::f32off is ``halo bytes < 2^24``: the large shapes must be on the far side of it (and just so), the table's
    shapes on the near side; a change of the threshold or of the layout then fails here instead of emptying the cases."""
    for X, Y, Z in K2R.LARGE:
        assert ops.halo_voxels((X, Y, Z)) * 4 >= 2 ** 24
        assert ops.halo_voxels((X - 1, Y, Z)) * 4 < 2 ** 24          # (a halo row is rounded up to 32 floats: Y has slack)
    for sz in K2R.SHAPES:
        assert ops.halo_voxels(sz) * 4 < 2 ** 24
    assert [sz[2] for sz in K2R.LARGE] == [1, 2]


@pytest.mark.parametrize("sz", ALL)
def test_fit_call(ops, sz):
    """Frames, no upstream gradient, A_tC not wanted: the PLAIN kernels and the finish kernel."""
    c = K2R.k2_case(sz)
    ref, host = reference(sz, "fit")
    times, B = c["times"], len(c["times"])
    t0 = time.perf_counter()
    d = device_inputs(ops, c)
    preset = preset_for(ref, times)
    grad = dev(preset)
    out = ops.warp_recon_grad(d["S"], d["s_ids"], d["frames"], d["frame_ids"], sz, d["beta"], d["times"], grad=grad,
                              norm_frames=c["norm_frames"])
    torch.cuda.synchronize()
    got = grad.cpu().numpy()
    gpu = time.perf_counter() - t0
    assert c["norm_frames"] != B and (sz[2] != 2 or d["frames"].stride(0) % 2 == 0)
    worst = check_grad(got, preset, ref, times, "fit call")
    fl = out["frame_loss"].cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(fl, ref["frame_loss"], rtol=1e-5)
    np.testing.assert_allclose(float(out["loss"][0]), fl.sum(), rtol=1e-5)
    np.testing.assert_allclose(float(out["loss"][0]), ref["frame_loss"].sum(), rtol=1e-5)
    keep = (np.abs(ref["det"]) >= 0.1).all(1)
    assert B - int(keep.sum()) <= 2
    reg = out["reg"].cpu().numpy()
    np.testing.assert_allclose(reg[keep], ref["reg"][keep], rtol=1e-4, atol=1e-8)
    lr = float(np.abs(fl / ref["frame_loss"] - 1).max() / 1e-5)
    rr = float((np.abs(reg[keep] - ref["reg"][keep]) / (1e-4 * np.abs(ref["reg"][keep]) + 1e-8)).max())
    print(f"\nfit {sz}: gradient {worst:.3g}, frame_loss {lr:.3g}, reg {rr:.3g} of the bound ({int(keep.sum())} of {B} frames); "
          f"host {host:.2f} s, GPU {gpu:.2f} s")


@pytest.mark.parametrize("sz", ALL)
def test_forward_backward_call(ops, sz):
    """What ExponentialFP.forward / backward ask of K2: A_tC (want_recon), then the gradient of a caller's upstream gradient
    (frames=None, gout) -- the kernels that are not PLAIN, S again addressed through s_ids."""
    c = K2R.k2_case(sz)
    fit, host0 = reference(sz, "fit")
    ref, host1 = reference(sz, "gout")
    times, B = c["times"], len(c["times"])
    P = int(np.prod(sz))
    t0 = time.perf_counter()
    d = device_inputs(ops, c)
    fwd = ops.warp_recon_grad(d["S"], d["s_ids"], d["frames"], d["frame_ids"], sz, d["beta"], d["times"], want_recon=True,
                              norm_frames=c["norm_frames"])
    preset = preset_for(ref, times)
    grad = dev(preset)
    ops.warp_recon_grad(d["S"], d["s_ids"], None, None, sz, d["beta"], d["times"], grad=grad, gout=dev(c["gout"].reshape(B, P)))
    torch.cuda.synchronize()
    recon, got = fwd["recon"].cpu().numpy().astype(np.float64).reshape(B, *sz), grad.cpu().numpy()
    gpu = time.perf_counter() - t0
    rtol = K2R.recon_tol(fit, float(np.abs(c["S32"]).max()))
    err = np.abs(recon - fit["recon"]).reshape(B, -1).max(1)
    assert (err <= rtol).all(), (err / rtol)
    np.testing.assert_allclose(fwd["frame_loss"].cpu().numpy(), fit["frame_loss"], rtol=1e-5)
    assert ref["scale"] == 1.0
    worst = check_grad(got, preset, ref, times, "upstream gradient")
    print(f"\nforward/backward {sz}: recon {float((err / rtol).max()):.3g}, gradient {worst:.3g} of the bound; "
          f"host {host0 + host1:.2f} s (shared with the fit call), GPU {gpu:.2f} s")


def test_odd_frame_stride_is_refused_at_two_slices(ops):
    """Z == 2 reads (x, y, 0), (x, y, 1) of a frame as one eight-byte load: an odd ldf would put odd rows on odd addresses, so
    both entry points refuse it before anything is launched (also without a GPU: tests/test_abi_and_host.py)."""
    sz = (6, 5, 2)
    P = 60
    S = torch.zeros((2, ops.halo_voxels(sz)), device="cuda")
    beta = dev(np.zeros((10, 3, 2), F32))
    with pytest.raises(RuntimeError, match=r"argument error -2.*even ldf"):
        ops.warp_recon_grad(S, None, torch.zeros((2, P + 1), device="cuda"), None, sz, beta, [0, 1], grad=torch.zeros_like(beta))
