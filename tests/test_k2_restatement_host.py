"""tests/k2_restatement.py, the float64 definition the GPU test holds K2 to, pinned without a GPU: against the reference's
captured gradient, loss and A_tC (fixtures G3, G2, G10), against torch's autograd through the reference's op sequence on the
strong warps of the GPU test, and the flip condition of every (shape, frame) that test uses.

Per-entry bound.  ``1e-4 * scale * abs_sum[a, d]`` is what the GPU test allows K2; the fixtures' gradients and autograd's are
fp32 sums over the same P terms in another order, so they are held to the same bound, entry by entry.  Measured (largest |error|
over the bound): G3 0.0049, G10 0.0022, autograd 0.0019 -- no entry of a fixture needs the older bound by the largest entry."""
import numpy as np
import pytest

import gn_restatement as GN
import k2_restatement as K2R
from conftest import golden
from oracle import dnmf_oracle as O


def worst(err, tol):
    """Largest err / tol over the entries with tol > 0; where tol == 0 the error must be an exact zero."""
    assert (err[tol == 0] == 0).all()
    return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


@pytest.mark.parametrize("label", ["id_b1", "id_b3", "pert_b1", "pert_b3", "pert_b4"])
def test_G3_gradient_and_loss_entry_by_entry(label):
    g = golden("G3_grad")
    sz = [int(s) for s in g["sz"]]
    A = O.gaussian_footprints(sz, g["positions"], np.full(4, 3.0))
    times = g[label + "_times"].tolist()
    frames = np.moveaxis(g["video"][..., times], -1, 0)
    ref = K2R.k2(GN.recon_images(A.reshape(-1, 4), g["C"], times), g[label + "_beta"], sz, times, frames=frames)
    np.testing.assert_allclose(ref["frame_loss"].sum(), g[label + "_loss"], rtol=1e-5)
    want = np.moveaxis(g[label + "_grad"][:, :, times], -1, 0)
    ratio = worst(np.abs(ref["grad"] - want), K2R.grad_tol(ref))
    print(f"\nG3 {label}: |restatement - fixture| / (1e-4 scale abs_sum) <= {ratio:.3g}")
    assert ratio <= 1.0
    others = [t for t in range(g[label + "_grad"].shape[2]) if t not in times]
    assert not g[label + "_grad"][:, :, others].any()
    np.testing.assert_allclose(ref["reg"], O.corner_reg(g[label + "_beta"][:, :, times], sz), rtol=1e-4, atol=1e-8)


def test_G2_reconstruction():
    g = golden("G2_forward")
    sz = [int(s) for s in g["sz"]]
    A = O.gaussian_footprints(sz, g["positions"], np.full(3, 3.0))
    times = g["times"].tolist()
    ref = K2R.k2(GN.recon_images(A.reshape(-1, 3), g["C"], times), g["beta"], sz, times, frames=np.zeros((len(times), *sz)))
    np.testing.assert_allclose(ref["recon"], g["A_tC"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(ref["reg"], g["reg"], rtol=1e-4, atol=1e-8)


def test_G10_z1_gradient_and_exact_zeros():
    g = golden("G10_2d")
    sz = [int(g["sz"][0]), int(g["sz"][1]), 1]
    T = g["beta"].shape[2]
    times = list(range(T))
    frames = np.moveaxis(g["Y2d"], -1, 0)[:, :, :, None]
    ref = K2R.k2(GN.recon_images(g["A2d"].reshape(-1, g["A2d"].shape[-1]), g["C"], times), g["beta"], sz, times, frames=frames)
    np.testing.assert_allclose(ref["frame_loss"].sum(), g["loss"], rtol=1e-5)
    np.testing.assert_allclose(ref["recon"][..., 0], g["A_tC"][..., 1], rtol=0, atol=2e-6)
    assert not ref["grad"][:, :, 2].any() and not ref["grad"][:, [3, 6, 8, 9]].any()          # exact zeros
    assert not ref["abs_sum"][:, :, 2].any() and not ref["abs_sum"][:, [3, 6, 8, 9]].any()
    noz = [0, 1, 2, 4, 5, 7]
    want = np.moveaxis(g["grad"], -1, 0)[:, noz, :2]
    ratio = worst(np.abs(ref["grad"][:, noz, :2] - want), K2R.grad_tol(ref)[:, noz, :2])
    print(f"\nG10: |restatement - fixture| / (1e-4 scale abs_sum) <= {ratio:.3g}")
    assert ratio <= 1.0


@pytest.mark.parametrize("sz", K2R.SHAPES[:3])
def test_strong_warps_against_autograd(sz):
    """All seven frames of the GPU test's case at one shape per Z class, through torch's grid_sample and autograd (the reference's
    op sequence, fp32).  Footprint k is the image of frame k and C picks it, so A . C_t is that image exactly."""
    c = K2R.k2_case(sz)
    B, times = len(c["times"]), c["times"]
    A = np.ascontiguousarray(np.moveaxis(c["S32"], 0, -1))
    C = np.zeros((B, K2R.T_COLS), np.float32)
    C[np.arange(B), times] = 1.0
    loss, grad = O.mse_beta_grad_autograd(A, O.quadratic_basis(O.voxel_lattice(sz)), c["beta"], sz, times, C, c["frames"])
    ref = K2R.k2(c["S32"], c["beta"], sz, times, frames=c["frames"])
    np.testing.assert_allclose(ref["frame_loss"].sum(), loss, rtol=1e-5)
    ratio = worst(np.abs(ref["grad"] - np.moveaxis(grad[:, :, times], -1, 0)), K2R.grad_tol(ref))
    print(f"\n{sz}: |restatement - autograd| / (1e-4 scale abs_sum) <= {ratio:.3g}")
    assert ratio <= 1.0
    assert not grad[:, :, K2R.UNUSED].any()
    assert ref["abs_sum"][:6].any(axis=(1, 2)).all() and not ref["abs_sum"][6].any()          # F6: all-zero traces


SLAB = slice(1000, 1064)     # the large volumes: 64 rows in the middle, two x-blocks' worth


@pytest.mark.parametrize("sz", K2R.SHAPES + K2R.LARGE)
def test_flip_condition(sz):
    """The gradient jumps where a source coordinate crosses an integer, and the kernel's fused coordinate chain may differ from
    the reference's by an ulp.  So the restatement is evaluated at its own coordinates and with every coordinate one fp32 step
    up, then down: the three gradients must agree to a quarter of what the GPU test allows the kernel, entry by entry, for the
    fit call and for the call with an upstream gradient, and the three reconstructions voxel by voxel.  A case that fails gets
    another seed or shift, never another factor (k2_restatement.SEED).
    The two large volumes take 3.5 s per frame and evaluation, so both calls run on the 64-row slab SLAB of the same warps -- and
    the call with an upstream gradient once more on the whole volume for F5, the one frame whose samples cross the far border
    planes at every fraction (what made K2 and the restatement differ before the large images were tapered: k2_restatement.SEED)."""
    c = K2R.k2_case(sz)
    smax = np.abs(c["S32"]).max()
    every = list(range(len(c["times"])))
    plan = [("gout", None, every), ("frames", None, every)]
    if sz in K2R.LARGE:
        plan = [("gout", SLAB, every), ("frames", SLAB, every), ("gout", None, [1])]
    for other, rows, sel in plan:
        kw = {other: c[other][sel], "norm_frames": c["norm_frames"], "rows": rows}
        runs = [K2R.k2(c["S32"][sel], c["beta"], sz, [c["times"][i] for i in sel], nudge=n, **kw) for n in (0, 1, -1)]
        grads = np.stack([r["grad"] for r in runs])
        spread = grads.max(0) - grads.min(0)
        ratio = worst(spread, 0.25 * K2R.grad_tol(runs[0]))
        recs = np.stack([r["recon"] for r in runs])
        rtol = 0.25 * K2R.recon_tol(runs[0], smax)
        rr = float(((recs.max(0) - recs.min(0)).reshape(len(sel), -1).max(1) / rtol).max())
        print(f"\n{sz} {other} rows {rows} frames {sel}: gradient spread / (0.25 tol) <= {ratio:.3g}, recon spread / (0.25 tol) <= {rr:.3g}")
        assert ratio <= 1.0 and rr <= 1.0
