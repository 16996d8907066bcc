"""The Gauss-Newton motion solver on the GPU: K16 and dnmf_lm_step against tests/gn_restatement.py on the very same fp32
inputs, against K2 and the reference's captured gradient, and update_motion(solver='gn') on noise-free problems.

Tolerances:
  H      |dH_ij| <= 1e-4 sqrt(H_ii H_jj), g: |dg_i| <= 1e-4 max|g|   fp32 sums of P terms in another order (K2's gradient bound)
         -- a bound by the diagonal and by the largest entry: an entry that is small beside them may be wrong by many times its
         own size, and no shape of check_eqs has Z > 3, where alone the z exponents 3 and 4 differ from 1 and 2.  The bound by
         the entry's own absolute sum, at shapes with Z = 4 and 5, is tests/test_gpu_k16_float64.py's; these tests stay.
  sse    rtol 1e-5
  step   the device writes the next trial as fp32(beta_acc + d beta); against fp32 of the restatement's float64 sum it may differ
         by 100 kappa 2.2e-16 max|d beta| (kappa: condition number of the damped scaled system) plus one fp32 rounding
"""
import numpy as np
import pytest
import torch

import gn_restatement as GN
from conftest import golden
from oracle import dnmf_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(12, 10, 1), (12, 10, 2), (9, 7, 3), (40, 130, 2), (70, 300, 1)]


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd.Demix import dNMF
    return dNMF


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def halo_images(S32, sz):
    """(T,X,Y,Z) fp32 images -> (T, lds) rows in the halo layout, zero border."""
    from dnmf_amd import ops
    out = torch.zeros((S32.shape[0], ops.halo_voxels(sz)), dtype=torch.float32, device="cuda")
    ops.halo_interior(out, sz).copy_(dev(S32))
    return out


def k16_case(sz, seed=0):
    """K = 5 Gaussians (some cut by the border), T = 6 frames: warps off the identity by several voxels (taps in the halo and
    wholly outside), frame 5 with a NaN coefficient, frame 0 with all-zero traces; frames stored in shuffled rows."""
    rng = np.random.default_rng(seed)
    sz = [int(s) for s in sz]
    T, K = 6, 5
    pos = np.stack([rng.uniform(-1, s, K) for s in sz], 1).astype(np.float32)
    A = O.gaussian_footprints(sz, pos, np.full(K, 3.0, np.float32))
    C = rng.uniform(0.5, 1.5, (K, T)).astype(np.float32)
    C[:, 0] = 0.0
    ext = np.array([max(s - 1, 1) for s in sz], dtype=np.float64)
    # Displacements are sized per target axis d, so that a thin or short axis is left by some samples and not by all of
    # them: shift and quadratic terms times amp_d = min(1, (S_d - 1) / 8), and an affine term from axis a moves d by at most
    # 0.15 of the shorter of the two extents.
    amp = np.minimum(1.0, ext / 8.0)
    beta = O.identity_beta(T).astype(np.float64)
    beta[0] += rng.uniform(-3, 3, (3, T)) * amp[:, None]
    beta[0, 0, 4] += 5.0                                   # frame 4: the first rows sample wholly outside
    beta[1:4] += rng.uniform(-0.15, 0.15, (3, 3, T)) * np.minimum(1.0, ext[None, :] / ext[:, None])[:, :, None]
    for a in range(4, 10):
        beta[a] += rng.uniform(-2, 2, (3, T)) * amp[:, None] / np.prod(ext ** GN.EXPO[a])
    beta = beta.astype(np.float32)
    beta[7, 1, 5] = np.nan
    frames = rng.uniform(0, 1, (T, *sz)).astype(np.float32)
    S32 = GN.recon_images(A, C, range(T)).astype(np.float32)
    rows = rng.permutation(T + 2)[:T]                      # frame t lives in row rows[t] of a buffer of T + 2 rows
    buf = np.zeros((T + 2, int(np.prod(sz))), np.float32)
    buf[rows] = frames.reshape(T, -1)
    return {"sz": sz, "beta": beta, "frames": frames, "S32": S32, "rows": rows, "buf": buf, "T": T}


def k16(c, times, out=None, accumulate=False):
    from dnmf_amd import ops
    tt = torch.tensor(times, dtype=torch.int32, device="cuda")
    res = ops.warp_normal_eqs(halo_images(c["S32"], c["sz"]), tt, dev(c["buf"]), dev(c["rows"][times], torch.int32), c["sz"],
                              dev(c["beta"]), tt, out=out, accumulate=accumulate)
    torch.cuda.synchronize()
    return res


def check_eqs(got, want, scale=1.0):
    H, g, sse = (got[k].cpu().numpy() / scale for k in ("H", "g", "sse"))
    Hw, gw, sw = want
    for b in range(len(sw)):
        d = np.sqrt(np.outer(np.diag(Hw[b]), np.diag(Hw[b])))
        assert (np.abs(H[b] - Hw[b]) <= 1e-4 * d).all(), (b, np.abs(H[b] - Hw[b]).max())
        assert (np.abs(g[b] - gw[b]) <= 1e-4 * np.abs(gw[b]).max()).all(), b
        if np.isnan(sw[b]):
            assert np.isnan(sse[b]) and not H[b].any() and not g[b].any()
        else:
            np.testing.assert_allclose(sse[b], sw[b], rtol=1e-5)
        assert (H[b] == H[b].T).all()                       # bit for bit


@pytest.mark.parametrize("sz", SHAPES)
def test_k16_against_the_restatement(M, sz):
    c = k16_case(sz)
    for times in ([4, 1, 3], [5, 0, 2]):
        want = GN.normal_eqs(None, None, c["beta"], sz, times, c["frames"][times], S=c["S32"][times])
        got = k16(c, times)
        check_eqs(got, want)
        if times[0] == 5:
            assert np.isnan(want[2][0]) and not want[0][1].any() and want[2][1] > 0      # NaN frame; zero traces: H = 0
        else:
            assert all(want[0][b].any() for b in range(3))
        if sz[2] == 1:
            off = np.setdiff1d(np.arange(30), GN.active(sz))
            H, g = got["H"].cpu().numpy(), got["g"].cpu().numpy()
            assert not H[:, off].any() and not H[:, :, off].any() and not g[:, off].any()   # exact zeros
        once = {k: got[k].clone() for k in ("H", "g", "sse")}
        twice = k16(c, times, out=got, accumulate=True)
        assert twice["H"].data_ptr() == got["H"].data_ptr()
        check_eqs(twice, want, scale=2.0)
        np.testing.assert_array_equal((2 * once["H"]).cpu().numpy(), twice["H"].cpu().numpy())   # x + x is exact


def test_k16_gradient_is_the_references_and_k2s(M):
    from dnmf_amd import ops
    g = golden("G3_grad")
    sz = [int(s) for s in g["sz"]]
    A = O.gaussian_footprints(sz, g["positions"], np.full(4, 3.0))
    P = int(np.prod(sz))
    for label in ["id_b1", "id_b3", "pert_b1", "pert_b3", "pert_b4"]:
        times = g[label + "_times"].tolist()
        B = len(times)
        frames = np.ascontiguousarray(np.moveaxis(g["video"][..., times], -1, 0)).astype(np.float32)
        beta = dev(g[label + "_beta"])
        S = halo_images(GN.recon_images(A, g["C"], times).astype(np.float32), sz)
        tt = torch.tensor(times, dtype=torch.int32, device="cuda")
        fr = dev(frames.reshape(B, -1))
        eq = ops.warp_normal_eqs(S, None, fr, None, sz, beta, tt)
        grad = torch.zeros_like(beta)
        ops.warp_recon_grad(S, None, fr, None, sz, beta, tt, grad=grad)
        want, k2 = g[label + "_grad"], grad.cpu().numpy()
        tol = 1e-4 * np.abs(want).max()
        for b, t in enumerate(times):
            got = GN.to_raw_grad(eq["g"][b].cpu().numpy(), sz) * 2.0 / (B * P)
            assert np.abs(got - want[:, :, t]).max() <= tol, label
            assert np.abs(got - k2[:, :, t]).max() <= tol, label
        np.testing.assert_allclose(float(eq["sse"].sum()) / (B * P), g[label + "_loss"], rtol=1e-5)


@pytest.mark.parametrize("sz", SHAPES[:3])
def test_k2_and_k16_see_the_same_sample_bit_for_bit(M, sz):
    """K2 and K16 call one warped sample (csrc/warp_taps.hpp) and reduce a block the same way, and these shapes are one block
    per frame: K2's finish kernel then adds a single partial sum and K16's float64 finish converts a single fp32 one.  So on the
    same images, frames and coefficients K2's per-frame loss is K16's sse and K2's gradient of the constant term is K16's g of
    it, up to the one fp32 scaling K2's finish kernel applies -- exactly."""
    from dnmf_amd import ops
    c = k16_case(sz)
    times = [0, 1, 2, 3, 4]                     # the finite frames; frame 4's first rows sample outside the volume
    B, P = len(times), int(np.prod(sz))
    eq = k16(c, times)
    tt = torch.tensor(times, dtype=torch.int32, device="cuda")
    grad = torch.zeros_like(dev(c["beta"]))
    k2 = ops.warp_recon_grad(halo_images(c["S32"], c["sz"]), tt, dev(c["buf"]), dev(c["rows"][times], torch.int32), c["sz"],
                             dev(c["beta"]), tt, grad=grad)
    torch.cuda.synchronize()
    sse, g = eq["sse"].cpu().numpy(), eq["g"].cpu().numpy()
    loss, grad = k2["frame_loss"].cpu().numpy(), grad.cpu().numpy()
    n = np.float32(B) * np.float32(P)
    assert np.isfinite(sse).all() and g[1:].any()
    np.testing.assert_array_equal(sse.astype(np.float32).astype(np.float64), sse)
    np.testing.assert_array_equal(loss, sse.astype(np.float32) * (np.float32(1) / n))
    for d in range(3 if sz[2] > 1 else 2):
        np.testing.assert_array_equal(grad[0, d, times], (np.float32(2) / n) * g[:, d].astype(np.float32))


def lm_inputs(sz, B, seed):
    rng = np.random.default_rng(seed)
    J = rng.normal(size=(B, 60, 30)) * rng.uniform(0.1, 10, (1, 1, 30))
    H = np.einsum("bpi,bpj->bij", J, J)
    g = rng.normal(size=(B, 30))
    if sz[2] == 1:
        off = np.setdiff1d(np.arange(30), GN.active(sz))
        H[:, off], H[:, :, off], g[:, off] = 0, 0, 0
    return H, g


@pytest.mark.parametrize("sz", [(12, 10, 1), (9, 7, 3)])
def test_lm_step_against_the_restatement(M, sz):
    from dnmf_amd import ops
    B, T = 3, 5
    times = [3, 0, 4]
    H1, g1 = lm_inputs(sz, B, 1)
    H2, g2 = lm_inputs(sz, B, 2)
    rng = np.random.default_rng(5)
    beta0 = (O.identity_beta(T) + rng.normal(size=(10, 3, T)).astype(np.float32) * 1e-2).astype(np.float32)
    calls = [(H1, g1, np.array([5.0, 6.0, 7.0])), (H2, g2, np.array([4.0, 6.5, np.nan])), (H1, g2, np.array([4.5, 5.0, 1.0]))]

    def run(keep, nan_frame=None):
        """Device and restatement side by side on the frames ``keep`` of the calls; returns the device's final beta."""
        tk = [times[i] for i in keep]
        ref_beta, ref = beta0.copy(), GN.new_state(len(keep))
        if nan_frame is not None:
            ref_beta[:, :, times[nan_frame]] = np.nan
        beta, st = dev(ref_beta), ops.lm_state(len(keep), "cuda")
        tt = torch.tensor(tk, dtype=torch.int32, device="cuda")
        for n, (H, g, sse) in enumerate(calls):
            H, g, sse = H[keep].copy(), g[keep].copy(), sse[keep].copy()
            if nan_frame is not None:
                j = keep.index(nan_frame)
                H[j], g[j], sse[j] = 0.0, 0.0, np.nan            # what K16 gives for a NaN frame
            last = n == len(calls) - 1
            out = GN.lm_step(ref, H, g, sse, ref_beta, tk, sz, accept_only=last)
            ops.lm_step(st, {"H": dev(H, torch.float64), "g": dev(g, torch.float64), "sse": dev(sse, torch.float64)}, sz, beta, tt,
                        accept_only=last)
            got = beta.cpu().numpy()
            np.testing.assert_array_equal(st["counts"].cpu().numpy(), ref["counts"])      # identical decisions
            np.testing.assert_array_equal(st["lam"].cpu().numpy(), ref["lam"])
            np.testing.assert_array_equal(st["beta"].cpu().numpy(), ref["beta"])
            np.testing.assert_array_equal(st["sse"].cpu().numpy(), ref["sse"])
            for j, t in enumerate(tk):
                if not np.isfinite(ref_beta[:, :, t]).all():
                    assert np.isnan(got[:, :, t]).any() and np.isnan(ref_beta[:, :, t]).any()
                    continue
                Ah, _, _ = GN.damped_system(ref["H"][j], ref["g"][j], ref["lam"][j], sz)
                kappa = np.linalg.cond(Ah)
                tol = 100 * kappa * 2.2e-16 * np.abs(out["dbeta"][j]).max() + 6e-8 * np.abs(ref_beta[:, :, t])
                assert (np.abs(got[:, :, t].astype(np.float64) - ref_beta[:, :, t]) <= tol).all(), (n, j, kappa)
            untouched = [t for t in range(T) if t not in tk]
            np.testing.assert_array_equal(got[:, :, untouched], beta0[:, :, untouched])
        return got

    run([0, 1, 2])
    with_nan = run([0, 1, 2], nan_frame=1)
    without = run([0, 2])
    assert np.isnan(with_nan[:, :, times[1]]).any()
    np.testing.assert_array_equal(with_nan[:, :, [times[0], times[2]]], without[:, :, [times[0], times[2]]])   # bit for bit


def test_lm_step_zero_H_leaves_beta(M):
    from dnmf_amd import ops
    sz = (12, 10, 2)
    beta = dev(O.identity_beta(2))
    z = {"H": torch.zeros((2, 30, 30), dtype=torch.float64, device="cuda"), "g": torch.zeros((2, 30), dtype=torch.float64, device="cuda"),
         "sse": torch.ones((2,), dtype=torch.float64, device="cuda")}
    ops.lm_step(ops.lm_state(2, "cuda"), z, sz, beta, [1, 0])
    np.testing.assert_array_equal(beta.cpu().numpy(), O.identity_beta(2))


# ---- the fit ---------------------------------------------------------------------------------------------------------
ITERS = 8
FIT_SHAPES = [(24, 20, 2), (24, 20, 1), (24, 20, 5)]


@pytest.fixture(scope="module")
def problems():
    return {sz: GN.fit_problem(sz) for sz in FIT_SHAPES}


def make_model(M, sz, p, cls=None, **kw):
    K, T = p["C"].shape
    model = (cls or M.DeformableNMF)(torch.tensor(sz), K, T, positions=torch.from_numpy(p["pos"]), **kw)
    model.fp.A = dev(p["A"])
    model.C = dev(p["C"])
    model.verbose = False
    return model


def resident(M, sz, frames, batch=2):
    return M.ResidentLoader(dev(frames.reshape(frames.shape[0], -1)), sz, batch)


@pytest.mark.parametrize("sz", FIT_SHAPES)
def test_fit_converges_without_a_step_size(M, problems, monkeypatch, sz):
    """fit_problem(sz): shift <= 0.6 voxel, affine <= 0.03, quadratic terms <= 0.25 voxel at the far corner, in-plane, start at
    the identity 0.87 .. 1.92 voxels off (24x20x2; 0.72 .. 1.78 at 24x20x1; up to 1.99 at 24x20x5, the one fit at Z > 2: all 30
    unknowns with u_z at five values).  The float64 restatement (fit_gn, 8 iterations) ends at most 3.2e-5 (24x20x2) / 3.7e-6
    (24x20x1) / 4.9e-6 (24x20x5) voxel off with sse / sse0 <= 7e-12 / 3e-11 / 8e-12 -- tests/test_gn_host.py asserts < 0.01 voxel
    and <= 1e-6."""
    from dnmf_amd import ops
    p = problems[sz]
    T = p["C"].shape[1]
    model = make_model(M, sz, p)
    history, real = [], ops.lm_step

    def spy(state, *a, **kw):
        out = real(state, *a, **kw)
        history.append(state["sse"].clone())
        return out

    monkeypatch.setattr(ops, "lm_step", spy)
    grad_before = model.fp.beta.grad
    model.update_motion(resident(M, sz, p["frames"]), None, solver='gn', iters=ITERS)
    assert len(history) == ITERS + 1
    for a, b in zip(history, history[1:]):
        assert bool((b <= a).all())
    beta = model.fp.beta.detach().cpu().numpy()
    err = GN.field_error(beta, p["beta_true"], sz)
    st = model.last_motion_gn
    ratio = (st["sse"] / st["sse0"]).cpu().numpy()
    print(f"\n{sz}: gn field error {err:.3g} voxel, sse/sse0 {ratio.max():.3g}, accepted {st['accepted'].tolist()}, "
          f"rejected {st['rejected'].tolist()}")
    assert model.fp.beta.requires_grad and model.fp.beta.grad is grad_before
    assert all(st[k].is_cuda and st[k].shape == (T,) for k in ("sse0", "sse", "accepted", "rejected", "lam"))
    assert err < 0.05
    assert (ratio <= 1e-6).all()
    # the demo's Adam on the same problem for the same number of passes over the data: printed, not asserted
    monkeypatch.setattr(ops, "lm_step", real)
    adam = make_model(M, sz, p)
    opt = torch.optim.Adam([adam.fp.beta], lr=1e-5)
    adam.update_motion(resident(M, sz, p["frames"]), opt, epochs=ITERS + 1)
    print(f"{sz}: adam lr=1e-5, {ITERS + 1} epochs: field error "
          f"{GN.field_error(adam.fp.beta.detach().cpu().numpy(), p['beta_true'], sz):.3g} voxel "
          f"(start {GN.field_error(O.identity_beta(T), p['beta_true'], sz):.3g})")


class HostFrames(torch.utils.data.Dataset):
    def __init__(self, frames):
        self.frames = torch.from_numpy(frames)

    def __len__(self):
        return self.frames.shape[0]

    def __getitem__(self, i):
        return self.frames[i], i


def test_fit_is_the_same_from_every_loader_and_chunking(M, problems):
    sz = (24, 20, 2)
    p = problems[sz]
    T = p["C"].shape[1]

    def fit(loader, **attrs):
        model = make_model(M, sz, p)
        for k, v in attrs.items():
            setattr(model, k, v)
        model.update_motion(loader, None, solver='gn', iters=ITERS)
        return model.fp.beta.detach().cpu().numpy()

    one = fit(resident(M, sz, p["frames"]))
    np.testing.assert_array_equal(fit(resident(M, sz, p["frames"]), motion_chunk=2), one)       # 2 + 2 + 1 frames
    staged = fit(torch.utils.data.DataLoader(HostFrames(p["frames"]), batch_size=2, shuffle=True))
    order = [3, 0, 4, 2, 1]
    batches = [(torch.from_numpy(p["frames"][order[i:i + 2]]), torch.tensor(order[i:i + 2])) for i in range(0, T, 2)]
    host = fit(batches, stream_loader=False)                                                    # batch by batch from the host
    errs = [GN.field_error(b, p["beta_true"], sz) for b in (one, staged, host)]
    assert max(errs) < 0.05 and max(errs) - min(errs) <= 1e-3, errs


def test_fit_multichannel(M, problems):
    sz = (24, 20, 1)
    p = problems[sz]
    K, T = p["C"].shape
    colours = np.array([[1.0, 0.5, 0.2, 1.0, 0.7, 0.3], [0.3, 1.0, 0.8, 0.1, 0.6, 1.0]], np.float32)
    basis = O.quadratic_basis(O.voxel_lattice(sz))
    frames = np.stack([O.forward(p["A"] * colours[c], basis, p["beta_true"], sz, list(range(T)), p["C"])[0] for c in range(2)], 1)
    model = make_model(M, sz, p, cls=M.MultiChannelDNMF, colours=colours)
    model.update_motion(resident(M, sz, frames.astype(np.float32)), None, solver='gn', iters=ITERS)
    assert GN.field_error(model.fp.beta.detach().cpu().numpy(), p["beta_true"], sz) < 0.05
    assert bool((model.last_motion_gn["sse"] <= 1e-6 * model.last_motion_gn["sse0"]).all())


@pytest.mark.parametrize("fused", [True, False])
def test_adam_default_is_unchanged(M, problems, fused):
    sz = (24, 20, 2)
    p = problems[sz]

    def run(**kw):
        model = make_model(M, sz, p)
        model.fused_motion = fused
        opt = torch.optim.Adam([model.fp.beta], lr=1e-3)
        model.update_motion(resident(M, sz, p["frames"]), opt, epochs=2, **kw)
        s = opt.state[model.fp.beta]
        return [t.detach().cpu().numpy() for t in (model.fp.beta, s["exp_avg"], s["exp_avg_sq"])]

    for a, b in zip(run(), run(solver='adam')):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(run()[0], O.identity_beta(p["C"].shape[1]))
