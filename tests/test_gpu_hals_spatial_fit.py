"""The exact footprint solver K6h through the model: ``update_footprints(live_spatial=True, spatial_solver='hals')`` on
the planted video of tests/test_hals_spatial_host.py (footprints 1.5 x too narrow, exact traces), a two-colour
``MultiChannelDNMF`` step against the restatement on its fused sums, and the default arguments, which must stay the
multiplicative path bit for bit.

Measured on MI355X (5 HALS sweeps with grow=2 against 5 multiplicative updates, the objective on the frames as the model
registered them, the truth registered the same way), list and dense form alike: depth 2 objective -5130.81 against
-5097.26, correlation with the true footprints 0.9998 against 0.9932; depth 1 -1934.67 against -1917.27, 0.9998 against
0.9882.  Asserted is the ordering the host test asserts.  A step of either form, one or two colours, is within 0.500 ulp of
the restatement on its sums (the rounding to fp32)."""
import numpy as np
import pytest
import torch

import hals_spatial_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd.Demix import dNMF
    return dNMF


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def planted_model(M, pl, kernel="auto"):
    sz, (K, T) = pl["sz"], pl["C"].shape
    dn = M.DeformableNMF(torch.tensor(sz), K, T, positions=torch.from_numpy(pl["centres"]).float())
    dn.verbose = False
    dn.spatial_kernel = kernel
    dn.fp.A = dev(pl["A_narrow"]).reshape(*sz, K)
    dn.C = dev(pl["C"])
    return dn


def figures(dn, pl):
    """(objective on the model's registered frames and traces, correlation of its footprints with the truth).  The footprints
    live in the coordinates the model registers the frames to, so the truth is the true footprints registered as the frames
    were (K7 is a gather: the registered video is the traces times these images, plus noise).  At depth 1 that is the identity
    map; at depth 2 the warp the model starts from samples the two slices half a voxel off."""
    from dnmf_amd import ops
    reg, C = dn._reg_buf.double().cpu().numpy(), dn.C.double().cpu().numpy()
    K = C.shape[0]
    A = dn.fp.A.reshape(-1, K).double().cpu().numpy()
    truth = ops.image_iwarp(dev(pl["A_true"].T), None, pl["sz"], dn.fp.beta.detach(), list(range(K))).cpu().numpy().T
    return R.objective(A, reg.T @ C.T, C @ C.T), R.footprint_correlation(A, truth)


@pytest.mark.parametrize("kernel", ["auto", "dense"])
@pytest.mark.parametrize("depth", [2, 1])
def test_hals_beats_mu_on_narrow_footprints(M, depth, kernel):
    pl = R.planted(depth)
    sz, K = pl["sz"], 6
    loader = M.ResidentLoader(dev(pl["video"]), sz, 8)
    mu, hals = planted_model(M, pl, kernel), planted_model(M, pl, kernel)
    # iter_c = 0: the traces stay the exact ones
    mu.update_footprints(loader, 8, sz, gamma_c=0, gamma_a=0, iter_c=0, live_spatial=True, iter_a=5)
    hals.update_footprints(loader, 8, sz, gamma_c=0, gamma_a=0, iter_c=0, live_spatial=True, iter_a=5, spatial_solver='hals', grow=2)
    assert torch.equal(mu.C, hals.C) and torch.equal(mu._reg_buf, hals._reg_buf)
    (f_mu, r_mu), (f_hals, r_hals) = figures(mu, pl), figures(hals, pl)
    print(f"\ndepth {depth} {kernel}: objective hals {f_hals:.2f} mu {f_mu:.2f}; correlation hals {r_hals:.4f} mu {r_mu:.4f}; "
          f"kkt {hals.last_spatial_kkt.numpy()}")
    assert f_hals <= f_mu and r_hals > r_mu
    kkt = hals.last_spatial_kkt
    assert tuple(kkt.shape) == (K,) and kkt.dtype == torch.float64 and not kkt.is_cuda and bool(torch.isfinite(kkt).all())
    assert mu.last_spatial_kkt is None
    # the grown support was used, and only it
    A, A0 = hals.fp.A.reshape(-1, K).cpu().numpy(), pl["A_narrow"]
    inside = R.box_mask(R.dilate_boxes(R.support_boxes(A0, sz), sz, 2), sz)
    assert ((A > 0) & (A0 == 0)).any() and (A[~inside] == 0).all()
    assert np.array_equal(mu.fp.A.reshape(-1, K).cpu().numpy() != 0, A0 != 0)      # the multiplicative update cannot


def test_both_forms_of_one_step_agree_with_the_restatement(M):
    """One 'hals' spatial_step of the single-channel model in the list form and in the dense form, each against the
    restatement on the sums it left in the model's buffer (dense) or made by the same K5 call (lists)."""
    from dnmf_amd import ops
    pl = R.planted(1)
    sz, K, P = pl["sz"], 6, 480
    frames = dev(pl["video"])
    D = np.random.default_rng(5).random((*sz, K)).astype(np.float32)
    for kernel in ("lists", "dense"):
        dn = planted_model(M, pl, kernel)
        boxes = ops.dilate_boxes(dn.fp.packed_lists(floor=0.0)["bbox"], sz, (2, 1, 0))
        if kernel == "lists":
            sl = ops.spatial_lists_setup({"bbox": boxes}, K, sz)
            A1c, Cs, _ = ops.spatial_accum_lists(frames, dn.C, sl, sz, K)
            A1 = R.expand_entries(A1c.cpu().numpy(), sl["tables"].cpu().numpy(), sl["ntiles"], sz, K)
            cached = dn._spatial_lists()
        got = dn.spatial_step(frames, D=D, gamma=0.25, solver='hals', sweeps=3, grow=(2, 1, 0)).reshape(P, K).cpu().numpy()
        if kernel == "dense":
            A1, Cs = dn._spatial_buf[:P * K].view(P, K).cpu().numpy(), dn._spatial_buf[P * K:].view(K, K)
        Cs64, b = Cs.double().cpu().numpy(), boxes.cpu().numpy()
        want = R.hals_spatial(pl["A_narrow"], A1, Cs64, D=D.reshape(P, K), gamma=0.25, sweeps=3, boxes=b, sz=sz)
        err = np.abs(got.astype(np.float64) - want)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        print(f"\n{kernel}: largest deviation {err.max():.3e}, {(err / ulp).max():.3f} ulp")
        assert (err[want != 0] <= ulp[want != 0]).all() and (got[want == 0] == 0).all()
        want_kkt = R.kkt(want, A1, Cs64, D=D.reshape(P, K), gamma=0.25, boxes=b, sz=sz)
        terms = R.term_sum(want, A1, Cs64, D=D.reshape(P, K), gamma=0.25, boxes=b, sz=sz).max(0)
        assert (np.abs(dn.last_spatial_kkt.numpy() - want_kkt) <= 1e-12 * terms).all()
        if kernel == "lists":
            assert sl["total"] > cached["total"]         # lists of the grown boxes; the cached ones were not touched
            assert dn._sl is None                        # ... and are dropped with the footprints they described, as ever


def test_two_colour_step_equals_the_restatement_on_its_fused_sums(M):
    from dnmf_amd import ops
    pl = R.planted(1)
    sz, K, P = pl["sz"], 6, 480
    T = pl["C"].shape[1]
    colours = torch.tensor([[1.0, 0.6, 0.3, 0.9, 0.5, 0.8], [0.2, 0.7, 1.0, 0.4, 0.9, 0.1]])
    dn = M.MultiChannelDNMF(torch.tensor(sz), K, T, colours, positions=torch.from_numpy(pl["centres"]).float())
    dn.verbose = False
    dn.spatial_kernel = "lists"
    dn.fp.A = dev(pl["A_narrow"]).reshape(*sz, K)
    dn.C = dev(pl["C"])
    video = torch.from_numpy(pl["video"])
    frames = torch.cat([video * 0.9, video * 0.5 + 0.05], dim=1).to("cuda").contiguous()     # rows of 2 P floats
    boxes = ops.dilate_boxes(dn.fp.packed_lists(floor=0.0)["bbox"], sz, 1)
    sl = ops.spatial_lists_setup({"bbox": boxes}, K, sz)
    A1c, Cs, _ = ops.spatial_accum_lists_channels(frames, dn.C, dn.colours, sl, sz, K)
    Cs.mul_(dn.colours.T @ dn.colours)
    A1 = R.expand_entries(A1c.cpu().numpy(), sl["tables"].cpu().numpy(), sl["ntiles"], sz, K)
    got = dn.spatial_step(frames, gamma=0.0, solver='hals', sweeps=4, grow=1).reshape(P, K).cpu().numpy()
    b = boxes.cpu().numpy()
    want = R.hals_spatial(pl["A_narrow"], A1, Cs.double().cpu().numpy(), sweeps=4, boxes=b, sz=sz)
    err = np.abs(got.astype(np.float64) - want)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print(f"\ntwo colours: largest deviation {err.max():.3e}, {(err / ulp).max():.3f} ulp")
    assert (err[want != 0] <= ulp[want != 0]).all() and (got[want == 0] == 0).all()
    assert tuple(dn.last_spatial_kkt.shape) == (K,) and dn._chan_fp is None
    # and through update_footprints: the arguments reach the step
    loader = M.ResidentLoader(frames, sz, 8)
    dn.update_footprints(loader, 8, sz, gamma_c=0, gamma_a=0, iter_c=2, live_spatial=True, iter_a=2, spatial_solver='hals', grow=1)
    assert dn.last_spatial_kkt is not None and bool(torch.isfinite(dn.last_spatial_kkt).all())


def test_default_arguments_are_the_multiplicative_path_bit_for_bit(M):
    from dnmf_amd import ops
    pl = R.planted(2)
    sz = pl["sz"]
    frames = dev(pl["video"])
    loader = M.ResidentLoader(frames, sz, 8)
    a, b, c = planted_model(M, pl), planted_model(M, pl), planted_model(M, pl)
    a.last_spatial_kkt = torch.zeros(6)
    a.update_footprints(loader, 8, sz, gamma_c=0, gamma_a=0.2, iter_c=3, live_spatial=True, iter_a=2)
    # the same call written as before this solver existed: the steps by hand
    b.update_footprints(loader, 8, sz, gamma_c=0, iter_c=3)
    reg = ops.image_iwarp(frames, None, sz, b.fp.beta.detach(), list(range(frames.shape[0])))
    for _ in range(2):
        b.spatial_step(reg, D=b.D, gamma=0.2, times=list(range(frames.shape[0])))
    assert torch.equal(a.fp.A, b.fp.A) and torch.equal(a.C, b.C) and a.last_spatial_kkt is None
    c.update_footprints(loader, 8, sz, gamma_c=0, gamma_a=0.2, iter_c=3, live_spatial=True, iter_a=2, spatial_solver='mu', grow=0)
    assert torch.equal(a.fp.A, c.fp.A)
    for bad in (dict(grow=2), dict(grow=(1, 0, 0)), dict(sweeps=3)):
        with pytest.raises(ValueError, match="hals"):
            b.spatial_step(reg, gamma=0.2, **bad)
    with pytest.raises(ValueError, match="grow"):
        b.spatial_step(reg, solver='hals', grow=-1)
    with pytest.raises(ValueError, match="sweeps"):
        b.spatial_step(reg, solver='hals', sweeps=0)
    with pytest.raises(ValueError):
        b.update_footprints(loader, 8, sz, live_spatial=True, spatial_solver='hals', iter_a=0)
    with pytest.raises(ValueError, match="hals"):
        b.update_footprints(loader, 8, sz, live_spatial=True, grow=1)
    assert torch.equal(a.fp.A, b.fp.A)        # refused before anything was written


def test_update_spatial_static_hals(M):
    """numpy in, float64 numpy out: the dense K5 and ``sweeps`` sweeps of K6h, against the restatement on float64 sums (the
    fp32 MFMA sums of K5 differ from them by 1e-6 relative; the solution inherits that, scaled by the conditioning of Cs)."""
    pl = R.planted(1)
    sz, K = pl["sz"], 6
    A0 = pl["A_narrow"].reshape(*sz, K)
    Yi = np.ascontiguousarray(pl["video"].T).reshape(*sz, -1)
    boxes = R.dilate_boxes(R.support_boxes(pl["A_narrow"], sz), sz, 2)
    got = M.DeformableNMF.update_spatial(A0, pl["C"], Yi, solver='hals', sweeps=5, boxes=boxes)
    Y, C = pl["video"].astype(np.float64), pl["C"].astype(np.float64)
    want = R.hals_spatial(pl["A_narrow"], Y.T @ C.T, C @ C.T, sweeps=5, boxes=boxes, sz=sz).reshape(*sz, K)
    assert got.dtype == np.float64 and got.shape == A0.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-4 * np.abs(want).max())
    mu = M.DeformableNMF.update_spatial(A0, pl["C"], Yi)
    assert np.array_equal(mu != 0, A0 != 0) and ((got > 0) & (A0 == 0)).any()
