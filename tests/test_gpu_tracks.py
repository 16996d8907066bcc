"""K11 / K12 / K13 on the GPU against their numpy float64 restatement (tests/tracks_restatement.py) and the fixture G12, and
the public methods built on them (ExponentialFP.beta_from_positions / positions, DeformableNMF.init_motion / positions,
WUtils.Simulator.get_roi_signals)."""
import numpy as np
import pytest
import torch

import tracks_restatement as TR
from conftest import golden

pytestmark = pytest.mark.gpu

JITTER = np.array([1.0, 1e-2, 1e-2, 1e-2, 1e-4, 1e-4, 1e-4, 1e-4, 1e-4, 1e-4])


@pytest.fixture(scope="module")
def M():
    from dnmf_amd.Demix import dNMF
    return dNMF


@pytest.fixture(scope="module")
def ops():
    from dnmf_amd import ops
    return ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return t if dtype is None else t.to(dtype)


def corners(sz):
    return np.array([[x, y, z] for x in (0, sz[0] - 1) for y in (0, sz[1] - 1) for z in (0, sz[2] - 1)], dtype=np.float64)


def near_identity(rng, sz, T, scale=1.0):
    """beta (10,3,T) float64 near the identity: shifts of a voxel, 1 % linear terms, quadratic terms that move a corner of
    a 64-voxel axis by a fraction of a voxel (scaled down with the volume so that the map stays invertible)."""
    s = max(sz)
    amp = JITTER * np.array([1, 1, 1, 1] + [64.0 / s] * 6) * scale
    b = TR.IDENTITY[:, :, None] + rng.randn(10, 3, T) * amp[:, None, None]
    if sz[2] == 1:
        b[:, 2] = TR.IDENTITY[:, 2:3]
        b[[3, 6, 8, 9]] = TR.IDENTITY[[3, 6, 8, 9]][:, :, None]
    return b


# ---- K13 ------------------------------------------------------------------------------------------------------------
def test_roi_signals_equal_the_reference_fixture(ops):
    """K13 against G12 (the reference's get_roi_signals): float64 sums against the reference's float32 ones, N 2^-23."""
    from dnmf_amd.WUtils import Simulator as S
    g = golden("G12_roi")
    frames = dev(np.moveaxis(g["video"], 3, 0).reshape(5, -1))
    for i in (0, 1):
        w = g[f"window{i}"]
        n = int(np.prod(2 * w + 1))
        for P in (dev(g["P"]), dev(g["P"]).double()):
            got = ops.roi_signals(frames, (20, 16, 2), P, w.tolist()).cpu().numpy()
            print(f"window {w.tolist()} {P.dtype}: max relative error {np.abs(got / g[f'signals{i}'] - 1).max():.3e}")
            np.testing.assert_allclose(got, g[f"signals{i}"], rtol=n * 2.0 ** -23, atol=0)
        # the reference's signature: (X,Y,Z,T) video, numpy or torch, host or device
        for video, P in ((g["video"], g["P"]), (torch.from_numpy(g["video"]), torch.from_numpy(g["P"])),
                         (dev(g["video"]), dev(g["P"]))):
            sig = S.get_roi_signals(video, P, w)
            assert isinstance(sig, np.ndarray) and sig.dtype == np.float64
            np.testing.assert_allclose(sig, g[f"signals{i}"], rtol=n * 2.0 ** -23, atol=0)
    np.testing.assert_allclose(S.get_roi_signals(g["video"], g["P"]), g["signals0"], rtol=49 * 2.0 ** -23, atol=0)


@pytest.mark.parametrize("window", [(3, 3, 0), (2, 1, 1), (0, 0, 0), (7, 7, 7), (5, 20, 1)])
def test_roi_signals_with_nans_and_positions_outside(ops, window):
    """64 x 48 x 3 with NaN voxels and positions off the volume, rows longer than a frame: K13 and the restatement sum the
    same float32 values in float64, in different orders -- N 2^-53 relative to the sum of magnitudes."""
    rng = np.random.RandomState(3)
    sz, K, T = (64, 48, 3), 40, 6
    video = rng.randn(*sz, T).astype(np.float32)
    video[rng.rand(*sz, T) < 0.02] = np.nan
    video[10:14, 10:14, :, 2] = np.nan
    P = rng.rand(K, 3, T) * (np.array(sz)[None, :, None] + 4) - 2
    P[0, :, 2] = [12.0, 12.0, 1.0]           # window 0: an all-NaN box
    P[1, :, :] = [[63.5], [47.49], [2.5]]    # 64 is outside
    P[2, 1, 3] = np.nan
    P[3, :, :] = [[62.5], [46.5], [1.5]]
    rows = torch.full((T + 1, 64 * 48 * 3 + 40), float("nan"), device="cuda")
    rows[:T, :64 * 48 * 3] = dev(np.moveaxis(video, 3, 0).reshape(T, -1))
    want = TR.roi_signals(video, P, window)
    assert np.isnan(want).any() and np.isfinite(want).sum() > K
    for Pt in (dev(P), dev(P.astype(np.float32))):
        got = ops.roi_signals(rows, sz, Pt, window).cpu().numpy()
        ref = want if Pt.dtype == torch.float64 else TR.roi_signals(video, P.astype(np.float32), window)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12, equal_nan=True)
    with pytest.raises(Exception, match="4096"):
        ops.roi_signals(rows, sz, dev(P), (8, 8, 8))


# ---- K11 ------------------------------------------------------------------------------------------------------------
def fit_case(rng, sz, K, T, order="quadratic"):
    """Tracks made by the inverse of a near-identity warp of ``order``: (beta_true (10,3,T), P (K,3,T), R (K,3))."""
    b = near_identity(rng, sz, T)
    rows = TR.free_rows(sz, order)
    for i in range(10):
        if i not in rows:
            b[i] = TR.IDENTITY[i][:, None]
    b = b.astype(np.float32).astype(np.float64)
    R = rng.rand(K, 3) * (np.array(sz) - 1) * 0.9 + 0.05 * (np.array(sz) - 1)
    P = TR.invert_quadratic_warp(b, R, tol=1e-10)
    assert np.isfinite(P).all()
    return b, P, R


@pytest.mark.parametrize("sz", [(64, 64, 2), (512, 512, 2), (64, 48, 1)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_fit_recovers_the_warp_that_made_the_tracks(ops, sz, dtype):
    """Exact recovery, compared as warps: max |basis(x) (beta_fit - beta_true)| over the eight corners.  beta is stored in
    fp32 and a corner's q is a sum of ten products of size <= S: rounding alone gives about 10 2^-24 S voxel (3e-4 at
    S = 512); ten times that is allowed, for the tracks as made (float64).  Tracks rounded to fp32 are other tracks (2^-24 S
    per coordinate, which the extrapolation to the corners amplifies): there the float64 restatement on the same rounded
    tracks says how far from the generating warp the exact fit is, and the kernel may add the rounding of beta to that."""
    rng = np.random.RandomState(sz[0] + sz[2])
    T, K = 5, 24
    b, P, R = fit_case(rng, sz, K, T)
    beta, ok = ops.fit_quadratic_warp(dev(P, dtype), dev(R), sz)
    assert beta.dtype == torch.float32 and tuple(beta.shape) == (10, 3, T) and ok.dtype == torch.bool and bool(ok.all())
    beta = beta.cpu().numpy().astype(np.float64)
    bound = 10 * (10 * 2.0 ** -24 * max(sz))
    err = max(np.abs(TR.warp(beta[:, :, t], corners(sz)) - TR.warp(b[:, :, t], corners(sz))).max() for t in range(T))
    print(f"{sz} {dtype}: corner error {err:.3e} voxel, bound {bound:.3e}")
    # the restatement on the same (rounded) tracks
    want, wok = TR.fit_quadratic_warp(dev(P, dtype).cpu().numpy(), R, sz)
    assert wok.all()
    werr = max(np.abs(TR.warp(beta[:, :, t], corners(sz)) - TR.warp(want[:, :, t], corners(sz))).max() for t in range(T))
    assert werr < 10 * 2.0 ** -24 * max(sz)
    if dtype == torch.float64:
        assert err < bound
    else:
        own = max(np.abs(TR.warp(want[:, :, t].astype(np.float64), corners(sz)) - TR.warp(b[:, :, t], corners(sz))).max()
                  for t in range(T))
        assert err < own + 10 * 2.0 ** -24 * max(sz)
    if sz[2] == 1:
        ident = np.broadcast_to(TR.IDENTITY[:, :, None], beta.shape)
        np.testing.assert_array_equal(beta[:, 2], ident[:, 2])
        np.testing.assert_array_equal(beta[[3, 6, 8, 9]], ident[[3, 6, 8, 9]])


@pytest.mark.parametrize("sz", [(64, 48, 2), (64, 48, 1)])
@pytest.mark.parametrize("order", ["translation", "affine", "quadratic"])
@pytest.mark.parametrize("ridge", [0.0, 0.3])
def test_fit_orders_ridge_and_untracked_neurons(ops, sz, order, ridge):
    """Noisy tracks with NaNs, every order, with and without ridge: the kernel against the restatement, as warps at the
    corners (both round the same float64 solution to fp32: one fp32 rounding of ten terms of size <= S apart, plus the
    difference of two float64 eliminations of a system with condition ~1e4), rows that are not free at the identity bit for
    bit, ok everywhere."""
    rng = np.random.RandomState(11)
    T, K = 6, 30
    b, P, R = fit_case(rng, sz, K, T, order)
    P += rng.randn(*P.shape) * 0.2 * (np.array(sz) > 1)[None, :, None]
    P = np.where((rng.rand(K, T) < 0.2)[:, None, :], np.nan, P)
    P[5, 1, :] = np.nan                        # one coordinate is enough to drop a neuron from a frame
    beta, ok = ops.fit_quadratic_warp(dev(P), dev(R), sz, order=order, ridge=ridge)
    want, wok = TR.fit_quadratic_warp(P, R, sz, order, ridge)
    assert bool(ok.all()) and wok.all()
    beta = beta.cpu().numpy()
    for t in range(T):
        d = np.abs(TR.warp(beta[:, :, t], corners(sz)) - TR.warp(want[:, :, t], corners(sz))).max()
        assert d < 10 * 2.0 ** -24 * max(sz), (t, d)
    rows = TR.free_rows(sz, order)
    ident = np.broadcast_to(TR.IDENTITY[:, :, None], beta.shape).astype(np.float32)
    if order != "translation":      # translation: rows 1..3 are the identity, row 0 is free
        fixed = [i for i in range(10) if i not in rows]
        np.testing.assert_array_equal(beta[fixed], ident[fixed])
    else:
        np.testing.assert_array_equal(beta[1:], ident[1:])
    if sz[2] == 1:
        np.testing.assert_array_equal(beta[:, 2], ident[:, 2])
        np.testing.assert_array_equal(beta[[3, 6, 8, 9]], ident[[3, 6, 8, 9]])


def test_fit_singular_frames_get_the_identity(ops):
    """ridge = 0: a frame with three collinear points (affine, Z = 1: three free rows), a frame with too few tracked neurons
    and a frame without any get the identity and ok = 0; the other frames are fitted; nothing is NaN.  Too few tracked
    neurons in every frame is refused on the host."""
    sz = (40, 30, 1)
    R = np.array([[5.0, 5.0, 0.0], [10.0, 20.0, 0.0], [30.0, 12.0, 0.0], [20.0, 20.0, 0.0]])
    P = np.repeat(R[:, :, None], 5, 2) + np.array([1.5, -0.5, 0.0])[None, :, None]
    P[:3, :, 1] = [[5.0, 5.0, 0.0], [10.0, 10.0, 0.0], [20.0, 20.0, 0.0]]      # frame 1: three collinear points ...
    P[3, :, 1] = np.nan                                                        # ... and nothing else
    P[2:, :, 2] = np.nan                                                       # frame 2: two points for three rows
    P[:, 0, 3] = np.nan                                                        # frame 3: nobody tracked
    beta, ok = ops.fit_quadratic_warp(dev(P), dev(R), sz, order="affine")
    assert ok.tolist() == [True, False, False, False, True]
    beta = beta.cpu().numpy()
    assert np.isfinite(beta).all()
    ident = TR.IDENTITY.astype(np.float32)
    for t in (1, 2, 3):
        np.testing.assert_array_equal(beta[:, :, t], ident)
    want, wok = TR.fit_quadratic_warp(P, R, sz, "affine")
    assert wok.tolist() == ok.tolist()
    np.testing.assert_allclose(beta, want, rtol=0, atol=1e-5)
    np.testing.assert_allclose(beta[0, :, 0], [-1.5, 0.5, 0.0], atol=1e-5)
    # with a ridge every frame is regular; the empty frame is the identity with ok = 1
    beta, ok = ops.fit_quadratic_warp(dev(P), dev(R), sz, order="affine", ridge=1e-3)
    assert bool(ok.all()) and np.isfinite(beta.cpu().numpy()).all()
    np.testing.assert_array_equal(beta[:, :, 3].cpu().numpy(), ident)
    with pytest.raises(ValueError, match="tracked"):
        ops.fit_quadratic_warp(dev(P[:2]), dev(R[:2]), sz, order="affine")
    with pytest.raises(ValueError, match="order"):
        ops.fit_quadratic_warp(dev(P), dev(R), sz, order="cubic")


# ---- K12 ------------------------------------------------------------------------------------------------------------
def test_inverse_at_the_identity_returns_the_targets_bit_for_bit(ops):
    rng = np.random.RandomState(1)
    R = rng.rand(50, 3) * [511, 511, 1]
    beta = dev(np.repeat(TR.IDENTITY[:, :, None], 7, 2), torch.float32)
    out = ops.invert_quadratic_warp(beta, dev(R))
    assert out.dtype == torch.float64 and tuple(out.shape) == (50, 3, 7)
    np.testing.assert_array_equal(out.cpu().numpy(), np.repeat(R[:, :, None], 7, 2))


@pytest.mark.parametrize("sz", [(64, 48, 4), (512, 512, 2), (64, 48, 1)])
def test_inverse_solves_the_warp_equation(ops, sz):
    """q_t(x*) evaluated in float64 equals the target within 10 tol; the kernel agrees with the restatement; a times subset
    and an explicit start."""
    rng = np.random.RandomState(8)
    T, K, tol = 9, 33, 1e-6
    b = near_identity(rng, sz, T).astype(np.float32)
    R = rng.rand(K, 3) * (np.array(sz) - 1)
    out = ops.invert_quadratic_warp(dev(b), dev(R), tol=tol).cpu().numpy()
    assert np.isfinite(out).all()
    for t in range(T):
        assert np.abs(TR.warp(b[:, :, t], out[:, :, t]) - R).max() < 10 * tol
    np.testing.assert_allclose(out, TR.invert_quadratic_warp(b, R, tol=tol), rtol=0, atol=2 * tol)
    times = [7, 0, 3]
    sub = ops.invert_quadratic_warp(dev(b), dev(R), times=times, tol=tol).cpu().numpy()
    np.testing.assert_array_equal(sub, out[:, :, times])
    start = out[:, :, times] + 0.25 * (np.array(sz) > 1)[None, :, None]
    again = ops.invert_quadratic_warp(dev(b), dev(R.astype(np.float32)), times=torch.tensor(times), start=dev(start), tol=tol)
    np.testing.assert_allclose(again.cpu().numpy(), TR.invert_quadratic_warp(b, R.astype(np.float32).astype(np.float64), times),
                               rtol=0, atol=2 * tol)
    with pytest.raises(ValueError, match="times"):
        ops.invert_quadratic_warp(dev(b), dev(R), times=[T])


def test_inverse_gives_nan_where_the_jacobian_vanishes(ops):
    """Frame 1: q_x does not depend on x (det J = 0 everywhere); frame 2: q_x = x^2 / 64 has no point with q_x = -5 and its
    Jacobian vanishes on x = 0: NaN for those, the call returns, the other frames are solved."""
    b = np.repeat(TR.IDENTITY[:, :, None], 4, 2)
    b[1, 0, 1] = 0.0
    b[1, 0, 2], b[4, 0, 2] = 0.0, 1.0 / 64
    R = np.array([[10.0, 12.0, 1.0], [-5.0, 3.0, 0.0], [0.0, 3.0, 0.0]])
    out = ops.invert_quadratic_warp(dev(b, torch.float32), dev(R)).cpu().numpy()
    np.testing.assert_array_equal(out[:, :, 0], R)
    np.testing.assert_array_equal(out[:, :, 3], R)
    assert np.isnan(out[:, :, 1]).all()
    assert np.isnan(out[1, :, 2]).all() and np.isnan(out[2, :, 2]).all()      # no solution / starts on the singular plane
    np.testing.assert_allclose(out[0, :, 2], [np.sqrt(640.0), 12.0, 1.0], atol=1e-5)


# ---- the public methods ---------------------------------------------------------------------------------------------
def test_round_trip_of_the_model_methods(M):
    """positions(beta_from_positions(P)) equals P within the fit's own residual as the restatement computes it."""
    rng = np.random.RandomState(21)
    sz, K, T = (64, 48, 2), 24, 6
    b, P, R = fit_case(rng, sz, K, T)
    P[:, :2] += rng.randn(K, 2, T) * 0.1                 # tracks no quadratic map reproduces
    fp = M.ExponentialFP(torch.tensor(sz), K, T, positions=torch.from_numpy(R).float())
    before = fp.beta.detach().clone()
    beta, ok = fp.beta_from_positions(P)
    assert bool(ok.all()) and torch.equal(fp.beta.detach(), before)          # no side effect
    with torch.no_grad():
        fp.beta.copy_(beta)
    back = fp.positions()
    assert back.dtype == np.float64 and back.shape == (K, 3, T)
    R32 = R.astype(np.float32).astype(np.float64)
    want_beta, _ = TR.fit_quadratic_warp(P, R32, sz)
    want = TR.invert_quadratic_warp(want_beta, R32)
    resid = np.abs(want - P).max()
    print(f"round trip: residual of the fit {resid:.3f} voxel, kernel vs restatement {np.abs(back - want).max():.3e}")
    assert np.abs(back - want).max() < 1e-3
    assert np.abs(back - P).max() <= resid + 1e-3
    # other points, a times subset
    other = fp.positions(points=R[:3] + 1.0, times=[4, 1])
    np.testing.assert_allclose(other, TR.invert_quadratic_warp(beta.cpu().numpy(), R[:3] + 1.0, times=[4, 1]), rtol=0, atol=1e-5)
    with pytest.raises(ValueError):
        fp.beta_from_positions(P[:5])


def motion_setup(M, cls, rng, sz, K, T, nchan=1):
    pos = rng.rand(K, 3) * (np.array(sz) - 1)
    if nchan == 1:
        dn = cls(torch.tensor(sz), K, T, positions=torch.from_numpy(pos).float())
    else:
        dn = cls(torch.tensor(sz), K, T, torch.rand(nchan, K) + 0.5, positions=torch.from_numpy(pos).float())
    dn.verbose = False
    return dn, pos


@pytest.mark.parametrize("T,bs", [(16, 4), (14, 4)])
def test_update_motion_after_init_motion_starts_from_the_new_beta(M, T, bs):
    """init_motion writes the leaf in place (same tensor object, version counter bumped, grad cleared), leaves frames it
    could not fit where they were, and update_motion then starts from the new beta on the fused and on the step-wise path:
    the two agree under the tolerance of tests/test_gpu_parity.py::test_fused_motion_epoch_equals_stepwise_adam (2e-4 of the
    largest displacement from the start), and both stay near the tracks' beta, far from the identity."""
    torch.manual_seed(3)
    rng = np.random.RandomState(3)
    sz, K = [24, 20, 2], 12
    frames = torch.rand(T, sz[0] * sz[1] * sz[2], device="cuda")
    C0 = torch.rand(K, T)
    res = []
    for fused in (False, True):
        rng = np.random.RandomState(3)
        dn, pos = motion_setup(M, M.DeformableNMF, rng, sz, K, T)
        dn.fused_motion = fused
        dn.C = C0.to("cuda")
        tracks = TR.invert_quadratic_warp(near_identity(rng, sz, T, scale=1.5).astype(np.float32), pos.astype(np.float32))
        tracks[:, :, 5] = np.nan                               # frame 5 cannot be fitted ...
        with torch.no_grad():
            dn.fp.beta[0, :, 5] = 0.125                        # ... and keeps what it had
        leaf, version = dn.fp.beta, dn.fp.beta._version
        opt = torch.optim.Adam([dn.fp.beta], lr=1e-3)
        dn.fp.beta.grad = torch.ones_like(dn.fp.beta)
        ok = dn.init_motion(tracks)
        assert dn.fp.beta is leaf and leaf._version > version and leaf.grad is None and leaf.requires_grad and leaf.is_leaf
        assert ok.tolist() == [t != 5 for t in range(T)]
        start = dn.fp.beta.detach().cpu().numpy().copy()
        want, _ = TR.fit_quadratic_warp(tracks, pos.astype(np.float32), sz)
        keep = [t for t in range(T) if t != 5]
        for t in keep:
            assert np.abs(TR.warp(start[:, :, t], corners(sz)) - TR.warp(want[:, :, t], corners(sz))).max() < 10 * 2.0 ** -24 * 24
        np.testing.assert_array_equal(start[0, :, 5], np.full(3, 0.125, dtype=np.float32))
        assert np.abs(start[0, :, keep] - 0.0).max() > 0.3      # the start is not the identity
        loader = M.ResidentLoader(frames, sz, bs, shuffle=True, generator=torch.Generator().manual_seed(5))
        dn.update_motion(loader, opt, gamma=1, epochs=3)
        assert dn.fp.beta is leaf and float(opt.state[leaf]["step"]) == 3 * ((T + bs - 1) // bs)
        res.append((start, dn.fp.beta.detach().cpu().numpy()))
    (s0, b0), (s1, b1) = res
    np.testing.assert_array_equal(s0, s1)
    disp = np.abs(b0 - s0).max()
    assert 0 < disp < 0.1                                       # 12 Adam steps of 1e-3 from the tracks' beta
    np.testing.assert_allclose(b1 - s1, b0 - s0, rtol=0, atol=2e-4 * disp)


def test_multichannel_model_inherits_both_methods(M):
    rng = np.random.RandomState(13)
    sz, K, T, NC = [24, 20, 2], 12, 6, 3
    torch.manual_seed(13)
    dn, pos = motion_setup(M, M.MultiChannelDNMF, rng, sz, K, T, nchan=NC)
    b = near_identity(rng, sz, T).astype(np.float32)
    tracks = TR.invert_quadratic_warp(b, pos.astype(np.float32))
    chans = dn._channels()
    ok = dn.init_motion(torch.from_numpy(tracks))
    assert bool(ok.all()) and all(f.beta is dn.fp.beta for f, _ in chans)      # the channels share the leaf that was written
    got = dn.positions()
    np.testing.assert_allclose(got, tracks, rtol=0, atol=1e-3)
    frames = torch.rand(T, NC * sz[0] * sz[1] * sz[2], device="cuda")
    before = dn.fp.beta.detach().clone()
    dn.update_motion(M.ResidentLoader(frames, sz, 3), torch.optim.Adam([dn.fp.beta], lr=1e-3), gamma=1, epochs=1)
    moved = (dn.fp.beta.detach() - before).abs().max()
    assert 0 < float(moved) < 5e-3


def median_correlation(C, traces):
    return float(np.median([np.corrcoef(C[k], traces[k])[0, 1] for k in range(C.shape[0])]))


def test_track_start_gives_better_traces_than_the_identity_start(M):
    """End to end on a simulated video with real motion: 48 x 48 x 2, K = 12, T = 12, motion='gp' with sigma = 16 (a standard
    deviation of 4 voxels in x and y), length scale 40, noise at -120 dB, seeds 1 / 2.  The same update_footprints (30
    multiplicative updates of C, no neighbour term) from the identity warp and from init_motion(dataset.positions); the
    median correlation of C with the simulator's traces must be higher from the tracks.

    The reference arithmetic on the CPU (oracle/dnmf_oracle.py: OracleModel.update_footprints, beta from the restatement's
    fit) gives 0.280 from the identity and 0.945 from the tracks on this video (affine tracks: 0.865, translation: 0.737);
    the GPU run has to reproduce the ordering, not the numbers."""
    sz, K, T = [48, 48, 2], 12, 12
    torch.manual_seed(1)
    np.random.seed(1)
    ds = M.SimulatedVideoDataset(K=K, T=T, sz=torch.tensor(sz), shape_std=3, density=.3, bg_snr=-120, traces='exp', motion='gp',
                                 motion_par={"sigma": [16, 16, .01], "ls": [40, 40, 40]})
    corr = {}
    for start in ("identity", "tracks"):
        torch.manual_seed(2)
        dn = M.DeformableNMF(torch.tensor(sz), K, T, positions=ds.positions[:, :, 0].contiguous())
        dn.verbose = False
        if start == "tracks":
            assert bool(dn.init_motion(ds.positions).all())
            # the model now puts every neuron where the simulator did
            assert np.abs(dn.positions() - ds.positions.numpy()).max() < 1.0
        dn.update_footprints(ds.loader(4), 4, sz, gamma_c=0, iter_c=30, return_dense=False)
        corr[start] = median_correlation(dn.C.cpu().numpy(), ds.traces)
    print(f"median correlation of C with the traces: identity start {corr['identity']:.3f}, track start {corr['tracks']:.3f}")
    assert corr["tracks"] > corr["identity"]
