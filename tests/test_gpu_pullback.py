"""K17 on the GPU: ops.warp_pullback (the trilinear registered movie under the quadratic warp) against its float64 restatement
(tests/pullback_restatement.py), its exact cases bit for bit, the channel and stride forms, and the public surface:
registered_video and update_footprints / fit (registered='linear')."""
import functools

import numpy as np
import pytest
import torch

import pullback_restatement as PB
from tracks_restatement import IDENTITY, warp

pytestmark = pytest.mark.gpu

SHAPES = [(12, 10, 1), (12, 10, 2), (9, 7, 3), (40, 130, 2), (70, 300, 1)]
# seeds for which min |det J| >= 0.5 over the lattice of every frame and the points within 2e-3 of a border plane stay under
# 1 % (both asserted below, on the CPU, from the restatement alone)
SEEDS = {(12, 10, 1): 0, (12, 10, 2): 0, (9, 7, 3): 0, (40, 130, 2): 0, (70, 300, 1): 0}
EXPO = {4: (2, 0, 0), 5: (0, 2, 0), 6: (0, 0, 2), 7: (1, 1, 0), 8: (1, 0, 1), 9: (0, 1, 1)}
TIMES = [4, 1, 5, 2]      # a permuted subset of the T = 6 columns of beta


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd.Demix import dNMF
    return dNMF


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def identity_beta(T):
    return np.repeat(IDENTITY[:, :, None], T, 2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pb_case(sz, seed=None):
    """T = 6 frames under warps built like test_gpu_gn.k16_case: shifts of a few voxels sized per axis (a thin axis is left by
    some samples and not by all), affine terms of +-0.15, small quadratic terms, frame 4 shifted so far that the first rows
    sample wholly outside; frames stored in shuffled rows of a wider buffer.  The float64 restatement of the frames TIMES is
    computed once, for both fill modes, and shared."""
    rng = np.random.default_rng(SEEDS[sz] if seed is None else seed)
    T, P = 6, int(np.prod(sz))
    ext = np.array([max(s - 1, 1) for s in sz], dtype=np.float64)
    amp = np.minimum(1.0, ext / 8.0)
    beta = identity_beta(T).astype(np.float64)
    beta[0] += rng.uniform(-3, 3, (3, T)) * amp[:, None]
    beta[0, 0, 4] += 5.0
    beta[1:4] += rng.uniform(-0.15, 0.15, (3, 3, T)) * np.minimum(1.0, ext[None, :] / ext[:, None])[:, :, None]
    for a in range(4, 10):
        beta[a] += rng.uniform(-1, 1, (3, T)) * amp[:, None] / np.prod(ext ** np.array(EXPO[a]))
    beta = beta.astype(np.float32)
    frames = rng.uniform(0, 1, (T, *sz)).astype(np.float32)
    rows = rng.permutation(T + 2)[:T]
    buf = np.full((T + 2, P + 5), -3.0, np.float32)          # ld > P; what lies between the rows is never read
    buf[rows, :P] = frames.reshape(T, -1)
    want = {fill: PB.pullback(frames[TIMES], beta, TIMES, fill=fill) for fill in (None, np.nan)}
    return {"sz": list(sz), "P": P, "beta": beta, "frames": frames, "rows": rows, "buf": buf, "want": want}


def run(c, fill=None, coords=False, count=False, **kw):
    from dnmf_amd import ops
    B = len(TIMES)
    xs = torch.full((B, c["P"], 3), 7.0, device="cuda") if coords else None
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda") if count else None
    out = ops.warp_pullback(dev(c["buf"]), dev(c["rows"][TIMES], torch.int32), c["sz"], dev(c["beta"]), dev(np.array(TIMES), torch.int32),
                            fill=fill, coords=xs, count=cnt, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if xs is None else xs.cpu().numpy().astype(np.float64), None if cnt is None else int(cnt)


def slope(frame, sz):
    """The largest absolute difference between voxels adjacent along an (active) axis, the zero border included."""
    act = PB.active_axes(sz)
    f = np.pad(frame.astype(np.float64), [(1, 1) if d in act else (0, 0) for d in range(3)])
    return max(np.abs(np.diff(f, axis=d)).max() for d in act)


@pytest.mark.parametrize("sz", SHAPES)
def test_inputs_meet_the_contract(sz):
    """A condition on the inputs, from the restatement alone: the accuracy contract holds where |det J| >= 0.5."""
    c = pb_case(sz)
    for t in TIMES:
        assert PB.lattice_abs_det(c["beta"][:, :, t], sz).min() >= 0.5, (sz, t)
    _, x, nbad = c["want"][None]
    assert nbad == 0 and np.isfinite(x).all()


@pytest.mark.parametrize("sz", SHAPES)
def test_coords_and_values_against_the_restatement(M, sz):
    c = pb_case(sz)
    want, xw, _ = c["want"][None]
    got, xg, nbad = run(c, coords=True, count=True)
    assert nbad == 0
    dx = np.abs(xg - xw).max()
    m = [slope(c["frames"][t], sz) for t in TIMES]
    dv = [np.abs(got[j].reshape(sz) - want[j]).max() for j in range(len(TIMES))]
    print(f"{sz}: max |coords - float64| = {dx:.3e} voxel; max |value - float64| per frame = {dv}, slopes {m}")
    assert dx <= 1e-3
    for j in range(len(TIMES)):
        assert dv[j] <= 3e-3 * m[j] + 1e-6, (sz, j)          # no voxel excluded: zero padding is continuous


@pytest.mark.parametrize("sz", SHAPES)
def test_fill_nan_against_the_restatement(M, sz):
    c = pb_case(sz)
    want, xw, _ = c["want"][np.nan]
    got, _, _ = run(c, fill=float("nan"))
    act = PB.active_axes(sz)
    hi = np.array(sz, dtype=np.float64) - 1
    near = ((np.abs(xw) <= 2e-3) | (np.abs(xw - hi) <= 2e-3))[:, :, act].any(2)       # (B, P)
    share = near.mean()
    print(f"{sz}: {share:.4%} of the points lie within 2e-3 of a border plane")
    assert share <= 0.01
    for j, t in enumerate(TIMES):
        g, w = got[j].reshape(-1)[~near[j]], want[j].reshape(-1)[~near[j]]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (sz, j)
        ok = ~np.isnan(w)
        assert np.abs(g[ok] - w[ok]).max(initial=0.0) <= 3e-3 * slope(c["frames"][t], sz) + 1e-6, (sz, j)
    assert np.isnan(want).any() and not np.isnan(want).all()


def shifted(frame, k, fill=0.0):
    out = np.full(frame.shape, fill, dtype=frame.dtype)
    src = tuple(slice(max(-k[d], 0), frame.shape[d] - max(k[d], 0)) for d in range(3))
    dst = tuple(slice(max(k[d], 0), frame.shape[d] - max(-k[d], 0)) for d in range(3))
    out[dst] = frame[src]
    return out


@pytest.mark.parametrize("sz", SHAPES)
def test_identity_and_integer_translation_are_bit_exact(M, sz):
    from dnmf_amd import ops
    c = pb_case(sz)
    T = 6
    beta = identity_beta(T)
    shifts = {1: (2, -3, 1 if sz[2] > 1 else 0), 2: (-1, 4, 0), 3: (0, 0, -1 if sz[2] > 1 else 0)}
    for t, k in shifts.items():
        beta[0, :, t] = k                                    # q(x) = x + k: out(u) = frame(u - k)
    frames = dev(c["frames"].reshape(T, -1))
    for fill in (None, float("nan")):
        xs = torch.empty((T, c["P"], 3), device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        got = ops.warp_pullback(frames, None, sz, dev(beta), None, fill=fill, coords=xs, count=cnt).cpu().numpy()
        assert int(cnt) == 0
        for t in range(T):
            k = shifts.get(t, (0, 0, 0))
            want = shifted(c["frames"][t], k, np.float32(0.0 if fill is None else fill))
            assert np.array_equal(got[t].reshape(sz), want, equal_nan=True), (sz, t, fill)
            assert np.array_equal(xs[t].cpu().numpy().astype(np.float64), PB.lattice(sz) - np.array(k, dtype=np.float64))


@pytest.mark.parametrize("sz", [(12, 10, 1), (9, 7, 3), (40, 130, 2)])
def test_channels_and_strided_output(M, sz):
    from dnmf_amd import ops
    c = pb_case(sz)
    P, NC, B = c["P"], 3, len(TIMES)
    rng = np.random.default_rng(5)
    frames = torch.rand(8, NC * P + 3, device="cuda")
    fid = dev(rng.permutation(8)[:B], torch.int32)
    beta, tt = dev(c["beta"]), dev(np.array(TIMES), torch.int32)
    for fill in (None, float("nan")):
        cnt, cnt1 = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
        fresh = ops.warp_pullback(frames, fid, sz, beta, tt, nchan=NC, fill=fill, count=cnt)
        assert fresh.shape == (B, NC * P)
        for ch in range(NC):
            one = ops.warp_pullback(frames[:, ch * P:(ch + 1) * P], fid, sz, beta, tt, fill=fill, count=cnt1 if ch == 0 else None)
            assert torch.equal(fresh[:, ch * P:(ch + 1) * P].view(torch.int32), one.view(torch.int32)), (sz, ch)   # bits: NaN too
        assert int(cnt) == int(cnt1)                         # per lattice point, not per channel
        out = torch.full((B + 1, NC * P + 13), -7.0, device="cuda")
        ret = ops.warp_pullback(frames, fid, sz, beta, tt, out=out, nchan=NC, fill=fill)
        assert ret is out and torch.equal(out[:B, :NC * P].view(torch.int32), fresh.view(torch.int32))
        assert bool((out[:, NC * P:] == -7.0).all()) and bool((out[B] == -7.0).all())     # nothing else is written


def test_affine_warp_of_linear_data(M):
    """Trilinear interpolation is exact on linear data: only the position error is left."""
    from dnmf_amd import ops
    sz = (40, 130, 2)
    rng = np.random.default_rng(6)
    b = IDENTITY.copy()
    b[0] = (1.3, -2.6, 0.2)
    b[1:4] += rng.uniform(-0.1, 0.1, (3, 3)) * np.array([[1, 1, 0.02], [1, 1, 0.005], [1, 1, 1]])
    b = b.astype(np.float32)
    s, c0 = np.array([0.7, -0.4, 0.3]), 5.0
    lat = PB.lattice(sz)
    frame = (warp(b, lat) @ s + c0).astype(np.float32)      # Y(x) = L(q(x)): registered, it is L(u)
    x, bad = PB.invert(b, sz)
    inside = (~bad) & ((x >= 0) & (x <= np.array(sz) - 1.0)).all(1)
    assert 0.25 < inside.mean() < 1.0                      # the z shift takes about half of the slab's points outside
    got = ops.warp_pullback(dev(frame[None]), None, sz, dev(b[:, :, None]), None).cpu().numpy()[0].astype(np.float64)
    err = np.abs(got - (lat @ s + c0))[inside].max()
    print(f"affine warp of linear data: max error {err:.3e}, bound {1e-3 * np.abs(s).sum():.3e}")
    assert err <= 1e-3 * np.abs(s).sum()


def test_linear_beats_nearest_on_smooth_frames(M):
    """Frames V(q_t(x)) of an analytic sum of Gaussians V under sub-voxel shifts: registered, they are V."""
    from dnmf_amd import ops
    sz, T = (40, 36, 1), 4
    rng = np.random.default_rng(7)
    centres = np.stack([rng.uniform(6, 34, 6), rng.uniform(6, 30, 6), np.zeros(6)], 1)

    def V(p):
        return sum(np.exp(-((p - c) ** 2).sum(-1) / 9.0) for c in centres)

    beta = identity_beta(T)
    beta[0, :2] = rng.uniform(0.2, 0.45, (2, T)) * rng.choice([-1.0, 1.0], (2, T))
    lat = PB.lattice(sz)
    frames = np.stack([V(warp(beta[:, :, t], lat)) for t in range(T)]).astype(np.float32)
    lin = ops.warp_pullback(dev(frames), None, sz, dev(beta), None).cpu().numpy().reshape(T, *sz)
    nst = ops.image_iwarp(dev(frames), None, sz, dev(beta), list(range(T))).cpu().numpy().reshape(T, *sz)
    inner = (slice(None), slice(3, -3), slice(3, -3))
    truth = V(lat).reshape(sz)[None]
    rms = [float(np.sqrt(((r - truth)[inner] ** 2).mean())) for r in (lin, nst)]
    print(f"RMS error against V on the interior: linear {rms[0]:.3e}, nearest (K7) {rms[1]:.3e}")
    assert rms[0] < rms[1]


# ---- the public surface -----------------------------------------------------------------------------------------------------
def small_model(M, NC=None, seed=3):
    rng = np.random.RandomState(seed)
    sz, K, T = [20, 16, 2], 4, 8
    pos = (np.array([3, 3, 0]) + rng.rand(K, 3) * np.array([14, 10, 1])).astype(np.float32)
    beta = identity_beta(T) + (rng.randn(10, 3, T) * np.array([0.6, 6e-3, 6e-3, 6e-3, 1e-4, 1e-4, 1e-4, 1e-4, 1e-4, 1e-4])[:, None, None]
                               ).astype(np.float32)
    C0 = 0.3 + rng.rand(K, T).astype(np.float32)
    colours = None if NC is None else torch.from_numpy(0.3 + rng.rand(NC, K)).float()

    def model():
        dn = M.DeformableNMF(torch.tensor(sz), K, T, positions=torch.from_numpy(pos)) if NC is None else \
            M.MultiChannelDNMF(torch.tensor(sz), K, T, colours, positions=torch.from_numpy(pos))
        dn.verbose = False
        dn.C = dev(C0)
        with torch.no_grad():
            dn.fp.beta.copy_(dev(beta))
        return dn

    return model, sz, K, T


def test_registered_video_numpy_and_cuda(M):
    from dnmf_amd import ops
    model, sz, K, T = small_model(M)
    dn = model()
    P = int(np.prod(sz))
    rows = torch.rand(T, P, device="cuda")
    times = [5, 2, 7]
    for fill in (None, float("nan")):
        got = dn.fp.registered_video(rows[:3], times=times, fill=fill)
        assert got.is_cuda and got.shape == (3, P)
        assert torch.equal(got.view(torch.int32), ops.warp_pullback(rows[:3], None, sz, dn.fp.beta.detach(), times, fill=fill).view(torch.int32))
        vid = rows[:3].view(3, *sz).permute(1, 2, 3, 0).cpu().numpy()          # (X, Y, Z, B), the layout of Y_i
        host = dn.fp.registered_video(vid, times=times, fill=fill)
        assert isinstance(host, np.ndarray) and host.dtype == np.float64 and host.shape == (*sz, 3)
        assert np.array_equal(host, got.view(3, *sz).permute(1, 2, 3, 0).double().cpu().numpy(), equal_nan=True)
    assert torch.equal(dn.fp.registered_video(rows), ops.warp_pullback(rows, None, sz, dn.fp.beta.detach(), None))
    nearest = dn.fp.registered_video(rows, interpolation='nearest')
    assert torch.equal(nearest, ops.image_iwarp(rows, None, sz, dn.fp.beta.detach(), list(range(T))))
    with pytest.raises(ValueError):
        dn.fp.registered_video(rows, interpolation='cubic')
    loader = M.ResidentLoader(rows, sz, 4)
    assert torch.equal(dn.registered_video(loader), dn.fp.registered_video(rows)) and dn.last_registered_bad == 0


@pytest.mark.parametrize("NC", [None, 3])
def test_update_footprints_registered_linear(M, NC):
    from dnmf_amd import ops
    model, sz, K, T = small_model(M, NC)
    P, bs, nch = int(np.prod(sz)), 4, NC or 1
    frames = torch.rand(T, nch * P, device="cuda")
    test = M.ResidentLoader(frames, sz, bs)
    kw = dict(gamma_c=0, gamma_a=0.2, iter_c=5)
    dense = {} if NC else {"return_dense": True}
    a, b = model(), model()
    out = a.update_footprints(test, bs, sz, live_spatial=True, registered='linear', **kw, **dense)
    b.update_footprints(test, bs, sz, return_dense=False, **kw)
    reg = ops.warp_pullback(frames, None, sz, b.fp.beta.detach(), list(range(T)), nchan=nch)
    b.spatial_step(reg, D=b.D, gamma=0.2)
    assert torch.equal(a.C, b.C) and torch.equal(a.fp.A, b.fp.A)
    assert not torch.equal(a.fp.A, model().fp.A)
    video = a.registered_video(test)
    assert torch.equal(video, reg) and torch.equal(a._reg_buf, reg) and a.last_registered_bad == 0
    if NC is None:
        assert np.array_equal(out[1], video.view(T, *sz).permute(1, 2, 3, 0).double().cpu().numpy())
    else:
        assert out == (None, None, None)
    # the default is what it was: 'nearest' equals the call without the keyword, bit for bit
    c, d = model(), model()
    oc = c.update_footprints(test, bs, sz, live_spatial=True, registered='nearest', **kw, **dense)
    od = d.update_footprints(test, bs, sz, live_spatial=True, **kw, **dense)
    assert torch.equal(c.C, d.C) and torch.equal(c.fp.A, d.fp.A) and torch.equal(c._reg_buf, d._reg_buf)
    if NC is None:
        assert all(np.array_equal(x, y) for x, y in zip(oc, od))
    assert not torch.equal(c.fp.A, a.fp.A)
    with pytest.raises(ValueError):
        c.update_footprints(test, bs, sz, registered='cubic', **kw)


def test_a_folded_frame_is_counted_and_stays_finite(M):
    """A warp that folds inside the volume, as data only: the points nothing maps to are counted and get 0."""
    model, sz, K, T = small_model(M)
    dn = model()
    with torch.no_grad():
        dn.fp.beta[4, 0, 3] = -0.08                          # q_x = x - 0.08 x^2 in frame 3: nothing maps above x = 3.1
    rows = torch.rand(T, int(np.prod(sz)), device="cuda")
    video = dn.registered_video(M.ResidentLoader(rows, sz, 4))
    assert dn.last_registered_bad > 0 and bool(torch.isfinite(video).all())
    _, _, want = PB.pullback(rows[3:4].view(1, *sz).cpu().numpy(), dn.fp.beta.detach().cpu().numpy(), [3])
    print(f"bad points: kernel {dn.last_registered_bad}, restatement (frame 3 alone) {want}")
    assert want > 0
