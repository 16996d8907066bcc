"""MultiChannelDNMF learns its footprints: the channel form of K7 (one nearest-point search per lattice point, a gather per
channel), the channel form of the list K5 (colours folded into the trace scalars), spatial_step at K = 200 in both forms,
update_footprints(live_spatial=True) and fit().  The colour axis has no reference semantics: the checks are the
per-channel kernels bit for bit, the update formula in float64, and the single-channel model for one channel of colour 1.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd.Demix import dNMF
    return dNMF


@pytest.fixture(scope="module")
def O():
    from oracle import dnmf_oracle
    return dnmf_oracle


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def near_identity_beta(O, rng, T, sz, scale=1.0):
    """A fit-sized warp per frame: shifts of ~0.6 voxel, linear and quadratic terms of 1e-2 / 1e-4 (pinned z for Z == 1)."""
    beta = O.identity_beta(T) + (rng.randn(10, 3, T) * scale * np.array([0.6, 6e-3, 6e-3, 6e-3, 1e-4, 1e-4, 1e-4, 1e-4, 1e-4, 1e-4])
                                 [:, None, None]).astype(np.float32)
    if sz[2] == 1:
        beta[:, 2] = O.identity_beta(T)[:, 2]
    return beta


# ---- K7 over channels ----------------------------------------------------------------------------------------------
# 30x26x1 and 20x16x2: the rows kernel; 1x24x3: an axis of one voxel, the window kernel (every point then goes on to the
# exhaustive kernel)
@pytest.mark.parametrize("sz", [[30, 26, 1], [20, 16, 2], [1, 24, 3]])
@pytest.mark.parametrize("exhaustive", [False, True])
def test_k7_channels_equal_per_channel_k7(M, O, sz, exhaustive):
    from dnmf_amd import ops
    rng = np.random.RandomState(11)
    T, NC = 7, 3
    P = int(np.prod(sz))
    frames = torch.rand(T + 2, NC * P, device="cuda")           # more rows than frames: rows are picked by frame_ids
    fid = torch.from_numpy(rng.permutation(T + 2)[:T].astype(np.int32)).cuda()
    times = torch.from_numpy(rng.permutation(T).astype(np.int32)).cuda()
    for scale in (1.0, 30.0):                                   # near identity, and strong enough to need boxes / fallbacks
        beta = dev(near_identity_beta(O, rng, T, sz, scale))
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        out = torch.full((T, NC * P + 13), -7.0, device="cuda")  # a row stride larger than NC * P
        ops.image_iwarp(frames, fid, sz, beta, times, out=out, exhaustive=exhaustive, count=cnt, nchan=NC)
        cnt1 = torch.zeros(1, dtype=torch.int64, device="cuda")
        for c in range(NC):
            ref = ops.image_iwarp(frames[:, c * P:(c + 1) * P], fid, sz, beta, times, exhaustive=exhaustive,
                                  count=cnt1 if c == 0 else None)
            assert torch.equal(out[:, c * P:(c + 1) * P], ref), (sz, scale, c)
        assert bool((out[:, NC * P:] == -7.0).all())             # the padding of a row is not written
        assert int(cnt) == int(cnt1), (sz, scale)                # the fallback count is per lattice point
        if exhaustive:
            assert int(cnt) == T * P


def test_k7_channels_without_frame_ids_and_default_output(M, O):
    from dnmf_amd import ops
    rng = np.random.RandomState(12)
    sz, T, NC = [30, 26, 1], 5, 2
    P = int(np.prod(sz))
    frames = torch.rand(T, NC * P, device="cuda")
    beta = dev(near_identity_beta(O, rng, T, sz))
    out = ops.image_iwarp(frames, None, sz, beta, list(range(T)), nchan=NC)
    assert out.shape == (T, NC * P)
    for c in range(NC):
        assert torch.equal(out[:, c * P:(c + 1) * P], ops.image_iwarp(frames[:, c * P:(c + 1) * P].contiguous(), None, sz, beta,
                                                                      list(range(T))))


# ---- K5, list form, over channels ----------------------------------------------------------------------------------
def compact_of_dense(sl, A1, sz):
    """The compact buffer of the list-form K5 built from a dense (P,K) A1: entry (tile q, slot i, lane l, v) at
    tile_off[q] + 256 i + 4 l + v holds A1[x*YZ + u, list[q][i]] for x = 4 qx + l // 16, u = 64 qu + 4 (l % 16) + v, and 0
    outside the volume."""
    X, Y, Z = sz
    YZ = Y * Z
    nt = sl["ntiles"]
    tab = sl["tables"].cpu().numpy()
    tile_n, tile_off, lists = tab[:nt], tab[nt:2 * nt], tab[2 * nt + 2:].reshape(nt, 32)
    nu = (YZ + 63) // 64
    out = np.zeros(sl["total"])
    lane, v = np.arange(64)[:, None], np.arange(4)[None, :]
    for q in range(nt):
        qu, qx = q % nu, q // nu
        x, u = 4 * qx + lane // 16, 64 * qu + 4 * (lane % 16) + v
        inside = (x < X) & (u < YZ)
        p = np.where(inside, x * YZ + u, 0)
        for i in range(tile_n[q]):
            out[tile_off[q] + 256 * i + 4 * lane + v] = np.where(inside, A1[p, lists[q, i]], 0.0)
    return out


@pytest.mark.parametrize("sz,K,T", [([40, 36, 1], 12, 70), ([20, 16, 2], 9, 300), ([33, 30, 1], 7, 5)])
def test_k5_list_channels_against_float64(M, sz, K, T):
    from dnmf_amd import ops
    rng = np.random.RandomState(13)
    NC = 3
    P = int(np.prod(sz))
    dn = M.DeformableNMF(torch.tensor(sz), K, T, positions=torch.from_numpy(rng.rand(K, 3) * np.array(sz)).float())
    sl = ops.spatial_lists_setup(dn.fp.packed_lists(floor=0.0), K, sz)
    assert sl["total"] > 0
    Yr = torch.rand(T + 3, NC * P, device="cuda")
    C = dev(0.2 + rng.rand(K, T + 3))
    colours = dev(0.3 + rng.rand(NC, K))
    fid = torch.from_numpy(rng.permutation(T + 3)[:T].astype(np.int32)).cuda()
    times = torch.from_numpy(rng.permutation(T + 3)[:T].astype(np.int32)).cuda()
    A1c, Cs, _ = ops.spatial_accum_lists_channels(Yr, C, colours, sl, sz, K, frame_ids=fid, times=times)
    Yd = Yr.double()[fid.long()].reshape(T, NC, P)
    Cd = C.double()[:, times.long()]
    A1 = sum(colours[c].double()[None, :] * (Yd[:, c].T @ Cd.T) for c in range(NC)).cpu().numpy()
    np.testing.assert_allclose(A1c.double().cpu().numpy(), compact_of_dense(sl, A1, sz), rtol=3e-5, atol=0)
    np.testing.assert_allclose(Cs.double().cpu().numpy(), (Cd @ Cd.T).cpu().numpy(), rtol=1e-6)
    # one channel of colour 1: the single-channel kernel bit for bit
    Y1 = Yr[:, :P].contiguous()
    a, cs_a, _ = ops.spatial_accum_lists_channels(Y1, C, torch.ones(1, K, device="cuda"), sl, sz, K, frame_ids=fid, times=times)
    b, cs_b, _ = ops.spatial_accum_lists(Y1, C, sl, sz, K, frame_ids=fid, times=times)
    assert torch.equal(a, b) and torch.equal(cs_a, cs_b)


# ---- spatial_step at K = 200 ---------------------------------------------------------------------------------------
def shard_model(M, K=200, T=8, NC=3, seed=21, colours=None):
    """The config-5 shard geometry: 512x512x1, K neurons, 61 x 61 footprint boxes (list form under 'auto')."""
    rng = np.random.RandomState(seed)
    sz = [512, 512, 1]
    pos = torch.from_numpy(rng.rand(K, 3) * np.array([512.0, 512.0, 0.0])).float()
    if colours is None:
        colours = torch.from_numpy(0.3 + rng.rand(NC, K)).float()
    dn = M.MultiChannelDNMF(torch.tensor(sz), K, T, colours, positions=pos)
    dn.verbose = False
    dn.C = dev(0.2 + rng.rand(K, T))
    return dn, sz, pos, rng


def update_formula(dn, A0, frames, D, gamma):
    """A * (sum_c colours_c Y_c^T C^T) / (A ((C C^T) o (colours^T colours)) + gamma D + 1e-32) in float64 on the device."""
    P, K = A0.shape
    NC = dn.colours.shape[0]
    Cd, col = dn.C.double(), dn.colours.double()
    T = frames.shape[0]
    Y = frames.double().reshape(T, NC, P)
    A1 = sum(col[c][None, :] * (Y[:, c].T @ Cd[:, :T].T) for c in range(NC))
    den = A0 @ ((Cd[:, :T] @ Cd[:, :T].T) * (col.T @ col)) + (0.0 if D is None else gamma * D) + 1e-32
    return A0 * A1 / den


@pytest.mark.parametrize("kernel", ["auto", "dense"])
def test_spatial_step_at_k200_against_float64(M, kernel):
    dn, sz, _, rng = shard_model(M)
    dn.spatial_kernel = kernel
    P, K, T = 512 * 512, 200, 8
    frames = torch.rand(T, 3 * P, device="cuda")
    D = rng.rand(*sz, K)
    assert (dn._spatial_lists() is not None) == (kernel == "auto")   # 'auto' takes the list form at this geometry
    A0 = dn.fp.A.reshape(P, K).double().clone()
    got = dn.spatial_step(frames, D=D, gamma=0.2).reshape(P, K).double()
    want = update_formula(dn, A0, frames, dev(D.reshape(P, K), torch.float64), 0.2)
    err = ((got - want).abs() / want.abs().clamp_min(1e-30)).max()
    assert float(err) < 3e-5, float(err)
    assert dn._chan_fp is None and dn._sl is None


def test_spatial_step_one_channel_lists_equals_single_channel_model(M):
    K, T = 200, 8
    a, sz, pos, _ = shard_model(M, colours=torch.ones(1, K))
    b = M.DeformableNMF(torch.tensor(sz), K, T, positions=pos)
    b.C = a.C.clone()
    a.spatial_kernel = b.spatial_kernel = "lists"
    frames = torch.rand(T, 512 * 512, device="cuda")
    ra = a.spatial_step(frames, D=a.D, gamma=0.2)
    rb = b.spatial_step(frames, D=b.D, gamma=0.2)
    assert torch.equal(ra, rb)


def test_config5_shard_spatial_step(M):
    """512x512x1, NC = 3, K = 200, T = 16: the list form is taken, the footprints stay finite and non-negative, and with
    gamma = 0 the registered-frame objective sum_c |Y^c - (colours_c o A) C|^2 does not increase (multiplicative update)."""
    T, NC, K = 16, 3, 200
    dn, sz, _, rng = shard_model(M, T=T, NC=NC)
    P = 512 * 512
    A = dn.fp.A.reshape(P, K).double()
    Ctrue = dev(0.5 + rng.rand(K, T), torch.float64)
    frames = torch.cat([((A * dn.colours[c].double()) @ Ctrue).T for c in range(NC)], 1).float()
    frames += 0.05 * torch.rand_like(frames)

    def objective():
        A2 = dn.fp.A.reshape(P, K).double()
        return sum(float(((frames[:, c * P:(c + 1) * P].double().T - (A2 * dn.colours[c].double()) @ dn.C.double()) ** 2).sum())
                   for c in range(NC))

    assert dn._spatial_lists() is not None
    before = objective()
    dn.spatial_step(frames, gamma=0.0)
    assert dn._spatial_buf.numel() < P * K                    # the compact buffer, not the dense P x K one
    assert bool(torch.isfinite(dn.fp.A).all()) and bool((dn.fp.A >= 0).all())
    after = objective()
    assert after <= before * (1 + 1e-6), (before, after)
    assert after < before


# ---- update_footprints(live_spatial=True) and fit() ----------------------------------------------------------------
def small_models(M, O, NC, kernel, colours=None, seed=3):
    rng = np.random.RandomState(seed)
    sz, K, T = [30, 26, 1], 5, 6
    pos = np.concatenate([4 + rng.rand(K, 2) * np.array([22, 18]), np.zeros((K, 1))], 1).astype(np.float32)
    if colours is None:
        colours = torch.from_numpy(0.3 + rng.rand(NC, K)).float()
    beta = near_identity_beta(O, rng, T, sz)
    C0 = 0.3 + rng.rand(K, T).astype(np.float32)

    def model(cls=M.MultiChannelDNMF):
        dn = cls(torch.tensor(sz), K, T, colours, positions=torch.from_numpy(pos)) if cls is M.MultiChannelDNMF else \
            cls(torch.tensor(sz), K, T, positions=torch.from_numpy(pos))
        dn.verbose = False
        dn.spatial_kernel = kernel
        dn.C = dev(C0)
        with torch.no_grad():
            dn.fp.beta.copy_(dev(beta))
        return dn

    return model, sz, K, T


@pytest.mark.parametrize("kernel", ["auto", "lists"])
def test_live_spatial_update_footprints_equals_the_steps_by_hand(M, O, kernel):
    from dnmf_amd import ops
    NC, bs = 3, 3
    model, sz, K, T = small_models(M, O, NC, kernel)
    P = int(np.prod(sz))
    frames = torch.rand(T, NC * P, device="cuda")
    a, b = model(), model()
    test = M.ResidentLoader(frames, sz, bs)
    out = a.update_footprints(test, bs, sz, gamma_c=0, gamma_a=0.2, iter_c=5, live_spatial=True, iter_a=2)
    assert out == (None, None, None)
    b.update_footprints(test, bs, sz, gamma_c=0, iter_c=5)
    reg = ops.image_iwarp(frames, None, sz, b.fp.beta.detach(), list(range(T)), nchan=NC)
    for _ in range(2):
        b.spatial_step(reg, D=b.D, gamma=0.2)
    assert torch.equal(a.C, b.C) and torch.equal(a.fp.A, b.fp.A)
    assert torch.equal(a._reg_buf, reg)
    assert not torch.equal(a.fp.A, model().fp.A)
    with pytest.raises(NotImplementedError):
        a.update_footprints(test, bs, sz, return_dense=True, live_spatial=True)


@pytest.mark.parametrize("kernel", ["auto", "dense"])
def test_live_spatial_one_channel_equals_single_channel_model(M, O, kernel):
    model, sz, K, T = small_models(M, O, 1, kernel, colours=torch.ones(1, 5))
    P, bs = int(np.prod(sz)), 3
    frames = torch.rand(T, P, device="cuda")
    a, b = model(), model(M.DeformableNMF)
    test = M.ResidentLoader(frames, sz, bs)
    a.update_footprints(test, bs, sz, gamma_c=0, gamma_a=0.2, iter_c=5, live_spatial=True)
    b.update_footprints(test, bs, sz, gamma_c=0, gamma_a=0.2, iter_c=5, return_dense=False, live_spatial=True)
    assert torch.equal(a.C, b.C) and torch.equal(a.fp.A, b.fp.A)


@pytest.mark.parametrize("spatial", [True, False])
def test_fit_equals_explicit_motion_and_footprint_updates(M, O, spatial):
    NC, bs = 3, 2
    model, sz, K, T = small_models(M, O, NC, "auto", seed=7)
    P = int(np.prod(sz))
    frames = torch.rand(T, NC * P, device="cuda")
    a, b = model(), model()

    def loaders():
        return (M.ResidentLoader(frames, sz, bs, shuffle=True, generator=torch.Generator().manual_seed(0)),
                M.ResidentLoader(frames, sz, bs))

    opt_a = torch.optim.Adam([a.fp.beta], lr=1e-3)
    opt_b = torch.optim.Adam([b.fp.beta], lr=1e-3)
    train, test = loaders()
    a.fit(train, test, opt_a, bs, outer=2, gamma=1, epochs=1, gamma_c=0, iter_c=5, spatial=spatial, gamma_a=0.2)
    train, test = loaders()
    for _ in range(2):
        b.update_motion(train, opt_b, gamma=1, epochs=1)
        b.update_footprints(test, bs, sz, gamma_c=0, gamma_a=0.2, iter_c=5, live_spatial=spatial)
    assert torch.equal(a.fp.beta, b.fp.beta) and torch.equal(a.C, b.C) and torch.equal(a.fp.A, b.fp.A)
    assert torch.equal(a.fp.A, model().fp.A) != spatial
