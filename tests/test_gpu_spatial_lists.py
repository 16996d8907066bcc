"""The list form of the footprint update -- K5 ``dnmf_spatial_accum_lists`` and K6 ``dnmf_mu_spatial_lists``
(csrc/spatial_update.hip) behind ``DeformableNMF.spatial_step`` -- against the oracle's float64 ``update_spatial``
(reference Demix/dNMF.py:151-160) and against the dense kernels, where the list form is most likely to go wrong:

  frame splits       the frames cut into ``ns`` splits whose partial sums ``sl_reduce_kernel`` adds: ragged (a run of 64
                     frames and a run of 3 per split, a shorter last split), exactly two runs, one frame short of them
  headline geometry  512x512x1, K = 100, the bench's Gaussian footprints: 8 splits, as ``bench.py --with-spatial`` runs
  K in (128, 256]    one launch for all neurons (the dense K5 goes by column groups of 128)
  tile capacity      exactly SL_MAXL = 32 neurons in a tile; 33 send 'auto' to the dense kernels
  alignment          frames read through a row stride and a base pointer that are not 16-byte multiples: same bits
  deep z             Z > 64: a tile covers part of one y row
  workspace reuse    one model, T = 1000, 70, 1000: the cached workspace changes nothing
  footprint floor    ``ExponentialFP.footprint_floor`` leaves the footprint update alone

Every test first proves that it reaches the path it is named for (the list form is chosen, the split count is the one
named).  Tolerances as in test_gpu_configs.py::test_list_form_of_the_footprint_update: 2e-5 against the oracle, 1e-5
against the dense kernels.  Where footprints reach fp32's subnormal range (the unthresholded Gaussians), the numerator
``A * A1`` of K6 and its result are rounded to multiples of 2^-149 ~ 1.4e-45: the comparisons allow that rounding of the
numerator, divided by the denominator, and of the result, on top of the relative tolerance.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SUBNORMAL = 1.5e-45      # > 2^-149, the spacing of fp32 subnormals


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


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd import _lib
    return _lib.load()


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def compact(O, sz, pos, sigma=1.2, cut=1e-5):
    """Gaussian footprints with the values below ``cut`` set to zero, as the list test of test_gpu_configs.py builds them."""
    A = O.gaussian_footprints(sz, pos, np.full(len(pos), sigma, dtype=np.float32))
    A[A < cut] = 0
    return A


def model(M, sz, K, T, A, C0, kernel, floor=0.0):
    dn = M.DeformableNMF(torch.tensor(sz), K, T)
    dn.verbose = False
    dn.fp.A = dev(A).reshape(*sz, K)
    dn.C = dev(C0)
    dn.spatial_kernel = kernel
    dn.fp.footprint_floor = floor
    return dn


def step(dn, frames, frame_ids=None, times=None, D=None, gamma=None):
    return dn.spatial_step(frames, D=D, gamma=gamma, frame_ids=frame_ids, times=times).cpu().numpy().astype(np.float64)


def oracle(O, A, C0, frames, sz, frame_ids=None, times=None, D=None, gamma=None, xs=None):
    """(update_spatial in float64, its denominator A C C^T + gamma D + 1e-32) on the x rows ``xs`` (None: all): the update is
    voxel-local once C is fixed.  Frame b is row frame_ids[b] (None: b) with trace column times[b] (None: frame_ids[b], else
    b), as spatial_step reads them."""
    X, YZ, K = sz[0], sz[1] * sz[2], A.shape[-1]
    T = len(frame_ids) if frame_ids is not None else (len(times) if times is not None else frames.shape[0])
    rows = torch.arange(T) if frame_ids is None else torch.as_tensor(frame_ids).cpu().long()
    cols = rows if times is None else torch.as_tensor(times).cpu().long()
    xs = list(range(X)) if xs is None else list(xs)
    Y = frames[rows.to(frames.device)].view(T, X, YZ)[:, xs]
    Yi = np.ascontiguousarray(Y.cpu().numpy().astype(np.float64).transpose(1, 2, 0))
    C = np.asarray(C0, dtype=np.float64)[:, cols.numpy()]
    A64 = np.asarray(A, dtype=np.float64).reshape(X, YZ, K)[xs]
    D64 = None if D is None else np.asarray(D, dtype=np.float64).reshape(X, YZ, K)[xs]
    want = O.update_spatial(A64, C, Yi, D=D64, gamma=gamma)
    den = np.einsum("mnk,kp->mnp", A64, C @ C.T) + (0 if D is None else gamma * D64) + 1e-32
    return want, den


def assert_close(got, want, den, rtol, what):
    """|got - want| <= rtol |want| + (one subnormal rounding of the numerator) / den + (one of the result), element by
    element."""
    err = np.abs(got - want)
    bound = rtol * np.abs(want) + SUBNORMAL / den + SUBNORMAL
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(err / bound), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} entries off; worst at {i}: got {got[i]!r}, want "
                             f"{want[i]!r}, bound {bound[i]!r}")


def assert_zeros_kept(got, A, exact=True):
    """A multiplicative update keeps every zero; with ``exact`` (compact footprints, no value near fp32's smallest) also every
    non-zero."""
    A = np.asarray(A).reshape(got.shape)
    assert not got[A == 0].any(), "a zero footprint value became non-zero"
    if exact:
        assert np.array_equal(got != 0, A != 0)


def check_splits(lib, dn, sz, T, ns):
    """The list form is taken and K5 cuts the T frames into ``ns`` splits (1: none, no workspace)."""
    sl = dn._spatial_lists()
    assert sl is not None and sl["total"] > 0
    need = lib.dnmf_spatial_accum_lists_workspace(*sz, sl["total"], T)
    assert need == (ns * sl["total"] * 4 if ns > 1 else 0)
    return sl


def frames_and_traces(rng, P, K, T, spare):
    frames = torch.rand(T + spare, P, device="cuda")
    C0 = (0.2 + rng.rand(K, T)).astype(np.float32)
    return frames, C0


@pytest.mark.parametrize("T,ns", [(1000, 15), (128, 2), (127, 1)])
def test_frame_splits_vs_oracle_and_dense(M, O, lib, T, ns):
    """32x32x2 (8 tiles): T = 1000 makes 15 splits of 67 frames -- a full run of 64 and a run of 3 each, the last split 62
    frames --; 128 exactly two splits of one run; 127 one split.  Frames picked from a larger buffer by a permutation, trace
    columns by another one; with and without D."""
    rng = np.random.RandomState(T)
    sz, K = [32, 32, 2], 9
    P = int(np.prod(sz))
    pos = rng.rand(K, 3) * np.array(sz)
    A = compact(O, sz, pos, sigma=1.5)
    frames, C0 = frames_and_traces(rng, P, K, T, 40)
    frame_ids = torch.randperm(T + 40)[:T].to(torch.int32).cuda()
    times = torch.randperm(T).to(torch.int32)
    assert not torch.equal(times.long(), frame_ids.cpu().long())
    D = rng.rand(*sz, K).astype(np.float32)
    for use_D in (False, True):
        kw = dict(frame_ids=frame_ids, times=times, D=D if use_D else None, gamma=0.3 if use_D else None)
        dl = model(M, sz, K, T, A, C0, "lists")
        check_splits(lib, dl, sz, T, ns)
        got = step(dl, frames, **kw)
        if ns > 1:
            assert dl._ws_k5 is not None and dl._ws_k5.numel() >= ns * (dl._spatial_buf.numel() - K * K)
        dense = step(model(M, sz, K, T, A, C0, "dense"), frames, **kw)
        want, den = oracle(O, A, C0, frames, sz, **kw)
        got = got.reshape(want.shape)
        assert_zeros_kept(got, A)
        assert_close(got, dense.reshape(want.shape), den, 1e-5, f"T={T} D={use_D}: lists vs dense")
        assert_close(got, want, den, 2e-5, f"T={T} D={use_D}: lists vs oracle")


def test_headline_geometry_vs_dense_and_oracle(M, O, lib):
    """512x512x1, K = 100, the footprints DeformableNMF builds (Gaussians exp(-d^2/9), every non-zero fp32 value kept:
    ~1.4 boxes per voxel, the list form chosen by 'auto'), as bench.py --with-spatial runs them; T = 600 gives the bench's
    8 splits (75 frames each).  The whole volume against the dense kernels, a subset of x rows -- tile edges (x = 3 mod 4)
    and the last row included -- against the oracle; without D and with the constructor's D."""
    torch.manual_seed(7)
    rng = np.random.RandomState(7)
    sz, K, T = [512, 512, 1], 100, 600
    P = int(np.prod(sz))
    dn = M.DeformableNMF(torch.tensor(sz), K, T, positions=(1 + torch.rand(K, 3) * torch.tensor(sz)))
    dn.verbose = False
    A = dn.fp.A.cpu().numpy()
    D = dn.D.astype(np.float32)
    frames, C0 = frames_and_traces(rng, P, K, T, 8)
    frame_ids = torch.randperm(T + 8)[:T].to(torch.int32).cuda()
    times = torch.randperm(T).to(torch.int32)
    xs = [0, 1, 3, 4, 127, 128, 130, 131, 255, 256, 383, 387, 508, 510, 511]
    Cu = np.asarray(C0, dtype=np.float64)[:, times.long().numpy()]
    for use_D in (False, True):
        kw = dict(frame_ids=frame_ids, times=times, D=D if use_D else None, gamma=1.0 if use_D else None)
        dl = model(M, sz, K, T, A, C0, "auto")
        check_splits(lib, dl, sz, T, 8)
        got = step(dl, frames, **kw).reshape(P, K)
        dense = step(model(M, sz, K, T, A, C0, "dense"), frames, **kw).reshape(P, K)
        A2 = torch.from_numpy(A.reshape(P, K)).cuda().double()
        den = A2 @ torch.from_numpy(Cu @ Cu.T).cuda()
        if use_D:
            den += 1.0 * torch.from_numpy(D.reshape(P, K)).cuda().double()
        den = (den + 1e-32).cpu().numpy()
        del A2
        assert_zeros_kept(got, A, exact=False)
        assert_close(got, dense, den, 1e-5, f"D={use_D}: lists vs dense")
        want, wden = oracle(O, A, C0, frames, sz, xs=xs, **kw)
        assert_close(got.reshape(sz[0], sz[1] * sz[2], K)[xs], want, wden, 2e-5, f"D={use_D}: lists vs oracle")


@pytest.mark.parametrize("K,T,ns", [(129, 72, 1), (200, 72, 1), (256, 72, 1), (256, 200, 3)])
def test_more_than_128_neurons_vs_oracle_and_dense(M, O, lib, K, T, ns):
    """K in (128, 256]: the list kernels and trace_gram_kernel take all K neurons in one launch, the dense path goes by
    column groups of 128 with the host C C^T.  Compact footprints on 128x128x2 (128 tiles: T = 200 makes 3 splits)."""
    rng = np.random.RandomState(K + T)
    sz = [128, 128, 2]
    P = int(np.prod(sz))
    pos = rng.rand(K, 3) * np.array(sz)
    A = compact(O, sz, pos)
    frames, C0 = frames_and_traces(rng, P, K, T, 5)
    frame_ids = torch.randperm(T + 5)[:T].to(torch.int32).cuda()
    times = torch.randperm(T).to(torch.int32)
    D = rng.rand(*sz, K).astype(np.float32)
    for use_D in (False, True):
        kw = dict(frame_ids=frame_ids, times=times, D=D if use_D else None, gamma=0.3 if use_D else None)
        dl = model(M, sz, K, T, A, C0, "lists")
        check_splits(lib, dl, sz, T, ns)
        got = step(dl, frames, **kw)
        dense = step(model(M, sz, K, T, A, C0, "dense"), frames, **kw)
        want, den = oracle(O, A, C0, frames, sz, **kw)
        got = got.reshape(want.shape)
        assert_zeros_kept(got, A)
        assert_close(got, dense.reshape(want.shape), den, 1e-5, f"K={K} T={T} D={use_D}: lists vs dense")
        assert_close(got, want, den, 2e-5, f"K={K} T={T} D={use_D}: lists vs oracle")


def test_tile_capacity(M, O, lib):
    """A tile listing exactly SL_MAXL = 32 neurons takes the list form and matches the oracle; with 33 the tables report an
    overflow (total = -1), 'auto' falls back to the dense kernels and 'lists' raises."""
    from dnmf_amd import ops
    rng = np.random.RandomState(32)
    sz, T = [32, 32, 2], 70
    P = int(np.prod(sz))
    for K in (32, 33):
        pos = np.array([16.0, 16.0, 1.0]) + rng.uniform(-1, 1, (K, 3)) * np.array([1.0, 1.0, 0.0])
        A = compact(O, sz, pos, sigma=2.0, cut=1e-3)
        frames, C0 = frames_and_traces(rng, P, K, T, 0)
        want, den = oracle(O, A, C0, frames, sz)
        dl = model(M, sz, K, T, A, C0, "auto")
        total = ops.spatial_lists_setup(dl.fp.packed_lists(), K, sz)["total"]
        if K == 32:
            assert total > 0 and dl._spatial_lists() is not None
            tables = dl._spatial_lists()["tables"].cpu()
            assert int(tables[:ops.spatial_lists_setup(dl.fp.packed_lists(), K, sz)["ntiles"]].max()) == 32
        else:
            assert total == -1 and dl._spatial_lists() is None
        got = step(dl, frames).reshape(want.shape)
        assert_zeros_kept(got, A)
        assert_close(got, want, den, 2e-5, f"K={K}")
        if K == 33:
            dl = model(M, sz, K, T, A, C0, "lists")
            with pytest.raises(ValueError):
                dl.spatial_step(frames)


def test_unaligned_frame_rows_give_the_same_bits(M, O, lib):
    """The same frames as a contiguous tensor (16-byte loads) and as the column slice buf[:, 1:P+1] of a (T, P+3) buffer: row
    stride P+3 and a base pointer 4 bytes past a 16-byte boundary take the element loads.  Y*Z = 48 is a multiple of 4, so
    only the pointer and the stride decide.  Both sum the same values in the same order: the footprints are bit-identical."""
    rng = np.random.RandomState(11)
    sz, K, T = [40, 24, 2], 7, 200
    P = int(np.prod(sz))
    assert (sz[1] * sz[2]) % 4 == 0
    pos = rng.rand(K, 3) * np.array(sz)
    A = compact(O, sz, pos, sigma=1.5)
    C0 = (0.2 + rng.rand(K, T)).astype(np.float32)
    buf = torch.rand(T, P + 3, device="cuda")
    sliced = buf[:, 1:P + 1]
    flat = sliced.contiguous()
    assert flat.data_ptr() % 16 == 0 and flat.stride(0) % 4 == 0
    assert sliced.data_ptr() % 16 != 0 and sliced.stride(0) % 4 != 0 and sliced.stride(1) == 1
    res = []
    for frames in (flat, sliced):
        dl = model(M, sz, K, T, A, C0, "lists")
        check_splits(lib, dl, sz, T, 3)
        res.append(step(dl, frames))
    assert np.array_equal(res[0], res[1])
    want, den = oracle(O, A, C0, flat, sz)
    got = res[1].reshape(want.shape)
    assert_zeros_kept(got, A)
    assert_close(got, want, den, 2e-5, "unaligned vs oracle")


def test_deep_volume_vs_oracle(M, O, lib):
    """Z = 80 > 64: a 64-position tile of the (y,z) plane covers part of one y row (the tile lists select on x and y only).
    Footprints confined to a few z slices; the zero pattern kept, the oracle matched, the dense kernels too."""
    rng = np.random.RandomState(80)
    sz, K, T = [12, 3, 80], 6, 300
    P = int(np.prod(sz))
    pos = np.stack([rng.rand(K) * 12, rng.rand(K) * 3, 10 + rng.rand(K) * 50], 1)
    A = compact(O, sz, pos, sigma=1.0, cut=1e-4)
    assert (A.reshape(-1, K) != 0).any(0).all() and (A.sum((0, 1, 3)) == 0).sum() > 20
    frames, C0 = frames_and_traces(rng, P, K, T, 3)
    kw = dict(frame_ids=torch.randperm(T + 3)[:T].to(torch.int32).cuda(), times=torch.randperm(T).to(torch.int32))
    dl = model(M, sz, K, T, A, C0, "lists")
    check_splits(lib, dl, sz, T, 4)
    got = step(dl, frames, **kw)
    dense = step(model(M, sz, K, T, A, C0, "dense"), frames, **kw)
    want, den = oracle(O, A, C0, frames, sz, **kw)
    got = got.reshape(want.shape)
    assert_zeros_kept(got, A)
    assert_close(got, dense.reshape(want.shape), den, 1e-5, "deep z: lists vs dense")
    assert_close(got, want, den, 2e-5, "deep z: lists vs oracle")


def test_workspace_reuse_across_frame_counts(M, O, lib):
    """One model steps at T = 1000 (15 splits, workspace made), 70 (one split, no workspace needed) and 1000 again (the
    cached workspace reused): every result equals a fresh model's on the same footprints and frames, bit for bit."""
    rng = np.random.RandomState(5)
    sz, K, T = [32, 32, 2], 8, 1000
    P = int(np.prod(sz))
    pos = rng.rand(K, 3) * np.array(sz)
    A = compact(O, sz, pos, sigma=1.5)
    frames, C0 = frames_and_traces(rng, P, K, T, 0)
    dn = model(M, sz, K, T, A, C0, "lists")
    ws = None
    for n, Tc in enumerate((1000, 70, 1000)):
        ids = torch.randperm(T)[:Tc].to(torch.int32).cuda()
        A_before = dn.fp.A.cpu().numpy()
        check_splits(lib, dn, sz, Tc, 15 if Tc == 1000 else 1)
        got = step(dn, frames, frame_ids=ids)
        if n == 0:
            ws = dn._ws_k5
            assert ws is not None
        else:
            assert dn._ws_k5 is ws
        fresh = step(model(M, sz, K, T, A_before, C0, "lists"), frames, frame_ids=ids)
        assert np.array_equal(got, fresh), f"call {n} (T={Tc})"


@pytest.mark.parametrize("floor", [1e-20, 1e-10])
def test_footprint_floor_leaves_the_footprint_update_alone(M, O, lib, floor):
    """``footprint_floor`` takes values out of the neuron lists of the Gram data and the reconstruction only: spatial_step
    on the constructor's Gaussians (every non-zero fp32 value, out to 1e-45) equals the same step with no floor bit for
    bit, the sub-floor values are updated (none zeroed, none left stale) as the oracle says.  Then the floor flips between
    steps of one model, after its tile lists were built: each step still equals the floor-0 model's."""
    torch.manual_seed(3)
    rng = np.random.RandomState(3)
    sz, K, T = [128, 128, 1], 8, 130
    P = int(np.prod(sz))
    ref = M.DeformableNMF(torch.tensor(sz), K, T, positions=1 + torch.rand(K, 3) * torch.tensor(sz))
    A = ref.fp.A.cpu().numpy()
    sub = (A > 0) & (A < floor)
    assert sub.sum() > 1000
    frames, C0 = frames_and_traces(rng, P, K, T, 0)
    want, den = oracle(O, A, C0, frames, sz)
    res = {}
    for f in (0.0, floor):
        dl = model(M, sz, K, T, A, C0, "auto", floor=f)
        check_splits(lib, dl, sz, T, 2)
        res[f] = step(dl, frames)
    assert np.array_equal(res[floor], res[0.0]), \
        f"{int((res[floor] != res[0.0]).sum())} values differ, {int((res[floor][sub.reshape(res[floor].shape)] == 0).sum())} " \
        "sub-floor values zeroed"
    got = res[floor].reshape(want.shape)
    assert_zeros_kept(got, A, exact=False)
    assert_close(got, want, den, 2e-5, f"floor {floor:g} vs oracle")
    assert np.all(got.reshape(A.shape)[sub & (want.reshape(A.shape) > 1e-30)] != 0)
    # the floor changes between steps of one model; the tile lists of the first floor were built before the change
    a, b = model(M, sz, K, T, A, C0, "auto"), model(M, sz, K, T, A, C0, "auto")
    a._spatial_lists()
    for n, f in enumerate((floor, 0.0, floor)):
        a.fp.footprint_floor = f
        a.fp.packed_lists()          # the Gram's layout of the new floor, as the fit builds it before the update
        ids = torch.randperm(T)[:T - 5 * n].to(torch.int32).cuda()
        ga, gb = step(a, frames, frame_ids=ids), step(b, frames, frame_ids=ids)
        assert np.array_equal(ga, gb), f"step {n} with floor {f:g}"
