"""K10 (dnmf_nearest_points, ops.nearest_points, ExponentialFP.image_iwarp) on the GPU.

The contract: per frame and query the point of the smallest float64 (d2, index), d2 = ((qx - px)^2 + (qy - py)^2) +
(qz - pz)^2 on the coordinates as stored.  A brute-force numpy search with the same arithmetic is therefore matched exactly,
everywhere.  scipy (cKDTree, the reference's NearestNDInterpolator) and K7 may pick another of (nearly) equidistant points:
those mismatches are proved to be ties (the two best float64 distances differ by < 1e-6), as test_G6_pushforward_surface
does.
"""
import numpy as np
import pytest
import torch

from conftest import golden

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


def brute(pts, qs):
    """Index of the smallest (d2, index) per query, float64 numpy: (N,3), (Q,3) -> (Q,) int64, and the sorted two best d2."""
    p = np.asarray(pts, dtype=np.float64)
    out, two = np.empty(len(qs), np.int64), np.empty((len(qs), 2))
    for s in range(0, len(qs), 256):
        q = np.asarray(qs[s:s + 256], dtype=np.float64)
        d = (q[:, None, 0] - p[None, :, 0]) ** 2 + (q[:, None, 1] - p[None, :, 1]) ** 2
        d = d + (q[:, None, 2] - p[None, :, 2]) ** 2
        out[s:s + 256] = d.argmin(1)          # first of the minima = lowest index
        two[s:s + 256] = np.sort(d, 1)[:, :2] if p.shape[0] > 1 else np.concatenate([d, d + 1], 1)
    return out, two


def check_cloud(pts, qs, got):
    """got (Q,) from the kernel: equal to brute force everywhere, to cKDTree where the nearest point is unique."""
    from scipy.spatial import cKDTree
    want, two = brute(pts, qs)
    np.testing.assert_array_equal(got, want)
    kd = cKDTree(np.asarray(pts, dtype=np.float64)).query(np.asarray(qs, dtype=np.float64))[1]
    diff = kd != got
    assert (two[diff, 1] - two[diff, 0] < 1e-6).all(), two[diff][:5]


def cuda(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


# ---- 1. G6: the reference's registered video ---------------------------------------------------------------------------

def test_G6_pin(M, O):
    from dnmf_amd import ops
    g = golden("G6_pushforward")
    sz = g["sz"]
    lattice = O.voxel_lattice(sz)
    lat = lattice.reshape(-1, 3).astype(np.float64)
    basis = O.quadratic_basis(lattice)
    exact_ties = 0
    for t in range(g["beta"].shape[2]):
        _, n = O.poly_grid(basis, g["beta"][:, :, [t]], sz)
        flow = O.pushforward_flow(n, sz)[..., 0]                       # (X,Y,Z,3) fp32, the reference's flow_
        got = M.ExponentialFP.image_iwarp(g["video"][..., t], flow, lattice)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == tuple(sz)
        pts = flow.reshape(-1, 3)
        idx = ops.nearest_points(cuda(pts)[None], cuda(lat)).cpu().numpy()[0]
        want, two = brute(pts, lat)
        np.testing.assert_array_equal(idx, want)                       # lowest index among exact ties, exact elsewhere
        mism = (got != g["Y_i"][..., t]).reshape(-1)
        assert (two[mism, 1] - two[mism, 0] < 1e-6).all(), (t, two[mism][:3])
        exact_ties += int((two[:, 1] == two[:, 0]).sum())
    # the identity frames put the odd z slice midway between warped slices: the tie rule is exercised
    assert exact_ties > 0


# ---- 2. random clouds against scipy --------------------------------------------------------------------------------------

def clouds(kind, rng):
    """(points (B,N,3), queries (Q,3) or (B,Q,3), B)"""
    if kind == "uniform":
        return (rng.rand(3, 1000, 3) * [50, 40, 6]).astype(np.float32), rng.rand(3, 777, 3) * [52, 42, 7] - 1, 3
    if kind == "clusters":
        c = rng.rand(2, 8, 3) * 100
        p = c[:, rng.randint(0, 8, 2000)] + rng.randn(2, 2000, 3) * 1.5
        return p.astype(np.float32), rng.rand(1501, 3) * 100, 2
    if kind == "plane":
        p = rng.rand(2, 1500, 3).astype(np.float32) * 30
        p[..., 2] = 4.0
        return p, rng.rand(2, 999, 3) * 30, 2
    if kind == "far_queries":
        p = rng.rand(1, 500, 3).astype(np.float32) * 10
        return p, (rng.rand(400, 3) - 0.5) * 1e5, 1
    if kind == "outlier":
        p = rng.rand(2, 3000, 3).astype(np.float32) * 10
        p[0, 1234] = [1e6, -3e5, 2e5]
        p[1, 0] = [-1e7, 0, 0]
        return p, rng.rand(2, 1000, 3) * 12 - 1, 2
    if kind == "one_point":
        return rng.rand(4, 1, 3).astype(np.float32), rng.rand(100, 3) * 5, 4
    if kind == "line":
        t = rng.rand(1, 4096, 1)
        return (t * [[[30, 20, 10]]] + 2).astype(np.float32), rng.rand(1, 1000, 3) * 35, 1
    if kind == "f64":
        # coordinates an fp32 copy cannot hold: neighbours 1e-9 apart
        base = rng.rand(1, 1500, 3) * 100
        p = np.concatenate([base, base + 1e-9 * rng.rand(1, 1500, 3)], 1)
        return p, base[0, ::3] + 3e-10 * rng.rand(500, 3), 1
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["uniform", "clusters", "plane", "far_queries", "outlier", "one_point", "line", "f64"])
def test_random_clouds_match_scipy(M, kind):
    from dnmf_amd import ops
    rng = np.random.RandomState(sum(map(ord, kind)))
    pts, qs, B = clouds(kind, rng)
    idx = ops.nearest_points(cuda(pts), cuda(qs)).cpu().numpy()
    assert idx.dtype == np.int32 and idx.shape == (B, qs.shape[-2])
    for b in range(B):
        check_cloud(pts[b], qs if qs.ndim == 2 else qs[b], idx[b])


def test_frame_chunks_and_row_strides(M):
    """B = 37 frames through a workspace of three frames (13 chunks) equal the one-chunk call and brute force; outputs with
    wider rows are written inside their rows only."""
    from dnmf_amd import ops, _lib
    rng = np.random.RandomState(3)
    B, N, Q = 37, 301, 203
    pts = (rng.rand(B, N, 3) * [20, 20, 3]).astype(np.float32)
    qs = rng.rand(B, Q, 3) * [21, 21, 4]
    vals = cuda(rng.rand(B, N), torch.float32)
    one = _lib.load().dnmf_nearest_points_workspace(N, 1)
    idx_c = torch.full((B, Q + 3), -7, dtype=torch.int32, device="cuda")
    out_c = torch.full((B, Q + 5), -7.0, device="cuda")
    ops.nearest_points(cuda(pts), cuda(qs), values=vals, out_index=idx_c, out=out_c, _workspace_bytes=3 * one)
    idx, out = ops.nearest_points(cuda(pts), cuda(qs), values=vals)
    assert torch.equal(idx_c[:, :Q], idx) and torch.equal(out_c[:, :Q], out)
    assert bool((idx_c[:, Q:] == -7).all()) and bool((out_c[:, Q:] == -7.0).all())
    assert torch.equal(out, torch.gather(vals, 1, idx.long()))
    idx = idx.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(idx[b], brute(pts[b], qs[b])[0])


# ---- 3. exact ties -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f64", [False, True])
def test_exact_ties_go_to_the_lowest_index(M, f64):
    """Integer coordinates (duplicates, points at equal distances): every d2 is exact in any order of summation."""
    from dnmf_amd import ops
    rng = np.random.RandomState(11)
    dt = np.float64 if f64 else np.float32
    pts = rng.randint(0, 5, (2, 2000, 3)).astype(dt)
    pts[1, :, 2] = 0
    qs = rng.randint(-1, 6, (700, 3)) + 0.5 * rng.randint(0, 2, (700, 3))
    idx = ops.nearest_points(cuda(pts), cuda(qs)).cpu().numpy()
    for b in range(2):
        np.testing.assert_array_equal(idx[b], brute(pts[b], qs)[0])
    # one cell holds everything: N identical points, every query ties N ways
    same = np.full((1, 4096, 3), 2.5, dt)
    idx = ops.nearest_points(cuda(same), cuda(qs)).cpu().numpy()
    assert (idx == 0).all()
    # N = 1; Q = 0
    assert (ops.nearest_points(cuda(pts[:, :1]), cuda(qs)).cpu().numpy() == 0).all()
    assert ops.nearest_points(cuda(pts), torch.zeros((0, 3), device="cuda")).shape == (2, 0)


# ---- 4. against K7 on the flows of a quadratic warp ---------------------------------------------------------------------

def k7_betas(O, sz, T):
    """The beta sets of test_registered_video_window_search_equals_exhaustive: identity, a shift, mild to folding warps."""
    rng = np.random.RandomState(sum(sz))
    beta = O.identity_beta(T)
    amp = np.array([0.0, 0.0] + list(np.logspace(-2, 1.3, T - 2)))
    base = np.array([3.0, 2e-2, 2e-2, 2e-2, 2e-4, 2e-4, 2e-4, 2e-4, 2e-4, 2e-4])
    beta += (rng.randn(10, 3, T) * base[:, None, None] * amp[None, None, :]).astype(np.float32)
    beta[0, 0, 1] = 7.3
    if sz[2] == 1:
        beta[:, 2] = O.identity_beta(T)[:, 2]
    return beta


def tie_proof(pts, lat, qi, got, want):
    """pts (P,3) fp32 CUDA, lat (P,3) float64 CUDA, mismatching queries qi: the two best float64 distances nearly equal and
    both choices among them."""
    p = pts.double()
    for s in range(0, len(qi), 64):
        q = lat[qi[s:s + 64]]
        d = ((q[:, None, 0] - p[None, :, 0]) ** 2 + (q[:, None, 1] - p[None, :, 1]) ** 2) + (q[:, None, 2] - p[None, :, 2]) ** 2
        two = torch.topk(d, 2, dim=1, largest=False).values
        assert bool((two[:, 1] - two[:, 0] < 1e-6).all()), two[:4]
        rows = torch.arange(len(q), device=d.device)
        for c in (got, want):
            assert bool((d[rows, c[qi[s:s + 64]]] - two[:, 0] < 1e-6).all())


@pytest.mark.parametrize("sz,frames", [([64, 48, 1], None), ([40, 36, 3], None), ([160, 128, 1], None),
                                       ([512, 512, 1], [0, 1, 2, 3, 4])])
def test_matches_K7_on_warp_flows(M, O, sz, frames):
    from dnmf_amd import ops
    T = 14
    beta = cuda(k7_betas(O, sz, T))
    times = list(range(T)) if frames is None else frames
    B, P = len(times), int(np.prod(sz))
    vals = torch.arange(P, device="cuda", dtype=torch.float32).repeat(B, 1)   # the value is the index (exact below 2^24)
    A = torch.zeros((*sz, 1), device="cuda")
    _, grid = ops.warp_gather(A, beta, times, want_A_t=False)         # (X,Y,Z,3,B) normalised
    szt = torch.tensor([float(s) for s in sz], device="cuda")
    flow = ((grid + 1) / 2) * szt[None, None, None, :, None]           # the reference's pushforward scaling, fp32
    pts = flow.permute(4, 0, 1, 2, 3).reshape(B, P, 3).contiguous()
    lat = cuda(O.voxel_lattice(sz).reshape(-1, 3), torch.float64)
    idx, got = ops.nearest_points(pts, lat, values=vals)
    k7 = ops.image_iwarp(vals, None, sz, beta, times)
    assert torch.equal(got, torch.gather(vals, 1, idx.long()))
    for b in range(B):
        mism = torch.nonzero(got[b] != k7[b]).flatten()
        if len(mism):
            tie_proof(pts[b], lat, mism, idx[b].long(), k7[b].long())


# ---- 5. determinism and the surface of ExponentialFP.image_iwarp -----------------------------------------------------------

def test_two_runs_are_identical(M):
    from dnmf_amd import ops
    rng = np.random.RandomState(5)
    pts = cuda((rng.rand(4, 20000, 3) * [100, 100, 10]).astype(np.float32))
    pts[:, 5000:5100] = pts[:, 100:200]                                 # duplicates: ties decided by the index rule
    qs = cuda(rng.rand(4, 20000, 3) * [100, 100, 10])
    a = ops.nearest_points(pts, qs)
    b = ops.nearest_points(pts, qs)
    assert torch.equal(a, b)


def test_image_iwarp_surface(M):
    rng = np.random.RandomState(9)
    X, Y, Z = 12, 9, 3
    im = rng.rand(X, Y, Z).astype(np.float32)
    flow = (np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1)
            + rng.rand(X, Y, Z, 3) * 0.8 - 0.4).astype(np.float32)
    grid = np.array(np.where(np.ones((X, Y, Z)))).T.reshape(X, Y, Z, 3)      # the reference's lattice, int64
    from oracle.dnmf_oracle import image_iwarp as scipy_iwarp
    want = scipy_iwarp(im, flow, grid)
    a = M.ExponentialFP.image_iwarp(im, flow, grid)
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == im.shape
    np.testing.assert_array_equal(a, want)                               # jittered lattice: no ties
    b = M.ExponentialFP.image_iwarp(torch.from_numpy(im), torch.from_numpy(flow), torch.from_numpy(grid))
    assert isinstance(b, np.ndarray) and b.dtype == np.float32
    np.testing.assert_array_equal(b, want)
    c = M.ExponentialFP.image_iwarp(cuda(im), cuda(flow), cuda(grid))
    assert isinstance(c, torch.Tensor) and c.is_cuda and c.dtype == torch.float32
    np.testing.assert_array_equal(c.cpu().numpy(), want)
    d = M.ExponentialFP.image_iwarp(im.astype(np.float64), flow.astype(np.float64), grid.astype(np.float32))
    assert d.dtype == np.float64
    np.testing.assert_array_equal(d, want.astype(np.float64))
    e = M.ExponentialFP.image_iwarp(cuda(im, torch.float64), cuda(flow), grid)
    assert e.is_cuda and e.dtype == torch.float64
    ints = M.ExponentialFP.image_iwarp((im * 1000).astype(np.int32), flow, grid)
    assert ints.dtype == np.int32
    np.testing.assert_array_equal(ints, (want * 1000).astype(np.int32))
    with pytest.raises(ValueError):
        M.ExponentialFP.image_iwarp(im, flow, grid[:-1])
    with pytest.raises(ValueError):
        M.ExponentialFP.image_iwarp(im, flow[:-1], grid[:-1])
    bad = flow.copy()
    bad[3, 2, 1, 0] = np.nan
    with pytest.raises(ValueError):
        M.ExponentialFP.image_iwarp(im, bad, grid)
    with pytest.raises(ValueError):
        M.ExponentialFP.image_iwarp(im, flow, grid + np.inf)


def test_reference_import_path_has_the_method():
    from Demix.dNMF import ExponentialFP
    assert callable(ExponentialFP.image_iwarp)
