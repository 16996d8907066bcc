"""The dense forward kernels -- ``dnmf_recon_image`` (ops.recon_image, ExponentialFP.recon_image with use_lists = False), K1
``dnmf_warp_gather`` (ops.warp_gather) and ``dnmf_render_frames`` (ops.render_frames) -- against the float64 definitions of
tests/forward_restatement.py, entry by entry.  What the case tables reach, and that every case tells a wrong kernel from the
right one by ten bounds, is checked without a GPU in tests/test_forward_restatement_host.py.

Cases (forward_restatement.CASES_RECON, CASES_K1, CASES_RENDER):
  recon_image  volumes (3,5,1) (4,4,1) (1,17,1) (32,32,1) (41,25,1) (9,7,5) (33,31,2) (65,63,1) (64,64,1) (17,241,1): P = 15,
               16, 17 (fewer voxels than a group, one group, a ragged second), 1024 / 1025 and 4096 / 4097 (a block of the
               B <= 16 and of the B > 16 form and one voxel past it), 315, 2046, 4095 (ragged last groups, Z > 1);
               K = 1, 15 | 16, 31 | .. | 112, 127: both ends of the eight register blocks Kp / 16 = 1 .. 8;
               B = 1, 16 | 17, 64 | 65, 70: the two frame forms (NF = 1 | 4), one and two frame blocks, a ragged one.
               Every K at (9,7,5) and (41,25,1) with one B on each side of 16; every volume at two K and all six B.
               ``times`` is a permutation with one repeat out of a C of B + 3 columns, passed as a column window of a wider
               buffer (ldc > T); S has two spare rows and a row stride 24 floats wider, all preset to 7.
               Three input families, dense signed footprints: one-hot traces over all K columns (as many calls as name every
               channel; the interior of S[t] is A[:, k(t)] bit for bit), integers 0 .. 15 (bit-equal to the integer
               product), random signed fp32 (the bound below).
  frame chunk  (4,4,1), K = 3, B = 32770, integers: two launches of the wrapper, bit-equal.
  K > 127      ExponentialFP.recon_image, use_lists = False, K = 128, 130, 225 (groups 112 + 16, 112 + 18, 112 + 112 + 1) and
               K = 127 (one launch), (33,31,2), B = 5 and 20, out = None and a caller's wider out; integers bit-equal, random
               within the grouped bound.
  K1           k2_restatement.SHAPES (33,257,1) (65,300,2) (34,90,3) (9,7,5): 34, 153, 36 and 2 blocks of 256 threads a frame,
               none full at the end; frames F0 .. F6 of case_betas as times = columns 4 0 6 1 7 2 5 0 (not monotone, F0 twice),
               an extreme warp in the column no call names; K = 5 Gaussians of sigma 3, some cut by the border.  A_t and grid
               are written into larger buffers preset to 7; want_A_t = False / want_grid = False give the same bits.
  render       (19,23,1) and (9,7,5), K = 3 and 300 (one pass and two of the LDS table loop), windows (t0, T) = (0, all),
               (4, 3), (10, 1) of 11 frames, positions inside, up to 8 voxels outside and 10^4 voxels away, traces float64 in
               [0, 1]; one amplitude of 1e30 and one of -1e30 in one frame (the r2_cut skip must widen with the largest
               MAGNITUDE); two spare rows and a stride 9 floats wider, preset to 7; K = 2049 is refused by name.

Bounds (forward_restatement; U = 2^-24; none was tuned):
  recon random   (Kp + 1) U (|A| . |C|) per entry -- every product and addition of a length-Kp fp32 dot product rounds at most
                 once, whatever the matrix core's order; a zero abs sum asks for an exact zero
  recon grouped  the groups' bounds summed + U |running sum| per group added
  K1 A_t         k2_restatement.recon_tol per channel and frame: 4 spacing_fp32(max|u|) slope(A_k) + 1e-6 max|A_k|
  K1 grid        13 U sum_a |phi_a| |2 beta_a| / (S_d - 1) + 2 U max(1, |n_d|); Z = 1: n_z == -1
  render         (K + 1) U sum_k |term_k|
Every test prints its worst |error| / bound and its host and GPU seconds.

The render cut-off.  ops.render_frames told the library float(traces.max()) as the amplitude its r2_cut is sized for.  With
the -1e30 case that is at most 1: the kernel skipped every term past r^2 = 629 although |term| there is up to 1e-16, and
the case failed by far more than its bound, as the reading of the code had it (see the measured lines).  The wrapper now passes
traces.abs().max().  The wrapper of recon_image also refused a C that is a column window of a wider table although the
kernel takes ldc; it now takes any row stride.

Measured on the MI355X (kept apart from the bounds above, which they did not set):
50 tests, 4.4 s in all (the slowest 0.5 s; every float64 reference under 0.2 s of host time).  Largest |error| / bound:
  recon random, by padded width 16 | 32 | .. | 128   0.23  0.10  0.079  0.051  0.049  0.047  0.040  0.030 (K sweep);
                by volume 0.041 .. 0.24 (the largest at (64,64,1), K = 15, and (3,5,1), K = 15: short sums);
                every one-hot and integer case, the 32770 frames and the integer cases by column groups bit-equal
  recon by column groups, random   K 127 0.026, 128 0.029, 130 0.023, 225 0.019
  K1 A_t   0.035 (33,257,1), 0.067 (65,300,2), 0.055 (34,90,3), 0.099 (9,7,5);   grid 0.44, 0.36, 0.40, 0.30
  render   0 in all fourteen cases: the bit-equal share is 1.000000 everywhere, K = 300 and the two 1e30 cases included (the
           device exp never moved a term across an fp32 rounding boundary, and the sum is taken in neuron order: the host test
           shows the reverse order changing more than 5 % of the entries at K = 300)
  render amp-1e30 before the change of the wrapper: |error| = 4.2e6 bounds at frame 5, voxel 412 (value -1.65e-17 written as 0),
           bit-equal share 0.996255; every other test passed in that run as well.
No defect was found in the three kernels themselves."""
import functools
import time

import numpy as np
import pytest
import torch

import forward_restatement as FR

pytestmark = pytest.mark.gpu
F32 = np.float32
PATTERN = 7.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def window(a, extra=4, fill=-3.5):
    """``a`` (rows, cols) on the device as the first columns of a buffer ``extra`` columns wider (they hold ``fill``)."""
    buf = torch.full((a.shape[0], a.shape[1] + extra), fill, device="cuda")
    buf[:, :a.shape[1]] = dev(a)
    return buf[:, :a.shape[1]]


def halo_split(ops, rows, sz):
    """rows (B, >= halo_voxels) numpy -> (interior (B, P) copy, True when every border float of the halo images is zero)."""
    X, Y, Z = sz
    from dnmf_amd import _lib
    rowf = _lib.load().dnmf_halo_row(Y, Z)
    assert ops.halo_voxels(sz) == (X + 2 * FR.HALO) * rowf
    img = rows[:, :(X + 2 * FR.HALO) * rowf].reshape(len(rows), X + 2 * FR.HALO, rowf).copy()
    inner = img[:, FR.HALO:FR.HALO + X, FR.HALO * Z:(FR.HALO + Y) * Z].reshape(len(rows), -1).copy()
    img[:, FR.HALO:FR.HALO + X, FR.HALO * Z:(FR.HALO + Y) * Z] = 0
    return inner, not img.any()


def run_recon(ops, call, sz, B, what, spare=2, pad=24):
    """``call(out)`` writes B halo images into the first rows of a preset buffer; returns the interiors (B, P) after checking
    that the border inside the images is zero and that spare rows and row padding still hold the pattern."""
    lds = ops.halo_voxels(sz)
    buf = torch.full((B + spare, lds + pad), PATTERN, device="cuda")
    res = call(buf)
    assert res.data_ptr() == buf.data_ptr()
    got = buf.cpu().numpy()
    assert (got[B:] == PATTERN).all() and (got[:, lds:] == PATTERN).all(), f"{what}: spare rows or row padding were written"
    inner, border_zero = halo_split(ops, got[:B], sz)
    assert border_zero, f"{what}: the halo border is not zero"
    return inner


def recon_check(ops, sz, K, B, family):
    """One case and family; returns the largest |error| / bound (0 for the exact families, which are asserted bit-equal)."""
    c = FR.recon_case(sz, K, B, family)
    Apk = ops.pack_footprints(dev(c["A"]))
    assert Apk.shape[1] == FR.padded_k(K) == ops.padded_k(K)
    Cw = window(c["C"])
    assert Cw.stride(0) > Cw.shape[1] or K == 1
    top = 0.0
    for times in c["calls"]:
        what = f"recon {sz} K {K} B {B} {family}"
        got = run_recon(ops, lambda out: ops.recon_image(Apk, K, sz, Cw, dev(np.array(times), torch.int32), out=out), sz, B, what)
        S, ab = FR.recon(c["A"], c["C"], times)
        if family == "onehot":
            assert np.array_equal(got, c["A"][:, times].T), f"{what}: S[t] is not A[:, k(t)] bit for bit"
        elif family == "integers":
            assert np.array_equal(got.astype(np.float64), S.T), f"{what}: not the integer product"
        else:
            ratio, idx, zeros_ok = FR.worst(np.abs(got.astype(np.float64) - S.T), FR.recon_tol(K, ab).T)
            assert zeros_ok and ratio <= 1.0, f"{what}: entry {idx}: |error| = {ratio:.3g} of the bound"
            top = max(top, ratio)
    return top


def recon_group(ops, cases, label):
    t0 = time.perf_counter()
    top = max(recon_check(ops, sz, K, B, family) for sz, K, B in cases for family in FR.FAMILIES)
    torch.cuda.synchronize()
    print(f"\nrecon {label}: {len(cases)} cases x 3 families, one-hot and integers bit-equal, random |error| / bound <= {top:.3g}; "
          f"host + GPU {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("K", list(FR.SWEEP_K))
def test_recon_every_padded_width(ops, K):
    """Every K at (9,7,5) and (41,25,1) (ragged last voxel groups), one B on each side of 16."""
    recon_group(ops, FR.SWEEP_K[K], f"K {K} (Kp {FR.padded_k(K)})")


@pytest.mark.parametrize("sz", list(FR.SWEEP_VOLUME), ids=lambda s: "x".join(map(str, s)))
def test_recon_every_volume(ops, sz):
    """Every volume at two K and B = 1, 16, 17, 64, 65, 70."""
    recon_group(ops, FR.SWEEP_VOLUME[sz], f"{sz} P {int(np.prod(sz))} K {sorted({c[1] for c in FR.SWEEP_VOLUME[sz]})}")


def test_recon_frame_chunks(ops):
    """B = 32770: the wrapper's second launch starts at frame 32768 of ``times`` and of ``out``."""
    sz, K, B = FR.CHUNK_CASE
    rng = np.random.default_rng(1)
    A, C = rng.integers(0, 16, (int(np.prod(sz)), K)).astype(F32), rng.integers(0, 16, (K, 50)).astype(F32)
    times = rng.integers(0, 50, B)
    t0 = time.perf_counter()
    Apk, Cw = ops.pack_footprints(dev(A)), window(C)
    got = run_recon(ops, lambda out: ops.recon_image(Apk, K, sz, Cw, dev(times, torch.int32), out=out), sz, B, "frame chunks",
                    spare=1, pad=8)
    assert np.array_equal(got.astype(np.float64), FR.recon(A, C, times)[0].T)
    print(f"\nrecon frame chunks: B {B} bit-equal; host + GPU {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("K", (127,) + FR.GROUPED_K)
def test_recon_by_column_groups(ops, K):
    """ExponentialFP.recon_image with use_lists = False: one launch at K = 127, groups of 112 summed in fp32 above."""
    from dnmf_amd.Demix.dNMF import ExponentialFP
    sz, P = FR.GROUPED_SZ, int(np.prod(FR.GROUPED_SZ))
    t0 = time.perf_counter()
    fp = ExponentialFP(list(sz), K, 4, positions=torch.zeros(K, 3))
    fp.use_lists = False
    top = 0.0
    for B in FR.GROUPED_B:
        for family in ("integers", "random"):
            rng = np.random.default_rng(FR._seed(K, B, family == "random"))
            if family == "integers":
                A, C = rng.integers(0, 16, (P, K)).astype(F32), rng.integers(0, 16, (K, B + 3)).astype(F32)
            else:
                A, C = rng.uniform(-1, 1, (P, K)).astype(F32), rng.uniform(-1, 1, (K, B + 3)).astype(F32)
            times = FR.call_times(B + 3, B, rng)
            fp.A = dev(A).reshape(*sz, K)
            fp.invalidate_layouts()
            S, bound = FR.recon_grouped(A, C, times) if K > 127 else (FR.recon(A, C, times)[0], FR.recon_tol(K, FR.recon(A, C, times)[1]))
            what = f"K {K} B {B} {family}"
            tt = dev(np.array(times), torch.int32)
            wide = run_recon(ops, lambda out: fp.recon_image(dev(C), tt, out=out), sz, B, what + " wider out")
            res = fp.recon_image(dev(C), tt)
            assert tuple(res.shape) == (B, ops.halo_voxels(sz))
            own, border_zero = halo_split(ops, res.cpu().numpy(), sz)
            assert border_zero and np.array_equal(own, wide), f"{what}: out = None and a caller's out differ"
            if family == "integers":
                assert np.array_equal(own.astype(np.float64), S.T), f"{what}: not the integer product"
            else:
                ratio, idx, zeros_ok = FR.worst(np.abs(own.astype(np.float64) - S.T), bound.T)
                assert zeros_ok and ratio <= 1.0, f"{what}: entry {idx}: |error| = {ratio:.3g} of the bound"
                top = max(top, ratio)
    print(f"\nrecon by column groups K {K}: integers bit-equal, random |error| / bound <= {top:.3g}; host + GPU "
          f"{time.perf_counter() - t0:.2f} s")


# ---- K1 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sz", FR.CASES_K1, ids=lambda s: "x".join(map(str, s)))
def test_k1(ops, sz):
    from dnmf_amd import _lib
    c = FR.k1_case(sz)
    ref, host = FR.k1_reference(sz)
    X, Y, Z = sz
    P, K, B = X * Y * Z, 5, len(c["times"])
    t0 = time.perf_counter()
    A, beta, tt = dev(c["A"]), dev(c["beta"]), dev(np.array(c["times"]), torch.int32)
    A_buf = torch.full((B * K * P + 64,), PATTERN, device="cuda")
    g_buf = torch.full((P * 3 * B + 64,), PATTERN, device="cuda")
    _lib.check(_lib.load().dnmf_warp_gather(A.data_ptr(), X, Y, Z, K, beta.data_ptr(), beta.shape[2], tt.data_ptr(), B,
                                            A_buf.data_ptr(), g_buf.data_ptr(), torch.cuda.current_stream().cuda_stream), "dnmf_warp_gather")
    A_t, grid = A_buf.cpu().numpy(), g_buf.cpu().numpy()
    assert (A_t[B * K * P:] == PATTERN).all() and (grid[P * 3 * B:] == PATTERN).all(), "written past the end"
    A_t, grid = A_t[:B * K * P].reshape(B, K, X, Y, Z), grid[:P * 3 * B].reshape(X, Y, Z, 3, B)
    both = ops.warp_gather(A, beta, tt)
    only_a, none_g = ops.warp_gather(A, beta, tt, want_grid=False)
    none_a, only_g = ops.warp_gather(A, beta, tt, want_A_t=False)
    assert none_g is None and none_a is None and tuple(both[0].shape) == A_t.shape and tuple(both[1].shape) == grid.shape
    for name, got in (("the wrapper's A_t", both[0]), ("A_t alone", only_a)):
        assert np.array_equal(got.cpu().numpy(), A_t), f"{sz}: {name} differs from the full call"
    for name, got in (("the wrapper's grid", both[1]), ("grid alone", only_g)):
        assert np.array_equal(got.cpu().numpy(), grid), f"{sz}: {name} differs from the full call"
    gpu = time.perf_counter() - t0
    a, b = FR.K1_REPEAT
    assert np.array_equal(A_t[a], A_t[b]) and np.array_equal(grid[..., a], grid[..., b]), f"{sz}: a repeated time gives two results"
    err = np.abs(A_t.astype(np.float64) - ref["A_t"]).reshape(B, K, -1).max(-1)
    ra, ia, _ = FR.worst(err, ref["tol_A"])
    assert ra <= 1.0, f"{sz}: A_t of frame {ia[0]} (column {c['times'][ia[0]]}) channel {ia[1]}: |error| = {ra:.3g} of the bound"
    rg, ig, zeros_ok = FR.worst(np.abs(grid.astype(np.float64) - ref["grid"]), ref["tol_grid"])
    assert zeros_ok, f"{sz}: the z component of the grid is not exactly -1"
    assert rg <= 1.0, f"{sz}: grid entry {ig}: |error| = {rg:.3g} of the bound"
    print(f"\nK1 {sz}: |error| / bound A_t {ra:.3g}, grid {rg:.3g}; host {host:.2f} s, GPU {gpu:.2f} s")


# ---- render_frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FR.CASES_RENDER))
def test_render(ops, name):
    """amp-1e30 is the case of the cut-off: it failed while the wrapper sized r2_cut from the largest signed trace."""
    c = FR.render_case(name)
    (video, ab), host = FR.render_reference(name)
    T, P = video.shape
    K = c["positions"].shape[0]
    t0 = time.perf_counter()
    buf = torch.full((T + 2, P + 9), PATTERN, device="cuda")
    res = ops.render_frames(dev(c["positions"]), dev(c["traces"], torch.float64), c["sz"], c["shape_std"], t0=c["t0"], T=c["T"], out=buf)
    assert res.data_ptr() == buf.data_ptr()
    got = buf.cpu().numpy()
    gpu = time.perf_counter() - t0
    assert (got[T:] == PATTERN).all() and (got[:, P:] == PATTERN).all(), f"{name}: spare rows or row padding were written"
    got = got[:T, :P]
    own = ops.render_frames(dev(c["positions"]), dev(c["traces"], torch.float64), c["sz"], c["shape_std"], t0=c["t0"], T=c["T"])
    assert tuple(own.shape) == (T, P) and np.array_equal(own.cpu().numpy(), got)
    ratio, idx, zeros_ok = FR.worst(np.abs(got.astype(np.float64) - video), FR.render_tol(K, ab))
    share = float((got == video).mean())
    print(f"\nrender {name}: |error| / bound {ratio:.3g}, bit-equal share {share:.6f}; host {host:.2f} s, GPU {gpu:.2f} s")
    assert zeros_ok, f"{name}: an entry without a term is not an exact zero"
    assert ratio <= 1.0, f"{name}: frame {idx[0]} voxel {idx[1]}: |error| = {ratio:.3g} of the bound (value {video[idx]:.3g})"


def test_render_refuses_more_neurons_than_the_lds_table_holds(ops):
    from dnmf_amd import _lib
    K = FR.RENDER_REFUSED_K
    out = torch.full((1, 15), PATTERN, device="cuda")
    with pytest.raises(_lib.DnmfHipError, match=f"K={K} too large for the LDS table"):
        ops.render_frames(torch.zeros(K, 3, 1, device="cuda"), torch.ones(K, 1, dtype=torch.float64, device="cuda"), (3, 5, 1), 3.0, out=out)
    assert (out == PATTERN).all()
    ops.render_frames(torch.zeros(K - 1, 3, 1, device="cuda"), torch.ones(K - 1, 1, dtype=torch.float64, device="cuda"), (3, 5, 1), 3.0,
                      out=out)
    assert float(out[0, 0]) == K - 1
