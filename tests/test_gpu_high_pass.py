"""The spatial high-pass (K22, ``dnmf_high_pass_frames``) on the GPU against the float64 definition
(tests/high_pass_restatement.py), and ``high_pass_filter_space`` built on it.

Tolerance, derived: with m non-zero taps, u = 2^-24 and S = sum |taps_ij| |in| per output voxel (float64),
|got - def| <= (m + 3) u S -- one rounding of every tap to fp32, m fused multiply-adds in any fixed order, the final store.
The largest observed ratio |got - def| / ((m + 3) u S) is printed by every comparison."""
import functools

import numpy as np
import pytest
import torch

import high_pass_restatement as HR

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# (X, Y, Z), gSig: several bounces, an extent of 1, odd Z, extents beyond one tile and no multiple of it, the smallest and the
# largest kernel.  The last one is this file's own: Z = 10 at gSig 10 no longer fits a tile with every slice in LDS (one slice per
# workgroup).
CASES = [((5, 37, 1), 7), ((3, 4, 2), 10), ((1, 9, 1), 3), ((40, 33, 2), 3), ((33, 31, 3), 2), ((70, 67, 1), 7), ((64, 56, 2), 1),
         ((6, 5, 10), 10)]
BATCHES = [1, 5]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dnmf_amd import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


@functools.lru_cache(maxsize=None)
def video(sz, T=5):
    rng = np.random.RandomState(sum(sz))
    x = (10.0 + 3.0 * rng.randn(T, *sz)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def definition(sz, gsig, T=5):
    """(the definition of video(sz), S): computed once, never changed."""
    out, S = HR.filter_frames(video(sz, T), HR.high_pass_taps(gsig))
    out.setflags(write=False), S.setflags(write=False)
    return out, S


def check(got, want, S, m, what):
    err = np.abs(got.astype(np.float64) - want)
    bound = (m + 3) * U * S
    ratio = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    print(f"K22 {what}: largest |got - def| / ((m + 3) u S) = {ratio:.4f} (m = {m})")
    assert (err <= bound).all(), f"{what}: ratio {ratio}"
    return ratio


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("sz,gsig", CASES)
def test_against_the_definition(ops, sz, gsig, B):
    P = int(np.prod(sz))
    want, S = definition(sz, gsig)
    m = int(np.count_nonzero(HR.high_pass_taps(gsig)))
    frames = dev(video(sz)[:B].reshape(B, P))
    got = ops.high_pass_frames(frames, sz, (gsig, gsig))
    assert got.shape == (B, P) and got.dtype == torch.float32
    check(got.cpu().numpy().reshape(B, *sz), want[:B], S[:B], m, f"{sz} gSig {gsig} B {B}")
    again = ops.high_pass_frames(frames, sz, gsig)
    assert torch.equal(got, again)                      # the same bits on every run


def test_row_strides_and_untouched_padding(ops):
    sz, gsig, B = (40, 33, 2), 3, 5
    P = int(np.prod(sz))
    want, S = definition(sz, gsig)
    m = int(np.count_nonzero(HR.high_pass_taps(gsig)))
    wide = torch.full((B, P + 7), float("nan"), device="cuda")
    wide[:, :P] = dev(video(sz).reshape(B, P))
    out = torch.full((B + 1, P + 5), -7.0, device="cuda")
    ret = ops.high_pass_frames(wide[:, :P], sz, gsig, out=out[:, :P])
    assert ret.data_ptr() == out.data_ptr()
    check(out[:B, :P].cpu().numpy().reshape(B, *sz), want, S, m, "ldf > P, ldo > P")
    assert (out[:, P:] == -7.0).all() and (out[B] == -7.0).all()


def test_frame_ids_permute_and_repeat(ops):
    sz, gsig = (33, 31, 3), 2
    P = int(np.prod(sz))
    want, S = definition(sz, gsig)
    m = int(np.count_nonzero(HR.high_pass_taps(gsig)))
    ids = [3, 0, 0, 4, 1, 3, 2]
    got = ops.high_pass_frames(dev(video(sz).reshape(5, P)), sz, gsig, frame_ids=ids)
    assert got.shape == (len(ids), P)
    check(got.cpu().numpy().reshape(len(ids), *sz), want[ids], S[ids], m, "frame_ids")


@pytest.mark.parametrize("sz,gsig,at", [((40, 33, 2), 3, (20, 15, 1)), ((5, 37, 1), 7, (0, 36, 0)), ((6, 5, 10), 10, (2, 2, 7))])
def test_a_nan_voxel_spreads_as_in_the_definition(ops, sz, gsig, at):
    P = int(np.prod(sz))
    v = video(sz)[:1].copy()
    v[(0,) + at] = np.nan
    want, _ = HR.filter_frames(v, HR.high_pass_taps(gsig))
    got = ops.high_pass_frames(dev(v.reshape(1, P)), sz, gsig).cpu().numpy().reshape(1, *sz)
    assert np.isnan(want).any() and np.array_equal(np.isnan(got), np.isnan(want))
    # the other slices of the frame are untouched by it
    clean, _ = definition(sz, gsig)
    other = [z for z in range(sz[2]) if z != at[2]]
    assert np.allclose(got[0][..., other], clean[0][..., other], rtol=0, atol=1e-3)


def test_taps_with_zeros_inside_a_column(ops):
    """A kernel no gSig makes: zeros between non-zero taps, an empty column, an empty row.  The zeros are not applied."""
    sz = (37, 70, 2)
    P = int(np.prod(sz))
    rng = np.random.RandomState(3)
    taps = rng.randn(11, 11)
    taps[rng.rand(11, 11) < 0.4] = 0
    taps[:, 4] = 0
    taps[7, :] = 0
    taps[5, 5] = 0
    taps = taps.astype(np.float32).astype(np.float64)
    v = video(sz)[:2].copy()
    v[1, 20, 30, 1] = np.nan
    want, S = HR.filter_frames(v, taps)
    got = ops.high_pass_frames(dev(v.reshape(2, P)), sz, None, taps=taps).cpu().numpy().reshape(2, *sz)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == np.count_nonzero(taps)
    ok = ~np.isnan(want)
    check(np.where(ok, got, 0), np.where(ok, want, 0), np.where(ok, S, 0), int(np.count_nonzero(taps)), "taps with holes")


def test_refusals(ops):
    from dnmf_amd._lib import DnmfHipError
    frames = torch.zeros((2, 24), device="cuda")
    with pytest.raises(DnmfHipError, match="argument error -3"):
        ops.high_pass_frames(frames, (2, 3, 4), (11, 11))                     # n = 33
    with pytest.raises(DnmfHipError, match="argument error -2"):
        ops.high_pass_frames(frames, (2, 3, 4), None, taps=np.ones((4, 4)))   # an even n
    for sz in ((0, 3, 4), (2, 0, 4), (2, 3, 0)):
        with pytest.raises(DnmfHipError, match="argument error -2"):
            ops.high_pass_frames(frames, sz, 2)
    with pytest.raises(ValueError):
        ops.high_pass_frames(frames, (2, 3, 4), (0, 3))
    with pytest.raises(ValueError, match="overlaps"):
        ops.high_pass_frames(frames, (2, 3, 4), 2, out=frames)
    buf = torch.zeros((4, 30), device="cuda")
    with pytest.raises(ValueError, match="overlaps"):
        ops.high_pass_frames(buf[:2, :24], (2, 3, 4), 2, out=buf[1:3, :24])
    with pytest.raises(ValueError, match="overlaps"):
        ops.high_pass_frames(buf[:, :24], (2, 3, 4), 2, frame_ids=[0], out=buf[3:, :24])
    # (the check is by address range; two halves of one buffer pass)
    ops.high_pass_frames(buf[:2, :24], (2, 3, 4), 2, out=buf[2:, :24])


@pytest.mark.parametrize("shape", [(40, 33), (33, 31, 3)])
def test_high_pass_filter_space_numpy_and_cuda(ops, shape):
    from dnmf_amd.Demix.MotionCorrect import high_pass_filter_space
    sz = shape if len(shape) == 3 else shape + (1,)
    gsig = 3 if len(shape) == 2 else 2
    img = video(sz)[0].reshape(shape)
    want, S = definition(sz, gsig)
    m = int(np.count_nonzero(HR.high_pass_taps(gsig)))
    a = high_pass_filter_space(img, (gsig, gsig))
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == shape
    b = high_pass_filter_space(dev(img), (gsig, gsig))
    assert torch.is_tensor(b) and b.is_cuda and b.dtype == torch.float32 and tuple(b.shape) == shape
    assert np.array_equal(a, b.cpu().numpy())
    check(a.reshape(sz), want[0], S[0], m, f"high_pass_filter_space {shape}")
    c = high_pass_filter_space(img.astype(np.float64), gsig)                 # float32(img), as the reference casts it
    assert c.dtype == np.float32 and np.array_equal(a, c)
