"""K15c on the GPU against its float64 definition (tests/follow_restatement.py), and the public entry points built on it.

The chain feeds its own fp32 results back, so a whole run is compared with the definition in three steps: the recurrence alone,
bit for bit, from the kernel's own positions; every row against K15's definition searched around the kernel's own prediction;
and the whole chain against the definition's, for the neurons whose predictions stay clear of a half-integer -- where the
rounding of a position cannot move a window."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import follow_restatement as FR
import track_restatement as TR
from test_gpu_track import compare, rows_of      # K15's tolerances and margin rule, as they stand

pytestmark = pytest.mark.gpu

COMBOS = [(case, anchor, momentum) for case in range(len(FR.CASES)) for anchor in ("first", 4, "last") for momentum in (0.0, 1.0)]
# tests/test_gpu_track.py lets the margin rule leave out no row of its planted cases; the definition alone leaves out none here
# (test_definition_alone_...)
LEFT_OUT_CAP = 0.0


def anchor_of(case, anchor):
    T = FR.CASES[case][1]
    return {"first": 0, "last": T - 1}.get(anchor, anchor)


@functools.lru_cache(maxsize=None)
def video(case):
    """-> (frames, truth, rows on the GPU in a shuffled order, times: slot j is row times[j])."""
    frames, truth, _ = FR.drifting_case(case)
    T = frames.shape[0]
    times = np.random.RandomState(50 + case).permutation(T)
    shuffled = np.empty_like(frames)
    shuffled[times] = frames
    return frames, truth, rows_of(shuffled), [int(t) for t in times]


def start_of(case, anchor):
    return np.rint(video(case)[1][:, :, anchor_of(case, anchor)])


@functools.lru_cache(maxsize=None)
def definition(case, anchor, momentum):
    sz, T, v, search, _, _, _, threshold, max_gap = FR.CASES[case]
    return FR.follow(video(case)[0], start_of(case, anchor), FR.SIGMA, search, anchor=anchor_of(case, anchor), momentum=momentum,
                     max_gap=max_gap, threshold=threshold)


def gpu_follow(case, anchor, momentum, **kw):
    from dnmf_amd import ops
    sz, T, v, search, _, _, _, threshold, max_gap = FR.CASES[case]
    frames, _, rows, times = video(case)
    out = ops.follow_neurons(rows, sz, torch.from_numpy(start_of(case, anchor)).cuda(), shape_std=FR.SIGMA, search=search,
                             anchor=anchor_of(case, anchor), momentum=momentum, max_gap=max_gap, threshold=threshold, times=times, **kw)
    assert out["positions"].dtype == torch.float64 and out["predicted"].dtype == torch.float64 and out["lost_at"].dtype == torch.int32
    assert out["amplitudes"].dtype == torch.float32 and out["peaks"].dtype == torch.float32 and out["positions"].is_cuda
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def kernel(case, anchor, momentum):
    return gpu_follow(case, anchor, momentum)


def as_track(out):
    return out["positions"], out["amplitudes"].astype(np.float64), out["peaks"].astype(np.float64)


@pytest.mark.parametrize("case,anchor,momentum", COMBOS)
def test_recurrence_is_the_definitions_bit_for_bit(case, anchor, momentum):
    """predicted and lost_at from the kernel's own positions and their found / NaN pattern, in float64 numpy."""
    got = kernel(case, anchor, momentum)
    max_gap = FR.CASES[case][8]
    predicted, lost_at = FR.predicted_from(got["positions"], start_of(case, anchor), anchor_of(case, anchor), momentum, max_gap)
    np.testing.assert_array_equal(got["predicted"].view(np.int64), predicted.view(np.int64))
    np.testing.assert_array_equal(got["lost_at"], lost_at)
    # the positions are fp32 values
    np.testing.assert_array_equal(got["positions"], got["positions"].astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("case,anchor,momentum", COMBOS)
def test_every_row_is_k15s_search_around_its_own_prediction(case, anchor, momentum):
    sz, T, v, search, _, _, _, threshold, _ = FR.CASES[case]
    got = kernel(case, anchor, momentum)
    ref = TR.track(video(case)[0], got["predicted"], FR.SIGMA, search, threshold=threshold)
    left_out = compare(ref, as_track(got), f"fixed point, case {case}, anchor {anchor}, momentum {momentum}")
    assert left_out <= LEFT_OUT_CAP


@pytest.mark.parametrize("case,anchor,momentum", COMBOS)
def test_whole_chain_equals_the_definition_away_from_half_integers(case, anchor, momentum):
    ref = definition(case, anchor, momentum)
    got = kernel(case, anchor, momentum)
    clear = np.where(np.isnan(ref["half"]), np.inf, ref["half"]).min(1) > 1e-3
    if not clear.any():
        return
    np.testing.assert_array_equal(got["lost_at"][clear], ref["lost_at"][clear])
    np.testing.assert_array_equal(np.isnan(got["predicted"][clear]), np.isnan(ref["predicted"][clear]))
    sub = {k: v[clear] for k, v in ref.items() if k != "lost_at"}
    left_out = compare(sub, tuple(a[clear] for a in as_track(got)), f"chain, case {case}, anchor {anchor}, momentum {momentum}")
    assert left_out <= LEFT_OUT_CAP
    found = np.isfinite(ref["predicted"][clear])
    # positions within 1e-3 (compare): last within 1e-3, the velocity within 2e-3 / n', carried over at most max_gap + 1 frames
    assert np.abs(got["predicted"][clear][found] - ref["predicted"][clear][found]).max() <= 1e-3 * (3 + 2 * FR.CASES[case][8])


def test_definition_alone_keeps_its_margins_and_three_quarters_of_the_neurons_clear():
    """Conditions on the inputs, met by the definition alone: no pick is decided by rounding, and at least three quarters of
    the neurons of all runs stay more than 1e-3 from a half-integer in every frame.  The blob that leaves its volume does
    leave: a window misses the volume and the chain is lost."""
    clear = total = 0
    for case, anchor, momentum in COMBOS:
        ref = definition(case, anchor, momentum)
        found = np.isfinite(ref["positions"]).all(1)
        assert (ref["margin"][found] >= 1e-3).all()
        clear += int((np.where(np.isnan(ref["half"]), np.inf, ref["half"]).min(1) > 1e-3).sum())
        total += ref["half"].shape[0]
    print(f"{clear} of {total} neurons clear of a half-integer")
    assert 4 * clear >= 3 * total
    sz, T, v, search = FR.CASES[3][:4]
    ref = definition(3, "first", 1.0)
    outside = np.rint(ref["predicted"][:, 1, :]) - search[1] > sz[1] - 1
    assert outside.any() and np.isnan(ref["positions"][:, 0, :][outside]).all()
    assert (ref["lost_at"][outside.any(1), 0] >= 0).all()


@pytest.mark.parametrize("case", range(len(FR.CASES)))
def test_second_call_gives_the_same_bits(case):
    first = kernel(case, 4, 1.0)
    again = gpu_follow(case, 4, 1.0)
    for name in first:
        np.testing.assert_array_equal(first[name].view(np.int64 if first[name].dtype == np.float64 else np.int32),
                                      again[name].view(np.int64 if again[name].dtype == np.float64 else np.int32), err_msg=name)


def test_rows_in_order_background_and_a_start_that_is_not_finite():
    from dnmf_amd import ops
    case, anchor = 0, 4
    sz, T, v, search = FR.CASES[case][:4]
    frames, truth, _, _ = video(case)
    start = start_of(case, anchor)
    # times=None on the rows in order: the bits of the shuffled rows with their permutation
    rows = rows_of(frames)
    plain = ops.follow_neurons(rows, sz, torch.from_numpy(start).cuda(), shape_std=FR.SIGMA, search=search, anchor=anchor, momentum=1.0)
    for name, ref in kernel(case, anchor, 1.0).items():
        np.testing.assert_array_equal(plain[name].cpu().numpy(), ref, err_msg=name)
    # a per-frame background is taken off before the filter
    bg = np.linspace(-0.2, 0.3, T)
    lifted = frames + bg[:, None, None, None].astype(np.float32)
    got = ops.follow_neurons(rows_of(lifted), sz, torch.from_numpy(start).cuda(), shape_std=FR.SIGMA, search=search, anchor=anchor,
                             background=torch.from_numpy(bg))
    got = {k: v.cpu().numpy() for k, v in got.items()}
    ref = TR.track(lifted, got["predicted"], FR.SIGMA, search, background=bg)
    assert compare(ref, as_track(got), "background") <= LEFT_OUT_CAP
    assert (got["lost_at"] == -1).all()
    # a start row that is not finite: NaN rows, lost at the anchor, the others untouched
    bad = start.copy()
    bad[2, 0] = np.inf
    out = ops.follow_neurons(rows, sz, torch.from_numpy(bad).cuda(), shape_std=FR.SIGMA, search=search, anchor=anchor, momentum=1.0)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    np.testing.assert_array_equal(out["lost_at"], [[-1, -1], [-1, -1], [anchor, anchor], [-1, -1]])
    for name in ("positions", "predicted", "amplitudes", "peaks"):
        assert np.isnan(out[name][2]).all(), name
        np.testing.assert_array_equal(out[name][[0, 1, 3]], kernel(case, anchor, 1.0)[name][[0, 1, 3]], err_msg=name)


def test_model_surface_and_refusals():
    from dnmf_amd import _lib, ops
    from dnmf_amd.Demix.dNMF import DeformableNMF, ExponentialFP
    case, anchor = 1, 4
    sz, T, v, search = FR.CASES[case][:4]
    frames, truth, _, _ = video(case)
    K = truth.shape[0]
    start = start_of(case, anchor)
    rows = rows_of(frames)
    direct = ops.follow_neurons(rows, sz, torch.from_numpy(start).cuda(), shape_std=FR.SIGMA, search=search, anchor=anchor, momentum=1.0)
    # numpy in, numpy out; CUDA in, CUDA out
    P_T, amp, info = ExponentialFP.follow_positions(frames, start, shape_std=FR.SIGMA, search=search, anchor=anchor, momentum=1.0)
    assert isinstance(P_T, np.ndarray) and P_T.dtype == np.float64 and P_T.shape == (K, 3, T) and amp.shape == (K, T)
    assert sorted(info) == ["lost_at", "peaks", "predicted"] and isinstance(info["lost_at"], np.ndarray)
    np.testing.assert_array_equal(P_T, direct["positions"].cpu().numpy())
    np.testing.assert_array_equal(info["predicted"], direct["predicted"].cpu().numpy())
    assert np.abs(P_T - truth).max() <= 0.5
    vt = torch.from_numpy(frames).cuda()
    P_G, amp_g, info_g = ExponentialFP.follow_positions((vt.reshape(T, -1), sz), torch.from_numpy(start).cuda(), shape_std=FR.SIGMA,
                                                        search=search, anchor=anchor, momentum=1.0)
    assert P_G.is_cuda and amp_g.is_cuda and info_g["lost_at"].is_cuda
    np.testing.assert_array_equal(P_G.cpu().numpy(), P_T)
    # the model: its own centres in the anchor frame under the current warp, its own width
    torch.manual_seed(0)
    dn = DeformableNMF(torch.tensor(sz), K, T, positions=torch.from_numpy(start).float())
    dn.verbose = False
    assert dn.last_follow is None
    P_M, amp_m, info_m = dn.follow(vt, anchor=anchor, search=search, momentum=1.0)
    assert dn.last_follow[0] is P_M and P_M.is_cuda and tuple(P_M.shape) == (K, 3, T)
    at_anchor = torch.from_numpy(dn.positions(times=[anchor])[:, :, 0]).cuda()
    same = ops.follow_neurons(vt.reshape(T, -1), sz, at_anchor, shape_std=float(dn.fp.sigma[0]), search=search, anchor=anchor, momentum=1.0)
    np.testing.assert_array_equal(P_M.cpu().numpy(), same["positions"].cpu().numpy())
    np.testing.assert_array_equal(info_m["predicted"].cpu().numpy(), same["predicted"].cpu().numpy())
    np.testing.assert_array_equal(amp_m.cpu().numpy(), same["amplitudes"].cpu().numpy())
    # fp.sigma is the constructor's 3, not the planted 2: a wider filter follows the same blobs
    assert np.abs(P_M.cpu().numpy() - truth).max() <= 0.5
    ok = dn.init_motion(P_M, order='affine', ridge=1e-3)
    assert bool(ok.all())
    P_S, _, _ = dn.follow(frames, anchor=anchor, start=start, search=search)
    assert isinstance(P_S, np.ndarray) and dn.last_follow[0] is P_S
    # refusals, in the driver and in the library
    s = torch.from_numpy(start).cuda()
    for kw, word in ((dict(anchor=-1), "anchor"), (dict(anchor=T), "anchor"), (dict(momentum=1.5), "momentum"),
                     (dict(momentum=-0.1), "momentum"), (dict(momentum=float("nan")), "momentum"), (dict(max_gap=-1), "max_gap"),
                     (dict(search=(1, -1, 0)), "search"), (dict(times=[0, T]), "times")):
        with pytest.raises(ValueError, match=word):
            ops.follow_neurons(rows, sz, s, shape_std=FR.SIGMA, **kw)
    with pytest.raises(_lib.DnmfHipError, match="LDS"):
        ops.follow_neurons(torch.zeros((2, 64 * 64 * 4), device="cuda"), (64, 64, 4), s, shape_std=8.0, search=(12, 12, 1))
    lib = _lib.load()
    I3 = ctypes.c_int * 3
    canary = torch.full((K * 3 * T,), -7.0, dtype=torch.float64, device="cuda")
    lost = torch.full((K, 2), -7, dtype=torch.int32, device="cuda")
    for anchor_, momentum_, gap_ in ((T, 0.0, 5), (0, 2.0, 5), (0, float("nan"), 5), (0, 0.0, -1)):
        rc = lib.dnmf_follow_neurons(rows.data_ptr(), rows.stride(0), I3(*sz), T, None, s.data_ptr(), K, FR.SIGMA, I3(*search), anchor_,
                                     momentum_, gap_, 0.0, None, canary.data_ptr(), None, None, canary.data_ptr(), lost.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == -2 and bool((canary == -7).all()) and bool((lost == -7).all())
